// The PSK31 skimmer's plan, staging geometry and event slots (pysdr_amd/csrc/psk_plan.h, the very code psk.hip steps with)
// on the CPU under AddressSanitizer + UBSan.
//   * the rules: S in {8, 12}, nk >= 1, nk NSUB <= 2^18, max_out in [1, 2^20] and the settings' rules; the groups tile
//     [0, nk), the row pitch holds the history's room and max_out, the event cap is max_out / (3 S / 2) + 1.
//   * the tile walk of the kernel, through the index functions of PskGeom that psk.hip itself uses: every staging load
//     goes to a Y of exactly nk x pitch elements and an LDS tile of exactly rows x pitch elements (heap: the sanitizer guards both ends), every decoder's filter window stays inside the tile
//     and sees sample m - i at tap i, every (row, output) is consumed exactly once and in order, the history roll reads
//     and writes inside the row, and the energies' LDS layout puts the lanes of a wave on different banks.
//   * the mixer and matched filter (psk_filter) on that walk with real samples, heap-backed tables and tile, against a
//     plain sum over the row's memory, bit for bit; a NaN, an infinite and an over-pmax sample blank exactly the outputs
//     whose window reaches them.
//   * the event slots: the symbol step (psk_symbol) driven by EVERY sequence of five symbols of (bit, timing move in
//     {earliest, none, latest}), from every kind of start state and every start count, sample by sample as the kernel
//     counts, storing into exactly `cap` slots for every call length: two events are never closer than 3 S / 2 samples, the
//     closest ARE 3 S / 2 apart, and the count never exceeds the cap.
//   * the event word round-trips.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "psk_plan.h"

using namespace pysdr;

#define REQUIRE(c, ...) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static pysdr_psk_cfg good_cfg() {
  pysdr_psk_cfg c{};
  c.a_t = 1.f / 32; c.a_q = 1.f / 64; c.hi = 0.75f; c.lo = 0.3f; c.hy = 1.125f; c.pmax = 1e18f; c.n0 = 128;
  return c;
}

template <int S>
static long walk(int nk, int n_out, const PskPlan& p) {
  using G = PskGeom<S>;
  constexpr int L = G::kL, NSUB = G::kNsub, ROWS = G::kRows, TH = G::kThreads, YP = G::kYp;
  std::vector<int> loads((size_t)nk * p.ypitch, 0);              // Y as allocated: a.y = Y + kPskHpad
  long steps = 0;
  for (int g = 0; g < p.groups; ++g) {
    const int row0 = g * ROWS;
    std::vector<long> tile((size_t)ROWS * YP);
    std::vector<int> next((size_t)TH, 0);
    for (int i0 = 0; i0 < n_out; i0 += kPskTile) {
      std::vector<long> carry((size_t)TH, -1L);
      REQUIRE(G::kCarry <= TH, "a thread per carried sample");
      for (int tid = 0; tid < G::kCarry; ++tid) {                  // the L - 1 in front: history, or the last tile's end
        const int hr = G::carry_row(tid), hc = G::carry_col(tid);
        if (i0 > 0) carry[(size_t)tid] = tile.data()[(size_t)G::carry_src(hr, hc)];
        else if (row0 + hr < nk) { carry[(size_t)tid] = (long)(row0 + hr) * p.ypitch + kPskHpad + G::hist_off(hc); loads.data()[carry[(size_t)tid]] += 1; }
      }
      std::fill(tile.begin(), tile.end(), -2L);
      for (int tid = 0; tid < G::kCarry; ++tid) {
        long& slot = tile.data()[(size_t)G::carry_dst(G::carry_row(tid), G::carry_col(tid))];
        REQUIRE(slot == -2, "carried slot written twice");
        slot = carry[(size_t)tid];
      }
      for (int tid = 0; tid < TH; ++tid)
        for (int k = tid; k < ROWS * kPskTile; k += TH) {
          const int rr = G::stage_row(k), c = G::stage_col(k), i = i0 + c;
          long v = -1;
          if (row0 + rr < nk && i < n_out) {
            v = (long)(row0 + rr) * p.ypitch + kPskHpad + i;
            loads.data()[v] += 1;
          }
          long& slot = tile.data()[(size_t)G::stage_dst(rr, c)];
          REQUIRE(slot == -2, "LDS slot written twice");
          slot = v;
        }
      const int nj = n_out - i0 < kPskTile ? n_out - i0 : kPskTile;
      for (int tid = 0; tid < TH; ++tid) {
        const int r = tid / NSUB, row = row0 + r;
        for (int jj = 0; jj < nj; ++jj) {
          for (int i = 0; i < L; ++i) {
            const long v = tile.data()[(size_t)G::win(r, jj) - i];
            if (row < nk) REQUIRE(v == (long)row * p.ypitch + kPskHpad + i0 + jj - i, "tap %d of output %d reads %ld", i, i0 + jj, v);
            else REQUIRE(v == -1, "a thread without a row reads memory");
          }
          if (row < nk) { REQUIRE(next[(size_t)tid] == i0 + jj, "out of order"); next[(size_t)tid] += 1; ++steps; }
        }
      }
    }
    for (int tid = 0; tid < TH; ++tid) {
      const int r = tid / NSUB, j = tid % NSUB, row = row0 + r;
      if (row >= nk) continue;
      REQUIRE(next[(size_t)tid] == n_out, "thread %d walked %d of %d", tid, next[(size_t)tid], n_out);
      if (j < L - 1) {                                             // the history roll
        const long src = (long)row * p.ypitch + kPskHpad + G::roll_src(n_out, j), dst = (long)row * p.ypitch + kPskHpad + G::roll_dst(j);
        REQUIRE(src >= (long)row * p.ypitch && src < (long)(row + 1) * p.ypitch && dst >= (long)row * p.ypitch && dst < (long)row * p.ypitch + kPskHpad, "roll");
        loads.data()[src] += 0;
        loads.data()[dst] += 0;
      }
    }
  }
  for (int r = 0; r < nk; ++r)
    for (int i = 0; i < p.ypitch; ++i) {
      const int rel = i - kPskHpad;                                // the history and the call's outputs: read once each
      const int want = (rel >= -(L - 1) && rel < n_out) ? 1 : 0;
      REQUIRE(loads[(size_t)r * p.ypitch + i] == want, "nk %d n_out %d: (%d, %d) loaded %d x, expected %d", nk, n_out, r, rel, loads[(size_t)r * p.ypitch + i], want);
    }
  // e[phase][thread]: the 32 lanes of a half-wave on 32 different banks, whatever the phase
  for (int ph = 0; ph < S; ++ph)
    for (int w0 = 0; w0 < TH; w0 += 32) {
      unsigned banks = 0;
      for (int l = 0; l < 32; ++l) { const int b = G::e_at(ph, w0 + l) % 32; REQUIRE(!(banks >> b & 1), "bank"); banks |= 1u << b; }
    }
  return steps;
}

// psk_filter itself, on the tile walk above with real samples: Y of exactly nk x pitch samples, an LDS tile of exactly
// rows x YP samples, tw and g of exactly NT and L (all heap: the sanitizer guards both ends), from a first output m0 deep
// in a stream.  Every (row, decoder, output) is held against a plain sum over the row's memory, float for float in the
// definition's order (bit-equal: contraction is off), and the outputs blanked are exactly those whose window reaches a
// NaN, an infinite or an over-pmax sample; a large sample below pmax is not blanked.
template <int S>
static long filter_check(int nk, int n_out, long m0, const PskPlan& p) {
  using G = PskGeom<S>;
  constexpr int L = G::kL, NT = G::kNt, NSUB = G::kNsub, ROWS = G::kRows, TH = G::kThreads, YP = G::kYp;
  const float pmax = 1e18f;
  std::vector<PskC> tw((size_t)NT), Y((size_t)nk * p.ypitch, PskC{7e30f, -7e30f});   // what is never staged would blank
  std::vector<float> g((size_t)L);
  double gs = 0;
  for (int i = 0; i < L; ++i) gs += 0.5 * (1.0 - cos(2 * M_PI * (i + 0.5) / L));
  for (int i = 0; i < L; ++i) g[(size_t)i] = (float)(0.5 * (1.0 - cos(2 * M_PI * (i + 0.5) / L)) / gs);
  for (int t = 0; t < NT; ++t) tw[(size_t)t] = PskC{(float)cos(2 * M_PI * t / NT), (float)-sin(2 * M_PI * t / NT)};
  unsigned rng = 12345u + (unsigned)(nk * 131 + n_out);
  auto rnd = [&]() { rng = rng * 1664525u + 1013904223u; return (float)((int)(rng >> 8) - (1 << 23)) / (float)(1 << 23); };
  std::vector<char> bad((size_t)nk * p.ypitch, 0);
  for (int r = 0; r < nk; ++r)
    for (int i = -(L - 1); i < n_out; ++i) Y[(size_t)r * p.ypitch + kPskHpad + i] = PskC{rnd(), rnd()};
  auto poke = [&](int r, int i, PskC v, bool blanks) {
    if (r < nk && i < n_out) { Y[(size_t)r * p.ypitch + kPskHpad + i] = v; bad[(size_t)r * p.ypitch + kPskHpad + i] = blanks; }
  };
  poke(0, 3, PskC{__builtin_nanf(""), 0.25f}, true);
  poke(nk - 1, n_out / 2, PskC{-0.5f, __builtin_inff()}, true);
  poke(nk / 2, n_out - 1, PskC{3e19f, 0.f}, true);
  poke(0, -(L - 1), PskC{0.f, -3e19f}, true);                     // in the history
  poke(nk - 1, kPskTile - 1, PskC{1e6f, 1e6f}, false);             // large, below pmax: kept
  long checked = 0, blanked = 0;
  for (int g0 = 0; g0 < p.groups; ++g0) {
    const int row0 = g0 * ROWS;
    std::vector<PskC> tile((size_t)ROWS * YP);
    for (int i0 = 0; i0 < n_out; i0 += kPskTile) {
      std::vector<PskC> carry((size_t)G::kCarry, PskC{0.f, 0.f});
      for (int tid = 0; tid < G::kCarry; ++tid) {
        const int hr = G::carry_row(tid), hc = G::carry_col(tid);
        if (i0 > 0) carry[(size_t)tid] = tile.data()[G::carry_src(hr, hc)];
        else if (row0 + hr < nk) carry[(size_t)tid] = Y.data()[(size_t)(row0 + hr) * p.ypitch + kPskHpad + G::hist_off(hc)];
      }
      for (int tid = 0; tid < G::kCarry; ++tid) tile.data()[G::carry_dst(G::carry_row(tid), G::carry_col(tid))] = carry[(size_t)tid];
      for (int k = 0; k < ROWS * kPskTile; ++k) {
        const int rr = G::stage_row(k), c = G::stage_col(k), i = i0 + c;
        PskC v{0.f, 0.f};
        if (row0 + rr < nk && i < n_out) v = Y.data()[(size_t)(row0 + rr) * p.ypitch + kPskHpad + i];
        tile.data()[G::stage_dst(rr, c)] = v;
      }
      const int nj = n_out - i0 < kPskTile ? n_out - i0 : kPskTile;
      for (int tid = 0; tid < TH; ++tid) {
        const int r = tid / NSUB, j = tid % NSUB, row = row0 + r;
        if (row >= nk) continue;
        const int qm = psk_qmod(j, S);
        const long q = 2 * j - NSUB + 1;
        for (int jj = 0; jj < nj; ++jj) {
          const long m = m0 + i0 + jj;
          const int t = psk_mulmod(qm, (int)(m % NT), NT);
          float ur = -1.f, ui = -1.f;
          const float pw = psk_filter<S>(tile.data() + G::win(r, jj), tw.data(), g.data(), t, qm, pmax, ur, ui);
          // the definition, from the row's memory
          float ar = 0.f, ai = 0.f;
          bool reach = false;
          for (int i = 0; i < L; ++i) {
            const size_t at = (size_t)row * p.ypitch + kPskHpad + i0 + jj - i;
            const PskC y = Y[at], w = tw[(size_t)((((q * (m - i)) % NT) + NT) % NT)];
            reach = reach || bad[at];
            const float vr = y.x * w.x - y.y * w.y, vi = y.x * w.y + y.y * w.x;
            if (i == 0) { ar = g[0] * vr; ai = g[0] * vi; }
            else { ar = ar + g[(size_t)i] * vr; ai = ai + g[(size_t)i] * vi; }
          }
          float want = ar * ar + ai * ai;
          const bool blank = !(want <= pmax);
          REQUIRE(blank == reach, "row %d decoder %d output %d: blanked %d, a bad sample in reach %d", row, j, i0 + jj, (int)blank, (int)reach);
          if (blank) { ar = 0.f; ai = 0.f; want = 0.f; ++blanked; }
          REQUIRE(memcmp(&pw, &want, 4) == 0 && memcmp(&ur, &ar, 4) == 0 && memcmp(&ui, &ai, 4) == 0 && pw == pw,
                  "row %d decoder %d output %d: filter (%g, %g, %g), definition (%g, %g, %g)", row, j, i0 + jj, (double)ur, (double)ui,
                  (double)pw, (double)ar, (double)ai, (double)want);
          ++checked;
        }
      }
    }
  }
  if (n_out > 4 * L) REQUIRE(blanked > 0 && blanked < checked, "%ld of %ld outputs blanked", blanked, checked);   // both kinds were seen
  return checked;
}

// One decoder driven symbol by symbol: choice = bit + 2 * move, move in {0: the earliest phase, 1: stay, 2: the latest}
template <int S>
static void drive(const pysdr_psk_cfg& c, PskDec z, int p0, const int* choice, int nsym, int* min_gap, long* worst_fill) {
  std::vector<int> at;                                             // sample index of every event
  float e[S];
  int p = p0, i = 0, k = 0;
  float sign = 1.f;
  for (; k < nsym || z.cnt > 1; ++i) {
    z.cnt -= 1;
    if (z.cnt == 0) {
      if (k == nsym) break;
      const int bit = choice[k] & 1, move = choice[k] >> 1;
      ++k;
      // the phase that gives d = -S / 2 (earliest next symbol), 0, or S / 2 - 1 (latest)
      const int d = move == 0 ? -S / 2 : (move == 1 ? 0 : S / 2 - 1);
      const int b = ((p + d) % S + S) % S;
      for (int q = 0; q < S; ++q) e[q] = q == b ? 2.f : (q == z.pt ? 1.f : 0.f);
      if (b == z.pt) e[b] = 2.f;
      if (!bit) sign = -sign;                                      // a 0 reverses the phase
      z.qn = 1e6f; z.qd = 1e6f;                                    // the squelch stays open
      const int code = psk_symbol<S>(z, c, sign, 0.f, e, 1, p);
      REQUIRE(z.cnt == S + d && z.cnt >= S / 2 && z.cnt < 3 * S / 2 + 1, "cnt %d after move %d", z.cnt, move);
      REQUIRE(z.sh >= 0 && z.sh < 8192 && code >= 0 && code < 2048 && z.pt >= 0 && z.pt < S, "state left its range");
      if (code) at.push_back(i);
    }
    p = p + 1 == S ? 0 : p + 1;
  }
  for (size_t a = 1; a < at.size(); ++a)
    if (at[a] - at[a - 1] < *min_gap) *min_gap = at[a] - at[a - 1];
  // every call length n: the events with index < n fit the cap's slots exactly as the kernel stores them
  for (int n = 1; n <= i; ++n) {
    const int cap = psk_event_cap(n, S);
    std::vector<int32_t> slots((size_t)cap);
    int cnt = 0;
    for (int v : at)
      if (v < n) { REQUIRE(cnt < cap, "event %d of a call of %d outputs does not fit %d slots", cnt + 1, n, cap); slots.data()[cnt++] = psk_pack(v, 1); }
    if (cnt * 1000L / cap > *worst_fill) *worst_fill = cnt * 1000L / cap;
  }
}

template <int S>
static long slots() {
  pysdr_psk_cfg c = good_cfg();
  c.n0 = 1; c.lo = 1e-6f; c.hi = 1e-6f;
  long seqs = 0, fill = 0;
  int gap = 1 << 30;
  constexpr int N = 5;
  int choice[N];
  const int shs[5] = {0, 1, 2, 4097, 8190};                        // nothing pending, 1, 10 (the next 0 emits), overflow marks
  for (int code = 0; code < 7776; ++code) {                        // 6^5 sequences
    int v = code;
    for (int k = 0; k < N; ++k) { choice[k] = v % 6; v /= 6; }
    for (int si = 0; si < 5; ++si)
      for (int cnt0 = 1; cnt0 < 3 * S / 2; cnt0 += (code % 7 == 0 ? 1 : S / 2)) {
        PskDec z = psk_dec_init(S);
        z.sh = shs[si]; z.cnt = cnt0; z.open = 1; z.seen = 1; z.pt = code % S; z.cr = 1.f;
        drive<S>(c, z, (code / 3) % S, choice, N, &gap, &fill);
        ++seqs;
      }
  }
  REQUIRE(gap == psk_event_gap(S), "S %d: two events %d samples apart, the bound is %d", S, gap, psk_event_gap(S));
  REQUIRE(fill == 1000, "S %d: no call fills its slots (%ld / 1000)", S, fill);
  return seqs;
}

int main() {
  const pysdr_psk_cfg cfg = good_cfg();
  PskPlan p;
  // ---- refusals
  REQUIRE(!psk_plan(0, 8, 16, &cfg, &p) && !psk_plan(-1, 8, 16, &cfg, &p) && psk_plan(1, 8, 16, &cfg, &p), "nk");
  REQUIRE(psk_plan(8192, 8, 16, &cfg, &p) && !psk_plan(8193, 8, 16, &cfg, &p) && psk_plan(5461, 12, 16, &cfg, &p) && !psk_plan(5462, 12, 16, &cfg, &p), "nk NSUB <= 2^18");
  for (int S : {-8, 0, 1, 4, 7, 9, 10, 11, 13, 16, 24}) REQUIRE(!psk_plan(4, S, 16, &cfg, &p), "S %d accepted", S);
  REQUIRE(!psk_plan(4, 8, 0, &cfg, &p) && !psk_plan(4, 8, -5, &cfg, &p) && !psk_plan(4, 8, kPskMaxOutMax + 1, &cfg, &p) && psk_plan(4, 8, kPskMaxOutMax, &cfg, &p), "max_out");
  REQUIRE(!psk_plan(4, 8, 16, nullptr, &p), "NULL cfg");
  {
    const float nan = __builtin_nanf(""), inf = __builtin_inff();
    float pysdr_psk_cfg::* const fl[] = {&pysdr_psk_cfg::a_t, &pysdr_psk_cfg::a_q, &pysdr_psk_cfg::hi, &pysdr_psk_cfg::lo, &pysdr_psk_cfg::hy, &pysdr_psk_cfg::pmax};
    for (size_t k = 0; k < sizeof fl / sizeof fl[0]; ++k)
      for (float v : {0.f, -1.f, nan, inf, -inf}) { pysdr_psk_cfg b = cfg; b.*fl[k] = v; REQUIRE(!psk_plan(4, 8, 16, &b, &p), "float field %zu = %g accepted", k, (double)v); }
    for (int k = 0; k < 2; ++k) { pysdr_psk_cfg b = cfg; b.*fl[k] = 1.0000001f; REQUIRE(!psk_plan(4, 8, 16, &b, &p), "a > 1"); b.*fl[k] = 1.f; REQUIRE(psk_plan(4, 8, 16, &b, &p), "a = 1"); }
    pysdr_psk_cfg b = cfg; b.lo = 0.8f; REQUIRE(!psk_plan(4, 8, 16, &b, &p), "lo > hi"); b.lo = b.hi; REQUIRE(psk_plan(4, 8, 16, &b, &p), "lo = hi");
    b = cfg; b.pmax = 1.1e18f; REQUIRE(!psk_plan(4, 8, 16, &b, &p), "pmax");
    b = cfg; b.n0 = 0; REQUIRE(!psk_plan(4, 8, 16, &b, &p), "n0 0"); b.n0 = kPskSettleMax + 1; REQUIRE(!psk_plan(4, 8, 16, &b, &p), "n0"); b.n0 = 1; REQUIRE(psk_plan(4, 8, 16, &b, &p), "n0 1");
  }
  // ---- plans and tile walks
  long plans = 0, steps = 0;
  const int outs[9] = {1, 2, 15, 16, kPskTile - 1, kPskTile, kPskTile + 1, 2 * kPskTile + 3, 256};
  for (int S : {8, 12})
    for (int nk : {1, 2, 3, 4, 5, 9})
      for (int mo : outs) {
        REQUIRE(psk_plan(nk, S, mo, &cfg, &p), "nk %d S %d max_out %d refused", nk, S, mo);
        REQUIRE(p.cap == mo / (3 * S / 2) + 1 && p.nsub == 4 * S && p.nfine == nk * 4 * S, "cap %d", p.cap);
        REQUIRE(p.ypitch >= kPskHpad + mo && p.ypitch % 16 == 0 && p.ypitch < kPskHpad + mo + 16 && kPskHpad >= 2 * S - 1, "pitch %d", p.ypitch);
        REQUIRE(p.groups * psk_rows(S) >= nk && (p.groups - 1) * psk_rows(S) < nk, "nk %d: %d groups", nk, p.groups);
        ++plans;
        for (int n_out : {mo, mo > 1 ? mo - 1 : 1})
          steps += S == 8 ? walk<8>(nk, n_out, p) : walk<12>(nk, n_out, p);
      }
  long filtered = 0;
  for (int S : {8, 12})
    for (int nk : {1, 3, 5, 9})
      for (int n_out : {1, 2 * S - 2, kPskTile, kPskTile + 1, 2 * kPskTile + 3}) {
        REQUIRE(psk_plan(nk, S, 256, &cfg, &p), "plan");
        filtered += S == 8 ? filter_check<8>(nk, n_out, 1000003L + n_out, p) : filter_check<12>(nk, n_out, 1000003L + n_out, p);
      }
  REQUIRE(PskGeom<8>::kThreads == 64 && PskGeom<12>::kThreads == 192 && PskGeom<8>::kLdsBytes == 5424 && PskGeom<12>::kLdsBytes == 15168, "geometry");
  REQUIRE(PskGeom<8>::kYp % 2 == 1 && PskGeom<12>::kYp % 2 == 1 && psk_threads(8) % 64 == 0 && psk_threads(12) % 64 == 0, "geometry");
  for (int S : {8, 12})
    for (int j = 0; j < 4 * S; ++j) {
      const int q = 2 * j - 4 * S + 1, NT = 32 * S;
      REQUIRE(psk_qmod(j, S) == ((q % NT) + NT) % NT, "qmod");
      for (long m : {0L, 1L, 255L, 383L, 1000003L}) REQUIRE(psk_mulmod(psk_qmod(j, S), (int)(m % NT), NT) == (int)((((long)q * m) % NT + NT) % NT), "phase index");
    }
  // ---- event slots
  const long seqs = slots<8>() + slots<12>();
  // ---- the event word
  for (int i : {0, 1, 2047, 2048, kPskMaxOutMax - 1})
    for (int c : {1, 2, 3, 1023, 2047}) {
      const int32_t w = psk_pack(i, c);
      REQUIRE(w >= 0 && psk_event_index(w) == i && psk_event_code(w) == c, "word (%d, %d)", i, c);
    }
  REQUIRE(sizeof(pysdr_psk_cfg) == 28 && sizeof(PskC) == 8, "layouts %zu %zu", sizeof(pysdr_psk_cfg), sizeof(PskC));
  printf("psk plan: %ld plans, %ld outputs walked, %ld outputs filtered and held against the definition, %ld symbol sequences, closest events 3 S / 2 apart\nPSK_PLAN_OK\n", plans, steps, filtered, seqs);
  return 0;
}
