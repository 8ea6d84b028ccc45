// The RTTY raster skimmer's plan, staging geometry, steps and event slots (pysdr_amd/csrc/fsk_plan.h, the very code fsk.hip
// steps with) on the CPU under AddressSanitizer + UBSan.
//   * the rules: S in {22, 33}, nk >= 1, nk S <= 2^18, max_out in [1, 2^20] and the settings' rules; the groups tile
//     [0, nk), the row pitch holds the history's room and max_out, the event cap is max_out / (6 S + S / 2 + 1) + 1.
//   * the tile walk of the kernel, through the index functions of FskGeom that fsk.hip itself uses: every staging load
//     goes to a Y of exactly nk x pitch elements and an LDS tile of exactly rows x pitch elements (heap: the sanitizer
//     guards both ends), every decoder's window stays inside the tile and sees sample m - i at tap i, every (row, output)
//     is consumed exactly once and in order, the lanes beyond the last decoder read a valid row, and the history roll
//     reads and writes inside the row.
//   * the tone filter (fsk_tone) on that walk with real samples, heap-backed tables and tile, for both tones of every
//     decoder against a plain sum over the row's memory, bit for bit; a NaN, an infinite and an over-pmax sample blank
//     exactly the outputs whose window reaches them.
//   * the step (fsk_step) against a plain transcription of steps 2 and 3 of the definition on random tone powers whose
//     decisions frame characters: every state field after every output, floats by their bits.
//   * the event slots: the step driven by EVERY sequence of decisions over two characters -- the wait in front of the
//     start edge, the start bit's sample, four data patterns (the two shifts among them), the stop bit's sample -- from
//     every start count, output by output as the kernel counts, storing into exactly `cap` slots for every call length:
//     two events are never closer than 6 S + S / 2 + 1 outputs, the closest ARE that far apart, and the count never
//     exceeds the cap.
//   * the event word round-trips.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fsk_plan.h"

using namespace pysdr;

#define REQUIRE(c, ...) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static pysdr_fsk_cfg good_cfg() {
  pysdr_fsk_cfg c{};
  c.a_q = 1.f / 64; c.a_b = 1.f / 32; c.hi = 0.8f; c.lo = 0.65f; c.bal = 0.25f; c.pmax = 1e18f; c.n0 = 64;
  return c;
}

// the kernel's thread -> (row of the workgroup, decoder of the row); the lanes beyond the last decoder take (0, 0)
template <int S>
static void thread_of(int tid, bool* has, int* r, int* j) {
  using G = FskGeom<S>;
  *has = tid < G::kDecoders;
  *r = *has ? tid / G::kNsub : 0;
  *j = *has ? tid - *r * G::kNsub : 0;
}

template <int S>
static long walk(int nk, int n_out, const FskPlan& p) {
  using G = FskGeom<S>;
  constexpr int ROWS = G::kRows, TH = G::kThreads, YP = G::kYp;
  std::vector<int> loads((size_t)nk * p.ypitch, 0);              // Y as allocated: a.y = Y + kFskHpad
  long steps = 0;
  for (int g = 0; g < p.groups; ++g) {
    const int row0 = g * ROWS;
    std::vector<long> tile((size_t)ROWS * YP);
    std::vector<int> next((size_t)TH, 0);
    for (int i0 = 0; i0 < n_out; i0 += kFskTile) {
      std::vector<long> carry((size_t)TH, -1L);
      REQUIRE(G::kCarry <= TH, "a thread per carried sample");
      for (int tid = 0; tid < G::kCarry; ++tid) {                  // the S - 1 in front: history, or the last tile's end
        const int hr = G::carry_row(tid), hc = G::carry_col(tid);
        if (i0 > 0) carry[(size_t)tid] = tile.data()[(size_t)G::carry_src(hr, hc)];
        else if (row0 + hr < nk) { carry[(size_t)tid] = (long)(row0 + hr) * p.ypitch + kFskHpad + G::hist_off(hc); loads.data()[carry[(size_t)tid]] += 1; }
      }
      std::fill(tile.begin(), tile.end(), -2L);
      for (int tid = 0; tid < G::kCarry; ++tid) {
        long& slot = tile.data()[(size_t)G::carry_dst(G::carry_row(tid), G::carry_col(tid))];
        REQUIRE(slot == -2, "carried slot written twice");
        slot = carry[(size_t)tid];
      }
      for (int tid = 0; tid < TH; ++tid)
        for (int k = tid; k < ROWS * kFskTile; k += TH) {
          const int rr = G::stage_row(k), c = G::stage_col(k), i = i0 + c;
          long v = -1;
          if (row0 + rr < nk && i < n_out) {
            v = (long)(row0 + rr) * p.ypitch + kFskHpad + i;
            loads.data()[v] += 1;
          }
          long& slot = tile.data()[(size_t)G::stage_dst(rr, c)];
          REQUIRE(slot == -2, "LDS slot written twice");
          slot = v;
        }
      for (size_t k = 0; k < tile.size(); ++k) REQUIRE(tile[k] != -2, "LDS slot %zu never written", k);
      const int nj = n_out - i0 < kFskTile ? n_out - i0 : kFskTile;
      for (int tid = 0; tid < TH; ++tid) {
        bool has; int r, j;
        thread_of<S>(tid, &has, &r, &j);
        const int row = row0 + r;
        for (int jj = 0; jj < nj; ++jj) {
          for (int i = 0; i < S; ++i) {
            const long v = tile.data()[(size_t)G::win(r, jj) - i];
            if (row < nk) REQUIRE(v == (long)row * p.ypitch + kFskHpad + i0 + jj - i, "tap %d of output %d reads %ld", i, i0 + jj, v);
            else REQUIRE(v == -1, "a thread without a row reads memory");
          }
          if (has && row < nk) { REQUIRE(next[(size_t)tid] == i0 + jj, "out of order"); next[(size_t)tid] += 1; ++steps; }
        }
      }
    }
    for (int tid = 0; tid < TH; ++tid) {
      bool has; int r, j;
      thread_of<S>(tid, &has, &r, &j);
      const int row = row0 + r;
      if (!has || row >= nk) continue;
      REQUIRE(next[(size_t)tid] == n_out, "thread %d walked %d of %d", tid, next[(size_t)tid], n_out);
      if (j < S - 1) {                                             // the history roll
        const long src = (long)row * p.ypitch + kFskHpad + G::roll_src(n_out, j), dst = (long)row * p.ypitch + kFskHpad + G::roll_dst(j);
        REQUIRE(src >= (long)row * p.ypitch && src < (long)(row + 1) * p.ypitch && dst >= (long)row * p.ypitch && dst < (long)row * p.ypitch + kFskHpad, "roll");
        loads.data()[src] += 0;
        loads.data()[dst] += 0;
      }
    }
  }
  for (int r = 0; r < nk; ++r)
    for (int i = 0; i < p.ypitch; ++i) {
      const int rel = i - kFskHpad;                                // the history and the call's outputs: read once each
      const int want = (rel >= -(S - 1) && rel < n_out) ? 1 : 0;
      REQUIRE(loads[(size_t)r * p.ypitch + i] == want, "nk %d n_out %d: (%d, %d) loaded %d x, expected %d", nk, n_out, r, rel, loads[(size_t)r * p.ypitch + i], want);
    }
  return steps;
}

static std::vector<float> window(int S) {                          // kaiser(S, 8.6) scaled to sum 1, in float64, rounded once
  auto i0 = [](double x) { double s = 1, t = 1; for (int k = 1; k < 60; ++k) { t *= (x / 2) / k; s += t * t; } return s; };
  std::vector<double> w((size_t)S);
  double sum = 0;
  for (int i = 0; i < S; ++i) { const double r = 2.0 * i / (S - 1) - 1.0; w[(size_t)i] = i0(8.6 * sqrt(1 - r * r)) / i0(8.6); sum += w[(size_t)i]; }
  std::vector<float> g((size_t)S);
  for (int i = 0; i < S; ++i) g[(size_t)i] = (float)(w[(size_t)i] / sum);
  return g;
}

// fsk_tone itself, on the tile walk above with real samples: Y of exactly nk x pitch samples, an LDS tile of exactly
// rows x YP samples, tw and g of exactly NT and S (all heap: the sanitizer guards both ends), from a first output m0 deep
// in a stream.  Both tones of every (row, decoder, output) are held against a plain sum over the row's memory, float for
// float in the definition's order (bit-equal: contraction is off), and the outputs blanked are exactly those whose window
// reaches a NaN, an infinite or an over-pmax sample; a large sample below pmax is not blanked.
template <int S>
static long tone_check(int nk, int n_out, long m0, const FskPlan& p) {
  using G = FskGeom<S>;
  constexpr int NT = G::kNt, ROWS = G::kRows, TH = G::kThreads, YP = G::kYp;
  const float pmax = 1e18f;
  std::vector<FskC> tw((size_t)NT), Y((size_t)nk * p.ypitch, FskC{7e30f, -7e30f});   // what is never staged would blank
  const std::vector<float> g = window(S);
  for (int t = 0; t < NT; ++t) tw[(size_t)t] = FskC{(float)cos(2 * M_PI * t / NT), (float)-sin(2 * M_PI * t / NT)};
  unsigned rng = 12345u + (unsigned)(nk * 131 + n_out);
  auto rnd = [&]() { rng = rng * 1664525u + 1013904223u; return (float)((int)(rng >> 8) - (1 << 23)) / (float)(1 << 23); };
  std::vector<char> bad((size_t)nk * p.ypitch, 0);
  for (int r = 0; r < nk; ++r)
    for (int i = -(S - 1); i < n_out; ++i) Y[(size_t)r * p.ypitch + kFskHpad + i] = FskC{rnd(), rnd()};
  auto poke = [&](int r, int i, FskC v, bool blanks) {
    if (r < nk && i < n_out) { Y[(size_t)r * p.ypitch + kFskHpad + i] = v; bad[(size_t)r * p.ypitch + kFskHpad + i] = blanks; }
  };
  poke(0, 3, FskC{__builtin_nanf(""), 0.25f}, true);
  poke(nk - 1, n_out / 2, FskC{-0.5f, __builtin_inff()}, true);
  poke(nk / 2, n_out - 1, FskC{3e19f, 0.f}, true);
  poke(0, -(S - 1), FskC{0.f, -3e19f}, true);                     // in the history
  poke(nk - 1, kFskTile - 1, FskC{1e6f, 1e6f}, false);             // large, below pmax: kept
  long checked = 0, blanked = 0;
  for (int g0 = 0; g0 < p.groups; ++g0) {
    const int row0 = g0 * ROWS;
    std::vector<FskC> tile((size_t)ROWS * YP);
    for (int i0 = 0; i0 < n_out; i0 += kFskTile) {
      std::vector<FskC> carry((size_t)G::kCarry, FskC{0.f, 0.f});
      for (int tid = 0; tid < G::kCarry; ++tid) {
        const int hr = G::carry_row(tid), hc = G::carry_col(tid);
        if (i0 > 0) carry[(size_t)tid] = tile.data()[G::carry_src(hr, hc)];
        else if (row0 + hr < nk) carry[(size_t)tid] = Y.data()[(size_t)(row0 + hr) * p.ypitch + kFskHpad + G::hist_off(hc)];
      }
      for (int tid = 0; tid < G::kCarry; ++tid) tile.data()[G::carry_dst(G::carry_row(tid), G::carry_col(tid))] = carry[(size_t)tid];
      for (int k = 0; k < ROWS * kFskTile; ++k) {
        const int rr = G::stage_row(k), c = G::stage_col(k), i = i0 + c;
        FskC v{0.f, 0.f};
        if (row0 + rr < nk && i < n_out) v = Y.data()[(size_t)(row0 + rr) * p.ypitch + kFskHpad + i];
        tile.data()[G::stage_dst(rr, c)] = v;
      }
      const int nj = n_out - i0 < kFskTile ? n_out - i0 : kFskTile;
      for (int tid = 0; tid < TH; ++tid) {
        bool has; int r, j;
        thread_of<S>(tid, &has, &r, &j);
        const int row = row0 + r;
        if (!has || row >= nk) continue;
        for (int tone : {j, j + kFskToneGap}) {
          const int qm = fsk_qmod(tone, S);
          const long q = 2 * tone - S - 14;
          for (int jj = 0; jj < nj; ++jj) {
            const long m = m0 + i0 + jj;
            const int t = fsk_mulmod(qm, (int)(m % NT), NT);
            const float pw = fsk_tone<S>(tile.data() + G::win(r, jj), tw.data(), g.data(), t, qm, pmax);
            // the definition, from the row's memory
            float ar = 0.f, ai = 0.f;
            bool reach = false;
            for (int i = 0; i < S; ++i) {
              const size_t at = (size_t)row * p.ypitch + kFskHpad + i0 + jj - i;
              const FskC y = Y[at], w = tw[(size_t)((((q * (m - i)) % NT) + NT) % NT)];
              reach = reach || bad[at];
              const float vr = y.x * w.x - y.y * w.y, vi = y.x * w.y + y.y * w.x;
              if (i == 0) { ar = g[0] * vr; ai = g[0] * vi; }
              else { ar = ar + g[(size_t)i] * vr; ai = ai + g[(size_t)i] * vi; }
            }
            float want = ar * ar + ai * ai;
            const bool blank = !(want <= pmax);
            REQUIRE(blank == reach, "row %d tone %d output %d: blanked %d, a bad sample in reach %d", row, tone, i0 + jj, (int)blank, (int)reach);
            if (blank) { want = 0.f; ++blanked; }
            REQUIRE(memcmp(&pw, &want, 4) == 0 && pw == pw, "row %d tone %d output %d: filter %g, definition %g", row, tone, i0 + jj, (double)pw, (double)want);
            ++checked;
          }
        }
      }
    }
  }
  if (n_out > 4 * S) REQUIRE(blanked > 0 && blanked < checked, "%ld of %ld outputs blanked", blanked, checked);   // both kinds were seen
  return checked;
}

// ---- steps 2 and 3 as the definition writes them, on variables of their own ------------------------------------------------
struct Plain {
  float qn = 0, qd = 0, bm = 0, bs = 0;
  int st = 0, cnt, sh = 0, nb = 0, prev = 1, fig = 0, open = 0, seen = 0;
};

static int plain_step(Plain& z, const pysdr_fsk_cfg& c, int S, float PS, float PM) {
  const int d = PM > PS;
  int code = -1;
  z.cnt -= 1;
  if (z.st == 0 && z.prev == 1 && d == 0) { z.st = 1; z.cnt = S / 2; }
  else if (z.cnt == 0) {
    int inch = z.st != 0, framed = 0;
    switch (z.st) {
      case 0: z.cnt = S; break;
      case 1: if (d == 0) { z.st = 2; z.nb = 0; z.sh = 0; z.cnt = S; } else { z.st = 0; z.cnt = S; inch = 0; } break;
      case 2: z.sh |= d << z.nb; z.nb += 1; z.cnt = S; if (z.nb == 5) z.st = 3; break;
      default: framed = d == 1; z.st = 0; z.cnt = S; break;
    }
    const float w = fmaxf(PM, PS), l = fminf(PM, PS);
    { const float diff = w - l, e = diff - z.qn, s = c.a_q * e; z.qn = z.qn + s; }
    { const float sum = w + l, e = sum - z.qd, s = c.a_q * e; z.qd = z.qd + s; }
    if (inch && d) { const float e = PM - z.bm, s = c.a_b * e; z.bm = z.bm + s; }
    if (inch && !d) { const float e = PS - z.bs, s = c.a_b * e; z.bs = z.bs + s; }
    if (z.seen < c.n0) { z.seen += 1; z.open = 0; }
    else {
      const float thr = (z.open ? c.lo : c.hi) * z.qd, floor = c.bal * fmaxf(z.bm, z.bs);
      z.open = z.qd > 0 && z.qn >= thr && fminf(z.bm, z.bs) >= floor;
    }
    if (framed) {
      if (z.open) code = z.sh + 32 * z.fig;
      if (z.sh == 27) z.fig = 1;
      if (z.sh == 31) z.fig = 0;
    }
  }
  z.prev = d;
  return code;
}

template <int S>
static long step_check() {
  pysdr_fsk_cfg c = good_cfg();
  c.n0 = 5;
  FskDec z = fsk_dec_init(S);
  Plain w;
  w.cnt = S;
  unsigned rng = 99u + S;
  auto rnd = [&]() { rng = rng * 1664525u + 1013904223u; return (float)(rng >> 8) / (float)(1 << 24); };
  long events = 0, n = 0;
  int figs = 0;
  // characters of random data and stop lengths keyed onto two levels with noise: mark 1 +- 0.3, space 0.9 +- 0.3 where
  // keyed, 0.1 +- 0.1 where not; now and then a dropout on both tones, an equal pair and a burst of decisions at random
  for (int ch = 0; ch < 4000; ++ch) {
    const int data = ch % 9 == 0 ? 27 : (ch % 9 == 4 ? 31 : (int)(rnd() * 32) & 31);
    const int stop = S + (int)(rnd() * 2 * S);
    int bits[8] = {0, data & 1, (data >> 1) & 1, (data >> 2) & 1, (data >> 3) & 1, (data >> 4) & 1, 1, 1};
    const int mode = ch % 50 == 17 ? 1 : (ch % 50 == 33 ? 2 : 0);   // 1: decisions at random, 2: both tones silent
    for (int k = 0; k < 6 * S + stop; ++k) {
      const int b = bits[k / S < 7 ? k / S : 7];
      float PM = b ? 1.f + 0.3f * (rnd() - 0.5f) : 0.1f * rnd(), PS = b ? 0.1f * rnd() : 0.9f + 0.3f * (rnd() - 0.5f);
      if (mode == 1) { PM = rnd(); PS = rnd(); }
      if (mode == 2) { PM = 0.f; PS = 0.f; }
      if (k == 3 && ch % 7 == 0) PS = PM;
      const int a = fsk_step<S>(z, c, PS, PM), b2 = plain_step(w, c, S, PS, PM);
      REQUIRE(a == b2, "S %d output %ld: code %d, the transcription's %d", S, n, a, b2);
      REQUIRE(memcmp(&z.qn, &w.qn, 4) == 0 && memcmp(&z.qd, &w.qd, 4) == 0 && memcmp(&z.bm, &w.bm, 4) == 0 && memcmp(&z.bs, &w.bs, 4) == 0,
              "S %d output %ld: floats (%g %g %g %g), the transcription's (%g %g %g %g)", S, n, (double)z.qn, (double)z.qd, (double)z.bm, (double)z.bs,
              (double)w.qn, (double)w.qd, (double)w.bm, (double)w.bs);
      REQUIRE(z.st == w.st && z.cnt == w.cnt && z.sh == w.sh && z.nb == w.nb && z.prev == w.prev && z.fig == w.fig && z.open == w.open && z.seen == w.seen,
              "S %d output %ld: ints", S, n);
      REQUIRE(z.st >= 0 && z.st <= 3 && z.cnt >= 1 && z.cnt <= S && z.sh >= 0 && z.sh < 32 && z.nb >= 0 && z.nb <= 5 && a < 64, "state left its range");
      if (a >= 0) { ++events; if (a >= 32) ++figs; }
      ++n;
    }
  }
  REQUIRE(events > 2000 && figs > 200 && figs < events, "S %d: %ld events, %d in figures", S, events, figs);
  return n;
}

// ---- the event slots -------------------------------------------------------------------------------------------------------
// One decoder driven through two characters: per character a wait of mark in front of the start edge (0: the edge comes at
// once), the decision at the start bit's sample, one of four data patterns and the decision at the stop bit's sample.
// Between the samples the decisions are the bit's own, so the walk is what the state machine can see.
template <int S>
static void drive(const pysdr_fsk_cfg& c, FskDec z, const int* choice, int nchar, int* min_gap, long* worst_fill) {
  static const int waits[4] = {0, 1, S - 1, S + 3};
  static const int datas[4] = {0, 27, 31, 21};
  std::vector<int> at;                                             // output index of every event
  int i = 0;
  auto out = [&](int d) {
    z.qn = 1e6f; z.qd = 1e6f; z.bm = 1.f; z.bs = 1.f;              // the squelch stays open
    const int code = fsk_step<S>(z, c, d ? 0.f : 1.f, d ? 1.f : 0.f);
    REQUIRE(z.cnt >= 1 && z.cnt <= S && code < 64, "cnt %d", z.cnt);
    if (code >= 0) at.push_back(i);
    ++i;
  };
  if (z.st == 3) {                                                 // a call that begins inside a character: its stop bit first
    while (z.cnt > 1) out(1);
    out(1);
  }
  for (int k = 0; k < nchar; ++k) {
    const int wait = waits[choice[k] & 3], start = (choice[k] >> 2) & 1, data = datas[(choice[k] >> 3) & 3], stop = (choice[k] >> 5) & 1;
    for (int s = 0; s < wait; ++s) out(1);
    if (z.st == 0 && z.prev == 0) out(1);                         // after a bad stop bit an edge needs one output of mark
    out(0);                                                        // the edge
    if (z.st != 1) continue;                                       // (the edge fell on a character under way)
    while (z.cnt > 1) out(0);
    out(start);                                                    // the start bit's sample: 0 is a start bit, 1 a glitch
    if (z.st != 2) continue;
    for (int b = 0; b < 5; ++b) {
      const int d = (data >> b) & 1;
      while (z.cnt > 1) out(d);
      out(d);
    }
    while (z.cnt > 1) out(stop);
    out(stop);                                                     // the stop bit's sample: 1 frames the character
  }
  for (size_t a = 1; a < at.size(); ++a)
    if (at[a] - at[a - 1] < *min_gap) *min_gap = at[a] - at[a - 1];
  // every call length n: the events with index < n fit the cap's slots exactly as the kernel stores them
  for (int n = 1; n <= i; ++n) {
    const int cap = fsk_event_cap(n, S);
    std::vector<int32_t> slots((size_t)cap);
    int cnt = 0;
    for (int v : at)
      if (v < n) { REQUIRE(cnt < cap, "event %d of a call of %d outputs does not fit %d slots", cnt + 1, n, cap); slots.data()[cnt++] = fsk_pack(v, 1); }
    if (cnt * 1000L / cap > *worst_fill) *worst_fill = cnt * 1000L / cap;
  }
}

template <int S>
static long slots() {
  pysdr_fsk_cfg c = good_cfg();
  c.n0 = 1;
  long seqs = 0, fill = 0;
  int gap = 1 << 30;
  int choice[2];
  for (int c0 = 0; c0 < 64; ++c0)
    for (int c1 = 0; c1 < 64; ++c1) {
      choice[0] = c0; choice[1] = c1;
      // start states: hunting, or in front of a stop bit's sample (the call's first output may emit), with every count
      for (int st0 : {0, 3})
        for (int cnt0 = 1; cnt0 <= S; cnt0 += ((c0 * 64 + c1) % 5 == 0 ? 1 : S / 2)) {
          FskDec z = fsk_dec_init(S);
          z.st = st0; z.cnt = cnt0; z.open = 1; z.seen = 1; z.fig = c1 & 1; z.sh = c0 & 31; z.nb = st0 == 3 ? 5 : 0;
          drive<S>(c, z, choice, 2, &gap, &fill);
          ++seqs;
        }
    }
  REQUIRE(gap == fsk_event_gap(S), "S %d: two events %d outputs apart, the bound is %d", S, gap, fsk_event_gap(S));
  REQUIRE(fill == 1000, "S %d: no call fills its slots (%ld / 1000)", S, fill);
  return seqs;
}

int main() {
  const pysdr_fsk_cfg cfg = good_cfg();
  FskPlan p;
  // ---- refusals
  REQUIRE(!fsk_plan(0, 22, 16, &cfg, &p) && !fsk_plan(-1, 22, 16, &cfg, &p) && fsk_plan(1, 22, 16, &cfg, &p), "nk");
  REQUIRE(fsk_plan(11915, 22, 16, &cfg, &p) && !fsk_plan(11916, 22, 16, &cfg, &p) && fsk_plan(7943, 33, 16, &cfg, &p) && !fsk_plan(7944, 33, 16, &cfg, &p), "nk S <= 2^18");
  for (int S : {-22, 0, 1, 8, 11, 12, 21, 23, 32, 34, 44, 66}) REQUIRE(!fsk_plan(4, S, 16, &cfg, &p), "S %d accepted", S);
  REQUIRE(!fsk_plan(4, 22, 0, &cfg, &p) && !fsk_plan(4, 22, -5, &cfg, &p) && !fsk_plan(4, 22, kFskMaxOutMax + 1, &cfg, &p) && fsk_plan(4, 22, kFskMaxOutMax, &cfg, &p), "max_out");
  REQUIRE(!fsk_plan(4, 22, 16, nullptr, &p), "NULL cfg");
  {
    const float nan = __builtin_nanf(""), inf = __builtin_inff();
    float pysdr_fsk_cfg::* const fl[] = {&pysdr_fsk_cfg::a_q, &pysdr_fsk_cfg::a_b, &pysdr_fsk_cfg::hi, &pysdr_fsk_cfg::lo, &pysdr_fsk_cfg::bal, &pysdr_fsk_cfg::pmax};
    for (size_t k = 0; k < sizeof fl / sizeof fl[0]; ++k)
      for (float v : {0.f, -1.f, nan, inf, -inf}) { pysdr_fsk_cfg b = cfg; b.*fl[k] = v; REQUIRE(!fsk_plan(4, 22, 16, &b, &p), "float field %zu = %g accepted", k, (double)v); }
    for (int k = 0; k < 5; ++k) {
      pysdr_fsk_cfg b = cfg; b.hi = 1.f; b.*fl[k] = 1.0000001f; REQUIRE(!fsk_plan(4, 22, 16, &b, &p), "field %d > 1", k);
      b.*fl[k] = 1.f; REQUIRE(fsk_plan(4, 22, 16, &b, &p), "field %d = 1", k);
    }
    pysdr_fsk_cfg b = cfg; b.lo = 0.85f; REQUIRE(!fsk_plan(4, 22, 16, &b, &p), "lo > hi"); b.lo = b.hi; REQUIRE(fsk_plan(4, 22, 16, &b, &p), "lo = hi");
    b = cfg; b.pmax = 1.1e18f; REQUIRE(!fsk_plan(4, 22, 16, &b, &p), "pmax");
    b = cfg; b.n0 = 0; REQUIRE(!fsk_plan(4, 22, 16, &b, &p), "n0 0"); b.n0 = kFskSettleMax + 1; REQUIRE(!fsk_plan(4, 22, 16, &b, &p), "n0"); b.n0 = 1; REQUIRE(fsk_plan(4, 22, 16, &b, &p), "n0 1");
  }
  // ---- plans and tile walks
  long plans = 0, steps = 0;
  const int outs[9] = {1, 2, 31, 32, kFskTile - 1, kFskTile, kFskTile + 1, 2 * kFskTile + 3, 256};
  for (int S : {22, 33})
    for (int nk : {1, 4, 7, 8, 9, 15, 17})
      for (int mo : outs) {
        REQUIRE(fsk_plan(nk, S, mo, &cfg, &p), "nk %d S %d max_out %d refused", nk, S, mo);
        REQUIRE(p.cap == mo / (6 * S + S / 2 + 1) + 1 && p.nsub == S && p.nfine == nk * S, "cap %d", p.cap);
        REQUIRE(p.ypitch >= kFskHpad + mo && p.ypitch % 16 == 0 && p.ypitch < kFskHpad + mo + 16 && kFskHpad >= S - 1, "pitch %d", p.ypitch);
        REQUIRE(p.groups * fsk_rows(S) >= nk && (p.groups - 1) * fsk_rows(S) < nk, "nk %d: %d groups", nk, p.groups);
        ++plans;
        for (int n_out : {mo, mo > 1 ? mo - 1 : 1})
          steps += S == 22 ? walk<22>(nk, n_out, p) : walk<33>(nk, n_out, p);
      }
  long filtered = 0;
  for (int S : {22, 33})
    for (int nk : {1, 4, 9})
      for (int n_out : {1, S - 2, kFskTile, kFskTile + 1, 2 * kFskTile + 3}) {
        REQUIRE(fsk_plan(nk, S, 256, &cfg, &p), "plan");
        filtered += S == 22 ? tone_check<22>(nk, n_out, 1000003L + n_out, p) : tone_check<33>(nk, n_out, 1000003L + n_out, p);
      }
  REQUIRE(FskGeom<22>::kThreads == 192 && FskGeom<33>::kThreads == 256 && FskGeom<22>::kLdsBytes == 6936 && FskGeom<33>::kLdsBytes == 7620, "geometry");
  REQUIRE(FskGeom<22>::kDecoders == 176 && FskGeom<33>::kDecoders == 231 && fsk_threads(22) % 64 == 0 && fsk_threads(33) % 64 == 0, "geometry");
  for (int S : {22, 33})
    for (int t = 0; t < S + kFskToneGap; ++t) {
      const int q = 2 * t - S - 14, NT = 8 * S;
      REQUIRE(fsk_qmod(t, S) == ((q % NT) + NT) % NT, "qmod");
      for (long m : {0L, 1L, 175L, 263L, 1000003L}) REQUIRE(fsk_mulmod(fsk_qmod(t, S), (int)(m % NT), NT) == (int)((((long)q * m) % NT + NT) % NT), "phase index");
    }
  for (int S : {22, 33})
    for (int j = 0; j < S; ++j)                                    // space below, mark above the decoder's centre 2 j - S + 1, 15 baud / 8 each
      REQUIRE((2 * j - S - 14) + 15 == 2 * j - S + 1 && (2 * (j + kFskToneGap) - S - 14) - 15 == 2 * j - S + 1, "tones");
  // ---- the step against the transcription, and the event slots
  const long stepped = step_check<22>() + step_check<33>();
  const long seqs = slots<22>() + slots<33>();
  // ---- the event word
  for (int i : {0, 1, 63, 64, kFskMaxOutMax - 1})
    for (int c : {0, 1, 27, 31, 32, 63}) {
      const int32_t w = fsk_pack(i, c);
      REQUIRE(w >= 0 && fsk_event_index(w) == i && fsk_event_code(w) == c, "word (%d, %d)", i, c);
    }
  REQUIRE(sizeof(pysdr_fsk_cfg) == 28 && sizeof(FskC) == 8, "layouts %zu %zu", sizeof(pysdr_fsk_cfg), sizeof(FskC));
  printf("fsk plan: %ld plans, %ld outputs walked, %ld tone outputs filtered and held against the definition, %ld outputs stepped beside the "
         "transcription, %ld decision sequences, closest events 6 S + S / 2 + 1 apart\nFSK_PLAN_OK\n", plans, steps, filtered, stepped, seqs);
  return 0;
}
