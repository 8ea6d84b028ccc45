// The FT4 skimmer's plan, staging geometry, steps and event slots (pysdr_amd/csrc/ft4_plan.h, the very code ft4.hip steps
// with) on the CPU under AddressSanitizer + UBSan.
//   * the rules: S in {48, 72}, nk >= 1, nk S / 2 <= 2^18, max_out in [1, 2^20], the ring's byte limit and the settings'
//     rules; one workgroup per row, the row pitch holds the history's room and max_out, cap and ring depth as written.
//   * the tile walk of the spectrum kernel, through the index functions of Ft4Geom that ft4.hip itself uses, over streams
//     cut into calls: every staging load goes to a Y of exactly nk x pitch elements and an LDS tile of exactly kYp
//     elements (heap: the sanitizer guards both ends), every sample of a call and of the history is loaded exactly once,
//     every step of the stream is computed exactly once, in its call -- at every call position, found by brute force from
//     the stream -- its window holds outputs QS t .. QS t + S - 1 in order, and the history roll reads and writes inside
//     the row.
//   * the spectrum (ft4_bin) on that walk with real samples against a plain sum over the row's memory, bit for bit; a
//     NaN, an infinite and an over-pmax sample blank exactly the steps whose window holds them.
//   * ft4_sync's symbol and tone tables (ft4_costas_sym, ft4_costas, ft4_data_sym, ft4_gray) against the lists written out.
//   * the sync score (ft4_sync), the peak rule (ft4_peak) and the soft bits (ft4_llr_bit) on a ring of random powers with
//     frames planted in it, against plain transcriptions of steps 2 and 3 that index by absolute step.
//   * the cap proof: over random and adversarial score sequences two events of a decoder are never closer than 5 steps,
//     the closest ARE 5 apart, and the events of every call of every length fit exactly `cap` slots.
//   * the ring-depth rule: for every way of cutting a stream into calls of at most max_out outputs, a frame emitted in a
//     call is still valid for pysdr_ft4_llr at the end of the next call, and at the end of the first call that completes
//     step t0 + 416; ft4_llr_ok's window is [done - TR, done - 409].
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ft4_plan.h"

using namespace pysdr;

#define REQUIRE(c, ...) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static pysdr_ft4_cfg good_cfg() {
  pysdr_ft4_cfg c{};
  c.smin = 4.f; c.hmin = 12; c.pmax = 1e18f;
  return c;
}

static unsigned g_rng = 2025u;
static float rnd() { g_rng = g_rng * 1664525u + 1013904223u; return (float)((int)(g_rng >> 8) - (1 << 23)) / (float)(1 << 23); }
static float rnd01() { return 0.5f * (rnd() + 1.f); }

// One row group of a stream cut into calls: the walk of ft4_spectrum_kernel with real samples.  `stream` holds the row's
// outputs from the stream's start; every step is held against the definition computed from the stream itself.
template <int S>
static long walk_stream(int nk, const std::vector<int>& calls, const Ft4Plan& p, float pmax) {
  using G = Ft4Geom<S>;
  constexpr int NT = G::kNt, NB = G::kNb, TH = G::kThreads, QS = G::kQs;
  long total = 0;
  for (int n : calls) total += n;
  std::vector<Ft8C> tw((size_t)NT);
  for (int t = 0; t < NT; ++t) tw[(size_t)t] = Ft8C{(float)cos(2 * M_PI * t / NT), (float)-sin(2 * M_PI * t / NT)};
  std::vector<std::vector<Ft8C>> stream((size_t)nk, std::vector<Ft8C>((size_t)total));
  std::vector<std::vector<char>> bad((size_t)nk, std::vector<char>((size_t)total, 0));
  for (int r = 0; r < nk; ++r)
    for (long i = 0; i < total; ++i) stream[(size_t)r][(size_t)i] = Ft8C{rnd(), rnd()};
  auto poke = [&](int r, long i, Ft8C v, bool blanks) { if (r < nk && i >= 0 && i < total) { stream[(size_t)r][(size_t)i] = v; bad[(size_t)r][(size_t)i] = blanks; } };
  poke(0, 3, Ft8C{__builtin_nanf(""), 0.25f}, true);
  poke(nk - 1, total / 2, Ft8C{-0.5f, __builtin_inff()}, true);
  poke(nk / 2, total - 1, Ft8C{3e19f, 0.f}, true);
  poke(nk - 1, total / 3, Ft8C{1e6f, 1e6f}, false);                 // large, below pmax: kept
  const long T = (long)ft8_steps_done((unsigned long long)total, S);
  std::vector<int> computed((size_t)nk * (size_t)(T > 0 ? T : 1), 0);
  std::vector<Ft8C> Y((size_t)nk * p.ypitch, Ft8C{0.f, 0.f});       // as allocated and reset: a.y = Y + kFt4Hpad
  long m0 = 0, t_done = 0, blanked = 0, checked = 0;
  for (int n_out : calls) {
    REQUIRE(n_out <= p.ypitch - kFt4Hpad, "a call of %d outputs", n_out);
    for (int r = 0; r < nk; ++r)                                     // the channelizer's pass
      for (int i = 0; i < n_out; ++i) Y.data()[(size_t)r * p.ypitch + kFt4Hpad + i] = stream[(size_t)r][(size_t)(m0 + i)];
    if (n_out == 0) continue;                                        // nothing launched
    const long t1 = (long)ft8_steps_done((unsigned long long)(m0 + n_out), S);
    const int ns = (int)(t1 - t_done);
    REQUIRE(ns >= 0 && ns <= ft4_steps_per_call(p.ypitch - kFt4Hpad, S), "%d steps in a call of %d", ns, n_out);
    // brute force: the steps whose last output QS t + S - 1 falls into [m0, m0 + n_out)
    int brute = 0;
    for (long t = 0; t < T; ++t) brute += (QS * t + S - 1 >= m0 && QS * t + S - 1 < m0 + n_out) ? 1 : 0;
    REQUIRE(brute == ns, "%d steps end in the call, the plan says %d", brute, ns);
    const int e_first = ns > 0 ? (int)(QS * t_done + S - 1 - m0) : 0;
    REQUIRE(e_first >= 0 && e_first < (t_done ? QS : S), "e_first %d", e_first);
    for (int row = 0; row < nk; ++row) {                             // a workgroup
      std::vector<int> loads((size_t)p.ypitch, 0);
      std::vector<Ft8C> tile((size_t)G::kYp);
      std::vector<long> from((size_t)G::kYp, -1000000L);             // call-relative output held by every LDS slot
      const size_t yb = (size_t)row * p.ypitch + kFt4Hpad;
      int done_in_call = 0;
      for (int i0 = 0; i0 < n_out; i0 += G::kTile) {
        std::vector<Ft8C> carry((size_t)G::kCarry);
        std::vector<long> cfrom((size_t)G::kCarry);
        for (int tid = 0; tid < G::kCarry; ++tid) {
          if (i0 > 0) { carry[(size_t)tid] = tile.data()[G::carry_src(tid)]; cfrom[(size_t)tid] = from.data()[G::carry_src(tid)]; }
          else { carry[(size_t)tid] = Y.data()[yb + G::hist_off(tid)]; cfrom[(size_t)tid] = G::hist_off(tid); loads.data()[kFt4Hpad + G::hist_off(tid)] += 1; }
        }
        std::vector<int> written((size_t)G::kYp, 0);
        for (int tid = 0; tid < G::kCarry; ++tid) { tile.data()[G::carry_dst(tid)] = carry[(size_t)tid]; from.data()[G::carry_dst(tid)] = cfrom[(size_t)tid]; written.data()[G::carry_dst(tid)] += 1; }
        for (int tid = 0; tid < TH; ++tid)
          for (int c = tid; c < G::kTile; c += TH) {
            const int i = i0 + c;
            Ft8C v{0.f, 0.f};
            if (i < n_out) { v = Y.data()[yb + i]; loads.data()[kFt4Hpad + i] += 1; }
            tile.data()[G::stage_dst(c)] = v; from.data()[G::stage_dst(c)] = i; written.data()[G::stage_dst(c)] += 1;
          }
        for (int k = 0; k < G::kYp; ++k) REQUIRE(written[(size_t)k] == 1, "LDS slot %d written %d x", k, written[(size_t)k]);
        for (int tid = 0; tid < TH; ++tid) {
          const bool has = tid < G::kItems;
          const int s = has ? G::item_step(tid) : 0, b = has ? G::item_bin(tid) : 0;
          REQUIRE(s >= 0 && s < kFt4StepsPerSym && b >= 0 && b < NB, "item");
          const int u = G::tile_step(i0, e_first, s);
          if (!(has && u >= 0 && u < ns)) continue;
          const long t = t_done + u;
          const int w0 = G::win(e_first, s);
          REQUIRE(w0 >= 0 && w0 + S <= G::kYp, "window at %d", w0);
          for (int i = 0; i < S; ++i)
            REQUIRE(from.data()[w0 + i] == QS * t + i - m0 && QS * t + i - m0 < n_out, "step %ld tap %d holds output %ld", t, i, from.data()[w0 + i]);
          const float pw = ft4_bin<S>(tile.data() + w0, tw.data(), ft4_qmod(b, S), pmax);
          // the definition, from the stream
          const long q = 2 * b - (NB - 1);
          float ar = 0.f, ai = 0.f;
          bool reach = false;
          for (int i = 0; i < S; ++i) {
            const Ft8C y = stream[(size_t)row][(size_t)(QS * t + i)], w = tw[(size_t)((((q * i) % NT) + NT) % NT)];
            reach = reach || bad[(size_t)row][(size_t)(QS * t + i)];
            const float vr = y.x * w.x - y.y * w.y, vi = y.x * w.y + y.y * w.x;
            if (i == 0) { ar = vr; ai = vi; } else { ar = ar + vr; ai = ai + vi; }
          }
          float want = ar * ar + ai * ai;
          const bool blank = !(want <= pmax);
          REQUIRE(blank == reach, "row %d step %ld bin %d: blanked %d, a bad sample in reach %d", row, t, b, (int)blank, (int)reach);
          if (blank) { want = 0.f; ++blanked; }
          REQUIRE(memcmp(&pw, &want, 4) == 0 && pw == pw, "row %d step %ld bin %d: %g, the definition's %g", row, t, b, (double)pw, (double)want);
          ++checked;
          if (b == 0) { computed.data()[(size_t)row * T + t] += 1; ++done_in_call; }
        }
      }
      REQUIRE(done_in_call == ns, "row %d: %d of %d steps", row, done_in_call, ns);
      for (int i = 0; i < p.ypitch; ++i) {
        const int rel = i - kFt4Hpad;
        REQUIRE(loads[(size_t)i] == ((rel >= -(S - 1) && rel < n_out) ? 1 : 0), "(%d, %d) loaded %d x", row, rel, loads[(size_t)i]);
      }
      std::vector<Ft8C> keep((size_t)(S - 1));                        // the roll: reads first, then writes
      for (int j = 0; j < S - 1; ++j) {
        const long src = kFt4Hpad + G::roll_src(n_out, j), dst = kFt4Hpad + G::roll_dst(j);
        REQUIRE(src >= 0 && src < p.ypitch && dst >= 0 && dst < kFt4Hpad, "roll");
        keep[(size_t)j] = Y.data()[(size_t)row * p.ypitch + src];
      }
      for (int j = 0; j < S - 1; ++j) Y.data()[(size_t)row * p.ypitch + kFt4Hpad + G::roll_dst(j)] = keep[(size_t)j];
      for (int j = 0; j < S - 1; ++j) {                              // the history is the stream's last S - 1 outputs (zeros before it)
        const long k = m0 + n_out - (S - 1) + j;
        const Ft8C h = Y[yb + G::hist_off(j)], w = k >= 0 ? stream[(size_t)row][(size_t)k] : Ft8C{0.f, 0.f};
        REQUIRE(memcmp(&h, &w, 8) == 0, "history %d after output %ld", j, m0 + n_out);
      }
    }
    m0 += n_out;
    t_done = t1;
  }
  REQUIRE(t_done == T, "steps");
  for (size_t k = 0; k < (size_t)nk * (size_t)T; ++k) REQUIRE(computed[k] == 1, "step %zu computed %d x", k, computed[k]);
  if (T > 8) REQUIRE(blanked > 0 && blanked < checked, "%ld of %ld blanked", blanked, checked);
  return checked;
}

// ---- the tables, steps 2 and 3 and the soft bits as the definition writes them, indexed by absolute step ---------------
static const int kSyncSym[16] = {0, 1, 2, 3, 33, 34, 35, 36, 66, 67, 68, 69, 99, 100, 101, 102};
static const int kSyncTone[16] = {0, 1, 3, 2, 1, 0, 2, 3, 2, 3, 1, 0, 3, 2, 0, 1};   // A, B, C, D
static const int kGray4[4] = {0, 1, 3, 2};

static void tables_check() {
  for (int n = 0; n < 16; ++n) REQUIRE(ft4_costas_sym(n) == kSyncSym[n] && ft4_costas(n) == kSyncTone[n], "sync symbol %d: (%d, %d)", n, ft4_costas_sym(n), ft4_costas(n));
  for (int v = 0; v < 4; ++v) REQUIRE(ft4_gray(v) == kGray4[v], "Gray");
  for (int blk = 0; blk < 4; ++blk) {                                // each array is a permutation of the four tones, and no two agree anywhere
    int seen = 0;
    for (int k = 0; k < 4; ++k) seen |= 1 << ft4_costas(4 * blk + k);
    REQUIRE(seen == 15, "array %d", blk);
    for (int other = 0; other < blk; ++other)
      for (int k = 0; k < 4; ++k) REQUIRE(ft4_costas(4 * blk + k) != ft4_costas(4 * other + k), "arrays %d and %d agree at %d", blk, other, k);
  }
  std::vector<int> seen(103, 0), order;
  for (int n = 0; n < 16; ++n) seen[(size_t)ft4_costas_sym(n)] += 1;
  for (int d = 0; d < 87; ++d) { seen[(size_t)ft4_data_sym(d)] += 1; order.push_back(ft4_data_sym(d)); }
  for (int s = 0; s < 103; ++s) REQUIRE(seen[(size_t)s] == 1, "symbol %d", s);
  for (size_t d = 1; d < order.size(); ++d) REQUIRE(order[d] > order[d - 1], "data symbols ascend");
  REQUIRE(ft4_data_sym(0) == 4 && ft4_data_sym(28) == 32 && ft4_data_sym(29) == 37 && ft4_data_sym(57) == 65 && ft4_data_sym(58) == 70 && ft4_data_sym(86) == 98, "data blocks");
  REQUIRE(kFt4Lag == 408 && kFt4EmitLag == 412 && kFt4Hold == 417 && kFt4Bits == 174 && kFt8Keep == 9 && kFt8MinGap == 5, "constants");
}

static long sync_check(int S, int max_out) {
  const int nsub = S / 2, nb = nsub + 6, tr = ft4_ring_steps(max_out, S);
  const long T = 700;
  std::vector<float> P((size_t)T * nb);                              // by absolute step
  for (auto& v : P) v = rnd01();
  // frames planted at (t0, j): the Costas tones and random data, strong
  const int plant[4][2] = {{3, 0}, {40, nsub - 1}, {200, 15}, {204, 16}};   // no two share a bin
  for (auto& pl : plant)
    for (int sym = 0; sym < kFt4Syms; ++sym) {
      int tone = (int)(rnd01() * 3.99f);
      for (int n = 0; n < 16; ++n) if (kSyncSym[n] == sym) tone = kSyncTone[n];
      P[(size_t)(pl[0] + 4 * sym) * nb + pl[1] + 2 * tone] += 20.f + rnd01();
    }
  long checked = 0, events = 0;
  std::vector<float> sc((size_t)kFt8Keep * nsub, 0.f), all((size_t)T * nsub, -1.f);
  std::vector<int32_t> hi((size_t)kFt8Keep * nsub, 0), allh((size_t)T * nsub, 0);
  std::vector<float> ring((size_t)tr * nb, 0.f);
  // Uniform random powers hit a sync symbol with chance 1 / 4, twelve of sixteen about once in 30000 scores, and this check
  // makes some 25000: it counts the planted frames, so it asks for 14 hits (the peak rule is held against the
  // transcription at every score either way).
  pysdr_ft4_cfg c = good_cfg();
  c.hmin = 14;
  for (long t = 0; t < T; ++t) {
    memcpy(ring.data() + (size_t)(t % tr) * nb, P.data() + (size_t)t * nb, nb * sizeof(float));
    const long t0 = t - kFt4Lag;
    if (t0 < 0) continue;
    for (int j = 0; j < nsub; ++j) {
      const Ft8Score z = ft4_sync(ring.data(), tr, nb, (int)(t0 % tr), j);
      float sig = 0.f, tot = 0.f;
      int hits = 0;
      for (int n = 0; n < 16; ++n) {
        const float* p = P.data() + (size_t)(t0 + 4 * kSyncSym[n]) * nb + j;
        const float e = p[2 * kSyncTone[n]];
        sig = sig + e;
        float r = p[0];
        r = r + p[2]; r = r + p[4]; r = r + p[6];
        tot = tot + r;
        int hit = 1;
        for (int tone = 0; tone < 4; ++tone) if (tone != kSyncTone[n] && !(e > p[2 * tone])) hit = 0;
        hits += hit;
      }
      const float den = tot - sig, three = 3.f * sig;
      const float want = den > 0.f ? three / den : 0.f;
      REQUIRE(memcmp(&want, &z.score, 4) == 0 && hits == z.hits, "t0 %ld decoder %d: score %g hits %d, the transcription's %g %d", t0, j, (double)z.score, z.hits, (double)want, hits);
      sc[(size_t)(t0 % kFt8Keep) * nsub + j] = z.score; hi[(size_t)(t0 % kFt8Keep) * nsub + j] = z.hits;
      all[(size_t)t0 * nsub + j] = z.score; allh[(size_t)t0 * nsub + j] = z.hits;
      ++checked;
      const long tc = t0 - kFt8Reach;
      if (tc < 0) continue;
      const bool ev = ft4_peak(sc.data() + j, hi.data() + j, nsub, tc, c);
      bool want_ev = all[(size_t)tc * nsub + j] >= c.smin && allh[(size_t)tc * nsub + j] >= c.hmin;
      for (int d = 1; d <= 4 && want_ev; ++d) {
        if (tc - d >= 0 && !(all[(size_t)tc * nsub + j] > all[(size_t)(tc - d) * nsub + j])) want_ev = false;
        if (!(all[(size_t)tc * nsub + j] >= all[(size_t)(tc + d) * nsub + j])) want_ev = false;
      }
      REQUIRE(ev == want_ev, "t0 %ld decoder %d: event %d, the transcription's %d", tc, j, (int)ev, (int)want_ev);
      if (ev) {
        // a planted frame with all 16 hits; the four arrays differ in every place, so a frame has no image 33 symbols away
        bool planted = false;
        for (auto& pl : plant) planted = planted || (tc == pl[0] && j == pl[1]);
        REQUIRE(planted && allh[(size_t)tc * nsub + j] == 16, "an event at (%ld, %d) with %d hits", tc, j, allh[(size_t)tc * nsub + j]);
        ++events;
        // its soft bits, while the frame is in the ring
        REQUIRE(ft4_llr_ok(j, tc, t + 1, nsub, tr), "valid at its emission");
        for (int i = 0; i < kFt4Bits; ++i) {
          const int d = i / 2, sym = d < 29 ? 4 + d : (d < 58 ? 37 + d - 29 : 70 + d - 58), mask = 2 >> (i % 2);
          float m1 = -1.f, m0 = -1.f;
          for (int v = 0; v < 4; ++v) {
            const float pv = P[(size_t)(tc + 4 * sym) * nb + j + 2 * kGray4[v]];
            if (v & mask) m1 = pv > m1 ? pv : m1; else m0 = pv > m0 ? pv : m0;
          }
          const float want_l = m1 - m0, got = ft4_llr_bit(ring.data(), tr, nb, (int)(tc % tr), j, i);
          REQUIRE(memcmp(&want_l, &got, 4) == 0, "soft bit %d of (%ld, %d)", i, tc, j);
        }
      }
    }
  }
  REQUIRE(events == 4, "S %d: %ld events; 4 frames were planted (two of them a symbol and a raster step apart: each decoder sees its own)", S, events);
  return checked;
}

// ---- the cap: events of one decoder over score sequences, stored call by call as the kernel stores them ------------------
static long cap_check(int S) {
  const pysdr_ft4_cfg c = good_cfg();
  long seqs = 0, fill = 0;
  int gap = 1 << 30;
  for (int kind = 0; kind < 40; ++kind) {
    const int T = 400;
    std::vector<float> score((size_t)T);
    for (int t = 0; t < T; ++t) {
      switch (kind % 5) {
        case 0: score[(size_t)t] = 4.f + 10.f * rnd01(); break;                                   // noise above smin
        case 1: score[(size_t)t] = 5.f; break;                                                   // a plateau: ties
        case 2: score[(size_t)t] = (t % 5 == kind % 5) ? 9.f : 4.f; break;                       // a peak every 5 steps: the closest the rule allows
        case 3: score[(size_t)t] = (t % 4 == 0) ? 9.f : 4.f; break;                              // every 4: equal peaks inside each other's reach
        default: score[(size_t)t] = 4.f + (float)(t % 7) + (float)((t * 37) % 11); break;
      }
    }
    std::vector<int> at;
    float sc[kFt8Keep] = {0};
    int32_t hi[kFt8Keep] = {0};
    for (int t0 = 0; t0 < T; ++t0) {
      sc[t0 % kFt8Keep] = score[(size_t)t0]; hi[t0 % kFt8Keep] = 16;
      const long tc = t0 - kFt8Reach;
      if (tc >= 0 && ft4_peak(sc, hi, 1, tc, c)) at.push_back(t0);   // the step index (shifted by a constant) at which it is emitted
    }
    for (size_t a = 1; a < at.size(); ++a) if (at[a] - at[a - 1] < gap) gap = at[a] - at[a - 1];
    // every call of ns steps beginning at every step: the events in it fit the cap of the smallest max_out that gives ns
    for (int max_out : {1, S / 4 - 1, S / 4, 4 * (S / 4), 5 * (S / 4) - 1, 9 * (S / 4), 16, 256, 1000}) {
      const int spc = ft4_steps_per_call(max_out, S), cap = ft4_event_cap(max_out, S);
      for (int first = 0; first + spc <= T; ++first) {
        std::vector<int32_t> slots((size_t)cap * kFt8EventWords);
        int cnt = 0;
        for (int v : at)
          if (v >= first && v < first + spc) {
            REQUIRE(cnt < cap, "event %d of a call of %d steps does not fit %d slots", cnt + 1, spc, cap);
            slots.data()[kFt8EventWords * cnt] = ft8_pack(v - first, 16); slots.data()[kFt8EventWords * cnt + 1] = 0; ++cnt;
          }
        if (cnt * 1000L / cap > fill) fill = cnt * 1000L / cap;
      }
    }
    ++seqs;
  }
  REQUIRE(gap == kFt8MinGap, "S %d: two events %d steps apart, the bound is %d", S, gap, kFt8MinGap);
  REQUIRE(fill == 1000, "S %d: no call fills its slots (%ld / 1000)", S, fill);
  return seqs;
}

// ---- the ring depth: every cut of a stream into calls --------------------------------------------------------------------
static long ring_check(int S, int max_out) {
  const int QS = S / 4, tr = ft4_ring_steps(max_out, S), spc = ft4_steps_per_call(max_out, S);
  long cases = 0;
  for (int trial = 0; trial < 100; ++trial) {
    long m = 0;
    std::vector<long> ends;                                          // steps done at the end of every call
    const long total = 500L * QS + S + (long)(rnd01() * 300 * QS);
    while (m < total) {
      int n = trial % 4 == 0 ? max_out : (trial % 4 == 1 ? 1 + (int)(rnd01() * (max_out - 0.01f)) : (rnd01() < 0.5f ? max_out : (int)(rnd01() * 3)));
      if (n > max_out) n = max_out;
      m += n;
      ends.push_back((long)ft8_steps_done((unsigned long long)m, S));
    }
    for (size_t k = 1; k < ends.size(); ++k) REQUIRE(ends[k] - ends[k - 1] <= spc, "%ld steps in a call, at most %d", ends[k] - ends[k - 1], spc);
    size_t a = 0;
    for (long t0 = 0; t0 + kFt4Hold < ends.back(); t0 += 1 + trial % 3) {
      while (ends[a] <= t0 + kFt4EmitLag) ++a;                       // the call that emits t0
      REQUIRE(ft4_llr_ok(0, t0, ends[a], 1, tr), "t0 %ld invalid at the end of its own call", t0);
      if (a + 1 < ends.size()) REQUIRE(ft4_llr_ok(0, t0, ends[a + 1], 1, tr), "t0 %ld gone a call later (%ld done, ring %d)", t0, ends[a + 1], tr);
      size_t b = a;
      while (ends[b] < t0 + kFt4Hold) ++b;                           // the call at whose end the host releases it
      REQUIRE(ft4_llr_ok(0, t0, ends[b], 1, tr), "t0 %ld gone at its release (%ld done, ring %d)", t0, ends[b], tr);
      ++cases;
    }
  }
  // the window itself
  for (long done : {409L, 500L, (long)tr, (long)tr + 1, 100000L}) {
    for (long t0 = -2; t0 <= done; ++t0) {
      const bool want = t0 >= 0 && t0 <= done - 409 && t0 >= done - tr;
      REQUIRE(ft4_llr_ok(0, t0, done, 1, tr) == want, "done %ld t0 %ld", done, t0);
    }
    REQUIRE(!ft4_llr_ok(-1, done - 409, done, 1, tr) && !ft4_llr_ok(1, done - 409, done, 1, tr) && ft4_llr_ok(6, done - 409, done, 7, tr), "F");
  }
  return cases;
}

int main() {
  const pysdr_ft4_cfg cfg = good_cfg();
  Ft4Plan p;
  // ---- refusals
  REQUIRE(!ft4_plan(0, 48, 16, &cfg, &p) && !ft4_plan(-1, 48, 16, &cfg, &p) && ft4_plan(1, 48, 16, &cfg, &p), "nk");
  REQUIRE(ft4_plan(10922, 48, 16, &cfg, &p) && !ft4_plan(10923, 48, 16, &cfg, &p) && ft4_plan(7281, 72, 16, &cfg, &p) && !ft4_plan(7282, 72, 16, &cfg, &p), "nk S / 2 <= 2^18");
  for (int S : {-48, 0, 1, 12, 24, 47, 49, 64, 71, 73, 96, 144}) REQUIRE(!ft4_plan(4, S, 16, &cfg, &p), "S %d accepted", S);
  REQUIRE(!ft4_plan(4, 48, 0, &cfg, &p) && !ft4_plan(4, 48, -5, &cfg, &p) && !ft4_plan(4, 48, kFt4MaxOutMax + 1, &cfg, &p) && ft4_plan(4, 48, kFt4MaxOutMax, &cfg, &p), "max_out");
  REQUIRE(!ft4_plan(4, 48, 16, nullptr, &p), "NULL cfg");
  {
    const float nan = __builtin_nanf(""), inf = __builtin_inff();
    for (float v : {-1.f, -1e-30f, nan, inf, -inf}) { pysdr_ft4_cfg b = cfg; b.smin = v; REQUIRE(!ft4_plan(4, 48, 16, &b, &p), "smin %g accepted", (double)v); }
    for (float v : {0.f, -1.f, nan, inf, -inf, 1.1e18f}) { pysdr_ft4_cfg b = cfg; b.pmax = v; REQUIRE(!ft4_plan(4, 48, 16, &b, &p), "pmax %g accepted", (double)v); }
    for (int v : {-1, 17, 21, 1 << 30}) { pysdr_ft4_cfg b = cfg; b.hmin = v; REQUIRE(!ft4_plan(4, 48, 16, &b, &p), "hmin %d accepted", v); }
    pysdr_ft4_cfg b = cfg; b.smin = 0.f; b.hmin = 0; b.pmax = 1e18f; REQUIRE(ft4_plan(4, 48, 16, &b, &p), "the rules' edges");
    b.hmin = 16; b.smin = 1e30f; b.pmax = 1e-30f; REQUIRE(ft4_plan(4, 48, 16, &b, &p), "the rules' edges");
  }
  // the ring's byte limit: nk TR NB 4 <= 2^30
  REQUIRE(ft4_plan(10922, 48, 256, &cfg, &p) && p.ring_bytes == 10922LL * 461 * 30 * 4 && p.ring_bytes <= kFt4RingBytesMax, "ring of 10922 rows");
  REQUIRE(!ft4_plan(10922, 48, 4096, &cfg, &p) && ft4_plan(512, 48, 4096, &cfg, &p), "a ring above the limit");
  REQUIRE(ft4_plan(1, 48, kFt4MaxOutMax, &cfg, &p) && p.ring_bytes == 1LL * (417 + 2 * 87382) * 30 * 4, "one row at the largest max_out");
  // ---- plans
  long plans = 0;
  for (int S : {48, 72})
    for (int nk : {1, 3, 32, 512})
      for (int mo : {1, 11, 12, 13, 15, 16, 17, 18, 19, 47, 48, 49, 71, 72, 73, 256, 1000}) {
        REQUIRE(ft4_plan(nk, S, mo, &cfg, &p), "nk %d S %d max_out %d refused", nk, S, mo);
        const int spc = mo / (S / 4) + 1;
        REQUIRE(p.cap == spc / 5 + 1 && p.nsub == S / 2 && p.nb == S / 2 + 6 && p.nfine == nk * (S / 2) && p.groups == nk, "plan");
        REQUIRE(p.tr == 417 + 2 * spc && p.tr > kFt4Lag + 1 && p.ring_bytes == (long long)nk * p.tr * p.nb * 4, "ring");
        REQUIRE(p.ypitch >= kFt4Hpad + mo && p.ypitch % 16 == 0 && p.ypitch < kFt4Hpad + mo + 16 && kFt4Hpad >= S - 1, "pitch %d", p.ypitch);
        ++plans;
      }
  REQUIRE(Ft4Geom<48>::kThreads == 128 && Ft4Geom<72>::kThreads == 192 && Ft4Geom<48>::kItems == 120 && Ft4Geom<72>::kItems == 168, "geometry");
  REQUIRE(Ft4Geom<48>::kLdsBytes == 2296 && Ft4Geom<72>::kLdsBytes == 3448 && Ft4Geom<48>::kNb == 30 && Ft4Geom<72>::kNb == 42, "geometry");
  REQUIRE(kFt4Hpad % 16 == 0 && kFt4Hpad >= 71 && kFt4Hpad < 71 + 16, "the history's room");
  for (int S : {48, 72})
    for (int b = 0; b < S / 2 + 6; ++b) {
      const int q = 2 * b - (S / 2 + 5), NT = 4 * S;
      REQUIRE(ft4_qmod(b, S) == ((q % NT) + NT) % NT, "qmod");
    }
  tables_check();
  REQUIRE(ft8_steps_done(0, 48) == 0 && ft8_steps_done(47, 48) == 0 && ft8_steps_done(48, 48) == 1 && ft8_steps_done(59, 48) == 1 && ft8_steps_done(60, 48) == 2, "steps");
  REQUIRE(ft8_steps_done(71, 72) == 0 && ft8_steps_done(72, 72) == 1 && ft8_steps_done(90, 72) == 2 && ft8_steps_done(7000, 48) == 580, "steps");
  // ---- the tile walk and the spectrum, over streams cut into calls
  long bins = 0;
  for (int S : {48, 72})
    for (int nk : {1, 3}) {
      REQUIRE(ft4_plan(nk, S, 256, &cfg, &p), "plan");
      const int QS = S / 4;
      const std::vector<std::vector<int>> cuts = {
          {256, 256, 256}, {1, 0, 2, QS - 1, 1, QS, QS + 1, S - 1, S, S + 1, 0, 2 * S + 5, 256, 7, 255},
          {S - 1, 1, 1, QS - 1, 1}, {S, QS, QS, 2 * S, 2 * S + 1, 2 * S - 1}, {3, 200, 1, 1, 1, 130, 64}};
      for (auto& c : cuts) bins += S == 48 ? walk_stream<48>(nk, c, p, 1e18f) : walk_stream<72>(nk, c, p, 1e18f);
      // every call position: a call of every length from 0 to 2 S + 1 behind every residue of the stream's length mod S
      for (int lead = 0; lead <= S; lead += 5)
        for (int len : {1, QS - 1, QS, S - 1, S, S + 1, 2 * S + 1})
          bins += S == 48 ? walk_stream<48>(nk, {S + lead, len, len, 3}, p, 1e18f) : walk_stream<72>(nk, {S + lead, len, len, 3}, p, 1e18f);
    }
  REQUIRE(ft4_plan(2, 48, 16, &cfg, &p), "plan");
  bins += walk_stream<48>(2, std::vector<int>(40, 16), p, 1e18f) + walk_stream<48>(2, {5, 11, 16, 0, 16, 1, 15, 16, 16, 16, 9}, p, 1e18f);
  REQUIRE(ft4_plan(2, 72, 16, &cfg, &p), "plan");
  bins += walk_stream<72>(2, std::vector<int>(40, 16), p, 1e18f);
  // ---- sync, peak and soft bits against the transcription; the cap; the ring
  const long scored = sync_check(48, 256) + sync_check(72, 256) + sync_check(48, 16);
  const long seqs = cap_check(48) + cap_check(72);
  long rings = 0;
  for (int S : {48, 72})
    for (int mo : {1, 16, 18, 100, 256, 1000}) rings += ring_check(S, mo);
  // ---- the event words
  for (int u : {0, 1, 31, 32, 87381, 87382})
    for (int h : {0, 1, 12, 16, 31}) {
      const int32_t w = ft8_pack(u, h);
      REQUIRE(w >= 0 && ft8_event_step(w) == u && ft8_event_hits(w) == h, "word (%d, %d)", u, h);
    }
  REQUIRE(ft4_steps_per_call(kFt4MaxOutMax, 48) == 87382, "the largest step index");
  REQUIRE(sizeof(pysdr_ft4_cfg) == 12 && sizeof(Ft8C) == 8, "layouts %zu %zu", sizeof(pysdr_ft4_cfg), sizeof(Ft8C));
  printf("ft4 plan: %ld plans, %ld bins walked and held against the definition, %ld scores beside the transcription, %ld score sequences "
         "with events 5 steps apart at the closest, %ld frames followed through cut streams\nFT4_PLAN_OK\n", plans, bins, scored, seqs, rings);
  return 0;
}
