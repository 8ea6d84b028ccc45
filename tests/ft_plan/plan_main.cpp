// The FT8 and FT4 skimmers' plan, staging geometry, steps and event slots (pysdr_amd/csrc/ft_plan.h, the very code ft.hip
// steps with) on the CPU under AddressSanitizer + UBSan.  `plan_main ft8`, `plan_main ft4`, or both without an argument.
// Written once and run for each mode:
//   * the rules: S one of the mode's two, nk >= 1, nk S / 2 <= 2^18, max_out in [1, 2^20], the ring's byte limit and the
//     settings' rules; one workgroup per row, the row pitch holds the history's room and max_out, cap and ring depth as
//     written.
//   * the tile walk of the spectrum kernel, through the index functions of FtGeom that ft.hip itself uses, over streams
//     cut into calls: every staging load goes to a Y of exactly nk x pitch elements and an LDS tile of exactly kYp
//     elements (heap: the sanitizer guards both ends), every sample of a call and of the history is loaded exactly once,
//     every step of the stream is computed exactly once, in its call -- at every call position, found by brute force from
//     the stream -- its window holds outputs QS t .. QS t + S - 1 in order, and the history roll reads and writes inside
//     the row.
//   * the spectrum (ft_bin) on that walk with real samples against a plain sum over the row's memory, bit for bit; a
//     NaN, an infinite and an over-pmax sample blank exactly the steps whose window holds them.
//   * the peak rule (ft_peak) against a transcription that indexes by absolute step, at every score.
//   * the cap proof: over random and adversarial score sequences two events of a decoder are never closer than 5 steps,
//     the closest ARE 5 apart, and the events of every call of every length fit exactly `cap` slots.
//   * the ring-depth rule: for every way of cutting a stream into calls of at most max_out outputs, a frame emitted in a
//     call is still valid for pysdr_*_llr at the end of the next call, and at the end of the first call that completes
//     step t0 + hold - 1; ft_llr_ok's window is [done - TR, done - (lag + 1)].
//   * the event words round-trip.
// Written out by hand for each mode, in Ref8 and Ref4 -- the reference the traits of ft_plan.h are held against, so nothing
// in them is taken from the traits: the tables, the sync score (ft_sync) and the soft bits (ft_llr_bit) as the definition
// writes them, on a ring of random powers with frames planted in it, and every expected number.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "ft_plan.h"

using namespace pysdr;

#define REQUIRE(c, ...) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static unsigned g_rng = 0;
static float rnd() { g_rng = g_rng * 1664525u + 1013904223u; return (float)((int)(g_rng >> 8) - (1 << 23)) / (float)(1 << 23); }
static float rnd01() { return 0.5f * (rnd() + 1.f); }

// ---- FT8 as the definition writes it -------------------------------------------------------------------------------------
struct Ref8 {
  typedef pysdr_ft8_cfg PublicCfg;
  static constexpr unsigned kSeed = 2024u;
  static constexpr const char* kLower = "ft8";
  static constexpr const char* kMarker = "FT8_PLAN_OK";
  static FtCfg good_cfg() {
    FtCfg c{};
    c.smin = 3.f; c.hmin = 13; c.pmax = 1e18f;
    return c;
  }
  static FtCfg sync_cfg() { return good_cfg(); }
  // the expected numbers
  static constexpr int kS0 = 64, kS1 = 96, kLag = 312, kEmitLag = 316, kHold = 321, kExtra = 14, kSyms = 79, kSync = 21;
  static constexpr int kNkMax0 = 8192, kNkMax1 = 5461;                // nk S / 2 <= 2^18
  static constexpr long long kRingOfNkMax0 = 8192LL * 355 * 46 * 4;   // max_out 256
  static constexpr int kSpcMax = 65537;                               // steps of a call of 2^20 outputs at S0
  static constexpr long long kRingOfOneRow = 1LL * (321 + 2 * 65537) * 46 * 4;
  static constexpr int kThreads0 = 192, kThreads1 = 256, kItems0 = 184, kItems1 = 248, kLds0 = 3064, kLds1 = 4600, kNb0 = 46, kNb1 = 62;
  static constexpr int kHpadLeast = 95;
  static constexpr long kRingCheckSteps = 400;
  static std::vector<int> bad_S() { return {-64, 0, 1, 22, 32, 48, 63, 65, 95, 97, 128, 192}; }
  static std::vector<int> bad_hmin() { return {-1, 22, 1 << 30}; }
  static std::vector<int> plan_nk() { return {1, 3, 80, 512}; }
  static std::vector<int> plan_max_out() { return {1, 15, 16, 17, 23, 24, 25, 63, 64, 65, 95, 96, 97, 256, 1000}; }
  static std::vector<int> ring_max_out() { return {1, 16, 24, 100, 256, 1000}; }
  static std::vector<int> word_steps() { return {0, 1, 31, 32, 65536, 65537}; }
  static std::vector<int> word_hits() { return {0, 1, 13, 21, 31}; }
  static void steps_check() {
    REQUIRE(ft_steps_done(0, 64) == 0 && ft_steps_done(63, 64) == 0 && ft_steps_done(64, 64) == 1 && ft_steps_done(79, 64) == 1 && ft_steps_done(80, 64) == 2, "steps");
    REQUIRE(ft_steps_done(95, 96) == 0 && ft_steps_done(96, 96) == 1 && ft_steps_done(120, 96) == 2 && ft_steps_done(8400, 96) == 347, "steps");
  }

  static constexpr int kCostas[7] = {3, 1, 4, 0, 6, 5, 2};
  static constexpr int kGray[8] = {0, 1, 3, 2, 5, 6, 4, 7};
  static void tables_check() {
    for (int k = 0; k < 7; ++k) REQUIRE(Ft8Mode::costas(k) == kCostas[k], "Costas");
    for (int v = 0; v < 8; ++v) REQUIRE(Ft8Mode::gray(v) == kGray[v], "Gray");
    for (int n = 0; n < 21; ++n) REQUIRE(Ft8Mode::costas_sym(n) == (n / 7) * 36 + n % 7 && Ft8Mode::sync_tone(n) == kCostas[n % 7], "sync symbols");
    std::vector<int> seen(79, 0);
    for (int n = 0; n < 21; ++n) seen[(size_t)Ft8Mode::costas_sym(n)] += 1;
    for (int d = 0; d < 58; ++d) seen[(size_t)Ft8Mode::data_sym(d)] += 1;
    for (int s = 0; s < 79; ++s) REQUIRE(seen[(size_t)s] == 1, "symbol %d", s);
  }
  // a planted frame's tone at symbol sym: the Costas tones and random data
  static int plant_tone(int sym) {
    const int k = sym % 36;
    return (k < 7 && sym / 36 * 36 + 6 >= sym) ? kCostas[k] : (int)(rnd01() * 7.99f);
  }
  // step 2 for the frame at t0 of decoder j, P by absolute step
  static void score(const float* P, int nb, long t0, int j, float* want, int* want_hits) {
    float sig = 0.f, tot = 0.f;
    int hits = 0;
    for (int blk = 0; blk < 3; ++blk)
      for (int k = 0; k < 7; ++k) {
        const float* p = P + (size_t)(t0 + 4 * (36 * blk + k)) * nb + j;
        const float e = p[2 * kCostas[k]];
        sig = sig + e;
        float r = p[0];
        r = r + p[2]; r = r + p[4]; r = r + p[6]; r = r + p[8]; r = r + p[10]; r = r + p[12];
        tot = tot + r;
        int hit = 1;
        for (int tone = 0; tone < 8; ++tone) if (tone != kCostas[k] && !(e > p[2 * tone])) hit = 0;
        hits += hit;
      }
    const float den = tot - sig, six = 6.f * sig;
    *want = den > 0.f ? six / den : 0.f;
    *want_hits = hits;
  }
  // An event is a planted frame with all 21 hits, or its image 36 symbols earlier or later, where two of the three Costas
  // arrays meet two of the frame's: 14 hits and what chance adds.
  static void judge(const int plant[4][2], long tc, int j, int hits, long* events, long* images) {
    bool planted = false, image = false;
    for (int k = 0; k < 4; ++k) {
      planted = planted || (tc == plant[k][0] && j == plant[k][1]);
      image = image || ((tc == plant[k][0] - 144 || tc == plant[k][0] + 144) && j == plant[k][1]);
    }
    REQUIRE(planted || image, "an event at (%ld, %d)", tc, j);
    if (image) { REQUIRE(hits >= 14 && hits < 21, "the image at (%ld, %d) has %d hits", tc, j, hits); ++*images; }
    else { REQUIRE(hits == 21, "hits"); ++*events; }
  }
  static void totals(int S, long events, long images) {
    REQUIRE(events == 4 && images >= 4, "S %d: %ld events, %ld images; 4 frames were planted (two of them a symbol and a raster step apart: each decoder sees its own)", S, events, images);
  }
  static float llr(const float* P, int nb, long tc, int j, int i) {
    const int d = i / 3, sym = d < 29 ? 7 + d : 43 + d - 29, mask = 4 >> (i % 3);
    float m1 = -1.f, m0 = -1.f;
    for (int v = 0; v < 8; ++v) {
      const float pv = P[(size_t)(tc + 4 * sym) * nb + j + 2 * kGray[v]];
      if (v & mask) m1 = pv > m1 ? pv : m1; else m0 = pv > m0 ? pv : m0;
    }
    return m1 - m0;
  }
};

// ---- FT4 as the definition writes it -------------------------------------------------------------------------------------
struct Ref4 {
  typedef pysdr_ft4_cfg PublicCfg;
  static constexpr unsigned kSeed = 2025u;
  static constexpr const char* kLower = "ft4";
  static constexpr const char* kMarker = "FT4_PLAN_OK";
  static FtCfg good_cfg() {
    FtCfg c{};
    c.smin = 4.f; c.hmin = 12; c.pmax = 1e18f;
    return c;
  }
  // Uniform random powers hit a sync symbol with chance 1 / 4, twelve of sixteen about once in 30000 scores, and the sync
  // check makes some 25000: it counts the planted frames, so it asks for 14 hits (the peak rule is held against the
  // transcription at every score either way).
  static FtCfg sync_cfg() {
    FtCfg c = good_cfg();
    c.hmin = 14;
    return c;
  }
  static constexpr int kS0 = 48, kS1 = 72, kLag = 408, kEmitLag = 412, kHold = 417, kExtra = 6, kSyms = 103, kSync = 16;
  static constexpr int kNkMax0 = 10922, kNkMax1 = 7281;
  static constexpr long long kRingOfNkMax0 = 10922LL * 461 * 30 * 4;
  static constexpr int kSpcMax = 87382;
  static constexpr long long kRingOfOneRow = 1LL * (417 + 2 * 87382) * 30 * 4;
  static constexpr int kThreads0 = 128, kThreads1 = 192, kItems0 = 120, kItems1 = 168, kLds0 = 2296, kLds1 = 3448, kNb0 = 30, kNb1 = 42;
  static constexpr int kHpadLeast = 71;
  static constexpr long kRingCheckSteps = 500;
  static std::vector<int> bad_S() { return {-48, 0, 1, 12, 24, 47, 49, 64, 71, 73, 96, 144}; }
  static std::vector<int> bad_hmin() { return {-1, 17, 21, 1 << 30}; }
  static std::vector<int> plan_nk() { return {1, 3, 32, 512}; }
  static std::vector<int> plan_max_out() { return {1, 11, 12, 13, 15, 16, 17, 18, 19, 47, 48, 49, 71, 72, 73, 256, 1000}; }
  static std::vector<int> ring_max_out() { return {1, 16, 18, 100, 256, 1000}; }
  static std::vector<int> word_steps() { return {0, 1, 31, 32, 87381, 87382}; }
  static std::vector<int> word_hits() { return {0, 1, 12, 16, 31}; }
  static void steps_check() {
    REQUIRE(ft_steps_done(0, 48) == 0 && ft_steps_done(47, 48) == 0 && ft_steps_done(48, 48) == 1 && ft_steps_done(59, 48) == 1 && ft_steps_done(60, 48) == 2, "steps");
    REQUIRE(ft_steps_done(71, 72) == 0 && ft_steps_done(72, 72) == 1 && ft_steps_done(90, 72) == 2 && ft_steps_done(7000, 48) == 580, "steps");
  }

  static constexpr int kSyncSym[16] = {0, 1, 2, 3, 33, 34, 35, 36, 66, 67, 68, 69, 99, 100, 101, 102};
  static constexpr int kSyncTone[16] = {0, 1, 3, 2, 1, 0, 2, 3, 2, 3, 1, 0, 3, 2, 0, 1};   // A, B, C, D
  static constexpr int kGray4[4] = {0, 1, 3, 2};
  static void tables_check() {
    for (int n = 0; n < 16; ++n)
      REQUIRE(Ft4Mode::costas_sym(n) == kSyncSym[n] && Ft4Mode::costas(n) == kSyncTone[n] && Ft4Mode::sync_tone(n) == kSyncTone[n],
              "sync symbol %d: (%d, %d)", n, Ft4Mode::costas_sym(n), Ft4Mode::costas(n));
    for (int v = 0; v < 4; ++v) REQUIRE(Ft4Mode::gray(v) == kGray4[v], "Gray");
    for (int blk = 0; blk < 4; ++blk) {                                // each array is a permutation of the four tones, and no two agree anywhere
      int seen = 0;
      for (int k = 0; k < 4; ++k) seen |= 1 << Ft4Mode::costas(4 * blk + k);
      REQUIRE(seen == 15, "array %d", blk);
      for (int other = 0; other < blk; ++other)
        for (int k = 0; k < 4; ++k) REQUIRE(Ft4Mode::costas(4 * blk + k) != Ft4Mode::costas(4 * other + k), "arrays %d and %d agree at %d", blk, other, k);
    }
    std::vector<int> seen(103, 0), order;
    for (int n = 0; n < 16; ++n) seen[(size_t)Ft4Mode::costas_sym(n)] += 1;
    for (int d = 0; d < 87; ++d) { seen[(size_t)Ft4Mode::data_sym(d)] += 1; order.push_back(Ft4Mode::data_sym(d)); }
    for (int s = 0; s < 103; ++s) REQUIRE(seen[(size_t)s] == 1, "symbol %d", s);
    for (size_t d = 1; d < order.size(); ++d) REQUIRE(order[d] > order[d - 1], "data symbols ascend");
    REQUIRE(Ft4Mode::data_sym(0) == 4 && Ft4Mode::data_sym(28) == 32 && Ft4Mode::data_sym(29) == 37 && Ft4Mode::data_sym(57) == 65 &&
            Ft4Mode::data_sym(58) == 70 && Ft4Mode::data_sym(86) == 98, "data blocks");
  }
  static int plant_tone(int sym) {
    int tone = (int)(rnd01() * 3.99f);
    for (int n = 0; n < 16; ++n) if (kSyncSym[n] == sym) tone = kSyncTone[n];
    return tone;
  }
  static void score(const float* P, int nb, long t0, int j, float* want, int* want_hits) {
    float sig = 0.f, tot = 0.f;
    int hits = 0;
    for (int n = 0; n < 16; ++n) {
      const float* p = P + (size_t)(t0 + 4 * kSyncSym[n]) * nb + j;
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
    *want = den > 0.f ? three / den : 0.f;
    *want_hits = hits;
  }
  // a planted frame with all 16 hits; the four arrays differ in every place, so a frame has no image 33 symbols away
  static void judge(const int plant[4][2], long tc, int j, int hits, long* events, long*) {
    bool planted = false;
    for (int k = 0; k < 4; ++k) planted = planted || (tc == plant[k][0] && j == plant[k][1]);
    REQUIRE(planted && hits == 16, "an event at (%ld, %d) with %d hits", tc, j, hits);
    ++*events;
  }
  static void totals(int S, long events, long) {
    REQUIRE(events == 4, "S %d: %ld events; 4 frames were planted (two of them a symbol and a raster step apart: each decoder sees its own)", S, events);
  }
  static float llr(const float* P, int nb, long tc, int j, int i) {
    const int d = i / 2, sym = d < 29 ? 4 + d : (d < 58 ? 37 + d - 29 : 70 + d - 58), mask = 2 >> (i % 2);
    float m1 = -1.f, m0 = -1.f;
    for (int v = 0; v < 4; ++v) {
      const float pv = P[(size_t)(tc + 4 * sym) * nb + j + 2 * kGray4[v]];
      if (v & mask) m1 = pv > m1 ? pv : m1; else m0 = pv > m0 ? pv : m0;
    }
    return m1 - m0;
  }
};

// One row group of a stream cut into calls: the walk of ft_spectrum_kernel with real samples.  `stream` holds the row's
// outputs from the stream's start; every step is held against the definition computed from the stream itself.
template <class Mode, int S>
static long walk_stream(int nk, const std::vector<int>& calls, const FtPlan& p, float pmax) {
  using G = FtGeom<Mode, S>;
  constexpr int NT = G::kNt, NB = G::kNb, TH = G::kThreads, QS = G::kQs, HP = Mode::kHpad;
  long total = 0;
  for (int n : calls) total += n;
  std::vector<FtC> tw((size_t)NT);
  for (int t = 0; t < NT; ++t) tw[(size_t)t] = FtC{(float)cos(2 * M_PI * t / NT), (float)-sin(2 * M_PI * t / NT)};
  std::vector<std::vector<FtC>> stream((size_t)nk, std::vector<FtC>((size_t)total));
  std::vector<std::vector<char>> bad((size_t)nk, std::vector<char>((size_t)total, 0));
  for (int r = 0; r < nk; ++r)
    for (long i = 0; i < total; ++i) stream[(size_t)r][(size_t)i] = FtC{rnd(), rnd()};
  auto poke = [&](int r, long i, FtC v, bool blanks) { if (r < nk && i >= 0 && i < total) { stream[(size_t)r][(size_t)i] = v; bad[(size_t)r][(size_t)i] = blanks; } };
  poke(0, 3, FtC{__builtin_nanf(""), 0.25f}, true);
  poke(nk - 1, total / 2, FtC{-0.5f, __builtin_inff()}, true);
  poke(nk / 2, total - 1, FtC{3e19f, 0.f}, true);
  poke(nk - 1, total / 3, FtC{1e6f, 1e6f}, false);                  // large, below pmax: kept
  const long T = (long)ft_steps_done((unsigned long long)total, S);
  std::vector<int> computed((size_t)nk * (size_t)(T > 0 ? T : 1), 0);
  std::vector<FtC> Y((size_t)nk * p.ypitch, FtC{0.f, 0.f});         // as allocated and reset: a.y = Y + the history's room
  long m0 = 0, t_done = 0, blanked = 0, checked = 0;
  for (int n_out : calls) {
    REQUIRE(n_out <= p.ypitch - HP, "a call of %d outputs", n_out);
    for (int r = 0; r < nk; ++r)                                     // the channelizer's pass
      for (int i = 0; i < n_out; ++i) Y.data()[(size_t)r * p.ypitch + HP + i] = stream[(size_t)r][(size_t)(m0 + i)];
    if (n_out == 0) continue;                                        // nothing launched
    const long t1 = (long)ft_steps_done((unsigned long long)(m0 + n_out), S);
    const int ns = (int)(t1 - t_done);
    REQUIRE(ns >= 0 && ns <= ft_steps_per_call(p.ypitch - HP, S), "%d steps in a call of %d", ns, n_out);
    // brute force: the steps whose last output QS t + S - 1 falls into [m0, m0 + n_out)
    int brute = 0;
    for (long t = 0; t < T; ++t) brute += (QS * t + S - 1 >= m0 && QS * t + S - 1 < m0 + n_out) ? 1 : 0;
    REQUIRE(brute == ns, "%d steps end in the call, the plan says %d", brute, ns);
    const int e_first = ns > 0 ? (int)(QS * t_done + S - 1 - m0) : 0;
    REQUIRE(e_first >= 0 && e_first < (t_done ? QS : S), "e_first %d", e_first);
    for (int row = 0; row < nk; ++row) {                             // a workgroup
      std::vector<int> loads((size_t)p.ypitch, 0);
      std::vector<FtC> tile((size_t)G::kYp);
      std::vector<long> from((size_t)G::kYp, -1000000L);             // call-relative output held by every LDS slot
      const size_t yb = (size_t)row * p.ypitch + HP;
      int done_in_call = 0;
      for (int i0 = 0; i0 < n_out; i0 += G::kTile) {
        std::vector<FtC> carry((size_t)G::kCarry);
        std::vector<long> cfrom((size_t)G::kCarry);
        for (int tid = 0; tid < G::kCarry; ++tid) {
          if (i0 > 0) { carry[(size_t)tid] = tile.data()[G::carry_src(tid)]; cfrom[(size_t)tid] = from.data()[G::carry_src(tid)]; }
          else { carry[(size_t)tid] = Y.data()[yb + G::hist_off(tid)]; cfrom[(size_t)tid] = G::hist_off(tid); loads.data()[HP + G::hist_off(tid)] += 1; }
        }
        std::vector<int> written((size_t)G::kYp, 0);
        for (int tid = 0; tid < G::kCarry; ++tid) { tile.data()[G::carry_dst(tid)] = carry[(size_t)tid]; from.data()[G::carry_dst(tid)] = cfrom[(size_t)tid]; written.data()[G::carry_dst(tid)] += 1; }
        for (int tid = 0; tid < TH; ++tid)
          for (int c = tid; c < G::kTile; c += TH) {
            const int i = i0 + c;
            FtC v{0.f, 0.f};
            if (i < n_out) { v = Y.data()[yb + i]; loads.data()[HP + i] += 1; }
            tile.data()[G::stage_dst(c)] = v; from.data()[G::stage_dst(c)] = i; written.data()[G::stage_dst(c)] += 1;
          }
        for (int k = 0; k < G::kYp; ++k) REQUIRE(written[(size_t)k] == 1, "LDS slot %d written %d x", k, written[(size_t)k]);
        for (int tid = 0; tid < TH; ++tid) {
          const bool has = tid < G::kItems;
          const int s = has ? G::item_step(tid) : 0, b = has ? G::item_bin(tid) : 0;
          REQUIRE(s >= 0 && s < kFtStepsPerSym && b >= 0 && b < NB, "item");
          const int u = G::tile_step(i0, e_first, s);
          if (!(has && u >= 0 && u < ns)) continue;
          const long t = t_done + u;
          const int w0 = G::win(e_first, s);
          REQUIRE(w0 >= 0 && w0 + S <= G::kYp, "window at %d", w0);
          for (int i = 0; i < S; ++i)
            REQUIRE(from.data()[w0 + i] == QS * t + i - m0 && QS * t + i - m0 < n_out, "step %ld tap %d holds output %ld", t, i, from.data()[w0 + i]);
          const float pw = ft_bin<S>(tile.data() + w0, tw.data(), ft_qmod<Mode>(b, S), pmax);
          // the definition, from the stream
          const long q = 2 * b - (NB - 1);
          float ar = 0.f, ai = 0.f;
          bool reach = false;
          for (int i = 0; i < S; ++i) {
            const FtC y = stream[(size_t)row][(size_t)(QS * t + i)], w = tw[(size_t)((((q * i) % NT) + NT) % NT)];
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
        const int rel = i - HP;
        REQUIRE(loads[(size_t)i] == ((rel >= -(S - 1) && rel < n_out) ? 1 : 0), "(%d, %d) loaded %d x", row, rel, loads[(size_t)i]);
      }
      std::vector<FtC> keep((size_t)(S - 1));                         // the roll: reads first, then writes
      for (int j = 0; j < S - 1; ++j) {
        const long src = HP + G::roll_src(n_out, j), dst = HP + G::roll_dst(j);
        REQUIRE(src >= 0 && src < p.ypitch && dst >= 0 && dst < HP, "roll");
        keep[(size_t)j] = Y.data()[(size_t)row * p.ypitch + src];
      }
      for (int j = 0; j < S - 1; ++j) Y.data()[(size_t)row * p.ypitch + HP + G::roll_dst(j)] = keep[(size_t)j];
      for (int j = 0; j < S - 1; ++j) {                              // the history is the stream's last S - 1 outputs (zeros before it)
        const long k = m0 + n_out - (S - 1) + j;
        const FtC h = Y[yb + G::hist_off(j)], w = k >= 0 ? stream[(size_t)row][(size_t)k] : FtC{0.f, 0.f};
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

template <class Mode>
static long walk(int S, int nk, const std::vector<int>& calls, const FtPlan& p) {
  return S == Mode::kS0 ? walk_stream<Mode, Mode::kS0>(nk, calls, p, 1e18f) : walk_stream<Mode, Mode::kS1>(nk, calls, p, 1e18f);
}

// ---- steps 2 and 3 and the soft bits beside the mode's transcription, on a ring that wraps ------------------------------
template <class Mode, class Ref>
static long sync_check(int S, int max_out) {
  const int nsub = S / 2, nb = nsub + Ref::kExtra, tr = ft_ring_steps<Mode>(max_out, S);
  const long T = 700;
  std::vector<float> P((size_t)T * nb);                              // by absolute step
  for (auto& v : P) v = rnd01();
  // frames planted at (t0, j): the Costas tones and random data, strong
  const int plant[4][2] = {{3, 0}, {40, nsub - 1}, {200, 15}, {204, 16}};   // no two share a bin
  for (auto& pl : plant)
    for (int sym = 0; sym < Ref::kSyms; ++sym) {
      const int tone = Ref::plant_tone(sym);
      P[(size_t)(pl[0] + 4 * sym) * nb + pl[1] + 2 * tone] += 20.f + rnd01();
    }
  long checked = 0, events = 0, images = 0;
  std::vector<float> sc((size_t)kFtKeep * nsub, 0.f), all((size_t)T * nsub, -1.f);
  std::vector<int32_t> hi((size_t)kFtKeep * nsub, 0), allh((size_t)T * nsub, 0);
  std::vector<float> ring((size_t)tr * nb, 0.f);
  const FtCfg c = Ref::sync_cfg();
  for (long t = 0; t < T; ++t) {
    memcpy(ring.data() + (size_t)(t % tr) * nb, P.data() + (size_t)t * nb, nb * sizeof(float));
    const long t0 = t - Ref::kLag;
    if (t0 < 0) continue;
    for (int j = 0; j < nsub; ++j) {
      const FtScore z = ft_sync<Mode>(ring.data(), tr, nb, (int)(t0 % tr), j);
      float want = 0.f;
      int hits = 0;
      Ref::score(P.data(), nb, t0, j, &want, &hits);
      REQUIRE(memcmp(&want, &z.score, 4) == 0 && hits == z.hits, "t0 %ld decoder %d: score %g hits %d, the transcription's %g %d", t0, j, (double)z.score, z.hits, (double)want, hits);
      sc[(size_t)(t0 % kFtKeep) * nsub + j] = z.score; hi[(size_t)(t0 % kFtKeep) * nsub + j] = z.hits;
      all[(size_t)t0 * nsub + j] = z.score; allh[(size_t)t0 * nsub + j] = z.hits;
      ++checked;
      const long tc = t0 - kFtReach;
      if (tc < 0) continue;
      const bool ev = ft_peak(sc.data() + j, hi.data() + j, nsub, tc, c);
      bool want_ev = all[(size_t)tc * nsub + j] >= c.smin && allh[(size_t)tc * nsub + j] >= c.hmin;
      for (int d = 1; d <= 4 && want_ev; ++d) {
        if (tc - d >= 0 && !(all[(size_t)tc * nsub + j] > all[(size_t)(tc - d) * nsub + j])) want_ev = false;
        if (!(all[(size_t)tc * nsub + j] >= all[(size_t)(tc + d) * nsub + j])) want_ev = false;
      }
      REQUIRE(ev == want_ev, "t0 %ld decoder %d: event %d, the transcription's %d", tc, j, (int)ev, (int)want_ev);
      if (ev) {
        Ref::judge(plant, tc, j, allh[(size_t)tc * nsub + j], &events, &images);
        // its soft bits, while the frame is in the ring
        REQUIRE(ft_llr_ok<Mode>(j, tc, t + 1, nsub, tr), "valid at its emission");
        for (int i = 0; i < 174; ++i) {
          const float want_l = Ref::llr(P.data(), nb, tc, j, i), got = ft_llr_bit<Mode>(ring.data(), tr, nb, (int)(tc % tr), j, i);
          REQUIRE(memcmp(&want_l, &got, 4) == 0, "soft bit %d of (%ld, %d)", i, tc, j);
        }
      }
    }
  }
  Ref::totals(S, events, images);
  return checked;
}

// ---- the cap: events of one decoder over score sequences, stored call by call as the kernel stores them ------------------
template <class Mode, class Ref>
static long cap_check(int S) {
  const FtCfg c = Ref::good_cfg();
  long seqs = 0, fill = 0;
  int gap = 1 << 30;
  for (int kind = 0; kind < 40; ++kind) {
    const int T = 400;
    std::vector<float> score((size_t)T);
    for (int t = 0; t < T; ++t) {
      switch (kind % 5) {
        case 0: score[(size_t)t] = c.smin + 10.f * rnd01(); break;                               // noise above smin
        case 1: score[(size_t)t] = 5.f; break;                                                   // a plateau: ties
        case 2: score[(size_t)t] = (t % 5 == kind % 5) ? 9.f : 4.f; break;                       // a peak every 5 steps: the closest the rule allows
        case 3: score[(size_t)t] = (t % 4 == 0) ? 9.f : 4.f; break;                              // every 4: equal peaks inside each other's reach
        default: score[(size_t)t] = 4.f + (float)(t % 7) + (float)((t * 37) % 11); break;
      }
    }
    std::vector<int> at;
    float sc[kFtKeep] = {0};
    int32_t hi[kFtKeep] = {0};
    for (int t0 = 0; t0 < T; ++t0) {
      sc[t0 % kFtKeep] = score[(size_t)t0]; hi[t0 % kFtKeep] = Ref::kSync;
      const long tc = t0 - kFtReach;
      if (tc >= 0 && ft_peak(sc, hi, 1, tc, c)) at.push_back(t0);    // the step index (shifted by a constant) at which it is emitted
    }
    for (size_t a = 1; a < at.size(); ++a) if (at[a] - at[a - 1] < gap) gap = at[a] - at[a - 1];
    // every call of ns steps beginning at every step: the events in it fit the cap of the smallest max_out that gives ns
    for (int max_out : {1, S / 4 - 1, S / 4, 4 * (S / 4), 5 * (S / 4) - 1, 9 * (S / 4), 16, 256, 1000}) {
      const int spc = ft_steps_per_call(max_out, S), cap = ft_event_cap(max_out, S);
      for (int first = 0; first + spc <= T; ++first) {
        std::vector<int32_t> slots((size_t)cap * kFtEventWords);
        int cnt = 0;
        for (int v : at)
          if (v >= first && v < first + spc) {
            REQUIRE(cnt < cap, "event %d of a call of %d steps does not fit %d slots", cnt + 1, spc, cap);
            slots.data()[kFtEventWords * cnt] = ft_pack(v - first, Ref::kSync); slots.data()[kFtEventWords * cnt + 1] = 0; ++cnt;
          }
        if (cnt * 1000L / cap > fill) fill = cnt * 1000L / cap;
      }
    }
    ++seqs;
  }
  REQUIRE(gap == 5 && kFtMinGap == 5, "S %d: two events %d steps apart, the bound is %d", S, gap, kFtMinGap);
  REQUIRE(fill == 1000, "S %d: no call fills its slots (%ld / 1000)", S, fill);
  return seqs;
}

// ---- the ring depth: every cut of a stream into calls --------------------------------------------------------------------
template <class Mode, class Ref>
static long ring_check(int S, int max_out) {
  const int QS = S / 4, tr = ft_ring_steps<Mode>(max_out, S), spc = ft_steps_per_call(max_out, S);
  long cases = 0;
  for (int trial = 0; trial < 100; ++trial) {
    long m = 0;
    std::vector<long> ends;                                          // steps done at the end of every call
    const long total = Ref::kRingCheckSteps * QS + S + (long)(rnd01() * 300 * QS);
    while (m < total) {
      int n = trial % 4 == 0 ? max_out : (trial % 4 == 1 ? 1 + (int)(rnd01() * (max_out - 0.01f)) : (rnd01() < 0.5f ? max_out : (int)(rnd01() * 3)));
      if (n > max_out) n = max_out;
      m += n;
      ends.push_back((long)ft_steps_done((unsigned long long)m, S));
    }
    for (size_t k = 1; k < ends.size(); ++k) REQUIRE(ends[k] - ends[k - 1] <= spc, "%ld steps in a call, at most %d", ends[k] - ends[k - 1], spc);
    size_t a = 0;
    for (long t0 = 0; t0 + Ref::kHold < ends.back(); t0 += 1 + trial % 3) {
      while (ends[a] <= t0 + Ref::kEmitLag) ++a;                     // the call that emits t0
      REQUIRE(ft_llr_ok<Mode>(0, t0, ends[a], 1, tr), "t0 %ld invalid at the end of its own call", t0);
      if (a + 1 < ends.size()) REQUIRE(ft_llr_ok<Mode>(0, t0, ends[a + 1], 1, tr), "t0 %ld gone a call later (%ld done, ring %d)", t0, ends[a + 1], tr);
      size_t b = a;
      while (ends[b] < t0 + Ref::kHold) ++b;                         // the call at whose end the host releases it
      REQUIRE(ft_llr_ok<Mode>(0, t0, ends[b], 1, tr), "t0 %ld gone at its release (%ld done, ring %d)", t0, ends[b], tr);
      ++cases;
    }
  }
  // the window itself
  const long first_whole = Ref::kLag + 1;
  for (long done : {first_whole, Ref::kRingCheckSteps, (long)tr, (long)tr + 1, 100000L}) {
    for (long t0 = -2; t0 <= done; ++t0) {
      const bool want = t0 >= 0 && t0 <= done - first_whole && t0 >= done - tr;
      REQUIRE(ft_llr_ok<Mode>(0, t0, done, 1, tr) == want, "done %ld t0 %ld", done, t0);
    }
    REQUIRE(!ft_llr_ok<Mode>(-1, done - first_whole, done, 1, tr) && !ft_llr_ok<Mode>(1, done - first_whole, done, 1, tr) &&
            ft_llr_ok<Mode>(6, done - first_whole, done, 7, tr), "F");
  }
  return cases;
}

template <class Mode, class Ref>
static void run_mode() {
  g_rng = Ref::kSeed;
  constexpr int S0 = Ref::kS0, S1 = Ref::kS1;
  const FtCfg cfg = Ref::good_cfg();
  FtPlan p;
  // ---- the traits against the numbers written out
  REQUIRE(Mode::kS0 == S0 && Mode::kS1 == S1 && Mode::kSyms == Ref::kSyms && Mode::kSync == Ref::kSync && strcmp(Mode::kName, Ref::kLower) == 0, "traits");
  REQUIRE(kFtLag<Mode> == Ref::kLag && kFtEmitLag<Mode> == Ref::kEmitLag && kFtHold<Mode> == Ref::kHold && kFtExtra<Mode> == Ref::kExtra &&
          Mode::kBitsPerSym * Mode::kData == 174 && kFtBits == 174 && kFtKeep == 9 && kFtMinGap == 5, "constants");
  // ---- refusals
  REQUIRE(!ft_plan<Mode>(0, S0, 16, &cfg, &p) && !ft_plan<Mode>(-1, S0, 16, &cfg, &p) && ft_plan<Mode>(1, S0, 16, &cfg, &p), "nk");
  REQUIRE(ft_plan<Mode>(Ref::kNkMax0, S0, 16, &cfg, &p) && !ft_plan<Mode>(Ref::kNkMax0 + 1, S0, 16, &cfg, &p) &&
          ft_plan<Mode>(Ref::kNkMax1, S1, 16, &cfg, &p) && !ft_plan<Mode>(Ref::kNkMax1 + 1, S1, 16, &cfg, &p), "nk S / 2 <= 2^18");
  for (int S : Ref::bad_S()) REQUIRE(!ft_plan<Mode>(4, S, 16, &cfg, &p), "S %d accepted", S);
  REQUIRE(!ft_plan<Mode>(4, S0, 0, &cfg, &p) && !ft_plan<Mode>(4, S0, -5, &cfg, &p) && !ft_plan<Mode>(4, S0, kFtMaxOutMax + 1, &cfg, &p) &&
          ft_plan<Mode>(4, S0, kFtMaxOutMax, &cfg, &p), "max_out");
  REQUIRE(!ft_plan<Mode>(4, S0, 16, nullptr, &p), "NULL cfg");
  {
    const float nan = __builtin_nanf(""), inf = __builtin_inff();
    for (float v : {-1.f, -1e-30f, nan, inf, -inf}) { FtCfg b = cfg; b.smin = v; REQUIRE(!ft_plan<Mode>(4, S0, 16, &b, &p), "smin %g accepted", (double)v); }
    for (float v : {0.f, -1.f, nan, inf, -inf, 1.1e18f}) { FtCfg b = cfg; b.pmax = v; REQUIRE(!ft_plan<Mode>(4, S0, 16, &b, &p), "pmax %g accepted", (double)v); }
    for (int v : Ref::bad_hmin()) { FtCfg b = cfg; b.hmin = v; REQUIRE(!ft_plan<Mode>(4, S0, 16, &b, &p), "hmin %d accepted", v); }
    FtCfg b = cfg; b.smin = 0.f; b.hmin = 0; b.pmax = 1e18f; REQUIRE(ft_plan<Mode>(4, S0, 16, &b, &p), "the rules' edges");
    b.hmin = Ref::kSync; b.smin = 1e30f; b.pmax = 1e-30f; REQUIRE(ft_plan<Mode>(4, S0, 16, &b, &p), "the rules' edges");
  }
  // the ring's byte limit: nk TR NB 4 <= 2^30
  REQUIRE(ft_plan<Mode>(Ref::kNkMax0, S0, 256, &cfg, &p) && p.ring_bytes == Ref::kRingOfNkMax0 && p.ring_bytes <= kFtRingBytesMax, "ring of %d rows", Ref::kNkMax0);
  REQUIRE(!ft_plan<Mode>(Ref::kNkMax0, S0, 4096, &cfg, &p) && ft_plan<Mode>(512, S0, 4096, &cfg, &p), "a ring above the limit");
  REQUIRE(ft_plan<Mode>(1, S0, kFtMaxOutMax, &cfg, &p) && p.ring_bytes == Ref::kRingOfOneRow, "one row at the largest max_out");
  // ---- plans
  long plans = 0;
  for (int S : {S0, S1})
    for (int nk : Ref::plan_nk())
      for (int mo : Ref::plan_max_out()) {
        REQUIRE(ft_plan<Mode>(nk, S, mo, &cfg, &p), "nk %d S %d max_out %d refused", nk, S, mo);
        const int spc = mo / (S / 4) + 1;
        REQUIRE(p.cap == spc / 5 + 1 && p.nsub == S / 2 && p.nb == S / 2 + Ref::kExtra && p.nfine == nk * (S / 2) && p.groups == nk, "plan");
        REQUIRE(p.tr == Ref::kHold + 2 * spc && p.tr > Ref::kLag + 1 && p.ring_bytes == (long long)nk * p.tr * p.nb * 4, "ring");
        REQUIRE(p.ypitch >= Mode::kHpad + mo && p.ypitch % 16 == 0 && p.ypitch < Mode::kHpad + mo + 16 && Mode::kHpad >= S - 1, "pitch %d", p.ypitch);
        ++plans;
      }
  using G0 = FtGeom<Mode, S0>;
  using G1 = FtGeom<Mode, S1>;
  REQUIRE(G0::kThreads == Ref::kThreads0 && G1::kThreads == Ref::kThreads1 && G0::kItems == Ref::kItems0 && G1::kItems == Ref::kItems1, "geometry");
  REQUIRE(G0::kLdsBytes == Ref::kLds0 && G1::kLdsBytes == Ref::kLds1 && G0::kNb == Ref::kNb0 && G1::kNb == Ref::kNb1, "geometry");
  REQUIRE(ft_threads<Mode>(S0) == Ref::kThreads0 && ft_threads<Mode>(S1) == Ref::kThreads1 && ft_lds_bytes<Mode>(S0) == Ref::kLds0 && ft_lds_bytes<Mode>(S1) == Ref::kLds1, "geometry");
  REQUIRE(Mode::kHpad % 16 == 0 && Mode::kHpad >= Ref::kHpadLeast && Mode::kHpad < Ref::kHpadLeast + 16, "the history's room");
  for (int S : {S0, S1})
    for (int b = 0; b < S / 2 + Ref::kExtra; ++b) {
      const int q = 2 * b - (S / 2 + Ref::kExtra - 1), NT = 4 * S;
      REQUIRE(ft_qmod<Mode>(b, S) == ((q % NT) + NT) % NT, "qmod");
    }
  Ref::tables_check();
  Ref::steps_check();
  // ---- the tile walk and the spectrum, over streams cut into calls
  long bins = 0;
  for (int S : {S0, S1})
    for (int nk : {1, 3}) {
      REQUIRE(ft_plan<Mode>(nk, S, 256, &cfg, &p), "plan");
      const int QS = S / 4;
      const std::vector<std::vector<int>> cuts = {
          {256, 256, 256}, {1, 0, 2, QS - 1, 1, QS, QS + 1, S - 1, S, S + 1, 0, 2 * S + 5, 256, 7, 255},
          {S - 1, 1, 1, QS - 1, 1}, {S, QS, QS, 2 * S, 2 * S + 1, 2 * S - 1}, {3, 200, 1, 1, 1, 130, 64}};
      for (auto& c : cuts) bins += walk<Mode>(S, nk, c, p);
      // every call position: a call of every length from 0 to 2 S + 1 behind every residue of the stream's length mod S
      for (int lead = 0; lead <= S; lead += 5)
        for (int len : {1, QS - 1, QS, S - 1, S, S + 1, 2 * S + 1}) bins += walk<Mode>(S, nk, {S + lead, len, len, 3}, p);
    }
  REQUIRE(ft_plan<Mode>(2, S0, 16, &cfg, &p), "plan");
  bins += walk<Mode>(S0, 2, std::vector<int>(40, 16), p) + walk<Mode>(S0, 2, {5, 11, 16, 0, 16, 1, 15, 16, 16, 16, 9}, p);
  REQUIRE(ft_plan<Mode>(2, S1, 16, &cfg, &p), "plan");
  bins += walk<Mode>(S1, 2, std::vector<int>(40, 16), p);
  // ---- sync, peak and soft bits against the transcription; the cap; the ring
  const long scored = sync_check<Mode, Ref>(S0, 256) + sync_check<Mode, Ref>(S1, 256) + sync_check<Mode, Ref>(S0, 16);
  const long seqs = cap_check<Mode, Ref>(S0) + cap_check<Mode, Ref>(S1);
  long rings = 0;
  for (int S : {S0, S1})
    for (int mo : Ref::ring_max_out()) rings += ring_check<Mode, Ref>(S, mo);
  // ---- the event words
  for (int u : Ref::word_steps())
    for (int h : Ref::word_hits()) {
      const int32_t w = ft_pack(u, h);
      REQUIRE(w >= 0 && ft_event_step(w) == u && ft_event_hits(w) == h, "word (%d, %d)", u, h);
    }
  REQUIRE(ft_steps_per_call(kFtMaxOutMax, S0) == Ref::kSpcMax, "the largest step index");
  REQUIRE(sizeof(typename Ref::PublicCfg) == 12 && sizeof(FtCfg) == 12 && sizeof(FtC) == 8, "layouts %zu %zu", sizeof(typename Ref::PublicCfg), sizeof(FtC));
  printf("%s plan: %ld plans, %ld bins walked and held against the definition, %ld scores beside the transcription, %ld score sequences "
         "with events 5 steps apart at the closest, %ld frames followed through cut streams\n%s\n", Ref::kLower, plans, bins, scored, seqs, rings,
         Ref::kMarker);
}

int main(int argc, char** argv) {
  const bool all = argc < 2;
  if (!all && strcmp(argv[1], "ft8") != 0 && strcmp(argv[1], "ft4") != 0) { fprintf(stderr, "usage: %s [ft8 | ft4]\n", argv[0]); return 2; }
  if (all || strcmp(argv[1], "ft8") == 0) run_mode<Ft8Mode, Ref8>();
  if (all || strcmp(argv[1], "ft4") == 0) run_mode<Ft4Mode, Ref4>();
  return 0;
}
