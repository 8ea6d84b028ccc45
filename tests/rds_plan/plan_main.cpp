// The RDS skimmer's plan, tile geometry, steps and event slots (pysdr_amd/csrc/rds_plan.h, the very code rds.hip steps with)
// on the CPU under AddressSanitizer + UBSan.
//   * the rules: L odd in [385, 863] and the one that belongs to w19, nk >= 1, 16 nk <= 2^18, max_out in [1, 2^20]; the
//     groups tile [0, nk), the row pitch holds the history's room and max_out.
//   * the chip grid: the closed form rds_chips_upto counts exactly the outputs that rds_tick marks, for every rate edge and
//     where the absolute index wraps; no call holds more chips than rds_max_chips, no phase more bits than rds_max_bits.
//   * the tile walk of the kernel, through the index functions of RdsGeom that rds.hip itself uses: every product of every
//     row is made once, from samples inside the row's memory; the carried products are the previous tile's last L; every
//     (row, chip, segment) is filtered once over the products m_c - i at tap i; every (row, chip) is decided once, in order,
//     by its phase's thread; the history roll stays in the row.
//   * every step with real samples -- RDS groups on FM carriers with a pilot, noise, a NaN, an infinite and a zero
//     sample -- as the kernel runs them, call after call (1 output, tile - 1, tile, tile + 1, max_out), against a plain
//     transcription of DESIGN.md 3 item 31 over the rows' memory: z bit for bit, counts, event words and every state field
//     after every call; the groups sent are the groups read.
//   * the cap: the densest stream there is -- a register that completes a group at every bit -- fills exactly the slots.
//   * the constants: x has order 341 modulo g, and (o x^325) mod g are the standard's syndromes of the five offset words.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rds_plan.h"

using namespace pysdr;

#define REQUIRE(c, ...) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static uint32_t word_of(double f, double fs) { return (uint32_t)llround(f / fs * 4294967296.0); }
static int length_of(double fs) { return 2 * (int)floor(fs / 1187.5) + 1; }
static uint32_t rng_state = 2024u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float rndf() { return (float)((int)(rnd() & 0xFFFF) - 32768) / 32768.f; }
static uint32_t fbits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }

// ---- the rules --------------------------------------------------------------------------------------------------------
static void rules() {
  RdsPlan p;
  for (double fs : {228000.0, 250000.0, 400000.0, 456000.0, 512000.0}) {
    const pysdr_rds_cfg c{word_of(19000, fs)};
    const int L0 = length_of(fs);
    for (int L = 300; L < 900; ++L) REQUIRE(rds_plan(4, L, 64, &c, &p) == (L == L0), "fs %g L %d (its own %d)", fs, L, L0);
  }
  const pysdr_rds_cfg c{word_of(19000, 400000.0)};
  REQUIRE(length_of(228000.0) == 385 && length_of(400000.0) == 673 && length_of(512000.0) == 863, "L at the edges");
  REQUIRE(word_of(19000, 512000.0) == kRdsW19Min && word_of(19000, 228000.0) <= kRdsW19Max && word_of(19000, 228000.0) + 1 >= kRdsW19Max, "w19 at the edges");
  REQUIRE(!rds_plan(0, 673, 64, &c, &p) && !rds_plan(-1, 673, 64, &c, &p) && !rds_plan((1 << 14) + 1, 673, 64, &c, &p) && rds_plan(1 << 14, 673, 64, &c, &p), "nk");
  REQUIRE(!rds_plan(4, 673, 0, &c, &p) && !rds_plan(4, 673, (1 << 20) + 1, &c, &p) && rds_plan(4, 673, 1 << 20, &c, &p) && !rds_plan(4, 673, 64, nullptr, &p), "max_out, cfg");
  { pysdr_rds_cfg b{kRdsW19Min - 1}; REQUIRE(!rds_plan(4, 863, 64, &b, &p), "w19 below"); b.w19 = kRdsW19Max + 1; REQUIRE(!rds_plan(4, 385, 64, &b, &p), "w19 above");
    b.w19 = 0; REQUIRE(!rds_plan(4, 673, 64, &b, &p), "w19 0"); }
  for (int nk : {1, 2, 3, 16, 17, 100})
    for (int mo : {1, 16, 1023, 1024, 1025, 4096, 65536, 1 << 20}) {
      REQUIRE(rds_plan(nk, 673, mo, &c, &p), "good");
      REQUIRE(p.ndec == 16 * nk && p.groups * RdsGeom::kRows >= nk && (p.groups - 1) * RdsGeom::kRows < nk && p.nseg == 11, "groups");
      REQUIRE(p.ypitch >= kRdsHpad + mo && p.ypitch % 16 == 0 && p.cap == rds_event_cap(mo, c.w19) && p.cap >= 3 && p.cap % 3 == 0, "pitch, cap");
    }
  REQUIRE(sizeof(pysdr_rds_cfg) == 4 && sizeof(RdsC) == 8, "sizes");
}

// ---- the chip grid ------------------------------------------------------------------------------------------------------
static long grid() {
  long chips = 0;
  for (double fs : {228000.0, 250000.0, 400000.0, 512000.0})
    for (uint32_t m0 : {0u, 1u, 12u, 777777u, 0xFFFFF000u, 0xFFFFFFFFu}) {
      const uint32_t w = word_of(19000, fs), A = rds_acc_before(m0, w);
      int count = 0;
      int per_phase[16] = {0};
      REQUIRE(rds_chips_upto(A, -1, w) == 0, "no chip in front of the call");
      for (int j = 0; j < 6000; ++j) {
        if (rds_tick(m0 + (uint32_t)j, w)) { per_phase[count & 15] += 1; ++count; }
        REQUIRE(rds_chips_upto(A, j, w) == count, "fs %g m0 %u output %d: %d chips, counted %d", fs, m0, j, rds_chips_upto(A, j, w), count);
        REQUIRE(count <= rds_max_chips(j + 1, w), "more chips than the bound");
        for (int ph = 0; ph < 16; ++ph) REQUIRE(per_phase[ph] <= rds_max_bits(j + 1, w), "more bits than the bound");
      }
      chips += count;
    }
  REQUIRE(rds_tick(0u, word_of(19000, 400000.0)), "output 0 opens a chip");
  for (int i0 = 0; i0 < 5000; i0 += 7) {                                 // a tile never holds more than kRdsChipsMax
    const uint32_t A = rds_acc_before((uint32_t)i0 * 2654435761u, kRdsW19Max);
    REQUIRE(rds_chips_upto(A, i0 + kRdsTile - 1, kRdsW19Max) - rds_chips_upto(A, i0 - 1, kRdsW19Max) <= kRdsChipsMax, "chips of a tile");
  }
  return chips;
}

// ---- the tile walk ------------------------------------------------------------------------------------------------------
static long walk(int nk, int n_out, int L, uint32_t w19, uint32_t m0, uint32_t chips0) {
  using G = RdsGeom;
  constexpr int ROWS = G::kRows;
  RdsPlan p;
  const pysdr_rds_cfg c{w19};
  REQUIRE(rds_plan(nk, L, n_out, &c, &p), "plan");
  const uint32_t A0 = rds_acc_before(m0, w19);
  std::vector<int> made((size_t)nk * (size_t)(L + n_out), 0);          // product (row, i), i from -L
  long steps = 0;
  for (int g = 0; g < p.groups; ++g) {
    const int row0 = g * ROWS;
    std::vector<long> tv((size_t)ROWS * G::kVp, -1000000L);             // the call index i whose product a slot holds
    std::vector<int> next_chip((size_t)G::kDecoders, -1);
    int done_chips = 0;
    for (int i0 = 0; i0 < n_out; i0 += kRdsTile) {
      const int nj = n_out - i0 < kRdsTile ? n_out - i0 : kRdsTile;
      const int kbase = rds_chips_upto(A0, i0 - 1, w19), nct = rds_chips_upto(A0, i0 + nj - 1, w19) - kbase;
      REQUIRE(kbase == done_chips && nct >= 0 && nct <= kRdsChipsMax, "chips of the tile");
      if (i0 > 0)
        for (int k = 0; k < G::carry_n(L); ++k) {
          const int hr = G::carry_row(k, L), hc = G::carry_col(k, L);
          REQUIRE(hr < ROWS && hc < L && G::carry_src(hr, hc) != G::carry_dst(hr, hc), "carry index");
          REQUIRE(tv.at((size_t)G::carry_src(hr, hc)) == (long)i0 - L + hc, "the carried product is the previous tile's");
          tv.at((size_t)G::carry_dst(hr, hc)) = tv.at((size_t)G::carry_src(hr, hc));
        }
      for (int k = 0; k < G::mix_n(i0, nj, L); ++k) {                   // phase A1
        const int rr = G::mix_row(k, i0, nj, L), cc = G::mix_col(k, i0, nj, L);
        REQUIRE(rr < ROWS && cc >= G::mix_lo(i0, L) && cc < L + nj, "mixer index");
        const int i = i0 + G::mix_rel(cc, L);
        if (row0 + rr < nk) {
          REQUIRE(i - 1 >= -kRdsHpad && i < n_out && i >= -L, "the mixer reads inside the row");
          made.at((size_t)(row0 + rr) * (size_t)(L + n_out) + (size_t)(i + L)) += 1;
        }
        tv.at((size_t)G::at(rr, cc)) = i;
      }
      std::vector<int> s_chip((size_t)G::kCp, -1);
      for (int jj = 0; jj < nj; ++jj)
        if (rds_tick(m0 + (uint32_t)(i0 + jj), w19)) {
          int& slot = s_chip.at((size_t)(rds_chips_upto(A0, i0 + jj, w19) - kbase - 1));
          REQUIRE(slot == -1, "chip slot written twice");
          slot = jj;
        }
      for (int ci = 0; ci < nct; ++ci) REQUIRE(s_chip[(size_t)ci] >= 0 && (ci == 0 || s_chip[(size_t)ci] > s_chip[(size_t)ci - 1]), "the chips in order");
      std::vector<int> parts((size_t)kRdsSegMax * ROWS * G::kCp, 0);
      for (int k = 0; k < G::fir_n(p.nseg, nct); ++k) {                 // phase A2
        const int ci = G::fir_chip(k, nct), rr = G::fir_row(k, nct), seg = G::fir_seg(k, nct);
        REQUIRE(ci < nct && rr < ROWS && seg < p.nseg, "filter index");
        const int jj = s_chip[(size_t)ci];
        for (int i = seg * kRdsSeg; i < L && i < (seg + 1) * kRdsSeg; ++i)
          REQUIRE(tv.at((size_t)G::newest(rr, jj, L) - (size_t)i) == (long)i0 + jj - i, "tap %d of the chip at %d", i, i0 + jj);
        parts.at((size_t)G::part_at(seg, rr, ci)) += 1;
      }
      for (int tid = 0; tid < G::kDecoders; ++tid) {                    // phase B
        const int r = tid / kRdsPhases, ph = tid % kRdsPhases;
        if (row0 + r >= nk) continue;
        for (int ci = (int)(((uint32_t)ph - (chips0 + (uint32_t)kbase)) & 15u); ci < nct; ci += kRdsPhases) {
          for (int s = 0; s < p.nseg; ++s) REQUIRE(parts.at((size_t)G::part_at(0, r, ci) + (size_t)s * ROWS * G::kCp) == 1, "segment sum missing");
          const int n = kbase + ci;                                     // the chip's number within the call
          REQUIRE(((chips0 + (uint32_t)n) & 15u) == (uint32_t)ph, "the chip's phase");
          REQUIRE(next_chip[(size_t)tid] < 0 ? n < 16 : n == next_chip[(size_t)tid] + 16, "every sixteenth chip, in order");
          next_chip[(size_t)tid] = n;
          ++steps;
        }
      }
      done_chips += nct;
    }
    for (int k = 0; k < G::roll_n(L); ++k) {
      const int row = row0 + G::roll_row(k, L), j = G::roll_col(k, L);
      if (row >= nk) continue;
      const long src = G::roll_src(n_out, j, L), dst = G::roll_dst(j, L);
      REQUIRE(j <= L && src >= -kRdsHpad && src < n_out && dst >= -kRdsHpad && dst < 0 && src - dst == n_out, "roll");
    }
    REQUIRE(G::roll_n(L) <= G::kRollPer * G::kThreads, "the roll fits the threads' registers");
  }
  for (int v : made) REQUIRE(v == 1, "a product made %d times", v);
  REQUIRE(steps == (long)nk * rds_chips_upto(A0, n_out - 1, w19), "every chip of every row decided once");
  return steps;
}

// ---- the plain transcription of DESIGN.md 3 item 31 -------------------------------------------------------------------------
static uint32_t plain_mod(uint64_t b, int bits) {                       // long division, a bit at a time, from the top
  for (int k = bits - 1; k >= 10; --k)
    if (b >> k & 1) b ^= (uint64_t)0x5B9 << (k - 10);
  return (uint32_t)b;
}

struct Plain {
  int L; uint32_t w19; std::vector<RdsC> tw; std::vector<float> g;
  struct Row { uint32_t chips = 0; RdsC ring[16] = {}; std::vector<int> bits[16]; };
  std::vector<Row> rows;
  static RdsC sample(const std::vector<RdsC>& y, long n) { return n < 0 ? RdsC{0.f, 0.f} : y[(size_t)n]; }
  static float arg(RdsC a, RdsC b) {
    const float re = a.x * b.x + a.y * b.y, im = a.y * b.x - a.x * b.y;
    const float ar = fabsf(re), ai = fabsf(im);
    if (std::isnan(ar) || std::isnan(ai) || std::isinf(ar) || std::isinf(ai) || (ar == 0.f && ai == 0.f)) return 0.f;
    const bool steep = ai > ar;
    const float t = steep ? ar / ai : ai / ar, t2 = t * t;
    float s = t2 * kRdsA4;
    s = kRdsA3 + s; s = t2 * s; s = kRdsA2 + s; s = t2 * s; s = kRdsA1 + s; s = t2 * s; s = kRdsA0 + s;
    float phi = t * s;
    if (steep) phi = kRdsHalfPi - phi;
    if (re < 0.f) phi = kRdsPi - phi;
    return im < 0.f ? -phi : phi;
  }
  RdsC v(const std::vector<RdsC>& y, long n, uint32_t m_base) const {
    const float d = arg(sample(y, n), sample(y, n - 1));
    const uint32_t m = m_base + (uint32_t)n;
    const RdsC t = tw[(uint32_t)(m * 3u * w19) >> 22];
    return RdsC{d * t.x, d * t.y};
  }
  RdsC z(const std::vector<RdsC>& y, long m, uint32_t m_base) const {
    RdsC total{0.f, 0.f};
    for (int lo = 0; lo < L; lo += 64) {
      RdsC u{0.f, 0.f};
      for (int i = lo; i < L && i < lo + 64; ++i) {
        const RdsC p = v(y, m - i, m_base);
        if (i == lo) u = RdsC{g[(size_t)i] * p.x, g[(size_t)i] * p.y};
        else u = RdsC{u.x + g[(size_t)i] * p.x, u.y + g[(size_t)i] * p.y};
      }
      total = lo == 0 ? u : RdsC{total.x + u.x, total.y + u.y};
    }
    return total;
  }
  // steps 4 to 6 for a chip of row a; words: the events of the phase's decoder in this call
  void chip(int a, RdsC zc, int i, std::vector<int32_t>* words) {
    Row& r = rows[(size_t)a];
    const int ph = (int)(r.chips & 15u);
    r.chips += 1;
    const float q = zc.x * r.ring[ph].x + zc.y * r.ring[ph].y;
    r.ring[ph] = zc;
    std::vector<int>& b = r.bits[ph];
    b.push_back(q < 0.f ? 1 : 0);
    if (b.size() > 104) b.erase(b.begin());
    if (b.size() < 104) return;
    uint64_t blk[4] = {0, 0, 0, 0};
    for (int k = 0; k < 104; ++k) blk[k / 26] = blk[k / 26] << 1 | (uint64_t)b[(size_t)k];
    const uint32_t sc = plain_mod(blk[2], 26);
    if (plain_mod(blk[0], 26) != 0x0FC || plain_mod(blk[1], 26) != 0x198 || (sc != 0x168 && sc != 0x350) || plain_mod(blk[3], 26) != 0x1B4) return;
    words[ph].push_back((int32_t)((uint32_t)i << 5 | (uint32_t)ph << 1 | (sc == 0x350 ? 1u : 0u)));
    words[ph].push_back((int32_t)((uint32_t)(blk[0] >> 10) << 16 | (uint32_t)(blk[1] >> 10)));
    words[ph].push_back((int32_t)((uint32_t)(blk[2] >> 10) << 16 | (uint32_t)(blk[3] >> 10)));
  }
};

// ---- the kernel's phases, as rds.hip runs them, on heap arrays of exactly their size ---------------------------------------------
struct Device {
  int nk, L; RdsPlan p; uint32_t w19;
  std::vector<RdsC> Y, tw, ring; std::vector<float> g; std::vector<uint32_t> regs, chips; std::vector<int32_t> events, counts;
  std::vector<RdsC> last_z;                                            // [nk][chips of the last call]
  void init() {
    Y.assign((size_t)nk * p.ypitch, RdsC{0.f, 0.f});
    regs.assign((size_t)4 * p.ndec, 0u); chips.assign((size_t)nk, 0u); ring.assign((size_t)p.ndec, RdsC{0.f, 0.f});
    events.assign((size_t)p.ndec * p.cap, 0); counts.assign((size_t)p.ndec, 0);
  }
  int call(int n_out, uint32_t m0) {
    using G = RdsGeom;
    constexpr int ROWS = G::kRows;
    RdsC* y = Y.data() + kRdsHpad;
    const size_t nd = (size_t)p.ndec;
    const uint32_t A0 = rds_acc_before(m0, w19);
    const int total = rds_chips_upto(A0, n_out - 1, w19);
    last_z.assign((size_t)nk * (size_t)total, RdsC{0.f, 0.f});
    for (int grp = 0; grp < p.groups; ++grp) {
      const int row0 = grp * ROWS;
      std::vector<RdsC> s_v((size_t)ROWS * G::kVp), s_part((size_t)kRdsSegMax * ROWS * G::kCp);
      std::vector<float> s_g(g);
      std::vector<int> s_chip((size_t)G::kCp);
      std::vector<RdsDec> z((size_t)G::kDecoders);
      std::vector<int> cnt((size_t)G::kDecoders, 0);
      std::vector<uint32_t> chips0((size_t)G::kDecoders, 0u);
      auto mine = [&](int tid) { return row0 + tid / kRdsPhases < nk; };
      auto dec_of = [&](int tid) { return (row0 + tid / kRdsPhases) * kRdsPhases + tid % kRdsPhases; };
      for (int tid = 0; tid < G::kDecoders; ++tid) {
        if (!mine(tid)) continue;
        const size_t dec = (size_t)dec_of(tid);
        for (int b = 0; b < 4; ++b) z[(size_t)tid].w[b] = regs[(size_t)b * nd + dec];
        z[(size_t)tid].zprev = ring[dec];
        chips0[(size_t)tid] = chips[(size_t)(row0 + tid / kRdsPhases)];
      }
      for (int i0 = 0; i0 < n_out; i0 += kRdsTile) {
        const int nj = n_out - i0 < kRdsTile ? n_out - i0 : kRdsTile;
        const int kbase = rds_chips_upto(A0, i0 - 1, w19), nct = rds_chips_upto(A0, i0 + nj - 1, w19) - kbase;
        if (i0 > 0)
          for (int k = 0; k < G::carry_n(L); ++k) s_v.at((size_t)G::carry_dst(G::carry_row(k, L), G::carry_col(k, L))) = s_v.at((size_t)G::carry_src(G::carry_row(k, L), G::carry_col(k, L)));
        for (int k = 0; k < G::mix_n(i0, nj, L); ++k) {
          const int rr = G::mix_row(k, i0, nj, L), cc = G::mix_col(k, i0, nj, L), i = i0 + G::mix_rel(cc, L);
          RdsC v{0.f, 0.f};
          if (row0 + rr < nk) {
            const RdsC* q = y + (long long)(row0 + rr) * p.ypitch + i;
            v = rds_mix(q[0], q[-1], m0 + (uint32_t)i, w19, tw.data());
          }
          s_v.at((size_t)G::at(rr, cc)) = v;
        }
        for (int jj = 0; jj < nj; ++jj)
          if (rds_tick(m0 + (uint32_t)(i0 + jj), w19)) s_chip.at((size_t)(rds_chips_upto(A0, i0 + jj, w19) - kbase - 1)) = jj;
        for (int k = 0; k < G::fir_n(p.nseg, nct); ++k) {
          const int ci = G::fir_chip(k, nct), rr = G::fir_row(k, nct), seg = G::fir_seg(k, nct);
          s_part.at((size_t)G::part_at(seg, rr, ci)) = rds_segment(s_v.data() + G::newest(rr, s_chip[(size_t)ci], L), s_g.data(), L, seg);
        }
        for (int tid = 0; tid < G::kDecoders; ++tid) {
          if (!mine(tid)) continue;
          const int r = tid / kRdsPhases, ph = tid % kRdsPhases;
          const size_t dec = (size_t)dec_of(tid);
          for (int ci = (int)(((uint32_t)ph - (chips0[(size_t)tid] + (uint32_t)kbase)) & 15u); ci < nct; ci += kRdsPhases) {
            const RdsC zc = rds_sum(s_part.data() + G::part_at(0, r, ci), ROWS * G::kCp, p.nseg);
            last_z[(size_t)(row0 + r) * (size_t)total + (size_t)(kbase + ci)] = zc;
            rds_bit(z[(size_t)tid], zc, i0 + s_chip[(size_t)ci], ph, events.data() + dec * (size_t)p.cap, cnt[(size_t)tid], p.cap);
          }
        }
      }
      std::vector<RdsC> keep((size_t)G::roll_n(L));
      for (int k = 0; k < G::roll_n(L); ++k)
        if (row0 + G::roll_row(k, L) < nk) keep[(size_t)k] = y[(long long)(row0 + G::roll_row(k, L)) * p.ypitch + G::roll_src(n_out, G::roll_col(k, L), L)];
      for (int k = 0; k < G::roll_n(L); ++k)
        if (row0 + G::roll_row(k, L) < nk) y[(long long)(row0 + G::roll_row(k, L)) * p.ypitch + G::roll_dst(G::roll_col(k, L), L)] = keep[(size_t)k];
      for (int tid = 0; tid < G::kDecoders; ++tid) {
        if (!mine(tid)) continue;
        const size_t dec = (size_t)dec_of(tid);
        for (int b = 0; b < 4; ++b) regs[(size_t)b * nd + dec] = z[(size_t)tid].w[b];
        ring[dec] = z[(size_t)tid].zprev;
        counts[dec] = cnt[(size_t)tid];
        if (tid % kRdsPhases == 0) chips[(size_t)(row0 + tid / kRdsPhases)] = chips0[(size_t)tid] + (uint32_t)total;
      }
    }
    return total;
  }
};

// ---- signals ------------------------------------------------------------------------------------------------------------------
static uint32_t make_block(uint32_t info, uint32_t off) { return info << 10 | (plain_mod((uint64_t)info << 10, 26) ^ off); }
struct Group { uint32_t w[4]; int c2; };
static std::vector<int> group_bits(const std::vector<Group>& gs) {
  std::vector<int> bits;
  for (const Group& g : gs) {
    const uint32_t off[4] = {0x0FC, 0x198, g.c2 ? 0x350u : 0x168u, 0x1B4};
    for (int b = 0; b < 4; ++b) { const uint32_t blk = make_block(g.w[b], off[b]); for (int k = 25; k >= 0; --k) bits.push_back((int)(blk >> k & 1u)); }
  }
  return bits;
}
static double shaping(double t) {
  auto sinc = [](double x) { return x == 0 ? 1.0 : sin(M_PI * x) / (M_PI * x); };
  return 2.0 * (sinc(0.5 + 4.0 * t) + sinc(0.5 - 4.0 * t));
}
static double pulse(double t) { return shaping(t + 0.25) - shaping(t - 0.25); }
// a station at the row's rate: pilot and RDS on an FM carrier `off` Hz from the centre, added to y from `at` on
static void add_station(std::vector<RdsC>& y, size_t at, const std::vector<int>& bits, double fs, double off, double amp) {
  std::vector<double> a;
  int e = 0;
  a.push_back(-1.0);
  for (int b : bits) { e ^= b; a.push_back(e ? 1.0 : -1.0); }
  const size_t n = (size_t)((double)(a.size() + 2) * fs / 1187.5);
  double ph = 0;
  for (size_t i = 0; i < n && at + i < y.size(); ++i) {
    const double t = (double)i * 1187.5 / fs - 1.0;                    // in bits; symbol k is centred at k + 0.5
    double s = 0;
    for (long k = (long)floor(t) - 2; k <= (long)floor(t) + 2; ++k)
      if (k >= 0 && k < (long)a.size()) s += a[(size_t)k] * pulse(t - (double)k - 0.5);
    const double th = 2 * M_PI * 19000.0 * (double)i / fs;
    const double mpx = 6750.0 * sin(th) + 2000.0 * (s / 2.5) * sin(3 * th) + 20000.0 * sin(2 * M_PI * 1000.0 * (double)i / fs);
    ph += 2 * M_PI * (mpx + off) / fs;
    y[at + i].x += (float)(amp * cos(ph));
    y[at + i].y += (float)(amp * sin(ph));
  }
}

static long phases(double fs_out, int nk, int max_out, uint32_t m_base) {
  const int L = length_of(fs_out);
  Device dv;
  dv.nk = nk; dv.L = L; dv.w19 = word_of(19000, fs_out);
  const pysdr_rds_cfg c{dv.w19};
  REQUIRE(rds_plan(nk, L, max_out, &c, &dv.p), "plan");
  dv.tw.resize(kRdsNt);
  for (int k = 0; k < kRdsNt; ++k) dv.tw[(size_t)k] = RdsC{(float)cos(2 * M_PI * k / kRdsNt), (float)-sin(2 * M_PI * k / kRdsNt)};
  double norm = 0;
  for (int i = 0; i < L; ++i) norm += fabs(pulse((i - (L - 1) / 2) * 1187.5 / fs_out));
  for (int i = 0; i < L; ++i) dv.g.push_back((float)(pulse((i - (L - 1) / 2) * 1187.5 / fs_out) / norm));
  dv.init();
  std::vector<Group> sent;
  const size_t n = (size_t)(0.21 * fs_out);
  std::vector<std::vector<RdsC>> rows((size_t)nk, std::vector<RdsC>(n));
  for (int a = 0; a < nk; ++a) {
    for (RdsC& v : rows[(size_t)a]) v = RdsC{0.002f * rndf(), 0.002f * rndf()};
    if (a % 3 == 2) continue;                                          // noise alone
    std::vector<Group> gs;
    gs.push_back(Group{{0x1234u + (uint32_t)a, 0x0408u + (uint32_t)a, 0xE0CDu, 0x4142u + (uint32_t)a}, 0});
    gs.push_back(Group{{0x1234u + (uint32_t)a, 0x2810u | (uint32_t)a, 0x1234u + (uint32_t)a, 0x6162u}, 1});   // version B
    sent.insert(sent.end(), gs.begin(), gs.end());
    add_station(rows[(size_t)a], (size_t)(300 + 17 * a), group_bits(gs), fs_out, a % 2 ? 12000.0 : -8000.0, 0.1);
  }
  const long bad[3] = {(long)n - 9000, (long)n - 7000, (long)n - 5000};
  rows[0][(size_t)bad[0]] = RdsC{NAN, 0.1f}; rows[0][(size_t)bad[1]] = RdsC{0.1f, INFINITY}; rows[0][(size_t)bad[2]] = RdsC{0.f, 0.f};
  Plain pl;
  pl.L = L; pl.w19 = dv.w19; pl.tw = dv.tw; pl.g = dv.g; pl.rows.resize((size_t)nk);
  for (long b : bad)                                                   // d is 0 at the sample and at the one behind it, and finite everywhere
    for (long q = b; q <= b + 1; ++q) REQUIRE(Plain::arg(rows[0][(size_t)q], rows[0][(size_t)q - 1]) == 0.f && rds_arg(rows[0][(size_t)q], rows[0][(size_t)q - 1]) == 0.f, "d at a bad sample");
  std::vector<int> cuts = {1, 1, kRdsTile - 1, kRdsTile, kRdsTile + 1, 2, 2 * kRdsTile + 5};
  for (int& v : cuts) if (v > max_out) v = max_out;
  std::vector<Group> got;
  long at = 0, words_total = 0, chips_total = 0;
  size_t ci = 0;
  while (at < (long)n) {
    int n_out = ci < cuts.size() ? cuts[ci++] : max_out;
    if (n_out > (long)n - at) n_out = (int)((long)n - at);
    for (int a = 0; a < nk; ++a) memcpy(dv.Y.data() + (size_t)a * dv.p.ypitch + kRdsHpad, rows[(size_t)a].data() + at, (size_t)n_out * sizeof(RdsC));
    const int total = dv.call(n_out, m_base + (uint32_t)at);
    chips_total += total;
    for (int a = 0; a < nk; ++a) {
      std::vector<int32_t> words[16];
      int k = 0;
      for (int j = 0; j < n_out; ++j) {
        if (!rds_tick(m_base + (uint32_t)(at + j), dv.w19)) continue;
        const RdsC want = pl.z(rows[(size_t)a], at + j, m_base), have = dv.last_z[(size_t)a * (size_t)total + (size_t)k];
        REQUIRE(fbits(have.x) == fbits(want.x) && fbits(have.y) == fbits(want.y) && std::isfinite(want.x) && std::isfinite(want.y),
                "fs_out %g row %d output %ld: z (%g, %g), expected (%g, %g)", fs_out, a, at + j, have.x, have.y, want.x, want.y);
        pl.chip(a, want, j, words);
        ++k;
      }
      REQUIRE(k == total && dv.chips[(size_t)a] == pl.rows[(size_t)a].chips, "row %d: chips", a);
      for (int ph = 0; ph < 16; ++ph) {
        const size_t dec = (size_t)a * 16 + (size_t)ph, nd = (size_t)dv.p.ndec;
        const std::vector<int32_t>& w = words[ph];
        REQUIRE(dv.counts[dec] == (int)w.size() && (int)w.size() <= dv.p.cap, "decoder %zu: %d words, expected %zu", dec, dv.counts[dec], w.size());
        for (size_t q = 0; q < w.size(); ++q) REQUIRE(dv.events[dec * (size_t)dv.p.cap + q] == w[q], "decoder %zu word %zu", dec, q);
        words_total += (long)w.size();
        for (size_t q = 0; q + 2 < w.size(); q += 3) {
          REQUIRE(rds_header_index(w[q]) < n_out && rds_header_phase(w[q]) == ph, "header");
          got.push_back(Group{{(uint32_t)w[q + 1] >> 16, (uint32_t)w[q + 1] & 0xFFFFu, (uint32_t)w[q + 2] >> 16, (uint32_t)w[q + 2] & 0xFFFFu}, rds_header_c2(w[q])});
        }
        const std::vector<int>& b = pl.rows[(size_t)a].bits[ph];
        uint64_t blk[4] = {0, 0, 0, 0};
        for (size_t q = 0; q < b.size(); ++q) { const size_t pos = 104 - b.size() + q; blk[pos / 26] = blk[pos / 26] << 1 | (uint64_t)b[q]; }
        for (int q = 0; q < 4; ++q) REQUIRE(dv.regs[(size_t)q * nd + dec] == (uint32_t)blk[q], "decoder %zu block %d after output %ld", dec, q, at + n_out);
        const RdsC r0 = dv.ring[dec], r1 = pl.rows[(size_t)a].ring[ph];
        REQUIRE(fbits(r0.x) == fbits(r1.x) && fbits(r0.y) == fbits(r1.y), "decoder %zu ring", dec);
      }
    }
    at += n_out;
  }
  auto same = [](const Group& p, const Group& q) { return !memcmp(p.w, q.w, sizeof p.w) && p.c2 == q.c2; };
  for (const Group& s : sent) { int copies = 0; for (const Group& q : got) copies += same(s, q); REQUIRE(copies >= 3, "a group was read on %d phases", copies); }
  for (const Group& q : got) { bool ok = false; for (const Group& s : sent) ok = ok || same(s, q); REQUIRE(ok, "a group that was not sent"); }
  REQUIRE(chips_total > 0, "chips");
  return words_total;
}

// ---- the cap --------------------------------------------------------------------------------------------------------------------
static long densest() {
  // a register whose every shift completes a group does not exist, so the slots are filled through rds_bit's own door: a
  // decoder that holds a good group gets it again after 104 bits; here every bit is made to complete one by reloading.
  long checked = 0;
  const Group g{{0xABCDu, 0x0123u, 0x4567u, 0x89ABu}, 0};
  const std::vector<int> bits = group_bits({g});
  for (uint32_t w : {kRdsW19Min, word_of(19000, 400000.0), kRdsW19Max})
    for (int mo : {1, 11, 12, 13, 26, 27, 28, 400, 1024, 65536}) {
      const int cap = rds_event_cap(mo, w), nbits = rds_max_bits(mo, w);
      std::vector<int32_t> ev((size_t)cap, 0);
      int cnt = 0;
      for (int b = 0; b < nbits; ++b) {
        RdsDec d{};
        uint64_t blk[4] = {0, 0, 0, 0};
        for (int k = 0; k < 103; ++k) blk[(k + 1) / 26] = blk[(k + 1) / 26] << 1 | (uint64_t)bits[(size_t)k];   // all but the last bit, shifted in
        for (int q = 0; q < 4; ++q) d.w[q] = (uint32_t)blk[q];
        d.zprev = RdsC{1.f, 0.f};
        rds_bit(d, RdsC{bits[103] ? -1.f : 1.f, 0.f}, b, 5, ev.data(), cnt, cap);
      }
      REQUIRE(cnt == cap && cnt == 3 * nbits, "w %u max_out %d: %d words of %d", w, mo, cnt, cap);
      REQUIRE((uint32_t)ev[1] == 0xABCD0123u && (uint32_t)ev[2] == 0x456789ABu && rds_header_phase(ev[0]) == 5 && rds_header_c2(ev[0]) == 0, "the words");
      ++checked;
    }
  for (int i : {0, 1, 1023, 1024, (1 << 20) - 1})
    for (int ph = 0; ph < 16; ++ph)
      for (int c2 = 0; c2 < 2; ++c2) { const int32_t h = rds_header(i, ph, c2); REQUIRE(rds_header_index(h) == i && rds_header_phase(h) == ph && rds_header_c2(h) == c2 && h >= 0, "header"); }
  return checked;
}

// ---- the constants ------------------------------------------------------------------------------------------------------------------
static void constants() {
  auto mulx = [](uint32_t v) { v <<= 1; return (v & 0x400u) ? (v ^ 0x5B9u) & 0x3FFu : v; };   // v x mod g
  uint32_t v = 1;
  int order = 0;
  do { v = mulx(v); ++order; } while (v != 1);
  REQUIRE(order == 341, "x has order %d modulo g", order);
  const uint32_t off[5] = {kRdsOffA, kRdsOffB, kRdsOffC, kRdsOffC2, kRdsOffD}, want[5] = {0x3D8, 0x3D4, 0x25C, 0x3CC, 0x258};
  for (int k = 0; k < 5; ++k) {
    uint32_t s = off[k];
    for (int e = 0; e < 325; ++e) s = mulx(s);
    REQUIRE(s == want[k], "offset %d: (o x^325) mod g = 0x%X", k, s);
    REQUIRE(rds_syndrome(make_block(0xFFFFu, off[k])) == off[k] && rds_syndrome(make_block(0x1u, off[k]) ^ 4u) != off[k], "a block checks with its offset");
  }
  for (uint32_t b = 0; b < (1u << 26); b += 977u) REQUIRE(rds_syndrome(b) == plain_mod(b, 26), "remainder of 0x%X", b);
  REQUIRE(rds_syndrome(0u) == 0u, "a zeroed register matches no offset");
}

int main() {
  rules();
  constants();
  const long chips = grid();
  long steps = 0;
  for (double fs : {228000.0, 400000.0, 512000.0})
    for (int nk : {1, 2, 3, 5})
      for (int n_out : {1, 2, 11, 12, 13, 1023, 1024, 1025, 2048, 2049, 3500})
        steps += walk(nk, n_out, length_of(fs), word_of(19000, fs), (uint32_t)(n_out * 2654435761u), (uint32_t)(nk * 7 + n_out));
  long w = 0;
  w += phases(400000.0, 3, 4096, 0u);
  w += phases(228000.0, 2, 256, 0xFFFFF000u);                          // the absolute index wraps inside the run
  w += phases(512000.0, 1, 1500, 123456789u);
  const long d = densest();
  printf("RDS_PLAN_OK chips %ld, walk steps %ld, event words %ld, cap cases %ld\n", chips, steps, w, d);
  return 0;
}
