// The packet skimmer's plan, staging geometry, steps and event slots (pysdr_amd/csrc/pkt_plan.h, the very code pkt.hip steps
// with) on the CPU under AddressSanitizer + UBSan.
//   * the rules: L in [8, 40], nk >= 1, 8 nk <= 2^18, max_out in [1, 2^20] and the settings' rules; the groups tile [0, nk),
//     the row pitch holds the history's room and max_out.
//   * the tile walk of the kernel, through the index functions of PktGeom that pkt.hip itself uses: every staging load
//     goes to a Y of exactly nk x pitch elements and LDS tiles of exactly their size (heap: the sanitizer guards both
//     ends); every row sample is loaded once; the mixer sees sample n and n - 1; every window sees product m - i at tap i;
//     every (row, output) gets its powers once, and the decoders consume them in order; the history roll stays in the row.
//   * both phases with real samples -- AFSK frames on FM carriers, noise, a NaN, an infinite and an over-pmax sample --
//     as the kernel runs them, call after call (1 output, tile - 1, tile, tile + 1, max_out = 16 and 256), against a plain
//     transcription of DESIGN.md 3 item 29 over the rows' memory: powers bit for bit, counts, event words, every state
//     field and the frame buffers after every call; the frames sent are the frames read.
//   * the cap: the clock's samplings are never closer than pkt_sample_gap under any slicer sequence tried (none, all,
//     random and the ones that pull hardest), for every pll_shift; the words of a frame never exceed its samplings / 24;
//     the densest stream there is -- a 330-byte frame carried in, then frames of 15 and of 17 bytes that share their
//     flags, a bit at every sampling the clock allows -- fills no more than the cap for every call length and offset.
//   * the event words round-trip.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pkt_plan.h"

using namespace pysdr;

#define REQUIRE(c, ...) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

typedef std::vector<uint8_t> Bytes;

static uint32_t word_of(double f, double fs) { return (uint32_t)llround(f / fs * 4294967296.0); }

static pysdr_pkt_cfg good_cfg(double fs_out) {
  pysdr_pkt_cfg c{};
  for (int s = 0; s < 8; ++s) c.gain[s] = (float)pow(10.0, (-6 + 2 * s) / 10.0);
  c.pmax = 1e18f; c.w_mark = word_of(1200, fs_out); c.w_space = word_of(2200, fs_out); c.w_baud = word_of(1200, fs_out); c.pll_shift = 2;
  return c;
}

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float rndf() { return (float)((int)(rnd() & 0xFFFF) - 32768) / 32768.f; }

// ---- the rules --------------------------------------------------------------------------------------------------------
static void rules() {
  PktPlan p;
  const pysdr_pkt_cfg c = good_cfg(25000.0);
  for (int L = 0; L < 50; ++L) REQUIRE(pkt_plan(4, L, 64, &c, &p) == (L >= 8 && L <= 40), "L %d", L);
  REQUIRE(!pkt_plan(0, 21, 64, &c, &p) && !pkt_plan(-1, 21, 64, &c, &p) && !pkt_plan((1 << 15) + 1, 21, 64, &c, &p) && pkt_plan(1 << 15, 21, 64, &c, &p), "nk");
  REQUIRE(!pkt_plan(4, 21, 0, &c, &p) && !pkt_plan(4, 21, (1 << 20) + 1, &c, &p) && pkt_plan(4, 21, 1 << 20, &c, &p) && !pkt_plan(4, 21, 64, nullptr, &p), "max_out, cfg");
  const float badf[] = {0.f, -1.f, NAN, INFINITY, -INFINITY};
  for (float v : badf) {
    for (int s = 0; s < 8; ++s) { pysdr_pkt_cfg b = c; b.gain[s] = v; REQUIRE(!pkt_plan(4, 21, 64, &b, &p), "gain"); }
    pysdr_pkt_cfg b = c; b.pmax = v; REQUIRE(!pkt_plan(4, 21, 64, &b, &p), "pmax");
  }
  { pysdr_pkt_cfg b = c; b.pmax = 1.1e18f; REQUIRE(!pkt_plan(4, 21, 64, &b, &p), "pmax above"); }
  { pysdr_pkt_cfg b = c; b.w_mark = 0; REQUIRE(!pkt_plan(4, 21, 64, &b, &p), "w_mark"); b = c; b.w_space = 0; REQUIRE(!pkt_plan(4, 21, 64, &b, &p), "w_space");
    b = c; b.w_baud = 0; REQUIRE(!pkt_plan(4, 21, 64, &b, &p), "w_baud"); b.w_baud = (1u << 29) + 1; REQUIRE(!pkt_plan(4, 21, 64, &b, &p), "w_baud above");
    b.w_baud = 1u << 29; REQUIRE(pkt_plan(4, 21, 64, &b, &p), "w_baud at 8 samples per bit"); }
  for (int sh = -1; sh < 7; ++sh) { pysdr_pkt_cfg b = c; b.pll_shift = sh; REQUIRE(pkt_plan(4, 21, 64, &b, &p) == (sh >= 1 && sh <= 4), "pll_shift %d", sh); }
  const int nks[] = {1, 7, 8, 9, 16, 17, 800}, mos[] = {1, 16, 63, 64, 65, 256, 4096, 1 << 20};
  for (int nk : nks) for (int mo : mos) {
    REQUIRE(pkt_plan(nk, 21, mo, &c, &p), "good");
    REQUIRE(p.ndec == 8 * nk && p.groups * PktGeom::kRows >= nk && (p.groups - 1) * PktGeom::kRows < nk, "groups");
    REQUIRE(p.ypitch >= kPktHpad + mo && p.ypitch % 16 == 0 && p.cap == pkt_event_cap(mo, c.w_baud) && p.cap >= 84, "pitch, cap");
  }
  REQUIRE(pkt_sample_gap(c.w_baud) == 11 && pkt_sample_gap(1u << 29) == 5 && pkt_max_samplings(4096, c.w_baud) == 373 && pkt_event_cap(4096, c.w_baud) == 99, "gap");
  REQUIRE(sizeof(pysdr_pkt_cfg) == 52 && sizeof(PktV) == 16 && sizeof(PktP) == 8 && sizeof(PktC) == 8, "sizes");
}

// ---- the tile walk ------------------------------------------------------------------------------------------------------
static long walk(int nk, int n_out, int L, const PktPlan& p) {
  using G = PktGeom;
  constexpr int ROWS = G::kRows, TH = G::kThreads;
  std::vector<int> loads((size_t)nk * p.ypitch, 0);
  long steps = 0;
  REQUIRE(G::carry_n(L) <= 2 * TH, "two carried samples per thread");
  for (int g = 0; g < p.groups; ++g) {
    const int row0 = g * ROWS;
    std::vector<long> ty((size_t)ROWS * G::kYp, -2L), tv((size_t)ROWS * G::kYp, -2L);   // the memory index a slot holds; -1: a zero
    std::vector<int> tp((size_t)ROWS * G::kPp, -2);
    std::vector<int> next((size_t)G::kDecoders, 0);
    for (int i0 = 0; i0 < n_out; i0 += kPktTile) {
      std::vector<long> carry((size_t)G::carry_n(L), -1L);
      for (int k = 0; k < G::carry_n(L); ++k) {
        const int hr = G::carry_row(k, L), hc = G::carry_col(k, L);
        REQUIRE(hr < ROWS && hc < L, "carry index");
        if (i0 > 0) carry[(size_t)k] = ty.at((size_t)G::carry_src(hr, hc));
        else if (row0 + hr < nk) { carry[(size_t)k] = (long)(row0 + hr) * p.ypitch + kPktHpad + G::hist_off(hc, L); loads.at((size_t)carry[(size_t)k]) += 1; }
      }
      std::fill(ty.begin(), ty.end(), -2L);
      for (int k = 0; k < G::carry_n(L); ++k) {
        long& slot = ty.at((size_t)G::carry_dst(G::carry_row(k, L), G::carry_col(k, L)));
        REQUIRE(slot == -2, "carried slot written twice");
        slot = carry[(size_t)k];
      }
      for (int k = 0; k < ROWS * kPktTile; ++k) {
        const int rr = G::stage_row(k), c = G::stage_col(k), i = i0 + c;
        long v = -1;
        if (row0 + rr < nk && i < n_out) { v = (long)(row0 + rr) * p.ypitch + kPktHpad + i; loads.at((size_t)v) += 1; }
        long& slot = ty.at((size_t)G::stage_dst(rr, c, L));
        REQUIRE(slot == -2, "LDS slot written twice");
        slot = v;
      }
      for (int r = 0; r < ROWS; ++r)
        for (int c = 0; c < L + kPktTile; ++c) {
          const long v = ty[(size_t)G::at(r, c)];
          const int rel = i0 + c - L;
          if (row0 + r < nk && rel < n_out) REQUIRE(v == (long)(row0 + r) * p.ypitch + kPktHpad + rel, "slot (%d, %d) holds %ld", r, c, v);
          else REQUIRE(v == -1, "a zero expected");
        }
      std::fill(tv.begin(), tv.end(), -2L);
      for (int k = 0; k < G::mix_n(L); ++k) {                       // phase A1
        const int rr = G::mix_row(k, L), c = G::mix_col(k, L);
        REQUIRE(rr < ROWS && c >= 1 && c < L + kPktTile, "mixer index");
        REQUIRE(ty[(size_t)G::at(rr, c)] != -2 && ty[(size_t)G::at(rr, c - 1)] != -2, "the mixer reads a slot never written");
        long& slot = tv.at((size_t)G::at(rr, c));
        REQUIRE(slot == -2, "product written twice");
        slot = i0 + G::mix_rel(c, L);                               // the sample's index within the call
      }
      const int nj = n_out - i0 < kPktTile ? n_out - i0 : kPktTile;
      std::fill(tp.begin(), tp.end(), -2);
      for (int k = 0; k < ROWS * kPktTile; ++k) {                   // phase A2
        const int rr = G::stage_row(k), jj = G::stage_col(k);
        for (int i = 0; i < L; ++i) REQUIRE(tv.at((size_t)G::win(rr, jj, L) - i) == i0 + jj - i, "tap %d of output %d", i, i0 + jj);
        int& slot = tp.at((size_t)G::pw_at(rr, jj));
        REQUIRE(slot == -2, "power written twice");
        slot = i0 + jj;
      }
      for (int tid = 0; tid < G::kDecoders; ++tid) {                // phase B
        const int r = tid / kPktSlicers, row = row0 + r;
        if (row >= nk) continue;
        for (int jj = 0; jj < nj; ++jj) {
          REQUIRE(tp.at((size_t)G::pw_at(r, jj)) == i0 + jj && next[(size_t)tid] == i0 + jj, "out of order");
          next[(size_t)tid] += 1;
          ++steps;
        }
      }
    }
    for (int k = 0; k < G::carry_n(L); ++k) {                       // the history roll
      const int row = row0 + G::carry_row(k, L), j = G::carry_col(k, L);
      if (row >= nk) continue;
      const long src = (long)row * p.ypitch + kPktHpad + G::roll_src(n_out, j, L), dst = (long)row * p.ypitch + kPktHpad + G::roll_dst(j, L);
      REQUIRE(src >= (long)row * p.ypitch && src < (long)row * p.ypitch + kPktHpad + n_out && dst >= (long)row * p.ypitch && dst < (long)row * p.ypitch + kPktHpad, "roll");
      REQUIRE(src - dst == n_out, "the roll moves by the call's outputs");
    }
  }
  for (int r = 0; r < nk; ++r)
    for (int i = 0; i < p.ypitch; ++i) {
      const int rel = i - kPktHpad;
      const int want = (rel >= -L && rel < n_out) ? 1 : 0;
      REQUIRE(loads[(size_t)r * p.ypitch + i] == want, "nk %d n_out %d: (%d, %d) loaded %d x", nk, n_out, r, rel, loads[(size_t)r * p.ypitch + i]);
    }
  return steps;
}

// ---- signals ----------------------------------------------------------------------------------------------------------------
static uint16_t fcs_of(const Bytes& f) {
  uint32_t crc = 0xFFFF;
  for (uint8_t b : f)
    for (int k = 0; k < 8; ++k) { crc = (crc >> 1) ^ (((crc ^ (uint32_t)(b >> k)) & 1u) ? 0x8408u : 0u); }
  return (uint16_t)(crc ^ 0xFFFFu);
}

static Bytes make_frame(int n, int salt) {
  Bytes f((size_t)n);
  for (int i = 0; i < n; ++i) f[(size_t)i] = (uint8_t)((i < 14 ? ('A' + (i + salt) % 26) << 1 : (salt == 99 ? 0xFF : (i * 37 + salt * 11) & 0xFF)));
  return f;
}

// the bits of a transmission: flags, frames (FCS, stuffing) that share single flags, flags
static std::vector<int> hdlc_bits(const std::vector<Bytes>& frames, int pre, int post) {
  static const int flag[8] = {0, 1, 1, 1, 1, 1, 1, 0};
  std::vector<int> bits;
  for (int k = 0; k < pre; ++k) bits.insert(bits.end(), flag, flag + 8);
  for (size_t q = 0; q < frames.size(); ++q) {
    Bytes f = frames[q];
    const uint16_t c = fcs_of(f);
    f.push_back((uint8_t)(c & 0xFF)); f.push_back((uint8_t)(c >> 8));
    int ones = 0;
    for (uint8_t b : f)
      for (int i = 0; i < 8; ++i) {
        const int bit = (b >> i) & 1;
        bits.push_back(bit);
        ones = bit ? ones + 1 : 0;
        if (ones == 5) { bits.push_back(0); ones = 0; }
      }
    for (int k = 0; k < (q + 1 == frames.size() ? post : 1); ++k) bits.insert(bits.end(), flag, flag + 8);
  }
  return bits;
}

// AFSK on an FM carrier at the row's rate, added to y from `at` on
static void add_station(std::vector<PktC>& y, size_t at, const std::vector<int>& bits, double fs, double off, double amp, double bal) {
  const size_t n = (size_t)floor((double)bits.size() * fs / 1200.0);
  double th = 0, ph = 0;
  int level = 1;
  size_t bit_at = (size_t)-1;
  for (size_t i = 0; i < n && at + i < y.size(); ++i) {
    const size_t b = (size_t)((double)i * 1200.0 / fs);
    if (b != bit_at) { bit_at = b; if (!bits[b < bits.size() ? b : bits.size() - 1]) level ^= 1; }
    th += 2 * M_PI * (level ? 1200.0 : 2200.0) / fs;
    const double a = (level ? 1.0 : bal) / (bal > 1 ? bal : 1.0) * sin(th);
    ph += 2 * M_PI * (3000.0 * a + off) / fs;
    y[at + i].x += (float)(amp * cos(ph));
    y[at + i].y += (float)(amp * sin(ph));
  }
}

// ---- the plain transcription of DESIGN.md 3 item 29 ----------------------------------------------------------------------------
struct Plain {
  int L; pysdr_pkt_cfg c; std::vector<PktC> tw; std::vector<float> g;
  struct D { int32_t clk = 0, xprev = 0, xlast = 0, sr = 0, ones = 0, inframe = 0, byte = 0, nb = 0, nbytes = 0, crc = 0xFFFF; Bytes fb = Bytes(332, 0); };
  std::vector<D> d;
  static PktC sample(const std::vector<PktC>& y, long n) { return n < 0 ? PktC{0.f, 0.f} : y[(size_t)n]; }
  // steps 1 and 2 for the output m of the row whose whole stream is y; the stream's first output has the absolute index m_base
  PktP powers(const std::vector<PktC>& y, long m, uint32_t m_base) const {
    float P[2];
    const uint32_t w[2] = {c.w_mark, c.w_space};
    for (int t = 0; t < 2; ++t) {
      float ux = 0.f, uy = 0.f;
      for (int i = 0; i < L; ++i) {
        const long n = m - i;
        const PktC a = sample(y, n), b = sample(y, n - 1);
        const float dd = a.y * b.x - a.x * b.y;
        const uint32_t k = (uint32_t)((m_base + (uint32_t)n) * w[t]) >> 22;   // the absolute index: its low 32 bits
        const float vx = dd * tw[k].x, vy = dd * tw[k].y;
        if (i == 0) { ux = g[0] * vx; uy = g[0] * vy; }
        else { ux = ux + g[(size_t)i] * vx; uy = uy + g[(size_t)i] * vy; }
      }
      const float pw = ux * ux + uy * uy;
      P[t] = !(pw <= c.pmax) ? 0.f : pw;
    }
    return PktP{P[0], P[1]};
  }
  // steps 3 to 6; words: the decoder's events of this call
  void step(int dec, PktP p, int i, std::vector<int32_t>& words) {
    D& z = d[(size_t)dec];
    const int x = c.gain[dec % 8] * p.space > p.mark ? 1 : 0;
    const int32_t prev = z.clk;
    z.clk = (int32_t)((uint32_t)z.clk + c.w_baud);
    if (x != z.xprev) z.clk -= z.clk >> c.pll_shift;
    z.xprev = x;
    if (!(prev >= 0 && z.clk < 0)) return;
    const int bit = x == z.xlast;
    z.xlast = x;
    z.sr = (z.sr >> 1) | (bit << 7);
    if (z.sr == 0x7E) {
      if (z.inframe && z.nb == 7 && z.nbytes >= 17 && z.crc == 0xF0B8) {
        const int n = z.nbytes - 2;
        words.push_back((int32_t)(((uint32_t)i << 10) | (uint32_t)n));
        for (int k = 0; k < n; k += 4) {
          uint32_t v = 0;
          for (int q = 0; q < 4 && k + q < n; ++q) v |= (uint32_t)z.fb[(size_t)(k + q)] << (8 * q);
          words.push_back((int32_t)v);
        }
      }
      z.inframe = 1; z.nb = z.byte = z.nbytes = z.ones = 0; z.crc = 0xFFFF;
      return;
    }
    bool dropped = false;
    if (bit) { z.ones += 1; if (z.ones >= 7) z.inframe = 0; }
    else { dropped = z.ones == 5; z.ones = 0; }
    if (dropped || !z.inframe) return;
    z.byte |= bit << z.nb;
    z.nb += 1;
    if (z.nb == 8) {
      if (z.nbytes < 332) {                                          // a byte that opens a word clears the rest of it
        z.fb[(size_t)z.nbytes] = (uint8_t)z.byte;
        if (z.nbytes % 4 == 0) for (int q = 1; q < 4; ++q) z.fb[(size_t)z.nbytes + q] = 0;
      }
      int32_t b = z.byte;
      for (int k = 0; k < 8; ++k) { z.crc = (z.crc >> 1) ^ (((z.crc ^ b) & 1) ? 0x8408 : 0); b >>= 1; }
      z.nbytes += 1; z.nb = 0; z.byte = 0;
      if (z.nbytes > 332) z.inframe = 0;
    }
  }
};

// ---- the kernel's two phases, as pkt.hip runs them, on heap arrays of exactly their size ---------------------------------------
struct Device {
  int nk, L; PktPlan p; pysdr_pkt_cfg c;
  std::vector<PktC> Y, tw; std::vector<float> g, gain; std::vector<int32_t> si, events, counts; std::vector<uint32_t> frames;
  std::vector<PktP> last_p;                                        // [nk][n_out] of the last call, for the comparison
  void init() {
    Y.assign((size_t)nk * p.ypitch, PktC{0.f, 0.f});
    si.assign((size_t)kPktStateInts * p.ndec, 0);
    for (int i = 0; i < p.ndec; ++i) si[(size_t)9 * p.ndec + i] = kPktCrcInit;
    frames.assign((size_t)p.ndec * kPktFrameWords, 0u);
    events.assign((size_t)p.ndec * p.cap, 0);
    counts.assign((size_t)p.ndec, 0);
    gain.assign(c.gain, c.gain + 8);
  }
  void call(int n_out, uint32_t m0) {
    using G = PktGeom;
    constexpr int ROWS = G::kRows;
    last_p.assign((size_t)nk * n_out, PktP{0.f, 0.f});
    PktC* y = Y.data() + kPktHpad;
    const size_t nd = (size_t)p.ndec;
    for (int grp = 0; grp < p.groups; ++grp) {
      const int row0 = grp * ROWS;
      std::vector<PktC> s_y((size_t)ROWS * G::kYp), s_tw(tw);
      std::vector<PktV> s_v((size_t)ROWS * G::kYp);
      std::vector<PktP> s_p((size_t)ROWS * G::kPp);
      std::vector<float> s_g(g);
      std::vector<PktDec> z((size_t)G::kDecoders);
      std::vector<int> cnt((size_t)G::kDecoders, 0);
      auto mine = [&](int tid) { return row0 + tid / kPktSlicers < nk; };
      auto dec_of = [&](int tid) { return (row0 + tid / kPktSlicers) * kPktSlicers + tid % kPktSlicers; };
      for (int tid = 0; tid < G::kDecoders; ++tid) {
        z[(size_t)tid] = pkt_dec_init();
        if (!mine(tid)) continue;
        const size_t dec = (size_t)dec_of(tid);
        PktDec& q = z[(size_t)tid];
        q.clk = si[dec]; q.xprev = si[nd + dec]; q.xlast = si[2 * nd + dec]; q.sr = si[3 * nd + dec]; q.ones = si[4 * nd + dec];
        q.inframe = si[5 * nd + dec]; q.byte = si[6 * nd + dec]; q.nb = si[7 * nd + dec]; q.nbytes = si[8 * nd + dec]; q.crc = si[9 * nd + dec];
        pkt_word_load(q, frames.data() + dec * kPktFrameWords);
      }
      for (int i0 = 0; i0 < n_out; i0 += kPktTile) {
        std::vector<PktC> carry((size_t)G::carry_n(L), PktC{0.f, 0.f});
        for (int k = 0; k < G::carry_n(L); ++k) {
          const int hr = G::carry_row(k, L), hc = G::carry_col(k, L);
          if (i0 > 0) carry[(size_t)k] = s_y.data()[G::carry_src(hr, hc)];
          else if (row0 + hr < nk) carry[(size_t)k] = y[(long long)(row0 + hr) * p.ypitch + G::hist_off(hc, L)];
        }
        for (int k = 0; k < G::carry_n(L); ++k) s_y.data()[G::carry_dst(G::carry_row(k, L), G::carry_col(k, L))] = carry[(size_t)k];
        for (int k = 0; k < ROWS * kPktTile; ++k) {
          const int rr = G::stage_row(k), c2 = G::stage_col(k), i = i0 + c2;
          PktC v{0.f, 0.f};
          if (row0 + rr < nk && i < n_out) v = y[(long long)(row0 + rr) * p.ypitch + i];
          s_y.data()[G::stage_dst(rr, c2, L)] = v;
        }
        for (int k = 0; k < G::mix_n(L); ++k) {
          const int rr = G::mix_row(k, L), c2 = G::mix_col(k, L);
          const uint32_t n = m0 + (uint32_t)(i0 + G::mix_rel(c2, L));
          s_v.data()[G::at(rr, c2)] = pkt_mix(s_y.data()[G::at(rr, c2)], s_y.data()[G::at(rr, c2 - 1)], n, c.w_mark, c.w_space, s_tw.data());
        }
        for (int k = 0; k < ROWS * kPktTile; ++k) {
          const int rr = G::stage_row(k), jj = G::stage_col(k);
          s_p.data()[G::pw_at(rr, jj)] = pkt_tones(s_v.data() + G::win(rr, jj, L), s_g.data(), L, c.pmax);
        }
        const int nj = n_out - i0 < kPktTile ? n_out - i0 : kPktTile;
        for (int tid = 0; tid < G::kDecoders; ++tid) {
          if (!mine(tid)) continue;
          const int r = tid / kPktSlicers;
          const size_t dec = (size_t)dec_of(tid);
          for (int jj = 0; jj < nj; ++jj) {
            const PktP pw = s_p.data()[G::pw_at(r, jj)];
            last_p[(size_t)(row0 + r) * n_out + i0 + jj] = pw;
            const int x = pkt_slice(gain[(size_t)(tid % kPktSlicers)], pw);
            if (pkt_clock(z[(size_t)tid], x, c.w_baud, c.pll_shift))
              pkt_sample(z[(size_t)tid], x, i0 + jj, frames.data() + dec * kPktFrameWords, events.data() + dec * p.cap, cnt[(size_t)tid], p.cap);
          }
        }
      }
      std::vector<PktC> keep((size_t)G::carry_n(L));
      for (int k = 0; k < G::carry_n(L); ++k)
        if (row0 + G::carry_row(k, L) < nk) keep[(size_t)k] = y[(long long)(row0 + G::carry_row(k, L)) * p.ypitch + G::roll_src(n_out, G::carry_col(k, L), L)];
      for (int k = 0; k < G::carry_n(L); ++k)
        if (row0 + G::carry_row(k, L) < nk) y[(long long)(row0 + G::carry_row(k, L)) * p.ypitch + G::roll_dst(G::carry_col(k, L), L)] = keep[(size_t)k];
      for (int tid = 0; tid < G::kDecoders; ++tid) {
        if (!mine(tid)) continue;
        const size_t dec = (size_t)dec_of(tid);
        const PktDec& q = z[(size_t)tid];
        pkt_word_flush(q, frames.data() + dec * kPktFrameWords);
        si[dec] = q.clk; si[nd + dec] = q.xprev; si[2 * nd + dec] = q.xlast; si[3 * nd + dec] = q.sr; si[4 * nd + dec] = q.ones;
        si[5 * nd + dec] = q.inframe; si[6 * nd + dec] = q.byte; si[7 * nd + dec] = q.nb; si[8 * nd + dec] = q.nbytes; si[9 * nd + dec] = q.crc;
        counts[dec] = cnt[(size_t)tid];
      }
    }
  }
};

static uint32_t fbits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }

static long phases(double fs_out, int nk, int max_out, uint32_t m_base) {
  const int L = (int)floor(fs_out / 1200.0 + 0.5);
  Device dv;
  dv.nk = nk; dv.L = L; dv.c = good_cfg(fs_out);
  REQUIRE(pkt_plan(nk, L, max_out, &dv.c, &dv.p), "plan");
  dv.tw.resize(kPktNt);
  for (int k = 0; k < kPktNt; ++k) dv.tw[(size_t)k] = PktC{(float)cos(2 * M_PI * k / kPktNt), (float)-sin(2 * M_PI * k / kPktNt)};
  dv.g.assign((size_t)L, (float)(1.0 / L));
  dv.init();
  // the rows: a station on some, two frames that share a flag on one, noise on all; three samples that must be blanked
  std::vector<Bytes> sent;
  const size_t n = (size_t)(0.5 * fs_out);
  std::vector<std::vector<PktC>> rows((size_t)nk, std::vector<PktC>(n));
  for (int a = 0; a < nk; ++a) {
    for (PktC& v : rows[(size_t)a]) v = PktC{0.004f * rndf(), 0.004f * rndf()};
    if (a % 3 == 2) continue;                                        // noise alone
    std::vector<Bytes> fr;
    fr.push_back(make_frame(15 + (a * 7) % 20, a == 4 ? 99 : a));
    if (a % 3 == 1) fr.push_back(make_frame(16 + a, a + 40));
    sent.insert(sent.end(), fr.begin(), fr.end());
    add_station(rows[(size_t)a], (size_t)(40 + 13 * a), hdlc_bits(fr, 6, 2), fs_out, (a % 2 ? 700.0 : -300.0), 0.1, a % 3 ? 1.0 : 0.6);
  }
  rows[0][n - 900] = PktC{NAN, 0.1f}; rows[0][n - 700] = PktC{0.1f, INFINITY}; rows[0][n - 500] = PktC{1e15f, 1e15f};
  rows[0][n - 501] = PktC{0.004f, -0.002f}; rows[0][n - 499] = PktC{0.003f, 0.001f};   // so that both of its d are far over pmax
  rows[0][n - 300] = PktC{100.f, 100.f};                             // large, below pmax: not blanked
  Plain pl;
  pl.L = L; pl.c = dv.c; pl.tw = dv.tw; pl.g = dv.g; pl.d.resize((size_t)dv.p.ndec);
  const int tile = kPktTile;
  std::vector<int> cuts = {1, 1, tile - 1, tile, tile + 1, 2, 3 * tile + 5};
  for (int& v : cuts) if (v > max_out) v = max_out;
  std::vector<Bytes> read((size_t)dv.p.ndec);
  std::vector<Bytes> got;
  long at = 0, blanked = 0, words_total = 0;
  size_t ci = 0;
  while (at < (long)n) {
    int n_out = ci < cuts.size() ? cuts[ci++] : max_out;
    if (n_out > (long)n - at) n_out = (int)((long)n - at);
    for (int a = 0; a < nk; ++a) memcpy(dv.Y.data() + (size_t)a * dv.p.ypitch + kPktHpad, rows[(size_t)a].data() + at, (size_t)n_out * sizeof(PktC));
    dv.call(n_out, m_base + (uint32_t)at);
    for (int a = 0; a < nk; ++a) {
      std::vector<std::vector<int32_t>> words(8);
      for (int j = 0; j < n_out; ++j) {
        const PktP want = pl.powers(rows[(size_t)a], at + j, m_base);
        const PktP have = dv.last_p[(size_t)a * n_out + j];
        REQUIRE(fbits(have.mark) == fbits(want.mark) && fbits(have.space) == fbits(want.space), "fs_out %g row %d output %ld: powers (%g, %g), expected (%g, %g)",
                fs_out, a, at + j, have.mark, have.space, want.mark, want.space);
        if (a == 0 && at + j > 0) {                                   // (output 0 has no sample in front of it: d = 0)
          bool touched = false;
          for (long bad : {(long)n - 900, (long)n - 700, (long)n - 500}) touched = touched || (at + j >= bad && at + j <= bad + L);
          REQUIRE(touched == (want.mark == 0.f && want.space == 0.f), "output %ld: blanked %d", at + j, (int)!touched);
          blanked += touched;
        }
        for (int s = 0; s < 8; ++s) pl.step(a * 8 + s, want, j, words[(size_t)s]);
      }
      for (int s = 0; s < 8; ++s) {
        const size_t dec = (size_t)a * 8 + (size_t)s, nd = (size_t)dv.p.ndec;
        const std::vector<int32_t>& w = words[(size_t)s];
        REQUIRE(dv.counts[dec] == (int)w.size() && (int)w.size() <= dv.p.cap, "decoder %zu: %d words, expected %zu", dec, dv.counts[dec], w.size());
        for (size_t k = 0; k < w.size(); ++k) REQUIRE(dv.events[dec * dv.p.cap + k] == w[k], "decoder %zu word %zu", dec, k);
        words_total += (long)w.size();
        for (size_t k = 0; k < w.size();) {
          const int nb = pkt_header_bytes(w[k]);
          REQUIRE(pkt_header_index(w[k]) < n_out && nb >= 15 && nb <= 330, "header");
          Bytes f;
          for (int q = 0; q < nb; ++q) f.push_back((uint8_t)((uint32_t)w[k + 1 + (size_t)q / 4] >> (8 * (q % 4))));
          got.push_back(f);
          k += (size_t)pkt_event_words(nb);
        }
        const Plain::D& z = pl.d[dec];
        const int32_t want_s[10] = {z.clk, z.xprev, z.xlast, z.sr, z.ones, z.inframe, z.byte, z.nb, z.nbytes, z.crc};
        for (int f = 0; f < 10; ++f) REQUIRE(dv.si[(size_t)f * nd + dec] == want_s[f], "decoder %zu field %d after output %ld: %d, expected %d", dec, f, at + n_out, dv.si[(size_t)f * nd + dec], want_s[f]);
        for (int k = 0; k < kPktFrameWords; ++k) {
          uint32_t v = 0;
          for (int q = 0; q < 4; ++q) v |= (uint32_t)z.fb[(size_t)(4 * k + q)] << (8 * q);
          REQUIRE(dv.frames[dec * kPktFrameWords + (size_t)k] == v, "decoder %zu frame word %d after output %ld", dec, k, at + n_out);
        }
      }
    }
    at += n_out;
  }
  REQUIRE(blanked == 3 * (L + 1), "blanked %ld outputs", blanked);
  for (const Bytes& f : sent) {
    int copies = 0;
    for (const Bytes& q : got) copies += q == f;
    REQUIRE(copies >= 2, "a frame of %zu bytes was read %d times", f.size(), copies);
  }
  for (const Bytes& q : got) {
    bool was_sent = false;
    for (const Bytes& f : sent) was_sent = was_sent || q == f;
    REQUIRE(was_sent, "a frame that was not sent");
  }
  return words_total;
}

// ---- the cap ----------------------------------------------------------------------------------------------------------------
static long clock_gaps() {
  long samplings = 0;
  const double rates[] = {9600, 11025, 12500, 19200, 22050, 24000, 25000, 44100, 48000};
  for (double fs : rates)
    for (int sh = 1; sh <= 4; ++sh)
      for (int mode = 0; mode < 6; ++mode) {
        const uint32_t w = word_of(1200, fs);
        const int gap = pkt_sample_gap(w);
        REQUIRE((long long)gap * w > (1ll << 31) && (long long)(gap - 1) * w <= (1ll << 31), "gap");
        PktDec z = pkt_dec_init();
        z.clk = (int32_t)(rnd() << 8);
        long last = -1000;
        int x = 0;
        for (long m = 0; m < 60000; ++m) {
          switch (mode) {
            case 0: break;                                           // no change
            case 1: x ^= 1; break;                                   // a change at every output
            case 2: x = (int)(rnd() & 1); break;
            case 3: if (z.clk < 0) x ^= 1; break;                    // pull while negative: towards the next >= 0
            case 4: if (z.clk >= 0 && (uint32_t)z.clk + w >= (1u << 31)) x ^= 1; break;   // pull at the wrap
            default: if ((rnd() & 7) == 0) x ^= 1; break;
          }
          const int32_t before = z.clk;
          if (pkt_clock(z, x, w, sh)) {
            REQUIRE(m - last >= gap, "fs %g shift %d mode %d: samplings %ld outputs apart, gap %d", fs, sh, mode, m - last, gap);
            REQUIRE(before >= 0 && z.clk < 0, "a sampling is a wrap");
            last = m;
            ++samplings;
          }
        }
      }
  // a nudge never takes the clock across 0 (only -1 to 0)
  for (int sh = 1; sh <= 4; ++sh)
    for (long long c = -70000; c <= 70000; ++c) {
      const int32_t v = (int32_t)c, r = v - (v >> sh);
      REQUIRE(v >= 0 ? (r >= 0 && r <= v) : (r <= 0 && r >= v && (r < 0 || v == -1)), "nudge of %d by %d gives %d", v, sh, r);
    }
  for (int32_t v : {INT32_MIN, INT32_MIN + 1, INT32_MAX, INT32_MAX - 1})
    for (int sh = 1; sh <= 4; ++sh) { const int32_t r = v - (v >> sh); REQUIRE((v < 0) == (r < 0), "nudge at the ends"); }
  return samplings;
}

static long densest() {
  for (int n = 15; n <= 330; ++n)
    REQUIRE(pkt_event_words(n) * kPktSamplingsPerWord <= 8 * n + 24 && pkt_event_words(n) <= kPktFrameWords + 1, "a frame of %d bytes: %d words for %d samplings", n, pkt_event_words(n), 8 * n + 24);
  REQUIRE(pkt_event_words(330) == kPktCarriedWords, "the carried frame");
  // a 330-byte frame, then frames of 17 bytes (6 words per 160 samplings: the densest) and of 15 that share their flags
  std::vector<Bytes> frames;
  frames.push_back(make_frame(330, 3));
  for (int k = 0; k < 40; ++k) { Bytes f((size_t)(k % 3 == 2 ? 15 : 17), 0); for (size_t i = 0; i < f.size(); ++i) f[i] = (uint8_t)(2 * ((i + (size_t)k) % 4)); frames.push_back(f); }
  const std::vector<int> bits = hdlc_bits(frames, 2, 1);
  std::vector<int> level(bits.size());
  int lv = 1;
  for (size_t i = 0; i < bits.size(); ++i) { if (!bits[i]) lv ^= 1; level[i] = lv; }
  long checked = 0;
  const uint32_t ws[] = {word_of(1200, 25000), 1u << 29, word_of(1200, 48000)};
  for (uint32_t w : ws) {
    const int gap = pkt_sample_gap(w);
    const int mos[] = {1, 16, gap, 24 * gap, 24 * gap + 1, 160 * gap, 161 * gap, 1000};
    for (int mo : mos) {
      const int cap = pkt_event_cap(mo, w);
      for (int offset = 0; offset < mo && offset < 400; offset += (mo > 64 ? 7 : 1)) {
        // a sampling every `gap` outputs, the first call `offset` outputs long
        PktDec z = pkt_dec_init();
        std::vector<uint32_t> fb(kPktFrameWords, 0u);
        std::vector<int32_t> ev((size_t)cap, 0);
        int cnt = 0, most = 0;
        long out = 0, call_end = offset ? offset : mo;
        long total_words = 0, frames_read = 0;
        for (size_t b = 0; b < level.size(); ++b) {
          const long m = (long)b * gap;
          while (m >= call_end) {                                    // the call ends: the word in hand goes to memory, the slots start over
            pkt_word_flush(z, fb.data());
            most = cnt > most ? cnt : most;
            total_words += cnt;
            cnt = 0;
            out = call_end;
            call_end += mo;
            pkt_word_load(z, fb.data());
          }
          const int before = cnt;
          pkt_sample(z, level[b], (int)(m - out), fb.data(), ev.data(), cnt, cap);
          frames_read += cnt > before;
        }
        total_words += cnt;
        most = cnt > most ? cnt : most;
        REQUIRE(most <= cap, "w %u max_out %d offset %d: %d words, cap %d", w, mo, offset, most, cap);
        REQUIRE(frames_read == (long)frames.size(), "w %u max_out %d offset %d: %ld of %zu frames (a frame dropped at the cap?)", w, mo, offset, frames_read, frames.size());
        long want = 0;
        for (const Bytes& f : frames) want += pkt_event_words((int)f.size());
        REQUIRE(total_words == want, "words");
        ++checked;
      }
    }
  }
  return checked;
}

static void words() {
  const int is[] = {0, 1, 63, 64, 1023, 4095, (1 << 20) - 1}, ns[] = {15, 16, 17, 18, 329, 330};
  for (int i : is) for (int n : ns) {
    const int32_t w = pkt_header(i, n);
    REQUIRE(pkt_header_index(w) == i && pkt_header_bytes(w) == n && w >= 0, "header (%d, %d)", i, n);
  }
  REQUIRE(pkt_event_words(15) == 5 && pkt_event_words(16) == 5 && pkt_event_words(17) == 6 && pkt_event_words(330) == 84, "words");
}

int main() {
  rules();
  long steps = 0;
  for (int L : {8, 16, 20, 21, 40})
    for (int nk : {1, 7, 8, 9, 17})
      for (int n_out : {1, 2, 39, 40, 41, 63, 64, 65, 128, 129, 300}) {
        PktPlan p;
        const pysdr_pkt_cfg c = good_cfg(1200.0 * L);
        REQUIRE(pkt_plan(nk, L, n_out, &c, &p), "plan");
        steps += walk(nk, n_out, L, p);
      }
  long w = 0;
  w += phases(25000.0, 9, 256, 0u);
  w += phases(19200.0, 3, 16, 0xFFFFF000u);                         // the absolute index wraps inside the run
  w += phases(9600.0, 2, 256, 123456789u);
  w += phases(48000.0, 1, 256, 77u);
  const long s = clock_gaps(), d = densest();
  words();
  printf("PKT_PLAN_OK walk steps %ld, event words %ld, samplings %ld, cap cases %ld\n", steps, w, s, d);
  return 0;
}
