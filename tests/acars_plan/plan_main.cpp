// The ACARS skimmer's plan, staging geometry, steps and event slots (pysdr_amd/csrc/acars_plan.h, the very code acars.hip
// steps with) on the CPU under AddressSanitizer + UBSan.
//   * the rules: L in [8, 21], nk in [1, 2^15], max_out in [1, 2^20] and the settings' rules; the groups tile [0, nk), the
//     row pitch holds the history's room and max_out.
//   * the tile walk of the kernel, through the index functions of AcGeom that acars.hip itself uses: every staging load
//     goes to a Y of exactly nk x pitch elements and LDS tiles of exactly their size (heap: the sanitizer guards both
//     ends); every tile holds the powers of its outputs and of the 5 L samples in front of them; every mixed sample sees
//     power m - i at tap i; the detector sees a[m] and a[m - L]; every (row, output) gets its bit once, and the decoder
//     consumes them in order; the history roll stays in the row.
//   * all phases with real samples -- MSK blocks on AM carriers, noise, a NaN, an infinite and an over-pmax sample -- as
//     the kernel runs them, call after call (1 output, tile - 1, tile, tile + 1, max_out = 16 and 256), against a plain
//     transcription of DESIGN.md 3 item 32 over the rows' memory: the detector's bit, counts, event words, every state
//     field and the frame buffers after every call; the blocks sent are the blocks read.
//   * the cap: the clock's samplings are never closer than acars_sample_gap under any detector sequence tried, for every
//     pll_shift; the words of a frame never exceed its samplings / 24; the densest stream there is -- a 238-byte block
//     carried in, then blocks of 13 bytes whose block check is the next sync word one bit early, a bit at every sampling
//     the clock allows -- fills no more than the cap for every call length and offset.
//   * the frame machine alone: either polarity, ETB, every single flipped bit of a block and its check, a missing SOH,
//     238, 239 and 12 bytes.
//   * the event words round-trip.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "acars_plan.h"

using namespace pysdr;

#define REQUIRE(c, ...) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

typedef std::vector<uint8_t> Bytes;

static uint32_t word_of(double f, double fs) { return (uint32_t)llround(f / fs * 4294967296.0); }

static pysdr_acars_cfg good_cfg(double fs_out) {
  pysdr_acars_cfg c{};
  c.pmax = 1e18f; c.w_car = word_of(1800, fs_out); c.w_baud = word_of(2400, fs_out); c.pll_shift = 2;
  return c;
}

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float rndf() { return (float)((int)(rnd() & 0xFFFF) - 32768) / 32768.f; }

// ---- the rules --------------------------------------------------------------------------------------------------------
static void rules() {
  AcPlan p;
  const pysdr_acars_cfg c = good_cfg(25000.0);
  for (int L = 0; L < 30; ++L) REQUIRE(acars_plan(4, L, 64, &c, &p) == (L >= 8 && L <= 21), "L %d", L);
  REQUIRE(!acars_plan(0, 10, 64, &c, &p) && !acars_plan(-1, 10, 64, &c, &p) && !acars_plan((1 << 15) + 1, 10, 64, &c, &p) && acars_plan(1 << 15, 10, 64, &c, &p), "nk");
  REQUIRE(!acars_plan(4, 10, 0, &c, &p) && !acars_plan(4, 10, (1 << 20) + 1, &c, &p) && acars_plan(4, 10, 1 << 20, &c, &p) && !acars_plan(4, 10, 64, nullptr, &p), "max_out, cfg");
  const float badf[] = {0.f, -1.f, NAN, INFINITY, -INFINITY, 1.1e18f};
  for (float v : badf) { pysdr_acars_cfg b = c; b.pmax = v; REQUIRE(!acars_plan(4, 10, 64, &b, &p), "pmax"); }
  { pysdr_acars_cfg b = c; b.w_car = 0; REQUIRE(!acars_plan(4, 10, 64, &b, &p), "w_car");
    b = c; b.w_baud = 0; REQUIRE(!acars_plan(4, 10, 64, &b, &p), "w_baud"); b.w_baud = (1u << 29) + 1; REQUIRE(!acars_plan(4, 10, 64, &b, &p), "w_baud above");
    b.w_baud = 1u << 29; REQUIRE(acars_plan(4, 10, 64, &b, &p), "w_baud at 8 samples per bit"); }
  for (int sh = -1; sh < 7; ++sh) { pysdr_acars_cfg b = c; b.pll_shift = sh; REQUIRE(acars_plan(4, 10, 64, &b, &p) == (sh >= 1 && sh <= 4), "pll_shift %d", sh); }
  const int nks[] = {1, 7, 8, 9, 16, 17, 400}, mos[] = {1, 16, 63, 64, 65, 256, 4096, 1 << 20};
  for (int nk : nks) for (int mo : mos) {
    REQUIRE(acars_plan(nk, 10, mo, &c, &p), "good");
    REQUIRE(p.NT == 41 && p.groups * AcGeom::kRows >= nk && (p.groups - 1) * AcGeom::kRows < nk, "groups");
    REQUIRE(p.ypitch >= kAcHpad + mo && p.ypitch % 16 == 0 && p.cap == acars_event_cap(mo, c.w_baud) && p.cap >= 61, "pitch, cap");
  }
  REQUIRE(acars_sample_gap(c.w_baud) == 6 && acars_sample_gap(1u << 29) == 5 && acars_max_samplings(4096, c.w_baud) == 683 && acars_event_cap(4096, c.w_baud) == 89, "gap");
  REQUIRE(sizeof(pysdr_acars_cfg) == 16 && sizeof(AcC) == 8, "sizes");
}

// ---- the tile walk ------------------------------------------------------------------------------------------------------
constexpr long kUnset = -9000000L, kZero = -1000000L;   // a slot never written; a slot that holds a zero
static long walk(int nk, int n_out, int L, const AcPlan& p) {
  using G = AcGeom;
  constexpr int ROWS = G::kRows, TH = G::kThreads;
  long steps = 0;
  REQUIRE(G::roll_n(L) <= G::kRollPerThread * TH && G::taps(L) <= kAcTapsMax && G::hist(L) <= kAcHpad, "geometry");
  std::vector<int> touched((size_t)nk * p.ypitch, 0);
  for (int g = 0; g < p.groups; ++g) {
    const int row0 = g * ROWS;
    std::vector<int> next((size_t)ROWS, 0);
    for (int i0 = 0; i0 < n_out; i0 += kAcTile) {
      std::vector<long> tp((size_t)ROWS * G::kPp, kUnset), ta((size_t)ROWS * G::kAp, kUnset);   // the index within the call a slot holds
      std::vector<long> tx((size_t)ROWS * G::kXp, kUnset);
      for (int k = 0; k < G::stage_n(L); ++k) {                     // phase A1
        const int rr = G::stage_row(k, L), c = G::stage_col(k, L), i = i0 + G::stage_rel(c, L);
        REQUIRE(rr < ROWS && c < G::stage_w(L), "stage index");
        long v = kZero;
        if (row0 + rr < nk && i < n_out) { touched.at((size_t)((long)(row0 + rr) * p.ypitch + kAcHpad + i)) += 1; v = i; }
        long& slot = tp.at((size_t)G::p_at(rr, c));
        REQUIRE(slot == kUnset, "power written twice");
        slot = v;
      }
      for (int k = 0; k < G::mix_n(L); ++k) {                       // phase A2
        const int rr = G::mix_row(k, L), c = G::mix_col(k, L), rel = i0 + G::mix_rel(c, L);
        REQUIRE(rr < ROWS && c < G::mix_w(L), "mixer index");
        for (int i = 0; i < G::taps(L); ++i) {
          const long v = tp.at((size_t)G::win(rr, c, L) - (size_t)i);
          REQUIRE(v != kUnset, "the mixer reads a slot never written");
          if (row0 + rr < nk && rel - i < n_out) REQUIRE(v == rel - i, "tap %d of output %d holds %ld", i, rel, v);
          else REQUIRE(v == kZero, "a zero expected");
        }
        long& slot = ta.at((size_t)G::a_at(rr, c));
        REQUIRE(slot == kUnset, "a written twice");
        slot = rel;
      }
      for (int k = 0; k < ROWS * kAcTile; ++k) {                    // phase A3
        const int rr = G::det_row(k), jj = G::det_col(k);
        REQUIRE(ta.at((size_t)G::a_at(rr, jj + L)) == i0 + jj && ta.at((size_t)G::a_at(rr, jj)) == i0 + jj - L, "detector of output %d", i0 + jj);
        long& slot = tx.at((size_t)G::x_at(rr, jj));
        REQUIRE(slot == kUnset, "bit written twice");
        slot = i0 + jj;
      }
      const int nj = n_out - i0 < kAcTile ? n_out - i0 : kAcTile;
      for (int r = 0; r < ROWS; ++r) {                              // phase B
        if (row0 + r >= nk) continue;
        for (int jj = 0; jj < nj; ++jj) {
          REQUIRE(tx.at((size_t)G::x_at(r, jj)) == i0 + jj && next[(size_t)r] == i0 + jj, "out of order");
          next[(size_t)r] += 1;
          ++steps;
        }
      }
    }
    for (int k = 0; k < G::roll_n(L); ++k) {                        // the history roll
      const int row = row0 + G::roll_row(k, L), j = G::roll_col(k, L);
      if (row >= nk) continue;
      const long src = (long)row * p.ypitch + kAcHpad + G::roll_src(n_out, j, L), dst = (long)row * p.ypitch + kAcHpad + G::roll_dst(j, L);
      REQUIRE(src >= (long)row * p.ypitch && src < (long)row * p.ypitch + kAcHpad + n_out && dst >= (long)row * p.ypitch && dst < (long)row * p.ypitch + kAcHpad, "roll");
      REQUIRE(src - dst == n_out, "the roll moves by the call's outputs");
    }
  }
  for (int r = 0; r < nk; ++r)
    for (int i = 0; i < p.ypitch; ++i) {
      const int rel = i - kAcHpad;
      REQUIRE((touched[(size_t)r * p.ypitch + i] > 0) == (rel >= -5 * L && rel < n_out), "nk %d n_out %d: (%d, %d) loaded %d x", nk, n_out, r, rel, touched[(size_t)r * p.ypitch + i]);
    }
  return steps;
}

// ---- signals ----------------------------------------------------------------------------------------------------------------
static uint8_t with_parity(uint8_t b) { b &= 0x7F; return (uint8_t)(b | (__builtin_parity(b) ? 0 : 0x80)); }

static uint16_t bcs_of(const Bytes& f) {
  uint32_t crc = 0;
  for (uint8_t b : f)
    for (int k = 0; k < 8; ++k) { crc = (crc >> 1) ^ (((crc ^ (uint32_t)(b >> k)) & 1u) ? 0x8408u : 0u); }
  return (uint16_t)crc;
}

// a block of n bytes, mode character to ETX (etb: ETB), parity set
static Bytes make_block(int n, int salt, bool etb = false) {
  Bytes f((size_t)n);
  for (int i = 0; i < n - 1; ++i) {
    uint8_t ch = (uint8_t)(0x20 + (i * 7 + salt * 13) % 0x5F);
    f[(size_t)i] = with_parity(ch);
  }
  if (n > 13) f[12] = with_parity(0x02);
  f[(size_t)n - 1] = with_parity(etb ? 0x17 : 0x03);
  return f;
}

// the characters of a transmission: pre-key, + *, SYN SYN, SOH, block, BCS, DEL
static Bytes chars_of(const Bytes& blk, int prekey) {
  Bytes c((size_t)prekey, 0xFF);
  for (uint8_t b : {(uint8_t)'+', (uint8_t)'*', (uint8_t)0x16, (uint8_t)0x16, (uint8_t)0x01}) c.push_back(with_parity(b));
  c.insert(c.end(), blk.begin(), blk.end());
  const uint16_t k = bcs_of(blk);
  c.push_back((uint8_t)(k & 0xFF)); c.push_back((uint8_t)(k >> 8));
  c.push_back(with_parity(0x7F));
  return c;
}

static std::vector<int> bits_of(const Bytes& c) {
  std::vector<int> b;
  for (uint8_t v : c) for (int i = 0; i < 8; ++i) b.push_back((v >> i) & 1);
  return b;
}

// MSK on an AM carrier at the row's rate, added to y from `at` on; first: the level before the first bit
static void add_station(std::vector<AcC>& y, size_t at, const std::vector<int>& bits, double fs, double off, double amp, double depth, int first) {
  const size_t n = (size_t)floor((double)bits.size() * fs / 2400.0);
  double th = 0;
  for (size_t i = 0; i < n && at + i < y.size(); ++i) {
    const size_t b = (size_t)((double)i * 2400.0 / fs);
    const int prev = b == 0 ? first : bits[b - 1];
    th += 2 * M_PI * (bits[b] == prev ? 2400.0 : 1200.0) / fs;
    const double e = amp * (1.0 + depth * sin(th)), ph = 2 * M_PI * off * (double)i / fs;
    y[at + i].x += (float)(e * cos(ph));
    y[at + i].y += (float)(e * sin(ph));
  }
}

// ---- the plain transcription of DESIGN.md 3 item 32 ----------------------------------------------------------------------------
struct Plain {
  int L; pysdr_acars_cfg c; std::vector<AcC> tw, taps;
  struct D { int32_t clk = 0, xprev = 0, lev = 0, sr = 0, st = 0, byte = 0, nb = 0, nbytes = 0, crc = 0; Bytes fb = Bytes(240, 0); };
  std::vector<D> d;
  static AcC sample(const std::vector<AcC>& y, long n) { return n < 0 ? AcC{0.f, 0.f} : y[(size_t)n]; }
  float power(const std::vector<AcC>& y, long n) const {
    const AcC v = sample(y, n);
    const float p = v.x * v.x + v.y * v.y;
    return !(p <= c.pmax) ? 0.f : p;
  }
  // steps 1 to 3 for the output m of the row whose whole stream is y; the stream's first output has the absolute index m_base
  AcC mixed(const std::vector<AcC>& y, long m, uint32_t m_base) const {
    float br = 0.f, bi = 0.f;
    for (int i = 0; i < 4 * L + 1; ++i) {
      const float p = power(y, m - i);
      if (i == 0) { br = taps[0].x * p; bi = taps[0].y * p; }
      else { br = br + taps[(size_t)i].x * p; bi = bi + taps[(size_t)i].y * p; }
    }
    const AcC t = tw[(uint32_t)((m_base + (uint32_t)m) * c.w_car) >> 22];
    return AcC{br * t.x - bi * t.y, br * t.y + bi * t.x};
  }
  int detect(const std::vector<AcC>& y, long m, uint32_t m_base) const {
    const AcC a = mixed(y, m, m_base), aL = mixed(y, m - L, m_base);
    const float q = a.y * aL.x - a.x * aL.y;
    return q > 0.f ? 1 : 0;
  }
  void store(D& z, int32_t b) {
    if (z.nbytes < 240) {                                            // a byte that opens a word clears the rest of it
      z.fb[(size_t)z.nbytes] = (uint8_t)b;
      if (z.nbytes % 4 == 0) for (int q = 1; q < 4; ++q) z.fb[(size_t)z.nbytes + q] = 0;
    }
    for (int k = 0; k < 8; ++k) { z.crc = (z.crc >> 1) ^ (((z.crc ^ b) & 1) ? 0x8408 : 0); b >>= 1; }
    z.nbytes += 1;
  }
  // steps 5 to 8; words: the decoder's events of this call
  void step(int dec, int x, int i, std::vector<int32_t>& words) {
    D& z = d[(size_t)dec];
    const int32_t prev = z.clk;
    z.clk = (int32_t)((uint32_t)z.clk + c.w_baud);
    if (x != z.xprev) z.clk -= z.clk >> c.pll_shift;
    z.xprev = x;
    if (!(prev >= 0 && z.clk < 0)) return;
    z.lev ^= 1 - x;
    const int bit = z.lev;
    z.sr = (z.sr >> 1) | (bit << 15);
    if (z.st == 0) {
      if (z.sr == 0x1616) { z.st = 1; z.nb = z.byte = 0; }
      else if (z.sr == 0xE9E9) { z.lev ^= 1; z.st = 1; z.nb = z.byte = 0; }
      return;
    }
    z.byte |= bit << z.nb;
    z.nb += 1;
    if (z.nb < 8) return;
    const int32_t b = z.byte;
    z.nb = z.byte = 0;
    switch (z.st) {
      case 1:
        if (b == 0x01) { z.st = 2; z.crc = 0; z.nbytes = 0; } else z.st = 0;
        break;
      case 2:
        if (!__builtin_parity((unsigned)b)) { z.st = 0; break; }
        store(z, b);
        if ((b & 0x7F) == 0x03 || (b & 0x7F) == 0x17) z.st = 3;
        else if (z.nbytes >= 238) z.st = 0;
        break;
      case 3:
        store(z, b);
        z.st = 4;
        break;
      default: {
        store(z, b);
        const int n = z.nbytes - 2;
        if (z.crc == 0 && n >= 13) {
          words.push_back((int32_t)(((uint32_t)i << 10) | (uint32_t)n));
          for (int k = 0; k < n; k += 4) {
            uint32_t v = 0;
            for (int q = 0; q < 4 && k + q < n; ++q) v |= (uint32_t)z.fb[(size_t)(k + q)] << (8 * q);
            words.push_back((int32_t)v);
          }
        }
        z.st = 0;
      }
    }
  }
};

// ---- the kernel's phases, as acars.hip runs them, on heap arrays of exactly their size -------------------------------------------
struct Device {
  int nk, L; AcPlan p; pysdr_acars_cfg c;
  std::vector<AcC> Y, tw, taps; std::vector<int32_t> si, events, counts; std::vector<uint32_t> frames;
  std::vector<int> last_x;                                         // [nk][n_out] of the last call, for the comparison
  void init() {
    Y.assign((size_t)nk * p.ypitch, AcC{0.f, 0.f});
    si.assign((size_t)kAcStateInts * nk, 0);
    frames.assign((size_t)nk * kAcFrameWords, 0u);
    events.assign((size_t)nk * p.cap, 0);
    counts.assign((size_t)nk, 0);
  }
  void call(int n_out, uint32_t m0) {
    using G = AcGeom;
    constexpr int ROWS = G::kRows;
    last_x.assign((size_t)nk * n_out, -1);
    AcC* y = Y.data() + kAcHpad;
    const size_t nd = (size_t)nk;
    const int NT = G::taps(L);
    for (int grp = 0; grp < p.groups; ++grp) {
      const int row0 = grp * ROWS;
      std::vector<AcC> s_tw(tw), s_c(taps), s_a((size_t)ROWS * G::kAp);
      std::vector<float> s_p((size_t)ROWS * G::kPp);
      std::vector<int> s_x((size_t)ROWS * G::kXp);
      std::vector<AcDec> z((size_t)ROWS);
      std::vector<int> cnt((size_t)ROWS, 0);
      for (int r = 0; r < ROWS; ++r) {
        z[(size_t)r] = acars_dec_init();
        if (row0 + r >= nk) continue;
        const size_t dec = (size_t)(row0 + r);
        AcDec& q = z[(size_t)r];
        q.clk = si[dec]; q.xprev = si[nd + dec]; q.lev = si[2 * nd + dec]; q.sr = si[3 * nd + dec]; q.st = si[4 * nd + dec];
        q.byte = si[5 * nd + dec]; q.nb = si[6 * nd + dec]; q.nbytes = si[7 * nd + dec]; q.crc = si[8 * nd + dec];
        acars_word_load(q, frames.data() + dec * kAcFrameWords);
      }
      for (int i0 = 0; i0 < n_out; i0 += kAcTile) {
        for (int k = 0; k < G::stage_n(L); ++k) {
          const int rr = G::stage_row(k, L), c2 = G::stage_col(k, L), i = i0 + G::stage_rel(c2, L);
          AcC v{0.f, 0.f};
          if (row0 + rr < nk && i < n_out) v = y[(long long)(row0 + rr) * p.ypitch + i];
          s_p.at((size_t)G::p_at(rr, c2)) = acars_power(v, c.pmax);
        }
        for (int k = 0; k < G::mix_n(L); ++k) {
          const int rr = G::mix_row(k, L), c2 = G::mix_col(k, L);
          const uint32_t m = m0 + (uint32_t)(i0 + G::mix_rel(c2, L));
          s_a.at((size_t)G::a_at(rr, c2)) = acars_mix(s_p.data() + G::win(rr, c2, L), s_c.data(), NT, m, c.w_car, s_tw.data());
        }
        for (int k = 0; k < ROWS * kAcTile; ++k) {
          const int rr = G::det_row(k), jj = G::det_col(k);
          s_x.at((size_t)G::x_at(rr, jj)) = acars_detect(s_a.at((size_t)G::a_at(rr, jj + L)), s_a.at((size_t)G::a_at(rr, jj)));
        }
        const int nj = n_out - i0 < kAcTile ? n_out - i0 : kAcTile;
        for (int r = 0; r < ROWS; ++r) {
          if (row0 + r >= nk) continue;
          const size_t dec = (size_t)(row0 + r);
          for (int jj = 0; jj < nj; ++jj) {
            const int x = s_x.at((size_t)G::x_at(r, jj));
            last_x[dec * n_out + (size_t)(i0 + jj)] = x;
            if (acars_clock(z[(size_t)r], x, c.w_baud, c.pll_shift))
              acars_sample(z[(size_t)r], x, i0 + jj, frames.data() + dec * kAcFrameWords, events.data() + dec * p.cap, cnt[(size_t)r], p.cap);
          }
        }
      }
      std::vector<AcC> keep((size_t)G::roll_n(L));
      for (int k = 0; k < G::roll_n(L); ++k)
        if (row0 + G::roll_row(k, L) < nk) keep[(size_t)k] = y[(long long)(row0 + G::roll_row(k, L)) * p.ypitch + G::roll_src(n_out, G::roll_col(k, L), L)];
      for (int k = 0; k < G::roll_n(L); ++k)
        if (row0 + G::roll_row(k, L) < nk) y[(long long)(row0 + G::roll_row(k, L)) * p.ypitch + G::roll_dst(G::roll_col(k, L), L)] = keep[(size_t)k];
      for (int r = 0; r < ROWS; ++r) {
        if (row0 + r >= nk) continue;
        const size_t dec = (size_t)(row0 + r);
        const AcDec& q = z[(size_t)r];
        acars_word_flush(q, frames.data() + dec * kAcFrameWords);
        si[dec] = q.clk; si[nd + dec] = q.xprev; si[2 * nd + dec] = q.lev; si[3 * nd + dec] = q.sr; si[4 * nd + dec] = q.st;
        si[5 * nd + dec] = q.byte; si[6 * nd + dec] = q.nb; si[7 * nd + dec] = q.nbytes; si[8 * nd + dec] = q.crc;
        counts[dec] = cnt[(size_t)r];
      }
    }
  }
};

static long phases(double fs_out, int nk, int max_out, uint32_t m_base) {
  const int L = (int)floor(fs_out / 2400.0 + 0.5), NT = 4 * L + 1;
  Device dv;
  dv.nk = nk; dv.L = L; dv.c = good_cfg(fs_out);
  REQUIRE(acars_plan(nk, L, max_out, &dv.c, &dv.p), "plan");
  dv.tw.resize(kAcNt);
  for (int k = 0; k < kAcNt; ++k) dv.tw[(size_t)k] = AcC{(float)cos(2 * M_PI * k / kAcNt), (float)-sin(2 * M_PI * k / kAcNt)};
  // the taps: a Hamming low-pass of 1500 Hz at +1800 Hz, mean subtracted (the steps do not ask which window it was)
  std::vector<double> cr((size_t)NT), ci((size_t)NT);
  double sum = 0, mr = 0, mi = 0;
  std::vector<double> h((size_t)NT);
  for (int i = 0; i < NT; ++i) {
    const double t = i - 2 * L, fc = 2 * 1500.0 / fs_out;
    h[(size_t)i] = (t == 0 ? fc : sin(M_PI * fc * t) / (M_PI * t)) * (0.54 - 0.46 * cos(2 * M_PI * i / (NT - 1)));
    sum += h[(size_t)i];
  }
  for (int i = 0; i < NT; ++i) { cr[(size_t)i] = h[(size_t)i] / sum * cos(2 * M_PI * 1800.0 * (i - 2 * L) / fs_out); ci[(size_t)i] = h[(size_t)i] / sum * sin(2 * M_PI * 1800.0 * (i - 2 * L) / fs_out); mr += cr[(size_t)i] / NT; mi += ci[(size_t)i] / NT; }
  dv.taps.resize((size_t)NT);
  for (int i = 0; i < NT; ++i) dv.taps[(size_t)i] = AcC{(float)(cr[(size_t)i] - mr), (float)(ci[(size_t)i] - mi)};
  dv.init();
  // the rows: a station on some (every third inverted), noise on all; three samples that must be blanked
  std::vector<Bytes> sent;
  const size_t n = (size_t)(0.45 * fs_out);
  std::vector<std::vector<AcC>> rows((size_t)nk, std::vector<AcC>(n));
  for (int a = 0; a < nk; ++a) {
    for (AcC& v : rows[(size_t)a]) v = AcC{0.002f * rndf(), 0.002f * rndf()};
    if (a % 3 == 2) continue;                                        // noise alone
    const Bytes blk = make_block(a == 0 ? 13 : 20 + (a * 17) % 50, a, a % 2 == 1);
    sent.push_back(blk);
    add_station(rows[(size_t)a], (size_t)(40 + 13 * a), bits_of(chars_of(blk, 10)), fs_out, (a % 2 ? 700.0 : -300.0), 0.1, a % 4 ? 0.8 : 0.5, a % 3 == 1 ? 0 : 1);
  }
  const long bads[3] = {(long)n - 900, (long)n - 700, (long)n - 500};
  rows[0][(size_t)bads[0]] = AcC{NAN, 0.1f}; rows[0][(size_t)bads[1]] = AcC{0.1f, INFINITY}; rows[0][(size_t)bads[2]] = AcC{1e15f, 1e15f};
  rows[0][n - 300] = AcC{100.f, 100.f};                              // large, below pmax: not blanked
  Plain pl;
  pl.L = L; pl.c = dv.c; pl.tw = dv.tw; pl.taps = dv.taps; pl.d.resize((size_t)nk);
  Plain clean = pl;                                                  // the same row with the three samples at zero power: what blanking means
  std::vector<AcC> row0_clean = rows[0];
  for (long b : bads) row0_clean[(size_t)b] = AcC{0.f, 0.f};
  const int tile = kAcTile;
  std::vector<int> cuts = {1, 1, tile - 1, tile, tile + 1, 2, 3 * tile + 5};
  for (int& v : cuts) if (v > max_out) v = max_out;
  std::vector<Bytes> got;
  long at = 0, words_total = 0, in_windows = 0;
  size_t ci2 = 0;
  while (at < (long)n) {
    int n_out = ci2 < cuts.size() ? cuts[ci2++] : max_out;
    if (n_out > (long)n - at) n_out = (int)((long)n - at);
    for (int a = 0; a < nk; ++a) memcpy(dv.Y.data() + (size_t)a * dv.p.ypitch + kAcHpad, rows[(size_t)a].data() + at, (size_t)n_out * sizeof(AcC));
    dv.call(n_out, m_base + (uint32_t)at);
    for (int a = 0; a < nk; ++a) {
      std::vector<int32_t> w;
      for (int j = 0; j < n_out; ++j) {
        const int want = pl.detect(rows[(size_t)a], at + j, m_base);
        REQUIRE(dv.last_x[(size_t)a * n_out + j] == want, "fs_out %g row %d output %ld: bit %d, expected %d", fs_out, a, at + j, dv.last_x[(size_t)a * n_out + j], want);
        if (a == 0) {                                                // the blanked samples are zero powers, and reach NT + L outputs each
          bool touched = false;
          for (long bad : bads) touched = touched || (at + j >= bad && at + j < bad + NT + L);
          in_windows += touched;
          REQUIRE(want == clean.detect(row0_clean, at + j, m_base), "output %ld: blanking is not a zero power", at + j);
        }
        pl.step(a, want, j, w);
      }
      const size_t dec = (size_t)a, nd = (size_t)nk;
      REQUIRE(dv.counts[dec] == (int)w.size() && (int)w.size() <= dv.p.cap, "decoder %zu: %d words, expected %zu", dec, dv.counts[dec], w.size());
      for (size_t k = 0; k < w.size(); ++k) REQUIRE(dv.events[dec * dv.p.cap + k] == w[k], "decoder %zu word %zu", dec, k);
      words_total += (long)w.size();
      for (size_t k = 0; k < w.size();) {
        const int nb = acars_header_bytes(w[k]);
        REQUIRE(acars_header_index(w[k]) < n_out && nb >= 13 && nb <= 238, "header");
        Bytes f;
        for (int q = 0; q < nb; ++q) f.push_back((uint8_t)((uint32_t)w[k + 1 + (size_t)q / 4] >> (8 * (q % 4))));
        got.push_back(f);
        k += (size_t)acars_event_words(nb);
      }
      const Plain::D& z = pl.d[dec];
      const int32_t want_s[9] = {z.clk, z.xprev, z.lev, z.sr, z.st, z.byte, z.nb, z.nbytes, z.crc};
      for (int f = 0; f < 9; ++f) REQUIRE(dv.si[(size_t)f * nd + dec] == want_s[f], "decoder %zu field %d after output %ld: %d, expected %d", dec, f, at + n_out, dv.si[(size_t)f * nd + dec], want_s[f]);
      for (int k = 0; k < kAcFrameWords; ++k) {
        uint32_t v = 0;
        for (int q = 0; q < 4; ++q) v |= (uint32_t)z.fb[(size_t)(4 * k + q)] << (8 * q);
        REQUIRE(dv.frames[dec * kAcFrameWords + (size_t)k] == v, "decoder %zu frame word %d after output %ld", dec, k, at + n_out);
      }
    }
    at += n_out;
  }
  REQUIRE(in_windows == 3 * (NT + L), "the windows hold %ld outputs", in_windows);
  REQUIRE(got.size() == sent.size(), "%zu blocks read, %zu sent", got.size(), sent.size());
  for (const Bytes& f : sent) {
    int copies = 0;
    for (const Bytes& q : got) copies += q == f;
    REQUIRE(copies == 1, "a block of %zu bytes was read %d times", f.size(), copies);
  }
  return words_total;
}

// ---- the cap ----------------------------------------------------------------------------------------------------------------
static long clock_gaps() {
  long samplings = 0;
  const double rates[] = {19200, 20000, 22050, 24000, 25000, 44100, 48000, 50000};
  for (double fs : rates)
    for (int sh = 1; sh <= 4; ++sh)
      for (int mode = 0; mode < 6; ++mode) {
        const uint32_t w = word_of(2400, fs);
        const int gap = acars_sample_gap(w);
        REQUIRE((long long)gap * w > (1ll << 31) && (long long)(gap - 1) * w <= (1ll << 31), "gap");
        AcDec z = acars_dec_init();
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
          if (acars_clock(z, x, w, sh)) {
            REQUIRE(m - last >= gap, "fs %g shift %d mode %d: samplings %ld outputs apart, gap %d", fs, sh, mode, m - last, gap);
            last = m;
            ++samplings;
          }
        }
      }
  return samplings;
}

static long densest() {
  for (int n = 13; n <= 238; ++n)
    REQUIRE(acars_event_words(n) * kAcSamplingsPerWord <= 8 * n + 24 && acars_event_words(n) <= kAcFrameWords + 1, "a block of %d bytes: %d words for %d samplings", n, acars_event_words(n), 8 * n + 24);
  REQUIRE(acars_event_words(238) == kAcCarriedWords, "the carried block");
  // A 238-byte block, then blocks of 13 bytes (5 words per 129 samplings: the densest) each found for a block check of
  // 0x2C2C or 0x2C2D, whose upper 15 bits and one 0 behind them are SYN SYN, so that the next SOH follows after one bit.
  // The decoder is driven with x = 1 - (bit ^ lev), which makes lev the bit.
  std::vector<Bytes> blocks;
  blocks.push_back(make_block(238, 3));
  int made = 0;
  for (int salt = 0; made < 30 && salt < 8000000; ++salt) {
    Bytes f = make_block(13, salt & 63);
    f[1] = with_parity((uint8_t)(0x20 + (salt >> 6) % 0x5F)); f[2] = with_parity((uint8_t)(0x20 + (salt >> 6) / 0x5F % 0x5F)); f[3] = with_parity((uint8_t)(0x20 + (salt >> 6) / (0x5F * 0x5F) % 0x5F));
    if ((bcs_of(f) | 1) == 0x2C2D) { blocks.push_back(f); ++made; }
  }
  REQUIRE(made == 30, "only %d blocks whose check is the sync word one bit early", made);
  std::vector<int> bits = bits_of(Bytes{0x16, 0x16});
  for (const Bytes& f : blocks) {
    Bytes c{0x01};
    c.insert(c.end(), f.begin(), f.end());
    const uint16_t v = bcs_of(f);
    c.push_back((uint8_t)(v & 0xFF)); c.push_back((uint8_t)(v >> 8));
    if ((v | 1) != 0x2C2D) { c.push_back(0x16); c.push_back(0x16); }
    const std::vector<int> b = bits_of(c);
    bits.insert(bits.end(), b.begin(), b.end());
    if ((v | 1) == 0x2C2D) bits.push_back(0);
  }
  long checked = 0;
  const uint32_t ws[] = {word_of(2400, 25000), 1u << 29, word_of(2400, 50000)};
  for (uint32_t w : ws) {
    const int gap = acars_sample_gap(w);
    const int mos[] = {1, 16, gap, 24 * gap, 24 * gap + 1, 128 * gap, 129 * gap, 1000};
    for (int mo : mos) {
      const int cap = acars_event_cap(mo, w);
      for (int offset = 0; offset < mo && offset < 400; offset += (mo > 64 ? 7 : 1)) {
        AcDec z = acars_dec_init();
        std::vector<uint32_t> fb(kAcFrameWords, 0u);
        std::vector<int32_t> ev((size_t)cap, 0);
        int cnt = 0, most = 0;
        long out = 0, call_end = offset ? offset : mo;
        long total_words = 0, frames_read = 0;
        for (size_t b = 0; b < bits.size(); ++b) {
          const long m = (long)b * gap;
          while (m >= call_end) {                                    // the call ends: the word in hand goes to memory, the slots start over
            acars_word_flush(z, fb.data());
            most = cnt > most ? cnt : most;
            total_words += cnt;
            cnt = 0;
            out = call_end;
            call_end += mo;
            acars_word_load(z, fb.data());
          }
          const int before = cnt;
          acars_sample(z, 1 - (bits[b] ^ z.lev), (int)(m - out), fb.data(), ev.data(), cnt, cap);
          frames_read += cnt > before;
        }
        total_words += cnt;
        most = cnt > most ? cnt : most;
        REQUIRE(most <= cap, "w %u max_out %d offset %d: %d words, cap %d", w, mo, offset, most, cap);
        REQUIRE(frames_read == (long)blocks.size(), "w %u max_out %d offset %d: %ld of %zu blocks (a block dropped at the cap?)", w, mo, offset, frames_read, blocks.size());
        long want = 0;
        for (const Bytes& f : blocks) want += acars_event_words((int)f.size());
        REQUIRE(total_words == want, "words");
        ++checked;
      }
    }
  }
  return checked;
}

// the frame machine alone: polarity, parity, the length limit, ETB, a failed SOH
static void machine() {
  // the tones of the characters (x = 1: this bit equals the one before) into a decoder whose level starts at `lev0`; the
  // sender's starts at 0, so lev0 = 1 makes the decoder's bits come out inverted until the sync word sets them right
  auto run = [](const Bytes& chars, bool invert, std::vector<int32_t>& ev_out) {
    AcDec z = acars_dec_init();
    z.lev = invert ? 1 : 0;
    std::vector<uint32_t> fb(kAcFrameWords, 0u);
    std::vector<int32_t> ev(128, 0);
    int cnt = 0, sent = 0;
    const std::vector<int> bits = bits_of(chars);
    for (size_t b = 0; b < bits.size(); ++b) {
      acars_sample(z, 1 - (bits[b] ^ sent), (int)b, fb.data(), ev.data(), cnt, 128);
      sent = bits[b];
    }
    ev_out.assign(ev.begin(), ev.begin() + cnt);
    return z;
  };
  std::vector<int32_t> ev;
  const Bytes blk = make_block(40, 5), etb = make_block(17, 6, true);
  run(chars_of(blk, 4), false, ev);
  REQUIRE((int)ev.size() == acars_event_words(40) && acars_header_bytes(ev[0]) == 40, "a block is read");
  run(chars_of(etb, 4), false, ev);
  REQUIRE((int)ev.size() == acars_event_words(17) && (((uint32_t)ev[1 + 16 / 4]) & 0x7F) == 0x17, "ETB ends a block too");
  run(chars_of(blk, 4), true, ev);
  REQUIRE((int)ev.size() == acars_event_words(40), "an inverted start is set right by the sync word");
  for (size_t at = 0; at < blk.size() + 2; ++at)
    for (int bit = 0; bit < 8; ++bit) {                              // one flipped bit anywhere in the block or its check
      Bytes c = chars_of(blk, 2);
      c[2 + 5 + at] ^= (uint8_t)(1u << bit);
      run(c, false, ev);
      REQUIRE(ev.empty(), "a block with byte %zu bit %d flipped was read", at, bit);
    }
  { Bytes c = chars_of(blk, 2); c[2 + 4] = with_parity(0x02); run(c, false, ev); REQUIRE(ev.empty(), "no SOH, no block"); }
  { // 238 bytes are read, 239 are not
    run(chars_of(make_block(238, 9), 2), false, ev);
    REQUIRE(!ev.empty() && acars_header_bytes(ev[0]) == 238, "238 bytes");
    const AcDec z = run(chars_of(make_block(239, 9), 2), false, ev);
    REQUIRE(ev.empty() && z.nbytes <= kAcFrameBytes, "239 bytes");
    run(chars_of(make_block(12, 9), 2), false, ev);
    REQUIRE(ev.empty(), "12 bytes");
  }
}

static void words() {
  const int is[] = {0, 1, 63, 64, 1023, 4095, (1 << 20) - 1}, ns[] = {13, 14, 16, 17, 237, 238};
  for (int i : is) for (int n : ns) {
    const int32_t w = acars_header(i, n);
    REQUIRE(acars_header_index(w) == i && acars_header_bytes(w) == n && w >= 0, "header (%d, %d)", i, n);
  }
  REQUIRE(acars_event_words(13) == 5 && acars_event_words(16) == 5 && acars_event_words(17) == 6 && acars_event_words(238) == 61, "words");
}

int main() {
  rules();
  long steps = 0;
  for (int L : {8, 10, 16, 20, 21})
    for (int nk : {1, 7, 8, 9, 17})
      for (int n_out : {1, 2, 39, 63, 64, 65, 128, 129, 300}) {
        AcPlan p;
        const pysdr_acars_cfg c = good_cfg(2400.0 * L);
        REQUIRE(acars_plan(nk, L, n_out, &c, &p), "plan");
        steps += walk(nk, n_out, L, p);
      }
  long w = 0;
  w += phases(25000.0, 9, 256, 0u);
  w += phases(19200.0, 3, 16, 0xFFFFF000u);                         // the absolute index wraps inside the run
  w += phases(50000.0, 2, 256, 123456789u);
  w += phases(48000.0, 1, 256, 77u);
  const long s = clock_gaps(), d = densest();
  machine();
  words();
  printf("ACARS_PLAN_OK walk steps %ld, event words %ld, samplings %ld, cap cases %ld\n", steps, w, s, d);
  return 0;
}
