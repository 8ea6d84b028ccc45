// The SSTV skimmer's pure half: settings and their rules, the mode table's checks, the workgroup's
// geometry, LDS budget and the index arithmetic of its tile walk, the event words, the event cap with its proof, and the
// decoder's steps themselves -- mixer, low-pass, lag product, frequency of a sum, tick, VIS match, anchor and pixel -- the
// very code the kernel (sstv.hip) steps with, the host half (api_sstv.hip) plans with and tests/sstv_plan/plan_main.cpp
// runs on the CPU.  Plain C++: nothing here calls the HIP runtime, and the only traces of the device are the function
// qualifier and the division below.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/pysdr_hip.h"

#if defined(__HIPCC__)
#define PYSDR_SSTV_HD __host__ __device__
#else
#define PYSDR_SSTV_HD
#endif

namespace pysdr {

constexpr int kSstvTile = 64;                 // outputs of every row worked on at once
constexpr int kSstvLmin = 9, kSstvLmax = 96;  // L, the low-pass in row samples
constexpr int kSstvR0Max = 480, kSstvWMax = 96;                        // at fs_out = 48000
constexpr int kSstvQMax = 2 * kSstvR0Max + 2 * kSstvWMax;              // hard decisions an anchor looks at
constexpr int kSstvHpad = 1280;               // complex samples kept in front of a row of Y: the history's room
constexpr int kSstvRowsMax = 1 << 15;
constexpr int kSstvMaxOutMax = 1 << 20;       // the header word holds the index within the call above bit 12
constexpr long long kSstvSlotsMax = 1ll << 28;                         // event words of all rows
constexpr float kSstvPmaxMax = 1.0e18f;
constexpr int kSstvNt = 1024;                 // twiddle table: one turn, indexed by a phase word's top ten bits
constexpr int kSstvRing = 64;                 // tick frequencies kept per row
constexpr int kSstvModesMax = 16, kSstvWidthMax = 800, kSstvScansMax = 4, kSstvLinesMax = 4096;
constexpr int kSstvLineWords = kSstvScansMax * kSstvWidthMax / 4;      // a row's line buffer
constexpr int kSstvStateInts = 7;             // ticks, phase, mode, m_a, e0, line, pix
constexpr int kSstvStateFloats = 7;           // acc (2), bprev (2), f_lead, pacc (2)
constexpr float kSstvTol = 40.f, kSstvLeadMax = 150.f;                 // Hz
constexpr float kSstvA0 = 0.9998660f, kSstvA1 = -0.3302995f, kSstvA2 = 0.1801410f, kSstvA3 = -0.0851330f, kSstvA4 = 0.0208351f;
constexpr float kSstvPixScale = 255.f / 800.f;
enum { kSstvIdle = 0, kSstvWait = 1, kSstvPicture = 2 };               // a row's phase
enum { kSstvEvStart = 1, kSstvEvLine = 2, kSstvEvEnd = 3 };            // event kinds

static_assert(kSstvQMax + kSstvLmax + 1 <= kSstvHpad, "the history fits its room");

// ---- the mode table ------------------------------------------------------------------------------------------------------
PYSDR_SSTV_HD inline unsigned long long sstv_line_q(const pysdr_sstv_mode& m) {
  return (unsigned long long)m.sync_q + m.porch_q + (unsigned long long)m.scans * ((unsigned long long)m.scan_q + m.sep_q);
}
PYSDR_SSTV_HD inline int sstv_line_bytes(const pysdr_sstv_mode& m) { return m.scans * m.width; }
PYSDR_SSTV_HD inline int sstv_line_words(const pysdr_sstv_mode& m) { return (m.scans * m.width + 3) / 4; }
// Least outputs between the ends of two lines of this mode, in one picture or in two: see the cap below.
inline long long sstv_line_gap(const pysdr_sstv_mode& m) { return (long long)((sstv_line_q(m) - m.sep_q) >> 16) - 2; }

inline bool sstv_mode_ok(const pysdr_sstv_mode& m) {
  if (m.code < 0 || m.code > 127 || m.scans < 1 || m.scans > kSstvScansMax || m.width < 1 || m.width > kSstvWidthMax) return false;
  if (m.lines < 1 || m.lines > kSstvLinesMax) return false;
  if ((unsigned long long)m.scan_q < (unsigned long long)m.width << 16) return false;   // a pixel of at least one sample
  if (sstv_line_q(m) >= (1ull << 32)) return false;
  return sstv_line_gap(m) >= 1;
}

inline bool sstv_cfg_ok(const pysdr_sstv_cfg& c) {
  if (c.det != 0 && c.det != 1) return false;
  if (!(c.pmax > 0.f && c.pmax <= kSstvPmaxMax)) return false;
  if (c.R0 < 80 || c.R0 > kSstvR0Max || c.W < 1 || c.W > kSstvWMax) return false;       // fs_out from 8000 to 48000
  const long long turn = (long long)c.R0 * (long long)c.w_tick - (1ll << 32);           // R0 samples are one tick
  if (c.w_tick == 0 || turn > (long long)c.w_tick || -turn > (long long)c.w_tick) return false;
  if (5 * c.W - c.R0 > 3 || c.R0 - 5 * c.W > 3) return false;                           // W = R0 / 5
  if (c.lag != 2 * c.R0 + c.W + 1) return false;
  if (!(std::fabs(c.k_hz * 0.06283185307f - (float)c.R0) <= 1.f)) return false;         // k_hz = fs_out / 2 pi
  if (!(std::fabs(c.k_rho * (float)c.R0 - 10.24f) <= 0.16f)) return false;              // k_rho = 1024 / fs_out
  if (c.nmodes < 1 || c.nmodes > kSstvModesMax) return false;
  for (int i = 0; i < c.nmodes; ++i) {
    if (!sstv_mode_ok(c.modes[i])) return false;
    for (int j = 0; j < i; ++j)
      if (c.modes[j].code == c.modes[i].code) return false;
  }
  return true;
}

// ---- the event words ----------------------------------------------------------------------------------------------------
// header = (index within the call of the output that completed the event) << 12 | kind << 10 | payload words
PYSDR_SSTV_HD constexpr int32_t sstv_header(int i, int kind, int nw) { return (int32_t)(((uint32_t)i << 12) | ((uint32_t)kind << 10) | (uint32_t)nw); }
PYSDR_SSTV_HD constexpr int sstv_header_index(int32_t w) { return (int)((uint32_t)w >> 12); }
PYSDR_SSTV_HD constexpr int sstv_header_kind(int32_t w) { return (int)(((uint32_t)w >> 10) & 3u); }
PYSDR_SSTV_HD constexpr int sstv_header_words(int32_t w) { return (int)((uint32_t)w & 1023u); }
constexpr int kSstvStartWords = 5, kSstvEndWords = 2;                  // header + mode, code, f_lead, e0; header + lines

// ---- the event cap: words one row can emit in a call of max_out outputs -----------------------------------------------------
// A line's event leaves with the output that completes the line's last pixel.  Within a picture the last pixels of lines
// l and l + 1 are floor((l + 1) X / 2^16) - floor(l X / 2^16) >= floor(X / 2^16) samples apart, X the mode's line in Q16.
// Between pictures: the row is idle from the output m_end of the last line's event; the next VIS tick m_v comes later, the
// new e0 is at least m_v + 1 + sync - R0, and the new line 0 ends lag + floor((X - sync_q - sep_q) / 2^16) - 1 outputs
// behind e0, which is more than floor((X - sep_q) / 2^16) - 2 behind m_v since lag > R0.  So two line events of a row are
// never closer than gap = the least sstv_line_gap of the table, and a call of n outputs holds at most NL = ceil(n / gap) of
// them, each of at most 2 + the widest line's words.  An end event (2 words) leaves with a last line; a start event (5
// words) is followed by a line event of its picture before the next start, so there are at most NL + 1 of them.
inline long long sstv_event_cap(int max_out, const pysdr_sstv_cfg& c) {
  long long gap = 1ll << 40;
  int nw = 0;
  for (int i = 0; i < c.nmodes; ++i) {
    const long long g = sstv_line_gap(c.modes[i]);
    if (g < gap) gap = g;
    if (sstv_line_words(c.modes[i]) > nw) nw = sstv_line_words(c.modes[i]);
  }
  const long long NL = ((long long)max_out + gap - 1) / gap;
  return NL * (2 + nw + kSstvEndWords + kSstvStartWords) + kSstvStartWords;
}

// ---- the workgroup ----------------------------------------------------------------------------------------------------------
// Whole rows: 8 of them, each seen twice per tile -- the tile's outputs themselves (ticks, VIS, anchor) and the outputs
// `lag` earlier (pixels): 16 pseudo-rows of 64 lag products.  All 256 threads mix, filter and multiply; thread r < 8 then
// walks row r's tile in order.
struct SstvGeom {
  static constexpr int kRows = 8;
  static constexpr int kPseudo = 2 * kRows;
  static constexpr int kThreads = 256;
  static constexpr int kVp = kSstvLmax + kSstvTile + 1;             // LDS pitch of the products v: L + tile are used
  static constexpr int kUp = kSstvTile + 1;                         // of the filtered u: the output in front of the tile, then the tile
  static constexpr int kCp = kSstvTile;                             // of the lag products c
  // tw, g, v, u, c, q, the settings
  static constexpr int kLdsBytes = kSstvNt * 8 + kSstvLmax * 4 + kPseudo * kVp * 8 + kPseudo * kUp * 8 + kPseudo * kCp * 8 + kRows * kSstvQMax +
                                   (int)sizeof(pysdr_sstv_cfg);
  // pseudo-row pr = which * kRows + r; its first sample, as an index within the call
  PYSDR_SSTV_HD static constexpr int base(int i0, int pr, int lag) { return i0 - (pr / kRows) * lag; }
  PYSDR_SSTV_HD static constexpr int row(int pr) { return pr % kRows; }
  // products: k < kPseudo (L + tile); column cc holds sample base - L + cc
  PYSDR_SSTV_HD static constexpr int mix_n(int L) { return kPseudo * (L + kSstvTile); }
  PYSDR_SSTV_HD static constexpr int mix_pr(int k, int L) { return k / (L + kSstvTile); }
  PYSDR_SSTV_HD static constexpr int mix_col(int k, int L) { return k % (L + kSstvTile); }
  PYSDR_SSTV_HD static constexpr int mix_rel(int cc, int L) { return cc - L; }                    // from base
  PYSDR_SSTV_HD static constexpr int v_at(int pr, int cc) { return pr * kVp + cc; }
  // filtered: k < kPseudo (tile + 1); column kk holds sample base - 1 + kk, whose newest product is column L - 1 + kk
  PYSDR_SSTV_HD static constexpr int fir_n() { return kPseudo * kUp; }
  PYSDR_SSTV_HD static constexpr int fir_pr(int k) { return k / kUp; }
  PYSDR_SSTV_HD static constexpr int fir_col(int k) { return k % kUp; }
  PYSDR_SSTV_HD static constexpr int fir_newest(int pr, int kk, int L) { return pr * kVp + L - 1 + kk; }
  PYSDR_SSTV_HD static constexpr int u_at(int pr, int kk) { return pr * kUp + kk; }
  // lag products: k < kPseudo tile; column jj holds sample base + jj = u columns jj + 1 and jj
  PYSDR_SSTV_HD static constexpr int lag_n() { return kPseudo * kCp; }
  PYSDR_SSTV_HD static constexpr int lag_pr(int k) { return k / kCp; }
  PYSDR_SSTV_HD static constexpr int lag_col(int k) { return k % kCp; }
  PYSDR_SSTV_HD static constexpr int c_at(int pr, int jj) { return pr * kCp + jj; }
  // the history roll: element k < kRows H of the workgroup is column k % H of row k / H; memory offsets from the row's
  // first output of the call
  PYSDR_SSTV_HD static constexpr int roll_row(int k, int H) { return k / H; }
  PYSDR_SSTV_HD static constexpr int roll_src(int k, int H, int n_out) { return n_out - H + k % H; }
  PYSDR_SSTV_HD static constexpr int roll_dst(int k, int H) { return k % H - H; }
};
static_assert(SstvGeom::kLdsBytes <= 64 * 1024 && sizeof(pysdr_sstv_cfg) % sizeof(uint32_t) == 0, "static LDS");

struct SstvPlan {
  int L = 0;
  int H = 0;           // samples of history in front of a row: 2 R0 + 2 W + L + 1
  int cap = 0;         // event words per row
  int groups = 0;      // workgroups
  int ypitch = 0;      // row pitch of Y, complex samples: kSstvHpad of history room, then the call's outputs
};

inline bool sstv_plan(int nk, int L, int max_out, const pysdr_sstv_cfg* cfg, SstvPlan* p) {
  if (L < kSstvLmin || L > kSstvLmax || nk < 1 || nk > kSstvRowsMax || max_out < 1 || max_out > kSstvMaxOutMax || !cfg || !sstv_cfg_ok(*cfg))
    return false;
  const long long cap = sstv_event_cap(max_out, *cfg);
  if (cap * nk > kSstvSlotsMax) return false;
  SstvPlan q;
  q.L = L;
  q.H = 2 * cfg->R0 + 2 * cfg->W + L + 1;
  q.cap = (int)cap;
  q.groups = (nk + SstvGeom::kRows - 1) / SstvGeom::kRows;
  q.ypitch = kSstvHpad + ((max_out + 15) & ~15);
  *p = q;
  return true;
}

struct alignas(8) SstvC { float x, y; };   // a complex sample as the channelizer stores it

// ---- steps 1 and 2 ----------------------------------------------------------------------------------------------------------
// Every float operation rounds on its own (-ffp-contract=off).
// The mixer for the row sample of absolute index n (its low 32 bits): s from the sample (and, FM, the one before it),
// times the table entry.
PYSDR_SSTV_HD inline SstvC sstv_mix(SstvC y, SstvC y1, uint32_t n, int det, uint32_t w_sub, const SstvC* tw) {
  const SstvC t = tw[(uint32_t)(n * w_sub) >> 22];
  if (det == 0) {
    const float d = y.y * y1.x - y.x * y1.y;
    return SstvC{d * t.x, d * t.y};
  }
  return SstvC{y.x * t.x - y.y * t.y, y.x * t.y + y.y * t.x};
}

// u for the sample whose product is vw[0] (vw[-i] = v[m - i]): sum g[i] v[m - i], i ascending, the first term assigned
PYSDR_SSTV_HD inline SstvC sstv_fir(const SstvC* vw, const float* g, int L) {
  float ur = 0.f, ui = 0.f;
#pragma unroll 8
  for (int i = 0; i < L; ++i) {                            // (unrolled so that the reads run ahead of the chain of adds)
    const SstvC v = vw[-i];
    const float gi = g[i];
    if (i == 0) { ur = gi * v.x; ui = gi * v.y; }
    else { ur = ur + gi * v.x; ui = ui + gi * v.y; }
  }
  return SstvC{ur, ui};
}

// c = u conj(u1), 0 where either power is not <= pmax
PYSDR_SSTV_HD inline SstvC sstv_lag(SstvC u, SstvC u1, float pmax) {
  const float p = u.x * u.x + u.y * u.y, p1 = u1.x * u1.x + u1.y * u1.y;
  if (!(p <= pmax) || !(p1 <= pmax)) return SstvC{0.f, 0.f};
  return SstvC{u.x * u1.x + u.y * u1.y, u.y * u1.x - u.x * u1.y};
}

// The same from the row's memory, for the anchor: y points at the sample of absolute index n; y[-L - 1] is read (FM).
PYSDR_SSTV_HD inline SstvC sstv_u_at(const SstvC* y, uint32_t n, int det, uint32_t w_sub, const SstvC* tw, const float* g, int L) {
  float ur = 0.f, ui = 0.f;
  for (int i = 0; i < L; ++i) {
    const SstvC v = sstv_mix(y[-i], y[-i - 1], n - (uint32_t)i, det, w_sub, tw);
    const float gi = g[i];
    if (i == 0) { ur = gi * v.x; ui = gi * v.y; }
    else { ur = ur + gi * v.x; ui = ui + gi * v.y; }
  }
  return SstvC{ur, ui};
}

// ---- step 3: the frequency of a sum of lag products, Hz from the subcarrier --------------------------------------------------
PYSDR_SSTV_HD inline float sstv_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn(a, b);
#else
  return a / b;
#endif
}
PYSDR_SSTV_HD inline float sstv_hz(SstvC P, float k_hz) {
  float t;
  if (P.x > 0.f) {
    t = sstv_div(P.y, P.x);
    t = t < -1.f ? -1.f : (t > 1.f ? 1.f : t);
  } else {
    t = P.y > 0.f ? 1.f : (P.y < 0.f ? -1.f : 0.f);
  }
  const float t2 = t * t;
  float s = t2 * kSstvA4;
  s = kSstvA3 + s; s = t2 * s;
  s = kSstvA2 + s; s = t2 * s;
  s = kSstvA1 + s; s = t2 * s;
  s = kSstvA0 + s;
  const float phi = t * s;
  return phi * k_hz;
}

// ---- a row's state, in registers for the call -------------------------------------------------------------------------------
struct SstvRow {
  uint32_t ticks;        // ticks ended so far
  int32_t phase, mode;
  uint32_t m_a;          // wait: the output at which the anchor is taken (low 32 bits)
  uint32_t e0;           // picture: the anchor
  int32_t line, pix;     // picture: the sent line and the flat pixel scan * width + p being summed
  SstvC acc, bprev;      // the open tick's sum, the last tick's
  float f_lead;
  SstvC pacc;            // the open pixel's sum
  // not state: derived at load
  uint32_t a_lo, a_hi;   // the open pixel's samples a_lo <= n < a_hi
  uint32_t word;         // the line buffer's word being filled
};

PYSDR_SSTV_HD inline SstvRow sstv_row_init() {
  SstvRow z{};
  z.mode = -1;
  return z;
}

// step 7's boundaries: the first sample of pixel p of scan j of line l
PYSDR_SSTV_HD inline uint32_t sstv_pixel_start(const pysdr_sstv_mode& m, uint32_t e0, int l, int j, int p) {
  const unsigned long long off = (unsigned long long)l * sstv_line_q(m) + m.porch_q + (unsigned long long)j * ((unsigned long long)m.scan_q + m.sep_q) +
                                 (unsigned long long)p * m.scan_q / (unsigned long long)m.width;
  return e0 + (uint32_t)(off >> 16);
}
PYSDR_SSTV_HD inline void sstv_pixel_bounds(SstvRow& z, const pysdr_sstv_mode& m) {
  const int j = z.pix / m.width, p = z.pix % m.width;
  z.a_lo = sstv_pixel_start(m, z.e0, z.line, j, p);
  z.a_hi = sstv_pixel_start(m, z.e0, z.line, j, p + 1);
}

// the word being filled, as the last call left it in the row's line buffer lb
PYSDR_SSTV_HD inline bool sstv_word_open(const SstvRow& z) { return z.phase == kSstvPicture && (z.pix & 3) != 0; }
PYSDR_SSTV_HD inline void sstv_row_load(SstvRow& z, const pysdr_sstv_mode* modes, const uint32_t* lb) {
  z.word = sstv_word_open(z) ? lb[z.pix >> 2] : 0u;
  z.a_lo = z.a_hi = 0u;
  if (z.phase == kSstvPicture) sstv_pixel_bounds(z, modes[z.mode]);
}
PYSDR_SSTV_HD inline void sstv_word_flush(const SstvRow& z, uint32_t* lb) {
  if (sstv_word_open(z)) lb[z.pix >> 2] = z.word;
}

// ---- steps 4 and 5 -------------------------------------------------------------------------------------------------------
PYSDR_SSTV_HD inline bool sstv_tick_first(uint32_t m, uint32_t w_tick) { return (uint32_t)(m * w_tick) < w_tick; }
PYSDR_SSTV_HD inline bool sstv_tick_last(uint32_t m, uint32_t w_tick) { return (uint32_t)((m + 1u) * w_tick) < w_tick; }

// The VIS match at tick k (just written to the ring): the mode's index, or -1; *f_lead is set on a match.
PYSDR_SSTV_HD inline int sstv_vis(const float* ring, uint32_t k, const pysdr_sstv_mode* modes, int nmodes, float* f_lead) {
  float lead[4];
  for (int i = 0; i < 4; ++i) lead[i] = ring[(k - (uint32_t)(34 + 6 * i)) & (kSstvRing - 1)];
  float s = lead[0];
  s = s + lead[1]; s = s + lead[2]; s = s + lead[3];
  const float f = s * 0.25f;
  if (!(fabsf(f) <= kSstvLeadMax)) return -1;
  for (int i = 0; i < 4; ++i)
    if (!(fabsf(lead[i] - f) <= kSstvTol)) return -1;
  int code = 0, ones = 0;
  for (int b = 0; b < 10; ++b) {
    const float x = ring[(k - (uint32_t)(3 * b + 1)) & (kSstvRing - 1)] - f;
    if (b == 0 || b == 9) {
      if (!(fabsf(x + 700.f) <= kSstvTol)) return -1;
      continue;
    }
    int bit;
    if (fabsf(x + 800.f) <= kSstvTol) bit = 1;
    else if (fabsf(x + 600.f) <= kSstvTol) bit = 0;
    else return -1;
    ones += bit;
    if (b >= 2) code |= bit << (8 - b);
  }
  if (ones & 1) return -1;
  for (int i = 0; i < nmodes; ++i)
    if (modes[i].code == code) { *f_lead = f; return i; }
  return -1;
}

// Step 4 (and 5 while idle) for the output of absolute index m with lag product c; ring is the row's [kSstvRing].
PYSDR_SSTV_HD inline void sstv_tick(SstvRow& z, SstvC c, uint32_t m, const pysdr_sstv_cfg& cfg, const pysdr_sstv_mode* modes, float* ring) {
  if (sstv_tick_first(m, cfg.w_tick)) z.acc = c;
  else { z.acc.x = z.acc.x + c.x; z.acc.y = z.acc.y + c.y; }
  if (!sstv_tick_last(m, cfg.w_tick)) return;
  const SstvC P{z.acc.x + z.bprev.x, z.acc.y + z.bprev.y};
  z.bprev = z.acc;
  const uint32_t k = z.ticks;
  ring[k & (kSstvRing - 1)] = sstv_hz(P, cfg.k_hz);
  z.ticks = k + 1u;
  if (z.phase != kSstvIdle) return;
  float f = 0.f;
  const int mode = sstv_vis(ring, k, modes, cfg.nmodes, &f);
  if (mode < 0) return;
  z.phase = kSstvWait;
  z.mode = mode;
  z.f_lead = f;
  z.m_a = m + (modes[mode].sync_q >> 16) + (uint32_t)cfg.R0 + (uint32_t)cfg.W;
}

// ---- step 6: the anchor, taken at output m_a = m_v + sync + R0 + W --------------------------------------------------------------
// y points at the row's sample m_a; q [2 R0 + 2 W] is scratch for the hard decisions of the samples m_a - (2 R0 + 2 W) + 1
// .. m_a, the first of which is e_lo - W with e_lo = m_v + 1 + sync - R0.  -> e0 (low 32 bits)
PYSDR_SSTV_HD inline uint32_t sstv_anchor(const SstvC* y, uint32_t m_a, float f_lead, const pysdr_sstv_cfg& cfg, const SstvC* tw, const float* g,
                                          int L, signed char* q) {
  const int R0 = cfg.R0, W = cfg.W, nq = 2 * R0 + 2 * W;
  const SstvC rho = tw[(int)floorf((f_lead - 550.f) * cfg.k_rho + 0.5f) & (kSstvNt - 1)];
  const uint32_t first = m_a - (uint32_t)(nq - 1);
  SstvC u1 = sstv_u_at(y - nq, first - 1u, cfg.det, cfg.w_sub, tw, g, L);
  for (int k = 0; k < nq; ++k) {
    const SstvC u = sstv_u_at(y - (nq - 1) + k, first + (uint32_t)k, cfg.det, cfg.w_sub, tw, g, L);
    const SstvC c = sstv_lag(u, u1, cfg.pmax);
    u1 = u;
    int v = 0;
    if (!(c.x == 0.f && c.y == 0.f)) v = (c.x * rho.y + c.y * rho.x) < 0.f ? 1 : -1;
    q[k] = (signed char)v;
  }
  // D[e_lo + t] over q[t .. t + W) minus q[t + W .. t + 2 W), t = 0 .. 2 R0: the first of the greatest
  int D = 0;
  for (int k = 0; k < W; ++k) D += q[k] - q[W + k];
  int best = D, at = 0;
  for (int t = 1; t <= 2 * R0; ++t) {
    D += 2 * q[t - 1 + W] - q[t - 1] - q[t - 1 + 2 * W];
    if (D > best) { best = D; at = t; }
  }
  return first + (uint32_t)W + (uint32_t)at;
}

// the start event, and the row's first pixel
PYSDR_SSTV_HD inline void sstv_start(SstvRow& z, uint32_t e0, int i, const pysdr_sstv_mode* modes, int32_t* ev, int& cnt, int cap) {
  z.phase = kSstvPicture;
  z.e0 = e0;
  z.line = 0;
  z.pix = 0;
  z.word = 0u;
  z.pacc = SstvC{0.f, 0.f};
  sstv_pixel_bounds(z, modes[z.mode]);
  if (cnt + kSstvStartWords <= cap) {
    ev[cnt++] = sstv_header(i, kSstvEvStart, kSstvStartWords - 1);
    ev[cnt++] = z.mode;
    ev[cnt++] = modes[z.mode].code;
    union { float f; int32_t i; } b;
    b.f = z.f_lead;
    ev[cnt++] = b.i;
    ev[cnt++] = (int32_t)e0;
  }
}

// ---- step 7: the sample of absolute index n = m - lag with lag product c, while a picture runs -----------------------------------
// i: the index within the call of output m; lb: the row's line buffer [kSstvLineWords].  An event that does not fit is
// dropped (sstv_event_cap: it fits).
PYSDR_SSTV_HD inline int sstv_pixel_value(SstvC P, float f_lead, float k_hz) {
  float a = sstv_hz(P, k_hz) - f_lead;
  a = a + 400.f;
  a = a * kSstvPixScale;
  a = floorf(a + 0.5f);
  return a < 0.f ? 0 : (a > 255.f ? 255 : (int)a);
}

PYSDR_SSTV_HD inline void sstv_pixel(SstvRow& z, SstvC c, uint32_t n, int i, const pysdr_sstv_cfg& cfg, const pysdr_sstv_mode* modes, uint32_t* lb,
                                     int32_t* ev, int& cnt, int cap) {
  if ((int32_t)(n - z.a_lo) < 0) return;                   // sync, porch or a separator
  if (n == z.a_lo) z.pacc = c;
  else { z.pacc.x = z.pacc.x + c.x; z.pacc.y = z.pacc.y + c.y; }
  if (n + 1u != z.a_hi) return;
  const pysdr_sstv_mode& md = modes[z.mode];
  const uint32_t v = (uint32_t)sstv_pixel_value(z.pacc, z.f_lead, cfg.k_hz);
  const int sh = 8 * (z.pix & 3), nb = sstv_line_bytes(md);
  z.word = (sh ? z.word : 0u) | (v << sh);
  if (sh == 24 || z.pix == nb - 1) lb[z.pix >> 2] = z.word;
  z.pix += 1;
  if (z.pix == nb) {
    const int nw = sstv_line_words(md);
    if (cnt + 2 + nw <= cap) {
      ev[cnt++] = sstv_header(i, kSstvEvLine, 1 + nw);
      ev[cnt++] = z.line;
      for (int k = 0; k < nw; ++k) ev[cnt++] = (int32_t)lb[k];
    }
    z.pix = 0;
    z.word = 0u;
    z.line += 1;
    if (z.line == md.lines) {
      if (cnt + kSstvEndWords <= cap) {
        ev[cnt++] = sstv_header(i, kSstvEvEnd, kSstvEndWords - 1);
        ev[cnt++] = md.lines;
      }
      z.phase = kSstvIdle;
      return;
    }
  }
  sstv_pixel_bounds(z, md);
}

// One output of a row, in the order the definition fixes: tick and VIS, anchor, pixel.  c_now and c_lag are the lag
// products of outputs m and m - lag; y points at the row's sample m.
PYSDR_SSTV_HD inline void sstv_step(SstvRow& z, SstvC c_now, SstvC c_lag, const SstvC* y, uint32_t m, int i, const pysdr_sstv_cfg& cfg,
                                    const pysdr_sstv_mode* modes, const SstvC* tw, const float* g, int L, float* ring, uint32_t* lb,
                                    signed char* q, int32_t* ev, int& cnt, int cap) {
  sstv_tick(z, c_now, m, cfg, modes, ring);
  if (z.phase == kSstvWait && m == z.m_a) sstv_start(z, sstv_anchor(y, m, z.f_lead, cfg, tw, g, L, q), i, modes, ev, cnt, cap);
  else if (z.phase == kSstvPicture) sstv_pixel(z, c_lag, m - (uint32_t)cfg.lag, i, cfg, modes, lb, ev, cnt, cap);
}

// ---- kernel arguments and the launch (sstv.hip) ------------------------------------------------------------------------------
struct SstvArgs {
  SstvC* y;                // Y + kSstvHpad: y[a * ypitch + i] = output i of this call, i >= -H the row's history
  long long ypitch;
  int n_out, nk, cap, L, H;
  uint32_t m0;             // the low 32 bits of the absolute index of the call's first output
  const pysdr_sstv_cfg* cfg;   // device copy
  const SstvC* tw;         // [kSstvNt]
  const float* g;          // [L]
  int32_t* si;             // [kSstvStateInts][nk]
  float* sf;               // [kSstvStateFloats][nk]
  float* ring;             // [nk][kSstvRing]
  uint32_t* lines;         // [nk][kSstvLineWords]
  int32_t* events;         // [nk][cap]
  int32_t* counts;         // [nk]
};

}  // namespace pysdr
