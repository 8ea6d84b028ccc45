// The RDS skimmer's pure half: settings and their rules, the event cap and its proof's terms, the
// event words, the workgroup's geometry, LDS budget and the index arithmetic of its tile walk, and the decoder's steps
// themselves -- four-quadrant discriminator and subcarrier mixer for one row sample, the chip grid, the matched filter in
// segments, the differential decision, the 104-bit register and the block check -- the very code the kernel (rds.hip)
// steps with, the host half (api_rds.hip) plans with and tests/rds_plan/plan_main.cpp runs on the CPU.  Plain C++: nothing
// here calls the HIP runtime, and the only traces of the device are the function qualifier and the division below.
#pragma once

#include <cfloat>
#include <cstdint>

#include "../../include/pysdr_hip.h"

#if defined(__HIPCC__)
#define PYSDR_RDS_HD __host__ __device__
#else
#define PYSDR_RDS_HD
#endif

namespace pysdr {

constexpr int kRdsTile = 1024;               // outputs of every row staged at once (behind the L of history)
constexpr int kRdsLmin = 385, kRdsLmax = 863; // L = 2 floor(fs_out / 1187.5) + 1, the matched pulse: fs_out from 228 to 512 kHz
constexpr int kRdsHpad = 864;                // complex samples kept in front of a row of Y: the history's room, >= L + 1
constexpr int kRdsPhases = 16;               // chips of a bit: decoders per row
constexpr int kRdsDecMax = 1 << 18;          // decoders: nk kRdsPhases
constexpr int kRdsMaxOutMax = 1 << 20;       // the header word holds the index within the call above bit 5
constexpr int kRdsNt = 1024;                 // twiddle table: one turn, indexed by a phase word's top ten bits
constexpr int kRdsSeg = 64;                  // taps of a segment of the matched filter's sum
constexpr int kRdsSegMax = (kRdsLmax + kRdsSeg - 1) / kRdsSeg;
constexpr uint32_t kRdsW19Min = 159383552u;  // 19 kHz at 512 kHz rows, in turns / 2^32
constexpr uint32_t kRdsW19Max = 357913942u;  // at 228 kHz rows
constexpr int kRdsChipsMax = (int)(((uint64_t)kRdsTile * kRdsW19Max) >> 32) + 1;   // chips that open inside one tile
constexpr uint32_t kRdsPoly = 0x5B9u;        // g(x) = x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1
constexpr uint32_t kRdsOffA = 0x0FCu, kRdsOffB = 0x198u, kRdsOffC = 0x168u, kRdsOffC2 = 0x350u, kRdsOffD = 0x1B4u;
constexpr uint32_t kRdsBlockMask = (1u << 26) - 1u;
// arctangent on [0, 1] (Abramowitz & Stegun 4.4.47), item 30's coefficients
constexpr float kRdsA0 = 0.9998660f, kRdsA1 = -0.3302995f, kRdsA2 = 0.1801410f, kRdsA3 = -0.0851330f, kRdsA4 = 0.0208351f;
constexpr float kRdsPi = 3.14159274f, kRdsHalfPi = 1.57079637f;   // float32 nearest pi and pi / 2

// The workgroup: whole rows, two of them, 256 threads.  All threads mix (phase A1) and filter (phase A2: one thread per
// segment of a chip of a row); thread (row, phase) of the first half wavefront walks its chips in order (phase B).
struct RdsGeom {
  static constexpr int kRows = 2;
  static constexpr int kDecoders = kRows * kRdsPhases;
  static constexpr int kThreads = 256;
  static constexpr int kVp = kRdsLmax + kRdsTile;                       // LDS row pitch of the mixer's products v
  static constexpr int kCp = kRdsChipsMax + 2;                          // of a (segment, row)'s partial sums
  static constexpr int kRollPer = (kRows * (kRdsLmax + 1) + kThreads - 1) / kThreads;   // history samples per thread
  // v, g, the partial sums, the tile's chips
  static constexpr int kLdsBytes = kRows * kVp * 8 + kRdsLmax * 4 + kRdsSegMax * kRows * kCp * 8 + kCp * 4;
  // The index arithmetic of the kernel's tile walk, used by rds.hip and walked by tests/rds_plan.  LDS columns are into
  // the product tile [kRows][kVp], of which a row uses L + kRdsTile: column c holds the product of the call's output
  // i0 + c - L.  Memory offsets are in complex samples from the row's first output of the call (the history sits at
  // -(L + 1) .. -1).
  PYSDR_RDS_HD static constexpr int carry_n(int L) { return kRows * L; }                 // products in front of a tile
  PYSDR_RDS_HD static constexpr int carry_row(int k, int L) { return k / L; }
  PYSDR_RDS_HD static constexpr int carry_col(int k, int L) { return k % L; }
  PYSDR_RDS_HD static constexpr int carry_src(int r, int c) { return r * kVp + kRdsTile + c; }   // the previous (full) tile's last L
  PYSDR_RDS_HD static constexpr int carry_dst(int r, int c) { return r * kVp + c; }              // L <= kRdsTile: never a source
  PYSDR_RDS_HD static constexpr int at(int r, int c) { return r * kVp + c; }
  // phase A1: the first tile makes the L products in front of it from the history, every tile its own nj
  PYSDR_RDS_HD static constexpr int mix_lo(int i0, int L) { return i0 == 0 ? 0 : L; }
  PYSDR_RDS_HD static constexpr int mix_n(int i0, int nj, int L) { return kRows * (L + nj - mix_lo(i0, L)); }
  PYSDR_RDS_HD static constexpr int mix_row(int k, int i0, int nj, int L) { return k / (L + nj - mix_lo(i0, L)); }
  PYSDR_RDS_HD static constexpr int mix_col(int k, int i0, int nj, int L) { return k % (L + nj - mix_lo(i0, L)) + mix_lo(i0, L); }
  PYSDR_RDS_HD static constexpr int mix_rel(int c, int L) { return c - L; }              // from the tile's first output
  // phase A2: work item k < nseg kRows nct -> (segment, row, chip of the tile), the chip fastest
  PYSDR_RDS_HD static constexpr int fir_n(int nseg, int nct) { return nseg * kRows * nct; }
  PYSDR_RDS_HD static constexpr int fir_chip(int k, int nct) { return k % nct; }
  PYSDR_RDS_HD static constexpr int fir_row(int k, int nct) { return (k / nct) % kRows; }
  PYSDR_RDS_HD static constexpr int fir_seg(int k, int nct) { return k / (nct * kRows); }
  PYSDR_RDS_HD static constexpr int newest(int r, int jj, int L) { return r * kVp + L + jj; }    // LDS: v of the tile's output jj
  PYSDR_RDS_HD static constexpr int part_at(int seg, int r, int ci) { return (seg * kRows + r) * kCp + ci; }
  // the history roll: the last L + 1 of [old history | this call's outputs]
  PYSDR_RDS_HD static constexpr int roll_n(int L) { return kRows * (L + 1); }
  PYSDR_RDS_HD static constexpr int roll_row(int k, int L) { return k / (L + 1); }
  PYSDR_RDS_HD static constexpr int roll_col(int k, int L) { return k % (L + 1); }
  PYSDR_RDS_HD static constexpr int roll_src(int n_out, int j, int L) { return n_out - (L + 1) + j; }
  PYSDR_RDS_HD static constexpr int roll_dst(int j, int L) { return j - (L + 1); }
};
static_assert(kRdsLmax + 1 <= kRdsHpad && kRdsHpad % 16 == 0, "the history fits its room");
static_assert(RdsGeom::kDecoders <= 64, "the decoders of a workgroup are within one wavefront");
static_assert(RdsGeom::kLdsBytes <= 64 * 1024, "static LDS");
static_assert(2 * RdsGeom::kLdsBytes <= 160 * 1024, "two workgroups per CU");
static_assert(kRdsChipsMax == 86 && kRdsSegMax == 14, "chips of a tile at 228 kHz rows, segments at 512 kHz rows");

// ---- settings -----------------------------------------------------------------------------------------------------------
// w19 and L come from one fs_out: n = (L - 1) / 2 = floor(fs_out / 1187.5), and fs_out / 1187.5 = 16 2^32 / w19 up to
// w19's rounding (half a unit, times n <= 431 < 512): n = floor((16 2^32 + 512) / w19), so that a rate with a whole number
// of samples per bit (228 kHz: 192) keeps its n.
constexpr long long kRdsBitTurns = (16ll << 32) + 512;
inline bool rds_cfg_ok(const pysdr_rds_cfg& c, int L) {
  if (c.w19 < kRdsW19Min || c.w19 > kRdsW19Max) return false;
  if (L < kRdsLmin || L > kRdsLmax || !(L & 1)) return false;
  const long long n = (L - 1) / 2;
  return n * (long long)c.w19 <= kRdsBitTurns && (n + 1) * (long long)c.w19 > kRdsBitTurns;
}

// ---- the chip grid ---------------------------------------------------------------------------------------------------------
// Output m opens a chip iff (m w19) mod 2^32 < w19: the 19 kHz accumulator wrapped on its way to m.  With
// A = ((m0 - 1) w19) mod 2^32, the accumulator in front of a call whose first output is m0, the chips that open at the
// call's outputs 0 .. j are floor((A + (j + 1) w19) / 2^32): every wrap is one chip.
PYSDR_RDS_HD inline bool rds_tick(uint32_t m, uint32_t w19) { return (uint32_t)(m * w19) < w19; }
PYSDR_RDS_HD inline uint32_t rds_acc_before(uint32_t m0, uint32_t w19) { return (uint32_t)((m0 - 1u) * w19); }
PYSDR_RDS_HD inline int rds_chips_upto(uint32_t A, int j, uint32_t w19) {                 // j >= -1
  return (int)(((uint64_t)A + (uint64_t)(j + 1) * (uint64_t)w19) >> 32);
}

// ---- the event cap: words one decoder can emit in a call of max_out outputs -----------------------------------------------
// A call of n outputs opens floor((A + n w19) / 2^32) chips, at most rds_max_chips = floor(n w19 / 2^32) + 1 since
// A < 2^32.  The row counts chips, and a chip whose count is c goes to phase c & 15: a phase gets every sixteenth chip, so
// at most ceil(chips / 16) of a call's, each of which is one bit to that phase's decoder.  A bit completes at most one
// group, and a group is three words.
constexpr int kRdsGroupWords = 3;
constexpr int rds_max_chips(int n_out, uint32_t w19) { return (int)(((uint64_t)n_out * (uint64_t)w19) >> 32) + 1; }
constexpr int rds_max_bits(int n_out, uint32_t w19) { return (rds_max_chips(n_out, w19) + kRdsPhases - 1) / kRdsPhases; }
constexpr int rds_event_cap(int max_out, uint32_t w19) { return kRdsGroupWords * rds_max_bits(max_out, w19); }

struct RdsPlan {
  int L = 0;
  int nseg = 0;        // segments of the matched filter's sum
  int ndec = 0;        // decoders: nk kRdsPhases
  int cap = 0;         // event words per decoder
  int groups = 0;      // workgroups
  int ypitch = 0;      // row pitch of Y, complex samples: kRdsHpad of history room, then the call's outputs
};

inline bool rds_plan(int nk, int L, int max_out, const pysdr_rds_cfg* cfg, RdsPlan* p) {
  if (nk < 1 || (long long)nk * kRdsPhases > kRdsDecMax || max_out < 1 || max_out > kRdsMaxOutMax || !cfg || !rds_cfg_ok(*cfg, L)) return false;
  RdsPlan q;
  q.L = L;
  q.nseg = (L + kRdsSeg - 1) / kRdsSeg;
  q.ndec = nk * kRdsPhases;
  q.cap = rds_event_cap(max_out, cfg->w19);
  q.groups = (nk + RdsGeom::kRows - 1) / RdsGeom::kRows;
  q.ypitch = kRdsHpad + ((max_out + 15) & ~15);
  *p = q;
  return true;
}

// the header word: (index within the call of the output that completed the group) << 5 | phase << 1 | C'
PYSDR_RDS_HD constexpr int32_t rds_header(int i, int phase, int c2) { return (int32_t)(((uint32_t)i << 5) | ((uint32_t)phase << 1) | (uint32_t)c2); }
PYSDR_RDS_HD constexpr int rds_header_index(int32_t w) { return (int)((uint32_t)w >> 5); }
PYSDR_RDS_HD constexpr int rds_header_phase(int32_t w) { return (int)(((uint32_t)w >> 1) & 15u); }
PYSDR_RDS_HD constexpr int rds_header_c2(int32_t w) { return (int)((uint32_t)w & 1u); }

struct alignas(8) RdsC { float x, y; };    // a complex sample as the channelizer stores it; a product v; a sum z

// ---- step 1: the discriminator, arg(y conj(y1)) in radians, four quadrants ----------------------------------------------------
PYSDR_RDS_HD inline float rds_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn(a, b);
#else
  return a / b;
#endif
}
// Every float operation rounds on its own (-ffp-contract=off).  d = 0 unless 0 < max <= FLT_MAX and min <= max: where the
// product is zero, infinite or not a number -- so d is always finite, and at most pi.
PYSDR_RDS_HD inline float rds_arg(RdsC y, RdsC y1) {
  const float re = y.x * y1.x + y.y * y1.y;
  const float im = y.y * y1.x - y.x * y1.y;
  const float ax = re < 0.f ? -re : re, ay = im < 0.f ? -im : im;
  const bool swap = ay > ax;
  const float mx = swap ? ay : ax, mn = swap ? ax : ay;
  if (!(mx > 0.f && mx <= FLT_MAX && mn <= mx)) return 0.f;
  const float t = rds_div(mn, mx);
  const float t2 = t * t;
  float s = t2 * kRdsA4;
  s = kRdsA3 + s; s = t2 * s;
  s = kRdsA2 + s; s = t2 * s;
  s = kRdsA1 + s; s = t2 * s;
  s = kRdsA0 + s;
  float phi = t * s;
  if (swap) phi = kRdsHalfPi - phi;        // the octant: |im| > |re|
  if (re < 0.f) phi = kRdsPi - phi;        // the left half plane
  if (im < 0.f) phi = -phi;                // the lower one
  return phi;
}

// ---- step 2: the subcarrier, 57 kHz = 3 x 19 kHz, for the row sample of absolute index m (its low 32 bits) ---------------------
PYSDR_RDS_HD inline RdsC rds_mix(RdsC y, RdsC y1, uint32_t m, uint32_t w19, const RdsC* tw) {
  const float d = rds_arg(y, y1);
  const RdsC t = tw[(uint32_t)(m * 3u * w19) >> 22];
  return RdsC{d * t.x, d * t.y};
}

// ---- step 3: the matched filter at a chip whose newest product is vw[0] (vw[-i] = v[m_c - i], i < L) ---------------------------
// z = sum over the segments, ascending, of the segment's sum; segment s sums g[i] v[m_c - i] over i = 64 s .. min(L,
// 64 s + 64) - 1, ascending; in both the first term is assigned, not added to a zero.
PYSDR_RDS_HD inline RdsC rds_segment(const RdsC* vw, const float* g, int L, int seg) {
  const int lo = seg * kRdsSeg, hi = lo + kRdsSeg < L ? lo + kRdsSeg : L;
  RdsC u{g[lo] * vw[-lo].x, g[lo] * vw[-lo].y};
  for (int i = lo + 1; i < hi; ++i) {
    const RdsC v = vw[-i];
    const float gi = g[i];
    u.x = u.x + gi * v.x;
    u.y = u.y + gi * v.y;
  }
  return u;
}
PYSDR_RDS_HD inline RdsC rds_sum(const RdsC* part, int stride, int nseg) {
  RdsC z = part[0];
  for (int s = 1; s < nseg; ++s) { z.x = z.x + part[s * stride].x; z.y = z.y + part[s * stride].y; }
  return z;
}

// ---- steps 4 to 6: one decoder, in registers for the call ---------------------------------------------------------------------
struct RdsDec {
  uint32_t w[4];       // the last 104 bits, 26 to a word: w[0] the oldest block, bit 25 of each its first bit
  RdsC zprev;          // the phase's z one bit ago: entry `phase` of the row's ring
};

// the remainder of a 26-bit block by g(x), MSB first
PYSDR_RDS_HD inline uint32_t rds_syndrome(uint32_t b) {
  for (int k = 25; k >= 10; --k)
    if (b >> k & 1u) b ^= kRdsPoly << (k - 10);
  return b;
}

// Steps 4 to 6 for the chip z of this decoder's phase, at the output of index i within the call: the decoder's event
// slots ev [cap] and the words used so far, cnt.  A group whose event does not fit is dropped (rds_event_cap: it fits).
PYSDR_RDS_HD inline void rds_bit(RdsDec& d, RdsC z, int i, int phase, int32_t* ev, int& cnt, int cap) {
  const float q = z.x * d.zprev.x + z.y * d.zprev.y;
  const uint32_t bit = q < 0.f ? 1u : 0u;
  d.zprev = z;
  d.w[0] = ((d.w[0] << 1) | (d.w[1] >> 25)) & kRdsBlockMask;
  d.w[1] = ((d.w[1] << 1) | (d.w[2] >> 25)) & kRdsBlockMask;
  d.w[2] = ((d.w[2] << 1) | (d.w[3] >> 25)) & kRdsBlockMask;
  d.w[3] = ((d.w[3] << 1) | bit) & kRdsBlockMask;
  if (rds_syndrome(d.w[0]) != kRdsOffA || rds_syndrome(d.w[1]) != kRdsOffB || rds_syndrome(d.w[3]) != kRdsOffD) return;
  const uint32_t sc = rds_syndrome(d.w[2]);
  if (sc != kRdsOffC && sc != kRdsOffC2) return;
  if (cnt + kRdsGroupWords > cap) return;
  ev[cnt++] = rds_header(i, phase, sc == kRdsOffC2 ? 1 : 0);
  ev[cnt++] = (int32_t)(((d.w[0] >> 10) << 16) | (d.w[1] >> 10));
  ev[cnt++] = (int32_t)(((d.w[2] >> 10) << 16) | (d.w[3] >> 10));
}

// ---- kernel arguments and the launch (rds.hip) ----------------------------------------------------------------------------
struct RdsArgs {
  RdsC* y;                 // Y + kRdsHpad: y[a * ypitch + i] = output i of this call, i >= -(L + 1) the row's history
  long long ypitch;
  int n_out, nk, cap, ndec, L, nseg;
  uint32_t m0;             // the low 32 bits of the absolute index of the call's first output
  uint32_t w19;
  const RdsC* tw;          // [kRdsNt]
  const float* g;          // [L]
  uint32_t* regs;          // [4][ndec]
  uint32_t* chips;         // [nk]: chips since reset
  RdsC* ring;              // [nk][kRdsPhases]
  int32_t* events;         // [ndec][cap]
  int32_t* counts;         // [ndec]
};

}  // namespace pysdr
