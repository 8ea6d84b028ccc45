// The RTTY raster skimmer's pure half: settings and their rules, the event cap and word, the
// workgroup's geometry, LDS budget and the index arithmetic of its tile walk, and the decoder's steps themselves -- mixer +
// one-bit matched filter for one tone of one row output, and the clock / framing / squelch step -- the very code the
// kernel (fsk.hip) steps with, the host half (api_fsk.hip) plans with and tests/fsk_plan/plan_main.cpp runs on the CPU.
// Plain C++: nothing here calls the HIP runtime, and the only trace of the device is the function qualifier below.
#pragma once

#include <cfloat>
#include <cstdint>

#include "../../include/pysdr_hip.h"

#if defined(__HIPCC__)
#define PYSDR_FSK_HD __host__ __device__
#else
#define PYSDR_FSK_HD
#endif

namespace pysdr {

constexpr int kFskTile = 64;               // outputs of every row staged at once (behind the S - 1 of history)
constexpr int kFskHpad = 32;               // complex samples kept in front of a row of Y: the history's room, >= S - 1
constexpr int kFskFineMax = 1 << 18;       // decoders: nk NSUB
constexpr int kFskMaxOutMax = 1 << 20;     // the event word holds the index within the call above bit 6
constexpr int kFskSettleMax = 1 << 22;     // settling instants n0
constexpr float kFskPmaxMax = 1.0e18f;     // w + l <= 2 pmax stays far below FLT_MAX
constexpr int kFskStateInts = 8;           // st, cnt, sh, nb, prev, fig, open, seen
constexpr int kFskStateFloats = 4;         // qn, qd, bm, bs
constexpr int kFskOpenAt = 6;              // where `open` sits among the state's ints
constexpr int kFskToneGap = 15;            // mark is this many tones (raster steps of baud / 4) above space

// everything that follows from S, the row samples per bit
template <int S>
struct FskGeom {
  static_assert(S == 22 || S == 33, "S is 22 or 33");
  static constexpr int kS = S;
  static constexpr int kNsub = S;                     // decoders per row
  static constexpr int kNt = 8 * S;                   // twiddle table: one turn in steps of baud / 8
  // Rows per workgroup.  A row has 22 or 33 decoders, so rows share waves: 8 x 22 = 176 threads fill 3 waves to 92 %, 7 x 33
  // = 231 fill 4 waves to 90 % (one row per wave would leave 66 % and 48 % of the lanes idle).  The lanes of a row read one
  // sample address (a broadcast); the rows of a wave read kYp apart.
  static constexpr int kRows = S == 22 ? 8 : 7;
  static constexpr int kDecoders = kRows * kNsub;     // threads that own a decoder
  static constexpr int kThreads = (kDecoders + 63) / 64 * 64;   // whole waves; the last lanes own none
  static constexpr int kYp = kFskTile + S - 1;        // LDS row pitch of the staged samples
  static constexpr int kLdsBytes = kNt * 8 + S * 4 + kRows * kYp * 8;   // tw, g, y
  // The index arithmetic of the kernel's tile walk, used by fsk.hip and walked by tests/fsk_plan.  LDS indices are into
  // the sample tile [kRows][kYp]; memory offsets are in complex samples from the row's first output of the call (the
  // history sits at -(S - 1) .. -1).
  static constexpr int kCarry = kRows * (S - 1);      // samples in front of a tile: history, or the last tile's end
  PYSDR_FSK_HD static constexpr int carry_row(int k) { return k / (S - 1); }
  PYSDR_FSK_HD static constexpr int carry_col(int k) { return k % (S - 1); }
  PYSDR_FSK_HD static constexpr int carry_src(int hr, int hc) { return hr * kYp + kFskTile + hc; }   // LDS: the previous tile's last samples
  PYSDR_FSK_HD static constexpr int carry_dst(int hr, int hc) { return hr * kYp + hc; }             // LDS
  PYSDR_FSK_HD static constexpr int hist_off(int hc) { return hc - (S - 1); }                        // memory: the row's history
  PYSDR_FSK_HD static constexpr int stage_row(int k) { return k / kFskTile; }                        // staging load k < kRows kFskTile
  PYSDR_FSK_HD static constexpr int stage_col(int k) { return k % kFskTile; }
  PYSDR_FSK_HD static constexpr int stage_dst(int rr, int c) { return rr * kYp + S - 1 + c; }        // LDS
  PYSDR_FSK_HD static constexpr int win(int r, int jj) { return r * kYp + jj + S - 1; }              // LDS: newest sample of the tile's output jj
  PYSDR_FSK_HD static constexpr int roll_src(int n_out, int j) { return n_out - (S - 1) + j; }       // memory, j < S - 1
  PYSDR_FSK_HD static constexpr int roll_dst(int j) { return j - (S - 1); }                          // memory
};
static_assert(FskGeom<22>::kCarry <= FskGeom<22>::kThreads && FskGeom<33>::kCarry <= FskGeom<33>::kThreads, "one thread per carried sample");
static_assert(33 - 1 <= kFskTile && 33 - 1 <= kFskHpad, "the history fits a tile and its room");

constexpr bool fsk_s_ok(int S) { return S == 22 || S == 33; }
constexpr int fsk_rows(int S) { return S == 22 ? FskGeom<22>::kRows : FskGeom<33>::kRows; }
constexpr int fsk_threads(int S) { return S == 22 ? FskGeom<22>::kThreads : FskGeom<33>::kThreads; }
constexpr int fsk_lds_bytes(int S) { return S == 22 ? FskGeom<22>::kLdsBytes : FskGeom<33>::kLdsBytes; }

inline bool fsk_cfg_ok(const pysdr_fsk_cfg& c) {
  if (!(c.a_q > 0.f && c.a_q <= 1.f) || !(c.a_b > 0.f && c.a_b <= 1.f)) return false;
  const float g[3] = {c.hi, c.lo, c.bal};
  for (float v : g)
    if (!(v > 0.f && v <= 1.f)) return false;          // ratios of non-negative powers: above 1 nothing would ever open
  if (!(c.lo <= c.hi)) return false;
  if (!(c.pmax > 0.f && c.pmax <= kFskPmaxMax)) return false;
  return c.n0 >= 1 && c.n0 <= kFskSettleMax;
}

// Most events one decoder can emit in a call of max_out outputs.  An event is emitted at a stop bit's sampling instant;
// the next start edge is at least one output later, its start bit is sampled S / 2 outputs after the edge, then five data
// bits and the stop bit S apart: two events are at least 6 S + S / 2 + 1 outputs apart.
constexpr int fsk_event_gap(int S) { return 6 * S + S / 2 + 1; }
constexpr int fsk_event_cap(int max_out, int S) { return max_out / fsk_event_gap(S) + 1; }

struct FskPlan {
  int S = 0, nsub = 0;
  int nfine = 0;       // decoders: nk nsub
  int cap = 0;         // event slots per decoder
  int groups = 0;      // workgroups
  int ypitch = 0;      // row pitch of Y, complex samples: kFskHpad of history room, then the call's outputs
};

inline bool fsk_plan(int nk, int S, int max_out, const pysdr_fsk_cfg* cfg, FskPlan* p) {
  if (!fsk_s_ok(S) || nk < 1 || (long long)nk * S > kFskFineMax || max_out < 1 || max_out > kFskMaxOutMax || !cfg || !fsk_cfg_ok(*cfg))
    return false;
  FskPlan q;
  q.S = S;
  q.nsub = S;
  q.nfine = nk * q.nsub;
  q.cap = fsk_event_cap(max_out, S);
  q.groups = (nk + fsk_rows(S) - 1) / fsk_rows(S);
  q.ypitch = kFskHpad + ((max_out + 15) & ~15);
  *p = q;
  return true;
}

// the event word: (index within the call) << 6 | code, code = sh + 32 fig in 0 .. 63
PYSDR_FSK_HD constexpr int32_t fsk_pack(int i, int code) { return (int32_t)(((uint32_t)i << 6) | (uint32_t)code); }
PYSDR_FSK_HD constexpr int fsk_event_index(int32_t w) { return (int)((uint32_t)w >> 6); }
PYSDR_FSK_HD constexpr int fsk_event_code(int32_t w) { return (int)((uint32_t)w & 63u); }

struct alignas(8) FskC { float x, y; };   // a complex sample as the channelizer stores it

struct FskDec {                        // one decoder's state, in registers for the call
  float qn, qd, bm, bs;
  int32_t st, cnt, sh, nb, prev, fig, open, seen;
};

PYSDR_FSK_HD inline FskDec fsk_dec_init(int S) {
  FskDec z{};
  z.cnt = S;
  z.prev = 1;
  return z;
}

// (a b) mod n for 0 <= a, b < n <= 264
PYSDR_FSK_HD constexpr int fsk_mulmod(int a, int b, int n) { return (a * b) % n; }
// q mod NT as a non-negative number for tone t of a row, q = 2 t - S - 14, t < S + 15: decoder j's space tone is t = j,
// its mark tone t = j + 15
PYSDR_FSK_HD constexpr int fsk_qmod(int t, int S) { return ((2 * t - S - 14) + 8 * S) % (8 * S); }

// Step 1 of the definition for one tone of the row output whose newest sample is yw[0] (yw[-i] = y[m - i], i < S, zeros
// before the stream's start): v = y tw[(q k) mod NT], u = sum g[i] v[m - i], i ascending; t = (q m) mod NT, qm = q mod NT.
// Every float operation rounds on its own (-ffp-contract=off).  Returns P = |u|^2, 0 where it is not <= pmax.
template <int S>
PYSDR_FSK_HD inline float fsk_tone(const FskC* yw, const FskC* tw, const float* g, int t, int qm, float pmax) {
  constexpr int NT = FskGeom<S>::kNt;
  float ar = 0.f, ai = 0.f;
#pragma unroll
  for (int i = 0; i < S; ++i) {
    const FskC y = yw[-i], w = tw[t];
    const float vr = y.x * w.x - y.y * w.y, vi = y.x * w.y + y.y * w.x;
    if (i == 0) { ar = g[0] * vr; ai = g[0] * vi; }
    else { ar = ar + g[i] * vr; ai = ai + g[i] * vi; }
    t -= qm;
    if (t < 0) t += NT;
  }
  const float pw = ar * ar + ai * ai;
  return pw <= pmax ? pw : 0.f;
}

// Steps 2 and 3 for one row output with the tone powers PS and PM.  Returns the code 0 .. 63 of the event this output
// emits, or -1.
template <int S>
PYSDR_FSK_HD inline int fsk_step(FskDec& z, const pysdr_fsk_cfg& c, float PS, float PM) {
  const int d = PM > PS ? 1 : 0;
  int code = -1;
  z.cnt -= 1;
  if (z.st == 0 && z.prev == 1 && d == 0) {            // a start edge
    z.st = 1;
    z.cnt = S / 2;
  } else if (z.cnt == 0) {                             // a sampling instant
    bool inch = z.st != 0, framed = false;
    if (z.st == 1) {
      if (d == 0) { z.st = 2; z.nb = 0; z.sh = 0; }
      else { z.st = 0; inch = false; }
    } else if (z.st == 2) {
      z.sh |= d << z.nb;
      z.nb += 1;
      if (z.nb == 5) z.st = 3;
    } else if (z.st == 3) {
      framed = d == 1;
      z.st = 0;
    }
    z.cnt = S;
    const float w = PM > PS ? PM : PS, l = PM > PS ? PS : PM;
    z.qn = z.qn + c.a_q * ((w - l) - z.qn);
    z.qd = z.qd + c.a_q * ((w + l) - z.qd);
    if (inch && d) z.bm = z.bm + c.a_b * (PM - z.bm);
    if (inch && !d) z.bs = z.bs + c.a_b * (PS - z.bs);
    if (z.seen < c.n0) { z.seen += 1; z.open = 0; }
    else {
      const float lo = z.bm < z.bs ? z.bm : z.bs, hi = z.bm < z.bs ? z.bs : z.bm;
      z.open = (z.qd > 0.f && z.qn >= (z.open ? c.lo : c.hi) * z.qd && lo >= c.bal * hi) ? 1 : 0;
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

// ---- kernel arguments and the launch (fsk.hip) -----------------------------------------------------------------------
struct FskArgs {
  FskC* y;                 // Y + kFskHpad: y[a * ypitch + i] = output i of this call, i >= -(S - 1) the row's history
  long long ypitch;
  int n_out, nk, cap, nfine;
  int m0_mod;              // (absolute index of the call's first output) mod NT
  pysdr_fsk_cfg cfg;
  const FskC* tw;          // [NT]
  const float* g;          // [S]
  float* sf;               // [4][nfine]: qn, qd, bm, bs
  int32_t* si;             // [8][nfine]: st, cnt, sh, nb, prev, fig, open, seen
  int32_t* events;         // [nfine][cap]
  int32_t* counts;         // [nfine]
};

}  // namespace pysdr
