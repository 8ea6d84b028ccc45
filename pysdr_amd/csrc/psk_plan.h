// The PSK31 skimmer's pure half: settings and their rules, the event cap and word, the workgroup's
// geometry, LDS budget and the index arithmetic of its tile walk, and the decoder's two steps themselves -- mixer +
// matched filter for one row output, and the symbol step -- the very code the kernel (psk.hip) steps with, the host half
// (api_psk.hip) plans with and tests/psk_plan/plan_main.cpp runs on the CPU.  Plain C++: nothing here calls the HIP
// runtime, and the only trace of the device is the function qualifier below.
#pragma once

#include <cfloat>
#include <cstdint>

#include "../../include/pysdr_hip.h"

#if defined(__HIPCC__)
#define PYSDR_PSK_HD __host__ __device__
#else
#define PYSDR_PSK_HD
#endif

namespace pysdr {

constexpr int kPskTile = 64;               // outputs of every row staged at once (behind the L - 1 of history)
constexpr int kPskHpad = 32;               // complex samples kept in front of a row of Y: the history's room, >= L - 1
constexpr int kPskFineMax = 1 << 18;       // decoders: nk NSUB
constexpr int kPskMaxOutMax = 1 << 20;     // the event word holds the index within the call above bit 11
constexpr int kPskSettleMax = 1 << 22;     // settling symbols n0
constexpr float kPskPmaxMax = 1.0e18f;     // |z|^2 <= (2 pmax)^2 stays below FLT_MAX
constexpr int kPskStateInts = 5;           // pt, cnt, sh, open, seen
constexpr int kPskStateFloats = 4;         // qn, qd, cr, ci

// everything that follows from S, the row samples per symbol
template <int S>
struct PskGeom {
  static_assert(S == 8 || S == 12, "S is 8 or 12");
  static constexpr int kS = S;
  static constexpr int kNsub = 4 * S;                 // decoders per row
  static constexpr int kL = 2 * S;                    // taps of the matched filter
  static constexpr int kNt = 32 * S;                  // twiddle table: one turn in steps of baud / 32
  static constexpr int kRows = S == 8 ? 2 : 4;        // rows per workgroup: whole waves (64 and 192 threads)
  static constexpr int kThreads = kRows * kNsub;
  static constexpr int kYp = kPskTile + kL - 1;       // LDS row pitch of the staged samples; odd
  static constexpr int kLdsBytes = kNt * 8 + kL * 4 + kRows * kYp * 8 + S * kThreads * 4;   // tw, g, y, e
  // The index arithmetic of the kernel's tile walk, used by psk.hip and walked by tests/psk_plan.  LDS indices are into
  // the sample tile [kRows][kYp]; memory offsets are in complex samples from the row's first output of the call (the
  // history sits at -(L - 1) .. -1).
  static constexpr int kCarry = kRows * (kL - 1);     // threads that bring the L - 1 samples in front of a tile
  PYSDR_PSK_HD static constexpr int carry_row(int tid) { return tid / (kL - 1); }
  PYSDR_PSK_HD static constexpr int carry_col(int tid) { return tid % (kL - 1); }
  PYSDR_PSK_HD static constexpr int carry_src(int hr, int hc) { return hr * kYp + kPskTile + hc; }   // LDS: the previous tile's last samples
  PYSDR_PSK_HD static constexpr int carry_dst(int hr, int hc) { return hr * kYp + hc; }             // LDS
  PYSDR_PSK_HD static constexpr int hist_off(int hc) { return hc - (kL - 1); }                       // memory: the row's history
  PYSDR_PSK_HD static constexpr int stage_row(int k) { return k / kPskTile; }                        // staging load k < kRows kPskTile
  PYSDR_PSK_HD static constexpr int stage_col(int k) { return k % kPskTile; }
  PYSDR_PSK_HD static constexpr int stage_dst(int rr, int c) { return rr * kYp + kL - 1 + c; }       // LDS
  PYSDR_PSK_HD static constexpr int win(int r, int jj) { return r * kYp + jj + kL - 1; }             // LDS: newest sample of the tile's output jj
  PYSDR_PSK_HD static constexpr int roll_src(int n_out, int j) { return n_out - (kL - 1) + j; }      // memory, j < L - 1
  PYSDR_PSK_HD static constexpr int roll_dst(int j) { return j - (kL - 1); }                         // memory
  PYSDR_PSK_HD static constexpr int e_at(int p, int tid) { return p * kThreads + tid; }              // LDS: symbol energy of phase p
};

constexpr bool psk_s_ok(int S) { return S == 8 || S == 12; }
constexpr int psk_nsub(int S) { return 4 * S; }
constexpr int psk_rows(int S) { return S == 8 ? PskGeom<8>::kRows : PskGeom<12>::kRows; }
constexpr int psk_threads(int S) { return S == 8 ? PskGeom<8>::kThreads : PskGeom<12>::kThreads; }
constexpr int psk_lds_bytes(int S) { return S == 8 ? PskGeom<8>::kLdsBytes : PskGeom<12>::kLdsBytes; }

inline bool psk_cfg_ok(const pysdr_psk_cfg& c) {
  if (!(c.a_t > 0.f && c.a_t <= 1.f) || !(c.a_q > 0.f && c.a_q <= 1.f)) return false;
  const float g[3] = {c.hi, c.lo, c.hy};
  for (float v : g)
    if (!(v > 0.f && v <= FLT_MAX)) return false;
  if (!(c.lo <= c.hi)) return false;
  if (!(c.pmax > 0.f && c.pmax <= kPskPmaxMax)) return false;
  return c.n0 >= 1 && c.n0 <= kPskSettleMax;
}

// most events one decoder can emit in a call of max_out outputs: a character needs three symbols (a 1, then 00), and a
// symbol is taken at least S / 2 samples after the last, so two events are at least 3 S / 2 samples apart
constexpr int psk_event_gap(int S) { return 3 * S / 2; }
constexpr int psk_event_cap(int max_out, int S) { return max_out / psk_event_gap(S) + 1; }

struct PskPlan {
  int S = 0, nsub = 0;
  int nfine = 0;       // decoders: nk nsub
  int cap = 0;         // event slots per decoder
  int groups = 0;      // workgroups
  int ypitch = 0;      // row pitch of Y, complex samples: kPskHpad of history room, then the call's outputs
};

inline bool psk_plan(int nk, int S, int max_out, const pysdr_psk_cfg* cfg, PskPlan* p) {
  if (!psk_s_ok(S) || nk < 1 || (long long)nk * psk_nsub(S) > kPskFineMax || max_out < 1 || max_out > kPskMaxOutMax || !cfg ||
      !psk_cfg_ok(*cfg))
    return false;
  PskPlan q;
  q.S = S;
  q.nsub = psk_nsub(S);
  q.nfine = nk * q.nsub;
  q.cap = psk_event_cap(max_out, S);
  q.groups = (nk + psk_rows(S) - 1) / psk_rows(S);
  q.ypitch = kPskHpad + ((max_out + 15) & ~15);
  *p = q;
  return true;
}

// the event word: (index within the call) << 11 | code, code = the Varicode bits 1 .. 2047
PYSDR_PSK_HD constexpr int32_t psk_pack(int i, int code) { return (int32_t)(((uint32_t)i << 11) | (uint32_t)code); }
PYSDR_PSK_HD constexpr int psk_event_index(int32_t w) { return (int)((uint32_t)w >> 11); }
PYSDR_PSK_HD constexpr int psk_event_code(int32_t w) { return (int)((uint32_t)w & 2047u); }

struct alignas(8) PskC { float x, y; };   // a complex sample as the channelizer stores it

struct PskDec {                        // one decoder's state but e[S], in registers for the call
  float qn, qd, cr, ci;
  int32_t pt, cnt, sh, open, seen;
};

PYSDR_PSK_HD inline PskDec psk_dec_init(int S) {
  PskDec z{};
  z.cnt = S;
  return z;
}

// (a b) mod n for 0 <= a, b < n <= 384
PYSDR_PSK_HD constexpr int psk_mulmod(int a, int b, int n) { return (a * b) % n; }
// q mod NT as a non-negative number, q = 2 j - NSUB + 1
PYSDR_PSK_HD constexpr int psk_qmod(int j, int S) { return ((2 * j - 4 * S + 1) + 32 * S) % (32 * S); }

// Step 1 of the definition for the row output whose newest sample is yw[0] (yw[-i] = y[m - i], i < L, zeros before the
// stream's start): v = y tw[(q k) mod NT], u = sum g[i] v[m - i], i ascending; t = (q m) mod NT, qm = q mod NT.  Every
// float operation rounds on its own (-ffp-contract=off).  Returns pw, 0 with u = 0 where it is not <= pmax.
template <int S>
PYSDR_PSK_HD inline float psk_filter(const PskC* yw, const PskC* tw, const float* g, int t, int qm, float pmax, float& ur, float& ui) {
  constexpr int L = PskGeom<S>::kL, NT = PskGeom<S>::kNt;
  float ar = 0.f, ai = 0.f;
#pragma unroll
  for (int i = 0; i < L; ++i) {
    const PskC y = yw[-i], w = tw[t];
    const float vr = y.x * w.x - y.y * w.y, vi = y.x * w.y + y.y * w.x;
    if (i == 0) { ar = g[0] * vr; ai = g[0] * vi; }
    else { ar = ar + g[i] * vr; ai = ai + g[i] * vi; }
    t -= qm;
    if (t < 0) t += NT;
  }
  float pw = ar * ar + ai * ai;
  if (!(pw <= pmax)) { ar = 0.f; ai = 0.f; pw = 0.f; }
  ur = ar; ui = ai;
  return pw;
}

// Step 3 (a) to (e) for the symbol taken at a sample of phase p = m mod S; e[i * estride] is the symbol energy of phase
// i, already updated for this sample.  Returns the code of the event this symbol emits, or 0.
template <int S>
PYSDR_PSK_HD inline int psk_symbol(PskDec& z, const pysdr_psk_cfg& c, float ur, float ui, const float* e, int estride, int p) {
  const float zr = ur * z.cr + ui * z.ci, zi = ui * z.cr - ur * z.ci;
  z.cr = ur; z.ci = ui;
  const float A = zr * zr, B = zi * zi;
  z.qn = z.qn + c.a_q * ((A - B) - z.qn);
  z.qd = z.qd + c.a_q * ((A + B) - z.qd);
  if (z.seen < c.n0) { z.seen += 1; z.open = 0; }
  else z.open = (z.qd > 0.f && z.qn >= (z.open ? c.lo : c.hi) * z.qd) ? 1 : 0;
  z.sh = 2 * z.sh + (zr >= 0.f ? 1 : 0);
  if (z.sh >= 8192) z.sh = 4096 | (z.sh & 4095);
  int code = 0;
  if ((z.sh & 3) == 0) {
    const int cd = z.sh >> 2;
    if (cd != 0 && z.open) code = cd;
    z.sh = 0;
  }
  float best = e[0], ept = e[0];
  int b = 0;
#pragma unroll
  for (int i = 1; i < S; ++i) {
    const float v = e[i * estride];
    if (v > best) { best = v; b = i; }
    if (i == z.pt) ept = v;
  }
  if (best > c.hy * ept) z.pt = b;
  const int d = (z.pt - p + S / 2 + S) % S - S / 2;
  z.cnt = S + d;
  return code;
}

// ---- kernel arguments and the launch (psk.hip) -----------------------------------------------------------------------
struct PskArgs {
  PskC* y;                 // Y + kPskHpad: y[a * ypitch + i] = output i of this call, i >= -(L - 1) the row's history
  long long ypitch;
  int n_out, nk, cap, nfine;
  int m0_mod;              // (absolute index of the call's first output) mod NT
  pysdr_psk_cfg cfg;
  const PskC* tw;          // [NT]
  const float* g;          // [L]
  float* e;                // [S][nfine]
  float* sf;               // [4][nfine]: qn, qd, cr, ci
  int32_t* si;             // [5][nfine]: pt, cnt, sh, open, seen
  int32_t* events;         // [nfine][cap]
  int32_t* counts;         // [nfine]
};

}  // namespace pysdr
