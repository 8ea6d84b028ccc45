// The FT4 skimmer's pure half: settings and their rules, the ring depth, the workgroup's geometry,
// LDS budget and the index arithmetic of its tile walk, and the steps themselves -- one bin of one step's spectrum, the
// score of one decoder over the four Costas arrays, one soft bit -- the very code the kernels (ft4.hip) step with, the host
// half (api_ft4.hip) plans with and tests/ft4_plan/plan_main.cpp runs on the CPU.  What item 22 already has in a generic
// form comes from ft8_plan.h: the complex sample Ft8C, the event words (ft8_pack and its readers), ft8_steps_done, the
// peak rule ft8_peak (the two cfg layouts are the same) and the reach, keep and gap constants that belong to it.
// Plain C++: nothing here calls the HIP runtime.
#pragma once

#include "ft8_plan.h"

namespace pysdr {

constexpr int kFt4Hpad = 80;               // complex samples kept in front of a row of Y: the history's room, >= S - 1
constexpr int kFt4FineMax = kFt8FineMax;   // decoders: nk NSUB
constexpr int kFt4MaxOutMax = kFt8MaxOutMax;
constexpr float kFt4PmaxMax = kFt8PmaxMax; // 64 powers <= pmax sum far below FLT_MAX
constexpr int kFt4StepsPerSym = 4;         // steps per symbol: QS = S / 4 outputs each
constexpr int kFt4Syms = 103;              // symbols of a frame as the device sees it (the ramps are not among them)
constexpr int kFt4Sync = 16;               // Costas symbols: four arrays of four
constexpr int kFt4Lag = kFt4StepsPerSym * (kFt4Syms - 1);   // 408: the last Costas symbol's step behind the frame's first
constexpr int kFt4EmitLag = kFt4Lag + kFt8Reach;            // 412: t0 is judged at step t0 + 412
constexpr int kFt4Hold = kFt4EmitLag + kFt8Reach + 1;       // 417: every rival of t0 has arrived once step t0 + 416 is complete
constexpr int kFt4Tones = 4;
constexpr int kFt4Data = 87;               // data symbols
constexpr int kFt4Bits = 2 * kFt4Data;     // 174 soft bits
constexpr int kFt4LlrMax = 4096;           // candidates of one pysdr_ft4_llr call
constexpr long long kFt4RingBytesMax = 1LL << 30;   // the spectrum ring [nk][TR][NB] float32

// The Costas arrays A = [0,1,3,2], B = [1,0,2,3], C = [2,3,1,0], D = [3,2,0,1], a nibble per symbol, A's first symbol
// lowest: expected tone of sync symbol n < 16, in frame order.  The Gray map [0,1,3,2] likewise.
PYSDR_FT8_HD constexpr int ft4_costas(int n) { return (int)((0x1023013232012310ULL >> (4 * n)) & 3ULL); }
PYSDR_FT8_HD constexpr int ft4_gray(int v) { return (int)((0x2310u >> (4 * v)) & 3u); }
// frame symbol of sync symbol n < 16 and of data symbol d < 87
PYSDR_FT8_HD constexpr int ft4_costas_sym(int n) { return 33 * (n / 4) + n % 4; }
PYSDR_FT8_HD constexpr int ft4_data_sym(int d) { return d < 29 ? 4 + d : (d < 58 ? 37 + (d - 29) : 70 + (d - 58)); }

// everything that follows from S, the row samples per symbol
template <int S>
struct Ft4Geom {
  static_assert(S == 48 || S == 72, "S is 48 or 72");
  static constexpr int kS = S;
  static constexpr int kNsub = S / 2;                 // decoders per row, one every baud / 2
  static constexpr int kNb = kNsub + 6;               // bins per row: decoder j uses bins j + 2 tone
  static constexpr int kNt = 4 * S;                   // twiddle table: one turn in steps of baud / 4
  static constexpr int kQs = S / 4;                   // outputs per step
  static constexpr int kTile = S;                     // outputs staged at once: four steps end in a whole tile
  static constexpr int kYp = 2 * S - 1;               // LDS: S - 1 earlier samples, then the tile
  // One row per workgroup: a tile's 4 steps x NB bins are 120 or 168 independent sums of S terms, 94 % and 88 % of 2 and
  // 3 waves.  The lanes of one step read one sample address (a broadcast), each its own twiddle.
  static constexpr int kItems = kFt4StepsPerSym * kNb;
  static constexpr int kThreads = (kItems + 63) / 64 * 64;
  static constexpr int kLdsBytes = kNt * 8 + kYp * 8; // tw, y
  // The index arithmetic of the kernel's tile walk, used by ft4.hip and walked by tests/ft4_plan.  LDS indices are into
  // the sample tile [kYp]; memory offsets are in complex samples from the row's first output of the call (the history
  // sits at -(S - 1) .. -1).
  static constexpr int kCarry = S - 1;                // samples in front of a tile: history, or the last tile's end
  PYSDR_FT8_HD static constexpr int carry_src(int hc) { return kTile + hc; }                          // LDS: the previous tile's last samples
  PYSDR_FT8_HD static constexpr int carry_dst(int hc) { return hc; }                                  // LDS
  PYSDR_FT8_HD static constexpr int hist_off(int hc) { return hc - (S - 1); }                         // memory: the row's history
  PYSDR_FT8_HD static constexpr int stage_dst(int c) { return S - 1 + c; }                            // LDS, c < kTile
  PYSDR_FT8_HD static constexpr int item_step(int k) { return k / kNb; }                              // item k < kItems: step of the tile
  PYSDR_FT8_HD static constexpr int item_bin(int k) { return k % kNb; }
  // e_first: the call-relative output that completes the call's first step, < QS except at the stream's start, where step 0
  // waits for S outputs (< S).  Step u of the call ends at e_first + QS u, four in a tile: the tile at i0 holds in place s
  // the step u = i0 / QS + s - e_first / QS (if 0 <= u < ns), and its window begins in the LDS at win
  PYSDR_FT8_HD static constexpr int tile_step(int i0, int e_first, int s) { return i0 / kQs + s - e_first / kQs; }
  PYSDR_FT8_HD static constexpr int win(int e_first, int s) { return e_first % kQs + kQs * s; }
  PYSDR_FT8_HD static constexpr int roll_src(int n_out, int j) { return n_out - (S - 1) + j; }        // memory, j < S - 1
  PYSDR_FT8_HD static constexpr int roll_dst(int j) { return j - (S - 1); }                           // memory
};
static_assert(Ft4Geom<48>::kCarry <= Ft4Geom<48>::kThreads && Ft4Geom<72>::kCarry <= Ft4Geom<72>::kThreads, "one thread per carried sample");
static_assert(72 - 1 <= kFt4Hpad && kFt4Hpad % 16 == 0, "the history fits its room");
static_assert(sizeof(pysdr_ft4_cfg) == sizeof(pysdr_ft8_cfg), "ft8_peak judges both");

constexpr bool ft4_s_ok(int S) { return S == 48 || S == 72; }
constexpr int ft4_threads(int S) { return S == 48 ? Ft4Geom<48>::kThreads : Ft4Geom<72>::kThreads; }
constexpr int ft4_lds_bytes(int S) { return S == 48 ? Ft4Geom<48>::kLdsBytes : Ft4Geom<72>::kLdsBytes; }

inline bool ft4_cfg_ok(const pysdr_ft4_cfg& c) {
  if (!(c.smin >= 0.f && c.smin <= FLT_MAX)) return false;          // finite, not negative
  if (c.hmin < 0 || c.hmin > kFt4Sync) return false;
  return c.pmax > 0.f && c.pmax <= kFt4PmaxMax;
}

// Most steps a call of max_out outputs completes, the events one decoder can emit in it (at least 5 steps apart: the peak
// rule is item 22's), and the ring depth in steps: item 22's argument with the hold of 417.
constexpr int ft4_steps_per_call(int max_out, int S) { return max_out / (S / 4) + 1; }
constexpr int ft4_event_cap(int max_out, int S) { return ft4_steps_per_call(max_out, S) / kFt8MinGap + 1; }
constexpr int ft4_ring_steps(int max_out, int S) { return kFt4Hold + 2 * ft4_steps_per_call(max_out, S); }

struct Ft4Plan {
  int S = 0, nsub = 0, nb = 0;
  int nfine = 0;       // decoders: nk nsub
  int cap = 0;         // event slots per decoder
  int groups = 0;      // workgroups of the spectrum kernel: one per row
  int ypitch = 0;      // row pitch of Y, complex samples: kFt4Hpad of history room, then the call's outputs
  int tr = 0;          // ring depth, steps
  long long ring_bytes = 0;
};

inline bool ft4_plan(int nk, int S, int max_out, const pysdr_ft4_cfg* cfg, Ft4Plan* p) {
  if (!ft4_s_ok(S) || nk < 1 || (long long)nk * (S / 2) > kFt4FineMax || max_out < 1 || max_out > kFt4MaxOutMax || !cfg || !ft4_cfg_ok(*cfg))
    return false;
  Ft4Plan q;
  q.S = S;
  q.nsub = S / 2;
  q.nb = q.nsub + 6;
  q.nfine = nk * q.nsub;
  q.cap = ft4_event_cap(max_out, S);
  q.groups = nk;
  q.ypitch = kFt4Hpad + ((max_out + 15) & ~15);
  q.tr = ft4_ring_steps(max_out, S);
  q.ring_bytes = (long long)nk * q.tr * q.nb * 4;
  if (q.ring_bytes > kFt4RingBytesMax) return false;
  *p = q;
  return true;
}

// A candidate (F, t0) of pysdr_ft4_llr with t_done steps complete: the whole frame is in, and its first step has not left
// the ring.
PYSDR_FT8_HD constexpr bool ft4_llr_ok(long long F, long long t0, long long t_done, int nfine, int tr) {
  return F >= 0 && F < nfine && t0 >= 0 && t0 + kFt4Lag < t_done && t_done - t0 <= tr;
}

// q_b mod NT as a non-negative number for bin b < NB of a row, q_b = 2 b - (NB - 1)
PYSDR_FT8_HD constexpr int ft4_qmod(int b, int S) { return ((2 * b - (S / 2 + 5)) + 4 * S) % (4 * S); }

// Step 1 for one bin of the step whose window begins at yw[0]: item 22's sum over this S.  Every float operation rounds on
// its own (-ffp-contract=off).  Returns P = |u|^2, 0 where it is not <= pmax.
template <int S>
PYSDR_FT8_HD inline float ft4_bin(const Ft8C* yw, const Ft8C* tw, int qm, float pmax) {
  constexpr int NT = Ft4Geom<S>::kNt;
  float ar = 0.f, ai = 0.f;
  int t = 0;
#pragma unroll 8
  for (int i = 0; i < S; ++i) {
    const Ft8C y = yw[i], w = tw[t];
    const float vr = y.x * w.x - y.y * w.y, vi = y.x * w.y + y.y * w.x;
    if (i == 0) { ar = vr; ai = vi; }
    else { ar = ar + vr; ai = ai + vi; }
    t += qm;
    if (t >= NT) t -= NT;
  }
  const float pw = ar * ar + ai * ai;
  return pw <= pmax ? pw : 0.f;
}

// Step 2 for decoder j of a row whose ring is ring[tr][nb]: slot0 = t0 mod tr.  The 16 Costas symbols in frame order, each
// against its own block's array.
PYSDR_FT8_HD inline Ft8Score ft4_sync(const float* ring, int tr, int nb, int slot0, int j) {
  float sig = 0.f, tot = 0.f;
  int hits = 0;
  for (int n = 0; n < kFt4Sync; ++n) {
    const int c = ft4_costas(n);
    int sl = slot0 + kFt4StepsPerSym * ft4_costas_sym(n);
    if (sl >= tr) sl -= tr;                                // 4 * 102 < tr
    const float* p = ring + (size_t)sl * (size_t)nb + j;
    const float e = p[2 * c];
    sig = sig + e;
    float r = p[0];
    for (int tone = 1; tone < kFt4Tones; ++tone) r = r + p[2 * tone];
    tot = tot + r;
    bool hit = true;
    for (int tone = 0; tone < kFt4Tones; ++tone)
      if (tone != c && !(e > p[2 * tone])) hit = false;
    hits += hit ? 1 : 0;
  }
  const float den = tot - sig;
  Ft8Score out;
  out.score = den > 0.f ? (3.f * sig) / den : 0.f;
  out.hits = hits;
  return out;
}

// Step 3 is item 22's: the same rule over the same nine kept scores, judged by this skimmer's settings.
PYSDR_FT8_HD inline bool ft4_peak(const float* sc, const int32_t* hi, long long stride, long long tc, const pysdr_ft4_cfg& c) {
  pysdr_ft8_cfg k{};
  k.smin = c.smin; k.hmin = c.hmin; k.pmax = c.pmax;
  return ft8_peak(sc, hi, stride, tc, k);
}

// Soft bit i < 174 of the frame whose first step sits in slot0 of the row's ring, decoder j: data symbol i / 2, bit 2, 1
// of its value; max over the values with the bit minus max over those without.
PYSDR_FT8_HD inline float ft4_llr_bit(const float* ring, int tr, int nb, int slot0, int j, int i) {
  const int d = i / 2, mask = 2 >> (i % 2);
  const int sl = (slot0 + kFt4StepsPerSym * ft4_data_sym(d)) % tr;
  const float* p = ring + (size_t)sl * (size_t)nb + j;
  float m1 = 0.f, m0 = 0.f;
  bool f1 = true, f0 = true;
  for (int v = 0; v < kFt4Tones; ++v) {
    const float pv = p[2 * ft4_gray(v)];
    if (v & mask) { m1 = (f1 || pv > m1) ? pv : m1; f1 = false; }
    else { m0 = (f0 || pv > m0) ? pv : m0; f0 = false; }
  }
  return m1 - m0;
}

// ---- kernel arguments and the launches (ft4.hip) ---------------------------------------------------------------------
struct Ft4Args {
  Ft8C* y;                 // Y + kFt4Hpad: y[a * ypitch + i] = output i of this call, i >= -(S - 1) the row's history
  long long ypitch;
  int n_out, nk, cap, nfine;
  int ns;                  // steps this call completes
  int e_first;             // call-relative output that completes the first of them, < QS (< S at the stream's start)
  int tr;                  // ring depth
  long long t_first;       // absolute index of the call's first step
  pysdr_ft4_cfg cfg;
  const Ft8C* tw;          // [NT]
  float* ring;             // [nk][tr][NB]
  float* sc;               // [9][nfine]
  int32_t* hi;             // [9][nfine]
  int32_t* events;         // [nfine][cap][2]
  int32_t* counts;         // [nfine]
};

struct Ft4LlrArgs {
  const float* ring;
  int tr, nb, nsub, n;
  const int32_t* cand;     // [n][2]: fine row F, slot0 = t0 mod tr
  float* out;              // [n][174]
};

}  // namespace pysdr
