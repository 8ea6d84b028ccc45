// The FT8 skimmer's pure half: settings and their rules, the event cap and words, the ring depth,
// the workgroup's geometry, LDS budget and the index arithmetic of its tile walk, and the steps themselves -- one bin of
// one step's spectrum, the Costas score of one decoder, the peak rule, one soft bit -- the very code the kernels (ft8.hip)
// step with, the host half (api_ft8.hip) plans with and tests/ft8_plan/plan_main.cpp runs on the CPU.
// Plain C++: nothing here calls the HIP runtime, and the only trace of the device is the function qualifier below.
#pragma once

#include <cfloat>
#include <cstddef>
#include <cstdint>

#include "../../include/pysdr_hip.h"

#if defined(__HIPCC__)
#define PYSDR_FT8_HD __host__ __device__
#else
#define PYSDR_FT8_HD
#endif

namespace pysdr {

constexpr int kFt8Hpad = 96;               // complex samples kept in front of a row of Y: the history's room, >= S - 1
constexpr int kFt8FineMax = 1 << 18;       // decoders: nk NSUB
constexpr int kFt8MaxOutMax = 1 << 20;     // the event word holds the step within the call above bit 5
constexpr float kFt8PmaxMax = 1.0e18f;     // 147 powers <= pmax sum far below FLT_MAX
constexpr int kFt8StepsPerSym = 4;         // steps per symbol: QS = S / 4 outputs each
constexpr int kFt8Syms = 79;               // symbols of a frame
constexpr int kFt8Lag = kFt8StepsPerSym * (kFt8Syms - 1);   // 312: the last Costas symbol's step behind the frame's first
constexpr int kFt8Reach = 4;               // steps to either side a peak beats
constexpr int kFt8Keep = 2 * kFt8Reach + 1;   // 9 scores and hit counts per decoder
constexpr int kFt8EmitLag = kFt8Lag + kFt8Reach;          // 316: t0 is judged at step t0 + 316
constexpr int kFt8Hold = kFt8EmitLag + kFt8Reach + 1;     // 321: every rival of t0 has arrived once step t0 + 320 is complete
constexpr int kFt8MinGap = kFt8Reach + 1;  // two events of a decoder are at least 5 steps apart
constexpr int kFt8Tones = 8;
constexpr int kFt8Data = 58;               // data symbols
constexpr int kFt8Bits = 3 * kFt8Data;     // 174 soft bits
constexpr int kFt8EventWords = 2;          // (step within the call) << 5 | hits, the score's bits
constexpr int kFt8LlrMax = 4096;           // candidates of one pysdr_ft8_llr call
constexpr long long kFt8RingBytesMax = 1LL << 30;   // the spectrum ring [nk][TR][NB] float32

// Costas array [3,1,4,0,6,5,2] and Gray map [0,1,3,2,5,6,4,7], a nibble each, lowest first
PYSDR_FT8_HD constexpr int ft8_costas(int k) { return (int)((0x2560413u >> (4 * k)) & 7u); }
PYSDR_FT8_HD constexpr int ft8_gray(int v) { return (int)((0x74652310u >> (4 * v)) & 7u); }
// frame symbol of Costas symbol n < 21 and of data symbol d < 58
PYSDR_FT8_HD constexpr int ft8_costas_sym(int n) { return 36 * (n / 7) + n % 7; }
PYSDR_FT8_HD constexpr int ft8_data_sym(int d) { return d < 29 ? 7 + d : 43 + (d - 29); }

// everything that follows from S, the row samples per symbol
template <int S>
struct Ft8Geom {
  static_assert(S == 64 || S == 96, "S is 64 or 96");
  static constexpr int kS = S;
  static constexpr int kNsub = S / 2;                 // decoders per row, one every baud / 2
  static constexpr int kNb = kNsub + 14;              // bins per row: decoder j uses bins j + 2 tone
  static constexpr int kNt = 4 * S;                   // twiddle table: one turn in steps of baud / 4
  static constexpr int kQs = S / 4;                   // outputs per step
  static constexpr int kTile = S;                     // outputs staged at once: four steps end in a whole tile
  static constexpr int kYp = 2 * S - 1;               // LDS: S - 1 earlier samples, then the tile
  // One row per workgroup: a tile's 4 steps x NB bins are 184 or 248 independent sums of S terms, 96 % and 97 % of 3 and
  // 4 waves.  The lanes of one step read one sample address (a broadcast), each its own twiddle.
  static constexpr int kItems = kFt8StepsPerSym * kNb;
  static constexpr int kThreads = (kItems + 63) / 64 * 64;
  static constexpr int kLdsBytes = kNt * 8 + kYp * 8; // tw, y
  // The index arithmetic of the kernel's tile walk, used by ft8.hip and walked by tests/ft8_plan.  LDS indices are into
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
  // waits for S outputs (< S).  The steps end QS apart, so step u of the call ends at e_first + QS u, four in a tile: the
  // tile at i0 holds in place s the step u = i0 / QS + s - e_first / QS (if 0 <= u < ns), and its window begins in the LDS at
  PYSDR_FT8_HD static constexpr int tile_step(int i0, int e_first, int s) { return i0 / kQs + s - e_first / kQs; }
  PYSDR_FT8_HD static constexpr int win(int e_first, int s) { return e_first % kQs + kQs * s; }
  PYSDR_FT8_HD static constexpr int roll_src(int n_out, int j) { return n_out - (S - 1) + j; }        // memory, j < S - 1
  PYSDR_FT8_HD static constexpr int roll_dst(int j) { return j - (S - 1); }                           // memory
};
static_assert(Ft8Geom<64>::kCarry <= Ft8Geom<64>::kThreads && Ft8Geom<96>::kCarry <= Ft8Geom<96>::kThreads, "one thread per carried sample");
static_assert(96 - 1 <= kFt8Hpad && kFt8Hpad % 16 == 0, "the history fits its room");

constexpr bool ft8_s_ok(int S) { return S == 64 || S == 96; }
constexpr int ft8_threads(int S) { return S == 64 ? Ft8Geom<64>::kThreads : Ft8Geom<96>::kThreads; }
constexpr int ft8_lds_bytes(int S) { return S == 64 ? Ft8Geom<64>::kLdsBytes : Ft8Geom<96>::kLdsBytes; }

inline bool ft8_cfg_ok(const pysdr_ft8_cfg& c) {
  if (!(c.smin >= 0.f && c.smin <= FLT_MAX)) return false;          // finite, not negative
  if (c.hmin < 0 || c.hmin > 21) return false;
  return c.pmax > 0.f && c.pmax <= kFt8PmaxMax;
}

// steps complete once n_abs outputs of a row exist: step t needs outputs QS t .. QS t + S - 1
PYSDR_FT8_HD constexpr unsigned long long ft8_steps_done(unsigned long long n_abs, int S) {
  return n_abs >= (unsigned long long)S ? (n_abs - (unsigned long long)S) / (unsigned long long)(S / 4) + 1ULL : 0ULL;
}
// Most steps a call of max_out outputs completes, and most events one decoder can emit in it: two events of a decoder
// are peaks over 4 steps to either side, so at least 5 steps apart.
constexpr int ft8_steps_per_call(int max_out, int S) { return max_out / (S / 4) + 1; }
constexpr int ft8_event_cap(int max_out, int S) { return ft8_steps_per_call(max_out, S) / kFt8MinGap + 1; }
// Ring depth in steps.  An event t0 is released by the host at the end of the first call that completes step t0 + 320;
// that call began with at most t0 + 320 steps done and adds at most a call's steps; and the frame must outlive one whole
// call behind the call that emitted t0 (at step t0 + 316): both hold with 321 + 2 calls' steps.
constexpr int ft8_ring_steps(int max_out, int S) { return kFt8Hold + 2 * ft8_steps_per_call(max_out, S); }

struct Ft8Plan {
  int S = 0, nsub = 0, nb = 0;
  int nfine = 0;       // decoders: nk nsub
  int cap = 0;         // event slots per decoder
  int groups = 0;      // workgroups of the spectrum kernel: one per row
  int ypitch = 0;      // row pitch of Y, complex samples: kFt8Hpad of history room, then the call's outputs
  int tr = 0;          // ring depth, steps
  long long ring_bytes = 0;
};

inline bool ft8_plan(int nk, int S, int max_out, const pysdr_ft8_cfg* cfg, Ft8Plan* p) {
  if (!ft8_s_ok(S) || nk < 1 || (long long)nk * (S / 2) > kFt8FineMax || max_out < 1 || max_out > kFt8MaxOutMax || !cfg || !ft8_cfg_ok(*cfg))
    return false;
  Ft8Plan q;
  q.S = S;
  q.nsub = S / 2;
  q.nb = q.nsub + 14;
  q.nfine = nk * q.nsub;
  q.cap = ft8_event_cap(max_out, S);
  q.groups = nk;
  q.ypitch = kFt8Hpad + ((max_out + 15) & ~15);
  q.tr = ft8_ring_steps(max_out, S);
  q.ring_bytes = (long long)nk * q.tr * q.nb * 4;
  if (q.ring_bytes > kFt8RingBytesMax) return false;
  *p = q;
  return true;
}

// the event words: (step within the call at which t0 was judged) << 5 | hits, then the score's bits; t0 = the call's
// first step + that index - 316
PYSDR_FT8_HD constexpr int32_t ft8_pack(int u, int hits) { return (int32_t)(((uint32_t)u << 5) | (uint32_t)hits); }
PYSDR_FT8_HD constexpr int ft8_event_step(int32_t w) { return (int)((uint32_t)w >> 5); }
PYSDR_FT8_HD constexpr int ft8_event_hits(int32_t w) { return (int)((uint32_t)w & 31u); }

// A candidate (F, t0) of pysdr_ft8_llr with t_done steps complete: the whole frame is in, and its first step has not left
// the ring.
PYSDR_FT8_HD constexpr bool ft8_llr_ok(long long F, long long t0, long long t_done, int nfine, int tr) {
  return F >= 0 && F < nfine && t0 >= 0 && t0 + kFt8Lag < t_done && t_done - t0 <= tr;
}

struct alignas(8) Ft8C { float x, y; };   // a complex sample as the channelizer stores it

// q_b mod NT as a non-negative number for bin b < NB of a row, q_b = 2 b - (NB - 1)
PYSDR_FT8_HD constexpr int ft8_qmod(int b, int S) { return ((2 * b - (S / 2 + 13)) + 4 * S) % (4 * S); }

// Step 1 of the definition for one bin of the step whose window begins at yw[0]: sum_{i<S} yw[i] tw[(q i) mod NT], i
// ascending, qm = q mod NT.  Every float operation rounds on its own (-ffp-contract=off).  Returns P = |u|^2, 0 where it
// is not <= pmax.
template <int S>
PYSDR_FT8_HD inline float ft8_bin(const Ft8C* yw, const Ft8C* tw, int qm, float pmax) {
  constexpr int NT = Ft8Geom<S>::kNt;
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

struct Ft8Score { float score; int32_t hits; };

// Step 2 for decoder j of a row whose ring is ring[tr][nb]: slot0 = t0 mod tr.  The 21 Costas symbols in order.
PYSDR_FT8_HD inline Ft8Score ft8_sync(const float* ring, int tr, int nb, int slot0, int j) {
  float sig = 0.f, tot = 0.f;
  int hits = 0;
  for (int n = 0; n < 21; ++n) {
    const int c = ft8_costas(n % 7);
    int sl = slot0 + kFt8StepsPerSym * ft8_costas_sym(n);
    if (sl >= tr) sl -= tr;                                // 4 * 78 < tr
    const float* p = ring + (size_t)sl * (size_t)nb + j;
    const float e = p[2 * c];
    sig = sig + e;
    float r = p[0];
    for (int tone = 1; tone < 7; ++tone) r = r + p[2 * tone];
    tot = tot + r;
    bool hit = true;
    for (int tone = 0; tone < kFt8Tones; ++tone)
      if (tone != c && !(e > p[2 * tone])) hit = false;
    hits += hit ? 1 : 0;
  }
  const float den = tot - sig;
  Ft8Score out;
  out.score = den > 0.f ? (6.f * sig) / den : 0.f;
  out.hits = hits;
  return out;
}

// Step 3: is tc an event?  sc and hi hold the decoder's last 9 scores and hit counts, that of step t at index
// (t mod 9) * stride; score[tc + 4] is the newest.
PYSDR_FT8_HD inline bool ft8_peak(const float* sc, const int32_t* hi, long long stride, long long tc, const pysdr_ft8_cfg& c) {
  const int s0 = (int)(tc % kFt8Keep);
  const float v = sc[s0 * stride];
  if (!(v >= c.smin) || hi[s0 * stride] < c.hmin) return false;
  for (int d = 1; d <= kFt8Reach; ++d) {
    if (tc - d >= 0 && !(v > sc[((s0 + kFt8Keep - d) % kFt8Keep) * stride])) return false;
    if (!(v >= sc[((s0 + d) % kFt8Keep) * stride])) return false;
  }
  return true;
}

// Soft bit i < 174 of the frame whose first step sits in slot0 of the row's ring, decoder j: data symbol i / 3, bit
// 4, 2, 1 of its value; max over the values with the bit minus max over those without.
PYSDR_FT8_HD inline float ft8_llr_bit(const float* ring, int tr, int nb, int slot0, int j, int i) {
  const int d = i / 3, mask = 4 >> (i % 3);
  const int sl = (slot0 + kFt8StepsPerSym * ft8_data_sym(d)) % tr;
  const float* p = ring + (size_t)sl * (size_t)nb + j;
  float m1 = 0.f, m0 = 0.f;
  bool f1 = true, f0 = true;
  for (int v = 0; v < 8; ++v) {
    const float pv = p[2 * ft8_gray(v)];
    if (v & mask) { m1 = (f1 || pv > m1) ? pv : m1; f1 = false; }
    else { m0 = (f0 || pv > m0) ? pv : m0; f0 = false; }
  }
  return m1 - m0;
}

// ---- kernel arguments and the launches (ft8.hip) ---------------------------------------------------------------------
struct Ft8Args {
  Ft8C* y;                 // Y + kFt8Hpad: y[a * ypitch + i] = output i of this call, i >= -(S - 1) the row's history
  long long ypitch;
  int n_out, nk, cap, nfine;
  int ns;                  // steps this call completes
  int e_first;             // call-relative output that completes the first of them, < QS (< S at the stream's start)
  int tr;                  // ring depth
  long long t_first;       // absolute index of the call's first step
  pysdr_ft8_cfg cfg;
  const Ft8C* tw;          // [NT]
  float* ring;             // [nk][tr][NB]
  float* sc;               // [9][nfine]
  int32_t* hi;             // [9][nfine]
  int32_t* events;         // [nfine][cap][2]
  int32_t* counts;         // [nfine]
};

struct Ft8LlrArgs {
  const float* ring;
  int tr, nb, nsub, n;
  const int32_t* cand;     // [n][2]: fine row F, slot0 = t0 mod tr
  float* out;              // [n][174]
};

}  // namespace pysdr
