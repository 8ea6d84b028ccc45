// The FT8 and FT4 skimmers' pure half: what a mode is -- two traits structs, Ft8Mode and
// Ft4Mode, and nothing else is written per mode -- and, once for both, settings and their rules, the event cap and words,
// the ring depth, the workgroup's geometry, LDS budget and the index arithmetic of its tile walk, and the steps themselves
// -- one bin of one step's spectrum, the Costas score of one decoder, the peak rule, one soft bit -- the very code the
// kernels (ft.hip) step with, the host half (api_ft.hip) plans with and tests/ft_plan/plan_main.cpp runs on the CPU.
// Plain C++: nothing here calls the HIP runtime, and the only trace of the device is the function qualifier below.
#pragma once

#include <cfloat>
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "../../include/pysdr_hip.h"

#if defined(__HIPCC__)
#define PYSDR_FT_HD __host__ __device__
#else
#define PYSDR_FT_HD
#endif

namespace pysdr {

// ---- what both modes share ---------------------------------------------------------------------------------------------
constexpr int kFtFineMax = 1 << 18;        // decoders: nk NSUB
constexpr int kFtMaxOutMax = 1 << 20;      // the event word holds the step within the call above bit 5
constexpr float kFtPmaxMax = 1.0e18f;      // 147 (FT4: 64) powers <= pmax sum far below FLT_MAX
constexpr int kFtStepsPerSym = 4;          // steps per symbol: QS = S / 4 outputs each
constexpr int kFtReach = 4;                // steps to either side a peak beats
constexpr int kFtKeep = 2 * kFtReach + 1;  // 9 scores and hit counts per decoder
constexpr int kFtMinGap = kFtReach + 1;    // two events of a decoder are at least 5 steps apart
constexpr int kFtBits = 174;               // soft bits of a frame: the LDPC codeword
constexpr int kFtEventWords = 2;           // (step within the call) << 5 | hits, the score's bits
constexpr int kFtLlrMax = 4096;            // candidates of one pysdr_*_llr call
constexpr long long kFtRingBytesMax = 1LL << 30;   // the spectrum ring [nk][TR][NB] float32

// The names a mode goes by outside this file: the decoder's source of soft bits (ldpc.hip, osd.hip) and the frame report's
// mode (report.hip), which is the public one.
enum LdpcSource { kLdpcFromBuffer = 0, kLdpcFromFt8Ring = 1, kLdpcFromFt4Ring = 2 };
enum ReportMode { kReportFt8 = PYSDR_REPORT_FT8, kReportFt4 = PYSDR_REPORT_FT4 };

// The settings: pysdr_ft8_cfg and pysdr_ft4_cfg are this layout, and api_ft.hip reads either as it.
struct FtCfg {
  float smin;
  int32_t hmin;
  float pmax;
};
static_assert(sizeof(pysdr_ft8_cfg) == sizeof(FtCfg) && offsetof(pysdr_ft8_cfg, smin) == offsetof(FtCfg, smin) &&
              offsetof(pysdr_ft8_cfg, hmin) == offsetof(FtCfg, hmin) && offsetof(pysdr_ft8_cfg, pmax) == offsetof(FtCfg, pmax), "one layout");
static_assert(sizeof(pysdr_ft4_cfg) == sizeof(FtCfg) && offsetof(pysdr_ft4_cfg, smin) == offsetof(FtCfg, smin) &&
              offsetof(pysdr_ft4_cfg, hmin) == offsetof(FtCfg, hmin) && offsetof(pysdr_ft4_cfg, pmax) == offsetof(FtCfg, pmax), "one layout");

// ---- the modes -----------------------------------------------------------------------------------------------------------
// FT8: 8-FSK, 79 symbols, the Costas array [3,1,4,0,6,5,2] at symbols 0, 36 and 72.  The array has seven tones: the sync
// score's denominator sums tones 0 .. 6, the hit test runs over all eight.
struct Ft8Mode {
  static constexpr int kS0 = 64, kS1 = 96;   // row samples per symbol
  static constexpr int kHpad = 96;           // complex samples kept in front of a row of Y: the history's room, >= S - 1
  static constexpr int kSyms = 79;           // symbols of a frame
  static constexpr int kSync = 21;           // Costas symbols
  static constexpr int kTones = 8;
  static constexpr int kSyncTones = 7;       // tones summed in the sync score's denominator
  static constexpr int kBitsPerSym = 3;
  static constexpr int kData = 58;           // data symbols
  static constexpr const char* kName = "ft8";
  static constexpr LdpcSource kLdpcSource = kLdpcFromFt8Ring;
  static constexpr ReportMode kReportMode = kReportFt8;
  // Costas array [3,1,4,0,6,5,2] and Gray map [0,1,3,2,5,6,4,7], a nibble each, lowest first
  PYSDR_FT_HD static constexpr int costas(int k) { return (int)((0x2560413u >> (4 * k)) & 7u); }
  PYSDR_FT_HD static constexpr int gray(int v) { return (int)((0x74652310u >> (4 * v)) & 7u); }
  // expected tone and frame symbol of Costas symbol n < 21, frame symbol of data symbol d < 58
  PYSDR_FT_HD static constexpr int sync_tone(int n) { return costas(n % 7); }
  PYSDR_FT_HD static constexpr int costas_sym(int n) { return 36 * (n / 7) + n % 7; }
  PYSDR_FT_HD static constexpr int data_sym(int d) { return d < 29 ? 7 + d : 43 + (d - 29); }
};

// FT4: 4-GFSK, 103 symbols as the device sees it (the ramps are not among them), four different Costas arrays of four at
// symbols 0, 33, 66 and 99.
struct Ft4Mode {
  static constexpr int kS0 = 48, kS1 = 72;
  static constexpr int kHpad = 80;
  static constexpr int kSyms = 103;
  static constexpr int kSync = 16;           // Costas symbols: four arrays of four
  static constexpr int kTones = 4;
  static constexpr int kSyncTones = 4;
  static constexpr int kBitsPerSym = 2;
  static constexpr int kData = 87;
  static constexpr const char* kName = "ft4";
  static constexpr LdpcSource kLdpcSource = kLdpcFromFt4Ring;
  static constexpr ReportMode kReportMode = kReportFt4;
  // The Costas arrays A = [0,1,3,2], B = [1,0,2,3], C = [2,3,1,0], D = [3,2,0,1], a nibble per symbol, A's first symbol
  // lowest: expected tone of sync symbol n < 16, in frame order.  The Gray map [0,1,3,2] likewise.
  PYSDR_FT_HD static constexpr int costas(int n) { return (int)((0x1023013232012310ULL >> (4 * n)) & 3ULL); }
  PYSDR_FT_HD static constexpr int gray(int v) { return (int)((0x2310u >> (4 * v)) & 3u); }
  // expected tone and frame symbol of sync symbol n < 16, frame symbol of data symbol d < 87
  PYSDR_FT_HD static constexpr int sync_tone(int n) { return costas(n); }
  PYSDR_FT_HD static constexpr int costas_sym(int n) { return 33 * (n / 4) + n % 4; }
  PYSDR_FT_HD static constexpr int data_sym(int d) { return d < 29 ? 4 + d : (d < 58 ? 37 + (d - 29) : 70 + (d - 58)); }
};

// the traits of the mode a source of soft bits or a report mode names
template <int SRC> using FtRingMode = std::conditional_t<SRC == Ft4Mode::kLdpcSource, Ft4Mode, Ft8Mode>;
template <int MODE> using FtReportMode = std::conditional_t<MODE == Ft4Mode::kReportMode, Ft4Mode, Ft8Mode>;

// what follows from a mode's numbers
template <class Mode> constexpr int kFtLag = kFtStepsPerSym * (Mode::kSyms - 1);   // the last Costas symbol's step behind the frame's first
template <class Mode> constexpr int kFtEmitLag = kFtLag<Mode> + kFtReach;           // t0 is judged at step t0 + this
template <class Mode> constexpr int kFtHold = kFtEmitLag<Mode> + kFtReach + 1;      // every rival of t0 has arrived once step t0 + this - 1 is complete
template <class Mode> constexpr int kFtExtra = 2 * (Mode::kTones - 1);              // bins of a row beyond its decoders: decoder j uses bins j + 2 tone
template <class Mode> constexpr float kFtScore = (float)(Mode::kSyncTones - 1);     // the other tones of the sync score, per signal tone
static_assert(kFtLag<Ft8Mode> == 312 && kFtEmitLag<Ft8Mode> == 316 && kFtHold<Ft8Mode> == 321 && kFtExtra<Ft8Mode> == 14 && kFtScore<Ft8Mode> == 6.f, "FT8");
static_assert(kFtLag<Ft4Mode> == 408 && kFtEmitLag<Ft4Mode> == 412 && kFtHold<Ft4Mode> == 417 && kFtExtra<Ft4Mode> == 6 && kFtScore<Ft4Mode> == 3.f, "FT4");
static_assert(Ft8Mode::kBitsPerSym * Ft8Mode::kData == kFtBits && Ft4Mode::kBitsPerSym * Ft4Mode::kData == kFtBits, "174 soft bits");
static_assert(Ft8Mode::kSync + Ft8Mode::kData == Ft8Mode::kSyms && Ft4Mode::kSync + Ft4Mode::kData == Ft4Mode::kSyms, "a frame's symbols");
static_assert((1 << Ft8Mode::kBitsPerSym) == Ft8Mode::kTones && (1 << Ft4Mode::kBitsPerSym) == Ft4Mode::kTones, "a tone per value");

// everything that follows from S, the row samples per symbol
template <class Mode, int S>
struct FtGeom {
  static_assert(S == Mode::kS0 || S == Mode::kS1, "S is one of the mode's two");
  static constexpr int kS = S;
  static constexpr int kNsub = S / 2;                 // decoders per row, one every baud / 2
  static constexpr int kNb = kNsub + kFtExtra<Mode>;  // bins per row: decoder j uses bins j + 2 tone
  static constexpr int kNt = 4 * S;                   // twiddle table: one turn in steps of baud / 4
  static constexpr int kQs = S / 4;                   // outputs per step
  static constexpr int kTile = S;                     // outputs staged at once: four steps end in a whole tile
  static constexpr int kYp = 2 * S - 1;               // LDS: S - 1 earlier samples, then the tile
  // One row per workgroup: a tile's 4 steps x NB bins are independent sums of S terms -- FT8: 184 or 248, 96 % and 97 % of
  // 3 and 4 waves; FT4: 120 or 168, 94 % and 88 % of 2 and 3 waves.  The lanes of one step read one sample address (a
  // broadcast), each its own twiddle.
  static constexpr int kItems = kFtStepsPerSym * kNb;
  static constexpr int kThreads = (kItems + 63) / 64 * 64;
  static constexpr int kLdsBytes = kNt * 8 + kYp * 8; // tw, y
  // The index arithmetic of the kernel's tile walk, used by ft.hip and walked by tests/ft_plan.  LDS indices are into the
  // sample tile [kYp]; memory offsets are in complex samples from the row's first output of the call (the history sits at
  // -(S - 1) .. -1).
  static constexpr int kCarry = S - 1;                // samples in front of a tile: history, or the last tile's end
  PYSDR_FT_HD static constexpr int carry_src(int hc) { return kTile + hc; }                          // LDS: the previous tile's last samples
  PYSDR_FT_HD static constexpr int carry_dst(int hc) { return hc; }                                  // LDS
  PYSDR_FT_HD static constexpr int hist_off(int hc) { return hc - (S - 1); }                         // memory: the row's history
  PYSDR_FT_HD static constexpr int stage_dst(int c) { return S - 1 + c; }                            // LDS, c < kTile
  PYSDR_FT_HD static constexpr int item_step(int k) { return k / kNb; }                              // item k < kItems: step of the tile
  PYSDR_FT_HD static constexpr int item_bin(int k) { return k % kNb; }
  // e_first: the call-relative output that completes the call's first step, < QS except at the stream's start, where step 0
  // waits for S outputs (< S).  The steps end QS apart, so step u of the call ends at e_first + QS u, four in a tile: the
  // tile at i0 holds in place s the step u = i0 / QS + s - e_first / QS (if 0 <= u < ns), and its window begins in the LDS at
  PYSDR_FT_HD static constexpr int tile_step(int i0, int e_first, int s) { return i0 / kQs + s - e_first / kQs; }
  PYSDR_FT_HD static constexpr int win(int e_first, int s) { return e_first % kQs + kQs * s; }
  PYSDR_FT_HD static constexpr int roll_src(int n_out, int j) { return n_out - (S - 1) + j; }        // memory, j < S - 1
  PYSDR_FT_HD static constexpr int roll_dst(int j) { return j - (S - 1); }                           // memory
  static_assert(kCarry <= kThreads, "one thread per carried sample");
  static_assert(S - 1 <= Mode::kHpad && Mode::kHpad % 16 == 0, "the history fits its room");
};

template <class Mode> constexpr bool ft_s_ok(int S) { return S == Mode::kS0 || S == Mode::kS1; }
template <class Mode> constexpr int ft_threads(int S) { return S == Mode::kS0 ? FtGeom<Mode, Mode::kS0>::kThreads : FtGeom<Mode, Mode::kS1>::kThreads; }
template <class Mode> constexpr int ft_lds_bytes(int S) { return S == Mode::kS0 ? FtGeom<Mode, Mode::kS0>::kLdsBytes : FtGeom<Mode, Mode::kS1>::kLdsBytes; }

template <class Mode>
inline bool ft_cfg_ok(const FtCfg& c) {
  if (!(c.smin >= 0.f && c.smin <= FLT_MAX)) return false;          // finite, not negative
  if (c.hmin < 0 || c.hmin > Mode::kSync) return false;
  return c.pmax > 0.f && c.pmax <= kFtPmaxMax;
}

// steps complete once n_abs outputs of a row exist: step t needs outputs QS t .. QS t + S - 1
PYSDR_FT_HD constexpr unsigned long long ft_steps_done(unsigned long long n_abs, int S) {
  return n_abs >= (unsigned long long)S ? (n_abs - (unsigned long long)S) / (unsigned long long)(S / 4) + 1ULL : 0ULL;
}
// Most steps a call of max_out outputs completes, and most events one decoder can emit in it: two events of a decoder
// are peaks over 4 steps to either side, so at least 5 steps apart.
constexpr int ft_steps_per_call(int max_out, int S) { return max_out / (S / 4) + 1; }
constexpr int ft_event_cap(int max_out, int S) { return ft_steps_per_call(max_out, S) / kFtMinGap + 1; }
// Ring depth in steps.  An event t0 is released by the host at the end of the first call that completes step t0 + hold - 1
// (320, FT4: 416); that call began with at most that many steps done and adds at most a call's steps; and the frame must
// outlive one whole call behind the call that emitted t0 (at step t0 + 316, FT4: 412): both hold with the hold + 2 calls'
// steps.
template <class Mode> constexpr int ft_ring_steps(int max_out, int S) { return kFtHold<Mode> + 2 * ft_steps_per_call(max_out, S); }

struct FtPlan {
  int S = 0, nsub = 0, nb = 0;
  int nfine = 0;       // decoders: nk nsub
  int cap = 0;         // event slots per decoder
  int groups = 0;      // workgroups of the spectrum kernel: one per row
  int ypitch = 0;      // row pitch of Y, complex samples: the mode's kHpad of history room, then the call's outputs
  int tr = 0;          // ring depth, steps
  long long ring_bytes = 0;
};

template <class Mode>
inline bool ft_plan(int nk, int S, int max_out, const FtCfg* cfg, FtPlan* p) {
  if (!ft_s_ok<Mode>(S) || nk < 1 || (long long)nk * (S / 2) > kFtFineMax || max_out < 1 || max_out > kFtMaxOutMax || !cfg || !ft_cfg_ok<Mode>(*cfg))
    return false;
  FtPlan q;
  q.S = S;
  q.nsub = S / 2;
  q.nb = q.nsub + kFtExtra<Mode>;
  q.nfine = nk * q.nsub;
  q.cap = ft_event_cap(max_out, S);
  q.groups = nk;
  q.ypitch = Mode::kHpad + ((max_out + 15) & ~15);
  q.tr = ft_ring_steps<Mode>(max_out, S);
  q.ring_bytes = (long long)nk * q.tr * q.nb * 4;
  if (q.ring_bytes > kFtRingBytesMax) return false;
  *p = q;
  return true;
}

// the event words: (step within the call at which t0 was judged) << 5 | hits, then the score's bits; t0 = the call's
// first step + that index - the mode's emit lag
PYSDR_FT_HD constexpr int32_t ft_pack(int u, int hits) { return (int32_t)(((uint32_t)u << 5) | (uint32_t)hits); }
PYSDR_FT_HD constexpr int ft_event_step(int32_t w) { return (int)((uint32_t)w >> 5); }
PYSDR_FT_HD constexpr int ft_event_hits(int32_t w) { return (int)((uint32_t)w & 31u); }

// A candidate (F, t0) of pysdr_*_llr with t_done steps complete: the whole frame is in, and its first step has not left
// the ring.
template <class Mode>
PYSDR_FT_HD constexpr bool ft_llr_ok(long long F, long long t0, long long t_done, int nfine, int tr) {
  return F >= 0 && F < nfine && t0 >= 0 && t0 + kFtLag<Mode> < t_done && t_done - t0 <= tr;
}

struct alignas(8) FtC { float x, y; };   // a complex sample as the channelizer stores it

// q_b mod NT as a non-negative number for bin b < NB of a row, q_b = 2 b - (NB - 1)
template <class Mode>
PYSDR_FT_HD constexpr int ft_qmod(int b, int S) { return ((2 * b - (S / 2 + (kFtExtra<Mode> - 1))) + 4 * S) % (4 * S); }

// Step 1 of the definition for one bin of the step whose window begins at yw[0]: sum_{i<S} yw[i] tw[(q i) mod NT], i
// ascending, qm = q mod NT, NT = 4 S.  Every float operation rounds on its own (-ffp-contract=off).  Returns P = |u|^2, 0
// where it is not <= pmax.
template <int S>
PYSDR_FT_HD inline float ft_bin(const FtC* yw, const FtC* tw, int qm, float pmax) {
  constexpr int NT = 4 * S;
  float ar = 0.f, ai = 0.f;
  int t = 0;
#pragma unroll 8
  for (int i = 0; i < S; ++i) {
    const FtC y = yw[i], w = tw[t];
    const float vr = y.x * w.x - y.y * w.y, vi = y.x * w.y + y.y * w.x;
    if (i == 0) { ar = vr; ai = vi; }
    else { ar = ar + vr; ai = ai + vi; }
    t += qm;
    if (t >= NT) t -= NT;
  }
  const float pw = ar * ar + ai * ai;
  return pw <= pmax ? pw : 0.f;
}

struct FtScore { float score; int32_t hits; };

// Step 2 for decoder j of a row whose ring is ring[tr][nb]: slot0 = t0 mod tr.  The mode's Costas symbols in frame order,
// each against its own expected tone.
template <class Mode>
PYSDR_FT_HD inline FtScore ft_sync(const float* ring, int tr, int nb, int slot0, int j) {
  float sig = 0.f, tot = 0.f;
  int hits = 0;
  for (int n = 0; n < Mode::kSync; ++n) {
    const int c = Mode::sync_tone(n);
    int sl = slot0 + kFtStepsPerSym * Mode::costas_sym(n);
    if (sl >= tr) sl -= tr;                                // the lag < tr
    const float* p = ring + (size_t)sl * (size_t)nb + j;
    const float e = p[2 * c];
    sig = sig + e;
    float r = p[0];
    for (int tone = 1; tone < Mode::kSyncTones; ++tone) r = r + p[2 * tone];
    tot = tot + r;
    bool hit = true;
    for (int tone = 0; tone < Mode::kTones; ++tone)
      if (tone != c && !(e > p[2 * tone])) hit = false;
    hits += hit ? 1 : 0;
  }
  const float den = tot - sig;
  FtScore out;
  out.score = den > 0.f ? (kFtScore<Mode> * sig) / den : 0.f;
  out.hits = hits;
  return out;
}

// Step 3: is tc an event?  sc and hi hold the decoder's last 9 scores and hit counts, that of step t at index
// (t mod 9) * stride; score[tc + 4] is the newest.
// The comparison itself, for any store of scores: v and hits are step tc's, at(d) the score of step tc + d, d = -4 .. 4
// without 0.  The streaming kernel's nine slots (ft_peak) and the second pass's dense window (pass.hip) both judge with it.
template <class At>
PYSDR_FT_HD inline bool ft_peak_rule(float v, int32_t hits, long long tc, const FtCfg& c, At at) {
  if (!(v >= c.smin) || hits < c.hmin) return false;
  for (int d = 1; d <= kFtReach; ++d) {
    if (tc - d >= 0 && !(v > at(-d))) return false;
    if (!(v >= at(d))) return false;
  }
  return true;
}
PYSDR_FT_HD inline bool ft_peak(const float* sc, const int32_t* hi, long long stride, long long tc, const FtCfg& c) {
  const int s0 = (int)(tc % kFtKeep);
  return ft_peak_rule(sc[s0 * stride], hi[s0 * stride], tc, c,
                      [=](int d) { return sc[((s0 + kFtKeep + d) % kFtKeep) * stride]; });
}

// Soft bit i < 174 of the frame whose first step sits in slot0 of the row's ring, decoder j: data symbol i / 3 (FT4: i / 2),
// bit 4, 2, 1 (2, 1) of its value; max over the values with the bit minus max over those without.
template <class Mode>
PYSDR_FT_HD inline float ft_llr_bit(const float* ring, int tr, int nb, int slot0, int j, int i) {
  constexpr int BPS = Mode::kBitsPerSym;
  const int d = i / BPS, mask = (1 << (BPS - 1)) >> (i % BPS);
  const int sl = (slot0 + kFtStepsPerSym * Mode::data_sym(d)) % tr;
  const float* p = ring + (size_t)sl * (size_t)nb + j;
  float m1 = 0.f, m0 = 0.f;
  bool f1 = true, f0 = true;
  for (int v = 0; v < Mode::kTones; ++v) {
    const float pv = p[2 * Mode::gray(v)];
    if (v & mask) { m1 = (f1 || pv > m1) ? pv : m1; f1 = false; }
    else { m0 = (f0 || pv > m0) ? pv : m0; f0 = false; }
  }
  return m1 - m0;
}

// ---- kernel arguments and the launches (ft.hip) ------------------------------------------------------------------------
struct FtArgs {
  FtC* y;                  // Y + the mode's kHpad: y[a * ypitch + i] = output i of this call, i >= -(S - 1) the row's history
  long long ypitch;
  int n_out, nk, cap, nfine;
  int ns;                  // steps this call completes
  int e_first;             // call-relative output that completes the first of them, < QS (< S at the stream's start)
  int tr;                  // ring depth
  long long t_first;       // absolute index of the call's first step
  FtCfg cfg;
  const FtC* tw;           // [NT]
  float* ring;             // [nk][tr][NB]
  float* sc;               // [9][nfine]
  int32_t* hi;             // [9][nfine]
  int32_t* events;         // [nfine][cap][2]
  int32_t* counts;         // [nfine]
};

struct FtLlrArgs {
  const float* ring;
  int tr, nb, nsub, n;
  const int32_t* cand;     // [n][2]: fine row F, slot0 = t0 mod tr
  float* out;              // [n][174]
};

}  // namespace pysdr
