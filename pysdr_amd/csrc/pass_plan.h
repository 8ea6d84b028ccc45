// The pure half of the FT8 / FT4 second pass: a decoded frame is known sample by sample but for its
// amplitude, so it can be taken out of the row samples and the spectrum of what is left searched again.  Here: what a
// second pass keeps (a ring of row samples yk and a second spectrum ring, ring2) and how deep, the rows that hold a frame's
// tones (the jobs of a subtraction), the reference's integer phase, one symbol's amplitude and its subtraction, the rule
// for a frame and for a rescan window, the plan and every refusal -- the very code the kernels (pass.hip) step with, the
// host half (pass_host.h) checks with and tests/pass_plan/plan_main.cpp runs on the CPU.  float32, every operation rounded
// on its own (-ffp-contract=off); the phase is 32-bit integer arithmetic, one turn = 2^32.  Plain C++: nothing here calls
// the HIP runtime.
#pragma once

#include "ft_plan.h"
#include "report_plan.h"

namespace pysdr {

constexpr int kPassThreads = 256;          // of every kernel here
constexpr int kPassTrials = 9;             // (dn, fw) pairs a frame may carry
constexpr int kPassMax = 256;              // frames of one subtract call
constexpr int kPassRowJobs = 2;            // rows that hold tones of one frame: its own and at most one neighbour
constexpr int kPassJobsMax = kPassRowJobs * kPassMax;
constexpr int kPassReachMax = 120;         // reach_t, steps
constexpr int kPassWindowMax = 256;        // start steps of one rescan: t_lo - 4 .. t_hi + 4, a thread each
constexpr int kPassRowsMax = 256;          // fine rows of one rescan
constexpr int kPassEventCap = kPassWindowMax / kFtMinGap + 1;   // 52: events of a fine row in one rescan
constexpr int kPassLutBits = 12;           // the cos / sin table: 4096 places of a turn
constexpr int kPassLut = 1 << kPassLutBits;
constexpr int kPassOutWords = 4;           // power before, power after (float bits), the trial chosen, the symbols used
constexpr int kPassJobWords = 12 + 2 * kPassTrials;   // 30: see PassJob
constexpr int kPassTileSteps = kFtStepsPerSym;        // steps one workgroup of the respectrum recomputes
constexpr int kPassMargin = 4;             // steps to either side of a frame whose windows a trial's dn may reach

// symbols the frequency pulse of one symbol spans (ft8.waveform: BT = 2, a symbol and a half to either side of its middle;
// ft4.waveform: BT = 1, two and a half)
template <class Mode> constexpr int kPassPulse = Mode::kTones == 8 ? 3 : 5;
template <class Mode> constexpr int kPassSymsSpan = kFtLag<Mode> + 2 * kPassMargin + 1;   // steps t0 - 4 .. t0 + lag + 4
template <class Mode> constexpr int kPassTiles = (kPassSymsSpan<Mode> + kPassTileSteps - 1) / kPassTileSteps;

// The settings of pysdr_*_keep: pysdr_pass_cfg is this layout.
struct PassCfg {
  int32_t reach_t;         // steps a rescan looks to either side of a subtracted frame, [1, 120]
  int32_t trials;          // (dn, fw) pairs per frame of a subtract call, [1, 9]
  const uint32_t* pulse;   // [kPassPulse S]: the cumulative phase of one symbol of tone 1, 2^32 a turn
  const float* lut;        // [4096][2]: (cos, sin)(2 pi i / 4096)
};
static_assert(sizeof(pysdr_pass_cfg) == sizeof(PassCfg) && offsetof(pysdr_pass_cfg, reach_t) == offsetof(PassCfg, reach_t) &&
              offsetof(pysdr_pass_cfg, trials) == offsetof(PassCfg, trials) && offsetof(pysdr_pass_cfg, pulse) == offsetof(PassCfg, pulse) &&
              offsetof(pysdr_pass_cfg, lut) == offsetof(PassCfg, lut), "one layout");

constexpr bool pass_cfg_ok(const PassCfg* c) {
  return c && c->reach_t >= 1 && c->reach_t <= kPassReachMax && c->trials >= 1 && c->trials <= kPassTrials && c->pulse && c->lut;
}

// ---- how much is kept ----------------------------------------------------------------------------------------------------
// A decoded frame t0 is due at the end of the first call that completes step t0 + hold + reach_t - 1.  That call began with
// at most that many steps done and adds at most a call's steps, so done <= t0 + hold + reach_t - 1 + steps_per_call; the
// oldest step a due frame needs is t0 - reach_t - 4, the newest t0 + reach_t + lag + 4 < t0 + hold + reach_t <= done.  One
// step to spare.
template <class Mode> constexpr int pass_ring_steps(int max_out, int S, int reach_t) {
  return kFtHold<Mode> + 2 * reach_t + kPassMargin + ft_steps_per_call(max_out, S);
}
// The sample ring holds every sample of the steps ring2 holds: TY >= QS TR2 + S, rounded up to 16.
constexpr int pass_ring_samples(int tr2, int S) { return (S / 4 * tr2 + S + 15) & ~15; }

struct PassPlan {
  int tr2 = 0, ty = 0, lds_bytes = 0;
  long long bytes = 0;     // of both rings
};

template <class Mode>
inline bool pass_plan(int nk, int S, int max_out, int reach_t, PassPlan* p) {
  if (!ft_s_ok<Mode>(S) || nk < 1 || (long long)nk * (S / 2) > kFtFineMax || max_out < 1 || max_out > kFtMaxOutMax || reach_t < 1 ||
      reach_t > kPassReachMax || !p)
    return false;
  PassPlan q;
  q.tr2 = pass_ring_steps<Mode>(max_out, S, reach_t);
  q.ty = pass_ring_samples(q.tr2, S);
  const long long nb = S / 2 + kFtExtra<Mode>;
  const long long r2 = (long long)nk * q.tr2 * nb * 4, yk = (long long)nk * q.ty * 8;
  if (r2 > kFtRingBytesMax || yk > kFtRingBytesMax) return false;
  q.bytes = r2 + yk;
  // the subtract kernel's LDS, the largest here: codeword, tones, pulse, every trial's amplitudes, flags and score, the
  // symbols' powers before and after, the choice (a symbol's pitch is 104)
  q.lds_bytes = kReportCwBytes + 4 * 104 + 4 * kPassPulse<Mode> * S + kPassTrials * 104 * (8 + 1) + 4 * kPassTrials + 2 * 4 * 104 + 4;
  *p = q;
  return true;
}

// ---- the rows of a frame -------------------------------------------------------------------------------------------------
// The phase word per row sample of q quarter-bauds from a row's centre: q 2^32 / (4 S) turns, rounded half up, mod 2^32.
constexpr uint32_t pass_word(long long q, int S) {
  const long long num = q * (1LL << 31) + S, den = 2LL * S;            // floor((q 2^30 / S) + 1/2)
  long long f = num / den;
  if (num % den != 0 && num < 0) --f;
  return (uint32_t)(unsigned long long)f;
}

struct PassRows {
  int n;                  // 1 or 2
  int row[kPassRowJobs];
  int q[kPassRowJobs];    // tone 0 of the frame in quarter-bauds from that row's centre
};

// Fine row F = a nsub + j: its tones are bins j .. j + extra of row a, which are bins j - nsub .. of row a + 1 (there where
// j + extra >= nsub) and bins j + nsub .. of row a - 1 (there where j <= extra - 1).  `circular`: the raster is the whole
// circle and the neighbours wrap.
template <class Mode>
constexpr PassRows pass_rows(int F, int S, int nk, bool circular) {
  const int nsub = S / 2, nb = nsub + kFtExtra<Mode>;
  const int a = F / nsub, j = F - a * nsub;
  PassRows r{1, {a, 0}, {2 * j - (nb - 1), 0}};
  int nbr = -1, dq = 0;
  if (j + kFtExtra<Mode> >= nsub) { nbr = a + 1; dq = -2 * nsub; }
  else if (j <= kFtExtra<Mode> - 1) { nbr = a - 1; dq = 2 * nsub; }
  else return r;
  if (circular) nbr = (nbr + nk) % nk;
  if (nbr < 0 || nbr >= nk || nbr == a) return r;
  r.n = 2; r.row[1] = nbr; r.q[1] = r.q[0] + dq;
  return r;
}

// ---- what a call may touch ---------------------------------------------------------------------------------------------
PYSDR_FT_HD constexpr long long pass_first_step(long long t_done, int tr2) { return t_done > tr2 ? t_done - tr2 : 0; }
// A frame to subtract: every step whose window a trial can reach, t0 - 4 .. t0 + lag + 4 (from step 0 on), is complete
// and held in ring2 -- and with it, by pass_ring_samples, every sample in yk.
template <class Mode>
PYSDR_FT_HD constexpr bool pass_frame_ok(long long t0, long long t_done, int tr2) {
  return t0 >= 0 && t0 + kFtLag<Mode> + kPassMargin < t_done && (t0 - kPassMargin < 0 ? 0 : t0 - kPassMargin) >= pass_first_step(t_done, tr2);
}
// dn of a trial: less than a step, so that no window outside t0 - 4 .. t0 + lag + 4 meets the frame
PYSDR_FT_HD constexpr bool pass_dn_ok(long long dn, int S) { return dn > -(S / 4) && dn < S / 4; }
// A rescan window: start steps t_lo - 4 .. t_hi + 4 (those >= 0) are whole frames held in ring2.
template <class Mode>
PYSDR_FT_HD constexpr bool pass_window_arg_ok(long long t_lo, long long t_hi) {
  return t_lo >= 0 && t_hi >= t_lo && t_hi - t_lo + 2 * kFtReach + 1 <= kPassWindowMax;
}
template <class Mode>
PYSDR_FT_HD constexpr bool pass_window_ok(long long t_lo, long long t_hi, long long t_done, int tr2) {
  return t_hi + kFtReach + kFtLag<Mode> < t_done && (t_lo - kFtReach < 0 ? 0 : t_lo - kFtReach) >= pass_first_step(t_done, tr2);
}

// ---- the reference -------------------------------------------------------------------------------------------------------
// Phase of sample m < S of symbol k of a frame whose tone 0 turns by `w` per row sample: n w for the frame's sample n =
// S k + m, plus every symbol's tone times the pulse table at the sample's place in that symbol's pulse.  A symbol whose
// pulse is wholly in the past has added tone 2^32 = 0; the first and the last tone are held beyond the frame.
template <class Mode, int S, class Tone>
PYSDR_FT_HD inline uint32_t pass_phase(const Tone* tone, const uint32_t* pulse, uint32_t w, int k, int m) {
  constexpr int H = kPassPulse<Mode> / 2, NS = Mode::kSyms;
  uint32_t ph = (uint32_t)(S * k + m) * w;
#pragma unroll
  for (int d = -H; d <= H; ++d) {
    int kk = k + d;
    kk = kk < 0 ? 0 : (kk > NS - 1 ? NS - 1 : kk);
    ph += (uint32_t)tone[kk] * pulse[(H - d) * S + m];
  }
  return ph;
}
PYSDR_FT_HD constexpr int pass_lut_index(uint32_t ph) { return (int)((ph + (1u << (31 - kPassLutBits))) >> (32 - kPassLutBits)); }

// Where sample n (absolute) of a row sits in yk[TY], and whether it is held: n_lo <= n < n_hi.
PYSDR_FT_HD constexpr bool pass_held(long long n, long long n_lo, long long n_hi) { return n >= n_lo && n < n_hi; }

// a_k = (1 / S) sum_m y[m] conj(r[m]), m ascending from the first term; y: the row's ring yk[TY], the symbol's first sample
// at absolute index n0.  -> false (and a = 0) where a sample is not held.
template <class Mode, int S, class Tone>
PYSDR_FT_HD inline bool pass_amp(const FtC* yk, int ty, long long n0, long long n_lo, long long n_hi, const Tone* tone, const uint32_t* pulse,
                                 const FtC* lut, uint32_t w, int k, FtC* a) {
  a->x = 0.f; a->y = 0.f;
  if (!pass_held(n0, n_lo, n_hi) || !pass_held(n0 + S - 1, n_lo, n_hi)) return false;
  int at = (int)(n0 % ty);
  float sr = 0.f, si = 0.f;
  for (int m = 0; m < S; ++m) {
    const FtC y = yk[at], r = lut[pass_lut_index(pass_phase<Mode, S>(tone, pulse, w, k, m))];
    const float vr = y.x * r.x + y.y * r.y, vi = y.y * r.x - y.x * r.y;
    if (m == 0) { sr = vr; si = vi; }
    else { sr = sr + vr; si = si + vi; }
    if (++at == ty) at = 0;
  }
  constexpr float inv = 1.0f / (float)S;
  a->x = sr * inv; a->y = si * inv;
  return true;
}

// y[m] -= a r[m] over a symbol whose samples are all held; *before, *after: sum_m |y[m]|^2, m ascending from the first term
template <class Mode, int S, class Tone>
PYSDR_FT_HD inline void pass_sub(FtC* yk, int ty, long long n0, const Tone* tone, const uint32_t* pulse, const FtC* lut, uint32_t w, int k,
                                 FtC a, float* before, float* after) {
  int at = (int)(n0 % ty);
  float pb = 0.f, pa = 0.f;
  for (int m = 0; m < S; ++m) {
    const FtC y = yk[at], r = lut[pass_lut_index(pass_phase<Mode, S>(tone, pulse, w, k, m))];
    const float b = y.x * y.x + y.y * y.y;
    FtC z;
    z.x = y.x - (a.x * r.x - a.y * r.y);
    z.y = y.y - (a.x * r.y + a.y * r.x);
    const float c = z.x * z.x + z.y * z.y;
    if (m == 0) { pb = b; pa = c; }
    else { pb = pb + b; pa = pa + c; }
    yk[at] = z;
    if (++at == ty) at = 0;
  }
  *before = pb; *after = pa;
}

// ---- kernel arguments and the launches (pass.hip) ------------------------------------------------------------------------
// One job: a frame on one row.  30 words: row, the place of its four words in out, w (tone 0's word in this row), the
// message's three words, QS t0 (low, high), trials, three spare, then (dn, fw) of every trial.
struct PassJob {
  int32_t row, out_at;
  uint32_t w, m0, m1, m2;
  int32_t n0_lo, n0_hi, ntr, t0_lo, t0_hi, spare;
  int32_t trial[2 * kPassTrials];
};
static_assert(sizeof(PassJob) == 4 * kPassJobWords, "30 words");

struct PassKeepArgs {
  const FtC* y;            // the skimmer's Y + kHpad: the call's outputs
  long long ypitch;
  int n_out, nk, nb;
  long long m0;            // absolute index of the call's first output
  const float* ring;       // [nk][tr][nb]
  int tr, ns;
  long long t_first;
  FtC* yk;                 // [nk][ty]
  int ty;
  float* ring2;            // [nk][tr2][nb]
  int tr2;
};

struct PassSubArgs {
  FtC* yk;
  int ty, nrows;
  long long n_lo, n_hi;    // absolute row samples held: n_lo <= n < n_hi
  const PassJob* jobs;     // sorted by row, in the order given within a row
  const int32_t* rows;     // [nrows][2]: first job, jobs
  const uint32_t* pulse;
  const FtC* lut;
  int32_t* out;            // [n][2][4]
};

struct PassSpecArgs {
  const FtC* yk;
  int ty, njobs;
  const PassJob* jobs;
  const FtC* tw;
  float pmax;
  float* ring2;
  int tr2;
  long long t_done;
};

struct PassScanArgs {
  const float* ring2;
  int tr2, nb, nsub;
  int F_lo, nF;
  long long t_lo;
  int nt;                  // t_hi - t_lo + 1
  FtCfg cfg;
  int32_t* counts;         // [nF]
  int32_t* events;         // [nF][kPassEventCap][2]
};

}  // namespace pysdr
