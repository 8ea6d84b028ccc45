// What the host half of libpysdr_hip.so (api.hip) works out per context and per call without touching the device: the
// tuning values with their measured defaults and the environment that overrides them (read once at create), the
// segmentation plans of the two serial loops, the call-invariant part of the broadcast-FM arguments.  Pure host
// arithmetic, no HIP calls: the sanitizer harness (tests/host_san) calls it the way it calls plan_mixdec.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "common.h"

namespace pysdr {

constexpr double kTwo32 = 4294967296.0;
constexpr double kPllBwHz = 50.0, kPllZeta = 0.7071;
constexpr double kWfmPllBwHz = 30.0;
constexpr int kPllSegMax = 8192;

// The A/B and tuning switches of INTEGRATION.md ("tuning environment") are read ONLY when PYSDR_TUNING=1 is set as
// well: a drop-in library must not change kernels because of a variable that happens to be in the environment.
inline const char* tuning_env(const char* name) {
  const char* on = getenv("PYSDR_TUNING");
  if (!on || atoi(on) <= 0) return nullptr;
  return getenv(name);
}

// Tuning values of a context (pysdr_create reads the environment once: from_env; pysdr_set_tile writes tile_bytes / threads).
struct Tuning {
  int tile_bytes = 0, threads = 1024;  // per LDS buffer (two per workgroup); 0 = as large as fits
  int wgs_per_cu = 1;
  int grid_override = 0;               // PYSDR_MIXDEC_GRID: workgroups of the mix+decimate launches (tests: many tiles per workgroup in a small call)
  int resamp_plain = 0;                // PYSDR_RESAMP_PLAIN: the audio resampler of broadcast FM 0 = a wave per branch, taps in scalar registers (resamp_wave_kernel),
                                       // 1 = one output per thread (resamp_small_kernel), 2 = a half-wave per branch (resamp_branch_kernel) (A/B)
  int mfma_enable = 1;                 // long single-RX prototypes on the matrix cores (mixdec_mfma.hip); 0: VALU form (A/B)
  int dbg_flags = 0, yflush_cap = 0;      // tuning / diagnostic switches, read from the environment once
  int overlap_env = -1;          // PYSDR_OVERLAP=0/1/2 (under PYSDR_TUNING): pysdr_set_overlap is overruled (A/B runs, the test suite in every form)
  int tail_first = -1;           // PYSDR_OVERLAP_ORDER=0/1 (A/B): the deferred tail behind / in front of the next call's walks; -1: by mode
  bool overlap_prio_set = false; // PYSDR_OVERLAP_PRIO: priority of the second stream; unset = the lowest of the device's range (known when the
  int overlap_prio = 0;          //   stream is created)
  // carrier-PLL segmentation (PYSDR_AM_PLL = "taus,taus_exact,coarse_sweeps,kmax,tmin" overrides for A/B runs): warm-up of 16
  // time constants from the block mean of the signal's own phase (joins 7-40 words of 2^32 against a tolerance of 1024 in the
  // NumPy model of the sweeps, scripts/experiments/am_pll_sweeps.py; 14 leave up to 730 on a noisy carrier 40 Hz off tune),
  // the first 11 of them at 4 sweeps per block (5: joins 5 -> 6 words on the bench's carrier, 58 -> 316 in the model's noisy
  // one, segment kernel 105 -> 97 us; 3: the noisy model leaves 2700), the last 5 to the fixed point (8-10 sweeps)
  double am_taus = 16.0, am_taus_exact = 5.0;
  int am_coarse_sweeps = 4, am_kmax = 2048, am_tmin = 512;
  int am_seeded = 1, am_wseed = 0;     // PYSDR_AM_SEED=on[,walked]: warm-ups by the linear solve where the window allows (stage2.hip am_linear_start)
  int am_direct = 1;                   // PYSDR_AM_DIRECT=0: blocks start from the free-running line (A/B)
  int am_phase_on_2 = 1;               // PYSDR_AM_PHASE_STREAM=0: arg y on the front stream in the overlapped form too (A/B)
  // pilot-PLL segmentation (PYSDR_WFM_PLL = "taus,taus_fast,taus_exact,coarse_sweeps,kmax,tmin,exact_cap" overrides for A/B runs)
  // measured on MI355X (bench.py --workload c4, scripts/diag/pll_sweep.sh; front end ms per 2048 chunks):
  //   exact warm-ups 1.70 | 3 coarse sweeps + 6 / 5 / 4 tau exact 1.56 / 1.57 / 1.54 | 4 sweeps 1.61 | 2 sweeps: every join
  //   misses (180 ms of serial patching) | 3 sweeps + 3 tau exact: 115 joins miss | fast warm-up 11 / 9 tau: the check pass
  //   redoes the call (1.85 / 2.4) | 4096 / 3072 / 1024 segments with exact warm-ups 1.96 / 1.78 / 1.71 (2048: 1.70)
  // round 4, after the sweeps went from 35 to 22 vector instructions (stage2.hip wfm_pll_walk; scripts/diag/c4_kt.sh, us per
  // segment-kernel launch, same box): 1024 / 1280 / 1536 / 1792 / 2048 segments 388 / 365 / 349-351 / 379 / 370 -- the walk
  // is now as much the latency of one segment's chain as the SIMDs' issue rate, and fewer, longer segments walk less warm-up
  // judged by the widest join they leave (pysdr_pll_join_margin, tolerance 512 words; scripts/diag/c4_pll4.sh): exact tail 5 / 4 tau
  // 107 / 122 words (C4 step 1.170 / 1.160 ms); two sweeps over the first half of the coarse part 280; exact tail at 4 sweeps 422;
  // both: joins miss; warm-up of 12 / 14 tau instead of 13: 283 / 104
  double wfm_taus = 20.0, wfm_taus_fast = 13.0, wfm_taus_exact = 4.0;
  int wfm_coarse_sweeps = 3, wfm_kmax = 1536, wfm_tmin = 2048;
  double wfm_taus_hi = 0.0, wfm_taus_mid = 0.0;   // staged coarse warm-up (PllPlan::Wc_hi / Wc_mid) in time constants; 0, 0: one stage
  int wfm_tail_cap = 0;                // sweeps per block of the exact tail of a warm-up (0: wfm_exact_cap)
  int wfm_exact_cap = 5;               // sweeps per block of the pilot loop's exact walks (0: to the bit-stable fixed point)
  // Round 5: the segments of the pilot loop start from Newton-in-time seeds (pllseed.hip; two linearised passes over the call by
  // parallel scans of affine maps: within ~30 words of 2^32 of the exact walk) instead of a 13-tau warm-up, whenever the previous
  // call left a mean phase increment; PYSDR_WFM_SEED="0" switches it off, "1,n" walks n samples from the seed first (A/B)
  int wfm_seeded = 1, wfm_wseed = 0;

  // tuning / ablation switches (bench.py and DESIGN.md 4.1 use them; all default to off, read only under PYSDR_TUNING=1)
  static Tuning from_env() {
    Tuning t;
    { const char* e = tuning_env("PYSDR_MIXDEC_WGS"); if (e && atoi(e) > 0) t.wgs_per_cu = atoi(e); }
    { const char* e = tuning_env("PYSDR_MIXDEC_YFLUSH"); if (e && atoi(e) > 0) t.yflush_cap = atoi(e); }
    { const char* e = tuning_env("PYSDR_AM_PLL");
      if (e && *e) {
        double a = 0, tx = 0; int cs = 0, km = 0, tm = 0;
        const int nf = sscanf(e, "%lf,%lf,%d,%d,%d", &a, &tx, &cs, &km, &tm);
        if (nf >= 1 && a > 0) t.am_taus = a;
        if (nf >= 2 && tx >= 0) t.am_taus_exact = tx;
        if (nf >= 3 && cs >= 0) t.am_coarse_sweeps = std::min(cs, 8);
        if (nf >= 4 && km > 0) t.am_kmax = std::min(km, kPllSegMax);
        if (nf >= 5 && tm >= 64) t.am_tmin = (tm + 63) & ~63;
      } }
    { const char* e = tuning_env("PYSDR_AM_SEED");
      if (e && *e) { int on = 1, ws = 0; const int nf = sscanf(e, "%d,%d", &on, &ws); if (nf >= 1) t.am_seeded = on ? 1 : 0; if (nf >= 2 && ws >= 0) t.am_wseed = ws; } }
    { const char* e = tuning_env("PYSDR_AM_DIRECT"); if (e && *e) t.am_direct = atoi(e) ? 1 : 0; }
    { const char* e = tuning_env("PYSDR_AM_PHASE_STREAM"); if (e && *e) t.am_phase_on_2 = atoi(e) ? 1 : 0; }
    { const char* e = tuning_env("PYSDR_MIXDEC_MFMA"); if (e && *e) t.mfma_enable = atoi(e) ? 1 : 0; }
    { const char* e = tuning_env("PYSDR_WFM_SEED");
      if (e && *e) { int on = 1, ws = 0; const int nf = sscanf(e, "%d,%d", &on, &ws); if (nf >= 1) t.wfm_seeded = on ? 1 : 0; if (nf >= 2 && ws >= 0) t.wfm_wseed = ws; } }
    { const char* e = tuning_env("PYSDR_OVERLAP_ORDER"); if (e && *e) t.tail_first = atoi(e); }
    { const char* e = tuning_env("PYSDR_OVERLAP"); if (e && *e) t.overlap_env = std::max(0, std::min(2, atoi(e))); }
    { const char* e = tuning_env("PYSDR_OVERLAP_PRIO"); if (e && *e) { t.overlap_prio_set = true; t.overlap_prio = atoi(e); } }
    { const char* e = tuning_env("PYSDR_RESAMP_PLAIN"); if (e && *e) t.resamp_plain = atoi(e); }
    { const char* e = tuning_env("PYSDR_MIXDEC_GRID"); if (e && atoi(e) > 0) t.grid_override = atoi(e); }
    { const char* e = tuning_env("PYSDR_WFM_PLL");
      if (e && *e) {
        double a = t.wfm_taus, b = t.wfm_taus_fast, x = t.wfm_taus_exact;
        int sw = t.wfm_coarse_sweeps, km = t.wfm_kmax, tm = t.wfm_tmin, xc = t.wfm_exact_cap;
        double th = t.wfm_taus_hi, tmid = t.wfm_taus_mid;
        int tc = t.wfm_tail_cap;
        const int got = sscanf(e, "%lf,%lf,%lf,%d,%d,%d,%d,%lf,%lf,%d", &a, &b, &x, &sw, &km, &tm, &xc, &th, &tmid, &tc);
        if (got >= 10 && tc >= 0) t.wfm_tail_cap = tc;
        if (got >= 9 && th >= 0 && tmid >= 0) { t.wfm_taus_hi = th; t.wfm_taus_mid = tmid; }
        if (got >= 7 && xc >= 0) t.wfm_exact_cap = xc;
        if (got >= 1 && a > 0) t.wfm_taus = a;
        if (got >= 2 && b >= 0) t.wfm_taus_fast = b;
        if (got >= 3 && x > 0) t.wfm_taus_exact = x;
        if (got >= 4 && sw >= 0) t.wfm_coarse_sweeps = sw;
        if (got >= 5 && km >= 1) t.wfm_kmax = std::min(km, kPllSegMax);
        if (got >= 6 && tm >= 64) t.wfm_tmin = tm;
      } }
#ifdef PYSDR_DIAG
    // work-skipping ablation switches exist only in a diagnostic build (python -m pysdr_amd.build --diag)
    { const char* e = getenv("PYSDR_DEBUG_FLAGS"); t.dbg_flags = e ? atoi(e) : 0; }
#endif
    return t;
  }
};

// Tuning values of a spectrum object (pysdr_spectrum_create)
constexpr int kPsdColsMaxG = 4096;   // most grid rows PYSDR_PSD_PATH=loop:<G> can ask for (far above any residency)
constexpr int kPsdRowsMaxR = 4096;   // the same for rows=loop:<R>
struct SpectrumTuning {
  bool force_rocfft = false;  // PYSDR_PSD_ROCFFT: rocFFT even for the 32768 -> 65536 size
  int group = 0;              // frames per launch pair of the four-step path (PYSDR_PSD_GROUP); 0 = 480 with the 24-bit intermediate, 448 with float2
  int packed = 1;             // four-step intermediate as block-scaled 24-bit fixed point (psdfft.hip; PYSDR_PSD_PACKED=0: float2)
  // PYSDR_PSD_STREAMS=2: the groups alternate between two streams, each with its own half-size intermediate
  // (2 x group/2 frames = the same Infinity Cache footprint), so that the columns of one group run beside
  // the rows of the other and the kernel boundaries of one stream hide behind the other's kernels
  static constexpr int kMaxStreams = 4;
  int nstreams = 2;
  // PYSDR_PSD_PATH: the two passes of the 24-bit path, as comma-separated parts.  The columns part -- "unit": one unit (16
  // columns of one frame) per workgroup, grid 16 x frames; "loop:<G>": psd_cols_pk_kernel's loop over frames on 16 x G
  // workgroups; absent: the loop with the G of plan_psd_cols.  (cols_g: -1 = default, 0 = unit, > 0 = forced G)
  // The rows part -- "rows=unit": one unit (32 rows of one frame) per workgroup, grid 8 x frames; "rows=loop:<R>":
  // psd_rows_pk_kernel's loop on 8 x R workgroups; absent: the loop with the R of plan_psd_rows.  (rows_r: as cols_g)
  // "unit" with no rows part is the unit form of BOTH passes: the pair of every round before the loops.
  int cols_g = -1, rows_r = -1;
  int frames_per_group() const { return group > 0 ? group : (packed ? 480 : 448); }

  static SpectrumTuning from_env() {
    SpectrumTuning t;
    t.force_rocfft = tuning_env("PYSDR_PSD_ROCFFT") != nullptr;
    { const char* e = tuning_env("PYSDR_PSD_GROUP"); if (e && atoi(e) > 0) t.group = atoi(e); }
    { const char* e = tuning_env("PYSDR_PSD_PACKED"); if (e && *e) t.packed = atoi(e) ? 1 : 0; }
    { const char* e = tuning_env("PYSDR_PSD_STREAMS"); if (e && atoi(e) >= 1 && atoi(e) <= kMaxStreams) t.nstreams = atoi(e); }
    { const char* e = tuning_env("PYSDR_PSD_PATH");
      bool rows_given = false;
      while (e && *e) {
        const char* end = strchr(e, ',');
        const size_t len = end ? (size_t)(end - e) : strlen(e);
        const bool rows = len >= 5 && !strncmp(e, "rows=", 5);
        const char* p = rows ? e + 5 : e;
        const size_t plen = rows ? len - 5 : len;
        int v = -1;                                                      // a malformed part leaves its default
        if (plen == 4 && !strncmp(p, "unit", 4)) v = 0;
        else if (plen > 5 && !strncmp(p, "loop:", 5) && atoi(p + 5) > 0) v = std::min(atoi(p + 5), rows ? kPsdRowsMaxR : kPsdColsMaxG);
        if (rows) { t.rows_r = v; rows_given = true; } else t.cols_g = v;
        e = end ? end + 1 : nullptr;
      }
      if (!rows_given && t.cols_g == 0) t.rows_r = 0; }
    return t;
  }
};

// The grid of the columns pass as a loop over frames (psdfft.hip psd_cols_pk_kernel): 16 column blocks x G workgroups, of
// which workgroup (cb, g) walks over the frames g, g + G, g + 2 G, ... < nframes of the launch, the next one's samples
// already in flight while one is transformed.  All 16 G workgroups must be resident at once: the 37 KB of LDS of a
// workgroup allow kPsdColsWgPerCu of them on a CU.  Among the G that need the fewest rounds, the smallest is taken, so that
// the frames deal as evenly as they can (240 frames on 256 CUs: 4 rounds, G = 60 with 4 frames each, not 64 of which
// sixteen get 3); no workgroup ever gets more than one frame more than another, and G <= nframes: a single frame is 16
// workgroups of one iteration.  `forced` (PYSDR_PSD_PATH=loop:<G>) is taken as it is, residency included (A/B runs).
constexpr int kPsdColBlocks = 16, kPsdColsWgPerCu = 4;
inline int psd_cols_max_g(int num_cus) { return std::max(1, std::min(kPsdColsMaxG, num_cus * kPsdColsWgPerCu / kPsdColBlocks)); }
inline int plan_psd_cols(int nframes, int num_cus, int forced) {
  if (nframes < 1) return 1;
  if (forced > 0) return std::min(forced, nframes);
  const int gmax = psd_cols_max_g(num_cus);
  const int rounds = (nframes + gmax - 1) / gmax;
  return (nframes + rounds - 1) / rounds;
}
// launch_psd64k's columns form: 0 = float2 intermediate, 1 = 24-bit with one columns unit per workgroup, 1 + G = 24-bit, loop on 16 x G
inline int psd_form(const SpectrumTuning& t, int nframes, int num_cus) {
  if (!t.packed) return 0;
  return t.cols_g == 0 ? 1 : 1 + plan_psd_cols(nframes, num_cus, t.cols_g);
}

// The grid of the rows pass as a loop over frames (psdfft.hip psd_rows_pk_kernel): 8 row blocks x R workgroups, of which
// workgroup (rb, r) walks over the frames r, r + R, r + 2 R, ... < nframes, the next one's intermediate and block scales in
// flight while one is transformed.  The 72 KB of LDS of a workgroup allow kPsdRowsWgPerCu of them on a CU, and all 8 R are
// resident at once; among the R with the fewest rounds the smallest, R <= nframes, `forced` (rows=loop:<R>) as it is --
// plan_psd_cols' rules, and on every CU count the same rhythm (2 CUs / 8 = 4 CUs / 16: 240 frames on 256 CUs = R 60 x 4).
constexpr int kPsdRowBlocks = 8, kPsdRowsWgPerCu = 2;
inline int psd_rows_max_r(int num_cus) { return std::max(1, std::min(kPsdRowsMaxR, num_cus * kPsdRowsWgPerCu / kPsdRowBlocks)); }
inline int plan_psd_rows(int nframes, int num_cus, int forced) {
  if (nframes < 1) return 1;
  if (forced > 0) return std::min(forced, nframes);
  const int rmax = psd_rows_max_r(num_cus);
  const int rounds = (nframes + rmax - 1) / rmax;
  return (nframes + rounds - 1) / rounds;
}
// launch_psd64k's rows form (24-bit path only): 0 = one rows unit per workgroup, R = the loop on 8 x R
inline int psd_rows_form(const SpectrumTuning& t, int nframes, int num_cus) {
  if (!t.packed || t.rows_r == 0) return 0;
  return plan_psd_rows(nframes, num_cus, t.rows_r);
}
// launch_psd64k's `form`: the columns form (psd_form: below kPsdRowsFormShift bits, kPsdColsMaxG + 1 at most) and the rows
// form above it.  (psd_form itself stays the columns' value: tests/psd_cols_plan pins it.)
constexpr int kPsdRowsFormShift = 16;
static_assert(kPsdColsMaxG + 1 < (1 << kPsdRowsFormShift) && kPsdRowsMaxR < (1 << (31 - kPsdRowsFormShift)), "the two forms share an int");
inline int psd_launch_form(const SpectrumTuning& t, int nframes, int num_cus) {
  return psd_form(t, nframes, num_cus) | (psd_rows_form(t, nframes, num_cus) << kPsdRowsFormShift);
}

inline int round_up64(int v) { return (v + 63) & ~63; }
// time constant 1/(zeta*wn) of a second-order loop of bandwidth bw_hz, in samples at fs
inline double pll_tau(double fs, double bw_hz) { return fs / (kPllZeta * 2.0 * M_PI * bw_hz); }
inline int pll_warmup(double taus, double tau) { return round_up64((int)std::ceil(taus * tau)); }

// Segmentation of a serial PLL over n samples (PllPlan, common.h).  W = warm-up in samples = `taus`
// time constants 1/(zeta*wn) of the loop; calls shorter than three warm-ups stay one segment.
inline PllPlan plan_pll(int n, double tau, double taus, double taus_fast, int t_min, int k_max, uint32_t* seg) {
  PllPlan p;
  p.W = pll_warmup(taus, tau);
  p.Wfast = taus_fast > 0 ? pll_warmup(taus_fast, tau) : 0;
  p.Wexact = 0;
  p.Wc_hi = p.Wc_mid = 0;
  p.tail_cap = 0;
  p.coarse_sweeps = 0;
  p.exact_cap = 0;
  p.seeded = 0;
  p.Wseed = 0;
  p.direct = 0;
  if (n < 3 * p.W || k_max <= 1) {
    p.K = 1;
    p.T = round_up64(std::max(n, 64));
  } else {
    p.T = std::max(t_min, round_up64((n + k_max - 1) / k_max));
    p.K = (n + p.T - 1) / p.T;
  }
  p.seg = seg;
  p.lin = seg + (size_t)PYSDR_MAX_RX * kPllSegMax * 4;
  return p;
}

// The carrier loop (AM-Synch) over the n_out outputs of a call at fs_out; pll_kmax: pysdr_set_pll_segments (0 = default, 1 = serial)
inline PllPlan plan_am_pll(const Tuning& t, int n_out, double fs_out, int pll_kmax, uint32_t* seg) {
  const double tau = pll_tau(fs_out, kPllBwHz);
  PllPlan p = plan_pll(n_out, tau, t.am_taus, 0.0, t.am_tmin, pll_kmax > 0 ? std::min(pll_kmax, t.am_kmax) : t.am_kmax, seg);
  if (t.am_coarse_sweeps > 0 && p.K > 1) {
    p.Wexact = pll_warmup(t.am_taus_exact, tau);
    p.coarse_sweeps = t.am_coarse_sweeps;
  }
  p.seeded = (t.am_seeded && p.K > 1) ? 1 : 0;
  p.direct = t.am_direct;
  p.Wseed = std::min(round_up64(std::max(0, t.am_wseed)), std::max(0, p.W - 64));
  return p;
}

// The pilot loop (WFM2) over the n1 IF-rate samples of a call at fs1.
// measured (scripts/experiments/pll_warmup.py), words of 2^32 left of a wrong start state: from
// the call's initial state free-running, 60-270 after 32768 samples = 17.5 tau (one segment in
// 200 beyond the 512-word tolerance: 20 tau); from the previous call's MEAN increment (the loop
// follows a crystal, so its phase is a straight line plus a bounded wobble) 54 after 13 tau
inline PllPlan plan_wfm_pll(const Tuning& t, int n1, double fs1, int pll_kmax, uint32_t* seg) {
  const double tau = pll_tau(fs1, kWfmPllBwHz);
  PllPlan p = plan_pll(n1, tau, t.wfm_taus, t.wfm_taus_fast, t.wfm_tmin, pll_kmax > 0 ? std::min(pll_kmax, t.wfm_kmax) : t.wfm_kmax, seg);
  p.exact_cap = t.wfm_exact_cap;
  p.tail_cap = t.wfm_tail_cap;
  p.seeded = (t.wfm_seeded && p.K > 1) ? 1 : 0;
  p.Wseed = round_up64(std::max(0, t.wfm_wseed));
  if (t.wfm_coarse_sweeps > 0 && p.K > 1) {
    p.Wexact = pll_warmup(t.wfm_taus_exact, tau);
    p.coarse_sweeps = t.wfm_coarse_sweeps;
    if (t.wfm_taus_hi > 0 || t.wfm_taus_mid > 0) {
      p.Wc_hi = pll_warmup(t.wfm_taus_hi, tau);
      p.Wc_mid = pll_warmup(t.wfm_taus_mid, tau);
    }
  }
  return p;
}

// The call-invariant part of the broadcast-FM arguments: discriminator scale, the pilot loop's gains and its 19 kHz word
inline WfmArgs wfm_args(int nrx, int n1, double fs1) {
  WfmArgs w;
  memset(&w, 0, sizeof(w));
  w.nrx = nrx; w.n1 = n1;
  w.scale = (float)(fs1 / (2.0 * M_PI * 75e3));
  const double wn = 2.0 * M_PI * kWfmPllBwHz / fs1;
  w.kp = (float)(2.0 * kPllZeta * wn);
  w.ki = (float)(wn * wn);
  w.norm = (float)(2.0 / 0.1);
  w.rad2word = (float)(kTwo32 / (2.0 * M_PI));
  w.fword0 = pysdr_freq_word(19000.0, fs1, nullptr);
  return w;
}

}  // namespace pysdr
