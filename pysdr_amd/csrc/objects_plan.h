// What the four stream objects -- waterfall, RTTY decoder bank, channelizer, channel bank -- share between their kernels
// (waterfall.hip, rtty.hip, chan.hip, bank.hip), their host half (api_objects.hip) and the checking launch layer of
// tests/host_san: constants, pure plans, kernel argument structs, and DECLARATIONS ONLY of the launch functions (defined in
// the four kernel files, or by the harness's stubs) and of api.hip's two create helpers.  In the channelizer's section: what
// an object that borrows one may know of it (chan_client.h).  At its end: the launches of the CW skimmer (api_cw.hip,
// cw.hip; its plan and step: cw_plan.h) and of the PSK31 skimmer (api_psk.hip, psk.hip; psk_plan.h).  Nothing in this
// header calls the HIP runtime; plain C++.  Not part of the public ABI.
#pragma once

#include "common.h"
#include "fft_plan.h"

namespace pysdr {

// api.hip: what every create function of the host layer shares
int use_device(int dev);                        // hipSetDevice, PYSDR_ERR_NO_DEVICE with a message
int failed_in(const char* entry, int rc);       // the message gains the entry point's name; returns rc

// ---- waterfall (waterfall.hip) ---------------------------------------------------------
constexpr float kFill = -1.0e38f;    // Plotting.py:385

struct WfArgs {
  const float* wf;        // [ncols][nfft]
  int nfft, ncols, head, cnt, shift;
  float* mean;            // [nfft]
  float* stat;            // [0] bkgnd, [1] max(wf) as an ordered key
  float* image;           // [ncols][nfft]
};
int launch_wf_fill(float* p, size_t n, float v, hipStream_t st);
int launch_wf_push(const float* line, int n, int nfft, int shift, float* slot, hipStream_t st);
int launch_wf_mean_median(const WfArgs& a, hipStream_t st);                         // mean, then stat[0]
int launch_wf_max_image(const WfArgs& a, int npsd, float pan_dr, hipStream_t st);   // stat[1] (zeroed by the caller), then image
int launch_wf_peaks(const float* x, int n, double height, int dist, int* pos, int* state, int* kept, int* count, hipStream_t st);

// ---- RTTY decoder bank (rtty.hip) ------------------------------------------------------
constexpr int kM = 30;                // lines per character (rtty.py:386)
constexpr int kHist = 128;            // ring rows beyond max_lines
constexpr int kMaxLines = 32768;

struct RttyArgs {         // one decode call: lines n0 .. n0 + nlines - 1, decisions at n_first + 30 j, j < nd
  const float* lines;     // [nlines][nfft]
  int nfft, flipped, nlines;
  int band_lo, nband, moff, nsh, nb, flo, fhi;    // moff, flo, fhi: counted from band_lo
  long long n0, n_first;
  int nd, max_dec, R;
  float *band, *s4, *best, *sc2;                  // rings [R][nband] / [R][nb]
  int* isym;                                      // ring [R][nb]
  int* shift;                                     // [nb]
  long long* t; double* snr; int* held; int* code;   // [max_dec][nb]
  int* ndet;                                      // [max_lines]
};
int launch_rtty_decode(const RttyArgs& a, hipStream_t st);   // rt_gather .. rt_sc2, (rt_decide, rt_emit,) rt_find

// ---- polyphase channelizer (chan.hip; its FFT's passes, multipliers, positions and twiddles: fft_plan.h) ----------------
constexpr int kChanLdsElems = 16384;      // complex LDS elements a workgroup may hold (128 KB of the 160 KB)
constexpr int kChanMaxIn = 1 << 28;

struct ChanPlan {
  int npass = 0, radix[kFftMaxPass] = {};     // fft_factor(M)
  int C = 0;          // M / D
  int fw = 0;         // frames per workgroup
  int fi = 0;         // frames per FIR work item
  int threads = 0;
  int mp = 0;         // LDS pitch of a frame, odd: the store reads one element of every frame side by side
  int lds_bytes = 0;
};

// Pure arithmetic: which launch a channelizer of this shape runs with; false: outside the rules of DESIGN §3 item 15.
inline bool chan_plan(int M, int D, ChanPlan* p) {
  if (M < 16 || M > 4096 || D < 1 || M % D != 0) return false;
  const int C = M / D;
  if (C != 1 && C != 2 && C != 4) return false;
  ChanPlan q;
  if (!fft_factor(M, &q.npass, q.radix)) return false;
  q.C = C;
  // 16 frames = 128-byte row segments while they fit the LDS; small M: as many groups of 16 as fill 256 branches
  if (M <= 256) q.fw = 16 * (256 / M);
  else if (M * 16 <= kChanLdsElems) q.fw = 16;
  else if (M * 8 <= kChanLdsElems) q.fw = 8;
  else q.fw = 4;
  q.fi = q.fw < 8 ? 4 : 8;
  q.mp = M | 1;
  q.threads = q.fw * M > 4096 ? 1024 : 256;
  q.lds_bytes = q.fw * q.mp * (int)sizeof(float2);
  *p = q;
  return true;
}

struct ChanArgs {
  const float2* x;        // this call's samples, x[0] = absolute sample s0
  const float2* hist;     // hist[H]: samples s0 - H .. s0 - 1 (zeros before the stream's start)
  int H, n;
  int off0;               // mf D - s0, 0 <= off0 < D: where the call's first frame mf ends
  int mf_lo;              // mf mod 4
  int nframes;
  int M, D, P, mp, fw;
  const float* taps;      // [P][M]
  const float2* tw;       // [M] e^{+j 2 pi j / M}
  const int* perm;        // [nk] LDS position of row a's channel
  int nk;
  float2* y;              // y[a * pitch + (m - mf)]
  long long pitch;
  uint32_t magic_M, magic_fw;
  FftPasses fft;          // of M points (fft_plan.h)
  int xq, xr;             // grid / 8, grid % 8: the workgroups that share an L2 take consecutive runs of frames
};
int chan_prepare(const ChanPlan& p);            // more than 64 KB of LDS is an opt-in per kernel
int launch_chan(const ChanPlan& p, const ChanArgs& a, int grid, hipStream_t st);
// new history = last H samples of [old history | x[0 .. n)]
int launch_chan_roll(const float2* x, int n, const float2* old, float2* neu, int H, hipStream_t st);
// What an object that borrows a channelizer of either kind knows of it (api_objects.hip; taken under the channelizer's lock).
struct ChanInfo {
  int device, M, D, nk, max_in;
  int out_cap;                    // most outputs one call can complete, rounded up to 16
  hipStream_t stream;             // every launch and copy of the channelizer is queued here
  unsigned long long n_abs;       // input samples since create / reset
};
int chan_info(pysdr_chan* c, ChanInfo* out);

// ---- channel bank (bank.hip) -----------------------------------------------------------
constexpr int kBankThreads = 256;
constexpr int kBankW = 8;                               // outputs per thread = taps per step
constexpr int kBankTile = kBankThreads * kBankW;        // outputs per workgroup
constexpr int kBankTapsMin = 3, kBankTapsMax = 255;     // 3: the squelch's second difference reaches d[m - 2]
constexpr int kBankNkMax = 4096;
constexpr float kAgcRefDefault = 0.5f;

struct BankPlan {
  int tp = 0;          // taps rounded up to whole steps of 8
  int hpad = 0;        // history samples kept in front of a row, >= T + 1, a multiple of 8
  int lds_floats = 0;  // kBankTile + tp (the complex-tap modes hold two such planes)
  int tiles = 0;       // per row, for max_out outputs
};

inline bool bank_plan(int nk, int ntaps, int max_out, BankPlan* p) {
  if (nk < 1 || nk > kBankNkMax || ntaps < kBankTapsMin || ntaps > kBankTapsMax || max_out < 1) return false;
  BankPlan q;
  q.tp = (ntaps + kBankW - 1) / kBankW * kBankW;
  q.hpad = (ntaps + 1 + 7) & ~7;
  q.lds_floats = kBankTile + q.tp;
  q.tiles = (max_out + kBankTile - 1) / kBankTile;
  *p = q;
  return true;
}

struct BankState {       // one per channel, in device memory
  float agc, gain, maxbuf, err, level;
  int open;
};

struct BankArgs {
  const float2* y;        // Y + Hpad: y[a * ypitch + i] = output i of this call, i >= -Hpad (history)
  long long ypitch;
  float* a;               // a[a * apitch + i]
  long long apitch;
  int n_out, T, tp;
  const float* taps;      // [tp], zero beyond T (never multiplied: 0 * NaN would widen a NaN's footprint); USB / LSB / CW: [2 tp], re then -im
  float fm_scale;
  int noise;              // 1: leave the squelch's partial sums
  float* pmax;            // [nk][ptiles]
  double* psum;           // [nk][ptiles]
  int ptiles;
  uint32_t m0_lo;         // CW: low 32 bits of the absolute index of the call's first output
  uint32_t fword;         // CW: the BFO's phase increment per output
};

struct FinishArgs {
  float2* ybase;          // Y: row a at ybase + a * ypitch, history in [0, hpad)
  long long ypitch;
  float* a;
  long long apitch;
  int n_out, hpad, ntiles, ptiles;
  const float* pmax;
  const double* psum;
  BankState* state;
  int agc_active;         // AGC enabled and mode AM, USB, LSB or CW
  int squelch;            // mode NFM and threshold > 0
  float ref, thresh;
};
int launch_bank(int mode, const BankPlan& p, const BankArgs& a, int ntiles, int nk, hipStream_t st);   // mode: PYSDR_AM | PYSDR_NFM | PYSDR_USB | PYSDR_LSB | PYSDR_CW
int launch_bank_finish(const FinishArgs& f, int nk, hipStream_t st);

// ---- CW skimmer (cw.hip, host half api_cw.hip; plan, state and kernel arguments: cw_plan.h) ----------------------------
struct CwArgs;
int launch_cw_decode(const CwArgs& a, hipStream_t st);

// ---- PSK31 skimmer (psk.hip, host half api_psk.hip; plan, steps and kernel arguments: psk_plan.h) ----------------------
struct PskArgs;
int launch_psk_decode(int S, const PskArgs& a, hipStream_t st);

// ---- RTTY raster skimmer (fsk.hip, host half api_fsk.hip; plan, steps and kernel arguments: fsk_plan.h) ----------------
struct FskArgs;
int launch_fsk_decode(int S, const FskArgs& a, hipStream_t st);

// ---- packet skimmer (pkt.hip, host half api_pkt.hip; plan, steps and kernel arguments: pkt_plan.h) ----------------------
struct PktArgs;
int launch_pkt_decode(const PktArgs& a, hipStream_t st);

// ---- SSTV skimmer (sstv.hip, host half api_sstv.hip; plan, steps and kernel arguments: sstv_plan.h) -------------------------
struct SstvArgs;
int launch_sstv_decode(const SstvArgs& a, hipStream_t st);

// ---- RDS skimmer (rds.hip, host half api_rds.hip; plan, steps and kernel arguments: rds_plan.h) -----------------------------
struct RdsArgs;
int launch_rds_decode(const RdsArgs& a, hipStream_t st);

// ---- ACARS skimmer (acars.hip, host half api_acars.hip; plan, steps and kernel arguments: acars_plan.h) ---------------------
struct AcArgs;
int launch_acars_decode(const AcArgs& a, hipStream_t st);

// ---- FT8 and FT4 skimmers (ft.hip, host half api_ft.hip; modes, plan, steps and kernel arguments: ft_plan.h) ----------------
struct FtArgs;
struct FtLlrArgs;
int launch_ft_steps(int source, int S, const FtArgs& a, hipStream_t st);   // spectrum of the call's steps, then sync and peaks; source:
int launch_ft_llr(int source, const FtLlrArgs& a, hipStream_t st);         // the mode's LdpcSource

// ---- LDPC(174,91) decoder (ldpc.hip, host half ldpc_host.h; tables, steps and kernel arguments: ldpc_plan.h) -----------
struct LdpcArgs;
int launch_ldpc_decode(int source, const LdpcArgs& a, hipStream_t st);   // source: LdpcSource

// ---- ordered-statistics decoding behind it (osd.hip; steps and kernel arguments: osd_plan.h) -----------------------------
struct OsdArgs;
int launch_osd_decode(int source, const OsdArgs& a, hipStream_t st);     // source: LdpcSource, the min-sum launch's

// ---- a-priori decoding (ap.hip, host half ap_host.h; rules, steps and kernel arguments: ap_plan.h) -------------------------
struct ApArgs;
int launch_ap_decode(int source, const ApArgs& a, hipStream_t st);       // every pair's decode, then the pick; source: LdpcSource

// ---- frame report and row floor (report.hip, host half report_host.h; steps and kernel arguments: report_plan.h) ---------
struct ReportArgs;
struct FloorArgs;
int launch_frame_report(int mode, const ReportArgs& a, hipStream_t st);  // mode: ReportMode
int launch_ring_floor(const FloorArgs& a, hipStream_t st);

// ---- second pass (pass.hip, host half pass_host.h; steps and kernel arguments: pass_plan.h) --------------------------------
struct PassKeepArgs;
struct PassSubArgs;
struct PassSpecArgs;
struct PassScanArgs;
int launch_pass_keep(const PassKeepArgs& a, hipStream_t st);
int launch_pass_subtract(int source, int S, const PassSubArgs& a, const PassSpecArgs& s, hipStream_t st);   // subtract, then respectrum
int launch_pass_rescan(int source, const PassScanArgs& a, hipStream_t st);                                  // source: LdpcSource

}  // namespace pysdr
