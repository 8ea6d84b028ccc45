// C ABI of libpysdr_hip.so (include/pysdr_hip.h): context management, the per-call
// launch sequence of the receiver hot path, spectrum (rocFFT), device-memory helpers
// and the RCCL broadcast (the four stream objects: api_objects.hip).  Host-side only; kernels live in mixdec/stage2/misc.hip.
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <rocfft/rocfft.h>

#include <cmath>
#include <algorithm>
#include <cstdarg>
#include <map>

#include "common.h"
#include "host_plan.h"
#include "host_res.h"
#include "mixdec_mfma_geom.h"
#include "mixdec_plan.h"
#include "objects_plan.h"

namespace pysdr {

static thread_local char g_err[2048] = "";

void set_last_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// (these two are shared with api_objects.hip: objects_plan.h)
int use_device(int dev) {
  hipError_t e = hipSetDevice(dev);
  if (e != hipSuccess) {
    set_last_error("hipSetDevice(%d): %s", dev, hipGetErrorString(e));
    return PYSDR_ERR_NO_DEVICE;
  }
  return PYSDR_OK;
}

// A create function that failed half-way: the message gains the entry point's name in front of the failing call and
// its HIP error string; the caller then destroys the half-built object (its owners free what exists).
int failed_in(const char* entry, int rc) {
  const std::string what = pysdr_last_error();
  set_last_error("%s: %s", entry, what.c_str());
  return rc;
}

}  // namespace pysdr

using namespace pysdr;

namespace {

constexpr float kNfmFullScaleDev = 5000.0f;

inline bool mode_has_agc(int m) {
  return m == PYSDR_AM || m == PYSDR_AM_SYNCH || m == PYSDR_SSB || m == PYSDR_USB ||
         m == PYSDR_LSB || m == PYSDR_CW || m == PYSDR_RTTY;
}
inline int mode_detector(int m) {
  switch (m) {
    case PYSDR_AM: return kDetAbs;
    case PYSDR_AM_SYNCH: return kDetPll;
    case PYSDR_NFM: return kDetFm;
    case PYSDR_CW: return kDetBfo;
    default: return kDetNone;
  }
}

// One polyphase decimator instance (mixdec kernel): geometry, raw-sample history (double
// buffered), LO-modulated taps on the device, absolute input counter.
struct Decim {
  int up = 1, down = 1, ntaps = 0, kdec = 0, kpad = 0, hist_len = 0, max_rx = 0;
  BufPair<float2> d_hist;              // flips on every launch of this decimator
  int hist_cur = 0;
  DevBuf<float2> d_taps;               // [max_rx][up][kpad]
  std::vector<float2> h_taps;
  unsigned long long s_abs = 0;        // absolute index of the next input sample
  size_t per() const { return (size_t)up * kpad; }
};

struct RxHost {
  int mode = PYSDR_AM;
  double lo_freq = 0;
  uint32_t fword = 0, phase = 0;
  std::vector<double> h;        // prototype, ntaps_dec
  std::vector<double> af;       // complex AF taps, 2*ntaps_af
  double bfo = 0;
  uint32_t bfo_fword = 0;
  bool taps_dirty = true, af_dirty = true, agc_dirty = true;
  unsigned reset_pending = 3;
  int agc_enable = 1;
  float agc_ref = 0.5f;
  float sq_thresh = 0.f;
  float sq_ratio = 0.f;         // ratio squelch armed (> 0: the least sq1 / sq2 that keeps the gate open); takes precedence
  // The pairs: what the front end of a call writes and its tail reads a call later alternates between two buffers when the
  // context overlaps its calls (pysdr_set_overlap); the context's `par` selects, the second buffers come into being then
  BufPair<float2> d_y;          // [hy + mmax]
  BufPair<float2> d_ypll;       // [hy + mmax], allocated on first AM-Synch use
  DevBuf<float2> d_a;           // [mmax]
  DevBuf<float> d_am;           // [2*mmax]
  DevBuf<float2> d_aftaps;      // [ntaps_af rounded up to 4], zero padded
  int taps_real = 0;
  // broadcast FM (WFM / WFM2)
  std::vector<double> wfm_video;   // pre-detection filter at SRATE (ntaps_dec)
  std::vector<double> wfm_resamp;  // fs1 -> FS_OUT prototype (up2 * taps per phase)
  bool wfm_dirty = true;
  Decim wfm_audio;                 // per-RX resampler fs1 -> FS_OUT
  BufPair<float2> d_y1;            // [2 + m1max] IF-rate IQ (1-sample history in slot 1)
  BufPair<float2> d_w;             // [m1max] composite * (1 + 2j sin 2theta)
  DevBuf<double> d_seed;           // WFM2: scan buffers of the pilot loop's Newton-in-time seeds (pllseed.hip), allocated on first stereo use
  BufPair<float> d_mnt;            // ... and mpx * norm in the seed kernels' order, written by the discriminator: a pair like d_w
};

// What one pysdr_process_batch call uses of the receivers' host-side state.  Taken under
// c->mu by apply_pending, so that a setter running on another thread (gui.py:1713,1938)
// between two lines of the launch sequence can only affect the NEXT call: the taps on the
// device, the NCO word, the detector kind and the buffers it needs always belong together.  Plain pointers: a snapshot
// is handed to launches and owns nothing.
struct RxSnap {
  int mode = PYSDR_AM;
  uint32_t fword = 0, phase = 0, bfo_fword = 0;
  float sq_thresh = 0.f, sq_ratio = 0.f;
  int taps_real = 0;
  float2 *d_y = nullptr, *d_ypll = nullptr, *d_a = nullptr, *d_y1 = nullptr, *d_w = nullptr;   // d_y / d_ypll / d_y1 / d_w: THIS call's buffer of each pair
  float2 *d_y_next = nullptr, *d_ypll_next = nullptr, *d_y1_next = nullptr;   // the next call's (the same one unless the calls overlap): gets the history prefix
  double* d_seed = nullptr;
  float* d_mnt = nullptr;
  float* d_am = nullptr;
  float2* d_aftaps = nullptr;
};
struct CallSnap {
  int nrx = 0, nwfm = 0;
  bool use2 = false;             // this call's tail is deferred (pysdr_set_overlap)
  RxSnap rx[PYSDR_MAX_RX];
};

// The tail of a call (T in pysdr_ctx): everything it needs that the front part of the call worked out.
struct TailJob {
  bool valid = false;
  CallSnap snap;
  bool wfm = false;
  bool wait_pll = false;         // the call's loop walks run on stream2: the tail waits for ev_pll[par]
  int par = 0, nchunks = 0, n1 = 0;
  size_t chunk_len = 0, n = 0;
  unsigned long long s0 = 0;
  Stage2Args s;                  // narrow-band: complete.  Broadcast FM: the output counts come from the audio resampler, which is part of the tail
  hipEvent_t ev_end = nullptr;   // the profile's last mark of that call (nullptr: not profiled)
};

}  // namespace

struct pysdr_ctx {
  pysdr_cfg cfg;
  int nrx = 0;
  RxHost rx[PYSDR_MAX_RX];
  std::mutex mu;
  // Everything that queues work on the context's streams or moves the deferred tail -- process / process_batch, fetch, sync,
  // the state getters (they queue the deferred tail: flush_tail), get_elapsed_ms, set_overlap, a spectrum ordering itself
  // against the context, the ingest ring's submit / collect, the broadcast -- runs under this lock: the reference reads the
  // AGC fields from its GUI / watchdog thread (watchdog.py:298-302) while the RX thread is inside demod_data, and a getter
  // that ran the tail beside pysdr_process_batch's `c->tail = job` could run it twice or from a half-copied job.
  // Recursive: pysdr_process is process_batch + fetch.  The setters keep to `mu` (they only mark work as pending).
  std::recursive_mutex run_mu;
  // Every device resource below is an owner (host_res.h): deleting the context frees them.  pysdr_destroy drains the
  // streams first, so the order of the members does not matter for that.
  Stream stream;
  // pysdr_set_overlap: a call is three groups of launches --
  //   F  the front end (mix + decimate; + the short parallel kernels in front of a serial loop: arg y for the carrier
  //      loop, the discriminator for broadcast FM),
  //   P  the segment walks of a serial loop (AM-Synch carrier PLL, WFM2 pilot PLL): a few thousand single-wave chains,
  //      latency bound, no LDS, a third to a half of such a call's time,
  //   T  the tail (audio resampler of broadcast FM, detector + AF FIR, AGC, output): LDS-tiled and throughput bound --
  // and in the single-stream form they run F P T, F P T, ...  Overlapped, P(k) goes on `stream2` and `stream` runs
  //   F(k)  [wait P(k-1)]  T(k-1)  F(k+1)  [wait P(k)]  T(k) ...
  // i.e. the TAIL OF A CALL IS DEFERRED until the front end of the next one has been queued (or until anything asks
  // for its results: flush_tail), so that the walks of call k run beside T(k-1) and F(k+1).  What F writes and T reads a
  // call later -- the FS_OUT-rate IQ y, the IF-rate IQ y1, the loops' buffers -- alternates between two buffers (`par`);
  // each history prefix is rolled into the OTHER buffer.  Two events order it: ev_front (F(k) done -> P(k) may start) and
  // ev_pll[par] (P(k) done -> T(k) may start); everything else is stream order.
  // Round 5's first form put P AND T on stream2; measured (profiles/r05_overlap_*.txt): the AF FIR cannot start while the
  // persistent workgroups of a front end hold their CUs' LDS, so T took turns with F whatever the streams said, and a P
  // that shares its SIMDs with matrix-core waves runs 2.2-2.5x longer (a vector instruction waits for the MFMA in
  // front of it) -- P + T behind one another on stream2 was then LONGER than F, and the front end idled.
  // WHICH calls: those with a serial loop in them (overlap = 1); overlap = 2 defers every call's tail (tests: nothing
  // runs on stream2 then, the buffers and the deferral are exercised all the same).  A change of form between two calls
  // flushes and drains.
  Stream stream2;
  int overlap = 0;               // pysdr_set_overlap: 0 off, 1 the calls with a serial loop, 2 every call
  bool use2 = false;             // the form of the LAST call
  int par = 0;                   // buffer of each pair the NEXT call's front end writes
  int last_par = 0;              // ... and the one the last finished call wrote (pysdr_fetch reads its IQ)
  Event ev_pll[2];
  int n_ingest = 0;              // ingest rings on this context (they run it single-stream)
  TailJob tail;                  // the deferred tail of the last call (tail.valid)
  int hy = 0, mmax = 0;
  size_t cap_samples = 0;
  Decim main;                    // SRATE -> FS_OUT (UP/DOWN) for the narrow-band modes
  Decim wfm_front;               // SRATE -> fs1 = SRATE/d1 for WFM/WFM2
  int d1 = 0, up2 = 0, down2 = 0, m1max = 0;
  int last_wfm = 0;              // the last call ran the broadcast-FM pipeline
  DevBuf<float2> d_stage;        // host input of a call, grown on demand
  BufPair<unsigned> d_peak2;     // [max_chunks] raw-chunk peaks, two buffers: the history-roll kernel of a call zeroes the OTHER one for the
  int peak_cur = 0;              //   next call (a memset per call was one more kernel + 4 us on the stream); peak_cur: the last call's
  bool peak_clean[2] = {true, true};   // that buffer is all zero (a call that failed before its history roll leaves the other dirty)
#ifdef PYSDR_DIAG
  DevBuf<unsigned long long> d_stamps;      // mixdec phase stamps (PYSDR_DEBUG_FLAGS & 256)
  DevBuf<unsigned long long> d_mm_stamps;   // mixdec_mfma: per-workgroup placement and clocks (PYSDR_DEBUG_FLAGS & 512), [1024][24]
#endif
  DevBuf<unsigned> d_peak_scratch;     // [1] sink for decimators whose raw peak is not wanted
  DevBuf<unsigned> d_blkpeak;    // [MAX_RX][max_chunks]
  DevBuf<float> d_gain;          // [MAX_RX][max_chunks]
  DevBuf<float> d_blknoise;      // [MAX_RX][max_chunks]
  DevBuf<float> d_blknoise2;     // [MAX_RX][max_chunks] ratio squelch: the low-pass envelope's block sums (allocated when first armed)
  DevBuf<float> d_sqtaps;        // [2][kSqTapsMax] its two FIRs
  int sq_ntaps = 0;
  DevBuf<unsigned> d_blkcnt;     // [MAX_RX][max_chunks]
  DevBuf<RxDevState> d_state;    // [MAX_RX]
  DevBuf<uint32_t> d_pllseg;     // [MAX_RX][kPllSegMax][4] start/end states of the time-parallel PLLs + [MAX_RX][kPllSegMax] flags (PllPlan::lin)
  // last call
  int last_nout = 0, last_nchunks = 0, last_nrx = 0;
  size_t last_chunk_len = 0;
  unsigned long long last_s0 = 0;
  int last_complex[PYSDR_MAX_RX] = {0};
  // tuning / profiling
  Tuning tune;                            // host_plan.h: the measured defaults, the environment read once at create, pysdr_set_tile
  int num_cus = 256;
  int pll_kmax = 0;                       // pysdr_set_pll_segments: 0 = default, 1 = serial
  int profile = 0;
  static constexpr int kSlots = 64;       // ring of per-call event sets (profiling)
  Event ev[kSlots][4];
  Event ev_front;                         // the input of the last call has been consumed (front end done)
  hipEvent_t front_marker = nullptr;      // the event that marks it for the LAST call (ev_front, the profile's, or none)
  int front_wanted = 0;                   // a spectrum has ordered itself behind the front end: keep recording ev_front
  unsigned long long ncalls = 0;
  // RCCL
  void* rccl_lib = nullptr;
  ncclComm_t comm = nullptr;
};

struct pysdr_spectrum {
  int device = 0, chunk = 0, nfft = 0, max_frames = 0;
  int num_cus = 256;          // read once at create: the grids of the columns and rows loops (host_plan.h plan_psd_cols / plan_psd_rows)
  Stream stream;
  DevBuf<float> d_win;
  DevBuf<float2> d_work;      // [frames][nfft], grown on demand
  DevBuf<float2> d_in;        // [chunk] staging for host frames
  DevBuf<float> d_out;        // [nfft] staging for host frames
  DevBuf<unsigned char> d_fftwork;   // rocFFT's work buffer, grown on demand
  std::map<int, rocfft_plan> plans;
  rocfft_execution_info info = nullptr;
  Event ev[2];
  Event ev_order;
  SpectrumTuning tune;        // host_plan.h
  bool ran = false;           // spectrum_run has recorded ev[1] at least once
  static constexpr int kMaxStreams = SpectrumTuning::kMaxStreams;
  Stream xstream[kMaxStreams];               // [0] unused (= stream)
  DevBuf<float2> xwork[kMaxStreams];         // [0] unused (= d_work)
  size_t xwork_frames = 0;
  Event ev_join[kMaxStreams];
};

// N4: ingest ring.  Pinned host chunk buffers the device reads directly over PCIe (async H2D on
// its own stream into two device staging buffers) and pinned per-slot result buffers.
struct pysdr_ingest {
  pysdr_ctx* c = nullptr;
  int nslots = 0;
  int chunks_per_slot = 1;
  size_t cap = 0;                         // samples per slot buffer (chunks_per_slot chunks)
  int ocap = 0;                           // outputs per RX per chunk
  Stream copy_stream;
  std::vector<PinnedBuf<float2>> h_in;    // [nslots] pinned
  DevBuf<float2> d_in[2];
  Event ev_free[2];                       // the kernels that read d_in[i] have finished
  bool used[2] = {false, false};
  std::vector<Event> ev_copied, ev_done;  // [nslots]
  std::vector<PinnedBuf<float2>> h_am, h_iq;   // [nslots*MAX_RX] pinned
  std::vector<PinnedBuf<float>> h_peak;   // [nslots] pinned
  std::vector<int> n_out, in_flight, n_chunks;
  std::vector<int> nrx;                   // [nslots] sub-receivers of the slot's submit (pysdr_rx_add may run before its collect)
  std::vector<std::vector<int>> chunk_nout;     // [nslots][chunks of the slot's last submit]
  std::vector<int> cx;                    // [nslots*MAX_RX]
  unsigned long long seq = 0;
  bool counted = false;                   // this ring is in its context's n_ingest
};

namespace {

std::mutex g_rocfft_mu;
int g_rocfft_users = 0;

// g[p][k] = h[p + up*k] * exp(-j*w*k), w = 2*pi*fword/2^32
void build_taps(const Decim& d, const double* h, int nt, uint32_t fword, float2* out) {
  for (int p = 0; p < d.up; ++p) {
    for (int k = 0; k < d.kpad; ++k) {
      const int j = p + d.up * k;
      float2 g = make_float2(0.f, 0.f);
      if (j < nt) {
        const uint32_t ph = (uint32_t)((uint64_t)fword * (uint64_t)k);   // mod 2^32
        const double ang = -2.0 * M_PI * ((double)(int32_t)ph / kTwo32);
        g.x = (float)(h[j] * std::cos(ang));
        g.y = (float)(h[j] * std::sin(ang));
      }
      out[(size_t)p * d.kpad + k] = g;
    }
  }
}

// All initial fills go to the context's own stream: it is a non-blocking stream, i.e. NOT ordered
// against the null stream a plain hipMemset runs on, and the first tap upload follows on it.
int decim_init(Decim& d, int up, int down, int ntaps, int max_rx, hipStream_t st) {
  d.up = up; d.down = down; d.ntaps = ntaps; d.max_rx = max_rx;
  d.kdec = (ntaps + up - 1) / up;
  d.kpad = (d.kdec + 15) / 16 * 16;
  d.hist_len = decim_hist_len(d.kpad);
  d.h_taps.assign((size_t)max_rx * d.per(), make_float2(0.f, 0.f));
  PYSDR_HIP_CHECK(d.d_hist.alloc_both_zeroed((size_t)d.hist_len, st));
  PYSDR_HIP_CHECK(d.d_taps.alloc_zeroed((size_t)max_rx * d.per(), st));      // (the last one: a decimator with taps is complete)
  return PYSDR_OK;
}

int decim_upload_taps(pysdr_ctx* c, Decim& d, int slot, const double* h, int nt, uint32_t fword) {
  float2* dst = d.h_taps.data() + (size_t)slot * d.per();
  build_taps(d, h, nt, fword, dst);
  PYSDR_HIP_CHECK(hipMemcpyAsync(d.d_taps.get() + (size_t)slot * d.per(), dst, d.per() * sizeof(float2),
                                 hipMemcpyHostToDevice, c->stream));
  return PYSDR_OK;
}

// The divisor of SRATE whose quotient is closest to 250 kHz
int wfm_if_decim(double srate) {
  const long long sr = (long long)std::llround(srate);
  long long best = 1;
  double bd = -1.0;
  const long long lim = std::max<long long>(2, sr / 100000);
  for (long long d = 1; d <= lim; ++d) {
    if (sr % d) continue;
    const double err = std::fabs((double)sr / (double)d - 250e3);
    if (bd < 0 || err < bd) { best = d; bd = err; }
  }
  return (int)best;
}

inline bool is_wfm(int m) { return m == PYSDR_WFM || m == PYSDR_WFM2; }

// One launch of the fused mix+decimate kernel on `nrx` receivers that share `d`.
struct DecimResult { int n_out; uint32_t t0; unsigned long long m0; };
int decim_run(pysdr_ctx* c, Decim& d, const float2* d_x, size_t n, int nrx, float2* const* y,
              const uint32_t* phase0, const uint32_t* fword, unsigned* peak, size_t chunk_len,
              int y_cap, DecimResult* res, hipStream_t st) {
  const int up = d.up, down = d.down;
  const unsigned long long s0 = d.s_abs, s1 = s0 + n;
  const unsigned long long m0 = (s0 * up + down - 1) / down, m1 = (s1 * up + down - 1) / down;
  const int n_out = (int)(m1 - m0);
  if (n_out > y_cap) { set_last_error("decimator: n_out %d > capacity %d", n_out, y_cap); return PYSDR_ERR_STATE; }
  if ((double)n * up + down >= 2147483647.0) { set_last_error("decimator: call too long for 31-bit indices"); return PYSDR_ERR_ARG; }
  // Which form runs -- the matrix-core one (one RX, a long prototype at a rate that has an instantiation), the small resampler
  // (one RX, no raw peak wanted, short prototype and a small DOWN/UP: the fs1 -> FS_OUT stage of broadcast FM) or the vector
  // kernel with its plan -- is plan_front_end's decision (mixdec_plan.h; pysdr_front_end_plan reports the same).  It depends
  // on the decimator's shape and its call site only -- never on the call -- so every call of a stream sums in the same order
  // (batch == chunk by chunk bit for bit), whatever the alignment of the caller's device pointer (the LDS-DMA takes any
  // 4-byte aligned source: scripts/diag/glds_align_test.hip).
  MixDecArgs a;
  memset(&a, 0, sizeof(a));
  a.n_out = n_out;
  a.up = up; a.down = down;
  a.kpad = d.kpad;
  a.nrx = nrx;
  const FrontEndPlan fe = plan_front_end(a, d.kdec, peak != nullptr, c->tune.tile_bytes, c->tune.threads, c->tune.wgs_per_cu,
                                         c->tune.yflush_cap, c->tune.mfma_enable);
  const int mshape = fe.mshape;
  MfmaPlan plan;
  if (mshape >= 0 && !mixdec_mfma_plan(mshape, s0, m0, n, &plan)) {
    // (falling through to the vector form here would sum THIS call in another order than its neighbours: an error instead)
    set_last_error("decimator: call of %zu samples too long for the matrix-core form (2^30 samples per call)", n);
    return PYSDR_ERR_ARG;
  }
  if (mshape >= 0) {
    MixMfmaArgs b;
    memset(&b, 0, sizeof(b));
    b.x = d_x;
    b.hist = d.d_hist.buf(d.hist_cur);
    b.hist_len = d.hist_len;
    b.n_total = (uint32_t)n;
    b.n_out = n_out;
    b.origin_rel0 = plan.origin_rel0; b.d = plan.d; b.nrel0 = plan.nrel0; b.mrel0 = plan.mrel0; b.ntiles = plan.ntiles;
    b.kpad = d.kpad;
    b.taps = d.d_taps.get();
    b.y = y[0];
    b.phase0 = phase0[0]; b.fword = fword[0];
    b.peak = peak ? peak : c->d_peak_scratch.get();
    b.chunk_len = peak ? (uint32_t)chunk_len : (uint32_t)std::max<size_t>(n, 1);
    b.magic_chunk = (b.chunk_len == 1) ? 0u : (uint32_t)(4294967296ULL / (unsigned long long)b.chunk_len) + 1u;
    // the history roll rides in the launch (hist_roll.h): the epilogue waves of workgroup 0 during their idle first trip
    b.hist_new = d.d_hist.buf(d.hist_cur ^ 1);
    b.zero = peak ? c->d_peak2.buf(c->peak_cur ^ 1) : nullptr;
    b.zero_n = peak ? c->cfg.max_chunks : 0;
#ifdef PYSDR_DIAG
    if ((c->tune.dbg_flags & 512) && !c->d_mm_stamps) {
      PYSDR_HIP_CHECK(c->d_mm_stamps.alloc(1024 * 24));
      PYSDR_HIP_CHECK(hipMemset(c->d_mm_stamps.get(), 0, 1024 * 24 * sizeof(unsigned long long)));
    }
    b.wg_stamps = (c->tune.dbg_flags & 512) ? c->d_mm_stamps.get() : nullptr;
#endif
    int rc = launch_mixdec_mfma(mshape, b, c->tune.grid_override > 0 ? c->tune.grid_override : c->num_cus, st);
    if (rc) return rc;
    if (peak) c->peak_clean[c->peak_cur ^ 1] = true;
    d.hist_cur ^= 1;
    d.s_abs = s1;
    if (res) { res->n_out = n_out; res->t0 = (uint32_t)(m0 * down - s0 * up); res->m0 = m0; }
    return PYSDR_OK;
  }
  const bool small = fe.form == PYSDR_FORM_SMALL;      // one thread per output (resamp_small.hip)
  const MdKey key = fe.key;
  if (!fe.fits) {
    set_last_error("decimator: filter (%d taps, %d rx, up %d) does not fit LDS", d.ntaps, nrx, up);
    return PYSDR_ERR_ARG;
  }
  a.x = d_x;
  a.hist = d.d_hist.buf(d.hist_cur);
  a.hist_len = d.hist_len;
  a.aligned16 = ((reinterpret_cast<uintptr_t>(d_x) & 15u) == 0) ? 1 : 0;
  a.n_total = (uint32_t)n;
  a.t0 = (uint32_t)(m0 * down - s0 * up);
  a.magic = (up == 1) ? 0u : (uint32_t)(4294967296ULL / (unsigned)up) + 1u;
  a.taps = d.d_taps.get();
  for (int r = 0; r < nrx; ++r) { a.y[r] = y[r]; a.phase0[r] = phase0[r]; a.fword[r] = fword[r]; }
  a.peak = peak ? peak : c->d_peak_scratch.get();
  a.chunk_len = peak ? (uint32_t)chunk_len : (uint32_t)std::max<size_t>(n, 1);
  a.magic_chunk = (a.chunk_len == 1) ? 0u : (uint32_t)(4294967296ULL / (unsigned long long)a.chunk_len) + 1u;
  a.dbg = c->tune.dbg_flags;
#ifdef PYSDR_DIAG
  if ((c->tune.dbg_flags & 256) && !c->d_stamps) {
    PYSDR_HIP_CHECK(c->d_stamps.alloc(2 * 16 * 24 * 8));
    PYSDR_HIP_CHECK(hipMemset(c->d_stamps.get(), 0, 2 * 16 * 24 * 8 * sizeof(unsigned long long)));
  }
  a.stamps = (c->tune.dbg_flags & 256) ? c->d_stamps.get() : nullptr;
#endif
  // the history roll rides in the launch (hist_roll.h: workgroup 0, while its first tile's copies are in flight)
  a.hist_new = d.d_hist.buf(d.hist_cur ^ 1);
  a.zero = peak ? c->d_peak2.buf(c->peak_cur ^ 1) : nullptr;
  a.zero_n = peak ? c->cfg.max_chunks : 0;
  int rc = small ? launch_resamp_small(a, c->tune.grid_override, c->tune.resamp_plain, st)
                 : launch_mixdec(a, key, c->tune.threads, c->tune.grid_override > 0 ? c->tune.grid_override : c->num_cus * c->tune.wgs_per_cu, st);
  if (rc) return rc;
  if (small && n_out <= 0) {          // the resampler starts no kernel for a call without outputs: the roll on its own
    rc = launch_hist_roll(d_x, d.d_hist.buf(d.hist_cur), d.d_hist.buf(d.hist_cur ^ 1), d.hist_len, (uint32_t)n, a.zero, a.zero_n, st);
    if (rc) return rc;
  }
  if (peak) c->peak_clean[c->peak_cur ^ 1] = true;
  d.hist_cur ^= 1;
  d.s_abs = s1;
  if (res) { res->n_out = n_out; res->t0 = a.t0; res->m0 = m0; }
  return PYSDR_OK;
}

int wfm_setup(pysdr_ctx* c) {
  if (c->wfm_front.d_taps) return PYSDR_OK;
  c->d1 = wfm_if_decim(c->cfg.srate);
  const double fs1 = c->cfg.srate / c->d1;
  const long long a = (long long)std::llround(std::floor(c->cfg.srate * c->cfg.up / c->cfg.down));
  const long long b = (long long)std::llround(fs1);
  long long g = std::__gcd(a, b);
  c->up2 = (int)(a / g);
  c->down2 = (int)(b / g);
  c->m1max = (int)(c->cap_samples / (size_t)c->d1) + 4;
  return decim_init(c->wfm_front, 1, c->d1, c->cfg.ntaps_dec, PYSDR_MAX_RX, c->stream);
}

int flush_tail(pysdr_ctx* c);

int apply_pending(pysdr_ctx* c, CallSnap* snap) {
  std::lock_guard<std::mutex> lk(c->mu);
  snap->nrx = c->nrx;
  snap->nwfm = 0;
  for (int r = 0; r < c->nrx; ++r) snap->nwfm += is_wfm(c->rx[r].mode) ? 1 : 0;
  if (snap->nwfm != 0 && snap->nwfm != c->nrx) {
    // the reference's mode is global (P.MODE) and the rate-reduction order differs for
    // broadcast FM (receiver.py:718-719): one context runs one pipeline
    set_last_error("pysdr_process_batch: WFM/WFM2 cannot be mixed with narrow-band modes in one context");
    return PYSDR_ERR_STATE;
  }
  // Overlapping calls: a deferred tail belongs to the PREVIOUS call and must see the taps / AGC settings / buffers of that
  // call, so whatever a setter left to do (taps, resets, buffers) and any change of form first flushes it and drains both
  // streams -- it is rare, and everything below may then go on `stream` as in the single-stream form (drained again at
  // the end, so that the loop walks on stream2 see it).
  bool drained = false;
  snap->use2 = c->overlap >= 2;
  for (int r = 0; r < c->nrx && c->overlap == 1; ++r)
    snap->use2 |= (c->rx[r].mode == PYSDR_AM_SYNCH || c->rx[r].mode == PYSDR_WFM2);
  // the second buffer of every pair exists while the calls overlap AND afterwards for as long as the current buffer is the
  // second one (par only moves in overlapped calls; a single-stream call stays on whichever buffer is current)
  const bool need_alt = snap->use2 || c->par != 0;
  bool dirty = snap->use2 != c->use2;
  for (int r = 0; r < c->nrx && (need_alt || c->tail.valid); ++r) {
    const RxHost& x = c->rx[r];
    dirty |= x.taps_dirty || x.af_dirty || x.agc_dirty || x.reset_pending != 0 || (is_wfm(x.mode) && x.wfm_dirty) ||
             (x.mode == PYSDR_AM_SYNCH && (!x.d_ypll || (need_alt && x.d_ypll.lacks_second()))) ||
             (x.mode == PYSDR_WFM2 && !x.d_seed && c->tune.wfm_seeded) ||
             (need_alt && (x.d_y.lacks_second() || x.d_y1.lacks_second()));
  }
  if (dirty) {
    int rc = flush_tail(c);
    if (rc) return rc;
    PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (c->stream2) PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream2));
    if (snap->use2 && !c->stream2) {
      // The second stream exists from the first call that uses it, not from pysdr_set_overlap: the runtime maps streams
      // onto a handful of hardware queues, and an IDLE fifth stream beside a spectrum's two made the PSD's streams share
      // one (measured, same box: C3's PSD call 2.39 -> 2.95 ms, at a low priority 3.6 ms; scripts/diag/ab_r04.sh).
      // LOW priority: where both have work the dispatcher places the front end's workgroups first (they are persistent
      // over a static share of the tiles: one that starts late ends late, and the launch with it).
      int lo = 0, hi = 0;
      PYSDR_HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
      for (int i = 0; i < 2; ++i) PYSDR_HIP_CHECK(c->ev_pll[i].create(hipEventDisableTiming));
      PYSDR_HIP_CHECK(c->stream2.create(hipStreamNonBlocking, c->tune.overlap_prio_set ? c->tune.overlap_prio : lo));   // (the last one: its presence says all three exist)
    }
    c->use2 = snap->use2;
    drained = true;
  }
  for (int r = 0; r < c->nrx; ++r) {
    RxHost& x = c->rx[r];
    if (x.taps_dirty) {
      int rc = decim_upload_taps(c, c->main, r, x.h.data(), c->cfg.ntaps_dec, x.fword);
      if (rc) return rc;
      x.taps_dirty = false;
      x.wfm_dirty = true;             // the LO moved: the WFM front taps carry it too
    }
    if (is_wfm(x.mode) && x.wfm_dirty) {
      if (x.wfm_video.empty() || x.wfm_resamp.empty()) {
        set_last_error("rx %d is in WFM mode but pysdr_set_wfm_taps was never called", r);
        return PYSDR_ERR_STATE;
      }
      int rc = wfm_setup(c);
      if (rc) return rc;
      if (!x.wfm_audio.d_taps) {              // (the last of the three to come into being)
        PYSDR_HIP_CHECK(x.d_y1.first.alloc_zeroed((size_t)c->m1max + 2, c->stream));
        drained = drained || need_alt;        // (the pair's second buffer follows below)
        PYSDR_HIP_CHECK(x.d_w.first.alloc((size_t)c->m1max));
        rc = decim_init(x.wfm_audio, c->up2, c->down2, (int)x.wfm_resamp.size(), 1, c->stream);
        if (rc) return rc;
      }
      rc = decim_upload_taps(c, c->wfm_front, r, x.wfm_video.data(), c->cfg.ntaps_dec, x.fword);
      if (rc) return rc;
      rc = decim_upload_taps(c, x.wfm_audio, 0, x.wfm_resamp.data(), (int)x.wfm_resamp.size(), 0u);
      if (rc) return rc;
      x.wfm_dirty = false;
    }
    if (x.af_dirty) {
      std::vector<float2> t((c->cfg.ntaps_af + 7) & ~7, make_float2(0.f, 0.f));
      x.taps_real = 1;
      for (int k = 0; k < c->cfg.ntaps_af; ++k) {
        t[k] = make_float2((float)x.af[2 * k], (float)x.af[2 * k + 1]);
        if (t[k].y != 0.f) x.taps_real = 0;
      }
      PYSDR_HIP_CHECK(hipMemcpyAsync(x.d_aftaps.get(), t.data(), t.size() * sizeof(float2),
                                     hipMemcpyHostToDevice, c->stream));
      PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream));   // t goes out of scope
      x.af_dirty = false;
    }
    if (x.reset_pending) {
      RxDevState st;
      PYSDR_HIP_CHECK(hipMemcpyAsync(&st, c->d_state.get() + r, sizeof(st), hipMemcpyDeviceToHost, c->stream));
      PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream));
      if (x.reset_pending & 1u) { st.env = 0.f; st.gain = 1.f; st.maxbuf = 0.f; st.err = 0.f; st.sq_level = 0.f; st.sq_open = 1; st.sq_lp = 0.f; st.sq_hp = 0.f; }
      if (x.reset_pending & 2u) { st.pll_phase = 0u; st.pll_w = 0.f; st.wfm_phase = 0u; st.wfm_w = 0.f; st.wfm_slope_ok = 0; }
      st.ref = x.agc_ref; st.agc_enable = x.agc_enable;
      PYSDR_HIP_CHECK(hipMemcpyAsync(c->d_state.get() + r, &st, sizeof(st), hipMemcpyHostToDevice, c->stream));
      PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream));
      x.reset_pending = 0; x.agc_dirty = false;
    }
    if (x.agc_dirty) {
      PYSDR_HIP_CHECK(hipMemcpyAsync(&(c->d_state.get() + r)->ref, &x.agc_ref, sizeof(float), hipMemcpyHostToDevice, c->stream));
      PYSDR_HIP_CHECK(hipMemcpyAsync(&(c->d_state.get() + r)->agc_enable, &x.agc_enable, sizeof(int), hipMemcpyHostToDevice, c->stream));
      PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream));
      x.agc_dirty = false;
    }
    if (x.mode == PYSDR_WFM2 && !x.d_seed && c->tune.wfm_seeded && c->m1max > 0) {
      PYSDR_HIP_CHECK(x.d_mnt.alloc_both_zeroed(pll_seed_mnt_floats(c->m1max), c->stream));
      PYSDR_HIP_CHECK(x.d_seed.alloc(pll_seed_doubles(c->m1max)));
    }
    if (x.mode == PYSDR_AM_SYNCH && !x.d_ypll)
      PYSDR_HIP_CHECK(x.d_ypll.first.alloc_zeroed((size_t)c->hy + c->mmax, c->stream));
    if (need_alt) {
      // the history prefix a second buffer inherits when it comes into being as the current one (BufPair::ensure_second)
      if (x.d_ypll) PYSDR_HIP_CHECK(x.d_ypll.ensure_second(c->stream, c->par, (size_t)c->hy));
      PYSDR_HIP_CHECK(x.d_y.ensure_second(c->stream, c->par, (size_t)c->hy));
      if (x.d_y1) PYSDR_HIP_CHECK(x.d_y1.ensure_second(c->stream, c->par, 2));
      if (x.d_w.lacks_second()) PYSDR_HIP_CHECK(x.d_w.alloc_second());
    }
    RxSnap& q = snap->rx[r];
    q.mode = x.mode; q.fword = x.fword; q.phase = x.phase; q.bfo_fword = x.bfo_fword;
    q.sq_thresh = x.sq_thresh; q.sq_ratio = x.sq_ratio; q.taps_real = x.taps_real;
    q.d_a = x.d_a.get(); q.d_am = x.d_am.get(); q.d_aftaps = x.d_aftaps.get();
    q.d_seed = x.d_seed.get();
    // this call's buffer of each pair and the next call's (the other one when the calls overlap)
    const int p = c->par;
    q.d_mnt = x.d_mnt.cur(p);
    q.d_y = x.d_y.cur(p);       q.d_y_next = x.d_y.next(p, snap->use2);
    q.d_ypll = x.d_ypll.cur(p); q.d_ypll_next = x.d_ypll.next(p, snap->use2);
    q.d_y1 = x.d_y1.cur(p);     q.d_y1_next = x.d_y1.next(p, snap->use2);
    q.d_w = x.d_w.cur(p);
  }
  if (drained) PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream));
  return PYSDR_OK;
}

// Stage2Args of a call from its snapshot (everything but the carrier-loop plan)
void fill_stage2(pysdr_ctx* c, const CallSnap& snap, bool wfm, int nchunks, size_t chunk_len, const DecimResult& res,
                 Stage2Args* out) {
  Stage2Args& s = *out;
  memset(&s, 0, sizeof(s));
  const int up = c->cfg.up, down = c->cfg.down, nrx = snap.nrx;
  s.nrx = nrx; s.n_out = res.n_out; s.ntaps = c->cfg.ntaps_af; s.hy = c->hy;
  s.t0 = res.t0; s.up = up; s.down = down; s.chunk_len = (uint32_t)chunk_len; s.nchunks = nchunks;
  s.m0_lo = (uint32_t)(res.m0 & 0xFFFFFFFFull);
  const double fs_out = std::floor(c->cfg.srate * up / down);
  s.fm_scale = (float)(fs_out / (2.0 * M_PI * kNfmFullScaleDev));
  const double wn = 2.0 * M_PI * kPllBwHz / fs_out;
  s.pll_kp = (float)(2.0 * kPllZeta * wn);
  s.pll_ki = (float)(wn * wn);
  for (int r = 0; r < nrx; ++r) {
    const RxSnap& x = snap.rx[r];
    s.y[r] = x.d_y + c->hy;
    s.ypll[r] = x.d_ypll ? x.d_ypll + c->hy : nullptr;
    s.aftaps[r] = x.d_aftaps;
    s.taps_real[r] = x.taps_real;
    s.a[r] = x.d_a;
    s.am[r] = x.d_am;
    s.det[r] = mode_detector(x.mode);
    s.out_complex[r] = (x.mode == PYSDR_IQ || wfm) ? 1 : 0;
    s.fir_complex[r] = s.out_complex[r];
    s.single_block[r] = wfm ? 1 : 0;
    s.single_spread = 1;
    while (s.single_spread * 2 <= std::min(nchunks, 32)) s.single_spread *= 2;
    s.matrix[r] = (x.mode == PYSDR_WFM2) ? 1 : 0;
    s.bfo_fword[r] = x.bfo_fword;
    s.sq_ratio[r] = (x.sq_ratio > 0.f && c->d_sqtaps) ? 1 : 0;
    s.sq_thresh[r] = s.sq_ratio[r] ? x.sq_ratio : x.sq_thresh;
  }
  s.blkpeak = c->d_blkpeak.get(); s.gain = c->d_gain.get(); s.state = c->d_state.get();
  s.blknoise = c->d_blknoise.get(); s.blkcnt = c->d_blkcnt.get();
  s.blknoise2 = c->d_blknoise2.get(); s.sqtaps = c->d_sqtaps.get(); s.sq_ntaps = c->sq_ntaps;
}

// T: the tail of a call on `stream` -- for broadcast FM the audio resamplers first, then detector + AF FIR, the block
// gains (+ the history rolls into the next call's buffers) and the output stage.  Called at the end of the call itself
// (single-stream form) or from the NEXT call / a flush (deferred).
int run_tail(pysdr_ctx* c, TailJob& j) {
  j.valid = false;
  const CallSnap& snap = j.snap;
  const int nrx = snap.nrx;
  if (j.wait_pll) PYSDR_HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_pll[j.par], 0));
  Stage2Args& s = j.s;
  int rc;
  if (j.wfm) {
    DecimResult res;
    const uint32_t zero = 0u;
    for (int r = 0; r < nrx; ++r) {
      float2* y1 = snap.rx[r].d_y + c->hy;
      rc = decim_run(c, c->rx[r].wfm_audio, snap.rx[r].d_w, (size_t)j.n1, 1, &y1, &zero, &zero, nullptr, 0,
                     c->mmax, &res, c->stream);
      if (rc) return rc;
    }
    fill_stage2(c, snap, true, j.nchunks, j.chunk_len, res, &s);
  }
  const int n_out = s.n_out;
  rc = launch_demod_fir(s, c->stream); if (rc) return rc;
  // the gains, and beside them (same launch) the history roll of the FS_OUT-rate buffers: the AF FIR was their last reader
  EpilogueArgs e;
  memset(&e, 0, sizeof(e));
  e.nrx = nrx; e.n_out = n_out; e.hy = c->hy;
  for (int r = 0; r < nrx; ++r) {
    e.ybase[r] = snap.rx[r].d_y;
    e.ydst[r] = snap.rx[r].d_y_next;
    e.ypllbase[r] = (s.det[r] == kDetPll) ? snap.rx[r].d_ypll : nullptr;
    e.yplldst[r] = (s.det[r] == kDetPll) ? snap.rx[r].d_ypll_next : nullptr;
  }
  rc = launch_agc_scan(s, e, c->stream); if (rc) return rc;
  // WFM (mono) emits the real part of the complex pipeline
  for (int r = 0; r < nrx; ++r) if (snap.rx[r].mode == PYSDR_WFM) s.out_complex[r] = 0;
  rc = launch_apply(s, c->stream); if (rc) return rc;
  if (j.ev_end) PYSDR_HIP_CHECK(hipEventRecord(j.ev_end, c->stream));
  for (int r = 0; r < nrx; ++r) c->last_complex[r] = (snap.rx[r].mode == PYSDR_IQ || snap.rx[r].mode == PYSDR_WFM2) ? 1 : 0;
  c->last_par = j.par;
  c->last_nrx = nrx;
  c->last_nout = n_out; c->last_nchunks = j.nchunks;
  c->last_chunk_len = j.chunk_len; c->last_s0 = j.s0; c->last_wfm = j.wfm ? 1 : 0;
  return PYSDR_OK;
}

// Whatever asks for a call's results (fetch, sync, the state getters, a setter's pending work, a spectrum that orders
// itself behind the whole demodulation) first queues its deferred tail.
int flush_tail(pysdr_ctx* c) {
  if (!c->tail.valid) return PYSDR_OK;
  return run_tail(c, c->tail);
}

// The device allocations of a new context and their initial fills
int ctx_alloc(pysdr_ctx* c) {
  const pysdr_cfg& cfg = c->cfg;
  const size_t nblk = (size_t)PYSDR_MAX_RX * cfg.max_chunks;
  PYSDR_HIP_CHECK(c->stream.create(hipStreamNonBlocking));
  int rc = decim_init(c->main, cfg.up, cfg.down, cfg.ntaps_dec, PYSDR_MAX_RX, c->stream);
  if (rc) return rc;
  PYSDR_HIP_CHECK(c->d_peak2.alloc_both_zeroed((size_t)cfg.max_chunks, c->stream));
  PYSDR_HIP_CHECK(c->d_peak_scratch.alloc(64));
  PYSDR_HIP_CHECK(c->d_blkpeak.alloc_zeroed(nblk * kBlkStride, c->stream));
  PYSDR_HIP_CHECK(c->d_gain.alloc(nblk));
  PYSDR_HIP_CHECK(c->d_blknoise.alloc_zeroed(nblk * kBlkStride, c->stream));
  PYSDR_HIP_CHECK(c->d_blkcnt.alloc_zeroed(nblk * kBlkStride, c->stream));
  PYSDR_HIP_CHECK(c->d_state.alloc_zeroed(PYSDR_MAX_RX, c->stream));
  PYSDR_HIP_CHECK(c->d_pllseg.alloc((size_t)PYSDR_MAX_RX * kPllSegMax * 5));
  for (int k = 0; k < pysdr_ctx::kSlots; ++k)
    for (int i = 0; i < 4; ++i) PYSDR_HIP_CHECK(c->ev[k][i].create());
  PYSDR_HIP_CHECK(c->ev_front.create(hipEventDisableTiming));
  return PYSDR_OK;
}

// What the six state getters share: the deferred tail queued (its wait for the loop walks orders `stream` behind
// stream2 as well), then RxDevState[irx] as it stands behind everything queued
int read_rx_state(pysdr_ctx* c, int irx, RxDevState* d) {
  if (!c || irx < 0 || irx >= c->nrx) return PYSDR_ERR_ARG;
  std::lock_guard<std::recursive_mutex> run_lk(c->run_mu);
  int rc = use_device(c->cfg.device);
  if (rc) return rc;
  rc = flush_tail(c);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipMemcpyAsync(d, c->d_state.get() + irx, sizeof(*d), hipMemcpyDeviceToHost, c->stream));
  PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream));
  return PYSDR_OK;
}

}  // namespace

extern "C" {

const char* pysdr_strerror(int status) {
  switch (status) {
    case PYSDR_OK: return "ok";
    case PYSDR_ERR_ARG: return "bad argument";
    case PYSDR_ERR_NO_DEVICE: return "no HIP device";
    case PYSDR_ERR_HIP: return "HIP runtime error";
    case PYSDR_ERR_FFT: return "rocFFT error";
    case PYSDR_ERR_STATE: return "bad state / capacity exceeded";
    case PYSDR_ERR_RCCL: return "RCCL error";
    default: return "unknown status";
  }
}

const char* pysdr_last_error(void) { return g_err; }

int pysdr_version(void) { return 100; }

int pysdr_device_count(int* n) {
  if (!n) return PYSDR_ERR_ARG;
  int k = 0;
  hipError_t e = hipGetDeviceCount(&k);
  if (e != hipSuccess) {
    *n = 0;
    set_last_error("hipGetDeviceCount: %s", hipGetErrorString(e));
    return PYSDR_ERR_NO_DEVICE;
  }
  *n = k;
  return PYSDR_OK;
}

uint32_t pysdr_freq_word(double f_hz, double fs_hz, double* f_actual) {
  const double w = std::nearbyint(f_hz / fs_hz * kTwo32);
  long long wi = (long long)w;
  long long ws = ((wi + (1LL << 31)) % (1LL << 32) + (1LL << 32)) % (1LL << 32) - (1LL << 31);
  if (f_actual) *f_actual = (double)ws * fs_hz / kTwo32;
  return (uint32_t)(ws & 0xFFFFFFFFLL);
}

int pysdr_create(const pysdr_cfg* cfg, pysdr_ctx** out) {
  if (!cfg || !out) return PYSDR_ERR_ARG;
  if (cfg->up < 1 || cfg->down < 1 || cfg->in_chunk < 1 || cfg->max_chunks < 1 ||
      cfg->ntaps_dec < 1 || cfg->ntaps_af < 1 || cfg->ntaps_af > 2048 || cfg->srate <= 0) {
    set_last_error("pysdr_create: invalid cfg");
    return PYSDR_ERR_ARG;
  }
  if (cfg->max_chunks > 16384) {
    // agc_scan_kernel holds two words per AGC block of a call (+ 1/16 padding) in LDS: 160 KB end at ~19 k blocks
    set_last_error("pysdr_create: max_chunks %d > 16384 (the AGC scan keeps a call's blocks in LDS)", cfg->max_chunks);
    return PYSDR_ERR_ARG;
  }
  int rc = use_device(cfg->device);
  if (rc) return rc;
  pysdr_ctx* c = new pysdr_ctx();
  c->cfg = *cfg;
  c->hy = fir_history(cfg->ntaps_af);
  c->cap_samples = (size_t)cfg->max_chunks * (size_t)cfg->in_chunk;
  c->tune = Tuning::from_env();
  c->mmax = (int)((c->cap_samples * (size_t)cfg->up) / (size_t)cfg->down) + 4;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0)
      c->num_cus = prop.multiProcessorCount;
  }
  if ((double)c->cap_samples * cfg->up + cfg->down >= 2147483647.0) {
    // the same bound decim_run enforces per call (31-bit index arithmetic in the kernel)
    set_last_error("pysdr_create: max_chunks*in_chunk*up must stay below 2^31");
    delete c;
    return PYSDR_ERR_ARG;
  }
  rc = ctx_alloc(c);
  if (rc) { failed_in("pysdr_create", rc); pysdr_destroy(c); return rc; }
  if (c->tune.overlap_env >= 1) { rc = pysdr_set_overlap(c, c->tune.overlap_env); if (rc) { pysdr_destroy(c); return rc; } }
  *out = c;
  return PYSDR_OK;
}

void pysdr_destroy(pysdr_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->cfg.device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->stream2) (void)hipStreamSynchronize(c->stream2);
  pysdr_comm_destroy(c);
  delete c;                               // (the owners free: host_res.h)
}

int pysdr_rx_add(pysdr_ctx* c, int mode, double lo_freq, const double* h, const double* af,
                 double bfo, int* irx) {
  if (!c || !h || !af) return PYSDR_ERR_ARG;
  if (mode < 0 || mode > PYSDR_RTTY) return PYSDR_ERR_ARG;
  int rc = use_device(c->cfg.device);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  if (c->nrx >= PYSDR_MAX_RX) {
    set_last_error("pysdr_rx_add: more than %d receivers", PYSDR_MAX_RX);
    return PYSDR_ERR_STATE;
  }
  const int r = c->nrx;
  RxHost& x = c->rx[r];
  x.mode = mode;
  x.lo_freq = lo_freq;
  x.fword = pysdr_freq_word(lo_freq, c->cfg.srate, nullptr);
  x.phase = 0;
  x.h.assign(h, h + c->cfg.ntaps_dec);
  x.af.assign(af, af + 2 * c->cfg.ntaps_af);
  x.bfo = bfo;
  const double fs_out = c->cfg.srate * c->cfg.up / c->cfg.down;
  x.bfo_fword = pysdr_freq_word(bfo, std::floor(fs_out), nullptr);
  x.agc_enable = mode_has_agc(mode);
  x.taps_dirty = x.af_dirty = x.agc_dirty = true;
  x.reset_pending = 3;
  // (a call that fails here leaves nrx as it was: the next pysdr_rx_add takes the slot over, and what it already holds is freed)
  PYSDR_HIP_CHECK(x.d_y.first.alloc_zeroed((size_t)c->hy + c->mmax, c->stream));
  PYSDR_HIP_CHECK(x.d_a.alloc((size_t)c->mmax));
  PYSDR_HIP_CHECK(x.d_am.alloc((size_t)c->mmax * 2));
  PYSDR_HIP_CHECK(x.d_aftaps.alloc((size_t)((c->cfg.ntaps_af + 7) & ~7)));
  c->nrx = r + 1;
  if (irx) *irx = r;
  return PYSDR_OK;
}

int pysdr_set_lo(pysdr_ctx* c, int irx, double f_hz, double* f_actual) {
  if (!c || irx < 0 || irx >= c->nrx) return PYSDR_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  RxHost& x = c->rx[irx];
  x.lo_freq = f_hz;
  x.fword = pysdr_freq_word(f_hz, c->cfg.srate, f_actual);
  x.taps_dirty = true;
  return PYSDR_OK;
}

int pysdr_set_dec_taps(pysdr_ctx* c, int irx, const double* h, int n) {
  if (!c || !h || irx < 0 || irx >= c->nrx) return PYSDR_ERR_ARG;
  if (n != c->cfg.ntaps_dec) {
    set_last_error("pysdr_set_dec_taps: got %d taps, context was created for %d", n, c->cfg.ntaps_dec);
    return PYSDR_ERR_ARG;
  }
  std::lock_guard<std::mutex> lk(c->mu);
  c->rx[irx].h.assign(h, h + n);
  c->rx[irx].taps_dirty = true;
  return PYSDR_OK;
}

int pysdr_set_mode(pysdr_ctx* c, int irx, int mode, const double* af, int n, double bfo) {
  if (!c || irx < 0 || irx >= c->nrx || mode < 0 || mode > PYSDR_RTTY) return PYSDR_ERR_ARG;
  if (af && n != c->cfg.ntaps_af) {
    set_last_error("pysdr_set_mode: got %d AF taps, context was created for %d", n, c->cfg.ntaps_af);
    return PYSDR_ERR_ARG;
  }
  std::lock_guard<std::mutex> lk(c->mu);
  RxHost& x = c->rx[irx];
  x.mode = mode;
  if (af) { x.af.assign(af, af + 2 * n); x.af_dirty = true; }
  x.bfo = bfo;
  const double fs_out = std::floor(c->cfg.srate * c->cfg.up / c->cfg.down);
  x.bfo_fword = pysdr_freq_word(bfo, fs_out, nullptr);
  x.agc_enable = mode_has_agc(mode);
  x.agc_dirty = true;
  return PYSDR_OK;
}

int pysdr_reset(pysdr_ctx* c, int irx, unsigned what) {
  if (!c || irx < 0 || irx >= c->nrx) return PYSDR_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  c->rx[irx].reset_pending |= (what & 3u);
  return PYSDR_OK;
}

int pysdr_set_agc(pysdr_ctx* c, int irx, int enable, float ref) {
  if (!c || irx < 0 || irx >= c->nrx || !(ref > 0.f)) return PYSDR_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  c->rx[irx].agc_enable = enable ? 1 : 0;
  c->rx[irx].agc_ref = ref;
  c->rx[irx].agc_dirty = true;
  return PYSDR_OK;
}

int pysdr_set_squelch(pysdr_ctx* c, int irx, float thresh) {
  if (!c || irx < 0 || irx >= c->nrx) return PYSDR_ERR_ARG;
  std::lock_guard<std::mutex> lk(c->mu);
  c->rx[irx].sq_thresh = thresh > 0.f ? thresh : 0.f;
  return PYSDR_OK;
}

int pysdr_set_squelch_ratio(pysdr_ctx* c, int irx, float min_ratio, const float* lp, const float* hp, int ntaps) {
  if (!c || irx < 0 || irx >= c->nrx || (min_ratio > 0.f && (!lp || !hp || ntaps < 1 || ntaps > kSqTapsMax))) return PYSDR_ERR_ARG;
  // (before anything is allocated, uploaded or changed: the taps are the context's, and a refused call for one sub-receiver
  // leaves the armed squelch of another as it was)
  if (min_ratio > 0.f && ntaps > sq_taps_bound(c->cfg.ntaps_af)) {
    set_last_error("pysdr_set_squelch_ratio: squelch filters of %d taps beside an AF filter of %d taps: at most %d (the AF stage "
                   "stages and keeps no more detector history)", ntaps, c->cfg.ntaps_af, sq_taps_bound(c->cfg.ntaps_af));
    return PYSDR_ERR_ARG;
  }
  std::lock_guard<std::recursive_mutex> run_lk(c->run_mu);     // allocates and uploads on the context's stream
  int rc = use_device(c->cfg.device);
  if (rc) return rc;
  if (min_ratio > 0.f) {
    if (!c->d_blknoise2) PYSDR_HIP_CHECK(c->d_blknoise2.alloc_zeroed((size_t)PYSDR_MAX_RX * c->cfg.max_chunks * kBlkStride, c->stream));
    if (!c->d_sqtaps) PYSDR_HIP_CHECK(c->d_sqtaps.alloc(2 * kSqTapsMax));
    float h[2 * kSqTapsMax] = {0.f};
    for (int q = 0; q < ntaps; ++q) { h[q] = lp[q]; h[kSqTapsMax + q] = hp[q]; }
    // (the two FIRs belong to the context -- they depend on FS_OUT only; pageable source: the copy is staged before the call returns)
    PYSDR_HIP_CHECK(hipMemcpyAsync(c->d_sqtaps.get(), h, sizeof(h), hipMemcpyHostToDevice, c->stream));
    PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->sq_ntaps = ntaps;
  }
  std::lock_guard<std::mutex> lk(c->mu);
  c->rx[irx].sq_ratio = min_ratio > 0.f ? min_ratio : 0.f;
  return PYSDR_OK;
}

int pysdr_squelch_ratio_get(pysdr_ctx* c, int irx, float* sq_lp, float* sq_hp, int* open) {
  RxDevState d;
  const int rc = read_rx_state(c, irx, &d);
  if (rc) return rc;
  if (sq_lp) *sq_lp = d.sq_lp;
  if (sq_hp) *sq_hp = d.sq_hp;
  if (open) *open = d.sq_open;
  return PYSDR_OK;
}

int pysdr_squelch_get(pysdr_ctx* c, int irx, float* level, int* open) {
  RxDevState d;
  const int rc = read_rx_state(c, irx, &d);
  if (rc) return rc;
  if (level) *level = d.sq_level;
  if (open) *open = d.sq_open;
  return PYSDR_OK;
}

int pysdr_pll_stats(pysdr_ctx* c, int irx, int* segments, int* patched) {
  RxDevState d;
  const int rc = read_rx_state(c, irx, &d);
  if (rc) return rc;
  if (segments) *segments = d.pll_segments;
  if (patched) *patched = d.pll_patched;
  return PYSDR_OK;
}

int pysdr_pll_linear_starts(pysdr_ctx* c, int irx, int* n) {
  if (!n) return PYSDR_ERR_ARG;
  RxDevState d;
  const int rc = read_rx_state(c, irx, &d);
  if (rc) return rc;
  *n = d.pll_linear;
  return PYSDR_OK;
}

int pysdr_pll_join_margin(pysdr_ctx* c, int irx, int* max_words, float* max_dw) {
  RxDevState d;
  const int rc = read_rx_state(c, irx, &d);
  if (rc) return rc;
  if (max_words) *max_words = d.pll_join_words;
  if (max_dw) *max_dw = d.pll_join_dw;
  return PYSDR_OK;
}

int pysdr_set_pll_segments(pysdr_ctx* c, int max_segments) {
  if (!c || max_segments < 0) return PYSDR_ERR_ARG;
  c->pll_kmax = max_segments;
  return PYSDR_OK;
}

int pysdr_agc_get(pysdr_ctx* c, int irx, pysdr_agc_state* st) {
  if (!st) return PYSDR_ERR_ARG;
  RxDevState d;
  const int rc = read_rx_state(c, irx, &d);
  if (rc) return rc;
  st->agc = d.env; st->gain = d.gain; st->maxbuf = d.maxbuf; st->ref = d.ref; st->err = d.err;
  return PYSDR_OK;
}

#ifdef PYSDR_DIAG
// diagnostic build only: where every workgroup of the last mixdec_mfma launch ran and at what clock, [1024][24] uint64
extern "C" int pysdr_diag_mfma_stamps(pysdr_ctx* c, unsigned long long* host) {
  if (!c || !host || !c->d_mm_stamps) return PYSDR_ERR_ARG;
  PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream));
  PYSDR_HIP_CHECK(hipMemcpy(host, c->d_mm_stamps.get(), 1024 * 24 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return PYSDR_OK;
}
// diagnostic build only: the last launch's mixdec phase stamps, [2][16][24][8] uint64
extern "C" int pysdr_diag_stamps(pysdr_ctx* c, unsigned long long* host) {
  if (!c || !host || !c->d_stamps) return PYSDR_ERR_ARG;
  PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream));
  PYSDR_HIP_CHECK(hipMemcpy(host, c->d_stamps.get(), 2 * 16 * 24 * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return PYSDR_OK;
}
#endif

int pysdr_build_flags_hash(void) {
#ifdef PYSDR_EXTRA_FLAGS_HASH
  return (int)(PYSDR_EXTRA_FLAGS_HASH);
#else
  return 0;
#endif
}

int pysdr_get_tuning(pysdr_ctx* c, int32_t out[8]) {
  if (!c || !out) return PYSDR_ERR_ARG;
#ifdef PYSDR_DIAG
  out[0] = 1;
#else
  out[0] = 0;
#endif
  const Tuning& t = c->tune;
  out[1] = t.dbg_flags; out[2] = t.wgs_per_cu; out[3] = t.yflush_cap;
  out[4] = t.tile_bytes; out[5] = t.threads; out[6] = c->num_cus; out[7] = t.mfma_enable;
  return PYSDR_OK;
}

int pysdr_set_profile(pysdr_ctx* c, int enable) {
  if (!c) return PYSDR_ERR_ARG;
  c->profile = enable;
  return PYSDR_OK;
}

int pysdr_set_tile(pysdr_ctx* c, int tile_bytes, int threads) {
  if (!c || (tile_bytes != 0 && (tile_bytes < 4096 || tile_bytes > 150 * 1024)) || threads < 64 || threads > 1024 ||
      (threads & 63))
    return PYSDR_ERR_ARG;
  c->tune.tile_bytes = tile_bytes;
  c->tune.threads = threads;
  return PYSDR_OK;
}

int pysdr_front_end_plan(int nrx, int up, int down, int ntaps, int tile_bytes, int threads, int wgs_per_cu, int yflush_cap,
                         int mfma_enable, int want_peak, int32_t out[12]) {
  if (!out || nrx < 1 || nrx > PYSDR_MAX_RX || up < 1 || down < 1 || ntaps < 1 || wgs_per_cu < 1 || yflush_cap < 0 ||
      (tile_bytes != 0 && (tile_bytes < 4096 || tile_bytes > 150 * 1024)) || threads < 64 || threads > 1024 || (threads & 63))
    return PYSDR_ERR_ARG;
  // the shape as decim_init derives it, the decision as decim_run takes it
  const int kdec = (ntaps + up - 1) / up;
  MixDecArgs a;
  memset(&a, 0, sizeof(a));
  a.nrx = nrx; a.up = up; a.down = down;
  a.kpad = (kdec + 15) / 16 * 16;
  const FrontEndPlan fe = plan_front_end(a, kdec, want_peak != 0, tile_bytes, threads, wgs_per_cu, yflush_cap, mfma_enable);
  const bool vec = fe.form != PYSDR_FORM_MFMA;
  out[0] = fe.form; out[1] = fe.fits ? 1 : 0;
  out[2] = vec ? fe.key.r : 0; out[3] = vec ? fe.key.nj : 0; out[4] = vec ? fe.key.tpb : 0; out[5] = vec ? fe.key.mm : 0;
  out[6] = fe.mshape;
  out[7] = a.taps_lds; out[8] = a.tile_out; out[9] = a.yflush; out[10] = a.tile_cap; out[11] = a.kpad;
  return PYSDR_OK;
}

int pysdr_front_end_shapes(int family, int index, int32_t out[4], int* count) {
  static const int32_t vec[][4] = {
#define PYSDR_SHAPE_ROW(R, NJ, TPB, MM) {R, NJ, TPB, MM},
      PYSDR_MIXDEC_SHAPES(PYSDR_SHAPE_ROW)
#undef PYSDR_SHAPE_ROW
  };
  static const int32_t mm[][4] = {
#define PYSDR_SHAPE_ROW(ID, UP, DOWN, S, KT, NB, WK, NP, NBUF, CARRY) {ID, UP, DOWN, KT},
      PYSDR_MFMA_SHAPES(PYSDR_SHAPE_ROW)
#undef PYSDR_SHAPE_ROW
  };
  if (family != PYSDR_FORM_VECTOR && family != PYSDR_FORM_MFMA) return PYSDR_ERR_ARG;
  const int32_t (*tab)[4] = family == PYSDR_FORM_VECTOR ? vec : mm;
  const int n = family == PYSDR_FORM_VECTOR ? (int)(sizeof(vec) / sizeof(vec[0])) : (int)(sizeof(mm) / sizeof(mm[0]));
  if (count) *count = n;
  if (index < 0 || index >= n) return (out == nullptr && count != nullptr) ? PYSDR_OK : PYSDR_ERR_ARG;
  if (!out) return PYSDR_ERR_ARG;
  for (int j = 0; j < 4; ++j) out[j] = tab[index][j];
  return PYSDR_OK;
}

int pysdr_resamp_plan(int up, int down, int ntaps, int plain, int32_t out[8]) {
  if (!out || up < 1 || down < 1 || ntaps < 1 || plain < 0 || plain > 2) return PYSDR_ERR_ARG;
  // the shape as decim_init derives it, the decision as launch_resamp_small takes it
  const int kdec = (ntaps + up - 1) / up;
  const int kpad = (kdec + 15) / 16 * 16;
  const ResampPlan p = plan_resamp_small(up, down, kpad, plain);
  out[0] = p.eligible ? 1 : 0; out[1] = p.kernel; out[2] = p.threads; out[3] = (int32_t)p.lds; out[4] = p.tile_out;
  out[5] = kpad; out[6] = decim_hist_len(kpad); out[7] = p.span;
  return PYSDR_OK;
}

int pysdr_get_resamp_tuning(pysdr_ctx* c, int32_t out[2]) {
  if (!c || !out) return PYSDR_ERR_ARG;
  out[0] = c->tune.resamp_plain; out[1] = c->tune.grid_override;
  return PYSDR_OK;
}

int pysdr_get_elapsed_ms(pysdr_ctx* c, int which, int back, float* ms) {
  if (!c || !ms || which < 0 || which > 3 || back < 0 || back >= pysdr_ctx::kSlots - (which == 3 ? 1 : 0)) return PYSDR_ERR_ARG;
  std::lock_guard<std::recursive_mutex> run_lk(c->run_mu);
  if ((unsigned long long)back + (which == 3 ? 1u : 0u) >= c->ncalls) { set_last_error("pysdr_get_elapsed_ms: no such call"); return PYSDR_ERR_STATE; }
  int rc = use_device(c->cfg.device);
  if (rc) return rc;
  // the end mark of an overlapped context's LAST call is recorded by its deferred tail: queue that first (otherwise the event
  // is unrecorded, or still holds the record of 64 calls ago: ADVICE r5)
  rc = flush_tail(c);
  if (rc) return rc;
  const Event* ev = c->ev[(c->ncalls - 1 - back) % pysdr_ctx::kSlots];
  PYSDR_HIP_CHECK(hipEventSynchronize(ev[3]));
  hipEvent_t a = ev[0], b = ev[1];
  if (which == 1) { a = ev[1]; b = ev[3]; }
  if (which == 2) { a = ev[0]; b = ev[3]; }
  if (which == 3) {              // start of the previous call -> start of this one: the period of a step
    a = c->ev[(c->ncalls - 2 - back) % pysdr_ctx::kSlots][0];
    b = ev[0];
  }
  PYSDR_HIP_CHECK(hipEventElapsedTime(ms, a, b));
  return PYSDR_OK;
}

int pysdr_sync(pysdr_ctx* c) {
  if (!c) return PYSDR_ERR_ARG;
  std::lock_guard<std::recursive_mutex> run_lk(c->run_mu);
  int rc = use_device(c->cfg.device);
  if (rc) return rc;
  rc = flush_tail(c);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (c->stream2) PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream2));
  return PYSDR_OK;
}

int pysdr_set_overlap(pysdr_ctx* c, int enable) {
  if (!c || enable < 0 || enable > 2) return PYSDR_ERR_ARG;
  std::lock_guard<std::recursive_mutex> run_lk(c->run_mu);
  int rc = use_device(c->cfg.device);
  if (rc) return rc;
  if (enable && c->n_ingest > 0) {
    set_last_error("pysdr_set_overlap: the context feeds an ingest ring, which queues its result copies behind each call on one stream");
    return PYSDR_ERR_STATE;
  }
  // a deferred tail queued, both streams drained: the switch happens between two calls, whatever is queued
  rc = flush_tail(c);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream));
  if (c->stream2) PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream2));
  if (c->tune.overlap_env >= 0 && c->n_ingest == 0) enable = c->tune.overlap_env;
  c->overlap = enable;
  return PYSDR_OK;
}

int pysdr_get_overlap(pysdr_ctx* c) { return c ? c->overlap : 0; }
int pysdr_last_call_overlapped(pysdr_ctx* c) { return (c && c->use2) ? 1 : 0; }

int pysdr_wfm_params(double srate, double fs_out, int* d1, int* up2, int* down2) {
  if (srate <= 0 || fs_out <= 0) return PYSDR_ERR_ARG;
  const int d = wfm_if_decim(srate);
  const long long a = (long long)std::llround(fs_out), b = (long long)std::llround(srate / d);
  const long long g = std::__gcd(a, b);
  if (d1) *d1 = d;
  if (up2) *up2 = (int)(a / g);
  if (down2) *down2 = (int)(b / g);
  return PYSDR_OK;
}

int pysdr_set_wfm_taps(pysdr_ctx* c, int irx, const double* video, int nv, const double* resamp, int nr) {
  if (!c || !video || !resamp || irx < 0 || irx >= c->nrx) return PYSDR_ERR_ARG;
  int d1 = 0, up2 = 0, down2 = 0;
  pysdr_wfm_params(c->cfg.srate, std::floor(c->cfg.srate * c->cfg.up / c->cfg.down), &d1, &up2, &down2);
  if (nv != c->cfg.ntaps_dec || nr < up2 || nr % up2) {
    set_last_error("pysdr_set_wfm_taps: need %d video taps and a multiple of %d resampler taps (got %d, %d)",
                   c->cfg.ntaps_dec, up2, nv, nr);
    return PYSDR_ERR_ARG;
  }
  std::lock_guard<std::mutex> lk(c->mu);
  RxHost& x = c->rx[irx];
  if (!x.wfm_resamp.empty() && (int)x.wfm_resamp.size() != nr) {
    set_last_error("pysdr_set_wfm_taps: resampler length cannot change (%zu -> %d)", x.wfm_resamp.size(), nr);
    return PYSDR_ERR_ARG;
  }
  x.wfm_video.assign(video, video + nv);
  x.wfm_resamp.assign(resamp, resamp + nr);
  x.wfm_dirty = true;
  return PYSDR_OK;
}

namespace {

// A call's input on the device: a device pointer as it is, host samples through the staging buffer (grown on demand)
int stage_input(pysdr_ctx* c, const void* iq, size_t n, int on_device, const float2** d_x) {
  *d_x = reinterpret_cast<const float2*>(iq);
  if (on_device) return PYSDR_OK;
  PYSDR_HIP_CHECK(c->d_stage.grow(n));
  PYSDR_HIP_CHECK(hipMemcpyAsync(c->d_stage.get(), iq, n * sizeof(float2), hipMemcpyHostToDevice, c->stream));
  *d_x = c->d_stage.get();
  return PYSDR_OK;
}

// The raw-peak buffer of this call: the other one of the pair
int flip_peak(pysdr_ctx* c, unsigned** peak) {
  c->peak_cur ^= 1;                       // zeroed by the previous call's history roll (both are zero at the start)
  *peak = c->d_peak2.buf(c->peak_cur);
  if (!c->peak_clean[c->peak_cur])        // ... unless that call failed on the way: then by hand
    PYSDR_HIP_CHECK(hipMemsetAsync(*peak, 0, (size_t)c->cfg.max_chunks * sizeof(unsigned), c->stream));
  c->peak_clean[c->peak_cur] = false;
  return PYSDR_OK;
}

// What the pieces of one call share
struct Call {
  const float2* d_x = nullptr;
  unsigned* peak = nullptr;
  uint32_t ph[PYSDR_MAX_RX], fw[PYSDR_MAX_RX];
  bool any_loop = false;                  // this call has segment walks (P)
  WfmArgs w;                              // broadcast FM only
};

// F of the narrow-band modes: mix + decimate to FS_OUT, the carrier loop's plan, and arg y where it belongs to F
int front_narrow(pysdr_ctx* c, Call& k, TailJob& job) {
  const CallSnap& snap = job.snap;
  const int nrx = snap.nrx;
  float2* yptr[PYSDR_MAX_RX];
  DecimResult res;
  for (int r = 0; r < nrx; ++r) yptr[r] = snap.rx[r].d_y + c->hy;
  int rc = decim_run(c, c->main, k.d_x, job.n, nrx, yptr, k.ph, k.fw, k.peak, job.chunk_len, c->mmax, &res, c->stream);
  if (rc) return rc;
  c->wfm_front.s_abs = c->main.s_abs;       // both pipelines count the same input stream
  fill_stage2(c, snap, false, job.nchunks, job.chunk_len, res, &job.s);
  Stage2Args& s = job.s;
  for (int r = 0; r < nrx; ++r) k.any_loop |= (s.det[r] == kDetPll);
  k.any_loop = k.any_loop && s.n_out > 0;
  if (!k.any_loop) return PYSDR_OK;
  s.pll = plan_am_pll(c->tune, s.n_out, std::floor(c->cfg.srate * c->cfg.up / c->cfg.down), c->pll_kmax, c->d_pllseg.get());
  // arg y of every sample: parallel, no LDS.  Single-stream form: part of F.  Overlapped form: in front of the walks on
  // their stream -- 17 us that the front stream does not wait for (profiles/r05_am_phase_stream.txt)
  if (!(snap.use2 && c->tune.am_phase_on_2)) { rc = launch_am_phase(s, c->stream); if (rc) return rc; }
  return PYSDR_OK;
}

// F of broadcast FM
int front_wfm(pysdr_ctx* c, Call& k, TailJob& job) {
  // SRATE -> fs1 (video filter, all RX in one launch) and the discriminator at fs1 are F; the pilot loop is P; each
  // RX's own fs1 -> FS_OUT resampler opens T
  const CallSnap& snap = job.snap;
  const int nrx = snap.nrx;
  float2* yptr[PYSDR_MAX_RX];
  for (int r = 0; r < nrx; ++r) yptr[r] = snap.rx[r].d_y1 + 2;
  DecimResult r1;
  int rc = decim_run(c, c->wfm_front, k.d_x, job.n, nrx, yptr, k.ph, k.fw, k.peak, job.chunk_len, c->m1max, &r1, c->stream);
  if (rc) return rc;
  c->main.s_abs = c->wfm_front.s_abs;
  job.n1 = r1.n_out;
  const double fs1 = c->cfg.srate / c->d1;
  WfmArgs& w = k.w;
  w = wfm_args(nrx, job.n1, fs1);
  for (int r = 0; r < nrx; ++r) {
    w.y1[r] = snap.rx[r].d_y1 + 2;
    w.y1base[r] = snap.rx[r].d_y1;
    w.y1dst[r] = snap.rx[r].d_y1_next;
    w.w[r] = snap.rx[r].d_w;
    w.stereo[r] = (snap.rx[r].mode == PYSDR_WFM2) ? 1 : 0;
    w.seed[r] = snap.rx[r].d_seed;
    w.mnT[r] = (snap.rx[r].mode == PYSDR_WFM2) ? snap.rx[r].d_mnt : nullptr;
  }
  w.state = c->d_state.get();
  w.pll = plan_wfm_pll(c->tune, job.n1, fs1, c->pll_kmax, c->d_pllseg.get());
  rc = launch_wfm_disc(w, c->stream);
  if (rc) return rc;
  k.any_loop = wfm_any_stereo(w);
  return PYSDR_OK;
}

// The front marker and P: the segment walks of the call's serial loop, on stream2 when the call's tail is deferred
int mark_and_walk(pysdr_ctx* c, Call& k, TailJob& job, const Event* ev) {
  const bool wfm = job.wfm, use2 = job.snap.use2;
  hipStream_t SP = use2 ? c->stream2.get() : c->stream.get();
  int rc;
  // "the input of this call has been consumed": a spectrum that orders itself behind the front end waits for it
  // (pysdr_spectrum_order, direction 2), and so do the loop walks of an overlapped call.  An event record costs ~5.5 us
  // of the stream's timeline on this runtime (the kernel behind it starts that much later: scripts/diag/timeline.sh), so
  // ONE event serves the profile and both orderings, and none is recorded when nobody asked for any.
  // (broadcast FM, single-stream form: the profile's mark sits behind the pilot loop as it always has -- "front" there
  //  is the whole FM front end)
  const bool loop_on_2 = use2 && k.any_loop;
  c->front_marker = nullptr;
  // WHERE the previous call's tail goes: behind the start of this call's walks (P(k) beside T(k-1) and F(k+1)) or in FRONT
  // of the mark they wait for (P(k) starts behind T(k-1) and shares the machine with F(k+1) only).  Measured, one box,
  // GS/s (profiles/r05_overlap_order_ab.txt): broadcast FM single-stream 377, behind 372-382, in front 432-433 -- the AF FIR
  // and the audio resampler ran 3.5-5x longer beside the pilot loop's waves (58 -> 320 us, 36 -> 125: the two share the vector
  // pipe, the walks' DPP scans and v_cos hold it), which put the tail on the critical path; AM-Synch single-stream 370,
  // behind 426, in front 415-416 (its tail is 85 us against walks of 100).  So: in front for broadcast FM, behind otherwise.
  if (loop_on_2 && (c->tune.tail_first >= 0 ? c->tune.tail_first != 0 : wfm)) { rc = flush_tail(c); if (rc) return rc; }
  if (wfm && !loop_on_2 && k.any_loop) { rc = launch_wfm_pll(k.w, c->stream); if (rc) return rc; }
  if (c->profile) { PYSDR_HIP_CHECK(hipEventRecord(ev[1], c->stream)); c->front_marker = ev[1]; }
  else if (c->front_wanted || loop_on_2) { PYSDR_HIP_CHECK(hipEventRecord(c->ev_front, c->stream)); c->front_marker = c->ev_front; }
  if (loop_on_2) {
    PYSDR_HIP_CHECK(hipStreamWaitEvent(SP, c->front_marker, 0));
    if (!wfm && c->tune.am_phase_on_2) { rc = launch_am_phase(job.s, SP); if (rc) return rc; }
    rc = wfm ? launch_wfm_pll(k.w, SP) : launch_pll(job.s, SP);
    if (rc) return rc;
    PYSDR_HIP_CHECK(hipEventRecord(c->ev_pll[job.par], SP));
    job.wait_pll = true;
  } else if (!wfm && k.any_loop) {
    rc = launch_pll(job.s, c->stream);
    if (rc) return rc;
  }
  return PYSDR_OK;
}

}  // namespace

int pysdr_process_batch(pysdr_ctx* c, const void* iq, int nchunks, size_t chunk_len, int on_device) {
  if (!c || !iq || nchunks < 1 || chunk_len < 1) return PYSDR_ERR_ARG;
  std::lock_guard<std::recursive_mutex> run_lk(c->run_mu);
  if (c->nrx < 1) { set_last_error("pysdr_process_batch: no receivers"); return PYSDR_ERR_STATE; }
  const size_t n = (size_t)nchunks * chunk_len;
  if (nchunks > c->cfg.max_chunks || n > c->cap_samples) {
    set_last_error("pysdr_process_batch: %d chunks x %zu samples exceeds capacity (%d chunks, %zu samples)",
                   nchunks, chunk_len, c->cfg.max_chunks, c->cap_samples);
    return PYSDR_ERR_STATE;
  }
  int rc = use_device(c->cfg.device);
  if (rc) return rc;
  Call k;
  rc = stage_input(c, iq, n, on_device, &k.d_x);
  if (rc) return rc;
  // everything below uses the snapshot taken under the lock, never c->rx[] fields a setter may
  // change (mode / fword / pointers re-read after the lock was released)
  TailJob job;
  rc = apply_pending(c, &job.snap);
  if (rc) return rc;
  const CallSnap& snap = job.snap;
  const int nrx = snap.nrx;
  // F on `stream`; P on stream2 when this call's tail is deferred (the loop walks then run beside the previous call's
  // tail and the next call's front end), else `stream`; T on `stream`, now or a call later (pysdr_ctx, run_tail)
  job.wfm = snap.nwfm > 0; job.par = c->par; job.nchunks = nchunks; job.chunk_len = chunk_len; job.n = n;
  job.s0 = job.wfm ? c->wfm_front.s_abs : c->main.s_abs;
  rc = flip_peak(c, &k.peak);
  if (rc) return rc;
  for (int r = 0; r < nrx; ++r) { k.ph[r] = snap.rx[r].phase; k.fw[r] = snap.rx[r].fword; }

  const Event* ev = c->ev[c->ncalls % pysdr_ctx::kSlots];
  if (c->profile) PYSDR_HIP_CHECK(hipEventRecord(ev[0], c->stream));
  job.ev_end = c->profile ? ev[3].get() : nullptr;
  rc = job.wfm ? front_wfm(c, k, job) : front_narrow(c, k, job);
  if (rc) return rc;
  rc = mark_and_walk(c, k, job, ev);
  if (rc) return rc;
  c->ncalls++;
  {
    // the NCO phase belongs to the process thread; the lock only orders it against pysdr_rx_add
    std::lock_guard<std::mutex> lk(c->mu);
    for (int r = 0; r < nrx; ++r) c->rx[r].phase = snap.rx[r].phase + snap.rx[r].fword * (uint32_t)n;
  }
  // T: the previous call's if it was deferred, then this call's -- now, or left for the next call / a flush
  rc = flush_tail(c);
  if (rc) return rc;
  if (snap.use2) {
    c->tail = job;
    c->tail.valid = true;
    c->par = job.par ^ 1;
    return PYSDR_OK;
  }
  return run_tail(c, job);
}

// outputs of the last call per chunk: those whose newest input sample falls into chunk k (a
// two-level cascade for WFM); host arithmetic only
static void last_chunk_counts(pysdr_ctx* c, int* chunk_nout) {
  auto first_out = [&](unsigned long long s) -> unsigned long long {
    if (!c->last_wfm) {
      const unsigned long long up = c->cfg.up, down = c->cfg.down;
      return (s * up + down - 1) / down;
    }
    const unsigned long long m1 = (s + c->d1 - 1) / (unsigned long long)c->d1;
    return (m1 * (unsigned long long)c->up2 + c->down2 - 1) / (unsigned long long)c->down2;
  };
  for (int k = 0; k < c->last_nchunks; ++k) {
    const unsigned long long a0 = c->last_s0 + (unsigned long long)k * c->last_chunk_len;
    chunk_nout[k] = (int)(first_out(a0 + c->last_chunk_len) - first_out(a0));
  }
}

int pysdr_fetch(pysdr_ctx* c, int irx, float* am, float* iq, int cap, int* n_out,
                int* am_is_complex, int* chunk_nout, float* peaks) {
  if (!c || irx < 0 || irx >= c->nrx) return PYSDR_ERR_ARG;
  std::lock_guard<std::recursive_mutex> run_lk(c->run_mu);
  int rc = use_device(c->cfg.device);
  if (rc) return rc;
  rc = flush_tail(c);                     // a deferred tail (pysdr_set_overlap) is queued now: its results are what is asked for
  if (rc) return rc;
  const int n = c->last_nout;
  if ((am || iq) && cap < n) { set_last_error("pysdr_fetch: cap %d < n_out %d", cap, n); return PYSDR_ERR_ARG; }
  const int cx = c->last_complex[irx];
  // The epilogue rolled the last hy outputs into the prefix but left [hy, hy+n) intact.
  hipStream_t S2 = c->stream;
  const float2* yb = c->rx[irx].d_y.buf(c->last_par);
  if (am && n > 0)
    PYSDR_HIP_CHECK(hipMemcpyAsync(am, c->rx[irx].d_am.get(), (size_t)n * (cx ? 2 : 1) * sizeof(float), hipMemcpyDeviceToHost, S2));
  if (iq && n > 0)
    PYSDR_HIP_CHECK(hipMemcpyAsync(iq, yb + c->hy, (size_t)n * sizeof(float2), hipMemcpyDeviceToHost, S2));
  if (peaks && c->last_nchunks > 0)
    PYSDR_HIP_CHECK(hipMemcpyAsync(peaks, c->d_peak2.buf(c->peak_cur), (size_t)c->last_nchunks * sizeof(float), hipMemcpyDeviceToHost, S2));
  PYSDR_HIP_CHECK(hipStreamSynchronize(S2));
  if (n_out) *n_out = n;
  if (am_is_complex) *am_is_complex = cx;
  if (chunk_nout) last_chunk_counts(c, chunk_nout);
  return PYSDR_OK;
}

int pysdr_process(pysdr_ctx* c, const float* iq, size_t n, pysdr_out* outs) {
  if (!c || !iq || !outs || n < 1) return PYSDR_ERR_ARG;
  std::lock_guard<std::recursive_mutex> run_lk(c->run_mu);
  int rc = pysdr_process_batch(c, iq, 1, n, 0);
  if (rc) return rc;
  rc = flush_tail(c);                     // (an overlapped context deferred the call's tail: its results are wanted now)
  if (rc) return rc;
  for (int r = 0; r < c->last_nrx; ++r) {
    int nout = 0, cx = 0;
    float pk = 0.f;
    rc = pysdr_fetch(c, r, outs[r].am, outs[r].iq, outs[r].cap, &nout, &cx, nullptr, &pk);
    if (rc) return rc;
    outs[r].n_out = nout;
    outs[r].am_is_complex = cx;
    outs[r].peak_in = pk;
  }
  return PYSDR_OK;
}

// ---------------------------------------------------------------- quad mixer
int pysdr_quad_mixer(int device, const float* x, float* y, size_t n, uint32_t phase0,
                     uint32_t fword, uint32_t* phase_out) {
  if (!x || !y) return PYSDR_ERR_ARG;
  int rc = use_device(device);
  if (rc) return rc;
  if (phase_out) *phase_out = phase0 + fword * (uint32_t)n;
  if (n == 0) return PYSDR_OK;
  DevBuf<float2> dx, dy;
  PYSDR_HIP_CHECK(dx.alloc(n));
  PYSDR_HIP_CHECK(dy.alloc(n));
  PYSDR_HIP_CHECK(hipMemcpy(dx.get(), x, n * sizeof(float2), hipMemcpyHostToDevice));
  rc = launch_quad_mixer(dx.get(), dy.get(), n, phase0, fword, nullptr);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipMemcpy(y, dy.get(), n * sizeof(float2), hipMemcpyDeviceToHost));
  return PYSDR_OK;
}

// ---------------------------------------------------------------- convolver
int pysdr_fir_real(int device, const float* xx, const float* h, int ntaps, float* y, size_t n) {
  if (!xx || !h || !y || ntaps < 1) return PYSDR_ERR_ARG;
  if (n == 0) return PYSDR_OK;
  int rc = use_device(device);
  if (rc) return rc;
  const size_t nin = n + (size_t)ntaps - 1;
  DevBuf<float> dx, dh, dy;
  PYSDR_HIP_CHECK(dx.alloc(nin));
  PYSDR_HIP_CHECK(dh.alloc((size_t)ntaps));
  PYSDR_HIP_CHECK(dy.alloc(n));
  PYSDR_HIP_CHECK(hipMemcpy(dx.get(), xx, nin * sizeof(float), hipMemcpyHostToDevice));
  PYSDR_HIP_CHECK(hipMemcpy(dh.get(), h, (size_t)ntaps * sizeof(float), hipMemcpyHostToDevice));
  rc = launch_fir_real(dx.get(), dh.get(), ntaps, dy.get(), (int)n, nullptr);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipMemcpy(y, dy.get(), n * sizeof(float), hipMemcpyDeviceToHost));
  return PYSDR_OK;
}

// ---------------------------------------------------------------- spectrum
static int get_plan(pysdr_spectrum* sp, int batch, rocfft_plan* out) {
  auto it = sp->plans.find(batch);
  if (it != sp->plans.end()) { *out = it->second; return PYSDR_OK; }
  rocfft_plan plan = nullptr;
  size_t len[1] = {(size_t)sp->nfft};
  rocfft_status s = rocfft_plan_create(&plan, rocfft_placement_inplace, rocfft_transform_type_complex_forward,
                                       rocfft_precision_single, 1, len, (size_t)batch, nullptr);
  if (s != rocfft_status_success) { set_last_error("rocfft_plan_create(nfft=%d,batch=%d) = %d", sp->nfft, batch, (int)s); return PYSDR_ERR_FFT; }
  size_t wbs = 0;
  rocfft_plan_get_work_buffer_size(plan, &wbs);
  const hipError_t e = sp->d_fftwork.grow(wbs);
  if (e != hipSuccess) {
    rocfft_plan_destroy(plan);            // (not in the map yet: nobody else would)
    set_last_error("rocFFT work buffer of %zu bytes: %s", wbs, hipGetErrorString(e));
    return PYSDR_ERR_HIP;
  }
  if (sp->d_fftwork) rocfft_execution_info_set_work_buffer(sp->info, sp->d_fftwork.get(), sp->d_fftwork.size());
  sp->plans[batch] = plan;
  *out = plan;
  return PYSDR_OK;
}

static int spectrum_alloc(pysdr_spectrum* sp, const float* window) {
  PYSDR_HIP_CHECK(sp->stream.create(hipStreamNonBlocking));
  PYSDR_HIP_CHECK(sp->d_win.alloc((size_t)sp->chunk));
  PYSDR_HIP_CHECK(hipMemcpy(sp->d_win.get(), window, (size_t)sp->chunk * sizeof(float), hipMemcpyHostToDevice));
  PYSDR_HIP_CHECK(sp->d_in.alloc((size_t)sp->chunk));
  PYSDR_HIP_CHECK(sp->d_out.alloc((size_t)sp->nfft));
  PYSDR_HIP_CHECK(sp->ev[0].create());
  PYSDR_HIP_CHECK(sp->ev[1].create());
  return PYSDR_OK;
}

int pysdr_spectrum_create(int device, int chunk_size, int nfft, int max_frames, const float* window,
                          pysdr_spectrum** out) {
  if (!out || !window || chunk_size < 1 || nfft < chunk_size || max_frames < 1) return PYSDR_ERR_ARG;
  int rc = use_device(device);
  if (rc) return rc;
  {
    std::lock_guard<std::mutex> lk(g_rocfft_mu);
    if (g_rocfft_users++ == 0) rocfft_setup();
  }
  pysdr_spectrum* sp = new pysdr_spectrum();
  sp->device = device; sp->chunk = chunk_size; sp->nfft = nfft; sp->max_frames = max_frames;
  sp->tune = SpectrumTuning::from_env();
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) sp->num_cus = prop.multiProcessorCount;
  }
  rc = spectrum_alloc(sp, window);
  if (rc) { failed_in("pysdr_spectrum_create", rc); pysdr_spectrum_destroy(sp); return rc; }
  if (rocfft_execution_info_create(&sp->info) != rocfft_status_success ||
      rocfft_execution_info_set_stream(sp->info, sp->stream.get()) != rocfft_status_success) {
    set_last_error("rocfft_execution_info_create failed");
    pysdr_spectrum_destroy(sp);
    return PYSDR_ERR_FFT;
  }
  *out = sp;
  return PYSDR_OK;
}

void pysdr_spectrum_destroy(pysdr_spectrum* sp) {
  if (!sp) return;
  (void)hipSetDevice(sp->device);
  if (sp->stream) (void)hipStreamSynchronize(sp->stream);
  for (int i = 1; i < pysdr_spectrum::kMaxStreams; ++i) if (sp->xstream[i]) (void)hipStreamSynchronize(sp->xstream[i]);
  for (auto& kv : sp->plans) rocfft_plan_destroy(kv.second);
  if (sp->info) rocfft_execution_info_destroy(sp->info);
  delete sp;                              // (the owners free: host_res.h)
  std::lock_guard<std::mutex> lk(g_rocfft_mu);
  if (--g_rocfft_users == 0) rocfft_cleanup();
}

// the transform's work area: `frames` frames of nfft complex (the 64k path only ever needs one
// group of frames, the rocFFT path the whole batch)
static int ensure_work(pysdr_spectrum* sp, size_t frames) {
  const size_t n = frames * (size_t)sp->nfft;
  if (sp->d_work.size() >= n) return PYSDR_OK;
  PYSDR_HIP_CHECK(hipStreamSynchronize(sp->stream));
  PYSDR_HIP_CHECK(sp->d_work.grow(n));
  return PYSDR_OK;
}

static int spectrum_run(pysdr_spectrum* sp, const float2* d_x, size_t hop, int nframes, int is_complex,
                        int db, float* d_out) {
  int rc;
  if (is_complex && sp->chunk == 32768 && sp->nfft == 65536 && !sp->tune.force_rocfft) {
    // the RF-waterfall size: fused four-step transform, in groups of 448 frames: the 224 MB
    // of intermediate of one group then stays in the 256 MB Infinity Cache between the two
    // kernels (the input and the PSD stream past it with non-temporal accesses).  Measured per
    // 10666 frames: 3.45 ms for groups of 4096, 3.02 ms at 320 and 2.96 ms at 448-512 with the
    // streaming hints, 3.6 ms at 576 (no longer fits); below 128 frames launch gaps dominate.
    // Running the rows of group g beside the columns of group g+1 on a second stream with two FULL groups
    // of intermediate is slower (3.9 ms, round 1: the two working sets evict each other); with HALF a group per
    // stream it is 5 % faster (round 3, below).
    // (round 4: the 24-bit intermediate is 384 KB per frame and the mix + decimate kernel beside it now copies
    //  nontemporal: 320 / 384 / 448 / 512 / 576 / 640 frames = C3 step 3.04 / 2.97 / 2.96-2.97 / 2.93 / 2.94 / 3.26 ms,
    //  scripts/diag/psd_group_sweep.sh; on a second box 448 / 512 / 576 = 2.99-3.01 / 2.95-2.99 / 3.05: the cliff moves from box
    //  to box, so the default sits between the old 448 and the best 512)
    // The columns pass of a launch is a loop over its frames on 16 x G resident workgroups (psd_form / plan_psd_cols in
    // host_plan.h from the CU count read at create: 240 frames on 256 CUs = 60 rows of 4 frames each; a single frame = 16
    // workgroups of one iteration); PYSDR_PSD_PATH=unit / loop:<G> for A/B.  Same bits either way.  Measured (LABNOTES 15):
    // the columns kernel alone 134.3 -> 129.5 ns per frame, the C3 step 2.945 -> 2.893 ms (medians of 15 + 15 runs: 1.8 %).
    // The rows pass is the same kind of loop on 8 x R resident workgroups (psd_rows_form / plan_psd_rows; LABNOTES 25);
    // PYSDR_PSD_PATH=rows=unit / rows=loop:<R> for A/B, `unit` alone for the unit form of both passes.  Same bits either way.
    const int group = sp->tune.frames_per_group();
    if (sp->tune.nstreams > 1 && nframes > group) {
      // The groups are dealt out over `nstreams` streams, each with its own intermediate of group / nstreams
      // frames (together the same Infinity Cache footprint as one group): the columns of one sub-group run
      // beside the rows of another, and the kernel boundaries of one stream hide behind the other's kernels.
      // Measured on C3 (PSD ms per 10666 frames): 1 stream 2.77-2.78, 2 streams x 224 frames 2.63-2.67.
      // (Round 1 tried two streams with FULL 448-frame groups each: 448 MB of intermediate, slower.)
      const int ns = sp->tune.nstreams;
      const int part = (group + ns - 1) / ns;
      rc = ensure_work(sp, (size_t)part);
      if (rc) return rc;
      if (sp->xwork_frames < (size_t)part) {
        for (int i = 1; i < ns; ++i) {
          if (!sp->xstream[i]) PYSDR_HIP_CHECK(sp->xstream[i].create(hipStreamNonBlocking));
          if (!sp->ev_join[i]) PYSDR_HIP_CHECK(sp->ev_join[i].create(hipEventDisableTiming));
          PYSDR_HIP_CHECK(hipStreamSynchronize(sp->xstream[i]));
          PYSDR_HIP_CHECK(sp->xwork[i].alloc((size_t)part * sp->nfft));
        }
        sp->xwork_frames = (size_t)part;
      }
      PYSDR_HIP_CHECK(hipEventRecord(sp->ev[0], sp->stream));
      // the side streams start behind whatever sp->stream waited for: they wait for the call's start event itself (a
      // second event for the fork was 5.5 us more on the stream)
      for (int i = 1; i < ns; ++i) PYSDR_HIP_CHECK(hipStreamWaitEvent(sp->xstream[i], sp->ev[0], 0));
      int k = 0;
      for (int f0 = 0; f0 < nframes; f0 += part, ++k) {
        const int nf = (nframes - f0 < part) ? nframes - f0 : part;
        const int w = k % ns;
        rc = launch_psd64k(d_x + (size_t)f0 * hop, hop, nf, sp->d_win.get(), w ? sp->xwork[w].get() : sp->d_work.get(),
                           d_out + (size_t)f0 * sp->nfft, db, w ? sp->xstream[w].get() : sp->stream.get(),
                           psd_launch_form(sp->tune, nf, sp->num_cus));
        if (rc) break;             // a failed launch still joins the side streams below: what was forked keeps writing
      }                            // d_out / xwork until it is done, and the caller reacts to the error right away
      for (int i = 1; i < ns; ++i) {
        PYSDR_HIP_CHECK(hipEventRecord(sp->ev_join[i], sp->xstream[i]));
        PYSDR_HIP_CHECK(hipStreamWaitEvent(sp->stream, sp->ev_join[i], 0));
      }
      PYSDR_HIP_CHECK(hipEventRecord(sp->ev[1], sp->stream));
      return rc;
    }
    rc = ensure_work(sp, (size_t)std::min(group, nframes));
    if (rc) return rc;
    PYSDR_HIP_CHECK(hipEventRecord(sp->ev[0], sp->stream));
    for (int f0 = 0; f0 < nframes; f0 += group) {
      const int nf = (nframes - f0 < group) ? nframes - f0 : group;
      rc = launch_psd64k(d_x + (size_t)f0 * hop, hop, nf, sp->d_win.get(), sp->d_work.get(),
                         d_out + (size_t)f0 * sp->nfft, db, sp->stream, psd_launch_form(sp->tune, nf, sp->num_cus));
      if (rc) return rc;
    }
    PYSDR_HIP_CHECK(hipEventRecord(sp->ev[1], sp->stream));
    return PYSDR_OK;
  }
  rocfft_plan plan;
  rc = get_plan(sp, nframes, &plan);
  if (rc) return rc;
  rc = ensure_work(sp, (size_t)nframes);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipEventRecord(sp->ev[0], sp->stream));
  rc = launch_psd_pre(d_x, hop, nframes, sp->chunk, sp->nfft, sp->d_win.get(), sp->d_work.get(), is_complex, sp->stream);
  if (rc) return rc;
  void* bufs[1] = {sp->d_work.get()};
  rocfft_status s = rocfft_execute(plan, bufs, nullptr, sp->info);
  if (s != rocfft_status_success) { set_last_error("rocfft_execute = %d", (int)s); return PYSDR_ERR_FFT; }
  rc = launch_psd_post(sp->d_work.get(), nframes, sp->nfft, is_complex ? 0 : 1, db, d_out, sp->stream);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipEventRecord(sp->ev[1], sp->stream));
  return PYSDR_OK;
}

int pysdr_spectrum_frame(pysdr_spectrum* sp, const float* x, int is_complex, int db, float* psd_out,
                         int* n_out) {
  if (!sp || !x || !psd_out) return PYSDR_ERR_ARG;
  int rc = use_device(sp->device);
  if (rc) return rc;
  const size_t bytes = (size_t)sp->chunk * (is_complex ? sizeof(float2) : sizeof(float));
  PYSDR_HIP_CHECK(hipMemcpyAsync(sp->d_in.get(), x, bytes, hipMemcpyHostToDevice, sp->stream));
  rc = spectrum_run(sp, sp->d_in.get(), 0, 1, is_complex, db, sp->d_out.get());
  if (!rc) sp->ran = true;
  if (rc) return rc;
  const int nout = is_complex ? sp->nfft : sp->nfft / 2;
  PYSDR_HIP_CHECK(hipMemcpyAsync(psd_out, sp->d_out.get(), (size_t)nout * sizeof(float), hipMemcpyDeviceToHost, sp->stream));
  PYSDR_HIP_CHECK(hipStreamSynchronize(sp->stream));
  if (n_out) *n_out = nout;
  return PYSDR_OK;
}

int pysdr_spectrum_batch(pysdr_spectrum* sp, const void* d_iq, int nframes, size_t hop, void* d_out) {
  if (!sp || !d_iq || !d_out || nframes < 1 || nframes > sp->max_frames) return PYSDR_ERR_ARG;
  int rc = use_device(sp->device);
  if (rc) return rc;
  rc = spectrum_run(sp, reinterpret_cast<const float2*>(d_iq), hop, nframes, 1, 1, reinterpret_cast<float*>(d_out));
  if (!rc) sp->ran = true;
  return rc;
}

int pysdr_spectrum_get_tuning(pysdr_spectrum* sp, int32_t out[4]) {
  if (!sp || !out) return PYSDR_ERR_ARG;
  out[0] = sp->tune.frames_per_group(); out[1] = sp->tune.force_rocfft ? 1 : 0; out[2] = sp->tune.nstreams; out[3] = sp->tune.packed;
  return PYSDR_OK;
}

int pysdr_spectrum_sync(pysdr_spectrum* sp) {
  if (!sp) return PYSDR_ERR_ARG;
  int rc = use_device(sp->device);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipStreamSynchronize(sp->stream));
  return PYSDR_OK;
}

int pysdr_spectrum_elapsed_ms(pysdr_spectrum* sp, float* ms) {
  if (!sp || !ms) return PYSDR_ERR_ARG;
  int rc = use_device(sp->device);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipEventSynchronize(sp->ev[1]));
  PYSDR_HIP_CHECK(hipEventElapsedTime(ms, sp->ev[0], sp->ev[1]));
  return PYSDR_OK;
}

int pysdr_spectrum_order(pysdr_spectrum* sp, pysdr_ctx* c, int direction) {
  if (!sp || !c || direction < 0 || direction > 2 || sp->device != c->cfg.device) return PYSDR_ERR_ARG;
  std::lock_guard<std::recursive_mutex> run_lk(c->run_mu);
  int rc = use_device(sp->device);
  if (rc) return rc;
  if (direction == 2) {
    c->front_wanted = 1;                  // from the next call on the front end's end is marked
    if (c->front_marker) {
      PYSDR_HIP_CHECK(hipStreamWaitEvent(sp->stream, c->front_marker, 0));
      return PYSDR_OK;
    }
    direction = 0;                        // this call was not marked: behind everything the context has queued (stricter)
  }
  if (direction == 1 && sp->ran) {        // the context behind the spectrum's last call: its end event is already there
    PYSDR_HIP_CHECK(hipStreamWaitEvent(c->stream, sp->ev[1], 0));
    return PYSDR_OK;
  }
  if (!sp->ev_order) PYSDR_HIP_CHECK(sp->ev_order.create(hipEventDisableTiming));
  if (direction == 0) { rc = flush_tail(c); if (rc) return rc; }   // "behind the whole demodulation" includes a deferred tail
  hipStream_t first = direction == 0 ? c->stream : sp->stream;
  hipStream_t then = direction == 0 ? sp->stream : c->stream;
  PYSDR_HIP_CHECK(hipEventRecord(sp->ev_order, first));
  PYSDR_HIP_CHECK(hipStreamWaitEvent(then, sp->ev_order, 0));
  return PYSDR_OK;
}

// ---------------------------------------------------------------- device memory
int pysdr_dev_alloc(int device, size_t bytes, void** out) {
  if (!out || bytes == 0) return PYSDR_ERR_ARG;
  int rc = use_device(device);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipMalloc(out, bytes));
  return PYSDR_OK;
}
int pysdr_dev_free(int device, void* p) {
  if (!p) return PYSDR_OK;
  int rc = use_device(device);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipFree(p));
  return PYSDR_OK;
}
int pysdr_dev_upload(int device, void* dst, const void* src_host, size_t bytes) {
  if (!dst || !src_host) return PYSDR_ERR_ARG;
  int rc = use_device(device);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipMemcpy(dst, src_host, bytes, hipMemcpyHostToDevice));
  return PYSDR_OK;
}
int pysdr_dev_download(int device, void* dst_host, const void* src, size_t bytes) {
  if (!dst_host || !src) return PYSDR_ERR_ARG;
  int rc = use_device(device);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipMemcpy(dst_host, src, bytes, hipMemcpyDeviceToHost));
  return PYSDR_OK;
}
int pysdr_dev_copy(int device, void* dst, const void* src, size_t bytes) {
  if (!dst || !src) return PYSDR_ERR_ARG;
  int rc = use_device(device);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice));
  return PYSDR_OK;
}

// ---------------------------------------------------------------- ingest ring (N4)
void pysdr_ingest_destroy(pysdr_ingest* g) {
  if (!g) return;
  if (g->c) (void)hipSetDevice(g->c->cfg.device);
  if (g->copy_stream) (void)hipStreamSynchronize(g->copy_stream);
  if (g->c && g->c->stream) (void)hipStreamSynchronize(g->c->stream);
  if (g->c && g->counted) { g->c->n_ingest--; g->counted = false; }
  delete g;                               // (the owners free: host_res.h)
}

static int ingest_alloc(pysdr_ingest* g) {
  const int nslots = g->nslots;
  PYSDR_HIP_CHECK(g->copy_stream.create(hipStreamNonBlocking));
  g->h_in.resize(nslots);
  g->ev_copied.resize(nslots);
  g->ev_done.resize(nslots);
  g->h_am.resize((size_t)nslots * PYSDR_MAX_RX);
  g->h_iq.resize((size_t)nslots * PYSDR_MAX_RX);
  g->h_peak.resize(nslots);
  g->n_out.assign(nslots, 0);
  g->in_flight.assign(nslots, 0);
  g->n_chunks.assign(nslots, 0);
  g->nrx.assign(nslots, 0);
  g->chunk_nout.assign(nslots, std::vector<int>());
  g->cx.assign((size_t)nslots * PYSDR_MAX_RX, 0);
  for (int s = 0; s < nslots; ++s) {
    PYSDR_HIP_CHECK(g->h_in[s].alloc(g->cap));
    PYSDR_HIP_CHECK(g->h_peak[s].alloc((size_t)g->chunks_per_slot));
    PYSDR_HIP_CHECK(g->ev_copied[s].create(hipEventDisableTiming));
    PYSDR_HIP_CHECK(g->ev_done[s].create(hipEventDisableTiming));
    for (int r = 0; r < PYSDR_MAX_RX; ++r) {
      PYSDR_HIP_CHECK(g->h_am[(size_t)s * PYSDR_MAX_RX + r].alloc((size_t)g->ocap));
      PYSDR_HIP_CHECK(g->h_iq[(size_t)s * PYSDR_MAX_RX + r].alloc((size_t)g->ocap));
    }
  }
  for (int i = 0; i < 2; ++i) {
    PYSDR_HIP_CHECK(g->d_in[i].alloc(g->cap));
    PYSDR_HIP_CHECK(g->ev_free[i].create(hipEventDisableTiming));
  }
  return PYSDR_OK;
}

int pysdr_ingest_create(pysdr_ctx* c, int nslots, pysdr_ingest** out) {
  return pysdr_ingest_create_batched(c, nslots, 1, out);
}

int pysdr_ingest_create_batched(pysdr_ctx* c, int nslots, int chunks_per_slot, pysdr_ingest** out) {
  if (!c || !out || nslots < 2 || nslots > 64 || chunks_per_slot < 1) return PYSDR_ERR_ARG;
  if (chunks_per_slot > c->cfg.max_chunks) {
    set_last_error("pysdr_ingest_create_batched: %d chunks per slot > the context's max_chunks %d", chunks_per_slot,
                   c->cfg.max_chunks);
    return PYSDR_ERR_ARG;
  }
  int rc = use_device(c->cfg.device);
  if (rc) return rc;
  // A ring queues the result copies of a slot behind its call and the next slot's call behind those, all on ONE stream:
  // the context runs single-stream from here on (the ring's rate is the PCIe link's, two orders below the kernels')
  c->n_ingest++;
  if (c->overlap) { rc = pysdr_set_overlap(c, 0); if (rc) { c->n_ingest--; return rc; } }
  pysdr_ingest* g = new pysdr_ingest();
  g->c = c; g->nslots = nslots; g->chunks_per_slot = chunks_per_slot;
  g->counted = true;
  g->cap = (size_t)c->cfg.in_chunk * (size_t)chunks_per_slot;
  g->ocap = (int)((g->cap * (size_t)c->cfg.up) / (size_t)c->cfg.down) + 8;
  rc = ingest_alloc(g);
  if (rc) { failed_in("pysdr_ingest_create", rc); pysdr_ingest_destroy(g); return rc; }
  *out = g;
  return PYSDR_OK;
}

int pysdr_ingest_buffer(pysdr_ingest* g, int slot, float** iq, size_t* cap_samples) {
  if (!g || !iq || slot < 0 || slot >= g->nslots) return PYSDR_ERR_ARG;
  if (g->in_flight[slot]) { set_last_error("pysdr_ingest_buffer: slot %d is in flight (collect it first)", slot); return PYSDR_ERR_STATE; }
  *iq = reinterpret_cast<float*>(g->h_in[slot].get());
  if (cap_samples) *cap_samples = g->cap;
  return PYSDR_OK;
}

int pysdr_ingest_submit(pysdr_ingest* g, int slot, size_t n) {
  if (!g || slot < 0 || slot >= g->nslots || n < 1 || n > g->cap) return PYSDR_ERR_ARG;
  if (g->in_flight[slot]) { set_last_error("pysdr_ingest_submit: slot %d is already in flight", slot); return PYSDR_ERR_STATE; }
  pysdr_ctx* c = g->c;
  std::lock_guard<std::recursive_mutex> run_lk(c->run_mu);
  int rc = use_device(c->cfg.device);
  if (rc) return rc;
  const int b = (int)(g->seq & 1ull);
  // the copy may not overwrite a staging buffer the kernels of two chunks ago still read
  if (g->used[b]) PYSDR_HIP_CHECK(hipStreamWaitEvent(g->copy_stream, g->ev_free[b], 0));
  PYSDR_HIP_CHECK(hipMemcpyAsync(g->d_in[b].get(), g->h_in[slot].get(), n * sizeof(float2), hipMemcpyHostToDevice, g->copy_stream));
  PYSDR_HIP_CHECK(hipEventRecord(g->ev_copied[slot], g->copy_stream));
  PYSDR_HIP_CHECK(hipStreamWaitEvent(c->stream, g->ev_copied[slot], 0));
  // a slot of whole chunks is ONE launch sequence over all of them (same arithmetic as chunk by
  // chunk: pysdr_process_batch); anything else is a single (possibly short) chunk
  const size_t lc = (size_t)c->cfg.in_chunk;
  const int nch = (n > lc && n % lc == 0) ? (int)(n / lc) : 1;
  rc = pysdr_process_batch(c, g->d_in[b].get(), nch, nch > 1 ? lc : n, 1);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipEventRecord(g->ev_free[b], c->stream));
  g->used[b] = true;
  const int nout = c->last_nout;
  if (nout > g->ocap) { set_last_error("pysdr_ingest_submit: %d outputs > capacity %d", nout, g->ocap); return PYSDR_ERR_STATE; }
  g->n_out[slot] = nout;
  g->nrx[slot] = c->last_nrx;
  for (int r = 0; r < c->last_nrx; ++r) {
    const int cx = c->last_complex[r];
    g->cx[(size_t)slot * PYSDR_MAX_RX + r] = cx;
    if (nout > 0) {
      PYSDR_HIP_CHECK(hipMemcpyAsync(g->h_am[(size_t)slot * PYSDR_MAX_RX + r].get(), c->rx[r].d_am.get(),
                                     (size_t)nout * (cx ? 2 : 1) * sizeof(float), hipMemcpyDeviceToHost, c->stream));
      PYSDR_HIP_CHECK(hipMemcpyAsync(g->h_iq[(size_t)slot * PYSDR_MAX_RX + r].get(), c->rx[r].d_y.buf(c->last_par) + c->hy,
                                     (size_t)nout * sizeof(float2), hipMemcpyDeviceToHost, c->stream));
    }
  }
  PYSDR_HIP_CHECK(hipMemcpyAsync(g->h_peak[slot].get(), c->d_peak2.buf(c->peak_cur), (size_t)nch * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  PYSDR_HIP_CHECK(hipEventRecord(g->ev_done[slot], c->stream));
  g->n_chunks[slot] = nch;
  g->chunk_nout[slot].assign(nch, 0);
  last_chunk_counts(c, g->chunk_nout[slot].data());
  g->in_flight[slot] = 1;
  g->seq += 1;
  return PYSDR_OK;
}

int pysdr_ingest_chunks(pysdr_ingest* g, int slot, int cap, int* nchunks, int* chunk_nout, float* peaks) {
  if (!g || slot < 0 || slot >= g->nslots || !nchunks) return PYSDR_ERR_ARG;
  if (!g->in_flight[slot]) { set_last_error("pysdr_ingest_chunks: slot %d was not submitted", slot); return PYSDR_ERR_STATE; }
  int rc = use_device(g->c->cfg.device);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipEventSynchronize(g->ev_done[slot]));
  const int n = g->n_chunks[slot];
  *nchunks = n;
  if ((chunk_nout || peaks) && cap < n) { set_last_error("pysdr_ingest_chunks: cap %d < %d chunks", cap, n); return PYSDR_ERR_ARG; }
  for (int k = 0; k < n; ++k) {
    if (chunk_nout) chunk_nout[k] = g->chunk_nout[slot][k];
    if (peaks) peaks[k] = g->h_peak[slot].get()[k];
  }
  return PYSDR_OK;
}

int pysdr_ingest_collect(pysdr_ingest* g, int slot, pysdr_out* outs) {
  if (!g || !outs || slot < 0 || slot >= g->nslots) return PYSDR_ERR_ARG;
  if (!g->in_flight[slot]) { set_last_error("pysdr_ingest_collect: slot %d was not submitted", slot); return PYSDR_ERR_STATE; }
  int rc = use_device(g->c->cfg.device);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipEventSynchronize(g->ev_done[slot]));
  for (int r = 0; r < g->nrx[slot]; ++r) {        // the RX set of THIS slot's submit, not of the latest call
    outs[r].am = reinterpret_cast<float*>(g->h_am[(size_t)slot * PYSDR_MAX_RX + r].get());
    outs[r].iq = reinterpret_cast<float*>(g->h_iq[(size_t)slot * PYSDR_MAX_RX + r].get());
    outs[r].cap = g->ocap;
    outs[r].n_out = g->n_out[slot];
    outs[r].am_is_complex = g->cx[(size_t)slot * PYSDR_MAX_RX + r];
    outs[r].peak_in = *g->h_peak[slot].get();
  }
  g->in_flight[slot] = 0;
  return PYSDR_OK;
}

// ---------------------------------------------------------------- RCCL (lazy dlopen: librccl is ~0.5 GB)
namespace {
struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
RcclApi g_rccl;
std::mutex g_rccl_mu;

int rccl_load() {
  std::lock_guard<std::mutex> lk(g_rccl_mu);
  if (g_rccl.lib) return PYSDR_OK;
  void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
  if (!lib) { set_last_error("dlopen(librccl.so.1): %s", dlerror()); return PYSDR_ERR_RCCL; }
  g_rccl.GetUniqueId = reinterpret_cast<decltype(g_rccl.GetUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
  g_rccl.CommInitRank = reinterpret_cast<decltype(g_rccl.CommInitRank)>(dlsym(lib, "ncclCommInitRank"));
  g_rccl.Broadcast = reinterpret_cast<decltype(g_rccl.Broadcast)>(dlsym(lib, "ncclBroadcast"));
  g_rccl.CommDestroy = reinterpret_cast<decltype(g_rccl.CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
  g_rccl.GetErrorString = reinterpret_cast<decltype(g_rccl.GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
  if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.Broadcast || !g_rccl.CommDestroy) {
    set_last_error("librccl: missing symbols");
    dlclose(lib);
    return PYSDR_ERR_RCCL;
  }
  g_rccl.lib = lib;
  return PYSDR_OK;
}
int rccl_fail(const char* what, ncclResult_t r) {
  set_last_error("%s: %s", what, g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "rccl error");
  return PYSDR_ERR_RCCL;
}
}  // namespace

int pysdr_comm_unique_id(char id_out[128]) {
  if (!id_out) return PYSDR_ERR_ARG;
  int rc = rccl_load();
  if (rc) return rc;
  ncclUniqueId id;
  ncclResult_t r = g_rccl.GetUniqueId(&id);
  if (r != ncclSuccess) return rccl_fail("ncclGetUniqueId", r);
  memcpy(id_out, id.internal, 128);
  return PYSDR_OK;
}

int pysdr_comm_init(pysdr_ctx* c, const char id[128], int rank, int nranks) {
  if (!c || !id || rank < 0 || rank >= nranks) return PYSDR_ERR_ARG;
  int rc = rccl_load();
  if (rc) return rc;
  rc = use_device(c->cfg.device);
  if (rc) return rc;
  if (c->comm) { set_last_error("pysdr_comm_init: already initialised"); return PYSDR_ERR_STATE; }
  ncclUniqueId uid;
  memcpy(uid.internal, id, 128);
  ncclResult_t r = g_rccl.CommInitRank(&c->comm, nranks, uid, rank);
  if (r != ncclSuccess) { c->comm = nullptr; return rccl_fail("ncclCommInitRank", r); }
  return PYSDR_OK;
}

int pysdr_comm_bcast(pysdr_ctx* c, void* d_buf, size_t bytes, int root) {
  if (!c || !d_buf) return PYSDR_ERR_ARG;
  if (!c->comm) { set_last_error("pysdr_comm_bcast: communicator not initialised"); return PYSDR_ERR_STATE; }
  std::lock_guard<std::recursive_mutex> run_lk(c->run_mu);
  int rc = use_device(c->cfg.device);
  if (rc) return rc;
  ncclResult_t r = g_rccl.Broadcast(d_buf, d_buf, bytes, ncclUint8, root, c->comm, c->stream);
  if (r != ncclSuccess) return rccl_fail("ncclBroadcast", r);
  return PYSDR_OK;
}

int pysdr_comm_destroy(pysdr_ctx* c) {
  if (!c) return PYSDR_ERR_ARG;
  if (c->comm && g_rccl.CommDestroy) {
    (void)hipSetDevice(c->cfg.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    g_rccl.CommDestroy(c->comm);
  }
  c->comm = nullptr;
  return PYSDR_OK;
}

}  // extern "C"
