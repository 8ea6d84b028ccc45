/*
 * pysdr_hip.h -- C ABI of libpysdr_hip.so: the MI355X (gfx950) implementation of
 * the pySDR receiver hot path (per-sub-receiver LO mix -> rational polyphase
 * resample -> detect -> AF filter -> AGC, plus the PSD FFT).
 *
 * The reference (aa2il/pySDR) is pure Python and has no FFI of its own; its hot
 * path is the Python surface of module `sig_proc` (absent from the tree,
 * reconstructed from call sites in SURVEY.md 2.2).  Every entry point below names
 * the reference call site it stands behind.  The Python facade
 * `pysdr_amd/sig_proc.py` binds these with ctypes.
 *
 * Conventions
 *  - plain C, no C++/torch types; all functions return 0 or a negative
 *    pysdr_status (never throw, never abort) -- the reference convention is
 *    "print + carry on" (receiver.py:603-605).
 *  - caller owns every host buffer; the context owns all device memory.
 *  - pysdr_process*() are called from ONE thread (the RX thread,
 *    receiver.py:684-725).  Setters may be called concurrently from another thread
 *    (the Qt thread, gui.py:1713,1938) and take effect at the next process call.
 *  - complex data are interleaved float pairs (numpy complex64 layout).
 */
#ifndef PYSDR_HIP_H
#define PYSDR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PYSDR_MAX_RX 8 /* reference MAX_RX = 6 (params.py:33) */

typedef enum {
  PYSDR_OK = 0,
  PYSDR_ERR_ARG = -1,      /* bad argument                                   */
  PYSDR_ERR_NO_DEVICE = -2,/* no HIP device / hipSetDevice failed            */
  PYSDR_ERR_HIP = -3,      /* a HIP runtime call failed (see pysdr_last_error)*/
  PYSDR_ERR_FFT = -4,      /* rocFFT failure                                  */
  PYSDR_ERR_STATE = -5,    /* call order / capacity violation                */
  PYSDR_ERR_RCCL = -6      /* RCCL failure                                    */
} pysdr_status;

/* Index into the reference's MODES list (Tables.py:34). */
typedef enum {
  PYSDR_AM = 0, PYSDR_AM_SYNCH = 1, PYSDR_SSB = 2, PYSDR_USB = 3, PYSDR_LSB = 4,
  PYSDR_CW = 5, PYSDR_IQ = 6, PYSDR_WFM = 7, PYSDR_WFM2 = 8, PYSDR_NFM = 9,
  PYSDR_RTTY = 10
} pysdr_mode;

/* Rates and sizes: the fields of the reference's P object that Receiver reads
 * (params.py:405-406,440-444; receiver.py:818-820). */
typedef struct {
  double  srate;       /* P.SRATE, input complex sample rate (Hz)              */
  int32_t up, down;    /* P.UP, P.DOWN = up_dn(SRATE, FS_OUT)                  */
  int32_t in_chunk;    /* P.IN_CHUNK_SIZE, nominal samples per chunk           */
  int32_t max_chunks;  /* capacity: chunks per pysdr_process_batch call, <= 16384 */
  int32_t ntaps_dec;   /* P.FILT_LEN, prototype length at srate*up             */
  int32_t ntaps_af;    /* AF filter length at FS_OUT                           */
  int32_t device;      /* HIP device ordinal                                   */
  int32_t reserved;
} pysdr_cfg;

typedef struct pysdr_ctx pysdr_ctx;
typedef struct pysdr_spectrum pysdr_spectrum;

/* rx.agc fields read by watchdog.py:298-302 */
typedef struct { float agc, gain, maxbuf, ref, err; } pysdr_agc_state;

/* Per-RX result of one pysdr_process() call.  `am`/`iq` are caller buffers with
 * room for `cap` output samples (complex ones need 2*cap floats); either may be
 * NULL to skip the copy.  On return n_out = samples produced (1023/1024 at
 * 8 MS/s -> 48 kHz, SURVEY.md 5 "non-integer chunk ratio"). */
typedef struct {
  float*  am;            /* rx.am  : demodulated audio (receiver.py:235)       */
  float*  iq;            /* rx.iq  : baseband IQ at FS_OUT (receiver.py:265)   */
  int32_t cap;
  int32_t n_out;
  int32_t am_is_complex; /* 1 in IQ mode                                        */
  float   peak_in;       /* max |x|^2 of the raw chunk (rx.auto_mute input)    */
} pysdr_out;

/* ---- library ------------------------------------------------------------- */
const char* pysdr_strerror(int status);
const char* pysdr_last_error(void);          /* text of the last HIP/rocFFT error (thread local) */
int pysdr_device_count(int* n);
int pysdr_version(void);

/* ---- context = one wideband stream + its sub-receivers ------------------------
 * stands behind SDR_EXECUTIVE.create_Receivers (receiver.py:826-835). */
int  pysdr_create(const pysdr_cfg* cfg, pysdr_ctx** out);
void pysdr_destroy(pysdr_ctx* ctx);

/* dsp.Receiver(P, frq, irx, ...) (receiver.py:835).  lo_freq is the generator
 * frequency (= -frq); h = rx.dec.h prototype (ntaps_dec doubles);
 * af = complex AF taps (2*ntaps_af doubles, re/im interleaved). */
int pysdr_rx_add(pysdr_ctx* ctx, int mode, double lo_freq, const double* h,
                 const double* af, double bfo, int* irx);

/* rx.lo.change_freq(f) -> actual f (receiver.py:112,352; gui.py:1938,2011) */
int pysdr_set_lo(pysdr_ctx* ctx, int irx, double f_hz, double* f_actual);
/* rx.dec.h = rx.dec.filter_bank[idx] (receiver.py:127,371; gui.py:1713,1762) */
int pysdr_set_dec_taps(pysdr_ctx* ctx, int irx, const double* h, int n);
/* P.MODE / P.AF_FILTER_NUM / P.BFO as read by Receiver each chunk
 * (receiver.py:114-116,130-131; gui.py:1756-1757) */
int pysdr_set_mode(pysdr_ctx* ctx, int irx, int mode, const double* af, int n, double bfo);
/* Broadcast FM (modes WFM/WFM2; gui.py:1703-1704 `rx.demod.wfm_video.h = wfm_filter_bank[idx]`):
 * video = pre-detection low-pass at SRATE (ntaps_dec doubles); resamp = prototype of the
 * fs1 -> FS_OUT resampler (a multiple of up2 doubles).  pysdr_wfm_params gives the IF
 * decimation d1 (fs1 = SRATE/d1 ~ 250 kHz) and up2/down2 = up_dn(fs1, FS_OUT). */
int pysdr_wfm_params(double srate, double fs_out, int* d1, int* up2, int* down2);
int pysdr_set_wfm_taps(pysdr_ctx* ctx, int irx, const double* video, int nv, const double* resamp, int nr);
/* rx.agc.reset() / rx.demod.am_pll.reset() (receiver.py:648-649): what = 1 AGC, 2 PLL, 3 both */
int pysdr_reset(pysdr_ctx* ctx, int irx, unsigned what);
int pysdr_agc_get(pysdr_ctx* ctx, int irx, pysdr_agc_state* st);
/* The serial PLLs (rx.demod.am_pll, receiver.py:649; the WFM2 pilot PLL) run time-parallel on
 * long calls: `segments` the last call was cut into, `patched` = segments a serial patch-up pass
 * had to recompute because the loop had not forgotten its start state (0 for a locked loop). */
int pysdr_pll_stats(pysdr_ctx* ctx, int irx, int* segments, int* patched);
/* A/B knob for the above: at most `max_segments` per call (1 = the plain serial walk, 0 = default) */
int pysdr_set_pll_segments(pysdr_ctx* ctx, int max_segments);
/* WFM2 pilot loop of the last batch: the widest join between two segments of the time-parallel walk BEFORE any patching --
 * |phase difference| in words of 2^32 (accepted up to 512) and |integrator difference| in rad/sample (up to 1e-9).  A
 * diagnostic of this build (no reference call site): what a shorter / cheaper warm-up setting (PYSDR_WFM_PLL) is judged by. */
int pysdr_pll_join_margin(pysdr_ctx* ctx, int irx, int* max_words, float* max_dw);
/* AM-Synch carrier loop of the last batch: how many of its segments got their start state from ONE LINEAR SOLVE over the
 * warm-up window instead of walking it (the loop is linear in the phase domain while its detector does not wrap, which is
 * checked per window; a noisy or badly guessed window is walked as before).  A diagnostic of this build. */
int pysdr_pll_linear_starts(pysdr_ctx* ctx, int irx, int* n);
/* NFM noise squelch (north_star "AGC/squelch"; design notes sigs/squelch.m:92-145): per chunk the
 * mean |2nd difference| of the discriminator output is smoothed (one pole) and the chunk is
 * muted while it exceeds `thresh`; thresh <= 0 disables (default). */
int pysdr_set_squelch(pysdr_ctx* ctx, int irx, float thresh);
int pysdr_squelch_get(pysdr_ctx* ctx, int irx, float* level, int* open);
/* The RATIO squelch, as the only design the reference holds sketches it (sigs/squelch.m:92-145; no run-time call site): z1 =
 * low-pass < 3 kHz and z2 = high-pass > 4 kHz of the discriminator output (`lp`, `hp`: FIR taps, ntaps <= 64, for the
 * context's FS_OUT; there: elliptic IIRs of order 5, :103-105), sq1 / sq2 = one-pole envelopes of |z1| / |z2| per SAMPLE with
 * alpha = 0.001 (:131-134), and the gate open while sq1 / sq2 >= min_ratio (:145) -- independent of the signal's level.  One
 * decision per chunk (the AGC block), on the envelopes behind its last sample.  min_ratio > 0 arms it for that sub-receiver
 * (NFM) and takes precedence over pysdr_set_squelch; 0 disarms.  pysdr_squelch_ratio_get: the two envelopes and the gate
 * behind the last call.  The two FIRs read the detector output the AF stage stages and keeps for its own filter of ntaps_af
 * taps: ntaps <= min(64, 12 ceil(ntaps_af / 12) + 3, history - 1), history = 16 ceil((8 ceil(ntaps_af / 8) + 5) / 16) -- 63 from
 * 49 AF taps on, 64 from 61 on.  Longer ones are refused (PYSDR_ERR_ARG, pysdr_last_error names both lengths) and nothing of
 * the context changes. */
int pysdr_set_squelch_ratio(pysdr_ctx* ctx, int irx, float min_ratio, const float* lp, const float* hp, int ntaps);
int pysdr_squelch_ratio_get(pysdr_ctx* ctx, int irx, float* sq_lp, float* sq_hp, int* open);
/* AGC on/off and reference level */
int pysdr_set_agc(pysdr_ctx* ctx, int irx, int enable, float ref);

/* rx.demod_data(x) for every RX of the stream on ONE chunk of host samples
 * (receiver.py:231-235,724-725).  n = complex samples; outs[num_rx]. */
int pysdr_process(pysdr_ctx* ctx, const float* iq_interleaved, size_t n, pysdr_out* outs);

/* Same arithmetic on `nchunks` consecutive chunks of `chunk_len` samples in one
 * launch sequence; results are identical, bit for bit, to nchunks pysdr_process() calls -- except
 * in the two modes with a serial loop (AM-Synch carrier PLL, WFM2 pilot PLL): a long call runs the
 * loop in segments whose joins are accepted within 2e-6 rad / 512 words of 2^32 of phase, so there
 * the audio equals the chunk-by-chunk run within the 1e-5 parity bar, not bitwise
 * (pysdr_set_pll_segments(ctx, 1) forces the serial walk).
 * on_device != 0: iq is a device pointer (pysdr_dev_alloc) -- the replay path
 * (receiver.py:541-559) and the throughput benchmark. */
int pysdr_process_batch(pysdr_ctx* ctx, const void* iq, int nchunks, size_t chunk_len, int on_device);
/* Batch pipelining (a build feature, no reference call site; the analogue in the reference is MP_SCHEME 2/3 running the
 * demodulators beside the chunk acquisition, receiver.py:726-739).  A call is three groups of launches: F the front end
 * (mix + decimate, and the parallel kernel in front of a serial loop), P the segment walks of a serial loop (AM-Synch
 * carrier PLL, WFM2 pilot PLL: thousands of single-wave chains, latency bound, no LDS), T the tail (detector + AF
 * filter, AGC, output; for broadcast FM the audio resampler first).  Overlapped, P(k) is queued on a second HIP stream and
 * T(k) is DEFERRED: it is queued behind F(k+1) by the next pysdr_process_batch, or at once by whatever asks for the
 * call's results (pysdr_fetch, pysdr_sync, the state getters, a setter with pending work) -- so the walks of call k run
 * beside the tail of call k-1 and the front end of call k+1.  Results, state and every other entry point are unchanged, bit
 * for bit (tests/test_gpu_overlap.py).  enable = 0 off (default), 1 = the calls with a serial loop in them, 2 = every
 * call (tests: without a loop nothing runs on the second stream, the buffers and the deferral are exercised all the
 * same).  A context that feeds an ingest ring runs single-stream: pysdr_ingest_create* switches this off, and switching it
 * on then fails with PYSDR_ERR_STATE.  pysdr_last_call_overlapped: the form the last call really took. */
/* 0 for a library built from the sources as they are; otherwise a 31-bit hash of the extra compiler flags (A/B switches
 * from PYSDR_*_FLAGS under PYSDR_TUNING=1, or the diagnostic build's) it was built with -- echoed by bench.py. */
int pysdr_build_flags_hash(void);
int pysdr_set_overlap(pysdr_ctx* ctx, int enable);
int pysdr_get_overlap(pysdr_ctx* ctx);
int pysdr_last_call_overlapped(pysdr_ctx* ctx);
/* Copy results of the last process call to the host.  am/iq may be NULL.
 * chunk_nout[nchunks] (may be NULL) receives the per-chunk output counts,
 * peaks[nchunks] the raw-chunk max |x|^2. */
int pysdr_fetch(pysdr_ctx* ctx, int irx, float* am, float* iq, int cap, int* n_out,
                int* am_is_complex, int* chunk_nout, float* peaks);
int pysdr_sync(pysdr_ctx* ctx);

/* Per-call timing with HIP events recorded on the context's stream (a ring of the last
 * 64 calls; back = 0 is the most recent call): which = 0 mix+decimate kernel (front end),
 * 1 detector/AF/AGC kernels and the history roll behind them, 2 whole call, 3 from the start of the call before it to the start of
 * this one (the period of a step when calls follow each other on the stream).  Events are only
 * recorded while enabled. */
int pysdr_set_profile(pysdr_ctx* ctx, int enable);
int pysdr_get_elapsed_ms(pysdr_ctx* ctx, int which, int back, float* ms);
/* tuning knob: LDS bytes of input tile per workgroup in the mix+decimate kernel */
int pysdr_set_tile(pysdr_ctx* ctx, int tile_bytes, int threads);
/* What the context was really created with, so that a benchmark line can echo it (VERDICT r1
 * hygiene): out = {diagnostic build (-DPYSDR_DIAG) 0/1, PYSDR_DEBUG_FLAGS (always 0 outside a
 * diagnostic build), workgroups per CU, output-stage flush cap, tile bytes, threads, CUs,
 * long single-RX prototypes on the matrix cores 0/1}. */
int pysdr_get_tuning(pysdr_ctx* ctx, int32_t out[8]);

/* ---- the front end's decision, without a device ----------------------------------
 * Which form of the mix + decimate front end a decimator of this shape runs on, and with what plan.  Pure
 * arithmetic: needs no device and no context, and is the helper every launch takes its decision from, so what
 * it reports is what a context with this tuning runs.  nrx sub-receivers share a decimator UP/DOWN with an
 * ntaps-tap prototype; tile_bytes, threads, wgs_per_cu, yflush_cap, mfma_enable as pysdr_get_tuning reports them
 * (defaults 0, 1024, 1, 0, 1); want_peak = the raw chunk peak is wanted (1 for a context's main decimator).
 * out = {form, fits (0: the vector plan does not fit the LDS -- such a call is refused),
 *        R, NJ, TPB, MM of the vector instantiation mixdec_kernel<R, NJ, TPB, 0, MM>,
 *        matrix-core shape id (-1 unless form = PYSDR_FORM_MFMA),
 *        taps_lds (1: taps staged in LDS, 0: held in registers), tile_out (outputs per tile),
 *        yflush (tiles per flush of the output stage), tile_cap (samples per LDS tile buffer),
 *        kpad (taps per polyphase branch, padded to 16)}.
 * With PYSDR_FORM_MFMA the vector fields (R .. tile_cap) are 0: that form has a fixed geometry per shape. */
#define PYSDR_FORM_VECTOR 0 /* mixdec_kernel: any number of sub-receivers */
#define PYSDR_FORM_MFMA 1   /* one sub-receiver, long prototype, on the matrix cores */
#define PYSDR_FORM_SMALL 2  /* one sub-receiver, short prototype, small DOWN/UP, no raw peak */
int pysdr_front_end_plan(int nrx, int up, int down, int ntaps, int tile_bytes, int threads, int wgs_per_cu,
                         int yflush_cap, int mfma_enable, int want_peak, int32_t out[12]);
/* What is compiled.  family = PYSDR_FORM_VECTOR: entry `index` = {R, NJ, TPB, MM}; PYSDR_FORM_MFMA: {shape id, UP,
 * DOWN, taps per polyphase branch}.  *count (if not null) = entries of the family; index outside 0 .. count-1 with a
 * null `out` only counts. */
int pysdr_front_end_shapes(int family, int index, int32_t out[4], int* count);
/* Which of its three kernels the PYSDR_FORM_SMALL resampler (broadcast FM's fs1 -> FS_OUT stage) runs for a decimator
 * UP/DOWN with an ntaps-tap prototype, and with what launch.  Pure arithmetic like pysdr_front_end_plan, and the helper
 * the launch itself takes its decision from.  plain = PYSDR_RESAMP_PLAIN as pysdr_get_resamp_tuning reports it (0: the
 * production choice, 1: one output per thread, 2: no wave-per-branch form).
 * out = {eligible for PYSDR_FORM_SMALL 0/1, kernel (0 a wave per polyphase branch, 1 one output per thread, 2 a half-wave
 *        per branch; -1 if not eligible), threads per workgroup, dynamic LDS bytes, outputs per tile,
 *        kpad (taps per polyphase branch, padded to 16), hist_len (input samples kept between calls), input samples of
 *        one tile's LDS span}. */
int pysdr_resamp_plan(int up, int down, int ntaps, int plain, int32_t out[8]);
/* out = {PYSDR_RESAMP_PLAIN, PYSDR_MIXDEC_GRID (0: not held)} as the context read them at create (under PYSDR_TUNING=1) */
int pysdr_get_resamp_tuning(pysdr_ctx* ctx, int32_t out[2]);

/* ---- signal_generator.quad_mixer (receiver.py:552-553,822) --------------------
 * y = x * exp(+j*phi_n), 32-bit phase accumulator, returns phase after n samples */
int pysdr_quad_mixer(int device, const float* x, float* y, size_t n, uint32_t phase0,
                     uint32_t fword, uint32_t* phase_out);
uint32_t pysdr_freq_word(double f_hz, double fs_hz, double* f_actual);

/* ---- convolver.convolve_fast (receiver.py:207,216,862): streaming real FIR.
 * xx = [ntaps-1 history samples | n new samples]; y[i] = sum_k h[k]*xx[i+ntaps-1-k] */
int pysdr_fir_real(int device, const float* xx, const float* h, int ntaps, float* y, size_t n);

/* ---- spectrum (Plotting.py:376,462; gui.py:611-631) --------------------------- */
int  pysdr_spectrum_create(int device, int chunk_size, int nfft, int max_frames,
                           const float* window, pysdr_spectrum** out);
void pysdr_spectrum_destroy(pysdr_spectrum* sp);
/* spectrum.periodogram: one frame of chunk_size (complex or real) host samples ->
 * psd_db[nfft] (complex, fftshifted) or psd_db[nfft/2] (real input) */
int pysdr_spectrum_frame(pysdr_spectrum* sp, const float* x, int is_complex, int db,
                         float* psd_out, int* n_out);
/* nframes frames taken every `hop` samples from a device-resident complex stream;
 * d_out = device [nframes][nfft] float (dB, fftshifted).  The fused 64k path deals its groups of frames over two HIP
 * streams by default (per-kernel durations of a profiler trace then overlap; PYSDR_TUNING=1 PYSDR_PSD_STREAMS=1 for
 * un-overlapped kernel times, INTEGRATION.md "tuning environment"); the call's own stream waits for the side stream. */
int pysdr_spectrum_batch(pysdr_spectrum* sp, const void* d_iq, int nframes, size_t hop,
                         void* d_out);
int pysdr_spectrum_sync(pysdr_spectrum* sp);
/* out = {frames per launch group of the fused 64k path, rocFFT forced 0/1, streams the groups are dealt over,
 * four-step intermediate stored as 24-bit block-scaled fixed point 0/1} */
int pysdr_spectrum_get_tuning(pysdr_spectrum* sp, int32_t out[4]);
int pysdr_spectrum_elapsed_ms(pysdr_spectrum* sp, float* ms);
/* Ordering between the spectrum's stream and a receiver context's stream (both read the same
 * device-resident chunk; Plotting.py:462 runs the PSD after the chunk's demod in one thread):
 * direction 0: spectrum work queued from now on starts after everything queued on ctx so far;
 * direction 1: ctx work queued from now on starts after everything queued on sp so far;
 * direction 2: like 0, but only behind the FRONT END (mix + decimate) of ctx's last process call --
 *   the PSD reads the same input and may run beside the audio-rate stages. */
int pysdr_spectrum_order(pysdr_spectrum* sp, pysdr_ctx* ctx, int direction);

/* ---- waterfall numeric back-end (three_box_plot.plot, Plotting.py:536-626; shift_waterfall
 * :689-695): device history ring [nfft][ncols]; push = shift-in of one PSD line (shorter lines
 * padded with -1e38); roll = np.roll(wf, -nbins, axis=0); image = max(wf - median(mean(wf[:,
 * -cnt:], 1)), nanmax(wf - bkgnd) - pan_dr), returned column-major: image_out[c][i], c = 0 the
 * oldest column (numpy: image_out.reshape(ncols, nfft).T).  mean_out[nfft] is the PSD2 vector the
 * reference feeds to find_peaks (Plotting.py:583,595). */
typedef struct pysdr_waterfall pysdr_waterfall;
int  pysdr_waterfall_create(int device, int nfft, int ncols, pysdr_waterfall** out);
void pysdr_waterfall_destroy(pysdr_waterfall* wf);
int  pysdr_waterfall_push(pysdr_waterfall* wf, const float* line_db, int n, int on_device);
int  pysdr_waterfall_roll(pysdr_waterfall* wf, int nbins);
int  pysdr_waterfall_image(pysdr_waterfall* wf, float pan_dr, float* image_out, float* mean_out,
                           float* bkgnd_out);
/* The same with the dynamic-range maximum taken over the rows [0, npsd) only, npsd = length of the
 * PSD line just pushed: `zz = self.wf[0:npsd,:] - med; zmax = np.nanmax(zz)` (Plotting.py:618-619;
 * a real-input line is half length, :536-540).  image_out stays [ncols][nfft]; the reference draws
 * its first npsd rows. */
int  pysdr_waterfall_image_rows(pysdr_waterfall* wf, float pan_dr, int npsd, float* image_out,
                                float* mean_out, float* bkgnd_out);

/* The peak pick of the display, `peaks, _ = signal.find_peaks(PSD2, distance=dist, height=bkgnd+10)` (Plotting.py:594-602), on
 * the device: local maxima with flat tops (midpoint of a plateau, none at the ends of the line), height >= `height` (double),
 * then SciPy's priority-by-height distance rule with distance = ceil(PEAK_DIST / df) >= 1 (a kept peak removes every peak
 * closer than that).  line == NULL: over the first n values of the averaged line the last pysdr_waterfall_image left on the
 * device (PSD2); otherwise over the n host values given.  idx_out[min(*n_out, cap)] ascending; *n_out = how many there are.
 * Equal heights closer than `distance`: SciPy's choice rests on an unstable argsort; here the higher index outranks. */
int  pysdr_waterfall_peaks(pysdr_waterfall* wf, const float* line, int n, double height, int distance, int* idx_out, int cap,
                           int* n_out);

/* ---- wideband RTTY decoder bank (RTTY_Decoder.decode, rtty.py:483-565,609-700; find_sigs :744-764) ----------------
 * One Baudot decoder per mark bin b in [bin_lo, bin_hi) (space bin b + nbins_shift) and the signal finder over the mark
 * bins [find_lo, find_hi) (may be empty), fed the filterbank lines [nlines][nfft] of pysdr_spectrum_batch: flipped = 1 is
 * the reference's np.flipud order (what RTTY_Filterbank.push returns), flipped = 0 the unflipped order it leaves in device
 * memory.  Both ranges lie inside [0, nfft - nbins_shift); nlines <= max_lines <= 32768.  Lines are numbered 1, 2, ...
 * across calls (pysdr_rtty_reset starts again at 1 with zeroed history); any cut of a stream into calls gives the same
 * results bit for bit.  decode reports, for every decision the call completes (lines n = 30 j; *n_dec of them, at most
 * nlines / 30 + 1) and every decoder, row-major [decision][bin - bin_lo]: codes (-1 nothing emitted, else
 * sym + 32 * FIGS shift), t (the timing line minus one, rtty.py:554) and snr2 (NaN where t - tlast < 25: no symbol
 * decided).  ndet[nlines]: the finder's count per line.  isym / best [nlines][nbins] (NULL skips them): the best
 * symbol and its score per line.  Host buffers; lines is a device pointer when on_device != 0. */
typedef struct pysdr_rtty pysdr_rtty;
int  pysdr_rtty_create(int device, int nfft, int nbins_shift, int bin_lo, int bin_hi, int find_lo, int find_hi,
                       int max_lines, pysdr_rtty** out);
void pysdr_rtty_destroy(pysdr_rtty* rt);
int  pysdr_rtty_reset(pysdr_rtty* rt);
int  pysdr_rtty_decode(pysdr_rtty* rt, const float* lines, int nlines, int on_device, int flipped, int* codes,
                       long long* t, double* snr2, int* n_dec, int* ndet, int* isym, float* best);

/* ---- polyphase channelizer: every channel of an M-channel raster in one pass (a build feature,
 * no reference call site: the reference tunes one sub-receiver per channel, receiver.py:826-835) ----------------------
 * M = 2^a 5^b in [16, 4096] channels centred on k fs / M (k >= M/2: the negative frequency (k - M) fs / M), decimation D
 * with M / D in {1, 2, 4} (output rate fs / D), real prototype h of 1 <= ntaps <= 16 M taps:
 *   y_k[m] = sum_i h[i] x[mD - i] exp(-j 2 pi ((k (mD - i)) mod M) / M),  x[n] = 0 for n < 0, n and m absolute since create
 * or reset -- channel k is NCO(-k fs / M) + the rational resampler with UP = 1 of a sub-receiver's rx.iq.  A call that brings
 * the samples [s0, s1) produces the outputs with s0 <= mD < s1 (any n, 0 and n < D included); any cut of a stream into
 * calls gives the same bits.  Output is channel-major: out[a * out_pitch + i] (complex samples), row a = channel
 * (k_first + a) mod M, a < nk, i < *n_out.
 * pysdr_chan_plan needs no device: PYSDR_ERR_ARG for a shape outside these rules, else out = {passes, radix of pass
 * 0 .. 7 (0 beyond the last), frames per workgroup, frames per FIR work item, threads, LDS bytes, history length
 * ceil(ntaps / M) M - 1, taps per branch, 0}.
 * create: max_taps bounds later set_taps, max_in the samples of one call; no output before the first set_taps
 * (PYSDR_ERR_STATE).  set_taps takes effect at the next call, for the whole window of that call's outputs (rx.dec.h).
 * process: iq / out are device pointers where on_device / out_on_device != 0; with both the call only queues work on the
 * channelizer's stream (pysdr_chan_sync waits for it), otherwise it returns with the host buffers filled.
 * The device staging of a host input (max_in samples) and of a host output (nk rows) is allocated by the first call that
 * passes a host pointer on that side; a handle fed device pointers only never holds it.
 * PYSDR_ERR_STATE: n > max_in, or out_pitch smaller than the call's output count.
 * set_taps / reset / sync / process of one handle exclude each other (a lock in the handle); destroy must not race them. */
typedef struct pysdr_chan pysdr_chan;
int  pysdr_chan_plan(int M, int D, int ntaps, int k_first, int nk, int32_t out[16]);
int  pysdr_chan_create(int device, int M, int D, int k_first, int nk, int max_taps, int max_in, pysdr_chan** out);
void pysdr_chan_destroy(pysdr_chan* ch);
int  pysdr_chan_set_taps(pysdr_chan* ch, const double* h, int ntaps);
int  pysdr_chan_reset(pysdr_chan* ch);
int  pysdr_chan_sync(pysdr_chan* ch);
int  pysdr_chan_process(pysdr_chan* ch, const void* iq, int n, int on_device, void* out, long long out_pitch,
                        int out_on_device, int* n_out);

/* ---- fine channelizer: two channelizer stages for bands wider than 4096 channels of the wanted width (DESIGN.md 3 item
 * 20; a build feature) ------------------------------------------------------------------------------------------------
 * Stage 1 is the channelizer above with M1, D1, h1 and M1 / D1 in {2, 4}; stage 2 applies the same formula with M2, D2, h2
 * (M2 = 2^a 5^b in [16, 1024], M2 / D2 in {1, 2, 4}) to every coarse row that is needed, x := the row as stage 1 rounded
 * it, and keeps the Q = M2 D1 / M1 (even, >= 8) channels q in [-Q/2, Q/2) inside the row's own spacing.  The kept
 * channels of all coarse rows form one raster of Mf = M1 Q fine channels fs / Mf apart: fine channel G is channel
 * (G - c Q) mod M2 of coarse row c mod M1, c = floor((G + Q/2) / Q).  The handle is a pysdr_chan with M = Mf, D = D1 D2:
 * process / reset / sync / destroy above and every object that borrows a channelizer work on it unchanged; row a of the
 * output is fine channel (g_first + a) mod Mf, a < ng <= min(Mf, 65536); a call that brings the samples [s0, s1) produces
 * the outputs with s0 <= m D < s1, and any cut of a stream into calls gives the same bits.  The rows of stage 1 never
 * leave the device.
 * pysdr_chan_fine_plan needs no device: PYSDR_ERR_ARG for a shape outside these rules, else out = {Q, Mf, D, M2 / D2,
 * first coarse row, coarse rows used, frames per workgroup, LDS bytes, stage-1 outputs kept in front of every row, taps
 * per branch of stage 2, passes, radix of pass 0 .. 4 (0 beyond the last)}.
 * fine_set_taps sets both prototypes (1 <= n <= max_taps of the stage), from the next call on; pysdr_chan_set_taps on a
 * fine handle and fine_set_taps on a plain one return PYSDR_ERR_STATE. */
int  pysdr_chan_fine_plan(int M1, int D1, int M2, int D2, int ntaps1, int ntaps2, int g_first, int ng, int32_t out[16]);
int  pysdr_chan_fine_create(int device, int M1, int D1, int M2, int D2, int g_first, int ng, int max_taps1, int max_taps2,
                            int max_in, pysdr_chan** out);
int  pysdr_chan_fine_set_taps(pysdr_chan* ch, const double* h1, int n1, const double* h2, int n2);

/* ---- channel bank: AM / NFM audio, AGC and squelch on every row of a channelizer (a build feature:
 * the reference demodulates one sub-receiver per channel, receiver.py:826-835) -----------------------------------------
 * Every row a < nk of the channelizer `ch` gets a sub-receiver's stage 2 in mode PYSDR_AM or PYSDR_NFM: with y[m] the
 * row (bit for bit what pysdr_chan_process delivers, 0 for m < 0) and c[0 .. ntaps_af) real AF taps, 3 <= ntaps_af <= 255,
 *   d[m] = |y[m]|  (AM)   or   f32(fs_out / (2 pi 5000)) fm(y[m-2], y[m-1], y[m])  (NFM, sigs/nfm.m:124-127),
 *   a[m] = sum_i c[i] d[m - i],   am[m] = a[m] gain.
 * One mode, one AF filter, one AGC setting and one squelch threshold hold for the whole bank.  A call that completes
 * n_out >= 1 outputs is one AGC block per channel: peak = max |a| over its outputs goes through the block AGC (active
 * in AM while enabled; NFM has gain 1), and in NFM with a threshold > 0 the mean of |d[m] - 2 d[m-1] + d[m-2]| over
 * its outputs goes through level += 0.64 (noise - level); a channel whose level exceeds the threshold is closed and gets
 * gain 0.  A call that completes no output changes no AGC and no squelch state.  The un-gained a does not depend on how
 * a stream is cut into calls, bit for bit; am, AGC and squelch do, by definition.
 * pysdr_bank_plan needs no device: PYSDR_ERR_ARG for nk outside [1, 4096], ntaps_af outside [3, 255] or max_out < 1, else
 * out = {outputs per workgroup, threads, LDS bytes, workgroups per row for max_out outputs, history samples kept per
 * row, taps rounded up to steps of 8, 0, 0}.
 * create borrows ch, which must outlive the bank, and resets it (pysdr_chan_reset: the bank's stream starts at sample 0
 * of an empty channelizer); while a bank exists, feed ch only through it.  fs_out = the channelizer's
 * output rate fs / D (the NFM scale).  No output before the first set_mode (PYSDR_ERR_STATE); set_mode takes a mode and
 * ntaps == ntaps_af real taps and holds from the next call on, for the whole AF window of that call's outputs; any other
 * mode or tap count: PYSDR_ERR_ARG.  set_agc: enable and the target block peak ref > 0 (0.5 at create); set_squelch: the
 * threshold, 0 = off.  reset also resets the channelizer.
 * process: iq as in pysdr_chan_process (device pointer where on_device != 0).  am[a * am_pitch + i], i < *n_out, is a host
 * or (am_on_device != 0) device buffer, or NULL: the results stay on the device for pysdr_bank_fetch.  With a device or
 * no am buffer and device input the call only queues work on the channelizer's stream (pysdr_bank_sync waits for it).
 * PYSDR_ERR_STATE: n > max_in of the channelizer, or am_pitch smaller than the call's output count.
 * state: agc (smoothed peak), gain (before the gate), maxbuf (last block peak), squelch level and gate of every channel,
 * [nk] each, NULL skips.  fetch: the last call's outputs of the named rows only -- am[i * pitch + j] and the channel
 * samples iq[2 (i * pitch + j)] of row rows[i]; either may be NULL.  After a call that completed no output (and after
 * create and reset) there is nothing to fetch: the buffers are left as they are.
 * The calls on one handle exclude each other (a lock in the handle); destroy must not race them.  An error leaves the
 * handle usable.
 * The complex-tap modes: pysdr_bank_set_mode_cplx takes mode PYSDR_USB, PYSDR_LSB or PYSDR_CW and
 * ntaps == ntaps_af complex taps c = af_re + j af_im (create names only the start mode, and set_mode's real taps cannot
 * express these modes: both go on refusing them); it holds from the next call on like set_mode, with the same locking
 * and stream discipline.  NULL pointers, another tap count or any other mode (AM, NFM, SSB, IQ, ...): PYSDR_ERR_ARG, the
 * handle unchanged.  With m the absolute output index since create / reset,
 *   d[m] = y[m]  (USB, LSB)   or   y[m] exp(j 2 pi ph(m) / 2^32), ph(m) = fword m mod 2^32 as a signed 32-bit value,
 *          fword = pysdr_freq_word(bfo_hz, fs_out)  (CW; bfo_hz is not used otherwise),
 *   a[m] = Re sum_i c[i] d[m - i],   am[m] = a[m] gain,
 * and the block AGC is active while enabled, as in AM.  There is no squelch in these modes: a threshold is ignored, level
 * keeps its value and every gate stays open.  The un-gained a does not depend on how the stream is cut into calls, bit for
 * bit, the BFO phase included.  The kernels of these modes use twice the LDS bytes pysdr_bank_plan reports. */
typedef struct pysdr_bank pysdr_bank;
int  pysdr_bank_plan(int nk, int ntaps_af, int max_out, int32_t out[8]);
int  pysdr_bank_create(pysdr_chan* ch, double fs_out, int mode, int ntaps_af, pysdr_bank** out);
void pysdr_bank_destroy(pysdr_bank* b);
int  pysdr_bank_set_mode(pysdr_bank* b, int mode, const double* af, int ntaps);
int  pysdr_bank_set_mode_cplx(pysdr_bank* b, int mode, const double* af_re, const double* af_im, int ntaps, double bfo_hz);
int  pysdr_bank_set_agc(pysdr_bank* b, int enable, float ref);
int  pysdr_bank_set_squelch(pysdr_bank* b, float thresh);
int  pysdr_bank_reset(pysdr_bank* b);
int  pysdr_bank_process(pysdr_bank* b, const void* iq, int n, int on_device, float* am, long long am_pitch,
                        int am_on_device, int* n_out);
int  pysdr_bank_state(pysdr_bank* b, float* agc, float* gain, float* maxbuf, float* level, uint8_t* open);
int  pysdr_bank_fetch(pysdr_bank* b, const int* rows, int nrows, float* am, float* iq, long long pitch);
int  pysdr_bank_sync(pysdr_bank* b);

/* ---- CW skimmer: a Morse decoder on every row of a channelizer (a build feature with a definition
 * of its own: the reference holds no Morse decoder) ----------------------------------------------------------------------
 * Every row a < nk of the channelizer `ch` gets one decoder that walks the power of the row's samples y[m] (bit for bit
 * what pysdr_chan_process delivers) in order: envelope, peak and noise-floor followers in float32 with every operation
 * rounded on its own, a key decision with hysteresis, and from there integer arithmetic -- mark lengths, a dot length
 * that follows adjacent short / long marks, the element string `code` behind a leading 1 (dot appends 0, dash 1; 0 = more
 * than 7 elements), character and word-space events.  DESIGN.md 3 item 18 is the normative text, step by step.  The
 * settings hold for the whole bank and arrive already derived (pysdr_amd.cw.params): the smoothing constants a_s, a_p,
 * a_n in (0, 1], snr_min, hi >= lo and fl > 0, and the dot lengths d0, dmin, dmax in 1 / 16 sample with
 * 16 <= dmin <= d0 <= dmax <= 2^22, and the number n0 of settling samples in [1, 2^22] during which the noise floor
 * is the peak and no key decision is made (seen counts them; they cover the run-in of the channelizer's filter).  Any cut of a stream into calls gives the same events and the same state bits; a call
 * that completes no output launches nothing and changes no state.
 * pysdr_cw_plan needs no device: PYSDR_ERR_ARG for nk outside [1, 4096], max_out outside [1, 2^21] or a cfg outside
 * these rules, else out = {rows per workgroup, threads, LDS bytes, tile samples, event cap, workgroups, 0, 0}; the event
 * cap 2 (max_out / 3 + 1) is the most events one channel can emit in a call of max_out outputs.
 * create borrows ch, which must outlive the skimmer, and resets it (pysdr_chan_reset); while a skimmer exists, feed ch
 * only through it.  reset also resets the channelizer.
 * process: iq as in pysdr_chan_process (device pointer where on_device != 0); the decoder is queued behind the
 * channelizer on the channelizer's stream.  counts[nk] (events of every row in this call) and
 * events[a * ev_pitch + j], j < counts[a], are host buffers or NULL: with NULL the results stay on the device (and a call
 * with device input and no host buffer only queues work; pysdr_cw_sync waits for it).  An event word is
 * (index of the output within the call) << 9 | c, c = the character's code 0 .. 255, or 256 = word space.
 * PYSDR_ERR_STATE: n > max_in of the channelizer, the call would complete more than max_out outputs, or ev_pitch smaller
 * than the event cap; the stream does not advance.
 * fetch: the last call's event slots of the named rows only, events[i * pitch + j] for rows[i], pitch >= the event cap;
 * runs of consecutive rows go as one strided copy.  After a call that completed no output it copies nothing.
 * state: s, pk, nf [nk] and ints [nk][8] = key, run, dot, last, code, nel, sp, seen of every channel; NULL skips.
 * Calls on one handle exclude each other; an error leaves the handle usable. */
typedef struct pysdr_cw_cfg {
  float a_s, a_p, a_n;      /* smoothing constants of the envelope, the peak's decay and the noise floor */
  float snr_min, hi, lo;    /* presence: pk > snr_min nf; key down above q hi, up below q lo */
  float fl;                 /* floor of the threshold: q >= pk^2 fl */
  int32_t d0, dmin, dmax;   /* dot length at the start and its limits, 1 / 16 sample */
  int32_t n0;               /* settling samples after create / reset: nf = pk and the key stays up; 1 <= n0 <= 2^22 */
} pysdr_cw_cfg;
typedef struct pysdr_cw pysdr_cw;
int  pysdr_cw_plan(int nk, int max_out, const pysdr_cw_cfg* cfg, int32_t out[8]);
int  pysdr_cw_create(pysdr_chan* ch, const pysdr_cw_cfg* cfg, int max_out, pysdr_cw** out);
void pysdr_cw_destroy(pysdr_cw* cw);
int  pysdr_cw_reset(pysdr_cw* cw);
int  pysdr_cw_sync(pysdr_cw* cw);
int  pysdr_cw_process(pysdr_cw* cw, const void* iq, int n, int on_device, int* n_out, int32_t* counts, int32_t* events,
                      long long ev_pitch);
int  pysdr_cw_fetch(pysdr_cw* cw, const int* rows, int nrows, int32_t* events, long long pitch);
int  pysdr_cw_state(pysdr_cw* cw, float* s, float* pk, float* nf, int32_t* ints);

/* ---- PSK31 skimmer: a Varicode decoder on a fine raster inside every row of a channelizer (a build
 * feature with a definition of its own: the reference holds no PSK decoder) ------------------------------------------------
 * The channelizer `ch` delivers rows at fs_out = S baud, S = 8 or 12 samples per symbol.  Inside every row a < nk a bank
 * of NSUB = 4 S decoders runs, decoder j tuned (2 j - NSUB + 1) baud / 32 from the row's centre; fine row F = a NSUB + j.
 * Each mixes the row down (table tw[NT][2] = (cos, -sin)(2 pi t / NT), NT = 32 S, indexed by (q k) mod NT of the absolute
 * output index k), applies the matched filter g[L], L = 2 S, follows the symbol energy at every phase of the symbol,
 * takes one symbol per S + d samples at the best phase, decides the differential bit, measures the coherence qn / qd of
 * the doubled differential phase (the squelch `open`) and shifts Varicode bits until 00.  All float arithmetic is
 * float32 with every operation rounded on its own; DESIGN.md 3 item 19 is the normative text, step by step.  The
 * settings hold for the whole bank: a_t, a_q in (0, 1], 0 < lo <= hi, hy > 0, 0 < pmax <= 1e18 (all finite), 1 <= n0 <= 2^22
 * settling symbols during which the squelch stays shut.  Any cut of a stream into calls gives the same events and the
 * same state bits; a call that completes no output launches nothing and changes no state.
 * pysdr_psk_plan needs no device: PYSDR_ERR_ARG for S not 8 or 12, nk < 1, nk NSUB > 2^18, max_out outside [1, 2^20] or a
 * cfg outside these rules, else out = {rows per workgroup, threads, LDS bytes, tile samples, event cap, workgroups,
 * NSUB, 0}; the event cap max_out / (3 S / 2) + 1 is the most events one decoder can emit in a call of max_out outputs.
 * create borrows ch, which must outlive the skimmer, and resets it; while a skimmer exists, feed ch only through it.  tw
 * and g are host arrays of NT x 2 and L floats, copied.  reset also resets the channelizer.
 * process: iq as in pysdr_chan_process (device pointer where on_device != 0); the decoders are queued behind the
 * channelizer on the channelizer's stream.  counts[nk NSUB] (events of every fine row in this call), events[F * ev_pitch
 * + i], i < counts[F], and the end state's qn[nk NSUB] and open[nk NSUB] are host buffers or NULL: with NULL the results
 * stay on the device (and a call with device input and no host buffer only queues work; pysdr_psk_sync waits for it).
 * An event word is (index of the output within the call) << 11 | code, code = the Varicode bits 1 .. 2047.
 * PYSDR_ERR_STATE: n > max_in of the channelizer, the call would complete more than max_out outputs, or ev_pitch smaller
 * than the event cap; the stream does not advance.
 * fetch: the last call's event slots of the named fine rows only, events[i * pitch + k] for rows[i], pitch >= the event
 * cap; runs of consecutive rows go as one strided copy.  After a call that completed no output it copies nothing.
 * state: e [S][nk NSUB], f [4][nk NSUB] = qn, qd, cr, ci and ints [5][nk NSUB] = pt, cnt, sh, open, seen; NULL skips.
 * Calls on one handle exclude each other; an error leaves the handle usable. */
typedef struct pysdr_psk_cfg {
  float a_t, a_q;           /* smoothing constants of the symbol energies and of the coherence sums */
  float hi, lo;             /* squelch: opens at qn >= hi qd, shuts below lo qd */
  float hy;                 /* the timing phase moves when the best energy exceeds hy times the current one */
  float pmax;               /* outputs of power above this (or not finite) are blanked */
  int32_t n0;               /* settling symbols after create / reset */
} pysdr_psk_cfg;
typedef struct pysdr_psk pysdr_psk;
int  pysdr_psk_plan(int nk, int S, int max_out, const pysdr_psk_cfg* cfg, int32_t out[8]);
int  pysdr_psk_create(pysdr_chan* ch, int S, const pysdr_psk_cfg* cfg, const float* tw, const float* g, int max_out,
                      pysdr_psk** out);
void pysdr_psk_destroy(pysdr_psk* psk);
int  pysdr_psk_reset(pysdr_psk* psk);
int  pysdr_psk_sync(pysdr_psk* psk);
int  pysdr_psk_process(pysdr_psk* psk, const void* iq, int n, int on_device, int* n_out, int32_t* counts, int32_t* events,
                       long long ev_pitch, float* qn, int32_t* open);
int  pysdr_psk_fetch(pysdr_psk* psk, const int* rows, int nrows, int32_t* events, long long pitch);
int  pysdr_psk_state(pysdr_psk* psk, float* e, float* f, int32_t* ints);

/* ---- RTTY raster skimmer: a Baudot decoder on a fine raster inside every row of a channelizer (a
 * build feature with a definition of its own: the reference's RTTY decoder, pysdr_rtty_*, works on dB lines of its own
 * FFT and cannot run on channelizer rows) ---------------------------------------------------------------------------------
 * 45.45 baud (500 / 11), 170 Hz shift, mark the upper tone.  The channelizer `ch` delivers rows at fs_out = S baud, S = 22
 * or 33 samples per bit.  Inside every row a < nk a bank of NSUB = S decoders runs, decoder j centred (2 j - S + 1) baud / 8
 * from the row's centre; fine row F = a S + j.  Each mixes the row down to its space tone, q = 2 j - S - 14, and its mark
 * tone, q = 2 j - S + 16, in units of baud / 8 (table tw[NT][2] = (cos, -sin)(2 pi t / NT), NT = 8 S, indexed by (q k) mod
 * NT of the absolute output index k), applies the one-bit window g[S] to both and compares the two powers at every output;
 * a mark-to-space edge starts a character, whose start, five data and stop bits are sampled S outputs apart from half a
 * bit after the edge; the contrast qn / qd of the two powers and the balance of the two tones' levels bm, bs gate the
 * output (the squelch `open`).  All float arithmetic is float32 with every operation rounded on its own; DESIGN.md 3 item
 * 21 is the normative text, step by step.  The settings hold for the whole bank: a_q, a_b in (0, 1], 0 < lo <= hi <= 1,
 * 0 < bal <= 1, 0 < pmax <= 1e18 (all finite), 1 <= n0 <= 2^22 settling instants during which the squelch stays shut.  Any
 * cut of a stream into calls gives the same events and the same state bits; a call that completes no output launches
 * nothing and changes no state.
 * pysdr_fsk_plan needs no device: PYSDR_ERR_ARG for S not 22 or 33, nk < 1, nk S > 2^18, max_out outside [1, 2^20] or a cfg
 * outside these rules, else out = {rows per workgroup, threads, LDS bytes, tile samples, event cap, workgroups, NSUB, 0};
 * the event cap max_out / (6 S + S / 2 + 1) + 1 is the most events one decoder can emit in a call of max_out outputs.
 * create borrows ch, which must outlive the skimmer, and resets it; while a skimmer exists, feed ch only through it.  tw
 * and g are host arrays of NT x 2 and S floats, copied.  reset also resets the channelizer.
 * process: iq as in pysdr_chan_process (device pointer where on_device != 0); the decoders are queued behind the
 * channelizer on the channelizer's stream.  counts[nk S] (events of every fine row in this call), events[F * ev_pitch + i],
 * i < counts[F], and the end state's qn[nk S] and open[nk S] are host buffers or NULL: with NULL the results stay on the
 * device (and a call with device input and no host buffer only queues work; pysdr_fsk_sync waits for it).
 * An event word is (index of the output within the call) << 6 | code, code = the five data bits + 32 in figures shift.
 * PYSDR_ERR_STATE: n > max_in of the channelizer, the call would complete more than max_out outputs, or ev_pitch smaller
 * than the event cap; the stream does not advance.
 * fetch: the last call's event slots of the named fine rows only, events[i * pitch + k] for rows[i], pitch >= the event
 * cap; runs of consecutive rows go as one strided copy.  After a call that completed no output it copies nothing.
 * state: f [4][nk S] = qn, qd, bm, bs and ints [8][nk S] = st, cnt, sh, nb, prev, fig, open, seen; NULL skips.
 * Calls on one handle exclude each other; an error leaves the handle usable. */
typedef struct pysdr_fsk_cfg {
  float a_q, a_b;           /* smoothing constants of the contrast sums and of the two tones' levels */
  float hi, lo;             /* squelch: opens at qn >= hi qd, shuts below lo qd */
  float bal;                /* and only while the weaker tone's level is at least bal times the stronger's */
  float pmax;               /* tone powers above this (or not finite) are blanked */
  int32_t n0;               /* settling instants after create / reset */
} pysdr_fsk_cfg;
typedef struct pysdr_fsk pysdr_fsk;
int  pysdr_fsk_plan(int nk, int S, int max_out, const pysdr_fsk_cfg* cfg, int32_t out[8]);
int  pysdr_fsk_create(pysdr_chan* ch, int S, const pysdr_fsk_cfg* cfg, const float* tw, const float* g, int max_out,
                      pysdr_fsk** out);
void pysdr_fsk_destroy(pysdr_fsk* fsk);
int  pysdr_fsk_reset(pysdr_fsk* fsk);
int  pysdr_fsk_sync(pysdr_fsk* fsk);
int  pysdr_fsk_process(pysdr_fsk* fsk, const void* iq, int n, int on_device, int* n_out, int32_t* counts, int32_t* events,
                       long long ev_pitch, float* qn, int32_t* open);
int  pysdr_fsk_fetch(pysdr_fsk* fsk, const int* rows, int nrows, int32_t* events, long long pitch);
int  pysdr_fsk_state(pysdr_fsk* fsk, float* f, int32_t* ints);

/* ---- packet skimmer: an AX.25 decoder on every row of an NFM raster (a build feature with a
 * definition of its own: the reference holds no packet decoder) -------------------------------------------------------
 * 1200 baud AFSK (Bell 202: mark 1200 Hz, space 2200 Hz) on narrow-band FM, HDLC framing, AX.25 UI frames: APRS.  The sixth
 * client of a channelizer (either kind; rows at any fs_out from 9600 to 48000 Hz, which need not be a multiple of the
 * baud rate).  Every row a < nk is discriminated (d[m] = Im(y[m] conj(y[m - 1])), no division), d is mixed down by the
 * two tones (table tw[1024][2] = (cos, -sin)(2 pi k / 1024), indexed by the top ten bits of (m w) mod 2^32 of the
 * absolute output index m), both go through the bit window g[L], L = round(fs_out / 1200) in [8, 40], and their powers
 * are compared by eight slicers, gain[s] P_space > P_mark: decoder dec = a * 8 + s.  Each decoder has a 32-bit bit clock
 * (+ w_baud per output, pulled towards 0 by clk >> pll_shift at every change of its slicer, a bit sampled where it turns
 * negative), an NRZI / HDLC receiver with bit de-stuffing, the CRC-16 of AX.25 and a frame buffer of 83 words.  All float
 * arithmetic is float32 with every operation rounded on its own, the rest is integer; DESIGN.md 3 item 29 is the
 * normative text, step by step.  Any cut of a stream into calls gives the same events and the same state; a call that
 * completes no output launches nothing and changes no state.
 * pysdr_pkt_plan needs no device: PYSDR_ERR_ARG for L outside [8, 40], nk < 1, 8 nk > 2^18, max_out outside [1, 2^20] or a
 * cfg outside its rules (every gain > 0, 0 < pmax <= 1e18, all finite; the three words > 0 and w_baud <= 2^29; pll_shift
 * in [1, 4]), else out = {rows per workgroup, threads, LDS bytes, tile samples, event cap, workgroups, slicers per row,
 * words of a frame buffer}; the event cap 84 + (ceil(max_out / (2^31 / w_baud + 1)) - 1) / 24, in words, is the most one
 * decoder can emit in a call of max_out outputs.
 * create borrows ch, which must outlive the skimmer, and resets it; while a skimmer exists, feed ch only through it.  tw
 * and g are host arrays of 1024 x 2 and L floats, copied.  reset also resets the channelizer.
 * process: as pysdr_fsk_process without its two further outputs; counts[8 nk] are the words of every decoder in this
 * call, events[dec * ev_pitch + i], i < counts[dec].  A frame's event is a header word, (index within the call of the
 * output that completed the closing flag) << 10 | n, and then (n + 3) / 4 words with the frame's n bytes, FCS left out,
 * the first byte in the low bits, zero-padded; only frames of 15 <= n <= 330 bytes with a good FCS are events.
 * PYSDR_ERR_STATE: n > max_in of the channelizer, the call would complete more than max_out outputs, or ev_pitch smaller
 * than the event cap; the stream does not advance.
 * fetch: the last call's event words of the named decoders, events[i * pitch + k] for rows[i], pitch >= the event cap.
 * state: ints [10][8 nk] = clk, xprev, xlast, sr, ones, inframe, byte, nb, nbytes, crc and frames [8 nk][83], the frame
 * buffers (bytes four to a word; a byte that opens a word clears the rest of it); NULL skips.
 * Calls on one handle exclude each other; an error leaves the handle usable. */
typedef struct pysdr_pkt_cfg {
  float gain[8];            /* the slicers' weights of the space tone's power */
  float pmax;               /* tone powers above this (or not finite) are blanked */
  uint32_t w_mark, w_space; /* the tones' phase per row output, in turns / 2^32 */
  uint32_t w_baud;          /* the bit clock's */
  int32_t pll_shift;        /* the clock's pull at a change of the slicer: clk -= clk >> pll_shift */
} pysdr_pkt_cfg;
typedef struct pysdr_pkt pysdr_pkt;
int  pysdr_pkt_plan(int nk, int L, int max_out, const pysdr_pkt_cfg* cfg, int32_t out[8]);
int  pysdr_pkt_create(pysdr_chan* ch, int L, const pysdr_pkt_cfg* cfg, const float* tw, const float* g, int max_out,
                      pysdr_pkt** out);
void pysdr_pkt_destroy(pysdr_pkt* pkt);
int  pysdr_pkt_reset(pysdr_pkt* pkt);
int  pysdr_pkt_sync(pysdr_pkt* pkt);
int  pysdr_pkt_process(pysdr_pkt* pkt, const void* iq, int n, int on_device, int* n_out, int32_t* counts, int32_t* events,
                       long long ev_pitch);
int  pysdr_pkt_fetch(pysdr_pkt* pkt, const int* rows, int nrows, int32_t* events, long long pitch);
int  pysdr_pkt_state(pysdr_pkt* pkt, int32_t* ints, uint32_t* frames);

/* ---- SSTV skimmer: a VIS and image decoder on every row of a raster (a build feature with a
 * definition of its own: the reference holds no SSTV decoder) -----------------------------------------------------------
 * Analogue slow-scan television: the VIS header, an anchor on the end of line 0's sync pulse, a free-running line clock
 * and the pixels.  The seventh client of a channelizer (either kind; rows at any fs_out from 8000 to 48000 Hz).  Every
 * row a < nk is detected (det 0, FM: the discriminator d[m] = Im(y[m] conj(y[m - 1])) as a real signal, w_sub the phase
 * word of 1900 Hz; det 1, USB: the row itself, its centre where 1900 Hz of audio lands), mixed by the table
 * tw[1024][2] = (cos, -sin)(2 pi k / 1024) indexed by the top ten bits of (m w_sub) mod 2^32 of the absolute output index
 * m, low-passed by g[L], L in [9, 96], and turned into lag products c[m] = u[m] conj(u[m - 1]), 0 where a power is above
 * pmax or not finite.  Sums of lag products give frequencies through a five-term arctangent polynomial: of every 10 ms
 * tick into a ring of 64, on which the VIS header is matched while the row is idle; of every pixel once a picture runs,
 * `lag` outputs behind the stream, from the anchor that hard decisions against 1350 Hz fix at the end of the first sync
 * pulse.  All float arithmetic is float32 with every operation rounded on its own, the rest is integer; DESIGN.md 3 item
 * 30 is the normative text, step by step.  Any cut of a stream into calls gives the same events and the same state; a
 * call that completes no output launches nothing and changes no state.
 * pysdr_sstv_plan needs no device: PYSDR_ERR_ARG for L outside [9, 96], nk outside [1, 2^15], max_out outside [1, 2^20],
 * nk times the event cap above 2^28 words, or a cfg outside its rules (det 0 or 1; 0 < pmax <= 1e18; R0 in [80, 480] with
 * |R0 w_tick - 2^32| <= w_tick; |5 W - R0| <= 3; lag = 2 R0 + W + 1; k_hz = fs_out / 2 pi and k_rho = 1024 / fs_out to
 * within R0's rounding; 1 to 16 modes with distinct codes in [0, 127], 1 to 4 scans, width in [1, 800], lines in
 * [1, 4096], scan_q >= width 2^16 -- a pixel of at least one sample -- and a line of at least three samples and less
 * than 2^16), else out = {rows per workgroup, threads, LDS bytes, tile samples, event cap, workgroups, history samples
 * in front of a row, words of a line buffer}.
 * create borrows ch, which must outlive the skimmer, and resets it; while a skimmer exists, feed ch only through it.  tw
 * and g are host arrays of 1024 x 2 and L floats, copied.  reset also resets the channelizer.
 * process: as pysdr_pkt_process; counts[nk] are the words of every row in this call, events[a * ev_pitch + i],
 * i < counts[a].  An event is a header word, (index within the call of the output that completed it) << 12 | kind << 10 |
 * payload words, and its payload: kind 1, start: mode index, VIS code, f_lead (float bits, Hz from the subcarrier), the
 * low 32 bits of the anchor e0; kind 2, line: the sent line's number, then the bytes of its scans in order, four to a
 * word, the first in the low bits, zero-padded; kind 3, end: the number of sent lines.
 * fetch: the last call's event words of the named rows, events[i * pitch + k] for rows[i], pitch >= the event cap.
 * state: ints [7][nk] = ticks, phase (0 idle, 1 waiting for the anchor, 2 picture), mode, m_a, e0, line, pix; floats
 * [7][nk] = the open tick's sum (re, im), the last tick's, f_lead, the open pixel's sum; ring [nk][64]; lines [nk][800],
 * the line buffers (a byte that opens a word clears the rest of it); NULL skips.
 * Calls on one handle exclude each other; an error leaves the handle usable. */
typedef struct pysdr_sstv_mode {
  int32_t code;             /* the VIS code's seven data bits */
  int32_t scans;            /* scans of a sent line */
  int32_t width;            /* pixels of a scan */
  int32_t lines;            /* sent lines */
  uint32_t sync_q, porch_q, scan_q, sep_q;   /* row samples in Q16: sync pulse, porch, one scan, the separator behind a scan */
} pysdr_sstv_mode;
typedef struct pysdr_sstv_cfg {
  int32_t det;              /* 0: FM, 1: USB */
  int32_t nmodes;
  uint32_t w_sub;           /* the subcarrier's phase per row output, in turns / 2^32 */
  uint32_t w_tick;          /* the 100 Hz tick's */
  float k_hz;               /* fs_out / 2 pi: radians per output -> Hz */
  float k_rho;              /* 1024 / fs_out: Hz -> table index */
  float pmax;               /* powers above this (or not finite) blank their lag products */
  int32_t W, R0, lag;       /* the anchor's half window, 10 ms, and the pixels' lag, in row outputs */
  pysdr_sstv_mode modes[16];
} pysdr_sstv_cfg;
typedef struct pysdr_sstv pysdr_sstv;
int  pysdr_sstv_plan(int nk, int L, int max_out, const pysdr_sstv_cfg* cfg, int32_t out[8]);
int  pysdr_sstv_create(pysdr_chan* ch, int L, const pysdr_sstv_cfg* cfg, const float* tw, const float* g, int max_out,
                       pysdr_sstv** out);
void pysdr_sstv_destroy(pysdr_sstv* sstv);
int  pysdr_sstv_reset(pysdr_sstv* sstv);
int  pysdr_sstv_sync(pysdr_sstv* sstv);
int  pysdr_sstv_process(pysdr_sstv* sstv, const void* iq, int n, int on_device, int* n_out, int32_t* counts, int32_t* events,
                        long long ev_pitch);
int  pysdr_sstv_fetch(pysdr_sstv* sstv, const int* rows, int nrows, int32_t* events, long long pitch);
int  pysdr_sstv_state(pysdr_sstv* sstv, int32_t* ints, float* floats, float* ring, uint32_t* lines);

/* ---- RDS skimmer: station names on every row of an FM broadcast raster (a build feature with a
 * definition of its own: the reference holds no RDS decoder) ------------------------------------------------------------
 * RDS / RBDS: 1187.5 bit/s, differentially encoded biphase symbols on a suppressed 57 kHz subcarrier of the FM multiplex,
 * blocks of 16 + 10 bits, groups of four blocks.  The eighth client of a channelizer (either kind; rows at any fs_out
 * from 228 to 512 kHz).  Every row a < nk is discriminated (d[m] = arg(y[m] conj(y[m - 1])) in radians, four quadrants,
 * through a five-term arctangent polynomial and one division; 0 where the product is zero or not finite), d is mixed
 * down by 57 kHz (table tw[1024][2] = (cos, -sin)(2 pi k / 1024), indexed by the top ten bits of (3 m w19) mod 2^32 of
 * the absolute output index m), and at every chip -- a sixteenth of a bit: the outputs m with (m w19) mod 2^32 < w19 --
 * the matched pulse g[L], L = 2 floor(fs_out / 1187.5) + 1, is applied once, in segments of 64 taps summed in order.  The
 * row counts its chips; chip count c belongs to timing phase c & 15, decoder dec = a * 16 + phase, whose bit is
 * Re(z[c] conj(z[c - 16])) < 0 and goes into a register of the last 104 bits.  A group is emitted whenever the register's
 * four 26-bit blocks leave the remainders of the offset words A, B, C or C', D modulo x^10 + x^8 + x^7 + x^5 + x^4 + x^3 +
 * 1: no error correction, no flywheel.  All float arithmetic is float32 with every operation rounded on its own, the
 * rest is integer; DESIGN.md 3 item 31 is the normative text, step by step.  Any cut of a stream into calls gives the
 * same events and the same state; a call that completes no output launches nothing and changes no state.
 * pysdr_rds_plan needs no device: PYSDR_ERR_ARG for L even or outside [385, 863], nk < 1, 16 nk > 2^18, max_out outside
 * [1, 2^20] or a cfg outside its rules (w19 in [159383552, 357913942], and L the length that belongs to it:
 * (L - 1) / 2 = floor((16 2^32 + 512) / w19), the 512 for w19's rounding), else out = {rows per workgroup, threads, LDS bytes, tile
 * samples, event cap, workgroups, decoders per row, segments of the matched filter}; the event cap
 * 3 ceil((floor(max_out w19 / 2^32) + 1) / 16), in words, is the most one decoder can emit in a call of max_out outputs.
 * create borrows ch, which must outlive the skimmer, and resets it; while a skimmer exists, feed ch only through it.  tw
 * and g are host arrays of 1024 x 2 and L floats, copied.  reset also resets the channelizer.
 * process: as pysdr_pkt_process; counts[16 nk] are the words of every decoder in this call, events[dec * ev_pitch + i],
 * i < counts[dec].  A group's event is three words: (index within the call of the output that completed the group) << 5
 * | phase << 1 | (1 if the third block carries offset C'), then A << 16 | B and C << 16 | D, the blocks' information words.
 * fetch: the last call's event words of the named decoders, events[i * pitch + k] for rows[i], pitch >= the event cap.
 * state: regs [4][16 nk], the registers' blocks, the oldest first; chips [nk], the chips since reset (mod 2^32); ring
 * [nk][16][2], z of the last chip of every phase; NULL skips.
 * Calls on one handle exclude each other; an error leaves the handle usable. */
typedef struct pysdr_rds_cfg {
  uint32_t w19;             /* 19 kHz per row output, in turns / 2^32: the chip grid, and a third of the subcarrier */
} pysdr_rds_cfg;
typedef struct pysdr_rds pysdr_rds;
int  pysdr_rds_plan(int nk, int L, int max_out, const pysdr_rds_cfg* cfg, int32_t out[8]);
int  pysdr_rds_create(pysdr_chan* ch, int L, const pysdr_rds_cfg* cfg, const float* tw, const float* g, int max_out,
                      pysdr_rds** out);
void pysdr_rds_destroy(pysdr_rds* rds);
int  pysdr_rds_reset(pysdr_rds* rds);
int  pysdr_rds_sync(pysdr_rds* rds);
int  pysdr_rds_process(pysdr_rds* rds, const void* iq, int n, int on_device, int* n_out, int32_t* counts, int32_t* events,
                       long long ev_pitch);
int  pysdr_rds_fetch(pysdr_rds* rds, const int* rows, int nrows, int32_t* events, long long pitch);
int  pysdr_rds_state(pysdr_rds* rds, uint32_t* regs, uint32_t* chips, float* ring);

/* ---- ACARS skimmer: aircraft messages on every row of an airband raster (a build feature with a
 * definition of its own: the reference holds no ACARS decoder) ---------------------------------------------------------
 * 2400 bit/s MSK (1200 / 2400 Hz) inside the envelope of an AM carrier, characters of seven bits with odd parity, a
 * CRC-16 behind every block.  The ninth client of a channelizer (either kind; rows at any fs_out from 19200 to 50000 Hz).
 * Every row a < nk: the envelope power p[m] = |y[m]|^2 (0 where it is not <= pmax; no square root), a complex band-pass
 * at +1800 Hz of NT = 4 L + 1 taps c (L = round(fs_out / 2400) in [8, 21]; their mean is zero, which nulls the carrier), a
 * mix-down by the table tw[1024][2] = (cos, -sin)(2 pi k / 1024) indexed by the top ten bits of (m w_car) mod 2^32 of the
 * absolute output index m, and a differential detector over one bit, x = Im(a[m] conj(a[m - L])) > 0.  One decoder per
 * row: packet's 32-bit bit clock (+ w_baud per output, pulled towards 0 by clk >> pll_shift at every change of x, a bit
 * sampled where it turns negative), the tone rule lev ^= 1 - x, a 16-bit sync register (SYN SYN, or its inverse, which
 * flips lev), SOH, the text with odd parity on every byte, ETX or ETB and the two bytes of the block check.  All float
 * arithmetic is float32 with every operation rounded on its own, the rest is integer; DESIGN.md 3 item 32 is the normative
 * text, step by step.  Any cut of a stream into calls gives the same events and the same state; a call that completes no
 * output launches nothing and changes no state.
 * pysdr_acars_plan needs no device: PYSDR_ERR_ARG for L outside [8, 21], nk outside [1, 2^15], max_out outside [1, 2^20]
 * or a cfg outside its rules (0 < pmax <= 1e18, finite; both words > 0 and w_baud <= 2^29; pll_shift in [1, 4]), else
 * out = {rows per workgroup, threads, LDS bytes, tile samples, event cap, workgroups, taps, words of a frame buffer}; the
 * event cap 61 + (ceil(max_out / (2^31 / w_baud + 1)) - 1) / 24, in words, is the most one decoder can emit in a call of
 * max_out outputs.
 * create borrows ch, which must outlive the skimmer, and resets it; while a skimmer exists, feed ch only through it.  tw
 * and c are host arrays of 1024 x 2 and (4 L + 1) x 2 floats, copied.  reset also resets the channelizer.
 * process: as pysdr_pkt_process; counts[nk] are the words of every row in this call, events[a * ev_pitch + i],
 * i < counts[a].  A frame's event is a header word, (index within the call of the output that completed the block
 * check) << 10 | n, and then (n + 3) / 4 words with the frame's n bytes, mode character to ETX / ETB, parity bits
 * included, the first byte in the low bits, zero-padded; only frames of 13 <= n <= 238 bytes whose every byte has odd
 * parity and whose block check is good are events.
 * fetch: the last call's event words of the named rows, events[i * pitch + k] for rows[i], pitch >= the event cap.
 * state: ints [9][nk] = clk, xprev, lev, sr, st, byte, nb, nbytes, crc and frames [nk][60], the frame buffers (bytes four
 * to a word; a byte that opens a word clears the rest of it); NULL skips.
 * Calls on one handle exclude each other; an error leaves the handle usable. */
typedef struct pysdr_acars_cfg {
  float pmax;               /* envelope powers above this (or not finite) are blanked */
  uint32_t w_car;           /* 1800 Hz: the mixer's phase per row output, in turns / 2^32 */
  uint32_t w_baud;          /* the bit clock's */
  int32_t pll_shift;        /* the clock's pull at a change of the detector: clk -= clk >> pll_shift */
} pysdr_acars_cfg;
typedef struct pysdr_acars pysdr_acars;
int  pysdr_acars_plan(int nk, int L, int max_out, const pysdr_acars_cfg* cfg, int32_t out[8]);
int  pysdr_acars_create(pysdr_chan* ch, int L, const pysdr_acars_cfg* cfg, const float* tw, const float* c, int max_out,
                        pysdr_acars** out);
void pysdr_acars_destroy(pysdr_acars* acars);
int  pysdr_acars_reset(pysdr_acars* acars);
int  pysdr_acars_sync(pysdr_acars* acars);
int  pysdr_acars_process(pysdr_acars* acars, const void* iq, int n, int on_device, int* n_out, int32_t* counts,
                         int32_t* events, long long ev_pitch);
int  pysdr_acars_fetch(pysdr_acars* acars, const int* rows, int nrows, int32_t* events, long long pitch);
int  pysdr_acars_state(pysdr_acars* acars, int32_t* ints, uint32_t* frames);

/* ---- FT8 skimmer: Costas sync and soft bits on a fine raster of the band --------------------
 * The fourth client of a channelizer (either kind, M / D = 4, rows at S = 64 or 96 samples per symbol of 6.25 baud).
 * Inside every row NSUB = S / 2 decoders, one every baud / 2, over NB = NSUB + 14 bins baud / 2 apart whose powers are
 * taken four times per symbol (a step: QS = S / 4 row outputs) into a device ring [nk][TR][NB].  Fine row F = a NSUB + j.
 * Step t is complete with row output QS t + S - 1.  An event is a frame start t0 whose Costas score is a peak over four
 * steps to either side, at least smin, with at least hmin of the 21 sync symbols strongest on their own tone; it is
 * emitted at step t0 + 316.  Every float operation is float32 and rounded on its own; any cut of a stream into calls
 * gives the same events, state bits and soft bits; a call that completes no output launches nothing and changes no
 * state; one that completes outputs but no step only rolls the rows' history.
 * pysdr_ft8_plan needs no device: PYSDR_ERR_ARG for S not 64 or 96, nk < 1, nk S / 2 > 2^18, max_out outside [1, 2^20], a
 * ring above 2^30 bytes or a cfg outside its rules (smin >= 0, hmin in [0, 21], pmax in (0, 1e18], all finite), else out =
 * {rows per workgroup, threads, LDS bytes, tile samples, event cap, workgroups, NSUB, TR}; cap = (max_out / QS + 1) / 5 + 1
 * (two events of a decoder are at least 5 steps apart), TR = 321 + 2 (max_out / QS + 1) steps.
 * create: tw [4 S][2] = (cos, -sin)(2 pi i / (4 S)).  The skimmer borrows ch, resets it, and ch must be fed only through it.
 * process: as pysdr_fsk_process.  An event is two int32 words: (index within the call of the step at which it was
 * emitted) << 5 | hits, then the score's float32 bits; t0 = steps[0] + index - 316.  events[F * ev_pitch + 2 i], i <
 * counts[F]; ev_pitch counts words and is at least 2 cap.  steps (NULL or [2]) receives the steps complete before the
 * call and the steps the call completed.  Refusals as pysdr_fsk_process (PYSDR_ERR_STATE: n > max_in, more than max_out
 * outputs, ev_pitch too small; the stream does not advance).
 * fetch: the last call's event words of the named fine rows, events[i * pitch + w], pitch >= 2 cap.
 * llr: the 174 soft bits, in transmission order, of n <= 4096 candidates (F[i], t0[i]) to out[i * 174 + b]: for data
 * symbol d (frame symbol 7 + d, or 43 + (d - 29) from d = 29 on) and the powers p[v] of its eight values v (sent on tone
 * GRAY[v]), bit 4, 2, 1 of v in that order gives max over the values with the bit minus max over those without.  Before
 * any launch and changing nothing it refuses every call in which some F is outside [0, nk NSUB) (PYSDR_ERR_ARG) or some
 * frame is not yet complete (t0 + 312 >= steps done) or has left the ring (steps done - t0 > TR, or t0 < 0):
 * PYSDR_ERR_STATE.  A frame is in the ring for at least one whole call of max_out outputs behind the call that emitted it.
 * state: sc [9][nk NSUB] and hits [9][nk NSUB], the score and hit count of frame start t at index t mod 9; ring
 * [nk][TR][NB], step t at index t mod TR; t_done, the steps complete.  NULL skips. */
typedef struct pysdr_ft8_cfg {
  float smin;               /* least score of an event */
  int32_t hmin;             /* least hit count of an event, of 21 */
  float pmax;               /* bin powers above this (or not finite) are blanked */
} pysdr_ft8_cfg;
typedef struct pysdr_ft8 pysdr_ft8;
int  pysdr_ft8_plan(int nk, int S, int max_out, const pysdr_ft8_cfg* cfg, int32_t out[8]);
int  pysdr_ft8_create(pysdr_chan* ch, int S, const pysdr_ft8_cfg* cfg, const float* tw, int max_out, pysdr_ft8** out);
void pysdr_ft8_destroy(pysdr_ft8* ft8);
int  pysdr_ft8_reset(pysdr_ft8* ft8);
int  pysdr_ft8_sync(pysdr_ft8* ft8);
int  pysdr_ft8_process(pysdr_ft8* ft8, const void* iq, int n, int on_device, int* n_out, int32_t* counts, int32_t* events,
                       long long ev_pitch, long long* steps);
int  pysdr_ft8_fetch(pysdr_ft8* ft8, const int* rows, int nrows, int32_t* events, long long pitch);
int  pysdr_ft8_llr(pysdr_ft8* ft8, const int32_t* F, const long long* t0, int n, float* out);
int  pysdr_ft8_state(pysdr_ft8* ft8, float* sc, int32_t* hits, float* ring, long long* t_done);

/* ---- FT4 skimmer: four Costas arrays and soft bits on a fine raster of the band --------------
 * The fifth client of a channelizer (either kind, M / D = 4, rows at S = 48 or 72 samples per symbol of 125 / 6 baud).
 * Inside every row NSUB = S / 2 decoders, one every baud / 2, over NB = NSUB + 6 bins baud / 2 apart whose powers are
 * taken four times per symbol (a step: QS = S / 4 row outputs) into a device ring [nk][TR][NB].  Fine row F = a NSUB + j.
 * A frame is 103 symbols of 4 tones with four different 4-symbol Costas arrays at symbols 0, 33, 66 and 99.  An event is
 * a frame start t0 whose Costas score is a peak over four steps to either side, at least smin, with at least hmin of the
 * 16 sync symbols strongest on their own tone; it is emitted at step t0 + 412.  Steps, calls, event words, fetch, state
 * and every refusal are pysdr_ft8_*'s with these numbers: S 48 or 72, nk S / 2 <= 2^18, hmin in [0, 16], t0 = steps[0] +
 * index - 412, cap = (max_out / QS + 1) / 5 + 1, TR = 417 + 2 (max_out / QS + 1) steps.
 * llr: the 174 soft bits, in transmission order, of n <= 4096 candidates: for data symbol d (frame symbol 4 + d, 37 +
 * (d - 29) from d = 29 on, 70 + (d - 58) from d = 58 on) and the powers p[v] of its four values v (sent on tone GRAY4[v],
 * GRAY4 = [0,1,3,2]), bit 2, 1 of v in that order gives max over the values with the bit minus max over those without.
 * A frame is not yet complete while t0 + 408 >= steps done. */
typedef struct pysdr_ft4_cfg {
  float smin;               /* least score of an event */
  int32_t hmin;             /* least hit count of an event, of 16 */
  float pmax;               /* bin powers above this (or not finite) are blanked */
} pysdr_ft4_cfg;
typedef struct pysdr_ft4 pysdr_ft4;
int  pysdr_ft4_plan(int nk, int S, int max_out, const pysdr_ft4_cfg* cfg, int32_t out[8]);
int  pysdr_ft4_create(pysdr_chan* ch, int S, const pysdr_ft4_cfg* cfg, const float* tw, int max_out, pysdr_ft4** out);
void pysdr_ft4_destroy(pysdr_ft4* ft4);
int  pysdr_ft4_reset(pysdr_ft4* ft4);
int  pysdr_ft4_sync(pysdr_ft4* ft4);
int  pysdr_ft4_process(pysdr_ft4* ft4, const void* iq, int n, int on_device, int* n_out, int32_t* counts, int32_t* events,
                       long long ev_pitch, long long* steps);
int  pysdr_ft4_fetch(pysdr_ft4* ft4, const int* rows, int nrows, int32_t* events, long long pitch);
int  pysdr_ft4_llr(pysdr_ft4* ft4, const int32_t* F, const long long* t0, int n, float* out);
int  pysdr_ft4_state(pysdr_ft4* ft4, float* sc, int32_t* hits, float* ring, long long* t_done);

/* ---- LDPC(174,91), CRC-14: the back half of the FT8 and FT4 skimmers ---------------------------
 * Normalised min-sum on a flooding schedule over the 83 sparse checks (degree 6 or 7, every column in 3), one workgroup
 * of 192 threads per candidate, float32 with every operation rounded on its own.  Soft bits are positive for bit 1 and
 * need no scaling: the decoder works on L = -llr, messages c start at +0, and for k = 0, 1, ..: tot[n] = ((L[n] + c[e0]) +
 * c[e1]) + c[e2] over the column's edges in ascending check order; hard[n] = tot[n] < 0; every check even: stop, a
 * codeword after `iterations` = k; k == iters: stop, no codeword; else v[e] = L[n] + the two other messages into n in
 * ascending check order and c[e] = s * (alpha * min |v| over the check's other edges), s the product of the other edges'
 * signs (v < 0 is negative, +0 and -0 positive) applied by negation (a zero minimum under a negative sign is -0).
 * Per candidate: status[4] = {status, iterations, nerr, 0} -- status 2: a codeword whose 14 CRC bits match (polynomial
 * 0x2757 over the 77 message bits and five zeros, zero start, no reflection, no final XOR) and whose message is not all
 * zero; 1: any other codeword; 0: none; nerr: positions where llr > 0 differs from the final hard bit -- bits[12]: the
 * first 91 final hard bits, MSB first, 5 zero bits of padding, filled for every status; post (or NULL) [174]: the final tot.
 * pysdr_ldpc_plan needs no device: PYSDR_ERR_ARG for a NULL cfg, iters outside [1, 200] or alpha not in (0, 1] (a NaN
 * is not), else out = {threads per candidate, LDS bytes, candidates per call (4096), iters}.
 * pysdr_ft8_decode / pysdr_ft4_decode: the candidates (F[i], t0[i]) of pysdr_ft8_llr / pysdr_ft4_llr, under its rules
 * and refusals, decoded from the spectrum ring: the soft bits never reach memory.  status [n][4], bits [n][12], post
 * [n][174] or NULL are host arrays.  A bad candidate, n outside [0, 4096], a bad cfg or a NULL array: nothing is launched,
 * no output changes.
 * pysdr_ft8_decode_llr / pysdr_ft4_decode_llr: host soft bits llr [n][174]; a value that is not finite is refused
 * (PYSDR_ERR_ARG) before any launch.  Runs on the skimmer's stream through its soft-bit buffer. */
typedef struct pysdr_ldpc_cfg {
  int32_t iters;            /* most iterations, [1, 200] */
  float alpha;              /* the normalisation, (0, 1] */
} pysdr_ldpc_cfg;
int  pysdr_ldpc_plan(const pysdr_ldpc_cfg* cfg, int32_t out[4]);
int  pysdr_ft8_decode(pysdr_ft8* ft8, const int32_t* F, const long long* t0, int n, const pysdr_ldpc_cfg* cfg, int32_t* status,
                      uint8_t* bits, float* post);
int  pysdr_ft8_decode_llr(pysdr_ft8* ft8, const float* llr, int n, const pysdr_ldpc_cfg* cfg, int32_t* status, uint8_t* bits,
                          float* post);
int  pysdr_ft4_decode(pysdr_ft4* ft4, const int32_t* F, const long long* t0, int n, const pysdr_ldpc_cfg* cfg, int32_t* status,
                      uint8_t* bits, float* post);
int  pysdr_ft4_decode_llr(pysdr_ft4* ft4, const float* llr, int n, const pysdr_ldpc_cfg* cfg, int32_t* status, uint8_t* bits,
                          float* post);

/* ---- Ordered-statistics decoding behind min-sum -------------------------------------------------
 * A second stage for the candidates min-sum left without a message (status != 2), on the same channel soft bits x:
 * r = |x|, h = x > 0; the positions ranked by descending r, ties by ascending position; the most reliable basis (the
 * first 91 ranks whose generator columns are independent, `last` the 91st); G', the generator whose columns at those
 * ranks are the identity; e0 = (the re-encoding of h on the basis) xor h; the patterns k = 0: e0; 1 + i: e0 xor G'[i];
 * 92 + the place of (i, j), i < j, in lexicographic order: e0 xor G'[i] xor G'[j] -- 1, 92 or 4187 of them for order 0,
 * 1, 2; a pattern's distance is the float32 sum, in rank order, of r where its bit is set; the least (distance, k) wins.
 * If the winner's word h xor pattern has a matching CRC-14 and a message that is not all zero, the candidate becomes
 * status 2 with the word's first 91 bits and nerr = the pattern's weight; iterations and post stay min-sum's.  THE CRC IS
 * THE ONLY GUARD: a candidate that reaches this stage comes out as a false message with probability about 2^-14.
 * status[3] is 0 where the stage did not run, else 1, 2, 3 for a winner k = 0, k in 1..91, k >= 92, accepted or not.
 * detail (or NULL) [n][4]: {k, last, the pattern's weight, the bits of the float32 distance}, or {-1, -1, -1, 0} where
 * the stage did not run.  One wavefront per candidate, launched behind min-sum on the skimmer's stream.
 * pysdr_osd_plan needs no device: PYSDR_ERR_ARG for a NULL cfg or out or an order outside [0, 2], else out = {threads
 * per candidate, LDS bytes, patterns, candidates per call}.  The four calls are pysdr_*_decode / pysdr_*_decode_llr with
 * their rules and refusals, plus PYSDR_ERR_ARG for a NULL or bad osd cfg; a refusal launches nothing and changes no
 * output. */
typedef struct pysdr_osd_cfg {
  int32_t order;            /* rows of G' flipped at once, [0, 2] */
} pysdr_osd_cfg;
int  pysdr_osd_plan(const pysdr_osd_cfg* cfg, int32_t out[4]);
int  pysdr_ft8_decode_osd(pysdr_ft8* ft8, const int32_t* F, const long long* t0, int n, const pysdr_ldpc_cfg* cfg, int32_t* status,
                          uint8_t* bits, float* post, const pysdr_osd_cfg* osd, int32_t* detail);
int  pysdr_ft8_decode_llr_osd(pysdr_ft8* ft8, const float* llr, int n, const pysdr_ldpc_cfg* cfg, int32_t* status, uint8_t* bits,
                              float* post, const pysdr_osd_cfg* osd, int32_t* detail);
int  pysdr_ft4_decode_osd(pysdr_ft4* ft4, const int32_t* F, const long long* t0, int n, const pysdr_ldpc_cfg* cfg, int32_t* status,
                          uint8_t* bits, float* post, const pysdr_osd_cfg* osd, int32_t* detail);
int  pysdr_ft4_decode_llr_osd(pysdr_ft4* ft4, const float* llr, int n, const pysdr_ldpc_cfg* cfg, int32_t* status, uint8_t* bits,
                              float* post, const pysdr_osd_cfg* osd, int32_t* detail);

/* ---- A-priori decoding -----------------------------------------------------------------------------
 * The decoder of item 24 told some message bits in advance, once per hypothesis.  A hypothesis is two words of 12 bytes,
 * mask then value, packed as `bits`: message bit i is bit 7 - (i & 7) of byte i >> 3; only bits 0 .. 76 may be set in the
 * mask, the mask is not empty, and value & ~mask == 0.  A call names n candidates (as pysdr_*_decode or pysdr_*_decode_llr
 * takes them), a table hyps [H][24] and pairs [P][2] = (candidate, hypothesis): n in [0, 4096], H in [1, 4096], P in
 * [0, 65536], the pairs strictly increasing in (candidate, hypothesis), candidate in [0, n), hypothesis in [0, H); a
 * candidate may have no pair.  Per pair: amax = the greatest |llr| of the candidate's 174 soft bits, A = f32(mag amax),
 * every soft bit k under the mask becomes +A (hypothesised 1) or -A (0), and item 24's decoder runs on that word
 * unchanged (iters and alpha of cfg).  nerr counts the positions OUTSIDE the mask where llr > 0 differs from the final
 * hard bit, nap the positions inside it where the final hard bit differs from the value.  The pair's status is 2 for a
 * codeword with a matching CRC-14, a message that is not all zero, nap == 0 and nerr <= nerr_max; 1 for any other
 * codeword; 0 for none.  Per candidate: among its pairs of status 2 the least nerr, ties to the lower pair index;
 * ap [n][4] = {that pair or -1, its iterations, its nerr, the candidate's pairs of status 2} (zeros behind a -1),
 * bits [n][12] = the picked pair's 91 bits, zero where there is none; detail (or NULL) [P][4] = {status, iterations,
 * nerr, nap} of every pair.  One workgroup of 192 threads per pair, then one thread per candidate, on the skimmer's
 * stream.  Candidates come from the first spectrum ring only, and no second stage runs behind these calls.
 * pysdr_ap_plan needs no device: PYSDR_ERR_ARG for a NULL cfg or out, a mag that is not in [0.25, 16] (a NaN is not) or
 * a nerr_max outside [0, 174], else out = {threads per pair, LDS bytes, pairs per call, hypotheses per call}.
 * The four calls refuse what pysdr_*_decode / pysdr_*_decode_llr refuse, and a bad ap cfg, table or pair list
 * (PYSDR_ERR_ARG); every check comes before any launch, and a refusal launches nothing and changes no output. */
typedef struct pysdr_ap_cfg {
  float mag;                /* the clamp, in units of the word's greatest |llr|, [0.25, 16] */
  int32_t nerr_max;         /* most hard errors outside the mask of an accepted pair, [0, 174] */
} pysdr_ap_cfg;
int  pysdr_ap_plan(const pysdr_ap_cfg* cfg, int32_t out[4]);
int  pysdr_ft8_decode_ap(pysdr_ft8* ft8, const int32_t* F, const long long* t0, int n, const uint8_t* hyps, int H, const int32_t* pairs,
                         int P, const pysdr_ldpc_cfg* cfg, const pysdr_ap_cfg* apcfg, int32_t* ap, uint8_t* bits, int32_t* detail);
int  pysdr_ft8_decode_llr_ap(pysdr_ft8* ft8, const float* llr, int n, const uint8_t* hyps, int H, const int32_t* pairs, int P,
                             const pysdr_ldpc_cfg* cfg, const pysdr_ap_cfg* apcfg, int32_t* ap, uint8_t* bits, int32_t* detail);
int  pysdr_ft4_decode_ap(pysdr_ft4* ft4, const int32_t* F, const long long* t0, int n, const uint8_t* hyps, int H, const int32_t* pairs,
                         int P, const pysdr_ldpc_cfg* cfg, const pysdr_ap_cfg* apcfg, int32_t* ap, uint8_t* bits, int32_t* detail);
int  pysdr_ft4_decode_llr_ap(pysdr_ft4* ft4, const float* llr, int n, const uint8_t* hyps, int H, const int32_t* pairs, int P,
                             const pysdr_ldpc_cfg* cfg, const pysdr_ap_cfg* apcfg, int32_t* ap, uint8_t* bits, int32_t* detail);

/* ---- Frame report and row floor ------------------------------------------------------------------
 * What the spectrum ring says about a frame whose 91 bits are known.  float32, every operation rounded on its own.
 * pysdr_ft8_report / pysdr_ft4_report: n <= 4096 candidates (F[i], t0[i]) under pysdr_*_llr's rules and refusals, and
 * bits [n][12], the 91 bits MSB first as pysdr_*_decode packs them (the CRC is not checked).  Per candidate the bits are
 * encoded again to the 174-bit codeword, the codeword gives the frame's tones tone[k], k < 79 (FT4: 103) -- the Costas
 * arrays in their places, the data symbols' bits MSB first through the Gray map -- and
 *   power[0 .. 8] = sig9[dt][dF], dt in -1, 0, 1 outer, dF in -1, 0, 1 inner: the sum over k ascending, from the first
 *     term, of P[a'][t0 + dt + 4 k][j' + 2 tone[k]], (a', j') = divmod(F + dF, NSUB); F + dF wraps modulo the raster where
 *     the raster is the whole circle (nk == M).  A place is missing -- exactly -1 -- where its fine row is outside the
 *     raster, or where the frame from t0 + dt is not whole yet, begins before step 0 or has left the ring;
 *   power[9] = tot: the sum over k ascending of (the symbol's 8 (4) tones at the candidate's own place, added ascending);
 *   errs[0] = nhard, errs[1] = nsync: the data and the Costas symbols whose sent tone is not strictly greater than
 *     every other tone of the symbol at the candidate's own place.
 * pysdr_ft8_floor / pysdr_ft4_floor: out [nk][NB], out[a][b] = the sum over i < nsym ascending, from the first term, of
 * P[a][t_end - 4 (nsym - 1 - i)][b].  PYSDR_ERR_ARG unless 1 <= nsym <= 128; PYSDR_ERR_STATE unless every one of those
 * steps is complete and still in the ring.
 * A refused call launches nothing and changes no output.  pysdr_report_plan needs no device: PYSDR_ERR_ARG for a mode
 * that is neither or a NULL out, else out = {threads per candidate, LDS bytes, symbols, candidates per call}. */
#define PYSDR_REPORT_FT8 0
#define PYSDR_REPORT_FT4 1
int  pysdr_report_plan(int mode, int32_t out[4]);
int  pysdr_ft8_report(pysdr_ft8* ft8, const int32_t* F, const long long* t0, const uint8_t* bits, int n, float* power, int32_t* errs);
int  pysdr_ft4_report(pysdr_ft4* ft4, const int32_t* F, const long long* t0, const uint8_t* bits, int n, float* power, int32_t* errs);
int  pysdr_ft8_floor(pysdr_ft8* ft8, long long t_end, int nsym, float* out);
int  pysdr_ft4_floor(pysdr_ft4* ft4, long long t_end, int nsym, float* out);

/* ---- Second pass: subtract decoded frames, search the residue ---------------------------------------
 * Off unless pysdr_ft8_keep / pysdr_ft4_keep is called, which is allowed only before the stream begins (after create or
 * reset; PYSDR_ERR_STATE later).  From then on every process call also copies its outputs into a sample ring yk [nk][TY]
 * (row sample n at n mod TY) and its new steps into a residue ring ring2 [nk][TR2][NB] (step t at t mod TR2), which is
 * bit for bit the spectrum ring until a subtraction touches it; reset clears both.  The first pass never reads either.
 * TR2 = hold + 2 reach_t + 4 + max_out / QS + 1 steps, TY = QS TR2 + S rounded up to 16; each ring is at most 2^30 bytes.
 * cfg: reach_t in [1, 120], trials in [1, 9], pulse [P S] uint32 (P = 3, FT4: 5: the cumulative phase of one symbol of
 * tone 1 over the P symbols its frequency pulse spans, 2^32 a turn, the last entry 2^32 = 0), lut [4096][2] = (cos, sin)
 * (2 pi i / 4096); both tables derived by the caller in float64 and rounded once.
 * pysdr_*_subtract: n <= 256 frames (F[i], t0[i]) with bits [n][12] as pysdr_*_report takes them and trials
 * [n][cfg.trials][2] = (dn, fw): dn, |dn| < QS, the row samples the frame starts away from QS t0, fw the 32-bit phase word
 * per row sample of tone 0's offset from fine row F.  Every row that holds tones of the frame is a job -- the frame's own
 * and at most one neighbour; the jobs of a row run in the order given.  A job builds the unit reference r[n] =
 * lut[(phase + 2^19) >> 20], phase = n (w + fw) + sum of tone[k'] pulse[..] over the symbols whose pulse covers the sample
 * (w: tone 0's word in that row, round(q 2^32 / (4 S))), takes a_k = (1 / S) sum y[n] conj(r[n]) per symbol k (n ascending)
 * for every trial, picks the trial of greatest sum |a_k|^2 (k ascending; the lower index on a tie) and sets y[n] -= a_k r[n]
 * in yk.  A symbol with a sample before the stream's start is left alone.  out [n][2][4] per (frame, row job): the bits of
 * the float32 power of the symbols used before and after, the trial chosen, the symbols used (zeros where a frame has
 * one job).  Then the steps t0 - 4 .. t0 + lag + 4 of ring2 are recomputed from yk for every job's row, with the streaming
 * kernel's arithmetic.  PYSDR_ERR_STATE unless those steps are all complete and held.
 * pysdr_*_rescan: the fine rows F_lo .. F_hi (at most 256) of ring2 scored at the start steps t_lo - 4 .. t_hi + 4 (at most
 * 256) and judged by the streaming kernel's peak rule at t_lo .. t_hi under cfg; counts [nF], events [nF][52][2], the
 * existing two words with the step counted from t_lo.  PYSDR_ERR_STATE unless every such frame is whole and held.
 * pysdr_*_pass_decode: pysdr_*_decode_osd on ring2 (osd may be NULL: min-sum alone; detail then must be NULL).
 * pysdr_*_pass_llr: pysdr_*_llr on ring2.
 * pysdr_*_pass_state: yk [nk][TY][2] and ring2 (either may be NULL); kept = {row samples so far, TY, TR2}.
 * Every call checks all of its arguments before any launch, and a refusal changes nothing; PYSDR_ERR_STATE without keep.
 * pysdr_pass_plan needs no device: mode PYSDR_REPORT_FT8 / FT4 -> out = {threads, LDS bytes, TY, TR2, jobs per call,
 * frames per call, events per fine row of a rescan, P}. */
typedef struct pysdr_pass_cfg {
  int32_t reach_t;
  int32_t trials;
  const uint32_t* pulse;
  const float* lut;
} pysdr_pass_cfg;
int  pysdr_pass_plan(int mode, int nk, int S, int max_out, int reach_t, int32_t out[8]);
int  pysdr_ft8_keep(pysdr_ft8* ft8, const pysdr_pass_cfg* cfg);
int  pysdr_ft4_keep(pysdr_ft4* ft4, const pysdr_pass_cfg* cfg);
int  pysdr_ft8_subtract(pysdr_ft8* ft8, const int32_t* F, const long long* t0, const uint8_t* bits, const int32_t* trials, int n,
                        int32_t* out);
int  pysdr_ft4_subtract(pysdr_ft4* ft4, const int32_t* F, const long long* t0, const uint8_t* bits, const int32_t* trials, int n,
                        int32_t* out);
int  pysdr_ft8_rescan(pysdr_ft8* ft8, int F_lo, int F_hi, long long t_lo, long long t_hi, const pysdr_ft8_cfg* cfg, int32_t* counts,
                      int32_t* events);
int  pysdr_ft4_rescan(pysdr_ft4* ft4, int F_lo, int F_hi, long long t_lo, long long t_hi, const pysdr_ft4_cfg* cfg, int32_t* counts,
                      int32_t* events);
int  pysdr_ft8_pass_decode(pysdr_ft8* ft8, const int32_t* F, const long long* t0, int n, const pysdr_ldpc_cfg* cfg, int32_t* status,
                           uint8_t* bits, float* post, const pysdr_osd_cfg* osd, int32_t* detail);
int  pysdr_ft4_pass_decode(pysdr_ft4* ft4, const int32_t* F, const long long* t0, int n, const pysdr_ldpc_cfg* cfg, int32_t* status,
                           uint8_t* bits, float* post, const pysdr_osd_cfg* osd, int32_t* detail);
int  pysdr_ft8_pass_llr(pysdr_ft8* ft8, const int32_t* F, const long long* t0, int n, float* out);
int  pysdr_ft4_pass_llr(pysdr_ft4* ft4, const int32_t* F, const long long* t0, int n, float* out);
int  pysdr_ft8_pass_state(pysdr_ft8* ft8, float* yk, float* ring2, long long* kept);
int  pysdr_ft4_pass_state(pysdr_ft4* ft4, float* yk, float* ring2, long long* kept);

/* ---- device memory for resident streams --------------------------------------- */
int pysdr_dev_alloc(int device, size_t bytes, void** out);
int pysdr_dev_free(int device, void* p);
int pysdr_dev_upload(int device, void* dst, const void* src_host, size_t bytes);
int pysdr_dev_download(int device, void* dst_host, const void* src, size_t bytes);
int pysdr_dev_copy(int device, void* dst, const void* src, size_t bytes);

/* ---- multi-GPU: RCCL broadcast of the wideband chunk when ONE stream's
 * sub-receivers are split across GPUs (the analogue of MP_SCHEME 3's
 * que[irx].put(x), receiver.py:728-739).  id = 128-byte ncclUniqueId. */
int pysdr_comm_unique_id(char id_out[128]);
int pysdr_comm_init(pysdr_ctx* ctx, const char id[128], int rank, int nranks);
int pysdr_comm_bcast(pysdr_ctx* ctx, void* d_buf, size_t bytes, int root);
int pysdr_comm_destroy(pysdr_ctx* ctx);

/* ---- ingest ring (receiver.py:579-631, soapy.py:33-48) ------------------
 * The step in front of pysdr_process for a live device: `nslots` pinned host chunk buffers
 * that sdr.readStream() fills directly, an asynchronous H2D copy on its own stream, the
 * chunk's kernels behind it and an asynchronous D2H of every sub-receiver's result into pinned
 * per-slot buffers.  submit() returns at once, so the host assembles chunk k+1 (short reads,
 * xold carry) while chunk k is copied and demodulated; collect() waits for one slot and hands
 * out pointers into its result buffers (valid until the slot is submitted again).  Destroy the
 * ring before the context it was created on. */
typedef struct pysdr_ingest pysdr_ingest;
int  pysdr_ingest_create(pysdr_ctx* ctx, int nslots, pysdr_ingest** out);
/* Slots of `chunks_per_slot` chunks (<= cfg.max_chunks): one DMA, one launch sequence and one set of
 * result copies per slot instead of per chunk -- the per-chunk fixed costs (about ten kernel
 * launches, 2 NUM_RX + 1 copies) are what bounds the one-chunk ring at 1.6 GS/s.  A slot submitted
 * with a whole number of IN_CHUNK_SIZE chunks is processed exactly as that many pysdr_process
 * calls; pysdr_ingest_chunks tells the per-chunk output counts and raw peaks (rx.auto_mute input)
 * so that the caller can cut the slot's audio back into chunks (receiver.py:238-252). */
int  pysdr_ingest_create_batched(pysdr_ctx* ctx, int nslots, int chunks_per_slot, pysdr_ingest** out);
int  pysdr_ingest_chunks(pysdr_ingest* ing, int slot, int cap, int* nchunks, int* chunk_nout, float* peaks);
void pysdr_ingest_destroy(pysdr_ingest* ing);
int  pysdr_ingest_buffer(pysdr_ingest* ing, int slot, float** iq, size_t* cap_samples);
int  pysdr_ingest_submit(pysdr_ingest* ing, int slot, size_t n);
int  pysdr_ingest_collect(pysdr_ingest* ing, int slot, pysdr_out* outs);

#ifdef __cplusplus
}
#endif
#endif /* PYSDR_HIP_H */
