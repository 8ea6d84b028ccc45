// C ABI of the four stream objects of libpysdr_hip.so (include/pysdr_hip.h): waterfall, RTTY decoder bank, polyphase
// channelizer and channel bank.  Host-side only, like api.hip: the kernels and their launch functions live in
// waterfall.hip / rtty.hip / chan.hip / bank.hip, what both sides share in objects_plan.h.  Every device resource is an
// owner (host_res.h): deleting an object frees it.  In each struct the stream is declared in front of the buffers, so it
// is destroyed after them; the destroy functions drain it first.
#include <cmath>

#include "chan_client.h"      // what the bank shares with the channelizer's other clients
#include "chan_object.h"      // struct pysdr_chan: the channelizer's own entry points and chan_info, nothing of the bank's

using namespace pysdr;

struct pysdr_waterfall {
  int device = 0, nfft = 0, ncols = 0;
  int head = 0;        // slot that receives the next line (= oldest column)
  int cnt = 0;         // valid columns (wf_cnt, Plotting.py:545-546)
  int shift = 0;       // accumulated retune roll: logical bin i lives at (i + shift) mod nfft
  Stream stream;
  DevBuf<float> d_wf;     // [ncols][nfft]
  DevBuf<float> d_image;  // [ncols][nfft]
  DevBuf<float> d_line;   // staging for host lines
  DevBuf<float> d_mean;   // [nfft]
  DevBuf<float> d_stat;   // [0] bkgnd, [1] max(wf)
  DevBuf<int> d_pk;       // peak pick scratch: [3][nfft / 2 + 2] positions, states, kept indices; + [1] the count
};

struct pysdr_rtty {
  int device = 0, nfft = 0, nsh = 0, bin_lo = 0, bin_hi = 0, find_lo = 0, find_hi = 0, max_lines = 0;
  int nb = 0;              // decoders = bin_hi - bin_lo
  int band_lo = 0, nband = 0;
  int R = 0;               // ring rows; line n >= 1 lives in row n % R
  int max_dec = 0;         // decisions one call can complete
  long long n = 0;         // lines decoded so far
  Stream stream;
  DevBuf<float> d_lines;       // staging for host lines [max_lines][nfft]
  DevBuf<float> d_band;        // ring [R][nband]
  DevBuf<float> d_s4, d_best, d_sc2;   // rings [R][nb]
  DevBuf<int> d_isym;          // ring [R][nb]
  DevBuf<int> d_shift;         // [nb]
  DevBuf<long long> d_t;       // [max_dec][nb]
  DevBuf<double> d_snr;        // [max_dec][nb]
  DevBuf<int> d_held, d_code;  // [max_dec][nb]
  DevBuf<int> d_ndet;          // [max_lines]
};

struct pysdr_bank : ChanClient {
  BankPlan plan;
  int mode = PYSDR_NFM, T = 0;
  bool have_taps = false;
  int agc_enable = 1;
  float ref = kAgcRefDefault, thresh = 0.f, fm_scale = 0.f;
  double fs_out = 0.0;
  uint32_t fword = 0;               // CW: the BFO's phase increment per output
  long long ypitch = 0, apitch = 0;
  DevBuf<float2> d_y;               // [nk][hpad + out_cap]
  DevBuf<float> d_a;                // [nk][out_cap]
  DevBuf<float> d_taps;             // [2 tp]: real taps in the first half; USB / LSB / CW: re, then -im
  DevBuf<float> d_pmax;             // [nk][tiles]
  DevBuf<double> d_psum;            // [nk][tiles]
  DevBuf<BankState> d_state;
  std::vector<float> h_taps;
  std::vector<BankState> h_state;
};

namespace {

constexpr double kNfmFullScaleDev = 5000.0;

int waterfall_alloc(pysdr_waterfall* w) {
  const size_t n = (size_t)w->nfft * w->ncols;
  PYSDR_HIP_CHECK(w->stream.create(hipStreamNonBlocking));
  PYSDR_HIP_CHECK(w->d_wf.alloc(n));
  PYSDR_HIP_CHECK(w->d_image.alloc(n));
  PYSDR_HIP_CHECK(w->d_line.alloc((size_t)w->nfft));
  PYSDR_HIP_CHECK(w->d_mean.alloc((size_t)w->nfft));
  PYSDR_HIP_CHECK(w->d_stat.alloc(4));
  PYSDR_HIP_CHECK(w->d_pk.alloc(3 * ((size_t)w->nfft / 2 + 2) + 1));
  const int rc = launch_wf_fill(w->d_wf.get(), n, kFill, w->stream);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipStreamSynchronize(w->stream));
  return PYSDR_OK;
}

int rtty_alloc(pysdr_rtty* r) {
  const size_t ring = (size_t)r->R * r->nb, dec = (size_t)r->max_dec * r->nb;
  PYSDR_HIP_CHECK(r->stream.create(hipStreamNonBlocking));
  PYSDR_HIP_CHECK(r->d_lines.alloc((size_t)r->max_lines * r->nfft));
  PYSDR_HIP_CHECK(r->d_band.alloc((size_t)r->R * r->nband));
  PYSDR_HIP_CHECK(r->d_s4.alloc(ring));
  PYSDR_HIP_CHECK(r->d_best.alloc(ring));
  PYSDR_HIP_CHECK(r->d_sc2.alloc(ring));
  PYSDR_HIP_CHECK(r->d_isym.alloc(ring));
  PYSDR_HIP_CHECK(r->d_shift.alloc((size_t)r->nb));
  PYSDR_HIP_CHECK(r->d_t.alloc(dec));
  PYSDR_HIP_CHECK(r->d_snr.alloc(dec));
  PYSDR_HIP_CHECK(r->d_held.alloc(dec));
  PYSDR_HIP_CHECK(r->d_code.alloc(dec));
  PYSDR_HIP_CHECK(r->d_ndet.alloc((size_t)r->max_lines));
  return PYSDR_OK;
}

int chan_alloc(pysdr_chan* c) {
  const int M = c->M, nk = c->nk;
  const std::vector<float> tw = fft_twiddles(M);
  std::vector<int> perm(nk);                      // where the passes leave the channel of row a
  for (int a = 0; a < nk; ++a) perm[a] = fft_position((c->k_first + a) % M, M, c->plan.npass, c->plan.radix);
  PYSDR_HIP_CHECK(c->stream.create(hipStreamNonBlocking));
  PYSDR_HIP_CHECK(c->d_hist[0].alloc((size_t)c->H));
  PYSDR_HIP_CHECK(c->d_hist[1].alloc((size_t)c->H));
  PYSDR_HIP_CHECK(c->d_taps.alloc((size_t)(c->H + 1)));            // [Pmax][M]
  PYSDR_HIP_CHECK(c->d_tw.alloc((size_t)M));
  PYSDR_HIP_CHECK(c->d_perm.alloc((size_t)nk));
  PYSDR_HIP_CHECK(hipMemcpy(c->d_tw.get(), tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice));
  PYSDR_HIP_CHECK(hipMemcpy(c->d_perm.get(), perm.data(), (size_t)nk * sizeof(int), hipMemcpyHostToDevice));
  return chan_prepare(c->plan);
}

int bank_alloc(pysdr_bank* b) {
  const size_t nk = (size_t)b->nk;
  PYSDR_HIP_CHECK(b->d_y.alloc(nk * b->ypitch));
  PYSDR_HIP_CHECK(b->d_a.alloc(nk * b->apitch));
  PYSDR_HIP_CHECK(b->d_taps.alloc(2 * (size_t)b->plan.tp));
  PYSDR_HIP_CHECK(b->d_pmax.alloc(nk * b->plan.tiles));
  PYSDR_HIP_CHECK(b->d_psum.alloc(nk * b->plan.tiles));
  PYSDR_HIP_CHECK(b->d_state.alloc(nk));
  return PYSDR_OK;
}

int bank_reset_locked(pysdr_bank* b) {
  const int rc = pysdr_chan_reset(b->ch);
  if (rc != PYSDR_OK) return rc;
  PYSDR_HIP_CHECK(hipSetDevice(b->device));
  hipStream_t st = b->stream;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));                          // h_state may still feed an earlier copy
  PYSDR_HIP_CHECK(hipMemsetAsync(b->d_y.get(), 0, (size_t)b->nk * b->ypitch * sizeof(float2), st));
  b->h_state.assign((size_t)b->nk, BankState{0.f, 1.f, 0.f, 0.f, 0.f, 1});
  PYSDR_HIP_CHECK(hipMemcpyAsync(b->d_state.get(), b->h_state.data(), b->h_state.size() * sizeof(BankState), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  b->last_n_out = 0;
  return PYSDR_OK;
}

}  // namespace

namespace pysdr {

int chan_info(pysdr_chan* c, ChanInfo* out) {
  if (!c || !out) { set_last_error("chan_info: NULL channelizer or out"); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(c->mu);
  out->device = c->device; out->M = c->M; out->D = c->D; out->nk = c->nk; out->max_in = c->max_in;
  out->out_cap = c->out_cap; out->stream = c->queue(); out->n_abs = c->n_abs;
  return PYSDR_OK;
}

}  // namespace pysdr

extern "C" {

// ---- waterfall ---------------------------------------------------------------------------

int pysdr_waterfall_create(int device, int nfft, int ncols, pysdr_waterfall** out) {
  if (!out || nfft < 2 || ncols < 1) { set_last_error("pysdr_waterfall_create: out is NULL, nfft %d < 2 or ncols %d < 1", nfft, ncols); return PYSDR_ERR_ARG; }
  int rc = use_device(device);
  if (rc) return rc;
  pysdr_waterfall* w = new pysdr_waterfall();
  w->device = device; w->nfft = nfft; w->ncols = ncols;
  rc = waterfall_alloc(w);
  if (rc) { failed_in("pysdr_waterfall_create", rc); pysdr_waterfall_destroy(w); return rc; }
  *out = w;
  return PYSDR_OK;
}

void pysdr_waterfall_destroy(pysdr_waterfall* w) {
  if (!w) return;
  (void)hipSetDevice(w->device);
  if (w->stream) (void)hipStreamSynchronize(w->stream);
  delete w;                               // (the owners free: host_res.h)
}

int pysdr_waterfall_push(pysdr_waterfall* w, const float* line, int n, int on_device) {
  if (!w || !line || n < 0 || n > w->nfft) { set_last_error("pysdr_waterfall_push: NULL waterfall or line, or n %d outside [0, nfft]", n); return PYSDR_ERR_ARG; }
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  const float* src = line;
  if (!on_device) {
    PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_line.get(), line, (size_t)n * sizeof(float), hipMemcpyHostToDevice, w->stream));
    src = w->d_line.get();
  }
  const int rc = launch_wf_push(src, n, w->nfft, w->shift, w->d_wf.get() + (size_t)w->head * w->nfft, w->stream);
  if (rc) return rc;
  if (!on_device) PYSDR_HIP_CHECK(hipStreamSynchronize(w->stream));   // the caller may reuse `line`
  w->head = (w->head + 1) % w->ncols;
  if (w->cnt < w->ncols) w->cnt++;
  return PYSDR_OK;
}

int pysdr_waterfall_roll(pysdr_waterfall* w, int nbins) {
  if (!w) { set_last_error("pysdr_waterfall_roll: NULL waterfall"); return PYSDR_ERR_ARG; }
  long s = ((long)w->shift + nbins) % w->nfft;
  if (s < 0) s += w->nfft;
  w->shift = (int)s;
  return PYSDR_OK;
}

int pysdr_waterfall_image_rows(pysdr_waterfall* w, float pan_dr, int npsd, float* image_out, float* mean_out,
                               float* bkgnd_out) {
  if (!w || npsd < 1 || npsd > w->nfft) { set_last_error("pysdr_waterfall_image: NULL waterfall or npsd %d outside [1, nfft]", npsd); return PYSDR_ERR_ARG; }
  if (w->cnt < 1) { set_last_error("pysdr_waterfall_image: no line pushed yet"); return PYSDR_ERR_STATE; }
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  const size_t n = (size_t)w->nfft * w->ncols;
  const WfArgs a{w->d_wf.get(), w->nfft, w->ncols, w->head, w->cnt, w->shift, w->d_mean.get(), w->d_stat.get(), w->d_image.get()};
  int rc = launch_wf_mean_median(a, w->stream);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_stat.get() + 1, 0, sizeof(float), w->stream));
  rc = launch_wf_max_image(a, npsd, pan_dr, w->stream);
  if (rc) return rc;
  if (image_out) PYSDR_HIP_CHECK(hipMemcpyAsync(image_out, w->d_image.get(), n * sizeof(float), hipMemcpyDeviceToHost, w->stream));
  if (mean_out) PYSDR_HIP_CHECK(hipMemcpyAsync(mean_out, w->d_mean.get(), (size_t)w->nfft * sizeof(float), hipMemcpyDeviceToHost, w->stream));
  if (bkgnd_out) PYSDR_HIP_CHECK(hipMemcpyAsync(bkgnd_out, w->d_stat.get(), sizeof(float), hipMemcpyDeviceToHost, w->stream));
  PYSDR_HIP_CHECK(hipStreamSynchronize(w->stream));
  return PYSDR_OK;
}

int pysdr_waterfall_peaks(pysdr_waterfall* w, const float* line, int n, double height, int distance, int* idx_out, int cap,
                          int* n_out) {
  if (!w || !n_out || n < 0 || n > w->nfft || distance < 1 || cap < 0 || (cap > 0 && !idx_out)) {
    set_last_error("pysdr_waterfall_peaks: NULL waterfall, n_out or idx_out, n %d outside [0, nfft], distance %d < 1 or cap %d < 0", n, distance, cap);
    return PYSDR_ERR_ARG;
  }
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  const float* x = w->d_mean.get();
  if (line) {
    PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_line.get(), line, (size_t)n * sizeof(float), hipMemcpyHostToDevice, w->stream));
    x = w->d_line.get();
  } else if (w->cnt < 1) {
    set_last_error("pysdr_waterfall_peaks: no averaged line yet (pysdr_waterfall_image first, or pass a line)");
    return PYSDR_ERR_STATE;
  }
  const size_t half = (size_t)w->nfft / 2 + 2;
  int* pos = w->d_pk.get(), *state = pos + half, *kept = pos + 2 * half, *count = pos + 3 * half;
  const int rc = launch_wf_peaks(x, n, height, distance, pos, state, kept, count, w->stream);
  if (rc) return rc;
  int np_ = 0;
  PYSDR_HIP_CHECK(hipMemcpyAsync(&np_, count, sizeof(int), hipMemcpyDeviceToHost, w->stream));
  PYSDR_HIP_CHECK(hipStreamSynchronize(w->stream));
  *n_out = np_;
  const int m = np_ < cap ? np_ : cap;
  if (m > 0) {
    PYSDR_HIP_CHECK(hipMemcpyAsync(idx_out, kept, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, w->stream));
    PYSDR_HIP_CHECK(hipStreamSynchronize(w->stream));
  }
  return PYSDR_OK;
}

int pysdr_waterfall_image(pysdr_waterfall* w, float pan_dr, float* image_out, float* mean_out,
                          float* bkgnd_out) {
  if (!w) { set_last_error("pysdr_waterfall_image: NULL waterfall"); return PYSDR_ERR_ARG; }
  return pysdr_waterfall_image_rows(w, pan_dr, w->nfft, image_out, mean_out, bkgnd_out);
}

// ---- RTTY decoder bank -------------------------------------------------------------------

int pysdr_rtty_create(int device, int nfft, int nbins_shift, int bin_lo, int bin_hi, int find_lo, int find_hi,
                      int max_lines, pysdr_rtty** out) {
  if (!out) { set_last_error("pysdr_rtty_create: out is NULL"); return PYSDR_ERR_ARG; }
  *out = nullptr;
  if (nfft < 2 || nbins_shift < 1 || nbins_shift >= nfft) {
    set_last_error("pysdr_rtty_create: nfft %d / nbins_shift %d", nfft, nbins_shift);
    return PYSDR_ERR_ARG;
  }
  const int top = nfft - nbins_shift;
  if (bin_lo < 0 || bin_hi > top || bin_lo >= bin_hi) {
    set_last_error("pysdr_rtty_create: decoder bins [%d, %d) not a non-empty range inside [0, %d)", bin_lo, bin_hi, top);
    return PYSDR_ERR_ARG;
  }
  if (find_lo < 0 || find_hi > top || find_lo > find_hi) {
    set_last_error("pysdr_rtty_create: finder bins [%d, %d) not a range inside [0, %d)", find_lo, find_hi, top);
    return PYSDR_ERR_ARG;
  }
  if (max_lines < 1 || max_lines > kMaxLines) {
    set_last_error("pysdr_rtty_create: max_lines %d outside [1, %d]", max_lines, kMaxLines);
    return PYSDR_ERR_ARG;
  }
  int rc = use_device(device);
  if (rc) return rc;
  pysdr_rtty* r = new pysdr_rtty();
  r->device = device; r->nfft = nfft; r->nsh = nbins_shift; r->bin_lo = bin_lo; r->bin_hi = bin_hi;
  r->find_lo = find_lo; r->find_hi = find_hi; r->max_lines = max_lines;
  r->nb = bin_hi - bin_lo;
  r->band_lo = find_lo < find_hi ? (bin_lo < find_lo ? bin_lo : find_lo) : bin_lo;
  const int hi = find_lo < find_hi ? (bin_hi > find_hi ? bin_hi : find_hi) : bin_hi;
  r->nband = hi + nbins_shift - r->band_lo;                       // <= nfft - band_lo
  r->R = max_lines + kHist;
  r->max_dec = max_lines / kM + 1;
  rc = rtty_alloc(r);
  if (rc) { failed_in("pysdr_rtty_create", rc); pysdr_rtty_destroy(r); return rc; }
  rc = pysdr_rtty_reset(r);
  if (rc != PYSDR_OK) { pysdr_rtty_destroy(r); return rc; }
  *out = r;
  return PYSDR_OK;
}

void pysdr_rtty_destroy(pysdr_rtty* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  if (r->stream) (void)hipStreamSynchronize(r->stream);
  delete r;
}

int pysdr_rtty_reset(pysdr_rtty* r) {
  if (!r) { set_last_error("pysdr_rtty_reset: NULL decoder"); return PYSDR_ERR_ARG; }
  PYSDR_HIP_CHECK(hipSetDevice(r->device));
  const size_t ring = (size_t)r->R * r->nb;
  PYSDR_HIP_CHECK(hipMemsetAsync(r->d_band.get(), 0, (size_t)r->R * r->nband * sizeof(float), r->stream));
  PYSDR_HIP_CHECK(hipMemsetAsync(r->d_s4.get(), 0, ring * sizeof(float), r->stream));
  PYSDR_HIP_CHECK(hipMemsetAsync(r->d_best.get(), 0, ring * sizeof(float), r->stream));
  PYSDR_HIP_CHECK(hipMemsetAsync(r->d_sc2.get(), 0, ring * sizeof(float), r->stream));
  PYSDR_HIP_CHECK(hipMemsetAsync(r->d_isym.get(), 0, ring * sizeof(int), r->stream));
  PYSDR_HIP_CHECK(hipMemsetAsync(r->d_shift.get(), 0, (size_t)r->nb * sizeof(int), r->stream));   // shift off
  PYSDR_HIP_CHECK(hipStreamSynchronize(r->stream));
  r->n = 0;
  return PYSDR_OK;
}

int pysdr_rtty_decode(pysdr_rtty* r, const float* lines, int nlines, int on_device, int flipped, int* codes,
                      long long* t, double* snr2, int* n_dec, int* ndet, int* isym, float* best) {
  if (!r) { set_last_error("pysdr_rtty_decode: NULL decoder"); return PYSDR_ERR_ARG; }
  if (nlines < 0 || nlines > r->max_lines) {
    set_last_error("pysdr_rtty_decode: nlines %d outside [0, max_lines = %d]", nlines, r->max_lines);
    return PYSDR_ERR_ARG;
  }
  if ((nlines > 0 && !lines) || !codes || !t || !snr2 || !n_dec || !ndet) {
    set_last_error("pysdr_rtty_decode: NULL lines, codes, t, snr2, n_dec or ndet");
    return PYSDR_ERR_ARG;
  }
  *n_dec = 0;
  if (nlines == 0) return PYSDR_OK;
  PYSDR_HIP_CHECK(hipSetDevice(r->device));
  hipStream_t st = r->stream;
  const long long n0 = r->n + 1, n1 = r->n + nlines;                 // lines n0..n1
  const long long j_first = r->n / kM + 1, j_last = n1 / kM;         // decisions at n = 30 j
  const int nd = (int)(j_last - j_first + 1);                        // <= nlines / 30 + 1 = max_dec
  RttyArgs a{};
  a.lines = lines;
  if (!on_device) {
    PYSDR_HIP_CHECK(hipMemcpyAsync(r->d_lines.get(), lines, (size_t)nlines * r->nfft * sizeof(float), hipMemcpyHostToDevice, st));
    a.lines = r->d_lines.get();
  }
  a.nfft = r->nfft; a.flipped = flipped ? 1 : 0; a.nlines = nlines;
  a.band_lo = r->band_lo; a.nband = r->nband; a.moff = r->bin_lo - r->band_lo; a.nsh = r->nsh; a.nb = r->nb;
  a.flo = r->find_lo - r->band_lo; a.fhi = r->find_hi - r->band_lo;
  a.n0 = n0; a.n_first = j_first * kM; a.nd = nd; a.max_dec = r->max_dec; a.R = r->R;
  a.band = r->d_band.get(); a.s4 = r->d_s4.get(); a.best = r->d_best.get(); a.sc2 = r->d_sc2.get(); a.isym = r->d_isym.get();
  a.shift = r->d_shift.get(); a.t = r->d_t.get(); a.snr = r->d_snr.get(); a.held = r->d_held.get(); a.code = r->d_code.get();
  a.ndet = r->d_ndet.get();
  const int rc = launch_rtty_decode(a, st);
  if (rc) return rc;
  const size_t dn = (size_t)nd * r->nb;
  if (nd > 0) {
    PYSDR_HIP_CHECK(hipMemcpyAsync(codes, a.code, dn * sizeof(int), hipMemcpyDeviceToHost, st));
    PYSDR_HIP_CHECK(hipMemcpyAsync(t, a.t, dn * sizeof(long long), hipMemcpyDeviceToHost, st));
    PYSDR_HIP_CHECK(hipMemcpyAsync(snr2, a.snr, dn * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  PYSDR_HIP_CHECK(hipMemcpyAsync(ndet, a.ndet, (size_t)nlines * sizeof(int), hipMemcpyDeviceToHost, st));
  // the per-line rows of the call: ring rows n0 % R .., in at most two pieces
  const int r0 = (int)(n0 % r->R);
  const int first = nlines < r->R - r0 ? nlines : r->R - r0;
  const size_t w = (size_t)r->nb;
  if (isym) {
    PYSDR_HIP_CHECK(hipMemcpyAsync(isym, a.isym + r0 * w, first * w * sizeof(int), hipMemcpyDeviceToHost, st));
    if (first < nlines)
      PYSDR_HIP_CHECK(hipMemcpyAsync(isym + first * w, a.isym, (nlines - first) * w * sizeof(int), hipMemcpyDeviceToHost, st));
  }
  if (best) {
    PYSDR_HIP_CHECK(hipMemcpyAsync(best, a.best + r0 * w, first * w * sizeof(float), hipMemcpyDeviceToHost, st));
    if (first < nlines)
      PYSDR_HIP_CHECK(hipMemcpyAsync(best + first * w, a.best, (nlines - first) * w * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  r->n = n1;
  *n_dec = nd;
  return PYSDR_OK;
}

// ---- polyphase channelizer ---------------------------------------------------------------

int pysdr_chan_plan(int M, int D, int ntaps, int k_first, int nk, int32_t out[16]) {
  if (!out) { set_last_error("pysdr_chan_plan: out is NULL"); return PYSDR_ERR_ARG; }
  ChanPlan p;
  if (!chan_plan(M, D, &p)) {
    set_last_error("pysdr_chan_plan: M %d / D %d: M = 2^a 5^b in [16, 4096], D | M, M / D in {1, 2, 4}", M, D);
    return PYSDR_ERR_ARG;
  }
  if (ntaps < 1 || ntaps > 16 * M) { set_last_error("pysdr_chan_plan: ntaps %d outside [1, 16 M]", ntaps); return PYSDR_ERR_ARG; }
  if (k_first < 0 || k_first >= M || nk < 1 || nk > M) {
    set_last_error("pysdr_chan_plan: channels k_first %d, nk %d outside [0, M) / [1, M]", k_first, nk);
    return PYSDR_ERR_ARG;
  }
  const int P = (ntaps + M - 1) / M;
  for (int i = 0; i < 16; ++i) out[i] = 0;
  out[0] = p.npass;
  for (int i = 0; i < p.npass; ++i) out[1 + i] = p.radix[i];
  out[9] = p.fw; out[10] = p.fi; out[11] = p.threads; out[12] = p.lds_bytes; out[13] = P * M - 1; out[14] = P;
  return PYSDR_OK;
}

int pysdr_chan_create(int device, int M, int D, int k_first, int nk, int max_taps, int max_in, pysdr_chan** out) {
  if (!out) { set_last_error("pysdr_chan_create: out is NULL"); return PYSDR_ERR_ARG; }
  *out = nullptr;
  int32_t pl[16];
  int rc = pysdr_chan_plan(M, D, max_taps, k_first, nk, pl);
  if (rc != PYSDR_OK) return rc;
  if (max_in < 1 || max_in > kChanMaxIn) {
    set_last_error("pysdr_chan_create: max_in %d outside [1, %d]", max_in, kChanMaxIn);
    return PYSDR_ERR_ARG;
  }
  rc = use_device(device);
  if (rc) return rc;
  pysdr_chan* c = new pysdr_chan();
  c->device = device; c->M = M; c->D = D; c->k_first = k_first; c->nk = nk; c->max_taps = max_taps; c->max_in = max_in;
  chan_plan(M, D, &c->plan);
  c->H = (max_taps + M - 1) / M * M - 1;
  c->out_cap = ((max_in + D - 1) / D + 1 + 15) & ~15;
  rc = chan_alloc(c);
  if (rc) { failed_in("pysdr_chan_create", rc); pysdr_chan_destroy(c); return rc; }
  rc = pysdr_chan_reset(c);
  if (rc != PYSDR_OK) { pysdr_chan_destroy(c); return rc; }
  *out = c;
  return PYSDR_OK;
}

void pysdr_chan_destroy(pysdr_chan* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->queue()) (void)hipStreamSynchronize(c->queue());
  if (c->ops) c->ops->destroy(c);
  delete c;
}

int pysdr_chan_set_taps(pysdr_chan* c, const double* h, int ntaps) {
  if (!c || !h) { set_last_error("pysdr_chan_set_taps: NULL channelizer or taps"); return PYSDR_ERR_ARG; }
  if (c->ops) { set_last_error("pysdr_chan_set_taps: a fine channelizer takes its two prototypes through pysdr_chan_fine_set_taps"); return PYSDR_ERR_STATE; }
  if (ntaps < 1 || ntaps > c->max_taps) {
    set_last_error("pysdr_chan_set_taps: ntaps %d outside [1, max_taps = %d]", ntaps, c->max_taps);
    return PYSDR_ERR_ARG;
  }
  std::lock_guard<std::mutex> lk(c->mu);
  PYSDR_HIP_CHECK(hipSetDevice(c->device));
  const int P = (ntaps + c->M - 1) / c->M;
  PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream));              // the staging vector may still feed an earlier copy
  c->h_taps.assign((size_t)P * c->M, 0.f);
  for (int i = 0; i < ntaps; ++i) c->h_taps[i] = (float)h[i];
  PYSDR_HIP_CHECK(hipMemcpyAsync(c->d_taps.get(), c->h_taps.data(), c->h_taps.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream));
  c->P = P;
  return PYSDR_OK;
}

int pysdr_chan_reset(pysdr_chan* c) {
  if (!c) { set_last_error("pysdr_chan_reset: NULL channelizer"); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(c->mu);
  if (c->ops) return c->ops->reset(c);
  PYSDR_HIP_CHECK(hipSetDevice(c->device));
  PYSDR_HIP_CHECK(hipMemsetAsync(c->d_hist[0].get(), 0, (size_t)c->H * sizeof(float2), c->stream));
  PYSDR_HIP_CHECK(hipMemsetAsync(c->d_hist[1].get(), 0, (size_t)c->H * sizeof(float2), c->stream));
  PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream));
  c->cur = 0;
  c->n_abs = 0;
  return PYSDR_OK;
}

int pysdr_chan_sync(pysdr_chan* c) {
  if (!c) { set_last_error("pysdr_chan_sync: NULL channelizer"); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(c->mu);
  PYSDR_HIP_CHECK(hipSetDevice(c->device));
  PYSDR_HIP_CHECK(hipStreamSynchronize(c->queue()));
  return PYSDR_OK;
}

int pysdr_chan_process(pysdr_chan* c, const void* iq, int n, int on_device, void* out, long long out_pitch, int out_on_device,
                       int* n_out) {
  if (!c || !n_out) { set_last_error("pysdr_chan_process: NULL channelizer or n_out"); return PYSDR_ERR_ARG; }
  *n_out = 0;
  std::lock_guard<std::mutex> lk(c->mu);
  if (c->ops) return c->ops->process(c, iq, n, on_device, out, out_pitch, out_on_device, n_out);
  if (n < 0 || (n > 0 && !iq)) { set_last_error("pysdr_chan_process: n %d / NULL input", n); return PYSDR_ERR_ARG; }
  if (n > c->max_in) { set_last_error("pysdr_chan_process: n %d > max_in %d", n, c->max_in); return PYSDR_ERR_STATE; }
  if (c->P == 0) { set_last_error("pysdr_chan_process: no taps set"); return PYSDR_ERR_STATE; }
  const unsigned long long D = (unsigned long long)c->D, s0 = c->n_abs, s1 = s0 + (unsigned long long)n;
  const unsigned long long mf = (s0 + D - 1) / D, ml = (s1 + D - 1) / D;          // out_index_range(s0, s1, 1, D)
  const int nf = (int)(ml - mf);
  if (nf > 0 && !out) { set_last_error("pysdr_chan_process: NULL output"); return PYSDR_ERR_ARG; }
  if (out_pitch < nf) { set_last_error("pysdr_chan_process: pitch %lld < the call's %d outputs", out_pitch, nf); return PYSDR_ERR_STATE; }
  if (n == 0) return PYSDR_OK;
  PYSDR_HIP_CHECK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const float2* src = static_cast<const float2*>(iq);
  int rc;
  if (!on_device) {
    PYSDR_HIP_CHECK(c->d_in.grow((size_t)c->max_in));
    PYSDR_HIP_CHECK(hipMemcpyAsync(c->d_in.get(), iq, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, st));
    src = c->d_in.get();
  }
  if (nf > 0) {
    if (!out_on_device) PYSDR_HIP_CHECK(c->d_out.grow((size_t)c->nk * c->out_cap));
    const ChanPlan& pl = c->plan;
    ChanArgs a{};
    a.x = src; a.hist = c->d_hist[c->cur].get(); a.H = c->H; a.n = n;
    a.off0 = (int)(mf * D - s0); a.mf_lo = (int)(mf & 3ull); a.nframes = nf;
    a.M = c->M; a.D = c->D; a.P = c->P; a.mp = pl.mp; a.fw = pl.fw;
    a.taps = c->d_taps.get(); a.tw = c->d_tw.get(); a.perm = c->d_perm.get(); a.nk = c->nk;
    a.y = out_on_device ? static_cast<float2*>(out) : c->d_out.get();
    a.pitch = out_on_device ? out_pitch : (long long)c->out_cap;
    a.magic_M = magic_of(c->M); a.magic_fw = magic_of(pl.fw);
    a.fft = fft_passes(c->M, pl.npass, pl.radix);
    const int grid = (nf + pl.fw - 1) / pl.fw;
    a.xq = grid / 8; a.xr = grid % 8;
    rc = launch_chan(pl, a, grid, st);
    if (rc) return rc;
  }
  rc = launch_chan_roll(src, n, c->d_hist[c->cur].get(), c->d_hist[c->cur ^ 1].get(), c->H, st);
  if (rc) return rc;
  c->cur ^= 1;
  c->n_abs = s1;
  *n_out = nf;
  if (nf > 0 && !out_on_device)
    PYSDR_HIP_CHECK(hipMemcpy2DAsync(out, (size_t)out_pitch * sizeof(float2), c->d_out.get(), (size_t)c->out_cap * sizeof(float2),
                                     (size_t)nf * sizeof(float2), (size_t)c->nk, hipMemcpyDeviceToHost, st));
  if (!on_device || !out_on_device) PYSDR_HIP_CHECK(hipStreamSynchronize(st));   // host buffers are the caller's again
  return PYSDR_OK;
}

// ---- channel bank ------------------------------------------------------------------------

int pysdr_bank_plan(int nk, int ntaps_af, int max_out, int32_t out[8]) {
  if (!out) { set_last_error("pysdr_bank_plan: out is NULL"); return PYSDR_ERR_ARG; }
  BankPlan p;
  if (!bank_plan(nk, ntaps_af, max_out, &p)) {
    set_last_error("pysdr_bank_plan: nk %d outside [1, %d], ntaps_af %d outside [%d, %d] or max_out %d < 1", nk, kBankNkMax,
                   ntaps_af, kBankTapsMin, kBankTapsMax, max_out);
    return PYSDR_ERR_ARG;
  }
  out[0] = kBankTile; out[1] = kBankThreads; out[2] = p.lds_floats * (int)sizeof(float); out[3] = p.tiles; out[4] = p.hpad;
  out[5] = p.tp; out[6] = 0; out[7] = 0;
  return PYSDR_OK;
}

int pysdr_bank_create(pysdr_chan* ch, double fs_out, int mode, int ntaps_af, pysdr_bank** out) {
  if (!out) { set_last_error("pysdr_bank_create: out is NULL"); return PYSDR_ERR_ARG; }
  *out = nullptr;
  if (!ch) { set_last_error("pysdr_bank_create: NULL channelizer"); return PYSDR_ERR_ARG; }
  if (mode != PYSDR_AM && mode != PYSDR_NFM) { set_last_error("pysdr_bank_create: mode %d is neither AM nor NFM", mode); return PYSDR_ERR_ARG; }
  if (!(fs_out > 0.0)) { set_last_error("pysdr_bank_create: fs_out %g", fs_out); return PYSDR_ERR_ARG; }
  pysdr_bank* b = new pysdr_bank();
  int rc = client_bind(b, ch);
  if (rc != PYSDR_OK) { delete b; return rc; }
  if (!bank_plan(b->nk, ntaps_af, b->out_cap, &b->plan)) {
    set_last_error("pysdr_bank_create: ntaps_af %d outside [%d, %d]", ntaps_af, kBankTapsMin, kBankTapsMax);
    delete b;
    return PYSDR_ERR_ARG;
  }
  b->mode = mode; b->T = ntaps_af;
  b->fs_out = fs_out;
  b->fm_scale = (float)(fs_out / (2.0 * M_PI * kNfmFullScaleDev));
  b->ypitch = (long long)b->plan.hpad + b->out_cap;
  b->apitch = b->out_cap;
  return client_create(b, "pysdr_bank_create", bank_alloc, bank_reset_locked, out);
}

void pysdr_bank_destroy(pysdr_bank* b) { client_destroy(b); }

int pysdr_bank_set_mode(pysdr_bank* b, int mode, const double* af, int ntaps) {
  if (!b || !af) { set_last_error("pysdr_bank_set_mode: NULL bank or taps"); return PYSDR_ERR_ARG; }
  if (mode != PYSDR_AM && mode != PYSDR_NFM) { set_last_error("pysdr_bank_set_mode: mode %d is neither AM nor NFM", mode); return PYSDR_ERR_ARG; }
  if (ntaps != b->T) { set_last_error("pysdr_bank_set_mode: ntaps %d != ntaps_af %d", ntaps, b->T); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(b->mu);
  PYSDR_HIP_CHECK(hipSetDevice(b->device));
  hipStream_t st = b->stream;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));                          // the staging vector may still feed an earlier copy
  b->h_taps.assign((size_t)b->plan.tp, 0.f);
  for (int i = 0; i < ntaps; ++i) b->h_taps[i] = (float)af[i];
  PYSDR_HIP_CHECK(hipMemcpyAsync(b->d_taps.get(), b->h_taps.data(), b->h_taps.size() * sizeof(float), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  b->mode = mode;
  b->have_taps = true;
  return PYSDR_OK;
}

int pysdr_bank_set_mode_cplx(pysdr_bank* b, int mode, const double* af_re, const double* af_im, int ntaps, double bfo_hz) {
  if (!b || !af_re || !af_im) { set_last_error("pysdr_bank_set_mode_cplx: NULL bank or taps"); return PYSDR_ERR_ARG; }
  if (mode != PYSDR_USB && mode != PYSDR_LSB && mode != PYSDR_CW) { set_last_error("pysdr_bank_set_mode_cplx: mode %d is none of USB, LSB, CW", mode); return PYSDR_ERR_ARG; }
  if (ntaps != b->T) { set_last_error("pysdr_bank_set_mode_cplx: ntaps %d != ntaps_af %d", ntaps, b->T); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(b->mu);
  PYSDR_HIP_CHECK(hipSetDevice(b->device));
  hipStream_t st = b->stream;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));                          // the staging vector may still feed an earlier copy
  const size_t tp = (size_t)b->plan.tp;
  b->h_taps.assign(2 * tp, 0.f);
  for (int i = 0; i < ntaps; ++i) { b->h_taps[i] = (float)af_re[i]; b->h_taps[tp + i] = -(float)af_im[i]; }   // -im: every term an fma
  PYSDR_HIP_CHECK(hipMemcpyAsync(b->d_taps.get(), b->h_taps.data(), b->h_taps.size() * sizeof(float), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  b->mode = mode;
  b->fword = (mode == PYSDR_CW) ? pysdr_freq_word(bfo_hz, b->fs_out, nullptr) : 0u;
  b->have_taps = true;
  return PYSDR_OK;
}

int pysdr_bank_set_agc(pysdr_bank* b, int enable, float ref) {
  if (!b) { set_last_error("pysdr_bank_set_agc: NULL bank"); return PYSDR_ERR_ARG; }
  if (!(ref > 0.f)) { set_last_error("pysdr_bank_set_agc: ref %g", (double)ref); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(b->mu);
  b->agc_enable = enable ? 1 : 0;
  b->ref = ref;
  return PYSDR_OK;
}

int pysdr_bank_set_squelch(pysdr_bank* b, float thresh) {
  if (!b) { set_last_error("pysdr_bank_set_squelch: NULL bank"); return PYSDR_ERR_ARG; }
  if (!(thresh >= 0.f)) { set_last_error("pysdr_bank_set_squelch: threshold %g", (double)thresh); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(b->mu);
  b->thresh = thresh;
  return PYSDR_OK;
}

int pysdr_bank_reset(pysdr_bank* b) {
  if (!b) { set_last_error("pysdr_bank_reset: NULL bank"); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(b->mu);
  return bank_reset_locked(b);
}

int pysdr_bank_sync(pysdr_bank* b) {
  if (!b) { set_last_error("pysdr_bank_sync: NULL bank"); return PYSDR_ERR_ARG; }
  return client_sync(b);
}

int pysdr_bank_process(pysdr_bank* b, const void* iq, int n, int on_device, float* am, long long am_pitch, int am_on_device,
                       int* n_out) {
  if (!b || !n_out) { set_last_error("pysdr_bank_process: NULL bank or n_out"); return PYSDR_ERR_ARG; }
  *n_out = 0;
  std::lock_guard<std::mutex> lk(b->mu);
  ClientStep step;
  int rc = client_begin(b, "pysdr_bank_process", iq, n, &step);
  if (rc != PYSDR_OK) return rc;
  if (!b->have_taps) { set_last_error("pysdr_bank_process: no mode set"); return PYSDR_ERR_STATE; }
  if (am && am_pitch < (long long)step.nf_want) {
    set_last_error("pysdr_bank_process: pitch %lld < the call's %d outputs", am_pitch, (int)step.nf_want);
    return PYSDR_ERR_STATE;
  }
  int nf = 0;
  rc = client_feed(b, "pysdr_bank_process", "bank", iq, n, on_device, b->d_y.get() + b->plan.hpad, b->ypitch, step, &nf);
  if (rc != PYSDR_OK) return rc;
  if (nf == 0) return PYSDR_OK;                                       // no output: no AGC block, no state change, nothing to fetch
  PYSDR_HIP_CHECK(hipSetDevice(b->device));
  hipStream_t st = b->stream;
  const int ntiles = (nf + kBankTile - 1) / kBankTile;
  const int squelch = (b->mode == PYSDR_NFM && b->thresh > 0.f) ? 1 : 0;
  BankArgs a{};
  a.y = b->d_y.get() + b->plan.hpad; a.ypitch = b->ypitch; a.a = b->d_a.get(); a.apitch = b->apitch;
  a.n_out = nf; a.T = b->T; a.tp = b->plan.tp; a.taps = b->d_taps.get(); a.fm_scale = b->fm_scale; a.noise = squelch;
  a.pmax = b->d_pmax.get(); a.psum = b->d_psum.get(); a.ptiles = b->plan.tiles;
  a.m0_lo = (uint32_t)step.m0; a.fword = b->fword;          // CW: the BFO phase follows the absolute output index
  rc = launch_bank(b->mode, b->plan, a, ntiles, b->nk, st);
  if (rc) return rc;
  FinishArgs f{};
  f.ybase = b->d_y.get(); f.ypitch = b->ypitch; f.a = a.a; f.apitch = b->apitch;
  f.n_out = nf; f.hpad = b->plan.hpad; f.ntiles = ntiles; f.ptiles = b->plan.tiles;
  f.pmax = a.pmax; f.psum = a.psum; f.state = b->d_state.get();
  f.agc_active = (b->agc_enable && b->mode != PYSDR_NFM) ? 1 : 0;      // AM, USB, LSB, CW: the oracle's AGC_MODES
  f.squelch = squelch; f.ref = b->ref; f.thresh = b->thresh;
  rc = launch_bank_finish(f, b->nk, st);
  if (rc) return rc;
  *n_out = nf;
  if (am) {
    PYSDR_HIP_CHECK(hipMemcpy2DAsync(am, (size_t)am_pitch * sizeof(float), a.a, (size_t)b->apitch * sizeof(float),
                                     (size_t)nf * sizeof(float), (size_t)b->nk,
                                     am_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    if (!am_on_device) PYSDR_HIP_CHECK(hipStreamSynchronize(st));     // the host buffer is the caller's again
  }
  return PYSDR_OK;
}

int pysdr_bank_state(pysdr_bank* b, float* agc, float* gain, float* maxbuf, float* level, uint8_t* open) {
  if (!b) { set_last_error("pysdr_bank_state: NULL bank"); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(b->mu);
  PYSDR_HIP_CHECK(hipSetDevice(b->device));
  hipStream_t st = b->stream;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  PYSDR_HIP_CHECK(hipMemcpyAsync(b->h_state.data(), b->d_state.get(), b->h_state.size() * sizeof(BankState), hipMemcpyDeviceToHost, st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  for (int i = 0; i < b->nk; ++i) {
    const BankState& s = b->h_state[i];
    if (agc) agc[i] = s.agc;
    if (gain) gain[i] = s.gain;
    if (maxbuf) maxbuf[i] = s.maxbuf;
    if (level) level[i] = s.level;
    if (open) open[i] = s.open ? 1 : 0;
  }
  return PYSDR_OK;
}

int pysdr_bank_fetch(pysdr_bank* b, const int* rows, int nrows, float* am, float* iq, long long pitch) {
  if (!b) { set_last_error("pysdr_bank_fetch: NULL bank"); return PYSDR_ERR_ARG; }
  if (nrows < 0 || (nrows > 0 && !rows)) { set_last_error("pysdr_bank_fetch: nrows %d / NULL rows", nrows); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(b->mu);
  if (!rows_inside("pysdr_bank_fetch", "row", rows, nrows, b->nk)) return PYSDR_ERR_ARG;
  const int nf = b->last_n_out;
  if (pitch < nf) { set_last_error("pysdr_bank_fetch: pitch %lld < the last call's %d outputs", pitch, nf); return PYSDR_ERR_STATE; }
  if (nf == 0 || nrows == 0 || (!am && !iq)) return PYSDR_OK;
  PYSDR_HIP_CHECK(hipSetDevice(b->device));
  hipStream_t st = b->stream;
  for (int i = 0, run; i < nrows; i += run) {                         // run by run, audio then IQ of each
    run = row_run(rows, nrows, i);
    int rc = am ? copy_row_run<float>(rows, i, run, b->d_a.get(), b->apitch, am, pitch, (size_t)nf, st) : PYSDR_OK;
    if (rc == PYSDR_OK && iq)
      rc = copy_row_run<float2>(rows, i, run, b->d_y.get() + b->plan.hpad, b->ypitch, reinterpret_cast<float2*>(iq), pitch, (size_t)nf, st);
    if (rc) return rc;
  }
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  return PYSDR_OK;
}

}  // extern "C"
