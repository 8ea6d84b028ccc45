// C ABI of the FT8 and FT4 skimmers (include/pysdr_hip.h).  Host-side only, like api_fsk.hip:
// the kernels and their launch functions live in ft.hip, what both sides share in ft_plan.h.  One skimmer, templated on
// the mode; every call is written once, and the extern "C" functions at the end forward to it under their own names.  A
// skimmer borrows a channelizer as the other skimmers do (chan_client.h: what the channelizer's clients share) and queues
// its kernels behind the channelizer's launch on the channelizer's stream.  The call list is skimmer_host.h's, the
// skimmers' shared core, which reset, sync and fetch forward to directly; here is what only this kind has: its struct,
// buffers, plan, the step count that a process call keeps, the soft bits and the state call.  Every device resource is
// an owner (host_res.h): deleting the object frees it.  The decoder's calls are ldpc_host.h's, the frame report's and
// the row floor's report_host.h's, a-priori decoding's ap_host.h's; all read the mode from the skimmer.
#include "ap_host.h"
#include "ft_plan.h"
#include "ldpc_host.h"
#include "pass_host.h"
#include "report_host.h"

using namespace pysdr;

template <class M>
struct FtSkimmer : SkimmerBase {    // rows = nfine, words = cap * kFtEventWords
  using Mode = M;
  FtCfg cfg{};
  FtPlan plan;
  unsigned long long t_done = 0;    // steps complete since create / reset
  DevBuf<FtC> d_y;                  // [nk][ypitch]: Mode::kHpad of history room, then the call's outputs
  DevBuf<FtC> d_tw;                 // [NT]
  DevBuf<float> d_ring;             // [nk][tr][NB]
  DevBuf<float> d_sc;               // [9][nfine]
  DevBuf<int32_t> d_hi;             // [9][nfine]
  DevBuf<int32_t> d_cand;           // [kFtLlrMax][2]
  DevBuf<float> d_llr;              // [kFtLlrMax][174]
  std::vector<float> h_tw;
  std::vector<int32_t> h_cand;
  LdpcBufs ldpc;                    // the decoder's results (ldpc_host.h)
  ReportBufs report;                // the frame report's and the row floor's (report_host.h)
  PassBufs pass;                    // the second pass's rings and tables, once kept (pass_host.h)
  ApBufs ap;                        // a-priori decoding's tables and results, once called (ap_host.h)
  FtC* feed_rows() { return d_y.get() + Mode::kHpad; }
};

struct pysdr_ft8 : FtSkimmer<Ft8Mode> {};
struct pysdr_ft4 : FtSkimmer<Ft4Mode> {};

namespace {

// the two public cfg structs are FtCfg's layout (ft_plan.h asserts it)
const FtCfg* ft_cfg(const pysdr_ft8_cfg* c) { return reinterpret_cast<const FtCfg*>(c); }
const FtCfg* ft_cfg(const pysdr_ft4_cfg* c) { return reinterpret_cast<const FtCfg*>(c); }

template <class W>
int ft_alloc(W* w) {
  const size_t nk = (size_t)w->nk, nf = (size_t)w->plan.nfine, S = (size_t)w->plan.S;
  PYSDR_HIP_CHECK(w->d_y.alloc(nk * (size_t)w->plan.ypitch));
  PYSDR_HIP_CHECK(w->d_tw.alloc(4 * S));
  PYSDR_HIP_CHECK(w->d_ring.alloc(nk * (size_t)w->plan.tr * (size_t)w->plan.nb));
  PYSDR_HIP_CHECK(w->d_sc.alloc((size_t)kFtKeep * nf));
  PYSDR_HIP_CHECK(w->d_hi.alloc((size_t)kFtKeep * nf));
  PYSDR_HIP_CHECK(w->d_cand.alloc((size_t)kFtLlrMax * 2));
  PYSDR_HIP_CHECK(w->d_llr.alloc((size_t)kFtLlrMax * kFtBits));
  return skimmer_alloc(w);
}

template <class W>
int ft_reset_locked(W* w) {
  const int rc = pysdr_chan_reset(w->ch);
  if (rc != PYSDR_OK) return rc;
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  const size_t nk = (size_t)w->nk, nf = (size_t)w->plan.nfine;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));                          // the host arrays may still feed an earlier copy
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_tw.get(), w->h_tw.data(), w->h_tw.size() * sizeof(float), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_y.get(), 0, nk * (size_t)w->plan.ypitch * sizeof(FtC), st));   // y[k] = 0 for k < 0
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_ring.get(), 0, nk * (size_t)w->plan.tr * (size_t)w->plan.nb * sizeof(float), st));
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_sc.get(), 0, (size_t)kFtKeep * nf * sizeof(float), st));
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_hi.get(), 0, (size_t)kFtKeep * nf * sizeof(int32_t), st));
  if (const int rc2 = skimmer_clear(w, st)) return rc2;
  if (const int rc3 = pass_clear(&w->pass, w->nk, w->plan.nb, st)) return rc3;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  w->last_n_out = 0;
  w->t_done = 0;
  return PYSDR_OK;
}

// the first pass's spectrum ring, as the decoder asks for it under the skimmer's lock
template <class W> RingRef first_ring(W* w) { return RingRef{w->d_ring.get(), w->plan.tr}; }

// `who` in every call below: the public function's name, for the messages

template <class Mode>
int ft_plan_call(const char* who, int nk, int S, int max_out, const FtCfg* cfg, int32_t out[8]) {
  if (!out) { set_last_error("%s: out is NULL", who); return PYSDR_ERR_ARG; }
  FtPlan p;
  if (!ft_plan<Mode>(nk, S, max_out, cfg, &p)) {
    set_last_error("%s: S %d is neither %d nor %d, nk %d < 1 or nk S / 2 > %d, max_out %d outside [1, %d], a spectrum ring "
                   "above %lld bytes, or a cfg outside the rules (NULL; smin >= 0, 0 <= hmin <= %d, 0 < pmax <= 1e18, all finite)", who, S,
                   Mode::kS0, Mode::kS1, nk, kFtFineMax, max_out, kFtMaxOutMax, kFtRingBytesMax, Mode::kSync);
    return PYSDR_ERR_ARG;
  }
  out[0] = 1; out[1] = ft_threads<Mode>(S); out[2] = ft_lds_bytes<Mode>(S); out[3] = S; out[4] = p.cap; out[5] = p.groups;
  out[6] = p.nsub; out[7] = p.tr;
  return PYSDR_OK;
}

// who_plan: the plan function's name, whose refusal a create call passes on
template <class W>
int ft_create(const char* who, const char* who_plan, pysdr_chan* ch, int S, const FtCfg* cfg, const float* tw, int max_out, W** out) {
  using Mode = typename W::Mode;
  return skimmer_create(who, ch && cfg && tw, "NULL channelizer, cfg or tw", ch, max_out, out, ft_alloc<W>, ft_reset_locked<W>, [&](W* w) -> int {
    int32_t pl[8];
    if (!ft_plan<Mode>(w->nk, S, max_out, cfg, &w->plan)) return ft_plan_call<Mode>(who_plan, w->nk, S, max_out, cfg, pl);
    w->cfg = *cfg;
    w->rows = w->plan.nfine; w->words = w->plan.cap * kFtEventWords;
    w->h_tw.assign(tw, tw + 2 * 4 * (size_t)S);
    w->h_cand.reserve((size_t)kFtLlrMax * 2);
    return PYSDR_OK;
  });
}

template <class W>
int ft_process(W* w, const char* who, const void* iq, int n, int on_device, int* n_out, int32_t* counts, int32_t* events,
               long long ev_pitch, long long* steps) {
  using Mode = typename W::Mode;
  return skimmer_process(w, who, iq, n, on_device, n_out, counts, events, ev_pitch, [&](const ClientStep& step, int nf, hipStream_t st) -> int {
    const int S = w->plan.S;
    if (steps) { steps[0] = (long long)w->t_done; steps[1] = 0; }
    if (nf == 0) return PYSDR_OK;
    const unsigned long long t1 = ft_steps_done(step.m0 + (unsigned long long)nf, S);
    FtArgs a{};
    a.y = w->feed_rows(); a.ypitch = w->plan.ypitch; a.n_out = nf; a.nk = w->nk; a.cap = w->plan.cap; a.nfine = w->plan.nfine;
    a.ns = (int)(t1 - w->t_done);
    a.e_first = a.ns > 0 ? (int)((unsigned long long)(S / 4) * w->t_done + (unsigned long long)(S - 1) - step.m0) : 0;
    a.tr = w->plan.tr; a.t_first = (long long)w->t_done;
    a.cfg = w->cfg; a.tw = w->d_tw.get(); a.ring = w->d_ring.get(); a.sc = w->d_sc.get(); a.hi = w->d_hi.get();
    a.events = w->d_events.get(); a.counts = w->d_counts.get();
    if (a.ns < 0 || a.ns > ft_steps_per_call(w->max_out, S) || a.e_first < 0 || a.e_first >= (w->t_done ? S / 4 : S)) {
      set_last_error("%s: the step count lost its place (%d steps, first at output %d)", who, a.ns, a.e_first);
      return PYSDR_ERR_STATE;
    }
    if (a.ns == 0) PYSDR_HIP_CHECK(hipMemsetAsync(a.counts, 0, (size_t)w->rows * sizeof(int32_t), st));   // outputs but no step: only the history rolls
    const int rc = launch_ft_steps(Mode::kLdpcSource, S, a, st);
    if (rc) return rc;
    if (const int rc2 = pass_step(w, step.m0, nf, a.ns, a.t_first, st)) return rc2;   // (nothing unless pysdr_*_keep was called)
    w->t_done = t1;
    if (steps) steps[1] = a.ns;
    return PYSDR_OK;
  });
}

// residue: from the second pass's ring2 (PYSDR_ERR_STATE unless kept) instead of the spectrum ring
template <class W>
int ft_llr(W* w, const char* who, const int32_t* F, const long long* t0, int n, float* out, bool residue = false) {
  using Mode = typename W::Mode;
  if (!w) return no_skimmer(who);
  if (n < 0 || n > kFtLlrMax || (n > 0 && (!F || !t0 || !out))) {
    set_last_error("%s: n %d outside [0, %d] / NULL F, t0 or out", who, n, kFtLlrMax);
    return PYSDR_ERR_ARG;
  }
  std::lock_guard<std::mutex> lk(w->mu);
  if (residue && !w->pass.kept) return pass_not_kept(who);
  const float* ring = residue ? w->pass.d_ring2.get() : w->d_ring.get();
  const int tr = residue ? w->pass.plan.tr2 : w->plan.tr;
  const long long done = (long long)w->t_done;
  for (int i = 0; i < n; ++i)                                          // every candidate first: a refusal changes nothing
    if (!ft_llr_ok<Mode>(F[i], t0[i], done, w->plan.nfine, tr)) {
      set_last_error("%s: candidate %d (F %d, t0 %lld): F outside [0, %d), or a frame not yet complete or gone from the "
                     "ring (%lld steps done, its last is %lld, the ring holds %d)", who, i, (int)F[i], t0[i], w->plan.nfine, done,
                     t0[i] + kFtLag<Mode>, tr);
      return F[i] < 0 || F[i] >= w->plan.nfine ? PYSDR_ERR_ARG : PYSDR_ERR_STATE;
    }
  if (n == 0) return PYSDR_OK;
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));                          // h_cand may still feed an earlier copy
  w->h_cand.resize((size_t)n * 2);
  for (int i = 0; i < n; ++i) { w->h_cand[2 * (size_t)i] = F[i]; w->h_cand[2 * (size_t)i + 1] = (int32_t)(t0[i] % tr); }
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_cand.get(), w->h_cand.data(), (size_t)n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, st));
  FtLlrArgs a{};
  a.ring = ring; a.tr = tr; a.nb = w->plan.nb; a.nsub = w->plan.nsub; a.n = n; a.cand = w->d_cand.get(); a.out = w->d_llr.get();
  const int rc = launch_ft_llr(Mode::kLdpcSource, a, st);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipMemcpyAsync(out, a.out, (size_t)n * kFtBits * sizeof(float), hipMemcpyDeviceToHost, st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  return PYSDR_OK;
}

template <class W>
int ft_state(W* w, const char* who, float* sc, int32_t* hits, float* ring, long long* t_done) {
  if (!w) return no_skimmer(who);
  std::lock_guard<std::mutex> lk(w->mu);
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  const size_t nf = (size_t)w->plan.nfine;
  if (sc) PYSDR_HIP_CHECK(hipMemcpyAsync(sc, w->d_sc.get(), (size_t)kFtKeep * nf * sizeof(float), hipMemcpyDeviceToHost, st));
  if (hits) PYSDR_HIP_CHECK(hipMemcpyAsync(hits, w->d_hi.get(), (size_t)kFtKeep * nf * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (ring)
    PYSDR_HIP_CHECK(hipMemcpyAsync(ring, w->d_ring.get(), (size_t)w->nk * (size_t)w->plan.tr * (size_t)w->plan.nb * sizeof(float),
                                   hipMemcpyDeviceToHost, st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  if (t_done) *t_done = (long long)w->t_done;
  return PYSDR_OK;
}

}  // namespace

extern "C" {

// ---- FT8 ---------------------------------------------------------------------------------------------------------------
int pysdr_ft8_plan(int nk, int S, int max_out, const pysdr_ft8_cfg* cfg, int32_t out[8]) {
  return ft_plan_call<Ft8Mode>("pysdr_ft8_plan", nk, S, max_out, ft_cfg(cfg), out);
}
int pysdr_ft8_create(pysdr_chan* ch, int S, const pysdr_ft8_cfg* cfg, const float* tw, int max_out, pysdr_ft8** out) {
  return ft_create("pysdr_ft8_create", "pysdr_ft8_plan", ch, S, ft_cfg(cfg), tw, max_out, out);
}
void pysdr_ft8_destroy(pysdr_ft8* w) { client_destroy(w); }
int pysdr_ft8_reset(pysdr_ft8* w) { return skimmer_reset(w, "pysdr_ft8_reset", ft_reset_locked<pysdr_ft8>); }
int pysdr_ft8_sync(pysdr_ft8* w) { return skimmer_sync(w, "pysdr_ft8_sync"); }
int pysdr_ft8_process(pysdr_ft8* w, const void* iq, int n, int on_device, int* n_out, int32_t* counts, int32_t* events,
                      long long ev_pitch, long long* steps) {
  return ft_process(w, "pysdr_ft8_process", iq, n, on_device, n_out, counts, events, ev_pitch, steps);
}
int pysdr_ft8_fetch(pysdr_ft8* w, const int* rows, int nrows, int32_t* events, long long pitch) {
  return skimmer_fetch(w, "pysdr_ft8_fetch", "fine row", rows, nrows, events, pitch);
}
int pysdr_ft8_llr(pysdr_ft8* w, const int32_t* F, const long long* t0, int n, float* out) { return ft_llr(w, "pysdr_ft8_llr", F, t0, n, out); }
int pysdr_ft8_state(pysdr_ft8* w, float* sc, int32_t* hits, float* ring, long long* t_done) {
  return ft_state(w, "pysdr_ft8_state", sc, hits, ring, t_done);
}
int pysdr_ft8_decode(pysdr_ft8* w, const int32_t* F, const long long* t0, int n, const pysdr_ldpc_cfg* cfg, int32_t* status, uint8_t* bits,
                     float* post) {
  return ldpc_decode_ring(w, "pysdr_ft8_decode", first_ring<std::remove_pointer_t<decltype(w)>>, F, t0, n, cfg, status, bits, post);
}
int pysdr_ft8_decode_llr(pysdr_ft8* w, const float* llr, int n, const pysdr_ldpc_cfg* cfg, int32_t* status, uint8_t* bits, float* post) {
  return ldpc_decode_llr(w, "pysdr_ft8_decode_llr", llr, n, cfg, status, bits, post);
}
int pysdr_ft8_decode_osd(pysdr_ft8* w, const int32_t* F, const long long* t0, int n, const pysdr_ldpc_cfg* cfg, int32_t* status,
                         uint8_t* bits, float* post, const pysdr_osd_cfg* osd, int32_t* detail) {
  return ldpc_decode_ring(w, "pysdr_ft8_decode_osd", first_ring<std::remove_pointer_t<decltype(w)>>, F, t0, n, cfg, status, bits, post, OsdCall{true, osd, detail});
}
int pysdr_ft8_decode_llr_osd(pysdr_ft8* w, const float* llr, int n, const pysdr_ldpc_cfg* cfg, int32_t* status, uint8_t* bits,
                             float* post, const pysdr_osd_cfg* osd, int32_t* detail) {
  return ldpc_decode_llr(w, "pysdr_ft8_decode_llr_osd", llr, n, cfg, status, bits, post, OsdCall{true, osd, detail});
}
int pysdr_ft8_decode_ap(pysdr_ft8* w, const int32_t* F, const long long* t0, int n, const uint8_t* hyps, int H, const int32_t* pairs, int P,
                        const pysdr_ldpc_cfg* cfg, const pysdr_ap_cfg* apcfg, int32_t* ap, uint8_t* bits, int32_t* detail) {
  return ap_decode_ring(w, "pysdr_ft8_decode_ap", F, t0, n, cfg, ApCall{hyps, H, pairs, P, apcfg, detail}, ap, bits);
}
int pysdr_ft8_decode_llr_ap(pysdr_ft8* w, const float* llr, int n, const uint8_t* hyps, int H, const int32_t* pairs, int P,
                            const pysdr_ldpc_cfg* cfg, const pysdr_ap_cfg* apcfg, int32_t* ap, uint8_t* bits, int32_t* detail) {
  return ap_decode_llr(w, "pysdr_ft8_decode_llr_ap", llr, n, cfg, ApCall{hyps, H, pairs, P, apcfg, detail}, ap, bits);
}
int pysdr_ft8_report(pysdr_ft8* w, const int32_t* F, const long long* t0, const uint8_t* bits, int n, float* power, int32_t* errs) {
  return report_frames(w, "pysdr_ft8_report", F, t0, bits, n, power, errs);
}
int pysdr_ft8_floor(pysdr_ft8* w, long long t_end, int nsym, float* out) { return report_floor(w, "pysdr_ft8_floor", t_end, nsym, out); }
int pysdr_ft8_keep(pysdr_ft8* w, const pysdr_pass_cfg* cfg) { return pass_keep(w, "pysdr_ft8_keep", reinterpret_cast<const PassCfg*>(cfg)); }
int pysdr_ft8_subtract(pysdr_ft8* w, const int32_t* F, const long long* t0, const uint8_t* bits, const int32_t* trials, int n, int32_t* out) {
  return pass_subtract(w, "pysdr_ft8_subtract", F, t0, bits, trials, n, out);
}
int pysdr_ft8_rescan(pysdr_ft8* w, int F_lo, int F_hi, long long t_lo, long long t_hi, const pysdr_ft8_cfg* cfg, int32_t* counts,
                     int32_t* events) {
  return pass_rescan(w, "pysdr_ft8_rescan", F_lo, F_hi, t_lo, t_hi, ft_cfg(cfg), counts, events);
}
int pysdr_ft8_pass_decode(pysdr_ft8* w, const int32_t* F, const long long* t0, int n, const pysdr_ldpc_cfg* cfg, int32_t* status,
                          uint8_t* bits, float* post, const pysdr_osd_cfg* osd, int32_t* detail) {
  return pass_decode(w, "pysdr_ft8_pass_decode", F, t0, n, cfg, status, bits, post, osd, detail);
}
int pysdr_ft8_pass_llr(pysdr_ft8* w, const int32_t* F, const long long* t0, int n, float* out) {
  return ft_llr(w, "pysdr_ft8_pass_llr", F, t0, n, out, true);
}
int pysdr_ft8_pass_state(pysdr_ft8* w, float* yk, float* ring2, long long* kept) { return pass_state(w, "pysdr_ft8_pass_state", yk, ring2, kept); }

// ---- FT4 ---------------------------------------------------------------------------------------------------------------
int pysdr_ft4_plan(int nk, int S, int max_out, const pysdr_ft4_cfg* cfg, int32_t out[8]) {
  return ft_plan_call<Ft4Mode>("pysdr_ft4_plan", nk, S, max_out, ft_cfg(cfg), out);
}
int pysdr_ft4_create(pysdr_chan* ch, int S, const pysdr_ft4_cfg* cfg, const float* tw, int max_out, pysdr_ft4** out) {
  return ft_create("pysdr_ft4_create", "pysdr_ft4_plan", ch, S, ft_cfg(cfg), tw, max_out, out);
}
void pysdr_ft4_destroy(pysdr_ft4* w) { client_destroy(w); }
int pysdr_ft4_reset(pysdr_ft4* w) { return skimmer_reset(w, "pysdr_ft4_reset", ft_reset_locked<pysdr_ft4>); }
int pysdr_ft4_sync(pysdr_ft4* w) { return skimmer_sync(w, "pysdr_ft4_sync"); }
int pysdr_ft4_process(pysdr_ft4* w, const void* iq, int n, int on_device, int* n_out, int32_t* counts, int32_t* events,
                      long long ev_pitch, long long* steps) {
  return ft_process(w, "pysdr_ft4_process", iq, n, on_device, n_out, counts, events, ev_pitch, steps);
}
int pysdr_ft4_fetch(pysdr_ft4* w, const int* rows, int nrows, int32_t* events, long long pitch) {
  return skimmer_fetch(w, "pysdr_ft4_fetch", "fine row", rows, nrows, events, pitch);
}
int pysdr_ft4_llr(pysdr_ft4* w, const int32_t* F, const long long* t0, int n, float* out) { return ft_llr(w, "pysdr_ft4_llr", F, t0, n, out); }
int pysdr_ft4_state(pysdr_ft4* w, float* sc, int32_t* hits, float* ring, long long* t_done) {
  return ft_state(w, "pysdr_ft4_state", sc, hits, ring, t_done);
}
int pysdr_ft4_decode(pysdr_ft4* w, const int32_t* F, const long long* t0, int n, const pysdr_ldpc_cfg* cfg, int32_t* status, uint8_t* bits,
                     float* post) {
  return ldpc_decode_ring(w, "pysdr_ft4_decode", first_ring<std::remove_pointer_t<decltype(w)>>, F, t0, n, cfg, status, bits, post);
}
int pysdr_ft4_decode_llr(pysdr_ft4* w, const float* llr, int n, const pysdr_ldpc_cfg* cfg, int32_t* status, uint8_t* bits, float* post) {
  return ldpc_decode_llr(w, "pysdr_ft4_decode_llr", llr, n, cfg, status, bits, post);
}
int pysdr_ft4_decode_osd(pysdr_ft4* w, const int32_t* F, const long long* t0, int n, const pysdr_ldpc_cfg* cfg, int32_t* status,
                         uint8_t* bits, float* post, const pysdr_osd_cfg* osd, int32_t* detail) {
  return ldpc_decode_ring(w, "pysdr_ft4_decode_osd", first_ring<std::remove_pointer_t<decltype(w)>>, F, t0, n, cfg, status, bits, post, OsdCall{true, osd, detail});
}
int pysdr_ft4_decode_llr_osd(pysdr_ft4* w, const float* llr, int n, const pysdr_ldpc_cfg* cfg, int32_t* status, uint8_t* bits,
                             float* post, const pysdr_osd_cfg* osd, int32_t* detail) {
  return ldpc_decode_llr(w, "pysdr_ft4_decode_llr_osd", llr, n, cfg, status, bits, post, OsdCall{true, osd, detail});
}
int pysdr_ft4_decode_ap(pysdr_ft4* w, const int32_t* F, const long long* t0, int n, const uint8_t* hyps, int H, const int32_t* pairs, int P,
                        const pysdr_ldpc_cfg* cfg, const pysdr_ap_cfg* apcfg, int32_t* ap, uint8_t* bits, int32_t* detail) {
  return ap_decode_ring(w, "pysdr_ft4_decode_ap", F, t0, n, cfg, ApCall{hyps, H, pairs, P, apcfg, detail}, ap, bits);
}
int pysdr_ft4_decode_llr_ap(pysdr_ft4* w, const float* llr, int n, const uint8_t* hyps, int H, const int32_t* pairs, int P,
                            const pysdr_ldpc_cfg* cfg, const pysdr_ap_cfg* apcfg, int32_t* ap, uint8_t* bits, int32_t* detail) {
  return ap_decode_llr(w, "pysdr_ft4_decode_llr_ap", llr, n, cfg, ApCall{hyps, H, pairs, P, apcfg, detail}, ap, bits);
}
int pysdr_ft4_report(pysdr_ft4* w, const int32_t* F, const long long* t0, const uint8_t* bits, int n, float* power, int32_t* errs) {
  return report_frames(w, "pysdr_ft4_report", F, t0, bits, n, power, errs);
}
int pysdr_ft4_floor(pysdr_ft4* w, long long t_end, int nsym, float* out) { return report_floor(w, "pysdr_ft4_floor", t_end, nsym, out); }
int pysdr_ft4_keep(pysdr_ft4* w, const pysdr_pass_cfg* cfg) { return pass_keep(w, "pysdr_ft4_keep", reinterpret_cast<const PassCfg*>(cfg)); }
int pysdr_ft4_subtract(pysdr_ft4* w, const int32_t* F, const long long* t0, const uint8_t* bits, const int32_t* trials, int n, int32_t* out) {
  return pass_subtract(w, "pysdr_ft4_subtract", F, t0, bits, trials, n, out);
}
int pysdr_ft4_rescan(pysdr_ft4* w, int F_lo, int F_hi, long long t_lo, long long t_hi, const pysdr_ft4_cfg* cfg, int32_t* counts,
                     int32_t* events) {
  return pass_rescan(w, "pysdr_ft4_rescan", F_lo, F_hi, t_lo, t_hi, ft_cfg(cfg), counts, events);
}
int pysdr_ft4_pass_decode(pysdr_ft4* w, const int32_t* F, const long long* t0, int n, const pysdr_ldpc_cfg* cfg, int32_t* status,
                          uint8_t* bits, float* post, const pysdr_osd_cfg* osd, int32_t* detail) {
  return pass_decode(w, "pysdr_ft4_pass_decode", F, t0, n, cfg, status, bits, post, osd, detail);
}
int pysdr_ft4_pass_llr(pysdr_ft4* w, const int32_t* F, const long long* t0, int n, float* out) {
  return ft_llr(w, "pysdr_ft4_pass_llr", F, t0, n, out, true);
}
int pysdr_ft4_pass_state(pysdr_ft4* w, float* yk, float* ring2, long long* kept) { return pass_state(w, "pysdr_ft4_pass_state", yk, ring2, kept); }

// ---- the decoders' and the report's plans, which need no skimmer ---------------------------------------------------------
int pysdr_ldpc_plan(const pysdr_ldpc_cfg* cfg, int32_t out[4]) {
  if (!out) { set_last_error("pysdr_ldpc_plan: out is NULL"); return PYSDR_ERR_ARG; }
  if (!ldpc_cfg_ok(cfg)) {
    set_last_error("pysdr_ldpc_plan: a cfg outside the rules (NULL; iters in [1, %d]; alpha finite and in (0, 1])", kLdpcItersMax);
    return PYSDR_ERR_ARG;
  }
  out[0] = kLdpcThreads; out[1] = kLdpcLdsBytes; out[2] = kLdpcMax; out[3] = cfg->iters;
  return PYSDR_OK;
}

int pysdr_osd_plan(const pysdr_osd_cfg* cfg, int32_t out[4]) {
  if (!out) { set_last_error("pysdr_osd_plan: out is NULL"); return PYSDR_ERR_ARG; }
  if (!osd_cfg_ok(cfg)) {
    set_last_error("pysdr_osd_plan: a cfg outside the rule (NULL; order in [0, %d])", kOsdOrderMax);
    return PYSDR_ERR_ARG;
  }
  out[0] = kOsdThreads; out[1] = kOsdLdsBytes; out[2] = osd_patterns(cfg->order); out[3] = kLdpcMax;
  return PYSDR_OK;
}

int pysdr_ap_plan(const pysdr_ap_cfg* cfg, int32_t out[4]) {
  if (!out) { set_last_error("pysdr_ap_plan: out is NULL"); return PYSDR_ERR_ARG; }
  if (!ap_cfg_ok(cfg)) {
    set_last_error("pysdr_ap_plan: a cfg outside the rules (NULL; mag finite and in [%g, %g]; nerr_max in [0, %d])", (double)kApMagMin,
                   (double)kApMagMax, kLdpcN);
    return PYSDR_ERR_ARG;
  }
  out[0] = kLdpcThreads; out[1] = kApLdsBytes; out[2] = kApPairMax; out[3] = kApHypMax;
  return PYSDR_OK;
}

int pysdr_pass_plan(int mode, int nk, int S, int max_out, int reach_t, int32_t out[8]) {
  if (!out) { set_last_error("pysdr_pass_plan: out is NULL"); return PYSDR_ERR_ARG; }
  PassPlan p;
  const bool ok = mode == kReportFt8 ? pass_plan<Ft8Mode>(nk, S, max_out, reach_t, &p)
                                     : (mode == kReportFt4 ? pass_plan<Ft4Mode>(nk, S, max_out, reach_t, &p) : false);
  if (!ok) {
    set_last_error("pysdr_pass_plan: mode %d is neither PYSDR_REPORT_FT8 nor PYSDR_REPORT_FT4, S %d is not one of the mode's, nk %d < 1 or "
                   "nk S / 2 > %d, max_out %d outside [1, %d], reach_t %d outside [1, %d], or a ring above %lld bytes", mode, S, nk, kFtFineMax,
                   max_out, kFtMaxOutMax, reach_t, kPassReachMax, kFtRingBytesMax);
    return PYSDR_ERR_ARG;
  }
  out[0] = kPassThreads; out[1] = p.lds_bytes; out[2] = p.ty; out[3] = p.tr2; out[4] = kPassJobsMax; out[5] = kPassMax;
  out[6] = kPassEventCap; out[7] = mode == kReportFt8 ? kPassPulse<Ft8Mode> : kPassPulse<Ft4Mode>;
  return PYSDR_OK;
}

int pysdr_report_plan(int mode, int32_t out[4]) {
  if (!out) { set_last_error("pysdr_report_plan: out is NULL"); return PYSDR_ERR_ARG; }
  if (!report_plan(mode, out)) {
    set_last_error("pysdr_report_plan: mode %d is neither PYSDR_REPORT_FT8 nor PYSDR_REPORT_FT4", mode);
    return PYSDR_ERR_ARG;
  }
  return PYSDR_OK;
}

}  // extern "C"
