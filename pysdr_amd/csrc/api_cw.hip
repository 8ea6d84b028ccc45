// C ABI of the CW skimmer (include/pysdr_hip.h).  Host-side only, like api_objects.hip: the kernel
// and its launch function live in cw.hip, what both sides share in cw_plan.h.  The skimmer borrows a channelizer as the
// channel bank does (chan_client.h: what the channelizer's clients share) and queues its decoder behind the channelizer's
// launch on the channelizer's stream.  Every device resource is an owner (host_res.h): deleting the object frees it.
#include "chan_client.h"
#include "cw_plan.h"

using namespace pysdr;

struct pysdr_cw : ChanClient {
  int max_out = 0;
  pysdr_cw_cfg cfg{};
  CwPlan plan;
  DevBuf<float2> d_y;               // [nk][ypitch]
  DevBuf<CwState> d_state;          // [nk]
  DevBuf<int32_t> d_events;         // [nk][cap]
  DevBuf<int32_t> d_counts;         // [nk]
  std::vector<CwState> h_state;
};

namespace {

int cw_alloc(pysdr_cw* w) {
  const size_t nk = (size_t)w->nk;
  PYSDR_HIP_CHECK(w->d_y.alloc(nk * (size_t)w->plan.ypitch));
  PYSDR_HIP_CHECK(w->d_state.alloc(nk));
  PYSDR_HIP_CHECK(w->d_events.alloc(nk * (size_t)w->plan.cap));
  PYSDR_HIP_CHECK(w->d_counts.alloc(nk));
  return PYSDR_OK;
}

int cw_reset_locked(pysdr_cw* w) {
  const int rc = pysdr_chan_reset(w->ch);
  if (rc != PYSDR_OK) return rc;
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));                          // h_state may still feed an earlier copy
  w->h_state.assign((size_t)w->nk, cw_state_init(w->cfg));
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_state.get(), w->h_state.data(), w->h_state.size() * sizeof(CwState), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_counts.get(), 0, (size_t)w->nk * sizeof(int32_t), st));
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_events.get(), 0, (size_t)w->nk * w->plan.cap * sizeof(int32_t), st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  w->last_n_out = 0;
  return PYSDR_OK;
}

}  // namespace

extern "C" {

int pysdr_cw_plan(int nk, int max_out, const pysdr_cw_cfg* cfg, int32_t out[8]) {
  if (!out) { set_last_error("pysdr_cw_plan: out is NULL"); return PYSDR_ERR_ARG; }
  CwPlan p;
  if (!cw_plan(nk, max_out, cfg, &p)) {
    set_last_error("pysdr_cw_plan: nk %d outside [1, %d], max_out %d outside [1, %d], or a cfg outside the rules (NULL; a_s, a_p, a_n "
                   "in (0, 1]; snr_min, hi >= lo, fl > 0 and finite; %d <= dmin <= d0 <= dmax <= %d; 1 <= n0 <= %d)", nk, kCwNkMax, max_out,
                   kCwMaxOutMax, kCwDotMin, kCwDotMax, kCwSettleMax);
    return PYSDR_ERR_ARG;
  }
  out[0] = kCwRows; out[1] = kCwThreads; out[2] = kCwLdsBytes; out[3] = kCwTile; out[4] = p.cap; out[5] = p.groups;
  out[6] = 0; out[7] = 0;
  return PYSDR_OK;
}

int pysdr_cw_create(pysdr_chan* ch, const pysdr_cw_cfg* cfg, int max_out, pysdr_cw** out) {
  if (!out) { set_last_error("pysdr_cw_create: out is NULL"); return PYSDR_ERR_ARG; }
  *out = nullptr;
  if (!ch || !cfg) { set_last_error("pysdr_cw_create: NULL channelizer or cfg"); return PYSDR_ERR_ARG; }
  pysdr_cw* w = new pysdr_cw();
  int32_t pl[8];
  int rc = client_bind(w, ch);
  if (rc == PYSDR_OK) rc = pysdr_cw_plan(w->nk, max_out, cfg, pl);
  if (rc != PYSDR_OK) { delete w; return rc; }
  w->max_out = max_out; w->cfg = *cfg;
  cw_plan(w->nk, max_out, cfg, &w->plan);
  return client_create(w, "pysdr_cw_create", cw_alloc, cw_reset_locked, out);
}

void pysdr_cw_destroy(pysdr_cw* w) { client_destroy(w); }

int pysdr_cw_reset(pysdr_cw* w) {
  if (!w) { set_last_error("pysdr_cw_reset: NULL skimmer"); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(w->mu);
  return cw_reset_locked(w);
}

int pysdr_cw_sync(pysdr_cw* w) {
  if (!w) { set_last_error("pysdr_cw_sync: NULL skimmer"); return PYSDR_ERR_ARG; }
  return client_sync(w);
}

int pysdr_cw_process(pysdr_cw* w, const void* iq, int n, int on_device, int* n_out, int32_t* counts, int32_t* events,
                     long long ev_pitch) {
  if (!w || !n_out) { set_last_error("pysdr_cw_process: NULL skimmer or n_out"); return PYSDR_ERR_ARG; }
  *n_out = 0;
  std::lock_guard<std::mutex> lk(w->mu);
  ClientStep step;
  int rc = client_begin(w, "pysdr_cw_process", iq, n, &step);
  if (rc != PYSDR_OK) return rc;
  if (events && ev_pitch < w->plan.cap) {
    set_last_error("pysdr_cw_process: ev_pitch %lld < the event cap %d", ev_pitch, w->plan.cap);
    return PYSDR_ERR_STATE;
  }
  if (step.nf_want > (unsigned long long)w->max_out) {
    set_last_error("pysdr_cw_process: the call would complete %llu outputs, max_out is %d", step.nf_want, w->max_out);
    return PYSDR_ERR_STATE;
  }
  int nf = 0;
  rc = client_feed(w, "pysdr_cw_process", "skimmer", iq, n, on_device, w->d_y.get(), w->plan.ypitch, step, &nf);
  if (rc != PYSDR_OK) return rc;
  if (nf == 0) {                                                       // no output: nothing launched, no state change, no event
    if (counts) std::memset(counts, 0, (size_t)w->nk * sizeof(int32_t));
    return PYSDR_OK;
  }
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  CwArgs a{};
  a.y = w->d_y.get(); a.ypitch = w->plan.ypitch; a.n_out = nf; a.nk = w->nk; a.cap = w->plan.cap; a.cfg = w->cfg;
  a.state = w->d_state.get(); a.events = w->d_events.get(); a.counts = w->d_counts.get();
  rc = launch_cw_decode(a, st);
  if (rc) return rc;
  *n_out = nf;
  if (counts) PYSDR_HIP_CHECK(hipMemcpyAsync(counts, a.counts, (size_t)w->nk * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (events)
    PYSDR_HIP_CHECK(hipMemcpy2DAsync(events, (size_t)ev_pitch * sizeof(int32_t), a.events, (size_t)a.cap * sizeof(int32_t),
                                     (size_t)a.cap * sizeof(int32_t), (size_t)w->nk, hipMemcpyDeviceToHost, st));
  if (counts || events || !on_device) PYSDR_HIP_CHECK(hipStreamSynchronize(st));   // host buffers are the caller's again
  return PYSDR_OK;
}

int pysdr_cw_fetch(pysdr_cw* w, const int* rows, int nrows, int32_t* events, long long pitch) {
  if (!w) { set_last_error("pysdr_cw_fetch: NULL skimmer"); return PYSDR_ERR_ARG; }
  return client_fetch_events(w, "pysdr_cw_fetch", "row", w->d_events.get(), w->nk, w->plan.cap, rows, nrows, events, pitch);
}

int pysdr_cw_state(pysdr_cw* w, float* s, float* pk, float* nf, int32_t* ints) {
  if (!w) { set_last_error("pysdr_cw_state: NULL skimmer"); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(w->mu);
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->h_state.data(), w->d_state.get(), w->h_state.size() * sizeof(CwState), hipMemcpyDeviceToHost, st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  for (int i = 0; i < w->nk; ++i) {
    const CwState& z = w->h_state[(size_t)i];
    if (s) s[i] = z.s;
    if (pk) pk[i] = z.pk;
    if (nf) nf[i] = z.nf;
    if (ints) {
      int32_t* o = ints + 8 * (size_t)i;
      o[0] = z.key; o[1] = z.run; o[2] = z.dot; o[3] = z.last; o[4] = z.code; o[5] = z.nel; o[6] = z.sp; o[7] = z.seen;
    }
  }
  return PYSDR_OK;
}

}  // extern "C"
