// C ABI of the CW skimmer (include/pysdr_hip.h).  Host-side only, like api_objects.hip: the kernel
// and its launch function live in cw.hip, what both sides share in cw_plan.h.  The skimmer borrows a channelizer as the
// channel bank does and queues its decoder behind the channelizer's launch on the channelizer's stream, with no host
// synchronisation in between.  Every device resource is an owner (host_res.h): deleting the object frees it.
#include "cw_plan.h"
#include "host_res.h"
#include "objects_plan.h"

using namespace pysdr;

struct pysdr_cw {
  pysdr_chan* ch = nullptr;         // borrowed; outlives the skimmer
  int device = 0, D = 0, nk = 0, max_in = 0, max_out = 0;   // of the channelizer, fixed at its create; max_out: ours
  hipStream_t stream = nullptr;     // the channelizer's
  pysdr_cw_cfg cfg{};
  CwPlan plan;
  int last_n_out = 0;
  DevBuf<float2> d_y;               // [nk][ypitch]
  DevBuf<CwState> d_state;          // [nk]
  DevBuf<int32_t> d_events;         // [nk][cap]
  DevBuf<int32_t> d_counts;         // [nk]
  std::vector<CwState> h_state;
  std::mutex mu;                    // one call at a time on a handle
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
  ChanInfo ci;
  int rc = chan_info(ch, &ci);
  if (rc != PYSDR_OK) return rc;
  int32_t pl[8];
  rc = pysdr_cw_plan(ci.nk, max_out, cfg, pl);
  if (rc != PYSDR_OK) return rc;
  pysdr_cw* w = new pysdr_cw();
  w->ch = ch; w->device = ci.device; w->D = ci.D; w->nk = ci.nk; w->max_in = ci.max_in; w->stream = ci.stream;
  w->max_out = max_out; w->cfg = *cfg;
  cw_plan(w->nk, max_out, cfg, &w->plan);
  rc = use_device(w->device);
  if (rc) { delete w; return rc; }
  rc = cw_alloc(w);
  if (rc) { failed_in("pysdr_cw_create", rc); pysdr_cw_destroy(w); return rc; }
  rc = cw_reset_locked(w);
  if (rc != PYSDR_OK) { pysdr_cw_destroy(w); return rc; }
  *out = w;
  return PYSDR_OK;
}

void pysdr_cw_destroy(pysdr_cw* w) {
  if (!w) return;
  (void)hipSetDevice(w->device);
  if (w->stream) (void)hipStreamSynchronize(w->stream);
  delete w;                               // (the owners free: host_res.h)
}

int pysdr_cw_reset(pysdr_cw* w) {
  if (!w) { set_last_error("pysdr_cw_reset: NULL skimmer"); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(w->mu);
  return cw_reset_locked(w);
}

int pysdr_cw_sync(pysdr_cw* w) {
  if (!w) { set_last_error("pysdr_cw_sync: NULL skimmer"); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(w->mu);
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  PYSDR_HIP_CHECK(hipStreamSynchronize(w->stream));
  return PYSDR_OK;
}

int pysdr_cw_process(pysdr_cw* w, const void* iq, int n, int on_device, int* n_out, int32_t* counts, int32_t* events,
                     long long ev_pitch) {
  if (!w || !n_out) { set_last_error("pysdr_cw_process: NULL skimmer or n_out"); return PYSDR_ERR_ARG; }
  *n_out = 0;
  std::lock_guard<std::mutex> lk(w->mu);
  if (n < 0 || (n > 0 && !iq)) { set_last_error("pysdr_cw_process: n %d / NULL input", n); return PYSDR_ERR_ARG; }
  if (n > w->max_in) { set_last_error("pysdr_cw_process: n %d > max_in %d", n, w->max_in); return PYSDR_ERR_STATE; }
  if (events && ev_pitch < w->plan.cap) {
    set_last_error("pysdr_cw_process: ev_pitch %lld < the event cap %d", ev_pitch, w->plan.cap);
    return PYSDR_ERR_STATE;
  }
  // what the channelizer is about to complete: checked before it advances its stream
  ChanInfo ci;
  int rc = chan_info(w->ch, &ci);
  if (rc != PYSDR_OK) return rc;
  const unsigned long long D = (unsigned long long)w->D, s0 = ci.n_abs, s1 = s0 + (unsigned long long)n;
  const unsigned long long nf_want = (s1 + D - 1) / D - (s0 + D - 1) / D;
  if (nf_want > (unsigned long long)w->max_out) {
    set_last_error("pysdr_cw_process: the call would complete %llu outputs, max_out is %d", nf_want, w->max_out);
    return PYSDR_ERR_STATE;
  }
  int nf = 0;
  rc = pysdr_chan_process(w->ch, iq, n, on_device, w->d_y.get(), w->plan.ypitch, 1, &nf);
  if (rc != PYSDR_OK) return rc;
  if (nf != (int)nf_want) { set_last_error("pysdr_cw_process: the channelizer was fed beside its skimmer (%d outputs, %d expected)", nf, (int)nf_want); return PYSDR_ERR_STATE; }
  w->last_n_out = nf;
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
  if (nrows < 0 || (nrows > 0 && (!rows || !events))) { set_last_error("pysdr_cw_fetch: nrows %d / NULL rows or events", nrows); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(w->mu);
  for (int i = 0; i < nrows; ++i)
    if (rows[i] < 0 || rows[i] >= w->nk) { set_last_error("pysdr_cw_fetch: row %d outside [0, %d)", rows[i], w->nk); return PYSDR_ERR_ARG; }
  const size_t cap = (size_t)w->plan.cap;
  if (pitch < (long long)cap) { set_last_error("pysdr_cw_fetch: pitch %lld < the event cap %d", pitch, w->plan.cap); return PYSDR_ERR_STATE; }
  if (w->last_n_out == 0 || nrows == 0) return PYSDR_OK;
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  for (int i = 0; i < nrows; ++i) {
    // runs of consecutive rows go as one strided copy
    int run = 1;
    while (i + run < nrows && rows[i + run] == rows[i] + run) ++run;
    PYSDR_HIP_CHECK(hipMemcpy2DAsync(events + (size_t)i * pitch, (size_t)pitch * sizeof(int32_t),
                                     w->d_events.get() + (size_t)rows[i] * cap, cap * sizeof(int32_t), cap * sizeof(int32_t),
                                     (size_t)run, hipMemcpyDeviceToHost, st));
    i += run - 1;
  }
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  return PYSDR_OK;
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
