// C ABI of the CW skimmer (include/pysdr_hip.h).  Host-side only, like api_objects.hip: the kernel
// and its launch function live in cw.hip, what both sides share in cw_plan.h.  The skimmer borrows a channelizer as the
// channel bank does (chan_client.h: what the channelizer's clients share) and queues its decoder behind the channelizer's
// launch on the channelizer's stream.  The call list is skimmer_host.h's, the skimmers' shared core; here is what only
// this kind has: its struct, buffers, first state, plan, launch arguments and state call.  Every device resource is an
// owner (host_res.h): deleting the object frees it.
#include "cw_plan.h"
#include "skimmer_host.h"

using namespace pysdr;

struct pysdr_cw : SkimmerBase {    // rows = nk, words = cap
  pysdr_cw_cfg cfg{};
  CwPlan plan;
  DevBuf<float2> d_y;               // [nk][ypitch]
  DevBuf<CwState> d_state;          // [nk]
  std::vector<CwState> h_state;
  float2* feed_rows() { return d_y.get(); }
};

namespace {

int cw_alloc(pysdr_cw* w) {
  const size_t nk = (size_t)w->nk;
  PYSDR_HIP_CHECK(w->d_y.alloc(nk * (size_t)w->plan.ypitch));
  PYSDR_HIP_CHECK(w->d_state.alloc(nk));
  return skimmer_alloc(w);
}

int cw_reset_locked(pysdr_cw* w) {
  const int rc = pysdr_chan_reset(w->ch);
  if (rc != PYSDR_OK) return rc;
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));                          // h_state may still feed an earlier copy
  w->h_state.assign((size_t)w->nk, cw_state_init(w->cfg));
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_state.get(), w->h_state.data(), w->h_state.size() * sizeof(CwState), hipMemcpyHostToDevice, st));
  if (const int rc2 = skimmer_clear(w, st)) return rc2;
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
  return skimmer_create("pysdr_cw_create", ch && cfg, "NULL channelizer or cfg", ch, max_out, out, cw_alloc, cw_reset_locked, [&](pysdr_cw* w) -> int {
    int32_t pl[8];
    if (!cw_plan(w->nk, max_out, cfg, &w->plan)) return pysdr_cw_plan(w->nk, max_out, cfg, pl);
    w->cfg = *cfg;
    w->rows = w->nk; w->words = w->plan.cap;
    return PYSDR_OK;
  });
}

void pysdr_cw_destroy(pysdr_cw* w) { client_destroy(w); }
int pysdr_cw_reset(pysdr_cw* w) { return skimmer_reset(w, "pysdr_cw_reset", cw_reset_locked); }
int pysdr_cw_sync(pysdr_cw* w) { return skimmer_sync(w, "pysdr_cw_sync"); }

int pysdr_cw_process(pysdr_cw* w, const void* iq, int n, int on_device, int* n_out, int32_t* counts, int32_t* events,
                     long long ev_pitch) {
  return skimmer_process(w, "pysdr_cw_process", iq, n, on_device, n_out, counts, events, ev_pitch, [&](const ClientStep&, int nf, hipStream_t st) -> int {
    if (nf == 0) return PYSDR_OK;
    CwArgs a{};
    a.y = w->feed_rows(); a.ypitch = w->plan.ypitch; a.n_out = nf; a.nk = w->nk; a.cap = w->plan.cap; a.cfg = w->cfg;
    a.state = w->d_state.get(); a.events = w->d_events.get(); a.counts = w->d_counts.get();
    return launch_cw_decode(a, st);
  });
}

int pysdr_cw_fetch(pysdr_cw* w, const int* rows, int nrows, int32_t* events, long long pitch) {
  return skimmer_fetch(w, "pysdr_cw_fetch", "row", rows, nrows, events, pitch);
}

int pysdr_cw_state(pysdr_cw* w, float* s, float* pk, float* nf, int32_t* ints) {
  if (!w) return no_skimmer("pysdr_cw_state");
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
