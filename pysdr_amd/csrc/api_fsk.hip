// C ABI of the RTTY raster skimmer (include/pysdr_hip.h).  Host-side only, like api_psk.hip: the
// kernel and its launch function live in fsk.hip, what both sides share in fsk_plan.h.  The skimmer borrows a channelizer
// as the CW and PSK31 skimmers do (chan_client.h: what the channelizer's clients share) and queues its decoders behind
// the channelizer's launch on the channelizer's stream.  The call list is skimmer_host.h's, the skimmers' shared core;
// here is what only this kind has: its struct, buffers, tables, first state, plan, launch arguments, the two further
// outputs of a call and the state call.  Every device resource is an owner (host_res.h): deleting the object frees it.
#include "fsk_plan.h"
#include "skimmer_host.h"

using namespace pysdr;

struct pysdr_fsk : SkimmerBase {    // rows = nfine, words = cap
  pysdr_fsk_cfg cfg{};
  FskPlan plan;
  DevBuf<FskC> d_y;                 // [nk][ypitch]: kFskHpad of history room, then the call's outputs
  DevBuf<FskC> d_tw;                // [NT]
  DevBuf<float> d_g;                // [S]
  DevBuf<float> d_sf;               // [4][nfine]
  DevBuf<int32_t> d_si;             // [8][nfine]
  std::vector<float> h_tw, h_g;
  std::vector<int32_t> h_si;        // the state after create / reset
  FskC* feed_rows() { return d_y.get() + kFskHpad; }
};

namespace {

int fsk_alloc(pysdr_fsk* w) {
  const size_t nk = (size_t)w->nk, nf = (size_t)w->plan.nfine, S = (size_t)w->plan.S;
  PYSDR_HIP_CHECK(w->d_y.alloc(nk * (size_t)w->plan.ypitch));
  PYSDR_HIP_CHECK(w->d_tw.alloc(8 * S));
  PYSDR_HIP_CHECK(w->d_g.alloc(S));
  PYSDR_HIP_CHECK(w->d_sf.alloc((size_t)kFskStateFloats * nf));
  PYSDR_HIP_CHECK(w->d_si.alloc((size_t)kFskStateInts * nf));
  return skimmer_alloc(w);
}

int fsk_reset_locked(pysdr_fsk* w) {
  const int rc = pysdr_chan_reset(w->ch);
  if (rc != PYSDR_OK) return rc;
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  const size_t nk = (size_t)w->nk, nf = (size_t)w->plan.nfine;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));                          // the host arrays may still feed an earlier copy
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_tw.get(), w->h_tw.data(), w->h_tw.size() * sizeof(float), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_g.get(), w->h_g.data(), w->h_g.size() * sizeof(float), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_si.get(), w->h_si.data(), w->h_si.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_y.get(), 0, nk * (size_t)w->plan.ypitch * sizeof(FskC), st));   // y[k] = 0 for k < 0
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_sf.get(), 0, (size_t)kFskStateFloats * nf * sizeof(float), st));
  if (const int rc2 = skimmer_clear(w, st)) return rc2;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  w->last_n_out = 0;
  return PYSDR_OK;
}

}  // namespace

extern "C" {

int pysdr_fsk_plan(int nk, int S, int max_out, const pysdr_fsk_cfg* cfg, int32_t out[8]) {
  if (!out) { set_last_error("pysdr_fsk_plan: out is NULL"); return PYSDR_ERR_ARG; }
  FskPlan p;
  if (!fsk_plan(nk, S, max_out, cfg, &p)) {
    set_last_error("pysdr_fsk_plan: S %d is neither 22 nor 33, nk %d < 1 or nk S > %d, max_out %d outside [1, %d], or a cfg outside the "
                   "rules (NULL; a_q, a_b in (0, 1]; 0 < lo <= hi <= 1, 0 < bal <= 1, 0 < pmax <= 1e18, all finite; 1 <= n0 <= %d)", S, nk,
                   kFskFineMax, max_out, kFskMaxOutMax, kFskSettleMax);
    return PYSDR_ERR_ARG;
  }
  out[0] = fsk_rows(S); out[1] = fsk_threads(S); out[2] = fsk_lds_bytes(S); out[3] = kFskTile; out[4] = p.cap; out[5] = p.groups;
  out[6] = p.nsub; out[7] = 0;
  return PYSDR_OK;
}

int pysdr_fsk_create(pysdr_chan* ch, int S, const pysdr_fsk_cfg* cfg, const float* tw, const float* g, int max_out, pysdr_fsk** out) {
  return skimmer_create("pysdr_fsk_create", ch && cfg && tw && g, "NULL channelizer, cfg, tw or g", ch, max_out, out, fsk_alloc, fsk_reset_locked,
                        [&](pysdr_fsk* w) -> int {
    int32_t pl[8];
    if (!fsk_plan(w->nk, S, max_out, cfg, &w->plan)) return pysdr_fsk_plan(w->nk, S, max_out, cfg, pl);
    w->cfg = *cfg;
    w->rows = w->plan.nfine; w->words = w->plan.cap;
    w->h_tw.assign(tw, tw + 2 * 8 * (size_t)S);
    w->h_g.assign(g, g + (size_t)S);
    const size_t nf = (size_t)w->plan.nfine;
    w->h_si.assign((size_t)kFskStateInts * nf, 0);
    for (size_t i = 0; i < nf; ++i) { w->h_si[nf + i] = S; w->h_si[4 * nf + i] = 1; }   // cnt = S, prev = 1
    return PYSDR_OK;
  });
}

void pysdr_fsk_destroy(pysdr_fsk* w) { client_destroy(w); }
int pysdr_fsk_reset(pysdr_fsk* w) { return skimmer_reset(w, "pysdr_fsk_reset", fsk_reset_locked); }
int pysdr_fsk_sync(pysdr_fsk* w) { return skimmer_sync(w, "pysdr_fsk_sync"); }

int pysdr_fsk_process(pysdr_fsk* w, const void* iq, int n, int on_device, int* n_out, int32_t* counts, int32_t* events,
                      long long ev_pitch, float* qn, int32_t* open) {
  return skimmer_process(w, "pysdr_fsk_process", iq, n, on_device, n_out, counts, events, ev_pitch,
                         [&](const ClientStep& step, int nf, hipStream_t st) -> int {
    if (nf == 0) return PYSDR_OK;
    FskArgs a{};
    a.y = w->feed_rows(); a.ypitch = w->plan.ypitch; a.n_out = nf; a.nk = w->nk; a.cap = w->plan.cap; a.nfine = w->plan.nfine;
    a.m0_mod = (int)(step.m0 % (unsigned long long)(8 * w->plan.S));
    a.cfg = w->cfg; a.tw = w->d_tw.get(); a.g = w->d_g.get();
    a.sf = w->d_sf.get(); a.si = w->d_si.get(); a.events = w->d_events.get(); a.counts = w->d_counts.get();
    return launch_fsk_decode(w->plan.S, a, st);
  }, qn || open, [&](hipStream_t st) -> int {                          // the state as it stands, on an empty call too
    const size_t nfine = (size_t)w->plan.nfine;
    if (qn) PYSDR_HIP_CHECK(hipMemcpyAsync(qn, w->d_sf.get(), nfine * sizeof(float), hipMemcpyDeviceToHost, st));
    if (open) PYSDR_HIP_CHECK(hipMemcpyAsync(open, w->d_si.get() + kFskOpenAt * nfine, nfine * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    return PYSDR_OK;
  });
}

int pysdr_fsk_fetch(pysdr_fsk* w, const int* rows, int nrows, int32_t* events, long long pitch) {
  return skimmer_fetch(w, "pysdr_fsk_fetch", "fine row", rows, nrows, events, pitch);
}

int pysdr_fsk_state(pysdr_fsk* w, float* f, int32_t* ints) {
  if (!w) return no_skimmer("pysdr_fsk_state");
  std::lock_guard<std::mutex> lk(w->mu);
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  const size_t nf = (size_t)w->plan.nfine;
  if (f) PYSDR_HIP_CHECK(hipMemcpyAsync(f, w->d_sf.get(), (size_t)kFskStateFloats * nf * sizeof(float), hipMemcpyDeviceToHost, st));
  if (ints) PYSDR_HIP_CHECK(hipMemcpyAsync(ints, w->d_si.get(), (size_t)kFskStateInts * nf * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  return PYSDR_OK;
}

}  // extern "C"
