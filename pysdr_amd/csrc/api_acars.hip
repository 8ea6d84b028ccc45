// C ABI of the ACARS skimmer (include/pysdr_hip.h).  Host-side only, like api_pkt.hip: the kernel
// and its launch function live in acars.hip, what both sides share in acars_plan.h.  The skimmer borrows a channelizer as
// the other skimmers do (chan_client.h) and queues its decoders behind the channelizer's launch on the channelizer's
// stream.  The call list is skimmer_host.h's, the skimmers' shared core; here is what only this kind has: its struct,
// buffers, tables, plan, launch arguments and the state call.  Every device resource is an owner (host_res.h): deleting
// the object frees it.
#include "acars_plan.h"
#include "skimmer_host.h"

using namespace pysdr;

struct pysdr_acars : SkimmerBase {  // rows = nk, words = cap
  pysdr_acars_cfg cfg{};
  AcPlan plan;
  DevBuf<AcC> d_y;                  // [nk][ypitch]: kAcHpad of history room, then the call's outputs
  DevBuf<AcC> d_tw;                 // [kAcNt]
  DevBuf<AcC> d_c;                  // [NT]
  DevBuf<int32_t> d_si;             // [kAcStateInts][nk]
  DevBuf<uint32_t> d_frames;        // [nk][kAcFrameWords]
  std::vector<float> h_tw, h_c;
  AcC* feed_rows() { return d_y.get() + kAcHpad; }
};

namespace {

int acars_alloc(pysdr_acars* w) {
  const size_t nk = (size_t)w->nk;
  PYSDR_HIP_CHECK(w->d_y.alloc(nk * (size_t)w->plan.ypitch));
  PYSDR_HIP_CHECK(w->d_tw.alloc(kAcNt));
  PYSDR_HIP_CHECK(w->d_c.alloc((size_t)w->plan.NT));
  PYSDR_HIP_CHECK(w->d_si.alloc((size_t)kAcStateInts * nk));
  PYSDR_HIP_CHECK(w->d_frames.alloc((size_t)kAcFrameWords * nk));
  return skimmer_alloc(w);
}

int acars_reset_locked(pysdr_acars* w) {
  const int rc = pysdr_chan_reset(w->ch);
  if (rc != PYSDR_OK) return rc;
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  const size_t nk = (size_t)w->nk;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));                          // the host arrays may still feed an earlier copy
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_tw.get(), w->h_tw.data(), w->h_tw.size() * sizeof(float), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_c.get(), w->h_c.data(), w->h_c.size() * sizeof(float), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_si.get(), 0, (size_t)kAcStateInts * nk * sizeof(int32_t), st));
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_y.get(), 0, nk * (size_t)w->plan.ypitch * sizeof(AcC), st));   // y[m] = 0 for m < 0
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_frames.get(), 0, (size_t)kAcFrameWords * nk * sizeof(uint32_t), st));
  if (const int rc2 = skimmer_clear(w, st)) return rc2;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  w->last_n_out = 0;
  return PYSDR_OK;
}

}  // namespace

extern "C" {

int pysdr_acars_plan(int nk, int L, int max_out, const pysdr_acars_cfg* cfg, int32_t out[8]) {
  if (!out) { set_last_error("pysdr_acars_plan: out is NULL"); return PYSDR_ERR_ARG; }
  AcPlan p;
  if (!acars_plan(nk, L, max_out, cfg, &p)) {
    set_last_error("pysdr_acars_plan: L %d outside [%d, %d], nk %d outside [1, %d], max_out %d outside [1, %d], or a cfg outside the rules "
                   "(NULL; 0 < pmax <= 1e18, finite; w_car, w_baud > 0, w_baud <= 2^29; 1 <= pll_shift <= 4)",
                   L, kAcLmin, kAcLmax, nk, kAcRowsMax, max_out, kAcMaxOutMax);
    return PYSDR_ERR_ARG;
  }
  out[0] = AcGeom::kRows; out[1] = AcGeom::kThreads; out[2] = AcGeom::kLdsBytes; out[3] = kAcTile; out[4] = p.cap; out[5] = p.groups;
  out[6] = p.NT; out[7] = kAcFrameWords;
  return PYSDR_OK;
}

int pysdr_acars_create(pysdr_chan* ch, int L, const pysdr_acars_cfg* cfg, const float* tw, const float* c, int max_out, pysdr_acars** out) {
  return skimmer_create("pysdr_acars_create", ch && cfg && tw && c, "NULL channelizer, cfg, tw or c", ch, max_out, out, acars_alloc,
                        acars_reset_locked, [&](pysdr_acars* w) -> int {
    int32_t pl[8];
    if (!acars_plan(w->nk, L, max_out, cfg, &w->plan)) return pysdr_acars_plan(w->nk, L, max_out, cfg, pl);
    w->cfg = *cfg;
    w->rows = w->nk; w->words = w->plan.cap;
    w->h_tw.assign(tw, tw + 2 * (size_t)kAcNt);
    w->h_c.assign(c, c + 2 * (size_t)w->plan.NT);
    return PYSDR_OK;
  });
}

void pysdr_acars_destroy(pysdr_acars* w) { client_destroy(w); }
int pysdr_acars_reset(pysdr_acars* w) { return skimmer_reset(w, "pysdr_acars_reset", acars_reset_locked); }
int pysdr_acars_sync(pysdr_acars* w) { return skimmer_sync(w, "pysdr_acars_sync"); }

int pysdr_acars_process(pysdr_acars* w, const void* iq, int n, int on_device, int* n_out, int32_t* counts, int32_t* events,
                        long long ev_pitch) {
  return skimmer_process(w, "pysdr_acars_process", iq, n, on_device, n_out, counts, events, ev_pitch,
                         [&](const ClientStep& step, int nf, hipStream_t st) -> int {
    if (nf == 0) return PYSDR_OK;
    AcArgs a{};
    a.y = w->feed_rows(); a.ypitch = w->plan.ypitch; a.n_out = nf; a.nk = w->nk; a.cap = w->plan.cap; a.L = w->plan.L;
    a.m0 = (uint32_t)step.m0;
    a.w_car = w->cfg.w_car; a.w_baud = w->cfg.w_baud; a.pll_shift = w->cfg.pll_shift; a.pmax = w->cfg.pmax;
    a.tw = w->d_tw.get(); a.c = w->d_c.get();
    a.si = w->d_si.get(); a.frames = w->d_frames.get(); a.events = w->d_events.get(); a.counts = w->d_counts.get();
    return launch_acars_decode(a, st);
  });
}

int pysdr_acars_fetch(pysdr_acars* w, const int* rows, int nrows, int32_t* events, long long pitch) {
  return skimmer_fetch(w, "pysdr_acars_fetch", "row", rows, nrows, events, pitch);
}

int pysdr_acars_state(pysdr_acars* w, int32_t* ints, uint32_t* frames) {
  if (!w) return no_skimmer("pysdr_acars_state");
  std::lock_guard<std::mutex> lk(w->mu);
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  const size_t nk = (size_t)w->nk;
  if (ints) PYSDR_HIP_CHECK(hipMemcpyAsync(ints, w->d_si.get(), (size_t)kAcStateInts * nk * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (frames) PYSDR_HIP_CHECK(hipMemcpyAsync(frames, w->d_frames.get(), (size_t)kAcFrameWords * nk * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  return PYSDR_OK;
}

}  // extern "C"
