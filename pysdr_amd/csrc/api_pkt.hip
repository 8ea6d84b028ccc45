// C ABI of the packet skimmer (include/pysdr_hip.h).  Host-side only, like api_fsk.hip: the kernel
// and its launch function live in pkt.hip, what both sides share in pkt_plan.h.  The skimmer borrows a channelizer as the
// other skimmers do (chan_client.h: what the channelizer's clients share) and queues its decoders behind the
// channelizer's launch on the channelizer's stream.  The call list is skimmer_host.h's, the skimmers' shared core; here is
// what only this kind has: its struct, buffers, tables, first state, plan, launch arguments and the state call.  Every
// device resource is an owner (host_res.h): deleting the object frees it.
#include "pkt_plan.h"
#include "skimmer_host.h"

using namespace pysdr;

struct pysdr_pkt : SkimmerBase {    // rows = ndec, words = cap
  pysdr_pkt_cfg cfg{};
  PktPlan plan;
  DevBuf<PktC> d_y;                 // [nk][ypitch]: kPktHpad of history room, then the call's outputs
  DevBuf<PktC> d_tw;                // [kPktNt]
  DevBuf<float> d_g;                // [L]
  DevBuf<float> d_gain;             // [kPktSlicers]
  DevBuf<int32_t> d_si;             // [kPktStateInts][ndec]
  DevBuf<uint32_t> d_frames;        // [ndec][kPktFrameWords]
  std::vector<float> h_tw, h_g, h_gain;
  std::vector<int32_t> h_si;        // the state after create / reset
  PktC* feed_rows() { return d_y.get() + kPktHpad; }
};

namespace {

int pkt_alloc(pysdr_pkt* w) {
  const size_t nk = (size_t)w->nk, nd = (size_t)w->plan.ndec;
  PYSDR_HIP_CHECK(w->d_y.alloc(nk * (size_t)w->plan.ypitch));
  PYSDR_HIP_CHECK(w->d_tw.alloc(kPktNt));
  PYSDR_HIP_CHECK(w->d_g.alloc((size_t)w->plan.L));
  PYSDR_HIP_CHECK(w->d_gain.alloc(kPktSlicers));
  PYSDR_HIP_CHECK(w->d_si.alloc((size_t)kPktStateInts * nd));
  PYSDR_HIP_CHECK(w->d_frames.alloc((size_t)kPktFrameWords * nd));
  return skimmer_alloc(w);
}

int pkt_reset_locked(pysdr_pkt* w) {
  const int rc = pysdr_chan_reset(w->ch);
  if (rc != PYSDR_OK) return rc;
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  const size_t nk = (size_t)w->nk, nd = (size_t)w->plan.ndec;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));                          // the host arrays may still feed an earlier copy
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_tw.get(), w->h_tw.data(), w->h_tw.size() * sizeof(float), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_g.get(), w->h_g.data(), w->h_g.size() * sizeof(float), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_gain.get(), w->h_gain.data(), w->h_gain.size() * sizeof(float), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_si.get(), w->h_si.data(), w->h_si.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_y.get(), 0, nk * (size_t)w->plan.ypitch * sizeof(PktC), st));   // y[m] = 0 for m < 0
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_frames.get(), 0, (size_t)kPktFrameWords * nd * sizeof(uint32_t), st));
  if (const int rc2 = skimmer_clear(w, st)) return rc2;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  w->last_n_out = 0;
  return PYSDR_OK;
}

}  // namespace

extern "C" {

int pysdr_pkt_plan(int nk, int L, int max_out, const pysdr_pkt_cfg* cfg, int32_t out[8]) {
  if (!out) { set_last_error("pysdr_pkt_plan: out is NULL"); return PYSDR_ERR_ARG; }
  PktPlan p;
  if (!pkt_plan(nk, L, max_out, cfg, &p)) {
    set_last_error("pysdr_pkt_plan: L %d outside [%d, %d], nk %d < 1 or 8 nk > %d, max_out %d outside [1, %d], or a cfg outside the rules "
                   "(NULL; every gain > 0, 0 < pmax <= 1e18, all finite; w_mark, w_space, w_baud > 0, w_baud <= 2^29; 1 <= pll_shift <= 4)",
                   L, kPktLmin, kPktLmax, nk, kPktDecMax, max_out, kPktMaxOutMax);
    return PYSDR_ERR_ARG;
  }
  out[0] = PktGeom::kRows; out[1] = PktGeom::kThreads; out[2] = PktGeom::kLdsBytes; out[3] = kPktTile; out[4] = p.cap; out[5] = p.groups;
  out[6] = kPktSlicers; out[7] = kPktFrameWords;
  return PYSDR_OK;
}

int pysdr_pkt_create(pysdr_chan* ch, int L, const pysdr_pkt_cfg* cfg, const float* tw, const float* g, int max_out, pysdr_pkt** out) {
  return skimmer_create("pysdr_pkt_create", ch && cfg && tw && g, "NULL channelizer, cfg, tw or g", ch, max_out, out, pkt_alloc, pkt_reset_locked,
                        [&](pysdr_pkt* w) -> int {
    int32_t pl[8];
    if (!pkt_plan(w->nk, L, max_out, cfg, &w->plan)) return pysdr_pkt_plan(w->nk, L, max_out, cfg, pl);
    w->cfg = *cfg;
    w->rows = w->plan.ndec; w->words = w->plan.cap;
    w->h_tw.assign(tw, tw + 2 * (size_t)kPktNt);
    w->h_g.assign(g, g + (size_t)L);
    w->h_gain.assign(cfg->gain, cfg->gain + kPktSlicers);
    const size_t nd = (size_t)w->plan.ndec;
    w->h_si.assign((size_t)kPktStateInts * nd, 0);
    for (size_t i = 0; i < nd; ++i) w->h_si[9 * nd + i] = kPktCrcInit;
    return PYSDR_OK;
  });
}

void pysdr_pkt_destroy(pysdr_pkt* w) { client_destroy(w); }
int pysdr_pkt_reset(pysdr_pkt* w) { return skimmer_reset(w, "pysdr_pkt_reset", pkt_reset_locked); }
int pysdr_pkt_sync(pysdr_pkt* w) { return skimmer_sync(w, "pysdr_pkt_sync"); }

int pysdr_pkt_process(pysdr_pkt* w, const void* iq, int n, int on_device, int* n_out, int32_t* counts, int32_t* events,
                      long long ev_pitch) {
  return skimmer_process(w, "pysdr_pkt_process", iq, n, on_device, n_out, counts, events, ev_pitch,
                         [&](const ClientStep& step, int nf, hipStream_t st) -> int {
    if (nf == 0) return PYSDR_OK;
    PktArgs a{};
    a.y = w->feed_rows(); a.ypitch = w->plan.ypitch; a.n_out = nf; a.nk = w->nk; a.cap = w->plan.cap; a.ndec = w->plan.ndec; a.L = w->plan.L;
    a.m0 = (uint32_t)step.m0;
    a.w_mark = w->cfg.w_mark; a.w_space = w->cfg.w_space; a.w_baud = w->cfg.w_baud; a.pll_shift = w->cfg.pll_shift; a.pmax = w->cfg.pmax;
    a.tw = w->d_tw.get(); a.g = w->d_g.get(); a.gain = w->d_gain.get();
    a.si = w->d_si.get(); a.frames = w->d_frames.get(); a.events = w->d_events.get(); a.counts = w->d_counts.get();
    return launch_pkt_decode(a, st);
  });
}

int pysdr_pkt_fetch(pysdr_pkt* w, const int* rows, int nrows, int32_t* events, long long pitch) {
  return skimmer_fetch(w, "pysdr_pkt_fetch", "decoder", rows, nrows, events, pitch);
}

int pysdr_pkt_state(pysdr_pkt* w, int32_t* ints, uint32_t* frames) {
  if (!w) return no_skimmer("pysdr_pkt_state");
  std::lock_guard<std::mutex> lk(w->mu);
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  const size_t nd = (size_t)w->plan.ndec;
  if (ints) PYSDR_HIP_CHECK(hipMemcpyAsync(ints, w->d_si.get(), (size_t)kPktStateInts * nd * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (frames) PYSDR_HIP_CHECK(hipMemcpyAsync(frames, w->d_frames.get(), (size_t)kPktFrameWords * nd * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  return PYSDR_OK;
}

}  // extern "C"
