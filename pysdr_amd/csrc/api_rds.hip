// C ABI of the RDS skimmer (include/pysdr_hip.h).  Host-side only, like api_pkt.hip: the kernel and
// its launch function live in rds.hip, what both sides share in rds_plan.h.  The skimmer borrows a channelizer as the
// other skimmers do (chan_client.h: what the channelizer's clients share) and queues its decoders behind the
// channelizer's launch on the channelizer's stream.  The call list is skimmer_host.h's, the skimmers' shared core; here is
// what only this kind has: its struct, buffers, tables, plan, launch arguments and the state call.  Every device resource
// is an owner (host_res.h): deleting the object frees it.
#include "rds_plan.h"
#include "skimmer_host.h"

using namespace pysdr;

struct pysdr_rds : SkimmerBase {    // rows = ndec, words = cap
  pysdr_rds_cfg cfg{};
  RdsPlan plan;
  DevBuf<RdsC> d_y;                 // [nk][ypitch]: kRdsHpad of history room, then the call's outputs
  DevBuf<RdsC> d_tw;                // [kRdsNt]
  DevBuf<float> d_g;                // [L]
  DevBuf<uint32_t> d_regs;          // [4][ndec]
  DevBuf<uint32_t> d_chips;         // [nk]
  DevBuf<RdsC> d_ring;              // [nk][kRdsPhases]
  std::vector<float> h_tw, h_g;
  RdsC* feed_rows() { return d_y.get() + kRdsHpad; }
};

namespace {

int rds_alloc(pysdr_rds* w) {
  const size_t nk = (size_t)w->nk, nd = (size_t)w->plan.ndec;
  PYSDR_HIP_CHECK(w->d_y.alloc(nk * (size_t)w->plan.ypitch));
  PYSDR_HIP_CHECK(w->d_tw.alloc(kRdsNt));
  PYSDR_HIP_CHECK(w->d_g.alloc((size_t)w->plan.L));
  PYSDR_HIP_CHECK(w->d_regs.alloc(4 * nd));
  PYSDR_HIP_CHECK(w->d_chips.alloc(nk));
  PYSDR_HIP_CHECK(w->d_ring.alloc(nd));
  return skimmer_alloc(w);
}

int rds_reset_locked(pysdr_rds* w) {
  const int rc = pysdr_chan_reset(w->ch);
  if (rc != PYSDR_OK) return rc;
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  const size_t nk = (size_t)w->nk, nd = (size_t)w->plan.ndec;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));                          // the host arrays may still feed an earlier copy
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_tw.get(), w->h_tw.data(), w->h_tw.size() * sizeof(float), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_g.get(), w->h_g.data(), w->h_g.size() * sizeof(float), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_y.get(), 0, nk * (size_t)w->plan.ypitch * sizeof(RdsC), st));   // y[m] = 0 for m < 0
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_regs.get(), 0, 4 * nd * sizeof(uint32_t), st));
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_chips.get(), 0, nk * sizeof(uint32_t), st));
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_ring.get(), 0, nd * sizeof(RdsC), st));
  if (const int rc2 = skimmer_clear(w, st)) return rc2;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  w->last_n_out = 0;
  return PYSDR_OK;
}

}  // namespace

extern "C" {

int pysdr_rds_plan(int nk, int L, int max_out, const pysdr_rds_cfg* cfg, int32_t out[8]) {
  if (!out) { set_last_error("pysdr_rds_plan: out is NULL"); return PYSDR_ERR_ARG; }
  RdsPlan p;
  if (!rds_plan(nk, L, max_out, cfg, &p)) {
    set_last_error("pysdr_rds_plan: L %d not odd in [%d, %d], nk %d < 1 or 16 nk > %d, max_out %d outside [1, %d], or a cfg outside the rules "
                   "(NULL; w19 in [%u, %u] and L = 2 floor((16 2^32 + 512) / w19) + 1)",
                   L, kRdsLmin, kRdsLmax, nk, kRdsDecMax, max_out, kRdsMaxOutMax, kRdsW19Min, kRdsW19Max);
    return PYSDR_ERR_ARG;
  }
  out[0] = RdsGeom::kRows; out[1] = RdsGeom::kThreads; out[2] = RdsGeom::kLdsBytes; out[3] = kRdsTile; out[4] = p.cap; out[5] = p.groups;
  out[6] = kRdsPhases; out[7] = p.nseg;
  return PYSDR_OK;
}

int pysdr_rds_create(pysdr_chan* ch, int L, const pysdr_rds_cfg* cfg, const float* tw, const float* g, int max_out, pysdr_rds** out) {
  return skimmer_create("pysdr_rds_create", ch && cfg && tw && g, "NULL channelizer, cfg, tw or g", ch, max_out, out, rds_alloc, rds_reset_locked,
                        [&](pysdr_rds* w) -> int {
    int32_t pl[8];
    if (!rds_plan(w->nk, L, max_out, cfg, &w->plan)) return pysdr_rds_plan(w->nk, L, max_out, cfg, pl);
    w->cfg = *cfg;
    w->rows = w->plan.ndec; w->words = w->plan.cap;
    w->h_tw.assign(tw, tw + 2 * (size_t)kRdsNt);
    w->h_g.assign(g, g + (size_t)L);
    return PYSDR_OK;
  });
}

void pysdr_rds_destroy(pysdr_rds* w) { client_destroy(w); }
int pysdr_rds_reset(pysdr_rds* w) { return skimmer_reset(w, "pysdr_rds_reset", rds_reset_locked); }
int pysdr_rds_sync(pysdr_rds* w) { return skimmer_sync(w, "pysdr_rds_sync"); }

int pysdr_rds_process(pysdr_rds* w, const void* iq, int n, int on_device, int* n_out, int32_t* counts, int32_t* events,
                      long long ev_pitch) {
  return skimmer_process(w, "pysdr_rds_process", iq, n, on_device, n_out, counts, events, ev_pitch,
                         [&](const ClientStep& step, int nf, hipStream_t st) -> int {
    if (nf == 0) return PYSDR_OK;
    RdsArgs a{};
    a.y = w->feed_rows(); a.ypitch = w->plan.ypitch; a.n_out = nf; a.nk = w->nk; a.cap = w->plan.cap; a.ndec = w->plan.ndec; a.L = w->plan.L;
    a.nseg = w->plan.nseg;
    a.m0 = (uint32_t)step.m0;
    a.w19 = w->cfg.w19;
    a.tw = w->d_tw.get(); a.g = w->d_g.get();
    a.regs = w->d_regs.get(); a.chips = w->d_chips.get(); a.ring = w->d_ring.get();
    a.events = w->d_events.get(); a.counts = w->d_counts.get();
    return launch_rds_decode(a, st);
  });
}

int pysdr_rds_fetch(pysdr_rds* w, const int* rows, int nrows, int32_t* events, long long pitch) {
  return skimmer_fetch(w, "pysdr_rds_fetch", "decoder", rows, nrows, events, pitch);
}

int pysdr_rds_state(pysdr_rds* w, uint32_t* regs, uint32_t* chips, float* ring) {
  if (!w) return no_skimmer("pysdr_rds_state");
  std::lock_guard<std::mutex> lk(w->mu);
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  const size_t nk = (size_t)w->nk, nd = (size_t)w->plan.ndec;
  if (regs) PYSDR_HIP_CHECK(hipMemcpyAsync(regs, w->d_regs.get(), 4 * nd * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (chips) PYSDR_HIP_CHECK(hipMemcpyAsync(chips, w->d_chips.get(), nk * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (ring) PYSDR_HIP_CHECK(hipMemcpyAsync(ring, w->d_ring.get(), nd * sizeof(RdsC), hipMemcpyDeviceToHost, st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  return PYSDR_OK;
}

}  // extern "C"
