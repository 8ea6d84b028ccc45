// C ABI of the SSTV skimmer (include/pysdr_hip.h).  Host-side only, like api_pkt.hip: the kernel and
// its launch function live in sstv.hip, what both sides share in sstv_plan.h.  The skimmer borrows a channelizer as the
// other skimmers do (chan_client.h) and queues its decoders behind the channelizer's launch on the channelizer's stream.
// The call list is skimmer_host.h's, the skimmers' shared core; here is what only this kind has: its struct, buffers,
// tables, first state, plan, launch arguments and the state call.  Every device resource is an owner (host_res.h):
// deleting the object frees it.
#include "sstv_plan.h"
#include "skimmer_host.h"

using namespace pysdr;

struct pysdr_sstv : SkimmerBase {   // rows = nk, words = cap
  pysdr_sstv_cfg cfg{};
  SstvPlan plan;
  DevBuf<SstvC> d_y;                // [nk][ypitch]: kSstvHpad of history room, then the call's outputs
  DevBuf<SstvC> d_tw;               // [kSstvNt]
  DevBuf<float> d_g;                // [L]
  DevBuf<pysdr_sstv_cfg> d_cfg;     // [1]
  DevBuf<int32_t> d_si;             // [kSstvStateInts][nk]
  DevBuf<float> d_sf;               // [kSstvStateFloats][nk]
  DevBuf<float> d_ring;             // [nk][kSstvRing]
  DevBuf<uint32_t> d_lines;         // [nk][kSstvLineWords]
  std::vector<float> h_tw, h_g;
  std::vector<int32_t> h_si;        // the state after create / reset
  SstvC* feed_rows() { return d_y.get() + kSstvHpad; }
};

namespace {

int sstv_alloc(pysdr_sstv* w) {
  const size_t nk = (size_t)w->nk;
  PYSDR_HIP_CHECK(w->d_y.alloc(nk * (size_t)w->plan.ypitch));
  PYSDR_HIP_CHECK(w->d_tw.alloc(kSstvNt));
  PYSDR_HIP_CHECK(w->d_g.alloc((size_t)w->plan.L));
  PYSDR_HIP_CHECK(w->d_cfg.alloc(1));
  PYSDR_HIP_CHECK(w->d_si.alloc((size_t)kSstvStateInts * nk));
  PYSDR_HIP_CHECK(w->d_sf.alloc((size_t)kSstvStateFloats * nk));
  PYSDR_HIP_CHECK(w->d_ring.alloc((size_t)kSstvRing * nk));
  PYSDR_HIP_CHECK(w->d_lines.alloc((size_t)kSstvLineWords * nk));
  return skimmer_alloc(w);
}

int sstv_reset_locked(pysdr_sstv* w) {
  const int rc = pysdr_chan_reset(w->ch);
  if (rc != PYSDR_OK) return rc;
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  const size_t nk = (size_t)w->nk;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));                          // the host arrays may still feed an earlier copy
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_tw.get(), w->h_tw.data(), w->h_tw.size() * sizeof(float), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_g.get(), w->h_g.data(), w->h_g.size() * sizeof(float), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_cfg.get(), &w->cfg, sizeof(pysdr_sstv_cfg), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_si.get(), w->h_si.data(), w->h_si.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_sf.get(), 0, (size_t)kSstvStateFloats * nk * sizeof(float), st));
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_ring.get(), 0, (size_t)kSstvRing * nk * sizeof(float), st));
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_lines.get(), 0, (size_t)kSstvLineWords * nk * sizeof(uint32_t), st));
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_y.get(), 0, nk * (size_t)w->plan.ypitch * sizeof(SstvC), st));   // y[m] = 0 for m < 0
  if (const int rc2 = skimmer_clear(w, st)) return rc2;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  w->last_n_out = 0;
  return PYSDR_OK;
}

}  // namespace

extern "C" {

int pysdr_sstv_plan(int nk, int L, int max_out, const pysdr_sstv_cfg* cfg, int32_t out[8]) {
  if (!out) { set_last_error("pysdr_sstv_plan: out is NULL"); return PYSDR_ERR_ARG; }
  SstvPlan p;
  if (!sstv_plan(nk, L, max_out, cfg, &p)) {
    set_last_error("pysdr_sstv_plan: L %d outside [%d, %d], nk %d outside [1, %d], max_out %d outside [1, %d], nk times the event cap above 2^28 "
                   "words, or a cfg outside the rules (NULL; det 0 or 1; 0 < pmax <= 1e18; R0 in [80, 480] and one tick of w_tick; W = R0 / 5; "
                   "lag = 2 R0 + W + 1; k_hz = fs_out / 2 pi; k_rho = 1024 / fs_out; 1 to 16 modes of distinct codes in [0, 127], 1 to 4 scans, "
                   "1 to 800 pixels of at least one sample, 1 to 4096 lines of at least three and fewer than 2^16 samples)",
                   L, kSstvLmin, kSstvLmax, nk, kSstvRowsMax, max_out, kSstvMaxOutMax);
    return PYSDR_ERR_ARG;
  }
  out[0] = SstvGeom::kRows; out[1] = SstvGeom::kThreads; out[2] = SstvGeom::kLdsBytes; out[3] = kSstvTile; out[4] = p.cap; out[5] = p.groups;
  out[6] = p.H; out[7] = kSstvLineWords;
  return PYSDR_OK;
}

int pysdr_sstv_create(pysdr_chan* ch, int L, const pysdr_sstv_cfg* cfg, const float* tw, const float* g, int max_out, pysdr_sstv** out) {
  return skimmer_create("pysdr_sstv_create", ch && cfg && tw && g, "NULL channelizer, cfg, tw or g", ch, max_out, out, sstv_alloc, sstv_reset_locked,
                        [&](pysdr_sstv* w) -> int {
    int32_t pl[8];
    if (!sstv_plan(w->nk, L, max_out, cfg, &w->plan)) return pysdr_sstv_plan(w->nk, L, max_out, cfg, pl);
    w->cfg = *cfg;
    w->rows = w->nk; w->words = w->plan.cap;
    w->h_tw.assign(tw, tw + 2 * (size_t)kSstvNt);
    w->h_g.assign(g, g + (size_t)L);
    const size_t nk = (size_t)w->nk;
    w->h_si.assign((size_t)kSstvStateInts * nk, 0);
    for (size_t i = 0; i < nk; ++i) w->h_si[2 * nk + i] = -1;        // no mode yet
    return PYSDR_OK;
  });
}

void pysdr_sstv_destroy(pysdr_sstv* w) { client_destroy(w); }
int pysdr_sstv_reset(pysdr_sstv* w) { return skimmer_reset(w, "pysdr_sstv_reset", sstv_reset_locked); }
int pysdr_sstv_sync(pysdr_sstv* w) { return skimmer_sync(w, "pysdr_sstv_sync"); }

int pysdr_sstv_process(pysdr_sstv* w, const void* iq, int n, int on_device, int* n_out, int32_t* counts, int32_t* events,
                       long long ev_pitch) {
  return skimmer_process(w, "pysdr_sstv_process", iq, n, on_device, n_out, counts, events, ev_pitch,
                         [&](const ClientStep& step, int nf, hipStream_t st) -> int {
    if (nf == 0) return PYSDR_OK;
    SstvArgs a{};
    a.y = w->feed_rows(); a.ypitch = w->plan.ypitch; a.n_out = nf; a.nk = w->nk; a.cap = w->plan.cap; a.L = w->plan.L; a.H = w->plan.H;
    a.m0 = (uint32_t)step.m0;
    a.cfg = w->d_cfg.get(); a.tw = w->d_tw.get(); a.g = w->d_g.get();
    a.si = w->d_si.get(); a.sf = w->d_sf.get(); a.ring = w->d_ring.get(); a.lines = w->d_lines.get();
    a.events = w->d_events.get(); a.counts = w->d_counts.get();
    return launch_sstv_decode(a, st);
  });
}

int pysdr_sstv_fetch(pysdr_sstv* w, const int* rows, int nrows, int32_t* events, long long pitch) {
  return skimmer_fetch(w, "pysdr_sstv_fetch", "row", rows, nrows, events, pitch);
}

int pysdr_sstv_state(pysdr_sstv* w, int32_t* ints, float* floats, float* ring, uint32_t* lines) {
  if (!w) return no_skimmer("pysdr_sstv_state");
  std::lock_guard<std::mutex> lk(w->mu);
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  const size_t nk = (size_t)w->nk;
  if (ints) PYSDR_HIP_CHECK(hipMemcpyAsync(ints, w->d_si.get(), (size_t)kSstvStateInts * nk * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (floats) PYSDR_HIP_CHECK(hipMemcpyAsync(floats, w->d_sf.get(), (size_t)kSstvStateFloats * nk * sizeof(float), hipMemcpyDeviceToHost, st));
  if (ring) PYSDR_HIP_CHECK(hipMemcpyAsync(ring, w->d_ring.get(), (size_t)kSstvRing * nk * sizeof(float), hipMemcpyDeviceToHost, st));
  if (lines) PYSDR_HIP_CHECK(hipMemcpyAsync(lines, w->d_lines.get(), (size_t)kSstvLineWords * nk * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  return PYSDR_OK;
}

}  // extern "C"
