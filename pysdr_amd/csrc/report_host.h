// The host half of the frame report and the row floor, shared by the FT8 and the FT4 skimmer
// (api_ft.hip) over skimmer_host.h as ldpc_host.h is: the buffers a skimmer owns for it, and the two calls,
// written once for both objects, which name their fields alike (plan, t_done, d_ring).  The mask of places a candidate may
// read is computed here, per candidate, by report_plan.h's pure function.  Every check comes before any launch: a refusal
// changes nothing.  Host only; not part of the public ABI.
#pragma once

#include "report_plan.h"
#include "skimmer_host.h"

namespace pysdr {

struct ReportBufs {                 // allocated by the first report or floor call of a skimmer
  DevBuf<int32_t> d_cand;           // [kReportMax][6]
  DevBuf<float> d_power;            // [kReportMax][10]
  DevBuf<int32_t> d_errs;           // [kReportMax][2]
  DevBuf<float> d_floor;            // [nk][nb]
  std::vector<int32_t> h_cand;
  bool ready = false;
};

inline int report_bufs_ready(ReportBufs* b, int nk, int nb) {
  if (b->ready) return PYSDR_OK;
  PYSDR_HIP_CHECK(b->d_cand.alloc((size_t)kReportMax * kReportCandWords));
  PYSDR_HIP_CHECK(b->d_power.alloc((size_t)kReportMax * kReportCols));
  PYSDR_HIP_CHECK(b->d_errs.alloc((size_t)kReportMax * 2));
  PYSDR_HIP_CHECK(b->d_floor.alloc((size_t)nk * (size_t)nb));
  b->h_cand.reserve((size_t)kReportMax * kReportCandWords);
  b->ready = true;
  return PYSDR_OK;
}

// Candidates (F[i], t0[i]) with their message bits.  The skimmer's mode (W::Mode, ft_plan.h) gives the rule for a
// candidate, the last step of a frame behind its first and the kernel's mode.
template <class W>
int report_frames(W* w, const char* who, const int32_t* F, const long long* t0, const uint8_t* bits, int n, float* power, int32_t* errs) {
  using Mode = typename W::Mode;
  constexpr int lag = kFtLag<Mode>;
  if (!w) return no_skimmer(who);
  if (!report_n_ok(n) || (n > 0 && (!F || !t0 || !bits || !power || !errs))) {
    set_last_error("%s: n %d outside [0, %d] / NULL F, t0, bits, power or errs", who, n, kReportMax);
    return PYSDR_ERR_ARG;
  }
  std::lock_guard<std::mutex> lk(w->mu);
  const long long done = (long long)w->t_done;
  for (int i = 0; i < n; ++i)                                          // every candidate first: a refusal changes nothing
    if (!ft_llr_ok<Mode>(F[i], t0[i], done, w->plan.nfine, w->plan.tr)) {
      set_last_error("%s: candidate %d (F %d, t0 %lld): F outside [0, %d), or a frame not yet complete or gone from the ring "
                     "(%lld steps done, its last is %lld, the ring holds %d)", who, i, (int)F[i], t0[i], w->plan.nfine, done, t0[i] + lag,
                     w->plan.tr);
      return F[i] < 0 || F[i] >= w->plan.nfine ? PYSDR_ERR_ARG : PYSDR_ERR_STATE;
    }
  if (n == 0) return PYSDR_OK;
  ChanInfo ci;
  int rc = chan_info(w->ch, &ci);
  if (rc != PYSDR_OK) return rc;
  const bool circular = ci.M == w->nk;                                 // the raster is the whole circle
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  rc = report_bufs_ready(&w->report, w->nk, w->plan.nb);
  if (rc) return rc;
  hipStream_t st = w->stream;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));                          // h_cand may still feed an earlier copy
  std::vector<int32_t>& hc = w->report.h_cand;
  hc.resize((size_t)n * kReportCandWords);
  for (int i = 0; i < n; ++i) {
    int32_t* c = hc.data() + (size_t)i * kReportCandWords;
    uint32_t m[3];
    report_words(bits + (size_t)i * kReportBitsBytes, m);
    c[0] = F[i];
    c[1] = (int32_t)(t0[i] % w->plan.tr);
    c[2] = report_mask(F[i], t0[i], done, w->plan.nfine, w->plan.tr, lag, circular);
    c[3] = (int32_t)m[0]; c[4] = (int32_t)m[1]; c[5] = (int32_t)m[2];
  }
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->report.d_cand.get(), hc.data(), hc.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  ReportArgs a{};
  a.ring = w->d_ring.get(); a.tr = w->plan.tr; a.nb = w->plan.nb; a.nsub = w->plan.nsub; a.nfine = w->plan.nfine; a.n = n;
  a.cand = w->report.d_cand.get(); a.power = w->report.d_power.get(); a.errs = w->report.d_errs.get();
  rc = launch_frame_report(Mode::kReportMode, a, st);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipMemcpyAsync(power, a.power, (size_t)n * kReportCols * sizeof(float), hipMemcpyDeviceToHost, st));
  PYSDR_HIP_CHECK(hipMemcpyAsync(errs, a.errs, (size_t)n * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  return PYSDR_OK;
}

// Every bin of every row summed over the nsym symbol steps that end at t_end.
template <class W>
int report_floor(W* w, const char* who, long long t_end, int nsym, float* out) {
  if (!w) return no_skimmer(who);
  if (!floor_nsym_ok(nsym) || !out) {
    set_last_error("%s: nsym %d outside [1, %d] / NULL out", who, nsym, kFloorSymsMax);
    return PYSDR_ERR_ARG;
  }
  std::lock_guard<std::mutex> lk(w->mu);
  const long long done = (long long)w->t_done;
  if (!floor_ok(t_end, nsym, done, w->plan.tr)) {
    set_last_error("%s: the steps %lld to %lld are not all complete and in the ring (%lld steps done, the ring holds %d)", who,
                   t_end - kFtStepsPerSym * (long long)(nsym - 1), t_end, done, w->plan.tr);
    return PYSDR_ERR_STATE;
  }
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  int rc = report_bufs_ready(&w->report, w->nk, w->plan.nb);
  if (rc) return rc;
  hipStream_t st = w->stream;
  FloorArgs a{};
  a.ring = w->d_ring.get(); a.tr = w->plan.tr; a.nb = w->plan.nb; a.nk = w->nk; a.slot_end = (int)(t_end % w->plan.tr); a.nsym = nsym;
  a.out = w->report.d_floor.get();
  rc = launch_ring_floor(a, st);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipMemcpyAsync(out, a.out, (size_t)w->nk * (size_t)w->plan.nb * sizeof(float), hipMemcpyDeviceToHost, st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  return PYSDR_OK;
}

}  // namespace pysdr
