// The frame report of the FT8 and FT4 skimmers: what the spectrum ring says about a frame whose
// 91 bits are known.  frame_report_kernel<MODE>, one workgroup of 128 threads per candidate, three phases with a barrier
// between them:
//   A  lanes below 91 lay the message's bits into the LDS, lanes below 83 one parity bit each: three 32-bit message words
//      against the generator's row, AND and population count;
//   B  lane k below the symbol count derives its symbol's tone from the codeword, reads the symbol's tones at the
//      candidate's own place and the sent tone at the eight places around it that the host's mask allows, and puts ten
//      floats into its place of ten columns in the LDS; two ballots per wave count the symbols whose sent tone lost;
//   C  ten lanes add one column each in ascending symbol order -- the fixed order is the definition -- and store it.
// A column's pitch in the LDS is odd, so the ten lanes of phase C meet no bank twice; in phase B a wave stores 64
// consecutive floats of a column.  ring_floor_kernel: one workgroup of 64 threads per row, a lane per bin, the steps of
// the span in ascending order.  The steps are report_plan.h's, the very functions the scalar transcription runs.
#include "objects_plan.h"
#include "report_plan.h"

namespace pysdr {

namespace {

template <int MODE>
__global__ __launch_bounds__(kReportThreads) void frame_report_kernel(const ReportArgs a) {
  constexpr int NS = ReportGeom<MODE>::kSyms;
  __shared__ float s_col[kReportCols * kReportPitch];
  __shared__ uint8_t s_cw[kReportCwBytes];
  __shared__ int s_cnt[4];
  const int cand = blockIdx.x, tid = threadIdx.x;
  if (cand >= a.n) return;                                 // the whole workgroup: no barrier is left behind
  const int32_t* c = a.cand + (size_t)cand * kReportCandWords;
  const int F = c[0], slot0 = c[1], mask = c[2];
  const uint32_t w0 = (uint32_t)c[3], w1 = (uint32_t)c[4], w2 = (uint32_t)c[5];

  if (tid < kLdpcK) s_cw[tid] = report_msg_bit(w0, w1, w2, tid);
  if (tid < kLdpcM) s_cw[kLdpcK + tid] = report_parity(w0, w1, w2, tid);
  __syncthreads();

  bool miss = false, sync = false;
  if (tid < NS) {
    float v[kReportCols];
    report_symbol<MODE>(a.ring, a.tr, a.nb, a.nsub, a.nfine, F, slot0, mask, s_cw, tid, v, &miss, &sync);
#pragma unroll
    for (int k = 0; k < kReportCols; ++k) s_col[k * kReportPitch + tid] = v[k];
  }
  const unsigned long long lost_data = __ballot(miss && !sync), lost_sync = __ballot(miss && sync);
  if ((tid & 63) == 0) {
    s_cnt[2 * (tid >> 6)] = __popcll(lost_data);
    s_cnt[2 * (tid >> 6) + 1] = __popcll(lost_sync);
  }
  __syncthreads();

  if (tid < kReportCols)
    a.power[(size_t)cand * kReportCols + tid] = report_column(s_col + tid * kReportPitch, NS, tid == kReportPlaces || ((mask >> tid) & 1));
  if (tid == kReportCols) {
    a.errs[2 * (size_t)cand] = s_cnt[0] + s_cnt[2];
    a.errs[2 * (size_t)cand + 1] = s_cnt[1] + s_cnt[3];
  }
}

__global__ __launch_bounds__(kFloorThreads) void ring_floor_kernel(const FloorArgs a) {
  const int row = blockIdx.x, b = threadIdx.x;
  if (row >= a.nk || b >= a.nb) return;
  a.out[(size_t)row * a.nb + b] = floor_bin(a.ring + (size_t)row * (size_t)a.tr * (size_t)a.nb, a.tr, a.nb, a.slot_end, a.nsym, b);
}

}  // namespace

int launch_frame_report(int mode, const ReportArgs& a, hipStream_t st) {
  if (a.n < 1) return PYSDR_OK;
  if (a.n > kReportMax || !a.ring || !a.cand || !a.power || !a.errs || a.tr < 1 || a.nb < 1 || a.nsub < 1 || a.nfine < 1) {
    set_last_error("launch_frame_report: n %d or a NULL array", a.n);
    return PYSDR_ERR_ARG;
  }
  if (mode == kReportFt8) hipLaunchKernelGGL(frame_report_kernel<kReportFt8>, dim3(a.n), dim3(kReportThreads), 0, st, a);
  else if (mode == kReportFt4) hipLaunchKernelGGL(frame_report_kernel<kReportFt4>, dim3(a.n), dim3(kReportThreads), 0, st, a);
  else {
    set_last_error("launch_frame_report: mode %d", mode);
    return PYSDR_ERR_ARG;
  }
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

int launch_ring_floor(const FloorArgs& a, hipStream_t st) {
  if (!a.ring || !a.out || a.nk < 1 || a.nb < 1 || a.nb > kFloorThreads || !floor_nsym_ok(a.nsym) || a.slot_end < 0 || a.slot_end >= a.tr ||
      kFtStepsPerSym * (a.nsym - 1) >= a.tr) {
    set_last_error("launch_ring_floor: %d rows of %d bins, %d symbols ending in slot %d of %d", a.nk, a.nb, a.nsym, a.slot_end, a.tr);
    return PYSDR_ERR_ARG;
  }
  hipLaunchKernelGGL(ring_floor_kernel, dim3(a.nk), dim3(kFloorThreads), 0, st, a);
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

}  // namespace pysdr
