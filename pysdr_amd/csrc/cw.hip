// CW skimmer: one Morse decoder per row of the channelizer's channel-major output.  The
// recurrences are nonlinear and the definition fixes their order, so one lane owns one channel and walks its samples in
// order; a workgroup is one wave that owns 64 consecutive rows.  Tiles of [64 rows][32 samples] go through the LDS: the
// loads run along the rows (a half-wave reads 256 contiguous bytes), the lanes then read their own row column by column,
// the odd row stride keeping the 32 lanes of a half-wave on 32 different pairs of banks.  The next tile's loads are in
// flight in registers while the lanes walk the current one.  The channel state lives in registers for the call and is
// written back once; events go to the channel's own slots with plain stores, their count once at the end.
#include "cw_plan.h"
#include "objects_plan.h"

namespace pysdr {

namespace {

__global__ __launch_bounds__(kCwThreads) void cw_kernel(const CwArgs a) {
  __shared__ float2 tile[kCwRows * kCwStride];
  const int lane = threadIdx.x;
  const int row0 = blockIdx.x * kCwRows;
  const int row = row0 + lane;
  const bool mine = row < a.nk;
  const float2* __restrict__ Y = static_cast<const float2*>(a.y);
  const pysdr_cw_cfg cfg = a.cfg;

  CwState z = cw_state_init(cfg);
  if (mine) z = a.state[row];
  int32_t* __restrict__ ev = a.events + (size_t)(mine ? row : 0) * (size_t)a.cap;
  int cnt = 0;

  float2 pre[kCwLoads];
  auto fetch = [&](int i0) {
#pragma unroll
    for (int it = 0; it < kCwLoads; ++it) {
      const int r = row0 + cw_stage_row(it, lane), i = i0 + cw_stage_col(it, lane);
      pre[it] = (r < a.nk && i < a.n_out) ? Y[(size_t)r * (size_t)a.ypitch + i] : make_float2(0.f, 0.f);
    }
  };
  fetch(0);
  for (int i0 = 0; i0 < a.n_out; i0 += kCwTile) {
    __syncthreads();                                     // the lanes are done with the previous tile
#pragma unroll
    for (int it = 0; it < kCwLoads; ++it) tile[cw_stage_row(it, lane) * kCwStride + cw_stage_col(it, lane)] = pre[it];
    __syncthreads();
    if (i0 + kCwTile < a.n_out) fetch(i0 + kCwTile);
    const int nj = a.n_out - i0 < kCwTile ? a.n_out - i0 : kCwTile;   // the last tile may be partial
    for (int j = 0; j < nj; ++j) {
      const float2 y = tile[lane * kCwStride + j];
      const int e = cw_step(z, cfg, y.x, y.y);
      if (e >= 0 && mine && cnt < a.cap) ev[cnt++] = cw_pack(i0 + j, e);
    }
  }
  if (mine) {
    a.state[row] = z;
    a.counts[row] = cnt;
  }
}

}  // namespace

int launch_cw_decode(const CwArgs& a, hipStream_t st) {
  if (a.n_out < 1 || a.nk < 1) return PYSDR_OK;
  const int groups = (a.nk + kCwRows - 1) / kCwRows;
  hipLaunchKernelGGL(cw_kernel, dim3(groups), dim3(kCwThreads), 0, st, a);
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

}  // namespace pysdr
