// Polyphase channelizer: every channel k of an M-channel raster in one pass over the wideband input.
//   y_k[m] = sum_{i<L} h[i] x[mD - i] exp(-j 2 pi ((k (mD - i)) mod M) / M),   x[n] = 0 for n < 0, n and m absolute
// = NCO(-k fs/M) + RationalDecimator(h, 1, D) of the oracle for every k at once.  The polyphase form, with P = ceil(L/M)
// and h zero padded to P M taps:
//   v_m[r] = sum_{p<P} h[pM + r] x[mD - pM - r]                    (p ascending, one fma per tap and component)
//   y_k[m] = sum_r v_m[r] e^{+j 2 pi k (r - mD) / M}               = unnormalised inverse DFT of v_m rotated by mD mod M
// One kernel, chan_kernel<C, FI> (C = M/D): a workgroup owns `fw` consecutive frames m.
//   1. FIR: a work item is one branch r for FI consecutive frames.  Frame m and tap row p meet at x[(m - Cp) D - r], so the
//      item keeps a sliding register window of FI samples, shifts it by C per tap row and loads only C new samples: the
//      input comes from memory once, its re-use across work items from the L2.  No window is staged in LDS, so a 256 KB
//      window (M = 4096, 8 taps per branch) needs no special case.  v_m[r] goes to LDS at index (r - mD) mod M.
//   2. FFT: in-place decimation-in-frequency passes of radix 5 / 4 / 2 over all fw frames in LDS (fft_lds.h, shared with
//      fine.hip); twiddles from a table e^{+j 2 pi j / M} computed in float64 on the host.  The result is left in
//      digit-reversed order.
//   3. Store: row a = channel (k_first + a) mod M of the channel-major output takes its fw frames from LDS position
//      perm[a] (the digit reversal, a host table); consecutive lanes write consecutive frames of a row.
// No intermediate goes through memory; the only other launch of a call is the roll of the input history.
#include "fft_lds.h"
#include "objects_plan.h"

namespace pysdr {
namespace {

template <int C, int FI>
__global__ __launch_bounds__(1024) void chan_kernel(const ChanArgs a) {
  extern __shared__ float2 sm[];
  // Workgroups are dealt round-robin over the 8 XCDs, and neighbouring runs of frames share most of their input window:
  // the workgroups with the same blockIdx % 8 (one L2) take a contiguous eighth of the call (A/B: -DCHAN_PLAIN_ORDER).
#ifdef CHAN_PLAIN_ORDER
  const int wg = blockIdx.x;
#else
  const int xc = blockIdx.x & 7;
  const int wg = (xc < a.xr ? xc * (a.xq + 1) : a.xr * (a.xq + 1) + (xc - a.xr) * a.xq) + (blockIdx.x >> 3);
#endif
  const int f0 = wg * a.fw;                             // first frame of the workgroup, counted from the call's first
  // ---- 1. polyphase FIR into LDS
  const int nitems = a.M * (a.fw / FI);
  for (int i = threadIdx.x; i < nitems; i += blockDim.x) {
    const int g = (int)__umulhi((uint32_t)i, a.magic_M), r = i - g * a.M;
    const int fb = f0 + g * FI;
    // x[(t + mf) D - r] for a frame index t counted from the call's first (t < 0: frames of earlier calls); 0 outside
    // [s0 - H, s1), which no frame of this call reaches
    auto ld = [&](int t) -> float2 {
      const int rel = t * a.D + a.off0 - r;
      float2 v = make_float2(0.f, 0.f);
      if (rel >= -a.H && rel < a.n) v = rel >= 0 ? a.x[rel] : a.hist[a.H + rel];
      return v;
    };
    float2 X[FI], acc[FI];
#pragma unroll
    for (int f = 0; f < FI; ++f) {
      X[f] = ld(fb + f);
      acc[f] = make_float2(0.f, 0.f);
    }
    for (int p = 0; p < a.P; ++p) {
      const float h = a.taps[p * a.M + r];
#pragma unroll
      for (int f = 0; f < FI; ++f) {
        acc[f].x = __builtin_fmaf(h, X[f].x, acc[f].x);
        acc[f].y = __builtin_fmaf(h, X[f].y, acc[f].y);
      }
      if (p + 1 < a.P) {                                // tap row p + 1 of frame f reads what row p of frame f - C read
#pragma unroll
        for (int f = FI - 1; f >= C; --f) X[f] = X[f - C];
#pragma unroll
        for (int f = 0; f < (C < FI ? C : FI); ++f) X[f] = ld(fb + f - C * (p + 1));
      }
    }
#pragma unroll
    for (int f = 0; f < FI; ++f) {
      int q = r - ((a.mf_lo + fb + f) & (C - 1)) * a.D;   // (r - m D) mod M
      if (q < 0) q += a.M;
      sm[(g * FI + f) * a.mp + q] = acc[f];
    }
  }
  __syncthreads();
  // ---- 2. inverse DFT of every frame, in place, digit-reversed result
  int nb = a.M;
  for (int s = 0; s < a.fft.npass; ++s) {
    const int R = a.fft.radix[s];
    if (R == 4) fft_pass<4>(sm, a.tw, a.M, a.mp, a.fw, nb, a.fft.magic_per[s], a.fft.magic_nq[s]);
    else if (R == 5) fft_pass<5>(sm, a.tw, a.M, a.mp, a.fw, nb, a.fft.magic_per[s], a.fft.magic_nq[s]);
    else fft_pass<2>(sm, a.tw, a.M, a.mp, a.fw, nb, a.fft.magic_per[s], a.fft.magic_nq[s]);
    nb /= R;
    __syncthreads();
  }
  // ---- 3. channel-major store: consecutive lanes = consecutive frames of one row
  const int total = a.nk * a.fw;
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    const int row = (int)__umulhi((uint32_t)i, a.magic_fw), f = i - row * a.fw;
    if (f0 + f < a.nframes) a.y[(size_t)row * (size_t)a.pitch + (size_t)(f0 + f)] = sm[f * a.mp + a.perm[row]];
  }
}

// new history = last H samples of [old history | x[0 .. n)]
__global__ __launch_bounds__(256) void chan_roll(const float2* __restrict__ x, int n, const float2* __restrict__ old,
                                                 float2* __restrict__ neu, int H) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= H) return;
  const long long j = (long long)i + n;
  neu[i] = j < H ? old[j] : x[j - H];
}

using ChanKernel = void (*)(const ChanArgs);
ChanKernel chan_kernel_for(int C, int FI) {
  if (FI == 8) return C == 1 ? chan_kernel<1, 8> : C == 2 ? chan_kernel<2, 8> : chan_kernel<4, 8>;
  return C == 1 ? chan_kernel<1, 4> : C == 2 ? chan_kernel<2, 4> : chan_kernel<4, 4>;
}

}  // namespace

int chan_prepare(const ChanPlan& p) {
  PYSDR_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(chan_kernel_for(p.C, p.fi)),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, p.lds_bytes));
  return PYSDR_OK;
}

int launch_chan(const ChanPlan& p, const ChanArgs& a, int grid, hipStream_t st) {
  hipLaunchKernelGGL(chan_kernel_for(p.C, p.fi), dim3(grid), dim3(p.threads), (size_t)p.lds_bytes, st, a);
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

int launch_chan_roll(const float2* x, int n, const float2* old, float2* neu, int H, hipStream_t st) {
  hipLaunchKernelGGL(chan_roll, dim3((H + 255) / 256), dim3(256), 0, st, x, n, old, neu, H);
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

}  // namespace pysdr
