// Second stage of the fine channelizer: an M2-channel polyphase channelizer batched over the rows
// of a first-stage channelizer.  Input is the row buffer the first stage (chan.hip, untouched) has just written: row j
// holds `hist` earlier stage-1 outputs in front of this call's.  For coarse row j and fine frame m (absolute):
//   v[r]   = sum_{p<P2} h2[p M2 + r] y1_j[m D2 - p M2 - r]            (p ascending, one fma per tap and component;
//                                                                     taps beyond the prototype's length are skipped)
//   Y[k2]  = sum_r v[r] e^{+j 2 pi k2 (r - m D2) / M2}                (in-place DIF passes of radix 5 / 4 / 2 in LDS)
// and of the M2 results only the Q = M2 / C1 with k2 = q mod M2, q in [-Q/2, Q/2), are stored: fine channel k1 Q + q,
// output row a = (that - g_first) mod Mf where a < ng.  The arithmetic of an output depends on (j, m) alone, never on how
// a call tiles: a workgroup holds `slots` frames in LDS and a launch splits them into rw rows times fw frames
// (fine_tile, fine_plan.h) -- all frames when a call completes many, many rows when it completes one or two, which
// chan.hip with its single input stream has no use for.  Work items:
//   1. FIR: one (row, frame, branch r); consecutive lanes read consecutive samples, the re-use comes from the L2.
//   2. FFT: the very passes of chan.hip, over the workgroup's slots (fft_lds.h holds them for both).
//   3. Store: consecutive lanes = consecutive frames of one output row.
// fine_roll then moves the last `hist` samples of every row to its front: one workgroup per row reads all of them into
// registers before it writes any.
#include "fft_lds.h"
#include "fine_plan.h"

namespace pysdr {
namespace {

__global__ __launch_bounds__(kFineThreads) void fine_kernel(const FineArgs a) {
  extern __shared__ float2 sm[];
  const float2* rows = reinterpret_cast<const float2*>(a.rows);
  const float2* tw = reinterpret_cast<const float2*>(a.tw);
  float2* y = reinterpret_cast<float2*>(a.y);
  const int f0 = blockIdx.x * a.fw, j0 = blockIdx.y * a.rw;    // first frame (counted from the call's first) and row
  const int slots = a.fw * a.rw;
  // ---- 1. polyphase FIR into LDS: slot s = (row jl, frame f), branch r at (r - m D2) mod M2
  const int nitems = slots * a.M2;
  for (int i = threadIdx.x; i < nitems; i += blockDim.x) {
    const int s = (int)__umulhi((uint32_t)i, a.magic_M2), r = i - s * a.M2;
    const int j = j0 + (s >> a.fw_shift), fr = f0 + (s & (a.fw - 1));
    float2 acc = make_float2(0.f, 0.f);
    if (j < a.nk1 && fr < a.nframes) {
      const float2* x = rows + (size_t)j * (size_t)a.pitch1 + (a.off + fr * a.D2 - r);   // tap row p reads x[-p M2]
      for (int p = 0; p < a.P2; ++p) {
        const int idx = p * a.M2 + r;
        if (idx < a.L2) {
          const float h = a.taps[idx];
          const float2 v = x[-p * a.M2];
          acc.x = __builtin_fmaf(h, v.x, acc.x);
          acc.y = __builtin_fmaf(h, v.y, acc.y);
        }
      }
    }
    sm[s * a.mp + fine_rot(r, a.mf_lo + fr, a.C2, a.D2, a.M2)] = acc;
  }
  __syncthreads();
  // ---- 2. inverse DFT of every slot, in place, digit-reversed result
  int nb = a.M2;
  for (int s = 0; s < a.fft.npass; ++s) {
    const int R = a.fft.radix[s];
    if (R == 4) fft_pass<4>(sm, tw, a.M2, a.mp, slots, nb, a.fft.magic_per[s], a.fft.magic_nq[s]);
    else if (R == 5) fft_pass<5>(sm, tw, a.M2, a.mp, slots, nb, a.fft.magic_per[s], a.fft.magic_nq[s]);
    else fft_pass<2>(sm, tw, a.M2, a.mp, slots, nb, a.fft.magic_per[s], a.fft.magic_nq[s]);
    nb /= R;
    __syncthreads();
  }
  // ---- 3. the kept channels, channel-major: consecutive lanes = consecutive frames of one output row
  const int total = a.rw * a.Q * a.fw;
  for (int i = threadIdx.x; i < total; i += blockDim.x) {
    const int f = i & (a.fw - 1), t = i >> a.fw_shift;
    const int jl = (int)__umulhi((uint32_t)t, a.magic_Q), u = t - jl * a.Q;
    const int j = j0 + jl, fr = f0 + f;
    if (j < a.nk1 && fr < a.nframes) {
      const int row = fine_row_of(a.a0[j], u, a.Mf);
      if (row < a.ng) y[(size_t)row * (size_t)a.pitch + (size_t)fr] = sm[(jl * a.fw + f) * a.mp + a.perm[u]];
    }
  }
}

// every row: new [0, hist) = old [n1, n1 + hist); the ranges overlap when n1 < hist, so all reads come first
__global__ __launch_bounds__(kFineRollThreads) void fine_roll(float2* rows, long long pitch1, int hist, int n1) {
  float2* row = rows + (size_t)blockIdx.x * (size_t)pitch1;
  float2 v[kFineRollPer];
#pragma unroll
  for (int i = 0; i < kFineRollPer; ++i) {
    const int e = fine_roll_elem(threadIdx.x, i);
    if (e < hist) v[i] = row[e + n1];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kFineRollPer; ++i) {
    const int e = fine_roll_elem(threadIdx.x, i);
    if (e < hist) row[e] = v[i];
  }
}

}  // namespace

int fine_prepare(const FinePlan& p) {
  PYSDR_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(fine_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      p.lds_bytes));
  return PYSDR_OK;
}

int launch_fine(const FinePlan& p, const FineArgs& a, int gx, int gy, hipStream_t st) {
  hipLaunchKernelGGL(fine_kernel, dim3(gx, gy), dim3(kFineThreads), (size_t)p.lds_bytes, st, a);
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

int launch_fine_roll(float* rows, long long pitch1, int hist, int n1, int nk1, hipStream_t st) {
  hipLaunchKernelGGL(fine_roll, dim3(nk1), dim3(kFineRollThreads), 0, st, reinterpret_cast<float2*>(rows), pitch1, hist, n1);
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

}  // namespace pysdr
