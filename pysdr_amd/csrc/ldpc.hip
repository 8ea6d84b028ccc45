// LDPC(174,91) decoder of the FT8 and FT4 skimmers: normalised min-sum on a flooding
// schedule, one workgroup of 192 threads per candidate.  Thread n < 174 owns a variable and its three edges, thread
// m < 83 a check and its six or seven; the messages c (check -> variable) and v (variable -> check) are 522 floats each
// in the LDS, the thread's own table entries sit in its registers, and an iteration is two phases with a barrier behind
// each:
//   A  variables: tot = L + the three incoming c, the hard bit, and the three outgoing v;
//   B  checks: the parity of the hard bits (an odd one raises the iteration's flag in the LDS) and the new c.
// Behind the second barrier every thread reads the same flag, so all leave the loop together; the flags alternate
// between two words, so that the one being read is never the one being cleared.  The new c of a final iteration are
// computed and never read.  The steps are ldpc_plan.h's, the very functions the scalar transcription runs.
// Three sources of soft bits through one template flag: a device buffer [n][174], or the spectrum ring of an FT8 or an
// FT4 skimmer read through ft_llr_bit of the source's mode, so that soft bits never touch global memory.
#include "ft_plan.h"
#include "ldpc_plan.h"
#include "objects_plan.h"

namespace pysdr {

namespace {

template <int SRC>
__global__ __launch_bounds__(kLdpcThreads) void ldpc_decode_kernel(const LdpcArgs a) {
  __shared__ float s_c[kLdpcEdges];
  __shared__ float s_v[kLdpcEdges];
  __shared__ uint8_t s_hard[kLdpcN + 2];
  __shared__ int s_odd[2];
  __shared__ int s_nerr;
  const int cand = blockIdx.x, tid = threadIdx.x;
  if (cand >= a.n) return;                                 // the whole workgroup: no barrier is left behind
  const bool var = tid < kLdpcN, chk = tid < kLdpcM;

  float llr = 0.f;
  int e0 = 0, e1 = 0, e2 = 0;
  if (var) {
    if (SRC == kLdpcFromBuffer) {
      llr = a.llr[(size_t)cand * kLdpcN + tid];
    } else {
      const int F = a.cand[2 * cand], slot0 = a.cand[2 * cand + 1];
      const int row = F / a.nsub, j = F - row * a.nsub;
      const float* ring = a.ring + (size_t)row * (size_t)a.tr * (size_t)a.nb;
      llr = ft_llr_bit<FtRingMode<SRC>>(ring, a.tr, a.nb, slot0, j, tid);
    }
    e0 = kLdpc.edge[tid][0]; e1 = kLdpc.edge[tid][1]; e2 = kLdpc.edge[tid][2];
  }
  const float L = -llr;
  int deg = 0, base = 0;
  int col[kLdpcDegMax];
#pragma unroll
  for (int d = 0; d < kLdpcDegMax; ++d) col[d] = 0;
  if (chk) {
    deg = kLdpc.deg[tid];
    base = kLdpc.base[tid];
#pragma unroll
    for (int d = 0; d < kLdpcDegMax; ++d) col[d] = d < deg ? kLdpc.col[tid][d] : 0;
  }
  for (int e = tid; e < kLdpcEdges; e += kLdpcThreads) s_c[e] = 0.f;
  if (tid == 0) s_nerr = 0;
  __syncthreads();

  float tot = 0.f;
  bool hard = false, codeword = false;
  int k = 0;
  for (;; ++k) {
    if (tid == 0) s_odd[k & 1] = 0;
    if (var) {
      float v0, v1, v2;
      tot = ldpc_variable(L, s_c[e0], s_c[e1], s_c[e2], &v0, &v1, &v2);
      s_v[e0] = v0; s_v[e1] = v1; s_v[e2] = v2;
      hard = tot < 0.f;
      s_hard[tid] = hard ? 1 : 0;
    }
    __syncthreads();
    if (chk) {
      float v[kLdpcDegMax], c[kLdpcDegMax];
      int p = 0;
#pragma unroll
      for (int d = 0; d < kLdpcDegMax; ++d) {
        v[d] = 0.f; c[d] = 0.f;
        if (d < deg) { v[d] = s_v[base + d]; p ^= s_hard[col[d]]; }
      }
      if (p) s_odd[k & 1] = 1;
      ldpc_check(v, deg, a.alpha, c);
#pragma unroll
      for (int d = 0; d < kLdpcDegMax; ++d)
        if (d < deg) s_c[base + d] = c[d];
    }
    __syncthreads();
    codeword = s_odd[k & 1] == 0;                          // the same word for every thread: all leave together
    if (codeword || k >= a.iters) break;
  }

  const bool differs = var && ((llr > 0.f) != hard);
  const unsigned long long b = __ballot(differs);
  if ((tid & 63) == 0) atomicAdd(&s_nerr, __popcll(b));
  __syncthreads();
  if (var && a.post) a.post[(size_t)cand * kLdpcN + tid] = tot;
  if (tid == 0)                                            // one thread: the CRC and the packing
    ldpc_result(s_hard, codeword, k, s_nerr, a.status + (size_t)cand * kLdpcStatusWords, a.bits + (size_t)cand * kLdpcBitsBytes);
}

}  // namespace

int launch_ldpc_decode(int source, const LdpcArgs& a, hipStream_t st) {
  if (a.n < 1) return PYSDR_OK;
  if (a.n > kLdpcMax || a.iters < 1 || a.iters > kLdpcItersMax || !a.status || !a.bits) {
    set_last_error("launch_ldpc_decode: n %d, iters %d or a NULL output", a.n, a.iters);
    return PYSDR_ERR_ARG;
  }
  if (source == kLdpcFromBuffer && a.llr)
    hipLaunchKernelGGL(ldpc_decode_kernel<kLdpcFromBuffer>, dim3(a.n), dim3(kLdpcThreads), 0, st, a);
  else if (source == kLdpcFromFt8Ring && a.ring && a.cand)
    hipLaunchKernelGGL(ldpc_decode_kernel<kLdpcFromFt8Ring>, dim3(a.n), dim3(kLdpcThreads), 0, st, a);
  else if (source == kLdpcFromFt4Ring && a.ring && a.cand)
    hipLaunchKernelGGL(ldpc_decode_kernel<kLdpcFromFt4Ring>, dim3(a.n), dim3(kLdpcThreads), 0, st, a);
  else {
    set_last_error("launch_ldpc_decode: source %d without its input", source);
    return PYSDR_ERR_ARG;
  }
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

}  // namespace pysdr
