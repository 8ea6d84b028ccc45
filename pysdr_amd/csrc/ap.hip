// A-priori decoding of the FT8 and FT4 skimmers: every pair (candidate, hypothesis) of a call
// is one workgroup of ldpc.hip's shape -- 192 threads, thread n < 174 a variable and its three edges, thread m < 83 a
// check, the messages in the LDS -- in front of which the pair's soft bits are clamped: amax, the greatest |llr| of the
// word, by a wavefront reduction and three words of the LDS; A = mag amax; a soft bit under the hypothesis' mask becomes
// +A or -A.  The iteration is ldpc.hip's, step for step through ldpc_plan.h's functions.  Behind it nerr counts outside the
// mask, nap inside it, and one thread runs the CRC and the packing.  The workgroups of one candidate read the same ring
// columns, which the L2 serves after the first.  ap_pick_kernel, launched behind it on the same stream, walks every
// candidate's pairs with one thread: only ap, bits and (if asked for) detail go back to the host.
#include "ap_plan.h"
#include "ft_plan.h"
#include "objects_plan.h"

namespace pysdr {

namespace {

template <int SRC>
__global__ __launch_bounds__(kLdpcThreads) void ap_decode_kernel(const ApArgs a) {
  __shared__ float s_c[kLdpcEdges];
  __shared__ float s_v[kLdpcEdges];
  __shared__ uint8_t s_hard[kLdpcN + 2];
  __shared__ int s_odd[2];
  __shared__ int s_nerr, s_nap;
  __shared__ float s_max[kLdpcThreads / 64];
  const int pair = blockIdx.x, tid = threadIdx.x;
  if (pair >= a.npairs) return;                            // the whole workgroup: no barrier is left behind
  const int cand = a.pairs[2 * pair];
  const uint8_t* hyp = a.hyps + (size_t)a.pairs[2 * pair + 1] * kApHypBytes;
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
  // amax: a maximum does not depend on the order it is taken in
  float m = fabsf(llr);                                    // 0 beyond the word
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const float o = __shfl_xor(m, d, 64);
    m = o > m ? o : m;
  }
  if ((tid & 63) == 0) s_max[tid >> 6] = m;
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
  if (tid == 0) { s_nerr = 0; s_nap = 0; }
  __syncthreads();
  float amax = s_max[0];
#pragma unroll
  for (int w = 1; w < kLdpcThreads / 64; ++w) amax = s_max[w] > amax ? s_max[w] : amax;
  const float L = -(var ? ap_clamp(llr, ap_amp(a.mag, amax), hyp, tid) : 0.f);

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

  bool err = false, miss = false;
  if (var) ap_count(llr, hard, hyp, tid, &err, &miss);
  const unsigned long long be = __ballot(err), bm = __ballot(miss);
  if ((tid & 63) == 0) { atomicAdd(&s_nerr, __popcll(be)); atomicAdd(&s_nap, __popcll(bm)); }
  __syncthreads();
  if (tid == 0) {                                          // one thread: the CRC, the packing and the pair's status
    int32_t st[kLdpcStatusWords];
    ldpc_result(s_hard, codeword, k, s_nerr, st, a.pbits + (size_t)pair * kLdpcBitsBytes);
    int32_t* d = a.detail + (size_t)pair * kApDetailWords;
    d[0] = ap_status(st[0], s_nerr, s_nap, a.nerr_max); d[1] = k; d[2] = s_nerr; d[3] = s_nap;
  }
}

__global__ __launch_bounds__(kApPickThreads) void ap_pick_kernel(const ApArgs a) {
  const int c = blockIdx.x * kApPickThreads + threadIdx.x;
  if (c >= a.n) return;
  ap_pick(a.detail, a.pbits, a.first[c], a.first[c + 1], a.ap + (size_t)c * kApWords, a.bits + (size_t)c * kLdpcBitsBytes);
}

}  // namespace

int launch_ap_decode(int source, const ApArgs& a, hipStream_t st) {
  if (a.n < 1) return PYSDR_OK;
  if (a.n > kLdpcMax || a.npairs < 0 || a.npairs > kApPairMax || a.iters < 1 || a.iters > kLdpcItersMax || !a.hyps || !a.pairs || !a.first ||
      !a.detail || !a.pbits || !a.ap || !a.bits) {
    set_last_error("launch_ap_decode: n %d, %d pairs, iters %d or a NULL table or output", a.n, a.npairs, a.iters);
    return PYSDR_ERR_ARG;
  }
  const bool ring = (source == kLdpcFromFt8Ring || source == kLdpcFromFt4Ring) && a.ring && a.cand;
  if (!ring && !(source == kLdpcFromBuffer && a.llr)) {
    set_last_error("launch_ap_decode: source %d without its input", source);
    return PYSDR_ERR_ARG;
  }
  if (a.npairs > 0) {
    if (source == kLdpcFromBuffer)
      hipLaunchKernelGGL(ap_decode_kernel<kLdpcFromBuffer>, dim3(a.npairs), dim3(kLdpcThreads), 0, st, a);
    else if (source == kLdpcFromFt8Ring)
      hipLaunchKernelGGL(ap_decode_kernel<kLdpcFromFt8Ring>, dim3(a.npairs), dim3(kLdpcThreads), 0, st, a);
    else
      hipLaunchKernelGGL(ap_decode_kernel<kLdpcFromFt4Ring>, dim3(a.npairs), dim3(kLdpcThreads), 0, st, a);
    PYSDR_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(ap_pick_kernel, dim3((a.n + kApPickThreads - 1) / kApPickThreads), dim3(kApPickThreads), 0, st, a);
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

}  // namespace pysdr
