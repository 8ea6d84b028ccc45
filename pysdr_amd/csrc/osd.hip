// Ordered-statistics decoding behind min-sum: one wavefront of 64 lanes per candidate, grid n,
// launched behind ldpc_decode_kernel on the same stream and on the same soft bits.  A candidate whose min-sum status is 2
// leaves at once, before any barrier.  Otherwise:
//   rank         every position's key (the bits of |x|) against the 173 others in the LDS: its rank, and perm;
//   matrix       lane l holds rows l and l + 64 of G = [I | P^T] in rank order, six words each, in its registers;
//   elimination  a serial walk over the ranks until 91 are kept: two ballots find the lowest free row with the rank's bit,
//                six shuffles broadcast it, every other row with the bit XORs it in; no barrier, no LDS;
//   patterns     the rows go to the LDS in pivot order, six lanes form e0, then lane l scores k = l, l + 64, .., four
//                patterns at a time over the 174 ranks;
//   winner       the least (distance, k) by a shuffle butterfly; one lane does the CRC, the packing and the stores.
// The workgroup is one wavefront, so its barriers order the LDS between lanes and cost no wait; every one of them is
// reached by all 64 lanes.  The steps are osd_plan.h's, the very functions the scalar transcription runs.
#include "ft_plan.h"
#include "objects_plan.h"
#include "osd_plan.h"

namespace pysdr {

namespace {

constexpr int kOsdAtOnce = 4;                          // patterns a lane scores together: four independent chains of adds

template <int SRC>
__global__ __launch_bounds__(kOsdThreads) void osd_decode_kernel(const OsdArgs a) {
  __shared__ float s_rs[kLdpcN];                       // |x| in rank order
  __shared__ uint32_t s_key[kLdpcN];                   // the bits of |x| in transmission order
  __shared__ int16_t s_perm[kLdpcN];                   // rank -> position
  __shared__ uint32_t s_g[kLdpcK * kOsdWords];         // G' in pivot order
  __shared__ int16_t s_piv[kLdpcK];
  __shared__ uint32_t s_h[kOsdWords], s_e0[kOsdWords];
  __shared__ uint8_t s_hard[kLdpcN], s_word[kLdpcN];
  const int cand = blockIdx.x, lane = threadIdx.x;
  if (cand >= a.n) return;
  int32_t* status = a.status + (size_t)cand * kLdpcStatusWords;
  int32_t* detail = a.detail ? a.detail + (size_t)cand * kOsdDetailWords : nullptr;
  if (status[0] == 2) {                                // the whole wavefront: no barrier is left behind
    if (detail && lane < kOsdDetailWords) detail[lane] = lane < 3 ? -1 : 0;
    return;
  }

  // steps 1 and 2: keys, hard bits, ranks
  for (int n = lane; n < kLdpcN; n += kOsdThreads) {
    float x;
    if (SRC == kLdpcFromBuffer) {
      x = a.llr[(size_t)cand * kLdpcN + n];
    } else {
      const int F = a.cand[2 * cand], slot0 = a.cand[2 * cand + 1];
      const int row = F / a.nsub, j = F - row * a.nsub;
      const float* ring = a.ring + (size_t)row * (size_t)a.tr * (size_t)a.nb;
      x = ft_llr_bit<FtRingMode<SRC>>(ring, a.tr, a.nb, slot0, j, n);
    }
    s_key[n] = osd_key(x);
    s_hard[n] = x > 0.f ? 1 : 0;
  }
  for (int t = lane; t < kLdpcK; t += kOsdThreads) s_piv[t] = 0;
  __syncthreads();
  for (int n = lane; n < kLdpcN; n += kOsdThreads) {
    const uint32_t key = s_key[n];
    int rank = 0;
    for (int m = 0; m < kLdpcN; ++m) rank += osd_before(s_key[m], m, key, n) ? 1 : 0;
    s_perm[rank] = (int16_t)n;                         // the order is total: every rank is taken once
  }
  __syncthreads();
  for (int c = 0; c < 3; ++c) {
    const int p = kOsdThreads * c + lane;
    const int n = p < kLdpcN ? s_perm[p] : 0;
    if (p < kLdpcN) s_rs[p] = osd_magnitude(s_key[n]);
    const unsigned long long b = __ballot(p < kLdpcN && s_hard[n] != 0);
    if (lane == 0) { s_h[2 * c] = (uint32_t)b; s_h[2 * c + 1] = (uint32_t)(b >> 32); }
  }

  // the matrix in rank order: rows lane and lane + 64
  const bool two = lane + kOsdThreads < kLdpcK;
  const int i0 = lane, i1 = two ? lane + kOsdThreads : kLdpcK - 1;
  uint32_t r0[kOsdWords], r1[kOsdWords];
#pragma unroll
  for (int w = 0; w < kOsdWords; ++w) {
    const int nb = w + 1 < kOsdWords ? 32 : kLdpcN - 32 * (kOsdWords - 1);
    uint32_t v0 = 0, v1 = 0;
#pragma unroll 1
    for (int b = 0; b < nb; ++b) {
      const int n = s_perm[32 * w + b];
      v0 |= osd_gen_bit(i0, n) << b;
      v1 |= osd_gen_bit(i1, n) << b;
    }
    r0[w] = v0; r1[w] = two ? v1 : 0u;
  }

  // steps 3 and 4: the most reliable basis, G' in the registers
  int t0 = -1, t1 = two ? -1 : kLdpcK;                 // a row's place among the pivots once it holds one
  int kept = 0, last = 0;
#pragma unroll
  for (int w = 0; w < kOsdWords; ++w) {                // the word of the rank is a constant: the rows stay in registers
    const int nb = w + 1 < kOsdWords ? 32 : kLdpcN - 32 * (kOsdWords - 1);
#pragma unroll 1
    for (int sh = 0; sh < nb && kept < kLdpcK; ++sh) {
      const bool m0 = (r0[w] >> sh) & 1u, m1 = (r1[w] >> sh) & 1u;
      const unsigned long long b0 = __ballot(m0 && t0 < 0), b1 = __ballot(m1 && t1 < 0);
      if (!(b0 | b1)) continue;                        // dependent on the columns kept so far; the same for every lane
      const bool second = b0 == 0;
      const int src = (second ? __ffsll((long long)b1) : __ffsll((long long)b0)) - 1;
      const bool me0 = !second && lane == src, me1 = second && lane == src;
#pragma unroll
      for (int q = 0; q < kOsdWords; ++q) {
        const uint32_t pr = (uint32_t)__shfl((int)(second ? r1[q] : r0[q]), src, kOsdThreads);
        if (m0 && !me0) r0[q] ^= pr;
        if (m1 && !me1) r1[q] ^= pr;
      }
      if (me0) t0 = kept;
      if (me1) t1 = kept;
      last = 32 * w + sh;
      if (lane == 0) s_piv[kept] = (int16_t)last;
      ++kept;
    }
  }
#pragma unroll
  for (int w = 0; w < kOsdWords; ++w) {
    if (t0 >= 0 && t0 < kLdpcK) s_g[t0 * kOsdWords + w] = r0[w];
    if (t1 >= 0 && t1 < kLdpcK) s_g[t1 * kOsdWords + w] = r1[w];
  }
  __syncthreads();

  // step 5: e0
  if (lane < kOsdWords) {
    uint32_t v = s_h[lane];
    for (int t = 0; t < kLdpcK; ++t)
      if (osd_bit(s_h, s_piv[t])) v ^= s_g[t * kOsdWords + lane];
    s_e0[lane] = v;
  }
  __syncthreads();

  // steps 6 to 8: this lane's patterns, then the wavefront's winner
  const int np = osd_patterns(a.order);
  float bd = INFINITY;
  int bk = 0x7FFFFFFF;
  for (int k0 = 0; k0 < np; k0 += kOsdThreads * kOsdAtOnce) {
    uint32_t pat[kOsdAtOnce][kOsdWords];
    float d[kOsdAtOnce];
#pragma unroll
    for (int u = 0; u < kOsdAtOnce; ++u) {
      const int k = k0 + kOsdThreads * u + lane;
      int i, j;
      osd_ij_of(k < np ? k : 0, &i, &j);
      osd_pattern(s_e0, s_g, i, j, pat[u]);
    }
    osd_distances<kOsdAtOnce>(pat, s_rs, d);
#pragma unroll
    for (int u = 0; u < kOsdAtOnce; ++u) {
      const int k = k0 + kOsdThreads * u + lane;
      if (k < np && osd_better(d[u], k, bd, bk)) { bd = d[u]; bk = k; }
    }
  }
  for (int off = kOsdThreads / 2; off > 0; off >>= 1) {
    const float od = __shfl_xor(bd, off, kOsdThreads);
    const int ok = __shfl_xor(bk, off, kOsdThreads);
    if (osd_better(od, ok, bd, bk)) { bd = od; bk = ok; }
  }
  bk = __shfl(bk, 0, kOsdThreads);
  bd = __shfl(bd, 0, kOsdThreads);
  if (bk < 0 || bk >= np) bk = 0;                      // only a distance that is no number can leave no winner

  // step 9: the winner's word, back in transmission order
  int wi, wj;
  osd_ij_of(bk, &wi, &wj);
  int weight = 0;
#pragma unroll
  for (int w = 0; w < kOsdWords; ++w) weight += __popc(osd_pattern_word(s_e0, s_g, wi, wj, w));
  for (int p = lane; p < kLdpcN; p += kOsdThreads) {
    const int n = s_perm[p];
    s_word[n] = (uint8_t)(s_hard[n] ^ ((osd_pattern_word(s_e0, s_g, wi, wj, p >> 5) >> (p & 31)) & 1u));
  }
  __syncthreads();
  if (lane == 0)                                       // one lane: the CRC, the packing and the stores
    osd_result(s_word, bk, last, weight, bd, status, a.bits + (size_t)cand * kLdpcBitsBytes, detail);
}

}  // namespace

int launch_osd_decode(int source, const OsdArgs& a, hipStream_t st) {
  if (a.n < 1) return PYSDR_OK;
  if (a.n > kLdpcMax || a.order < 0 || a.order > kOsdOrderMax || !a.status || !a.bits) {
    set_last_error("launch_osd_decode: n %d, order %d or a NULL output", a.n, a.order);
    return PYSDR_ERR_ARG;
  }
  if (source == kLdpcFromBuffer && a.llr)
    hipLaunchKernelGGL(osd_decode_kernel<kLdpcFromBuffer>, dim3(a.n), dim3(kOsdThreads), 0, st, a);
  else if (source == kLdpcFromFt8Ring && a.ring && a.cand)
    hipLaunchKernelGGL(osd_decode_kernel<kLdpcFromFt8Ring>, dim3(a.n), dim3(kOsdThreads), 0, st, a);
  else if (source == kLdpcFromFt4Ring && a.ring && a.cand)
    hipLaunchKernelGGL(osd_decode_kernel<kLdpcFromFt4Ring>, dim3(a.n), dim3(kOsdThreads), 0, st, a);
  else {
    set_last_error("launch_osd_decode: source %d without its input", source);
    return PYSDR_ERR_ARG;
  }
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

}  // namespace pysdr
