// The channelizers' FFT on the device: an M-point inverse DFT of every frame a workgroup holds in LDS, as in-place
// decimation-in-frequency passes of radix 5 / 4 / 2 (which passes, their multipliers, the twiddle table and where the
// result of channel k is left: fft_plan.h).  chan.hip and fine.hip run fft_pass<R> for every pass of their FftPasses,
// a barrier behind each, between their own FIR and store phases.  That loop of nine lines stays in each kernel: as a
// function of this header it is simplified on its own before it is inlined, and both kernels then compile to longer
// per-pass set-up than with the loop in place (LABNOTES 21).  Everything here is inlined into the calling kernel.  The
// order of every floating-point operation below is part of the results of both stages bit for bit (the parentheses of
// bfly<5> too).  psdfft.hip's 64k FFT is another one.
#pragma once

#include "common.h"
#include "fft_plan.h"

namespace pysdr {

__device__ __forceinline__ float2 cmul(float2 a, float2 w) {
  return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// DFT of R points with the kernel e^{+j 2 pi n k / R}
template <int R>
__device__ __forceinline__ void bfly(float2* v);
template <>
__device__ __forceinline__ void bfly<2>(float2* v) {
  const float2 a = v[0], b = v[1];
  v[0] = cadd(a, b);
  v[1] = csub(a, b);
}
template <>
__device__ __forceinline__ void bfly<4>(float2* v) {
  const float2 s02 = cadd(v[0], v[2]), d02 = csub(v[0], v[2]), s13 = cadd(v[1], v[3]), d13 = csub(v[1], v[3]);
  v[0] = cadd(s02, s13);
  v[2] = csub(s02, s13);
  v[1] = make_float2(d02.x - d13.y, d02.y + d13.x);      // d02 + j d13
  v[3] = make_float2(d02.x + d13.y, d02.y - d13.x);      // d02 - j d13
}
template <>
__device__ __forceinline__ void bfly<5>(float2* v) {
  constexpr float c1 = 0.30901699437494742f, c2 = -0.80901699437494742f;    // cos(2 pi / 5), cos(4 pi / 5)
  constexpr float s1 = 0.95105651629515357f, s2 = 0.58778525229247313f;     // sin(2 pi / 5), sin(4 pi / 5)
  const float2 a = v[0];
  const float2 t1 = cadd(v[1], v[4]), t2 = cadd(v[2], v[3]), t3 = csub(v[1], v[4]), t4 = csub(v[2], v[3]);
  v[0] = cadd(cadd(a, t1), t2);
  const float2 m1 = make_float2((a.x + c1 * t1.x) + c2 * t2.x, (a.y + c1 * t1.y) + c2 * t2.y);
  const float2 m2 = make_float2((a.x + c2 * t1.x) + c1 * t2.x, (a.y + c2 * t1.y) + c1 * t2.y);
  const float2 n1 = make_float2(s1 * t3.x + s2 * t4.x, s1 * t3.y + s2 * t4.y);
  const float2 n2 = make_float2(s2 * t3.x - s1 * t4.x, s2 * t3.y - s1 * t4.y);
  v[1] = make_float2(m1.x - n1.y, m1.y + n1.x);          // m1 + j n1
  v[4] = make_float2(m1.x + n1.y, m1.y - n1.x);
  v[2] = make_float2(m2.x - n2.y, m2.y + n2.x);          // m2 + j n2
  v[3] = make_float2(m2.x + n2.y, m2.y - n2.x);
}

// One in-place decimation-in-frequency pass over `slots` frames of M points, frame f at sm + f mp: blocks of nb points
// split into R blocks of nq = nb / R; output k1 of the butterfly at n2 is turned by e^{+j 2 pi n2 k1 / nb} (nothing to
// turn in the last pass, nq = 1).
template <int R>
__device__ __forceinline__ void fft_pass(float2* sm, const float2* tw, int M, int mp, int slots, int nb, uint32_t magic_per,
                                         uint32_t magic_nq) {
  const int nq = nb / R, per = M / R, total = slots * per, tws = M / nb;
  for (int it = threadIdx.x; it < total; it += blockDim.x) {
    const int f = (int)__umulhi((uint32_t)it, magic_per), j = it - f * per;
    const int b = nq > 1 ? (int)__umulhi((uint32_t)j, magic_nq) : j, n2 = j - b * nq;
    float2* p = sm + f * mp + b * nb + n2;
    float2 v[R];
#pragma unroll
    for (int i = 0; i < R; ++i) v[i] = p[i * nq];
    bfly<R>(v);
    if (nq > 1) {
#pragma unroll
      for (int i = 1; i < R; ++i) v[i] = cmul(v[i], tw[n2 * i * tws]);
    }
#pragma unroll
    for (int i = 0; i < R; ++i) p[i * nq] = v[i];
  }
}

}  // namespace pysdr
