// Fused PSD frame path for the RF waterfall (spectrum.periodogram, Plotting.py:462; sizes
// gui.py:611-616 after the 2^16 clamp of Plotting.py:370-375): window -> zero-pad
// 32768 -> 65536 -> FFT -> re^2+im^2 -> 10*log10 -> fftshift (formula pinned by
// rtty.py:839-841).  rocFFT needs a pad kernel, two transform kernels and a dB kernel
// (~3.5 MB of traffic per frame); here the 64k transform is a four-step 256 x 256
// decomposition in TWO kernels with the window/zero-pad fused into the first and the
// power/dB/fftshift into the second:
//
//   n = 256 a + b (a < 128 non-zero rows),  k = p + 256 q
//   psd_cols:  Y[p][b] = W_65536^(b p) * sum_a xw[256 a + b] W_256^(a p)     (256-pt over a)
//   psd_rows:  X[p + 256 q] = sum_b Y[p][b] W_256^(b q)                      (256-pt over b)
//
// HBM traffic per frame = 256 KB in + 256 KB out; the 512 KB intermediate Y of a group of
// frames is written and re-read immediately, so it lives in L2 / Infinity Cache.  Y is stored
// as [b / 16][p][b % 16]: a columns workgroup (16 columns) writes one contiguous 32 KB block, and
// every wave-level store / load of the intermediate covers 512 contiguous bytes (the natural
// [p][b] order makes 128-byte pieces 2 KB apart: 257 -> 251 ns per frame).  Each
// 256-point transform is radix 16 x 16 (one 16-point butterfly per thread per pass), data
// exchanged through LDS with conflict-free strides.
// The shipped pair keeps the intermediate as block-scaled 24-bit fixed point (psd_cols_pk / psd_rows_pk below), and its
// columns pass is a LOOP OVER FRAMES: 16 x G resident workgroups, each keeping its column block -- table, window and
// four-step twiddles set up once -- and loading its next frame while it transforms one (psd_cols_pk_kernel; the grid is
// host_plan.h plan_psd_cols; LABNOTES 15).  The rows pass is the same kind of loop on 8 x R workgroups (psd_rows_pk_kernel,
// plan_psd_rows).  One unit per workgroup (psd_cols_pk_unit_kernel / psd_rows_pk_unit_kernel, PYSDR_PSD_PATH=unit) is the A/B form.
#include <algorithm>

#include "common.h"
#include "psd_cols_geom.h"
#include "psd_rows_geom.h"

namespace pysdr {

namespace {

constexpr int kN = 65536, kM = 32768;

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return make_float2(fmaf(a.x, b.x, -a.y * b.y), fmaf(a.x, b.y, a.y * b.x));
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
// exp(-j*pi*t): v_sin_f32 / v_cos_f32 take revolutions (1.2e-7 abs error on gfx950)
__device__ __forceinline__ float2 expmpi(float t) {
  const float rev = 0.5f * t;
  return make_float2(__builtin_amdgcn_cosf(rev), -__builtin_amdgcn_sinf(rev));
}

// Explicit global-address-space accesses: the unit bodies below are also compiled inside
// non-kernel functions (scripts/experiments), where a generic pointer would turn into
// flat_load / flat_store.
typedef float v2f_t __attribute__((ext_vector_type(2)));
#define PYSDR_AS1 __attribute__((address_space(1)))
__device__ __forceinline__ float2 ldg2(const float2* p) {
  const v2f_t v = *(const PYSDR_AS1 v2f_t*)p;
  return make_float2(v.x, v.y);
}
__device__ __forceinline__ void stg2(float2* p, float2 v) {
  const v2f_t w = {v.x, v.y};
  *(PYSDR_AS1 v2f_t*)p = w;
}
// streaming accesses (input read once, PSD written once): non-temporal, so that they do not
// displace the four-step intermediate from the Infinity Cache (measured: 3.15 -> 3.02 ms per
// 10666 frames; the same hint on the intermediate itself makes things worse, 3.37 ms)
__device__ __forceinline__ float2 ldg2_stream(const float2* p) {
  const v2f_t v = __builtin_nontemporal_load((const PYSDR_AS1 v2f_t*)p);
  return make_float2(v.x, v.y);
}
__device__ __forceinline__ void stg1_stream(float* p, float v) {
  __builtin_nontemporal_store(v, (PYSDR_AS1 float*)p);
}
__device__ __forceinline__ float ldg1(const float* p) {
  return *(const PYSDR_AS1 float*)p;
}
__device__ __forceinline__ void stg1(float* p, float v) {
  *(PYSDR_AS1 float*)p = v;
}

// 4-point DFT in place (W4 = -j): (a,b,c,d) -> (X0,X1,X2,X3)
__device__ __forceinline__ void dft4(float2& a, float2& b, float2& c, float2& d) {
  const float2 s0 = cadd(a, c), s1 = csub(a, c), s2 = cadd(b, d), s3 = csub(b, d);
  a = cadd(s0, s2);
  c = csub(s0, s2);
  b = make_float2(s1.x + s3.y, s1.y - s3.x);   // s1 - j*s3
  d = make_float2(s1.x - s3.y, s1.y + s3.x);   // s1 + j*s3
}

// 16-point DFT in place, natural order in and out.  n = n0 + 4 n1, k = k1 + 4 k0:
// DFT4 over n1, twiddle W16^(n0 k1), DFT4 over n0.
__device__ __forceinline__ void dft16(float2 (&v)[16]) {
  const float c1 = 0.92387953251128674f, s1 = 0.38268343236508977f;   // cos, sin(pi/8)
  const float h = 0.70710678118654752f;
#pragma unroll
  for (int n0 = 0; n0 < 4; ++n0) dft4(v[n0], v[n0 + 4], v[n0 + 8], v[n0 + 12]);
  // now v[n0 + 4*k1] = A[n0][k1]; twiddles W16^(n0*k1)
  v[5] = cmul(v[5], make_float2(c1, -s1));     // n0=1,k1=1 : W^1
  v[9] = cmul(v[9], make_float2(h, -h));       // n0=1,k1=2 : W^2
  v[13] = cmul(v[13], make_float2(s1, -c1));   // n0=1,k1=3 : W^3
  v[6] = cmul(v[6], make_float2(h, -h));       // n0=2,k1=1 : W^2
  v[10] = make_float2(v[10].y, -v[10].x);      // n0=2,k1=2 : W^4 = -j
  v[14] = cmul(v[14], make_float2(-h, -h));    // n0=2,k1=3 : W^6
  v[7] = cmul(v[7], make_float2(s1, -c1));     // n0=3,k1=1 : W^3
  v[11] = cmul(v[11], make_float2(-h, -h));    // n0=3,k1=2 : W^6
  v[15] = cmul(v[15], make_float2(-c1, s1));   // n0=3,k1=3 : W^9
#pragma unroll
  for (int k1 = 0; k1 < 4; ++k1) dft4(v[4 * k1], v[4 * k1 + 1], v[4 * k1 + 2], v[4 * k1 + 3]);
  // now v[4*k1 + k0] = X[k1 + 4*k0]: transpose the 4x4 index to natural order
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i + 1; j < 4; ++j) {
      const float2 t = v[4 * i + j];
      v[4 * i + j] = v[4 * j + i];
      v[4 * j + i] = t;
    }
}

// v[k] *= w0 * w^k, k = 0..15 (powers built with depth <= 4 multiplications)
__device__ __forceinline__ void twiddle_pow0(float2 (&v)[16], float2 w, float2 w0) {
  const float2 w2 = cmul(w, w), w4 = cmul(w2, w2), w8 = cmul(w4, w4);
  const float2 b0 = w0, b4 = cmul(w0, w4), b8 = cmul(w0, w8), b12 = cmul(b4, w8);
  const float2 w3 = cmul(w2, w);
  v[0] = cmul(v[0], b0); v[1] = cmul(v[1], cmul(b0, w)); v[2] = cmul(v[2], cmul(b0, w2)); v[3] = cmul(v[3], cmul(b0, w3));
  v[4] = cmul(v[4], b4); v[5] = cmul(v[5], cmul(b4, w)); v[6] = cmul(v[6], cmul(b4, w2)); v[7] = cmul(v[7], cmul(b4, w3));
  v[8] = cmul(v[8], b8); v[9] = cmul(v[9], cmul(b8, w)); v[10] = cmul(v[10], cmul(b8, w2)); v[11] = cmul(v[11], cmul(b8, w3));
  v[12] = cmul(v[12], b12); v[13] = cmul(v[13], cmul(b12, w)); v[14] = cmul(v[14], cmul(b12, w2)); v[15] = cmul(v[15], cmul(b12, w3));
}
// W_256^(i j), i, j < 16, as an LDS table of 16 rows of 17 float2; built by the first 256 threads of the workgroup,
// one v_sin/v_cos pair each.  Building the 15 powers per thread instead costs 14 complex
// multiplications (56 of the ~350 VALU instructions of a pass) and their rounding: the table is
// 2 % faster and three times closer to the exact transform (4.4e-7 vs 1.3e-6 of the peak).
// Row pitch: hipcc reads a row as ds_read2_b64 pairs, which the LDS serves 16 lanes at a time on 32 banks of 4 bytes.
// In psd_cols the 16 lanes of a group read the SAME row (broadcast); in psd_rows they read 16 DIFFERENT rows at the
// same column, row i at dword 2 * pitch * i: with the round-1 pitch of 18 that is 4 i mod 32 -- rows i and i + 8 on
// the same banks, the 795 k conflict cycles of 3.47 M LDS cycles in profiles/r03_c3_pmc_sq.json (23 %; the comments
// here claimed "conflict free") -- with 17 it is 2 i mod 32, two dwords per lane: all 32 banks once.
constexpr int kTwRow = 17;
__device__ __forceinline__ void tw256_build(float2* tw, int tid) {
  if (tid < 256) tw[kTwRow * (tid >> 4) + (tid & 15)] = expmpi((float)((tid >> 4) * (tid & 15)) * (1.0f / 128.0f));
}
// v[k] *= W_256^(i k)
__device__ __forceinline__ void twiddle_tab(float2 (&v)[16], const float2* tw, int i) {
  const float2* r = tw + kTwRow * i;
#pragma unroll
  for (int k = 1; k < 16; ++k) v[k] = cmul(v[k], r[k]);
}

// ---- step 1: 16 columns of one frame per workgroup (grid = 16 x frames, 256 threads).
//   a = a0 + 16 a1 (a1 < 8: the rest is zero padding), p = p1 + 16 p0
//   pass 1 thread (b, a0): DFT16 over a1, * W_256^(a0 p1)      -> LDS[p1][a0][b]
//   pass 2 thread (b, p1): DFT16 over a0, * W_65536^(bb p)      -> Y[p][bb], bb = 16 cb + b
// LDS slot(p1, a0, b) = 272 p1 + 16 a0 + b: consecutive lanes write consecutive slots in
// pass 1, and the 16-slot pad per p1 spreads pass 2's two p1 per half-wave over all banks.
constexpr int kColsPerWg = 16;
constexpr int kColLds = 16 * 272;

// one unit = 16 columns [16 cb, 16 cb + 16) of frame xf, 256 threads (tid), LDS kColLds
__device__ __forceinline__ void cols_unit(const float2* __restrict__ xf, const float* __restrict__ win,
                                          float2* __restrict__ yf, int cb, int tid, float2* lds,
                                          const float2* tw) {
  const int b = tid & 15, hi = tid >> 4;
  const int bb = cb * kColsPerWg + b;
  {
    const int a0 = hi;
    float2 u[16];
#pragma unroll
    for (int a1 = 0; a1 < 8; ++a1) {
      const int n = 256 * (a0 + 16 * a1) + bb;
      const float2 s = ldg2_stream(xf + n);
      const float g = ldg1(win + n);
      u[a1] = make_float2(s.x * g, s.y * g);
    }
#pragma unroll
    for (int a1 = 8; a1 < 16; ++a1) u[a1] = make_float2(0.f, 0.f);
    dft16(u);
    __syncthreads();                                                   // the table (the loads above were in flight)
    twiddle_tab(u, tw, a0);                                            // W_256^(a0 p1)
    float2* p = lds + 16 * a0 + b;
#pragma unroll
    for (int p1 = 0; p1 < 16; ++p1) p[272 * p1] = u[p1];
  }
  __syncthreads();
  {
    const int p1 = hi;
    const float2* p = lds + 272 * p1 + b;
    float2 v[16];
#pragma unroll
    for (int a0 = 0; a0 < 16; ++a0) v[a0] = p[16 * a0];
    dft16(v);
    // four-step twiddle W_65536^(bb * (p1 + 16 p0)) = W^(bb p1) * (W^(16 bb))^p0
    twiddle_pow0(v, expmpi((float)(16 * bb) * (1.0f / 32768.0f)),
                 expmpi((float)(bb * p1) * (1.0f / 32768.0f)));
    // intermediate layout Y[cb][p][b]: the workgroup's 16 columns x 256 rows are one contiguous
    // 32 KB block, and a wave's store covers 512 contiguous bytes (4 p1 x 16 b)
    float2* o = yf + (size_t)cb * 4096 + p1 * 16 + b;
#pragma unroll
    for (int p0 = 0; p0 < 16; ++p0) stg2(o + p0 * 256, v[p0]);
  }
}

__global__ __launch_bounds__(256) void psd_cols_kernel(const float2* __restrict__ x, size_t hop,
                                                       const float* __restrict__ win,
                                                       float2* __restrict__ work) {
  __shared__ __attribute__((aligned(16))) float2 lds[kColLds];
  __shared__ __attribute__((aligned(16))) float2 tw[16 * kTwRow];
  const int f = blockIdx.y;
  tw256_build(tw, threadIdx.x);
  cols_unit(x + (size_t)f * hop, win, work + (size_t)f * kN, blockIdx.x, threadIdx.x, lds, tw);
}

// ---- step 2: 32 rows p of one frame per workgroup (grid = 8 x frames, 512 threads).
//   b = c0 + 16 c1, q = q1 + 16 q0
//   pass 1 thread (c0, pl): DFT16 over c1, * W_256^(c0 q1)     -> LDS[q1][pl][c0]
//   pass 2 thread (pl, q1): DFT16 over c0 -> X[p + 256 (q1 + 16 q0)] -> dB -> fftshift
// LDS slot(q1, pl, c0) = 544 q1 + 17 pl + c0: pass 1's 16-lane groups write 16 consecutive
// slots; pass 2's lanes (pl) are 17 slots apart = 34 dwords = 2 pl mod 32 for the 16 lanes a ds_read2_b64 access
// serves at a time, so the data passes are conflict free (the conflicts the counters showed came from the twiddle
// table, see kTwRow).  32 consecutive p per store = one full 128-B line.
constexpr int kRowsPerWg = 32;
constexpr int kRowLds = 16 * 544;

// how the rows pass reads the intermediate: plain loads (two-kernel path: the kernel boundary
// made it visible) or agent-scope loads that miss the CU's L1 (fused path: written by other
// CUs of the same XCD during this kernel, served by their common L2)
template <bool kBypassL1>
__device__ __forceinline__ float2 load_work(const float2* p) {
  if (kBypassL1) {
    const unsigned long long v = __hip_atomic_load(
        (const PYSDR_AS1 unsigned long long*)p,
        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return make_float2(__uint_as_float((unsigned)(v & 0xffffffffull)), __uint_as_float((unsigned)(v >> 32)));
  }
  return ldg2(p);
}

// one unit = 32 rows [32 rb, 32 rb + 32) of frame yf, 512 threads, LDS kRowLds
template <bool kBypassL1>
__device__ __forceinline__ void rows_unit(const float2* yf, float* __restrict__ of, int rb, int db,
                                          int tid, float2* lds, const float2* tw) {
  {
    const int c0 = tid & 15, pl = tid >> 4;
    // Y[c1][p][c0]: a wave's load covers 512 contiguous bytes (4 rows x 16 columns)
    const float2* src = yf + (size_t)(rb * kRowsPerWg + pl) * 16 + c0;
    float2 u[16];
#pragma unroll
    for (int c1 = 0; c1 < 16; ++c1) u[c1] = load_work<kBypassL1>(src + 4096 * c1);
    dft16(u);
    __syncthreads();
    twiddle_tab(u, tw, c0);                                            // W_256^(c0 q1)
    float2* p = lds + 17 * pl + c0;
#pragma unroll
    for (int q1 = 0; q1 < 16; ++q1) p[544 * q1] = u[q1];
  }
  __syncthreads();
  {
    const int pl = tid & 31, q1 = tid >> 5;
    const float2* p = lds + 544 * q1 + 17 * pl;
    float2 v[16];
#pragma unroll
    for (int c0 = 0; c0 < 16; ++c0) v[c0] = p[c0];
    dft16(v);
    const int kb = rb * kRowsPerWg + pl + 256 * q1;
#pragma unroll
    for (int q0 = 0; q0 < 16; ++q0) {
      const int k = kb + 4096 * q0;
      float pw = v[q0].x * v[q0].x + v[q0].y * v[q0].y;
      // 10*log10(pw) = 10*log10(2) * log2(pw); pw + 1e-30 is a normal number, where v_log_f32 is
      // good to 1 ulp (log10f's expansion handles denormals and costs ~9 instructions per bin)
      if (db) pw = 3.0102999566398120f * __builtin_amdgcn_logf(pw + 1.0e-30f);
      stg1_stream(of + ((k + kM) & (kN - 1)), pw);
    }
  }
}

__global__ __launch_bounds__(512) void psd_rows_kernel(const float2* __restrict__ work,
                                                       float* __restrict__ out, int db) {
  __shared__ __attribute__((aligned(16))) float2 lds[kRowLds];
  __shared__ __attribute__((aligned(16))) float2 tw[16 * kTwRow];
  const int f = blockIdx.y;
  tw256_build(tw, threadIdx.x);
  rows_unit<false>(work + (size_t)f * kN, out + (size_t)f * kN, blockIdx.x, db, threadIdx.x, lds, tw);
}


// ---- the same pair with a 24-BIT intermediate (round 4).  The pair is bound by the bytes it moves across the XCD <->
// memory fabric (section 4.3 of DESIGN.md: 1.5 MB per frame, of which 1.0 MB is the intermediate written and read back),
// not by arithmetic, so the intermediate is stored as block-scaled 24-bit fixed point: 6 instead of 8 bytes per complex,
// 1.25 MB per frame.  Block = the 16 columns x 256 rows one columns workgroup produces; its scale maps the block's largest
// |component| to 8388600, so a stored value is off by at most 6e-8 of the block maximum -- the rows transform adds 256 of
// them incoherently (1e-6 of the block maximum) under a line that is at least ~16x the block's values: two orders inside the
// 5e-6 amplitude bar of psd_check.  The two planes keep every access a power of two wide: HI = the upper 16 bits of Re and Im
// in one dword per complex, LO = the low byte of each in one 16-bit word; same [cb][p][b] index order as the float2 form,
// so a wave's store / load covers 256 + 128 contiguous bytes.  v_perm_b32 packs and unpacks (6 vector instructions per
// complex on each side: +16 % on kernels that were never bound by them).
//   per frame (512 KB of the work buffer): [0, 256 K) HI dwords, [256 K, 384 K) LO shorts, [384 K, +256) the 16 x 4 block scales
constexpr int kPkLoOff = 65536 * 4, kPkScaleOff = 65536 * 6;

__device__ __forceinline__ unsigned pk_perm(unsigned s0, unsigned s1, unsigned sel) { return __builtin_amdgcn_perm(s0, s1, sel); }

__device__ __forceinline__ void cols_unit_pk(const float2* __restrict__ xf, const float* __restrict__ win,
                                             char* __restrict__ wf, int cb, int tid, float2* lds, const float2* tw,
                                             float* red) {
  const int b = tid & 15, hi = tid >> 4;
  const int bb = cb * kColsPerWg + b;
  {
    const int a0 = hi;
    float2 u[16];
#pragma unroll
    for (int a1 = 0; a1 < 8; ++a1) {
      const int n = 256 * (a0 + 16 * a1) + bb;
      const float2 s = ldg2_stream(xf + n);
      const float g = ldg1(win + n);
      u[a1] = make_float2(s.x * g, s.y * g);
    }
#pragma unroll
    for (int a1 = 8; a1 < 16; ++a1) u[a1] = make_float2(0.f, 0.f);
    dft16(u);
    __syncthreads();
    twiddle_tab(u, tw, a0);
    float2* p = lds + 16 * a0 + b;
#pragma unroll
    for (int p1 = 0; p1 < 16; ++p1) p[272 * p1] = u[p1];
  }
  __syncthreads();
  {
    const int p1 = hi;
    const float2* p = lds + 272 * p1 + b;
    float2 v[16];
#pragma unroll
    for (int a0 = 0; a0 < 16; ++a0) v[a0] = p[16 * a0];
    dft16(v);
    twiddle_pow0(v, expmpi((float)(16 * bb) * (1.0f / 32768.0f)),
                 expmpi((float)(bb * p1) * (1.0f / 32768.0f)));
    // the block's largest |component|: thread, wave (DPP-free butterflies through shuffles), workgroup.
    // Measured (scripts/diag/psd_variants.sh, PSD alone, ms per 10666 frames): shipped 2.27; a fixed scale (ablation PSDX_NO_SCALE,
    // results wrong; scripts/experiments/ablation_switches.patch.txt) 2.18; a scale per WAVE (-DPSDX_WAVE_SCALE: no barrier, no LDS round trip in front of the stores; parity
    // green) 2.35-2.41 against 2.35-2.37 on the same box: the barrier is not what the reduction costs.  Without the LO plane
    // (ablation PSDX_NO_LO, results wrong) 2.00, without both 1.85: the pair moves its bytes at ~6 TB/s in every variant.
    float m = 0.f;
#pragma unroll
    for (int p0 = 0; p0 < 16; ++p0) m = fmaxf(fmaxf(m, fabsf(v[p0].x)), fabsf(v[p0].y));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
#ifndef PSDX_WAVE_SCALE
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
#endif
    // (a block whose largest component is below 1e-20 contributes powers below 1e-36 * 65536: far under the 1e-30 that is
    //  added before the logarithm -- it is stored as zeros, which also keeps 8388600 / m finite for denormal m)
    const bool live = m >= 1.0e-20f;
    const float sc = live ? __fdiv_rn(8388600.0f, m) : 0.0f;
    // four scale slots per block, one per wave (the same value four times unless PSDX_WAVE_SCALE)
    if ((tid & 63) == 0)
      *(PYSDR_AS1 float*)(wf + kPkScaleOff + 4 * (4 * cb + (tid >> 6))) = live ? __fdiv_rn(m, 8388600.0f) * (1.0f / 256.0f) : 0.f;
    PYSDR_AS1 unsigned* oh = (PYSDR_AS1 unsigned*)wf + (size_t)cb * 4096 + p1 * 16 + b;
    PYSDR_AS1 unsigned short* ol = (PYSDR_AS1 unsigned short*)(wf + kPkLoOff) + (size_t)cb * 4096 + p1 * 16 + b;
#pragma unroll
    for (int p0 = 0; p0 < 16; ++p0) {
      const unsigned a = (unsigned)__float2int_rn(v[p0].x * sc), c = (unsigned)__float2int_rn(v[p0].y * sc);
      oh[p0 * 256] = pk_perm(c, a, 0x06050201u);                       // [a.b1, a.b2, c.b1, c.b2]
      ol[p0 * 256] = (unsigned short)pk_perm(c, a, 0x0c0c0400u);       // [a.b0, c.b0]
    }
  }
}

__global__ __launch_bounds__(256) void psd_cols_pk_unit_kernel(const float2* __restrict__ x, size_t hop,
                                                               const float* __restrict__ win, char* __restrict__ work) {
  __shared__ __attribute__((aligned(16))) float2 lds[kColLds];
  __shared__ __attribute__((aligned(16))) float2 tw[16 * kTwRow];
  __shared__ float red[4];
  const int f = blockIdx.y;
  tw256_build(tw, threadIdx.x);
  cols_unit_pk(x + (size_t)f * hop, win, work + (size_t)f * kN * sizeof(float2), blockIdx.x, threadIdx.x, lds, tw, red);
}


// ---- the same columns pass as a LOOP OVER FRAMES: grid = 16 x G, workgroup (cb, g) keeps column block cb and walks over
// the frames g, g + G, g + 2 G, ... of the launch (G = gridDim.y <= nframes: host_plan.h plan_psd_cols; all 16 G workgroups
// are resident at once, and no workgroup gets more than one frame more than another).  Nothing happens across workgroups.
// What a unit recomputed for every frame from inputs that never change is set up ONCE in front of the loop: the W_256 table
// (256 v_sin / v_cos pairs), the thread's 8 window values (8 L2 round trips in front of the first butterfly), and the 16
// four-step twiddles of twiddle_pow0 (two v_sin / v_cos pairs and 12 complex products that depend on (bb, p1) only).  The
// arithmetic of a frame is the unit's, operation by operation on the same values in the same order, so every bit of the
// intermediate is what psd_cols_pk_unit_kernel writes (tests/test_gpu_psd_cols_loop.py).
// A unit is a strict chain -- 16 loads, wait, DFT16, barrier, LDS, barrier, DFT16, reduce, barrier, 32 stores -- that only
// the CU's other three workgroups hide.  Here the 8 samples of the workgroup's NEXT frame are loaded while this one is
// transformed: issued in front of the first DFT16, taken at the top of the next iteration.  The loads come from inline asm
// and are waited for by hand (LABNOTES 7.4: hipcc cannot count vmcnt across a back edge and would wait for a prefetch it
// knows about in front of the first use of the CURRENT frame): "+v" ties the registers, so that nothing lies between the
// load and the wait that reads them, and the wait sits in front of the frame's stores -- vmcnt counts those too, and the
// loads have had the whole transform to land.
//   (saddr form: one 32-bit lane offset, the frame's base + 32 KB a1 in scalar registers)
__device__ __forceinline__ void cols_prefetch(v2f_t (&nx)[8], unsigned voff, const float2* xf) {
  const PYSDR_AS1 char* base = (const PYSDR_AS1 char*)xf;
#pragma unroll
  for (int a1 = 0; a1 < 8; ++a1)
    asm volatile("global_load_dwordx2 %0, %1, %2 nt" : "+v"(nx[a1]) : "v"(voff), "s"(base + 32768 * a1));
}
__device__ __forceinline__ void cols_prefetch_wait(v2f_t (&nx)[8]) {
  asm volatile("s_waitcnt vmcnt(0)"
               : "+v"(nx[0]), "+v"(nx[1]), "+v"(nx[2]), "+v"(nx[3]), "+v"(nx[4]), "+v"(nx[5]), "+v"(nx[6]), "+v"(nx[7]));
}

// (256 threads, four waves per SIMD: the 37 KB of LDS allow four workgroups per CU, so up to 128 registers cost nothing)
__global__ __launch_bounds__(256, 4) void psd_cols_pk_kernel(const float2* __restrict__ x, size_t hop,
                                                             const float* __restrict__ win, char* __restrict__ work,
                                                             int nframes) {
  __shared__ __attribute__((aligned(16))) float2 lds[kColLds];
  __shared__ __attribute__((aligned(16))) float2 tw[16 * kTwRow];
  __shared__ float red[4];
  const int tid = threadIdx.x, cb = blockIdx.x;
  const int b = tid & 15, hi = tid >> 4;
  const int bb = cb * kColsPerWg + b;
  PsdColsWalk fr((int)blockIdx.y, (int)gridDim.y, nframes);             // fr.f < nframes: the grid has at most nframes rows
  const unsigned voff = (unsigned)(256 * hi + bb) * (unsigned)sizeof(float2);   // sample n = 256 (a0 + 16 a1) + bb, a0 = hi
  v2f_t nx[8] = {};
  cols_prefetch(nx, voff, x + (size_t)fr.f * hop);                     // the first frame, behind which the set-up hides
  tw256_build(tw, tid);
  float g[8];
#pragma unroll
  for (int a1 = 0; a1 < 8; ++a1) g[a1] = ldg1(win + 256 * (hi + 16 * a1) + bb);
  // twiddle_pow0's factors W_65536^(bb (p1 + 16 p0)), p1 = hi: the same products in the same order, formed once
  float2 t[16];
  {
    const float2 w = expmpi((float)(16 * bb) * (1.0f / 32768.0f)), w0 = expmpi((float)(bb * hi) * (1.0f / 32768.0f));
    const float2 w2 = cmul(w, w), w4 = cmul(w2, w2), w8 = cmul(w4, w4);
    const float2 b0 = w0, b4 = cmul(w0, w4), b8 = cmul(w0, w8), b12 = cmul(b4, w8);
    const float2 w3 = cmul(w2, w);
    t[0] = b0; t[1] = cmul(b0, w); t[2] = cmul(b0, w2); t[3] = cmul(b0, w3);
    t[4] = b4; t[5] = cmul(b4, w); t[6] = cmul(b4, w2); t[7] = cmul(b4, w3);
    t[8] = b8; t[9] = cmul(b8, w); t[10] = cmul(b8, w2); t[11] = cmul(b8, w3);
    t[12] = b12; t[13] = cmul(b12, w); t[14] = cmul(b12, w2); t[15] = cmul(b12, w3);
  }
  float2* const p1w = lds + 16 * hi + b;                                // pass 1 writes slot(p1, a0 = hi, b)
  const float2* const p2r = lds + 272 * hi + b;                         // pass 2 reads slot(p1 = hi, a0, b)
  const size_t oidx = (size_t)cb * 4096 + hi * 16 + b;
  cols_prefetch_wait(nx);
  __syncthreads();                                                      // the table
  for (;;) {
    float2 u[16];
#pragma unroll
    for (int a1 = 0; a1 < 8; ++a1) {
      u[a1] = make_float2(nx[a1].x * g[a1], nx[a1].y * g[a1]);
      // the products are formed HERE, in front of the loads that overwrite nx: left alone, hipcc sinks them below the
      // prefetch and keeps the old samples alive in a second register block, which it then refills by copying the new
      // ones in front of their wait
      asm volatile("" : "+v"(u[a1].x), "+v"(u[a1].y));
    }
#pragma unroll
    for (int a1 = 8; a1 < 16; ++a1) u[a1] = make_float2(0.f, 0.f);
    if (fr.has_next()) cols_prefetch(nx, voff, x + (size_t)fr.fn * hop);   // never a frame the launch does not have
    dft16(u);
    twiddle_tab(u, tw, hi);
    // No barrier in front of these writes: every thread's pass-2 reads of the LAST frame lie in front of its reduction
    // barrier (C) below, which every thread has passed before any thread gets here.  The unit's first barrier was for the
    // table; in the loop, (C) of iteration i - 1 is what orders pass 2's LDS reads before iteration i's pass-1 writes.
#pragma unroll
    for (int p1 = 0; p1 < 16; ++p1) p1w[272 * p1] = u[p1];
    __syncthreads();                                                    // (B) pass 1 -> pass 2
    float2 v[16];
#pragma unroll
    for (int a0 = 0; a0 < 16; ++a0) v[a0] = p2r[16 * a0];
    dft16(v);
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = cmul(v[k], t[k]);
    float m = 0.f;
#pragma unroll
    for (int p0 = 0; p0 < 16; ++p0) m = fmaxf(fmaxf(m, fabsf(v[p0].x)), fabsf(v[p0].y));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    red[tid >> 6] = m;                     // every lane of the wave holds the same m: no single-lane block in front of (C)
    __syncthreads();                       // (C) the block maximum; red[] is rewritten only behind the next frame's (B)
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const bool live = m >= 1.0e-20f;
    const float sc = live ? __fdiv_rn(8388600.0f, m) : 0.0f;
    char* const wf = work + (size_t)fr.f * kN * sizeof(float2);
    cols_prefetch_wait(nx);                // the next frame's samples: in flight since the top of this iteration
    // the loop's one single-lane block (LABNOTES 7.1 (a)), behind the last barrier of the iteration
    if ((tid & 63) == 0)
      *(PYSDR_AS1 float*)(wf + kPkScaleOff + 4 * (4 * cb + (tid >> 6))) = live ? __fdiv_rn(m, 8388600.0f) * (1.0f / 256.0f) : 0.f;
    PYSDR_AS1 unsigned* oh = (PYSDR_AS1 unsigned*)wf + oidx;
    PYSDR_AS1 unsigned short* ol = (PYSDR_AS1 unsigned short*)(wf + kPkLoOff) + oidx;
#pragma unroll
    for (int p0 = 0; p0 < 16; ++p0) {
      const unsigned a = (unsigned)__float2int_rn(v[p0].x * sc), c = (unsigned)__float2int_rn(v[p0].y * sc);
      oh[p0 * 256] = pk_perm(c, a, 0x06050201u);
      ol[p0 * 256] = (unsigned short)pk_perm(c, a, 0x0c0c0400u);
    }
    if (!fr.has_next()) break;
    fr.advance();
  }
}

__device__ __forceinline__ void rows_unit_pk(const char* __restrict__ wf, float* __restrict__ of, int rb, int db,
                                             int tid, float2* lds, const float2* tw) {
  {
    const int c0 = tid & 15, pl = tid >> 4;
    const size_t idx = (size_t)(rb * kRowsPerWg + pl) * 16 + c0;
    const PYSDR_AS1 unsigned* sh = (const PYSDR_AS1 unsigned*)wf + idx;
    const PYSDR_AS1 unsigned short* sl = (const PYSDR_AS1 unsigned short*)(wf + kPkLoOff) + idx;
    const PYSDR_AS1 float* ss = (const PYSDR_AS1 float*)(wf + kPkScaleOff);
    unsigned h[16], l[16];
#pragma unroll
    for (int c1 = 0; c1 < 16; ++c1) { h[c1] = sh[4096 * c1]; l[c1] = sl[4096 * c1]; }
    float2 u[16];
#pragma unroll
    for (int c1 = 0; c1 < 16; ++c1) {
      const float inv = ss[4 * c1 + ((tid >> 6) & 3)];                   // block scale / 256 (wave-uniform: the wave's 4 rows p share p % 16 >> 2)
      const int xr = (int)pk_perm(l[c1], h[c1], 0x0100040cu);            // [0, l.b0, h.b0, h.b1] = Re * 256
      const int xi = (int)pk_perm(l[c1], h[c1], 0x0302050cu);            // [0, l.b1, h.b2, h.b3] = Im * 256
      u[c1] = make_float2((float)xr * inv, (float)xi * inv);
    }
    dft16(u);
    __syncthreads();
    twiddle_tab(u, tw, c0);
    float2* p = lds + 17 * pl + c0;
#pragma unroll
    for (int q1 = 0; q1 < 16; ++q1) p[544 * q1] = u[q1];
  }
  __syncthreads();
  {
    const int pl = tid & 31, q1 = tid >> 5;
    const float2* p = lds + 544 * q1 + 17 * pl;
    float2 v[16];
#pragma unroll
    for (int c0 = 0; c0 < 16; ++c0) v[c0] = p[c0];
    dft16(v);
    const int kb = rb * kRowsPerWg + pl + 256 * q1;
#pragma unroll
    for (int q0 = 0; q0 < 16; ++q0) {
      const int k = kb + 4096 * q0;
      float pw = v[q0].x * v[q0].x + v[q0].y * v[q0].y;
      if (db) pw = 3.0102999566398120f * __builtin_amdgcn_logf(pw + 1.0e-30f);
      stg1_stream(of + ((k + kM) & (kN - 1)), pw);
    }
  }
}

__global__ __launch_bounds__(512) void psd_rows_pk_unit_kernel(const char* __restrict__ work, float* __restrict__ out, int db) {
  __shared__ __attribute__((aligned(16))) float2 lds[kRowLds];
  __shared__ __attribute__((aligned(16))) float2 tw[16 * kTwRow];
  const int f = blockIdx.y;
  tw256_build(tw, threadIdx.x);
  rows_unit_pk(work + (size_t)f * kN * sizeof(float2), out + (size_t)f * kN, blockIdx.x, db, threadIdx.x, lds, tw);
}


// ---- the same rows pass as a LOOP OVER FRAMES, the columns loop's counterpart: grid = 8 x R, workgroup (rb, r) keeps row
// block rb and walks over the frames r, r + R, r + 2 R, ... of the launch (R = gridDim.y <= nframes: host_plan.h
// plan_psd_rows; all 8 R workgroups are resident at once, none gets more than one frame more than another).  Nothing happens
// across workgroups.  Set up ONCE in front of the loop: the W_256 table (256 v_sin / v_cos pairs and the barrier behind
// them) and every index that depends on (tid, rb) only.  The arithmetic of a frame is the unit's, operation by operation on
// the same values in the same order, so every bit of the PSD is what psd_rows_pk_unit_kernel writes
// (tests/test_gpu_psd_rows_loop.py).
// A unit is a strict chain -- 48 vector loads, wait, DFT16, barrier, LDS, barrier, DFT16, log, 16 stores -- that only the
// CU's one other workgroup hides.  Here the 16 HI dwords and 16 LO halfwords of the workgroup's NEXT frame are loaded while
// this one is transformed, the way cols_prefetch does it (inline asm, "+v" ties, waited for by hand in front of the frame's
// stores, taken at the top of the next iteration).  The 16 block scales a wave needs, ss[4 c1 + wave], are the same for all
// its lanes: they come over the scalar path (16 scalar loads from a base that holds the wave's slot; the unit spends 16
// vector loads per thread on them) into scalar registers, prefetched with the frame and waited for with it.  The intermediate
// was written by the columns kernel, a launch earlier on the same stream: nothing this kernel reads changes while it runs.
//   (saddr form: one 32-bit lane offset per plane; the frame's base + 16 KB c1 (HI) / + 256 KB + 8 KB c1 (LO) in scalar registers)
#define PYSDR_ROWS_SLOAD(c1, off) asm volatile("s_load_dword %0, %1, " #off : "+s"(ns[c1]) : "s"(sbase))
__device__ __forceinline__ void rows_prefetch(unsigned (&nh)[16], unsigned (&nl)[16], float (&ns)[16], unsigned voh, unsigned vol,
                                              const char* wf, int wave4) {
  const PYSDR_AS1 char* base = (const PYSDR_AS1 char*)wf;
#pragma unroll
  for (int c1 = 0; c1 < 16; ++c1)
    asm volatile("global_load_dword %0, %1, %2" : "+v"(nh[c1]) : "v"(voh), "s"(base + 16384 * c1));
#pragma unroll
  for (int c1 = 0; c1 < 16; ++c1)
    asm volatile("global_load_ushort %0, %1, %2" : "+v"(nl[c1]) : "v"(vol), "s"(base + kPkLoOff + 8192 * c1));
  const PYSDR_AS1 char* sbase = base + kPkScaleOff + wave4;              // slot 4 c1 + wave of the 16 x 4 scales
  PYSDR_ROWS_SLOAD(0, 0x00); PYSDR_ROWS_SLOAD(1, 0x10); PYSDR_ROWS_SLOAD(2, 0x20); PYSDR_ROWS_SLOAD(3, 0x30);
  PYSDR_ROWS_SLOAD(4, 0x40); PYSDR_ROWS_SLOAD(5, 0x50); PYSDR_ROWS_SLOAD(6, 0x60); PYSDR_ROWS_SLOAD(7, 0x70);
  PYSDR_ROWS_SLOAD(8, 0x80); PYSDR_ROWS_SLOAD(9, 0x90); PYSDR_ROWS_SLOAD(10, 0xa0); PYSDR_ROWS_SLOAD(11, 0xb0);
  PYSDR_ROWS_SLOAD(12, 0xc0); PYSDR_ROWS_SLOAD(13, 0xd0); PYSDR_ROWS_SLOAD(14, 0xe0); PYSDR_ROWS_SLOAD(15, 0xf0);
}
#undef PYSDR_ROWS_SLOAD
// one wait for both counters (the scalar loads count on lgkmcnt beside the LDS traffic, which hipcc counts without them:
// its own waits can only come out stricter); an asm statement takes 30 operands, so the LO plane and the scales are tied by
// two empty statements behind it -- volatile statements keep their order
__device__ __forceinline__ void rows_prefetch_wait(unsigned (&nh)[16], unsigned (&nl)[16], float (&ns)[16]) {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)"
               : "+v"(nh[0]), "+v"(nh[1]), "+v"(nh[2]), "+v"(nh[3]), "+v"(nh[4]), "+v"(nh[5]), "+v"(nh[6]), "+v"(nh[7]),
                 "+v"(nh[8]), "+v"(nh[9]), "+v"(nh[10]), "+v"(nh[11]), "+v"(nh[12]), "+v"(nh[13]), "+v"(nh[14]), "+v"(nh[15]));
  asm volatile(""
               : "+v"(nl[0]), "+v"(nl[1]), "+v"(nl[2]), "+v"(nl[3]), "+v"(nl[4]), "+v"(nl[5]), "+v"(nl[6]), "+v"(nl[7]),
                 "+v"(nl[8]), "+v"(nl[9]), "+v"(nl[10]), "+v"(nl[11]), "+v"(nl[12]), "+v"(nl[13]), "+v"(nl[14]), "+v"(nl[15]));
  asm volatile(""
               : "+s"(ns[0]), "+s"(ns[1]), "+s"(ns[2]), "+s"(ns[3]), "+s"(ns[4]), "+s"(ns[5]), "+s"(ns[6]), "+s"(ns[7]),
                 "+s"(ns[8]), "+s"(ns[9]), "+s"(ns[10]), "+s"(ns[11]), "+s"(ns[12]), "+s"(ns[13]), "+s"(ns[14]), "+s"(ns[15]));
}

// (512 threads and 72 KB of LDS: two workgroups per CU = four waves per SIMD, so up to 128 registers cost nothing)
__global__ __launch_bounds__(512, 4) void psd_rows_pk_kernel(const char* __restrict__ work, float* __restrict__ out, int db,
                                                             int nframes) {
  __shared__ __attribute__((aligned(16))) float2 lds[kRowLds];
  __shared__ __attribute__((aligned(16))) float2 tw[16 * kTwRow];
  const int tid = threadIdx.x, rb = blockIdx.x;
  PsdRowsWalk fr((int)blockIdx.y, (int)gridDim.y, nframes);             // fr.f < nframes: the grid has at most nframes rows
  // pass 1 thread (c0, pl): element (rb 32 + pl) 16 + c0 = 512 rb + tid of plane block c1
  const unsigned idx = 512u * (unsigned)rb + (unsigned)tid;
  const unsigned voh = idx * 4u, vol = idx * 2u;
  const int wave4 = 4 * __builtin_amdgcn_readfirstlane((tid >> 6) & 3);  // the wave's 4 rows p share (p % 16) >> 2
  unsigned nh[16] = {}, nl[16] = {};
  float ns[16] = {};
  rows_prefetch(nh, nl, ns, voh, vol, work + (size_t)fr.f * kN * sizeof(float2), wave4);   // the first frame, behind which the set-up hides
  tw256_build(tw, tid);
  const int c0 = tid & 15;
  float2* const p1w = lds + 17 * (tid >> 4) + c0;                        // pass 1 writes slot(q1, pl = tid >> 4, c0)
  const int pl = tid & 31, q1 = tid >> 5;
  const float2* const p2r = lds + 544 * q1 + 17 * pl;                    // pass 2 reads slot(q1, pl, c0 = 0 .. 15)
  // bin k = kb + 4096 q0 with kb < 4096, so its fftshifted place (k + 32768) & 65535 is kb + 4096 ((q0 + 8) & 15)
  const unsigned kbo = (unsigned)(rb * kRowsPerWg + pl + 256 * q1) * (unsigned)sizeof(float);
  rows_prefetch_wait(nh, nl, ns);
  __syncthreads();                                                      // the table
  for (;;) {
    float2 u[16];
#pragma unroll
    for (int c1 = 0; c1 < 16; ++c1) {
      const float inv = ns[c1];                                          // block scale / 256
      const int xr = (int)pk_perm(nl[c1], nh[c1], 0x0100040cu);          // [0, l.b0, h.b0, h.b1] = Re * 256
      const int xi = (int)pk_perm(nl[c1], nh[c1], 0x0302050cu);          // [0, l.b1, h.b2, h.b3] = Im * 256
      u[c1] = make_float2((float)xr * inv, (float)xi * inv);
      // formed HERE, in front of the loads that overwrite nh / nl / ns (see psd_cols_pk_kernel)
      asm volatile("" : "+v"(u[c1].x), "+v"(u[c1].y));
    }
    if (fr.has_next()) rows_prefetch(nh, nl, ns, voh, vol, work + (size_t)fr.fn * kN * sizeof(float2), wave4);   // never a frame the launch does not have
    dft16(u);
    twiddle_tab(u, tw, c0);                                              // W_256^(c0 q1)
    // No barrier in front of these writes: (C) of the last iteration lies behind every thread's pass-2 reads of it.
#pragma unroll
    for (int k = 0; k < 16; ++k) p1w[544 * k] = u[k];
    __syncthreads();                                                    // (B) pass 1 -> pass 2
    float2 v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = p2r[k];
    __syncthreads();                                                    // (C) pass 2 has read: the next frame's pass 1 may write
    dft16(v);
    float pw[16];
#pragma unroll
    for (int q0 = 0; q0 < 16; ++q0) {
      pw[q0] = v[q0].x * v[q0].x + v[q0].y * v[q0].y;
      if (db) pw[q0] = 3.0102999566398120f * __builtin_amdgcn_logf(pw[q0] + 1.0e-30f);
    }
    rows_prefetch_wait(nh, nl, ns);        // the next frame: in flight since the top of this iteration
    // (the frame's base + 16 KB ((q0 + 8) & 15) in scalar registers, one 32-bit lane offset)
    PYSDR_AS1 char* const o = (PYSDR_AS1 char*)(out + (size_t)fr.f * kN);
#pragma unroll
    for (int q0 = 0; q0 < 16; ++q0) {
      PYSDR_AS1 char* oq = o + 16384 * ((q0 + 8) & 15);
      asm("" : "+s"(oq));                  // kept a scalar base: reassociated with kbo it becomes a 64-bit vector sum per store
      __builtin_nontemporal_store(pw[q0], (PYSDR_AS1 float*)(oq + kbo));
    }
    if (!fr.has_next()) break;
    fr.advance();
  }
}

}  // namespace

// nframes frames; `work` holds nframes x 65536 complex of intermediate.
// form (host_plan.h psd_launch_form): 0 = float2 intermediate; otherwise the 24-bit intermediate, with the columns form in the
// low 16 bits (psd_form: 1 = one columns unit per workgroup, 1 + G = the loop over frames on 16 x min(G, nframes) workgroups)
// and the rows form above them (psd_rows_form: 0 = one rows unit per workgroup, R = the loop on 8 x min(R, nframes))
int launch_psd64k(const float2* x, size_t hop, int nframes, const float* win, float2* work,
                  float* out, int db, hipStream_t st, int form) {
  const int cform = form & 0xffff, rform = form >> 16;
  if (cform >= 1) {
    if (cform > 1) {
      const int rows = std::min(cform - 1, nframes);
      hipLaunchKernelGGL(psd_cols_pk_kernel, dim3(256 / kColsPerWg, rows), dim3(256), 0, st, x, hop, win, (char*)work, nframes);
    } else {
      hipLaunchKernelGGL(psd_cols_pk_unit_kernel, dim3(256 / kColsPerWg, nframes), dim3(256), 0, st, x, hop, win, (char*)work);
    }
    PYSDR_HIP_CHECK(hipGetLastError());
    if (rform > 0) {
      hipLaunchKernelGGL(psd_rows_pk_kernel, dim3(256 / kRowsPerWg, std::min(rform, nframes)), dim3(512), 0, st, (const char*)work, out, db, nframes);
    } else {
      hipLaunchKernelGGL(psd_rows_pk_unit_kernel, dim3(256 / kRowsPerWg, nframes), dim3(512), 0, st, (const char*)work, out, db);
    }
    PYSDR_HIP_CHECK(hipGetLastError());
    return PYSDR_OK;
  }
  hipLaunchKernelGGL(psd_cols_kernel, dim3(256 / kColsPerWg, nframes), dim3(256), 0, st, x, hop, win,
                     work);
  PYSDR_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(psd_rows_kernel, dim3(256 / kRowsPerWg, nframes), dim3(512), 0, st, work, out, db);
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

}  // namespace pysdr
