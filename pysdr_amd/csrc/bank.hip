// Channel bank: a channelizer plus, on every row a < nk, a sub-receiver's stage 2 in mode AM or NFM -- detector, real AF
// FIR, block AGC and the NFM noise squelch.  With y_a[m] the channelizer's row (0 for m < 0) and
// c[0 .. T) the AF taps:
//   d[m]  = |y[m]|                                                   (AM)
//         = f32(fs_out / (2 pi 5000)) fm(y[m-2], y[m-1], y[m])       (NFM: the discriminator of sigs/nfm.m:124-127)
//   a[m]  = sum_{i<T} c[i] d[m - i]                                  (partial sums of eight taps, i ascending: the same bits in any call)
//   am[m] = a[m] gain,  one gain per call and channel: the call is the AGC block, as a chunk is for a sub-receiver.
// The bank owns Y[nk][Hpad + out_cap]: the channelizer writes a call's outputs to Y + Hpad with that pitch, the Hpad
// samples in front of them are the row's history -- history and new samples are contiguous, nothing is gathered or
// copied.  Per call, all on the channelizer's stream:
//   bank_kernel<MODE>  grid (tiles, nk), 256 threads x 8 consecutive outputs.  The workgroup turns TILE + T + 1 samples
//       of its row into TILE + T - 1 detector outputs in LDS; a thread slides a register window of 15 of them over the
//       taps, eight taps a step (two 16-byte LDS reads, 64 fmas; the taps are uniform: scalar loads).  It stores a and
//       leaves one partial max |a| and one partial sum |d[m] - 2 d[m-1] + d[m-2]| (float64) per (channel, tile): no
//       atomics, the reduction order is fixed by the launch geometry alone.
//   bank_finish        one workgroup per channel: folds the partials in a fixed order, runs the oracle's float32 AGC and
//       squelch updates (one lane), scales the row in place where the gain is not 1, and moves the last Hpad samples of
//       the row to its front (read, barrier, write: the ranges may overlap).
// A call that completes no output launches neither and changes no state.
//
// The complex-tap modes USB / LSB / CW run bank_cplx_kernel in bank_kernel's place: with c[0 .. T)
// complex taps,
//   d[m]  = y[m]                                                     (USB, LSB: they differ in the taps only)
//         = y[m] exp(j 2 pi ph(m) / 2^32),  ph(m) = fword m mod 2^32 taken as signed: m the absolute output index  (CW)
//   a[m]  = Re sum_{i<T} c[i] d[m - i] = sum_i cr[i] dr[m - i] + sum_i (-ci[i]) di[m - i]
// Same grid, threads and outputs per thread; the detector output lies in LDS as two planes (re, im), the taps arrive as
// [cr | -ci] so that every term is an fma, and a step of eight taps forms one partial sum of its eight real-plane
// products and one of its eight imaginary-plane products (tap ascending), adds the two and adds that to the output's
// sum: the order depends on the tap index alone, so the bits do not depend on the call.  psum is written as 0 (no
// squelch in these modes) and bank_finish follows unchanged.
#include "objects_plan.h"

namespace pysdr {
namespace {

constexpr float kAgcBeta = 0.1f, kAgcGainMax = 1.0e4f, kAgcFloor = 1e-12f;
constexpr float kBankSqAlpha = 0.64f;

// max that keeps a NaN, as np.max does
__device__ __forceinline__ float nanmax(float a, float b) { return (a != a) ? a : ((b != b) ? b : fmaxf(a, b)); }

template <int MODE>   // PYSDR_AM | PYSDR_NFM
__device__ __forceinline__ float bank_detect(const float2* y, int i, float fm_scale) {
  const float2 yc = y[i];
  if (MODE == PYSDR_AM) return sqrtf(yc.x * yc.x + yc.y * yc.y);
  const float2 y1 = y[i - 1], ya = y[i - 2];
  const float dr = yc.x - ya.x, di = yc.y - ya.y;
  const float fm = y1.x * di - y1.y * dr;
  const float den = 2.f * (y1.x * y1.x + y1.y * y1.y) + 1e-20f;
  return (fm / den) * fm_scale;
}

// one step of eight taps c[0 .. 8) = taps 8 b ..: w[q] = d[o0 - 8 b - 7 + q], output j and tap t meet at q = j - t + 7.
// The step's eight products are summed on their own (t ascending) and then added to the output's sum: a chain of 255
// fmas carries its rounding through every later tap -- measured against the float64 helper 4.9e-6 of full scale on the
// tests' base input, where the float32 helper is at 5e-7 -- partial sums of eight are at 6.5e-7.
template <bool GUARD>
__device__ __forceinline__ void bank_step(const float* __restrict__ c, int left, const float (&w)[16], float (&acc)[kBankW]) {
  float part[kBankW];
  const float c0 = c[0];
#pragma unroll
  for (int j = 0; j < kBankW; ++j) part[j] = c0 * w[j + 7];
#pragma unroll
  for (int t = 1; t < kBankW; ++t) {
    if (GUARD && t >= left) break;
    const float ct = c[t];
#pragma unroll
    for (int j = 0; j < kBankW; ++j) part[j] = __builtin_fmaf(ct, w[j - t + 7], part[j]);
  }
#pragma unroll
  for (int j = 0; j < kBankW; ++j) acc[j] += part[j];
}

template <int MODE>
__global__ __launch_bounds__(kBankThreads) void bank_kernel(const BankArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sd[];       // sd[e] = d[tile0 + e - (tp - 1)], e < kBankTile + tp
  __shared__ double wsum[kBankThreads / 64];
  __shared__ float wmax[kBankThreads / 64];
  const int tid = threadIdx.x, row = blockIdx.y;
  const int tile0 = blockIdx.x * kBankTile;
  const float2* y = a.y + (size_t)row * (size_t)a.ypitch;
  const int E = kBankTile + a.tp;
  for (int e = tid; e < E; e += kBankThreads) {
    const int rel = e - (a.tp - 1), i = tile0 + rel;               // d[i]; only rel >= -(T - 1) is ever multiplied
    sd[e] = (rel >= -(a.T - 1) && i < a.n_out) ? bank_detect<MODE>(y, i, a.fm_scale) : 0.f;
  }
  __syncthreads();

  const int o0 = kBankW * tid;                                      // the thread's first output, from tile0
  float acc[kBankW], w[16];
#pragma unroll
  for (int j = 0; j < kBankW; ++j) acc[j] = 0.f;
  {
    const float4 h0 = *reinterpret_cast<const float4*>(sd + o0 + a.tp), h1 = *reinterpret_cast<const float4*>(sd + o0 + a.tp + 4);
    w[8] = h0.x; w[9] = h0.y; w[10] = h0.z; w[11] = h0.w; w[12] = h1.x; w[13] = h1.y; w[14] = h1.z; w[15] = h1.w;
  }
  const int nstep = a.tp / kBankW, nfull = a.T / kBankW;
  for (int b = 0; b < nstep; ++b) {
    const float* s = sd + o0 + a.tp - 8 - 8 * b;                    // d[o0 - 8 b - 7 ..]
    const float4 l0 = *reinterpret_cast<const float4*>(s), l1 = *reinterpret_cast<const float4*>(s + 4);
    w[0] = l0.x; w[1] = l0.y; w[2] = l0.z; w[3] = l0.w; w[4] = l1.x; w[5] = l1.y; w[6] = l1.z; w[7] = l1.w;
    if (b < nfull) bank_step<false>(a.taps + 8 * b, 8, w, acc);
    else bank_step<true>(a.taps + 8 * b, a.T - 8 * b, w, acc);
#pragma unroll
    for (int q = 0; q < 7; ++q) w[8 + q] = w[q];                    // the next step's window lies 8 lower
  }

  const int ib = tile0 + o0;
  float* out = a.a + (size_t)row * (size_t)a.apitch;
  float m = 0.f;
  double nz = 0.0;
  if (ib + kBankW <= a.n_out) {
    float4* o = reinterpret_cast<float4*>(out + ib);
    o[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    o[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
  }
#pragma unroll
  for (int j = 0; j < kBankW; ++j)
    if (ib + j < a.n_out) {
      if (ib + kBankW > a.n_out) out[ib + j] = acc[j];
      m = nanmax(m, fabsf(acc[j]));
      if (MODE == PYSDR_NFM && a.noise) {
        const int e = o0 + j + a.tp - 1;                            // d[ib + j]
        nz += (double)fabsf(sd[e] - 2.f * sd[e - 1] + sd[e - 2]);
      }
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    m = nanmax(m, __shfl_xor(m, o));
    if (MODE == PYSDR_NFM) nz += __shfl_xor(nz, o);
  }
  if ((tid & 63) == 0) { wmax[tid >> 6] = m; wsum[tid >> 6] = nz; }
  __syncthreads();
  if (tid == 0) {
    float mm = wmax[0];
    double ss = wsum[0];
#pragma unroll
    for (int v = 1; v < kBankThreads / 64; ++v) { mm = nanmax(mm, wmax[v]); ss += wsum[v]; }
    a.pmax[(size_t)row * a.ptiles + blockIdx.x] = mm;
    a.psum[(size_t)row * a.ptiles + blockIdx.x] = ss;
  }
}

__global__ __launch_bounds__(kBankThreads) void bank_finish(const FinishArgs f) {
  __shared__ double ssum[kBankThreads];
  __shared__ float smax[kBankThreads];
  __shared__ float sgain;
  const int tid = threadIdx.x, row = blockIdx.x;
  float m = 0.f;
  double s = 0.0;
  for (int t = tid; t < f.ntiles; t += kBankThreads) {
    m = nanmax(m, f.pmax[(size_t)row * f.ptiles + t]);
    s += f.psum[(size_t)row * f.ptiles + t];
  }
  smax[tid] = m;
  ssum[tid] = s;
  __syncthreads();
  for (int h = kBankThreads / 2; h > 0; h >>= 1) {
    if (tid < h) { smax[tid] = nanmax(smax[tid], smax[tid + h]); ssum[tid] += ssum[tid + h]; }
    __syncthreads();
  }
  if (tid == 0) {
    // AGC.update(peak, active) and the block-noise squelch of the oracle, operation by operation in float32
    BankState st = f.state[row];
    const float peak = smax[0];
    st.maxbuf = peak;
    st.agc = (peak > st.agc) ? peak : __fadd_rn(st.agc, __fmul_rn(kAgcBeta, __fsub_rn(peak, st.agc)));
    float g = 1.f;
    if (f.agc_active) {
      const float den = (kAgcFloor > st.agc) ? kAgcFloor : st.agc;      // max() / min() of the oracle: a NaN stays
      const float q = __fdiv_rn(f.ref, den);
      g = (kAgcGainMax < q) ? kAgcGainMax : q;
    }
    st.gain = g;
    st.err = __fsub_rn(f.ref, __fmul_rn(g, peak));
    if (f.squelch) {
      const float noise = (float)(ssum[0] / (double)f.n_out);
      st.level = __fadd_rn(st.level, __fmul_rn(kBankSqAlpha, __fsub_rn(noise, st.level)));
      st.open = (st.level <= f.thresh) ? 1 : 0;
      if (!st.open) g = 0.f;
    }
    f.state[row] = st;
    sgain = g;
  }
  __syncthreads();
  const float g = sgain;
  if (__float_as_uint(g) != 0x3f800000u) {                             // a * 1 is a
    float* a = f.a + (size_t)row * (size_t)f.apitch;
    for (int i = tid; i < f.n_out; i += kBankThreads) a[i] = a[i] * g;
  }
  // new history = the last hpad samples of [history | outputs] (hpad <= 256 = one per thread)
  float2* y = f.ybase + (size_t)row * (size_t)f.ypitch;
  float2 keep = make_float2(0.f, 0.f);
  if (tid < f.hpad) keep = y[f.n_out + tid];
  __syncthreads();
  if (tid < f.hpad) y[tid] = keep;
}

// ---- the complex-tap modes ---------------------------------------------------------------------------------------------
// bank_step for complex taps: cr[0 .. 8) and cn[0 .. 8) = -ci of taps 8 b .., wr / wi the windows of the two planes.
template <bool GUARD>
__device__ __forceinline__ void bank_step_cplx(const float* __restrict__ cr, const float* __restrict__ cn, int left,
                                               const float (&wr)[16], const float (&wi)[16], float (&acc)[kBankW]) {
  float pr[kBankW], pi[kBankW];
  const float r0 = cr[0], n0 = cn[0];
#pragma unroll
  for (int j = 0; j < kBankW; ++j) { pr[j] = r0 * wr[j + 7]; pi[j] = n0 * wi[j + 7]; }
#pragma unroll
  for (int t = 1; t < kBankW; ++t) {
    if (GUARD && t >= left) break;
    const float rt = cr[t], nt = cn[t];
#pragma unroll
    for (int j = 0; j < kBankW; ++j) {
      pr[j] = __builtin_fmaf(rt, wr[j - t + 7], pr[j]);
      pi[j] = __builtin_fmaf(nt, wi[j - t + 7], pi[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < kBankW; ++j) acc[j] += pr[j] + pi[j];
}

template <bool BFO>   // false: USB / LSB, true: CW
__global__ __launch_bounds__(kBankThreads) void bank_cplx_kernel(const BankArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sd[];       // two planes of E floats: re, im of d[tile0 + e - (tp - 1)]
  __shared__ float wmax[kBankThreads / 64];
  const int tid = threadIdx.x, row = blockIdx.y;
  const int tile0 = blockIdx.x * kBankTile;
  const float2* y = a.y + (size_t)row * (size_t)a.ypitch;
  const int E = kBankTile + a.tp;                                   // a multiple of 8: the second plane is 16-byte aligned
  float* const sr = sd;
  float* const si = sd + E;
  for (int e = tid; e < E; e += kBankThreads) {
    const int rel = e - (a.tp - 1), i = tile0 + rel;               // d[i]; only rel >= -(T - 1) is ever multiplied
    float2 d = make_float2(0.f, 0.f);
    if (rel >= -(a.T - 1) && i < a.n_out) {
      d = y[i];
      if (BFO) {                                                    // stage2.hip's kDetBfo phase, once per sample
        const uint32_t ph = a.fword * (a.m0_lo + (uint32_t)i);
        const float half_turns = (float)(int)ph * (1.0f / 2147483648.0f);
        float s, c;
        sincospif(half_turns, &s, &c);                              // staging is 1 / 500 of the work: the accurate form is free
        d = make_float2(d.x * c - d.y * s, d.x * s + d.y * c);
      }
    }
    sr[e] = d.x;
    si[e] = d.y;
  }
  __syncthreads();

  const int o0 = kBankW * tid;
  float acc[kBankW], wr[16], wi[16];
#pragma unroll
  for (int j = 0; j < kBankW; ++j) acc[j] = 0.f;
  {
    const float4 r0 = *reinterpret_cast<const float4*>(sr + o0 + a.tp), r1 = *reinterpret_cast<const float4*>(sr + o0 + a.tp + 4);
    const float4 i0 = *reinterpret_cast<const float4*>(si + o0 + a.tp), i1 = *reinterpret_cast<const float4*>(si + o0 + a.tp + 4);
    wr[8] = r0.x; wr[9] = r0.y; wr[10] = r0.z; wr[11] = r0.w; wr[12] = r1.x; wr[13] = r1.y; wr[14] = r1.z; wr[15] = r1.w;
    wi[8] = i0.x; wi[9] = i0.y; wi[10] = i0.z; wi[11] = i0.w; wi[12] = i1.x; wi[13] = i1.y; wi[14] = i1.z; wi[15] = i1.w;
  }
  const float* __restrict__ cr = a.taps;                            // [tp] re, then [tp] -im
  const float* __restrict__ cn = a.taps + a.tp;
  const int nstep = a.tp / kBankW, nfull = a.T / kBankW;
  for (int b = 0; b < nstep; ++b) {
    const int at = o0 + a.tp - 8 - 8 * b;                           // d[o0 - 8 b - 7 ..]
    const float4 r0 = *reinterpret_cast<const float4*>(sr + at), r1 = *reinterpret_cast<const float4*>(sr + at + 4);
    const float4 i0 = *reinterpret_cast<const float4*>(si + at), i1 = *reinterpret_cast<const float4*>(si + at + 4);
    wr[0] = r0.x; wr[1] = r0.y; wr[2] = r0.z; wr[3] = r0.w; wr[4] = r1.x; wr[5] = r1.y; wr[6] = r1.z; wr[7] = r1.w;
    wi[0] = i0.x; wi[1] = i0.y; wi[2] = i0.z; wi[3] = i0.w; wi[4] = i1.x; wi[5] = i1.y; wi[6] = i1.z; wi[7] = i1.w;
    if (b < nfull) bank_step_cplx<false>(cr + 8 * b, cn + 8 * b, 8, wr, wi, acc);
    else bank_step_cplx<true>(cr + 8 * b, cn + 8 * b, a.T - 8 * b, wr, wi, acc);
#pragma unroll
    for (int q = 0; q < 7; ++q) { wr[8 + q] = wr[q]; wi[8 + q] = wi[q]; }
  }

  const int ib = tile0 + o0;
  float* out = a.a + (size_t)row * (size_t)a.apitch;
  float m = 0.f;
  if (ib + kBankW <= a.n_out) {
    float4* o = reinterpret_cast<float4*>(out + ib);
    o[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    o[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
  }
#pragma unroll
  for (int j = 0; j < kBankW; ++j)
    if (ib + j < a.n_out) {
      if (ib + kBankW > a.n_out) out[ib + j] = acc[j];
      m = nanmax(m, fabsf(acc[j]));
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = nanmax(m, __shfl_xor(m, o));
  if ((tid & 63) == 0) wmax[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
    float mm = wmax[0];
#pragma unroll
    for (int v = 1; v < kBankThreads / 64; ++v) mm = nanmax(mm, wmax[v]);
    a.pmax[(size_t)row * a.ptiles + blockIdx.x] = mm;
    a.psum[(size_t)row * a.ptiles + blockIdx.x] = 0.0;
  }
}

}  // namespace

int launch_bank(int mode, const BankPlan& p, const BankArgs& a, int ntiles, int nk, hipStream_t st) {
  const size_t lds = (size_t)p.lds_floats * sizeof(float);
  const dim3 grid(ntiles, nk), block(kBankThreads);
  if (mode == PYSDR_AM) hipLaunchKernelGGL(bank_kernel<PYSDR_AM>, grid, block, lds, st, a);
  else if (mode == PYSDR_NFM) hipLaunchKernelGGL(bank_kernel<PYSDR_NFM>, grid, block, lds, st, a);
  else if (mode == PYSDR_USB || mode == PYSDR_LSB) hipLaunchKernelGGL(bank_cplx_kernel<false>, grid, block, 2 * lds, st, a);
  else if (mode == PYSDR_CW) hipLaunchKernelGGL(bank_cplx_kernel<true>, grid, block, 2 * lds, st, a);
  else { set_last_error("launch_bank: mode %d", mode); return PYSDR_ERR_ARG; }
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

int launch_bank_finish(const FinishArgs& f, int nk, hipStream_t st) {
  hipLaunchKernelGGL(bank_finish, dim3(nk), dim3(kBankThreads), 0, st, f);
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

}  // namespace pysdr
