// Wideband RTTY decoder bank: the reference's per-bin Baudot decoder (RTTY_Decoder.decode, rtty.py:483-565,609-700)
// and its signal finder (RTTY_Executive.find_sigs, :744-764) for every bin of a contiguous range at once.
// Spec: line n = 1, 2, ... of the flipped dB filterbank; for the decoder at mark bin b
//   d_n     = f32(line[b] - line[b + NBINS])
//   score_n[s] = sum_k H[s][k] d_{n-31+k}: 4 x stop(+1), 4 x start(-1), bits of s LSB first x4, 4 x stop(+1)
//   isym_n  = first argmax, best_n its score;  sc2_n = best_n + best_{n-30} + ... + best_{n-120}
//   n % 30 == 0: t = n - 30 + first argmax of sc2 over lines n-29..n; if t - tlast >= 25 the symbol held since
//   the last decision is gated by snr2 (mean of +-(mark - space) at lines tlast - 28 + 4k) >= 8; then tlast = t,
//   sym = isym_{t+1}.  Everything before line 1 is 0 (the FIFOs start zeroed).
// The parallel form: every quantity but the LTRS/FIGS shift bit is a function of a bounded window of lines, so the
// state is a ring of the last R lines of per-line quantities (R = max_lines + 128 > the deepest reach, 120 lines of
// best for sc2) and one call runs
//   rt_gather   (line, band column)  the call's lines into the band ring (either line order)
//   rt_s4       (line, bin)          S4_n = d_{n-3} + d_{n-2} + d_{n-1} + d_n
//   rt_best     (line, bin)          best/isym in the per-bit form: the 32 templates share 8 group sums S4_{n-28+4g},
//                                    so the best symbol takes bit b = (S4 of bit b > 0), ties -> 0 (= lowest index);
//                                    a window with an infinite or NaN group sum scores the 32 templates one by one
//   rt_sc2      (line, bin)
//   rt_decide   (decision, bin)      t, tlast (= the previous window's argmax, recomputed), held symbol, snr2
//   rt_emit     (bin)                one serial pass over the call's decisions carrying only `shift`
//   rt_find     (line)               the finder's 21-line sums and their count
// Sums are taken in the order NumPy takes them in the reference (sc2 sequential from best_n; snr2 and the finder
// pairwise), so a difference from it comes only from the 32 x 32 float32 matmul, whose order BLAS decides.
#include "objects_plan.h"

namespace pysdr {
namespace {

__device__ __forceinline__ size_t rrow(long long n, int R) { return (size_t)(n % R); }

__global__ __launch_bounds__(256) void rt_gather(const float* __restrict__ lines, int nfft, int flipped, int band_lo,
                                                 int nband, long long n0, int R, float* __restrict__ band) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= nband) return;
  const int l = blockIdx.y;
  const int bin = band_lo + c;
  const int col = flipped ? bin : nfft - 1 - bin;                 // flipped = 0: np.flipud not yet applied
  band[rrow(n0 + l, R) * nband + c] = lines[(size_t)l * nfft + col];
}

// value of a ring at line x of column k, 0 before line 1
__device__ __forceinline__ float at(const float* ring, long long x, int R, int w, int k) {
  return x >= 1 ? ring[rrow(x, R) * w + k] : 0.f;
}

__device__ __forceinline__ float dline(const float* band, long long x, int R, int nband, int m, int nsh) {
  if (x < 1) return 0.f;
  const float* row = band + rrow(x, R) * nband;
  return row[m] - row[m + nsh];
}

__global__ __launch_bounds__(256) void rt_s4(const float* __restrict__ band, int nband, int moff, int nsh, int nb,
                                             long long n0, int R, float* __restrict__ s4) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= nb) return;
  const long long n = n0 + blockIdx.y;
  const int m = moff + k;
  float a = dline(band, n - 3, R, nband, m, nsh);
  a += dline(band, n - 2, R, nband, m, nsh);
  a += dline(band, n - 1, R, nband, m, nsh);
  a += dline(band, n, R, nband, m, nsh);
  s4[rrow(n, R) * nb + k] = a;
}

__global__ __launch_bounds__(256) void rt_best(const float* __restrict__ s4, int nb, long long n0, int R,
                                               float* __restrict__ best, int* __restrict__ isym) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= nb) return;
  const long long n = n0 + blockIdx.y;
  // group g covers lines n-31+4g .. n-28+4g: g = 0 stop, 1 start, 2..6 bits b0..b4, 7 stop
  const float s0 = at(s4, n - 28, R, nb, k), s1 = at(s4, n - 24, R, nb, k), s7 = at(s4, n, R, nb, k);
  float g[5];
#pragma unroll
  for (int b = 0; b < 5; ++b) g[b] = at(s4, n - 20 + 4 * b, R, nb, k);
  float v = s0 - s1;
  int sym = 0;
  bool finite = __builtin_isfinite(s0) && __builtin_isfinite(s1) && __builtin_isfinite(s7);
#pragma unroll
  for (int b = 0; b < 5; ++b) {
    sym |= (g[b] > 0.f) << b;
    v += fabsf(g[b]);
    finite = finite && __builtin_isfinite(g[b]);
  }
  v += s7;
  if (!finite) {
    // Every template weighs every group by +-1, so each of the reference's 32 scores is +-inf or NaN, whatever order
    // its matmul adds in: score them and take np.argmax's choice (the first NaN, else the first maximum).
    for (int c = 0; c < 32; ++c) {
      float sc = s0 - s1;
#pragma unroll
      for (int b = 0; b < 5; ++b) sc += ((c >> b) & 1) ? g[b] : -g[b];
      sc += s7;
      if (c == 0 || sc > v || (sc != sc && v == v)) { sym = c; v = sc; }
    }
  }
  best[rrow(n, R) * nb + k] = v;
  isym[rrow(n, R) * nb + k] = sym;
}

__global__ __launch_bounds__(256) void rt_sc2(const float* __restrict__ best, int nb, long long n0, int R,
                                              float* __restrict__ sc2) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= nb) return;
  const long long n = n0 + blockIdx.y;
  float v = at(best, n, R, nb, k);                                // np.sum(sc_buf.x[-1::-M]): best_n first
#pragma unroll
  for (int i = 1; i < 5; ++i) v += at(best, n - i * kM, R, nb, k);
  sc2[rrow(n, R) * nb + k] = v;
}

// first argmax of sc2 over lines n-29..n (n >= 30), NaN first as np.argmax
__device__ __forceinline__ int argmax30(const float* sc2, long long n, int R, int nb, int k) {
  int bi = 0;
  float bv = sc2[rrow(n - 29, R) * nb + k];
  for (int i = 1; i < kM; ++i) {
    const float v = sc2[rrow(n - 29 + i, R) * nb + k];
    if (v > bv || (v != v && bv == bv)) { bi = i; bv = v; }
  }
  return bi;
}

__global__ __launch_bounds__(256) void rt_decide(const float* __restrict__ band, const float* __restrict__ sc2,
                                                 const int* __restrict__ isym, int nband, int moff, int nsh, int nb,
                                                 long long n_first, int R, long long* __restrict__ t_out,
                                                 double* __restrict__ snr_out, int* __restrict__ held_out) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= nb) return;
  const int j = blockIdx.y;
  const long long n = n_first + (long long)kM * j;
  const long long t = n - kM + argmax30(sc2, n, R, nb, k);
  long long tlast = 0;                                            // initial state: tlast = 0, sym = 0
  int held = 0;
  if (n > kM) {
    tlast = n - 2 * kM + argmax30(sc2, n - kM, R, nb, k);
    held = isym[rrow(tlast + 1, R) * nb + k];
  }
  double snr = __builtin_nan("");
  if (t - tlast >= 25) {
    // compute_snr: bits [1, 0, b0..b4, 1] at lines tlast-28+4q, float64, in the reference's form: every mark and space
    // on the path is also multiplied by 0, so one that is infinite makes snr2 NaN as there (finite: +-(mark - space))
    const int m = moff + k;
    double a[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const long long x = tlast - 28 + 4 * q;
      double mk = 0.0, sp = 0.0;
      if (x >= 1) {
        const float* row = band + rrow(x, R) * nband;
        mk = (double)row[m];
        sp = (double)row[m + nsh];
      }
      const double bit = q == 0 ? 1.0 : q == 1 ? 0.0 : q == 7 ? 1.0 : (double)((held >> (q - 2)) & 1);
      const double signal = bit * mk + (1.0 - bit) * sp, noise = (1.0 - bit) * mk + bit * sp;
      a[q] = signal - noise;
    }
    snr = (((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))) / 8.0;
  }
  const size_t o = (size_t)j * nb + k;
  t_out[o] = t;
  snr_out[o] = snr;
  held_out[o] = held;
}

// decode_symbol (rtty.py:667-700) in order of decisions; -1 = nothing emitted, else sym + 32 * shift
__global__ __launch_bounds__(256) void rt_emit(const double* __restrict__ snr, const int* __restrict__ held, int nb,
                                               int ndec, int* __restrict__ shift, int* __restrict__ code) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= nb) return;
  int sh = shift[k];
  for (int j = 0; j < ndec; ++j) {
    const size_t o = (size_t)j * nb + k;
    int c = -1;
    if (snr[o] >= 8.0 && __builtin_isfinite(snr[o])) {            // THRESH; a snr2 that is not finite emits nothing
      const int s = held[o];
      if (s == 31) sh = 0;
      else if (s == 27) sh = 1;
      else if (s != 0) c = s + 32 * sh;
    }
    code[o] = c;
  }
  shift[k] = sh;
}

// find_sigs: bins [find_lo, find_hi) whose sum over the last 21 lines of |f32(mark - space)| exceeds 20 * 21
__global__ __launch_bounds__(256) void rt_find(const float* __restrict__ band, int nband, int flo, int fhi, int nsh,
                                               long long n0, int R, int* __restrict__ ndet) {
  __shared__ int cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  const long long n = n0 + blockIdx.x;
  int mine = 0;
  for (int m = flo + threadIdx.x; m < fhi; m += 256) {
    double a[21];
#pragma unroll
    for (int q = 0; q < 21; ++q) a[q] = (double)fabsf(dline(band, n - 20 + q, R, nband, m, nsh));
    // np.sum of 21 float64: pairwise with eight accumulators, then the tail
    double r0 = a[0] + a[8], r1 = a[1] + a[9], r2 = a[2] + a[10], r3 = a[3] + a[11];
    double r4 = a[4] + a[12], r5 = a[5] + a[13], r6 = a[6] + a[14], r7 = a[7] + a[15];
    double s = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
#pragma unroll
    for (int q = 16; q < 21; ++q) s += a[q];
    mine += s > 420.0;
  }
  if (mine) atomicAdd(&cnt, mine);
  __syncthreads();
  if (threadIdx.x == 0) ndet[blockIdx.x] = cnt;
}

}  // namespace

int launch_rtty_decode(const RttyArgs& a, hipStream_t st) {
  const int gb = (a.nb + 255) / 256;
  hipLaunchKernelGGL(rt_gather, dim3((a.nband + 255) / 256, a.nlines), dim3(256), 0, st, a.lines, a.nfft, a.flipped, a.band_lo,
                     a.nband, a.n0, a.R, a.band);
  hipLaunchKernelGGL(rt_s4, dim3(gb, a.nlines), dim3(256), 0, st, a.band, a.nband, a.moff, a.nsh, a.nb, a.n0, a.R, a.s4);
  hipLaunchKernelGGL(rt_best, dim3(gb, a.nlines), dim3(256), 0, st, a.s4, a.nb, a.n0, a.R, a.best, a.isym);
  hipLaunchKernelGGL(rt_sc2, dim3(gb, a.nlines), dim3(256), 0, st, a.best, a.nb, a.n0, a.R, a.sc2);
  if (a.nd > 0) {
    hipLaunchKernelGGL(rt_decide, dim3(gb, a.nd), dim3(256), 0, st, a.band, a.sc2, a.isym, a.nband, a.moff, a.nsh, a.nb,
                       a.n_first, a.R, a.t, a.snr, a.held);
    hipLaunchKernelGGL(rt_emit, dim3(gb), dim3(256), 0, st, a.snr, a.held, a.nb, a.nd, a.shift, a.code);
  }
  hipLaunchKernelGGL(rt_find, dim3(a.nlines), dim3(256), 0, st, a.band, a.nband, a.flo, a.fhi, a.nsh, a.n0, a.R, a.ndet);
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

}  // namespace pysdr
