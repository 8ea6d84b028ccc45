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
#include "common.h"

struct pysdr_rtty {
  int device = 0, nfft = 0, nsh = 0, bin_lo = 0, bin_hi = 0, find_lo = 0, find_hi = 0, max_lines = 0;
  int nb = 0;              // decoders = bin_hi - bin_lo
  int band_lo = 0, nband = 0;
  int R = 0;               // ring rows; line n >= 1 lives in row n % R
  int max_dec = 0;         // decisions one call can complete
  long long n = 0;         // lines decoded so far
  float* d_lines = nullptr;     // staging for host lines [max_lines][nfft]
  float* d_band = nullptr;      // ring [R][nband]
  float* d_s4 = nullptr;        // ring [R][nb]
  float* d_best = nullptr;      // ring [R][nb]
  float* d_sc2 = nullptr;       // ring [R][nb]
  int* d_isym = nullptr;        // ring [R][nb]
  int* d_shift = nullptr;       // [nb]
  long long* d_t = nullptr;     // [max_dec][nb]
  double* d_snr = nullptr;      // [max_dec][nb]
  int* d_held = nullptr;        // [max_dec][nb]
  int* d_code = nullptr;        // [max_dec][nb]
  int* d_ndet = nullptr;        // [max_lines]
  hipStream_t stream = nullptr;
};

namespace pysdr {
namespace {

constexpr int kM = 30;                // lines per character (rtty.py:386)
constexpr int kHist = 128;            // ring rows beyond max_lines
constexpr int kMaxLines = 32768;

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
}  // namespace pysdr

using namespace pysdr;

extern "C" {

int pysdr_rtty_create(int device, int nfft, int nbins_shift, int bin_lo, int bin_hi, int find_lo, int find_hi,
                      int max_lines, pysdr_rtty** out) {
  if (!out) { set_last_error("pysdr_rtty_create: out is NULL"); return PYSDR_ERR_ARG; }
  *out = nullptr;
  if (nfft < 2 || nbins_shift < 1 || nbins_shift >= nfft) {
    set_last_error("pysdr_rtty_create: nfft %d / nbins_shift %d", nfft, nbins_shift);
    return PYSDR_ERR_ARG;
  }
  const int top = nfft - nbins_shift;
  if (bin_lo < 0 || bin_hi > top || bin_lo >= bin_hi) {
    set_last_error("pysdr_rtty_create: decoder bins [%d, %d) not a non-empty range inside [0, %d)", bin_lo, bin_hi, top);
    return PYSDR_ERR_ARG;
  }
  if (find_lo < 0 || find_hi > top || find_lo > find_hi) {
    set_last_error("pysdr_rtty_create: finder bins [%d, %d) not a range inside [0, %d)", find_lo, find_hi, top);
    return PYSDR_ERR_ARG;
  }
  if (max_lines < 1 || max_lines > kMaxLines) {
    set_last_error("pysdr_rtty_create: max_lines %d outside [1, %d]", max_lines, kMaxLines);
    return PYSDR_ERR_ARG;
  }
  hipError_t e0 = hipSetDevice(device);
  if (e0 != hipSuccess) { set_last_error("hipSetDevice(%d): %s", device, hipGetErrorString(e0)); return PYSDR_ERR_NO_DEVICE; }
  pysdr_rtty* r = new pysdr_rtty();
  r->device = device; r->nfft = nfft; r->nsh = nbins_shift; r->bin_lo = bin_lo; r->bin_hi = bin_hi;
  r->find_lo = find_lo; r->find_hi = find_hi; r->max_lines = max_lines;
  r->nb = bin_hi - bin_lo;
  r->band_lo = find_lo < find_hi ? (bin_lo < find_lo ? bin_lo : find_lo) : bin_lo;
  const int hi = find_lo < find_hi ? (bin_hi > find_hi ? bin_hi : find_hi) : bin_hi;
  r->nband = hi + nbins_shift - r->band_lo;                       // <= nfft - band_lo
  r->R = max_lines + kHist;
  r->max_dec = max_lines / kM + 1;
  const size_t ring = (size_t)r->R * r->nb, dec = (size_t)r->max_dec * r->nb;
#define CK(e) do { hipError_t _e = (e); if (_e != hipSuccess) { set_last_error("pysdr_rtty_create: %s -> %s", #e, hipGetErrorString(_e)); pysdr_rtty_destroy(r); return PYSDR_ERR_HIP; } } while (0)
  CK(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
  CK(hipMalloc(&r->d_lines, (size_t)max_lines * nfft * sizeof(float)));
  CK(hipMalloc(&r->d_band, (size_t)r->R * r->nband * sizeof(float)));
  CK(hipMalloc(&r->d_s4, ring * sizeof(float)));
  CK(hipMalloc(&r->d_best, ring * sizeof(float)));
  CK(hipMalloc(&r->d_sc2, ring * sizeof(float)));
  CK(hipMalloc(&r->d_isym, ring * sizeof(int)));
  CK(hipMalloc(&r->d_shift, (size_t)r->nb * sizeof(int)));
  CK(hipMalloc(&r->d_t, dec * sizeof(long long)));
  CK(hipMalloc(&r->d_snr, dec * sizeof(double)));
  CK(hipMalloc(&r->d_held, dec * sizeof(int)));
  CK(hipMalloc(&r->d_code, dec * sizeof(int)));
  CK(hipMalloc(&r->d_ndet, (size_t)max_lines * sizeof(int)));
#undef CK
  const int rc = pysdr_rtty_reset(r);
  if (rc != PYSDR_OK) { pysdr_rtty_destroy(r); return rc; }
  *out = r;
  return PYSDR_OK;
}

void pysdr_rtty_destroy(pysdr_rtty* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  if (r->stream) (void)hipStreamSynchronize(r->stream);
  for (void* p : {(void*)r->d_lines, (void*)r->d_band, (void*)r->d_s4, (void*)r->d_best, (void*)r->d_sc2, (void*)r->d_isym,
                  (void*)r->d_shift, (void*)r->d_t, (void*)r->d_snr, (void*)r->d_held, (void*)r->d_code, (void*)r->d_ndet})
    if (p) (void)hipFree(p);
  if (r->stream) (void)hipStreamDestroy(r->stream);
  delete r;
}

int pysdr_rtty_reset(pysdr_rtty* r) {
  if (!r) { set_last_error("pysdr_rtty_reset: NULL decoder"); return PYSDR_ERR_ARG; }
  PYSDR_HIP_CHECK(hipSetDevice(r->device));
  const size_t ring = (size_t)r->R * r->nb;
  PYSDR_HIP_CHECK(hipMemsetAsync(r->d_band, 0, (size_t)r->R * r->nband * sizeof(float), r->stream));
  PYSDR_HIP_CHECK(hipMemsetAsync(r->d_s4, 0, ring * sizeof(float), r->stream));
  PYSDR_HIP_CHECK(hipMemsetAsync(r->d_best, 0, ring * sizeof(float), r->stream));
  PYSDR_HIP_CHECK(hipMemsetAsync(r->d_sc2, 0, ring * sizeof(float), r->stream));
  PYSDR_HIP_CHECK(hipMemsetAsync(r->d_isym, 0, ring * sizeof(int), r->stream));
  PYSDR_HIP_CHECK(hipMemsetAsync(r->d_shift, 0, (size_t)r->nb * sizeof(int), r->stream));   // shift off
  PYSDR_HIP_CHECK(hipStreamSynchronize(r->stream));
  r->n = 0;
  return PYSDR_OK;
}

int pysdr_rtty_decode(pysdr_rtty* r, const float* lines, int nlines, int on_device, int flipped, int* codes,
                      long long* t, double* snr2, int* n_dec, int* ndet, int* isym, float* best) {
  if (!r) { set_last_error("pysdr_rtty_decode: NULL decoder"); return PYSDR_ERR_ARG; }
  if (nlines < 0 || nlines > r->max_lines) {
    set_last_error("pysdr_rtty_decode: nlines %d outside [0, max_lines = %d]", nlines, r->max_lines);
    return PYSDR_ERR_ARG;
  }
  if ((nlines > 0 && !lines) || !codes || !t || !snr2 || !n_dec || !ndet) {
    set_last_error("pysdr_rtty_decode: NULL lines, codes, t, snr2, n_dec or ndet");
    return PYSDR_ERR_ARG;
  }
  *n_dec = 0;
  if (nlines == 0) return PYSDR_OK;
  PYSDR_HIP_CHECK(hipSetDevice(r->device));
  hipStream_t st = r->stream;
  const long long n0 = r->n + 1, n1 = r->n + nlines;                 // lines n0..n1
  const long long j_first = r->n / kM + 1, j_last = n1 / kM;         // decisions at n = 30 j
  const int nd = (int)(j_last - j_first + 1);                        // <= nlines / 30 + 1 = max_dec
  const float* src = lines;
  if (!on_device) {
    PYSDR_HIP_CHECK(hipMemcpyAsync(r->d_lines, lines, (size_t)nlines * r->nfft * sizeof(float), hipMemcpyHostToDevice, st));
    src = r->d_lines;
  }
  const int gb = (r->nb + 255) / 256;
  const int moff = r->bin_lo - r->band_lo;
  hipLaunchKernelGGL(rt_gather, dim3((r->nband + 255) / 256, nlines), dim3(256), 0, st, src, r->nfft, flipped ? 1 : 0,
                     r->band_lo, r->nband, n0, r->R, r->d_band);
  hipLaunchKernelGGL(rt_s4, dim3(gb, nlines), dim3(256), 0, st, r->d_band, r->nband, moff, r->nsh, r->nb, n0, r->R, r->d_s4);
  hipLaunchKernelGGL(rt_best, dim3(gb, nlines), dim3(256), 0, st, r->d_s4, r->nb, n0, r->R, r->d_best, r->d_isym);
  hipLaunchKernelGGL(rt_sc2, dim3(gb, nlines), dim3(256), 0, st, r->d_best, r->nb, n0, r->R, r->d_sc2);
  if (nd > 0) {
    hipLaunchKernelGGL(rt_decide, dim3(gb, nd), dim3(256), 0, st, r->d_band, r->d_sc2, r->d_isym, r->nband, moff, r->nsh,
                       r->nb, j_first * kM, r->R, r->d_t, r->d_snr, r->d_held);
    hipLaunchKernelGGL(rt_emit, dim3(gb), dim3(256), 0, st, r->d_snr, r->d_held, r->nb, nd, r->d_shift, r->d_code);
  }
  hipLaunchKernelGGL(rt_find, dim3(nlines), dim3(256), 0, st, r->d_band, r->nband, r->find_lo - r->band_lo,
                     r->find_hi - r->band_lo, r->nsh, n0, r->R, r->d_ndet);
  PYSDR_HIP_CHECK(hipGetLastError());
  const size_t dn = (size_t)nd * r->nb;
  if (nd > 0) {
    PYSDR_HIP_CHECK(hipMemcpyAsync(codes, r->d_code, dn * sizeof(int), hipMemcpyDeviceToHost, st));
    PYSDR_HIP_CHECK(hipMemcpyAsync(t, r->d_t, dn * sizeof(long long), hipMemcpyDeviceToHost, st));
    PYSDR_HIP_CHECK(hipMemcpyAsync(snr2, r->d_snr, dn * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  PYSDR_HIP_CHECK(hipMemcpyAsync(ndet, r->d_ndet, (size_t)nlines * sizeof(int), hipMemcpyDeviceToHost, st));
  // the per-line rows of the call: ring rows n0 % R .., in at most two pieces
  const int r0 = (int)(n0 % r->R);
  const int first = nlines < r->R - r0 ? nlines : r->R - r0;
  const size_t w = (size_t)r->nb;
  if (isym) {
    PYSDR_HIP_CHECK(hipMemcpyAsync(isym, r->d_isym + r0 * w, first * w * sizeof(int), hipMemcpyDeviceToHost, st));
    if (first < nlines)
      PYSDR_HIP_CHECK(hipMemcpyAsync(isym + first * w, r->d_isym, (nlines - first) * w * sizeof(int), hipMemcpyDeviceToHost, st));
  }
  if (best) {
    PYSDR_HIP_CHECK(hipMemcpyAsync(best, r->d_best + r0 * w, first * w * sizeof(float), hipMemcpyDeviceToHost, st));
    if (first < nlines)
      PYSDR_HIP_CHECK(hipMemcpyAsync(best + first * w, r->d_best, (nlines - first) * w * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  r->n = n1;
  *n_dec = nd;
  return PYSDR_OK;
}

}  // extern "C"
