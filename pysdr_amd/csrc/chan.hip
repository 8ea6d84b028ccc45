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
//   2. FFT: in-place decimation-in-frequency passes of radix 5 / 4 / 2 over all fw frames in LDS; twiddles from a table
//      e^{+j 2 pi j / M} computed in float64 on the host.  The result is left in digit-reversed order.
//   3. Store: row a = channel (k_first + a) mod M of the channel-major output takes its fw frames from LDS position
//      perm[a] (the digit reversal, a host table); consecutive lanes write consecutive frames of a row.
// No intermediate goes through memory; the only other launch of a call is the roll of the input history.
#include "chan_internal.h"

#include <cmath>
#include <mutex>

namespace pysdr {
namespace {

constexpr int kChanMaxPass = 8;
constexpr int kChanLdsElems = 16384;      // complex LDS elements a workgroup may hold (128 KB of the 160 KB)

struct ChanPlan {
  int npass = 0, radix[kChanMaxPass] = {};
  int C = 0;          // M / D
  int fw = 0;         // frames per workgroup
  int fi = 0;         // frames per FIR work item
  int threads = 0;
  int mp = 0;         // LDS pitch of a frame, odd: the store reads one element of every frame side by side
  int lds_bytes = 0;
};

// Pure arithmetic: which launch a channelizer of this shape runs with; false: outside the rules of DESIGN §3 item 15.
bool chan_plan(int M, int D, ChanPlan* p) {
  if (M < 16 || M > 4096 || D < 1 || M % D != 0) return false;
  const int C = M / D;
  if (C != 1 && C != 2 && C != 4) return false;
  int twos = 0, fives = 0, m = M;
  while (m % 2 == 0) { m /= 2; ++twos; }
  while (m % 5 == 0) { m /= 5; ++fives; }
  if (m != 1) return false;
  ChanPlan q;
  q.C = C;
  for (int i = 0; i < fives; ++i) q.radix[q.npass++] = 5;
  for (int i = 0; i < twos / 2; ++i) q.radix[q.npass++] = 4;
  if (twos & 1) q.radix[q.npass++] = 2;
  // 16 frames = 128-byte row segments while they fit the LDS; small M: as many groups of 16 as fill 256 branches
  if (M <= 256) q.fw = 16 * (256 / M);
  else if (M * 16 <= kChanLdsElems) q.fw = 16;
  else if (M * 8 <= kChanLdsElems) q.fw = 8;
  else q.fw = 4;
  q.fi = q.fw < 8 ? 4 : 8;
  q.mp = M | 1;
  q.threads = q.fw * M > 4096 ? 1024 : 256;
  q.lds_bytes = q.fw * q.mp * (int)sizeof(float2);
  *p = q;
  return true;
}

inline uint32_t magic_of(int d) { return (uint32_t)(0x100000000ull / (unsigned)d) + 1u; }   // d >= 2; exact n / d while n d < 2^32

struct ChanArgs {
  const float2* x;        // this call's samples, x[0] = absolute sample s0
  const float2* hist;     // hist[H]: samples s0 - H .. s0 - 1 (zeros before the stream's start)
  int H, n;
  int off0;               // mf D - s0, 0 <= off0 < D: where the call's first frame mf ends
  int mf_lo;              // mf mod 4
  int nframes;
  int M, D, P, mp, fw;
  const float* taps;      // [P][M]
  const float2* tw;       // [M] e^{+j 2 pi j / M}
  const int* perm;        // [nk] LDS position of row a's channel
  int nk;
  float2* y;              // y[a * pitch + (m - mf)]
  long long pitch;
  int npass, radix[kChanMaxPass];
  uint32_t magic_M, magic_fw, magic_per[kChanMaxPass], magic_nq[kChanMaxPass];
  int xq, xr;             // grid / 8, grid % 8: the workgroups that share an L2 take consecutive runs of frames
};

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

// One in-place decimation-in-frequency pass over every frame: blocks of nb points split into R blocks of nq = nb / R;
// output k1 of the butterfly at n2 is turned by e^{+j 2 pi n2 k1 / nb} (nothing to turn in the last pass, nq = 1).
template <int R>
__device__ __forceinline__ void fft_pass(float2* sm, const ChanArgs& a, int nb, uint32_t magic_per, uint32_t magic_nq) {
  const int nq = nb / R, per = a.M / R, total = a.fw * per, tws = a.M / nb;
  for (int it = threadIdx.x; it < total; it += blockDim.x) {
    const int f = (int)__umulhi((uint32_t)it, magic_per), j = it - f * per;
    const int b = nq > 1 ? (int)__umulhi((uint32_t)j, magic_nq) : j, n2 = j - b * nq;
    float2* p = sm + f * a.mp + b * nb + n2;
    float2 v[R];
#pragma unroll
    for (int i = 0; i < R; ++i) v[i] = p[i * nq];
    bfly<R>(v);
    if (nq > 1) {
#pragma unroll
      for (int i = 1; i < R; ++i) v[i] = cmul(v[i], a.tw[n2 * i * tws]);
    }
#pragma unroll
    for (int i = 0; i < R; ++i) p[i * nq] = v[i];
  }
}

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
  for (int s = 0; s < a.npass; ++s) {
    const int R = a.radix[s];
    if (R == 4) fft_pass<4>(sm, a, nb, a.magic_per[s], a.magic_nq[s]);
    else if (R == 5) fft_pass<5>(sm, a, nb, a.magic_per[s], a.magic_nq[s]);
    else fft_pass<2>(sm, a, nb, a.magic_per[s], a.magic_nq[s]);
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

constexpr int kChanMaxIn = 1 << 28;

}  // namespace
}  // namespace pysdr

struct pysdr_chan {
  int device = 0, M = 0, D = 0, k_first = 0, nk = 0, max_taps = 0, max_in = 0;
  int H = 0;               // history kept: ceil(max_taps / M) M - 1 samples
  int P = 0;               // taps per branch of the current prototype (0: none set yet)
  int out_cap = 0;         // row pitch of the internal output buffer
  int cur = 0;             // which history buffer is current
  unsigned long long n_abs = 0;
  pysdr::ChanPlan plan;
  float2* d_hist[2] = {nullptr, nullptr};
  float* d_taps = nullptr;
  float2* d_tw = nullptr;
  int* d_perm = nullptr;
  float2* d_in = nullptr;   // staging of host input  [max_in]:      allocated by the first call that passes a host pointer
  float2* d_out = nullptr;  // staging of host output [nk][out_cap]: likewise
  hipStream_t stream = nullptr;
  std::vector<float> h_taps;
  std::mutex mu;            // one call at a time on a handle: set_taps / reset / sync / process
};

namespace pysdr {
ChanInfo chan_info(pysdr_chan* c) {
  std::lock_guard<std::mutex> lk(c->mu);
  return ChanInfo{c->device, c->M, c->D, c->nk, c->max_in, c->out_cap, c->n_abs, c->stream};
}
}  // namespace pysdr

using namespace pysdr;

extern "C" {

int pysdr_chan_plan(int M, int D, int ntaps, int k_first, int nk, int32_t out[16]) {
  if (!out) { set_last_error("pysdr_chan_plan: out is NULL"); return PYSDR_ERR_ARG; }
  ChanPlan p;
  if (!chan_plan(M, D, &p)) {
    set_last_error("pysdr_chan_plan: M %d / D %d: M = 2^a 5^b in [16, 4096], D | M, M / D in {1, 2, 4}", M, D);
    return PYSDR_ERR_ARG;
  }
  if (ntaps < 1 || ntaps > 16 * M) { set_last_error("pysdr_chan_plan: ntaps %d outside [1, 16 M]", ntaps); return PYSDR_ERR_ARG; }
  if (k_first < 0 || k_first >= M || nk < 1 || nk > M) {
    set_last_error("pysdr_chan_plan: channels k_first %d, nk %d outside [0, M) / [1, M]", k_first, nk);
    return PYSDR_ERR_ARG;
  }
  const int P = (ntaps + M - 1) / M;
  for (int i = 0; i < 16; ++i) out[i] = 0;
  out[0] = p.npass;
  for (int i = 0; i < p.npass; ++i) out[1 + i] = p.radix[i];
  out[9] = p.fw; out[10] = p.fi; out[11] = p.threads; out[12] = p.lds_bytes; out[13] = P * M - 1; out[14] = P;
  return PYSDR_OK;
}

int pysdr_chan_create(int device, int M, int D, int k_first, int nk, int max_taps, int max_in, pysdr_chan** out) {
  if (!out) { set_last_error("pysdr_chan_create: out is NULL"); return PYSDR_ERR_ARG; }
  *out = nullptr;
  int32_t pl[16];
  const int rc0 = pysdr_chan_plan(M, D, max_taps, k_first, nk, pl);
  if (rc0 != PYSDR_OK) return rc0;
  if (max_in < 1 || max_in > kChanMaxIn) {
    set_last_error("pysdr_chan_create: max_in %d outside [1, %d]", max_in, kChanMaxIn);
    return PYSDR_ERR_ARG;
  }
  hipError_t e0 = hipSetDevice(device);
  if (e0 != hipSuccess) { set_last_error("hipSetDevice(%d): %s", device, hipGetErrorString(e0)); return PYSDR_ERR_NO_DEVICE; }
  pysdr_chan* c = new pysdr_chan();
  c->device = device; c->M = M; c->D = D; c->k_first = k_first; c->nk = nk; c->max_taps = max_taps; c->max_in = max_in;
  chan_plan(M, D, &c->plan);
  const int Pmax = (max_taps + M - 1) / M;
  c->H = Pmax * M - 1;
  c->out_cap = ((max_in + D - 1) / D + 1 + 15) & ~15;
  // twiddles in float64, and where the in-place passes leave channel k: k = k1 + R1 (k2 + R2 (...)) sits at
  // k1 M / R1 + k2 M / (R1 R2) + ...
  std::vector<float2> tw(M);
  for (int j = 0; j < M; ++j) {
    const double ph = 2.0 * M_PI * (double)j / (double)M;
    tw[j] = make_float2((float)std::cos(ph), (float)std::sin(ph));
  }
  std::vector<int> perm(nk);
  for (int a = 0; a < nk; ++a) {
    int k = (k_first + a) % M, nb = M, pos = 0;
    for (int s = 0; s < c->plan.npass; ++s) {
      const int R = c->plan.radix[s];
      nb /= R;
      pos += (k % R) * nb;
      k /= R;
    }
    perm[a] = pos;
  }
#define CK(e) do { hipError_t _e = (e); if (_e != hipSuccess) { set_last_error("pysdr_chan_create: %s -> %s", #e, hipGetErrorString(_e)); pysdr_chan_destroy(c); return PYSDR_ERR_HIP; } } while (0)
  CK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  CK(hipMalloc(&c->d_hist[0], (size_t)c->H * sizeof(float2)));
  CK(hipMalloc(&c->d_hist[1], (size_t)c->H * sizeof(float2)));
  CK(hipMalloc(&c->d_taps, (size_t)Pmax * M * sizeof(float)));
  CK(hipMalloc(&c->d_tw, (size_t)M * sizeof(float2)));
  CK(hipMalloc(&c->d_perm, (size_t)nk * sizeof(int)));
  CK(hipMemcpy(c->d_tw, tw.data(), (size_t)M * sizeof(float2), hipMemcpyHostToDevice));
  CK(hipMemcpy(c->d_perm, perm.data(), (size_t)nk * sizeof(int), hipMemcpyHostToDevice));
  // more than 64 KB of LDS is an opt-in per kernel
  CK(hipFuncSetAttribute(reinterpret_cast<const void*>(chan_kernel_for(c->plan.C, c->plan.fi)),
                         hipFuncAttributeMaxDynamicSharedMemorySize, c->plan.lds_bytes));
#undef CK
  const int rc = pysdr_chan_reset(c);
  if (rc != PYSDR_OK) { pysdr_chan_destroy(c); return rc; }
  *out = c;
  return PYSDR_OK;
}

void pysdr_chan_destroy(pysdr_chan* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (void* p : {(void*)c->d_hist[0], (void*)c->d_hist[1], (void*)c->d_taps, (void*)c->d_tw, (void*)c->d_perm, (void*)c->d_in,
                  (void*)c->d_out})
    if (p) (void)hipFree(p);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int pysdr_chan_set_taps(pysdr_chan* c, const double* h, int ntaps) {
  if (!c || !h) { set_last_error("pysdr_chan_set_taps: NULL channelizer or taps"); return PYSDR_ERR_ARG; }
  if (ntaps < 1 || ntaps > c->max_taps) {
    set_last_error("pysdr_chan_set_taps: ntaps %d outside [1, max_taps = %d]", ntaps, c->max_taps);
    return PYSDR_ERR_ARG;
  }
  std::lock_guard<std::mutex> lk(c->mu);
  PYSDR_HIP_CHECK(hipSetDevice(c->device));
  const int P = (ntaps + c->M - 1) / c->M;
  PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream));              // the staging vector may still feed an earlier copy
  c->h_taps.assign((size_t)P * c->M, 0.f);
  for (int i = 0; i < ntaps; ++i) c->h_taps[i] = (float)h[i];
  PYSDR_HIP_CHECK(hipMemcpyAsync(c->d_taps, c->h_taps.data(), c->h_taps.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream));
  c->P = P;
  return PYSDR_OK;
}

int pysdr_chan_reset(pysdr_chan* c) {
  if (!c) { set_last_error("pysdr_chan_reset: NULL channelizer"); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(c->mu);
  PYSDR_HIP_CHECK(hipSetDevice(c->device));
  PYSDR_HIP_CHECK(hipMemsetAsync(c->d_hist[0], 0, (size_t)c->H * sizeof(float2), c->stream));
  PYSDR_HIP_CHECK(hipMemsetAsync(c->d_hist[1], 0, (size_t)c->H * sizeof(float2), c->stream));
  PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream));
  c->cur = 0;
  c->n_abs = 0;
  return PYSDR_OK;
}

int pysdr_chan_sync(pysdr_chan* c) {
  if (!c) { set_last_error("pysdr_chan_sync: NULL channelizer"); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(c->mu);
  PYSDR_HIP_CHECK(hipSetDevice(c->device));
  PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream));
  return PYSDR_OK;
}

int pysdr_chan_process(pysdr_chan* c, const void* iq, int n, int on_device, void* out, long long out_pitch, int out_on_device,
                       int* n_out) {
  if (!c || !n_out) { set_last_error("pysdr_chan_process: NULL channelizer or n_out"); return PYSDR_ERR_ARG; }
  *n_out = 0;
  std::lock_guard<std::mutex> lk(c->mu);
  if (n < 0 || (n > 0 && !iq)) { set_last_error("pysdr_chan_process: n %d / NULL input", n); return PYSDR_ERR_ARG; }
  if (n > c->max_in) { set_last_error("pysdr_chan_process: n %d > max_in %d", n, c->max_in); return PYSDR_ERR_STATE; }
  if (c->P == 0) { set_last_error("pysdr_chan_process: no taps set"); return PYSDR_ERR_STATE; }
  const unsigned long long D = (unsigned long long)c->D, s0 = c->n_abs, s1 = s0 + (unsigned long long)n;
  const unsigned long long mf = (s0 + D - 1) / D, ml = (s1 + D - 1) / D;          // out_index_range(s0, s1, 1, D)
  const int nf = (int)(ml - mf);
  if (nf > 0 && !out) { set_last_error("pysdr_chan_process: NULL output"); return PYSDR_ERR_ARG; }
  if (out_pitch < nf) { set_last_error("pysdr_chan_process: pitch %lld < the call's %d outputs", out_pitch, nf); return PYSDR_ERR_STATE; }
  if (n == 0) return PYSDR_OK;
  PYSDR_HIP_CHECK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const float2* src = static_cast<const float2*>(iq);
  if (!on_device) {
    if (!c->d_in) PYSDR_HIP_CHECK(hipMalloc(&c->d_in, (size_t)c->max_in * sizeof(float2)));
    PYSDR_HIP_CHECK(hipMemcpyAsync(c->d_in, iq, (size_t)n * sizeof(float2), hipMemcpyHostToDevice, st));
    src = c->d_in;
  }
  if (nf > 0) {
    if (!out_on_device && !c->d_out) PYSDR_HIP_CHECK(hipMalloc(&c->d_out, (size_t)c->nk * c->out_cap * sizeof(float2)));
    const ChanPlan& pl = c->plan;
    ChanArgs a{};
    a.x = src; a.hist = c->d_hist[c->cur]; a.H = c->H; a.n = n;
    a.off0 = (int)(mf * D - s0); a.mf_lo = (int)(mf & 3ull); a.nframes = nf;
    a.M = c->M; a.D = c->D; a.P = c->P; a.mp = pl.mp; a.fw = pl.fw;
    a.taps = c->d_taps; a.tw = c->d_tw; a.perm = c->d_perm; a.nk = c->nk;
    a.y = out_on_device ? static_cast<float2*>(out) : c->d_out;
    a.pitch = out_on_device ? out_pitch : (long long)c->out_cap;
    a.npass = pl.npass;
    a.magic_M = magic_of(c->M); a.magic_fw = magic_of(pl.fw);
    int nb = c->M;
    for (int s = 0; s < pl.npass; ++s) {
      a.radix[s] = pl.radix[s];
      a.magic_per[s] = magic_of(c->M / pl.radix[s]);
      a.magic_nq[s] = nb / pl.radix[s] > 1 ? magic_of(nb / pl.radix[s]) : 0;
      nb /= pl.radix[s];
    }
    const int grid = (nf + pl.fw - 1) / pl.fw;
    a.xq = grid / 8; a.xr = grid % 8;
    hipLaunchKernelGGL(chan_kernel_for(pl.C, pl.fi), dim3(grid), dim3(pl.threads), (size_t)pl.lds_bytes, st, a);
    PYSDR_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(chan_roll, dim3((c->H + 255) / 256), dim3(256), 0, st, src, n, c->d_hist[c->cur], c->d_hist[c->cur ^ 1], c->H);
  PYSDR_HIP_CHECK(hipGetLastError());
  c->cur ^= 1;
  c->n_abs = s1;
  *n_out = nf;
  if (nf > 0 && !out_on_device)
    PYSDR_HIP_CHECK(hipMemcpy2DAsync(out, (size_t)out_pitch * sizeof(float2), c->d_out, (size_t)c->out_cap * sizeof(float2),
                                     (size_t)nf * sizeof(float2), (size_t)c->nk, hipMemcpyDeviceToHost, st));
  if (!on_device || !out_on_device) PYSDR_HIP_CHECK(hipStreamSynchronize(st));   // host buffers are the caller's again
  return PYSDR_OK;
}

}  // extern "C"
