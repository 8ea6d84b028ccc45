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
#include "chan_internal.h"

#include <cmath>
#include <mutex>

namespace pysdr {
namespace {

constexpr int kBankThreads = 256;
constexpr int kBankW = 8;                               // outputs per thread = taps per step
constexpr int kBankTile = kBankThreads * kBankW;        // outputs per workgroup
constexpr int kBankTapsMin = 3, kBankTapsMax = 255;     // 3: the squelch's second difference reaches d[m - 2]
constexpr int kBankNkMax = 4096;
constexpr float kAgcBeta = 0.1f, kAgcGainMax = 1.0e4f, kAgcRefDefault = 0.5f, kAgcFloor = 1e-12f;
constexpr float kBankSqAlpha = 0.64f;
constexpr double kNfmFullScaleDev = 5000.0;

struct BankPlan {
  int tp = 0;          // taps rounded up to whole steps of 8
  int hpad = 0;        // history samples kept in front of a row, >= T + 1, a multiple of 8
  int lds_floats = 0;  // kBankTile + tp
  int tiles = 0;       // per row, for max_out outputs
};

bool bank_plan(int nk, int ntaps, int max_out, BankPlan* p) {
  if (nk < 1 || nk > kBankNkMax || ntaps < kBankTapsMin || ntaps > kBankTapsMax || max_out < 1) return false;
  BankPlan q;
  q.tp = (ntaps + kBankW - 1) / kBankW * kBankW;
  q.hpad = (ntaps + 1 + 7) & ~7;
  q.lds_floats = kBankTile + q.tp;
  q.tiles = (max_out + kBankTile - 1) / kBankTile;
  *p = q;
  return true;
}

struct BankState {       // one per channel, in device memory
  float agc, gain, maxbuf, err, level;
  int open;
};

struct BankArgs {
  const float2* y;        // Y + Hpad: y[a * ypitch + i] = output i of this call, i >= -Hpad (history)
  long long ypitch;
  float* a;               // a[a * apitch + i]
  long long apitch;
  int n_out, T, tp;
  const float* taps;      // [tp], zero beyond T (never multiplied: 0 * NaN would widen a NaN's footprint)
  float fm_scale;
  int noise;              // 1: leave the squelch's partial sums
  float* pmax;            // [nk][ptiles]
  double* psum;           // [nk][ptiles]
  int ptiles;
};

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

struct FinishArgs {
  float2* ybase;          // Y: row a at ybase + a * ypitch, history in [0, hpad)
  long long ypitch;
  float* a;
  long long apitch;
  int n_out, hpad, ntiles, ptiles;
  const float* pmax;
  const double* psum;
  BankState* state;
  int agc_active;         // AGC enabled and mode AM
  int squelch;            // mode NFM and threshold > 0
  float ref, thresh;
};

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

}  // namespace
}  // namespace pysdr

struct pysdr_bank {
  pysdr_chan* ch = nullptr;
  pysdr::ChanInfo ci{};
  pysdr::BankPlan plan;
  int mode = PYSDR_NFM, T = 0;
  bool have_taps = false;
  int agc_enable = 1;
  float ref = pysdr::kAgcRefDefault, thresh = 0.f, fm_scale = 0.f;
  int last_n_out = 0;
  long long ypitch = 0, apitch = 0;
  float2* d_y = nullptr;            // [nk][hpad + out_cap]
  float* d_a = nullptr;             // [nk][out_cap]
  float* d_taps = nullptr;          // [tp]
  float* d_pmax = nullptr;          // [nk][tiles]
  double* d_psum = nullptr;         // [nk][tiles]
  pysdr::BankState* d_state = nullptr;
  std::vector<float> h_taps;
  std::vector<pysdr::BankState> h_state;
  std::mutex mu;                    // one call at a time on a handle
};

using namespace pysdr;

static int bank_reset_locked(pysdr_bank* b) {
  const int rc = pysdr_chan_reset(b->ch);
  if (rc != PYSDR_OK) return rc;
  PYSDR_HIP_CHECK(hipSetDevice(b->ci.device));
  hipStream_t st = b->ci.stream;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));                          // h_state may still feed an earlier copy
  PYSDR_HIP_CHECK(hipMemsetAsync(b->d_y, 0, (size_t)b->ci.nk * b->ypitch * sizeof(float2), st));
  b->h_state.assign((size_t)b->ci.nk, BankState{0.f, 1.f, 0.f, 0.f, 0.f, 1});
  PYSDR_HIP_CHECK(hipMemcpyAsync(b->d_state, b->h_state.data(), b->h_state.size() * sizeof(BankState), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  b->last_n_out = 0;
  return PYSDR_OK;
}

extern "C" {

int pysdr_bank_plan(int nk, int ntaps_af, int max_out, int32_t out[8]) {
  if (!out) { set_last_error("pysdr_bank_plan: out is NULL"); return PYSDR_ERR_ARG; }
  BankPlan p;
  if (!bank_plan(nk, ntaps_af, max_out, &p)) {
    set_last_error("pysdr_bank_plan: nk %d outside [1, %d], ntaps_af %d outside [%d, %d] or max_out %d < 1", nk, kBankNkMax,
                   ntaps_af, kBankTapsMin, kBankTapsMax, max_out);
    return PYSDR_ERR_ARG;
  }
  out[0] = kBankTile; out[1] = kBankThreads; out[2] = p.lds_floats * (int)sizeof(float); out[3] = p.tiles; out[4] = p.hpad;
  out[5] = p.tp; out[6] = 0; out[7] = 0;
  return PYSDR_OK;
}

int pysdr_bank_create(pysdr_chan* ch, double fs_out, int mode, int ntaps_af, pysdr_bank** out) {
  if (!out) { set_last_error("pysdr_bank_create: out is NULL"); return PYSDR_ERR_ARG; }
  *out = nullptr;
  if (!ch) { set_last_error("pysdr_bank_create: NULL channelizer"); return PYSDR_ERR_ARG; }
  if (mode != PYSDR_AM && mode != PYSDR_NFM) { set_last_error("pysdr_bank_create: mode %d is neither AM nor NFM", mode); return PYSDR_ERR_ARG; }
  if (!(fs_out > 0.0)) { set_last_error("pysdr_bank_create: fs_out %g", fs_out); return PYSDR_ERR_ARG; }
  const ChanInfo ci = chan_info(ch);
  BankPlan p;
  if (!bank_plan(ci.nk, ntaps_af, ci.out_cap, &p)) {
    set_last_error("pysdr_bank_create: ntaps_af %d outside [%d, %d]", ntaps_af, kBankTapsMin, kBankTapsMax);
    return PYSDR_ERR_ARG;
  }
  hipError_t e0 = hipSetDevice(ci.device);
  if (e0 != hipSuccess) { set_last_error("hipSetDevice(%d): %s", ci.device, hipGetErrorString(e0)); return PYSDR_ERR_NO_DEVICE; }
  pysdr_bank* b = new pysdr_bank();
  b->ch = ch; b->ci = ci; b->plan = p; b->mode = mode; b->T = ntaps_af;
  b->fm_scale = (float)(fs_out / (2.0 * M_PI * kNfmFullScaleDev));
  b->ypitch = (long long)p.hpad + ci.out_cap;
  b->apitch = ci.out_cap;
#define CK(e) do { hipError_t _e = (e); if (_e != hipSuccess) { set_last_error("pysdr_bank_create: %s -> %s", #e, hipGetErrorString(_e)); pysdr_bank_destroy(b); return PYSDR_ERR_HIP; } } while (0)
  CK(hipMalloc(&b->d_y, (size_t)ci.nk * b->ypitch * sizeof(float2)));
  CK(hipMalloc(&b->d_a, (size_t)ci.nk * b->apitch * sizeof(float)));
  CK(hipMalloc(&b->d_taps, (size_t)p.tp * sizeof(float)));
  CK(hipMalloc(&b->d_pmax, (size_t)ci.nk * p.tiles * sizeof(float)));
  CK(hipMalloc(&b->d_psum, (size_t)ci.nk * p.tiles * sizeof(double)));
  CK(hipMalloc(&b->d_state, (size_t)ci.nk * sizeof(BankState)));
#undef CK
  const int rc = bank_reset_locked(b);
  if (rc != PYSDR_OK) { pysdr_bank_destroy(b); return rc; }
  *out = b;
  return PYSDR_OK;
}

void pysdr_bank_destroy(pysdr_bank* b) {
  if (!b) return;
  (void)hipSetDevice(b->ci.device);
  if (b->ci.stream) (void)hipStreamSynchronize(b->ci.stream);
  for (void* p : {(void*)b->d_y, (void*)b->d_a, (void*)b->d_taps, (void*)b->d_pmax, (void*)b->d_psum, (void*)b->d_state})
    if (p) (void)hipFree(p);
  delete b;
}

int pysdr_bank_set_mode(pysdr_bank* b, int mode, const double* af, int ntaps) {
  if (!b || !af) { set_last_error("pysdr_bank_set_mode: NULL bank or taps"); return PYSDR_ERR_ARG; }
  if (mode != PYSDR_AM && mode != PYSDR_NFM) { set_last_error("pysdr_bank_set_mode: mode %d is neither AM nor NFM", mode); return PYSDR_ERR_ARG; }
  if (ntaps != b->T) { set_last_error("pysdr_bank_set_mode: ntaps %d != ntaps_af %d", ntaps, b->T); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(b->mu);
  PYSDR_HIP_CHECK(hipSetDevice(b->ci.device));
  hipStream_t st = b->ci.stream;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));                          // the staging vector may still feed an earlier copy
  b->h_taps.assign((size_t)b->plan.tp, 0.f);
  for (int i = 0; i < ntaps; ++i) b->h_taps[i] = (float)af[i];
  PYSDR_HIP_CHECK(hipMemcpyAsync(b->d_taps, b->h_taps.data(), b->h_taps.size() * sizeof(float), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  b->mode = mode;
  b->have_taps = true;
  return PYSDR_OK;
}

int pysdr_bank_set_agc(pysdr_bank* b, int enable, float ref) {
  if (!b) { set_last_error("pysdr_bank_set_agc: NULL bank"); return PYSDR_ERR_ARG; }
  if (!(ref > 0.f)) { set_last_error("pysdr_bank_set_agc: ref %g", (double)ref); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(b->mu);
  b->agc_enable = enable ? 1 : 0;
  b->ref = ref;
  return PYSDR_OK;
}

int pysdr_bank_set_squelch(pysdr_bank* b, float thresh) {
  if (!b) { set_last_error("pysdr_bank_set_squelch: NULL bank"); return PYSDR_ERR_ARG; }
  if (!(thresh >= 0.f)) { set_last_error("pysdr_bank_set_squelch: threshold %g", (double)thresh); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(b->mu);
  b->thresh = thresh;
  return PYSDR_OK;
}

int pysdr_bank_reset(pysdr_bank* b) {
  if (!b) { set_last_error("pysdr_bank_reset: NULL bank"); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(b->mu);
  return bank_reset_locked(b);
}

int pysdr_bank_sync(pysdr_bank* b) {
  if (!b) { set_last_error("pysdr_bank_sync: NULL bank"); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(b->mu);
  PYSDR_HIP_CHECK(hipSetDevice(b->ci.device));
  PYSDR_HIP_CHECK(hipStreamSynchronize(b->ci.stream));
  return PYSDR_OK;
}

int pysdr_bank_process(pysdr_bank* b, const void* iq, int n, int on_device, float* am, long long am_pitch, int am_on_device,
                       int* n_out) {
  if (!b || !n_out) { set_last_error("pysdr_bank_process: NULL bank or n_out"); return PYSDR_ERR_ARG; }
  *n_out = 0;
  std::lock_guard<std::mutex> lk(b->mu);
  if (n < 0 || (n > 0 && !iq)) { set_last_error("pysdr_bank_process: n %d / NULL input", n); return PYSDR_ERR_ARG; }
  if (n > b->ci.max_in) { set_last_error("pysdr_bank_process: n %d > max_in %d", n, b->ci.max_in); return PYSDR_ERR_STATE; }
  if (!b->have_taps) { set_last_error("pysdr_bank_process: no mode set"); return PYSDR_ERR_STATE; }
  // what the channelizer is about to complete: checked before it advances its stream
  const unsigned long long D = (unsigned long long)b->ci.D, s0 = chan_info(b->ch).n_abs, s1 = s0 + (unsigned long long)n;
  const int nf_want = (int)((s1 + D - 1) / D - (s0 + D - 1) / D);
  if (am && am_pitch < nf_want) {
    set_last_error("pysdr_bank_process: pitch %lld < the call's %d outputs", am_pitch, nf_want);
    return PYSDR_ERR_STATE;
  }
  int nf = 0;
  const int rc = pysdr_chan_process(b->ch, iq, n, on_device, b->d_y + b->plan.hpad, b->ypitch, 1, &nf);
  if (rc != PYSDR_OK) return rc;
  if (nf != nf_want) { set_last_error("pysdr_bank_process: the channelizer was fed beside its bank (%d outputs, %d expected)", nf, nf_want); return PYSDR_ERR_STATE; }
  if (nf == 0) { b->last_n_out = 0; return PYSDR_OK; }                // no output: no AGC block, no state change, nothing to fetch
  PYSDR_HIP_CHECK(hipSetDevice(b->ci.device));
  hipStream_t st = b->ci.stream;
  const int ntiles = (nf + kBankTile - 1) / kBankTile;
  const int squelch = (b->mode == PYSDR_NFM && b->thresh > 0.f) ? 1 : 0;
  BankArgs a{};
  a.y = b->d_y + b->plan.hpad; a.ypitch = b->ypitch; a.a = b->d_a; a.apitch = b->apitch;
  a.n_out = nf; a.T = b->T; a.tp = b->plan.tp; a.taps = b->d_taps; a.fm_scale = b->fm_scale; a.noise = squelch;
  a.pmax = b->d_pmax; a.psum = b->d_psum; a.ptiles = b->plan.tiles;
  const size_t lds = (size_t)b->plan.lds_floats * sizeof(float);
  if (b->mode == PYSDR_AM) hipLaunchKernelGGL(bank_kernel<PYSDR_AM>, dim3(ntiles, b->ci.nk), dim3(kBankThreads), lds, st, a);
  else hipLaunchKernelGGL(bank_kernel<PYSDR_NFM>, dim3(ntiles, b->ci.nk), dim3(kBankThreads), lds, st, a);
  PYSDR_HIP_CHECK(hipGetLastError());
  FinishArgs f{};
  f.ybase = b->d_y; f.ypitch = b->ypitch; f.a = b->d_a; f.apitch = b->apitch;
  f.n_out = nf; f.hpad = b->plan.hpad; f.ntiles = ntiles; f.ptiles = b->plan.tiles;
  f.pmax = b->d_pmax; f.psum = b->d_psum; f.state = b->d_state;
  f.agc_active = (b->agc_enable && b->mode == PYSDR_AM) ? 1 : 0;
  f.squelch = squelch; f.ref = b->ref; f.thresh = b->thresh;
  hipLaunchKernelGGL(bank_finish, dim3(b->ci.nk), dim3(kBankThreads), 0, st, f);
  PYSDR_HIP_CHECK(hipGetLastError());
  b->last_n_out = nf;
  *n_out = nf;
  if (am) {
    PYSDR_HIP_CHECK(hipMemcpy2DAsync(am, (size_t)am_pitch * sizeof(float), b->d_a, (size_t)b->apitch * sizeof(float),
                                     (size_t)nf * sizeof(float), (size_t)b->ci.nk,
                                     am_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    if (!am_on_device) PYSDR_HIP_CHECK(hipStreamSynchronize(st));     // the host buffer is the caller's again
  }
  return PYSDR_OK;
}

int pysdr_bank_state(pysdr_bank* b, float* agc, float* gain, float* maxbuf, float* level, uint8_t* open) {
  if (!b) { set_last_error("pysdr_bank_state: NULL bank"); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(b->mu);
  PYSDR_HIP_CHECK(hipSetDevice(b->ci.device));
  hipStream_t st = b->ci.stream;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  PYSDR_HIP_CHECK(hipMemcpyAsync(b->h_state.data(), b->d_state, b->h_state.size() * sizeof(BankState), hipMemcpyDeviceToHost, st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  for (int i = 0; i < b->ci.nk; ++i) {
    const BankState& s = b->h_state[i];
    if (agc) agc[i] = s.agc;
    if (gain) gain[i] = s.gain;
    if (maxbuf) maxbuf[i] = s.maxbuf;
    if (level) level[i] = s.level;
    if (open) open[i] = s.open ? 1 : 0;
  }
  return PYSDR_OK;
}

int pysdr_bank_fetch(pysdr_bank* b, const int* rows, int nrows, float* am, float* iq, long long pitch) {
  if (!b) { set_last_error("pysdr_bank_fetch: NULL bank"); return PYSDR_ERR_ARG; }
  if (nrows < 0 || (nrows > 0 && !rows)) { set_last_error("pysdr_bank_fetch: nrows %d / NULL rows", nrows); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(b->mu);
  for (int i = 0; i < nrows; ++i)
    if (rows[i] < 0 || rows[i] >= b->ci.nk) { set_last_error("pysdr_bank_fetch: row %d outside [0, %d)", rows[i], b->ci.nk); return PYSDR_ERR_ARG; }
  const int nf = b->last_n_out;
  if (pitch < nf) { set_last_error("pysdr_bank_fetch: pitch %lld < the last call's %d outputs", pitch, nf); return PYSDR_ERR_STATE; }
  if (nf == 0 || nrows == 0 || (!am && !iq)) return PYSDR_OK;
  PYSDR_HIP_CHECK(hipSetDevice(b->ci.device));
  hipStream_t st = b->ci.stream;
  for (int i = 0; i < nrows; ++i) {
    // runs of consecutive rows go as one strided copy
    int run = 1;
    while (i + run < nrows && rows[i + run] == rows[i] + run) ++run;
    const size_t r = (size_t)rows[i];
    if (am)
      PYSDR_HIP_CHECK(hipMemcpy2DAsync(am + (size_t)i * pitch, (size_t)pitch * sizeof(float), b->d_a + r * b->apitch,
                                       (size_t)b->apitch * sizeof(float), (size_t)nf * sizeof(float), (size_t)run,
                                       hipMemcpyDeviceToHost, st));
    if (iq)
      PYSDR_HIP_CHECK(hipMemcpy2DAsync(iq + 2 * (size_t)i * pitch, (size_t)pitch * sizeof(float2),
                                       b->d_y + r * b->ypitch + b->plan.hpad, (size_t)b->ypitch * sizeof(float2),
                                       (size_t)nf * sizeof(float2), (size_t)run, hipMemcpyDeviceToHost, st));
    i += run - 1;
  }
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  return PYSDR_OK;
}

}  // extern "C"
