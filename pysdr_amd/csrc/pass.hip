// The second pass of the FT8 and FT4 skimmers: take decoded frames out of the row samples and
// search the spectrum of what is left.  Four kernels, the steps of pass_plan.h:
//   * pass_keep_kernel, queued behind the sync kernel of every process call once pysdr_*_keep was called: one workgroup per
//     row copies the call's outputs into the sample ring yk (sample n at n mod TY) and the call's new steps of the
//     spectrum ring into ring2 (step t at t mod TR2).  It reads Y after the spectrum kernel, whose roll writes only the
//     history room in front of a row.
//   * pass_subtract_kernel<Mode, S>: one workgroup per row that has jobs, which it runs in the order given, so no two
//     workgroups write the same samples.  A job: the codeword and the tones as the frame report derives them; every
//     (trial, symbol) pair's amplitude, a lane each, S terms in ascending order; a lane per trial adds its |a_k|^2 in
//     ascending k; lane 0 picks the greatest, the lower index on a tie; then a lane per symbol subtracts a_k r[n] and adds
//     the power before and after; lane 0 adds those in ascending k and stores the job's four words.
//   * pass_respectrum_kernel<Mode, S>, behind it: one workgroup per (job, tile of four steps) recomputes the steps
//     t0 - 4 .. t0 + lag + 4 of ring2 from yk with ft_bin<S>, the streaming kernel's twiddles, pmax and arithmetic.  Two jobs
//     of a row may recompute the same step: both store the same bits.
//   * pass_rescan_kernel<Mode>: one workgroup per fine row, a lane per start step t_lo - 4 .. t_hi + 4: ft_sync on ring2 to
//     the LDS, a barrier, ft_peak_rule on the dense array, a barrier, and lane 0 stores the row's events in step order.
// Plain vector stores only; every lane reaches every barrier.
#include "objects_plan.h"
#include "pass_plan.h"

namespace pysdr {

namespace {

__global__ __launch_bounds__(kPassThreads) void pass_keep_kernel(const PassKeepArgs a) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const FtC* __restrict__ Y = a.y + (long long)row * a.ypitch;
  FtC* __restrict__ yk = a.yk + (size_t)row * (size_t)a.ty;
  const int at0 = (int)(a.m0 % a.ty);
  for (int i = tid; i < a.n_out; i += kPassThreads) {
    int at = at0 + i;                                      // n_out < ty
    if (at >= a.ty) at -= a.ty;
    yk[at] = Y[i];
  }
  const float* __restrict__ ring = a.ring + (size_t)row * (size_t)a.tr * (size_t)a.nb;
  float* __restrict__ ring2 = a.ring2 + (size_t)row * (size_t)a.tr2 * (size_t)a.nb;
  for (int e = tid; e < a.ns * a.nb; e += kPassThreads) {
    const int u = e / a.nb, b = e - u * a.nb;
    const long long t = a.t_first + u;
    ring2[(size_t)(t % a.tr2) * (size_t)a.nb + b] = ring[(size_t)(t % a.tr) * (size_t)a.nb + b];
  }
}

constexpr int kPassSymPitch = 104;                         // >= 103 symbols

template <class Mode, int S>
__global__ __launch_bounds__(kPassThreads) void pass_subtract_kernel(const PassSubArgs a) {
  constexpr int NS = Mode::kSyms, NP = kPassPulse<Mode> * S, MODE = (int)Mode::kReportMode;
  static_assert(NS <= kPassSymPitch && NS <= kPassThreads && kPassTrials <= kPassThreads, "a lane per symbol, a lane per trial");
  __shared__ uint8_t s_cw[kReportCwBytes];
  __shared__ int s_tone[kPassSymPitch];
  __shared__ uint32_t s_pulse[NP];
  __shared__ FtC s_a[kPassTrials * kPassSymPitch];
  __shared__ uint8_t s_used[kPassTrials * kPassSymPitch];
  __shared__ float s_score[kPassTrials];
  __shared__ float s_pb[kPassSymPitch], s_pa[kPassSymPitch];
  __shared__ int s_best;
  const int tid = threadIdx.x;
  const int first = a.rows[2 * blockIdx.x], count = a.rows[2 * blockIdx.x + 1];
  for (int i = tid; i < NP; i += kPassThreads) s_pulse[i] = a.pulse[i];

  for (int jb = 0; jb < count; ++jb) {
    const PassJob* __restrict__ job = a.jobs + first + jb;
    const int ntr = job->ntr;
    const uint32_t w = job->w, m0 = job->m0, m1 = job->m1, m2 = job->m2;
    const long long n0 = (long long)(((unsigned long long)(uint32_t)job->n0_hi << 32) | (unsigned long long)(uint32_t)job->n0_lo);
    FtC* yk = a.yk + (size_t)job->row * (size_t)a.ty;
    __syncthreads();                                       // the previous job is done with the LDS, and its samples are stored
    if (tid < kLdpcK) s_cw[tid] = report_msg_bit(m0, m1, m2, tid);
    if (tid < kLdpcM) s_cw[kLdpcK + tid] = report_parity(m0, m1, m2, tid);
    __syncthreads();
    if (tid < NS) {
      bool sync;
      s_tone[tid] = report_tone<MODE>(s_cw, tid, &sync);
    }
    __syncthreads();
    for (int item = tid; item < ntr * NS; item += kPassThreads) {
      const int i = item / NS, k = item - i * NS;
      const long long dn = job->trial[2 * i];
      const uint32_t fw = (uint32_t)job->trial[2 * i + 1];
      FtC amp;
      const bool ok = pass_amp<Mode, S>(yk, a.ty, n0 + dn + (long long)S * k, a.n_lo, a.n_hi, s_tone, s_pulse, a.lut, w + fw, k, &amp);
      s_a[i * kPassSymPitch + k] = amp;
      s_used[i * kPassSymPitch + k] = ok ? 1 : 0;
    }
    __syncthreads();
    if (tid < ntr) {
      float acc = 0.f;
      for (int k = 0; k < NS; ++k) {
        const FtC v = s_a[tid * kPassSymPitch + k];
        const float p = v.x * v.x + v.y * v.y;
        acc = k == 0 ? p : acc + p;
      }
      s_score[tid] = acc;
    }
    __syncthreads();
    if (tid == 0) {
      int best = 0;
      for (int i = 1; i < ntr; ++i)
        if (s_score[i] > s_score[best]) best = i;
      s_best = best;
    }
    __syncthreads();
    const int best = s_best;
    if (tid < NS) {
      float pb = 0.f, pa = 0.f;
      if (s_used[best * kPassSymPitch + tid])
        pass_sub<Mode, S>(yk, a.ty, n0 + (long long)job->trial[2 * best] + (long long)S * tid, s_tone, s_pulse, a.lut,
                          w + (uint32_t)job->trial[2 * best + 1], tid, s_a[best * kPassSymPitch + tid], &pb, &pa);
      s_pb[tid] = pb;
      s_pa[tid] = pa;
    }
    __syncthreads();
    if (tid == 0) {
      float pb = 0.f, pa = 0.f;
      int used = 0;
      for (int k = 0; k < NS; ++k) {
        if (!s_used[best * kPassSymPitch + k]) continue;
        pb = used == 0 ? s_pb[k] : pb + s_pb[k];
        pa = used == 0 ? s_pa[k] : pa + s_pa[k];
        ++used;
      }
      int32_t* o = a.out + (size_t)job->out_at * kPassOutWords;
      o[0] = (int32_t)__float_as_uint(pb);
      o[1] = (int32_t)__float_as_uint(pa);
      o[2] = best;
      o[3] = used;
    }
  }
}

template <class Mode, int S>
__global__ __launch_bounds__(kPassThreads) void pass_respectrum_kernel(const PassSpecArgs a) {
  using G = FtGeom<Mode, S>;
  constexpr int NT = G::kNt, NB = G::kNb, QS = G::kQs, NW = (kPassTileSteps - 1) * QS + S;
  static_assert(G::kItems <= kPassThreads, "a lane per step and bin");
  __shared__ FtC s_tw[NT];
  __shared__ FtC s_y[NW];
  const int tid = threadIdx.x;
  const PassJob* __restrict__ job = a.jobs + blockIdx.y;
  const long long t0 = (long long)(((unsigned long long)(uint32_t)job->t0_hi << 32) | (unsigned long long)(uint32_t)job->t0_lo);
  const long long t_tile = t0 - kPassMargin + (long long)kPassTileSteps * blockIdx.x;
  const long long t_last = t0 + kFtLag<Mode> + kPassMargin;
  const FtC* __restrict__ yk = a.yk + (size_t)job->row * (size_t)a.ty;
  float* __restrict__ ring2 = a.ring2 + (size_t)job->row * (size_t)a.tr2 * NB;
  for (int i = tid; i < NT; i += kPassThreads) s_tw[i] = a.tw[i];
  for (int i = tid; i < NW; i += kPassThreads) {
    const long long n = (long long)QS * t_tile + i;
    FtC v{0.f, 0.f};
    if (n >= 0) v = yk[n % a.ty];                          // (a step before the stream's start is not computed)
    s_y[i] = v;
  }
  __syncthreads();
  const bool has = tid < G::kItems;
  const int s = has ? G::item_step(tid) : 0, b = has ? G::item_bin(tid) : 0;
  const long long t = t_tile + s;
  if (has && t >= 0 && t <= t_last && t < a.t_done) {
    const float P = ft_bin<S>(&s_y[QS * s], s_tw, ft_qmod<Mode>(b, S), a.pmax);
    ring2[(size_t)(t % a.tr2) * NB + b] = P;
  }
}

template <class Mode>
__global__ __launch_bounds__(kPassThreads) void pass_rescan_kernel(const PassScanArgs a) {
  __shared__ float s_sc[kPassThreads];
  __shared__ int32_t s_hi[kPassThreads];
  __shared__ uint8_t s_peak[kPassThreads];
  const int tid = threadIdx.x;
  const int F = a.F_lo + blockIdx.x;
  const int row = F / a.nsub, j = F - row * a.nsub;
  const float* __restrict__ ring = a.ring2 + (size_t)row * (size_t)a.tr2 * (size_t)a.nb;
  const long long t = a.t_lo - kFtReach + tid;
  FtScore z{0.f, 0};
  if (tid < a.nt + 2 * kFtReach && t >= 0) z = ft_sync<Mode>(ring, a.tr2, a.nb, (int)(t % a.tr2), j);
  s_sc[tid] = z.score;
  s_hi[tid] = z.hits;
  __syncthreads();
  bool peak = false;
  if (tid >= kFtReach && tid < a.nt + kFtReach)
    peak = ft_peak_rule(s_sc[tid], s_hi[tid], t, a.cfg, [&](int d) { return s_sc[tid + d]; });
  s_peak[tid] = peak ? 1 : 0;
  __syncthreads();
  if (tid == 0) {
    int32_t* ev = a.events + (size_t)blockIdx.x * kPassEventCap * kFtEventWords;
    int cnt = 0;
    for (int u = 0; u < a.nt; ++u) {
      if (!s_peak[u + kFtReach] || cnt >= kPassEventCap) continue;
      ev[kFtEventWords * cnt] = ft_pack(u, s_hi[u + kFtReach]);
      ev[kFtEventWords * cnt + 1] = (int32_t)__float_as_uint(s_sc[u + kFtReach]);
      ++cnt;
    }
    a.counts[blockIdx.x] = cnt;
  }
}

template <class Mode, int S>
void launch_sub(const PassSubArgs& a, const PassSpecArgs& s, hipStream_t st) {
  hipLaunchKernelGGL((pass_subtract_kernel<Mode, S>), dim3(a.nrows), dim3(kPassThreads), 0, st, a);
  hipLaunchKernelGGL((pass_respectrum_kernel<Mode, S>), dim3(kPassTiles<Mode>, s.njobs), dim3(kPassThreads), 0, st, s);
}

template <class Mode>
int launch_subtract(int S, const PassSubArgs& a, const PassSpecArgs& s, hipStream_t st) {
  if (a.nrows < 1 || s.njobs < 1) return PYSDR_OK;
  if (a.nrows > kPassJobsMax || s.njobs > kPassJobsMax || !a.yk || !a.jobs || !a.rows || !a.pulse || !a.lut || !a.out || !s.tw || !s.ring2 ||
      a.ty < 1 || s.tr2 < 1) {
    set_last_error("launch_pass_subtract: %d rows, %d jobs or a NULL array", a.nrows, s.njobs);
    return PYSDR_ERR_ARG;
  }
  if (S == Mode::kS0) launch_sub<Mode, Mode::kS0>(a, s, st);
  else if (S == Mode::kS1) launch_sub<Mode, Mode::kS1>(a, s, st);
  else {
    set_last_error("launch_pass_subtract: S %d is neither %d nor %d", S, Mode::kS0, Mode::kS1);
    return PYSDR_ERR_ARG;
  }
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

}  // namespace

int launch_pass_keep(const PassKeepArgs& a, hipStream_t st) {
  if (a.n_out < 1 || a.nk < 1) return PYSDR_OK;
  if (!a.y || !a.ring || !a.yk || !a.ring2 || a.n_out >= a.ty || a.ns < 0 || a.ns > a.tr2 || a.ns > a.tr || a.nb < 1) {
    set_last_error("launch_pass_keep: %d outputs into %d samples, %d steps into %d, or a NULL array", a.n_out, a.ty, a.ns, a.tr2);
    return PYSDR_ERR_ARG;
  }
  hipLaunchKernelGGL(pass_keep_kernel, dim3(a.nk), dim3(kPassThreads), 0, st, a);
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

int launch_pass_subtract(int source, int S, const PassSubArgs& a, const PassSpecArgs& s, hipStream_t st) {
  if (source == Ft8Mode::kLdpcSource) return launch_subtract<Ft8Mode>(S, a, s, st);
  if (source == Ft4Mode::kLdpcSource) return launch_subtract<Ft4Mode>(S, a, s, st);
  set_last_error("launch_pass_subtract: source %d names no mode", source);
  return PYSDR_ERR_ARG;
}

int launch_pass_rescan(int source, const PassScanArgs& a, hipStream_t st) {
  if (!a.ring2 || !a.counts || !a.events || a.nF < 1 || a.nF > kPassRowsMax || a.nt < 1 || a.nt + 2 * kFtReach > kPassWindowMax || a.F_lo < 0 ||
      a.t_lo < 0 || a.tr2 < 1 || a.nb < 1 || a.nsub < 1) {
    set_last_error("launch_pass_rescan: %d fine rows from %d, %d steps from %lld, or a NULL array", a.nF, a.F_lo, a.nt, a.t_lo);
    return PYSDR_ERR_ARG;
  }
  if (source == Ft8Mode::kLdpcSource) hipLaunchKernelGGL(pass_rescan_kernel<Ft8Mode>, dim3(a.nF), dim3(kPassThreads), 0, st, a);
  else if (source == Ft4Mode::kLdpcSource) hipLaunchKernelGGL(pass_rescan_kernel<Ft4Mode>, dim3(a.nF), dim3(kPassThreads), 0, st, a);
  else {
    set_last_error("launch_pass_rescan: source %d names no mode", source);
    return PYSDR_ERR_ARG;
  }
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

}  // namespace pysdr
