// FT8 and FT4 skimmers: inside every row of the channelizer's channel-major output
// NSUB = S / 2 sync decoders, one every baud / 2, over a spectrum of NB = NSUB + 14 (FT4: + 6) bins taken four times per
// symbol.  Three kernels, each written once and instantiated for the two modes of ft_plan.h:
//   * ft_spectrum_kernel: one workgroup owns one row.  Tiles of [S - 1 earlier samples + S outputs] go through the LDS
//     (the S - 1 in front are the row's history at the first tile and are carried over inside the LDS afterwards, so
//     global memory is read once per row sample); the four steps that end in a tile times NB bins are 184 or 248 (FT4:
//     120 or 168) independent sums of S terms, one lane each.  A bin's arithmetic is fixed by the definition, not its lane.
//     Powers go to the row's ring [TR][NB] with plain stores.  The row's last S - 1 samples move in front of the row at
//     the end (through registers: the source may overlap the destination), which is why a workgroup takes a whole row.
//   * ft_sync_kernel, queued behind it: one thread owns one decoder, walks the call's steps in order, reads the 21 (16)
//     Costas symbols of the frame that would end with each step from the ring (the lanes of a row read neighbouring bins;
//     tone and frame symbol are constexpr functions of the symbol's number, no table in memory), keeps the last 9 scores
//     and hit counts in the decoder's own slots and stores an event where the middle one is a peak.  Two launches, not
//     one: the score needs nothing but the ring, so it gets a lane per decoder and no barrier per step, and the spectrum
//     keeps all its lanes busy.
//   * ft_llr_kernel: 174 soft bits per candidate, one block each, on request.
#include "ft_plan.h"
#include "objects_plan.h"

namespace pysdr {

namespace {

template <class Mode, int S>
__global__ __launch_bounds__((FtGeom<Mode, S>::kThreads)) void ft_spectrum_kernel(const FtArgs a) {
  using G = FtGeom<Mode, S>;
  constexpr int NT = G::kNt, NB = G::kNb, TH = G::kThreads;
  __shared__ FtC s_tw[NT];
  __shared__ FtC s_y[G::kYp];
  const int tid = threadIdx.x;
  const int row = blockIdx.x;                              // the grid is nk workgroups
  const bool has = tid < G::kItems;                        // the last wave's spare lanes own no bin
  const int s = has ? G::item_step(tid) : 0, b = has ? G::item_bin(tid) : 0;
  const int qm = ft_qmod<Mode>(b, S);
  FtC* __restrict__ Y = a.y + (long long)row * a.ypitch;
  float* __restrict__ ring = a.ring + (size_t)row * (size_t)a.tr * NB;
  const int slot_first = (int)(a.t_first % a.tr);

  for (int i = tid; i < NT; i += TH) s_tw[i] = a.tw[i];

  for (int i0 = 0; i0 < a.n_out; i0 += G::kTile) {
    __syncthreads();                                       // everyone is done with the previous tile
    // the S - 1 samples in front of the tile: the row's history (first tile) or the previous tile's last ones
    FtC carry{0.f, 0.f};
    if (tid < G::kCarry) carry = i0 > 0 ? s_y[G::carry_src(tid)] : Y[G::hist_off(tid)];
    __syncthreads();                                       // (the loads below overwrite what was just read)
    if (tid < G::kCarry) s_y[G::carry_dst(tid)] = carry;
    for (int c = tid; c < G::kTile; c += TH) {
      const int i = i0 + c;
      FtC v{0.f, 0.f};
      if (i < a.n_out) v = Y[i];
      s_y[G::stage_dst(c)] = v;
    }
    __syncthreads();
    const int u = G::tile_step(i0, a.e_first, s);          // the step of the call whose last output falls in this tile
    if (has && u >= 0 && u < a.ns) {
      const float P = ft_bin<S>(&s_y[G::win(a.e_first, s)], s_tw, qm, a.cfg.pmax);
      const int slot = (slot_first + u) % a.tr;
      ring[(size_t)slot * NB + b] = P;
    }
  }

  // the row's new history: the last S - 1 of [old history | this call's outputs]
  FtC keep{0.f, 0.f};
  const bool roll = tid < S - 1;
  if (roll) keep = Y[G::roll_src(a.n_out, tid)];
  __syncthreads();                                         // every read of the row is done, the staging loop's too
  if (roll) Y[G::roll_dst(tid)] = keep;
}

constexpr int kSyncThreads = 256;

template <class Mode>
__global__ __launch_bounds__(kSyncThreads) void ft_sync_kernel(const FtArgs a, const int nsub, const int nb) {
  const int F = blockIdx.x * kSyncThreads + threadIdx.x;
  if (F >= a.nfine) return;
  const int row = F / nsub, j = F - row * nsub;
  const float* __restrict__ ring = a.ring + (size_t)row * (size_t)a.tr * nb;
  float* sc = a.sc + F;
  int32_t* hi = a.hi + F;
  int32_t* ev = a.events + (size_t)F * (size_t)a.cap * kFtEventWords;
  const long long nf = a.nfine;
  int cnt = 0;
  for (int u = 0; u < a.ns; ++u) {
    const long long t0 = a.t_first + u - kFtLag<Mode>;     // the frame that would end with this step
    if (t0 < 0) continue;
    const FtScore z = ft_sync<Mode>(ring, a.tr, nb, (int)(t0 % a.tr), j);
    const int k = (int)(t0 % kFtKeep);
    sc[k * nf] = z.score;
    hi[k * nf] = z.hits;
    const long long tc = t0 - kFtReach;                    // its score's neighbours are all known now
    if (tc >= 0 && ft_peak(sc, hi, nf, tc, a.cfg) && cnt < a.cap) {
      const int kc = (int)(tc % kFtKeep);
      ev[kFtEventWords * cnt] = ft_pack(u, hi[kc * nf]);
      ev[kFtEventWords * cnt + 1] = (int32_t)__float_as_uint(sc[kc * nf]);
      ++cnt;
    }
  }
  a.counts[F] = cnt;
}

constexpr int kLlrThreads = 192;

template <class Mode>
__global__ __launch_bounds__(kLlrThreads) void ft_llr_kernel(const FtLlrArgs a) {
  const int c = blockIdx.x, i = threadIdx.x;
  if (c >= a.n || i >= kFtBits) return;
  const int F = a.cand[2 * c], slot0 = a.cand[2 * c + 1];
  const int row = F / a.nsub, j = F - row * a.nsub;
  const float* ring = a.ring + (size_t)row * (size_t)a.tr * a.nb;
  a.out[(size_t)c * kFtBits + i] = ft_llr_bit<Mode>(ring, a.tr, a.nb, slot0, j, i);
}

template <class Mode, int S>
void launch_spectrum(const FtArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((ft_spectrum_kernel<Mode, S>), dim3(a.nk), dim3(FtGeom<Mode, S>::kThreads), 0, st, a);
}

template <class Mode>
int launch_steps(int S, const FtArgs& a, hipStream_t st) {
  if (a.n_out < 1 || a.nk < 1) return PYSDR_OK;
  if (S == Mode::kS0) launch_spectrum<Mode, Mode::kS0>(a, st);
  else if (S == Mode::kS1) launch_spectrum<Mode, Mode::kS1>(a, st);
  else {
    set_last_error("launch_%s_steps: S %d is neither %d nor %d", Mode::kName, S, Mode::kS0, Mode::kS1);
    return PYSDR_ERR_ARG;
  }
  PYSDR_HIP_CHECK(hipGetLastError());
  if (a.ns > 0) {
    hipLaunchKernelGGL(ft_sync_kernel<Mode>, dim3((a.nfine + kSyncThreads - 1) / kSyncThreads), dim3(kSyncThreads), 0, st, a, S / 2,
                       S / 2 + kFtExtra<Mode>);
    PYSDR_HIP_CHECK(hipGetLastError());
  }
  return PYSDR_OK;
}

template <class Mode>
int launch_llr(const FtLlrArgs& a, hipStream_t st) {
  if (a.n < 1) return PYSDR_OK;
  hipLaunchKernelGGL(ft_llr_kernel<Mode>, dim3(a.n), dim3(kLlrThreads), 0, st, a);
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

}  // namespace

int launch_ft_steps(int source, int S, const FtArgs& a, hipStream_t st) {
  if (source == Ft8Mode::kLdpcSource) return launch_steps<Ft8Mode>(S, a, st);
  if (source == Ft4Mode::kLdpcSource) return launch_steps<Ft4Mode>(S, a, st);
  set_last_error("launch_ft_steps: source %d names no mode", source);
  return PYSDR_ERR_ARG;
}

int launch_ft_llr(int source, const FtLlrArgs& a, hipStream_t st) {
  if (source == Ft8Mode::kLdpcSource) return launch_llr<Ft8Mode>(a, st);
  if (source == Ft4Mode::kLdpcSource) return launch_llr<Ft4Mode>(a, st);
  set_last_error("launch_ft_llr: source %d names no mode", source);
  return PYSDR_ERR_ARG;
}

}  // namespace pysdr
