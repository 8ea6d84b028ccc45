// SSTV skimmer: on every row of the channelizer's channel-major output a detector, a mixer to
// the 1900 Hz subcarrier, a low-pass of up to 96 taps and the lag product of neighbouring outputs; from sums of lag
// products the 10 ms tick frequencies, the VIS match, the anchor and the pixels.  Mixer, low-pass and lag product are
// parallel over the outputs; ticks, VIS and pixels are serial per row and cheap.  So a workgroup owns 8 whole rows and works
// in tiles of 64 outputs, each row seen twice: the tile's own outputs (ticks, VIS, anchor) and the outputs `lag` earlier
// (pixels) -- 16 pseudo-rows.  All 256 threads mix the L + 64 samples of every pseudo-row into the LDS (phase A1), filter
// 65 outputs of each (A2) and multiply neighbours (A3); then thread r < 8 walks row r's 64 outputs in order (phase B) with
// the row's state in registers.  The anchor, once per picture, is taken by the row's thread alone from the row's memory
// (sstv_anchor: 2 R0 + 2 W low-pass outputs), its hard decisions in the LDS.  The settings and the mode table are copied
// to the LDS once: read through the argument's pointer, every output of phase B waited for global memory.  The ring and
// the line buffer stay in the row's own global memory; events go to the row's own slots with plain stores, their count
// once at the end.  The row's last H samples move in front of the row at the end of the call, in ascending chunks
// through registers (source and destination may overlap), which is why a workgroup takes whole rows.  A first version:
// nothing else here is tuned.
#include "sstv_plan.h"
#include "objects_plan.h"

namespace pysdr {

namespace {

__global__ __launch_bounds__(SstvGeom::kThreads) void sstv_kernel(const SstvArgs a) {
  using G = SstvGeom;
  constexpr int ROWS = G::kRows, TH = G::kThreads, T = kSstvTile;
  __shared__ SstvC s_tw[kSstvNt];
  __shared__ float s_g[kSstvLmax];
  __shared__ SstvC s_v[G::kPseudo * G::kVp];
  __shared__ SstvC s_u[G::kPseudo * G::kUp];
  __shared__ SstvC s_c[G::kPseudo * G::kCp];
  __shared__ signed char s_q[ROWS * kSstvQMax];
  __shared__ pysdr_sstv_cfg s_cfg;                         // settings and mode table: what phase B reads at every output
  const int tid = threadIdx.x;
  const int L = a.L, H = a.H;
  const int row0 = blockIdx.x * ROWS;
  for (int i = tid; i < (int)(sizeof(pysdr_sstv_cfg) / sizeof(uint32_t)); i += TH)
    reinterpret_cast<uint32_t*>(&s_cfg)[i] = reinterpret_cast<const uint32_t*>(a.cfg)[i];
  __syncthreads();
  const pysdr_sstv_cfg& cfg = s_cfg;
  const pysdr_sstv_mode* __restrict__ modes = cfg.modes;
  const int det = cfg.det, lag = cfg.lag;
  const uint32_t w_sub = cfg.w_sub;
  const float pmax = cfg.pmax;
  // phase B: thread r of the first wavefront
  const int row = row0 + tid;
  const bool mine = tid < ROWS && row < a.nk;
  const size_t rw = (size_t)(mine ? row : 0), nk = (size_t)a.nk;

  for (int i = tid; i < kSstvNt; i += TH) s_tw[i] = a.tw[i];
  for (int i = tid; i < L; i += TH) s_g[i] = a.g[i];
  SstvRow z = sstv_row_init();
  float* __restrict__ ring = a.ring + rw * kSstvRing;
  uint32_t* __restrict__ lb = a.lines + rw * kSstvLineWords;
  if (mine) {
    z.ticks = (uint32_t)a.si[rw]; z.phase = a.si[nk + rw]; z.mode = a.si[2 * nk + rw]; z.m_a = (uint32_t)a.si[3 * nk + rw];
    z.e0 = (uint32_t)a.si[4 * nk + rw]; z.line = a.si[5 * nk + rw]; z.pix = a.si[6 * nk + rw];
    z.acc.x = a.sf[rw]; z.acc.y = a.sf[nk + rw]; z.bprev.x = a.sf[2 * nk + rw]; z.bprev.y = a.sf[3 * nk + rw];
    z.f_lead = a.sf[4 * nk + rw]; z.pacc.x = a.sf[5 * nk + rw]; z.pacc.y = a.sf[6 * nk + rw];
    sstv_row_load(z, modes, lb);
  }
  int32_t* __restrict__ ev = a.events + rw * (size_t)a.cap;
  int cnt = 0;
  const SstvC* __restrict__ Y = a.y;
  const int nmix = G::mix_n(L);

  for (int i0 = 0; i0 < a.n_out; i0 += T) {
    __syncthreads();                                       // the tables are there; phase B is done with the previous tile
    // phase A1: detector and mixer, once per sample of a pseudo-row
#pragma unroll 4
    for (int k = tid; k < nmix; k += TH) {                 // (unrolled: the loads of four samples are in flight together)
      const int pr = G::mix_pr(k, L), cc = G::mix_col(k, L);
      const int i = G::base(i0, pr, lag) + G::mix_rel(cc, L);         // >= -lag - L: inside the history
      const int rr = row0 + G::row(pr);
      SstvC v{0.f, 0.f};
      if (rr < a.nk && i < a.n_out) {
        const SstvC* p = Y + (long long)rr * a.ypitch + i;
        v = sstv_mix(p[0], p[-1], a.m0 + (uint32_t)i, det, w_sub, s_tw);
      }
      s_v[G::v_at(pr, cc)] = v;
    }
    __syncthreads();
    // phase A2: the low-pass: the output in front of the tile and the tile's
    for (int k = tid; k < G::fir_n(); k += TH) {
      const int pr = G::fir_pr(k), kk = G::fir_col(k);
      s_u[G::u_at(pr, kk)] = sstv_fir(&s_v[G::fir_newest(pr, kk, L)], s_g, L);
    }
    __syncthreads();
    // phase A3: the lag products
    for (int k = tid; k < G::lag_n(); k += TH) {
      const int pr = G::lag_pr(k), jj = G::lag_col(k);
      s_c[G::c_at(pr, jj)] = sstv_lag(s_u[G::u_at(pr, jj + 1)], s_u[G::u_at(pr, jj)], pmax);
    }
    __syncthreads();
    // phase B: ticks, VIS, anchor, pixels
    if (mine) {
      const int nj = a.n_out - i0 < T ? a.n_out - i0 : T;  // the last tile may be partial
      const SstvC* yr = Y + (long long)row * a.ypitch;
      for (int jj = 0; jj < nj; ++jj) {
        const int i = i0 + jj;
        sstv_step(z, s_c[G::c_at(tid, jj)], s_c[G::c_at(ROWS + tid, jj)], yr + i, a.m0 + (uint32_t)i, i, cfg, modes, s_tw, s_g, L, ring, lb,
                  s_q + tid * kSstvQMax, ev, cnt, a.cap);
      }
    }
  }

  // the row's new history: the last H of [old history | this call's outputs], in ascending chunks: a chunk's reads lie
  // behind every earlier chunk's writes (the destination is n_out >= 1 below the source)
  __syncthreads();                                         // every read of the rows is done, the anchors' too
  const int nroll = ROWS * H;
  for (int k0 = 0; k0 < nroll; k0 += TH) {
    const int k = k0 + tid;
    const bool on = k < nroll && row0 + G::roll_row(k, H) < a.nk;
    SstvC keep{0.f, 0.f};
    if (on) keep = Y[(long long)(row0 + G::roll_row(k, H)) * a.ypitch + G::roll_src(k, H, a.n_out)];
    __syncthreads();
    if (on) a.y[(long long)(row0 + G::roll_row(k, H)) * a.ypitch + G::roll_dst(k, H)] = keep;
  }

  if (mine) {
    sstv_word_flush(z, lb);
    a.si[rw] = (int32_t)z.ticks; a.si[nk + rw] = z.phase; a.si[2 * nk + rw] = z.mode; a.si[3 * nk + rw] = (int32_t)z.m_a;
    a.si[4 * nk + rw] = (int32_t)z.e0; a.si[5 * nk + rw] = z.line; a.si[6 * nk + rw] = z.pix;
    a.sf[rw] = z.acc.x; a.sf[nk + rw] = z.acc.y; a.sf[2 * nk + rw] = z.bprev.x; a.sf[3 * nk + rw] = z.bprev.y;
    a.sf[4 * nk + rw] = z.f_lead; a.sf[5 * nk + rw] = z.pacc.x; a.sf[6 * nk + rw] = z.pacc.y;
    a.counts[rw] = cnt;
  }
}

}  // namespace

int launch_sstv_decode(const SstvArgs& a, hipStream_t st) {
  if (a.n_out < 1 || a.nk < 1) return PYSDR_OK;
  if (a.L < kSstvLmin || a.L > kSstvLmax || a.H < 1 || a.H > kSstvHpad) {
    set_last_error("launch_sstv_decode: L %d outside [%d, %d] or history %d outside [1, %d]", a.L, kSstvLmin, kSstvLmax, a.H, kSstvHpad);
    return PYSDR_ERR_ARG;
  }
  const int groups = (a.nk + SstvGeom::kRows - 1) / SstvGeom::kRows;
  hipLaunchKernelGGL(sstv_kernel, dim3(groups), dim3(SstvGeom::kThreads), 0, st, a);
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

}  // namespace pysdr
