// RTTY raster skimmer: inside every row of the channelizer's channel-major output a bank of NSUB = S
// Baudot decoders, one every baud / 4, each comparing the powers of a space and a mark tone 15 raster steps apart.  The
// decoder's recurrences are nonlinear and the definition fixes their order, so one thread owns one decoder, computes its
// two tones itself (a tone's arithmetic is fixed by the definition, so it does not matter that a neighbour computes the
// same tone again) and walks the call's outputs in order.  A workgroup owns whole rows, and rows share waves: 8 rows = 176
// decoders in 3 waves at S = 22, 7 rows = 231 decoders in 4 waves at S = 33; the lanes beyond the last decoder walk along
// and store nothing.  Tiles of [rows][S - 1 earlier samples + 64 outputs] go through the LDS and are shared by the row's
// decoders (the lanes of a row read one address: a broadcast); the S - 1 in front are the row's history at the first tile
// and are carried over inside the LDS afterwards, so global memory is read once per row sample; the mixer's table tw and
// the bit window g are in the LDS too.  The state is in registers for the call and written back once; events go to the
// decoder's own slots with plain stores, their count once at the end.  The row's last S - 1 samples move in front of the
// row at the end of the call (through registers: the source may overlap the destination), which is why a workgroup takes
// whole rows.
#include "fsk_plan.h"
#include "objects_plan.h"

namespace pysdr {

namespace {

template <int S>
__global__ __launch_bounds__(FskGeom<S>::kThreads) void fsk_kernel(const FskArgs a) {
  using G = FskGeom<S>;
  constexpr int NT = G::kNt, NSUB = G::kNsub, ROWS = G::kRows, TH = G::kThreads, YP = G::kYp;
  __shared__ FskC s_tw[NT];
  __shared__ float s_g[S];
  __shared__ FskC s_y[ROWS * YP];
  const int tid = threadIdx.x;
  const bool has = tid < G::kDecoders;                     // the last wave's spare lanes own no decoder
  const int r = has ? tid / NSUB : 0, j = has ? tid - r * NSUB : 0;
  const int row0 = blockIdx.x * ROWS;
  const int row = row0 + r;
  const bool mine = has && row < a.nk;
  const int dec = (mine ? row : 0) * NSUB + j;
  const pysdr_fsk_cfg cfg = a.cfg;
  const size_t nf = (size_t)a.nfine;

  for (int i = tid; i < NT; i += TH) s_tw[i] = a.tw[i];
  for (int i = tid; i < S; i += TH) s_g[i] = a.g[i];
  FskDec z = fsk_dec_init(S);
  if (mine) {
    z.qn = a.sf[dec]; z.qd = a.sf[nf + dec]; z.bm = a.sf[2 * nf + dec]; z.bs = a.sf[3 * nf + dec];
    z.st = a.si[dec]; z.cnt = a.si[nf + dec]; z.sh = a.si[2 * nf + dec]; z.nb = a.si[3 * nf + dec];
    z.prev = a.si[4 * nf + dec]; z.fig = a.si[5 * nf + dec]; z.open = a.si[6 * nf + dec]; z.seen = a.si[7 * nf + dec];
  }
  int32_t* __restrict__ ev = a.events + (size_t)dec * (size_t)a.cap;
  int cnt = 0;

  const int qs = fsk_qmod(j, S), qk = fsk_qmod(j + kFskToneGap, S);
  int ts = fsk_mulmod(qs, a.m0_mod, NT), tk = fsk_mulmod(qk, a.m0_mod, NT);   // (q m) mod NT of the sample at hand
  const FskC* __restrict__ Y = a.y;

  for (int i0 = 0; i0 < a.n_out; i0 += kFskTile) {
    __syncthreads();                                       // everyone is done with the previous tile
    // the S - 1 samples in front of the tile: the row's history (first tile) or the previous tile's last ones
    FskC carry{0.f, 0.f};
    const int hr = G::carry_row(tid), hc = G::carry_col(tid);
    if (tid < G::kCarry) {
      if (i0 > 0) carry = s_y[G::carry_src(hr, hc)];
      else if (row0 + hr < a.nk) carry = Y[(long long)(row0 + hr) * a.ypitch + G::hist_off(hc)];
    }
    __syncthreads();                                       // (the loads below overwrite what was just read)
    if (tid < G::kCarry) s_y[G::carry_dst(hr, hc)] = carry;
    for (int k = tid; k < ROWS * kFskTile; k += TH) {
      const int rr = G::stage_row(k), c = G::stage_col(k);
      const int i = i0 + c;
      FskC v{0.f, 0.f};
      if (row0 + rr < a.nk && i < a.n_out) v = Y[(long long)(row0 + rr) * a.ypitch + i];
      s_y[G::stage_dst(rr, c)] = v;
    }
    __syncthreads();
    const int nj = a.n_out - i0 < kFskTile ? a.n_out - i0 : kFskTile;   // the last tile may be partial
    for (int jj = 0; jj < nj; ++jj) {
      const FskC* yw = &s_y[G::win(r, jj)];
      const float PS = fsk_tone<S>(yw, s_tw, s_g, ts, qs, cfg.pmax);
      const float PM = fsk_tone<S>(yw, s_tw, s_g, tk, qk, cfg.pmax);
      const int code = fsk_step<S>(z, cfg, PS, PM);
      if (code >= 0 && mine && cnt < a.cap) ev[cnt++] = fsk_pack(i0 + jj, code);
      ts += qs;
      if (ts >= NT) ts -= NT;
      tk += qk;
      if (tk >= NT) tk -= NT;
    }
  }

  // the row's new history: the last S - 1 of [old history | this call's outputs]
  FskC keep{0.f, 0.f};
  const bool roll = mine && j < S - 1;
  if (roll) keep = Y[(long long)row * a.ypitch + G::roll_src(a.n_out, j)];
  __syncthreads();                                         // every read of the row is done, the staging loop's too
  if (roll) a.y[(long long)row * a.ypitch + G::roll_dst(j)] = keep;

  if (mine) {
    a.sf[dec] = z.qn; a.sf[nf + dec] = z.qd; a.sf[2 * nf + dec] = z.bm; a.sf[3 * nf + dec] = z.bs;
    a.si[dec] = z.st; a.si[nf + dec] = z.cnt; a.si[2 * nf + dec] = z.sh; a.si[3 * nf + dec] = z.nb;
    a.si[4 * nf + dec] = z.prev; a.si[5 * nf + dec] = z.fig; a.si[6 * nf + dec] = z.open; a.si[7 * nf + dec] = z.seen;
    a.counts[dec] = cnt;
  }
}

template <int S>
void launch(const FskArgs& a, hipStream_t st) {
  const int groups = (a.nk + FskGeom<S>::kRows - 1) / FskGeom<S>::kRows;
  hipLaunchKernelGGL(fsk_kernel<S>, dim3(groups), dim3(FskGeom<S>::kThreads), 0, st, a);
}

}  // namespace

int launch_fsk_decode(int S, const FskArgs& a, hipStream_t st) {
  if (a.n_out < 1 || a.nk < 1) return PYSDR_OK;
  if (S == 22) launch<22>(a, st);
  else if (S == 33) launch<33>(a, st);
  else {
    set_last_error("launch_fsk_decode: S %d is neither 22 nor 33", S);
    return PYSDR_ERR_ARG;
  }
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

}  // namespace pysdr
