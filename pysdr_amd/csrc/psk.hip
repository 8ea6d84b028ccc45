// PSK31 skimmer: inside every row of the channelizer's channel-major output a bank of NSUB = 4 S
// BPSK decoders, one every baud / 32.  The decoder's recurrences are nonlinear and the definition fixes their order, so
// one thread owns one decoder and walks the call's outputs in order; a workgroup owns whole rows (2 rows = one wave at
// S = 8, 4 rows = three waves at S = 12).  Tiles of [rows][L - 1 earlier samples + 64 outputs] go through the LDS and are
// shared by the row's decoders (the lanes of a row read one address: a broadcast); the L - 1 in front are the row's
// history at the first tile and are carried over inside the LDS afterwards, so global memory is read once per row
// sample; the mixer's table tw and the matched filter g are in the LDS too.  The symbol energies e[S] are indexed by a
// run-time phase and live in the LDS as e[phase][thread]: consecutive lanes, consecutive banks.  The rest of the state is
// in registers for the call and written back once; events go to the decoder's own slots with plain stores, their count
// once at the end.  The row's last L - 1 samples move in front of the row at the end of the call (through registers: the
// source may overlap the destination), which is why a workgroup takes whole rows.
#include "psk_plan.h"
#include "objects_plan.h"

namespace pysdr {

namespace {

template <int S>
__global__ __launch_bounds__(PskGeom<S>::kThreads) void psk_kernel(const PskArgs a) {
  using G = PskGeom<S>;
  constexpr int L = G::kL, NT = G::kNt, NSUB = G::kNsub, ROWS = G::kRows, TH = G::kThreads, YP = G::kYp;
  static_assert(G::kCarry <= TH && L - 1 <= kPskTile && L - 1 <= kPskHpad, "one thread per carried sample");
  __shared__ PskC s_tw[NT];
  __shared__ float s_g[L];
  __shared__ PskC s_y[ROWS * YP];
  __shared__ float s_e[S * TH];
  const int tid = threadIdx.x;
  const int r = tid / NSUB, j = tid - r * NSUB;
  const int row0 = blockIdx.x * ROWS;
  const int row = row0 + r;
  const bool mine = row < a.nk;
  const int dec = (mine ? row : 0) * NSUB + j;
  const pysdr_psk_cfg cfg = a.cfg;
  const size_t nf = (size_t)a.nfine;

  for (int i = tid; i < NT; i += TH) s_tw[i] = a.tw[i];
  for (int i = tid; i < L; i += TH) s_g[i] = a.g[i];
#pragma unroll
  for (int i = 0; i < S; ++i) s_e[G::e_at(i, tid)] = mine ? a.e[(size_t)i * nf + dec] : 0.f;
  PskDec z = psk_dec_init(S);
  if (mine) {
    z.qn = a.sf[dec]; z.qd = a.sf[nf + dec]; z.cr = a.sf[2 * nf + dec]; z.ci = a.sf[3 * nf + dec];
    z.pt = a.si[dec]; z.cnt = a.si[nf + dec]; z.sh = a.si[2 * nf + dec]; z.open = a.si[3 * nf + dec]; z.seen = a.si[4 * nf + dec];
  }
  int32_t* __restrict__ ev = a.events + (size_t)dec * (size_t)a.cap;
  int cnt = 0;

  const int qm = psk_qmod(j, S);
  int t = psk_mulmod(qm, a.m0_mod, NT);          // (q m) mod NT of the sample at hand
  int p = a.m0_mod % S;                          // m mod S: S divides NT
  const PskC* __restrict__ Y = a.y;

  for (int i0 = 0; i0 < a.n_out; i0 += kPskTile) {
    __syncthreads();                                       // everyone is done with the previous tile
    // the L - 1 samples in front of the tile: the row's history (first tile) or the previous tile's last ones
    PskC carry{0.f, 0.f};
    const int hr = G::carry_row(tid), hc = G::carry_col(tid);
    if (tid < G::kCarry) {
      if (i0 > 0) carry = s_y[G::carry_src(hr, hc)];
      else if (row0 + hr < a.nk) carry = Y[(long long)(row0 + hr) * a.ypitch + G::hist_off(hc)];
    }
    __syncthreads();                                       // (the loads below overwrite what was just read)
    if (tid < G::kCarry) s_y[G::carry_dst(hr, hc)] = carry;
    for (int k = tid; k < ROWS * kPskTile; k += TH) {
      const int rr = G::stage_row(k), c = G::stage_col(k);
      const int i = i0 + c;
      PskC v{0.f, 0.f};
      if (row0 + rr < a.nk && i < a.n_out) v = Y[(long long)(row0 + rr) * a.ypitch + i];
      s_y[G::stage_dst(rr, c)] = v;
    }
    __syncthreads();
    const int nj = a.n_out - i0 < kPskTile ? a.n_out - i0 : kPskTile;   // the last tile may be partial
    for (int jj = 0; jj < nj; ++jj) {
      float ur, ui;
      const float pw = psk_filter<S>(&s_y[G::win(r, jj)], s_tw, s_g, t, qm, cfg.pmax, ur, ui);
      float* ep = &s_e[G::e_at(p, tid)];
      const float e0 = *ep;
      *ep = e0 + cfg.a_t * (pw - e0);
      z.cnt -= 1;
      if (z.cnt == 0) {
        const int code = psk_symbol<S>(z, cfg, ur, ui, &s_e[G::e_at(0, tid)], G::e_at(1, 0), p);
        if (code != 0 && mine && cnt < a.cap) ev[cnt++] = psk_pack(i0 + jj, code);
      }
      p = p + 1 == S ? 0 : p + 1;
      t += qm;
      if (t >= NT) t -= NT;
    }
  }

  // the row's new history: the last L - 1 of [old history | this call's outputs]
  PskC keep{0.f, 0.f};
  const bool roll = mine && j < L - 1;
  if (roll) keep = Y[(long long)row * a.ypitch + G::roll_src(a.n_out, j)];
  __syncthreads();                                         // every read of the row is done, the staging loop's too
  if (roll) a.y[(long long)row * a.ypitch + G::roll_dst(j)] = keep;

  if (mine) {
#pragma unroll
    for (int i = 0; i < S; ++i) a.e[(size_t)i * nf + dec] = s_e[G::e_at(i, tid)];
    a.sf[dec] = z.qn; a.sf[nf + dec] = z.qd; a.sf[2 * nf + dec] = z.cr; a.sf[3 * nf + dec] = z.ci;
    a.si[dec] = z.pt; a.si[nf + dec] = z.cnt; a.si[2 * nf + dec] = z.sh; a.si[3 * nf + dec] = z.open; a.si[4 * nf + dec] = z.seen;
    a.counts[dec] = cnt;
  }
}

}  // namespace

int launch_psk_decode(int S, const PskArgs& a, hipStream_t st) {
  if (a.n_out < 1 || a.nk < 1) return PYSDR_OK;
  if (S == 8) {
    const int groups = (a.nk + PskGeom<8>::kRows - 1) / PskGeom<8>::kRows;
    hipLaunchKernelGGL(psk_kernel<8>, dim3(groups), dim3(PskGeom<8>::kThreads), 0, st, a);
  } else if (S == 12) {
    const int groups = (a.nk + PskGeom<12>::kRows - 1) / PskGeom<12>::kRows;
    hipLaunchKernelGGL(psk_kernel<12>, dim3(groups), dim3(PskGeom<12>::kThreads), 0, st, a);
  } else {
    set_last_error("launch_psk_decode: S %d is neither 8 nor 12", S);
    return PYSDR_ERR_ARG;
  }
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

}  // namespace pysdr
