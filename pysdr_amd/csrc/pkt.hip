// Packet skimmer: on every row of the channelizer's channel-major output an FM discriminator, a
// mark and a space tone filter over one bit and eight slicers, each with its own bit clock, HDLC receiver and frame
// buffer: 1200 baud AFSK, AX.25 UI frames.  Discriminator, mixer and bit window are a FIR, equal for a row's eight slicers
// and parallel over the outputs; clock, HDLC and CRC are serial per decoder and cheap.  So a workgroup owns 8 whole rows
// and works in tiles of 64 outputs: all 256 threads mix the staged samples (phase A1: one product pair per row sample) and
// take the two tone powers of two row outputs each (phase A2) into the LDS, then the first wavefront -- thread (row,
// slicer), 64 decoders -- walks the tile's outputs in order from there (phase B) while the other three already stage the
// next tile.  Tiles of [rows][L earlier samples + 64 outputs] go through the LDS; the L in front are the row's history at
// the first tile and are carried over inside the LDS afterwards, so global memory is read once per row sample; the table
// tw and the bit window g are in the LDS too.  The state is in registers for the call and written back once; a frame's
// bytes are packed four to a register and stored as words; events go to the decoder's own slots with plain stores, their
// count once at the end.  The row's last L samples move in front of the row at the end of the call (through registers:
// the source may overlap the destination), which is why a workgroup takes whole rows.
#include "pkt_plan.h"
#include "objects_plan.h"

namespace pysdr {

namespace {

__global__ __launch_bounds__(PktGeom::kThreads) void pkt_kernel(const PktArgs a) {
  using G = PktGeom;
  constexpr int ROWS = G::kRows, TH = G::kThreads;
  __shared__ PktC s_tw[kPktNt];
  __shared__ float s_g[kPktLmax];
  __shared__ PktC s_y[ROWS * G::kYp];
  __shared__ PktV s_v[ROWS * G::kYp];
  __shared__ PktP s_p[ROWS * G::kPp];
  const int tid = threadIdx.x;
  const int L = a.L;
  const int row0 = blockIdx.x * ROWS;
  // phase B: thread (row, slicer) of the first wavefront
  const bool has = tid < G::kDecoders;
  const int r = has ? tid / kPktSlicers : 0, s = has ? tid % kPktSlicers : 0;
  const int row = row0 + r;
  const bool mine = has && row < a.nk;
  const int dec = (mine ? row : 0) * kPktSlicers + s;
  const size_t nd = (size_t)a.ndec;

  for (int i = tid; i < kPktNt; i += TH) s_tw[i] = a.tw[i];
  for (int i = tid; i < L; i += TH) s_g[i] = a.g[i];
  PktDec z = pkt_dec_init();
  uint32_t* __restrict__ fb = a.frames + (size_t)dec * kPktFrameWords;
  float gain = 1.f;
  if (mine) {
    z.clk = a.si[dec]; z.xprev = a.si[nd + dec]; z.xlast = a.si[2 * nd + dec]; z.sr = a.si[3 * nd + dec]; z.ones = a.si[4 * nd + dec];
    z.inframe = a.si[5 * nd + dec]; z.byte = a.si[6 * nd + dec]; z.nb = a.si[7 * nd + dec]; z.nbytes = a.si[8 * nd + dec];
    z.crc = a.si[9 * nd + dec];
    pkt_word_load(z, fb);
    gain = a.gain[s];
  }
  int32_t* __restrict__ ev = a.events + (size_t)dec * (size_t)a.cap;
  int cnt = 0;
  const PktC* __restrict__ Y = a.y;
  const int ncarry = G::carry_n(L), nmix = G::mix_n(L);

  for (int i0 = 0; i0 < a.n_out; i0 += kPktTile) {
    // The L samples in front of the tile: the row's history (first tile) or the previous tile's last ones.  (Everyone is
    // past the previous tile's mixer, the last reader of s_y: two barriers lie behind it.)
    PktC carry[2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int k = tid + q * TH;
      if (k < ncarry) {
        const int hr = G::carry_row(k, L), hc = G::carry_col(k, L);
        if (i0 > 0) carry[q] = s_y[G::carry_src(hr, hc)];
        else if (row0 + hr < a.nk) carry[q] = Y[(long long)(row0 + hr) * a.ypitch + G::hist_off(hc, L)];
      }
    }
    __syncthreads();                                       // (the loads below overwrite what was just read)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int k = tid + q * TH;
      if (k < ncarry) s_y[G::carry_dst(G::carry_row(k, L), G::carry_col(k, L))] = carry[q];
    }
    for (int k = tid; k < ROWS * kPktTile; k += TH) {
      const int rr = G::stage_row(k), c = G::stage_col(k);
      const int i = i0 + c;
      PktC v{0.f, 0.f};
      if (row0 + rr < a.nk && i < a.n_out) v = Y[(long long)(row0 + rr) * a.ypitch + i];
      s_y[G::stage_dst(rr, c, L)] = v;
    }
    __syncthreads();
    // phase A1: discriminator and mixer, once per row sample
    for (int k = tid; k < nmix; k += TH) {
      const int rr = G::mix_row(k, L), c = G::mix_col(k, L);
      const uint32_t n = a.m0 + (uint32_t)(i0 + G::mix_rel(c, L));
      s_v[G::at(rr, c)] = pkt_mix(s_y[G::at(rr, c)], s_y[G::at(rr, c - 1)], n, a.w_mark, a.w_space, s_tw);
    }
    __syncthreads();                                       // (and the first wavefront is done with the previous tile's powers)
    // phase A2: the bit window and the two powers, two row outputs per thread
    for (int k = tid; k < ROWS * kPktTile; k += TH) {
      const int rr = G::stage_row(k), jj = G::stage_col(k);
      s_p[G::pw_at(rr, jj)] = pkt_tones(&s_v[G::win(rr, jj, L)], s_g, L, a.pmax);
    }
    __syncthreads();
    // phase B: slicer, clock, HDLC
    if (mine) {
      const int nj = a.n_out - i0 < kPktTile ? a.n_out - i0 : kPktTile;   // the last tile may be partial
      for (int jj = 0; jj < nj; ++jj) {
        const int x = pkt_slice(gain, s_p[G::pw_at(r, jj)]);
        if (pkt_clock(z, x, a.w_baud, a.pll_shift)) pkt_sample(z, x, i0 + jj, fb, ev, cnt, a.cap);
      }
    }
  }

  // the row's new history: the last L of [old history | this call's outputs]
  PktC keep[2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int k = tid + q * TH;
    if (k < ncarry && row0 + G::carry_row(k, L) < a.nk)
      keep[q] = Y[(long long)(row0 + G::carry_row(k, L)) * a.ypitch + G::roll_src(a.n_out, G::carry_col(k, L), L)];
  }
  __syncthreads();                                         // every read of the rows is done, the staging loop's too
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int k = tid + q * TH;
    if (k < ncarry && row0 + G::carry_row(k, L) < a.nk)
      a.y[(long long)(row0 + G::carry_row(k, L)) * a.ypitch + G::roll_dst(G::carry_col(k, L), L)] = keep[q];
  }

  if (mine) {
    pkt_word_flush(z, fb);
    a.si[dec] = z.clk; a.si[nd + dec] = z.xprev; a.si[2 * nd + dec] = z.xlast; a.si[3 * nd + dec] = z.sr; a.si[4 * nd + dec] = z.ones;
    a.si[5 * nd + dec] = z.inframe; a.si[6 * nd + dec] = z.byte; a.si[7 * nd + dec] = z.nb; a.si[8 * nd + dec] = z.nbytes;
    a.si[9 * nd + dec] = z.crc;
    a.counts[dec] = cnt;
  }
}

}  // namespace

int launch_pkt_decode(const PktArgs& a, hipStream_t st) {
  if (a.n_out < 1 || a.nk < 1) return PYSDR_OK;
  if (a.L < kPktLmin || a.L > kPktLmax) {
    set_last_error("launch_pkt_decode: L %d outside [%d, %d]", a.L, kPktLmin, kPktLmax);
    return PYSDR_ERR_ARG;
  }
  const int groups = (a.nk + PktGeom::kRows - 1) / PktGeom::kRows;
  hipLaunchKernelGGL(pkt_kernel, dim3(groups), dim3(PktGeom::kThreads), 0, st, a);
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

}  // namespace pysdr
