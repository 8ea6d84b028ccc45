// RDS skimmer: on every row of the channelizer's channel-major output a four-quadrant FM
// discriminator, a mixer from 57 kHz, the matched filter of the biphase symbol at sixteen timing phases per bit, a
// differential decision and sixteen block-check decoders: 1187.5 bit/s RDS / RBDS groups off a broadcast band.  The
// matched filter is the load: L = 385 to 863 taps, evaluated once per chip, 19000 times per row-second; the rest is one
// arctangent per row sample and a few integer steps per bit.  A workgroup owns 2 whole rows and works in tiles of 1024
// outputs.  Phase A1, all 256 threads: discriminator and mixer of every staged sample, read from global memory once, into
// the LDS as 8-byte products (the first tile also makes the L products in front of it from the row's history; later tiles
// carry them over inside the LDS), and the tile's chips -- the same outputs on every row -- into a list.  Phase A2, all
// threads over (segment, row, chip): 64 taps of the filter each, the tap read as one LDS broadcast, the products 8 bytes
// per lane with neighbouring lanes one chip (12 to 27 entries) apart; the segment sums go to the LDS.  Phase B, thread
// (row, phase) of the first half wavefront: the segment sums added in order, the decision, the register, the block check,
// the event -- over the tile's chips of its phase, in order, while the other wavefronts already carry over.  The state is
// in registers for the call and written back once; events go to the decoder's own slots with plain stores, their count
// once at the end.  The row's last L + 1 samples move in front of the row at the end of the call (through registers: the
// source may overlap the destination), which is why a workgroup takes whole rows.
#include "rds_plan.h"
#include "objects_plan.h"

namespace pysdr {

namespace {

__global__ __launch_bounds__(RdsGeom::kThreads) void rds_kernel(const RdsArgs a) {
  using G = RdsGeom;
  constexpr int ROWS = G::kRows, TH = G::kThreads;
  __shared__ RdsC s_v[ROWS * G::kVp];
  __shared__ float s_g[kRdsLmax];
  __shared__ RdsC s_part[kRdsSegMax * ROWS * G::kCp];
  __shared__ int s_chip[G::kCp];
  const int tid = threadIdx.x;
  const int L = a.L, nseg = a.nseg;
  const int row0 = blockIdx.x * ROWS;
  // phase B: thread (row, phase)
  const bool has = tid < G::kDecoders;
  const int r = has ? tid / kRdsPhases : 0, ph = has ? tid % kRdsPhases : 0;
  const int row = row0 + r;
  const bool mine = has && row < a.nk;
  const int dec = (mine ? row : 0) * kRdsPhases + ph;
  const size_t nd = (size_t)a.ndec;

  for (int i = tid; i < L; i += TH) s_g[i] = a.g[i];
  RdsDec z{};
  uint32_t chips0 = 0u;
  if (mine) {
    z.w[0] = a.regs[dec]; z.w[1] = a.regs[nd + dec]; z.w[2] = a.regs[2 * nd + dec]; z.w[3] = a.regs[3 * nd + dec];
    z.zprev = a.ring[dec];
    chips0 = a.chips[row];
  }
  int32_t* __restrict__ ev = a.events + (size_t)dec * (size_t)a.cap;
  int cnt = 0;
  const RdsC* __restrict__ Y = a.y;
  const RdsC* __restrict__ tw = a.tw;
  const uint32_t A0 = rds_acc_before(a.m0, a.w19);
  const int ncarry = G::carry_n(L);

  for (int i0 = 0; i0 < a.n_out; i0 += kRdsTile) {
    const int nj = a.n_out - i0 < kRdsTile ? a.n_out - i0 : kRdsTile;          // the last tile may be partial
    const int kbase = rds_chips_upto(A0, i0 - 1, a.w19);                       // chips of the call in front of the tile
    const int nct = rds_chips_upto(A0, i0 + nj - 1, a.w19) - kbase;            // chips of the tile, <= kRdsChipsMax
    // The L products in front of the tile, from the previous tile's end.  (Everyone is past the previous tile's filter,
    // the last reader of s_v.)
    if (i0 > 0)
      for (int k = tid; k < ncarry; k += TH) {
        const int hr = G::carry_row(k, L), hc = G::carry_col(k, L);
        s_v[G::carry_dst(hr, hc)] = s_v[G::carry_src(hr, hc)];
      }
    __syncthreads();                                       // (the products below overwrite what was just read; the first
                                                           // wavefront is done with the previous tile's chips)
    // phase A1: discriminator and mixer, once per row sample; the tile's chips
    const int nmix = G::mix_n(i0, nj, L);
    for (int k = tid; k < nmix; k += TH) {
      const int rr = G::mix_row(k, i0, nj, L), c = G::mix_col(k, i0, nj, L);
      const int i = i0 + G::mix_rel(c, L);
      RdsC v{0.f, 0.f};
      if (row0 + rr < a.nk) {
        const RdsC* __restrict__ p = Y + (long long)(row0 + rr) * a.ypitch + i;
        v = rds_mix(p[0], p[-1], a.m0 + (uint32_t)i, a.w19, tw);
      }
      s_v[G::at(rr, c)] = v;
    }
    for (int jj = tid; jj < nj; jj += TH)
      if (rds_tick(a.m0 + (uint32_t)(i0 + jj), a.w19)) s_chip[rds_chips_upto(A0, i0 + jj, a.w19) - kbase - 1] = jj;
    __syncthreads();
    // phase A2: the matched filter, one segment of one chip of one row per thread and turn
    const int nfir = G::fir_n(nseg, nct);
    for (int k = tid; k < nfir; k += TH) {
      const int ci = G::fir_chip(k, nct), rr = G::fir_row(k, nct), seg = G::fir_seg(k, nct);
      s_part[G::part_at(seg, rr, ci)] = rds_segment(&s_v[G::newest(rr, s_chip[ci], L)], s_g, L, seg);
    }
    __syncthreads();
    // phase B: the chips of this thread's phase, in order
    if (mine)
      for (int ci = (int)((ph - (chips0 + (uint32_t)kbase)) & 15u); ci < nct; ci += kRdsPhases)
        rds_bit(z, rds_sum(&s_part[G::part_at(0, r, ci)], ROWS * G::kCp, nseg), i0 + s_chip[ci], ph, ev, cnt, a.cap);
  }

  // the row's new history: the last L + 1 of [old history | this call's outputs]
  RdsC keep[G::kRollPer];
  const int nroll = G::roll_n(L);
#pragma unroll
  for (int q = 0; q < G::kRollPer; ++q) {
    const int k = tid + q * TH;
    keep[q] = RdsC{0.f, 0.f};
    if (k < nroll && row0 + G::roll_row(k, L) < a.nk)
      keep[q] = Y[(long long)(row0 + G::roll_row(k, L)) * a.ypitch + G::roll_src(a.n_out, G::roll_col(k, L), L)];
  }
  __syncthreads();                                         // every read of the rows is done
#pragma unroll
  for (int q = 0; q < G::kRollPer; ++q) {
    const int k = tid + q * TH;
    if (k < nroll && row0 + G::roll_row(k, L) < a.nk)
      a.y[(long long)(row0 + G::roll_row(k, L)) * a.ypitch + G::roll_dst(G::roll_col(k, L), L)] = keep[q];
  }

  if (mine) {
    a.regs[dec] = z.w[0]; a.regs[nd + dec] = z.w[1]; a.regs[2 * nd + dec] = z.w[2]; a.regs[3 * nd + dec] = z.w[3];
    a.ring[dec] = z.zprev;
    a.counts[dec] = cnt;
  }
  __syncthreads();                                         // every phase has read the row's chip count
  if (mine && ph == 0) a.chips[row] = chips0 + (uint32_t)rds_chips_upto(A0, a.n_out - 1, a.w19);
}

}  // namespace

int launch_rds_decode(const RdsArgs& a, hipStream_t st) {
  if (a.n_out < 1 || a.nk < 1) return PYSDR_OK;
  if (a.L < kRdsLmin || a.L > kRdsLmax || a.nseg != (a.L + kRdsSeg - 1) / kRdsSeg || a.w19 < kRdsW19Min || a.w19 > kRdsW19Max) {
    set_last_error("launch_rds_decode: L %d outside [%d, %d], nseg %d not its segments, or w19 %u outside [%u, %u]", a.L, kRdsLmin, kRdsLmax, a.nseg,
                   a.w19, kRdsW19Min, kRdsW19Max);
    return PYSDR_ERR_ARG;
  }
  const int groups = (a.nk + RdsGeom::kRows - 1) / RdsGeom::kRows;
  hipLaunchKernelGGL(rds_kernel, dim3(groups), dim3(RdsGeom::kThreads), 0, st, a);
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

}  // namespace pysdr
