// ACARS skimmer: on every row of the channelizer's channel-major output the envelope power, a
// complex band-pass at +1800 Hz over four bits, a mixer, a differential detector over one bit and one decoder with its bit
// clock, frame machine, CRC and frame buffer: 2400 bit/s MSK inside the AM envelope.  Power, band-pass, mixer and detector
// are a FIR of up to 85 complex-by-real taps, parallel over the outputs; clock and frame machine are serial per row and
// cheap.  So a workgroup owns 8 whole rows and works in tiles of 64 outputs: all 256 threads stage the powers of the
// tile's samples and of the 5 L in front of them (phase A1; the samples in front are read again from the row, whose
// history sits in front of the call's outputs), band-pass and mix the L + 64 outputs the detector needs (phase A2) and
// slice two outputs each (phase A3) into the LDS; then one lane per row walks the tile's bits in order from there (phase
// B).  The table tw and the taps c are in the LDS too.  The state is in registers for the call and written back once; a
// frame's bytes are packed four to a register and stored as words; events go to the decoder's own slots with plain
// stores, their count once at the end.  The row's last 5 L samples move in front of the row at the end of the call
// (through registers: the source may overlap the destination), which is why a workgroup takes whole rows.
#include "acars_plan.h"
#include "objects_plan.h"

namespace pysdr {

namespace {

__global__ __launch_bounds__(AcGeom::kThreads) void acars_kernel(const AcArgs a) {
  using G = AcGeom;
  constexpr int ROWS = G::kRows, TH = G::kThreads;
  __shared__ AcC s_tw[kAcNt];
  __shared__ AcC s_c[kAcTapsMax];
  __shared__ float s_p[ROWS * G::kPp];
  __shared__ AcC s_a[ROWS * G::kAp];
  __shared__ int s_x[ROWS * G::kXp];
  const int tid = threadIdx.x;
  const int L = a.L, NT = G::taps(L);
  const int row0 = blockIdx.x * ROWS;
  // phase B: lane r of the first wavefront has row row0 + r
  const int r = tid < ROWS ? tid : 0;
  const int row = row0 + r;
  const bool mine = tid < ROWS && row < a.nk;
  const int dec = mine ? row : 0;
  const size_t nd = (size_t)a.nk;

  for (int i = tid; i < kAcNt; i += TH) s_tw[i] = a.tw[i];
  for (int i = tid; i < NT; i += TH) s_c[i] = a.c[i];
  AcDec z = acars_dec_init();
  uint32_t* __restrict__ fb = a.frames + (size_t)dec * kAcFrameWords;
  if (mine) {
    z.clk = a.si[dec]; z.xprev = a.si[nd + dec]; z.lev = a.si[2 * nd + dec]; z.sr = a.si[3 * nd + dec]; z.st = a.si[4 * nd + dec];
    z.byte = a.si[5 * nd + dec]; z.nb = a.si[6 * nd + dec]; z.nbytes = a.si[7 * nd + dec]; z.crc = a.si[8 * nd + dec];
    acars_word_load(z, fb);
  }
  int32_t* __restrict__ ev = a.events + (size_t)dec * (size_t)a.cap;
  int cnt = 0;
  const AcC* __restrict__ Y = a.y;
  const int nstage = G::stage_n(L), nmix = G::mix_n(L);

  for (int i0 = 0; i0 < a.n_out; i0 += kAcTile) {
    // phase A1: the powers of the tile's samples and of the 5 L in front of them.  (Everyone is past the previous tile's
    // mixer, the last reader of s_p: two barriers lie behind it.)
    for (int k = tid; k < nstage; k += TH) {
      const int rr = G::stage_row(k, L), c = G::stage_col(k, L);
      const int i = i0 + G::stage_rel(c, L);
      AcC v{0.f, 0.f};
      if (row0 + rr < a.nk && i < a.n_out) v = Y[(long long)(row0 + rr) * a.ypitch + i];
      s_p[G::p_at(rr, c)] = acars_power(v, a.pmax);
    }
    __syncthreads();
    // phase A2: band-pass and mixer for the outputs i0 - L .. i0 + 63
    for (int k = tid; k < nmix; k += TH) {
      const int rr = G::mix_row(k, L), c = G::mix_col(k, L);
      const uint32_t m = a.m0 + (uint32_t)(i0 + G::mix_rel(c, L));
      s_a[G::a_at(rr, c)] = acars_mix(&s_p[G::win(rr, c, L)], s_c, NT, m, a.w_car, s_tw);
    }
    __syncthreads();                                       // (and the rows' lanes are done with the previous tile's bits)
    // phase A3: the detector, two row outputs per thread
    for (int k = tid; k < ROWS * kAcTile; k += TH) {
      const int rr = G::det_row(k), jj = G::det_col(k);
      s_x[G::x_at(rr, jj)] = acars_detect(s_a[G::a_at(rr, jj + L)], s_a[G::a_at(rr, jj)]);
    }
    __syncthreads();
    // phase B: clock and frame machine
    if (mine) {
      const int nj = a.n_out - i0 < kAcTile ? a.n_out - i0 : kAcTile;     // the last tile may be partial
      for (int jj = 0; jj < nj; ++jj) {
        const int x = s_x[G::x_at(r, jj)];
        if (acars_clock(z, x, a.w_baud, a.pll_shift)) acars_sample(z, x, i0 + jj, fb, ev, cnt, a.cap);
      }
    }
  }

  // the row's new history: the last 5 L of [old history | this call's outputs]
  const int nroll = G::roll_n(L);
  AcC keep[G::kRollPerThread];
#pragma unroll
  for (int q = 0; q < G::kRollPerThread; ++q) {
    const int k = tid + q * TH;
    keep[q] = AcC{0.f, 0.f};
    if (k < nroll && row0 + G::roll_row(k, L) < a.nk)
      keep[q] = Y[(long long)(row0 + G::roll_row(k, L)) * a.ypitch + G::roll_src(a.n_out, G::roll_col(k, L), L)];
  }
  __syncthreads();                                         // every read of the rows is done, the staging loop's too
#pragma unroll
  for (int q = 0; q < G::kRollPerThread; ++q) {
    const int k = tid + q * TH;
    if (k < nroll && row0 + G::roll_row(k, L) < a.nk)
      a.y[(long long)(row0 + G::roll_row(k, L)) * a.ypitch + G::roll_dst(G::roll_col(k, L), L)] = keep[q];
  }

  if (mine) {
    acars_word_flush(z, fb);
    a.si[dec] = z.clk; a.si[nd + dec] = z.xprev; a.si[2 * nd + dec] = z.lev; a.si[3 * nd + dec] = z.sr; a.si[4 * nd + dec] = z.st;
    a.si[5 * nd + dec] = z.byte; a.si[6 * nd + dec] = z.nb; a.si[7 * nd + dec] = z.nbytes; a.si[8 * nd + dec] = z.crc;
    a.counts[dec] = cnt;
  }
}

}  // namespace

int launch_acars_decode(const AcArgs& a, hipStream_t st) {
  if (a.n_out < 1 || a.nk < 1) return PYSDR_OK;
  if (a.L < kAcLmin || a.L > kAcLmax) {
    set_last_error("launch_acars_decode: L %d outside [%d, %d]", a.L, kAcLmin, kAcLmax);
    return PYSDR_ERR_ARG;
  }
  const int groups = (a.nk + AcGeom::kRows - 1) / AcGeom::kRows;
  hipLaunchKernelGGL(acars_kernel, dim3(groups), dim3(AcGeom::kThreads), 0, st, a);
  PYSDR_HIP_CHECK(hipGetLastError());
  return PYSDR_OK;
}

}  // namespace pysdr
