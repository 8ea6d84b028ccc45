// The launch plan of the mix + decimate kernel (mixdec.hip): which instantiation a decimator's shape runs on, and the tile,
// LDS budget and output stage of one launch.  Plain C++, shared by the library (api.hip plans, mixdec.hip launches) and the
// host-side sanitizer harness (tests/host_san), so that all three see one decision.
#pragma once
#include <algorithm>

#include "common.h"

namespace pysdr {

// One instantiation mixdec_kernel<R, NJ, TPB, 0, MM>: R sub-receivers; NJ = kpad/16 known at compile time (fully unrolled tap
// loop) or 0 for a run-time loop; TPB threads per workgroup; MM = 1: the dot products on the matrix cores.
struct MdKey { int r, nj, tpb, mm; };
constexpr bool operator==(MdKey a, MdKey b) { return a.r == b.r && a.nj == b.nj && a.tpb == b.tpb && a.mm == b.mm; }

// Every instantiation compiled, X(R, NJ, TPB, MM):
//   <1..8, 0, 1024>       the generic form, taps in LDS
//   <1..8, 6, 1024>       255-tap prototypes at UP = 3 (the BASELINE configurations)
//   <1, {4,11,16,21}, 1024>  one sub-receiver: broadcast FM's resampler, 1001 taps at UP = 6, the broadcast-FM video filter,
//                         1001 taps at UP = 3
//   <2..6, 11, 768, MM>   1001 taps at UP = 6 from two sub-receivers
//   <2..4, 21, 768, MM>, <5..6, 21, 512, MM>   1001 taps at UP = 3 from two sub-receivers
#define PYSDR_MIXDEC_SHAPES(X)                                                                                                  \
  X(1, 0, 1024, 0) X(2, 0, 1024, 0) X(3, 0, 1024, 0) X(4, 0, 1024, 0) X(5, 0, 1024, 0) X(6, 0, 1024, 0) X(7, 0, 1024, 0)       \
  X(8, 0, 1024, 0)                                                                                                              \
  X(1, 6, 1024, 0) X(2, 6, 1024, 0) X(3, 6, 1024, 0) X(4, 6, 1024, 0) X(5, 6, 1024, 0) X(6, 6, 1024, 0) X(7, 6, 1024, 0)       \
  X(8, 6, 1024, 0)                                                                                                              \
  X(1, 4, 1024, 0) X(1, 11, 1024, 0) X(1, 16, 1024, 0) X(1, 21, 1024, 0)                                                        \
  X(2, 11, 768, 1) X(3, 11, 768, 1) X(4, 11, 768, 1) X(5, 11, 768, 1) X(6, 11, 768, 1)                                          \
  X(2, 21, 768, 1) X(3, 21, 768, 1) X(4, 21, 768, 1) X(5, 21, 512, 1) X(6, 21, 512, 1)

inline bool md_listed(MdKey k) {
#define PYSDR_MIXDEC_IS(R, NJ, TPB, MM) if (k == MdKey{R, NJ, TPB, MM}) return true;
  PYSDR_MIXDEC_SHAPES(PYSDR_MIXDEC_IS)
#undef PYSDR_MIXDEC_IS
  return false;
}

// Per-instantiation traits (mixdec.hip MdShape).  The register budget of a wave follows from TPB: 128 at 1024 threads, 168 at
// 768, 256 at 512.
constexpr int md_g(MdKey k) { return (k.r + 1) / 2; }                                       // MM: pairs of sub-receivers = 4-column groups
constexpr int md_budget(MdKey k) { return k.tpb > 768 ? 128 : (k.tpb > 512 ? 168 : 256); }  // registers per lane
// tap pairs per lane that may stay in registers (everything else of the tile loop takes ~75: <1,21> = 42 + 75)
constexpr int md_max_held(MdKey k) { return k.tpb > 768 ? 24 : (md_budget(k) - 80) / 2; }
// RX groups a tile's work is dealt out in: halves above 4 RX at 1024 threads, else as few as the registers allow
constexpr int md_nh(MdKey k) {
  if (k.mm) return 1;
  if (k.tpb > 768) return k.r > 4 ? 2 : 1;
  int nh = 1;
  while (k.nj > 0 && ((k.r + nh - 1) / nh) * k.nj > md_max_held(k) && nh < k.r) ++nh;
  return nh;
}
constexpr int md_rh(MdKey k) { return (k.r + md_nh(k) - 1) / md_nh(k); }                    // RX per task in hold mode
constexpr bool md_can_hold(MdKey k) {
  return k.nj > 0 && (k.mm ? (2 * md_g(k) * k.nj + 60 <= md_budget(k)) : (md_rh(k) * k.nj <= md_max_held(k)));
}

// Which instantiation a decimator's shape runs on.
inline MdKey md_select(int nrx, int up, int kpad, int threads) {
  // 255-tap prototypes at UP = 3 (the BASELINE configurations) have 96 taps per branch
  if (kpad == 96) return {nrx, 6, 1024, 0};
  // the default 1001-tap prototype at UP = 6 (1, 5, 7 MS/s -> 48 kHz: FT8:42, FT8FT4:34, FT8dual:43): 167 taps per branch.
  // From two sub-receivers on the matrix cores (12 waves, two per branch); one sub-receiver holds its eleven tap pairs per lane
  // in registers in six groups of waves.  Front end as a fraction of HBM, matrix cores / vector form: 1 MS/s x 1 RX 0.32 / 0.375,
  // x 2 0.31 / 0.27, x 3 0.245 / 0.187; 5 MS/s x 2 0.66 / 0.67, x 4 0.61 / 0.445; 7 MS/s x 3 0.73 / 0.61 (scripts/diag/up6_mm_ab.sh,
  // profiles/r06_launch_script_rates.txt)
  if (kpad == 176 && up == 6 && threads == 1024) {
    if (nrx >= 2 && nrx <= 6) return {nrx, 11, 768, 1};
    if (nrx == 1) return {1, 11, 1024, 0};
  }
  // single-RX long filters: the fs1 -> FS_OUT resampler of broadcast FM (24/125, 64 taps per branch: more branches than waves,
  // generic task order, but a compile-time tap loop), the 255-tap video filter of the broadcast-FM front end (UP = 1, 256 taps
  // in one branch) and the reference's default 1001-tap prototype at UP = 3 (336 per branch)
  if (nrx == 1) {
    if (kpad == 64) return {1, 4, 1024, 0};
    if (kpad == 256) return {1, 16, 1024, 0};
    if (kpad == 336) return {1, 21, 1024, 0};
  }
  // the default 1001-tap prototype at UP = 3 with several sub-receivers (8 and 4 MS/s -> 48 kHz: FT8tri, TEST) on the matrix
  // cores: 2 - 4 RX 12 waves; 5, 6 RX (three RX pairs = 126 registers of tap operands) 8 waves of up to 256 registers.  Only
  // with the default thread count: pysdr_set_tile(threads) asks for the generic form.
  if (nrx >= 2 && nrx <= 6 && kpad == 336 && up == 3 && threads == 1024) return {nrx, 21, nrx <= 4 ? 768 : 512, 1};
  return {nrx, 0, 1024, 0};
}

// LDS of one workgroup: two tile buffers, the taps (taps_lds), the output stage
inline size_t mixdec_lds_bytes(const MixDecArgs& a) {
  return (2 * (size_t)a.tile_cap + (a.taps_lds ? (size_t)a.nrx * a.up * a.kpad : 0) + (size_t)a.nrx * a.ycap) * sizeof(float2);
}

// The plan of one launch for the shape in `a` (nrx, up, down, kpad, n_out): fills taps_lds, tile_out, tile_cap, yflush, ycap,
// tpc, ntasks, magic_tpc, dq/dr_tile, dq/dr_last and ntiles, and the instantiation to launch.  tile_bytes = 0: the largest tile
// the LDS share of a workgroup allows; threads = the requested thread count (it selects the instantiation, which then clamps it
// to its own).  false: nothing fits the LDS.
inline bool plan_mixdec(MixDecArgs& a, int tile_bytes, int threads_req, int wgs_per_cu, int yflush_cap, MdKey& key) {
  const int nrx = a.nrx, up = a.up, down = a.down, kpad = a.kpad;
  const int ratio = (down + up - 1) / up;
  // The long-prototype multi-RX shapes (768 / 512 threads) read their taps from memory once per launch when their waves can
  // hold them, and the LDS holds tiles and the output stage only; the 1024-thread shapes keep their taps in LDS.
  key = md_select(nrx, up, kpad, threads_req);
  const int threads = std::min(threads_req, key.tpb);
  const int hold_step = (threads / 64) / (up * md_nh(key));       // waves per (branch, RX group); 0: not enough waves to hold
  bool taps_lds = !(key.tpb != 1024 && md_can_hold(key) && hold_step >= 1);
  // two tile buffers + the taps must fit the LDS share of one workgroup
  const long lds_share = (160L * 1024) / wgs_per_cu - 512;
  // tile_bytes == 0: the largest tile the LDS share allows (fewer tiles = less per-tile
  // scalar work, the kernel's scarcest resource).  What is left over holds the output stage
  // (yflush tiles of outputs per RX); if that is less than 4 tiles' worth the tile shrinks.
  const long slack = kpad + 2L * ratio + 8 + 128;   // halo, ownership overhang, whole 64-pair DMA pieces
  long cap = 0, tile_out = 0, yflush = 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    const size_t taps_bytes = taps_lds ? (size_t)nrx * up * kpad * sizeof(float2) : 0;
    long reserve = 0;
    for (int pass = 0; pass < 2; ++pass) {
      cap = tile_bytes > 0 ? tile_bytes / (long)sizeof(float2) : (1L << 30);
      if (2 * cap * (long)sizeof(float2) + (long)taps_bytes + reserve > lds_share)
        cap = (lds_share - (long)taps_bytes - reserve) / (2 * (long)sizeof(float2));
      tile_out = ((cap - slack) * up) / down;
      // whole quads of every polyphase branch -- and, where the waves hold their taps, the same number of quads for every
      // wave of a (branch, RX group): a tile of 60 outputs at 3/500 would give one wave in four a second task
      const long quantum = 4L * up * ((!taps_lds && tile_out >= 4L * up * hold_step) ? hold_step : 1);
      if (tile_out >= quantum) tile_out -= tile_out % quantum;
      tile_out &= ~1L;
      if (tile_out < 2) {
        tile_out = 2;
        cap = slack + (2L * down + up - 1) / up + 2;
      } else {
        cap = std::min(cap, slack + (tile_out * down + up - 1) / up + 2);   // no more LDS than the tile needs
      }
      cap = (cap + 1) & ~1L;
      const long per_tile = (long)nrx * tile_out * (long)sizeof(float2);
      const long left = lds_share - (long)taps_bytes - 2 * cap * (long)sizeof(float2);
      yflush = left > 0 ? std::min(16L, left / per_tile) : 0;
      if (yflush >= 4 || pass == 1) break;
      reserve = 4 * per_tile;
    }
    // hold mode needs every tile to start on the same polyphase branch; a tile too small for that reads its taps from LDS
    if (taps_lds || (tile_out % up) == 0) break;
    taps_lds = true;
  }
  if (yflush < 1) return false;
  // The matrix-core instantiations run only in hold mode (their lane mapping has no generic form): with the taps in LDS these
  // shapes take the generic instantiation, as they did before they had a matrix-core form.
  if (key.mm && taps_lds) key = {nrx, 0, 1024, 0};
  a.taps_lds = taps_lds ? 1 : 0;
  a.tile_out = (int)tile_out;
  a.tile_cap = (int)cap;
  if (yflush_cap > 0 && yflush_cap < yflush) yflush = yflush_cap;
  a.yflush = (int)yflush;
  a.ycap = (int)(yflush * tile_out);
  a.tpc = (int)((((tile_out + up - 1) / up) + 3) >> 2);
  a.ntasks = up * a.tpc;
  a.magic_tpc = (a.tpc == 1) ? 0u : (uint32_t)(4294967296ULL / (unsigned)a.tpc) + 1u;
  a.dq_tile = (int)((tile_out * down) / up);
  a.dr_tile = (int)((tile_out * down) % up);
  a.dq_last = (int)(((tile_out - 1) * down) / up);
  a.dr_last = (int)(((tile_out - 1) * down) % up);
  a.ntiles = a.n_out > 0 ? (a.n_out + a.tile_out - 1) / a.tile_out : 1;
  return true;
}

// The front end's whole decision for one decimator: which of its three forms runs, and for the vector form the plan above.
// A function of the decimator's shape, its call site (raw peak wanted or not) and the context's tuning only -- never of the
// call.  decim_run (api.hip) launches what this says and pysdr_front_end_plan reports it: one helper, so the two cannot drift.
struct FrontEndPlan {
  int form;      // PYSDR_FORM_VECTOR / _MFMA / _SMALL
  int mshape;    // _MFMA: the id in PYSDR_MFMA_SHAPES; -1 otherwise
  MdKey key;     // _VECTOR: the instantiation of PYSDR_MIXDEC_SHAPES
  bool fits;     // false: the vector plan does not fit the LDS (decim_run refuses the call; the small resampler needs it too)
};
// `a` holds the shape (nrx, up, down, kpad, n_out) and receives the vector plan unless the matrix-core form takes the shape.
inline FrontEndPlan plan_front_end(MixDecArgs& a, int kdec, bool want_peak, int tile_bytes, int threads_req, int wgs_per_cu,
                                   int yflush_cap, int mfma_enable) {
  FrontEndPlan f{PYSDR_FORM_VECTOR, -1, MdKey{a.nrx, 0, 1024, 0}, true};
  // one RX with a long prototype at a rate that has an instantiation: the matrix-core form (mixdec_mfma.hip)
  f.mshape = (a.nrx == 1 && mfma_enable) ? mixdec_mfma_shape(a.up, a.down, kdec) : -1;
  if (f.mshape >= 0) { f.form = PYSDR_FORM_MFMA; return f; }
  // one RX, no raw peak wanted, short prototype and a small DOWN/UP (the fs1 -> FS_OUT stage of broadcast FM): resamp_small.hip
  if (a.nrx == 1 && !want_peak && resamp_small_span(a.up, a.down, a.kpad) > 0) f.form = PYSDR_FORM_SMALL;
  f.fits = plan_mixdec(a, tile_bytes, threads_req, wgs_per_cu, yflush_cap, f.key);
  return f;
}

// launch the plan's instantiation (PYSDR_ERR_ARG for a key that is not in PYSDR_MIXDEC_SHAPES)
int launch_mixdec(const MixDecArgs& a, MdKey key, int threads, int grid, hipStream_t st);

}  // namespace pysdr
