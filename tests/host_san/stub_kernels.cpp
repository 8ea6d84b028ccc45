// The launch layer of libpysdr_hip.so for the sanitizer build of its HOST half (tests/host_san):
// every launch_* that the host files call (api.hip, api_objects.hip, api_cw.hip, api_psk.hip, api_fine.hip; the two
// skimmers bring skimmer_host.h, the call list they share with api_fsk.hip and api_ft.hip, into the build), as a host
// function that
//   * reads every input element and writes every output element the real kernel is entitled to touch
//     (the "device" memory is malloc'ed by the fake HIP runtime, so AddressSanitizer checks the sizes and
//     offsets the host code computed: capacities, history prefixes, strides of the per-block arrays);
//   * for the mix + decimate kernel walks ALL tiles of the launch with the kernel's own geometry code
//     (pysdr_amd/csrc/mixdec_geom.h): the incremental step must equal the division, the LDS image must
//     fit the tile buffer and stay inside history + call, outputs and owned samples must partition the
//     call exactly.
//   * with HOST_SAN_TRACE set (fake_hip/hip/hip_runtime.h) adds one line per launch to the queue trace: its name, stream and
//     the scalars and buffers that define it.
// No DSP is computed: parity is the GPU tests' business.  Not part of the product.
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>

#include "common.h"
#include "cw_plan.h"
#include "fine_plan.h"
#include "mixdec_geom.h"
#include "mixdec_mfma_geom.h"
#include "mixdec_plan.h"
#include "objects_plan.h"
#include "psk_plan.h"

namespace pysdr {

namespace {

#define SAN_CHECK(cond, ...)                                              \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "host_san: %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);                                  \
      std::fputc('\n', stderr);                                           \
      std::abort();                                                       \
    }                                                                     \
  } while (0)

volatile float g_sink;

template <class T> void read_all(const T* p, size_t n) {
  const volatile unsigned char* b = reinterpret_cast<const volatile unsigned char*>(p);
  unsigned acc = 0;
  for (size_t i = 0; i < n * sizeof(T); i += 1) acc += b[i];
  g_sink = (float)acc;
}
template <class T> void write_all(T* p, size_t n) { std::memset(p, 0, n * sizeof(T)); }

// ---- the queue trace
using fake_hip::Line;
std::string rk(const char* k, int r) { return std::string(k) + std::to_string(r); }
void tr_plan(Line& l, const PllPlan& p) {
  l.i("K", p.K).i("T", p.T).i("W", p.W).i("Wfast", p.Wfast).i("Wexact", p.Wexact).i("coarse", p.coarse_sweeps).i("Wc_hi", p.Wc_hi)
      .i("Wc_mid", p.Wc_mid).i("seeded", p.seeded).i("Wseed", p.Wseed).i("direct", p.direct).i("tail_cap", p.tail_cap)
      .i("exact_cap", p.exact_cap).p("seg", p.seg).p("lin", p.lin);
}
void tr_stage2(const char* what, const Stage2Args& a, hipStream_t st, const EpilogueArgs* e = nullptr) {
  if (!fake_hip::tracing()) return;
  Line l(what);
  l.st(st).i("nrx", a.nrx).i("n_out", a.n_out).i("ntaps", a.ntaps).i("hy", a.hy).i("t0", a.t0).i("up", a.up).i("down", a.down)
      .i("chunk_len", a.chunk_len).i("nchunks", a.nchunks).i("m0_lo", a.m0_lo).f("fm_scale", a.fm_scale).f("kp", a.pll_kp).f("ki", a.pll_ki)
      .i("spread", a.single_spread).i("sq_ntaps", a.sq_ntaps).p("sqtaps", a.sqtaps).p("blknoise2", a.blknoise2).p("blknoise", a.blknoise)
      .p("blkcnt", a.blkcnt).p("blkpeak", a.blkpeak).p("gain", a.gain).p("state", a.state);
  for (int r = 0; r < a.nrx; ++r) {
    l.p(rk("y", r).c_str(), a.y[r]).p(rk("ypll", r).c_str(), a.ypll[r]).p(rk("aftaps", r).c_str(), a.aftaps[r]).i(rk("real", r).c_str(), a.taps_real[r])
        .p(rk("a", r).c_str(), a.a[r]).p(rk("am", r).c_str(), a.am[r]).i(rk("det", r).c_str(), a.det[r]).i(rk("cx", r).c_str(), a.out_complex[r])
        .i(rk("fcx", r).c_str(), a.fir_complex[r]).i(rk("single", r).c_str(), a.single_block[r]).i(rk("matrix", r).c_str(), a.matrix[r])
        .i(rk("bfo", r).c_str(), a.bfo_fword[r]).f(rk("sq", r).c_str(), a.sq_thresh[r]).i(rk("sqr", r).c_str(), a.sq_ratio[r]);
    if (e) l.p(rk("ybase", r).c_str(), e->ybase[r]).p(rk("ydst", r).c_str(), e->ydst[r]).p(rk("ypllbase", r).c_str(), e->ypllbase[r])
               .p(rk("yplldst", r).c_str(), e->yplldst[r]);
  }
  if (e) l.i("e_nrx", e->nrx).i("e_n_out", e->n_out).i("e_hy", e->hy);
  tr_plan(l, a.pll);
}
void tr_wfm(const char* what, const WfmArgs& a, hipStream_t st) {
  if (!fake_hip::tracing()) return;
  Line l(what);
  l.st(st).i("nrx", a.nrx).i("n1", a.n1).f("scale", a.scale).f("kp", a.kp).f("ki", a.ki).f("norm", a.norm).f("rad2word", a.rad2word)
      .i("fword0", a.fword0).p("state", a.state).i("pass", a.pll_pass);
  for (int r = 0; r < a.nrx; ++r)
    l.p(rk("y1", r).c_str(), a.y1[r]).p(rk("y1base", r).c_str(), a.y1base[r]).p(rk("y1dst", r).c_str(), a.y1dst[r]).p(rk("w", r).c_str(), a.w[r])
        .i(rk("stereo", r).c_str(), a.stereo[r]).p(rk("seed", r).c_str(), a.seed[r]).p(rk("mnT", r).c_str(), a.mnT[r]);
  tr_plan(l, a.pll);
}
void tr_mixdec(const MixDecArgs& a, hipStream_t st, Line& l) {
  l.st(st).i("n_total", a.n_total).i("n_out", a.n_out).i("t0", a.t0).i("up", a.up).i("down", a.down).i("kpad", a.kpad).i("nrx", a.nrx)
      .i("hist_len", a.hist_len).i("aligned16", a.aligned16).i("tile_out", a.tile_out).i("tile_cap", a.tile_cap).i("ntiles", a.ntiles)
      .i("yflush", a.yflush).i("taps_lds", a.taps_lds).i("chunk_len", a.chunk_len).i("zero_n", a.zero_n).i("dbg", a.dbg)
      .p("x", a.x).p("hist", a.hist).p("hist_new", a.hist_new).p("taps", a.taps).p("peak", a.peak).p("zero", a.zero);
  for (int r = 0; r < a.nrx; ++r) l.p(rk("y", r).c_str(), a.y[r]).i(rk("phase", r).c_str(), a.phase0[r]).i(rk("fword", r).c_str(), a.fword[r]);
}

bool same_tile(const Tile& a, const Tile& b) {
  return a.i_first == b.i_first && a.tile_n == b.tile_n && a.rel_f == b.rel_f && a.p_f == b.p_f && a.rel_l == b.rel_l &&
         a.lo == b.lo && a.hi == b.hi && a.own_lo == b.own_lo && a.own_hi == b.own_hi && a.npairs == b.npairs;
}

}  // namespace

static void roll_on_host(const float2* x, const float2* hist_old, float2* hist_new, int hist_len, uint32_t n_total, unsigned* zero, int zero_n);
// What every plan_mixdec result must satisfy (launch_mixdec below; the planner sweep of san_main.cpp): an instantiation that
// exists; waves that hold their taps (taps_lds = 0) and the matrix-core form only in hold mode, with the instantiation's own
// thread count (mixdec.hip: `hold`); the LDS budget; a tile and output stage the kernel can walk.
void check_mixdec_plan(const MixDecArgs& a, MdKey key, int threads) {
  SAN_CHECK(threads >= 64 && threads <= 1024 && (threads & 63) == 0, "threads %d", threads);
  SAN_CHECK(md_listed(key), "no instantiation <%d,%d,%d,%d>", key.r, key.nj, key.tpb, key.mm);
  SAN_CHECK(key.r == a.nrx, "instantiation for %d RX, plan for %d", key.r, a.nrx);
  const int nwaves = std::min(threads, key.tpb) / 64;
  const bool hold = md_can_hold(key) && a.up * md_nh(key) <= nwaves && a.tile_out % a.up == 0;
  SAN_CHECK(hold || (a.taps_lds && !key.mm), "taps_lds %d, <%d,%d,%d,%d> without hold mode (tile_out %d, %d waves)", a.taps_lds,
            key.r, key.nj, key.tpb, key.mm, a.tile_out, nwaves);
  SAN_CHECK(mixdec_lds_bytes(a) <= 160 * 1024, "LDS %zu", mixdec_lds_bytes(a));
  SAN_CHECK(a.nrx >= 1 && a.nrx <= PYSDR_MAX_RX && a.up >= 1 && a.down >= 1 && a.kpad % 16 == 0, "shape");
  SAN_CHECK(a.tile_out >= 2 && (a.tile_out & 1) == 0 && a.ycap == a.yflush * a.tile_out && a.yflush >= 1, "tile_out %d", a.tile_out);
  SAN_CHECK(a.ntiles >= 1 && (long long)a.ntiles * a.tile_out >= a.n_out && (long long)(a.ntiles - 1) * a.tile_out <= std::max(a.n_out, 1), "ntiles");
  SAN_CHECK(a.dq_tile == (int)(((long long)a.tile_out * a.down) / a.up) && a.dr_tile == (int)(((long long)a.tile_out * a.down) % a.up), "tile step");
}

int launch_mixdec(const MixDecArgs& a, MdKey key, int threads, int grid, hipStream_t st) {
  if (fake_hip::tracing()) {
    Line l("launch_mixdec");
    tr_mixdec(a, st, l);
    l.i("key_r", key.r).i("key_nj", key.nj).i("key_tpb", key.tpb).i("key_mm", key.mm).i("threads", threads).i("grid", grid);
  }
  if (a.hist_new) roll_on_host(a.x, a.hist, a.hist_new, a.hist_len, a.n_total, a.zero, a.zero_n);
  check_mixdec_plan(a, key, threads);
  SAN_CHECK(grid >= 1, "grid %d", grid);
  SAN_CHECK(a.hist_len >= a.kpad + 2 && (a.hist_len & 1) == 0, "hist_len %d kpad %d", a.hist_len, a.kpad);
  // every byte the kernel may read or write exists
  read_all(a.x, a.n_total);
  read_all(a.hist, (size_t)a.hist_len);
  read_all(a.taps, (size_t)a.nrx * a.up * a.kpad);
  const uint32_t nchunks = (a.n_total + a.chunk_len - 1) / a.chunk_len;
  write_all(a.peak, nchunks);
  for (int r = 0; r < a.nrx; ++r) write_all(a.y[r], (size_t)a.n_out);
  // the tile walk
  long long outs = 0, own_next = 0;
  Tile prev{};
  for (int b = 0; b < a.ntiles; ++b) {
    const Tile t = tile_geometry(a, b);
    if (b > 0 && b + 1 < a.ntiles && prev.tile_n == a.tile_out) {
      const Tile s = tile_advance(a, prev);
      SAN_CHECK(same_tile(s, t), "tile %d: incremental step != division (i_first %d/%d lo %d/%d hi %d/%d p_f %d/%d)", b,
                s.i_first, t.i_first, s.lo, t.lo, s.hi, t.hi, s.p_f, t.p_f);
    }
    SAN_CHECK(t.i_first == outs && t.tile_n >= 0 && t.tile_n <= a.tile_out, "tile %d outputs", b);
    outs += t.tile_n;
    SAN_CHECK(t.own_lo == own_next, "tile %d owns from %d, expected %lld", b, t.own_lo, own_next);
    own_next = (long long)t.own_hi + 1;
    SAN_CHECK((t.lo & 1) == 0 && t.lo >= -a.hist_len, "tile %d image starts at %d (history %d)", b, t.lo, a.hist_len);
    SAN_CHECK(t.hi < (int)a.n_total || t.tile_n == 0, "tile %d image ends at %d (call %u)", b, t.hi, a.n_total);
    SAN_CHECK(2 * t.npairs <= a.tile_cap, "tile %d: %d samples > tile_cap %d", b, 2 * t.npairs, a.tile_cap);
    if (t.tile_n > 0) {
      // first tap of the first output and last tap of ... lie inside the image
      SAN_CHECK(t.rel_f - (a.kpad - 1) >= t.lo && t.rel_l <= t.hi, "tile %d: taps outside the image", b);
      // whole-piece DMA of interior tiles may read up to 63 pairs past `hi`: still inside the tile buffer
      const int npieces = (t.npairs + 63) >> 6;
      if (a.aligned16 && t.lo >= 0 && (uint32_t)(t.lo + 128 * npieces) <= a.n_total)
        SAN_CHECK(128 * npieces <= a.tile_cap + 128, "tile %d: whole pieces (%d samples) overrun tile_cap %d", b, 128 * npieces, a.tile_cap);
    }
    prev = t;
  }
  SAN_CHECK(outs == a.n_out, "tiles hold %lld outputs, call has %d", outs, a.n_out);
  SAN_CHECK(own_next == (long long)a.n_total, "tiles own %lld samples, call has %u", own_next, a.n_total);
  return PYSDR_OK;
}

// ---- the short-prototype resampler (resamp_small.hip): every workgroup's input span fits what the launch reserves
int g_small_launches = 0;
int launch_resamp_small(const MixDecArgs& a, int grid_cap, int plain, hipStream_t st) {
  if (fake_hip::tracing()) {
    Line l("launch_resamp_small");
    tr_mixdec(a, st, l);
    l.i("grid_cap", grid_cap).i("plain", plain);
  }
  ++g_small_launches;
  if (a.hist_new && a.n_out > 0) roll_on_host(a.x, a.hist, a.hist_new, a.hist_len, a.n_total, a.zero, a.zero_n);   // the real launcher starts no kernel without outputs
  const int span = resamp_small_span(a.up, a.down, a.kpad);
  SAN_CHECK(span > 0 && a.nrx == 1, "shape");
  SAN_CHECK(a.hist_len >= a.kpad - 1, "hist_len %d kpad %d", a.hist_len, a.kpad);
  read_all(a.x, a.n_total);
  read_all(a.hist, (size_t)a.hist_len);
  read_all(a.taps, (size_t)a.up * a.kpad);
  write_all(a.y[0], (size_t)a.n_out);
  for (int i0 = 0; i0 < a.n_out; i0 += 256) {
    const int n_here = std::min(256, a.n_out - i0);
    const long long lo = ((long long)a.t0 + (long long)i0 * a.down) / a.up - (a.kpad - 1);
    const long long hi = ((long long)a.t0 + (long long)(i0 + n_here - 1) * a.down) / a.up;
    SAN_CHECK(hi - lo + 1 <= span, "workgroup at output %d needs %lld samples, reserved %d", i0, hi - lo + 1, span);
    SAN_CHECK(hi < (long long)a.n_total, "output %d reads sample %lld of %u", i0 + n_here - 1, hi, a.n_total);
    SAN_CHECK(lo >= -(long long)a.hist_len - 1, "output %d reads %lld samples into the history of %d", i0, -lo, a.hist_len);
  }
  return PYSDR_OK;
}

// ---- the matrix-core form (mixdec_mfma.hip): the same walk the kernel takes, every DMA element read from the
// real buffers, every window checked against what the image holds
namespace {
template <class G>
int walk_mfma(const MixMfmaArgs& a, int grid) {
  SAN_CHECK(grid >= 1, "grid %d", grid);
  SAN_CHECK((a.hist_len & 1) == 0 && a.hist_len >= G::KT, "hist_len %d", a.hist_len);
  SAN_CHECK((a.origin_rel0 & 1) == 0 && a.origin_rel0 <= 0 && (a.d == 0 || a.d == 1), "origin %d d %d", a.origin_rel0, a.d);
  SAN_CHECK(a.nrel0 == a.origin_rel0 + G::KT - 1 + a.d, "nrel0 %d", a.nrel0);
  SAN_CHECK(a.mrel0 <= 0 && a.mrel0 > -G::US, "mrel0 %d", a.mrel0);
  SAN_CHECK(a.ntiles >= 1 && (long long)a.origin_rel0 + (long long)a.ntiles * G::TILE >= (long long)a.n_total, "tiles do not own the call");
  SAN_CHECK(a.mrel0 + (long long)a.ntiles * G::OUT_PER_TILE >= a.n_out, "tiles do not hold the outputs");
  read_all(a.taps, (size_t)G::UP * a.kpad);
  const uint32_t nchunks = (a.n_total + a.chunk_len - 1) / a.chunk_len;
  write_all(a.peak, nchunks);
  write_all(a.y, (size_t)a.n_out);
  std::vector<unsigned char> have((size_t)G::IMG_PIECES * 128);        // per 8-byte unit of the image: holds a stream sample
  long long own_next = 0, outs = 0;
  for (int tb = 0; tb < a.ntiles; ++tb) {
    const int origin = a.origin_rel0 + tb * G::TILE;
    std::fill(have.begin(), have.end(), 0);
    for (int q = 0; q < G::IMG_PIECES * 64; ++q) {
      const int seg = q / G::SPS, w = q - seg * G::SPS;
      const int rel = origin + seg * G::P + 2 * w;
      const bool ok = (w != G::P / 2) && rel >= -a.hist_len && rel + 1 < (int)a.n_total;
      if (!ok) continue;
      const float2* src = (rel >= 0) ? (a.x + rel) : (a.hist + (a.hist_len + rel));
      SAN_CHECK((reinterpret_cast<uintptr_t>(src) & 7u) == 0, "tile %d slot %d: source not 8-byte aligned", tb, q);
      read_all(src, 2);
      have[2 * (size_t)q] = have[2 * (size_t)q + 1] = 1;
    }
    if (a.n_total & 1u) {
      const int u = (int)a.n_total - 1 - origin;
      if (u >= 0) {
        const int seg = u / G::P, q = seg * G::SPS + ((u - seg * G::P) >> 1);
        if (q < G::IMG_PIECES * 64) { read_all(a.x + (a.n_total - 1), 1); have[2 * (size_t)q] = 1; }
      }
    }
    // ownership: the TILE samples from the image's origin
    const int r_lo = origin > 0 ? origin : 0;
    const int r_end = (origin + G::TILE < (int)a.n_total) ? origin + G::TILE : (int)a.n_total;
    if (r_end > r_lo) {
      SAN_CHECK(r_lo == own_next, "tile %d owns from %d, expected %lld", tb, r_lo, own_next);
      for (int r = r_lo; r < r_end; ++r) {
        const int u = r - origin, unit = u + 2 * (u / G::P);
        SAN_CHECK(unit < (int)have.size() && have[(size_t)unit], "tile %d: owned sample %d not in the image", tb, r);
      }
      own_next = r_end;
    }
    // every tap of every valid output reads a sample the image holds; every read of the padded window is inside the image
    for (int e = 0; e < G::OUT_PER_TILE; ++e) {
      const int idx = a.mrel0 + tb * G::OUT_PER_TILE + e;
      const int rho = e / G::US, rem = e - rho * G::US, t = rem / G::UP, c = rem - t * G::UP;
      for (int j : {0, G::KPP - 1}) {                                                  // first and last sample of the padded window
        const int unit = rho * (G::SEGB / 8) + (a.d + j) + 2 * ((a.d + j) / G::P);
        SAN_CHECK(unit >= 0 && unit < (int)have.size(), "tile %d row %d: window sample %d outside the image", tb, rho, j);
      }
      if (idx < 0 || idx >= a.n_out) continue;
      ++outs;
      const int jtop = G::KT - 1 + t * G::DOWN + (c * G::DOWN) / G::UP;
      const int rel_new = a.nrel0 + (tb * G::ROWS + rho) * G::P + t * G::DOWN + (c * G::DOWN) / G::UP;
      SAN_CHECK(rel_new >= 0 && rel_new < (int)a.n_total, "tile %d output %d: newest sample %d outside the call", tb, idx, rel_new);
      for (int k = 0; k < G::KT; ++k) {
        const int j = jtop - k;
        const int unit = rho * (G::SEGB / 8) + (a.d + j) + 2 * ((a.d + j) / G::P);
        SAN_CHECK(have[(size_t)unit], "tile %d output %d tap %d: sample not in the image", tb, idx, k);
      }
    }
  }
  SAN_CHECK(own_next == (long long)a.n_total, "tiles own %lld samples, call has %u", own_next, a.n_total);
  SAN_CHECK(outs == a.n_out, "tiles hold %lld outputs, call has %d", outs, a.n_out);
  return PYSDR_OK;
}
}  // namespace

// the history roll as hist_roll.h does it (one workgroup of the decimator kernel, or the launch of its own)
static void roll_on_host(const float2* x, const float2* hist_old, float2* hist_new, int hist_len, uint32_t n_total, unsigned* zero, int zero_n) {
  SAN_CHECK(hist_new != nullptr && hist_new != hist_old, "history roll in place");
  if (zero_n > 0) write_all(zero, (size_t)zero_n);
  for (int j = 0; j < hist_len; ++j) {
    const long long rel = (long long)n_total - hist_len + j;
    hist_new[j] = (rel >= 0) ? x[rel] : hist_old[hist_len + rel];
  }
}

bool mixdec_mfma_plan(int shape, unsigned long long s0, unsigned long long m0, unsigned long long n, MfmaPlan* p) {
#define PYSDR_MFMA_PLAN(ID, UP, DOWN, S, KT, NB, WK, NP, NBUF, CARRY) \
  if (shape == ID) return mfma_plan<MfmaGeo<UP, DOWN, S, KT, NB, WK, NP, NBUF, CARRY>>(s0, m0, n, p);
  PYSDR_MFMA_SHAPES(PYSDR_MFMA_PLAN)
#undef PYSDR_MFMA_PLAN
  return false;
}
int g_mfma_launches = 0;
int launch_mixdec_mfma(int shape, const MixMfmaArgs& a, int grid, hipStream_t st) {
  if (fake_hip::tracing())
    Line("launch_mixdec_mfma").st(st).i("shape", shape).i("grid", grid).i("n_total", a.n_total).i("n_out", a.n_out).i("hist_len", a.hist_len)
        .i("origin_rel0", a.origin_rel0).i("d", a.d).i("nrel0", a.nrel0).i("mrel0", a.mrel0).i("ntiles", a.ntiles).i("kpad", a.kpad)
        .i("phase", a.phase0).i("fword", a.fword).i("chunk_len", a.chunk_len).i("zero_n", a.zero_n).p("x", a.x).p("hist", a.hist)
        .p("hist_new", a.hist_new).p("taps", a.taps).p("y", a.y).p("peak", a.peak).p("zero", a.zero);
  ++g_mfma_launches;
  if (a.hist_new) roll_on_host(a.x, a.hist, a.hist_new, a.hist_len, a.n_total, a.zero, a.zero_n);
#define PYSDR_MFMA_LAUNCH(ID, UP, DOWN, S, KT, NB, WK, NP, NBUF, CARRY) \
  if (shape == ID) return walk_mfma<MfmaGeo<UP, DOWN, S, KT, NB, WK, NP, NBUF, CARRY>>(a, grid);
  PYSDR_MFMA_SHAPES(PYSDR_MFMA_LAUNCH)
#undef PYSDR_MFMA_LAUNCH
  SAN_CHECK(false, "no shape %d", shape);
  return PYSDR_ERR_ARG;
}

int launch_hist_roll(const float2* x, const float2* hist_old, float2* hist_new, int hist_len, uint32_t n_total, unsigned* zero, int zero_n, hipStream_t st) {
  if (fake_hip::tracing())
    Line("launch_hist_roll").st(st).i("hist_len", hist_len).i("n_total", n_total).i("zero_n", zero_n).p("x", x).p("hist", hist_old)
        .p("hist_new", hist_new).p("zero", zero);
  roll_on_host(x, hist_old, hist_new, hist_len, n_total, zero, zero_n);
  return PYSDR_OK;
}

static void check_plan(const PllPlan& p, int n, int nrx) {
  SAN_CHECK(p.K >= 1 && p.T >= 64 && (long long)p.K * p.T >= n && (long long)(p.K - 1) * p.T < std::max(n, 1), "PLL plan K %d T %d n %d", p.K, p.T, n);
  SAN_CHECK(p.W % 64 == 0 && p.Wfast % 64 == 0 && p.Wexact % 64 == 0 && p.T % 64 == 0, "PLL plan alignment");
  SAN_CHECK(p.Wc_hi % 64 == 0 && p.Wc_mid % 64 == 0 && p.Wc_hi >= 0 && p.Wc_mid >= 0 && p.tail_cap >= 0, "staged warm-up plan");
  write_all(p.seg, (size_t)nrx * p.K * 4);
}

int launch_am_phase(const Stage2Args& a, hipStream_t st) {
  tr_stage2("launch_am_phase", a, st);
  for (int r = 0; r < a.nrx; ++r)
    if (a.det[r] == kDetPll) {
      SAN_CHECK(a.ypll[r] != nullptr, "AM-Synch rx %d has no PLL buffer", r);
      read_all(a.y[r], (size_t)a.n_out);
      write_all(a.ypll[r], (size_t)a.n_out);
    }
  return PYSDR_OK;
}

int launch_pll(const Stage2Args& a, hipStream_t st) {
  tr_stage2("launch_pll", a, st);
  check_plan(a.pll, a.n_out, a.nrx);
  for (int r = 0; r < a.nrx; ++r)
    if (a.det[r] == kDetPll) {
      SAN_CHECK(a.ypll[r] != nullptr, "AM-Synch rx %d has no PLL buffer", r);
      read_all(a.y[r], (size_t)a.n_out);
      write_all(a.ypll[r], (size_t)a.n_out);
      // am_pll_seg_kernel: grid (K, nrx), one wave per segment; segment k > 0 with s0 - W > 0 reads the phase words of
      // [s0 - W, s1) -- the first 64 of them for its start guess, so W >= 64 must hold -- and segment 0 those of [0, s1)
      const int K = a.pll.K, T = a.pll.T, W = a.pll.W;
      SAN_CHECK(W >= 64 && a.pll.Wexact <= W && a.pll.coarse_sweeps >= 0 && a.pll.coarse_sweeps <= 8, "carrier-loop plan W %d Wexact %d coarse %d", W, a.pll.Wexact, a.pll.coarse_sweeps);
      for (int k = 0; k < K; ++k) {
        const long long s0 = (long long)k * T, s1 = std::min<long long>(s0 + T, a.n_out);
        const long long wb = (k > 0 && s0 - W > 0) ? s0 - W : 0;
        SAN_CHECK(s1 > s0 && s1 <= a.n_out, "carrier-loop segment %d is [%lld, %lld) of %d", k, s0, s1, a.n_out);
        if (wb > 0) SAN_CHECK(wb + 64 <= s0 && s0 <= a.n_out, "carrier-loop segment %d guesses from [%lld, %lld) of %d", k, wb, wb + 64, a.n_out);
      }
    }
  read_all(a.state, (size_t)a.nrx);
  return PYSDR_OK;
}

int launch_demod_fir(const Stage2Args& a, hipStream_t st) {
  tr_stage2("launch_demod_fir", a, st);
  for (int r = 0; r < a.nrx; ++r) {
    const float2* src = (a.det[r] == kDetPll) ? a.ypll[r] : a.y[r];
    read_all(src - a.hy, (size_t)a.hy + a.n_out);                  // history prefix + the call
    read_all(a.aftaps[r], (size_t)((a.ntaps + 3) & ~3));
    write_all(a.a[r], (size_t)a.n_out);
    for (int k = 0; k < a.nchunks; ++k) {                           // per-block accumulators, kBlkStride words apart
      a.blkpeak[((size_t)r * a.nchunks + k) * kBlkStride] = 0u;
      a.blknoise[((size_t)r * a.nchunks + k) * kBlkStride] = 0.f;
      a.blkcnt[((size_t)r * a.nchunks + k) * kBlkStride] = 0u;
    }
    if (a.sq_ratio[r] && a.sq_thresh[r] > 0.f && a.det[r] == kDetFm) {   // the ratio squelch's second set of block sums and its two FIRs
      SAN_CHECK(a.blknoise2 != nullptr && a.sqtaps != nullptr && a.sq_ntaps >= 1 && a.sq_ntaps <= kSqTapsMax, "ratio squelch armed without its buffers (%d taps)", a.sq_ntaps);
      SAN_CHECK(a.sq_ntaps - 1 <= a.hy - 2, "ratio squelch: %d taps reach behind the %d outputs of history", a.sq_ntaps, a.hy);
      read_all(a.sqtaps, (size_t)2 * kSqTapsMax);
      for (int k = 0; k < a.nchunks; ++k) a.blknoise2[((size_t)r * a.nchunks + k) * kBlkStride] = 0.f;
    }
  }
  return PYSDR_OK;
}

static int stub_epilogue(const EpilogueArgs& a);
int launch_agc_scan(const Stage2Args& a, const EpilogueArgs& e, hipStream_t st) {
  tr_stage2("launch_agc_scan", a, st, &e);
  for (int r = 0; r < a.nrx; ++r) {
    for (int k = 0; k < a.nchunks; ++k) g_sink = (float)a.blkpeak[((size_t)r * a.nchunks + k) * kBlkStride];
    write_all(a.gain + (size_t)r * a.nchunks, (size_t)a.nchunks);
  }
  read_all(a.state, (size_t)a.nrx);
  return stub_epilogue(e);
}

int launch_apply(const Stage2Args& a, hipStream_t st) {
  tr_stage2("launch_apply", a, st);
  for (int r = 0; r < a.nrx; ++r) {
    read_all(a.a[r], (size_t)a.n_out);
    write_all(a.am[r], (size_t)a.n_out * (a.out_complex[r] ? 2 : 1));
  }
  return PYSDR_OK;
}

static int stub_epilogue(const EpilogueArgs& a) {
  SAN_CHECK(a.hy <= 4096, "hy %d", a.hy);
  for (int r = 0; r < a.nrx; ++r) {
    SAN_CHECK(a.ydst[r] != nullptr, "rx %d: no destination for the next call's prefix", r);
    SAN_CHECK((a.ypllbase[r] == nullptr) == (a.yplldst[r] == nullptr), "rx %d: PLL buffer and its prefix destination", r);
    const std::pair<float2*, float2*> jobs[2] = {{a.ybase[r], a.ydst[r]}, {a.ypllbase[r], a.yplldst[r]}};
    for (const auto& j : jobs)
      if (j.first) {
        read_all(j.first, (size_t)a.hy + a.n_out);
        std::memmove(j.second, j.first + a.n_out, (size_t)a.hy * sizeof(float2));     // (the pair's other buffer when the calls overlap)
      }
  }
  return PYSDR_OK;
}

int launch_wfm_disc(const WfmArgs& a, hipStream_t st) {
  tr_wfm("launch_wfm_disc", a, st);
  for (int r = 0; r < a.nrx; ++r) {
    SAN_CHECK(a.y1[r] == a.y1base[r] + 2, "IF buffer layout");
    read_all(a.y1[r] - 1, (size_t)a.n1 + 1);
    write_all(a.w[r], (size_t)a.n1);
    if (a.mnT[r] != nullptr)                                 // the seed kernels' copy: every sample of the call lands inside the padded buffer
      for (int i = 0; i < a.n1; i += (a.n1 > 4096 ? 997 : 1)) { SAN_CHECK(pll_seed_index(i) < pll_seed_mnt_floats(a.n1), "mnT index of sample %d", i); a.mnT[r][pll_seed_index(i)] = 0.f; }
    SAN_CHECK(a.y1dst[r] != nullptr, "IF prefix destination");
    if (a.n1 > 0) a.y1dst[r][1] = a.y1[r][a.n1 - 1];
  }
  return PYSDR_OK;
}

size_t pll_seed_doubles(int n1max) {
  const size_t nlanes = ((size_t)n1max + kSeedRun - 1) / kSeedRun, nwaves = (nlanes + 63) / 64;
  return nlanes * 6 + nwaves * 6 + nwaves * 2 + nlanes * 2 + 16 * 6;
}

int launch_wfm_seed(const WfmArgs& a, hipStream_t) {
  // pllseed.hip: a lane per 32 samples, a wave per 2048; the scan buffers of a stereo RX hold both levels and pass 1's states
  for (int r = 0; r < a.nrx; ++r)
    if (a.stereo[r] && a.seed[r] != nullptr && a.mnT[r] != nullptr) {
      read_all(a.mnT[r], pll_seed_mnt_floats(a.n1));
      write_all(a.seed[r], pll_seed_doubles(a.n1));
      SAN_CHECK(a.pll.T % kSeedRun == 0 && a.pll.Wseed % kSeedRun == 0 && a.pll.Wseed >= 0, "seed plan T %d Wseed %d", a.pll.T, a.pll.Wseed);
    }
  return PYSDR_OK;
}

bool wfm_any_stereo(const WfmArgs& a) {
  bool any = false;
  for (int r = 0; r < a.nrx; ++r) any |= (a.stereo[r] != 0);
  return any && a.n1 > 0;
}

int launch_wfm_pll(const WfmArgs& a, hipStream_t st) {
  tr_wfm("launch_wfm_pll", a, st);
  check_plan(a.pll, a.n1, a.nrx);
  if (a.pll.seeded && a.pll.K > 1) { const int rc = launch_wfm_seed(a, st); if (rc) return rc; }
  for (int r = 0; r < a.nrx; ++r)
    if (a.stereo[r]) { read_all(a.w[r], (size_t)a.n1); write_all(a.w[r], (size_t)a.n1); }
  read_all(a.state, (size_t)a.nrx);
  return PYSDR_OK;
}

int launch_quad_mixer(const float2* x, float2* y, size_t n, uint32_t phase0, uint32_t fword, hipStream_t st) {
  if (fake_hip::tracing()) Line("launch_quad_mixer").st(st).i("n", (long long)n).i("phase", phase0).i("fword", fword).p("x", x).p("y", y);
  read_all(x, n);
  write_all(y, n);
  return PYSDR_OK;
}

int launch_fir_real(const float* xx, const float* h, int nt, float* y, int n, hipStream_t st) {
  if (fake_hip::tracing()) Line("launch_fir_real").st(st).i("nt", nt).i("n", n).p("x", xx).p("h", h).p("y", y);
  read_all(xx, (size_t)n + nt - 1);
  read_all(h, (size_t)nt);
  write_all(y, (size_t)n);
  return PYSDR_OK;
}

int launch_psd_pre(const float2* x, size_t hop, int nframes, int chunk, int nfft, const float* win, float2* work, int is_complex,
                   hipStream_t st) {
  if (fake_hip::tracing())
    Line("launch_psd_pre").st(st).i("hop", (long long)hop).i("nframes", nframes).i("chunk", chunk).i("nfft", nfft).i("complex", is_complex)
        .p("x", x).p("win", win).p("work", work);
  read_all(win, (size_t)chunk);
  for (int f = 0; f < nframes; ++f) {
    if (is_complex) read_all(x + (size_t)f * hop, (size_t)chunk);
    else read_all(reinterpret_cast<const float*>(x) + (size_t)f * hop, (size_t)chunk);
  }
  write_all(work, (size_t)nframes * nfft);
  return PYSDR_OK;
}

int launch_psd_post(const float2* work, int nframes, int nfft, int half, int db, float* out, hipStream_t st) {
  if (fake_hip::tracing())
    Line("launch_psd_post").st(st).i("nframes", nframes).i("nfft", nfft).i("half", half).i("db", db).p("work", work).p("out", out);
  read_all(work, (size_t)nframes * nfft);
  write_all(out, (size_t)nframes * (half ? nfft / 2 : nfft));
  return PYSDR_OK;
}

int launch_psd64k(const float2* x, size_t hop, int nframes, const float* win, float2* work, float* out, int db, hipStream_t st, int packed) {
  if (fake_hip::tracing())
    Line("launch_psd64k").st(st).i("hop", (long long)hop).i("nframes", nframes).i("db", db).i("packed", packed).p("x", x).p("win", win)
        .p("work", work).p("out", out);
  read_all(win, 32768);
  for (int f = 0; f < nframes; ++f) read_all(x + (size_t)f * hop, 32768);
  write_all(work, (size_t)nframes * 65536);
  write_all(out, (size_t)nframes * 65536);
  return PYSDR_OK;
}

// ==== the four stream objects (api_objects.hip; footprints read off waterfall.hip / rtty.hip / chan.hip / bank.hip) ====

// ---- waterfall
// wf_fill_kernel: writes p[0, n)
int launch_wf_fill(float* p, size_t n, float v, hipStream_t st) {
  if (fake_hip::tracing()) Line("launch_wf_fill").st(st).i("n", (long long)n).f("v", v).p("p", p);
  write_all(p, n);
  return PYSDR_OK;
}
// wf_push_kernel: reads line[0, n), writes slot[0, nfft) (every bin: the fill beyond n)
int launch_wf_push(const float* line, int n, int nfft, int shift, float* slot, hipStream_t st) {
  if (fake_hip::tracing()) Line("launch_wf_push").st(st).i("n", n).i("nfft", nfft).i("shift", shift).p("line", line).p("slot", slot);
  SAN_CHECK(n >= 0 && n <= nfft && shift >= 0 && shift < nfft, "n %d shift %d nfft %d", n, shift, nfft);
  read_all(line, (size_t)n);
  write_all(slot, (size_t)nfft);
  return PYSDR_OK;
}
static void check_wf(const WfArgs& a) {
  SAN_CHECK(a.cnt >= 1 && a.cnt <= a.ncols && a.head >= 0 && a.head < a.ncols && a.shift >= 0 && a.shift < a.nfft, "cnt %d head %d shift %d", a.cnt, a.head, a.shift);
}
// wf_mean_kernel: reads the newest cnt columns wf[((head - k) mod ncols) nfft + [0, nfft)], k = 1 .. cnt; writes mean[0, nfft).
// wf_median_kernel: reads mean[0, nfft), writes stat[0]
int launch_wf_mean_median(const WfArgs& a, hipStream_t st) {
  if (fake_hip::tracing())
    Line("launch_wf_mean_median").st(st).i("nfft", a.nfft).i("ncols", a.ncols).i("head", a.head).i("cnt", a.cnt).i("shift", a.shift).p("wf", a.wf)
        .p("mean", a.mean).p("stat", a.stat);
  check_wf(a);
  for (int k = 1; k <= a.cnt; ++k) read_all(a.wf + (size_t)((a.head - k + a.ncols) % a.ncols) * a.nfft, (size_t)a.nfft);
  write_all(a.mean, (size_t)a.nfft);
  read_all(a.mean, (size_t)a.nfft);
  write_all(a.stat, 1);
  return PYSDR_OK;
}
// wf_max_kernel: reads wf[0, nfft ncols), atomicMax on stat[1].  wf_image_kernel: reads wf (every column), stat[0], stat[1];
// writes image[0, ncols nfft)
int launch_wf_max_image(const WfArgs& a, int npsd, float pan_dr, hipStream_t st) {
  if (fake_hip::tracing())
    Line("launch_wf_max_image").st(st).i("nfft", a.nfft).i("ncols", a.ncols).i("head", a.head).i("shift", a.shift).i("npsd", npsd).f("pan_dr", pan_dr)
        .p("wf", a.wf).p("stat", a.stat).p("image", a.image);
  check_wf(a);
  SAN_CHECK(npsd >= 1 && npsd <= a.nfft, "npsd %d", npsd);
  read_all(a.wf, (size_t)a.nfft * a.ncols);
  read_all(a.stat, 2);
  write_all(a.stat + 1, 1);
  write_all(a.image, (size_t)a.nfft * a.ncols);
  return PYSDR_OK;
}
// wf_peaks_kernel: reads x[0, n); a peak needs a rise in front and a fall behind it, so at most (n - 1) / 2 of them: writes
// pos / state / kept [0, that many) and count[0].  The stub reports the most, so that the host's copy of `kept` is as long as it gets.
int launch_wf_peaks(const float* x, int n, double height, int dist, int* pos, int* state, int* kept, int* count, hipStream_t st) {
  if (fake_hip::tracing())
    Line("launch_wf_peaks").st(st).i("n", n).f("height", height).i("dist", dist).p("x", x).p("pos", pos).p("state", state).p("kept", kept).p("count", count);
  const size_t most = n >= 3 ? (size_t)(n - 1) / 2 : 0;
  SAN_CHECK(dist >= 1 && pos + most <= state && state + most <= kept && kept + most <= count, "the four parts of the peak scratch overlap (n %d)", n);
  read_all(x, (size_t)n);
  write_all(pos, most); write_all(state, most); write_all(kept, most);
  *count = (int)most;
  return PYSDR_OK;
}

// ---- RTTY decoder bank: line x >= 1 lives in ring row x % R; nothing before line 1 is read
namespace {
template <class T> void ring_rd(const T* ring, long long x, int R, int w, int col, int n) { if (x >= 1) read_all(ring + (size_t)(x % R) * w + col, (size_t)n); }
template <class T> void ring_wr(T* ring, long long x, int R, int w) { write_all(ring + (size_t)(x % R) * w, (size_t)w); }
}  // namespace
int launch_rtty_decode(const RttyArgs& a, hipStream_t st) {
  if (fake_hip::tracing())
    Line("launch_rtty_decode").st(st).i("nfft", a.nfft).i("flipped", a.flipped).i("nlines", a.nlines).i("band_lo", a.band_lo).i("nband", a.nband)
        .i("moff", a.moff).i("nsh", a.nsh).i("nb", a.nb).i("flo", a.flo).i("fhi", a.fhi).i("n0", a.n0).i("n_first", a.n_first).i("nd", a.nd).i("R", a.R)
        .p("lines", a.lines).p("band", a.band).p("s4", a.s4).p("best", a.best).p("sc2", a.sc2).p("isym", a.isym).p("shift", a.shift).p("t", a.t)
        .p("snr", a.snr).p("held", a.held).p("code", a.code).p("ndet", a.ndet);
  const int R = a.R, nb = a.nb, nband = a.nband;
  SAN_CHECK(a.nlines >= 1 && a.n0 >= 1 && a.nd >= 0 && a.nd <= a.max_dec, "nlines %d n0 %lld nd %d max_dec %d", a.nlines, a.n0, a.nd, a.max_dec);
  // the deepest reach is rt_sc2's best_{n-120}: its row must not be one this call writes
  SAN_CHECK(a.nlines + 4 * kM <= R, "%d lines + 120 of reach > %d ring rows", a.nlines, R);
  SAN_CHECK(a.band_lo >= 0 && a.band_lo + nband <= a.nfft, "band [%d, +%d) of %d", a.band_lo, nband, a.nfft);
  SAN_CHECK(a.moff >= 0 && a.moff + nb + a.nsh <= nband, "decoder columns [%d, +%d) + %d of %d", a.moff, nb, a.nsh, nband);
  SAN_CHECK(a.flo == a.fhi || (a.flo >= 0 && a.flo < a.fhi && a.fhi + a.nsh <= nband), "finder columns [%d, %d) + %d of %d", a.flo, a.fhi, a.nsh, nband);
  SAN_CHECK(a.nd == 0 || (a.n_first % kM == 0 && a.n_first >= a.n0 && a.n_first + (long long)kM * (a.nd - 1) < a.n0 + a.nlines), "decisions");
  for (int l = 0; l < a.nlines; ++l) {
    const long long n = a.n0 + l;
    // rt_gather: lines[l nfft + col], col = bin (flipped) or nfft - 1 - bin, bin in [band_lo, band_lo + nband); writes band row n
    read_all(a.lines + (size_t)l * a.nfft + (a.flipped ? a.band_lo : a.nfft - a.band_lo - nband), (size_t)nband);
    ring_wr(a.band, n, R, nband);
  }
  for (int l = 0; l < a.nlines; ++l) {
    const long long n = a.n0 + l;
    // rt_s4: band rows n-3 .. n, columns moff + k and moff + k + nsh, k < nb; writes s4 row n
    for (int q = 0; q < 4; ++q) { ring_rd(a.band, n - q, R, nband, a.moff, nb); ring_rd(a.band, n - q, R, nband, a.moff + a.nsh, nb); }
    ring_wr(a.s4, n, R, nb);
  }
  for (int l = 0; l < a.nlines; ++l) {
    const long long n = a.n0 + l;
    // rt_best: s4 rows n-28, n-24, ..., n; writes best and isym row n
    for (int g = 0; g < 8; ++g) ring_rd(a.s4, n - 28 + 4 * g, R, nb, 0, nb);
    ring_wr(a.best, n, R, nb); ring_wr(a.isym, n, R, nb);
  }
  for (int l = 0; l < a.nlines; ++l) {
    const long long n = a.n0 + l;
    // rt_sc2: best rows n, n-30, ..., n-120; writes sc2 row n
    for (int i = 0; i < 5; ++i) ring_rd(a.best, n - i * kM, R, nb, 0, nb);
    ring_wr(a.sc2, n, R, nb);
  }
  for (int j = 0; j < a.nd; ++j) {
    const long long n = a.n_first + (long long)kM * j;
    // rt_decide: sc2 rows n-29 .. n and (n > 30) n-59 .. n-30; isym row tlast + 1, band rows tlast - 28 + 4 q with tlast anywhere
    // in [n-60, n-31]: isym rows n-59 .. n-30, band rows n-88 .. n-31, columns moff + k and + nsh; writes t / snr / held [j][nb]
    for (long long x = n - (n > kM ? 59 : 29); x <= n; ++x) ring_rd(a.sc2, x, R, nb, 0, nb);
    if (n > kM) {
      for (long long x = n - 59; x <= n - 30; ++x) ring_rd(a.isym, x, R, nb, 0, nb);
      for (long long x = n - 88; x <= n - 31; ++x) { ring_rd(a.band, x, R, nband, a.moff, nb); ring_rd(a.band, x, R, nband, a.moff + a.nsh, nb); }
    }
    write_all(a.t + (size_t)j * nb, (size_t)nb); write_all(a.snr + (size_t)j * nb, (size_t)nb); write_all(a.held + (size_t)j * nb, (size_t)nb);
  }
  if (a.nd > 0) {
    // rt_emit: snr, held [nd][nb]; shift[nb] read and written; writes code [nd][nb]
    read_all(a.snr, (size_t)a.nd * nb); read_all(a.held, (size_t)a.nd * nb); read_all(a.shift, (size_t)nb);
    write_all(a.shift, (size_t)nb); write_all(a.code, (size_t)a.nd * nb);
  }
  for (int l = 0; l < a.nlines; ++l) {
    const long long n = a.n0 + l;
    // rt_find: band rows n-20 .. n, columns [flo, fhi) and + nsh; writes ndet[l]
    for (int q = 0; q <= 20 && a.fhi > a.flo; ++q) { ring_rd(a.band, n - q, R, nband, a.flo, a.fhi - a.flo); ring_rd(a.band, n - q, R, nband, a.flo + a.nsh, a.fhi - a.flo); }
    write_all(a.ndet + l, 1);
  }
  return PYSDR_OK;
}

// ---- the FFT passes of both channelizer stages (fft_lds.h, the loop in each kernel): what a kernel is handed for M points against the plan's
// npass / radix[] -- the same passes, making M; every multiplier magic_of of the divisor it stands for (M / R, and
// nq = nb / R or 0 where nq = 1); tw[0, M) read; every entry of perm[0, nperm) an LDS position of a frame
static void trace_passes(Line& l, const FftPasses& f) {
  for (int s = 0; s < f.npass; ++s) l.i(rk("radix", s).c_str(), f.radix[s]).i(rk("mper", s).c_str(), f.magic_per[s]).i(rk("mnq", s).c_str(), f.magic_nq[s]);
}
static void check_passes(const FftPasses& f, int M, int npass, const int* radix, const float* tw, const int* perm, int nperm) {
  SAN_CHECK(f.npass == npass && npass >= 1 && npass <= kFftMaxPass, "npass %d, the plan's %d", f.npass, npass);
  int nb = M;
  for (int s = 0; s < f.npass; ++s) {
    const int R = f.radix[s];
    SAN_CHECK(R == radix[s] && R >= 2 && nb % R == 0, "radix[%d] = %d, the plan's %d", s, R, radix[s]);
    SAN_CHECK(f.magic_per[s] == magic_of(M / R), "magic_per[%d] = %u for %d", s, f.magic_per[s], M / R);
    SAN_CHECK(f.magic_nq[s] == (nb / R > 1 ? magic_of(nb / R) : 0u), "magic_nq[%d] = %u for %d", s, f.magic_nq[s], nb / R);
    nb /= R;
  }
  SAN_CHECK(nb == 1, "passes do not make %d", M);
  read_all(tw, 2 * (size_t)M);
  for (int r = 0; r < nperm; ++r) SAN_CHECK(perm[r] >= 0 && perm[r] < M, "perm[%d] = %d", r, perm[r]);
}

// ---- polyphase channelizer
int chan_prepare(const ChanPlan& p) {
  SAN_CHECK(p.lds_bytes == p.fw * p.mp * (int)sizeof(float2) && p.lds_bytes <= 160 * 1024, "LDS %d", p.lds_bytes);
  return PYSDR_OK;
}
// chan_kernel: frame t of the call and tap row p read x[(t - C p) D + off0 - r], r < M -- from x where that is in [0, n), from
// hist[H + .] where in [-H, 0), nothing outside: all of x[0, n) and hist[0, H); taps[p M + r], p < P; tw[0, M); perm[0, nk).
// Writes y[a pitch + i], a < nk, i < nframes.
int launch_chan(const ChanPlan& p, const ChanArgs& a, int grid, hipStream_t st) {
  if (fake_hip::tracing()) {
    Line l("launch_chan");
    l.st(st).i("grid", grid).i("threads", p.threads).i("lds", p.lds_bytes).i("C", p.C).i("fi", p.fi).i("H", a.H).i("n", a.n).i("off0", a.off0)
        .i("mf_lo", a.mf_lo).i("nframes", a.nframes).i("M", a.M).i("D", a.D).i("P", a.P).i("mp", a.mp).i("fw", a.fw).i("nk", a.nk).i("pitch", a.pitch)
        .i("npass", a.fft.npass).i("magic_M", a.magic_M).i("magic_fw", a.magic_fw).i("xq", a.xq).i("xr", a.xr)
        .p("x", a.x).p("hist", a.hist).p("taps", a.taps).p("tw", a.tw).p("perm", a.perm).p("y", a.y);
    trace_passes(l, a.fft);
  }
  SAN_CHECK(grid == a.xq * 8 + a.xr && a.xr >= 0 && a.xr < 8, "grid %d != xq %d * 8 + xr %d", grid, a.xq, a.xr);
  SAN_CHECK(a.nframes >= 1 && (long long)grid * a.fw >= a.nframes && (long long)(grid - 1) * a.fw < a.nframes, "grid %d of %d frames covers %d", grid, a.fw, a.nframes);
  SAN_CHECK(a.fw == p.fw && a.mp == p.mp && a.mp == (a.M | 1) && p.fw % p.fi == 0 && p.C * a.D == a.M && (p.threads == 256 || p.threads == 1024), "plan");
  SAN_CHECK(a.off0 >= 0 && a.off0 < a.D && (long long)(a.nframes - 1) * a.D + a.off0 < a.n, "last frame ends at %lld of %d", (long long)(a.nframes - 1) * a.D + a.off0, a.n);
  SAN_CHECK(a.P >= 1 && a.P * a.M - 1 <= a.H, "P %d M %d reach behind the history of %d", a.P, a.M, a.H);
  SAN_CHECK(a.pitch >= a.nframes, "pitch %lld < %d frames", a.pitch, a.nframes);
  SAN_CHECK(a.magic_M == magic_of(a.M) && a.magic_fw == magic_of(a.fw), "magic_M %u for %d, magic_fw %u for %d", a.magic_M, a.M, a.magic_fw, a.fw);
  check_passes(a.fft, a.M, p.npass, p.radix, reinterpret_cast<const float*>(a.tw), a.perm, a.nk);
  read_all(a.x, (size_t)a.n);
  read_all(a.hist, (size_t)a.H);
  read_all(a.taps, (size_t)a.P * a.M);
  for (int r = 0; r < a.nk; ++r) write_all(a.y + (size_t)r * (size_t)a.pitch, (size_t)a.nframes);
  return PYSDR_OK;
}
// chan_roll: neu[i] = old[i + n] while i + n < H, else x[i + n - H], i < H
int launch_chan_roll(const float2* x, int n, const float2* old, float2* neu, int H, hipStream_t st) {
  if (fake_hip::tracing()) Line("launch_chan_roll").st(st).i("n", n).i("H", H).p("x", x).p("old", old).p("new", neu);
  SAN_CHECK(neu != old && n >= 1, "history roll in place / empty call");
  for (int i = 0; i < H; ++i) {
    const long long j = (long long)i + n;
    neu[i] = j < H ? old[j] : x[j - H];
  }
  return PYSDR_OK;
}

// ---- channel bank
// bank_kernel, per row: the detector at d[i], i in [-(T - 1), n_out), reads y[i] (AM) or y[i - 2 .. i] (NFM); taps[0, tp);
// writes a[row apitch + i], i < n_out (whole float4 pairs where 8 outputs fit) and pmax / psum[row ptiles + t], t < ntiles.
// bank_cplx_kernel (USB, LSB, CW) in its place: d[i] reads y[i] alone, the taps are [2 tp] (re, then -im); the same writes
int launch_bank(int mode, const BankPlan& p, const BankArgs& a, int ntiles, int nk, hipStream_t st) {
  if (fake_hip::tracing())
    Line("launch_bank").st(st).i("mode", mode).i("ntiles", ntiles).i("nk", nk).i("lds_floats", p.lds_floats).i("ypitch", a.ypitch).i("apitch", a.apitch)
        .i("n_out", a.n_out).i("T", a.T).i("tp", a.tp).f("fm_scale", a.fm_scale).i("noise", a.noise).i("ptiles", a.ptiles)
        .i("m0_lo", a.m0_lo).i("fword", a.fword).p("y", a.y).p("a", a.a).p("taps", a.taps).p("pmax", a.pmax).p("psum", a.psum);
  const bool cplx = mode == PYSDR_USB || mode == PYSDR_LSB || mode == PYSDR_CW;
  SAN_CHECK(mode == PYSDR_AM || mode == PYSDR_NFM || cplx, "mode %d", mode);
  SAN_CHECK(a.tp % 8 == 0 && a.tp == p.tp && a.T >= kBankTapsMin && a.T <= a.tp && a.tp - a.T < 8, "T %d tp %d", a.T, a.tp);
  SAN_CHECK(p.hpad >= a.T + 1 && p.hpad % 8 == 0 && p.hpad <= 256, "hpad %d for %d taps", p.hpad, a.T);
  SAN_CHECK(ntiles <= a.ptiles && ntiles == (a.n_out + kBankTile - 1) / kBankTile && a.n_out >= 1, "%d tiles for %d outputs, room for %d", ntiles, a.n_out, a.ptiles);
  SAN_CHECK(p.lds_floats == kBankTile + a.tp, "lds_floats %d", p.lds_floats);
  SAN_CHECK(a.apitch % 4 == 0 && a.apitch >= a.n_out && (reinterpret_cast<uintptr_t>(a.a) & 15u) == 0, "a: pitch %lld, float4 stores", a.apitch);
  const int back = mode == PYSDR_NFM ? a.T + 1 : a.T - 1;
  read_all(a.taps, (size_t)(cplx ? 2 : 1) * a.tp);
  for (int r = 0; r < nk; ++r) {
    read_all(a.y + (size_t)r * (size_t)a.ypitch - back, (size_t)back + a.n_out);
    write_all(a.a + (size_t)r * (size_t)a.apitch, (size_t)a.n_out);
    write_all(a.pmax + (size_t)r * a.ptiles, (size_t)ntiles);
    write_all(a.psum + (size_t)r * a.ptiles, (size_t)ntiles);
  }
  return PYSDR_OK;
}
// bank_finish, per row: reads pmax / psum[row ptiles + t], t < ntiles; state[row] read and written; a[row apitch + i], i < n_out
// scaled in place; y[n_out + t] -> y[t], t < hpad (y from the row's start: the last hpad samples of [history | outputs])
int launch_bank_finish(const FinishArgs& f, int nk, hipStream_t st) {
  if (fake_hip::tracing())
    Line("launch_bank_finish").st(st).i("nk", nk).i("ypitch", f.ypitch).i("apitch", f.apitch).i("n_out", f.n_out).i("hpad", f.hpad).i("ntiles", f.ntiles)
        .i("ptiles", f.ptiles).i("agc", f.agc_active).i("squelch", f.squelch).f("ref", f.ref).f("thresh", f.thresh)
        .p("ybase", f.ybase).p("a", f.a).p("pmax", f.pmax).p("psum", f.psum).p("state", f.state);
  SAN_CHECK(f.hpad >= 1 && f.hpad <= kBankThreads && f.ntiles >= 1 && f.ntiles <= f.ptiles && f.n_out >= 1, "hpad %d ntiles %d / %d", f.hpad, f.ntiles, f.ptiles);
  SAN_CHECK(f.ypitch >= (long long)f.hpad + f.n_out, "row of %lld holds %d + %d", f.ypitch, f.hpad, f.n_out);
  for (int r = 0; r < nk; ++r) {
    read_all(f.pmax + (size_t)r * f.ptiles, (size_t)f.ntiles);
    read_all(f.psum + (size_t)r * f.ptiles, (size_t)f.ntiles);
    read_all(f.state + r, 1); write_all(f.state + r, 1);
    read_all(f.a + (size_t)r * (size_t)f.apitch, (size_t)f.n_out); write_all(f.a + (size_t)r * (size_t)f.apitch, (size_t)f.n_out);
    float2* y = f.ybase + (size_t)r * (size_t)f.ypitch;
    std::memmove(y, y + f.n_out, (size_t)f.hpad * sizeof(float2));
  }
  return PYSDR_OK;
}

// ==== the channelizer's other clients and its second kind (api_cw.hip, api_psk.hip, api_fine.hip; footprints read off
// cw.hip / psk.hip / fine.hip, geometry checked with cw_plan.h / psk_plan.h / fine_plan.h) ====

// ---- CW skimmer
// cw_kernel, one lane per row < nk: reads y[row ypitch + i], i < n_out (the staging loads are guarded by r < nk and
// i < n_out); state[row] read and written; writes events[row cap + e], e < cap at the most, and counts[row]
int launch_cw_decode(const CwArgs& a, hipStream_t st) {
  if (fake_hip::tracing())
    Line("launch_cw_decode").st(st).i("ypitch", a.ypitch).i("n_out", a.n_out).i("nk", a.nk).i("cap", a.cap).i("d0", a.cfg.d0).i("n0", a.cfg.n0)
        .p("y", a.y).p("state", a.state).p("events", a.events).p("counts", a.counts);
  CwPlan p;
  SAN_CHECK(a.n_out >= 1 && cw_plan(a.nk, a.n_out, &a.cfg, &p), "no plan for nk %d and %d outputs", a.nk, a.n_out);
  SAN_CHECK(a.cap >= p.cap && a.cap == cw_event_cap((a.cap / 2 - 1) * 3), "cap %d for %d outputs (their own cap %d)", a.cap, a.n_out, p.cap);
  SAN_CHECK(a.ypitch >= p.ypitch && a.ypitch % 16 == 0, "ypitch %lld for %d outputs", a.ypitch, a.n_out);
  SAN_CHECK(cw_tiles(a.n_out) * kCwTile >= a.n_out && cw_event_index(cw_pack(a.n_out - 1, kCwWordSpace)) == a.n_out - 1, "tiles / event word");
  const float2* y = static_cast<const float2*>(a.y);
  for (int r = 0; r < a.nk; ++r) {
    read_all(y + (size_t)r * (size_t)a.ypitch, (size_t)a.n_out);
    read_all(a.state + r, 1); write_all(a.state + r, 1);
    write_all(a.events + (size_t)r * (size_t)a.cap, (size_t)a.cap);
    write_all(a.counts + r, 1);
  }
  return PYSDR_OK;
}

// ---- PSK31 skimmer
// psk_kernel<S>, NSUB = 4 S decoders per row < nk: reads y[row ypitch + i], i in [-(L - 1), n_out) -- the stub reads all
// kPskHpad >= L - 1 samples of room the plan keeps in front of a row -- tw[0, NT), g[0, L); e[S][nfine], sf[4][nfine],
// si[5][nfine] read and written; writes events[dec cap + e], e < cap at the most, and counts[dec], dec < nfine; moves the
// row's last L - 1 samples of [history | outputs] to y[-(L - 1), 0)
int launch_psk_decode(int S, const PskArgs& a, hipStream_t st) {
  if (fake_hip::tracing())
    Line("launch_psk_decode").st(st).i("S", S).i("ypitch", a.ypitch).i("n_out", a.n_out).i("nk", a.nk).i("cap", a.cap).i("nfine", a.nfine)
        .i("m0_mod", a.m0_mod).i("n0", a.cfg.n0).p("y", a.y).p("tw", a.tw).p("g", a.g).p("e", a.e).p("sf", a.sf).p("si", a.si)
        .p("events", a.events).p("counts", a.counts);
  PskPlan p;
  SAN_CHECK(a.n_out >= 1 && psk_plan(a.nk, S, a.n_out, &a.cfg, &p), "no plan for S %d, nk %d and %d outputs", S, a.nk, a.n_out);
  SAN_CHECK(a.nfine == p.nfine && a.cap >= p.cap, "nfine %d / %d, cap %d for %d outputs (their own cap %d)", a.nfine, p.nfine, a.cap, a.n_out, p.cap);
  SAN_CHECK(a.ypitch >= p.ypitch && (a.ypitch - kPskHpad) % 16 == 0, "ypitch %lld for %d outputs", a.ypitch, a.n_out);
  const int L = 2 * S, NT = 32 * S;
  SAN_CHECK(L - 1 <= kPskHpad && a.m0_mod >= 0 && a.m0_mod < NT, "m0_mod %d of %d", a.m0_mod, NT);
  SAN_CHECK(p.groups * psk_rows(S) >= a.nk && psk_event_index(psk_pack(a.n_out - 1, 2047)) == a.n_out - 1, "groups / event word");
  read_all(a.tw, (size_t)NT);
  read_all(a.g, (size_t)L);
  const size_t nf = (size_t)a.nfine;
  read_all(a.e, (size_t)S * nf); write_all(a.e, (size_t)S * nf);
  read_all(a.sf, (size_t)kPskStateFloats * nf); write_all(a.sf, (size_t)kPskStateFloats * nf);
  read_all(a.si, (size_t)kPskStateInts * nf); write_all(a.si, (size_t)kPskStateInts * nf);
  write_all(a.events, nf * (size_t)a.cap);
  write_all(a.counts, nf);
  for (int r = 0; r < a.nk; ++r) {
    PskC* y = a.y + (size_t)r * (size_t)a.ypitch;
    read_all(y - kPskHpad, (size_t)kPskHpad + a.n_out);
    std::memmove(y - (L - 1), y + a.n_out - (L - 1), (size_t)(L - 1) * sizeof(PskC));
  }
  return PYSDR_OK;
}

// ---- fine channelizer, second stage
int fine_prepare(const FinePlan& p) {
  SAN_CHECK(p.mp == (p.M2 | 1) && p.lds_bytes == p.slots * p.mp * 8 && p.lds_bytes <= 160 * 1024 && p.slots >= 1 && p.slots <= kFineSlotsMax, "LDS %d", p.lds_bytes);
  return PYSDR_OK;
}
// fine_kernel, row j < nk1 and frame fr < nframes: tap idx = p M2 + r < L2 reads rows[j pitch1 + off + fr D2 - idx], the
// lowest off - (L2 - 1) >= hist - (P2 M2 - 1) -- the stub reads every row from its start, all hist samples in front of the
// call's, to the last frame's newest sample; taps[0, L2); tw[0, M2); perm[0, Q); a0[0, nk1).
// Writes y[row pitch + fr], row = fine_row_of(a0[j], u, Mf) where that is < ng, u < Q.
int launch_fine(const FinePlan& p, const FineArgs& a, int gx, int gy, hipStream_t st) {
  if (fake_hip::tracing()) {
    Line l("launch_fine");
    l.st(st).i("gx", gx).i("gy", gy).i("lds", p.lds_bytes).i("pitch1", a.pitch1).i("hist", a.hist).i("M2", a.M2).i("D2", a.D2).i("C2", a.C2)
        .i("P2", a.P2).i("L2", a.L2).i("mp", a.mp).i("off", a.off).i("mf_lo", a.mf_lo).i("nframes", a.nframes).i("nk1", a.nk1).i("fw", a.fw)
        .i("rw", a.rw).i("fw_shift", a.fw_shift).i("Q", a.Q).i("Mf", a.Mf).i("ng", a.ng).i("pitch", a.pitch).i("npass", a.fft.npass)
        .i("magic_M2", a.magic_M2).i("magic_Q", a.magic_Q)
        .p("rows", a.rows).p("taps", a.taps).p("tw", a.tw).p("perm", a.perm).p("a0", a.a0).p("y", a.y);
    trace_passes(l, a.fft);
  }
  SAN_CHECK(a.nframes >= 1, "nframes %d", a.nframes);
  const FineTile t = fine_tile(p, a.nframes);
  SAN_CHECK(gx == t.gx && gy == t.gy && a.fw == t.fw && a.rw == t.rw && (1 << a.fw_shift) == a.fw && a.fw * a.rw == p.slots, "grid %d x %d, tile %d x %d", gx, gy, a.fw, a.rw);
  SAN_CHECK(a.M2 == p.M2 && a.D2 == p.D2 && a.C2 == p.C2 && a.mp == p.mp && a.Q == p.Q && a.Mf == p.Mf && a.ng == p.ng && a.nk1 == p.nk1 && a.hist == p.hist, "plan");
  SAN_CHECK(a.P2 >= 1 && a.P2 <= p.P2 && a.L2 > (a.P2 - 1) * a.M2 && a.L2 <= a.P2 * a.M2, "P2 %d (room for %d), L2 %d", a.P2, p.P2, a.L2);
  SAN_CHECK(a.mf_lo >= 0 && a.mf_lo < 4 && a.magic_M2 == magic_of(a.M2) && a.magic_Q == magic_of(a.Q), "mf_lo %d / magic", a.mf_lo);
  const long long last = (long long)a.off + (long long)(a.nframes - 1) * a.D2;       // the last frame's newest sample
  SAN_CHECK(a.off >= a.hist && a.off - (a.L2 - 1) >= 0 && last < a.pitch1, "window [%d, %lld] of a row of %lld", a.off - (a.L2 - 1), last, a.pitch1);
  SAN_CHECK(a.pitch >= a.nframes, "pitch %lld < %d frames", a.pitch, a.nframes);
  check_passes(a.fft, a.M2, p.npass, p.radix, a.tw, a.perm, a.Q);
  read_all(a.taps, (size_t)a.L2);
  for (int j = 0; j < a.nk1; ++j) {
    read_all(a.rows + 2 * (size_t)j * (size_t)a.pitch1, 2 * (size_t)(last + 1));
    SAN_CHECK(a.a0[j] == fine_a0(p, j), "a0[%d] = %d", j, a.a0[j]);
    for (int u = 0; u < a.Q; ++u) {
      const int row = fine_row_of(a.a0[j], u, a.Mf);
      if (row < a.ng) write_all(a.y + 2 * (size_t)row * (size_t)a.pitch, 2 * (size_t)a.nframes);
    }
  }
  return PYSDR_OK;
}
// fine_roll, one workgroup per row < nk1: rows[j pitch1 + e] = rows[j pitch1 + e + n1], e < hist (all reads first)
int launch_fine_roll(float* rows, long long pitch1, int hist, int n1, int nk1, hipStream_t st) {
  if (fake_hip::tracing()) Line("launch_fine_roll").st(st).i("pitch1", pitch1).i("hist", hist).i("n1", n1).i("nk1", nk1).p("rows", rows);
  SAN_CHECK(n1 >= 1 && hist >= 1 && hist <= kFineRollThreads * kFineRollPer && fine_roll_elem(kFineRollThreads - 1, kFineRollPer - 1) + 1 >= hist, "hist %d n1 %d", hist, n1);
  SAN_CHECK(pitch1 >= (long long)hist + n1, "row of %lld holds %d + %d", pitch1, hist, n1);
  for (int j = 0; j < nk1; ++j) {
    float* row = rows + 2 * (size_t)j * (size_t)pitch1;
    std::memmove(row, row + 2 * (size_t)n1, (size_t)hist * 2 * sizeof(float));
  }
  return PYSDR_OK;
}

}  // namespace pysdr
