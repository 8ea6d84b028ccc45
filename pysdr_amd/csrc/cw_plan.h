// The CW skimmer's pure half: settings and their rules, the event cap, the staging tile's geometry,
// the event word, and the per-sample step itself -- the very code the kernel (cw.hip) steps with, the host half
// (api_cw.hip) plans with and tests/cw_plan/plan_main.cpp walks on the CPU.  Plain C++: nothing here calls the HIP
// runtime, and the only trace of the device is the function qualifier below.
#pragma once

#include <cfloat>
#include <cstdint>

#include "../../include/pysdr_hip.h"

#if defined(__HIPCC__)
#define PYSDR_CW_HD __host__ __device__
#else
#define PYSDR_CW_HD
#endif

namespace pysdr {

constexpr int kCwRows = 64;               // rows per workgroup: one lane per channel, one wave per workgroup
constexpr int kCwThreads = 64;
constexpr int kCwTile = 32;               // samples of every row staged at once: 256-byte row segments
constexpr int kCwStride = kCwTile + 1;    // LDS row stride in complex samples, odd: the 32 lanes of a half-wave read one
                                          // column from 32 different pairs of banks
constexpr int kCwLdsBytes = kCwRows * kCwStride * 8;
constexpr int kCwLoads = kCwRows * kCwTile / kCwThreads;   // staging loads per lane and tile
constexpr int kCwNkMax = 4096;
constexpr int kCwMaxOutMax = 1 << 21;     // the event word holds the index within the call above bit 9
constexpr int kCwDotMax = 1 << 22;        // dot lengths, 1/16 sample
constexpr int kCwDotMin = 16;             // 2 dot >= 32: two character events are at least 3 samples apart
constexpr int kCwRunMax = 1 << 24;
constexpr int kCwSettleMax = 1 << 22;     // settling samples n0
constexpr int kCwWordSpace = 256;

inline bool cw_cfg_ok(const pysdr_cw_cfg& c) {
  const float a[3] = {c.a_s, c.a_p, c.a_n};
  for (float v : a)
    if (!(v > 0.f && v <= 1.f)) return false;
  const float g[4] = {c.snr_min, c.hi, c.lo, c.fl};
  for (float v : g)
    if (!(v > 0.f && v <= FLT_MAX)) return false;
  if (!(c.lo <= c.hi)) return false;
  if (c.n0 < 1 || c.n0 > kCwSettleMax) return false;
  return c.dmin >= kCwDotMin && c.dmin <= c.d0 && c.d0 <= c.dmax && c.dmax <= kCwDotMax;
}

// most events one channel can emit in a call of max_out outputs: a character event every third sample, each followed by
// its own word space
constexpr int cw_event_cap(int max_out) { return 2 * (max_out / 3 + 1); }

struct CwPlan {
  int cap = 0;         // event slots per channel
  int groups = 0;      // workgroups
  int ypitch = 0;      // row pitch of Y, complex samples
};

inline bool cw_plan(int nk, int max_out, const pysdr_cw_cfg* cfg, CwPlan* p) {
  if (nk < 1 || nk > kCwNkMax || max_out < 1 || max_out > kCwMaxOutMax || !cfg || !cw_cfg_ok(*cfg)) return false;
  CwPlan q;
  q.cap = cw_event_cap(max_out);
  q.groups = (nk + kCwRows - 1) / kCwRows;
  q.ypitch = (max_out + 15) & ~15;
  *p = q;
  return true;
}

// the event word: (index within the call) << 9 | c, c = the character's code 0 .. 255 or 256 = word space
PYSDR_CW_HD constexpr int32_t cw_pack(int i, int c) { return (int32_t)(((uint32_t)i << 9) | (uint32_t)c); }
PYSDR_CW_HD constexpr int cw_event_index(int32_t w) { return (int)((uint32_t)w >> 9); }
PYSDR_CW_HD constexpr int cw_event_code(int32_t w) { return (int)((uint32_t)w & 511u); }

// staging load `it` < kCwLoads of lane `lane`: which (row of the group, sample of the tile) it brings.  Consecutive lanes
// take consecutive samples of a row; a wave's load covers 64 / kCwTile rows.
PYSDR_CW_HD constexpr int cw_stage_row(int it, int lane) { return (it * kCwThreads + lane) / kCwTile; }
PYSDR_CW_HD constexpr int cw_stage_col(int it, int lane) { return (it * kCwThreads + lane) % kCwTile; }
constexpr int cw_tiles(int n_out) { return (n_out + kCwTile - 1) / kCwTile; }

struct CwState {         // one per channel, in device memory
  float s, pk, nf;
  int32_t key, run, dot, last, code, nel, sp, seen;
  int32_t pad;
};

PYSDR_CW_HD inline CwState cw_state_init(const pysdr_cw_cfg& c) {
  CwState z{};
  z.dot = c.d0;
  z.code = 1;
  return z;
}

// Steps 7 and 8 of the definition, all integer: the key decision `neu` of this sample ends or continues a run, a mark that
// ends moves the dot length and appends an element, and a key-up run that has lasted long enough emits.  Returns -1, or
// the code of the event this sample emits (0 .. 255, kCwWordSpace).
PYSDR_CW_HD inline int cw_step_key(CwState& z, const pysdr_cw_cfg& c, int neu) {
  if (neu != z.key) {
    if (z.key == 1) {
      const int32_t L = z.run;
      if (z.last > 0 && (L >= 2 * z.last || z.last >= 2 * L)) {
        z.dot += (4 * (z.last + L) - z.dot) >> 1;          // floor
        z.dot = z.dot < c.dmin ? c.dmin : (z.dot > c.dmax ? c.dmax : z.dot);
      }
      z.last = L;
      const int dash = (16 * L >= 2 * z.dot) ? 1 : 0;
      if (z.code != 0) {
        if (z.nel >= 7) z.code = 0;
        else { z.code = 2 * z.code + dash; z.nel += 1; }
      }
    }
    z.key = neu;
    z.run = 1;
  } else {
    z.run = z.run + 1 < kCwRunMax ? z.run + 1 : kCwRunMax;
  }
  if (z.key == 0) {
    if (z.code != 1 && 16 * z.run >= 2 * z.dot) {
      const int e = z.code;
      z.code = 1; z.nel = 0; z.sp = 1;
      return e;
    }
    if (z.sp && 16 * z.run >= 5 * z.dot) { z.sp = 0; return kCwWordSpace; }
  }
  return -1;
}

// Steps 1 to 8 of the definition for one sample (re, im); every float operation rounds on its own (the build's
// -ffp-contract=off).  Returns what cw_step_key returns.
PYSDR_CW_HD inline int cw_step(CwState& z, const pysdr_cw_cfg& c, float re, float im) {
  float p = re * re + im * im;
  if (!(p <= FLT_MAX)) p = z.s;
  z.s = z.s + c.a_s * (p - z.s);
  const bool settling = z.seen < c.n0;                      // the first n0 samples: the floor is the peak, the key stays up
  if (settling) z.seen += 1;
  if (z.s > z.pk) z.pk = z.s;
  else z.pk = z.pk + c.a_p * (z.s - z.pk);
  if (settling) z.nf = z.pk;
  const float A = z.nf * z.pk, B = (z.pk * z.pk) * c.fl;
  const float q = A > B ? A : B;
  const float u = z.s * z.s;
  const bool pres = z.pk > c.snr_min * z.nf;
  const int neu = (!settling && pres && (z.key ? u >= q * c.lo : u > q * c.hi)) ? 1 : 0;
  if (!neu && !settling) {
    const float lim = 4.0f * z.nf + 1e-30f;
    const float cl = z.s < lim ? z.s : lim;
    z.nf = z.nf + c.a_n * (cl - z.nf);
  }
  return cw_step_key(z, c, neu);
}

// ---- kernel arguments and the launch (cw.hip; tests may stub it) ---------------------------------------------------
struct CwArgs {
  const void* y;           // complex64 Y[nk][ypitch]: y[a * ypitch + i] = output i of this call
  long long ypitch;
  int n_out, nk, cap;
  pysdr_cw_cfg cfg;
  CwState* state;          // [nk]
  int32_t* events;         // [nk][cap]
  int32_t* counts;         // [nk]
};

}  // namespace pysdr
