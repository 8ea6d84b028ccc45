// The CW skimmer's plan, staging geometry and event slots (pysdr_amd/csrc/cw_plan.h, the very code cw.hip steps with) on
// the CPU under AddressSanitizer + UBSan.
//   * pysdr-side rules: every nk in 1 .. 4096 with max_out in {1, 2, 3, T - 1, T, T + 1, 1024} plans; the groups tile
//     [0, nk), the row pitch holds max_out, the event cap is 2 (max_out / 3 + 1); bad shapes and bad settings are refused.
//   * the tile walk of the kernel: every staging load goes to a Y of exactly nk x pitch elements and an LDS tile of exactly
//     rows x stride elements (heap: the sanitizer guards both ends), the 32 lanes of a half-wave read one column from 32
//     different bank pairs, and every (row, sample) is consumed exactly once, in order.  The last, partial group and the
//     first are walked for every nk, all groups for nk <= 256 and nk > 4032 (calls of 1024 outputs: nk <= 130, 4096 and
//     every 61st in between): a middle group runs the same code on 64 whole rows at another row0.
//   * the event slots: steps 7 and 8 (cw_step_key) driven by EVERY key sequence of up to 15 samples at the shortest dot,
//     from every kind of start state, and by the densest periodic sequences over 1024 samples, storing into exactly `cap`
//     slots as the kernel does: the count never exceeds the cap, and the densest sequence comes within a factor of two.
//   * the event word round-trips.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cw_plan.h"

using namespace pysdr;

#define REQUIRE(c, ...) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static pysdr_cw_cfg good_cfg() {
  pysdr_cw_cfg c{};
  c.a_s = 0.5333333f; c.a_p = 0.0017777778f; c.a_n = 0.010666667f; c.snr_min = 16.f; c.hi = 2.f; c.lo = 0.5f; c.fl = 1.f / 64;
  c.d0 = 360; c.dmin = 120; c.dmax = 1440; c.n0 = 24;
  return c;
}

static long walk_group(int nk, int n_out, const CwPlan& p, int g, std::vector<int>& seen_y) {
  const int row0 = g * kCwRows;
  std::vector<long> tile((size_t)kCwRows * kCwStride);          // what the LDS holds: the Y index, or -1
  long steps = 0;
  std::vector<int> next((size_t)kCwRows, 0);                     // next sample every lane expects
  for (int i0 = 0; i0 < n_out; i0 += kCwTile) {
    std::fill(tile.begin(), tile.end(), -2L);
    for (int it = 0; it < kCwLoads; ++it)
      for (int lane = 0; lane < kCwThreads; ++lane) {
        const int rr = cw_stage_row(it, lane), cc = cw_stage_col(it, lane);
        REQUIRE(rr >= 0 && rr < kCwRows && cc >= 0 && cc < kCwTile, "load %d lane %d -> (%d, %d)", it, lane, rr, cc);
        if (lane > 0 && lane % kCwTile) REQUIRE(cw_stage_row(it, lane - 1) == rr && cw_stage_col(it, lane - 1) == cc - 1, "lanes not along the row");
        const int r = row0 + rr, i = i0 + cc;
        long v = -1;
        if (r < nk && i < n_out) {
          v = (long)r * p.ypitch + i;
          seen_y.data()[v] += 1;                                 // the global load
        }
        long& slot = tile.data()[(size_t)rr * kCwStride + cc];
        REQUIRE(slot == -2, "LDS slot (%d, %d) written twice in a tile", rr, cc);
        slot = v;
      }
    const int nj = n_out - i0 < kCwTile ? n_out - i0 : kCwTile;
    for (int j = 0; j < nj; ++j) {
      unsigned long long banks[2] = {0, 0};
      for (int lane = 0; lane < kCwThreads; ++lane) {
        const size_t at = (size_t)lane * kCwStride + j;
        const int pair = (int)(at % 32);                         // 8-byte elements over 64 banks of 4 bytes
        REQUIRE(!(banks[lane / 32] >> pair & 1), "lanes of a half-wave share a bank pair at column %d", j);
        banks[lane / 32] |= 1ull << pair;
        const long v = tile.data()[at];
        if (row0 + lane < nk) {
          REQUIRE(v == (long)(row0 + lane) * p.ypitch + i0 + j, "lane %d column %d reads %ld", lane, j, v);
          REQUIRE(next[(size_t)lane] == i0 + j, "lane %d out of order", lane);
          next[(size_t)lane] += 1;
          ++steps;
        } else {
          REQUIRE(v == -1, "a lane without a row reads memory");
        }
      }
    }
  }
  REQUIRE(cw_tiles(n_out) == (n_out + kCwTile - 1) / kCwTile, "tiles");
  for (int lane = 0; lane < kCwRows; ++lane)
    if (row0 + lane < nk) REQUIRE(next[(size_t)lane] == n_out, "lane %d walked %d of %d", lane, next[(size_t)lane], n_out);
  return steps;
}

static int drive(const pysdr_cw_cfg& c, CwState z, const std::vector<int>& keys, int cap, int* first_gap = nullptr) {
  std::vector<int32_t> slots((size_t)cap);                       // exactly the channel's slots
  int cnt = 0, last = -1000;
  for (size_t i = 0; i < keys.size(); ++i) {
    const int e = cw_step_key(z, c, keys[i]);
    if (e >= 0) {
      REQUIRE(cnt < cap, "event %d of a call of %zu outputs does not fit %d slots", cnt + 1, keys.size(), cap);
      slots.data()[cnt++] = cw_pack((int)i, e);
      REQUIRE(e <= kCwWordSpace, "code %d", e);
      if (e != kCwWordSpace) { if (first_gap && last >= 0 && (int)i - last < *first_gap) *first_gap = (int)i - last; last = (int)i; }
    }
    REQUIRE(z.run >= 1 && z.run <= kCwRunMax && z.dot >= c.dmin && z.dot <= c.dmax && z.code >= 0 && z.code <= 255 && z.nel >= 0 && z.nel <= 7,
            "state left its range: run %d dot %d code %d nel %d", z.run, z.dot, z.code, z.nel);
  }
  for (int k = 0; k < cnt; ++k) REQUIRE(cw_event_index(slots[(size_t)k]) < (int)keys.size(), "index");
  return cnt;
}

int main() {
  const pysdr_cw_cfg cfg = good_cfg();
  CwPlan p;
  // ---- refusals
  REQUIRE(!cw_plan(0, 16, &cfg, &p) && !cw_plan(4097, 16, &cfg, &p) && !cw_plan(-1, 16, &cfg, &p), "nk");
  REQUIRE(!cw_plan(64, 0, &cfg, &p) && !cw_plan(64, -5, &cfg, &p) && !cw_plan(64, kCwMaxOutMax + 1, &cfg, &p) && cw_plan(64, kCwMaxOutMax, &cfg, &p), "max_out");
  REQUIRE(!cw_plan(64, 16, nullptr, &p), "NULL cfg");
  {
    const float nan = __builtin_nanf(""), inf = __builtin_inff();
    float pysdr_cw_cfg::* const fl[] = {&pysdr_cw_cfg::a_s, &pysdr_cw_cfg::a_p, &pysdr_cw_cfg::a_n, &pysdr_cw_cfg::snr_min, &pysdr_cw_cfg::hi, &pysdr_cw_cfg::lo, &pysdr_cw_cfg::fl};
    for (size_t k = 0; k < sizeof fl / sizeof fl[0]; ++k)
      for (float v : {0.f, -1.f, nan, inf}) { pysdr_cw_cfg b = cfg; b.*fl[k] = v; REQUIRE(!cw_plan(64, 16, &b, &p), "float field %zu = %g accepted", k, (double)v); }
    for (int k = 0; k < 3; ++k) { pysdr_cw_cfg b = cfg; b.*fl[k] = 1.0000001f; REQUIRE(!cw_plan(64, 16, &b, &p), "a > 1"); b.*fl[k] = 1.f; REQUIRE(cw_plan(64, 16, &b, &p), "a = 1"); }
    pysdr_cw_cfg b = cfg; b.lo = 3.f; REQUIRE(!cw_plan(64, 16, &b, &p), "lo > hi");
    b = cfg; b.dmin = 15; REQUIRE(!cw_plan(64, 16, &b, &p), "dmin 15");
    b = cfg; b.dmin = 16; b.d0 = 16; REQUIRE(cw_plan(64, 16, &b, &p), "dmin = d0 = 16");
    b = cfg; b.d0 = b.dmin - 1; REQUIRE(!cw_plan(64, 16, &b, &p), "d0 < dmin");
    b = cfg; b.d0 = b.dmax + 1; REQUIRE(!cw_plan(64, 16, &b, &p), "d0 > dmax");
    b = cfg; b.dmax = kCwDotMax + 1; REQUIRE(!cw_plan(64, 16, &b, &p), "dmax"); b.dmax = kCwDotMax; REQUIRE(cw_plan(64, 16, &b, &p), "dmax = 2^22");
    b = cfg; b.n0 = 0; REQUIRE(!cw_plan(64, 16, &b, &p), "n0 0"); b.n0 = kCwSettleMax + 1; REQUIRE(!cw_plan(64, 16, &b, &p), "n0"); b.n0 = 1; REQUIRE(cw_plan(64, 16, &b, &p), "n0 1");
  }
  // ---- plans and tile walks
  const int outs[7] = {1, 2, 3, kCwTile - 1, kCwTile, kCwTile + 1, 1024};
  long plans = 0, steps = 0;
  for (int nk = 1; nk <= kCwNkMax; ++nk)
    for (int oi = 0; oi < 7; ++oi) {
      const int mo = outs[oi];
      REQUIRE(cw_plan(nk, mo, &cfg, &p), "nk %d max_out %d refused", nk, mo);
      REQUIRE(p.cap == 2 * (mo / 3 + 1) && p.cap >= 2 && p.ypitch >= mo && p.ypitch % 16 == 0 && p.ypitch < mo + 16, "nk %d max_out %d: cap %d pitch %d", nk, mo, p.cap, p.ypitch);
      REQUIRE(p.groups * kCwRows >= nk && (p.groups - 1) * kCwRows < nk, "nk %d: %d groups", nk, p.groups);
      ++plans;
      const bool all = mo == 1024 ? (nk <= 130 || nk == kCwNkMax) : (nk <= 256 || nk > kCwNkMax - 64);
      if (mo == 1024 && !all && nk % 61) continue;                 // the long calls: every 61st shape beyond two groups
      std::vector<int> seen_y((size_t)nk * p.ypitch, 0);
      for (int g = 0; g < p.groups; ++g)
        if (all || g == 0 || g == p.groups - 1) steps += walk_group(nk, mo, p, g, seen_y);
      for (int r = 0; r < nk; ++r) {
        const int g = r / kCwRows;
        const int want = (all || g == 0 || g == p.groups - 1) ? 1 : 0;
        if (!want && r % kCwRows != 0 && r % kCwRows != kCwRows - 1) continue;     // of an unwalked group: the rows next to a walked one
        for (int i = 0; i < p.ypitch; ++i)
          REQUIRE(seen_y[(size_t)r * p.ypitch + i] == (i < mo ? want : 0), "nk %d max_out %d: (%d, %d) loaded %d x", nk, mo, r, i, seen_y[(size_t)r * p.ypitch + i]);
      }
    }
  REQUIRE(kCwLdsBytes == kCwRows * kCwStride * 8 && kCwStride % 2 == 1 && kCwLoads * kCwThreads == kCwRows * kCwTile, "geometry");
  // ---- event slots
  pysdr_cw_cfg tight = cfg;
  tight.dmin = tight.d0 = kCwDotMin; tight.dmax = 64;
  std::vector<CwState> starts;
  {
    CwState z = cw_state_init(tight);
    starts.push_back(z);
    z.sp = 1; z.run = 4; starts.push_back(z);                      // a word space is due with the next key-up sample
    z.sp = 0; z.key = 1; z.run = 3; starts.push_back(z);           // inside a mark
    z.key = 0; z.run = 1; z.code = 5; z.nel = 2; z.last = 1; starts.push_back(z);   // a character is due
    z.sp = 1; z.run = kCwRunMax; z.code = 0; z.nel = 7; starts.push_back(z);
    z = cw_state_init(tight); z.key = 1; z.run = kCwRunMax; z.last = kCwRunMax; z.code = 255; z.nel = 7; starts.push_back(z);
  }
  long seqs = 0;
  int gap = 1 << 30;
  for (int n = 1; n <= 15; ++n) {
    const int cap = cw_event_cap(n);
    std::vector<int> keys((size_t)n);
    for (unsigned bits = 0; bits < (1u << n); ++bits) {
      for (int i = 0; i < n; ++i) keys[(size_t)i] = (bits >> i) & 1;
      for (const CwState& z : starts) { drive(tight, z, keys, cap, &gap); ++seqs; }
    }
  }
  REQUIRE(gap == 3, "two character events %d samples apart", gap);
  int densest = 0;
  for (int period = 2; period <= 9; ++period)
    for (int down = 1; down < period; ++down)
      for (int phase = 0; phase < period; ++phase) {
        std::vector<int> keys(1024);
        for (int i = 0; i < 1024; ++i) keys[(size_t)i] = ((i + phase) % period) < down ? 1 : 0;
        for (const CwState& z : starts) { const int c = drive(tight, z, keys, cw_event_cap(1024)); densest = c > densest ? c : densest; ++seqs; }
      }
  REQUIRE(2 * densest >= cw_event_cap(1024) - 4 && densest <= cw_event_cap(1024), "densest %d of cap %d", densest, cw_event_cap(1024));
  // ---- the event word
  for (int i : {0, 1, 511, 512, 1023, kCwMaxOutMax - 1})
    for (int c = 0; c <= kCwWordSpace; ++c) {
      const int32_t w = cw_pack(i, c);
      REQUIRE(w >= 0 && cw_event_index(w) == i && cw_event_code(w) == c, "word (%d, %d)", i, c);
    }
  REQUIRE(sizeof(CwState) == 48 && sizeof(pysdr_cw_cfg) == 44, "layouts %zu %zu", sizeof(CwState), sizeof(pysdr_cw_cfg));
  printf("cw plan: %ld plans, %ld samples walked, %ld key sequences, densest call of 1024 outputs %d events of %d slots\nCW_PLAN_OK\n",
         plans, steps, seqs, densest, cw_event_cap(1024));
  return 0;
}
