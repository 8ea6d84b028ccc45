// The pure half of the second pass (pysdr_amd/csrc/pass_plan.h) walked on the CPU, a stand-alone program
// that tests/test_pass_plan.py builds and runs through tests/plan_program.py: the rows of a frame at every fine row of both
// modes' shapes, on open and circular rasters (printed, for the test to hold against the NumPy model); the phase word; the
// depth rules of both rings against a brute-force simulation of call sizes -- at the end of the first call that makes a
// frame due, every step and every sample a subtraction and a rescan around it may touch is complete and still held; the
// rules of a frame, a trial and a rescan window at their edges; the settings' rules.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pass_plan.h"

using namespace pysdr;

static int g_fail = 0;
#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++g_fail; } \
  } while (0)

template <class Mode>
static void rows_of(int mode, int S) {
  for (int nk : {1, 3, 4})
    for (int circular = 0; circular < 2; ++circular)
      for (int F = 0; F < nk * (S / 2); ++F) {
        const PassRows r = pass_rows<Mode>(F, S, nk, circular != 0);
        CHECK(r.n >= 1 && r.n <= kPassRowJobs && r.row[0] == F / (S / 2));
        for (int i = 0; i < r.n; ++i) CHECK(r.row[i] >= 0 && r.row[i] < nk);
        std::printf("ROWS %d %d %d %d %d %d", mode, S, nk, circular, F, r.n);
        for (int i = 0; i < r.n; ++i) std::printf(" %d %d %u", r.row[i], r.q[i], pass_word(r.q[i], S));
        std::printf("\n");
      }
}

// every call size from 1 to max_out held fixed, and a pseudo-random mixture: the frames that become due at a call's end
template <class Mode>
static long long depths(int S, int max_out, int reach_t) {
  const int qs = S / 4, tr2 = pass_ring_steps<Mode>(max_out, S, reach_t), ty = pass_ring_samples(tr2, S);
  const int hold = kFtHold<Mode>, lag = kFtLag<Mode>;
  CHECK(ty >= qs * tr2 + S && ty % 16 == 0 && max_out < ty);
  long long checked = 0;
  unsigned rnd = 12345u;
  for (int fixed = 0; fixed <= max_out; ++fixed) {                     // 0: the mixture
    long long n_abs = 0, done = 0, next_due = 0;                       // frames t0 < next_due have been due
    while (done < 3LL * tr2 + 50) {
      int n = fixed;
      if (!fixed) { rnd = rnd * 1664525u + 1013904223u; n = 1 + (int)((rnd >> 8) % (unsigned)max_out); }
      n_abs += n;
      done = (long long)ft_steps_done((unsigned long long)n_abs, S);
      for (; next_due + hold + reach_t <= done; ++next_due) {
        const long long t0 = next_due, first = pass_first_step(done, tr2), n_lo = n_abs > ty ? n_abs - ty : 0;
        const long long oldest = t0 - reach_t - kPassMargin < 0 ? 0 : t0 - reach_t - kPassMargin;
        CHECK(oldest >= first);                                        // still held in ring2 ...
        CHECK((long long)qs * oldest >= n_lo);                         // ... and in yk
        CHECK(t0 + reach_t + lag + kPassMargin < done);                // complete
        CHECK(pass_frame_ok<Mode>(t0, done, tr2));
        CHECK(pass_window_ok<Mode>(t0 - reach_t < 0 ? 0 : t0 - reach_t, t0 + reach_t, done, tr2));
        ++checked;
      }
    }
  }
  return checked;
}

template <class Mode>
static void edges(int S) {
  const int lag = kFtLag<Mode>, tr2 = 400 + lag;
  const long long done = 1000 + lag;
  // steps t0 - 4 .. t0 + lag + 4 complete and held: t0 from done - tr2 + 4 to done - lag - 5
  CHECK(pass_frame_ok<Mode>(done - tr2 + 4, done, tr2) && !pass_frame_ok<Mode>(done - tr2 + 3, done, tr2));
  CHECK(pass_frame_ok<Mode>(done - lag - 5, done, tr2) && !pass_frame_ok<Mode>(done - lag - 4, done, tr2));
  CHECK(!pass_frame_ok<Mode>(-1, done, tr2) && pass_frame_ok<Mode>(0, lag + 5, tr2) && !pass_frame_ok<Mode>(0, lag + 4, tr2));
  CHECK(pass_frame_ok<Mode>(2, lag + 7, tr2));                         // the steps before the stream's start are nobody's
  CHECK(pass_dn_ok(S / 4 - 1, S) && pass_dn_ok(-(S / 4 - 1), S) && !pass_dn_ok(S / 4, S) && !pass_dn_ok(-(S / 4), S));
  CHECK(pass_window_arg_ok<Mode>(0, 0) && pass_window_arg_ok<Mode>(5, 5 + kPassWindowMax - 9) && !pass_window_arg_ok<Mode>(5, 5 + kPassWindowMax - 8));
  CHECK(!pass_window_arg_ok<Mode>(-1, 3) && !pass_window_arg_ok<Mode>(4, 3));
  CHECK(pass_window_ok<Mode>(done - tr2 + 4, done - lag - 5, done, tr2) && !pass_window_ok<Mode>(done - tr2 + 3, done - lag - 5, done, tr2));
  CHECK(!pass_window_ok<Mode>(done - tr2 + 4, done - lag - 4, done, tr2) && pass_window_ok<Mode>(0, 3, lag + 8, tr2));
  PassPlan p;
  CHECK(pass_plan<Mode>(3, S, 64, 40, &p) && p.tr2 == pass_ring_steps<Mode>(64, S, 40) && p.ty == pass_ring_samples(p.tr2, S));
  CHECK(!pass_plan<Mode>(0, S, 64, 40, &p) && !pass_plan<Mode>(3, S + 1, 64, 40, &p) && !pass_plan<Mode>(3, S, 0, 40, &p));
  CHECK(!pass_plan<Mode>(3, S, 64, 0, &p) && !pass_plan<Mode>(3, S, 64, kPassReachMax + 1, &p) && pass_plan<Mode>(3, S, 64, kPassReachMax, &p));
  CHECK(!pass_plan<Mode>(3, S, 64, 40, nullptr) && !pass_plan<Mode>(kFtFineMax / (S / 2), S, kFtMaxOutMax, 40, &p));   // a ring above 2^30 bytes
}

int main() {
  rows_of<Ft8Mode>(0, 64); rows_of<Ft8Mode>(0, 96); rows_of<Ft4Mode>(1, 48); rows_of<Ft4Mode>(1, 72);
  // the phase word: q quarter-bauds are q / (4 S) turns per row sample, rounded half up
  CHECK(pass_word(0, 64) == 0u && pass_word(2, 64) == (1u << 25) && pass_word(-2, 64) == 0u - (1u << 25) && pass_word(4 * 96, 96) == 0u);
  CHECK(pass_word(1, 96) == 11184811u && pass_word(-1, 96) == 0u - 11184811u + 0u && pass_word(3, 48) == 67108864u);
  CHECK(pass_lut_index(0u) == 0 && pass_lut_index((1u << 19) - 1u) == 0 && pass_lut_index(1u << 19) == 1 && pass_lut_index(0xFFFFFFFFu) == 0 &&
        pass_lut_index(0xFFF80000u - 1u) == kPassLut - 1);
  long long n = 0;
  for (int reach : {1, 16, 40, kPassReachMax}) {
    n += depths<Ft8Mode>(64, 64, reach) + depths<Ft8Mode>(96, 7, reach) + depths<Ft4Mode>(48, 256, reach) + depths<Ft4Mode>(72, 100, reach);
  }
  edges<Ft8Mode>(64); edges<Ft8Mode>(96); edges<Ft4Mode>(48); edges<Ft4Mode>(72);
  uint32_t pulse[1] = {0};
  float lut[2] = {1.f, 0.f};
  PassCfg c{40, 9, pulse, lut};
  CHECK(pass_cfg_ok(&c) && !pass_cfg_ok(nullptr));
  c.reach_t = 0; CHECK(!pass_cfg_ok(&c)); c.reach_t = kPassReachMax + 1; CHECK(!pass_cfg_ok(&c)); c.reach_t = 1;
  c.trials = 0; CHECK(!pass_cfg_ok(&c)); c.trials = kPassTrials + 1; CHECK(!pass_cfg_ok(&c)); c.trials = 1; CHECK(pass_cfg_ok(&c));
  c.pulse = nullptr; CHECK(!pass_cfg_ok(&c)); c.pulse = pulse; c.lut = nullptr; CHECK(!pass_cfg_ok(&c));
  static_assert(kPassEventCap == 52 && kPassJobWords == 30 && kPassTiles<Ft8Mode> == 81 && kPassTiles<Ft4Mode> == 105, "the plan's numbers");
  if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
  std::printf("PASS_PLAN_OK %lld due frames\n", n);
  return 0;
}
