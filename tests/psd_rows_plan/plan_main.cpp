// The grid of the rows loop of the 64k PSD (pysdr_amd/csrc/host_plan.h plan_psd_rows) and the walk of its workgroups over
// the frames of a launch (psd_rows_geom.h PsdRowsWalk, the very code the kernel steps with), on the CPU under
// AddressSanitizer + UBSan: for nframes 1 ... 1000, for CU counts 1, 8, 256 and 304 and every grid the plan can return for
// them -- the default and every forced R from 1 to past the residency -- each of the 8 R workgroups' sequences is walked
// with a "load" of every (frame, row block) the kernel would load (the first frame in front of the loop, the next one
// inside it) into a table of exactly nframes x 8 entries, so that a frame index >= nframes is refused by the walk's own
// check and, without it, would be an out-of-bounds write the sanitizer reports.
//   every (frame, row block) is loaded exactly once and transformed exactly once, no index >= nframes is touched,
//   no workgroup has more than one frame more than another, the default's 8 R workgroups are resident at once.
// Built with -DPSD_ROWS_SEED_DEFECT the walk steps with `<=` for `<` in has_next -- the kernel's off-by-one that would read a
// frame the launch does not have -- and the program must FAIL (tests/test_psd_rows_plan.py runs both).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host_plan.h"
#include "psd_rows_geom.h"

using namespace pysdr;

#define REQUIRE(c, ...) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

#ifdef PSD_ROWS_SEED_DEFECT
struct Walk : PsdRowsWalk {
  using PsdRowsWalk::PsdRowsWalk;
  bool has_next() const { return fn <= nframes; }
};
#else
typedef PsdRowsWalk Walk;
#endif

// (the 8 row blocks of a grid row step alike: one walk per grid row, every step applied to the cells of all 8 workgroups)
static long walk(int nframes, int R) {
  REQUIRE(R >= 1 && R <= nframes, "R %d nframes %d", R, nframes);
  const size_t cells = (size_t)nframes * kPsdRowBlocks;
  std::vector<unsigned char> loaded(cells, 0), done(cells, 0);           // heap: the sanitizer guards both ends
  int lo = nframes, hi = 0;
  long steps = 0;
  for (int r = 0; r < R; ++r) {
    Walk fr(r, R, nframes);
    int mine = 0;
    REQUIRE(fr.f >= 0 && fr.f < nframes, "first frame %d of %d (R %d)", fr.f, nframes, R);
    for (int rb = 0; rb < kPsdRowBlocks; ++rb) loaded.data()[(size_t)fr.f * kPsdRowBlocks + rb] += 1;   // the prologue's load of the first frame
    for (;;) {
      if (fr.has_next()) {                                               // the prefetch: intermediate and block scales
        REQUIRE(fr.fn >= 0 && fr.fn < nframes, "prefetch of frame %d of %d (R %d, workgroup %d)", fr.fn, nframes, R, r);
        for (int rb = 0; rb < kPsdRowBlocks; ++rb) loaded.data()[(size_t)fr.fn * kPsdRowBlocks + rb] += 1;
      }
      for (int rb = 0; rb < kPsdRowBlocks; ++rb) {
        REQUIRE(loaded.data()[(size_t)fr.f * kPsdRowBlocks + rb] == 1, "frame %d block %d transformed without its data (nframes %d R %d)", fr.f, rb, nframes, R);
        done.data()[(size_t)fr.f * kPsdRowBlocks + rb] += 1;
      }
      ++mine; steps += kPsdRowBlocks;
      if (!fr.has_next()) break;
      fr.advance();
    }
    lo = std::min(lo, mine); hi = std::max(hi, mine);
  }
  for (size_t c = 0; c < cells; ++c)
    REQUIRE(loaded[c] == 1 && done[c] == 1, "frame %zu block %zu of %d at R %d: loaded %d x, transformed %d x", c / kPsdRowBlocks, c % kPsdRowBlocks, nframes, R, (int)loaded[c], (int)done[c]);
  REQUIRE(hi - lo <= 1, "nframes %d R %d: %d .. %d frames per workgroup", nframes, R, lo, hi);
  return steps;
}

int main() {
  long plans = 0, steps = 0;
  const int cus[4] = {1, 8, 256, 304};
  for (int ci = 0; ci < 4; ++ci) {
    const int residency = cus[ci] * kPsdRowsWgPerCu;                     // workgroups of 72 KB of LDS a device holds at once
    const int rmax = psd_rows_max_r(cus[ci]);
    REQUIRE(rmax >= 1 && (kPsdRowBlocks * rmax <= residency || rmax == 1), "cus %d rmax %d", cus[ci], rmax);
    const int walked_to = ci ? psd_rows_max_r(cus[ci - 1]) + 3 : 0;        // (the CU counts ascend)
    for (int nframes = 1; nframes <= 1000; ++nframes) {
      const int R = plan_psd_rows(nframes, cus[ci], -1);
      REQUIRE(R >= 1 && R <= rmax && R <= nframes, "cus %d nframes %d R %d", cus[ci], nframes, R);
      // 8 R <= 2 CUs (a device of fewer than 4 CUs cannot hold one frame's 8 workgroups: there R = 1 is all there is)
      REQUIRE(kPsdRowBlocks * R <= residency || R == 1, "cus %d nframes %d: %d workgroups, %d resident", cus[ci], nframes, kPsdRowBlocks * R, residency);
      // the fewest rounds, and no smaller R has as few
      const int rounds = (nframes + rmax - 1) / rmax;
      REQUIRE((nframes + R - 1) / R == rounds, "cus %d nframes %d R %d rmax %d", cus[ci], nframes, R, rmax);
      REQUIRE(R == 1 || (nframes + R - 2) / (R - 1) > rounds, "cus %d nframes %d: R %d is not the smallest with %d rounds", cus[ci], nframes, R, rounds);
      steps += walk(nframes, R); ++plans;
      for (int forced = 1; forced <= rmax + 3; ++forced) {                // rows=loop:<R>: taken as it is on every device,
        const int Rf = plan_psd_rows(nframes, cus[ci], forced);
        REQUIRE(Rf == std::min(forced, nframes), "forced %d nframes %d -> %d", forced, nframes, Rf);
        if (forced > walked_to && forced <= nframes) { steps += walk(nframes, Rf); ++plans; }   // so each (nframes, R) is walked once
      }
    }
  }
  REQUIRE(plan_psd_rows(240, 256, -1) == 60 && plan_psd_rows(1, 256, -1) == 1 && plan_psd_rows(16, 256, -1) == 16, "the bench's and the tests' grids");
  // the forms as launch_psd64k sees them: the columns form below, the rows form above
  SpectrumTuning t;
  REQUIRE(psd_rows_form(t, 240, 256) == 60 && psd_launch_form(t, 240, 256) == ((60 << kPsdRowsFormShift) | 61), "default form %d", psd_launch_form(t, 240, 256));
  REQUIRE(psd_launch_form(t, 1, 256) == ((1 << kPsdRowsFormShift) | 2), "one frame");
  t.rows_r = 0; REQUIRE(psd_rows_form(t, 240, 256) == 0 && psd_launch_form(t, 240, 256) == 61, "rows unit");
  t.rows_r = 3; REQUIRE(psd_rows_form(t, 240, 256) == 3 && psd_rows_form(t, 2, 256) == 2, "rows loop:3");
  t.cols_g = 0; REQUIRE(psd_launch_form(t, 240, 256) == ((3 << kPsdRowsFormShift) | 1), "columns unit, rows loop:3");
  t.packed = 0; REQUIRE(psd_launch_form(t, 240, 256) == 0, "float2");
  // ... and as the environment asks for them: read only under the master switch, a malformed part leaves its default
  const struct { const char* text; int cols, rows; } envs[] = {
      {"unit", 0, 0}, {"loop:3", 3, -1}, {"rows=unit", -1, 0}, {"rows=loop:3", -1, 3}, {"unit,rows=loop:30", 0, 30}, {"loop:64,rows=unit", 64, 0},
      {"rows=loop:5,loop:7", 7, 5}, {"rows=loop:0", -1, -1}, {"rows=loop:", -1, -1}, {"rows=loop:-2", -1, -1}, {"rows=loop:99999999", -1, kPsdRowsMaxR},
      {"rows=units", -1, -1}, {"rows=", -1, -1}, {"rows", -1, -1}, {"unit,", 0, 0}, {",rows=unit", -1, 0}, {"unit,rows=bogus", 0, -1}, {"", -1, -1}};
  for (const auto& e : envs) {
    setenv("PYSDR_PSD_PATH", e.text, 1);
    unsetenv("PYSDR_TUNING");
    REQUIRE(SpectrumTuning::from_env().cols_g == -1 && SpectrumTuning::from_env().rows_r == -1, "PYSDR_PSD_PATH=%s read without PYSDR_TUNING", e.text);
    setenv("PYSDR_TUNING", "1", 1);
    const SpectrumTuning got = SpectrumTuning::from_env();
    REQUIRE(got.cols_g == e.cols && got.rows_r == e.rows, "PYSDR_PSD_PATH=%s -> columns %d rows %d, expected %d %d", e.text, got.cols_g, got.rows_r, e.cols, e.rows);
  }
  unsetenv("PYSDR_PSD_PATH");
  REQUIRE(SpectrumTuning::from_env().rows_r == -1, "unset");
  printf("psd rows plan: %ld plans, %ld frames walked\nPSD_ROWS_PLAN_OK\n", plans, steps);
  return 0;
}
