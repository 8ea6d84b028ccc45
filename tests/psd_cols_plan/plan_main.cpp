// The grid of the columns loop of the 64k PSD (pysdr_amd/csrc/host_plan.h plan_psd_cols) and the walk of its workgroups
// over the frames of a launch (psd_cols_geom.h PsdColsWalk, the very code the kernel steps with), on the CPU under
// AddressSanitizer + UBSan: for nframes 1 ... 1000, for CU counts 1, 8, 256 and 304 and every grid the plan can return
// for them -- the default and every forced G from 1 to past the residency -- each workgroup's sequence is walked with a
// "load" of every frame index the kernel would load (the first frame in front of the loop, the next one inside it) into a
// table of exactly nframes entries, so that an index >= nframes is an out-of-bounds write the sanitizer reports.
//   every frame is transformed exactly once and loaded exactly once, no index >= nframes is touched,
//   no workgroup has more than one frame more than another, the default's 16 G workgroups are resident at once.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host_plan.h"
#include "psd_cols_geom.h"

using namespace pysdr;

#define REQUIRE(c, ...) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static long walk(int nframes, int G) {
  REQUIRE(G >= 1 && G <= nframes, "G %d nframes %d", G, nframes);
  std::vector<int> loaded((size_t)nframes, 0), done((size_t)nframes, 0);   // heap: the sanitizer guards both ends
  int lo = nframes, hi = 0;
  long steps = 0;
  for (int g = 0; g < G; ++g) {
    PsdColsWalk fr(g, G, nframes);
    int mine = 0;
    loaded.data()[fr.f] += 1;                         // the prologue's load of the first frame
    for (;;) {
      if (fr.has_next()) loaded.data()[fr.fn] += 1;   // the prefetch
      REQUIRE(loaded.data()[fr.f] == 1, "frame %d transformed without its samples (nframes %d G %d)", fr.f, nframes, G);
      done.data()[fr.f] += 1;
      ++mine; ++steps;
      if (!fr.has_next()) break;
      fr.advance();
    }
    lo = std::min(lo, mine); hi = std::max(hi, mine);
  }
  for (int f = 0; f < nframes; ++f)
    REQUIRE(loaded[(size_t)f] == 1 && done[(size_t)f] == 1, "frame %d of %d at G %d: loaded %d x, transformed %d x", f, nframes, G, loaded[(size_t)f], done[(size_t)f]);
  REQUIRE(hi - lo <= 1, "nframes %d G %d: %d .. %d frames per workgroup", nframes, G, lo, hi);
  return steps;
}

int main() {
  long plans = 0, steps = 0;
  const int cus[4] = {1, 8, 256, 304};
  for (int ci = 0; ci < 4; ++ci) {
    const int residency = cus[ci] * kPsdColsWgPerCu;                       // workgroups of 37 KB of LDS a device holds at once
    const int gmax = psd_cols_max_g(cus[ci]);
    REQUIRE(gmax >= 1 && (kPsdColBlocks * gmax <= residency || gmax == 1), "cus %d gmax %d", cus[ci], gmax);
    for (int nframes = 1; nframes <= 1000; ++nframes) {
      const int G = plan_psd_cols(nframes, cus[ci], -1);
      REQUIRE(G >= 1 && G <= gmax && G <= nframes, "cus %d nframes %d G %d", cus[ci], nframes, G);
      REQUIRE(kPsdColBlocks * G <= residency || G == 1, "cus %d nframes %d: %d workgroups, %d resident", cus[ci], nframes, kPsdColBlocks * G, residency);
      // the evened grid needs no more rounds than the full one
      REQUIRE((nframes + G - 1) / G == (nframes + gmax - 1) / gmax, "cus %d nframes %d G %d gmax %d", cus[ci], nframes, G, gmax);
      steps += walk(nframes, G); ++plans;
      for (int forced = 1; forced <= gmax + 3; ++forced) {                 // PYSDR_PSD_PATH=loop:<G>
        const int Gf = plan_psd_cols(nframes, cus[ci], forced);
        REQUIRE(Gf == std::min(forced, nframes), "forced %d nframes %d -> %d", forced, nframes, Gf);
        steps += walk(nframes, Gf); ++plans;
      }
    }
  }
  // the switch's forms as launch_psd64k sees them
  SpectrumTuning t;
  REQUIRE(psd_form(t, 240, 256) == 1 + 60 && psd_form(t, 1, 256) == 2 && psd_form(t, 104, 256) == 1 + 52, "default forms %d %d %d", psd_form(t, 240, 256), psd_form(t, 1, 256), psd_form(t, 104, 256));
  t.cols_g = 0; REQUIRE(psd_form(t, 240, 256) == 1, "unit");
  t.cols_g = 3; REQUIRE(psd_form(t, 240, 256) == 4 && psd_form(t, 2, 256) == 3, "loop:3");
  t.packed = 0; REQUIRE(psd_form(t, 240, 256) == 0, "float2");
  // ... and as the environment asks for them: read only under the master switch, anything malformed leaves the default
  const struct { const char* text; int want; } envs[] = {{"unit", 0}, {"loop:3", 3}, {"loop:64", 64}, {"loop:0", -1}, {"loop:", -1}, {"loop:-2", -1},
                                                         {"loop:99999999", kPsdColsMaxG}, {"loop", -1}, {"units", -1}, {"", -1}};
  for (const auto& e : envs) {
    setenv("PYSDR_PSD_PATH", e.text, 1);
    unsetenv("PYSDR_TUNING");
    REQUIRE(SpectrumTuning::from_env().cols_g == -1, "PYSDR_PSD_PATH=%s read without PYSDR_TUNING", e.text);
    setenv("PYSDR_TUNING", "1", 1);
    REQUIRE(SpectrumTuning::from_env().cols_g == e.want, "PYSDR_PSD_PATH=%s -> %d, expected %d", e.text, SpectrumTuning::from_env().cols_g, e.want);
  }
  unsetenv("PYSDR_PSD_PATH");
  REQUIRE(SpectrumTuning::from_env().cols_g == -1, "unset");
  printf("psd cols plan: %ld plans, %ld frames walked\nPSD_COLS_PLAN_OK\n", plans, steps);
  return 0;
}
