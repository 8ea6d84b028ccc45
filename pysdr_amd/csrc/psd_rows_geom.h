// The frames one workgroup of the rows loop walks over (psdfft.hip psd_rows_pk_kernel), shared by the kernel and by the
// host-side walk of tests/psd_rows_plan: workgroup r of the R rows of the grid (host_plan.h plan_psd_rows, R <= nframes)
// transforms the frames r, r + R, r + 2 R, ... < nframes, and while it transforms frame f it loads the intermediate and the
// block scales of frame f + R -- only if the launch has such a frame.
#pragma once

#if defined(__HIPCC__)
#define PYSDR_PSD_ROWS_HD __device__ __forceinline__
#else
#define PYSDR_PSD_ROWS_HD inline
#endif

namespace pysdr {

struct PsdRowsWalk {
  int f, fn, R, nframes;
  PYSDR_PSD_ROWS_HD PsdRowsWalk(int r, int R_, int nframes_) : f(r), fn(r + R_), R(R_), nframes(nframes_) {}
  PYSDR_PSD_ROWS_HD bool has_next() const { return fn < nframes; }   // the next frame exists: prefetch it, then go on with it
  PYSDR_PSD_ROWS_HD void advance() { f = fn; fn += R; }
};

}  // namespace pysdr
