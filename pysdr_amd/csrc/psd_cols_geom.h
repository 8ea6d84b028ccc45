// The frames one workgroup of the columns loop walks over (psdfft.hip psd_cols_pk_kernel), shared by the kernel and by the
// host-side walk of tests/psd_cols_plan: workgroup g of the G rows of the grid (host_plan.h plan_psd_cols, G <= nframes)
// transforms the frames g, g + G, g + 2 G, ... < nframes, and while it transforms frame f it loads frame f + G -- only if
// the launch has such a frame.
#pragma once

#if defined(__HIPCC__)
#define PYSDR_PSD_HD __device__ __forceinline__
#else
#define PYSDR_PSD_HD inline
#endif

namespace pysdr {

struct PsdColsWalk {
  int f, fn, G, nframes;
  PYSDR_PSD_HD PsdColsWalk(int g, int G_, int nframes_) : f(g), fn(g + G_), G(G_), nframes(nframes_) {}
  PYSDR_PSD_HD bool has_next() const { return fn < nframes; }   // the next frame exists: prefetch it, then go on with it
  PYSDR_PSD_HD void advance() { f = fn; fn += G; }
};

}  // namespace pysdr
