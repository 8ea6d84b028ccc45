// The channelizer's handle (include/pysdr_hip.h: pysdr_chan), shared by its host half (api_objects.hip) and the host half
// of the fine channelizer (api_fine.hip), which answers to the same handle type: a handle whose `ops` is set is a
// channelizer of another kind behind the same entry points -- pysdr_chan_process / reset / sync / destroy and chan_info
// hand over to it, so an object that borrows a channelizer runs on either kind unchanged.  Not part of the public ABI.
#pragma once

#include "host_res.h"
#include "objects_plan.h"

struct pysdr_chan;

namespace pysdr {
struct ChanOps {
  int (*process)(pysdr_chan* c, const void* iq, int n, int on_device, void* out, long long out_pitch, int out_on_device,
                 int* n_out);                           // called under c->mu, *n_out = 0
  int (*reset)(pysdr_chan* c);                          // called under c->mu
  void (*destroy)(pysdr_chan* c);                       // frees c->ext; the handle itself is deleted by the caller
};
}  // namespace pysdr

struct pysdr_chan {
  int device = 0, M = 0, D = 0, k_first = 0, nk = 0, max_taps = 0, max_in = 0;
  int H = 0;               // history kept: ceil(max_taps / M) M - 1 samples
  int P = 0;               // taps per branch of the current prototype (0: none set yet)
  int out_cap = 0;         // row pitch of the internal output buffer: most outputs one call can complete, rounded up to 16
  int cur = 0;             // which history buffer is current
  unsigned long long n_abs = 0;   // input samples since create / reset
  pysdr::ChanPlan plan;
  pysdr::Stream stream;    // every launch and copy of the channelizer (and of a bank on it) is queued here
  pysdr::DevBuf<float2> d_hist[2];
  pysdr::DevBuf<float> d_taps;
  pysdr::DevBuf<float2> d_tw;
  pysdr::DevBuf<int> d_perm;
  pysdr::DevBuf<float2> d_in;     // staging of host input  [max_in]:      allocated by the first call that passes a host pointer
  pysdr::DevBuf<float2> d_out;    // staging of host output [nk][out_cap]: likewise
  std::vector<float> h_taps;
  std::mutex mu;           // one call at a time on a handle: set_taps / reset / sync / process
  // a fine channelizer (api_fine.hip): M, D, k_first, nk, max_in and n_abs describe the fine raster; the fields of the
  // kernel's launch above stay unused, and the work is queued on the first stage's stream
  const pysdr::ChanOps* ops = nullptr;
  void* ext = nullptr;
  hipStream_t ext_stream = nullptr;
  hipStream_t queue() const { return ops ? ext_stream : stream.get(); }
};
