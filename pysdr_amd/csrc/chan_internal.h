// What the channel bank (bank.hip) needs to know of a channelizer it borrows (chan.hip).  Not part of the public ABI.
#pragma once

#include "common.h"

namespace pysdr {

struct ChanInfo {
  int device, M, D, nk, max_in;
  int out_cap;                  // most outputs one call can complete, rounded up to 16
  unsigned long long n_abs;     // input samples since create / reset
  hipStream_t stream;           // every launch and copy of the channelizer is queued here
};
ChanInfo chan_info(pysdr_chan* c);   // takes the handle's lock for the read

}  // namespace pysdr
