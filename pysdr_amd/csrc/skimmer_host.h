// The decoder bank under the five skimmers -- CW (api_cw.hip), PSK31 (api_psk.hip), RTTY raster (api_fsk.hip), FT8 and FT4
// (api_ft.hip) -- as skimmer.DecoderBank is under their Python classes: a client of a channelizer (chan_client.h) with rows
// of event slots and a count per row.  Here, once: the fields every skimmer holds, the refusal of a missing handle, reset,
// sync, fetch, the create sequence and the whole of a process call around the kind's own launch.  Nothing here asks which
// kind it serves: what differs is data (rows, words, the row's name, the public function's name `who` for the messages)
// or lives in the kind's file -- its struct, plan, alloc, reset_locked, state, and the callables it hands to
// skimmer_create and skimmer_process.  Those are template parameters: no call allocates for them.  Beside the base's
// fields a kind's struct has plan.cap, plan.ypitch and feed_rows().  Host only; not part of the public ABI.
#pragma once

#include "chan_client.h"

namespace pysdr {

struct SkimmerBase : ChanClient {
  int max_out = 0;                  // outputs of the channelizer a call may complete
  int rows = 0;                     // event rows: channels (CW) or fine rows
  int words = 0;                    // int32 words of a row's event slots: the event cap times the words of a slot
  DevBuf<int32_t> d_events;         // [rows][words]
  DevBuf<int32_t> d_counts;         // [rows]
};

// The refusal of every call on a missing handle.  `also`: what the call names beside the handle.
inline int no_skimmer(const char* who, const char* also = "") {
  set_last_error("%s: NULL skimmer%s", who, also);
  return PYSDR_ERR_ARG;
}

// The base's two buffers, for a kind's alloc and, zeroed on the stream, for its reset_locked.
inline int skimmer_alloc(SkimmerBase* w) {
  PYSDR_HIP_CHECK(w->d_events.alloc((size_t)w->rows * (size_t)w->words));
  PYSDR_HIP_CHECK(w->d_counts.alloc((size_t)w->rows));
  return PYSDR_OK;
}
inline int skimmer_clear(SkimmerBase* w, hipStream_t st) {
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_counts.get(), 0, (size_t)w->rows * sizeof(int32_t), st));
  PYSDR_HIP_CHECK(hipMemsetAsync(w->d_events.get(), 0, (size_t)w->rows * (size_t)w->words * sizeof(int32_t), st));
  return PYSDR_OK;
}

template <class W>
int skimmer_reset(W* w, const char* who, int (*reset_locked)(W*)) {
  if (!w) return no_skimmer(who);
  std::lock_guard<std::mutex> lk(w->mu);
  return reset_locked(w);
}

inline int skimmer_sync(SkimmerBase* w, const char* who) {
  if (!w) return no_skimmer(who);
  return client_sync(w);
}

// `what` names a row in the messages: "row", "fine row"
inline int skimmer_fetch(SkimmerBase* w, const char* who, const char* what, const int* rows, int nrows, int32_t* events, long long pitch) {
  if (!w) return no_skimmer(who);
  return client_fetch_events(w, who, what, w->d_events.get(), w->rows, w->words, rows, nrows, events, pitch);
}

// A create call.  `have`: the kind's own pointers are all there; `missing` names them for the refusal otherwise.
// plan(w), on the bound object: the kind's plan, or the refusal of its public plan call passed on; then cfg, rows, words
// and the kind's host tables stored.
template <class W, class Plan>
int skimmer_create(const char* who, bool have, const char* missing, pysdr_chan* ch, int max_out, W** out, int (*alloc)(W*),
                   int (*reset_locked)(W*), Plan plan) {
  if (!out) { set_last_error("%s: out is NULL", who); return PYSDR_ERR_ARG; }
  *out = nullptr;
  if (!have) { set_last_error("%s: %s", who, missing); return PYSDR_ERR_ARG; }
  W* w = new W();
  int rc = client_bind(w, ch);
  if (rc == PYSDR_OK) rc = plan(w);
  if (rc != PYSDR_OK) { delete w; return rc; }
  w->max_out = max_out;
  return client_create(w, who, alloc, reset_locked, out);
}

// A process call.  delivered(step, nf, st), once the channelizer has put nf outputs behind w->feed_rows(): the kind's
// launch (none when nf is 0: no state change, no event) and what it keeps of the call.  after(st): copies of the kind's
// further outputs, which it makes on empty calls too; `more_out`: there are some, to host memory.  The refusals of n, the
// input, max_in, ev_pitch and max_out come before the channelizer's pass: such a call moves neither the stream nor an output.
inline int no_more_out(hipStream_t) { return PYSDR_OK; }
template <class W, class Delivered, class After = int (*)(hipStream_t)>
int skimmer_process(W* w, const char* who, const void* iq, int n, int on_device, int* n_out, int32_t* counts, int32_t* events,
                    long long ev_pitch, Delivered delivered, bool more_out = false, After after = no_more_out) {
  if (!w || !n_out) return no_skimmer(who, " or n_out");
  *n_out = 0;
  std::lock_guard<std::mutex> lk(w->mu);
  ClientStep step;
  int rc = client_begin(w, who, iq, n, &step);
  if (rc != PYSDR_OK) return rc;
  if (events && ev_pitch < w->words) {
    set_last_error(w->words == w->plan.cap ? "%s: ev_pitch %lld < the event cap %d" : "%s: ev_pitch %lld < the event cap's %d words",
                   who, ev_pitch, w->words);
    return PYSDR_ERR_STATE;
  }
  if (step.nf_want > (unsigned long long)w->max_out) {
    set_last_error("%s: the call would complete %llu outputs, max_out is %d", who, step.nf_want, w->max_out);
    return PYSDR_ERR_STATE;
  }
  int nf = 0;
  rc = client_feed(w, who, "skimmer", iq, n, on_device, w->feed_rows(), w->plan.ypitch, step, &nf);
  if (rc != PYSDR_OK) return rc;
  const size_t rows = (size_t)w->rows, words = (size_t)w->words;
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  rc = delivered(step, nf, st);
  if (rc) return rc;
  if (nf == 0) {
    if (counts) std::memset(counts, 0, rows * sizeof(int32_t));
  } else {
    *n_out = nf;
    if (counts) PYSDR_HIP_CHECK(hipMemcpyAsync(counts, w->d_counts.get(), rows * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (events)
      PYSDR_HIP_CHECK(hipMemcpy2DAsync(events, (size_t)ev_pitch * sizeof(int32_t), w->d_events.get(), words * sizeof(int32_t),
                                       words * sizeof(int32_t), rows, hipMemcpyDeviceToHost, st));
  }
  rc = after(st);
  if (rc) return rc;
  // host buffers are the caller's again (on an empty call too, though the channelizer has synchronised by then if its
  // input was the host's)
  if (counts || events || more_out || !on_device) PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  return PYSDR_OK;
}

}  // namespace pysdr
