// What the objects that borrow a channelizer share -- the channel bank (api_objects.hip) and, through skimmer_host.h, the
// five skimmers (api_cw.hip, api_psk.hip, api_fsk.hip, api_ft.hip): each queues its own kernel behind the channelizer's
// launch, on the channelizer's stream, with no host synchronisation in between.  Here, once: the borrowed handle's
// fields, the two steps of a call around the client's own checks (what the channelizer is about to complete; the
// channelizer's pass into the client's row buffer), the copy of fetched rows, sync, destroy and the tail of create.  The
// layer above it that the skimmers share -- event rows, the handle check, the whole call list -- is skimmer_host.h.  A
// client knows the channelizer through chan_info() alone (objects_plan.h), so it runs on either kind of handle
// (chan_object.h) unchanged.  Host only; not part of the public ABI.
#pragma once

#include "host_res.h"
#include "objects_plan.h"

namespace pysdr {

struct ChanClient {
  pysdr_chan* ch = nullptr;         // borrowed; outlives the client
  int device = 0, D = 0, nk = 0, max_in = 0, out_cap = 0;   // of the channelizer, fixed at its create
  hipStream_t stream = nullptr;     // the channelizer's
  int last_n_out = 0;               // outputs of the last call: what a fetch may copy
  std::mutex mu;                    // one call at a time on a handle
};

inline int client_bind(ChanClient* c, pysdr_chan* ch) {
  ChanInfo ci;
  const int rc = chan_info(ch, &ci);
  if (rc != PYSDR_OK) return rc;
  c->ch = ch; c->device = ci.device; c->D = ci.D; c->nk = ci.nk; c->max_in = ci.max_in; c->out_cap = ci.out_cap;
  c->stream = ci.stream;
  return PYSDR_OK;
}

struct ClientStep {
  unsigned long long m0 = 0;        // absolute index of the call's first output
  unsigned long long nf_want = 0;   // outputs the call completes
};

// First step of a call, under the client's lock: n and the input pointer, then what the channelizer is about to complete
// -- known before it advances its stream, so that the client's own checks can still refuse the call.
inline int client_begin(const ChanClient* c, const char* who, const void* iq, int n, ClientStep* s) {
  if (n < 0 || (n > 0 && !iq)) { set_last_error("%s: n %d / NULL input", who, n); return PYSDR_ERR_ARG; }
  if (n > c->max_in) { set_last_error("%s: n %d > max_in %d", who, n, c->max_in); return PYSDR_ERR_STATE; }
  ChanInfo ci;
  const int rc = chan_info(c->ch, &ci);
  if (rc != PYSDR_OK) return rc;
  const unsigned long long D = (unsigned long long)c->D, s0 = ci.n_abs, s1 = s0 + (unsigned long long)n;
  s->m0 = (s0 + D - 1) / D;
  s->nf_want = (s1 + D - 1) / D - s->m0;
  return PYSDR_OK;
}

// Second step: the channelizer's pass, its outputs to rows[a * pitch + i] on the device.  `what`: the client's kind, for
// the message.
inline int client_feed(ChanClient* c, const char* who, const char* what, const void* iq, int n, int on_device, void* rows,
                       long long pitch, const ClientStep& s, int* nf) {
  const int rc = pysdr_chan_process(c->ch, iq, n, on_device, rows, pitch, 1, nf);
  if (rc != PYSDR_OK) return rc;
  if (*nf != (int)s.nf_want) {
    set_last_error("%s: the channelizer was fed beside its %s (%d outputs, %d expected)", who, what, *nf, (int)s.nf_want);
    return PYSDR_ERR_STATE;
  }
  c->last_n_out = *nf;
  return PYSDR_OK;
}

// ---- fetched rows: runs of consecutive rows go as one strided copy
inline bool rows_inside(const char* who, const char* what, const int* rows, int nrows, int bound) {
  for (int i = 0; i < nrows; ++i)
    if (rows[i] < 0 || rows[i] >= bound) { set_last_error("%s: %s %d outside [0, %d)", who, what, rows[i], bound); return false; }
  return true;
}
inline int row_run(const int* rows, int nrows, int i) {
  int run = 1;
  while (i + run < nrows && rows[i + run] == rows[i] + run) ++run;
  return run;
}
// the run of `run` rows that starts at rows[i]: `width` elements of each, to row i and on of dst
template <class T>
int copy_row_run(const int* rows, int i, int run, const T* src, long long spitch, T* dst, long long dpitch, size_t width, hipStream_t st) {
  PYSDR_HIP_CHECK(hipMemcpy2DAsync(dst + (size_t)i * dpitch, (size_t)dpitch * sizeof(T), src + (size_t)rows[i] * spitch,
                                   (size_t)spitch * sizeof(T), width * sizeof(T), (size_t)run, hipMemcpyDeviceToHost, st));
  return PYSDR_OK;
}
// The skimmers' fetch: rows of the event buffer d_events[bound][cap], as the last call left them, to events[i * pitch].
// `what` names a row in the message.
inline int client_fetch_events(ChanClient* c, const char* who, const char* what, const int32_t* d_events, int bound, int cap,
                               const int* rows, int nrows, int32_t* events, long long pitch) {
  if (nrows < 0 || (nrows > 0 && (!rows || !events))) { set_last_error("%s: nrows %d / NULL rows or events", who, nrows); return PYSDR_ERR_ARG; }
  std::lock_guard<std::mutex> lk(c->mu);
  if (!rows_inside(who, what, rows, nrows, bound)) return PYSDR_ERR_ARG;
  if (pitch < cap) { set_last_error("%s: pitch %lld < the event cap %d", who, pitch, cap); return PYSDR_ERR_STATE; }
  if (c->last_n_out == 0 || nrows == 0) return PYSDR_OK;
  PYSDR_HIP_CHECK(hipSetDevice(c->device));
  for (int i = 0, run; i < nrows; i += run) {
    run = row_run(rows, nrows, i);
    const int rc = copy_row_run(rows, i, run, d_events, cap, events, pitch, (size_t)cap, c->stream);
    if (rc) return rc;
  }
  PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream));
  return PYSDR_OK;
}

inline int client_sync(ChanClient* c) {
  std::lock_guard<std::mutex> lk(c->mu);
  PYSDR_HIP_CHECK(hipSetDevice(c->device));
  PYSDR_HIP_CHECK(hipStreamSynchronize(c->stream));
  return PYSDR_OK;
}

// drains the borrowed stream, then deletes the object: its owners free (host_res.h)
template <class Obj>
void client_destroy(Obj* o) {
  if (!o) return;
  (void)hipSetDevice(o->device);
  if (o->stream) (void)hipStreamSynchronize(o->stream);
  delete o;
}

// The rest of a create function, once the object is bound and planned: its buffers, its first reset, the handle.
template <class Obj>
int client_create(Obj* o, const char* who, int (*alloc)(Obj*), int (*reset_locked)(Obj*), Obj** out) {
  int rc = use_device(o->device);
  if (rc) { delete o; return rc; }
  rc = alloc(o);
  if (rc) { failed_in(who, rc); client_destroy(o); return rc; }
  rc = reset_locked(o);
  if (rc != PYSDR_OK) { client_destroy(o); return rc; }
  *out = o;
  return PYSDR_OK;
}

}  // namespace pysdr
