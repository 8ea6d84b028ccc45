// C ABI of the fine channelizer (include/pysdr_hip.h).  Host-side only: the second stage's kernel
// and its launch functions live in fine.hip, what both sides share in fine_plan.h.  The object answers to the
// channelizer's handle type (chan_object.h): it owns a first-stage channelizer of the needed coarse rows, which writes
// its rows straight behind the history of the row buffer, and queues the second stage and the roll behind it on the first
// stage's stream.  Every device resource is an owner (host_res.h): deleting the object frees it.
#include "chan_object.h"
#include "fine_plan.h"

namespace pysdr {
int fine_prepare(const FinePlan& p);
int launch_fine(const FinePlan& p, const FineArgs& a, int gx, int gy, hipStream_t st);
int launch_fine_roll(float* rows, long long pitch1, int hist, int n1, int nk1, hipStream_t st);
}  // namespace pysdr

using namespace pysdr;

namespace {

struct FineExt {
  FinePlan plan;                    // for max_taps2: hist and the taps' room follow from it
  pysdr_chan* s1 = nullptr;         // the first stage, owned
  int max_taps1 = 0, max_taps2 = 0;
  int L2 = 0, P2 = 0;               // the current second prototype (0: none set yet)
  long long pitch1 = 0;             // row pitch of d_rows: hist + the first stage's out_cap
  DevBuf<float2> d_rows;            // [nk1][pitch1]
  DevBuf<float> d_taps;             // [P2max][M2]
  DevBuf<float2> d_tw;              // [M2]
  DevBuf<int> d_perm;               // [Q]
  DevBuf<int> d_a0;                 // [nk1]
  std::vector<float> h_taps;
};

FineExt* ext_of(pysdr_chan* c) { return static_cast<FineExt*>(c->ext); }

int fine_alloc(pysdr_chan* c, FineExt* e) {
  const FinePlan& p = e->plan;
  const std::vector<float> tw = fft_twiddles(p.M2);
  std::vector<int> perm(p.Q), a0(p.nk1);          // where the passes leave the second-stage channel of kept channel u
  for (int u = 0; u < p.Q; ++u) perm[u] = fft_position(fine_k2(u - p.Q / 2, p.M2), p.M2, p.npass, p.radix);
  for (int j = 0; j < p.nk1; ++j) a0[j] = fine_a0(p, j);
  PYSDR_HIP_CHECK(e->d_rows.alloc((size_t)p.nk1 * (size_t)e->pitch1));
  PYSDR_HIP_CHECK(e->d_taps.alloc((size_t)p.P2 * p.M2));
  PYSDR_HIP_CHECK(e->d_tw.alloc((size_t)p.M2));
  PYSDR_HIP_CHECK(e->d_perm.alloc((size_t)p.Q));
  PYSDR_HIP_CHECK(e->d_a0.alloc((size_t)p.nk1));
  PYSDR_HIP_CHECK(hipMemcpy(e->d_tw.get(), tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice));
  PYSDR_HIP_CHECK(hipMemcpy(e->d_perm.get(), perm.data(), perm.size() * sizeof(int), hipMemcpyHostToDevice));
  PYSDR_HIP_CHECK(hipMemcpy(e->d_a0.get(), a0.data(), a0.size() * sizeof(int), hipMemcpyHostToDevice));
  return fine_prepare(p);
}

int fine_reset(pysdr_chan* c) {
  FineExt* e = ext_of(c);
  const int rc = pysdr_chan_reset(e->s1);
  if (rc != PYSDR_OK) return rc;
  PYSDR_HIP_CHECK(hipSetDevice(c->device));
  PYSDR_HIP_CHECK(hipMemsetAsync(e->d_rows.get(), 0, (size_t)e->plan.nk1 * (size_t)e->pitch1 * sizeof(float2), c->ext_stream));
  PYSDR_HIP_CHECK(hipStreamSynchronize(c->ext_stream));
  c->n_abs = 0;
  return PYSDR_OK;
}

void fine_destroy(pysdr_chan* c) {
  FineExt* e = ext_of(c);
  if (!e) return;
  pysdr_chan* s1 = e->s1;
  delete e;                               // (the owners free: host_res.h)
  c->ext = nullptr;
  pysdr_chan_destroy(s1);
}

int fine_process(pysdr_chan* c, const void* iq, int n, int on_device, void* out, long long out_pitch, int out_on_device, int* n_out) {
  FineExt* e = ext_of(c);
  const FinePlan& pl = e->plan;
  if (n < 0 || (n > 0 && !iq)) { set_last_error("pysdr_chan_process: n %d / NULL input", n); return PYSDR_ERR_ARG; }
  if (n > c->max_in) { set_last_error("pysdr_chan_process: n %d > max_in %d", n, c->max_in); return PYSDR_ERR_STATE; }
  if (e->L2 == 0) { set_last_error("pysdr_chan_process: no taps set (pysdr_chan_fine_set_taps)"); return PYSDR_ERR_STATE; }
  const unsigned long long D = (unsigned long long)c->D, D1 = (unsigned long long)pl.D1;
  const unsigned long long s0 = c->n_abs, s1 = s0 + (unsigned long long)n;
  const unsigned long long mf = (s0 + D - 1) / D, ml = (s1 + D - 1) / D;          // fine outputs with s0 <= m D < s1
  const int nf = (int)(ml - mf);
  if (nf > 0 && !out) { set_last_error("pysdr_chan_process: NULL output"); return PYSDR_ERR_ARG; }
  if (out_pitch < nf) { set_last_error("pysdr_chan_process: pitch %lld < the call's %d outputs", out_pitch, nf); return PYSDR_ERR_STATE; }
  if (n == 0) return PYSDR_OK;
  PYSDR_HIP_CHECK(hipSetDevice(c->device));
  hipStream_t st = c->ext_stream;
  // stage 1: its outputs m1f .. m1f + n1 - 1 go behind the history of every row
  const unsigned long long m1f = (s0 + D1 - 1) / D1;
  int n1 = 0;
  int rc = pysdr_chan_process(e->s1, iq, n, on_device, e->d_rows.get() + pl.hist, e->pitch1, 1, &n1);
  if (rc != PYSDR_OK) return rc;
  if (nf > 0) {
    if (!out_on_device) PYSDR_HIP_CHECK(c->d_out.grow((size_t)c->nk * c->out_cap));
    const FineTile t = fine_tile(pl, nf);
    FineArgs a{};
    a.rows = reinterpret_cast<const float*>(e->d_rows.get()); a.pitch1 = e->pitch1;
    a.hist = pl.hist; a.M2 = pl.M2; a.D2 = pl.D2; a.C2 = pl.C2; a.P2 = e->P2; a.L2 = e->L2; a.mp = pl.mp;
    a.off = (int)fine_pos(pl.hist, (long long)(mf * (unsigned long long)pl.D2), (long long)m1f);
    a.mf_lo = (int)(mf & 3ull); a.nframes = nf; a.nk1 = pl.nk1; a.fw = t.fw; a.rw = t.rw;
    a.fw_shift = 0;
    while ((1 << a.fw_shift) < t.fw) ++a.fw_shift;
    a.taps = e->d_taps.get(); a.tw = reinterpret_cast<const float*>(e->d_tw.get());
    a.perm = e->d_perm.get(); a.a0 = e->d_a0.get();
    a.Q = pl.Q; a.Mf = pl.Mf; a.ng = pl.ng;
    a.y = reinterpret_cast<float*>(out_on_device ? static_cast<float2*>(out) : c->d_out.get());
    a.pitch = out_on_device ? out_pitch : (long long)c->out_cap;
    a.magic_M2 = magic_of(pl.M2); a.magic_Q = magic_of(pl.Q);
    a.fft = fft_passes(pl.M2, pl.npass, pl.radix);
    rc = launch_fine(pl, a, t.gx, t.gy, st);
    if (rc) return rc;
  }
  if (n1 > 0) {
    rc = launch_fine_roll(reinterpret_cast<float*>(e->d_rows.get()), e->pitch1, pl.hist, n1, pl.nk1, st);
    if (rc) return rc;
  }
  c->n_abs = s1;
  *n_out = nf;
  if (nf > 0 && !out_on_device)
    PYSDR_HIP_CHECK(hipMemcpy2DAsync(out, (size_t)out_pitch * sizeof(float2), c->d_out.get(), (size_t)c->out_cap * sizeof(float2),
                                     (size_t)nf * sizeof(float2), (size_t)c->nk, hipMemcpyDeviceToHost, st));
  if (!on_device || !out_on_device) PYSDR_HIP_CHECK(hipStreamSynchronize(st));   // host buffers are the caller's again
  return PYSDR_OK;
}

const ChanOps kFineOps = {fine_process, fine_reset, fine_destroy};

}  // namespace

extern "C" {

int pysdr_chan_fine_plan(int M1, int D1, int M2, int D2, int ntaps1, int ntaps2, int g_first, int ng, int32_t out[16]) {
  if (!out) { set_last_error("pysdr_chan_fine_plan: out is NULL"); return PYSDR_ERR_ARG; }
  FinePlan p;
  ChanPlan p1;
  if (!fine_plan(M1, D1, M2, D2, ntaps1, ntaps2, g_first, ng, &p) || !chan_plan(M1, D1, &p1)) {
    set_last_error("pysdr_chan_fine_plan: M1 %d / D1 %d / M2 %d / D2 %d, taps %d / %d, channels %d + %d: M1 = 2^a 5^b in [16, 4096], "
                   "M1 / D1 in {2, 4}; M2 = 2^a 5^b in [%d, %d], M2 / D2 in {1, 2, 4}; Q = M2 D1 / M1 an even integer >= 8; "
                   "taps in [1, 16 M]; g_first in [0, M1 Q), ng in [1, min(M1 Q, %d)]",
                   M1, D1, M2, D2, ntaps1, ntaps2, g_first, ng, kFineM2Min, kFineM2Max, kFineNgMax);
    return PYSDR_ERR_ARG;
  }
  for (int i = 0; i < 16; ++i) out[i] = 0;
  out[0] = p.Q; out[1] = p.Mf; out[2] = p.D; out[3] = p.C2; out[4] = p.k1_first; out[5] = p.nk1; out[6] = p.slots;
  out[7] = p.lds_bytes; out[8] = p.hist; out[9] = p.P2; out[10] = p.npass;
  for (int i = 0; i < p.npass && i < 5; ++i) out[11 + i] = p.radix[i];
  return PYSDR_OK;
}

int pysdr_chan_fine_create(int device, int M1, int D1, int M2, int D2, int g_first, int ng, int max_taps1, int max_taps2, int max_in,
                           pysdr_chan** out) {
  if (!out) { set_last_error("pysdr_chan_fine_create: out is NULL"); return PYSDR_ERR_ARG; }
  *out = nullptr;
  int32_t pl[16];
  int rc = pysdr_chan_fine_plan(M1, D1, M2, D2, max_taps1, max_taps2, g_first, ng, pl);
  if (rc != PYSDR_OK) return rc;
  if (max_in < 1 || max_in > kChanMaxIn) {
    set_last_error("pysdr_chan_fine_create: max_in %d outside [1, %d]", max_in, kChanMaxIn);
    return PYSDR_ERR_ARG;
  }
  rc = use_device(device);
  if (rc) return rc;
  pysdr_chan* c = new pysdr_chan();
  FineExt* e = new FineExt();
  c->ops = &kFineOps; c->ext = e;
  fine_plan(M1, D1, M2, D2, max_taps1, max_taps2, g_first, ng, &e->plan);
  const FinePlan& p = e->plan;
  c->device = device; c->M = p.Mf; c->D = p.D; c->k_first = g_first; c->nk = ng; c->max_in = max_in;
  c->out_cap = ((max_in + p.D - 1) / p.D + 1 + 15) & ~15;
  e->max_taps1 = max_taps1; e->max_taps2 = max_taps2;
  rc = pysdr_chan_create(device, M1, D1, p.k1_first, p.nk1, max_taps1, max_in, &e->s1);
  if (rc != PYSDR_OK) { pysdr_chan_destroy(c); return rc; }
  c->ext_stream = e->s1->stream;
  e->pitch1 = (long long)p.hist + e->s1->out_cap;
  rc = fine_alloc(c, e);
  if (rc) { failed_in("pysdr_chan_fine_create", rc); pysdr_chan_destroy(c); return rc; }
  rc = pysdr_chan_reset(c);
  if (rc != PYSDR_OK) { pysdr_chan_destroy(c); return rc; }
  *out = c;
  return PYSDR_OK;
}

int pysdr_chan_fine_set_taps(pysdr_chan* c, const double* h1, int n1, const double* h2, int n2) {
  if (!c || !h1 || !h2) { set_last_error("pysdr_chan_fine_set_taps: NULL channelizer or taps"); return PYSDR_ERR_ARG; }
  if (!c->ops) { set_last_error("pysdr_chan_fine_set_taps: not a fine channelizer (pysdr_chan_set_taps)"); return PYSDR_ERR_STATE; }
  std::lock_guard<std::mutex> lk(c->mu);
  FineExt* e = ext_of(c);
  if (n1 < 1 || n1 > e->max_taps1 || n2 < 1 || n2 > e->max_taps2) {
    set_last_error("pysdr_chan_fine_set_taps: taps %d / %d outside [1, max_taps = %d / %d]", n1, n2, e->max_taps1, e->max_taps2);
    return PYSDR_ERR_ARG;
  }
  const int rc = pysdr_chan_set_taps(e->s1, h1, n1);
  if (rc != PYSDR_OK) return rc;
  PYSDR_HIP_CHECK(hipSetDevice(c->device));
  const int M2 = e->plan.M2, P2 = (n2 + M2 - 1) / M2;
  PYSDR_HIP_CHECK(hipStreamSynchronize(c->ext_stream));           // the staging vector may still feed an earlier copy
  e->h_taps.assign((size_t)P2 * M2, 0.f);
  for (int i = 0; i < n2; ++i) e->h_taps[i] = (float)h2[i];
  PYSDR_HIP_CHECK(hipMemcpyAsync(e->d_taps.get(), e->h_taps.data(), e->h_taps.size() * sizeof(float), hipMemcpyHostToDevice, c->ext_stream));
  PYSDR_HIP_CHECK(hipStreamSynchronize(c->ext_stream));
  e->L2 = n2; e->P2 = P2;
  return PYSDR_OK;
}

}  // extern "C"
