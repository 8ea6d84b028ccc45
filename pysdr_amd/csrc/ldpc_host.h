// The host half of the LDPC decoder, shared by the FT8 and the FT4 skimmer (api_ft.hip) over skimmer_host.h:
// the result buffers a skimmer owns, and the two calls -- candidates from the spectrum ring, soft bits from the host --
// written once for both objects, which name their fields alike (plan, t_done, d_ring, d_cand, h_cand, d_llr).  A call may
// ask for the second stage, ordered-statistics decoding (osd.hip), launched behind min-sum on the same stream.  Every
// check comes before any launch: a refusal changes nothing.  Host only; not part of the public ABI.
#pragma once

#include "ldpc_plan.h"
#include "osd_plan.h"
#include "skimmer_host.h"

namespace pysdr {

struct LdpcBufs {                   // allocated by the first decode call of a skimmer
  DevBuf<int32_t> d_status;         // [kLdpcMax][4]
  DevBuf<uint8_t> d_bits;           // [kLdpcMax][12]
  DevBuf<float> d_post;             // [kLdpcMax][174]
  DevBuf<int32_t> d_detail;         // [kLdpcMax][4]: the second stage's (osd_plan.h)
  bool ready = false;
};

inline int ldpc_bufs_ready(LdpcBufs* b) {
  if (b->ready) return PYSDR_OK;
  PYSDR_HIP_CHECK(b->d_status.alloc((size_t)kLdpcMax * kLdpcStatusWords));
  PYSDR_HIP_CHECK(b->d_bits.alloc((size_t)kLdpcMax * kLdpcBitsBytes));
  PYSDR_HIP_CHECK(b->d_post.alloc((size_t)kLdpcMax * kLdpcN));
  PYSDR_HIP_CHECK(b->d_detail.alloc((size_t)kLdpcMax * kOsdDetailWords));
  b->ready = true;
  return PYSDR_OK;
}

inline bool ldpc_call_ok(const char* who, int n, const pysdr_ldpc_cfg* cfg, const void* in0, const void* in1, const int32_t* status,
                         const uint8_t* bits) {
  if (!ldpc_n_ok(n) || (n > 0 && (!in0 || !in1 || !status || !bits))) {
    set_last_error("%s: n %d outside [0, %d] / a NULL input, status or bits", who, n, kLdpcMax);
    return false;
  }
  if (!ldpc_cfg_ok(cfg)) {
    set_last_error("%s: a cfg outside the rules (NULL; iters in [1, %d]; alpha finite and in (0, 1])", who, kLdpcItersMax);
    return false;
  }
  return true;
}

// The second stage of a call: none for the calls without it; the *_osd calls need a cfg inside the rule.
struct OsdCall {
  bool wanted;
  const pysdr_osd_cfg* cfg;
  int32_t* detail;                  // host [n][4] or NULL
};
constexpr OsdCall kNoOsd{false, nullptr, nullptr};

inline bool osd_call_ok(const char* who, const OsdCall& osd) {
  if (!osd.wanted || osd_cfg_ok(osd.cfg)) return true;
  set_last_error("%s: an osd cfg outside the rule (NULL; order in [0, %d])", who, kOsdOrderMax);
  return false;
}

// the launch and the way back, under the skimmer's lock, its device set
template <class W>
int ldpc_run(W* w, int source, LdpcArgs& a, const pysdr_ldpc_cfg* cfg, int32_t* status, uint8_t* bits, float* post, const OsdCall& osd) {
  hipStream_t st = w->stream;
  a.iters = cfg->iters; a.alpha = cfg->alpha;
  a.status = w->ldpc.d_status.get(); a.bits = w->ldpc.d_bits.get(); a.post = post ? w->ldpc.d_post.get() : nullptr;
  const int rc = launch_ldpc_decode(source, a, st);
  if (rc) return rc;
  const size_t n = (size_t)a.n;
  if (osd.wanted) {                                                    // behind min-sum on the same stream, before the copies back
    OsdArgs o{};
    o.llr = a.llr; o.ring = a.ring; o.tr = a.tr; o.nb = a.nb; o.nsub = a.nsub; o.cand = a.cand; o.n = a.n; o.order = osd.cfg->order;
    o.status = a.status; o.bits = a.bits; o.detail = osd.detail ? w->ldpc.d_detail.get() : nullptr;
    const int rc2 = launch_osd_decode(source, o, st);
    if (rc2) return rc2;
    if (osd.detail)
      PYSDR_HIP_CHECK(hipMemcpyAsync(osd.detail, o.detail, n * kOsdDetailWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  }
  PYSDR_HIP_CHECK(hipMemcpyAsync(status, a.status, n * kLdpcStatusWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  PYSDR_HIP_CHECK(hipMemcpyAsync(bits, a.bits, n * kLdpcBitsBytes, hipMemcpyDeviceToHost, st));
  if (post) PYSDR_HIP_CHECK(hipMemcpyAsync(post, a.post, n * kLdpcN * sizeof(float), hipMemcpyDeviceToHost, st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  return PYSDR_OK;
}

// A spectrum ring of a skimmer's, ring[nk][tr][nb], as a decode call names it; ring is NULL where there is none.
struct RingRef {
  const float* ring;
  int tr;
};

// Candidates (F[i], t0[i]) from a spectrum ring of the skimmer's: the first pass's, or the second pass's residue
// (pass_host.h).  which(w) names it and is asked under the skimmer's lock, so the ring it names cannot be replaced
// before the launch; a ring that is not there is PYSDR_ERR_STATE.  The skimmer's mode (W::Mode, ft_plan.h) gives the rule for a candidate, the last step of
// a frame behind its first, for the message, and the kernels' source.
template <class W, class Which>
int ldpc_decode_ring(W* w, const char* who, Which which, const int32_t* F, const long long* t0, int n, const pysdr_ldpc_cfg* cfg, int32_t* status,
                     uint8_t* bits, float* post, const OsdCall& osd = kNoOsd) {
  using Mode = typename W::Mode;
  if (!w) return no_skimmer(who);
  if (!ldpc_call_ok(who, n, cfg, F, t0, status, bits) || !osd_call_ok(who, osd)) return PYSDR_ERR_ARG;
  std::lock_guard<std::mutex> lk(w->mu);
  const RingRef ref = which(w);
  if (!ref.ring) {
    set_last_error("%s: nothing is kept for a second pass: call the skimmer's keep after create or reset", who);
    return PYSDR_ERR_STATE;
  }
  const float* ring = ref.ring;
  const int tr = ref.tr;
  const long long done = (long long)w->t_done;
  for (int i = 0; i < n; ++i)                                          // every candidate first: a refusal changes nothing
    if (!ft_llr_ok<Mode>(F[i], t0[i], done, w->plan.nfine, tr)) {
      set_last_error("%s: candidate %d (F %d, t0 %lld): F outside [0, %d), or a frame not yet complete or gone from the ring "
                     "(%lld steps done, its last is %lld, the ring holds %d)", who, i, (int)F[i], t0[i], w->plan.nfine, done,
                     t0[i] + kFtLag<Mode>, tr);
      return F[i] < 0 || F[i] >= w->plan.nfine ? PYSDR_ERR_ARG : PYSDR_ERR_STATE;
    }
  if (n == 0) return PYSDR_OK;
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  int rc = ldpc_bufs_ready(&w->ldpc);
  if (rc) return rc;
  hipStream_t st = w->stream;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));                          // h_cand may still feed an earlier copy
  w->h_cand.resize((size_t)n * 2);
  for (int i = 0; i < n; ++i) { w->h_cand[2 * (size_t)i] = F[i]; w->h_cand[2 * (size_t)i + 1] = (int32_t)(t0[i] % tr); }
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_cand.get(), w->h_cand.data(), (size_t)n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, st));
  LdpcArgs a{};
  a.ring = ring; a.tr = tr; a.nb = w->plan.nb; a.nsub = w->plan.nsub; a.cand = w->d_cand.get(); a.n = n;
  return ldpc_run(w, Mode::kLdpcSource, a, cfg, status, bits, post, osd);
}

// Soft bits from the host, through the skimmer's soft-bit buffer.
template <class W>
int ldpc_decode_llr(W* w, const char* who, const float* llr, int n, const pysdr_ldpc_cfg* cfg, int32_t* status, uint8_t* bits,
                    float* post, const OsdCall& osd = kNoOsd) {
  if (!w) return no_skimmer(who);
  if (!ldpc_call_ok(who, n, cfg, llr, llr, status, bits) || !osd_call_ok(who, osd)) return PYSDR_ERR_ARG;
  const long long bad = ldpc_first_nonfinite(llr, (size_t)n * kLdpcN);
  if (bad >= 0) {
    set_last_error("%s: soft bit %lld of candidate %lld is not finite", who, bad % kLdpcN, bad / kLdpcN);
    return PYSDR_ERR_ARG;
  }
  if (n == 0) return PYSDR_OK;
  std::lock_guard<std::mutex> lk(w->mu);
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  int rc = ldpc_bufs_ready(&w->ldpc);
  if (rc) return rc;
  hipStream_t st = w->stream;
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_llr.get(), llr, (size_t)n * kLdpcN * sizeof(float), hipMemcpyHostToDevice, st));
  LdpcArgs a{};
  a.llr = w->d_llr.get(); a.n = n;
  return ldpc_run(w, kLdpcFromBuffer, a, cfg, status, bits, post, osd);
}

}  // namespace pysdr
