// The host half of a-priori decoding, shared by the FT8 and the FT4 skimmer (api_ft.hip) beside
// ldpc_host.h, whose checks of a decode call it uses: the buffers a skimmer owns once its first AP call was made, and the two
// calls -- candidates from the first spectrum ring, soft bits from the host.  Every check comes before any launch: a
// refusal launches nothing and changes no output.  Host only; not part of the public ABI.
#pragma once

#include "ap_plan.h"
#include "ldpc_host.h"

namespace pysdr {

struct ApBufs {                     // allocated by the first AP call of a skimmer
  DevBuf<uint8_t> d_hyps;           // [kApHypMax][24]
  DevBuf<int32_t> d_pairs;          // [kApPairMax][2]
  DevBuf<int32_t> d_first;          // [kLdpcMax + 1]
  DevBuf<int32_t> d_detail;         // [kApPairMax][4]: every pair's status, iterations, nerr, nap
  DevBuf<uint8_t> d_pbits;          // [kApPairMax][12]
  DevBuf<int32_t> d_ap;             // [kLdpcMax][4]
  DevBuf<uint8_t> d_bits;           // [kLdpcMax][12]
  std::vector<int32_t> h_first;     // the offsets, as the pair list's check leaves them
  bool ready = false;
};

inline int ap_bufs_ready(ApBufs* b) {
  if (b->ready) return PYSDR_OK;
  PYSDR_HIP_CHECK(b->d_hyps.alloc((size_t)kApHypMax * kApHypBytes));
  PYSDR_HIP_CHECK(b->d_pairs.alloc((size_t)kApPairMax * 2));
  PYSDR_HIP_CHECK(b->d_first.alloc((size_t)kLdpcMax + 1));
  PYSDR_HIP_CHECK(b->d_detail.alloc((size_t)kApPairMax * kApDetailWords));
  PYSDR_HIP_CHECK(b->d_pbits.alloc((size_t)kApPairMax * kLdpcBitsBytes));
  PYSDR_HIP_CHECK(b->d_ap.alloc((size_t)kLdpcMax * kApWords));
  PYSDR_HIP_CHECK(b->d_bits.alloc((size_t)kLdpcMax * kLdpcBitsBytes));
  b->ready = true;
  return PYSDR_OK;
}

// what an AP call names beside its candidates
struct ApCall {
  const uint8_t* hyps;
  int H;
  const int32_t* pairs;
  int P;
  const pysdr_ap_cfg* cfg;
  int32_t* detail;                  // host [P][4] or NULL
};

// The table, the pair list and the settings; on success first[n + 1] holds the offsets.  Needs no lock and no device.
inline bool ap_call_ok(const char* who, int n, const ApCall& c, std::vector<int32_t>* first) {
  if (!ap_hyps_n_ok(c.H) || !ap_pairs_n_ok(c.P) || !c.hyps || (c.P > 0 && !c.pairs)) {
    set_last_error("%s: H %d outside [1, %d], P %d outside [0, %d] / a NULL table or pair list", who, c.H, kApHypMax, c.P, kApPairMax);
    return false;
  }
  if (!ap_cfg_ok(c.cfg)) {
    set_last_error("%s: an ap cfg outside the rules (NULL; mag finite and in [%g, %g]; nerr_max in [0, %d])", who, (double)kApMagMin,
                   (double)kApMagMax, kLdpcN);
    return false;
  }
  const int bad = ap_first_bad_hyp(c.hyps, c.H);
  if (bad >= 0) {
    set_last_error("%s: hypothesis %d is outside the rule (a mask that is empty or has a bit beyond 76, or a value bit outside the mask)", who, bad);
    return false;
  }
  first->assign((size_t)n + 1, 0);
  const int badp = ap_first_bad_pair(c.pairs, c.P, n, c.H, first->data());
  if (badp >= 0) {
    set_last_error("%s: pair %d (candidate %d, hypothesis %d) names a candidate outside [0, %d) or a hypothesis outside [0, %d), or "
                   "is not above the pair before it", who, badp, (int)c.pairs[2 * badp], (int)c.pairs[2 * badp + 1], n, c.H);
    return false;
  }
  return true;
}

// the launch and the way back, under the skimmer's lock, its device set, its AP buffers ready; `first` is w->ap.h_first
template <class W>
int ap_run(W* w, int source, ApArgs& a, const pysdr_ldpc_cfg* cfg, const ApCall& c, int32_t* ap, uint8_t* bits) {
  hipStream_t st = w->stream;
  ApBufs& b = w->ap;
  const size_t n = (size_t)a.n, P = (size_t)c.P;
  PYSDR_HIP_CHECK(hipMemcpyAsync(b.d_hyps.get(), c.hyps, (size_t)c.H * kApHypBytes, hipMemcpyHostToDevice, st));
  if (P) PYSDR_HIP_CHECK(hipMemcpyAsync(b.d_pairs.get(), c.pairs, P * 2 * sizeof(int32_t), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipMemcpyAsync(b.d_first.get(), b.h_first.data(), (n + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
  a.npairs = c.P; a.iters = cfg->iters; a.alpha = cfg->alpha; a.mag = c.cfg->mag; a.nerr_max = c.cfg->nerr_max;
  a.hyps = b.d_hyps.get(); a.pairs = b.d_pairs.get(); a.first = b.d_first.get();
  a.detail = b.d_detail.get(); a.pbits = b.d_pbits.get(); a.ap = b.d_ap.get(); a.bits = b.d_bits.get();
  const int rc = launch_ap_decode(source, a, st);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipMemcpyAsync(ap, a.ap, n * kApWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  PYSDR_HIP_CHECK(hipMemcpyAsync(bits, a.bits, n * kLdpcBitsBytes, hipMemcpyDeviceToHost, st));
  if (c.detail && P) PYSDR_HIP_CHECK(hipMemcpyAsync(c.detail, a.detail, P * kApDetailWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  return PYSDR_OK;
}

// Candidates (F[i], t0[i]) from the skimmer's first spectrum ring, under ldpc_decode_ring's rules.
template <class W>
int ap_decode_ring(W* w, const char* who, const int32_t* F, const long long* t0, int n, const pysdr_ldpc_cfg* cfg, const ApCall& c, int32_t* ap,
                   uint8_t* bits) {
  using Mode = typename W::Mode;
  if (!w) return no_skimmer(who);
  if (!ldpc_call_ok(who, n, cfg, F, t0, ap, bits)) return PYSDR_ERR_ARG;
  std::vector<int32_t> first;
  if (!ap_call_ok(who, n, c, &first)) return PYSDR_ERR_ARG;
  std::lock_guard<std::mutex> lk(w->mu);
  const int tr = w->plan.tr;
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
  const int rc = ap_bufs_ready(&w->ap);
  if (rc) return rc;
  hipStream_t st = w->stream;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));                          // h_cand and h_first may still feed an earlier copy
  w->ap.h_first.swap(first);
  w->h_cand.resize((size_t)n * 2);
  for (int i = 0; i < n; ++i) { w->h_cand[2 * (size_t)i] = F[i]; w->h_cand[2 * (size_t)i + 1] = (int32_t)(t0[i] % tr); }
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_cand.get(), w->h_cand.data(), (size_t)n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, st));
  ApArgs a{};
  a.ring = w->d_ring.get(); a.tr = tr; a.nb = w->plan.nb; a.nsub = w->plan.nsub; a.cand = w->d_cand.get(); a.n = n;
  return ap_run(w, Mode::kLdpcSource, a, cfg, c, ap, bits);
}

// Soft bits from the host, through the skimmer's soft-bit buffer.
template <class W>
int ap_decode_llr(W* w, const char* who, const float* llr, int n, const pysdr_ldpc_cfg* cfg, const ApCall& c, int32_t* ap, uint8_t* bits) {
  if (!w) return no_skimmer(who);
  if (!ldpc_call_ok(who, n, cfg, llr, llr, ap, bits)) return PYSDR_ERR_ARG;
  std::vector<int32_t> first;
  if (!ap_call_ok(who, n, c, &first)) return PYSDR_ERR_ARG;
  const long long bad = ldpc_first_nonfinite(llr, (size_t)n * kLdpcN);
  if (bad >= 0) {
    set_last_error("%s: soft bit %lld of candidate %lld is not finite", who, bad % kLdpcN, bad / kLdpcN);
    return PYSDR_ERR_ARG;
  }
  if (n == 0) return PYSDR_OK;
  std::lock_guard<std::mutex> lk(w->mu);
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  const int rc = ap_bufs_ready(&w->ap);
  if (rc) return rc;
  hipStream_t st = w->stream;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));                          // h_first may still feed an earlier copy
  w->ap.h_first.swap(first);
  PYSDR_HIP_CHECK(hipMemcpyAsync(w->d_llr.get(), llr, (size_t)n * kLdpcN * sizeof(float), hipMemcpyHostToDevice, st));
  ApArgs a{};
  a.llr = w->d_llr.get(); a.n = n;
  return ap_run(w, kLdpcFromBuffer, a, cfg, c, ap, bits);
}

}  // namespace pysdr
