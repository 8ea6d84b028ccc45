// The pure half of a-priori decoding: the rules of the settings, of a hypothesis table and of a pair
// list with its offsets first[n + 1]; the clamp; the counting of nerr and nap; a pair's status; the pick among a
// candidate's pairs; and the scalar transcription over ldpc_plan.h's decoder -- the very code the kernels (ap.hip) step
// with, the host half (ap_host.h) checks with and tests/ap_plan/plan_main.cpp runs on the CPU.  A hypothesis is two words
// of 12 bytes, mask then value, packed as the decoder packs `bits`: message bit i is bit 7 - (i & 7) of byte i >> 3.
// Plain C++: nothing here calls the HIP runtime.
#pragma once

#include "ldpc_plan.h"

namespace pysdr {

constexpr int kApHypMax = 4096;            // hypotheses of one call's table
constexpr int kApPairMax = 65536;          // pairs (candidate, hypothesis) of one call
constexpr int kApWordBytes = kLdpcBitsBytes;       // a mask or a value
constexpr int kApHypBytes = 2 * kApWordBytes;      // mask, then value
constexpr int kApWords = 4;                // ap[n][4]: pair or -1, iterations, nerr, pairs of status 2
constexpr int kApDetailWords = 4;          // detail[P][4]: status, iterations, nerr, nap
constexpr int kApPickThreads = 64;         // one thread per candidate
constexpr float kApMagMin = 0.25f, kApMagMax = 16.f;
constexpr int kApLdsBytes = kLdpcLdsBytes + 3 * 4 + 4;   // the decoder's, the three wavefronts' maxima and nap

// ---- settings, hypotheses, pairs ---------------------------------------------------------------------------------------
inline bool ap_cfg_ok(const pysdr_ap_cfg* c) {
  if (!c) return false;
  if (!(c->mag >= kApMagMin && c->mag <= kApMagMax)) return false;     // finite; a NaN fails both
  return c->nerr_max >= 0 && c->nerr_max <= kLdpcN;
}
constexpr bool ap_hyps_n_ok(long long H) { return H >= 1 && H <= kApHypMax; }
constexpr bool ap_pairs_n_ok(long long P) { return P >= 0 && P <= kApPairMax; }

PYSDR_LDPC_HD inline int ap_bit(const uint8_t* word, int i) { return (word[i >> 3] >> (7 - (i & 7))) & 1; }

// h: mask[12] then value[12].  Only bits 0 .. 76 in the mask, a mask that is not empty, no value bit outside the mask.
inline bool ap_hyp_ok(const uint8_t* h) {
  const uint8_t* mask = h;
  const uint8_t* value = h + kApWordBytes;
  if ((mask[9] & 0x07) || mask[10] || mask[11]) return false;         // bits 77 .. 95
  bool any = false;
  for (int b = 0; b < kApWordBytes; ++b) {
    any = any || mask[b];
    if (value[b] & (uint8_t)~mask[b]) return false;
  }
  return any;
}
// the first hypothesis outside the rule, or -1
inline int ap_first_bad_hyp(const uint8_t* hyps, int H) {
  for (int h = 0; h < H; ++h)
    if (!ap_hyp_ok(hyps + (size_t)h * kApHypBytes)) return h;
  return -1;
}
// pairs[P][2] = (candidate, hypothesis), strictly increasing, candidate in [0, n), hypothesis in [0, H): the first pair
// outside the rule, or -1 -- and then first[c] .. first[c + 1] are candidate c's pairs, first[n] = P.
inline int ap_first_bad_pair(const int32_t* pairs, int P, int n, int H, int32_t* first) {
  for (int p = 0; p < P; ++p) {
    const int32_t c = pairs[2 * p], h = pairs[2 * p + 1];
    if (c < 0 || c >= n || h < 0 || h >= H) return p;
    if (p > 0 && !(pairs[2 * p - 2] < c || (pairs[2 * p - 2] == c && pairs[2 * p - 1] < h))) return p;
  }
  int p = 0;
  for (int c = 0; c < n; ++c) {
    first[c] = p;
    while (p < P && pairs[2 * p] == c) ++p;
  }
  first[n] = P;
  return -1;
}

// ---- per pair ------------------------------------------------------------------------------------------------------------
PYSDR_LDPC_HD inline bool ap_masked(const uint8_t* hyp, int k) { return k < kLdpcMsg && ap_bit(hyp, k) != 0; }
PYSDR_LDPC_HD inline float ap_amp(float mag, float amax) { return mag * amax; }
// soft bit k under the hypothesis: +A for a hypothesised 1, -A for a 0 (so -0 where A is 0), its own value outside the mask
PYSDR_LDPC_HD inline float ap_clamp(float llr, float A, const uint8_t* hyp, int k) {
  if (!ap_masked(hyp, k)) return llr;
  return ap_bit(hyp + kApWordBytes, k) ? A : -A;
}
// what position k adds to nerr (outside the mask: llr > 0 differs from the final hard bit) and to nap (inside it: the
// final hard bit differs from the value)
PYSDR_LDPC_HD inline void ap_count(float llr, bool hard, const uint8_t* hyp, int k, bool* err, bool* miss) {
  const bool in = ap_masked(hyp, k);
  *err = !in && ((llr > 0.f) != hard);
  *miss = in && ((ap_bit(hyp + kApWordBytes, k) != 0) != hard);
}
// st: the decoder's status of the clamped word (ldpc_result)
PYSDR_LDPC_HD constexpr int ap_status(int st, int nerr, int nap, int nerr_max) {
  return st == 2 && nap == 0 && nerr <= nerr_max ? 2 : (st >= 1 ? 1 : 0);
}

// ---- per candidate: among its pairs lo .. hi - 1 of status 2 the least nerr, ties to the lower pair ---------------------------
PYSDR_LDPC_HD inline void ap_pick(const int32_t* detail, const uint8_t* pbits, int lo, int hi, int32_t* ap, uint8_t* bits) {
  int best = -1, count = 0;
  for (int p = lo; p < hi; ++p) {
    if (detail[(size_t)p * kApDetailWords] != 2) continue;
    ++count;
    if (best < 0 || detail[(size_t)p * kApDetailWords + 2] < detail[(size_t)best * kApDetailWords + 2]) best = p;
  }
  ap[0] = best;
  ap[1] = best < 0 ? 0 : detail[(size_t)best * kApDetailWords + 1];
  ap[2] = best < 0 ? 0 : detail[(size_t)best * kApDetailWords + 2];
  ap[3] = count;
  for (int b = 0; b < kLdpcBitsBytes; ++b) bits[b] = best < 0 ? (uint8_t)0 : pbits[(size_t)best * kLdpcBitsBytes + b];
}

// The scalar transcription of one pair: llr[174] positive for bit 1, hyp = mask then value.
inline void ap_decode_scalar(const float* llr, const uint8_t* hyp, float mag, int nerr_max, int iters, float alpha, int32_t* detail,
                             uint8_t* bits) {
  float amax = 0.f;
  for (int k = 0; k < kLdpcN; ++k) amax = fabsf(llr[k]) > amax ? fabsf(llr[k]) : amax;
  const float A = ap_amp(mag, amax);
  float x[kLdpcN], post[kLdpcN];
  for (int k = 0; k < kLdpcN; ++k) x[k] = ap_clamp(llr[k], A, hyp, k);
  int32_t st[kLdpcStatusWords];
  ldpc_decode_scalar(x, iters, alpha, st, bits, post);
  int nerr = 0, nap = 0;
  for (int k = 0; k < kLdpcN; ++k) {
    bool err, miss;
    ap_count(llr[k], post[k] < 0.f, hyp, k, &err, &miss);
    nerr += err ? 1 : 0;
    nap += miss ? 1 : 0;
  }
  detail[0] = ap_status(st[0], nerr, nap, nerr_max); detail[1] = st[1]; detail[2] = nerr; detail[3] = nap;
}

// ---- kernel arguments and the launch (ap.hip); the sources of soft bits are ft_plan.h's LdpcSource ---------------------------
struct ApArgs {
  const float* llr;        // kLdpcFromBuffer: [n][174]
  const float* ring;       // the ring sources, as LdpcArgs
  int tr, nb, nsub;
  const int32_t* cand;     // [n][2]
  int n, npairs, iters;
  float alpha, mag;
  int nerr_max;
  const uint8_t* hyps;     // [H][24]
  const int32_t* pairs;    // [P][2]
  const int32_t* first;    // [n + 1]
  int32_t* detail;         // [P][4]
  uint8_t* pbits;          // [P][12]
  int32_t* ap;             // [n][4]
  uint8_t* bits;           // [n][12]
};

}  // namespace pysdr
