// The pure half of the ordered-statistics decoder behind min-sum: the rule of its setting and the
// pattern count, k <-> (i, j), the rank rule, and the steps the kernel (osd.hip) and the CPU share -- the generator's bit
// in rank order, the pivot search, the row XOR on 6-word rows, a pattern and its distance, the result -- and the scalar
// transcription tests/osd_plan/plan_main.cpp runs on the CPU.  A row is 174 bits in rank order: rank p is bit p % 32 of
// word p / 32.  Plain C++: nothing here calls the HIP runtime.
#pragma once

#include "ldpc_plan.h"

namespace pysdr {

constexpr int kOsdOrderMax = 2;
constexpr int kOsdWords = 6;                          // 174 bits in 32-bit words
constexpr int kOsdThreads = 64;                       // one wavefront per candidate: lane l owns rows l and l + 64
constexpr int kOsdDetailWords = 4;                    // k, last, pattern weight, bits of the float32 distance
constexpr int kOsdPairs = kLdpcK * (kLdpcK - 1) / 2;  // 4095
// sorted magnitudes, keys, permutation; the 91 rows and their pivot ranks; h and e0; the hard bits and the winner's word
constexpr int kOsdLdsBytes = kLdpcN * 4 + kLdpcN * 4 + kLdpcN * 2 + kLdpcK * kOsdWords * 4 + kLdpcK * 2 + 2 * kOsdWords * 4 + 2 * kLdpcN;

// ---- the setting -------------------------------------------------------------------------------------------------------
inline bool osd_cfg_ok(const pysdr_osd_cfg* c) { return c && c->order >= 0 && c->order <= kOsdOrderMax; }
PYSDR_LDPC_HD constexpr int osd_patterns(int order) { return order <= 0 ? 1 : order == 1 ? 1 + kLdpcK : 1 + kLdpcK + kOsdPairs; }

// ---- k <-> (i, j): k = 0 is (-1, -1), k = 1 + i is (i, -1), k = 92 + the place of (i, j), i < j, in lexicographic order
PYSDR_LDPC_HD constexpr int osd_pair_base(int i) { return i * (2 * kLdpcK - 1 - i) / 2; }   // pairs whose first row is below i
PYSDR_LDPC_HD constexpr int osd_k_of(int i, int j) {
  return i < 0 ? 0 : j < 0 ? 1 + i : 1 + kLdpcK + osd_pair_base(i) + (j - i - 1);
}
PYSDR_LDPC_HD inline void osd_ij_of(int k, int* i, int* j) {
  *i = -1; *j = -1;
  if (k <= 0) return;
  if (k <= kLdpcK) { *i = k - 1; return; }
  const int q = k - 1 - kLdpcK;
  int a = 0;
  while (a + 1 < kLdpcK - 1 && osd_pair_base(a + 1) <= q) ++a;
  *i = a; *j = a + 1 + (q - osd_pair_base(a));
}

// ---- steps 1 and 2: the key of a soft bit is the bit pattern of |x|, which orders as the float32 does (and -0 is +0) ------
PYSDR_LDPC_HD inline uint32_t osd_key(float x) {
  uint32_t u;
  __builtin_memcpy(&u, &x, 4);
  return u & 0x7FFFFFFFu;
}
PYSDR_LDPC_HD inline float osd_magnitude(uint32_t key) {
  float r;
  __builtin_memcpy(&r, &key, 4);
  return r;
}
// position a stands before position b: the greater magnitude first, ties by ascending position
PYSDR_LDPC_HD constexpr bool osd_before(uint32_t ka, int a, uint32_t kb, int b) { return ka > kb || (ka == kb && a < b); }

// ---- steps 3 and 4 -----------------------------------------------------------------------------------------------------
// G = [I | P^T]: row i < 91 at codeword position n
PYSDR_LDPC_HD inline uint32_t osd_gen_bit(int i, int n) {
  return n < kLdpcK ? (uint32_t)(n == i) : (kLdpc.gen[n - kLdpcK][i >> 5] >> (31 - (i & 31))) & 1u;
}
PYSDR_LDPC_HD inline uint32_t osd_bit(const uint32_t* row, int p) { return (row[p >> 5] >> (p & 31)) & 1u; }
PYSDR_LDPC_HD inline void osd_row_xor(uint32_t* dst, const uint32_t* src) {
#pragma unroll
  for (int w = 0; w < kOsdWords; ++w) dst[w] ^= src[w];
}
// the pivot search among rows that hold no pivot yet: the lowest row with the rank's bit, or -1
inline int osd_pivot_row(const uint32_t (*rows)[kOsdWords], const int16_t* pivot_of, int p) {
  for (int i = 0; i < kLdpcK; ++i)
    if (pivot_of[i] < 0 && osd_bit(rows[i], p)) return i;
  return -1;
}

// ---- steps 6 to 8 ------------------------------------------------------------------------------------------------------
// g: G' as [91][6], row t has its 1 at rank piv[t]
PYSDR_LDPC_HD inline uint32_t osd_pattern_word(const uint32_t* e0, const uint32_t* g, int i, int j, int w) {
  uint32_t v = e0[w];
  if (i >= 0) v ^= g[i * kOsdWords + w];
  if (j >= 0) v ^= g[j * kOsdWords + w];
  return v;
}
PYSDR_LDPC_HD inline void osd_pattern(const uint32_t* e0, const uint32_t* g, int i, int j, uint32_t* out) {
#pragma unroll
  for (int w = 0; w < kOsdWords; ++w) out[w] = osd_pattern_word(e0, g, i, j, w);
}
// The distances of U patterns at once, each its own chain of adds in rank order; rs: the magnitudes in rank order.
// Adding +0 where the bit is clear changes no sum: every term and every sum is >= +0.
template <int U>
PYSDR_LDPC_HD inline void osd_distances(const uint32_t (*pat)[kOsdWords], const float* rs, float* d) {
#pragma unroll
  for (int u = 0; u < U; ++u) d[u] = 0.f;
#pragma unroll
  for (int w = 0; w < kOsdWords; ++w) {
    const int nb = w + 1 < kOsdWords ? 32 : kLdpcN - 32 * (kOsdWords - 1);
#pragma unroll 8
    for (int b = 0; b < nb; ++b) {
      const float r = rs[32 * w + b];
#pragma unroll
      for (int u = 0; u < U; ++u) d[u] = d[u] + (((pat[u][w] >> b) & 1u) ? r : 0.f);
    }
  }
}
PYSDR_LDPC_HD inline float osd_distance(const uint32_t* pat, const float* rs) {
  uint32_t one[1][kOsdWords];
  float d;
#pragma unroll
  for (int w = 0; w < kOsdWords; ++w) one[0][w] = pat[w];
  osd_distances<1>(one, rs, &d);
  return d;
}
PYSDR_LDPC_HD inline int osd_weight(const uint32_t* pat) {
  int n = 0;
#pragma unroll
  for (int w = 0; w < kOsdWords; ++w) n += __builtin_popcount(pat[w]);
  return n;
}
PYSDR_LDPC_HD constexpr bool osd_better(float d, int k, float bd, int bk) { return d < bd || (d == bd && k < bk); }

// ---- steps 9 to 11: word[174] is the winner in transmission order -----------------------------------------------------------
PYSDR_LDPC_HD inline void osd_result(const uint8_t* word, int k, int last, int weight, float dist, int32_t* status, uint8_t* bits,
                                     int32_t* detail) {
  bool any = false;
  for (int i = 0; i < kLdpcMsg; ++i) any = any || (word[i] & 1);
  if (any && ldpc_crc_matches(word)) {
    for (int b = 0; b < kLdpcBitsBytes; ++b) {
      uint32_t w = 0;
      for (int q = 0; q < 8; ++q) {
        const int i = 8 * b + q;
        w = (w << 1) | (uint32_t)(i < kLdpcK ? (word[i] & 1) : 0);
      }
      bits[b] = (uint8_t)w;
    }
    status[0] = 2; status[2] = weight;
  }
  status[3] = k == 0 ? 1 : k <= kLdpcK ? 2 : 3;
  if (detail) {
    uint32_t u;
    __builtin_memcpy(&u, &dist, 4);
    detail[0] = k; detail[1] = last; detail[2] = weight; detail[3] = (int32_t)u;
  }
}
PYSDR_LDPC_HD inline void osd_not_run(int32_t* detail) {
  if (detail) { detail[0] = -1; detail[1] = -1; detail[2] = -1; detail[3] = 0; }
}

// The scalar transcription: one candidate behind its min-sum result (status[4], bits[12]), llr[174] positive for bit 1.
inline void osd_decode_scalar(const float* llr, int order, int32_t* status, uint8_t* bits, int32_t* detail) {
  if (status[0] == 2) { osd_not_run(detail); return; }
  uint32_t key[kLdpcN];
  int perm[kLdpcN];
  float rs[kLdpcN];
  for (int n = 0; n < kLdpcN; ++n) key[n] = osd_key(llr[n]);
  for (int n = 0; n < kLdpcN; ++n) {
    int rank = 0;
    for (int m = 0; m < kLdpcN; ++m) rank += osd_before(key[m], m, key[n], n) ? 1 : 0;
    perm[rank] = n;
  }
  uint32_t h[kOsdWords] = {};
  for (int p = 0; p < kLdpcN; ++p) {
    rs[p] = osd_magnitude(key[perm[p]]);
    if (llr[perm[p]] > 0.f) h[p >> 5] |= 1u << (p & 31);
  }
  uint32_t rows[kLdpcK][kOsdWords] = {};
  for (int i = 0; i < kLdpcK; ++i)
    for (int p = 0; p < kLdpcN; ++p) rows[i][p >> 5] |= osd_gen_bit(i, perm[p]) << (p & 31);
  int16_t pivot_of[kLdpcK];                                  // row -> its place t among the pivots, or -1
  int piv[kLdpcK];
  for (int i = 0; i < kLdpcK; ++i) pivot_of[i] = -1;
  int kept = 0;
  for (int p = 0; p < kLdpcN && kept < kLdpcK; ++p) {
    const int row = osd_pivot_row(rows, pivot_of, p);
    if (row < 0) continue;
    for (int i = 0; i < kLdpcK; ++i)
      if (i != row && osd_bit(rows[i], p)) osd_row_xor(rows[i], rows[row]);
    pivot_of[row] = (int16_t)kept;
    piv[kept++] = p;
  }
  uint32_t g[kLdpcK * kOsdWords], e0[kOsdWords];
  for (int i = 0; i < kLdpcK; ++i)
    for (int w = 0; w < kOsdWords; ++w) g[pivot_of[i] * kOsdWords + w] = rows[i][w];
  for (int w = 0; w < kOsdWords; ++w) e0[w] = h[w];
  for (int t = 0; t < kLdpcK; ++t)
    if (osd_bit(h, piv[t])) osd_row_xor(e0, g + t * kOsdWords);
  int bk = -1;
  float bd = 0.f;
  uint32_t best[kOsdWords] = {};
  const int np = osd_patterns(order);
  for (int k = 0; k < np; ++k) {
    int i, j;
    uint32_t pat[kOsdWords];
    osd_ij_of(k, &i, &j);
    osd_pattern(e0, g, i, j, pat);
    const float d = osd_distance(pat, rs);
    if (bk < 0 || osd_better(d, k, bd, bk)) {
      bd = d; bk = k;
      for (int w = 0; w < kOsdWords; ++w) best[w] = pat[w];
    }
  }
  uint8_t word[kLdpcN];
  for (int p = 0; p < kLdpcN; ++p) word[perm[p]] = (uint8_t)(osd_bit(h, p) ^ osd_bit(best, p));
  osd_result(word, bk, piv[kLdpcK - 1], osd_weight(best), bd, status, bits, detail);
}

// ---- kernel arguments and the launch (osd.hip): the candidates and soft bits of the min-sum launch before it --------------------
struct OsdArgs {
  const float* llr;        // kLdpcFromBuffer: [n][174]
  const float* ring;       // the ring sources, as LdpcArgs
  int tr, nb, nsub;
  const int32_t* cand;
  int n, order;
  int32_t* status;         // [n][4], min-sum's: read first, then updated
  uint8_t* bits;           // [n][12]
  int32_t* detail;         // [n][4] or NULL
};

}  // namespace pysdr
