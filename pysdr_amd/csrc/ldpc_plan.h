// The pure half of the LDPC(174,91) decoder: the generator rows and the sparse parity checks as the
// protocol gives them, parsed at compile time into the tables of both directions (check -> columns, column -> its three
// edges); CRC-14; the rules of the settings and of a call's arguments; and the decoder itself, step by step -- the very
// code the kernel (ldpc.hip) steps with, the host half (ldpc_host.h) checks with and tests/ldpc_plan/plan_main.cpp runs on
// the CPU as a scalar transcription.  Plain C++: nothing here calls the HIP runtime.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/pysdr_hip.h"
#include "ft_plan.h"

#if defined(__HIPCC__)
#define PYSDR_LDPC_HD __host__ __device__
#else
#define PYSDR_LDPC_HD
#endif

namespace pysdr {

constexpr int kLdpcN = 174;                // codeword bits, in transmission order
constexpr int kLdpcK = 91;                 // systematic bits: 77 of the message, 14 of the CRC
constexpr int kLdpcM = 83;                 // parity bits, and sparse checks
constexpr int kLdpcMsg = 77;
constexpr int kLdpcCrcBits = 14;
constexpr uint32_t kLdpcCrcPoly = 0x2757;  // x^14 + these terms
constexpr int kLdpcEdges = 522;            // 59 checks of degree 6 and 24 of degree 7; every column in 3 checks
constexpr int kLdpcDegMax = 7;
constexpr int kLdpcColDeg = 3;
constexpr int kLdpcItersMax = 200;
constexpr int kLdpcMax = 4096;             // candidates of one call
constexpr int kLdpcThreads = 192;          // one workgroup per candidate: thread n < 174 owns a variable, m < 83 a check
constexpr int kLdpcStatusWords = 4;        // status, iterations, nerr, 0
constexpr int kLdpcBitsBytes = 12;         // the 91 systematic hard bits, MSB first, 5 bits of padding
constexpr int kLdpcLdsBytes = 2 * kLdpcEdges * 4 + (kLdpcN + 2) + 3 * 4;   // c, v; the hard bits; two vote flags, nerr

// Parity bit j (codeword bit 91 + j) is the XOR of the message bits i < 91 whose bit is set in row j: a row's 23 hex digits
// are a 92-bit number whose lowest bit is dropped; the remaining 91, most significant first, are i = 0 .. 90.
constexpr char kLdpcGenText[] =
    "8329ce11bf31eaf509f27fc 761c264e25c259335493132 dc265902fb277c6410a1bdc 1b3f417858cd2dd33ec7f62 "
    "09fda4fee04195fd034783a 077cccc11b8873ed5c3d48a 29b62afe3ca036f4fe1a9da 6054faf5f35d96d3b0c8c3e "
    "e20798e4310eed27884ae90 775c9c08e80e26ddae56318 b0b811028c2bf997213487c 18a0c9231fc60adf5c5ea32 "
    "76471e8302a0721e01b12b8 ffbccb80ca8341fafb47b2e 66a72a158f9325a2bf67170 c4243689fe85b1c51363a18 "
    "0dff739414d1a1b34b1c270 15b48830636c8b99894972e 29a89c0d3de81d665489b0e 4f126f37fa51cbe61bd6b94 "
    "99c47239d0d97d3c84e0940 1919b75119765621bb4f1e8 09db12d731faee0b86df6b8 488fc33df43fbdeea4eafb4 "
    "827423ee40b675f756eb5fe abe197c484cb74757144a9a 2b500e4bc0ec5a6d2bdbdd0 c474aa53d70218761669360 "
    "8eba1a13db3390bd6718cec 753844673a27782cc42012e 06ff83a145c37035a5c1268 3b37417858cc2dd33ec3f62 "
    "9a4a5a28ee17ca9c324842c bc29f465309c977e89610a4 2663ae6ddf8b5ce2bb29488 46f231efe457034c1814418 "
    "3fb2ce85abe9b0c72e06fbe de87481f282c153971a0a2e fcd7ccf23c69fa99bba1412 f0261447e9490ca8e474cec "
    "4410115818196f95cdd7012 088fc31df4bfbde2a4eafb4 b8fef1b6307729fb0a078c0 5afea7acccb77bbc9d99a90 "
    "49a7016ac653f65ecdc9076 1944d085be4e7da8d6cc7d0 251f62adc4032f0ee714002 56471f8702a0721e00b12b8 "
    "2b8e4923f2dd51e2d537fa0 6b550a40a66f4755de95c26 a18ad28d4e27fe92a4f6c84 10c2e586388cb82a3d80758 "
    "ef34a41817ee02133db2eb0 7e9c0c54325a9c15836e000 3693e572d1fde4cdf079e86 bfb2cec5abe1b0c72e07fbe "
    "7ee18230c583cccc57d4b08 a066cb2fedafc9f52664126 bb23725abc47cc5f4cc4cd2 ded9dba3bee40c59b5609b4 "
    "d9a7016ac653e6decdc9036 9ad46aed5f707f280ab5fc4 e5921c77822587316d7d3c2 4f14da8242a8b86dca73352 "
    "8b8b507ad467d4441df770e 22831c9cf1169467ad04b68 213b838fe2ae54c38ee7180 5d926b6dd71f085181a4e12 "
    "66ab79d4b29ee6e69509e56 958148682d748a38dd68baa b8ce020cf069c32a723ab14 f4331d6d461607e95752746 "
    "6da23ba424b9596133cf9c8 a636bcbc7b30c5fbeae67fe 5cb0d86a07df654a9089a20 f11f106848780fc9ecdd80a "
    "1fbb5364fb8d2c9d730d5ba fcb86bc70a50c9d02a5d034 a534433029eac15f322e34c c989d9c7c3d3b8c55d75130 "
    "7bb38b2f0186d46643ae962 2644ebadeb44b9467d1f42c 608cc857594bfbb55d69600";

// The sparse checks: all words of weight at most 7 in the dual code, as ascending column tuples, sorted ascending.  Check
// m is row m; edge numbers run row-major over this list.
constexpr char kLdpcCheckText[] =
    "0 3 51 56 85 135 151; 0 25 44 79 127 146; 0 32 71 105 106 156; 1 26 40 60 61 114 132; 1 47 73 112 127 159; "
    "1 53 85 100 134 163; 2 12 47 77 94 122; 2 23 29 71 103 138; 2 43 79 123 126 168; 3 28 67 119 133 172; "
    "3 30 58 90 91 95 152; 4 31 59 92 114 145; 4 33 64 77 97 106 153; 4 38 74 101 135 166; 5 23 60 93 121 150; "
    "5 31 63 96 125 137; 5 32 84 107 115 155; 6 32 61 94 95 142; 6 48 57 89 99 104 167; 6 49 80 98 131 172; "
    "7 24 62 82 92 95 147; 7 39 69 81 103 113 144; 7 45 70 111 118 165; 8 34 65 98 138 145; 8 39 89 105 133 150; "
    "8 53 62 130 146 154; 9 35 66 99 106 125; 9 43 81 90 110 143 148; 9 52 65 83 111 127 164; 10 36 66 86 100 138 157; "
    "10 43 74 109 120 165; 10 48 87 91 141 156; 11 37 67 101 104 154; 11 42 65 88 96 134 158; 11 49 60 117 118 143; "
    "12 38 68 102 148 161; 12 50 63 113 117 156; 13 29 82 112 124 169; 13 30 78 97 131 163; 13 40 70 87 101 122 155; "
    "14 41 58 105 122 158; 14 55 86 107 118 170; 14 57 59 73 110 149 162; 15 38 61 111 133 157; 15 42 72 107 140 159; "
    "15 46 75 129 136 153; 16 26 88 102 115 152; 16 36 73 80 108 130 153; 16 41 74 128 169 171; 17 35 75 88 112 113 142; "
    "17 41 78 143 145 151; 17 48 54 123 140 166; 18 34 58 72 109 124 160; 18 37 76 103 115 162; 18 45 80 116 134 166; "
    "19 35 62 93 135 160; 19 45 64 79 119 139 169; 19 46 69 91 137 164; 20 36 72 137 151 168; 20 44 77 82 116 120 150; "
    "20 53 76 99 139 170; 21 46 57 117 126 163; 21 52 67 108 120 173; 21 56 84 92 139 158; 22 33 70 93 126 152; "
    "22 42 78 119 130 144; 22 54 66 94 171 173; 23 51 75 128 147 148; 24 37 64 98 121 159; 24 52 68 89 100 129 155; "
    "25 40 76 108 140 147; 25 50 55 90 121 136 167; 26 39 55 123 124 125; 27 28 83 87 116 142 149; 27 31 71 102 131 165; "
    "27 47 69 84 104 128 157; 28 33 86 96 146 161; 29 49 59 85 136 141 161; 30 68 132 149 154 168; 34 81 132 141 170 173; "
    "44 54 63 110 129 160 172; 50 56 97 162 164 171; 51 83 109 114 144 167";

struct LdpcTables {
  int16_t col[kLdpcM][kLdpcDegMax];        // check -> its columns, ascending; -1 beyond its degree
  int16_t deg[kLdpcM];                     // 6 or 7
  int16_t base[kLdpcM];                    // check -> its first edge
  int16_t edge[kLdpcN][kLdpcColDeg];       // column -> its three edges, in ascending check order
  int16_t ncol[kLdpcN];                    // checks a column is in: 3
  uint32_t gen[kLdpcM][3];                 // parity row j: message bit i < 91 is bit 31 - i % 32 of word i / 32
  int nedges;
  bool ok;                                 // both texts parsed to the end, in order, and every count is what it must be
};

constexpr LdpcTables ldpc_make_tables() {
  LdpcTables t{};
  t.ok = true;
  // the generator: 83 words of 23 hex digits
  int at = 0;
  for (int j = 0; j < kLdpcM; ++j) {
    uint8_t nib[23] = {};
    for (int d = 0; d < 23; ++d) {
      const char ch = kLdpcGenText[at++];
      if (ch >= '0' && ch <= '9') nib[d] = (uint8_t)(ch - '0');
      else if (ch >= 'a' && ch <= 'f') nib[d] = (uint8_t)(ch - 'a' + 10);
      else t.ok = false;
    }
    for (int i = 0; i < kLdpcK; ++i)                                  // bit i of the 92, most significant first
      if ((nib[i / 4] >> (3 - i % 4)) & 1) t.gen[j][i / 32] |= 1u << (31 - i % 32);
    const char sep = kLdpcGenText[at++];
    if (sep != (j + 1 < kLdpcM ? ' ' : '\0')) t.ok = false;
  }
  // the checks: rows of ascending columns
  for (int m = 0; m < kLdpcM; ++m)
    for (int k = 0; k < kLdpcDegMax; ++k) t.col[m][k] = -1;
  at = 0;
  int e = 0;
  for (int m = 0; m < kLdpcM; ++m) {
    t.base[m] = (int16_t)e;
    int d = 0;
    for (;;) {
      int v = 0, digits = 0;
      while (kLdpcCheckText[at] >= '0' && kLdpcCheckText[at] <= '9') { v = 10 * v + (kLdpcCheckText[at++] - '0'); ++digits; }
      if (!digits || v >= kLdpcN || d >= kLdpcDegMax || (d > 0 && v <= t.col[m][d - 1])) { t.ok = false; break; }
      t.col[m][d++] = (int16_t)v;
      if (t.ncol[v] < kLdpcColDeg) t.edge[v][t.ncol[v]] = (int16_t)e;
      ++t.ncol[v];
      ++e;
      if (kLdpcCheckText[at] == ' ' && kLdpcCheckText[at + 1] >= '0' && kLdpcCheckText[at + 1] <= '9') { ++at; continue; }
      break;
    }
    t.deg[m] = (int16_t)d;
    if (d < 6) t.ok = false;
    if (m + 1 < kLdpcM) {
      if (kLdpcCheckText[at] == ';' && kLdpcCheckText[at + 1] == ' ') at += 2;
      else t.ok = false;
    } else if (kLdpcCheckText[at] != '\0') t.ok = false;
    if (!t.ok) break;
  }
  t.nedges = e;
  if (e != kLdpcEdges) t.ok = false;
  for (int n = 0; n < kLdpcN; ++n)
    if (t.ncol[n] != kLdpcColDeg) t.ok = false;
  return t;
}

inline constexpr LdpcTables kLdpc = ldpc_make_tables();
static_assert(kLdpc.ok, "the LDPC tables: 83 generator rows, 83 checks of 6 or 7 ascending columns, 522 edges, every column in 3 checks");

// ---- settings and arguments ------------------------------------------------------------------------------------------
inline bool ldpc_cfg_ok(const pysdr_ldpc_cfg* c) {
  if (!c) return false;
  if (c->iters < 1 || c->iters > kLdpcItersMax) return false;
  return c->alpha > 0.f && c->alpha <= 1.f;                           // finite; a NaN fails both
}
constexpr bool ldpc_n_ok(long long n) { return n >= 0 && n <= kLdpcMax; }
// every soft bit finite: the first index that is not, or -1
inline long long ldpc_first_nonfinite(const float* llr, size_t count) {
  for (size_t i = 0; i < count; ++i)
    if (!(llr[i] >= -FLT_MAX && llr[i] <= FLT_MAX)) return (long long)i;
  return -1;
}

// ---- CRC-14 and the generator ----------------------------------------------------------------------------------------
// Over 82 bits, MSB first: the 77 message bits and five zeros; zero initial value, no reflection, no final XOR.
PYSDR_LDPC_HD inline uint32_t ldpc_crc14(const uint8_t* bits77) {
  uint32_t r = 0;
  for (int i = 0; i < kLdpcMsg + 5; ++i) {
    const uint32_t b = i < kLdpcMsg ? (uint32_t)(bits77[i] & 1) : 0u;
    const uint32_t top = ((r >> 13) & 1u) ^ b;
    r = (r << 1) & 0x3FFFu;
    if (top) r ^= kLdpcCrcPoly;
  }
  return r;
}
// the CRC of a word's first 77 bits equals its bits 77 .. 90, most significant first
PYSDR_LDPC_HD inline bool ldpc_crc_matches(const uint8_t* bits91) {
  uint32_t got = 0;
  for (int i = 0; i < kLdpcCrcBits; ++i) got = (got << 1) | (uint32_t)(bits91[kLdpcMsg + i] & 1);
  return got == ldpc_crc14(bits91);
}
// 91 systematic bits -> the codeword's 174
inline void ldpc_encode91(const uint8_t* bits91, uint8_t* out174) {
  for (int i = 0; i < kLdpcK; ++i) out174[i] = bits91[i] & 1;
  for (int j = 0; j < kLdpcM; ++j) {
    int p = 0;
    for (int i = 0; i < kLdpcK; ++i)
      if ((kLdpc.gen[j][i / 32] >> (31 - i % 32)) & 1u) p ^= bits91[i] & 1;
    out174[kLdpcK + j] = (uint8_t)p;
  }
}

// ---- the decoder's steps -----------------------------------------------------------------------
// L = -llr is positive for bit 0.  Every float operation rounds on its own (-ffp-contract=off).
// Steps 1 and 5 for one variable: tot and the three messages v to its checks, each the sum of L and the two other
// incoming messages in ascending check order.
PYSDR_LDPC_HD inline float ldpc_variable(float L, float c0, float c1, float c2, float* v0, float* v1, float* v2) {
  const float l0 = L + c0;
  *v0 = (L + c1) + c2;
  *v1 = l0 + c2;
  *v2 = l0 + c1;
  return (l0 + c1) + c2;
}
// Step 6 for one check of `deg` edges, v -> c in place order: c[e] = s f32(alpha min |v| over the other edges), s the
// product of the other edges' signs (v < 0 is negative; +0 and -0 are positive), applied by negation -- so a zero minimum
// under a negative sign gives -0.  The minimum over the others is the check's least |v|, or its second least for the
// edge that holds the least (the first such edge; with a tie both are equal).
PYSDR_LDPC_HD inline void ldpc_check(const float* v, int deg, float alpha, float* c) {
  float m1 = fabsf(v[0]), m2 = 0.f;
  int at = 0;
  bool have2 = false, odd = v[0] < 0.f;
#pragma unroll
  for (int k = 1; k < kLdpcDegMax; ++k) {
    if (k < deg) {
      const float a = fabsf(v[k]);
      odd ^= v[k] < 0.f;
      if (a < m1) { m2 = m1; have2 = true; m1 = a; at = k; }
      else if (!have2 || a < m2) { m2 = a; have2 = true; }
    }
  }
  const float s1 = alpha * m1, s2 = alpha * m2;
#pragma unroll
  for (int k = 0; k < kLdpcDegMax; ++k) {
    if (k < deg) {
      const float mag = k == at ? s2 : s1;
      const bool neg = odd ^ (v[k] < 0.f);
      c[k] = neg ? -mag : mag;
    }
  }
}
// The result of a candidate from its final hard bits: status 2 for a codeword whose CRC matches and whose 77 message bits
// are not all zero, 1 for any other codeword, 0 for none; the first 91 hard bits packed MSB first.
PYSDR_LDPC_HD inline void ldpc_result(const uint8_t* hard, bool codeword, int iterations, int nerr, int32_t* status, uint8_t* bits) {
  for (int b = 0; b < kLdpcBitsBytes; ++b) {
    uint32_t w = 0;
    for (int k = 0; k < 8; ++k) {
      const int i = 8 * b + k;
      w = (w << 1) | (uint32_t)(i < kLdpcK ? (hard[i] & 1) : 0);
    }
    bits[b] = (uint8_t)w;
  }
  int st = 0;
  if (codeword) {
    bool any = false;
    for (int i = 0; i < kLdpcMsg; ++i) any = any || (hard[i] & 1);
    st = any && ldpc_crc_matches(hard) ? 2 : 1;
  }
  status[0] = st; status[1] = iterations; status[2] = nerr; status[3] = 0;
}

// The scalar transcription: one candidate, llr[174] positive for bit 1.
inline void ldpc_decode_scalar(const float* llr, int iters, float alpha, int32_t* status, uint8_t* bits, float* post) {
  float L[kLdpcN], c[kLdpcEdges], v[kLdpcEdges], tot[kLdpcN];
  uint8_t hard[kLdpcN];
  for (int n = 0; n < kLdpcN; ++n) L[n] = -llr[n];
  for (int e = 0; e < kLdpcEdges; ++e) c[e] = 0.f;
  bool codeword = false;
  int k = 0;
  for (;; ++k) {
    for (int n = 0; n < kLdpcN; ++n) {
      const int16_t* e = kLdpc.edge[n];
      tot[n] = ldpc_variable(L[n], c[e[0]], c[e[1]], c[e[2]], &v[e[0]], &v[e[1]], &v[e[2]]);
      hard[n] = tot[n] < 0.f ? 1 : 0;
    }
    bool odd = false;
    for (int m = 0; m < kLdpcM; ++m) {
      int p = 0;
      for (int d = 0; d < kLdpc.deg[m]; ++d) p ^= hard[kLdpc.col[m][d]];
      odd = odd || p;
    }
    if (!odd) { codeword = true; break; }
    if (k == iters) break;
    for (int m = 0; m < kLdpcM; ++m) ldpc_check(&v[kLdpc.base[m]], kLdpc.deg[m], alpha, &c[kLdpc.base[m]]);
  }
  int nerr = 0;
  for (int n = 0; n < kLdpcN; ++n) nerr += ((llr[n] > 0.f) != (hard[n] != 0)) ? 1 : 0;
  ldpc_result(hard, codeword, k, nerr, status, bits);
  if (post)
    for (int n = 0; n < kLdpcN; ++n) post[n] = tot[n];
}

// ---- kernel arguments and the launch (ldpc.hip); the sources of soft bits are ft_plan.h's LdpcSource -------------------
struct LdpcArgs {
  const float* llr;        // kLdpcFromBuffer: [n][174]
  const float* ring;       // the ring sources: the skimmer's spectrum ring [nk][tr][nb] ...
  int tr, nb, nsub;
  const int32_t* cand;     // ... and [n][2]: fine row F, slot0 = t0 mod tr
  int n, iters;
  float alpha;
  int32_t* status;         // [n][4]
  uint8_t* bits;           // [n][12]
  float* post;             // [n][174] or NULL
};

}  // namespace pysdr
