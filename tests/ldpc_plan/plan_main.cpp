// The pure half of the LDPC(174,91) decoder (pysdr_amd/csrc/ldpc_plan.h, the very code ldpc.hip steps with) on the CPU
// under AddressSanitizer + UBSan.
//   * the tables: the two directions (check -> columns, column -> its three edges) are inverses of each other, a column's
//     edges are in ascending check order, every column has weight 3, 59 checks have degree 6 and 24 degree 7.
//   * H annihilates the codeword of each of the 91 unit messages, and of random messages.
//   * CRC-14 of fixed and random vectors against a bit-serial long division of the 96-bit augmented word.
//   * every refusal of the settings, of n and of soft bits that are not finite.
//   * the check update (ldpc_check) against a direct transcription -- the minimum and the sign product over the other
//     edges, edge by edge -- bit for bit, with ties, zeros and -0 among the inputs.
//   * the scalar decoder: noise-free words stop at k = 0 with status 2; flipped strong bits are corrected and counted; a
//     broken CRC and the zero word give status 1; noise gives no status 2; the iteration limit is kept.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "ldpc_plan.h"

using namespace pysdr;

#define REQUIRE(c, ...) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static unsigned g_rng = 174u;
static unsigned rnd_u() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }
static float rnd() { return (float)((int)rnd_u() - (1 << 23)) / (float)(1 << 23); }
static uint32_t fbits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }

static bool parity_ok(const uint8_t* w) {
  for (int m = 0; m < kLdpcM; ++m) {
    int p = 0;
    for (int d = 0; d < kLdpc.deg[m]; ++d) p ^= w[kLdpc.col[m][d]];
    if (p) return false;
  }
  return true;
}

// the remainder of (82 bits, then 14 zeros) divided by x^14 + 0x2757, one bit at a time
static uint32_t crc_by_division(const uint8_t* bits77) {
  uint8_t w[96] = {};
  for (int i = 0; i < 77; ++i) w[i] = bits77[i] & 1;
  const uint32_t poly = (1u << 14) | kLdpcCrcPoly;                   // 15 bits
  for (int i = 0; i + 15 <= 96; ++i)
    if (w[i])
      for (int k = 0; k < 15; ++k) w[i + k] ^= (uint8_t)((poly >> (14 - k)) & 1u);
  uint32_t r = 0;
  for (int i = 82; i < 96; ++i) r = (r << 1) | w[i];
  return r;
}

static void random_message(uint8_t* bits91) {
  for (int i = 0; i < kLdpcMsg; ++i) bits91[i] = (uint8_t)(rnd_u() & 1);
  const uint32_t c = ldpc_crc14(bits91);
  for (int i = 0; i < kLdpcCrcBits; ++i) bits91[kLdpcMsg + i] = (uint8_t)((c >> (13 - i)) & 1);
}

static void plain_check(const float* v, int deg, float alpha, float* c) {
  for (int k = 0; k < deg; ++k) {
    float mn = 0.f;
    bool first = true, neg = false;
    for (int o = 0; o < deg; ++o) {
      if (o == k) continue;
      const float a = std::fabs(v[o]);
      if (first || a < mn) mn = a;
      first = false;
      if (v[o] < 0.f) neg = !neg;
    }
    const float mag = alpha * mn;
    c[k] = neg ? -mag : mag;
  }
}

int main() {
  // ---- the tables
  int n6 = 0, n7 = 0, e = 0;
  for (int m = 0; m < kLdpcM; ++m) {
    REQUIRE(kLdpc.deg[m] == 6 || kLdpc.deg[m] == 7, "check %d degree %d", m, kLdpc.deg[m]);
    (kLdpc.deg[m] == 6 ? n6 : n7) += 1;
    REQUIRE(kLdpc.base[m] == e, "check %d base", m);
    for (int d = 0; d < kLdpcDegMax; ++d) {
      const int n = kLdpc.col[m][d];
      if (d >= kLdpc.deg[m]) { REQUIRE(n == -1, "padding"); continue; }
      REQUIRE(n >= 0 && n < kLdpcN && (d == 0 || n > kLdpc.col[m][d - 1]), "check %d column %d", m, d);
      int hits = 0;
      for (int s = 0; s < kLdpcColDeg; ++s) hits += kLdpc.edge[n][s] == e ? 1 : 0;
      REQUIRE(hits == 1, "edge %d of check %d is not among column %d's", e, m, n);
      ++e;
    }
  }
  REQUIRE(e == kLdpcEdges && kLdpc.nedges == kLdpcEdges && n6 == 59 && n7 == 24, "%d edges, %d + %d checks", e, n6, n7);
  for (int n = 0; n < kLdpcN; ++n) {
    REQUIRE(kLdpc.ncol[n] == 3, "column %d weight %d", n, kLdpc.ncol[n]);
    int last = -1;
    for (int s = 0; s < kLdpcColDeg; ++s) {
      const int ed = kLdpc.edge[n][s];
      REQUIRE(ed >= 0 && ed < kLdpcEdges, "edge");
      int m = 0;
      while (m + 1 < kLdpcM && kLdpc.base[m + 1] <= ed) ++m;
      REQUIRE(ed - kLdpc.base[m] < kLdpc.deg[m] && kLdpc.col[m][ed - kLdpc.base[m]] == n, "column %d edge %d is not check %d's", n, ed, m);
      REQUIRE(m > last, "column %d: checks not ascending", n);
      last = m;
    }
  }

  // ---- H annihilates the code
  std::vector<uint8_t> cw(kLdpcN);
  uint8_t msg[kLdpcK];
  for (int i = 0; i < kLdpcK; ++i) {
    memset(msg, 0, sizeof msg);
    msg[i] = 1;
    ldpc_encode91(msg, cw.data());
    REQUIRE(parity_ok(cw.data()), "unit message %d", i);
    int w = 0;
    for (int n = 0; n < kLdpcN; ++n) w += cw[n];
    REQUIRE(w > 1, "unit message %d has no parity", i);
  }
  for (int t = 0; t < 200; ++t) {
    random_message(msg);
    ldpc_encode91(msg, cw.data());
    REQUIRE(parity_ok(cw.data()) && ldpc_crc_matches(cw.data()), "random message %d", t);
    cw[rnd_u() % kLdpcN] ^= 1;
    REQUIRE(!parity_ok(cw.data()), "a single error passes");
  }

  // ---- CRC-14
  {
    uint8_t z[77] = {};
    REQUIRE(ldpc_crc14(z) == 0, "zeros");
    uint8_t one[77] = {};
    one[76] = 1;                                                      // x^5 x^14 mod g = x^19 mod g
    REQUIRE(ldpc_crc14(one) == crc_by_division(one), "last bit");
    uint8_t first[77] = {};
    first[0] = 1;
    REQUIRE(ldpc_crc14(first) == crc_by_division(first) && ldpc_crc14(first) != 0, "first bit");
    uint8_t all[77];
    memset(all, 1, sizeof all);
    REQUIRE(ldpc_crc14(all) == crc_by_division(all), "ones");
    uint8_t low[77] = {};                                             // the 82-bit word 1 << 5 ... a message of 1 in its last place
    low[76 - 8] = 1;
    REQUIRE(ldpc_crc14(low) == crc_by_division(low), "bit 68");
    for (int t = 0; t < 500; ++t) {
      uint8_t r[77];
      for (int i = 0; i < 77; ++i) r[i] = (uint8_t)(rnd_u() & 1);
      const uint32_t c = ldpc_crc14(r);
      REQUIRE(c == crc_by_division(r) && c < (1u << 14), "random vector %d", t);
    }
  }

  // ---- refusals
  {
    pysdr_ldpc_cfg c{};
    c.iters = 30; c.alpha = 0.8125f;
    REQUIRE(ldpc_cfg_ok(&c) && !ldpc_cfg_ok(nullptr), "good cfg");
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (int it : {0, -1, 201, 1 << 30}) { pysdr_ldpc_cfg b = c; b.iters = it; REQUIRE(!ldpc_cfg_ok(&b), "iters %d", it); }
    for (int it : {1, 200}) { pysdr_ldpc_cfg b = c; b.iters = it; REQUIRE(ldpc_cfg_ok(&b), "iters %d", it); }
    for (float al : {0.f, -0.5f, 1.0001f, inf, -inf, nan}) { pysdr_ldpc_cfg b = c; b.alpha = al; REQUIRE(!ldpc_cfg_ok(&b), "alpha %g", al); }
    for (float al : {1.f, 0.75f, 1e-30f}) { pysdr_ldpc_cfg b = c; b.alpha = al; REQUIRE(ldpc_cfg_ok(&b), "alpha %g", al); }
    REQUIRE(ldpc_n_ok(0) && ldpc_n_ok(4096) && !ldpc_n_ok(-1) && !ldpc_n_ok(4097), "n");
    std::vector<float> x(2 * kLdpcN, 1.f);
    REQUIRE(ldpc_first_nonfinite(x.data(), x.size()) == -1, "finite");
    x[200] = nan;
    REQUIRE(ldpc_first_nonfinite(x.data(), x.size()) == 200, "nan");
    x[200] = 1e38f; x[347] = -inf;
    REQUIRE(ldpc_first_nonfinite(x.data(), x.size()) == 347, "inf");
    REQUIRE(ldpc_first_nonfinite(x.data(), 347) == -1, "short");
  }

  // ---- the check update against the direct transcription
  for (int t = 0; t < 20000; ++t) {
    const int deg = 6 + (int)(rnd_u() & 1);
    float v[kLdpcDegMax] = {}, got[kLdpcDegMax] = {}, want[kLdpcDegMax] = {};
    for (int k = 0; k < deg; ++k) {
      const unsigned pick = rnd_u() % 8;
      v[k] = pick == 0 ? 0.f : pick == 1 ? -0.f : pick == 2 ? 0.5f : pick == 3 ? -0.5f : rnd() * (t % 3 == 0 ? 1e18f : 4.f);
    }
    const float alpha = t % 2 ? 0.8125f : 1.f;
    ldpc_check(v, deg, alpha, got);
    plain_check(v, deg, alpha, want);
    for (int k = 0; k < deg; ++k) REQUIRE(fbits(got[k]) == fbits(want[k]), "check update %d edge %d: %g %g", t, k, got[k], want[k]);
    if (deg == 6) REQUIRE(got[6] == 0.f, "an edge beyond the degree was written");
  }

  // ---- the scalar decoder
  {
    std::vector<float> llr(kLdpcN), post(kLdpcN);
    int32_t st[4];
    uint8_t bits[kLdpcBitsBytes];
    int corrected = 0;
    for (int t = 0; t < 60; ++t) {
      random_message(msg);
      ldpc_encode91(msg, cw.data());
      for (int n = 0; n < kLdpcN; ++n) llr[n] = (cw[n] ? 1.f : -1.f) * (2.f + rnd());
      ldpc_decode_scalar(llr.data(), 30, 0.8125f, st, bits, post.data());
      REQUIRE(st[0] == 2 && st[1] == 0 && st[2] == 0 && st[3] == 0, "noise-free word %d: %d %d %d", t, st[0], st[1], st[2]);
      for (int i = 0; i < kLdpcK; ++i) REQUIRE(((bits[i / 8] >> (7 - i % 8)) & 1) == msg[i], "bit %d", i);
      REQUIRE((bits[11] & 31) == 0, "padding");
      for (int n = 0; n < kLdpcN; ++n) REQUIRE(fbits(post[n]) == fbits(-llr[n]), "post at k = 0 is L");
      const int flips = 1 + t % 5;
      std::vector<int> where;
      while ((int)where.size() < flips) {
        const int n = (int)(rnd_u() % kLdpcN);
        bool seen = false;
        for (int w : where) seen = seen || w == n;
        if (!seen) { where.push_back(n); llr[n] = -llr[n]; }
      }
      ldpc_decode_scalar(llr.data(), 30, 0.8125f, st, bits, nullptr);
      REQUIRE(st[0] == 2 && st[1] >= 1 && st[1] <= 30 && st[2] == flips, "%d flips: status %d after %d, nerr %d", flips, st[0], st[1], st[2]);
      for (int i = 0; i < kLdpcK; ++i) REQUIRE(((bits[i / 8] >> (7 - i % 8)) & 1) == msg[i], "bit %d after %d flips", i, flips);
      ++corrected;
      // one iteration is the limit it is
      ldpc_decode_scalar(llr.data(), 1, 0.8125f, st, bits, nullptr);
      REQUIRE(st[1] <= 1 && (st[0] != 0 || st[1] == 1), "iters = 1");
    }
    REQUIRE(corrected == 60, "corrected");
    // a codeword whose CRC is wrong, and the zero word
    random_message(msg);
    msg[kLdpcMsg + 3] ^= 1;
    ldpc_encode91(msg, cw.data());
    for (int n = 0; n < kLdpcN; ++n) llr[n] = cw[n] ? 3.f : -3.f;
    ldpc_decode_scalar(llr.data(), 30, 0.8125f, st, bits, nullptr);
    REQUIRE(st[0] == 1 && st[1] == 0 && st[2] == 0, "broken CRC: %d", st[0]);
    for (int n = 0; n < kLdpcN; ++n) llr[n] = 0.f;
    ldpc_decode_scalar(llr.data(), 30, 0.8125f, st, bits, post.data());
    REQUIRE(st[0] == 1 && st[1] == 0 && st[2] == 0, "zeros: %d", st[0]);
    for (int b = 0; b < kLdpcBitsBytes; ++b) REQUIRE(bits[b] == 0, "zeros' bits");
    int ok2 = 0;
    for (int t = 0; t < 200; ++t) {
      for (int n = 0; n < kLdpcN; ++n) llr[n] = rnd() * (t % 2 ? 1e18f : 1.f);
      ldpc_decode_scalar(llr.data(), 30, 0.8125f, st, bits, post.data());
      ok2 += st[0] == 2 ? 1 : 0;
      REQUIRE(st[0] != 0 || st[1] == 30, "no codeword after %d", st[1]);
      for (int n = 0; n < kLdpcN; ++n) REQUIRE(std::isfinite(post[n]), "post");
    }
    REQUIRE(ok2 == 0, "%d of 200 noise words decoded", ok2);
  }
  printf("LDPC_PLAN_OK %d edges, %d + %d checks, lds %d bytes\n", kLdpcEdges, n6, n7, kLdpcLdsBytes);
  return 0;
}
