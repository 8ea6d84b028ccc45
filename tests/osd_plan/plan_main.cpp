// The pure half of ordered-statistics decoding (pysdr_amd/csrc/osd_plan.h, the very code osd.hip steps with) on the CPU
// under AddressSanitizer + UBSan.
//   * the rule of the setting, the pattern counts, and k <-> (i, j) over all 4187 in both directions, in lexicographic order.
//   * the rank rule: the key orders as |x| does, -0 is +0, a tie goes to the lower position.
//   * the generator's bit against the encoder, row by row.
//   * zero input: ranks are positions, the basis is the systematic one (last = 90), k = 0, the status stays min-sum's 1.
//   * the scalar transcription, min-sum (ldpc_decode_scalar, iters 30, alpha 0.8125) and then osd_decode_scalar, on the
//     words of the file the environment variable OSD_PLAN_WORDS names (float32 [n][174], written by
//     tests/test_osd_plan.py from the oracle's inputs), for order 0, 1 and 2: one line per word and order with status,
//     bits and detail, which the test compares with the oracle for equality.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "osd_plan.h"

using namespace pysdr;

#define REQUIRE(c, ...) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

int main() {
  // ---- the setting and the counts
  {
    pysdr_osd_cfg c{};
    for (int o : {0, 1, 2}) { c.order = o; REQUIRE(osd_cfg_ok(&c), "order %d", o); }
    for (int o : {-1, 3, 1 << 30, -(1 << 30)}) { c.order = o; REQUIRE(!osd_cfg_ok(&c), "order %d", o); }
    REQUIRE(!osd_cfg_ok(nullptr), "NULL");
    REQUIRE(osd_patterns(0) == 1 && osd_patterns(1) == 92 && osd_patterns(2) == 4187 && kOsdPairs == 4095, "counts");
    REQUIRE(sizeof(pysdr_ldpc_cfg) == 8 && sizeof(pysdr_osd_cfg) == 4, "sizes");
  }
  // ---- k <-> (i, j)
  {
    int i = 0, j = 0, k = 0;
    osd_ij_of(0, &i, &j);
    REQUIRE(i == -1 && j == -1 && osd_k_of(-1, -1) == 0, "k = 0");
    for (int a = 0; a < kLdpcK; ++a) {
      osd_ij_of(1 + a, &i, &j);
      REQUIRE(i == a && j == -1 && osd_k_of(a, -1) == 1 + a, "k = %d", 1 + a);
    }
    k = 1 + kLdpcK;
    for (int a = 0; a < kLdpcK; ++a)
      for (int b = a + 1; b < kLdpcK; ++b, ++k) {                     // lexicographic
        REQUIRE(osd_k_of(a, b) == k, "(%d, %d) -> %d, not %d", a, b, osd_k_of(a, b), k);
        osd_ij_of(k, &i, &j);
        REQUIRE(i == a && j == b, "%d -> (%d, %d), not (%d, %d)", k, i, j, a, b);
      }
    REQUIRE(k == 4187, "%d patterns", k);
  }
  // ---- the rank rule
  {
    REQUIRE(osd_key(-0.f) == 0 && osd_key(0.f) == 0 && osd_key(-2.5f) == osd_key(2.5f), "keys");
    const float v[] = {0.f, 1e-45f, 1e-30f, 0.5f, 1.f, 1.0000001f, 3e17f, 1e18f, 3e38f};
    for (size_t a = 0; a + 1 < sizeof v / sizeof *v; ++a) {
      REQUIRE(osd_key(v[a]) < osd_key(-v[a + 1]), "key order at %zu", a);
      REQUIRE(osd_magnitude(osd_key(-v[a])) == v[a], "magnitude at %zu", a);
    }
    REQUIRE(osd_before(osd_key(2.f), 9, osd_key(-1.f), 3) && !osd_before(osd_key(1.f), 3, osd_key(2.f), 9), "greater first");
    REQUIRE(osd_before(osd_key(1.f), 3, osd_key(-1.f), 9) && !osd_before(osd_key(1.f), 9, osd_key(1.f), 3), "ties by position");
    REQUIRE(!osd_before(osd_key(1.f), 3, osd_key(1.f), 3), "not before itself");
  }
  // ---- the generator's bit against the encoder
  {
    uint8_t msg[kLdpcK], cw[kLdpcN];
    for (int i = 0; i < kLdpcK; ++i) {
      memset(msg, 0, sizeof msg);
      msg[i] = 1;
      ldpc_encode91(msg, cw);
      for (int n = 0; n < kLdpcN; ++n) REQUIRE(osd_gen_bit(i, n) == cw[n], "G[%d][%d]", i, n);
    }
  }
  // ---- zero input
  {
    std::vector<float> llr(kLdpcN, 0.f);
    int32_t st[4], de[4] = {7, 7, 7, 7};
    uint8_t bits[kLdpcBitsBytes];
    ldpc_decode_scalar(llr.data(), 30, 0.8125f, st, bits, nullptr);
    REQUIRE(st[0] == 1 && st[3] == 0, "min-sum on zeros");
    for (int order = 0; order <= kOsdOrderMax; ++order) {
      osd_decode_scalar(llr.data(), order, st, bits, de);
      REQUIRE(st[0] == 1 && st[1] == 0 && st[2] == 0 && st[3] == 1, "zeros: status %d %d %d %d", st[0], st[1], st[2], st[3]);
      REQUIRE(de[0] == 0 && de[1] == 90 && de[2] == 0 && de[3] == 0, "zeros: detail %d %d %d %d", de[0], de[1], de[2], de[3]);
      st[3] = 0;
    }
    // a status 2 is left alone
    st[0] = 2; st[3] = 0;
    osd_decode_scalar(llr.data(), 2, st, bits, de);
    REQUIRE(st[0] == 2 && st[3] == 0 && de[0] == -1 && de[1] == -1 && de[2] == -1 && de[3] == 0, "not run");
    osd_decode_scalar(llr.data(), 2, st, bits, nullptr);
  }
  // ---- the words of the test
  int nwords = 0;
  const char* path = getenv("OSD_PLAN_WORDS");
  if (path && *path) {
    FILE* f = fopen(path, "rb");
    REQUIRE(f != nullptr, "cannot open %s", path);
    std::vector<float> llr(kLdpcN);
    while (fread(llr.data(), sizeof(float), kLdpcN, f) == (size_t)kLdpcN) {
      for (int order = 0; order <= kOsdOrderMax; ++order) {
        int32_t st[4], de[4];
        uint8_t bits[kLdpcBitsBytes];
        ldpc_decode_scalar(llr.data(), 30, 0.8125f, st, bits, nullptr);
        osd_decode_scalar(llr.data(), order, st, bits, de);
        printf("WORD %d %d %d %d %d %d ", nwords, order, st[0], st[1], st[2], st[3]);
        for (int b = 0; b < kLdpcBitsBytes; ++b) printf("%02x", bits[b]);
        printf(" %d %d %d %d\n", de[0], de[1], de[2], de[3]);
      }
      ++nwords;
    }
    fclose(f);
  }
  printf("OSD_PLAN_OK %d words, %d patterns, lds %d bytes\n", nwords, osd_patterns(2), kOsdLdsBytes);
  return 0;
}
