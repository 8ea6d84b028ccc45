// The pure half of a-priori decoding (pysdr_amd/csrc/ap_plan.h, the very code ap.hip steps with) on the CPU under
// AddressSanitizer + UBSan.
//   * every refusal of the settings, of a hypothesis table and of a pair list, and the offsets first[n + 1].
//   * the clamp (+A, -A, -0 where A is 0, untouched outside the mask), the counting of nerr and nap, a pair's status.
//   * the pick: the least nerr, a tie to the lower pair, no pair of status 2, a candidate without pairs.
//   * the scalar transcription ap_decode_scalar and the pick on the case of the file the environment variable AP_PLAN_CASE
//     names (written by tests/test_ap_plan.py: int32 n, H, P, iters, nerr_max; float32 mag, alpha; llr [n][174]; hyps
//     [H][24]; pairs [P][2]): one line per pair with detail and bits, one per candidate with ap and bits, which the test
//     compares with the oracle for equality.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ap_plan.h"

using namespace pysdr;

#define REQUIRE(c, ...) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static void set_bit(uint8_t* w, int i) { w[i >> 3] |= (uint8_t)(1u << (7 - (i & 7))); }

int main() {
  // ---- the settings
  {
    pysdr_ap_cfg c{1.f, 174};
    REQUIRE(ap_cfg_ok(&c) && !ap_cfg_ok(nullptr), "default / NULL");
    for (float m : {0.25f, 0.5f, 16.f}) { c.mag = m; REQUIRE(ap_cfg_ok(&c), "mag %g", (double)m); }
    for (float m : {0.f, -1.f, 0.2499f, 16.001f, NAN, INFINITY, -INFINITY}) { c.mag = m; REQUIRE(!ap_cfg_ok(&c), "mag %g", (double)m); }
    c.mag = 1.f;
    for (int e : {0, 1, 173, 174}) { c.nerr_max = e; REQUIRE(ap_cfg_ok(&c), "nerr_max %d", e); }
    for (int e : {-1, 175, 1 << 30, -(1 << 30)}) { c.nerr_max = e; REQUIRE(!ap_cfg_ok(&c), "nerr_max %d", e); }
    REQUIRE(sizeof(pysdr_ap_cfg) == 8 && kApHypBytes == 24, "sizes");
    REQUIRE(ap_hyps_n_ok(1) && ap_hyps_n_ok(4096) && !ap_hyps_n_ok(0) && !ap_hyps_n_ok(4097) && !ap_hyps_n_ok(-1), "H");
    REQUIRE(ap_pairs_n_ok(0) && ap_pairs_n_ok(65536) && !ap_pairs_n_ok(65537) && !ap_pairs_n_ok(-1), "P");
  }
  // ---- a hypothesis
  {
    uint8_t h[kApHypBytes] = {};
    REQUIRE(!ap_hyp_ok(h), "an empty mask");
    for (int i = 0; i < 96; ++i) {                                    // every single bit: 0 .. 76 may be set, 77 .. 95 may not
      memset(h, 0, sizeof h);
      set_bit(h, i);
      REQUIRE(ap_hyp_ok(h) == (i < kLdpcMsg), "mask bit %d", i);
      REQUIRE(ap_bit(h, i) == 1 && (i == 0 || ap_bit(h, i - 1) == 0), "ap_bit %d", i);
      REQUIRE(ap_masked(h, i) == (i < kLdpcMsg), "ap_masked %d", i);
      set_bit(h + kApWordBytes, i);
      REQUIRE(ap_hyp_ok(h) == (i < kLdpcMsg), "mask and value bit %d", i);
      memset(h, 0, kApWordBytes);
      set_bit(h, (i + 1) % kLdpcMsg);
      REQUIRE(!ap_hyp_ok(h), "value bit %d outside the mask", i);
    }
    memset(h, 0, sizeof h);
    for (int i = 0; i < kLdpcMsg; ++i) { set_bit(h, i); set_bit(h + kApWordBytes, i); }
    REQUIRE(ap_hyp_ok(h), "all 77");
    REQUIRE(!ap_masked(h, 77) && !ap_masked(h, 173), "beyond the message");
    uint8_t tab[3 * kApHypBytes] = {};
    set_bit(tab, 0); set_bit(tab + kApHypBytes, 76); set_bit(tab + 2 * kApHypBytes, 5);
    REQUIRE(ap_first_bad_hyp(tab, 3) == -1, "a good table");
    set_bit(tab + kApHypBytes, 77);
    REQUIRE(ap_first_bad_hyp(tab, 3) == 1 && ap_first_bad_hyp(tab, 1) == -1, "the second is bad");
  }
  // ---- a pair list and first[]
  {
    const int32_t p[] = {0, 1, 0, 3, 2, 0, 2, 1, 2, 2, 5, 3};          // candidates 1, 3 and 4 have none
    int32_t first[8];
    REQUIRE(ap_first_bad_pair(p, 6, 6, 4, first) == -1, "a good list");
    const int32_t want[] = {0, 2, 2, 5, 5, 5, 6};
    for (int c = 0; c <= 6; ++c) REQUIRE(first[c] == want[c], "first[%d] = %d", c, first[c]);
    REQUIRE(ap_first_bad_pair(p, 0, 6, 4, first) == -1 && first[0] == 0 && first[6] == 0, "no pairs");
    REQUIRE(ap_first_bad_pair(nullptr, 0, 0, 1, first) == -1 && first[0] == 0, "no candidates");
    REQUIRE(ap_first_bad_pair(p, 6, 5, 4, first) == 5, "candidate 5 of 5");
    REQUIRE(ap_first_bad_pair(p, 6, 6, 3, first) == 1, "hypothesis 3 of 3");
    const int32_t same[] = {0, 1, 0, 1}, down[] = {1, 0, 0, 5}, hdown[] = {1, 2, 1, 1}, neg[] = {-1, 0}, hneg[] = {0, -1};
    REQUIRE(ap_first_bad_pair(same, 2, 2, 8, first) == 1, "a pair twice");
    REQUIRE(ap_first_bad_pair(down, 2, 2, 8, first) == 1, "a candidate below the one before");
    REQUIRE(ap_first_bad_pair(hdown, 2, 2, 8, first) == 1, "a hypothesis below the one before");
    REQUIRE(ap_first_bad_pair(neg, 1, 2, 8, first) == 0 && ap_first_bad_pair(hneg, 1, 2, 8, first) == 0, "negative");
  }
  // ---- the clamp, the counting, the status
  {
    uint8_t h[kApHypBytes] = {};
    set_bit(h, 3); set_bit(h, 4); set_bit(h + kApWordBytes, 4);
    REQUIRE(ap_amp(2.f, 3.f) == 6.f && ap_amp(1.f, 0.f) == 0.f, "A");
    REQUIRE(ap_clamp(0.5f, 6.f, h, 2) == 0.5f && ap_clamp(0.5f, 6.f, h, 3) == -6.f && ap_clamp(-0.5f, 6.f, h, 4) == 6.f, "the clamp");
    REQUIRE(ap_clamp(0.5f, 6.f, h, 100) == 0.5f, "beyond the message");
    REQUIRE(std::signbit(ap_clamp(1.f, 0.f, h, 3)) && !std::signbit(ap_clamp(-1.f, 0.f, h, 4)), "-0 and +0 where A is 0");
    bool err, miss;
    ap_count(0.5f, false, h, 2, &err, &miss); REQUIRE(err && !miss, "outside, llr > 0, hard 0");
    ap_count(0.5f, true, h, 2, &err, &miss); REQUIRE(!err && !miss, "outside, agree");
    ap_count(0.f, true, h, 2, &err, &miss); REQUIRE(err && !miss, "outside, llr 0 is bit 0");
    ap_count(0.5f, true, h, 3, &err, &miss); REQUIRE(!err && miss, "inside, value 0, hard 1");
    ap_count(-0.5f, true, h, 4, &err, &miss); REQUIRE(!err && !miss, "inside, value 1, hard 1");
    ap_count(0.5f, false, h, 4, &err, &miss); REQUIRE(!err && miss, "inside, value 1, hard 0");
    REQUIRE(ap_status(2, 10, 0, 10) == 2 && ap_status(2, 11, 0, 10) == 1 && ap_status(2, 0, 1, 174) == 1, "status 2 and its guards");
    REQUIRE(ap_status(1, 0, 0, 174) == 1 && ap_status(0, 0, 0, 174) == 0, "status 1 and 0");
  }
  // ---- the pick
  {
    //                      status it nerr nap
    const int32_t d[] = {1, 3, 2, 0,   2, 7, 9, 0,   2, 5, 4, 0,   2, 6, 4, 0,   0, 30, 50, 2,   1, 2, 0, 0,   2, 1, 8, 0};
    uint8_t pb[7 * kLdpcBitsBytes];
    for (int p = 0; p < 7; ++p) memset(pb + p * kLdpcBitsBytes, 0x10 + p, kLdpcBitsBytes);
    int32_t ap[4];
    uint8_t bits[kLdpcBitsBytes];
    ap_pick(d, pb, 0, 4, ap, bits);
    REQUIRE(ap[0] == 2 && ap[1] == 5 && ap[2] == 4 && ap[3] == 3 && bits[0] == 0x12 && bits[11] == 0x12, "least nerr, the tie to the lower pair");
    ap_pick(d, pb, 3, 4, ap, bits);
    REQUIRE(ap[0] == 3 && ap[1] == 6 && ap[2] == 4 && ap[3] == 1 && bits[5] == 0x13, "one pair");
    ap_pick(d, pb, 4, 6, ap, bits);
    REQUIRE(ap[0] == -1 && ap[1] == 0 && ap[2] == 0 && ap[3] == 0 && bits[0] == 0 && bits[11] == 0, "no pair of status 2");
    ap_pick(d, pb, 6, 6, ap, bits);
    REQUIRE(ap[0] == -1 && ap[3] == 0 && bits[3] == 0, "a candidate without pairs");
    ap_pick(d, pb, 0, 7, ap, bits);
    REQUIRE(ap[0] == 2 && ap[3] == 4, "all seven");
  }
  // ---- the case of the test
  int n = 0, H = 0, P = 0;
  const char* path = getenv("AP_PLAN_CASE");
  if (path && *path) {
    FILE* f = fopen(path, "rb");
    REQUIRE(f != nullptr, "cannot open %s", path);
    int32_t head[5];
    float fl[2];
    REQUIRE(fread(head, 4, 5, f) == 5 && fread(fl, 4, 2, f) == 2, "the head");
    n = head[0]; H = head[1]; P = head[2];
    REQUIRE(ldpc_n_ok(n) && ap_hyps_n_ok(H) && ap_pairs_n_ok(P), "n %d H %d P %d", n, H, P);
    std::vector<float> llr((size_t)n * kLdpcN);
    std::vector<uint8_t> hyps((size_t)H * kApHypBytes);
    std::vector<int32_t> pairs((size_t)P * 2 + 1), first((size_t)n + 1);
    REQUIRE(fread(llr.data(), 4, llr.size(), f) == llr.size() && fread(hyps.data(), 1, hyps.size(), f) == hyps.size() &&
            fread(pairs.data(), 4, (size_t)P * 2, f) == (size_t)P * 2, "the body");
    fclose(f);
    pysdr_ap_cfg c{fl[0], head[4]};
    REQUIRE(ap_cfg_ok(&c) && ap_first_bad_hyp(hyps.data(), H) == -1 && ap_first_bad_pair(pairs.data(), P, n, H, first.data()) == -1, "the case's rules");
    std::vector<int32_t> detail((size_t)P * kApDetailWords + 1);
    std::vector<uint8_t> pbits((size_t)P * kLdpcBitsBytes + 1);
    for (int p = 0; p < P; ++p) {
      ap_decode_scalar(llr.data() + (size_t)pairs[2 * p] * kLdpcN, hyps.data() + (size_t)pairs[2 * p + 1] * kApHypBytes, c.mag, c.nerr_max, head[3],
                       fl[1], detail.data() + (size_t)p * kApDetailWords, pbits.data() + (size_t)p * kLdpcBitsBytes);
      const int32_t* d = detail.data() + (size_t)p * kApDetailWords;
      printf("PAIR %d %d %d %d %d ", p, d[0], d[1], d[2], d[3]);
      for (int b = 0; b < kLdpcBitsBytes; ++b) printf("%02x", pbits[(size_t)p * kLdpcBitsBytes + b]);
      printf("\n");
    }
    for (int cnd = 0; cnd < n; ++cnd) {
      int32_t ap[kApWords];
      uint8_t bits[kLdpcBitsBytes];
      ap_pick(detail.data(), pbits.data(), first[cnd], first[cnd + 1], ap, bits);
      printf("CAND %d %d %d %d %d ", cnd, ap[0], ap[1], ap[2], ap[3]);
      for (int b = 0; b < kLdpcBitsBytes; ++b) printf("%02x", bits[b]);
      printf("\n");
    }
  }
  printf("AP_PLAN_OK %d candidates, %d hypotheses, %d pairs, lds %d bytes\n", n, H, P, kApLdsBytes);
  return 0;
}
