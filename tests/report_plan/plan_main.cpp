// The pure half of the frame report (pysdr_amd/csrc/report_plan.h, the very code report.hip steps with) on the CPU under
// AddressSanitizer + UBSan.
//   * the plan of both modes and its refusals; the LDS budget against the arrays the kernel declares.
//   * the message words, the parity bits against the encoder, the tones against the skimmers' own tables: the Costas
//     symbols in their places, the modes' data_sym in the other direction, the Gray maps.
//   * the mask of places: every combination of a first, a last and an inner fine row, circular or not, with a frame at
//     the ring's oldest step, its newest, at step 0 and in between; the wrap of a fine row.
//   * the row floor's rule: nsym, a span before step 0, one not complete, one that has left the ring.
//   * the scalar transcription on the cases of the files the environment variable REPORT_PLAN_CASES names (written by
//     tests/test_report_plan.py: a ring, candidates with their message bits, floor spans): one line per candidate with the
//     mask, the bits of the ten powers and the two counts, one per floor with the bits of every bin, which the test
//     compares with the oracle for equality.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "report_plan.h"

using namespace pysdr;

#define REQUIRE(c, ...) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static uint32_t bits_of(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }

template <int MODE>
static void check_tones() {
  constexpr int NS = ReportGeom<MODE>::kSyms;
  uint8_t cw[kReportCwBytes] = {};
  uint32_t seed = 12345u + MODE;
  for (int trial = 0; trial < 50; ++trial) {
    for (int i = 0; i < kLdpcN; ++i) { seed = seed * 1664525u + 1013904223u; cw[i] = (uint8_t)((seed >> 16) & 1u); }
    int nsync = 0, ndata = 0;
    for (int k = 0; k < NS; ++k) {
      bool sync = false;
      const int tone = report_tone<MODE>(cw, k, &sync);
      REQUIRE(tone >= 0 && tone < ReportGeom<MODE>::kTones, "tone %d of symbol %d", tone, k);
      nsync += sync ? 1 : 0;
      ndata += sync ? 0 : 1;
    }
    if (MODE == kReportFt8) {
      REQUIRE(nsync == 21 && ndata == Ft8Mode::kData, "%d sync, %d data", nsync, ndata);
      for (int n = 0; n < 21; ++n) {
        bool sync = false;
        REQUIRE(report_tone<MODE>(cw, Ft8Mode::costas_sym(n), &sync) == Ft8Mode::costas(n % 7) && sync, "Costas symbol %d", n);
      }
      for (int d = 0; d < Ft8Mode::kData; ++d) {
        bool sync = true;
        const int v = 4 * cw[3 * d] + 2 * cw[3 * d + 1] + cw[3 * d + 2];
        REQUIRE(report_tone<MODE>(cw, Ft8Mode::data_sym(d), &sync) == Ft8Mode::gray(v) && !sync, "data symbol %d", d);
      }
    } else {
      REQUIRE(nsync == Ft4Mode::kSync && ndata == Ft4Mode::kData, "%d sync, %d data", nsync, ndata);
      for (int n = 0; n < Ft4Mode::kSync; ++n) {
        bool sync = false;
        REQUIRE(report_tone<MODE>(cw, Ft4Mode::costas_sym(n), &sync) == Ft4Mode::costas(n) && sync, "Costas symbol %d", n);
      }
      for (int d = 0; d < Ft4Mode::kData; ++d) {
        bool sync = true;
        const int v = 2 * cw[2 * d] + cw[2 * d + 1];
        REQUIRE(report_tone<MODE>(cw, Ft4Mode::data_sym(d), &sync) == Ft4Mode::gray(v) && !sync, "data symbol %d", d);
      }
    }
  }
}

template <int MODE>
static void run_case(int ci, const int32_t* hd, const std::vector<float>& ring, const std::vector<int32_t>& Fs, const std::vector<long long>& t0s,
                     const std::vector<uint8_t>& bits) {
  const int tr = hd[2], nb = hd[3], nsub = hd[4], nfine = hd[1] * hd[4], n = hd[7];
  const long long t_done = hd[5];
  for (int i = 0; i < n; ++i) {
    const bool ok = ft_llr_ok<FtReportMode<MODE>>(Fs[i], t0s[i], t_done, nfine, tr);
    REQUIRE(ok, "case %d candidate %d (F %d, t0 %lld) is one the call refuses", ci, i, Fs[i], t0s[i]);
    const int mask = report_mask(Fs[i], t0s[i], t_done, nfine, tr, ReportGeom<MODE>::kLag, hd[6] != 0);
    REQUIRE((mask >> 4) & 1, "the candidate's own place");
    float power[kReportCols];
    int32_t errs[2];
    report_scalar<MODE>(ring.data(), tr, nb, nsub, nfine, Fs[i], (int)(t0s[i] % tr), mask, bits.data() + (size_t)i * kReportBitsBytes, power, errs);
    printf("CAND %d %d %d", ci, i, mask);
    for (int c = 0; c < kReportCols; ++c) printf(" %08x", bits_of(power[c]));
    printf(" %d %d\n", errs[0], errs[1]);
  }
}

int main() {
  // ---- the plan
  {
    int32_t out[4] = {-7, -7, -7, -7};
    REQUIRE(report_plan(kReportFt8, out) && out[0] == 128 && out[1] == kReportLdsBytes && out[2] == 79 && out[3] == 4096, "FT8 plan");
    REQUIRE(report_plan(kReportFt4, out) && out[0] == 128 && out[1] == kReportLdsBytes && out[2] == 103 && out[3] == 4096, "FT4 plan");
    int32_t keep[4] = {-7, -7, -7, -7};
    for (int mode : {-1, 2, 1 << 30}) REQUIRE(!report_plan(mode, keep) && keep[0] == -7 && keep[3] == -7, "mode %d", mode);
    REQUIRE(!report_plan(kReportFt8, nullptr), "NULL out");
    REQUIRE(kReportLdsBytes == 4400 && kReportLdsBytes >= kReportCols * kReportPitch * 4 + kReportCwBytes + 16, "LDS %d", kReportLdsBytes);
    REQUIRE(report_n_ok(0) && report_n_ok(4096) && !report_n_ok(-1) && !report_n_ok(4097), "n");
  }
  // ---- words, parity, tones
  {
    uint8_t b12[kReportBitsBytes] = {0x80, 0x00, 0x00, 0x01, 0xff, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x3f};
    uint32_t w[3];
    report_words(b12, w);
    REQUIRE(w[0] == 0x80000001u && w[1] == 0xff000000u && w[2] == 0x0000003fu, "words");
    REQUIRE(report_msg_bit(w[0], w[1], w[2], 0) == 1 && report_msg_bit(w[0], w[1], w[2], 1) == 0 && report_msg_bit(w[0], w[1], w[2], 31) == 1 &&
            report_msg_bit(w[0], w[1], w[2], 32) == 1 && report_msg_bit(w[0], w[1], w[2], 40) == 0 && report_msg_bit(w[0], w[1], w[2], 90) == 1, "bits");
    uint32_t seed = 99u;
    for (int trial = 0; trial < 200; ++trial) {
      uint8_t msg[kLdpcK], cw[kLdpcN], p12[kReportBitsBytes] = {};
      for (int i = 0; i < kLdpcK; ++i) { seed = seed * 1664525u + 1013904223u; msg[i] = (uint8_t)((seed >> 16) & 1u); }
      for (int i = 0; i < kLdpcK; ++i) p12[i / 8] |= (uint8_t)(msg[i] << (7 - i % 8));
      if (trial & 1) p12[11] |= 0x1f;                                 // padding that is not zero meets zeros in the generator
      ldpc_encode91(msg, cw);
      report_words(p12, w);
      for (int i = 0; i < kLdpcK; ++i) REQUIRE(report_msg_bit(w[0], w[1], w[2], i) == cw[i], "bit %d", i);
      for (int j = 0; j < kLdpcM; ++j) REQUIRE(report_parity(w[0], w[1], w[2], j) == cw[kLdpcK + j], "parity %d of trial %d", j, trial);
    }
    check_tones<kReportFt8>();
    check_tones<kReportFt4>();
  }
  // ---- the mask of places
  {
    const int nfine = 96, tr = 340, lag = kFtLag<Ft8Mode>;
    const long long done = 400;                                       // frames may begin at 60 .. 87
    REQUIRE(ft_llr_ok<Ft8Mode>(5, 60, done, nfine, tr) && !ft_llr_ok<Ft8Mode>(5, 59, done, nfine, tr) && ft_llr_ok<Ft8Mode>(5, 87, done, nfine, tr) &&
            !ft_llr_ok<Ft8Mode>(5, 88, done, nfine, tr), "the window");
    REQUIRE(report_mask(5, 70, done, nfine, tr, lag, false) == 0x1ff && report_mask(5, 70, done, nfine, tr, lag, true) == 0x1ff, "inner");
    REQUIRE(report_mask(5, 60, done, nfine, tr, lag, false) == 0x1f8 && report_mask(5, 87, done, nfine, tr, lag, false) == 0x03f, "time's ends");
    REQUIRE(report_mask(0, 70, done, nfine, tr, lag, false) == 0x1b6 && report_mask(95, 70, done, nfine, tr, lag, false) == 0x0db, "raster's ends");
    REQUIRE(report_mask(0, 70, done, nfine, tr, lag, true) == 0x1ff && report_mask(95, 70, done, nfine, tr, lag, true) == 0x1ff, "a circle has no end");
    REQUIRE(report_mask(0, 60, done, nfine, tr, lag, false) == 0x1b0 && report_mask(95, 87, done, nfine, tr, lag, false) == 0x01b, "corners");
    REQUIRE(report_mask(3, 0, 313, nfine, tr, lag, false) == 0x038 && report_mask(3, 0, 314, nfine, tr, lag, false) == 0x1f8 &&
            report_mask(3, 1, 314, nfine, tr, lag, false) == 0x03f, "a young stream");
    REQUIRE(report_mask(3, 70, done, nfine, tr, kFtLag<Ft4Mode>, false) == 0 , "an FT4 frame does not fit 340 steps");
    REQUIRE(report_wrap(-1, nfine) == 95 && report_wrap(96, nfine) == 0 && report_wrap(40, nfine) == 40, "wrap");
  }
  // ---- the row floor's rule
  {
    const int tr = 340;
    const long long done = 400;
    REQUIRE(floor_ok(399, 1, done, tr) && floor_ok(399, 79, done, tr) && floor_ok(399, 85, done, tr) && floor_ok(60, 1, done, tr) &&
            floor_ok(60 + 312, 79, done, tr), "good spans");
    REQUIRE(!floor_ok(400, 1, done, tr) && !floor_ok(399, 0, done, tr) && !floor_ok(399, 129, done, tr) && !floor_ok(399, 86, done, tr) &&
            !floor_ok(59, 1, done, tr) && !floor_ok(59 + 312, 79, done, tr) && !floor_ok(-1, 1, done, tr), "refused spans");
    REQUIRE(!floor_ok(99, 26, 100, tr) && floor_ok(99, 25, 100, tr) && floor_ok(0, 1, 1, tr) && !floor_ok(0, 1, 0, tr), "before step 0");
    REQUIRE(floor_nsym_ok(1) && floor_nsym_ok(128) && !floor_nsym_ok(0) && !floor_nsym_ok(129) && !floor_nsym_ok(-5), "nsym");
    const float rows[3 * 2] = {1.f, 10.f, 2.f, 20.f, 4.f, 40.f};       // tr 3, nb 2
    REQUIRE(floor_bin(rows, 3, 2, 1, 1, 0) == 2.f && floor_bin(rows, 3, 2, 1, 1, 1) == 20.f, "one step");
  }
  // ---- the cases of the test
  int ncases = 0, ncand = 0, nfloor = 0;
  const char* list = getenv("REPORT_PLAN_CASES");
  std::string paths = list ? list : "";
  while (!paths.empty()) {
    const size_t cut = paths.find(':');
    const std::string path = paths.substr(0, cut);
    paths = cut == std::string::npos ? "" : paths.substr(cut + 1);
    FILE* f = fopen(path.c_str(), "rb");
    REQUIRE(f != nullptr, "cannot open %s", path.c_str());
    int32_t hd[9];                                                    // mode, nk, tr, nb, nsub, t_done, circular, n, floors
    REQUIRE(fread(hd, sizeof(int32_t), 9, f) == 9, "header of %s", path.c_str());
    REQUIRE(report_mode_ok(hd[0]) && hd[1] > 0 && hd[2] > 0 && hd[3] == hd[4] + (hd[0] == kReportFt8 ? 14 : 6) && hd[7] >= 0 && hd[8] >= 0, "header");
    std::vector<float> ring((size_t)hd[1] * hd[2] * hd[3]);
    REQUIRE(fread(ring.data(), sizeof(float), ring.size(), f) == ring.size(), "ring");
    std::vector<int32_t> Fs(hd[7]), fl(2 * (size_t)hd[8]);
    std::vector<long long> t0s(hd[7]);
    std::vector<uint8_t> bits((size_t)hd[7] * kReportBitsBytes);
    REQUIRE(fread(Fs.data(), sizeof(int32_t), Fs.size(), f) == Fs.size(), "F");
    REQUIRE(fread(t0s.data(), sizeof(long long), t0s.size(), f) == t0s.size(), "t0");
    REQUIRE(fread(bits.data(), 1, bits.size(), f) == bits.size(), "bits");
    REQUIRE(fread(fl.data(), sizeof(int32_t), fl.size(), f) == fl.size(), "floors");
    fclose(f);
    if (hd[0] == kReportFt8) run_case<kReportFt8>(ncases, hd, ring, Fs, t0s, bits);
    else run_case<kReportFt4>(ncases, hd, ring, Fs, t0s, bits);
    for (int k = 0; k < hd[8]; ++k) {
      const int t_end = fl[2 * k], nsym = fl[2 * k + 1];
      const bool ok = floor_ok(t_end, nsym, hd[5], hd[2]);
      printf("FLOOR %d %d %d", ncases, k, ok ? 1 : 0);
      if (ok)
        for (int a = 0; a < hd[1]; ++a)
          for (int b = 0; b < hd[3]; ++b)
            printf(" %08x", bits_of(floor_bin(ring.data() + (size_t)a * hd[2] * hd[3], hd[2], hd[3], t_end % hd[2], nsym, b)));
      printf("\n");
      ++nfloor;
    }
    ncand += hd[7];
    ++ncases;
  }
  printf("REPORT_PLAN_OK %d cases, %d candidates, %d floors, lds %d bytes\n", ncases, ncand, nfloor, kReportLdsBytes);
  return 0;
}
