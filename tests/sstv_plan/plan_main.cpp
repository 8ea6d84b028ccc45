// The SSTV skimmer's plan, tile geometry, steps and event slots (pysdr_amd/csrc/sstv_plan.h, the very code sstv.hip steps
// with) on the CPU under AddressSanitizer + UBSan.
//   * the rules: L in [9, 96], nk in [1, 2^15], max_out in [1, 2^20], the settings' and the mode table's rules; every
//     refusal leaves the plan untouched; the groups tile [0, nk), the row pitch holds the history's room and max_out.
//   * the tile walk of the kernel, through the index functions of SstvGeom that sstv.hip itself uses: every access goes to
//     a Y of exactly nk x pitch elements and LDS tiles of exactly their size (heap: the sanitizer guards both ends); every
//     (row, output) gets its lag product once per pseudo-row, from the samples the definition names; the history roll
//     stays in the row and moves every sample once, whatever the overlap.
//   * the kernel's phases with real samples -- TINY pictures, USB and FM, two rows with different modes, two pictures back to
//     back, noise, a NaN, an infinite and an over-pmax sample -- call after call (1 output, tile - 1, tile, tile + 1,
//     16, 256, 4096) against a plain transcription of DESIGN.md 3 item 30 over the whole stream: lag products bit for
//     bit, every event word, the state at the end; the pictures sent are the pictures read; every cut gives the same.
//   * the Q16 pixel boundaries are strictly increasing and never empty for every mode at 8, 12, 25 and 48 kHz.
//   * the cap: under the densest stream there is -- the shortest mode's pictures back to back, each VIS matched on the tick
//     after the last line and each anchor at its earliest -- no window of max_out outputs holds more words than the cap.
//   * the event words round-trip.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sstv_plan.h"

using namespace pysdr;

#define REQUIRE(c, ...) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static uint32_t word_of(double f, double fs) { return (uint32_t)(long long)llround(f / fs * 4294967296.0); }
static uint32_t q16(double ms, double fs) { return (uint32_t)llround(ms * 1e-3 * fs * 65536.0); }

struct ModeMs { const char* name; int code, scans, width, lines; double sync, porch, pixel, sep; };
static const ModeMs kModes[] = {
    {"PD50", 93, 4, 320, 128, 20, 2.08, 0.286, 0},   {"PD90", 99, 4, 320, 128, 20, 2.08, 0.532, 0},  {"PD120", 95, 4, 640, 248, 20, 2.08, 0.19, 0},
    {"PD160", 98, 4, 512, 200, 20, 2.08, 0.382, 0},  {"PD180", 96, 4, 640, 248, 20, 2.08, 0.286, 0}, {"PD240", 97, 4, 640, 248, 20, 2.08, 0.382, 0},
    {"PD290", 94, 4, 800, 308, 20, 2.08, 0.286, 0},  {"Martin M1", 44, 3, 320, 256, 4.862, 0.572, 0.4576, 0.572},
    {"Martin M2", 40, 3, 320, 256, 4.862, 0.572, 0.2288, 0.572},
    {"TINY", 5, 3, 32, 6, 5.0, 1.0, 0.5, 0.5},       {"TINY2", 6, 1, 40, 4, 8.0, 1.5, 0.4, 0.0},
};
constexpr int kNModes = sizeof(kModes) / sizeof(kModes[0]);

static pysdr_sstv_mode mode_of(const ModeMs& m, double fs) {
  pysdr_sstv_mode o{};
  o.code = m.code; o.scans = m.scans; o.width = m.width; o.lines = m.lines;
  o.sync_q = q16(m.sync, fs); o.porch_q = q16(m.porch, fs); o.scan_q = q16(m.pixel * m.width, fs); o.sep_q = q16(m.sep, fs);
  return o;
}

static int filter_length(double fs) { return 2 * (int)floor(0.75 * fs / 1000.0) + 1; }

static pysdr_sstv_cfg good_cfg(double fs, int det) {
  pysdr_sstv_cfg c{};
  c.det = det; c.nmodes = kNModes;
  c.w_sub = det == 0 ? word_of(1900, fs) : 0u; c.w_tick = word_of(100, fs);
  c.k_hz = (float)(fs / (2 * M_PI)); c.k_rho = (float)(1024.0 / fs); c.pmax = 1e18f;
  c.R0 = (int)llround(0.010 * fs); c.W = (int)llround(fs / 500.0); c.lag = 2 * c.R0 + c.W + 1;
  for (int i = 0; i < kNModes; ++i) c.modes[i] = mode_of(kModes[i], fs);
  return c;
}

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float rndf() { return (float)((int)(rnd() & 0xFFFF) - 32768) / 32768.f; }

// ---- the rules --------------------------------------------------------------------------------------------------------
static bool same_plan(const SstvPlan& a, const SstvPlan& b) { return a.L == b.L && a.H == b.H && a.cap == b.cap && a.groups == b.groups && a.ypitch == b.ypitch; }

static void refused(int nk, int L, int mo, const pysdr_sstv_cfg* c, const char* what) {
  SstvPlan p;
  p.L = -7; p.H = -7; p.cap = -7; p.groups = -7; p.ypitch = -7;
  const SstvPlan before = p;
  REQUIRE(!sstv_plan(nk, L, mo, c, &p), "%s accepted", what);
  REQUIRE(same_plan(p, before), "%s: a refusal changed the plan", what);
}

static void rules() {
  SstvPlan p;
  const double rates[] = {8000, 12000, 16000, 25000, 48000};
  for (double fs : rates)
    for (int det = 0; det < 2; ++det) {
      const pysdr_sstv_cfg c = good_cfg(fs, det);
      const int L = filter_length(fs);
      REQUIRE(sstv_plan(4, L, 4096, &c, &p), "good plan at %g", fs);
      REQUIRE(p.L == L && p.H == 2 * c.R0 + 2 * c.W + L + 1 && p.H <= kSstvHpad && p.groups == 1 && p.ypitch == kSstvHpad + 4096, "plan at %g", fs);
      REQUIRE(p.cap == sstv_event_cap(4096, c) && p.cap >= 800 + 2, "cap at %g", fs);
    }
  const pysdr_sstv_cfg c = good_cfg(25000.0, 0);
  for (int L = 0; L < 110; ++L) {
    if (L >= 9 && L <= 96) REQUIRE(sstv_plan(4, L, 64, &c, &p), "L %d", L);
    else refused(4, L, 64, &c, "L");
  }
  refused(0, 37, 64, &c, "nk 0"); refused(-1, 37, 64, &c, "nk -1"); refused((1 << 15) + 1, 37, 64, &c, "nk above");
  refused(4, 37, 0, &c, "max_out 0"); refused(4, 37, (1 << 20) + 1, &c, "max_out above"); refused(4, 37, 64, nullptr, "no cfg");
  REQUIRE(sstv_plan(1 << 15, 37, 64, &c, &p) && sstv_plan(4, 37, 1 << 20, &c, &p), "limits");
  refused(1 << 15, 37, 1 << 20, &c, "slots above 2^28 words");
  const float badf[] = {0.f, -1.f, NAN, INFINITY, -INFINITY, 1.1e18f};
  for (float v : badf) { pysdr_sstv_cfg b = c; b.pmax = v; refused(4, 37, 64, &b, "pmax"); }
  { pysdr_sstv_cfg b = c; b.det = 2; refused(4, 37, 64, &b, "det"); b.det = -1; refused(4, 37, 64, &b, "det"); }
  { pysdr_sstv_cfg b = c; b.w_tick = 0; refused(4, 37, 64, &b, "w_tick 0"); b.w_tick = c.w_tick * 2; refused(4, 37, 64, &b, "w_tick twice");
    b.w_tick = c.w_tick / 2; refused(4, 37, 64, &b, "w_tick half"); }
  { pysdr_sstv_cfg b = c; b.R0 = c.R0 + 2; b.lag = 2 * b.R0 + b.W + 1; refused(4, 37, 64, &b, "R0"); b = c; b.R0 = 79; refused(4, 37, 64, &b, "R0 low"); }
  { pysdr_sstv_cfg b = c; b.W = c.W + 1; b.lag = 2 * b.R0 + b.W + 1; refused(4, 37, 64, &b, "W"); b.W = 0; b.lag = 2 * b.R0 + 1; refused(4, 37, 64, &b, "W 0"); }
  { pysdr_sstv_cfg b = c; b.lag = c.lag + 1; refused(4, 37, 64, &b, "lag"); b.lag = c.lag - 1; refused(4, 37, 64, &b, "lag"); }
  { pysdr_sstv_cfg b = c; b.k_hz = c.k_hz * 1.1f; refused(4, 37, 64, &b, "k_hz"); b.k_hz = NAN; refused(4, 37, 64, &b, "k_hz nan");
    b = c; b.k_rho = c.k_rho * 1.1f; refused(4, 37, 64, &b, "k_rho"); b.k_rho = NAN; refused(4, 37, 64, &b, "k_rho nan"); }
  { pysdr_sstv_cfg b = c; b.nmodes = 0; refused(4, 37, 64, &b, "no mode"); b.nmodes = 17; refused(4, 37, 64, &b, "17 modes"); }
  { pysdr_sstv_cfg b = c; b.modes[3].scan_q = ((uint32_t)b.modes[3].width << 16) - 1; refused(4, 37, 64, &b, "a pixel under one sample");
    b.modes[3].scan_q = (uint32_t)b.modes[3].width << 16; REQUIRE(sstv_plan(4, 37, 64, &b, &p), "a pixel of one sample"); }
  { pysdr_sstv_cfg b = c; b.modes[2].lines = 0; refused(4, 37, 64, &b, "zero lines"); b.modes[2].lines = 4097; refused(4, 37, 64, &b, "lines above"); }
  { pysdr_sstv_cfg b = c; b.modes[6].width = 801; b.modes[6].scan_q = 0xF0000000u; refused(4, 37, 64, &b, "width above 800");
    b.modes[6].width = 0; refused(4, 37, 64, &b, "width 0"); }
  { pysdr_sstv_cfg b = c; b.modes[5].code = b.modes[1].code; refused(4, 37, 64, &b, "a duplicate code"); b.modes[5].code = 128; refused(4, 37, 64, &b, "code 128");
    b.modes[5].code = -1; refused(4, 37, 64, &b, "code -1"); }
  { pysdr_sstv_cfg b = c; b.modes[0].scans = 0; refused(4, 37, 64, &b, "scans 0"); b.modes[0].scans = 5; refused(4, 37, 64, &b, "scans 5"); }
  { pysdr_sstv_cfg b = c; b.modes[0].sync_q = 0xFFFFFFFFu; refused(4, 37, 64, &b, "a line of 2^16 samples"); }
  { pysdr_sstv_cfg b = c; b.nmodes = 1; b.modes[0] = pysdr_sstv_mode{1, 1, 1, 1, 0, 0, 2u << 16, 0}; refused(4, 37, 64, &b, "a line of two samples");
    b.modes[0].scan_q = 3u << 16; REQUIRE(sstv_plan(4, 37, 64, &b, &p) && sstv_line_gap(b.modes[0]) == 1, "a line of three samples"); }
  const int nks[] = {1, 7, 8, 9, 16, 17, 800}, mos[] = {1, 16, 63, 64, 65, 256, 4096, 1 << 17};
  for (int nk : nks) for (int mo : mos) {
    REQUIRE(sstv_plan(nk, 37, mo, &c, &p), "good");
    REQUIRE(p.groups * SstvGeom::kRows >= nk && (p.groups - 1) * SstvGeom::kRows < nk, "groups");
    REQUIRE(p.ypitch >= kSstvHpad + mo && p.ypitch % 16 == 0 && (long long)p.cap * nk <= kSstvSlotsMax, "pitch, cap");
  }
  REQUIRE(sizeof(pysdr_sstv_mode) == 32 && sizeof(pysdr_sstv_cfg) == 40 + 16 * 32 && sizeof(SstvC) == 8, "sizes");
  REQUIRE(SstvGeom::kLdsBytes <= 65536 && kSstvLineWords == 800, "LDS");
  // the event words
  for (int i : {0, 1, 4095, (1 << 20) - 1}) for (int kind = 1; kind <= 3; ++kind) for (int nw : {1, 4, 801, 1023}) {
    const int32_t h = sstv_header(i, kind, nw);
    REQUIRE(sstv_header_index(h) == i && sstv_header_kind(h) == kind && sstv_header_words(h) == nw, "header %d %d %d", i, kind, nw);
  }
}

// ---- the pixel boundaries -----------------------------------------------------------------------------------------------
static void boundaries() {
  const double rates[] = {8000, 12000, 25000, 48000};
  for (double fs : rates)
    for (int k = 0; k < kNModes; ++k) {
      const pysdr_sstv_mode m = mode_of(kModes[k], fs);
      REQUIRE(sstv_mode_ok(m), "%s at %g", kModes[k].name, fs);
      const uint32_t e0 = 0xFFFFF000u;                                   // the low 32 bits wrap inside the picture
      uint32_t last = e0;                                                // the sync and the porch lie in front of the first pixel
      long long total = 0;
      const int lines = m.lines < 5 ? m.lines : 3;
      for (int pass = 0; pass < 2; ++pass)
        for (int l = pass == 0 ? 0 : m.lines - lines; l < (pass == 0 ? lines : m.lines); ++l) {
          if (pass == 1 && l == m.lines - lines) last = sstv_pixel_start(m, e0, l, 0, 0) - 1u;
          for (int j = 0; j < m.scans; ++j)
            for (int p = 0; p < m.width; ++p) {
              const uint32_t a = sstv_pixel_start(m, e0, l, j, p), b = sstv_pixel_start(m, e0, l, j, p + 1);
              REQUIRE((int32_t)(b - a) >= 1, "%s at %g: pixel (%d, %d, %d) is empty", kModes[k].name, fs, l, j, p);
              REQUIRE((int32_t)(a - last) >= 0, "%s at %g: pixel (%d, %d, %d) begins inside the one before", kModes[k].name, fs, l, j, p);
              last = b;
              total += (int32_t)(b - a);
            }
        }
      REQUIRE(total > 0, "pixels");
      // the end of a scan's last pixel is the scan's end
      REQUIRE(sstv_pixel_start(m, 0u, 0, 0, m.width) == (uint32_t)(((unsigned long long)m.porch_q + m.scan_q) >> 16), "scan end");
    }
}

// ---- the kernel, as sstv.hip runs it ---------------------------------------------------------------------------------------
struct Bank {
  int nk = 0, L = 0, max_out = 0;
  pysdr_sstv_cfg cfg{};
  SstvPlan plan;
  std::vector<SstvC> tw;
  std::vector<float> g;
  std::vector<SstvC> Y;                    // exactly nk x ypitch
  std::vector<int32_t> si;
  std::vector<float> sf, ring;
  std::vector<uint32_t> lines;
  std::vector<int32_t> events, counts;
  uint64_t m = 0;
  std::vector<std::vector<SstvC>> c_seen;  // per row: the lag products of the tile's own outputs, for the comparison
};

static void make_tables(double fs, int L, std::vector<SstvC>& tw, std::vector<float>& g) {
  tw.resize(kSstvNt);
  for (int k = 0; k < kSstvNt; ++k) tw[(size_t)k] = SstvC{(float)cos(2 * M_PI * k / 1024), (float)-sin(2 * M_PI * k / 1024)};
  std::vector<double> h((size_t)L);
  double sum = 0;
  for (int i = 0; i < L; ++i) {
    const double t = i - (L - 1) / 2.0, fc = 2 * 1900.0 / fs;
    const double s = t == 0 ? fc : sin(M_PI * fc * t) / (M_PI * t);
    h[(size_t)i] = s * (0.54 - 0.46 * cos(2 * M_PI * i / (L - 1)));
    sum += h[(size_t)i];
  }
  g.resize((size_t)L);
  for (int i = 0; i < L; ++i) g[(size_t)i] = (float)(h[(size_t)i] / sum);
}

static Bank make_bank(int nk, double fs, int det, int max_out) {
  Bank b;
  b.nk = nk; b.L = filter_length(fs); b.max_out = max_out; b.cfg = good_cfg(fs, det);
  REQUIRE(sstv_plan(nk, b.L, max_out, &b.cfg, &b.plan), "bank plan");
  make_tables(fs, b.L, b.tw, b.g);
  b.Y.assign((size_t)nk * b.plan.ypitch, SstvC{0.f, 0.f});
  b.si.assign((size_t)kSstvStateInts * nk, 0);
  for (int r = 0; r < nk; ++r) b.si[(size_t)(2 * nk + r)] = -1;
  b.sf.assign((size_t)kSstvStateFloats * nk, 0.f);
  b.ring.assign((size_t)kSstvRing * nk, 0.f);
  b.lines.assign((size_t)kSstvLineWords * nk, 0u);
  b.events.assign((size_t)nk * b.plan.cap, 0);
  b.counts.assign((size_t)nk, 0);
  b.c_seen.assign((size_t)nk, {});
  return b;
}

// one call: rows[r] + at .. + n are the call's outputs
static void run_call(Bank& b, const std::vector<std::vector<SstvC>>& rows, size_t at, int n_out) {
  using G = SstvGeom;
  constexpr int ROWS = G::kRows, T = kSstvTile;
  const int nk = b.nk, L = b.L, H = b.plan.H, lag = b.cfg.lag;
  const long long yp = b.plan.ypitch;
  REQUIRE(n_out >= 1 && n_out <= b.max_out, "call length");
  for (int r = 0; r < nk; ++r)
    for (int i = 0; i < n_out; ++i) b.Y.at((size_t)(r * yp + kSstvHpad + i)) = rows[(size_t)r][at + (size_t)i];
  const uint32_t m0 = (uint32_t)b.m;
  auto Yat = [&](int rr, int i) -> SstvC& { return b.Y.at((size_t)(rr * yp + kSstvHpad + i)); };
  for (int grp = 0; grp < b.plan.groups; ++grp) {
    const int row0 = grp * ROWS;
    std::vector<SstvC> s_v((size_t)G::kPseudo * G::kVp), s_u((size_t)G::kPseudo * G::kUp), s_c((size_t)G::kPseudo * G::kCp);
    std::vector<signed char> s_q((size_t)ROWS * kSstvQMax);
    std::vector<SstvRow> z((size_t)ROWS);
    std::vector<int> cnt((size_t)ROWS, 0);
    for (int t = 0; t < ROWS; ++t) {
      const int row = row0 + t;
      if (row >= nk) continue;
      SstvRow& q = z[(size_t)t];
      q = sstv_row_init();
      const size_t rw = (size_t)row, K = (size_t)nk;
      q.ticks = (uint32_t)b.si[rw]; q.phase = b.si[K + rw]; q.mode = b.si[2 * K + rw]; q.m_a = (uint32_t)b.si[3 * K + rw]; q.e0 = (uint32_t)b.si[4 * K + rw];
      q.line = b.si[5 * K + rw]; q.pix = b.si[6 * K + rw];
      q.acc.x = b.sf[rw]; q.acc.y = b.sf[K + rw]; q.bprev.x = b.sf[2 * K + rw]; q.bprev.y = b.sf[3 * K + rw]; q.f_lead = b.sf[4 * K + rw];
      q.pacc.x = b.sf[5 * K + rw]; q.pacc.y = b.sf[6 * K + rw];
      sstv_row_load(q, b.cfg.modes, &b.lines[rw * kSstvLineWords]);
    }
    for (int i0 = 0; i0 < n_out; i0 += T) {
      std::vector<int> vdone(s_v.size(), 0), udone(s_u.size(), 0), cdone(s_c.size(), 0);
      for (int k = 0; k < G::mix_n(L); ++k) {
        const int pr = G::mix_pr(k, L), cc = G::mix_col(k, L);
        REQUIRE(pr < G::kPseudo && cc < L + T, "mixer index");
        const int i = G::base(i0, pr, lag) + G::mix_rel(cc, L), rr = row0 + G::row(pr);
        REQUIRE(i - 1 >= -H, "the mixer reads in front of the history");
        SstvC v{0.f, 0.f};
        if (rr < nk && i < n_out) v = sstv_mix(Yat(rr, i), Yat(rr, i - 1), m0 + (uint32_t)i, b.cfg.det, b.cfg.w_sub, b.tw.data());
        s_v.at((size_t)G::v_at(pr, cc)) = v;
        REQUIRE(vdone[(size_t)G::v_at(pr, cc)]++ == 0, "product written twice");
      }
      for (int k = 0; k < G::fir_n(); ++k) {
        const int pr = G::fir_pr(k), kk = G::fir_col(k);
        const int newest = G::fir_newest(pr, kk, L);
        REQUIRE(newest - (L - 1) >= pr * G::kVp && newest < pr * G::kVp + L + T, "the window leaves its pseudo-row");
        for (int i = 0; i < L; ++i) REQUIRE(vdone.at((size_t)(newest - i)) == 1, "the window reads a slot never written");
        s_u.at((size_t)G::u_at(pr, kk)) = sstv_fir(&s_v[(size_t)newest], b.g.data(), L);
        REQUIRE(udone[(size_t)G::u_at(pr, kk)]++ == 0, "u written twice");
      }
      for (int k = 0; k < G::lag_n(); ++k) {
        const int pr = G::lag_pr(k), jj = G::lag_col(k);
        REQUIRE(udone.at((size_t)G::u_at(pr, jj + 1)) == 1 && udone.at((size_t)G::u_at(pr, jj)) == 1, "c reads a slot never written");
        s_c.at((size_t)G::c_at(pr, jj)) = sstv_lag(s_u[(size_t)G::u_at(pr, jj + 1)], s_u[(size_t)G::u_at(pr, jj)], b.cfg.pmax);
        REQUIRE(cdone[(size_t)G::c_at(pr, jj)]++ == 0, "c written twice");
      }
      for (size_t k = 0; k < cdone.size(); ++k) REQUIRE(cdone[k] == 1, "a lag product was not computed");
      for (int t = 0; t < ROWS; ++t) {
        const int row = row0 + t;
        if (row >= nk) continue;
        const int nj = n_out - i0 < T ? n_out - i0 : T;
        for (int jj = 0; jj < nj; ++jj) {
          const int i = i0 + jj;
          b.c_seen[(size_t)row].push_back(s_c[(size_t)G::c_at(t, jj)]);
          sstv_step(z[(size_t)t], s_c.at((size_t)G::c_at(t, jj)), s_c.at((size_t)G::c_at(ROWS + t, jj)), &Yat(row, i), m0 + (uint32_t)i, i, b.cfg,
                    b.cfg.modes, b.tw.data(), b.g.data(), L, &b.ring[(size_t)row * kSstvRing], &b.lines[(size_t)row * kSstvLineWords],
                    &s_q[(size_t)t * kSstvQMax], &b.events[(size_t)row * b.plan.cap], cnt[(size_t)t], b.plan.cap);
        }
      }
    }
    // the roll, in chunks of the workgroup's threads: reads of a chunk, then its writes
    const int nroll = ROWS * H;
    std::vector<int> moved((size_t)nroll, 0);
    for (int k0 = 0; k0 < nroll; k0 += G::kThreads) {
      std::vector<SstvC> keep((size_t)G::kThreads);
      for (int t = 0; t < G::kThreads; ++t) {
        const int k = k0 + t;
        if (k < nroll && row0 + G::roll_row(k, H) < nk) keep[(size_t)t] = Yat(row0 + G::roll_row(k, H), G::roll_src(k, H, n_out));
      }
      for (int t = 0; t < G::kThreads; ++t) {
        const int k = k0 + t;
        if (k < nroll && row0 + G::roll_row(k, H) < nk) { Yat(row0 + G::roll_row(k, H), G::roll_dst(k, H)) = keep[(size_t)t]; moved[(size_t)k] += 1; }
      }
    }
    for (int t = 0; t < ROWS; ++t) {
      const int row = row0 + t;
      if (row >= nk) continue;
      for (int c = 0; c < H; ++c) REQUIRE(moved[(size_t)(t * H + c)] == 1, "the roll skipped a sample");
      const SstvRow& q = z[(size_t)t];
      const size_t rw = (size_t)row, K = (size_t)nk;
      sstv_word_flush(q, &b.lines[rw * kSstvLineWords]);
      b.si[rw] = (int32_t)q.ticks; b.si[K + rw] = q.phase; b.si[2 * K + rw] = q.mode; b.si[3 * K + rw] = (int32_t)q.m_a; b.si[4 * K + rw] = (int32_t)q.e0;
      b.si[5 * K + rw] = q.line; b.si[6 * K + rw] = q.pix;
      b.sf[rw] = q.acc.x; b.sf[K + rw] = q.acc.y; b.sf[2 * K + rw] = q.bprev.x; b.sf[3 * K + rw] = q.bprev.y; b.sf[4 * K + rw] = q.f_lead;
      b.sf[5 * K + rw] = q.pacc.x; b.sf[6 * K + rw] = q.pacc.y;
      b.counts[rw] = cnt[(size_t)t];
    }
  }
  // the history now in front of every row is the stream's last H samples
  for (int r = 0; r < nk; ++r)
    for (int c = 1; c <= H; ++c) {
      const long long src = (long long)at + n_out - c;
      const SstvC want = src >= 0 ? rows[(size_t)r][(size_t)src] : SstvC{0.f, 0.f};
      const SstvC got = Yat(r, -c);
      REQUIRE(memcmp(&got, &want, sizeof(SstvC)) == 0, "history of row %d at -%d after the call at %zu", r, c, at);
    }
  b.m += (uint64_t)n_out;
}

// ---- the plain transcription of DESIGN.md 3 item 30 over a whole stream --------------------------------------------------------
struct Event { long long m; std::vector<int32_t> words; };
struct Plain { std::vector<Event> events; std::vector<SstvC> c; int phase = 0; long long ticks = 0; int line = 0, pix = 0; };

static float plain_hz(float re, float im, float k_hz) {
  float t;
  if (re > 0.f) { t = im / re; if (t > 1.f) t = 1.f; if (t < -1.f) t = -1.f; }
  else t = im > 0.f ? 1.f : (im < 0.f ? -1.f : 0.f);
  const float t2 = t * t;
  float s = t2 * 0.0208351f;
  s = -0.0851330f + s; s = t2 * s;
  s = 0.1801410f + s; s = t2 * s;
  s = -0.3302995f + s; s = t2 * s;
  s = 0.9998660f + s;
  const float phi = t * s;
  return phi * k_hz;
}

static Plain plain(const std::vector<SstvC>& y, const pysdr_sstv_cfg& cfg, const std::vector<SstvC>& tw, const std::vector<float>& g) {
  const long long N = (long long)y.size();
  const int L = (int)g.size();
  auto Y = [&](long long n) { return n >= 0 ? y[(size_t)n] : SstvC{0.f, 0.f}; };
  // steps 1 and 2 for the samples -1 .. N - 1 (u) and 0 .. N - 1 (c)
  std::vector<SstvC> v((size_t)(N + L + 1)), u((size_t)(N + 1));
  for (long long n = -L - 1; n < N; ++n) {
    const SstvC t = tw[(size_t)(((uint32_t)n * cfg.w_sub) >> 22)];
    SstvC o;
    if (cfg.det == 0) { const float d = Y(n).y * Y(n - 1).x - Y(n).x * Y(n - 1).y; o = SstvC{d * t.x, d * t.y}; }
    else o = SstvC{Y(n).x * t.x - Y(n).y * t.y, Y(n).x * t.y + Y(n).y * t.x};
    v[(size_t)(n + L + 1)] = o;
  }
  for (long long n = -1; n < N; ++n) {
    float re = 0.f, im = 0.f;
    for (int i = 0; i < L; ++i) {
      const SstvC o = v[(size_t)(n - i + L + 1)];
      if (i == 0) { re = g[0] * o.x; im = g[0] * o.y; } else { re = re + g[(size_t)i] * o.x; im = im + g[(size_t)i] * o.y; }
    }
    u[(size_t)(n + 1)] = SstvC{re, im};
  }
  Plain out;
  out.c.resize((size_t)N);
  for (long long n = 0; n < N; ++n) {
    const SstvC a = u[(size_t)(n + 1)], b = u[(size_t)n];
    const float pa = a.x * a.x + a.y * a.y, pb = b.x * b.x + b.y * b.y;
    out.c[(size_t)n] = (pa <= cfg.pmax && pb <= cfg.pmax) ? SstvC{a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y} : SstvC{0.f, 0.f};
  }
  auto C = [&](long long n) { return n >= 0 ? out.c[(size_t)n] : SstvC{0.f, 0.f}; };
  // steps 4 to 8, one output after the other
  std::vector<float> h;                                                   // every tick's frequency
  float ar = 0.f, ai = 0.f, br = 0.f, bi = 0.f, f_lead = 0.f;
  int phase = 0, mode = -1, line = 0, pix = 0;
  long long m_a = 0, e0 = 0;
  std::vector<uint8_t> bytes;
  for (long long m = 0; m < N; ++m) {
    if ((uint32_t)((uint32_t)m * cfg.w_tick) < cfg.w_tick) { ar = C(m).x; ai = C(m).y; } else { ar = ar + C(m).x; ai = ai + C(m).y; }
    if ((uint32_t)((uint32_t)(m + 1) * cfg.w_tick) < cfg.w_tick) {
      h.push_back(plain_hz(ar + br, ai + bi, cfg.k_hz));
      br = ar; bi = ai;
      const long long k = (long long)h.size() - 1;
      auto Hk = [&](long long j) { return k - j >= 0 ? h[(size_t)(k - j)] : 0.f; };
      if (phase == 0) {
        const float f = (((Hk(34) + Hk(40)) + Hk(46)) + Hk(52)) * 0.25f;
        bool ok = fabsf(f) <= 150.f;
        for (int j = 34; j <= 52; j += 6) ok = ok && fabsf(Hk(j) - f) <= 40.f;
        int code = 0, ones = 0;
        for (int bb = 0; bb < 10 && ok; ++bb) {
          const float x = Hk(3 * bb + 1) - f;
          if (bb == 0 || bb == 9) { ok = fabsf(x + 700.f) <= 40.f; continue; }
          int bit = -1;
          if (fabsf(x + 800.f) <= 40.f) bit = 1; else if (fabsf(x + 600.f) <= 40.f) bit = 0;
          if (bit < 0) { ok = false; break; }
          ones += bit;
          if (bb >= 2) code |= bit << (8 - bb);
        }
        int found = -1;
        for (int i = 0; i < cfg.nmodes && ok && !(ones & 1); ++i) if (cfg.modes[i].code == code) found = i;
        if (found >= 0) { phase = 1; mode = found; f_lead = f; m_a = m + (cfg.modes[found].sync_q >> 16) + cfg.R0 + cfg.W; }
      }
    }
    if (phase == 1 && m == m_a) {
      // step 6 by its definition: D[e] over the candidates, the first of the greatest
      const pysdr_sstv_mode& md = cfg.modes[mode];
      const long long m_v = m_a - (md.sync_q >> 16) - cfg.R0 - cfg.W, centre = m_v + 1 + (md.sync_q >> 16);
      const SstvC rho = tw[(size_t)((int)floorf((f_lead - 550.f) * cfg.k_rho + 0.5f) & 1023)];
      auto Q = [&](long long n) { const SstvC c = C(n); if (c.x == 0.f && c.y == 0.f) return 0; return (c.x * rho.y + c.y * rho.x) < 0.f ? 1 : -1; };
      long long best = -(1ll << 40);
      for (long long e = centre - cfg.R0; e <= centre + cfg.R0; ++e) {
        long long D = 0;
        for (int k = 1; k <= cfg.W; ++k) D += Q(e - k);
        for (int k = 0; k < cfg.W; ++k) D -= Q(e + k);
        if (D > best) { best = D; e0 = e; }
      }
      REQUIRE(centre + cfg.R0 + cfg.W - 1 == m_a, "the anchor looks past the output it is taken at");
      phase = 2; line = 0; pix = 0;
      union { float f; int32_t i; } fb; fb.f = f_lead;
      out.events.push_back(Event{m, {sstv_header(0, 1, 4), mode, md.code, fb.i, (int32_t)(uint32_t)e0}});
    } else if (phase == 2) {
      // step 7: does a pixel end with the sample n = m - lag?
      const pysdr_sstv_mode& md = cfg.modes[mode];
      const long long n = m - cfg.lag;
      const unsigned long long X = (unsigned long long)md.sync_q + md.porch_q + (unsigned long long)md.scans * ((unsigned long long)md.scan_q + md.sep_q);
      const int j = pix / md.width, p = pix % md.width;
      const unsigned long long at0 = (unsigned long long)line * X + md.porch_q + (unsigned long long)j * ((unsigned long long)md.scan_q + md.sep_q);
      const long long a = e0 + (long long)((at0 + (unsigned long long)p * md.scan_q / (unsigned long long)md.width) >> 16);
      const long long a1 = e0 + (long long)((at0 + (unsigned long long)(p + 1) * md.scan_q / (unsigned long long)md.width) >> 16);
      if (n == a1 - 1) {
        float pr = 0.f, pi = 0.f;
        for (long long s = a; s < a1; ++s) { if (s == a) { pr = C(s).x; pi = C(s).y; } else { pr = pr + C(s).x; pi = pi + C(s).y; } }
        float val = plain_hz(pr, pi, cfg.k_hz) - f_lead;
        val = val + 400.f; val = val * (255.f / 800.f); val = floorf(val + 0.5f);
        const int byte = val < 0.f ? 0 : (val > 255.f ? 255 : (int)val);
        if (pix == 0) bytes.assign((size_t)((md.scans * md.width + 3) / 4 * 4), 0);
        bytes[(size_t)pix] = (uint8_t)byte;
        pix += 1;
        if (pix == md.scans * md.width) {
          Event e{m, {sstv_header(0, 2, 1 + (int)bytes.size() / 4), line}};
          for (size_t k = 0; k < bytes.size(); k += 4)
            e.words.push_back((int32_t)((uint32_t)bytes[k] | (uint32_t)bytes[k + 1] << 8 | (uint32_t)bytes[k + 2] << 16 | (uint32_t)bytes[k + 3] << 24));
          out.events.push_back(e);
          pix = 0; line += 1;
          if (line == md.lines) { out.events.push_back(Event{m, {sstv_header(0, 3, 1), md.lines}}); phase = 0; }
        }
      }
    }
  }
  out.phase = phase; out.ticks = (long long)h.size(); out.line = line; out.pix = pix;
  return out;
}

// ---- test signals ---------------------------------------------------------------------------------------------------------
struct Tone { double hz, ms; };

static void add_vis(std::vector<Tone>& t, int code, bool bad_parity = false) {
  t.push_back({1900, 300}); t.push_back({1200, 10}); t.push_back({1900, 300}); t.push_back({1200, 30});
  int ones = 0;
  for (int k = 0; k < 7; ++k) { const int b = code >> k & 1; ones += b; t.push_back({b ? 1100.0 : 1300.0, 30}); }
  t.push_back({((ones & 1) ^ (bad_parity ? 1 : 0)) ? 1100.0 : 1300.0, 30});
  t.push_back({1200, 30});
}

static std::vector<uint8_t> picture(const ModeMs& m, int seed) {
  std::vector<uint8_t> p((size_t)(m.lines * m.scans * m.width));
  for (int l = 0; l < m.lines; ++l) for (int j = 0; j < m.scans; ++j) for (int x = 0; x < m.width; ++x)
    p[(size_t)((l * m.scans + j) * m.width + x)] = (uint8_t)lround(127.5 + 110.0 * sin(2 * M_PI * (1 + (l + j + seed) % 2) * x / m.width + l + 2 * j + seed));
  return p;
}

static void add_picture(std::vector<Tone>& t, const ModeMs& m, const std::vector<uint8_t>& pic) {
  for (int l = 0; l < m.lines; ++l) {
    t.push_back({1200, m.sync}); t.push_back({1500, m.porch});
    for (int j = 0; j < m.scans; ++j) {
      for (int x = 0; x < m.width; ++x) t.push_back({1500.0 + 800.0 * pic[(size_t)((l * m.scans + j) * m.width + x)] / 255.0, m.pixel});
      if (m.sep > 0) t.push_back({1500, m.sep});
    }
  }
}

// a row at fs_out: the station at `off` Hz from where it is expected, amplitude amp, noise of amplitude noise
static std::vector<SstvC> render(const std::vector<Tone>& t, double fs, int det, double off, double amp, double noise) {
  double total = 0;
  for (const Tone& o : t) total += o.ms * 1e-3;
  const long long n = (long long)floor(total * fs);
  std::vector<SstvC> y((size_t)n);
  size_t seg = 0;
  double end = t[0].ms * 1e-3, aph = 0, fph = 0;
  for (long long i = 0; i < n; ++i) {
    while ((i + 0.5) / fs >= end && seg + 1 < t.size()) { seg += 1; end += t[seg].ms * 1e-3; }
    aph += 2 * M_PI * t[seg].hz / fs;
    double ph;
    if (det == 0) { fph += 2 * M_PI * 3000.0 * cos(aph) / fs; ph = fph + 2 * M_PI * off * i / fs; }
    else ph = aph + 2 * M_PI * (off - 1900.0) * i / fs;
    y[(size_t)i] = SstvC{(float)(amp * cos(ph)) + (float)noise * rndf(), (float)(amp * sin(ph)) + (float)noise * rndf()};
  }
  return y;
}

static std::vector<uint8_t> lines_of(const std::vector<Event>& ev, const ModeMs& m, size_t first, int* nlines) {
  std::vector<uint8_t> out;
  *nlines = 0;
  for (size_t k = first; k < ev.size(); ++k) {
    const int kind = sstv_header_kind(ev[k].words[0]);
    if (kind == kSstvEvEnd) break;
    if (kind != kSstvEvLine) continue;
    REQUIRE(ev[k].words[1] == *nlines, "line number");
    for (int q = 0; q < m.scans * m.width; ++q) out.push_back((uint8_t)((uint32_t)ev[k].words[(size_t)(2 + q / 4)] >> (8 * (q % 4))));
    *nlines += 1;
  }
  return out;
}

static void same_events(const std::vector<Event>& a, const std::vector<Event>& b, const char* what) {
  REQUIRE(a.size() == b.size(), "%s: %zu events against %zu", what, a.size(), b.size());
  for (size_t k = 0; k < a.size(); ++k) {
    REQUIRE(a[k].m == b[k].m && a[k].words.size() == b[k].words.size(), "%s: event %zu at %lld / %lld", what, k, a[k].m, b[k].m);
    for (size_t w = 0; w < a[k].words.size(); ++w) REQUIRE(a[k].words[w] == b[k].words[w], "%s: event %zu word %zu", what, k, w);
  }
}

// run the bank over the rows with the calls `cuts` repeated; -> each row's events with absolute m, the header's index zeroed
static std::vector<std::vector<Event>> run_stream(Bank& b, const std::vector<std::vector<SstvC>>& rows, const std::vector<int>& cuts) {
  std::vector<std::vector<Event>> out((size_t)b.nk);
  const size_t N = rows[0].size();
  size_t at = 0, k = 0;
  while (at < N) {
    int n = cuts[k++ % cuts.size()];
    if ((size_t)n > N - at) n = (int)(N - at);
    run_call(b, rows, at, n);
    for (int r = 0; r < b.nk; ++r) {
      const int32_t* ev = &b.events[(size_t)r * b.plan.cap];
      const int cnt = b.counts[(size_t)r];
      REQUIRE(cnt <= b.plan.cap, "count above the cap");
      for (int w = 0; w < cnt;) {
        const int i = sstv_header_index(ev[w]), kind = sstv_header_kind(ev[w]), nw = sstv_header_words(ev[w]);
        REQUIRE(i < n && kind >= 1 && kind <= 3 && w + 1 + nw <= cnt, "event header");
        Event e{(long long)at + i, {sstv_header(0, kind, nw)}};
        for (int q = 0; q < nw; ++q) e.words.push_back(ev[w + 1 + q]);
        out[(size_t)r].push_back(e);
        w += 1 + nw;
      }
    }
    at += (size_t)n;
  }
  return out;
}

static void phases(double fs, int det) {
  const ModeMs& tiny = kModes[kNModes - 2];
  const ModeMs& tiny2 = kModes[kNModes - 1];
  const std::vector<uint8_t> p0 = picture(tiny, 0), p1 = picture(tiny, 1), p2 = picture(tiny2, 2);
  // row 0: two TINY pictures back to back; row 1: TINY2, 70 Hz off (USB), later; row 2: a header with wrong parity, an
  // unknown code, then noise; rows 3 .. 8: silence, so that the rows are no multiple of the workgroup's
  std::vector<Tone> t0{{1900, 37}}, t1{{1900, 391}}, t2{{1900, 20}};
  add_vis(t0, tiny.code); add_picture(t0, tiny, p0); add_vis(t0, tiny.code); add_picture(t0, tiny, p1); t0.push_back({1900, 150});
  add_vis(t1, tiny2.code); add_picture(t1, tiny2, p2); t1.push_back({1900, 150});
  add_vis(t2, tiny.code, true); add_picture(t2, tiny, p0); add_vis(t2, 7); t2.push_back({1500, 300});
  const int nk = 9;
  std::vector<std::vector<SstvC>> rows((size_t)nk);
  rows[0] = render(t0, fs, det, 0.0, 0.1, 0.001);
  rows[1] = render(t1, fs, det, det == 1 ? 70.0 : 0.0, 0.3, 0.002);
  rows[2] = render(t2, fs, det, 0.0, 0.1, 0.001);
  const size_t N = rows[0].size();
  for (int r = 1; r < nk; ++r) rows[(size_t)r].resize(N, SstvC{0.f, 0.f});
  for (size_t i = 0; i < N; ++i) rows[4][i] = SstvC{0.01f * rndf(), 0.01f * rndf()};
  // inside row 0's first picture: a NaN, an infinite and a sample above pmax
  const size_t bad = (size_t)(1.0 * fs);
  rows[0][bad] = SstvC{NAN, 0.25f}; rows[0][bad + 3 * (size_t)kSstvLmax] = SstvC{-0.5f, INFINITY}; rows[0][bad + 6 * (size_t)kSstvLmax] = SstvC{3e12f, 0.f};

  const std::vector<std::vector<int>> cutsets = {{4096}, {1, 63, 64, 65, 16, 256, 1, 1, 700}, {16}, {256}};
  std::vector<std::vector<Event>> first;
  Bank ref;
  for (size_t cs = 0; cs < cutsets.size(); ++cs) {
    Bank b = make_bank(nk, fs, det, 4096);
    const std::vector<std::vector<Event>> ev = run_stream(b, rows, cutsets[cs]);
    if (cs == 0) { first = ev; ref = b; continue; }
    for (int r = 0; r < nk; ++r) same_events(ev[(size_t)r], first[(size_t)r], "a cut");
    REQUIRE(b.si == ref.si && b.lines == ref.lines && memcmp(b.sf.data(), ref.sf.data(), b.sf.size() * 4) == 0 &&
            memcmp(b.ring.data(), ref.ring.data(), b.ring.size() * 4) == 0, "the state depends on the cut (set %zu)", cs);
  }
  // against the transcription
  long blanked = 0;
  for (int r = 0; r < nk; ++r) {
    const Plain pl = plain(rows[(size_t)r], ref.cfg, ref.tw, ref.g);
    REQUIRE(ref.c_seen[(size_t)r].size() == N && memcmp(ref.c_seen[(size_t)r].data(), pl.c.data(), N * sizeof(SstvC)) == 0, "lag products of row %d", r);
    same_events(first[(size_t)r], pl.events, "the transcription");
    const size_t K = (size_t)nk;
    REQUIRE(ref.si[K + (size_t)r] == pl.phase && (long long)(uint32_t)ref.si[(size_t)r] == pl.ticks, "phase and ticks of row %d", r);
    if (pl.phase == 2) REQUIRE(ref.si[5 * K + (size_t)r] == pl.line && ref.si[6 * K + (size_t)r] == pl.pix, "line and pixel of row %d", r);
    if (r == 0) {
      for (size_t i = bad; i < bad + 6 * (size_t)kSstvLmax; ++i) blanked += pl.c[i].x == 0.f && pl.c[i].y == 0.f;
      long over = 0;
      for (size_t i = bad + 6 * (size_t)kSstvLmax; i < bad + 8 * (size_t)kSstvLmax; ++i) over += pl.c[i].x == 0.f && pl.c[i].y == 0.f;
      REQUIRE(over >= 2, "the sample above pmax blanked %ld lag products", over);
    }
  }
  // a sample that is not finite blanks the L + 1 lag products whose windows hold it (FM: L + 2, it is in two discriminator outputs)
  const int L = filter_length(fs), per = L + 1 + (det == 0 ? 1 : 0);
  REQUIRE(blanked == 2 * per, "%ld lag products blanked, 2 x %d expected", blanked, per);
  // what was sent is what was read
  REQUIRE(first[0].size() == 2 * (size_t)(2 + tiny.lines) && first[1].size() == (size_t)(2 + tiny2.lines) && first[2].empty(), "events: %zu %zu %zu",
          first[0].size(), first[1].size(), first[2].size());
  for (int r = 3; r < nk; ++r) REQUIRE(first[(size_t)r].empty(), "row %d has events", r);
  int nl = 0;
  const std::vector<uint8_t> g1 = lines_of(first[0], tiny, 2 + (size_t)tiny.lines, &nl);
  REQUIRE(nl == tiny.lines && g1.size() == p1.size(), "second picture");
  double err = 0;
  for (size_t k = 0; k < g1.size(); ++k) err += abs((int)g1[k] - (int)p1[k]);
  REQUIRE(err / (double)g1.size() < 6.0, "second picture's mean error %.2f", err / (double)g1.size());
  const std::vector<uint8_t> g2 = lines_of(first[1], tiny2, 0, &nl);
  REQUIRE(nl == tiny2.lines && g2.size() == p2.size(), "row 1's picture");
  err = 0;
  for (size_t k = 0; k < g2.size(); ++k) err += abs((int)g2[k] - (int)p2[k]);
  REQUIRE(err / (double)g2.size() < 6.0, "row 1's mean error %.2f", err / (double)g2.size());
  REQUIRE(sstv_header_kind(first[1][0].words[0]) == kSstvEvStart && first[1][0].words[1] == kNModes - 1 && first[1][0].words[2] == tiny2.code, "row 1's start");
  printf("  %s at %g: %zu samples, pictures read, mean error %.2f levels\n", det ? "USB" : "FM", fs, N, err / (double)g2.size());
}

// ---- the cap under the densest stream ---------------------------------------------------------------------------------------
static void cap(double fs) {
  pysdr_sstv_cfg c = good_cfg(fs, 1);
  // the densest mode: the shortest line there is room for with a full line of bytes is not what fills slots fastest; TINY2's
  // 40 bytes in 27 ms and TINY's 96 in 55 ms are, so both tables are tried, and a table of TINY alone
  for (int variant = 0; variant < 2; ++variant) {
    if (variant == 1) { c.nmodes = 1; c.modes[0] = mode_of(kModes[kNModes - 2], fs); }
    const int pick = variant == 1 ? 0 : kNModes - 1;
    const pysdr_sstv_mode& md = c.modes[pick];
    std::vector<std::pair<long long, int>> ev;                             // (output, words)
    SstvRow z = sstv_row_init();
    std::vector<uint32_t> lb(kSstvLineWords);
    std::vector<int32_t> slots(4096);
    const long long N = 40 * (long long)(sstv_line_q(md) >> 16) * md.lines / 10 + 20000;
    long long wait_until = -1, last_line = -(1ll << 40), gap_seen = 1ll << 40;
    for (long long m = 0; m < N; ++m) {
      int cnt = 0;
      if (z.phase == kSstvIdle) {                                          // a VIS matched on this very output, its tick's last
        z.phase = kSstvWait; z.mode = pick; z.f_lead = 0.f;
        wait_until = m + (md.sync_q >> 16) + c.R0 + c.W;
      } else if (z.phase == kSstvWait && m == wait_until) {
        const uint32_t e_lo = (uint32_t)(wait_until - 2 * c.R0 - c.W + 1);   // the earliest candidate
        sstv_start(z, e_lo, 0, c.modes, slots.data(), cnt, (int)slots.size());
      } else if (z.phase == kSstvPicture) {
        sstv_pixel(z, SstvC{1.f, 0.f}, (uint32_t)(m - c.lag), 0, c, c.modes, lb.data(), slots.data(), cnt, (int)slots.size());
      }
      if (cnt) {
        ev.push_back({m, cnt});
        if (cnt > kSstvStartWords) { if (m - last_line < gap_seen) gap_seen = m - last_line; last_line = m; }
      }
    }
    REQUIRE(ev.size() > 30 && gap_seen >= sstv_line_gap(md), "line events %lld apart, the proof says %lld", gap_seen, sstv_line_gap(md));
    const int mos[] = {1, 16, 64, 700, 4096, 20000};
    for (int mo : mos) {
      const long long capw = sstv_event_cap(mo, c);
      long long most = 0;
      size_t lo = 0;
      long long sum = 0;
      for (size_t hi = 0; hi < ev.size(); ++hi) {                          // windows [ev[hi].m - mo + 1, ev[hi].m]
        sum += ev[hi].second;
        while (ev[lo].first <= ev[hi].first - mo) sum -= ev[lo++].second;
        if (sum > most) most = sum;
      }
      REQUIRE(most <= capw, "fs %g max_out %d: %lld words in a call, cap %lld", fs, mo, most, capw);
      REQUIRE(most >= 2 + sstv_line_words(md), "the stream holds no line");
    }
  }
}

int main() {
  rules();
  boundaries();
  phases(12000.0, 1);
  phases(25000.0, 0);
  cap(8000.0); cap(25000.0); cap(48000.0);
  printf("SSTV_PLAN_OK\n");
  return 0;
}
