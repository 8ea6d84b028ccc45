// The fine channelizer's pure half (pysdr_amd/csrc/fine_plan.h) in a stand-alone program: the shape rules against a
// re-derivation, the map between fine channels and (coarse row, kept channel) against brute force, the tiles of a launch,
// and a stream of ragged calls walked with the very index functions the kernel and the host half use -- every tap read
// of every frame must find the stage-1 output it wants in a row buffer of exactly the planned size (AddressSanitizer
// watches its ends), and the roll must leave the history the next call needs.  Before that, the pure half of the FFT
// both stages share (pysdr_amd/csrc/fft_plan.h) for every size either stage accepts: the passes, where they leave every
// channel, the multipliers of their index arithmetic and the twiddle table.  Built and run by tests/test_fine_plan.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "fine_plan.h"

using namespace pysdr;

static int failures = 0;
#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); if (++failures > 20) std::exit(1); } \
  } while (0)

static bool smooth(int M) {
  if (M < 1) return false;
  while (M % 2 == 0) M /= 2;
  while (M % 5 == 0) M /= 5;
  return M == 1;
}

// the rules of DESIGN 3 item 20, written down again
static bool rules(int M1, int D1, int M2, int D2, int n1, int n2, int g, int ng) {
  if (M1 < 16 || M1 > 4096 || !smooth(M1) || D1 < 1 || M1 % D1) return false;
  if (M1 / D1 != 2 && M1 / D1 != 4) return false;
  if (M2 < 16 || M2 > 1024 || !smooth(M2) || D2 < 1 || M2 % D2) return false;
  if (M2 / D2 != 1 && M2 / D2 != 2 && M2 / D2 != 4) return false;
  const int C1 = M1 / D1;
  if (M2 % C1) return false;
  const int Q = M2 / C1;
  if (Q < 8 || Q % 2) return false;
  if (n1 < 1 || n1 > 16 * M1 || n2 < 1 || n2 > 16 * M2) return false;
  const long long Mf = (long long)M1 * Q;
  return g >= 0 && g < Mf && ng >= 1 && ng <= Mf && ng <= 65536;
}

static long plans = 0;

static void check_map(const FinePlan& p) {
  // every output row exactly once, from the (row, kept channel) the definition names
  std::vector<int> seen(p.ng, 0);
  for (int j = 0; j < p.nk1; ++j) {
    const int k1 = (p.k1_first + j) % p.M1, a0 = fine_a0(p, j);
    for (int u = 0; u < p.Q; ++u) {
      const int a = fine_row_of(a0, u, p.Mf);
      CHECK(a >= 0 && a < p.Mf);
      const int G = fine_join(k1, u - p.Q / 2, p.Q, p.Mf);
      CHECK(fine_mod(G - p.g_first, p.Mf) == a);
      int kk, q;
      fine_split(G, p.Q, p.M1, &kk, &q);
      CHECK(kk == k1 && q == u - p.Q / 2 && fine_k2(q, p.M2) == (q + p.M2) % p.M2);
      if (a < p.ng) ++seen[a];
    }
  }
  for (int a = 0; a < p.ng; ++a) CHECK(seen[a] == 1);
  // ... and no coarse row is used in vain (unless one serves both ends of the whole raster)
  for (int a = 0; a < p.ng; ++a) {
    int k1, q;
    fine_split((p.g_first + a) % p.Mf, p.Q, p.M1, &k1, &q);
    CHECK(fine_mod(k1 - p.k1_first, p.M1) < p.nk1);
  }
}

static void check_tiles(const FinePlan& p) {
  CHECK(p.slots >= 1 && p.slots <= kFineSlotsMax && (p.slots & (p.slots - 1)) == 0);
  CHECK(p.mp % 2 == 1 && p.mp >= p.M2 && p.lds_bytes == p.slots * p.mp * 8 && p.lds_bytes <= 160 * 1024 / 2);
  CHECK(p.hist >= p.P2 * p.M2 && p.hist % 16 == 0 && p.hist <= kFineRollThreads * kFineRollPer);
  int prod = 1;
  for (int s = 0; s < p.npass; ++s) prod *= p.radix[s];
  CHECK(prod == p.M2 && p.npass <= kFftMaxPass);
  for (int nf : {1, 2, 3, 15, 16, 17, 63, 64, 65, 257}) {
    const FineTile t = fine_tile(p, nf);
    CHECK(t.fw * t.rw == p.slots && (t.fw & (t.fw - 1)) == 0);
    CHECK(t.gx * t.fw >= nf && (t.gx - 1) * t.fw < nf && t.gy * t.rw >= p.nk1 && (t.gy - 1) * t.rw < p.nk1);
    CHECK(t.fw == p.slots || t.fw >= nf);
  }
}

// A stream in ragged calls: the row buffer holds the absolute index of the stage-1 output kept there (-1: before the
// stream's start, -2: never written).
static void walk_stream(const FinePlan& p, int ntaps2, unsigned seed) {
  const int D = p.D, cap1 = 3 * p.M2 / p.D2 * p.D2 + 40;          // most stage-1 outputs of a call here
  const long long pitch1 = p.hist + cap1;
  std::vector<long long> row((size_t)pitch1, -2);
  for (int i = 0; i < p.hist; ++i) row[i] = -1;                   // reset: zeros in front of the stream
  unsigned long long s0 = 0;
  long long frames = 0;
  for (int call = 0; call < 60; ++call) {
    seed = seed * 1664525u + 1013904223u;
    int n = (int)((seed >> 8) % (unsigned)(cap1 * p.D1));
    if (call % 7 == 0) n = 0;
    if (call % 7 == 1) n = 1;
    if (call % 7 == 2) n = p.D1;                                   // completes a stage-1 output, rarely a fine one
    const unsigned long long s1 = s0 + n;
    const long long mf = (s0 + D - 1) / D, ml = (s1 + D - 1) / D;
    const long long m1f = (s0 + p.D1 - 1) / p.D1, m1l = (s1 + p.D1 - 1) / p.D1;
    const int n1 = (int)(m1l - m1f);
    CHECK(n1 <= cap1);
    for (int i = 0; i < n1; ++i) row[p.hist + i] = m1f + i;       // stage 1 writes behind the history
    for (long long m = mf; m < ml; ++m) {
      CHECK(m * p.D2 >= m1f && m * p.D2 < m1l);                   // complete when stage-1 output m D2 is
      for (int pp = 0; pp < (ntaps2 + p.M2 - 1) / p.M2; ++pp)
        for (int r = 0; r < p.M2; ++r) {
          if (pp * p.M2 + r >= ntaps2) continue;
          const long long t = fine_tap_index(m, p.D2, pp, p.M2, r), pos = fine_pos(p.hist, t, m1f);
          CHECK(pos >= 0 && pos < p.hist + n1);
          const long long got = row.at((size_t)pos);
          CHECK(got == (t < 0 ? -1 : t));
        }
      CHECK(fine_rot(0, (int)(m & 3), p.C2, p.D2, p.M2) == (int)(((-m * p.D2) % p.M2 + p.M2) % p.M2));
      ++frames;
    }
    if (n1 > 0) {                                                  // the roll: every read before any write
      std::vector<long long> v((size_t)kFineRollThreads * kFineRollPer, -3);
      for (int t = 0; t < kFineRollThreads; ++t)
        for (int i = 0; i < kFineRollPer; ++i) {
          const int e = fine_roll_elem(t, i);
          if (e < p.hist) v[(size_t)t * kFineRollPer + i] = row.at((size_t)e + n1);
        }
      std::vector<int> hit(p.hist, 0);
      for (int t = 0; t < kFineRollThreads; ++t)
        for (int i = 0; i < kFineRollPer; ++i) {
          const int e = fine_roll_elem(t, i);
          if (e < p.hist) { row.at((size_t)e) = v[(size_t)t * kFineRollPer + i]; ++hit[e]; }
        }
      for (int e = 0; e < p.hist; ++e) {
        CHECK(hit[e] == 1);
        const long long want = m1l - p.hist + e;
        CHECK(row[e] == (want < 0 ? -1 : want));
      }
    }
    s0 = s1;
  }
  CHECK(frames > 0);
}

// ---- the FFT's pure half (fft_plan.h), shared by both stages: every M = 2^a 5^b in [16, 4096]
static long ffts = 0;

// frames a workgroup of either stage holds for M points, written down again (chan_plan, fine_plan): the most work items a
// pass can present is that many times M / R
static int most_slots(int M) {
  const int fw = M <= 256 ? 16 * (256 / M) : M * 16 <= 16384 ? 16 : M * 8 <= 16384 ? 8 : 4;
  int s = 1;
  while (2 * s * M <= 8192 && 2 * s <= 64) s *= 2;
  return M <= 1024 && s > fw ? s : fw;
}

static void check_fft(int M) {
  int npass = -1, radix[kFftMaxPass];
  const bool ok = fft_factor(M, &npass, radix);
  CHECK(ok == smooth(M));
  if (!ok) return;
  ++ffts;
  // the passes: fives, fours, then a two, making M
  int prod = 1;
  CHECK(npass >= 1 && npass <= kFftMaxPass);
  for (int s = 0; s < npass; ++s) {
    prod *= radix[s];
    CHECK(radix[s] == 5 || radix[s] == 4 || (radix[s] == 2 && s == npass - 1));
    CHECK(s == 0 || radix[s] <= radix[s - 1]);
  }
  CHECK(prod == M);
  // where channel k is left: a permutation, the mixed-radix digit reversal -- digit s of k (least significant first,
  // radix[s]) becomes the s-th most significant digit of the position
  std::vector<int> hit(M, 0);
  for (int k = 0; k < M; ++k) {
    const int pos = fft_position(k, M, npass, radix);
    CHECK(pos >= 0 && pos < M);
    if (pos >= 0 && pos < M) ++hit[pos];
    int rest = k, want = 0;
    for (int s = 0; s < npass; ++s) {
      want = want * radix[s] + rest % radix[s];
      rest /= radix[s];
    }
    CHECK(rest == 0 && pos == want);
  }
  for (int i = 0; i < M; ++i) CHECK(hit[i] == 1);
  // the multipliers divide exactly, for every work item a pass of either kernel can present
  const FftPasses f = fft_passes(M, npass, radix);
  CHECK(f.npass == npass);
  const int slots = most_slots(M);
  CHECK(slots * M <= 16384);
  int nb = M;
  for (int s = 0; s < npass; ++s) {
    const int R = radix[s], per = M / R, nq = nb / R;
    CHECK(f.radix[s] == R && f.magic_per[s] == magic_of(per));
    for (int it = 0; it < slots * per; ++it) CHECK((int)(((uint64_t)it * f.magic_per[s]) >> 32) == it / per);
    if (nq > 1) {
      CHECK(f.magic_nq[s] == magic_of(nq));
      for (int j = 0; j < per; ++j) CHECK((int)(((uint64_t)j * f.magic_nq[s]) >> 32) == j / nq);
    } else {
      CHECK(f.magic_nq[s] == 0 && s == npass - 1);
    }
    nb /= R;
  }
  CHECK(nb == 1);
  for (int s = npass; s < kFftMaxPass; ++s) CHECK(f.radix[s] == 0 && f.magic_per[s] == 0 && f.magic_nq[s] == 0);
}

static void check_twiddles(int M) {
  const std::vector<float> tw = fft_twiddles(M);
  CHECK(tw.size() == 2 * (size_t)M);
  for (int j = 0; j < M; ++j) {
    const double ph = 2.0 * M_PI * (double)j / (double)M;
    CHECK(tw.at(2 * (size_t)j) == (float)std::cos(ph) && tw.at(2 * (size_t)j + 1) == (float)std::sin(ph));
  }
  CHECK(tw[0] == 1.0f && tw[1] == 0.0f);
}

int main() {
  for (int M = 16; M <= 4096; ++M) check_fft(M);
  {
    int n, r[kFftMaxPass];
    CHECK(!fft_factor(0, &n, r) && !fft_factor(-16, &n, r) && !fft_factor(48, &n, r) && fft_factor(1, &n, r) && n == 0);
    CHECK(!fft_factor(1 << 17, &n, r) && fft_factor(1 << 16, &n, r) && n == kFftMaxPass);   // never more passes than the arrays hold
  }
  for (int M : {16, 625, 4096}) check_twiddles(M);
  const int M1s[] = {8, 16, 20, 48, 64, 250, 4096, 8192}, C1s[] = {1, 2, 4, 8};
  const int M2s[] = {8, 10, 16, 20, 24, 32, 40, 50, 64, 250, 640, 1024, 1280, 2048}, C2s[] = {1, 2, 4, 5, 8};
  for (int M1 : M1s) for (int C1 : C1s) for (int M2 : M2s) for (int C2 : C2s) {
    if (M1 % C1 || M2 % C2) continue;
    const int D1 = M1 / C1, D2 = M2 / C2;
    const long long Mf = (long long)M1 * (M2 / C1);
    const long long gs[] = {0, 3, Mf / 2, Mf - 1, Mf, -1};
    const long long ngs[] = {0, 1, 7, Mf - 1, Mf, Mf + 1, 65536, 65537};
    for (long long g : gs) for (long long ng : ngs) for (int n2 : {0, 1, 5 * M2 + 3, 8 * M2, 16 * M2, 16 * M2 + 1}) {
      if (g > 2000000000ll || ng > 2000000000ll) continue;
      FinePlan p;
      const bool ok = fine_plan(M1, D1, M2, D2, 8 * M1, n2, (int)g, (int)ng, &p);
      CHECK(ok == rules(M1, D1, M2, D2, 8 * M1, n2, (int)g, (int)ng));
      if (!ok) continue;
      ++plans;
      CHECK(p.Q == M2 / C1 && p.Mf == Mf && p.D == D1 * D2 && p.C2 == C2 && p.P2 == (n2 + M2 - 1) / M2);
      check_tiles(p);
      if (Mf <= 4096 || ng <= 7) check_map(p);
    }
    FinePlan p;
    CHECK(!fine_plan(M1, D1, M2, D2, 0, 8 * M2, 0, 1, &p) && !fine_plan(M1, D1, M2, D2, 16 * M1 + 1, 8 * M2, 0, 1, &p));
  }
  // the whole map and a stream of ragged calls for the shapes the GPU tests use and a few more
  const int shapes[][6] = {{16, 8, 16, 8, 0, 128}, {16, 8, 16, 8, 5, 128}, {64, 16, 32, 32, 64 * 8 - 13, 37}, {256, 128, 20, 5, 705, 3},
                           {640, 320, 256, 128, 7000, 300}, {4096, 2048, 64, 16, 131072 - 500, 1000}, {64, 32, 1024, 256, 100, 9}};
  for (const auto& s : shapes)
    for (int n2 : {8 * s[2], 5 * s[2] + 3, 16 * s[2]}) {
      FinePlan p;
      CHECK(fine_plan(s[0], s[1], s[2], s[3], 8 * s[0], n2, s[4], s[5], &p));
      check_map(p);
      check_tiles(p);
      walk_stream(p, n2, 7u + (unsigned)n2);
    }
  if (failures) return 1;
  std::printf("FINE_PLAN_OK %ld plans, %ld FFT sizes\n", plans, ffts);
  return 0;
}
