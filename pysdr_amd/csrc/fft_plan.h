// The pure half of the channelizers' FFT: an M-point inverse DFT, M = 2^a 5^b, as in-place
// decimation-in-frequency passes of radix 5 / 4 / 2 over frames held in LDS (the passes themselves: fft_lds.h).  Here:
// which passes, the multipliers their index arithmetic divides with, where they leave channel k, and the twiddle table.
// The plans of both stages (objects_plan.h: chan_plan, fine_plan.h: fine_plan), their host halves (api_objects.hip,
// api_fine.hip), the checking launch layer of tests/host_san and tests/fine_plan/plan_main.cpp use the very same functions.
// Plain C++: nothing here calls the HIP runtime or names one of its types.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

namespace pysdr {

constexpr int kFftMaxPass = 8;       // 4096 = 4^6 and 4000 = 5^3 4^2 2 take six

// M -> its passes, first to last: the fives, the fours, then a two; false unless M = 2^a 5^b in at most kFftMaxPass passes
inline bool fft_factor(int M, int* npass, int radix[kFftMaxPass]) {
  if (M < 1) return false;
  int twos = 0, fives = 0, n = 0;
  while (M % 2 == 0) { M /= 2; ++twos; }
  while (M % 5 == 0) { M /= 5; ++fives; }
  if (M != 1 || fives + (twos + 1) / 2 > kFftMaxPass) return false;
  for (int i = 0; i < fives; ++i) radix[n++] = 5;
  for (int i = 0; i < twos / 2; ++i) radix[n++] = 4;
  if (twos & 1) radix[n++] = 2;
  *npass = n;
  return true;
}

inline uint32_t magic_of(int d) { return (uint32_t)(0x100000000ull / (unsigned)d) + 1u; }   // d >= 2; exact n / d while n d < 2^32

// What the passes of a kernel need, part of its arguments.  Pass s works on blocks of nb = M / (radix[0] .. radix[s - 1])
// points: work item `it` is butterfly j = it mod (M / R) of frame it / (M / R) (magic_per), and j is column j mod nq of
// block j / nq, nq = nb / R (magic_nq; 0 where nq = 1 and nothing is divided).
struct FftPasses {
  int npass, radix[kFftMaxPass];
  uint32_t magic_per[kFftMaxPass], magic_nq[kFftMaxPass];
};

inline FftPasses fft_passes(int M, int npass, const int* radix) {
  FftPasses f{};
  f.npass = npass;
  int nb = M;
  for (int s = 0; s < npass; ++s) {
    const int R = radix[s];
    f.radix[s] = R;
    f.magic_per[s] = magic_of(M / R);
    f.magic_nq[s] = nb / R > 1 ? magic_of(nb / R) : 0;
    nb /= R;
  }
  return f;
}

// Where the in-place passes leave channel k (the digit reversal): k = k1 + R1 (k2 + R2 (...)) sits at
// k1 M / R1 + k2 M / (R1 R2) + ...
inline int fft_position(int k, int M, int npass, const int* radix) {
  int nb = M, pos = 0;
  for (int s = 0; s < npass; ++s) {
    const int R = radix[s];
    nb /= R;
    pos += (k % R) * nb;
    k /= R;
  }
  return pos;
}

// e^{+j 2 pi j / M}, j < M, as interleaved (re, im): the phase in float64, rounded once
inline std::vector<float> fft_twiddles(int M) {
  std::vector<float> tw(2 * (size_t)M);
  for (int j = 0; j < M; ++j) {
    const double ph = 2.0 * M_PI * (double)j / (double)M;
    tw[2 * (size_t)j] = (float)std::cos(ph);
    tw[2 * (size_t)j + 1] = (float)std::sin(ph);
  }
  return tw;
}

}  // namespace pysdr
