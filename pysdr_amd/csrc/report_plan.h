// The pure half of the frame report: once a frame's 91 bits are decoded the whole frame is known --
// its codeword through the generator of ldpc_plan.h, its 79 (FT4: 103) tones through the mode's Costas arrays and Gray map
// -- and the spectrum ring holds the powers that say how strong it was, and where and when exactly: the sum of the sent
// tones on the candidate's own place and on its eight neighbours a fine row and a step away, the sum of all tones, and the
// symbols whose sent tone did not win.  Beside it the row floor, a sum of every bin of a row over a span of symbol steps,
// which the host turns into a noise level.  Here: the tones of a frame, which of the nine places a call may read (a pure
// function of the candidate and the ring's state: the kernel never reads a step it may not), one symbol of a candidate
// (report_symbol), one bin of a floor (floor_bin), the whole candidate as a scalar transcription (report_scalar), the plan
// and every refusal -- the very code the kernels (report.hip) step with, the host half (report_host.h) checks with and
// tests/report_plan/plan_main.cpp runs on the CPU.  float32, every operation rounded on its own (-ffp-contract=off).
// Plain C++: nothing here calls the HIP runtime.
#pragma once

#include "ft_plan.h"
#include "ldpc_plan.h"

namespace pysdr {

constexpr int kReportThreads = 128;        // one workgroup per candidate: lane k < 79 (103) owns symbol k
constexpr int kReportMax = 4096;           // candidates of one call
constexpr int kReportPlaces = 9;           // (dt, dF), dt in -1, 0, 1 outer, dF in -1, 0, 1 inner; place 4 is the candidate's own
constexpr int kReportCols = kReportPlaces + 1;   // the nine sums of the sent tones, then the sum of all tones
constexpr int kReportPitch = 105;          // floats of a column in the LDS: >= 103 and odd, so ten lanes on ten columns meet no bank twice
constexpr int kReportCwBytes = 176;        // the codeword's 174 bits, a byte each
constexpr int kReportLdsBytes = ((kReportCols * kReportPitch * 4 + 15) & ~15) + kReportCwBytes + 4 * 4;   // 4400: columns (to 16 bytes), codeword, two waves' two counts
constexpr int kReportCandWords = 6;        // F, slot0 = t0 mod tr, the mask of places, the message's 96 bits in three words
constexpr int kReportBitsBytes = kLdpcBitsBytes;   // 12: the 91 bits MSB first, as the decoder packs them
constexpr float kReportMissing = -1.0f;    // a place that may not be read
constexpr int kFloorThreads = 64;          // one workgroup per row, a lane per bin: NB <= 62
constexpr int kFloorSymsMax = 128;

// ReportMode (ft_plan.h) names the mode; its numbers are the mode's own
template <int MODE> struct ReportGeom {
  using Mode = FtReportMode<MODE>;
  static constexpr int kSyms = Mode::kSyms, kTones = Mode::kTones, kLag = kFtLag<Mode>, kExtra = kFtExtra<Mode>;
};
static_assert(ReportGeom<kReportFt8>::kSyms <= kReportThreads && ReportGeom<kReportFt4>::kSyms <= kReportThreads, "a lane per symbol");
static_assert(ReportGeom<kReportFt8>::kSyms <= kReportPitch && ReportGeom<kReportFt4>::kSyms <= kReportPitch && kReportPitch % 2 == 1,
              "a column holds every symbol");
static_assert(kLdpcN <= kReportCwBytes && kLdpcK <= kReportThreads, "a lane per systematic bit");
static_assert(FtGeom<Ft8Mode, Ft8Mode::kS1>::kNb <= kFloorThreads && FtGeom<Ft4Mode, Ft4Mode::kS1>::kNb <= kFloorThreads, "a lane per bin");

constexpr bool report_mode_ok(int mode) { return mode == kReportFt8 || mode == kReportFt4; }
constexpr int report_syms(int mode) { return mode == kReportFt8 ? Ft8Mode::kSyms : Ft4Mode::kSyms; }
constexpr bool report_n_ok(long long n) { return n >= 0 && n <= kReportMax; }

// ---- the message, the codeword, the tones ------------------------------------------------------------------------------
// The 12 bytes MSB first as three words: message bit i < 91 is bit 31 - i % 32 of word i / 32, the generator's layout.
inline void report_words(const uint8_t* bits12, uint32_t w[3]) {
  for (int k = 0; k < 3; ++k)
    w[k] = ((uint32_t)bits12[4 * k] << 24) | ((uint32_t)bits12[4 * k + 1] << 16) | ((uint32_t)bits12[4 * k + 2] << 8) | (uint32_t)bits12[4 * k + 3];
}
PYSDR_FT_HD inline int report_popc(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(v);
#else
  return __builtin_popcount(v);
#endif
}
PYSDR_FT_HD inline uint8_t report_msg_bit(uint32_t w0, uint32_t w1, uint32_t w2, int i) {
  const uint32_t w = i < 32 ? w0 : (i < 64 ? w1 : w2);
  return (uint8_t)((w >> (31 - (i & 31))) & 1u);
}
// parity bit j < 83 (codeword bit 91 + j): the generator's row and the message, AND, population count; bits beyond the 91st
// meet zeros in the row
PYSDR_FT_HD inline uint8_t report_parity(uint32_t w0, uint32_t w1, uint32_t w2, int j) {
  return (uint8_t)((report_popc(w0 & kLdpc.gen[j][0]) + report_popc(w1 & kLdpc.gen[j][1]) + report_popc(w2 & kLdpc.gen[j][2])) & 1);
}
// Tone of frame symbol k from the codeword (a byte per bit); *sync: k is a Costas symbol.
template <int MODE>
PYSDR_FT_HD inline int report_tone(const uint8_t* cw, int k, bool* sync) {
  if (MODE == kReportFt8) {
    const int blk = k / 36, r = k - 36 * blk;               // the arrays begin at 0, 36, 72
    *sync = r < 7;
    if (r < 7) return Ft8Mode::costas(r);
    const int d = k - 7 * (blk + 1);                        // data symbol: Ft8Mode::data_sym's inverse
    return Ft8Mode::gray(4 * cw[3 * d] + 2 * cw[3 * d + 1] + cw[3 * d + 2]);
  }
  const int blk = k / 33, r = k - 33 * blk;                 // 0, 33, 66, 99
  *sync = r < 4;
  if (r < 4) return Ft4Mode::costas(4 * blk + r);
  const int d = k - 4 * (blk + 1);
  return Ft4Mode::gray(2 * cw[2 * d] + cw[2 * d + 1]);
}

// ---- which places a call may read ----------------------------------------------------------------------------------------
// A frame that begins at step t is whole and in the ring: pysdr_*_llr's rule for t0, applied to t0 + dt.
PYSDR_FT_HD constexpr bool report_time_ok(long long t, int lag, long long t_done, int tr) {
  return t >= 0 && t + lag < t_done && t_done - t <= tr;
}
PYSDR_FT_HD constexpr int report_wrap(long long F, int nfine) { return (int)(((F % nfine) + nfine) % nfine); }
// bit 3 (dt + 1) + (dF + 1) is set where place (dt, dF) may be read; `circular`: the raster is the whole circle (nk == M)
PYSDR_FT_HD constexpr int report_mask(long long F, long long t0, long long t_done, int nfine, int tr, int lag, bool circular) {
  int m = 0;
  for (int dt = -1; dt <= 1; ++dt)
    for (int dF = -1; dF <= 1; ++dF)
      if (report_time_ok(t0 + dt, lag, t_done, tr) && (circular || (F + dF >= 0 && F + dF < nfine))) m |= 1 << (3 * (dt + 1) + (dF + 1));
  return m;
}

// ---- one symbol of a candidate ---------------------------------------------------------------------------------------------
// Symbol k of the frame (F, slot0 = t0 mod tr) on ring[nk][tr][nb]: v[0 .. 8] the sent tone's power at the nine places (0
// where the mask forbids the place: never read), v[9] the symbol's tones at the candidate's own place added ascending;
// *miss: the sent tone is not strictly greater than every other tone there.
template <int MODE>
PYSDR_FT_HD inline void report_symbol(const float* ring, int tr, int nb, int nsub, int nfine, int F, int slot0, int mask,
                                       const uint8_t* cw, int k, float* v, bool* miss, bool* sync) {
  constexpr int T = ReportGeom<MODE>::kTones;
  const int tone = report_tone<MODE>(cw, k, sync);
  {
    const int row = F / nsub, j = F - row * nsub;
    const int sl = (slot0 + kFtStepsPerSym * k) % tr;
    const float* p = ring + ((size_t)row * (size_t)tr + (size_t)sl) * (size_t)nb + j;
    float pt[T];
#pragma unroll
    for (int t = 0; t < T; ++t) pt[t] = p[2 * t];
    float e = pt[0], r = pt[0];
#pragma unroll
    for (int t = 1; t < T; ++t) {
      e = t == tone ? pt[t] : e;
      r = r + pt[t];
    }
    bool lost = false;
#pragma unroll
    for (int t = 0; t < T; ++t) lost = lost || (t != tone && !(e > pt[t]));
    v[4] = e;
    v[9] = r;
    *miss = lost;
  }
#pragma unroll
  for (int place = 0; place < kReportPlaces; ++place) {
    if (place == 4) continue;
    const int dt = place / 3 - 1, dF = place % 3 - 1;
    float e = 0.f;
    if ((mask >> place) & 1) {
      const int Fn = report_wrap((long long)F + dF, nfine);
      const int row = Fn / nsub, j = Fn - row * nsub;
      const int sl = (slot0 + dt + kFtStepsPerSym * k + tr) % tr;
      e = ring[((size_t)row * (size_t)tr + (size_t)sl) * (size_t)nb + j + 2 * tone];
    }
    v[place] = e;
  }
}
// A column of nsym values added ascending, from the first; a place that was not read is exactly -1.
PYSDR_FT_HD inline float report_column(const float* col, int nsym, bool read) {
  if (!read) return kReportMissing;
  float acc = col[0];
  for (int k = 1; k < nsym; ++k) acc = acc + col[k];
  return acc;
}

// The scalar transcription: one candidate, its 12 bytes of message bits -> power[10], errs[2] = nhard, nsync.
template <int MODE>
inline void report_scalar(const float* ring, int tr, int nb, int nsub, int nfine, int F, int slot0, int mask, const uint8_t* bits12,
                          float* power, int32_t* errs) {
  constexpr int NS = ReportGeom<MODE>::kSyms;
  uint32_t w[3];
  report_words(bits12, w);
  uint8_t cw[kReportCwBytes] = {};
  for (int i = 0; i < kLdpcK; ++i) cw[i] = report_msg_bit(w[0], w[1], w[2], i);
  for (int j = 0; j < kLdpcM; ++j) cw[kLdpcK + j] = report_parity(w[0], w[1], w[2], j);
  float col[kReportCols][kReportPitch];
  int nhard = 0, nsync = 0;
  for (int k = 0; k < NS; ++k) {
    float v[kReportCols];
    bool miss = false, sync = false;
    report_symbol<MODE>(ring, tr, nb, nsub, nfine, F, slot0, mask, cw, k, v, &miss, &sync);
    for (int c = 0; c < kReportCols; ++c) col[c][k] = v[c];
    nhard += miss && !sync ? 1 : 0;
    nsync += miss && sync ? 1 : 0;
  }
  for (int c = 0; c < kReportCols; ++c) power[c] = report_column(col[c], NS, c == kReportPlaces || ((mask >> c) & 1));
  errs[0] = nhard;
  errs[1] = nsync;
}

// ---- the row floor -----------------------------------------------------------------------------------------------------------
// The steps t_end - 4 (nsym - 1) .. t_end in fours are complete and in the ring.
PYSDR_FT_HD constexpr bool floor_nsym_ok(long long nsym) { return nsym >= 1 && nsym <= kFloorSymsMax; }
PYSDR_FT_HD constexpr bool floor_ok(long long t_end, long long nsym, long long t_done, int tr) {
  return floor_nsym_ok(nsym) && t_end - kFtStepsPerSym * (nsym - 1) >= 0 && t_end < t_done &&
         t_done - (t_end - kFtStepsPerSym * (nsym - 1)) <= tr;
}
// Bin b of a row's floor: rows[tr][nb] is the row's ring, slot_end = t_end mod tr; the span is shorter than the ring.
PYSDR_FT_HD inline float floor_bin(const float* rows, int tr, int nb, int slot_end, int nsym, int b) {
  float acc = 0.f;
  for (int i = 0; i < nsym; ++i) {
    const int sl = (slot_end - kFtStepsPerSym * (nsym - 1 - i) + tr) % tr;
    const float p = rows[(size_t)sl * (size_t)nb + b];
    acc = i == 0 ? p : acc + p;
  }
  return acc;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------
inline bool report_plan(int mode, int32_t out[4]) {
  if (!report_mode_ok(mode) || !out) return false;
  out[0] = kReportThreads; out[1] = kReportLdsBytes; out[2] = report_syms(mode); out[3] = kReportMax;
  return true;
}

// ---- kernel arguments and the launches (report.hip) ----------------------------------------------------------------------------
struct ReportArgs {
  const float* ring;       // the skimmer's spectrum ring [nk][tr][nb]
  int tr, nb, nsub, nfine, n;
  const int32_t* cand;     // [n][6]: F, slot0, mask, the message's three words
  float* power;            // [n][10]
  int32_t* errs;           // [n][2]
};

struct FloorArgs {
  const float* ring;
  int tr, nb, nk, slot_end, nsym;
  float* out;              // [nk][nb]
};

}  // namespace pysdr
