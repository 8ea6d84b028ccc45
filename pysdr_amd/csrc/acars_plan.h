// The ACARS skimmer's pure half: settings and their rules, the event cap and its proof's terms, the
// event words, the workgroup's geometry, LDS budget and the index arithmetic of its tile walk, and the decoder's steps
// themselves -- envelope power of one row sample, band-pass and mixer for one row output, the differential detector, the
// bit clock and the frame machine -- the very code the kernel (acars.hip) steps with, the host half (api_acars.hip) plans
// with and tests/acars_plan/plan_main.cpp runs on the CPU.  Plain C++: nothing here calls the HIP runtime, and the only
// trace of the device is the function qualifier below.
#pragma once

#include <cfloat>
#include <cstdint>

#include "../../include/pysdr_hip.h"

#if defined(__HIPCC__)
#define PYSDR_ACARS_HD __host__ __device__
#else
#define PYSDR_ACARS_HD
#endif

namespace pysdr {

constexpr int kAcTile = 64;                // outputs of every row staged at once (behind the 5 L of history)
constexpr int kAcLmin = 8, kAcLmax = 21;   // L, one bit in row samples: fs_out from 19200 to 50000
constexpr int kAcTapsMax = 4 * kAcLmax + 1;   // NT = 4 L + 1
constexpr int kAcHistMax = 5 * kAcLmax;    // NT - 1 + L: the samples in front of a call that its first output needs
constexpr int kAcHpad = 112;               // complex samples kept in front of a row of Y: the history's room, >= 5 L
constexpr int kAcRowsMax = 1 << 15;        // decoders: one per row
constexpr int kAcMaxOutMax = 1 << 20;      // the header word holds the index within the call above bit 10
constexpr float kAcPmaxMax = 1.0e18f;      // pysdr_pkt_cfg's rule
constexpr int kAcNt = 1024;                // twiddle table: one turn, indexed by a phase word's top ten bits
constexpr int kAcStateInts = 9;            // clk, xprev, lev, sr, st, byte, nb, nbytes, crc
constexpr int kAcMaxBytes = 238;           // most bytes of a frame, mode character to ETX / ETB
constexpr int kAcFrameBytes = 240;         // with the BCS
constexpr int kAcFrameWords = 60;          // a decoder's frame buffer
constexpr int kAcMinBytes = 13;            // mode, seven address characters, ack, two label characters, block id, suffix
constexpr int kAcSync = 0x1616, kAcSyncInv = 0xE9E9;   // SYN SYN in the 16-bit register, first bit lowest; and inverted
constexpr int kAcSoh = 0x01, kAcEtx = 0x03, kAcEtb = 0x17;
enum AcSt : int32_t { kAcSearch = 0, kAcSohSt = 1, kAcText = 2, kAcBcs1 = 3, kAcBcs2 = 4 };

// The workgroup: 8 whole rows.  All 256 threads do the data-parallel part (power, band-pass, mixer, detector); one lane
// per row walks the tile's slicer bits in order.
struct AcGeom {
  static constexpr int kRows = 8;
  static constexpr int kThreads = 256;
  static constexpr int kPp = kAcHistMax + kAcTile;                // LDS row pitch of the powers: 5 L of history, then the tile
  static constexpr int kAp = kAcLmax + kAcTile;                   // of the mixed samples a: L in front of the tile
  static constexpr int kXp = kAcTile + 1;                         // of the slicer bits: the 8 rows lie on 8 banks
  // tw, c, p, a, x
  static constexpr int kLdsBytes = kAcNt * 8 + kAcTapsMax * 8 + kRows * kPp * 4 + kRows * kAp * 8 + kRows * kXp * 4;
  // The index arithmetic of the kernel's tile walk, used by acars.hip and walked by tests/acars_plan.  Memory offsets
  // are in complex samples from the row's first output of the call (the history sits at -5 L .. -1).
  PYSDR_ACARS_HD static constexpr int hist(int L) { return 5 * L; }
  PYSDR_ACARS_HD static constexpr int taps(int L) { return 4 * L + 1; }
  // staging: the powers of the samples i0 - 5 L .. i0 + tile - 1 of every row
  PYSDR_ACARS_HD static constexpr int stage_w(int L) { return 5 * L + kAcTile; }
  PYSDR_ACARS_HD static constexpr int stage_n(int L) { return kRows * stage_w(L); }
  PYSDR_ACARS_HD static constexpr int stage_row(int k, int L) { return k / stage_w(L); }
  PYSDR_ACARS_HD static constexpr int stage_col(int k, int L) { return k % stage_w(L); }
  PYSDR_ACARS_HD static constexpr int stage_rel(int c, int L) { return c - 5 * L; }            // the sample's index from the tile's first output
  PYSDR_ACARS_HD static constexpr int p_at(int r, int c) { return r * kPp + c; }               // LDS
  // the mixed samples a of the outputs i0 - L .. i0 + tile - 1
  PYSDR_ACARS_HD static constexpr int mix_w(int L) { return L + kAcTile; }
  PYSDR_ACARS_HD static constexpr int mix_n(int L) { return kRows * mix_w(L); }
  PYSDR_ACARS_HD static constexpr int mix_row(int k, int L) { return k / mix_w(L); }
  PYSDR_ACARS_HD static constexpr int mix_col(int k, int L) { return k % mix_w(L); }
  PYSDR_ACARS_HD static constexpr int mix_rel(int c, int L) { return c - L; }
  PYSDR_ACARS_HD static constexpr int win(int r, int c, int L) { return r * kPp + c + 4 * L; } // LDS: the newest power under a's column c
  PYSDR_ACARS_HD static constexpr int a_at(int r, int c) { return r * kAp + c; }               // LDS
  // the detector: output jj of the tile from a's columns jj + L (new) and jj (one bit earlier)
  PYSDR_ACARS_HD static constexpr int det_row(int k) { return k / kAcTile; }
  PYSDR_ACARS_HD static constexpr int det_col(int k) { return k % kAcTile; }
  PYSDR_ACARS_HD static constexpr int x_at(int r, int jj) { return r * kXp + jj; }             // LDS
  // the history roll at the end of a call
  PYSDR_ACARS_HD static constexpr int roll_n(int L) { return kRows * 5 * L; }
  PYSDR_ACARS_HD static constexpr int roll_row(int k, int L) { return k / (5 * L); }
  PYSDR_ACARS_HD static constexpr int roll_col(int k, int L) { return k % (5 * L); }
  PYSDR_ACARS_HD static constexpr int roll_src(int n_out, int j, int L) { return n_out - 5 * L + j; }   // memory, j < 5 L
  PYSDR_ACARS_HD static constexpr int roll_dst(int j, int L) { return j - 5 * L; }                      // memory
  static constexpr int kRollPerThread = (kRows * kAcHistMax + kThreads - 1) / kThreads;
};
static_assert(kAcHistMax <= kAcHpad, "the history fits its room");
static_assert(AcGeom::kRows * kAcTile == 2 * AcGeom::kThreads, "two row outputs per thread");
static_assert(AcGeom::kRollPerThread == 4, "the roll keeps four samples per thread in registers");
static_assert(AcGeom::kLdsBytes <= 64 * 1024, "static LDS");

inline bool acars_cfg_ok(const pysdr_acars_cfg& c) {
  if (!(c.pmax > 0.f && c.pmax <= kAcPmaxMax)) return false;
  if (c.w_car == 0 || c.w_baud == 0 || c.w_baud > (1u << 29)) return false;   // fs_out >= 8 baud
  return c.pll_shift >= 1 && c.pll_shift <= 4;
}

// ---- the event cap: words a decoder can emit in a call of max_out outputs ---------------------------------------------
// The clock is packet's (pkt_plan.h, pkt_sample_gap): two samplings are more than 2^31 / w_baud outputs apart, that is at
// least acars_sample_gap, and a call of n outputs has at most ceil(n / gap) samplings.
constexpr int acars_sample_gap(uint32_t w_baud) { return (int)((1u << 31) / w_baud) + 1; }
constexpr int acars_max_samplings(int n_out, uint32_t w_baud) { return (n_out + acars_sample_gap(w_baud) - 1) / acars_sample_gap(w_baud); }
// words of the event of a frame of n bytes (BCS not counted): the header and the bytes, four to a word
PYSDR_ACARS_HD constexpr int acars_event_words(int n) { return 1 + (n + 3) / 4; }
// A good frame of n >= 13 bytes takes 8 samplings for its SOH and 8 (n + 2) for its bytes and BCS, all behind the sync
// word in front of it (15 of whose 16 bits may be the BCS of the frame before; the last is its own too): more than
// 8 n + 24 samplings of its own for (n + 7) / 4 words at most, and (n + 7) / 4 <= (8 n + 24) / 24 from n = 9 on.  A frame carried into a call, of up to 238 bytes, may end at
// the call's first sampling; every further frame has its samplings inside the call.  So the words are at most
// 61 + (samplings - 1) / 24.
constexpr int kAcSamplingsPerWord = 24;
constexpr int kAcCarriedWords = 1 + (kAcMaxBytes + 3) / 4;
constexpr int acars_event_cap(int max_out, uint32_t w_baud) {
  return kAcCarriedWords + (acars_max_samplings(max_out, w_baud) - 1) / kAcSamplingsPerWord;
}
static_assert(kAcCarriedWords == 61 && kAcFrameWords * 4 == kAcFrameBytes && kAcFrameBytes == kAcMaxBytes + 2, "238 bytes and a header; the buffer holds the BCS too");

struct AcPlan {
  int L = 0;
  int NT = 0;          // taps: 4 L + 1
  int cap = 0;         // event words per decoder
  int groups = 0;      // workgroups
  int ypitch = 0;      // row pitch of Y, complex samples: kAcHpad of history room, then the call's outputs
};

inline bool acars_plan(int nk, int L, int max_out, const pysdr_acars_cfg* cfg, AcPlan* p) {
  if (L < kAcLmin || L > kAcLmax || nk < 1 || nk > kAcRowsMax || max_out < 1 || max_out > kAcMaxOutMax || !cfg || !acars_cfg_ok(*cfg)) return false;
  AcPlan q;
  q.L = L;
  q.NT = AcGeom::taps(L);
  q.cap = acars_event_cap(max_out, cfg->w_baud);
  q.groups = (nk + AcGeom::kRows - 1) / AcGeom::kRows;
  q.ypitch = kAcHpad + ((max_out + 15) & ~15);
  *p = q;
  return true;
}

// the header word: (index within the call of the output that completed the BCS) << 10 | bytes
PYSDR_ACARS_HD constexpr int32_t acars_header(int i, int n) { return (int32_t)(((uint32_t)i << 10) | (uint32_t)n); }
PYSDR_ACARS_HD constexpr int acars_header_index(int32_t w) { return (int)((uint32_t)w >> 10); }
PYSDR_ACARS_HD constexpr int acars_header_bytes(int32_t w) { return (int)((uint32_t)w & 1023u); }

struct alignas(8) AcC { float x, y; };     // a complex sample as the channelizer stores it; a tap; a table entry

struct AcDec {                         // one decoder's state, in registers for the call
  int32_t clk, xprev, lev, sr, st, byte, nb, nbytes, crc;
  uint32_t word;                       // the frame buffer's word being filled; not state: the buffer holds it between calls
};

PYSDR_ACARS_HD inline AcDec acars_dec_init() { return AcDec{}; }

// the word being filled, as the last call left it in the decoder's frame buffer fb
PYSDR_ACARS_HD inline bool acars_word_open(const AcDec& z) { return (z.nbytes & 3) != 0 && z.nbytes < kAcFrameBytes; }
PYSDR_ACARS_HD inline void acars_word_load(AcDec& z, const uint32_t* fb) { z.word = acars_word_open(z) ? fb[z.nbytes >> 2] : 0u; }
PYSDR_ACARS_HD inline void acars_word_flush(const AcDec& z, uint32_t* fb) {
  if (acars_word_open(z)) fb[z.nbytes >> 2] = z.word;
}

// Step 1: the envelope power of a row sample, 0 where it is not <= pmax (too large, or not finite).
PYSDR_ACARS_HD inline float acars_power(AcC y, float pmax) {
  const float p = y.x * y.x + y.y * y.y;
  return p <= pmax ? p : 0.f;
}

// Steps 2 and 3 for the row output of absolute index m (its low 32 bits) whose newest power is pw[0] (pw[-i] = p[m - i],
// i < NT): b = sum c[i] p[m - i], i ascending, the first term assigned; a = b tw[(m w_car) >> 22].  Every float operation
// rounds on its own (-ffp-contract=off).
PYSDR_ACARS_HD inline AcC acars_mix(const float* pw, const AcC* c, int NT, uint32_t m, uint32_t w_car, const AcC* tw) {
  float br = 0.f, bi = 0.f;
  for (int i = 0; i < NT; ++i) {
    const float p = pw[-i];
    const AcC ci = c[i];
    if (i == 0) { br = ci.x * p; bi = ci.y * p; }
    else { br = br + ci.x * p; bi = bi + ci.y * p; }
  }
  const AcC t = tw[(uint32_t)(m * w_car) >> 22];
  return AcC{br * t.x - bi * t.y, br * t.y + bi * t.x};
}

// Step 4: the slicer bit from a[m] and a[m - L].
PYSDR_ACARS_HD inline int acars_detect(AcC a, AcC aL) {
  const float q = a.y * aL.x - a.x * aL.y;
  return q > 0.f ? 1 : 0;
}

// Step 5 for one row output: true where a bit is sampled.  Packet's clock (pkt_clock).
PYSDR_ACARS_HD inline bool acars_clock(AcDec& z, int x, uint32_t w_baud, int pll_shift) {
  const int32_t prev = z.clk;
  int32_t c = (int32_t)((uint32_t)z.clk + w_baud);
  if (x != z.xprev) c -= c >> pll_shift;
  z.xprev = x;
  z.clk = c;
  return prev >= 0 && c < 0;
}

PYSDR_ACARS_HD inline int32_t acars_crc_byte(int32_t crc, int32_t b) {
  for (int k = 0; k < 8; ++k) {
    crc = (crc >> 1) ^ (((crc ^ b) & 1) ? 0x8408 : 0);
    b >>= 1;
  }
  return crc;
}

PYSDR_ACARS_HD inline int acars_odd_parity(int32_t b) {
  b ^= b >> 4; b ^= b >> 2; b ^= b >> 1;
  return b & 1;
}

// a byte into the decoder's frame buffer at nbytes (a byte that opens a word clears the rest of it) and into the CRC
PYSDR_ACARS_HD inline void acars_store(AcDec& z, uint32_t* fb) {
  if (z.nbytes < kAcFrameBytes) {
    const int sh = 8 * (z.nbytes & 3);
    z.word = (sh ? z.word : 0u) | ((uint32_t)z.byte << sh);
    if (sh == 24) fb[z.nbytes >> 2] = z.word;
  }
  z.crc = acars_crc_byte(z.crc, z.byte);
  z.nbytes += 1;
}

// Steps 6 to 8 at a sampling, for the output of index i within the call: the decoder's frame buffer fb [kAcFrameWords],
// its event slots ev [cap] and the words used so far, cnt.  A frame whose event does not fit is dropped (acars_event_cap:
// it fits).
PYSDR_ACARS_HD inline void acars_sample(AcDec& z, int x, int i, uint32_t* fb, int32_t* ev, int& cnt, int cap) {
  z.lev ^= 1 - x;
  const int bit = z.lev;
  z.sr = (z.sr >> 1) | (bit << 15);
  if (z.st == kAcSearch) {
    if (z.sr == kAcSync || z.sr == kAcSyncInv) {
      if (z.sr == kAcSyncInv) z.lev ^= 1;
      z.st = kAcSohSt; z.nb = 0; z.byte = 0;
    }
    return;
  }
  z.byte |= bit << z.nb;
  z.nb += 1;
  if (z.nb < 8) return;
  const int32_t b = z.byte;
  if (z.st == kAcSohSt) {
    if (b == kAcSoh) {
      acars_word_flush(z, fb);             // so that the buffer does not depend on where the calls were cut
      z.st = kAcText; z.crc = 0; z.nbytes = 0; z.word = 0u;
    } else {
      z.st = kAcSearch;
    }
  } else if (z.st == kAcText) {
    if (!acars_odd_parity(b)) {
      z.st = kAcSearch;
    } else {
      acars_store(z, fb);
      if ((b & 0x7F) == kAcEtx || (b & 0x7F) == kAcEtb) z.st = kAcBcs1;
      else if (z.nbytes >= kAcMaxBytes) z.st = kAcSearch;
    }
  } else if (z.st == kAcBcs1) {
    acars_store(z, fb);
    z.st = kAcBcs2;
  } else {
    acars_store(z, fb);
    const int n = z.nbytes - 2, nw = (n + 3) >> 2;
    if (z.crc == 0 && n >= kAcMinBytes && cnt + 1 + nw <= cap) {
      ev[cnt++] = acars_header(i, n);
      for (int k = 0; k < nw; ++k) {
        uint32_t v = (acars_word_open(z) && k == (z.nbytes >> 2)) ? z.word : fb[k];
        if (k == nw - 1 && (n & 3)) v &= (1u << (8 * (n & 3))) - 1u;
        ev[cnt++] = (int32_t)v;
      }
    }
    z.st = kAcSearch;
  }
  z.nb = 0;
  z.byte = 0;
}

// ---- kernel arguments and the launch (acars.hip) ---------------------------------------------------------------------
struct AcArgs {
  AcC* y;                  // Y + kAcHpad: y[a * ypitch + i] = output i of this call, i >= -5 L the row's history
  long long ypitch;
  int n_out, nk, cap, L;
  uint32_t m0;             // the low 32 bits of the absolute index of the call's first output
  uint32_t w_car, w_baud;
  int pll_shift;
  float pmax;
  const AcC* tw;           // [kAcNt]
  const AcC* c;            // [4 L + 1]
  int32_t* si;             // [kAcStateInts][nk]
  uint32_t* frames;        // [nk][kAcFrameWords]
  int32_t* events;         // [nk][cap]
  int32_t* counts;         // [nk]
};

}  // namespace pysdr
