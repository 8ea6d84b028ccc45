// The packet skimmer's pure half: settings and their rules, the event cap and its proof's terms, the
// event words, the workgroup's geometry, LDS budget and the index arithmetic of its tile walk, and the decoder's steps
// themselves -- discriminator and mixer for one row sample, the bit window for one tone pair of one row output, the bit
// clock and the HDLC / CRC / frame step -- the very code the kernel (pkt.hip) steps with, the host half (api_pkt.hip) plans
// with and tests/pkt_plan/plan_main.cpp runs on the CPU.  Plain C++: nothing here calls the HIP runtime, and the only
// trace of the device is the function qualifier below.
#pragma once

#include <cfloat>
#include <cstdint>

#include "../../include/pysdr_hip.h"

#if defined(__HIPCC__)
#define PYSDR_PKT_HD __host__ __device__
#else
#define PYSDR_PKT_HD
#endif

namespace pysdr {

constexpr int kPktTile = 64;               // outputs of every row staged at once (behind the L of history)
constexpr int kPktLmin = 8, kPktLmax = 40; // L, the bit window in row samples: fs_out from 9600 to 48000
constexpr int kPktHpad = 48;               // complex samples kept in front of a row of Y: the history's room, >= L
constexpr int kPktSlicers = 8;             // decoders per row
constexpr int kPktDecMax = 1 << 18;        // decoders: nk kPktSlicers
constexpr int kPktMaxOutMax = 1 << 20;     // the header word holds the index within the call above bit 10
constexpr float kPktPmaxMax = 1.0e18f;     // pysdr_fsk_cfg's rule
constexpr int kPktNt = 1024;               // twiddle table: one turn, indexed by a phase word's top ten bits
constexpr int kPktStateInts = 10;          // clk, xprev, xlast, sr, ones, inframe, byte, nb, nbytes, crc
constexpr int kPktFrameBytes = 332;        // a frame's bytes, FCS included; one more shuts the frame
constexpr int kPktFrameWords = 83;         // a decoder's frame buffer
constexpr int kPktMinBytes = 17;           // least bytes of a good frame, FCS included
constexpr int kPktFcsGood = 0xF0B8;        // the CRC's value behind a frame and its FCS
constexpr int kPktCrcInit = 0xFFFF;

// The workgroup: whole rows, 8 rows x 8 slicers = one wavefront of decoders for the serial part; all 256 threads for the
// data-parallel part (discriminator, mixer, bit window), whose result a row's eight slicers share.
struct PktGeom {
  static constexpr int kRows = 8;
  static constexpr int kDecoders = kRows * kPktSlicers;           // the first wavefront owns them
  static constexpr int kThreads = 256;
  static constexpr int kYp = kPktLmax + kPktTile;                 // LDS row pitch of the staged samples (and of v)
  static constexpr int kPp = kPktTile + 1;                        // of the powers: the 8 rows a wavefront reads at once lie on 8 banks
  // tw, g, y, v (two tones, complex), P (two tones)
  static constexpr int kLdsBytes = kPktNt * 8 + kPktLmax * 4 + kRows * kYp * 8 + kRows * kYp * 16 + kRows * kPp * 8;
  // The index arithmetic of the kernel's tile walk, used by pkt.hip and walked by tests/pkt_plan.  LDS indices are into the
  // sample tile [kRows][kYp], of which a row uses L + kPktTile; memory offsets are in complex samples from the row's first
  // output of the call (the history sits at -L .. -1).
  PYSDR_PKT_HD static constexpr int carry_n(int L) { return kRows * L; }                            // samples in front of a tile
  PYSDR_PKT_HD static constexpr int carry_row(int k, int L) { return k / L; }
  PYSDR_PKT_HD static constexpr int carry_col(int k, int L) { return k % L; }
  PYSDR_PKT_HD static constexpr int carry_src(int hr, int hc) { return hr * kYp + kPktTile + hc; }  // LDS: the previous tile's last L
  PYSDR_PKT_HD static constexpr int carry_dst(int hr, int hc) { return hr * kYp + hc; }             // LDS
  PYSDR_PKT_HD static constexpr int hist_off(int hc, int L) { return hc - L; }                      // memory: the row's history
  PYSDR_PKT_HD static constexpr int stage_row(int k) { return k / kPktTile; }                       // staging load k < kRows kPktTile
  PYSDR_PKT_HD static constexpr int stage_col(int k) { return k % kPktTile; }
  PYSDR_PKT_HD static constexpr int stage_dst(int rr, int c, int L) { return rr * kYp + L + c; }    // LDS
  // the mixer's products v: one per staged sample but the first (whose predecessor is not staged): c = 1 .. L + tile - 1
  PYSDR_PKT_HD static constexpr int mix_n(int L) { return kRows * (L + kPktTile - 1); }
  PYSDR_PKT_HD static constexpr int mix_row(int k, int L) { return k / (L + kPktTile - 1); }
  PYSDR_PKT_HD static constexpr int mix_col(int k, int L) { return k % (L + kPktTile - 1) + 1; }
  PYSDR_PKT_HD static constexpr int at(int r, int c) { return r * kYp + c; }                        // LDS: y and v alike
  PYSDR_PKT_HD static constexpr int mix_rel(int c, int L) { return c - L; }                         // the sample's index from the tile's first output
  PYSDR_PKT_HD static constexpr int win(int r, int jj, int L) { return r * kYp + jj + L; }          // LDS: newest v of the tile's output jj
  PYSDR_PKT_HD static constexpr int pw_at(int r, int jj) { return r * kPp + jj; }                   // LDS: the power pair
  PYSDR_PKT_HD static constexpr int roll_src(int n_out, int j, int L) { return n_out - L + j; }     // memory, j < L
  PYSDR_PKT_HD static constexpr int roll_dst(int j, int L) { return j - L; }                        // memory
};
static_assert(kPktLmax <= kPktTile && kPktLmax <= kPktHpad, "the history fits a tile and its room");
static_assert(PktGeom::kDecoders == 64, "the decoders of a workgroup are one wavefront");
static_assert(PktGeom::kRows * kPktTile == 2 * PktGeom::kThreads, "two row outputs per thread");
static_assert(PktGeom::kLdsBytes <= 64 * 1024, "static LDS");

inline bool pkt_cfg_ok(const pysdr_pkt_cfg& c) {
  for (float v : c.gain)
    if (!(v > 0.f && v <= FLT_MAX)) return false;
  if (!(c.pmax > 0.f && c.pmax <= kPktPmaxMax)) return false;
  if (c.w_mark == 0 || c.w_space == 0 || c.w_baud == 0 || c.w_baud > (1u << 29)) return false;   // fs_out >= 8 baud
  return c.pll_shift >= 1 && c.pll_shift <= 4;
}

// ---- the event cap: words one decoder can emit in a call of max_out outputs -------------------------------------------
// A bit is sampled where the clock goes from >= 0 to < 0.  A nudge moves the clock towards 0 and never across it (-1 may
// become 0), so behind a sampling the clock is first >= 0 again with a value below w_baud, gains at most w_baud per output
// from there, and goes negative no sooner than it passes 2^31: two samplings are more than 2^31 / w_baud outputs apart,
// that is at least pkt_sample_gap.  A call of n outputs has at most ceil(n / gap) samplings.
constexpr int pkt_sample_gap(uint32_t w_baud) { return (int)((1u << 31) / w_baud) + 1; }
constexpr int pkt_max_samplings(int n_out, uint32_t w_baud) { return (n_out + pkt_sample_gap(w_baud) - 1) / pkt_sample_gap(w_baud); }
// words of the event of a frame of n bytes (FCS not counted): the header and the bytes, four to a word
PYSDR_PKT_HD constexpr int pkt_event_words(int n) { return 1 + (n + 3) / 4; }
// A good frame of n >= 15 bytes takes 8 (n + 2) samplings for its bytes and 8 for its closing flag, all behind the flag in
// front of it: 8 n + 24 samplings of its own for (n + 7) / 4 words at most, and (n + 7) / 4 <= (8 n + 24) / 24 from n = 9
// on.  The first flag of a call may close a frame carried into it, of up to 330 bytes, with that one sampling; every
// further frame has its samplings inside the call.  So the words are at most 84 + (samplings - 1) / 24.
constexpr int kPktSamplingsPerWord = 24;
constexpr int kPktCarriedWords = 1 + (kPktFrameBytes - 2 + 3) / 4;
constexpr int pkt_event_cap(int max_out, uint32_t w_baud) {
  return kPktCarriedWords + (pkt_max_samplings(max_out, w_baud) - 1) / kPktSamplingsPerWord;
}
static_assert(kPktCarriedWords == 84 && kPktFrameWords * 4 == kPktFrameBytes, "330 bytes and a header; the buffer holds the FCS too");

struct PktPlan {
  int L = 0;
  int ndec = 0;        // decoders: nk kPktSlicers
  int cap = 0;         // event words per decoder
  int groups = 0;      // workgroups
  int ypitch = 0;      // row pitch of Y, complex samples: kPktHpad of history room, then the call's outputs
};

inline bool pkt_plan(int nk, int L, int max_out, const pysdr_pkt_cfg* cfg, PktPlan* p) {
  if (L < kPktLmin || L > kPktLmax || nk < 1 || (long long)nk * kPktSlicers > kPktDecMax || max_out < 1 || max_out > kPktMaxOutMax || !cfg ||
      !pkt_cfg_ok(*cfg))
    return false;
  PktPlan q;
  q.L = L;
  q.ndec = nk * kPktSlicers;
  q.cap = pkt_event_cap(max_out, cfg->w_baud);
  q.groups = (nk + PktGeom::kRows - 1) / PktGeom::kRows;
  q.ypitch = kPktHpad + ((max_out + 15) & ~15);
  *p = q;
  return true;
}

// the header word: (index within the call of the output that completed the closing flag) << 10 | bytes
PYSDR_PKT_HD constexpr int32_t pkt_header(int i, int n) { return (int32_t)(((uint32_t)i << 10) | (uint32_t)n); }
PYSDR_PKT_HD constexpr int pkt_header_index(int32_t w) { return (int)((uint32_t)w >> 10); }
PYSDR_PKT_HD constexpr int pkt_header_bytes(int32_t w) { return (int)((uint32_t)w & 1023u); }

struct alignas(8) PktC { float x, y; };    // a complex sample as the channelizer stores it
struct alignas(16) PktV { float mx, my, sx, sy; };   // a sample's two mixer products: mark, space
struct alignas(8) PktP { float mark, space; };       // a row output's two tone powers

struct PktDec {                        // one decoder's state, in registers for the call
  int32_t clk, xprev, xlast, sr, ones, inframe, byte, nb, nbytes, crc;
  uint32_t word;                       // the frame buffer's word being filled; not state: the buffer holds it between calls
};

PYSDR_PKT_HD inline PktDec pkt_dec_init() {
  PktDec z{};
  z.crc = kPktCrcInit;
  return z;
}

// the word being filled, as the last call left it in the decoder's frame buffer fb
PYSDR_PKT_HD inline bool pkt_word_open(const PktDec& z) { return (z.nbytes & 3) != 0 && z.nbytes < kPktFrameBytes; }
PYSDR_PKT_HD inline void pkt_word_load(PktDec& z, const uint32_t* fb) { z.word = pkt_word_open(z) ? fb[z.nbytes >> 2] : 0u; }
PYSDR_PKT_HD inline void pkt_word_flush(const PktDec& z, uint32_t* fb) {
  if (pkt_word_open(z)) fb[z.nbytes >> 2] = z.word;
}

// Steps 1 and 2's mixer for the row sample of absolute index n (its low 32 bits): d from the sample and the one before
// it, then d times the two tones' table entries.  Every float operation rounds on its own (-ffp-contract=off).
PYSDR_PKT_HD inline PktV pkt_mix(PktC y, PktC y1, uint32_t n, uint32_t w_mark, uint32_t w_space, const PktC* tw) {
  const float d = y.y * y1.x - y.x * y1.y;
  const PktC m = tw[(uint32_t)(n * w_mark) >> 22], s = tw[(uint32_t)(n * w_space) >> 22];
  return PktV{d * m.x, d * m.y, d * s.x, d * s.y};
}

// Step 2's bit window for the row output whose newest product is vw[0] (vw[-i] = v[m - i], i < L): u = sum g[i] v[m - i],
// i ascending, the first term assigned; P = |u|^2, 0 where it is not <= pmax.
PYSDR_PKT_HD inline PktP pkt_tones(const PktV* vw, const float* g, int L, float pmax) {
  float mr = 0.f, mi = 0.f, sr = 0.f, si = 0.f;
  for (int i = 0; i < L; ++i) {
    const PktV v = vw[-i];
    const float gi = g[i];
    if (i == 0) { mr = gi * v.mx; mi = gi * v.my; sr = gi * v.sx; si = gi * v.sy; }
    else { mr = mr + gi * v.mx; mi = mi + gi * v.my; sr = sr + gi * v.sx; si = si + gi * v.sy; }
  }
  const float pm = mr * mr + mi * mi, ps = sr * sr + si * si;
  return PktP{pm <= pmax ? pm : 0.f, ps <= pmax ? ps : 0.f};
}

// step 3
PYSDR_PKT_HD inline int pkt_slice(float gain, PktP p) { return gain * p.space > p.mark ? 1 : 0; }

// Step 4 for one row output: true where a bit is sampled.
PYSDR_PKT_HD inline bool pkt_clock(PktDec& z, int x, uint32_t w_baud, int pll_shift) {
  const int32_t prev = z.clk;
  int32_t c = (int32_t)((uint32_t)z.clk + w_baud);
  if (x != z.xprev) c -= c >> pll_shift;
  z.xprev = x;
  z.clk = c;
  return prev >= 0 && c < 0;
}

PYSDR_PKT_HD inline int32_t pkt_crc_byte(int32_t crc, int32_t b) {
  for (int k = 0; k < 8; ++k) {
    crc = (crc >> 1) ^ (((crc ^ b) & 1) ? 0x8408 : 0);
    b >>= 1;
  }
  return crc;
}

// Steps 5 and 6 at a sampling, for the output of index i within the call: the decoder's frame buffer fb
// [kPktFrameWords], its event slots ev [cap] and the words used so far, cnt.  A frame whose event does not fit is dropped
// (pkt_event_cap: it fits).
PYSDR_PKT_HD inline void pkt_sample(PktDec& z, int x, int i, uint32_t* fb, int32_t* ev, int& cnt, int cap) {
  const int bit = x == z.xlast ? 1 : 0;
  z.xlast = x;
  z.sr = (z.sr >> 1) | (bit << 7);
  if (z.sr == 0x7E) {
    if (z.inframe && z.nb == 7 && z.nbytes >= kPktMinBytes && z.crc == kPktFcsGood) {
      const int n = z.nbytes - 2, nw = (n + 3) >> 2;
      if (cnt + 1 + nw <= cap) {
        ev[cnt++] = pkt_header(i, n);
        for (int k = 0; k < nw; ++k) {
          uint32_t v = (pkt_word_open(z) && k == (z.nbytes >> 2)) ? z.word : fb[k];
          if (k == nw - 1 && (n & 3)) v &= (1u << (8 * (n & 3))) - 1u;
          ev[cnt++] = (int32_t)v;
        }
      }
    }
    pkt_word_flush(z, fb);               // so that the buffer does not depend on where the calls were cut
    z.inframe = 1; z.nb = 0; z.byte = 0; z.nbytes = 0; z.ones = 0; z.crc = kPktCrcInit; z.word = 0u;
    return;
  }
  if (bit) {
    z.ones += 1;
    if (z.ones >= 7) z.inframe = 0;
  } else {
    const bool stuffed = z.ones == 5;
    z.ones = 0;
    if (stuffed) return;
  }
  if (!z.inframe) return;
  z.byte |= bit << z.nb;
  z.nb += 1;
  if (z.nb < 8) return;
  if (z.nbytes < kPktFrameBytes) {
    const int sh = 8 * (z.nbytes & 3);
    z.word = (sh ? z.word : 0u) | ((uint32_t)z.byte << sh);
    if (sh == 24) fb[z.nbytes >> 2] = z.word;
  }
  z.crc = pkt_crc_byte(z.crc, z.byte);
  z.nbytes += 1;
  z.nb = 0;
  z.byte = 0;
  if (z.nbytes > kPktFrameBytes) z.inframe = 0;
}

// ---- kernel arguments and the launch (pkt.hip) -----------------------------------------------------------------------
struct PktArgs {
  PktC* y;                 // Y + kPktHpad: y[a * ypitch + i] = output i of this call, i >= -L the row's history
  long long ypitch;
  int n_out, nk, cap, ndec, L;
  uint32_t m0;             // the low 32 bits of the absolute index of the call's first output
  uint32_t w_mark, w_space, w_baud;
  int pll_shift;
  float pmax;
  const PktC* tw;          // [kPktNt]
  const float* g;          // [L]
  const float* gain;       // [kPktSlicers]
  int32_t* si;             // [kPktStateInts][ndec]
  uint32_t* frames;        // [ndec][kPktFrameWords]
  int32_t* events;         // [ndec][cap]
  int32_t* counts;         // [ndec]
};

}  // namespace pysdr
