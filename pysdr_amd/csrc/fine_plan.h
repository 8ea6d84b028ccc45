// The fine channelizer's pure half: a first-stage channelizer cuts the band into M1 coarse rows, a
// second, batched stage runs an M2-channel channelizer on every coarse row that is needed and keeps the Q = M2 / C1
// channels that lie inside the row's own spacing.  Here: the shape rules, the map between a fine channel G and (coarse
// row k1, second-stage channel k2), the range of coarse rows a circular range of G uses, the launch geometry of fine.hip
// and the arithmetic of the row buffer (history in front of every row, roll); the second stage's FFT is the first
// stage's, and its pure half is fft_plan.h.  The kernel (fine.hip), the host half
// (api_fine.hip) and tests/fine_plan/plan_main.cpp use the very same functions.  Plain C++: nothing here calls the HIP
// runtime, and the only trace of the device is the function qualifier below.
#pragma once

#include <cstdint>

#include "fft_plan.h"

#if defined(__HIPCC__)
#define PYSDR_FINE_HD __host__ __device__
#else
#define PYSDR_FINE_HD
#endif

namespace pysdr {

constexpr int kFineM2Min = 16, kFineM2Max = 1024;
constexpr int kFineNgMax = 1 << 16;          // fine rows one object may deliver
constexpr int kFineLdsElems = 8192;          // complex elements of LDS a workgroup fills with frames (64 KB: two workgroups per CU)
constexpr int kFineSlotsMax = 64;            // frames (of any rows) per workgroup
constexpr int kFineThreads = 256;
constexpr int kFineRollThreads = 1024;       // one workgroup rolls one row: every item reads kFineRollPer samples, then writes
constexpr int kFineRollPer = 16;             // kFineRollThreads kFineRollPer >= the longest history, 16 kFineM2Max

struct FinePlan {
  int M1 = 0, D1 = 0, M2 = 0, D2 = 0;
  int C1 = 0, C2 = 0;
  int Q = 0;           // kept second-stage channels per coarse row
  int Mf = 0;          // fine channels in all: M1 Q
  int D = 0;           // D1 D2
  int g_first = 0, ng = 0;
  int k1_first = 0, nk1 = 0;   // the circular range of coarse rows the fine range uses
  int npass = 0, radix[kFftMaxPass] = {};     // fft_factor(M2)
  int P2 = 0;          // taps per branch of the second stage
  int hist = 0;        // stage-1 outputs kept in front of every row: P2 M2 rounded up to 16 (>= the P2 M2 - 1 a window reaches back)
  int slots = 0;       // frames per workgroup, a power of two; a launch splits them into rw rows times fw frames
  int mp = 0;          // LDS pitch of a frame (odd)
  int lds_bytes = 0;
};

PYSDR_FINE_HD inline int fine_floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }   // b > 0
PYSDR_FINE_HD inline int fine_mod(int a, int b) { const int r = a % b; return r < 0 ? r + b : r; }       // b > 0

// Fine channel G in [0, Mf) -> the coarse row it lives in, k1 = floor((G + Q/2) / Q) mod M1, and its offset q in
// [-Q/2, Q/2) from that row's centre; its second-stage channel is q mod M2.
PYSDR_FINE_HD inline void fine_split(int G, int Q, int M1, int* k1, int* q) {
  const int c = fine_floor_div(G + Q / 2, Q);
  *k1 = fine_mod(c, M1);
  *q = G - c * Q;
}
PYSDR_FINE_HD inline int fine_k2(int q, int M2) { return fine_mod(q, M2); }
// ... and back: the fine channel of offset q in coarse row k1
PYSDR_FINE_HD inline int fine_join(int k1, int q, int Q, int Mf) { return fine_mod(k1 * Q + q, Mf); }
// Output row of kept channel u = q + Q/2 in [0, Q) of the j-th used coarse row; kept if < ng.  a0 = fine_a0(j).
PYSDR_FINE_HD inline int fine_row_of(int a0, int u, int Mf) { const int a = a0 + u; return a >= Mf ? a - Mf : a; }

// output row of the first kept channel (q = -Q/2) of the j-th used coarse row
inline int fine_a0(const FinePlan& p, int j) {
  const int k1 = (p.k1_first + j) % p.M1;
  return fine_mod(k1 * p.Q - p.Q / 2 - p.g_first, p.Mf);
}

// Pure arithmetic: the plan of a fine channelizer of this shape; false: outside the rules of DESIGN §3 item 20.
inline bool fine_plan(int M1, int D1, int M2, int D2, int ntaps1, int ntaps2, int g_first, int ng, FinePlan* out) {
  FinePlan p;
  int npass1, radix1[kFftMaxPass];                               // the first stage's own plan keeps its passes (chan_plan)
  if (M1 < 16 || M1 > 4096 || D1 < 1 || M1 % D1 != 0 || !fft_factor(M1, &npass1, radix1)) return false;
  const int C1 = M1 / D1;
  if (C1 != 2 && C1 != 4) return false;                          // a coarse row must carry more than its own spacing
  if (M2 < kFineM2Min || M2 > kFineM2Max || D2 < 1 || M2 % D2 != 0 || !fft_factor(M2, &p.npass, p.radix)) return false;
  const int C2 = M2 / D2;
  if (C2 != 1 && C2 != 2 && C2 != 4) return false;
  if (M2 % C1 != 0) return false;
  const int Q = M2 / C1;
  if (Q < 8 || Q % 2 != 0) return false;
  if (ntaps1 < 1 || ntaps1 > 16 * M1 || ntaps2 < 1 || ntaps2 > 16 * M2) return false;
  const int Mf = M1 * Q;
  if (g_first < 0 || g_first >= Mf || ng < 1 || ng > Mf || ng > kFineNgMax) return false;
  p.M1 = M1; p.D1 = D1; p.M2 = M2; p.D2 = D2; p.C1 = C1; p.C2 = C2; p.Q = Q; p.Mf = Mf; p.D = D1 * D2;
  p.g_first = g_first; p.ng = ng;
  // coarse rows: from the row of g_first to the row of the last channel, never more than all of them
  const int c0 = fine_floor_div(g_first + Q / 2, Q), c1 = fine_floor_div(g_first + ng - 1 + Q / 2, Q);
  p.k1_first = fine_mod(c0, M1);
  p.nk1 = c1 - c0 + 1 > M1 ? M1 : c1 - c0 + 1;
  p.P2 = (ntaps2 + M2 - 1) / M2;
  p.hist = (p.P2 * M2 + 15) & ~15;
  p.mp = M2 | 1;
  int s = 1;
  while (2 * s * M2 <= kFineLdsElems && 2 * s <= kFineSlotsMax) s *= 2;
  p.slots = s;
  p.lds_bytes = s * p.mp * 8;
  *out = p;
  return true;
}

// How a launch splits the slots of a workgroup: fw frames (a power of two, as many as the call has, at most all slots)
// times rw = slots / fw rows.  Many frames: whole 128-byte row segments per store; one or two frames: many rows.
struct FineTile { int fw, rw, gx, gy; };
inline FineTile fine_tile(const FinePlan& p, int nframes) {
  FineTile t;
  t.fw = 1;
  while (t.fw < nframes && t.fw < p.slots) t.fw *= 2;
  t.rw = p.slots / t.fw;
  t.gx = (nframes + t.fw - 1) / t.fw;
  t.gy = (p.nk1 + t.rw - 1) / t.rw;
  return t;
}

// ---- the row buffer: row j at j pitch; [0, hist) the last hist stage-1 outputs before this call (zeros before the
// stream's start), [hist, hist + n1) this call's.  Stage-1 output t (absolute) of a call whose first is m1f:
PYSDR_FINE_HD inline long long fine_pos(int hist, long long t, long long m1f) { return (long long)hist + (t - m1f); }
// stage-1 index that tap (p, r) of fine frame m reads
PYSDR_FINE_HD inline long long fine_tap_index(long long m, int D2, int p, int M2, int r) { return m * D2 - (long long)p * M2 - r; }
// where frame m keeps branch r in LDS: (r - m D2) mod M2, m D2 mod M2 = (m mod C2) D2
PYSDR_FINE_HD inline int fine_rot(int r, int m_lo, int C2, int D2, int M2) {
  const int q = r - (m_lo & (C2 - 1)) * D2;
  return q < 0 ? q + M2 : q;
}
// roll: new [0, hist) = old [n1, n1 + hist): item t of kFineRollThreads moves elements t + i kFineRollThreads, i < kFineRollPer
PYSDR_FINE_HD inline int fine_roll_elem(int t, int i) { return t + i * kFineRollThreads; }

// kernel arguments of one call (fine.hip)
struct FineArgs {
  const float* rows;      // float2 [nk1][pitch1] as floats (plain C++ here); history first
  long long pitch1;
  int hist, M2, D2, C2, P2, L2, mp;
  int off;                // fine_pos of stage-1 index mf D2: hist + (mf D2 - m1f)
  int mf_lo;              // mf mod 4
  int nframes, nk1, fw, rw, fw_shift;
  const float* taps;      // [P2][M2], zero beyond L2 (never multiplied)
  const float* tw;        // float2 [M2] e^{+j 2 pi j / M2}
  const int* perm;        // [Q] LDS position of kept channel u (second-stage channel (u - Q/2) mod M2)
  const int* a0;          // [nk1] output row of the first kept channel of every used coarse row
  int Q, Mf, ng;
  float* y;               // float2 y[a * pitch + (m - mf)]
  long long pitch;
  uint32_t magic_M2, magic_Q;
  FftPasses fft;          // of M2 points (fft_plan.h)
};

}  // namespace pysdr
