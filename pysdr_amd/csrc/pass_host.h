// The host half of the second pass, shared by the FT8 and the FT4 skimmer (api_ft.hip) over
// skimmer_host.h as report_host.h is: the two rings and the tables a skimmer owns once pysdr_*_keep was called, the launch
// a process call queues for them, and the calls -- keep, subtract, rescan, state, and the decoder on the residue -- written
// once for both objects.  The jobs of a subtraction are expanded here by pass_plan.h's pure functions.  Every check comes
// before any launch: a refusal changes nothing.  Host only; not part of the public ABI.
#pragma once

#include <algorithm>

#include "ldpc_host.h"
#include "pass_plan.h"
#include "skimmer_host.h"

namespace pysdr {

struct PassBufs {                   // allocated by pysdr_*_keep
  bool kept = false;
  int reach_t = 0, trials = 0;
  PassPlan plan;
  unsigned long long n_abs = 0;     // row samples since create / reset: yk holds the last plan.ty of them
  DevBuf<FtC> d_yk;                 // [nk][ty]
  DevBuf<float> d_ring2;            // [nk][tr2][nb]
  DevBuf<uint32_t> d_pulse;         // [kPassPulse S]
  DevBuf<FtC> d_lut;                // [4096]
  DevBuf<int32_t> d_jobs;           // [kPassJobsMax][30]
  DevBuf<int32_t> d_rows;           // [kPassJobsMax][2]
  DevBuf<int32_t> d_out;            // [kPassMax][2][4]
  DevBuf<int32_t> d_counts;         // [kPassRowsMax]
  DevBuf<int32_t> d_events;         // [kPassRowsMax][52][2]
  std::vector<uint32_t> h_pulse;
  std::vector<float> h_lut;
  std::vector<PassJob> h_jobs;
  std::vector<int32_t> h_rows;
};

inline int pass_clear(PassBufs* b, int nk, int nb, hipStream_t st) {
  if (!b->kept) return PYSDR_OK;
  PYSDR_HIP_CHECK(hipMemsetAsync(b->d_yk.get(), 0, (size_t)nk * (size_t)b->plan.ty * sizeof(FtC), st));
  PYSDR_HIP_CHECK(hipMemsetAsync(b->d_ring2.get(), 0, (size_t)nk * (size_t)b->plan.tr2 * (size_t)nb * sizeof(float), st));
  b->n_abs = 0;
  return PYSDR_OK;
}

inline int pass_not_kept(const char* who) {
  set_last_error("%s: nothing is kept for a second pass: call the skimmer's keep after create or reset", who);
  return PYSDR_ERR_STATE;
}

template <class W>
int pass_keep(W* w, const char* who, const PassCfg* cfg) {
  using Mode = typename W::Mode;
  if (!w) return no_skimmer(who);
  if (!pass_cfg_ok(cfg)) {
    set_last_error("%s: a cfg outside the rules (NULL; reach_t in [1, %d]; trials in [1, %d]; pulse and lut not NULL)", who, kPassReachMax,
                   kPassTrials);
    return PYSDR_ERR_ARG;
  }
  std::lock_guard<std::mutex> lk(w->mu);
  ChanInfo ci;
  int rc = chan_info(w->ch, &ci);
  if (rc != PYSDR_OK) return rc;
  if (w->t_done != 0 || ci.n_abs != 0) {
    set_last_error("%s: the stream has begun (%llu samples in, %llu steps done): keep comes after create or reset", who, ci.n_abs, w->t_done);
    return PYSDR_ERR_STATE;
  }
  PassPlan p;
  if (!pass_plan<Mode>(w->nk, w->plan.S, w->max_out, cfg->reach_t, &p)) {
    set_last_error("%s: a sample ring or a residue ring above %lld bytes (%d rows, reach_t %d)", who, kFtRingBytesMax, w->nk, cfg->reach_t);
    return PYSDR_ERR_ARG;
  }
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));                          // the host tables may still feed an earlier copy
  PassBufs& b = w->pass;
  b.kept = false;
  const size_t np = (size_t)kPassPulse<Mode> * (size_t)w->plan.S;
  b.h_pulse.assign(cfg->pulse, cfg->pulse + np);
  b.h_lut.assign(cfg->lut, cfg->lut + 2 * (size_t)kPassLut);
  PYSDR_HIP_CHECK(b.d_yk.alloc((size_t)w->nk * (size_t)p.ty));
  PYSDR_HIP_CHECK(b.d_ring2.alloc((size_t)w->nk * (size_t)p.tr2 * (size_t)w->plan.nb));
  PYSDR_HIP_CHECK(b.d_pulse.alloc(np));
  PYSDR_HIP_CHECK(b.d_lut.alloc((size_t)kPassLut));
  PYSDR_HIP_CHECK(b.d_jobs.alloc((size_t)kPassJobsMax * kPassJobWords));
  PYSDR_HIP_CHECK(b.d_rows.alloc((size_t)kPassJobsMax * 2));
  PYSDR_HIP_CHECK(b.d_out.alloc((size_t)kPassMax * kPassRowJobs * kPassOutWords));
  PYSDR_HIP_CHECK(b.d_counts.alloc((size_t)kPassRowsMax));
  PYSDR_HIP_CHECK(b.d_events.alloc((size_t)kPassRowsMax * kPassEventCap * kFtEventWords));
  b.h_jobs.reserve(kPassJobsMax);
  b.h_rows.reserve((size_t)kPassJobsMax * 2);
  b.plan = p; b.reach_t = cfg->reach_t; b.trials = cfg->trials;
  b.kept = true;
  PYSDR_HIP_CHECK(hipMemcpyAsync(b.d_pulse.get(), b.h_pulse.data(), np * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipMemcpyAsync(b.d_lut.get(), b.h_lut.data(), 2 * (size_t)kPassLut * sizeof(float), hipMemcpyHostToDevice, st));
  rc = pass_clear(&b, w->nk, w->plan.nb, st);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  return PYSDR_OK;
}

// Behind the sync kernel of a process call that delivered nf outputs from m0 on and completed ns steps from t_first on.
template <class W>
int pass_step(W* w, unsigned long long m0, int nf, int ns, long long t_first, hipStream_t st) {
  PassBufs& b = w->pass;
  if (!b.kept || nf < 1) return PYSDR_OK;
  PassKeepArgs a{};
  a.y = w->feed_rows(); a.ypitch = w->plan.ypitch; a.n_out = nf; a.nk = w->nk; a.nb = w->plan.nb; a.m0 = (long long)m0;
  a.ring = w->d_ring.get(); a.tr = w->plan.tr; a.ns = ns; a.t_first = t_first;
  a.yk = b.d_yk.get(); a.ty = b.plan.ty; a.ring2 = b.d_ring2.get(); a.tr2 = b.plan.tr2;
  const int rc = launch_pass_keep(a, st);
  if (rc) return rc;
  b.n_abs = m0 + (unsigned long long)nf;
  return PYSDR_OK;
}

// Frames (F[i], t0[i]) with their 91 bits as report_frames takes them and trials [n][trials][2] = (dn, fw); out [n][2][4].
template <class W>
int pass_subtract(W* w, const char* who, const int32_t* F, const long long* t0, const uint8_t* bits, const int32_t* trials, int n, int32_t* out) {
  using Mode = typename W::Mode;
  if (!w) return no_skimmer(who);
  if (n < 0 || n > kPassMax || (n > 0 && (!F || !t0 || !bits || !trials || !out))) {
    set_last_error("%s: n %d outside [0, %d] / NULL F, t0, bits, trials or out", who, n, kPassMax);
    return PYSDR_ERR_ARG;
  }
  std::lock_guard<std::mutex> lk(w->mu);
  PassBufs& b = w->pass;
  if (!b.kept) return pass_not_kept(who);
  const long long done = (long long)w->t_done;
  const int S = w->plan.S, ntr = b.trials;
  for (int i = 0; i < n; ++i) {                                        // every frame first: a refusal changes nothing
    if (F[i] < 0 || F[i] >= w->plan.nfine) {
      set_last_error("%s: frame %d: F %d outside [0, %d)", who, i, (int)F[i], w->plan.nfine);
      return PYSDR_ERR_ARG;
    }
    for (int k = 0; k < ntr; ++k)
      if (!pass_dn_ok(trials[2 * ((size_t)i * ntr + k)], S)) {
        set_last_error("%s: frame %d, trial %d: dn %d is not inside (-%d, %d)", who, i, k, (int)trials[2 * ((size_t)i * ntr + k)], S / 4, S / 4);
        return PYSDR_ERR_ARG;
      }
  }
  for (int i = 0; i < n; ++i)
    if (!pass_frame_ok<Mode>(t0[i], done, b.plan.tr2)) {
      set_last_error("%s: frame %d (F %d, t0 %lld): the steps %lld to %lld are not all complete and held (%lld steps done, %d held)", who, i,
                     (int)F[i], t0[i], t0[i] - kPassMargin, t0[i] + kFtLag<Mode> + kPassMargin, done, b.plan.tr2);
      return PYSDR_ERR_STATE;
    }
  if (n == 0) return PYSDR_OK;
  ChanInfo ci;
  int rc = chan_info(w->ch, &ci);
  if (rc != PYSDR_OK) return rc;
  const bool circular = ci.M == w->nk;
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));                          // the host arrays may still feed an earlier copy
  std::vector<PassJob> all;
  all.reserve((size_t)n * kPassRowJobs);
  for (int i = 0; i < n; ++i) {
    const PassRows pr = pass_rows<Mode>(F[i], S, w->nk, circular);
    uint32_t m[3];
    report_words(bits + (size_t)i * kReportBitsBytes, m);
    const long long n0 = (long long)(S / 4) * t0[i];
    for (int r = 0; r < pr.n; ++r) {
      PassJob j{};
      j.row = pr.row[r]; j.out_at = kPassRowJobs * i + r; j.w = pass_word(pr.q[r], S); j.m0 = m[0]; j.m1 = m[1]; j.m2 = m[2];
      j.n0_lo = (int32_t)(uint32_t)((unsigned long long)n0 & 0xFFFFFFFFULL); j.n0_hi = (int32_t)(uint32_t)((unsigned long long)n0 >> 32);
      j.t0_lo = (int32_t)(uint32_t)((unsigned long long)t0[i] & 0xFFFFFFFFULL); j.t0_hi = (int32_t)(uint32_t)((unsigned long long)t0[i] >> 32);
      j.ntr = ntr;
      for (int k = 0; k < 2 * ntr; ++k) j.trial[k] = trials[2 * (size_t)i * ntr + k];
      all.push_back(j);
    }
  }
  // the jobs of a row together, in the order given; the rows in the order of their first job
  b.h_jobs.clear();
  b.h_rows.clear();
  std::vector<char> taken(all.size(), 0);
  for (size_t i = 0; i < all.size(); ++i) {
    if (taken[i]) continue;
    const int first = (int)b.h_jobs.size();
    for (size_t k = i; k < all.size(); ++k)
      if (!taken[k] && all[k].row == all[i].row) { b.h_jobs.push_back(all[k]); taken[k] = 1; }
    b.h_rows.push_back(first);
    b.h_rows.push_back((int)b.h_jobs.size() - first);
  }
  const int njobs = (int)b.h_jobs.size(), nrows = (int)b.h_rows.size() / 2;
  PYSDR_HIP_CHECK(hipMemcpyAsync(b.d_jobs.get(), b.h_jobs.data(), (size_t)njobs * sizeof(PassJob), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipMemcpyAsync(b.d_rows.get(), b.h_rows.data(), (size_t)nrows * 2 * sizeof(int32_t), hipMemcpyHostToDevice, st));
  PYSDR_HIP_CHECK(hipMemsetAsync(b.d_out.get(), 0, (size_t)n * kPassRowJobs * kPassOutWords * sizeof(int32_t), st));
  PassSubArgs a{};
  a.yk = b.d_yk.get(); a.ty = b.plan.ty; a.nrows = nrows;
  a.n_hi = (long long)b.n_abs; a.n_lo = a.n_hi > b.plan.ty ? a.n_hi - b.plan.ty : 0;
  a.jobs = reinterpret_cast<const PassJob*>(b.d_jobs.get()); a.rows = b.d_rows.get(); a.pulse = b.d_pulse.get(); a.lut = b.d_lut.get();
  a.out = b.d_out.get();
  PassSpecArgs s{};
  s.yk = a.yk; s.ty = a.ty; s.njobs = njobs; s.jobs = a.jobs; s.tw = w->d_tw.get(); s.pmax = w->cfg.pmax; s.ring2 = b.d_ring2.get();
  s.tr2 = b.plan.tr2; s.t_done = done;
  rc = launch_pass_subtract(Mode::kLdpcSource, S, a, s, st);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipMemcpyAsync(out, a.out, (size_t)n * kPassRowJobs * kPassOutWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  return PYSDR_OK;
}

// The fine rows F_lo .. F_hi of ring2 scored at the start steps t_lo - 4 .. t_hi + 4 and judged at t_lo .. t_hi:
// counts [nF], events [nF][52][2], the step of an event counted from t_lo.
template <class W>
int pass_rescan(W* w, const char* who, int F_lo, int F_hi, long long t_lo, long long t_hi, const FtCfg* cfg, int32_t* counts, int32_t* events) {
  using Mode = typename W::Mode;
  if (!w) return no_skimmer(who);
  if (!cfg || !ft_cfg_ok<Mode>(*cfg) || !counts || !events) {
    set_last_error("%s: NULL counts or events, or a cfg outside the skimmer's rules", who);
    return PYSDR_ERR_ARG;
  }
  std::lock_guard<std::mutex> lk(w->mu);
  if (F_lo < 0 || F_hi < F_lo || F_hi >= w->plan.nfine || F_hi - F_lo + 1 > kPassRowsMax || !pass_window_arg_ok<Mode>(t_lo, t_hi)) {
    set_last_error("%s: fine rows %d to %d outside [0, %d) or more than %d, or steps %lld to %lld: negative, reversed, or a window of more "
                   "than %d start steps with the %d to either side", who, F_lo, F_hi, w->plan.nfine, kPassRowsMax, t_lo, t_hi, kPassWindowMax,
                   kFtReach);
    return PYSDR_ERR_ARG;
  }
  PassBufs& b = w->pass;
  if (!b.kept) return pass_not_kept(who);
  const long long done = (long long)w->t_done;
  if (!pass_window_ok<Mode>(t_lo, t_hi, done, b.plan.tr2)) {
    set_last_error("%s: the frames that start at steps %lld to %lld are not all complete and held (%lld steps done, %d held)", who,
                   t_lo - kFtReach, t_hi + kFtReach, done, b.plan.tr2);
    return PYSDR_ERR_STATE;
  }
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  PassScanArgs a{};
  a.ring2 = b.d_ring2.get(); a.tr2 = b.plan.tr2; a.nb = w->plan.nb; a.nsub = w->plan.nsub; a.F_lo = F_lo; a.nF = F_hi - F_lo + 1;
  a.t_lo = t_lo; a.nt = (int)(t_hi - t_lo + 1); a.cfg = *cfg; a.counts = b.d_counts.get(); a.events = b.d_events.get();
  const int rc = launch_pass_rescan(Mode::kLdpcSource, a, st);
  if (rc) return rc;
  PYSDR_HIP_CHECK(hipMemcpyAsync(counts, a.counts, (size_t)a.nF * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  PYSDR_HIP_CHECK(hipMemcpyAsync(events, a.events, (size_t)a.nF * kPassEventCap * kFtEventWords * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  return PYSDR_OK;
}

// yk [nk][ty][2] and ring2 [nk][tr2][nb] (either may be NULL), kept[0] = row samples since create / reset, kept[1] = ty,
// kept[2] = tr2
template <class W>
int pass_state(W* w, const char* who, float* yk, float* ring2, long long* kept) {
  if (!w) return no_skimmer(who);
  std::lock_guard<std::mutex> lk(w->mu);
  PassBufs& b = w->pass;
  if (!b.kept) return pass_not_kept(who);
  PYSDR_HIP_CHECK(hipSetDevice(w->device));
  hipStream_t st = w->stream;
  if (yk) PYSDR_HIP_CHECK(hipMemcpyAsync(yk, b.d_yk.get(), (size_t)w->nk * (size_t)b.plan.ty * sizeof(FtC), hipMemcpyDeviceToHost, st));
  if (ring2)
    PYSDR_HIP_CHECK(hipMemcpyAsync(ring2, b.d_ring2.get(), (size_t)w->nk * (size_t)b.plan.tr2 * (size_t)w->plan.nb * sizeof(float),
                                   hipMemcpyDeviceToHost, st));
  PYSDR_HIP_CHECK(hipStreamSynchronize(st));
  if (kept) { kept[0] = (long long)b.n_abs; kept[1] = b.plan.ty; kept[2] = b.plan.tr2; }
  return PYSDR_OK;
}

// The decoder on the residue: pysdr_*_decode_osd's arguments and rules on ring2; osd may be NULL (min-sum alone).
template <class W>
int pass_decode(W* w, const char* who, const int32_t* F, const long long* t0, int n, const pysdr_ldpc_cfg* cfg, int32_t* status, uint8_t* bits,
                float* post, const pysdr_osd_cfg* osd, int32_t* detail) {
  if (!w) return no_skimmer(who);
  if (!osd && detail) {
    set_last_error("%s: detail is the second stage's: it needs an osd cfg", who);
    return PYSDR_ERR_ARG;
  }
  return ldpc_decode_ring(w, who, [](W* s) { return s->pass.kept ? RingRef{s->pass.d_ring2.get(), s->pass.plan.tr2} : RingRef{nullptr, 0}; },
                          F, t0, n, cfg, status, bits, post, osd ? OsdCall{true, osd, detail} : kNoOsd);
}

}  // namespace pysdr
