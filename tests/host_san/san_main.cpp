// Driver of the sanitizer build of the HOST half of libpysdr_hip.so (tests/host_san): the C ABI of
// include/pysdr_hip.h exercised end to end over the fake HIP runtime and the checking launch layer
// (stub_kernels.cpp) -- every BASELINE rate, ragged call lengths, every setter between calls, the
// lazily allocated buffers (AM-Synch, WFM), the spectrum object on both its paths, the ingest ring's
// slot state machine with its misuse errors.  `san_main race` runs pysdr_process on one thread against
// the setters on another (the reference's RX thread vs Qt thread) for ThreadSanitizer.  The mix + decimate
// planner (pysdr_amd/csrc/mixdec_plan.h) is also swept directly over every shape, tile override and thread count, and the
// plans of the two serial loops (pysdr_amd/csrc/host_plan.h) over rates, call lengths and tunings.  `san_main allocfail`
// runs a short scenario over every object kind with the n-th allocation / event / stream creation failing, n = 1, 2, ...
// The four stream objects of api_objects.hip (waterfall, RTTY decoder bank, channelizer, channel bank) have a scenario each,
// and so have the objects that borrow a channelizer beside the bank -- CW skimmer (api_cw.hip), PSK31 skimmer (api_psk.hip) --
// the fine channelizer (api_fine.hip) and the bank's complex-tap modes; all part of the default run.  `san_main objects`
// runs these alone (their queue trace on its own).
//   build + run: tests/host_san/run.sh   (tests/test_host_sanitizers.py does that)
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "../../include/pysdr_hip.h"
#include "host_plan.h"
#include "mixdec_plan.h"

#define OK(expr)                                                                                    \
  do {                                                                                              \
    const int rc_ = (expr);                                                                         \
    if (rc_ != 0) { std::fprintf(stderr, "%s:%d %s -> %d (%s)\n", __FILE__, __LINE__, #expr, rc_, pysdr_last_error()); std::exit(1); } \
  } while (0)
#define FAILS(expr)                                                                                 \
  do {                                                                                              \
    if ((expr) == 0) { std::fprintf(stderr, "%s:%d %s unexpectedly succeeded\n", __FILE__, __LINE__, #expr); std::exit(1); } \
    if (fake_hip::tracing()) fake_hip::Line("refused").t("error", pysdr_last_error());   /* the queue trace holds the message texts too */ \
  } while (0)

struct Rate { double fs; int up, down, in_chunk; };
static const Rate kRates[] = {{8e6, 3, 500, 170666}, {2.048e6, 3, 128, 43690}, {256e3, 3, 16, 5461}, {10e6, 3, 625, 213333},
                              {1.024e6, 3, 64, 21845}, {6e6, 1, 125, 128000}};

static std::vector<double> taps(int n, double scale = 1.0) {
  std::vector<double> h(n);
  for (int i = 0; i < n; ++i) h[i] = scale * std::sin(0.01 * (i + 1)) / n;
  return h;
}

static int g_overlap = 0;      // passes of main(): 0 single-stream, 2 every call in two overlapped halves, 1 the calls with a serial loop (pysdr_set_overlap)

static pysdr_ctx* make_ctx(const Rate& r, int max_chunks, int ntaps_dec, int ntaps_af) {
  pysdr_cfg cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  cfg.srate = r.fs; cfg.up = r.up; cfg.down = r.down; cfg.in_chunk = r.in_chunk;
  cfg.max_chunks = max_chunks; cfg.ntaps_dec = ntaps_dec; cfg.ntaps_af = ntaps_af;
  pysdr_ctx* c = nullptr;
  OK(pysdr_create(&cfg, &c));
  if (g_overlap) {
    FAILS(pysdr_set_overlap(c, 3));
    OK(pysdr_set_overlap(c, g_overlap));
    if (!pysdr_get_overlap(c)) { std::fprintf(stderr, "overlap did not switch on\n"); std::exit(1); }     // (PYSDR_OVERLAP may overrule WHICH form)
  }
  return c;
}

static void run_calls(pysdr_ctx* c, const Rate& r, int nrx, int max_chunks, const std::vector<size_t>& lens) {
  const size_t cap_in = (size_t)max_chunks * r.in_chunk;
  std::vector<float> x(2 * cap_in, 0.25f);
  const int cap_out = (int)(cap_in * r.up / r.down) + 8;
  std::vector<std::vector<float>> am(nrx, std::vector<float>(2 * cap_out)), iq(nrx, std::vector<float>(2 * cap_out));
  std::vector<pysdr_out> outs(nrx);
  for (size_t n : lens) {
    for (int i = 0; i < nrx; ++i) { outs[i].am = am[i].data(); outs[i].iq = iq[i].data(); outs[i].cap = cap_out; }
    if (n <= (size_t)r.in_chunk * max_chunks) OK(pysdr_process(c, x.data(), n, outs.data()));
  }
  // a batch of whole chunks + per-chunk counts
  OK(pysdr_process_batch(c, x.data(), max_chunks, r.in_chunk, 0));
  std::vector<int> cn(max_chunks);
  std::vector<float> pk(max_chunks);
  int n_out = 0, cx = 0;
  for (int i = 0; i < nrx; ++i) {
    OK(pysdr_fetch(c, i, am[i].data(), iq[i].data(), cap_out, &n_out, &cx, cn.data(), pk.data()));
    int s = 0;
    for (int k = 0; k < max_chunks; ++k) s += cn[k];
    if (s != n_out) { std::fprintf(stderr, "chunk counts %d != n_out %d\n", s, n_out); std::exit(1); }
    FAILS(pysdr_fetch(c, i, am[i].data(), nullptr, n_out - 1, nullptr, nullptr, nullptr, nullptr));   // cap too small
  }
  FAILS(pysdr_process_batch(c, x.data(), max_chunks + 1, r.in_chunk, 0));                             // over capacity
}

static void narrowband(const Rate& r, int ntaps_dec) {
  const int max_chunks = 3, ntaps_af = 255, nrx = 4;
  pysdr_ctx* c = make_ctx(r, max_chunks, ntaps_dec, ntaps_af);
  const auto h = taps(ntaps_dec), af = taps(2 * ntaps_af);
  const int modes[nrx] = {PYSDR_USB, PYSDR_CW, PYSDR_NFM, PYSDR_AM};
  for (int i = 0; i < nrx; ++i) {
    int irx = -1;
    OK(pysdr_rx_add(c, modes[i], -1000.0 * (i + 1), h.data(), af.data(), i == 1 ? 700.0 : 0.0, &irx));
    if (irx != i) std::exit(1);
  }
  OK(pysdr_set_profile(c, 1));
  const size_t L = (size_t)r.in_chunk;
  run_calls(c, r, nrx, max_chunks, {L, 1, 2, 3, 17, L - 7, L + 11, 3 * L, 333, 2 * L + 1, L});
  // controls between calls (receiver.py:112-131,648-649; gui.py:1713,1938)
  double fa = 0;
  OK(pysdr_set_lo(c, 2, -4567.0, &fa));
  const auto h2 = taps(ntaps_dec, 0.5);
  OK(pysdr_set_dec_taps(c, 0, h2.data(), ntaps_dec));
  FAILS(pysdr_set_dec_taps(c, 0, h2.data(), ntaps_dec - 1));
  OK(pysdr_set_mode(c, 3, PYSDR_AM_SYNCH, af.data(), ntaps_af, 0.0));          // lazily allocates the PLL buffer
  OK(pysdr_set_mode(c, 0, PYSDR_IQ, af.data(), ntaps_af, 0.0));                // complex audio
  FAILS(pysdr_set_mode(c, 0, PYSDR_IQ, af.data(), ntaps_af + 1, 0.0));
  OK(pysdr_reset(c, 1, 3));
  OK(pysdr_set_agc(c, 1, 0, 0.4f));
  OK(pysdr_set_squelch(c, 2, 0.05f));
  {
    // the ratio squelch: its two FIRs belong to the context, the block sums are allocated when it is first armed
    std::vector<float> lp(63, 1.0f / 63), hp(63, 0.f);
    hp[31] = 1.f;
    FAILS(pysdr_set_squelch_ratio(c, 2, 2.0f, lp.data(), hp.data(), 65));
    FAILS(pysdr_set_squelch_ratio(c, 2, 2.0f, nullptr, hp.data(), 63));
    OK(pysdr_set_squelch_ratio(c, 2, 2.0f, lp.data(), hp.data(), 63));
    OK(pysdr_set_squelch_ratio(c, 1, 0.0f, nullptr, nullptr, 0));                // disarming needs no taps
  }
  run_calls(c, r, nrx, max_chunks, {L, 5, L});
  {
    float sq1 = 0, sq2 = 0;
    int gate = 0;
    OK(pysdr_squelch_ratio_get(c, 2, &sq1, &sq2, &gate));
    FAILS(pysdr_squelch_ratio_get(c, 9, &sq1, &sq2, &gate));
  }
  pysdr_agc_state st;
  OK(pysdr_agc_get(c, 3, &st));
  int seg = 0, pat = 0, open = 0;
  float lvl = 0;
  OK(pysdr_pll_stats(c, 3, &seg, &pat));
  OK(pysdr_squelch_get(c, 2, &lvl, &open));
  OK(pysdr_set_pll_segments(c, 1));
  run_calls(c, r, nrx, max_chunks, {L});
  float ms = 0;
  for (int which = 0; which < 4; ++which) OK(pysdr_get_elapsed_ms(c, which, 0, &ms));
  FAILS(pysdr_get_elapsed_ms(c, 4, 0, &ms));
  int32_t tune[8];
  OK(pysdr_get_tuning(c, tune));
  FAILS(pysdr_set_lo(c, 9, 0.0, &fa));
  FAILS(pysdr_agc_get(c, -1, &st));
  // ingest ring: slot state machine
  pysdr_ingest* g = nullptr;
  OK(pysdr_ingest_create_batched(c, 3, 2, &g));
  // a ring runs its context single-stream: creating one switches the overlap off, and it stays off while the ring lives
  if (pysdr_get_overlap(c)) { std::fprintf(stderr, "ingest ring on an overlapped context\n"); std::exit(1); }
  FAILS(pysdr_set_overlap(c, 1));
  OK(pysdr_set_overlap(c, 0));
  { pysdr_ingest* bad = nullptr; FAILS(pysdr_ingest_create_batched(c, 3, max_chunks + 1, &bad)); }
  float* buf = nullptr;
  size_t cap = 0;
  std::vector<pysdr_out> outs(nrx);
  for (int round = 0; round < 4; ++round) {
    const int slot = round % 3;
    OK(pysdr_ingest_buffer(g, slot, &buf, &cap));
    const size_t n = (round == 2) ? L - 5 : 2 * L;                               // whole chunks, and a short single chunk
    for (size_t i = 0; i < 2 * n; ++i) buf[i] = 0.1f;
    OK(pysdr_ingest_submit(g, slot, n));
    FAILS(pysdr_ingest_submit(g, slot, n));                                      // already in flight
    int nch = 0, cn[4];
    float pk[4];
    OK(pysdr_ingest_chunks(g, slot, 4, &nch, cn, pk));
    OK(pysdr_ingest_collect(g, slot, outs.data()));
    FAILS(pysdr_ingest_collect(g, slot, outs.data()));                           // not submitted any more
    for (int i = 0; i < nrx; ++i) {                                              // the result buffers hold n_out samples
      volatile float s = 0;
      for (int k = 0; k < outs[i].n_out * (outs[i].am_is_complex ? 2 : 1); ++k) s = s + outs[i].am[k];
      for (int k = 0; k < 2 * outs[i].n_out; ++k) s = s + outs[i].iq[k];
    }
  }
  FAILS(pysdr_ingest_submit(g, 0, cap + 1));
  FAILS(pysdr_ingest_submit(g, 7, 1));
  pysdr_ingest_destroy(g);
  OK(pysdr_set_overlap(c, g_overlap));                                           // the ring is gone: allowed again
  run_calls(c, r, nrx, max_chunks, {L, 3});                                      // ... and the stream goes on from whichever buffer of the pair is current
  OK(pysdr_set_overlap(c, 0));
  run_calls(c, r, nrx, max_chunks, {L});
  pysdr_destroy(c);
}

// One sub-receiver with the reference's default 1001-tap prototype at the am.py rate: the matrix-core form of the
// mix + decimate kernel (mixdec_mfma.hip).  Ragged and odd call lengths flip the parity of its LDS image.
namespace pysdr { extern int g_mfma_launches; }
static void single_rx_long_prototype(const Rate& r) {
  const int max_chunks = 3, ntaps_dec = 1001, ntaps_af = 255;
  pysdr_ctx* c = make_ctx(r, max_chunks, ntaps_dec, ntaps_af);
  const auto h = taps(ntaps_dec), af = taps(2 * ntaps_af);
  int irx = -1;
  OK(pysdr_rx_add(c, PYSDR_AM, 100e3, h.data(), af.data(), 0.0, &irx));
  const size_t L = (size_t)r.in_chunk;
  const int before = pysdr::g_mfma_launches;
  run_calls(c, r, 1, max_chunks, {L, 1, 2, 3, 17, L - 7, L + 11, 3 * L, 333, 2 * L + 1, L, 8191, 8193, 1, 1, 255, 256, 257});
  const char* tun = getenv("PYSDR_TUNING");
  const char* off = getenv("PYSDR_MIXDEC_MFMA");
  const bool expect = !(tun && atoi(tun) > 0 && off && atoi(off) == 0);
  if ((pysdr::g_mfma_launches > before) != expect) { std::fprintf(stderr, "matrix-core path: launches %d, expected %d\n", pysdr::g_mfma_launches - before, (int)expect); std::exit(1); }
  // Mode changes across the forms of a call: AM-Synch batches (overlapped when the pass allows it: the pairs' current buffer
  // alternates and is left on the SECOND one by an odd number of calls), then modes whose buffers have not existed yet
  // (their second buffer must come into being as the current one), and back.
  std::vector<float> x(2 * (size_t)max_chunks * r.in_chunk, 0.2f);
  for (int round = 0; round < 2; ++round) {
    OK(pysdr_set_mode(c, 0, PYSDR_AM_SYNCH, af.data(), ntaps_af, 0.0));
    for (int k = 0; k < 3; ++k) OK(pysdr_process_batch(c, x.data(), max_chunks, r.in_chunk, 0));
    OK(pysdr_set_mode(c, 0, PYSDR_NFM, af.data(), ntaps_af, 0.0));
    OK(pysdr_process_batch(c, x.data(), 2, r.in_chunk, 0));
    if (r.fs == 2.048e6) {                                  // a rate pysdr_wfm_params accepts
      int d1 = 0, up2 = 0, down2 = 0;
      if (pysdr_wfm_params(r.fs, 48000.0, &d1, &up2, &down2) == 0) {
        const auto video = taps(ntaps_dec), res = taps(64 * up2);
        OK(pysdr_set_wfm_taps(c, 0, video.data(), ntaps_dec, res.data(), 64 * up2));
        OK(pysdr_set_mode(c, 0, PYSDR_WFM2, af.data(), ntaps_af, 0.0));
        for (int k = 0; k < 2 + round; ++k) OK(pysdr_process_batch(c, x.data(), max_chunks, r.in_chunk, 0));
        OK(pysdr_set_mode(c, 0, PYSDR_WFM, af.data(), ntaps_af, 0.0));
        OK(pysdr_process_batch(c, x.data(), 1, r.in_chunk, 0));
      }
    }
    run_calls(c, r, 1, max_chunks, {L, 5});
  }
  pysdr_destroy(c);
}

static void broadcast_fm() {
  const Rate r = kRates[3];
  const int max_chunks = 4, ntaps = 255;
  pysdr_ctx* c = make_ctx(r, max_chunks, ntaps, ntaps);
  const auto h = taps(ntaps), af = taps(2 * ntaps);
  int irx = -1;
  OK(pysdr_rx_add(c, PYSDR_WFM2, -300e3, h.data(), af.data(), 0.0, &irx));
  std::vector<float> x(2 * (size_t)max_chunks * r.in_chunk, 0.2f);
  FAILS(pysdr_process_batch(c, x.data(), 1, r.in_chunk, 0));                     // WFM taps never set
  int d1 = 0, up2 = 0, down2 = 0;
  OK(pysdr_wfm_params(r.fs, 48000.0, &d1, &up2, &down2));
  const auto video = taps(ntaps), res = taps(64 * up2);
  OK(pysdr_set_wfm_taps(c, 0, video.data(), ntaps, res.data(), 64 * up2));
  run_calls(c, r, 1, max_chunks, {(size_t)r.in_chunk, 7, (size_t)r.in_chunk - 3, 2 * (size_t)r.in_chunk + 1});
  OK(pysdr_set_mode(c, 0, PYSDR_WFM, af.data(), ntaps, 0.0));
  run_calls(c, r, 1, max_chunks, {(size_t)r.in_chunk});
  int seg = 0, pat = 0;
  OK(pysdr_pll_stats(c, 0, &seg, &pat));
  pysdr_destroy(c);
}

// A narrow-band and a broadcast-FM sub-receiver in one context: the call is refused (one context runs one pipeline,
// receiver.py:718-719) and the context is torn down with whatever the refused call left behind.
static void mixed_modes_are_refused() {
  const Rate r = kRates[1];
  const int ntaps = 255;
  pysdr_ctx* c = make_ctx(r, 1, ntaps, ntaps);
  const auto h = taps(ntaps), af = taps(2 * ntaps);
  int irx = -1;
  OK(pysdr_rx_add(c, PYSDR_AM, 100e3, h.data(), af.data(), 0.0, &irx));
  OK(pysdr_rx_add(c, PYSDR_AM, 200e3, h.data(), af.data(), 0.0, &irx));
  int d1 = 0, up2 = 0, down2 = 0;
  OK(pysdr_wfm_params(r.fs, 48000.0, &d1, &up2, &down2));
  const auto res = taps(64 * up2);
  OK(pysdr_set_wfm_taps(c, 1, h.data(), ntaps, res.data(), 64 * up2));
  OK(pysdr_set_mode(c, 1, PYSDR_WFM, af.data(), ntaps, 0.0));
  std::vector<float> x(2 * (size_t)r.in_chunk, 0.f);
  std::vector<float> am(4 * 2048), iq(4 * 2048);
  pysdr_out outs[2];
  for (int i = 0; i < 2; ++i) { outs[i].am = am.data() + 4096 * i; outs[i].iq = iq.data() + 4096 * i; outs[i].cap = 2048; }
  FAILS(pysdr_process(c, x.data(), r.in_chunk, outs));
  FAILS(pysdr_process(c, x.data(), r.in_chunk, outs));
  pysdr_destroy(c);
}

static void spectrum() {
  std::vector<float> win(32768, 1.0f);
  pysdr_spectrum* sp = nullptr;
  OK(pysdr_spectrum_create(0, 32768, 65536, 1000, win.data(), &sp));            // the fused 64k path
  void *d_x = nullptr, *d_o = nullptr;
  const int nframes = 1000;
  OK(pysdr_dev_alloc(0, (size_t)nframes * 32768 * 8, &d_x));
  OK(pysdr_dev_alloc(0, (size_t)nframes * 65536 * 4, &d_o));
  OK(pysdr_spectrum_batch(sp, d_x, nframes, 32768, d_o));                        // 448 + 448 + 104 frames
  OK(pysdr_spectrum_batch(sp, d_x, 37, 800000 < (size_t)nframes * 32768 / 37 ? 800000 : 32768, d_o));
  FAILS(pysdr_spectrum_batch(sp, d_x, nframes + 1, 32768, d_o));
  std::vector<float> one(2 * 32768, 0.1f), psd(65536);
  int n_out = 0;
  OK(pysdr_spectrum_frame(sp, one.data(), 1, 1, psd.data(), &n_out));
  OK(pysdr_spectrum_sync(sp));
  float ms = 0;
  OK(pysdr_spectrum_elapsed_ms(sp, &ms));
  int32_t t4[4];
  OK(pysdr_spectrum_get_tuning(sp, t4));
  pysdr_spectrum_destroy(sp);
  // the rocFFT path at the sizes the unchanged GUI passes (Plotting.py:370-376) and the AF PSD (real input)
  for (int chunk : {32818, 4096}) {
    std::vector<float> w(chunk, 1.0f), xin(2 * (size_t)chunk, 0.1f), out(2 * (size_t)chunk);
    OK(pysdr_spectrum_create(0, chunk, 2 * chunk, 4, w.data(), &sp));
    OK(pysdr_spectrum_frame(sp, xin.data(), 1, 1, out.data(), &n_out));
    if (n_out != 2 * chunk) std::exit(1);
    OK(pysdr_spectrum_frame(sp, xin.data(), 0, 1, out.data(), &n_out));          // real input: first NFFT/2 bins
    if (n_out != chunk) std::exit(1);
    pysdr_spectrum_destroy(sp);
  }
  OK(pysdr_dev_free(0, d_x));
  OK(pysdr_dev_free(0, d_o));
  // stand-alone helpers
  std::vector<float> a(2 * 1001, 0.5f), b(2 * 1001);
  uint32_t ph = 0;
  OK(pysdr_quad_mixer(0, a.data(), b.data(), 1001, 123u, 456789u, &ph));
  std::vector<float> xx(255 - 1 + 500, 0.1f), hh(255, 0.01f), yy(500);
  OK(pysdr_fir_real(0, xx.data(), hh.data(), 255, yy.data(), 500));
}

// plan_mixdec over 1 - 8 sub-receivers, the decimator shapes of the library, every tile override and thread count
namespace pysdr { void check_mixdec_plan(const MixDecArgs& a, MdKey key, int threads); }
static void planner_sweep() {
  int d1 = 0, up2 = 0, down2 = 0;
  OK(pysdr_wfm_params(10e6, 48000.0, &d1, &up2, &down2));
  struct Shape { int up, down, ntaps; };
  const Shape shapes[] = {{3, 500, 255}, {3, 128, 255}, {3, 500, 1001}, {3, 250, 1001}, {6, 125, 1001}, {3, 128, 1001},
                          {1, d1, 255}, {up2, down2, 64 * up2}};      // broadcast FM: the IF front end, the fs1 -> FS_OUT resampler
  int nplans = 0;
  for (const Shape& sh : shapes)
    for (int nrx = 1; nrx <= PYSDR_MAX_RX; ++nrx)
      for (int tile_bytes : {0, 4096, 12288, 32768, 150 * 1024})
        for (int threads : {1024, 512, 64})
          for (int n_out : {0, 12345}) {
            pysdr::MixDecArgs a;
            std::memset(&a, 0, sizeof(a));
            a.nrx = nrx; a.up = sh.up; a.down = sh.down; a.n_out = n_out;
            a.kpad = ((sh.ntaps + sh.up - 1) / sh.up + 15) / 16 * 16;
            pysdr::MdKey key;
            if (!pysdr::plan_mixdec(a, tile_bytes, threads, 1, 0, key)) {
              std::fprintf(stderr, "planner: no plan for %d RX, %d/%d, %d taps, tile %d, %d threads\n", nrx, sh.up, sh.down, sh.ntaps,
                           tile_bytes, threads);
              std::exit(1);
            }
            pysdr::check_mixdec_plan(a, key, threads);
            ++nplans;
          }
  std::printf("planner sweep: %d plans\n", nplans);
}

// plan_am_pll / plan_wfm_pll: what the segment kernels rely on, over the harness's rates, ragged call lengths up to
// max_chunks * in_chunk, pysdr_set_pll_segments 0 / 1 / 7, the default tuning and the two tuning strings of run.sh
static void check_pll_plan(const pysdr::PllPlan& p, int n, int pll_kmax, bool carrier, const char* what) {
  const bool ok = p.K >= 1 && p.K <= pysdr::kPllSegMax && (long long)p.K * p.T >= n && p.T % 64 == 0 && p.W % 64 == 0 && p.Wfast % 64 == 0 &&
                  p.Wexact % 64 == 0 && p.Wc_hi % 64 == 0 && p.Wc_mid % 64 == 0 && p.Wseed % 64 == 0 && p.Wexact <= p.W &&
                  (!carrier || p.Wseed <= std::max(0, p.W - 64)) && (pll_kmax != 1 || p.K == 1);
  if (!ok) {
    std::fprintf(stderr, "%s plan for n %d, kmax %d: K %d T %d W %d Wfast %d Wexact %d Wc %d/%d Wseed %d\n", what, n, pll_kmax, p.K, p.T, p.W,
                 p.Wfast, p.Wexact, p.Wc_hi, p.Wc_mid, p.Wseed);
    std::exit(1);
  }
}
struct ScopedEnv {             // a variable set for the lifetime of the object, then put back
  std::string name, old; bool had;
  ScopedEnv(const char* n, const char* v) : name(n) { const char* o = getenv(n); had = o != nullptr; if (o) old = o; setenv(n, v, 1); }
  ~ScopedEnv() { if (had) setenv(name.c_str(), old.c_str(), 1); else unsetenv(name.c_str()); }
};
static void pll_plan_sweep() {
  std::vector<pysdr::Tuning> tunings{pysdr::Tuning()};
  {
    ScopedEnv on("PYSDR_TUNING", "1"), wfm("PYSDR_WFM_PLL", "20,13,4,3,1536,2048,5,4,4,4"), am("PYSDR_AM_PLL", "14,4,4,1024,256");
    tunings.push_back(pysdr::Tuning::from_env());
    if (tunings[1].am_taus != 14.0 || tunings[1].am_tmin != 256 || tunings[1].wfm_tail_cap != 4) { std::fprintf(stderr, "tuning strings not parsed\n"); std::exit(1); }
  }
  std::vector<uint32_t> seg(1);          // (the plans only carry the pointer)
  int nplans = 0;
  for (const pysdr::Tuning& t : tunings)
    for (const Rate& r : kRates)
      for (int max_chunks : {1, 3, 64, 2048}) {
        const long long L = r.in_chunk, cap = L * max_chunks;
        int d1 = 1, up2 = 0, down2 = 0;
        const double fs_out = std::floor(r.fs * r.up / r.down);
        OK(pysdr_wfm_params(r.fs, fs_out, &d1, &up2, &down2));
        for (long long n : {1LL, 17LL, L - 7, L, L + 11, cap / 2 + 1, cap - 5, cap}) {
          if (n < 1 || n > cap) continue;
          for (int kmax : {0, 1, 7}) {
            const int n_out = (int)((n * r.up + r.down - 1) / r.down), n1 = (int)((n + d1 - 1) / d1);
            check_pll_plan(pysdr::plan_am_pll(t, n_out, fs_out, kmax, seg.data()), n_out, kmax, true, "carrier-loop");
            check_pll_plan(pysdr::plan_wfm_pll(t, n1, r.fs / d1, kmax, seg.data()), n1, kmax, false, "pilot-loop");
            nplans += 2;
          }
        }
      }
  std::printf("pll plan sweep: %d plans\n", nplans);
}

// ---- the four stream objects (pysdr_amd/csrc/api_objects.hip): `san_main objects` runs these alone
static int g_obj_calls = 0;
struct DevMem {              // device memory of the harness's own, freed at scope end
  void* p = nullptr;
  explicit DevMem(size_t bytes) { OK(pysdr_dev_alloc(0, bytes ? bytes : 1, &p)); std::memset(p, 0, bytes); }
  ~DevMem() { OK(pysdr_dev_free(0, p)); }
};

static void channelizer_scenario(int M, int D, int k_first, int nk, int max_taps, int max_in) {
  pysdr_chan* c = nullptr;
  OK(pysdr_chan_create(0, M, D, k_first, nk, max_taps, max_in, &c));
  const long long pitch = max_in / D + 2;
  std::vector<float> x(2 * (size_t)max_in, 0.25f), y(2 * (size_t)nk * pitch);
  DevMem dx(8 * (size_t)max_in), dy(8 * (size_t)nk * (pitch + 3));
  int nf = 0;
  FAILS(pysdr_chan_process(c, x.data(), 1, 0, y.data(), pitch, 0, &nf));                 // no taps yet
  auto h = taps(max_taps);
  FAILS(pysdr_chan_set_taps(c, h.data(), 0));
  FAILS(pysdr_chan_set_taps(c, h.data(), max_taps + 1));
  FAILS(pysdr_chan_set_taps(c, nullptr, 1));
  FAILS(pysdr_chan_set_taps(nullptr, h.data(), 1));
  OK(pysdr_chan_set_taps(c, h.data(), max_taps));
  unsigned long long s = 0;
  auto run = [&](int n, int in_dev, int out_dev) {
    const int want = (int)((s + n + D - 1) / D - (s + D - 1) / D);
    OK(pysdr_chan_process(c, in_dev ? dx.p : (void*)x.data(), n, in_dev, out_dev ? dy.p : (void*)y.data(), out_dev ? pitch + 3 : pitch, out_dev, &nf));
    if (nf != want) { std::fprintf(stderr, "channelizer: %d outputs, %d expected\n", nf, want); std::exit(1); }
    s += n; ++g_obj_calls;
  };
  for (int combo = 0; combo < 4; ++combo)                 // host / device input x host / device output: both lazy staging buffers
    for (int n : {0, 1, D - 1, D, D + 1, max_in, 7, max_in - 1}) run(n, combo & 1, combo >> 1);
  OK(pysdr_chan_set_taps(c, h.data(), M - 3));            // a shorter prototype: one tap row
  run(max_in, 0, 0); run(3, 1, 1);
  OK(pysdr_chan_reset(c)); s = 0;
  run(D + 1, 0, 1); run(max_in, 1, 0);
  OK(pysdr_chan_sync(c));
  FAILS(pysdr_chan_process(c, x.data(), max_in + 1, 0, y.data(), pitch, 0, &nf));        // over capacity
  FAILS(pysdr_chan_process(c, x.data(), -1, 0, y.data(), pitch, 0, &nf));
  FAILS(pysdr_chan_process(c, nullptr, 1, 0, y.data(), pitch, 0, &nf));
  FAILS(pysdr_chan_process(c, x.data(), 1, 0, y.data(), pitch, 0, nullptr));
  FAILS(pysdr_chan_process(nullptr, x.data(), 1, 0, y.data(), pitch, 0, &nf));
  FAILS(pysdr_chan_process(c, x.data(), 2 * D, 0, nullptr, pitch, 0, &nf));              // outputs and nowhere to put them
  FAILS(pysdr_chan_process(c, x.data(), 2 * D, 0, y.data(), 1, 0, &nf));                 // pitch too small
  run(2 * D, 0, 0);                                                                      // ... and none of them moved the stream
  FAILS(pysdr_chan_reset(nullptr));
  FAILS(pysdr_chan_sync(nullptr));
  pysdr_chan_destroy(c);
  pysdr_chan_destroy(nullptr);
}

static void channelizer_errors() {
  int32_t pl[16];
  pysdr_chan* c = nullptr;
  OK(pysdr_chan_plan(16, 4, 64, 0, 16, pl));
  FAILS(pysdr_chan_plan(16, 4, 64, 0, 16, nullptr));
  FAILS(pysdr_chan_plan(15, 5, 64, 0, 1, pl));            // M < 16
  FAILS(pysdr_chan_plan(8192, 8192, 64, 0, 1, pl));
  FAILS(pysdr_chan_plan(48, 48, 64, 0, 1, pl));           // a factor 3
  FAILS(pysdr_chan_plan(16, 3, 64, 0, 1, pl));            // D does not divide M
  FAILS(pysdr_chan_plan(16, 0, 64, 0, 1, pl));
  FAILS(pysdr_chan_plan(16, 2, 64, 0, 1, pl));            // M / D = 8
  FAILS(pysdr_chan_plan(16, 4, 0, 0, 1, pl));
  FAILS(pysdr_chan_plan(16, 4, 16 * 16 + 1, 0, 1, pl));
  FAILS(pysdr_chan_plan(16, 4, 64, -1, 1, pl));
  FAILS(pysdr_chan_plan(16, 4, 64, 16, 1, pl));
  FAILS(pysdr_chan_plan(16, 4, 64, 0, 0, pl));
  FAILS(pysdr_chan_plan(16, 4, 64, 0, 17, pl));
  FAILS(pysdr_chan_create(0, 16, 4, 0, 16, 64, 100, nullptr));
  FAILS(pysdr_chan_create(0, 16, 2, 0, 16, 64, 100, &c));
  FAILS(pysdr_chan_create(0, 16, 4, 0, 16, 64, 0, &c));
  FAILS(pysdr_chan_create(0, 16, 4, 0, 16, 64, (1 << 28) + 1, &c));
  FAILS(pysdr_chan_create(1, 16, 4, 0, 16, 64, 100, &c));  // no such device
  if (c) { std::fprintf(stderr, "a failed pysdr_chan_create left a handle\n"); std::exit(1); }
}

// cplx: 0, or the complex-tap mode (USB, LSB, CW) the bank runs in, set through pysdr_bank_set_mode_cplx on a bank created as `mode`
static void bank_scenario(int mode, int ntaps_af, int cplx = 0) {
  const int M = 16, D = 4, nk = 5, max_in = 2049 * D + 3;
  pysdr_chan* ch = nullptr;
  OK(pysdr_chan_create(0, M, D, 13, nk, 2 * M, max_in, &ch));      // rows 13, 14, 15, 0, 1
  auto h = taps(2 * M);
  OK(pysdr_chan_set_taps(ch, h.data(), 2 * M));
  pysdr_bank* b = nullptr;
  OK(pysdr_bank_create(ch, 12000.0, mode, ntaps_af, &b));
  const long long cap = 2049 + 8;
  std::vector<float> x(2 * (size_t)max_in, 0.25f), am((size_t)nk * cap), iq(2 * (size_t)nk * cap);
  DevMem dx(8 * (size_t)max_in), dam(4 * (size_t)nk * cap);
  int nf = 0;
  FAILS(pysdr_bank_process(b, x.data(), D, 0, am.data(), cap, 0, &nf));                  // no mode set
  auto af = taps(ntaps_af);
  FAILS(pysdr_bank_set_mode(b, mode, af.data(), ntaps_af + 1));
  FAILS(pysdr_bank_set_mode(b, PYSDR_USB, af.data(), ntaps_af));
  FAILS(pysdr_bank_set_mode(b, mode, nullptr, ntaps_af));
  FAILS(pysdr_bank_set_mode(nullptr, mode, af.data(), ntaps_af));
  OK(pysdr_bank_set_mode(b, mode, af.data(), ntaps_af));
  const auto af_im = taps(ntaps_af, 0.5);
  auto set_own_mode = [&] {
    if (cplx) OK(pysdr_bank_set_mode_cplx(b, cplx, af.data(), af_im.data(), ntaps_af, 700.0));
    else OK(pysdr_bank_set_mode(b, mode, af.data(), ntaps_af));
  };
  if (cplx) {
    FAILS(pysdr_bank_set_mode_cplx(b, cplx, af.data(), af_im.data(), ntaps_af + 1, 700.0));
    FAILS(pysdr_bank_set_mode_cplx(b, PYSDR_AM, af.data(), af_im.data(), ntaps_af, 700.0));
    FAILS(pysdr_bank_set_mode_cplx(b, PYSDR_IQ, af.data(), af_im.data(), ntaps_af, 700.0));
    FAILS(pysdr_bank_set_mode_cplx(b, cplx, nullptr, af_im.data(), ntaps_af, 700.0));
    FAILS(pysdr_bank_set_mode_cplx(b, cplx, af.data(), nullptr, ntaps_af, 700.0));
    FAILS(pysdr_bank_set_mode_cplx(nullptr, cplx, af.data(), af_im.data(), ntaps_af, 700.0));
    set_own_mode();
  }
  unsigned long long s = 0;
  // am: 0 none, 1 host at pitch n_out, 2 device at pitch n_out, 3 device at a wider pitch
  auto run = [&](int n, int in_dev, int how) {
    const int want = (int)((s + n + D - 1) / D - (s + D - 1) / D);
    float* out = how == 0 ? nullptr : how == 1 ? am.data() : (float*)dam.p;
    OK(pysdr_bank_process(b, in_dev ? dx.p : (void*)x.data(), n, in_dev, out, how == 3 ? want + 5 : want, how >= 2, &nf));
    if (nf != want) { std::fprintf(stderr, "bank: %d outputs, %d expected\n", nf, want); std::exit(1); }
    s += n; ++g_obj_calls;
  };
  const int rows_run[] = {0, 1, 2}, rows_far[] = {4, 0, 2}, rows_rep[] = {1, 1, 3, 4, 4};
  auto fetches = [&] {
    OK(pysdr_bank_fetch(b, rows_run, 3, am.data(), iq.data(), nf + 1));
    OK(pysdr_bank_fetch(b, rows_far, 3, am.data(), nullptr, nf));
    OK(pysdr_bank_fetch(b, rows_far, 3, am.data(), iq.data(), cap));                     // three runs, audio and IQ of each in turn
    OK(pysdr_bank_fetch(b, rows_rep, 5, nullptr, iq.data(), cap));
    OK(pysdr_bank_fetch(b, rows_rep, 5, nullptr, nullptr, cap));
    OK(pysdr_bank_fetch(b, nullptr, 0, am.data(), iq.data(), cap));
    if (nf > 0) FAILS(pysdr_bank_fetch(b, rows_run, 3, am.data(), iq.data(), nf - 1));   // pitch too small
  };
  for (int pass = 0; pass < 4; ++pass) {
    // from s = 0 (mod D): 1 output, 0 outputs, exactly one tile, one more than a tile, nothing at all
    int k = pass;
    for (int n : {1, 1, 2048 * D, 2049 * D, 0, D - 2}) { run(n, k & 1, k & 3); fetches(); ++k; }
    if (pass == 1) { OK(pysdr_bank_set_squelch(b, 0.5f)); OK(pysdr_bank_set_agc(b, 0, 0.3f)); }
    if (pass == 2) {                                      // the other mode and back, then from the start
      OK(pysdr_bank_set_mode(b, mode == PYSDR_AM ? PYSDR_NFM : PYSDR_AM, af.data(), ntaps_af));
      run(2049 * D, 0, 1); fetches();
      set_own_mode();
      OK(pysdr_bank_reset(b)); s = 0;
      OK(pysdr_bank_set_agc(b, 1, 0.5f));
    }
  }
  std::vector<float> agc(nk), gain(nk), mx(nk), lvl(nk);
  std::vector<uint8_t> open(nk);
  OK(pysdr_bank_state(b, agc.data(), gain.data(), mx.data(), lvl.data(), open.data()));
  OK(pysdr_bank_state(b, nullptr, gain.data(), nullptr, nullptr, nullptr));
  OK(pysdr_bank_sync(b));
  // errors that must leave the stream where it was
  FAILS(pysdr_bank_process(b, x.data(), 8 * D, 0, am.data(), 7, 0, &nf));                // pitch too small
  FAILS(pysdr_bank_process(b, x.data(), max_in + 1, 0, am.data(), cap, 0, &nf));
  FAILS(pysdr_bank_process(b, x.data(), -1, 0, am.data(), cap, 0, &nf));
  FAILS(pysdr_bank_process(b, nullptr, 1, 0, am.data(), cap, 0, &nf));
  FAILS(pysdr_bank_process(b, x.data(), 1, 0, am.data(), cap, 0, nullptr));
  run(8 * D, 0, 1);
  // The channelizer fed beside its bank, between two bank calls: the bank reads the channelizer's sample count before
  // each call, so its next call is sized right (its rows' history has a gap: the caller's business).  The error itself
  // needs the direct call to land between that read and the bank's own channelizer call -- another thread.
  {
    std::vector<float> y(2 * (size_t)nk * 16);
    int n2 = 0;
    OK(pysdr_chan_process(ch, x.data(), 3 * D + 1, 0, y.data(), 16, 0, &n2));
    s += 3 * D + 1;
    run(5 * D, 0, 1); fetches();
  }
  const int bad_rows[] = {0, nk};
  FAILS(pysdr_bank_fetch(b, bad_rows, 2, am.data(), nullptr, cap));
  FAILS(pysdr_bank_fetch(b, rows_run, -1, am.data(), nullptr, cap));
  FAILS(pysdr_bank_fetch(b, nullptr, 1, am.data(), nullptr, cap));
  FAILS(pysdr_bank_fetch(nullptr, rows_run, 1, am.data(), nullptr, cap));
  FAILS(pysdr_bank_set_agc(b, 1, 0.f));
  FAILS(pysdr_bank_set_agc(nullptr, 1, 0.5f));
  FAILS(pysdr_bank_set_squelch(b, -1.f));
  FAILS(pysdr_bank_set_squelch(nullptr, 0.f));
  FAILS(pysdr_bank_state(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  FAILS(pysdr_bank_reset(nullptr));
  FAILS(pysdr_bank_sync(nullptr));
  pysdr_bank_destroy(b);
  pysdr_bank_destroy(nullptr);
  // create and plan errors
  int32_t pl[8];
  b = nullptr;
  OK(pysdr_bank_plan(nk, ntaps_af, 2049, pl));
  FAILS(pysdr_bank_plan(nk, ntaps_af, 2049, nullptr));
  FAILS(pysdr_bank_plan(0, ntaps_af, 2049, pl));
  FAILS(pysdr_bank_plan(4097, ntaps_af, 2049, pl));
  FAILS(pysdr_bank_plan(nk, 2, 2049, pl));
  FAILS(pysdr_bank_plan(nk, 256, 2049, pl));
  FAILS(pysdr_bank_plan(nk, ntaps_af, 0, pl));
  FAILS(pysdr_bank_create(ch, 12000.0, mode, ntaps_af, nullptr));
  FAILS(pysdr_bank_create(nullptr, 12000.0, mode, ntaps_af, &b));
  FAILS(pysdr_bank_create(ch, 12000.0, PYSDR_CW, ntaps_af, &b));
  FAILS(pysdr_bank_create(ch, 0.0, mode, ntaps_af, &b));
  FAILS(pysdr_bank_create(ch, 12000.0, mode, 2, &b));
  FAILS(pysdr_bank_create(ch, 12000.0, mode, 256, &b));
  if (b) { std::fprintf(stderr, "a failed pysdr_bank_create left a handle\n"); std::exit(1); }
  pysdr_chan_destroy(ch);
}

static void rtty_scenario(int find_lo, int find_hi) {
  const int nfft = 64, nsh = 5, bin_lo = 10, bin_hi = 30, max_lines = 33, nb = bin_hi - bin_lo;
  pysdr_rtty* r = nullptr;
  OK(pysdr_rtty_create(0, nfft, nsh, bin_lo, bin_hi, find_lo, find_hi, max_lines, &r));
  const int R = max_lines + 128, max_dec = max_lines / 30 + 1;
  std::vector<float> lines((size_t)max_lines * nfft, -80.f), best((size_t)max_lines * nb);
  DevMem dl(4 * (size_t)max_lines * nfft);
  std::vector<int> codes((size_t)max_dec * nb), ndet(max_lines), isym((size_t)max_lines * nb);
  std::vector<long long> t((size_t)max_dec * nb);
  std::vector<double> snr((size_t)max_dec * nb);
  long long n = 0, ndec_all = 0;
  int k = 0, wrapped_with_rows = 0;
  for (int cycle = 0; cycle < 5; ++cycle) {
    for (int nl : {0, 1, 29, 30, 31, max_lines}) {
      const bool want_isym = (k & 4) == 0 || (k % 3) == 0, want_best = (k & 8) == 0, rows = want_isym || want_best, dev = k & 1;   // both, either alone, neither
      int nd = -1;
      OK(pysdr_rtty_decode(r, dev ? (const float*)dl.p : lines.data(), nl, dev, (k >> 1) & 1, codes.data(), t.data(), snr.data(), &nd, ndet.data(),
                           want_isym ? isym.data() : nullptr, want_best ? best.data() : nullptr));
      const int want = (int)((n + nl) / 30 - n / 30);
      if (nd != want) { std::fprintf(stderr, "rtty: %d decisions, %d expected\n", nd, want); std::exit(1); }
      if (rows && nl > 0 && (n + 1) % R + nl > R) ++wrapped_with_rows;                   // the two-piece copies took both pieces
      n += nl; ndec_all += nd; ++k; ++g_obj_calls;
    }
    if (cycle == 2) { OK(pysdr_rtty_reset(r)); n = 0; }
  }
  if (wrapped_with_rows < 1) { std::fprintf(stderr, "rtty: the ring never wrapped inside a call that fetched its rows\n"); std::exit(1); }
  int nd = 0;
  FAILS(pysdr_rtty_decode(nullptr, lines.data(), 1, 0, 1, codes.data(), t.data(), snr.data(), &nd, ndet.data(), nullptr, nullptr));
  FAILS(pysdr_rtty_decode(r, lines.data(), -1, 0, 1, codes.data(), t.data(), snr.data(), &nd, ndet.data(), nullptr, nullptr));
  FAILS(pysdr_rtty_decode(r, lines.data(), max_lines + 1, 0, 1, codes.data(), t.data(), snr.data(), &nd, ndet.data(), nullptr, nullptr));
  FAILS(pysdr_rtty_decode(r, nullptr, 1, 0, 1, codes.data(), t.data(), snr.data(), &nd, ndet.data(), nullptr, nullptr));
  FAILS(pysdr_rtty_decode(r, lines.data(), 1, 0, 1, nullptr, t.data(), snr.data(), &nd, ndet.data(), nullptr, nullptr));
  FAILS(pysdr_rtty_decode(r, lines.data(), 1, 0, 1, codes.data(), t.data(), snr.data(), nullptr, ndet.data(), nullptr, nullptr));
  FAILS(pysdr_rtty_reset(nullptr));
  pysdr_rtty_destroy(r);
  pysdr_rtty_destroy(nullptr);
  r = nullptr;
  const int top = nfft - nsh;
  FAILS(pysdr_rtty_create(0, nfft, nsh, bin_lo, bin_hi, 0, 0, max_lines, nullptr));
  FAILS(pysdr_rtty_create(0, 1, 1, 0, 1, 0, 0, max_lines, &r));
  FAILS(pysdr_rtty_create(0, nfft, 0, bin_lo, bin_hi, 0, 0, max_lines, &r));
  FAILS(pysdr_rtty_create(0, nfft, nfft, bin_lo, bin_hi, 0, 0, max_lines, &r));
  FAILS(pysdr_rtty_create(0, nfft, nsh, -1, bin_hi, 0, 0, max_lines, &r));
  FAILS(pysdr_rtty_create(0, nfft, nsh, bin_lo, top + 1, 0, 0, max_lines, &r));
  FAILS(pysdr_rtty_create(0, nfft, nsh, bin_hi, bin_hi, 0, 0, max_lines, &r));
  FAILS(pysdr_rtty_create(0, nfft, nsh, bin_lo, bin_hi, -1, 5, max_lines, &r));
  FAILS(pysdr_rtty_create(0, nfft, nsh, bin_lo, bin_hi, 0, top + 1, max_lines, &r));
  FAILS(pysdr_rtty_create(0, nfft, nsh, bin_lo, bin_hi, 9, 8, max_lines, &r));
  FAILS(pysdr_rtty_create(0, nfft, nsh, bin_lo, bin_hi, 0, 0, 0, &r));
  FAILS(pysdr_rtty_create(0, nfft, nsh, bin_lo, bin_hi, 0, 0, 32769, &r));
  FAILS(pysdr_rtty_create(1, nfft, nsh, bin_lo, bin_hi, 0, 0, max_lines, &r));
  if (r) { std::fprintf(stderr, "a failed pysdr_rtty_create left a handle\n"); std::exit(1); }
}

static void waterfall_scenario() {
  const int nfft = 64, ncols = 5;
  pysdr_waterfall* w = nullptr;
  OK(pysdr_waterfall_create(0, nfft, ncols, &w));
  std::vector<float> line(nfft, -70.f), img((size_t)nfft * ncols), mean(nfft);
  for (int i = 0; i < nfft; ++i) line[i] += (float)((i * 7) % 11);
  DevMem dl(4 * (size_t)nfft);
  float bk = 0;
  int np = 0;
  std::vector<int> idx(40);
  FAILS(pysdr_waterfall_image(w, 60.f, img.data(), mean.data(), &bk));                   // before the first push
  FAILS(pysdr_waterfall_peaks(w, nullptr, nfft, -60.0, 3, idx.data(), 40, &np));
  OK(pysdr_waterfall_peaks(w, line.data(), nfft, -60.0, 3, idx.data(), 40, &np));       // a passed line needs no push
  int k = 0;
  for (int n : {0, 10, nfft, 1, nfft - 1, nfft, 33, nfft}) {                             // more lines than columns
    OK(pysdr_waterfall_push(w, (k & 1) ? (const float*)dl.p : line.data(), n, k & 1));
    OK(pysdr_waterfall_roll(w, k == 2 ? 3 : k == 3 ? -7 : k == 4 ? 3 * nfft + 8 : k == 5 ? -2 * nfft - 9 : 0));
    OK(pysdr_waterfall_image(w, 60.f, img.data(), mean.data(), &bk));
    OK(pysdr_waterfall_image(w, 60.f, nullptr, mean.data(), &bk));
    OK(pysdr_waterfall_image(w, 60.f, img.data(), nullptr, &bk));
    OK(pysdr_waterfall_image(w, 60.f, img.data(), mean.data(), nullptr));
    OK(pysdr_waterfall_image_rows(w, 60.f, 20, img.data(), mean.data(), &bk));
    OK(pysdr_waterfall_peaks(w, nullptr, nfft, -60.0, 3, nullptr, 0, &np));              // from the mean, count only
    OK(pysdr_waterfall_peaks(w, nullptr, nfft, -60.0, 1, idx.data(), 40, &np));
    OK(pysdr_waterfall_peaks(w, line.data(), 17, -60.0, 2, idx.data(), 3, &np));         // fewer slots than peaks
    OK(pysdr_waterfall_peaks(w, line.data(), 0, -60.0, 2, idx.data(), 3, &np));
    ++k; ++g_obj_calls;
  }
  FAILS(pysdr_waterfall_push(w, nullptr, 1, 0));
  FAILS(pysdr_waterfall_push(w, line.data(), -1, 0));
  FAILS(pysdr_waterfall_push(w, line.data(), nfft + 1, 0));
  FAILS(pysdr_waterfall_push(nullptr, line.data(), 1, 0));
  FAILS(pysdr_waterfall_roll(nullptr, 1));
  FAILS(pysdr_waterfall_image(nullptr, 60.f, img.data(), mean.data(), &bk));
  FAILS(pysdr_waterfall_image_rows(w, 60.f, 0, img.data(), mean.data(), &bk));
  FAILS(pysdr_waterfall_image_rows(w, 60.f, nfft + 1, img.data(), mean.data(), &bk));
  FAILS(pysdr_waterfall_peaks(w, line.data(), nfft + 1, -60.0, 3, idx.data(), 40, &np));
  FAILS(pysdr_waterfall_peaks(w, line.data(), nfft, -60.0, 0, idx.data(), 40, &np));
  FAILS(pysdr_waterfall_peaks(w, line.data(), nfft, -60.0, 3, idx.data(), -1, &np));
  FAILS(pysdr_waterfall_peaks(w, line.data(), nfft, -60.0, 3, nullptr, 4, &np));
  FAILS(pysdr_waterfall_peaks(w, line.data(), nfft, -60.0, 3, idx.data(), 40, nullptr));
  pysdr_waterfall_destroy(w);
  pysdr_waterfall_destroy(nullptr);
  w = nullptr;
  FAILS(pysdr_waterfall_create(0, nfft, ncols, nullptr));
  FAILS(pysdr_waterfall_create(0, 1, ncols, &w));
  FAILS(pysdr_waterfall_create(0, nfft, 0, &w));
  FAILS(pysdr_waterfall_create(1, nfft, ncols, &w));
  if (w) { std::fprintf(stderr, "a failed pysdr_waterfall_create left a handle\n"); std::exit(1); }
}

static void stream_objects() {
  g_obj_calls = 0;
  channelizer_errors();
  for (int D : {16, 8, 4}) channelizer_scenario(16, D, 11, 9, 3 * 16 + 5, 300 * D + 5);  // rows 11 .. 15, 0 .. 3; more than one workgroup
  channelizer_scenario(80, 20, 77, 80, 2 * 80, 1000);                                    // 2^4 5: a radix-5 pass, every channel
  for (int mode : {PYSDR_AM, PYSDR_NFM})
    for (int ntaps_af : {3, 8, 9, 255}) bank_scenario(mode, ntaps_af);
  rtty_scenario(0, 0);                                    // finder range empty
  rtty_scenario(5, 50);                                   // ... and wider than the decoders' on both sides
  waterfall_scenario();
  std::printf("stream objects: %d calls\n", g_obj_calls);
}

// ---- the objects that borrow a channelizer beside the bank -- CW skimmer (api_cw.hip), PSK31 skimmer (api_psk.hip) -- the
// fine channelizer they may borrow instead (api_fine.hip), and the bank's complex-tap modes: part of `san_main objects`
static int g_skim_calls = 0, g_fine_calls = 0;

static pysdr_cw_cfg good_cw_cfg() {
  pysdr_cw_cfg c;
  c.a_s = 0.3f; c.a_p = 0.01f; c.a_n = 0.01f; c.snr_min = 4.f; c.hi = 0.5f; c.lo = 0.25f; c.fl = 1e-3f;
  c.d0 = 64; c.dmin = 16; c.dmax = 1024; c.n0 = 8;
  return c;
}
static pysdr_psk_cfg good_psk_cfg() {
  pysdr_psk_cfg c;
  c.a_t = 0.05f; c.a_q = 0.1f; c.hi = 0.5f; c.lo = 0.25f; c.hy = 1.5f; c.pmax = 1e6f; c.n0 = 4;
  return c;
}

// What the two skimmers' call lists have in common: one scenario runs over either.
struct Skimmer {
  int nrow = 0, cap = 0;     // event rows (channels / decoders) and the event cap
  std::function<int(const void* iq, int n, int on_device, int* n_out, int32_t* counts, int32_t* events, long long ev_pitch, bool extras)> process;
  std::function<int(const int* rows, int nrows, int32_t* events, long long pitch)> fetch;
  std::function<int(int which)> state;       // which: 0 every output, 1 .. some of them NULL
  std::function<int()> reset, sync;
};

static void skimmer_scenario(const Skimmer& sk, pysdr_chan* ch, int D, int max_in, int max_out) {
  const long long wide = sk.cap + 3;
  std::vector<float> x(2 * (size_t)max_in, 0.25f);
  DevMem dx(8 * (size_t)max_in);
  std::vector<int32_t> counts(sk.nrow), events((size_t)sk.nrow * wide);
  unsigned long long s = 0;
  int nf = 0, k = 0;
  // how: 0 neither counts nor events, 1 counts only, 2 both at pitch cap, 3 both at a wider pitch
  auto run = [&](int n, int in_dev, int how) {
    const int want = (int)((s + n + D - 1) / D - (s + D - 1) / D);
    OK(sk.process(in_dev ? dx.p : (void*)x.data(), n, in_dev, &nf, how ? counts.data() : nullptr, how >= 2 ? events.data() : nullptr,
                  how == 3 ? wide : sk.cap, (k % 3) != 0));
    if (nf != want) { std::fprintf(stderr, "skimmer: %d outputs, %d expected\n", nf, want); std::exit(1); }
    s += n; ++k; ++g_skim_calls;
  };
  const int rows_run[] = {0, 1, 2}, rows_far[] = {sk.nrow - 1, 0, 2}, rows_rep[] = {1, 1, 3, sk.nrow - 1, sk.nrow - 1};
  auto fetches = [&] {
    OK(sk.fetch(rows_run, 3, events.data(), sk.cap));
    OK(sk.fetch(rows_far, 3, events.data(), wide));
    OK(sk.fetch(rows_rep, 5, events.data(), wide));
    OK(sk.fetch(nullptr, 0, events.data(), sk.cap));
    OK(sk.fetch(rows_run, 0, nullptr, sk.cap));
  };
  for (int how : {3, 2, 1, 0})
    for (int in_dev : {0, 1})
      for (int n : {0, 1, D - 1, D, D + 1, 8 * D, 7}) { run(n, in_dev, how); fetches(); }
  for (int which = 0; which < 3; ++which) OK(sk.state(which));
  OK(sk.reset()); s = 0;
  fetches();                                              // nothing to fetch after a reset: no copy
  OK(sk.sync());
  // refused calls, and after each a good one: the stream did not move
  FAILS(sk.process(x.data(), (max_out + 1) * D, 0, &nf, counts.data(), nullptr, sk.cap, false));   // would complete max_out + 1
  if (nf != 0) { std::fprintf(stderr, "skimmer: a refused call left n_out %d\n", nf); std::exit(1); }
  run(max_out * D, 0, 2);
  FAILS(sk.process(x.data(), D, 0, &nf, counts.data(), events.data(), sk.cap - 1, false));        // ev_pitch below the cap
  run(D + 1, 1, 1);
  FAILS(sk.process(x.data(), max_in + 1, 0, &nf, counts.data(), nullptr, sk.cap, false));
  run(1, 0, 0);
  FAILS(sk.process(x.data(), -1, 0, &nf, counts.data(), nullptr, sk.cap, false));
  run(D, 0, 3);
  FAILS(sk.process(nullptr, 1, 0, &nf, counts.data(), nullptr, sk.cap, false));
  run(2, 1, 2);
  FAILS(sk.process(x.data(), 1, 0, nullptr, counts.data(), nullptr, sk.cap, false));
  run(D - 1, 0, 1); fetches();
  FAILS(sk.fetch(rows_run, 3, events.data(), sk.cap - 1));                                         // pitch below the cap
  const int bad_hi[] = {0, sk.nrow}, bad_lo[] = {-1};
  FAILS(sk.fetch(bad_hi, 2, events.data(), sk.cap));
  FAILS(sk.fetch(bad_lo, 1, events.data(), sk.cap));
  FAILS(sk.fetch(rows_run, -1, events.data(), sk.cap));
  FAILS(sk.fetch(nullptr, 1, events.data(), sk.cap));
  FAILS(sk.fetch(rows_run, 1, nullptr, sk.cap));
  fetches();
  // the channelizer fed beside its skimmer, between two calls (bank_scenario): the next call is sized right
  {
    std::vector<float> y(2 * (size_t)sk.nrow * 16);
    int n2 = 0;
    OK(pysdr_chan_process(ch, x.data(), 3 * D + 1, 0, y.data(), 16, 0, &n2));
    s += 3 * D + 1;
    run(5 * D, 0, 3); fetches();
  }
  run(0, 0, 1);                                           // no output: the counts are zeroed, (PSK) qn and open still copied
  run(0, 1, 0);
}

static void cw_scenario() {
  const int M = 16, D = 4, nk = 5, max_out = 8, max_in = (max_out + 1) * D + 3;
  pysdr_chan* ch = nullptr;
  OK(pysdr_chan_create(0, M, D, 13, nk, 2 * M, max_in, &ch));      // rows 13, 14, 15, 0, 1
  const auto h = taps(2 * M);
  OK(pysdr_chan_set_taps(ch, h.data(), 2 * M));
  const pysdr_cw_cfg cfg = good_cw_cfg();
  int32_t pl[8];
  OK(pysdr_cw_plan(nk, max_out, &cfg, pl));
  pysdr_cw* w = nullptr;
  OK(pysdr_cw_create(ch, &cfg, max_out, &w));
  std::vector<float> zs(nk), pk(nk), zn(nk);
  std::vector<int32_t> ints(8 * (size_t)nk);
  Skimmer sk;
  sk.nrow = nk; sk.cap = pl[4];
  sk.process = [&](const void* iq, int n, int dev, int* n_out, int32_t* counts, int32_t* events, long long pitch, bool) {
    return pysdr_cw_process(w, iq, n, dev, n_out, counts, events, pitch);
  };
  sk.fetch = [&](const int* rows, int nrows, int32_t* events, long long pitch) { return pysdr_cw_fetch(w, rows, nrows, events, pitch); };
  sk.state = [&](int which) {
    return which == 0 ? pysdr_cw_state(w, zs.data(), pk.data(), zn.data(), ints.data())
         : which == 1 ? pysdr_cw_state(w, nullptr, pk.data(), nullptr, nullptr) : pysdr_cw_state(w, nullptr, nullptr, nullptr, ints.data());
  };
  sk.reset = [&] { return pysdr_cw_reset(w); };
  sk.sync = [&] { return pysdr_cw_sync(w); };
  skimmer_scenario(sk, ch, D, max_in, max_out);
  int nf = 0;
  FAILS(pysdr_cw_process(nullptr, h.data(), 1, 0, &nf, nullptr, nullptr, 0));
  FAILS(pysdr_cw_fetch(nullptr, nullptr, 0, nullptr, 0));
  FAILS(pysdr_cw_state(nullptr, nullptr, nullptr, nullptr, nullptr));
  FAILS(pysdr_cw_reset(nullptr));
  FAILS(pysdr_cw_sync(nullptr));
  pysdr_cw_destroy(w);
  pysdr_cw_destroy(nullptr);
  // a cfg outside each rule of the plan, and the create errors
  FAILS(pysdr_cw_plan(nk, max_out, &cfg, nullptr));
  FAILS(pysdr_cw_plan(0, max_out, &cfg, pl));
  FAILS(pysdr_cw_plan(4097, max_out, &cfg, pl));
  FAILS(pysdr_cw_plan(nk, 0, &cfg, pl));
  FAILS(pysdr_cw_plan(nk, (1 << 21) + 1, &cfg, pl));
  FAILS(pysdr_cw_plan(nk, max_out, nullptr, pl));
  auto bad = [&](void (*change)(pysdr_cw_cfg&)) { pysdr_cw_cfg c = cfg; change(c); FAILS(pysdr_cw_plan(nk, max_out, &c, pl)); };
  bad([](pysdr_cw_cfg& c) { c.a_s = 0.f; });
  bad([](pysdr_cw_cfg& c) { c.a_p = 1.5f; });
  bad([](pysdr_cw_cfg& c) { c.a_n = NAN; });
  bad([](pysdr_cw_cfg& c) { c.snr_min = 0.f; });
  bad([](pysdr_cw_cfg& c) { c.hi = INFINITY; });
  bad([](pysdr_cw_cfg& c) { c.lo = 2.f * c.hi; });
  bad([](pysdr_cw_cfg& c) { c.fl = -1.f; });
  bad([](pysdr_cw_cfg& c) { c.dmin = 15; });
  bad([](pysdr_cw_cfg& c) { c.d0 = c.dmin - 1; });
  bad([](pysdr_cw_cfg& c) { c.dmax = c.d0 - 1; });
  bad([](pysdr_cw_cfg& c) { c.dmax = (1 << 22) + 1; });
  bad([](pysdr_cw_cfg& c) { c.n0 = 0; });
  bad([](pysdr_cw_cfg& c) { c.n0 = (1 << 22) + 1; });
  w = nullptr;
  pysdr_cw_cfg nope = cfg;
  nope.n0 = 0;
  FAILS(pysdr_cw_create(ch, &cfg, max_out, nullptr));
  FAILS(pysdr_cw_create(nullptr, &cfg, max_out, &w));
  FAILS(pysdr_cw_create(ch, nullptr, max_out, &w));
  FAILS(pysdr_cw_create(ch, &nope, max_out, &w));
  FAILS(pysdr_cw_create(ch, &cfg, 0, &w));
  if (w) { std::fprintf(stderr, "a failed pysdr_cw_create left a handle\n"); std::exit(1); }
  pysdr_chan_destroy(ch);
}

static void psk_scenario(int S) {
  const int M = 16, D = 4, nk = 3, max_out = 8, max_in = (max_out + 1) * D + 3;
  pysdr_chan* ch = nullptr;
  OK(pysdr_chan_create(0, M, D, 15, nk, 2 * M, max_in, &ch));      // rows 15, 0, 1
  const auto h = taps(2 * M);
  OK(pysdr_chan_set_taps(ch, h.data(), 2 * M));
  const pysdr_psk_cfg cfg = good_psk_cfg();
  int32_t pl[8];
  OK(pysdr_psk_plan(nk, S, max_out, &cfg, pl));
  const int nfine = nk * pl[6];
  std::vector<float> tw(2 * 32 * (size_t)S, 0.5f), g(2 * (size_t)S, 0.1f);
  pysdr_psk* w = nullptr;
  OK(pysdr_psk_create(ch, S, &cfg, tw.data(), g.data(), max_out, &w));
  std::vector<float> qn(nfine), e((size_t)S * nfine), f(4 * (size_t)nfine);
  std::vector<int32_t> open(nfine), ints(5 * (size_t)nfine);
  Skimmer sk;
  sk.nrow = nfine; sk.cap = pl[4];
  int extras_k = 0;
  sk.process = [&](const void* iq, int n, int dev, int* n_out, int32_t* counts, int32_t* events, long long pitch, bool extras) {
    const int which = extras ? 1 + (extras_k++ % 3) : 0;               // qn and open: both, either alone, neither
    return pysdr_psk_process(w, iq, n, dev, n_out, counts, events, pitch, (which & 1) ? qn.data() : nullptr, (which & 2) ? open.data() : nullptr);
  };
  sk.fetch = [&](const int* rows, int nrows, int32_t* events, long long pitch) { return pysdr_psk_fetch(w, rows, nrows, events, pitch); };
  sk.state = [&](int which) {
    return which == 0 ? pysdr_psk_state(w, e.data(), f.data(), ints.data())
         : which == 1 ? pysdr_psk_state(w, nullptr, f.data(), nullptr) : pysdr_psk_state(w, nullptr, nullptr, nullptr);
  };
  sk.reset = [&] { return pysdr_psk_reset(w); };
  sk.sync = [&] { return pysdr_psk_sync(w); };
  skimmer_scenario(sk, ch, D, max_in, max_out);
  int nf = 0;
  FAILS(pysdr_psk_process(nullptr, h.data(), 1, 0, &nf, nullptr, nullptr, 0, nullptr, nullptr));
  FAILS(pysdr_psk_fetch(nullptr, nullptr, 0, nullptr, 0));
  FAILS(pysdr_psk_state(nullptr, nullptr, nullptr, nullptr));
  FAILS(pysdr_psk_reset(nullptr));
  FAILS(pysdr_psk_sync(nullptr));
  pysdr_psk_destroy(w);
  pysdr_psk_destroy(nullptr);
  FAILS(pysdr_psk_plan(nk, S, max_out, &cfg, nullptr));
  FAILS(pysdr_psk_plan(nk, 10, max_out, &cfg, pl));
  FAILS(pysdr_psk_plan(0, S, max_out, &cfg, pl));
  FAILS(pysdr_psk_plan((1 << 18) / (4 * S) + 1, S, max_out, &cfg, pl));
  FAILS(pysdr_psk_plan(nk, S, 0, &cfg, pl));
  FAILS(pysdr_psk_plan(nk, S, (1 << 20) + 1, &cfg, pl));
  FAILS(pysdr_psk_plan(nk, S, max_out, nullptr, pl));
  auto bad = [&](void (*change)(pysdr_psk_cfg&)) { pysdr_psk_cfg c = cfg; change(c); FAILS(pysdr_psk_plan(nk, S, max_out, &c, pl)); };
  bad([](pysdr_psk_cfg& c) { c.a_t = 0.f; });
  bad([](pysdr_psk_cfg& c) { c.a_q = 1.5f; });
  bad([](pysdr_psk_cfg& c) { c.hi = INFINITY; });
  bad([](pysdr_psk_cfg& c) { c.lo = 2.f * c.hi; });
  bad([](pysdr_psk_cfg& c) { c.lo = 0.f; });
  bad([](pysdr_psk_cfg& c) { c.hy = NAN; });
  bad([](pysdr_psk_cfg& c) { c.pmax = 2e18f; });
  bad([](pysdr_psk_cfg& c) { c.pmax = 0.f; });
  bad([](pysdr_psk_cfg& c) { c.n0 = 0; });
  bad([](pysdr_psk_cfg& c) { c.n0 = (1 << 22) + 1; });
  w = nullptr;
  FAILS(pysdr_psk_create(ch, S, &cfg, tw.data(), g.data(), max_out, nullptr));
  FAILS(pysdr_psk_create(nullptr, S, &cfg, tw.data(), g.data(), max_out, &w));
  FAILS(pysdr_psk_create(ch, S, nullptr, tw.data(), g.data(), max_out, &w));
  FAILS(pysdr_psk_create(ch, S, &cfg, nullptr, g.data(), max_out, &w));
  FAILS(pysdr_psk_create(ch, S, &cfg, tw.data(), nullptr, max_out, &w));
  FAILS(pysdr_psk_create(ch, 10, &cfg, tw.data(), g.data(), max_out, &w));
  FAILS(pysdr_psk_create(ch, S, &cfg, tw.data(), g.data(), 0, &w));
  if (w) { std::fprintf(stderr, "a failed pysdr_psk_create left a handle\n"); std::exit(1); }
  pysdr_chan_destroy(ch);
}

static void fine_errors() {
  int32_t pl[16];
  pysdr_chan* c = nullptr;
  OK(pysdr_chan_fine_plan(16, 8, 16, 8, 32, 32, 5, 20, pl));
  if (pl[5] < 2) { std::fprintf(stderr, "fine: the scenario's shape uses %d coarse rows\n", pl[5]); std::exit(1); }
  FAILS(pysdr_chan_fine_plan(16, 8, 16, 8, 32, 32, 5, 20, nullptr));
  FAILS(pysdr_chan_fine_plan(15, 5, 16, 8, 32, 32, 0, 1, pl));             // M1 < 16
  FAILS(pysdr_chan_fine_plan(48, 24, 16, 8, 32, 32, 0, 1, pl));            // a factor 3
  FAILS(pysdr_chan_fine_plan(16, 16, 16, 8, 32, 32, 0, 1, pl));            // M1 / D1 = 1: a row carries its own spacing only
  FAILS(pysdr_chan_fine_plan(16, 3, 16, 8, 32, 32, 0, 1, pl));
  FAILS(pysdr_chan_fine_plan(16, 8, 8, 4, 32, 32, 0, 1, pl));              // M2 < 16
  FAILS(pysdr_chan_fine_plan(16, 8, 2048, 1024, 32, 32, 0, 1, pl));
  FAILS(pysdr_chan_fine_plan(16, 8, 48, 24, 32, 32, 0, 1, pl));
  FAILS(pysdr_chan_fine_plan(16, 8, 16, 2, 32, 32, 0, 1, pl));             // M2 / D2 = 8
  FAILS(pysdr_chan_fine_plan(16, 8, 16, 0, 32, 32, 0, 1, pl));
  FAILS(pysdr_chan_fine_plan(16, 4, 16, 8, 32, 32, 0, 1, pl));             // Q = 4
  FAILS(pysdr_chan_fine_plan(16, 4, 50, 25, 32, 32, 0, 1, pl));            // M2 not a multiple of M1 / D1
  FAILS(pysdr_chan_fine_plan(16, 8, 50, 25, 32, 32, 0, 1, pl));            // Q = 25, odd
  FAILS(pysdr_chan_fine_plan(16, 8, 16, 8, 0, 32, 0, 1, pl));
  FAILS(pysdr_chan_fine_plan(16, 8, 16, 8, 16 * 16 + 1, 32, 0, 1, pl));
  FAILS(pysdr_chan_fine_plan(16, 8, 16, 8, 32, 0, 0, 1, pl));
  FAILS(pysdr_chan_fine_plan(16, 8, 16, 8, 32, 16 * 16 + 1, 0, 1, pl));
  FAILS(pysdr_chan_fine_plan(16, 8, 16, 8, 32, 32, -1, 1, pl));
  FAILS(pysdr_chan_fine_plan(16, 8, 16, 8, 32, 32, 128, 1, pl));
  FAILS(pysdr_chan_fine_plan(16, 8, 16, 8, 32, 32, 0, 0, pl));
  FAILS(pysdr_chan_fine_plan(16, 8, 16, 8, 32, 32, 0, 129, pl));
  FAILS(pysdr_chan_fine_create(0, 16, 8, 16, 8, 5, 20, 32, 32, 100, nullptr));
  FAILS(pysdr_chan_fine_create(0, 16, 16, 16, 8, 5, 20, 32, 32, 100, &c));
  FAILS(pysdr_chan_fine_create(0, 16, 8, 16, 8, 5, 20, 32, 32, 0, &c));
  FAILS(pysdr_chan_fine_create(0, 16, 8, 16, 8, 5, 20, 32, 32, (1 << 28) + 1, &c));
  FAILS(pysdr_chan_fine_create(1, 16, 8, 16, 8, 5, 20, 32, 32, 100, &c));  // no such device
  if (c) { std::fprintf(stderr, "a failed pysdr_chan_fine_create left a handle\n"); std::exit(1); }
}

static void fine_scenario(int M1, int D1, int M2, int D2, int g_first, int ng) {
  const int D = D1 * D2, max_taps1 = 2 * M1 + 5, max_taps2 = 3 * M2 + 5, max_in = 5 * D + 5;
  pysdr_chan* c = nullptr;
  OK(pysdr_chan_fine_create(0, M1, D1, M2, D2, g_first, ng, max_taps1, max_taps2, max_in, &c));
  const long long pitch = max_in / D + 2;
  std::vector<float> x(2 * (size_t)max_in, 0.25f), y(2 * (size_t)ng * pitch);
  DevMem dx(8 * (size_t)max_in), dy(8 * (size_t)ng * (pitch + 3));
  int nf = 0;
  FAILS(pysdr_chan_process(c, x.data(), 1, 0, y.data(), pitch, 0, &nf));                 // no taps yet
  const auto h1 = taps(max_taps1), h2 = taps(max_taps2);
  FAILS(pysdr_chan_set_taps(c, h1.data(), max_taps1));                                   // a fine handle takes both prototypes at once
  FAILS(pysdr_chan_fine_set_taps(c, h1.data(), 0, h2.data(), max_taps2));
  FAILS(pysdr_chan_fine_set_taps(c, h1.data(), max_taps1 + 1, h2.data(), max_taps2));
  FAILS(pysdr_chan_fine_set_taps(c, h1.data(), max_taps1, h2.data(), 0));
  FAILS(pysdr_chan_fine_set_taps(c, h1.data(), max_taps1, h2.data(), max_taps2 + 1));
  FAILS(pysdr_chan_fine_set_taps(c, nullptr, max_taps1, h2.data(), max_taps2));
  FAILS(pysdr_chan_fine_set_taps(c, h1.data(), max_taps1, nullptr, max_taps2));
  FAILS(pysdr_chan_fine_set_taps(nullptr, h1.data(), max_taps1, h2.data(), max_taps2));
  OK(pysdr_chan_fine_set_taps(c, h1.data(), max_taps1, h2.data(), max_taps2));
  unsigned long long s = 0;
  auto run = [&](int n, int in_dev, int out_dev) {
    const int want = (int)((s + n + D - 1) / D - (s + D - 1) / D);
    OK(pysdr_chan_process(c, in_dev ? dx.p : (void*)x.data(), n, in_dev, out_dev ? dy.p : (void*)y.data(), out_dev ? pitch + 3 : pitch, out_dev, &nf));
    if (nf != want) { std::fprintf(stderr, "fine channelizer: %d outputs, %d expected\n", nf, want); std::exit(1); }
    s += n; ++g_fine_calls;
  };
  for (int combo = 0; combo < 4; ++combo)                 // host / device input x host / device output
    for (int n : {0, 1, D - 1, D, D + 1, max_in, 7, D1, D1 + 1, max_in - 1}) run(n, combo & 1, combo >> 1);
  OK(pysdr_chan_fine_set_taps(c, h1.data(), M1 - 3, h2.data(), M2 - 3));                 // shorter prototypes: one tap row each
  run(max_in, 0, 0); run(3, 1, 1);
  OK(pysdr_chan_reset(c)); s = 0;
  run(D + 1, 0, 1); run(max_in, 1, 0);
  OK(pysdr_chan_sync(c));
  FAILS(pysdr_chan_process(c, x.data(), max_in + 1, 0, y.data(), pitch, 0, &nf));
  FAILS(pysdr_chan_process(c, x.data(), -1, 0, y.data(), pitch, 0, &nf));
  FAILS(pysdr_chan_process(c, nullptr, 1, 0, y.data(), pitch, 0, &nf));
  FAILS(pysdr_chan_process(c, x.data(), 1, 0, y.data(), pitch, 0, nullptr));
  FAILS(pysdr_chan_process(c, x.data(), 2 * D, 0, nullptr, pitch, 0, &nf));              // outputs and nowhere to put them
  FAILS(pysdr_chan_process(c, x.data(), 2 * D, 0, y.data(), 1, 0, &nf));                 // pitch too small
  run(2 * D, 0, 0);                                                                      // ... and none of them moved the stream
  // a CW skimmer, then a bank, on the fine handle: two calls each
  const int max_out = max_in / D + 1;
  {
    const pysdr_cw_cfg cfg = good_cw_cfg();
    int32_t pl[8];
    OK(pysdr_cw_plan(ng, max_out, &cfg, pl));
    pysdr_cw* w = nullptr;
    OK(pysdr_cw_create(c, &cfg, max_out, &w));
    std::vector<int32_t> counts(ng), events((size_t)ng * pl[4]);
    OK(pysdr_cw_process(w, x.data(), max_in, 0, &nf, counts.data(), events.data(), pl[4]));
    OK(pysdr_cw_process(w, dx.p, D + 1, 1, &nf, counts.data(), nullptr, 0));
    const int rows[] = {ng - 1, 0, 1};
    OK(pysdr_cw_fetch(w, rows, 3, events.data(), pl[4]));
    g_fine_calls += 2;
    pysdr_cw_destroy(w);
  }
  {
    pysdr_bank* b = nullptr;
    OK(pysdr_bank_create(c, 12000.0, PYSDR_AM, 9, &b));
    const auto af = taps(9);
    OK(pysdr_bank_set_mode_cplx(b, PYSDR_CW, af.data(), af.data(), 9, 700.0));
    std::vector<float> am((size_t)ng * max_out), iq(2 * (size_t)ng * max_out);
    OK(pysdr_bank_process(b, x.data(), max_in, 0, am.data(), max_out, 0, &nf));
    OK(pysdr_bank_process(b, dx.p, D + 1, 1, nullptr, 0, 0, &nf));
    const int rows[] = {ng - 1, 0, 1};
    OK(pysdr_bank_fetch(b, rows, 3, am.data(), iq.data(), max_out));
    g_fine_calls += 2;
    pysdr_bank_destroy(b);
  }
  pysdr_chan_destroy(c);
}

static void channelizer_clients() {
  g_skim_calls = g_fine_calls = 0;
  const int before = g_obj_calls;
  cw_scenario();
  for (int S : {8, 12}) psk_scenario(S);
  fine_errors();
  fine_scenario(16, 8, 16, 8, 5, 20);                     // the smallest shape the plan accepts, three coarse rows
  fine_scenario(16, 8, 20, 5, 150, 25);                   // M2 = 2^2 5: a radix-5 pass; the fine range wraps
  for (int mode : {PYSDR_USB, PYSDR_LSB, PYSDR_CW})
    for (int ntaps_af : {3, 8, 9, 255}) bank_scenario(ntaps_af == 8 ? PYSDR_NFM : PYSDR_AM, ntaps_af, mode);
  std::printf("channelizer clients: %d skimmer calls, %d fine calls, %d sideband bank calls\n", g_skim_calls, g_fine_calls, g_obj_calls - before);
}

// ---- `san_main allocfail`: the n-th hipMalloc / hipHostMalloc / event / stream creation of a run fails (fake_hip).  Every
// step of the scenario that fails must leave a message, and must succeed when it is simply called again -- a half-built
// object was destroyed by its create function, a half-added receiver slot is taken over by the next pysdr_rx_add, a
// half-allocated lazy buffer set is completed by the next call -- and everything is destroyed at the end under
// AddressSanitizer / LeakSanitizer.  (A malloc that returns an error in a CPU process: nothing here can run on a device.)
static int g_failed_steps = 0;
#define STEP(expr)                                                                                                      \
  do {                                                                                                                  \
    int rc_ = (expr);                                                                                                   \
    if (rc_ != 0) {                                                                                                     \
      if (!fake_hip::state().fail_hit) { std::fprintf(stderr, "%s:%d %s -> %d (%s) without an injected failure\n", __FILE__, __LINE__, #expr, rc_, pysdr_last_error()); std::exit(1); } \
      if (!*pysdr_last_error()) { std::fprintf(stderr, "%s:%d %s -> %d without a message\n", __FILE__, __LINE__, #expr, rc_); std::exit(1); } \
      ++g_failed_steps;                                                                                                 \
      rc_ = (expr);                                                                                                     \
      if (rc_ != 0) { std::fprintf(stderr, "%s:%d %s fails again after the injected failure -> %d (%s)\n", __FILE__, __LINE__, #expr, rc_, pysdr_last_error()); std::exit(1); } \
    }                                                                                                                   \
  } while (0)

static void allocfail_scenario() {
  const int ntaps = 255, L = 8192, max_chunks = 2;
  const auto h = taps(ntaps), af = taps(2 * ntaps);
  std::vector<float> x(2 * (size_t)max_chunks * L, 0.2f), am(4 * 4096), iq(4 * 4096);
  int n_out = 0, cx = 0;
  // narrow band, overlapped: AM-Synch (its loop walks on the second stream) beside NFM with the ratio squelch, then an ingest ring
  pysdr_cfg cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  cfg.srate = 2.048e6; cfg.up = 3; cfg.down = 128; cfg.in_chunk = L; cfg.max_chunks = max_chunks; cfg.ntaps_dec = ntaps; cfg.ntaps_af = ntaps;
  pysdr_ctx* c = nullptr;
  STEP(pysdr_create(&cfg, &c));
  STEP(pysdr_set_overlap(c, 1));
  int irx = -1;
  STEP(pysdr_rx_add(c, PYSDR_AM_SYNCH, 100e3, h.data(), af.data(), 0.0, &irx));
  STEP(pysdr_rx_add(c, PYSDR_NFM, -50e3, h.data(), af.data(), 0.0, &irx));
  if (irx != 1) { std::fprintf(stderr, "second receiver got slot %d\n", irx); std::exit(1); }
  std::vector<float> lp(63, 1.0f / 63), hp(63, 0.f);
  STEP(pysdr_set_squelch_ratio(c, 1, 2.0f, lp.data(), hp.data(), 63));
  for (int k = 0; k < 3; ++k) STEP(pysdr_process_batch(c, x.data(), max_chunks, L, 0));
  STEP(pysdr_fetch(c, 0, am.data(), iq.data(), 4096, &n_out, &cx, nullptr, nullptr));
  pysdr_ingest* g = nullptr;
  STEP(pysdr_ingest_create_batched(c, 2, 1, &g));
  float* buf = nullptr;
  size_t cap = 0;
  STEP(pysdr_ingest_buffer(g, 0, &buf, &cap));
  for (size_t i = 0; i < 2 * (size_t)L; ++i) buf[i] = 0.1f;
  STEP(pysdr_ingest_submit(g, 0, L));
  pysdr_out outs[2];
  OK(pysdr_ingest_collect(g, 0, outs));
  pysdr_ingest_destroy(g);
  pysdr_destroy(c);
  // broadcast FM stereo, overlapped: the lazily allocated IF buffers, resampler, seeds
  int d1 = 0, up2 = 0, down2 = 0;
  OK(pysdr_wfm_params(cfg.srate, 48000.0, &d1, &up2, &down2));
  const auto res = taps(64 * up2);
  c = nullptr;
  STEP(pysdr_create(&cfg, &c));
  STEP(pysdr_set_overlap(c, 1));
  STEP(pysdr_rx_add(c, PYSDR_WFM2, 300e3, h.data(), af.data(), 0.0, &irx));
  OK(pysdr_set_wfm_taps(c, 0, h.data(), ntaps, res.data(), 64 * up2));
  for (int k = 0; k < 3; ++k) STEP(pysdr_process_batch(c, x.data(), max_chunks, L, 0));
  STEP(pysdr_fetch(c, 0, am.data(), iq.data(), 4096, &n_out, &cx, nullptr, nullptr));
  pysdr_destroy(c);
  // a spectrum on both paths (PYSDR_PSD_GROUP=4 below: 8 frames are dealt out over the side streams)
  std::vector<float> win(32768, 1.0f);
  pysdr_spectrum* sp = nullptr;
  void *d_x = nullptr, *d_o = nullptr;
  STEP(pysdr_spectrum_create(0, 32768, 65536, 8, win.data(), &sp));
  STEP(pysdr_dev_alloc(0, (size_t)8 * 32768 * 8, &d_x));
  STEP(pysdr_dev_alloc(0, (size_t)8 * 65536 * 4, &d_o));
  STEP(pysdr_spectrum_batch(sp, d_x, 8, 32768, d_o));
  pysdr_spectrum_destroy(sp);
  OK(pysdr_dev_free(0, d_x));
  OK(pysdr_dev_free(0, d_o));
  sp = nullptr;
  std::vector<float> xin(2 * 4096, 0.1f), out(2 * 4096);
  STEP(pysdr_spectrum_create(0, 4096, 8192, 2, win.data(), &sp));
  STEP(pysdr_spectrum_frame(sp, xin.data(), 1, 1, out.data(), &n_out));
  pysdr_spectrum_destroy(sp);
  // the four stream objects: create + one call + destroy of each
  pysdr_waterfall* w = nullptr;
  STEP(pysdr_waterfall_create(0, 64, 5, &w));
  STEP(pysdr_waterfall_push(w, xin.data(), 64, 0));
  STEP(pysdr_waterfall_image(w, 60.f, out.data(), nullptr, nullptr));
  pysdr_waterfall_destroy(w);
  pysdr_rtty* rt = nullptr;
  STEP(pysdr_rtty_create(0, 64, 5, 10, 30, 5, 50, 33, &rt));
  std::vector<int> codes(2 * 20), ndet(33);
  std::vector<long long> tt(2 * 20);
  std::vector<double> snr(2 * 20);
  int nd = 0;
  STEP(pysdr_rtty_decode(rt, xin.data(), 31, 0, 1, codes.data(), tt.data(), snr.data(), &nd, ndet.data(), nullptr, nullptr));
  pysdr_rtty_destroy(rt);
  pysdr_chan* ch = nullptr;
  STEP(pysdr_chan_create(0, 16, 4, 13, 5, 32, 400, &ch));
  OK(pysdr_chan_set_taps(ch, h.data(), 32));
  STEP(pysdr_chan_process(ch, xin.data(), 400, 0, out.data(), 128, 0, &nd));             // both lazy staging buffers
  if (nd != 100) { std::fprintf(stderr, "channelizer: %d outputs after the injected failure\n", nd); std::exit(1); }
  pysdr_bank* bk = nullptr;
  STEP(pysdr_bank_create(ch, 12000.0, PYSDR_NFM, 9, &bk));
  OK(pysdr_bank_set_mode(bk, PYSDR_NFM, h.data(), 9));
  STEP(pysdr_bank_process(bk, xin.data(), 400, 0, out.data(), 128, 0, &nd));
  pysdr_bank_destroy(bk);
  // the channelizer's other clients, and its second kind: create + one call + destroy of each
  const pysdr_cw_cfg ccfg = good_cw_cfg();
  std::vector<int32_t> counts(5 * 48);
  pysdr_cw* cw = nullptr;
  STEP(pysdr_cw_create(ch, &ccfg, 128, &cw));
  STEP(pysdr_cw_process(cw, xin.data(), 400, 0, &nd, counts.data(), nullptr, 0));
  pysdr_cw_destroy(cw);
  const pysdr_psk_cfg pcfg = good_psk_cfg();
  std::vector<float> ptw(2 * 32 * 12, 0.5f), pg(2 * 12, 0.1f);
  pysdr_psk* pk = nullptr;
  STEP(pysdr_psk_create(ch, 12, &pcfg, ptw.data(), pg.data(), 128, &pk));
  STEP(pysdr_psk_process(pk, xin.data(), 400, 0, &nd, counts.data(), nullptr, 0, nullptr, nullptr));
  pysdr_psk_destroy(pk);
  pysdr_chan_destroy(ch);
  pysdr_chan* fc = nullptr;
  STEP(pysdr_chan_fine_create(0, 16, 8, 16, 8, 5, 20, 32, 32, 400, &fc));
  OK(pysdr_chan_fine_set_taps(fc, h.data(), 32, h.data(), 32));
  STEP(pysdr_chan_process(fc, xin.data(), 400, 0, out.data(), 16, 0, &nd));              // the lazy staging buffers of both stages
  pysdr_chan_destroy(fc);
}

static void allocfail() {
  ScopedEnv on("PYSDR_TUNING", "1"), grp("PYSDR_PSD_GROUP", "4");
  for (long n = 1;; ++n) {
    fake_hip::State& f = fake_hip::state();
    f.creations = 0; f.fail_at = n; f.fail_hit = false;
    g_failed_steps = 0;
    allocfail_scenario();
    if (!f.fail_hit) {           // the scenario has fewer than n creations: every one of them has failed once
      f.fail_at = 0;
      std::printf("HOST_SAN_ALLOCFAIL_OK: %ld injected failures\n", n - 1);
      return;
    }
    if (g_failed_steps != 1) { std::fprintf(stderr, "creation %ld failed and %d steps reported it\n", n, g_failed_steps); std::exit(1); }
  }
}

static void race() {
  // one thread processes chunks, another turns the knobs (receiver.py RX thread vs the Qt thread)
  const Rate r = kRates[2];
  const int ntaps = 255;
  pysdr_ctx* c = make_ctx(r, 2, ntaps, ntaps);
  const auto h = taps(ntaps), af = taps(2 * ntaps);
  int irx = 0;
  OK(pysdr_rx_add(c, PYSDR_AM, -1000.0, h.data(), af.data(), 0.0, &irx));
  OK(pysdr_rx_add(c, PYSDR_NFM, 2000.0, h.data(), af.data(), 0.0, &irx));
  std::atomic<bool> stop{false};
  std::thread knobs([&] {
    int k = 0;
    while (!stop.load()) {
      double fa;
      OK(pysdr_set_lo(c, k & 1, -1000.0 - k, &fa));
      OK(pysdr_set_dec_taps(c, k & 1, h.data(), ntaps));
      OK(pysdr_set_mode(c, 0, (k & 2) ? PYSDR_AM_SYNCH : PYSDR_USB, af.data(), ntaps, 0.0));
      OK(pysdr_reset(c, 1, 3));
      OK(pysdr_set_agc(c, 0, k & 1, 0.5f));
      OK(pysdr_set_squelch(c, 1, (k & 1) ? 0.1f : 0.0f));
      pysdr_agc_state st;
      OK(pysdr_agc_get(c, 0, &st));
      ++k;
    }
  });
  std::vector<float> x(2 * (size_t)r.in_chunk * 2, 0.3f);
  const int cap = 2 * 1024 + 16;
  std::vector<float> am0(2 * cap), iq0(2 * cap), am1(2 * cap), iq1(2 * cap);
  for (int it = 0; it < 300; ++it) {
    pysdr_out outs[2] = {{am0.data(), iq0.data(), cap, 0, 0, 0.f}, {am1.data(), iq1.data(), cap, 0, 0, 0.f}};
    OK(pysdr_process(c, x.data(), (size_t)r.in_chunk - (it % 5), outs));
  }
  stop.store(true);
  knobs.join();
  pysdr_destroy(c);
  // the two stream objects that lock: one thread feeds the bank, another turns its knobs and waits on the borrowed channelizer
  pysdr_chan* ch = nullptr;
  OK(pysdr_chan_create(0, 16, 4, 13, 5, 32, 1024, &ch));
  OK(pysdr_chan_set_taps(ch, h.data(), 32));
  pysdr_bank* b = nullptr;
  OK(pysdr_bank_create(ch, 12000.0, PYSDR_NFM, 9, &b));
  OK(pysdr_bank_set_mode(b, PYSDR_NFM, h.data(), 9));
  stop.store(false);
  std::thread bank_knobs([&] {
    float g[5];
    uint8_t open[5];
    for (int k = 0; !stop.load(); ++k) {
      OK(pysdr_bank_set_agc(b, k & 1, 0.5f));
      OK(pysdr_bank_set_squelch(b, (k & 2) ? 0.1f : 0.0f));
      OK(pysdr_bank_state(b, nullptr, g, nullptr, nullptr, open));
      OK(pysdr_bank_sync(b));
      OK(pysdr_chan_sync(ch));
    }
  });
  std::vector<float> am(5 * 256);
  for (int it = 0; it < 300; ++it) {
    int nf = 0;
    OK(pysdr_bank_process(b, x.data(), 1024 - (it % 5), 0, am.data(), 256, 0, &nf));
  }
  stop.store(true);
  bank_knobs.join();
  pysdr_bank_destroy(b);
  // ... and a CW skimmer on the same channelizer: one thread feeds it, another reads its state and fetches rows
  const pysdr_cw_cfg cfg = good_cw_cfg();
  pysdr_cw* w = nullptr;
  OK(pysdr_cw_create(ch, &cfg, 256, &w));
  int32_t pl[8];
  OK(pysdr_cw_plan(5, 256, &cfg, pl));
  stop.store(false);
  std::thread cw_reader([&] {
    float pk[5];
    int32_t ints[5 * 8];
    std::vector<int32_t> ev(2 * (size_t)pl[4]);
    const int rows[] = {3, 4};
    while (!stop.load()) {
      OK(pysdr_cw_state(w, nullptr, pk, nullptr, ints));
      OK(pysdr_cw_fetch(w, rows, 2, ev.data(), pl[4]));
      OK(pysdr_cw_sync(w));
    }
  });
  std::vector<int32_t> counts(5);
  for (int it = 0; it < 300; ++it) {
    int nf = 0;
    OK(pysdr_cw_process(w, x.data(), 1024 - (it % 5), 0, &nf, counts.data(), nullptr, 0));
  }
  stop.store(true);
  cw_reader.join();
  pysdr_cw_destroy(w);
  pysdr_chan_destroy(ch);
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "race") == 0) {
    race();
    std::puts("HOST_SAN_RACE_OK");
    return 0;
  }
  if (argc > 1 && std::strcmp(argv[1], "allocfail") == 0) {
    allocfail();
    return 0;
  }
  if (argc > 1 && std::strcmp(argv[1], "objects") == 0) {
    stream_objects();
    channelizer_clients();
    return 0;
  }
  int ndev = 0;
  OK(pysdr_device_count(&ndev));
  FAILS(pysdr_create(nullptr, nullptr));
  FAILS(pysdr_set_overlap(nullptr, 1));
  planner_sweep();
  pll_plan_sweep();
  stream_objects();
  channelizer_clients();
  for (int pass = 0; pass < 3; ++pass) {
  g_overlap = pass == 0 ? 0 : (pass == 1 ? 2 : 1);
  for (const Rate& r : kRates) {
    if (r.fs == 10e6) continue;
    narrowband(r, 255);
  }
  narrowband(kRates[1], 1001);                       // the reference's default prototype at the am.py rate
  single_rx_long_prototype(kRates[1]);               // 3/128
  single_rx_long_prototype(kRates[4]);               // 3/64
  single_rx_long_prototype(Rate{2.56e6, 3, 160, 54613});
  single_rx_long_prototype(Rate{1.792e6, 3, 112, 38229});
  single_rx_long_prototype(Rate{1.536e6, 1, 32, 32768});   // 12-wave shapes: all 1001 taps in one branch
  single_rx_long_prototype(Rate{1.92e6, 1, 40, 40960});
  narrowband(kRates[0], 1001);
  {
    const int before = pysdr::g_mfma_launches;
    broadcast_fm();                                  // its 10 MS/s / 40 IF decimator is the second matrix-core shape
    const char* tun = getenv("PYSDR_TUNING");
    const char* off = getenv("PYSDR_MIXDEC_MFMA");
    const bool expect = !(tun && atoi(tun) > 0 && off && atoi(off) == 0);
    if ((pysdr::g_mfma_launches > before) != expect) { std::fprintf(stderr, "broadcast FM: matrix-core launches %d\n", pysdr::g_mfma_launches - before); return 1; }
  }
  mixed_modes_are_refused();
  spectrum();
  }
  std::puts("HOST_SAN_OK");
  return 0;
}
