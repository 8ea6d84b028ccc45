"""The case table of the audio-rate tail (demod_fir_kernel and its epilogue, stage2.hip): one context, seven sub-receivers,
one stream -- run at every AF filter length where the kernel's structure changes.

The AF filter length is a creation-time parameter (Cfg.ntaps_af, RunTimeParams(af_filt_len=)); pysdr_create accepts 1 .. 2048.
What depends on it: the taps are padded to groups of 12 (H) and walked three 4-tap blocks per loop trip, odd outputs read a copy
of the taps shifted by one whose tap H is a pad, the staged image and the squelch's indices are anchored on H, and the history
kept in front of a call is hy = roundup16(roundup8(ntaps) + 5).  LENGTHS names each edge; tests/test_af_stage_cases.py proves on
any machine that the signals make the bar meaningful, tests/test_gpu_af_stage_sweep.py runs them on the GPU.

The front end is not under test: 2.048 MS/s (3/128, 1023.98 outputs per chunk) with a 63-tap prototype, which keeps the CPU
oracle fast.  One carrier per sub-receiver at the first seven offsets of tests/front_end_cases.py.  Which signal each mode got,
and which form of the kernel it reaches:

  AM        'am' tone at depth 0.5                              kDetAbs   kFirRealReal   demod_fir_kernel<false>
  NFM       'fm', 3 kHz deviation, video_bw 20 kHz              kDetFm    kFirRealReal   demod_fir_kernel<false>
  AM-Synch  'am' at depth 0.5, the receiver 7 Hz off tune       kDetPll   kFirRealReal   demod_fir_kernel<false>  (from ypll)
  USB       'usb' two tones above the carrier                   kDetNone  kFirRePart     demod_fir_kernel<false>
  LSB       'usb' two tones, the receiver 3 kHz ABOVE them      kDetNone  kFirRePart     demod_fir_kernel<false>
  CW        a STEADY carrier ('am', depth 0), bfo 700, 500 Hz   kDetBfo   kFirRePart     demod_fir_kernel<false>
  IQ        'am' at depth 0.5, the receiver 1 kHz below it      kDetNone  kFirCplx       demod_fir_kernel<true>

CW is not keyed: a carrier keyed at 40 Hz in the company of six others leaves calls with the key up, whose peak is the other
carriers' leakage -- the float32 mirror was 4e-6 .. 1.2e-5 of THAT away from the master (the same sub-receiver alone: 4.3e-7).
With both kinds of output in one context both launches and the grouping of sub-receivers (fir_rx) run in every case."""
import numpy as np

from oracle import sdr_oracle as so
from tests import front_end_cases as fc
from tests.front_end_cases import COND, TOL, ragged_calls, relerr  # noqa: F401  (the sweep's bars and helpers, unchanged)

FS = 2.048e6
NTAPS_DEC = 63
SEED = 57
MODES = ("AM", "NFM", "AM-Synch", "USB", "LSB", "CW", "IQ")
PLL_START = 1024          # outputs of a stream over which AM-Synch is not compared (the project's exemption: tests/test_gpu_pll.py)

# why each length is there
LENGTHS = (1, 2, 3,        # one tap; two lengths the oracle could not run; the smallest it could
           8, 9,           # hy 16 -> 32
           11, 12, 13,     # the end, the exact fill and the start of a tap group: one and two loop trips, the pad tap H
           23, 24, 25,     # two and three trips; hy 32 -> 48
           35, 36, 37,     # all three register rotations used once; four trips
           40, 41,         # hy 48 -> 64
           48, 49,         # H 48 -> 60: the ratio squelch's bound for its designed 63 taps
           60, 61,         # exact fill and the start of the next group, near kSqTapsMax
           254, 255)       # even, one below the everyday length; the control


def _f(i):
    return round(fc._OFFSETS[i] * FS / 1e3) * 1e3 + 100.0 * i


def _amp(i):
    return 0.12 + 0.02 * ((3 * i) % 8)


def make_cfg():
    tone = [500.0 + 150.0 * i for i in range(7)]
    carriers = [dict(f=_f(0), kind='am', amp=_amp(0), tone=tone[0], depth=0.5),
                dict(f=_f(1), kind='fm', amp=_amp(1), tone=tone[1], dev=3000.0),
                dict(f=_f(2), kind='am', amp=_amp(2), tone=tone[2], depth=0.5),
                dict(f=_f(3), kind='usb', amp=_amp(3), tone=tone[3]),
                dict(f=_f(4), kind='usb', amp=_amp(4), tone=tone[4]),
                dict(f=_f(5), kind='am', amp=_amp(5), tone=tone[5], depth=0.0),
                dict(f=_f(6), kind='am', amp=_amp(6), tone=tone[6], depth=0.5)]
    rx = [dict(frq=_f(0), mode='AM', video_bw=10e3, af_bw=5e3),
          dict(frq=_f(1), mode='NFM', video_bw=20e3, af_bw=4e3),
          dict(frq=_f(2) - 7.0, mode='AM-Synch', video_bw=10e3, af_bw=5e3),
          dict(frq=_f(3), mode='USB', video_bw=10e3, af_bw=3e3),
          dict(frq=_f(4) + 3000.0, mode='LSB', video_bw=10e3, af_bw=3e3),
          dict(frq=_f(5), mode='CW', video_bw=10e3, af_bw=500.0, bfo=700.0),
          dict(frq=_f(6) - 1000.0, mode='IQ', video_bw=10e3, af_bw=5e3)]
    return dict(fs=FS, fs_out=fc.FS_OUT, ntaps_dec=NTAPS_DEC, noise=2e-3, carriers=carriers, rx=rx)


CFG = make_cfg()
assert tuple(r['mode'] for r in CFG['rx']) == MODES
L = so.chunk_sizes(FS, fc.FS_OUT)[3]
assert L == 43690
# The front end's ragged list, and four calls behind it.  At 3/128 the list alone yields 1024, 1024, 24, 0, 1024, 2048 and 8
# outputs: a call without output, but only even counts (every call starts at an even absolute output, par = 0), none above one
# workgroup tile of 2048 and none below 8.  The calls added give 7 outputs (the stream turns odd), 2050 from an odd start (par = 1
# across a tile boundary), a whole chunk from an odd start, and 3.  tests/test_af_stage_cases.py asserts all of this.
CALLS = ragged_calls(L) + [300, 2 * L + 100, L, 130]

_stream = None


def stream():
    """The one stream of the table (made once, never written to)."""
    global _stream
    if _stream is None:
        _stream = so.synth_iq(CFG, sum(CALLS), SEED)
        _stream.setflags(write=False)
    return _stream


def run_oracle(ntaps_af, dtype):
    """-> per sub-receiver, per call of CALLS: (iq, am) of the oracle in ``dtype`` with an AF filter of ``ntaps_af`` taps."""
    return fc.run_oracle(CFG, stream(), CALLS, dtype, ntaps_af=ntaps_af)


def call_starts(per_call):
    """First output index of every call of one sub-receiver's list of (iq, am)."""
    return np.r_[0, np.cumsum([len(iq) for iq, _ in per_call])][:-1]


def behind_pll_start(a, first):
    """The part of a call's outputs ``a`` (the call starts at output ``first`` of the stream) that AM-Synch is compared on."""
    return a[max(0, PLL_START - int(first)):]


# ---- the squelch cases: NFM sub-receivers alone on the same rate ---------------------------------------------------------------
def squelch_cfg(nrx=1):
    carriers = [dict(f=_f(i), kind='fm', amp=0.3 - 0.05 * i, tone=1000.0 - 300.0 * i, dev=3000.0 - 500.0 * i) for i in range(nrx)]
    rx = [dict(frq=_f(i), mode='NFM', video_bw=20e3, af_bw=4e3) for i in range(nrx)]
    return dict(fs=FS, fs_out=fc.FS_OUT, ntaps_dec=NTAPS_DEC, noise=2e-3, carriers=carriers, rx=rx)


RATIO_LENGTHS = (1, 12, 13, 40, 41, 48, 49)
RATIO_CHUNKS = 10         # chunks of the accepted run (carriers off the air for chunks 4 .. 6); one more follows the refused call
_ratio_cases = {}


def ratio_case(ntaps_af):
    """The ratio squelch beside an AF filter of ``ntaps_af`` taps, with squelch filters of exactly the bound's length: two NFM
    sub-receivers (the squelch is armed on the first), seeded random taps -- every tap matters, unlike a designed filter's tails --
    and a threshold that the oracle's sq1 / sq2 crosses when the carriers go and come: the middle of the widest gap between two
    chunks' ratios (the envelopes do not depend on the threshold).  -> dict(cfg, x, K, lp, hp, lp1, hp1 (one tap more), thr, ratios)."""
    if ntaps_af not in _ratio_cases:
        cfg = squelch_cfg(2)
        x = squelch_stream(cfg, RATIO_CHUNKS + 1, (4, 6))
        K = so.sq_ratio_taps_bound(ntaps_af)
        rng = np.random.default_rng(100 + ntaps_af)
        lp, hp, lp1, hp1 = [(rng.standard_normal(n) / np.sqrt(n)).astype(np.float32) for n in (K, K, K + 1, K + 1)]
        o = so.make_receivers(cfg, np.float32, ntaps_af=ntaps_af)[0]
        o._sq_taps = (lp, hp)
        o.squelch_ratio = np.float32(1.0)
        ratios = []
        for k in range(RATIO_CHUNKS + 1):
            o.demod_data(x[k * L:(k + 1) * L])
            ratios.append(float(o.sq_lp) / float(o.sq_hp))
        s = np.sort(ratios[:RATIO_CHUNKS])
        j = int(np.argmax(s[1:] / s[:-1]))                 # the widest gap between two chunks' ratios: the threshold in its middle
        thr = float(np.float32(np.sqrt(s[j] * s[j + 1])))
        x.setflags(write=False)
        _ratio_cases[ntaps_af] = dict(cfg=cfg, x=x, K=K, lp=lp, hp=hp, lp1=lp1, hp1=hp1, thr=thr, ratios=ratios)
    return _ratio_cases[ntaps_af]


def squelch_stream(cfg, nchunks, off, seed=14):
    """``nchunks`` chunks of ``cfg``'s stream; the carriers are off the air (noise alone) for the chunks ``off`` = (first, last)."""
    x = so.synth_iq(cfg, nchunks * L, seed)
    quiet = so.synth_iq(dict(cfg, carriers=[]), nchunks * L, seed + 1)
    a, b = off[0] * L, (off[1] + 1) * L
    x[a:b] = quiet[a:b]
    return x
