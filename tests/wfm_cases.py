"""The case table of broadcast FM (modes WFM and WFM2): every resampler ratio of the receiver rates, every kernel of the
fs1 -> FS_OUT resampler (resamp_small.hip) that the ratio can reach, the tap lengths where its staging and its eligibility
change -- each on a list of ragged calls.

Which kernel a resampler runs is decided by its shape and the context's PYSDR_RESAMP_PLAIN alone (common.h: plan_resamp_small).
Every case names the kernels it is meant to reach; tests/test_wfm_cases.py asks the library (pysdr_resamp_plan: no GPU needed)
that it reaches exactly those, that every rate of the rate tables has a ratio case, that both tap-staging branches of the
one-output-per-thread kernel are reached and that every call list holds the calls named below; tests/test_gpu_wfm_sweep.py runs
every case and kernel against the float64 master of oracle/wfm_oracle.py.

One receiver, a 63-tap video filter (the IF decimator is not under test -- tests/front_end_cases.py -- and the oracle stays
fast), the carrier of synth_wfm at 0.12 fs, mono and stereo.

Ratio cases, 64 taps per branch as pysdr_amd.design makes them (production = the first kernel named):
  24/125 (2 MS/s, d1 8), 6/25 (3.2 MS/s), 16/75 (1.8 MS/s), 25/128 (6.144 MS/s: an odd UP, 13 waves, the last owns one branch):
      a wave per branch; one output per thread and a half-wave per branch on request
  3/16 (2.048 MS/s): a wave per branch; the half-wave form refuses it (its register prefetch holds 6 x 96 samples, the tile
      spans 580), so PYSDR_RESAMP_PLAIN = 1 and 2 both run one output per thread -- run once
  1/5 (1.92 MS/s; 2.16, 2.4 and 2.88 MS/s share it): UP = 1, both tiled forms refuse one branch: one output per thread IS the
      production kernel, with magic = 0
  24/125 at 0.25 MS/s: d1 = 1, the IF "decimator" is 1/1
  25/131 (2.01216 MS/s, no rate of the tables): the wave form's tile is 96 bytes too large, a half-wave per branch IS the
      production kernel
  24/125 with the launch held to three workgroups and a call of 12 chunks: every workgroup walks several tiles (the half-wave
      form's register prefetch of the NEXT tile)

Tap lengths k per branch (prototype UP * firwin(UP * k, 19.5 kHz, hamming, fs1 * UP), the oracle's resampler rebuilt from it):
  24/125 with k = 1, 16 (kpad 16), 17 (kpad 32), 40 (kpad 48: 256 % 48 != 0, the tap table is staged by the generic loop)
  1/5 with k = 40: the same staging branch with UP = 1
  25/128 with k = 176: the largest the wave form takes (kpad 176: 79 776 of its 79 872 bytes of LDS), k = 192: both tiled
      forms refuse, one output per thread is the production kernel (as the library's plan says: hand arithmetic confirmed)

Calls: front_end_cases.ragged_calls(L) and, behind it, calls worked out per case from d1, UP2 / DOWN2 and where the ragged list
left the stream (added_calls), until the list holds every one of PROPERTIES:
  n1_zero      no IF sample at all (impossible at d1 = 1, where every input sample is an IF sample: not asked of that case)
  short_silent 0 < n1 < hist_len IF samples (fewer than roll_history keeps, so old history survives the call) and no output
  one_out      exactly one audio output
  odd_start    outputs, the first of them at an odd absolute index
  long         more than two chunks
and a closing call of 24 outputs, so that no list ends on a call whose effect nothing shows (an IF history handed on wrongly by a
call without IF samples is one wrong discriminator sample in the NEXT call: it needs outputs behind it to be seen)."""
import contextlib
import ctypes as C
import os
from collections import namedtuple

import numpy as np
from scipy import signal

from oracle import sdr_oracle as so
from oracle import wfm_oracle as wo
from tests.front_end_cases import COND, TOL, ragged_calls, relerr  # noqa: F401  (the sweeps' bars and helpers, unchanged)

FS_OUT = 48e3
NTAPS_VIDEO = 63
VIDEO_BW = 200e3
CARRIER = 0.12                  # of fs
SEED = 57
WAVE, THREAD, HALF = 0, 1, 2    # pysdr_resamp_plan's kernel ids
KERNEL_NAMES = {WAVE: "wave", THREAD: "thread", HALF: "half"}
MODES = ("WFM", "WFM2")

# kernels: what PYSDR_RESAMP_PLAIN = 0, 1, 2 reach, duplicates dropped (the first is production); grid: PYSDR_MIXDEC_GRID;
# long_chunks: a call of that many chunks (+ 7 samples) behind the ragged list
Case = namedtuple("Case", "name fs k kernels grid long_chunks noise")


def _case(name, fs, k=64, kernels=(WAVE, THREAD, HALF), grid=0, long_chunks=0, noise=2e-3):
    return Case(name, fs, k, tuple(kernels), grid, long_chunks, noise)


RATIO_CASES = [
    _case("24_125", 2e6),
    _case("3_16", 2.048e6, kernels=(WAVE, THREAD)),
    _case("6_25", 3.2e6),
    _case("1_5", 1.92e6, kernels=(THREAD,)),
    _case("16_75", 1.8e6),
    _case("25_128", 6.144e6),
    _case("24_125-d1_1", 0.25e6),
]
# no receiver rate of the tables makes the half-wave form the production kernel (wherever it is eligible the wave form is too);
# 2.01216 MS/s (d1 8, IF 251.52 kHz) does: 64 x 131 input samples + the outputs of 64 x 25 are 96 bytes beyond the wave form's LDS
EXTRA_CASES = [_case("25_131", 2.01216e6, kernels=(HALF, THREAD))]
# (the ragged list's longest call is 2049 outputs: two tiles of the wave form, three of the half-wave form -- with three
# workgroups nobody would walk a second tile; the 12-chunk call is 8 and 16 tiles)
GRID_CASES = [_case("24_125-grid3", 2e6, grid=3, long_chunks=12)]
TAP_CASES = (
    [_case(f"24_125-k{k}", 2e6, k=k) for k in (1, 16, 17, 40)]
    + [_case("1_5-k40", 1.92e6, k=40, kernels=(THREAD,)),
       _case("25_128-k176", 6.144e6, k=176, kernels=(WAVE, THREAD)),
       _case("25_128-k192", 6.144e6, k=192, kernels=(THREAD,))]
)
CASES = RATIO_CASES + EXTRA_CASES + GRID_CASES + TAP_CASES
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

Shape = namedtuple("Shape", "d1 fs1 up2 down2 L")


def shape(case_or_fs):
    """(d1, fs1, UP2, DOWN2, chunk length) of a rate, from the oracle's own helpers."""
    fs = case_or_fs.fs if isinstance(case_or_fs, Case) else float(case_or_fs)
    d1 = wo.wfm_if_decim(fs)
    up2, down2 = so.up_dn(fs / d1, so.chunk_sizes(fs, FS_OUT)[2])
    return Shape(d1, fs / d1, up2, down2, so.chunk_sizes(fs, FS_OUT)[3])


def resamp_taps(case):
    """UP2 * firwin(UP2 * k, 19.5 kHz, hamming, fs1 * UP2): at k = 64 what pysdr_amd.design and the oracle make themselves."""
    s = shape(case)
    return s.up2 * signal.firwin(s.up2 * case.k, wo.WFM_RESAMP_CUT, window='hamming', fs=float(s.fs1) * s.up2)


# ---- what the library says ------------------------------------------------------------------------------------------
Plan = namedtuple("Plan", "eligible kernel threads lds tile_out kpad hist_len span")


def query(case_or_shape, plain=0):
    """pysdr_resamp_plan for a Case (or (up, down, ntaps))."""
    from pysdr_amd import _lib
    if isinstance(case_or_shape, Case):
        s = shape(case_or_shape)
        args = (s.up2, s.down2, s.up2 * case_or_shape.k)
    else:
        args = tuple(case_or_shape)
    out = (C.c_int32 * 8)()
    _lib.check(_lib.lib().pysdr_resamp_plan(*args, plain, out), "pysdr_resamp_plan")
    return Plan(bool(out[0]), *list(out)[1:])


def reachable(case):
    """[(plain, kernel)]: the kernels PYSDR_RESAMP_PLAIN = 0, 1, 2 reach, a kernel reached twice listed under its first request."""
    seen, out = set(), []
    for plain in (0, 1, 2):
        p = query(case, plain)
        assert p.eligible, (case.name, p)
        if p.kernel not in seen:
            seen.add(p.kernel)
            out.append((plain, p.kernel))
    return out


def plain_for(case, kernel):
    """The PYSDR_RESAMP_PLAIN that makes ``case`` run ``kernel`` (0 where production does)."""
    return {k: p for p, k in reachable(case)}[kernel]


def context_plan(ctx_handle, case):
    """(plan, grid) a live context runs ``case``'s resampler with: pysdr_resamp_plan under pysdr_get_resamp_tuning."""
    from pysdr_amd import _lib
    t = (C.c_int32 * 2)()
    _lib.check(_lib.lib().pysdr_get_resamp_tuning(ctx_handle, t), "pysdr_get_resamp_tuning")
    return query(case, t[0]), t[1]


# ---- the calls ------------------------------------------------------------------------------------------------------
PROPERTIES = ("n1_zero", "short_silent", "one_out", "odd_start", "long")
CLOSING_OUTPUTS = 24            # of the call that closes every list
CallCount = namedtuple("CallCount", "n n1 nout first")     # input samples, IF samples, audio outputs, absolute index of the first output


def _ceil_div(a, b):
    return -(-a // b)


def count_calls(calls, s, start=(0, 0, 0)):
    """What each call yields, by the arithmetic of both stages: output m of a stage exists once input sample
    floor(m DOWN / UP) does.  ``start`` = (input samples, IF samples, outputs) in front of the first call."""
    pos, i1, m = start
    out = []
    for n in calls:
        i1_new = _ceil_div(pos + n, s.d1)
        m_new = _ceil_div(i1_new * s.up2, s.down2)
        out.append(CallCount(n, i1_new - i1, m_new - m, m))
        pos, i1, m = pos + n, i1_new, m_new
    return out, (pos, i1, m)


def properties_of(c, s, hist_len):
    """Which of PROPERTIES one call has."""
    p = set()
    if c.n1 == 0:
        p.add("n1_zero")
    if 0 < c.n1 < hist_len and c.nout == 0:
        p.add("short_silent")
    if c.nout == 1:
        p.add("one_out")
    if c.nout > 0 and c.first % 2 == 1:
        p.add("odd_start")
    if c.n > 2 * s.L:
        p.add("long")
    return p


def wanted(s):
    return set(PROPERTIES) - ({"n1_zero"} if s.d1 == 1 else set())


def added_calls(s, hist_len, base=None):
    """The calls behind ragged_calls(L): while a property is missing, the SHORTEST next call (up to 8 IF samples' worth of
    input) that has a missing one; where the stream stands so that none has, one IF sample more and again."""
    base = ragged_calls(s.L) if base is None else base
    counts, state = count_calls(base, s)
    missing = wanted(s) - set().union(*(properties_of(c, s, hist_len) for c in counts))
    added = []
    while missing:
        assert len(added) < 16, (s, missing)
        for n in range(1, 8 * s.d1 + 1):
            (c,), st = count_calls([n], s, state)
            got = properties_of(c, s, hist_len) & missing
            if got:
                break
        else:
            n, got = s.d1, set()
            st = count_calls([n], s, state)[1]
        added.append(n)
        state = st
        missing -= got
    # the stream does not end on a call without output: what the short calls handed on (history, parity) shows in these
    return added + [_ceil_div(CLOSING_OUTPUTS * s.down2, s.up2) * s.d1]


def calls_of(case):
    s = shape(case)
    kpad = -(-case.k // 16) * 16
    base = ragged_calls(s.L) + ([case.long_chunks * s.L + 7] if case.long_chunks else [])
    return base + added_calls(s, kpad + 2, base)


# ---- the stream and the float64 master --------------------------------------------------------------------------------
def stream(case):
    x = wo.synth_wfm(case.fs, sum(calls_of(case)), SEED, f_carrier=CARRIER * case.fs, noise=case.noise)
    x.setflags(write=False)
    return x


def make_oracle(case, mode, dtype):
    o = wo.WfmReceiver(case.fs, FS_OUT, CARRIER * case.fs, stereo=(mode == 'WFM2'), ntaps_dec=NTAPS_VIDEO, video_bw=VIDEO_BW,
                       dtype=dtype)
    if case.k != wo.WFM_RESAMP_TAPS_PER_PHASE:
        o.audio = so.RationalDecimator(resamp_taps(case), o.up2, o.down2, dtype)
    return o


def run_oracle(case, mode, x, calls, dtype):
    """-> per call (iq, am) of the oracle in ``dtype`` (np.float64: the master), and per call the CallCount read off the oracle's
    own counters (its decimators' absolute sample counts and the lengths of what it returned)."""
    o = make_oracle(case, mode, dtype)
    per, counts, pos, m = [], [], 0, 0
    for n in calls:
        i1 = o.audio.n_abs
        am = o.demod_data(x[pos:pos + n])
        per.append((np.array(o.iq), np.array(am)))
        assert o.front.n_abs == pos + n and len(am) == len(o.iq)
        counts.append(CallCount(n, o.audio.n_abs - i1, len(o.iq), m))
        pos, m = pos + n, m + len(o.iq)
    return per, counts


def cat(per, which):
    return np.concatenate([p[which] for p in per])


# ---- a GPU context of a case ----------------------------------------------------------------------------------------------
@contextlib.contextmanager
def tuning_env(plain, grid):
    """PYSDR_RESAMP_PLAIN / PYSDR_MIXDEC_GRID for the contexts created inside (the library reads them at create)."""
    keys = ("PYSDR_TUNING", "PYSDR_RESAMP_PLAIN", "PYSDR_MIXDEC_GRID")
    old = {k: os.environ.get(k) for k in keys}
    try:
        for k in keys[1:]:
            os.environ.pop(k, None)
        if plain or grid:
            os.environ["PYSDR_TUNING"] = "1"
        if plain:
            os.environ["PYSDR_RESAMP_PLAIN"] = str(plain)
        if grid:
            os.environ["PYSDR_MIXDEC_GRID"] = str(grid)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make_gpu_receiver(case, mode, plain, overlap, max_call, grid=None):
    """-> (receiver, stream context) sized for a call of ``max_call`` samples; ``overlap`` as pysdr_set_overlap takes it;
    ``grid`` overrides the case's PYSDR_MIXDEC_GRID."""
    from pysdr_amd import _lib, sig_proc
    from pysdr_amd.params import RunTimeParams
    s = shape(case)
    with tuning_env(plain, case.grid if grid is None else grid):
        P = RunTimeParams(fs=case.fs, fc=[98.1e6], mode=mode, nfilt=NTAPS_VIDEO, foffset=CARRIER * case.fs, vid_bw=VIDEO_BW,
                          max_batch_chunks=-(-max_call // s.L), overlap_calls=False)
        g = sig_proc.Receiver(P, CARRIER * case.fs, 0, '1')
    if case.k != wo.WFM_RESAMP_TAPS_PER_PHASE:
        g.demod.wfm_resamp = resamp_taps(case)           # (pushed with the video filter in front of the first call)
    ctx = P._pysdr_stream
    _lib.check(_lib.lib().pysdr_set_overlap(ctx.h, overlap), "pysdr_set_overlap")
    return g, ctx
