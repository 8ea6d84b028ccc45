"""The case table of the channel bank's AF stage (bank_kernel<AM|NFM>, bank_cplx_kernel<BFO>, bank_finish of
pysdr_amd/csrc/bank.hip; plan in objects_plan.h): one raster, one stream, one list of calls -- run at every AF tap count
where the kernels' structure changes, in all five modes.  Test infrastructure only, pure NumPy.

What depends on the tap count T: the taps are padded to tp = roundup8(T) and walked in nstep = tp / 8 steps of eight, of
which nfull = T / 8 are whole and the last, where T is no multiple of 8, is guarded and takes T - 8 nfull taps; a row
keeps hpad = roundup8(T + 1) samples of history, which bank_finish moves with one thread per sample.  LENGTHS names each
edge; tests/test_bank_edge_cases.py checks those claims against the library's plan, proves on any machine that the
inputs make a bar of TOL against the float64 helper meaningful and that the cases see the errors they are there for;
tests/test_gpu_bank_edge_sweep.py runs them on the GPU.

The taps are not designed filters.  A designed low-pass is symmetric, so a kernel that walks the taps backwards passes,
and its tails are 1e-4 of its centre, so a tap of the guarded step dropped or misplaced passes too.  Here, seeded per
length: real modes (0.5 + U[0, 1)) / T -- all positive, AM's DC passes (zero-mean real taps cancel it and make AM
ill-conditioned) -- and complex modes N(0, 1) + j N(0, 1) over sum |c|; LSB gets the conjugate of USB's, CW its own.
They reach the bank through pysdr_bank_set_mode / pysdr_bank_set_mode_cplx with ntaps == T (``install``).

NFM got other taps than those: AM's, tap i times 1 + 8 exp(-i / 4), over their sum.  The carrier row's audio is a 1 kHz
tone at 25 kS/s, and 247 .. 255 near-equal taps span 9.9 .. 10.2 of its periods: they average the tone away, what is
left is the few per cent that the taps' randomness spares, and the plain bar on the carrier row is relative to that.
With the flat taps the float32 helper was 2.5e-6 from the float64 helper at T = 247 (1.7e-6 at 249, 4e-7 .. 2.5e-6
over six seeds per length): no room under COND.  The head passes the tone, the tail still weighs 2e-3 .. 5e-3 a tap.

The measures (the GPU sweep's and the conditioning test's alike), per call and row:
  AM            max |got - want| / the row's peak |want| in the call
  USB, LSB, CW  max |got - want| / scale, the ``scale`` of tests/bank_sideband_oracle.py
  NFM           tests.test_gpu_bank.nfm_compare: the excess over the rounding allowance on every row, and the plain bar
                on the carrier row from output 256 on
Measured, float32 helper against float64 helper on rows of the float64 polyphase model rounded to complex64, worst over
LENGTHS and over the calls (tests/test_bank_edge_cases.py prints one BANKEDGE line per length and mode and asserts COND =
2.5e-6 on each):
  AM 4.2e-07 (T = 254, 255)   NFM 4.9e-07 (T = 3)   USB 1.0e-07 (T = 15)   LSB 1.2e-07 (T = 15)   CW 1.1e-07 (T = 3)
and, AGC on, on the step case below 4.2e-07 of gain x peak.  The least any of the four wrong filters of that test is
away from the float64 helper: 7.4e-4 (LSB at T = 254, the first history sample lost), 74 TOL."""
import functools

import numpy as np

from tests import bank_oracle as bo
from tests import bank_sideband_oracle as sbo
from tests.front_end_cases import COND, TOL  # noqa: F401  (the sweep's bars, unchanged)

M, D, CHANNELS = 64, 32, (60, 12)      # 12 rows that wrap k = 0: k = 3 is a carrier (row 7), k = 2 and 4 its neighbours, the rest noise
assert (M, D) == bo.BASE[:2]
MODES = ("AM", "NFM", "USB", "LSB", "CW")
BFO = sbo.BFO
FRAMES = 4400
SEED = 160

# why each length is there
LENGTHS = (3,              # kBankTapsMin: one guarded step of 3; hpad 8
           7,              # one guarded step of 7, nfull 0; hpad 8 = T + 1: NFM's y[i - 2] reaches the first history sample
           8,              # one whole step, no guarded step; hpad 16
           9,              # a guarded step with left = 1: its t loop never runs
           15, 16, 17,     # hpad 16 = T + 1, then hpad 24; two whole steps; a third step of one tap
           247,            # a tail of 7; hpad 248 = T + 1
           248,            # 31 whole steps; hpad 256: every thread of bank_finish moves a sample
           249,            # 32 steps, the last of one tap
           254,            # an even length, a tail of 6
           255)            # the control: the everyday length (a tail of 7, hpad 256 = T + 1)
# what the comments above claim, per length: (taps_padded, history, whole steps, taps of the guarded step)
CLAIMS = {3: (8, 8, 0, 3), 7: (8, 8, 0, 7), 8: (8, 16, 1, 0), 9: (16, 16, 1, 1), 15: (16, 16, 1, 7), 16: (16, 24, 2, 0),
          17: (24, 24, 2, 1), 247: (248, 248, 30, 7), 248: (248, 256, 31, 0), 249: (256, 256, 31, 1), 254: (256, 256, 31, 6),
          255: (256, 256, 31, 7)}

# The calls, as outputs: one, three, none, five, nine (one more than a thread's eight), exactly one tile of the kernel -- the
# next call's windows then lie wholly in the history bank_finish moved --, a tile plus one full thread plus one output,
# seven, and the rest of the stream.
CALL_OUTPUTS = (1, 3, 0, 5, 9, 2048, 2057, 7)
TILE = 2048
# where in its frame each of those calls ends (sample e ends a call of cumulative count c where (c - 1) D < e <= c D):
# chosen so that every call has an odd number of samples
_ENDS_IN_FRAME = (7, 12, 13, 20, 9, 30, 3, 18)


def sample_cuts():
    """CALL_OUTPUTS and the rest of the stream as call lengths in samples, all odd"""
    cuts, end, done = [], 0, 0
    for k, r in zip(CALL_OUTPUTS, _ENDS_IN_FRAME):
        done += k
        e = (done - 1) * D + r
        cuts.append(e - end)
        end = e
    cuts.append(D * FRAMES - 1 - end)
    assert all(c % 2 == 1 for c in cuts)
    return cuts


def counts_of(cuts):
    s = np.cumsum([0] + list(cuts))
    return [int(-(-b // D) - -(-a // D)) for a, b in zip(s[:-1], s[1:])]


@functools.lru_cache(maxsize=None)
def case():
    """-> dict(fs, fs_out, M, D, channels, x complex64 (read-only), cuts, counts, rows, carrier_rows): bank_oracle.case of
    the base shape on the 12 channels, cut into the table's calls"""
    c = bo.case(M, D, CHANNELS, frames=FRAMES)
    x = c["x"][:D * FRAMES - 1].copy()
    x.setflags(write=False)
    cuts = sample_cuts()
    assert sum(cuts) == len(x)
    return dict(fs=c["fs"], fs_out=c["fs"] / D, M=M, D=D, channels=CHANNELS, x=x, cuts=cuts, counts=counts_of(cuts),
                rows=c["rows"], carrier_rows=c["carrier_rows"])


def model_rows(x):
    """the float64 polyphase model's rows of the table's channels on x, rounded to complex64: [12, frames]"""
    from pysdr_amd.design import channelizer_taps
    from tests import channelizer_oracle as co
    frames = -(-len(x) // D)
    y = co.polyphase(np.asarray(x, np.complex128), channelizer_taps(M), M, D, 0, frames, bo.rows_of(M, CHANNELS))
    return y.astype(np.complex64)


@functools.lru_cache(maxsize=None)
def model_rows_per_call():
    c = case()
    y = model_rows(c["x"])
    y.setflags(write=False)
    return y, bo.cut_rows(y, c["cuts"], D)


# ---- the taps ----------------------------------------------------------------------------------------------------------
def taps(T, mode):
    """float64 (AM, NFM) or complex128 (USB, LSB, CW) [T]: every tap matters, none mirrors another"""
    if mode in ("AM", "NFM"):
        rng = np.random.default_rng(SEED + T)
        c = (0.5 + rng.random(T)) / T
        if mode == "NFM":                     # a head that passes the carrier's tone (the module's docstring says why)
            c = c * (1.0 + 8.0 * np.exp(-np.arange(T) / 4.0))
            c = c / np.sum(c)
        return c
    rng = np.random.default_rng(SEED + (2000 if mode == "CW" else 1000) + T)
    c = rng.standard_normal(T) + 1j * rng.standard_normal(T)
    c = c / np.sum(np.abs(c))
    return np.conj(c) if mode == "LSB" else c


def install(bank, T, mode):
    """hand ``taps(T, mode)`` to a live bank through the raw ABI"""
    from pysdr_amd import _lib
    from pysdr_amd.tables import MODE_INDEX
    c = taps(T, mode)
    L = _lib.lib()
    if mode in ("AM", "NFM"):
        c = np.ascontiguousarray(c, np.float64)
        _lib.check(L.pysdr_bank_set_mode(bank._h, MODE_INDEX[mode], _lib.as_pd(c), T), "pysdr_bank_set_mode")
    else:
        re, im = np.ascontiguousarray(c.real), np.ascontiguousarray(c.imag)
        _lib.check(L.pysdr_bank_set_mode_cplx(bank._h, MODE_INDEX[mode], _lib.as_pd(re), _lib.as_pd(im), T, BFO),
                   "pysdr_bank_set_mode_cplx")
    bank.mode, bank.af = mode, c


# ---- the helper --------------------------------------------------------------------------------------------------------
def helper(T, mode, dtype, agc, c=None):
    """bank_sideband_oracle.SidebandOracle on the table's raster with the table's taps (or the taps c)"""
    k = case()
    return sbo.SidebandOracle(CHANNELS[1], k["fs_out"], taps(T, mode) if c is None else c, mode, bfo=BFO, agc=agc, dtype=dtype)


def run_helper(T, mode, dtype, rows_per_call, agc):
    """-> the helper's answer to every call: a list of the dicts of SidebandOracle.process"""
    o = helper(T, mode, dtype, agc)
    return [o.process(r) for r in rows_per_call]


# ---- the measures ------------------------------------------------------------------------------------------------------
def peak_error(got, want):
    """AM: per row, max |got - want| / the row's peak |want| (0 where both are silent)"""
    pk = np.max(np.abs(want), axis=1).astype(np.float64)
    d = np.max(np.abs(got.astype(np.float64) - want), axis=1)
    return np.where(pk > 0, d / np.where(pk > 0, pk, 1.0), np.where(d > 0, np.inf, 0.0))


def scale_error(got, want, scale):
    """USB, LSB, CW: per row, max |got - want| / scale"""
    d = np.max(np.abs(got.astype(np.float64) - want), axis=1)
    return np.where(scale > 0, d / np.where(scale > 0, scale, 1.0), np.where(d > 0, np.inf, 0.0))


def audio_error(mode, got, w):
    """the measure of ``mode`` (not NFM) on the helper's answer w, AGC off: got against w['a']"""
    return peak_error(got, w["a"]) if mode == "AM" else scale_error(got, w["a"], w["scale"])


class NfmJudge:
    """tests.test_gpu_bank.nfm_compare, unchanged, over the calls of a stream: ``o`` is the helper the allowance is taken
    from, ``y`` all rows of the stream"""

    def __init__(self, o, y, carrier_rows):
        self.o, self.y, self.c = o, y, dict(carrier_rows=carrier_rows)
        self.pk, self.first = [0.0] * y.shape[0], 0

    def __call__(self, got, want):
        from tests.test_gpu_bank import nfm_compare
        n = got.shape[1]
        worst = nfm_compare(self.c, self.o, self.y[:, :self.first + n], self.pk, got, want, self.first)
        self.first += n
        return worst


# ---- the AGC through a step down, silence and the return -----------------------------------------------------------------
AGC_T, AGC_CALLS, AGC_OUTPUTS = 9, 140, 4
AGC_DOWN, AGC_SILENT, AGC_BACK = 20, 40, 100       # first call 40 dB down, first all-zero call, first call back at full level


@functools.lru_cache(maxsize=None)
def agc_case():
    """AM at 9 taps, 140 calls of 4 outputs (odd lengths in samples): the whole input at full level for calls 0 .. 19,
    40 dB down (x 0.01: the carrier and everything beside it) for 20 .. 39, all-zero for 40 .. 99, at full level again
    from call 100.  -> dict(x, cuts, level per call)"""
    ends = [(AGC_OUTPUTS * (j + 1) - 1) * D + (7 if j % 2 == 0 else 12) for j in range(AGC_CALLS)]
    cuts = list(np.diff([0] + ends))
    assert all(c % 2 == 1 for c in cuts) and counts_of(cuts) == [AGC_OUTPUTS] * AGC_CALLS
    level = np.ones(AGC_CALLS)
    level[AGC_DOWN:AGC_SILENT], level[AGC_SILENT:AGC_BACK] = 0.01, 0.0
    x = case()["x"][:ends[-1]].copy()
    for j, (a, b) in enumerate(zip([0] + ends[:-1], ends)):
        x[a:b] *= np.float32(level[j])
    assert not x[ends[AGC_SILENT - 1]:ends[AGC_BACK - 1]].any()
    x.setflags(write=False)
    return dict(x=x, cuts=[int(c) for c in cuts], level=level)


def agc_conditions(w32):
    """What the step case is there for, asserted on the float32 helper's answers (one dict per call): conditions on the
    input, not measurements.  The carrier row never reaches the clamp (its smoothed peak decays by 0.9 a call, 60 calls
    are 1.8e-3): it runs the unclamped decay through the whole silence.  Every other row sits at exactly 1e4 for ten
    calls and more, up to the last silent call.  The first call after the return holds four outputs of a prototype of
    16 frames that has only begun to fill: the rows next to the carrier leave the clamp in that very call, the three
    farthest from it one call later.  -> the rows that ran the clamp"""
    carrier = case()["carrier_rows"]
    top = np.float32(1e4)
    gain = np.array([w["agc_gain"] for w in w32])                       # [call, row]
    clamped = (gain[AGC_SILENT:AGC_BACK] == top).sum(axis=0)
    rows = np.flatnonzero(clamped >= 10)
    assert sorted(set(rows) | set(carrier)) == list(range(gain.shape[1])) and not clamped[carrier].any(), clamped
    assert (gain[AGC_BACK - 1, rows] == top).all()
    assert (gain[AGC_BACK, rows] < top).sum() >= 6, gain[AGC_BACK]       # the attack out of the clamp, in the call of the return
    assert (gain[AGC_BACK + 1] < top).all() and (gain[AGC_BACK + 1] < gain[AGC_BACK]).all()
    assert (gain[AGC_SILENT - 1, carrier] > 4 * gain[AGC_DOWN - 1, carrier]).all()      # the step down raised the carrier's gain
    flushed = [j for j in range(AGC_SILENT, AGC_BACK) if not w32[j]["maxbuf"].any()]
    assert len(flushed) >= 40 and flushed == list(range(flushed[0], AGC_BACK))
    for j in flushed:                                                    # the all-zero calls, once the prototype has flushed
        assert not w32[j]["am"].any() and not w32[j]["a"].any()
    return rows
