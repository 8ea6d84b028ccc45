"""The channel bank's complex-tap modes USB / LSB / CW on the GPU (bank_cplx_kernel of pysdr_amd/csrc/bank.hip,
DESIGN.md 3 item 17) against the oracle's demodulator and AGC (tests/bank_sideband_oracle.py).  As in
tests/test_gpu_bank.py the oracle side is fed the rows of an independent Channelizer on the same input, and that the
bank's rows are those rows is asserted first.

The bar is |am - want| <= TOL * gain * scale on every sample, scale = max |y| over what the call's AF windows hold
(bank_sideband_oracle.py says why the call's own peak is no measure in these modes).  float32 helper against float64
helper on that measure: 8.4e-7 (USB), 6.8e-7 (LSB), 1.9e-7 (CW) at 255 taps (tests/test_bank_sideband.py asserts
1e-6 on the start of the case), so two legitimate float32 summation orders fit under TOL = 1e-5 with room."""
import functools

import numpy as np
import pytest

from tests import bank_oracle as bo
from tests import bank_sideband_oracle as sbo
from tests.test_gpu_bank import cbits, fbits, nfm_compare, rel, shared
from tests.test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

SHAPES = [0, 1, 2]                       # bo.SHAPES[:3]: 255 taps (31 steps + a tail of 7), 125 (tail of 5), 64 (whole steps)
IDS = [f"{bo.SHAPES[i][0]}-{bo.SHAPES[i][1]}" for i in SHAPES]


def make_bank(c, mode, **kw):
    from pysdr_amd.bank import SidebandBank
    return SidebandBank(c["fs"], c["M"], c["D"], channels=c["channels"], mode=mode, af_bw=sbo.AF_BW[mode], ntaps_af=c["T"],
                        max_in=len(c["x"]), bfo=sbo.BFO, **kw)


@functools.lru_cache(maxsize=None)
def oracle_run(i, mode, agc, ncalls=None):
    """the float32 helper's answers to the first ncalls calls of case i (all: None)"""
    c = shared(i)
    o = sbo.SidebandOracle(len(c["rows"]), c["fs_out"], sbo.taps(mode, c["fs_out"], c["T"]), mode, agc=agc)
    return [o.process(r) for r in c["yc"][:ncalls]]


@pytest.mark.parametrize("i", SHAPES, ids=IDS)
@pytest.mark.parametrize("mode", ["USB", "LSB", "CW"])
def test_parity_agc_off(i, mode):
    c = shared(i)
    ncalls = 6 if (mode == "LSB" and i != 0) else None             # LSB is USB's kernel with other taps: full depth at the base shape
    want = oracle_run(i, mode, False, ncalls)
    b = make_bank(c, mode, agc=False)
    assert b.mode == mode and np.max(np.abs(b.af - sbo.taps(mode, c["fs_out"], c["T"]))) <= 1e-12
    nk, worst, seen = len(c["rows"]), 0.0, set()
    for x, y, w in zip(c["calls"], c["yc"], want):
        am = b.push(x)
        assert am.shape == w["am"].shape and am.dtype == np.float32
        seen.add(y.shape[1])
        if y.shape[1] == 0:
            continue
        assert np.array_equal(cbits(b.iq()), cbits(y))                    # the bank's rows are the channelizer's
        e = np.max(np.abs(am - w["am"]), axis=1) / w["scale"]
        worst = max(worst, float(e.max()))
        assert e.max() <= TOL, (y.shape, int(e.argmax()), float(e.max()))
        st = b.state()
        assert np.array_equal(st["gain"], np.ones(nk, np.float32)) and st["open"].all()
    assert {0, 1, 3} <= seen and (ncalls is not None or i != 0 or bo.BIG in seen)
    print(f"{mode} M {c['M']} D {c['D']} T {c['T']}, AGC off: worst |am - want| / scale {worst:.2e}")
    b.close()


@pytest.mark.parametrize("mode", ["USB", "CW"])
def test_parity_agc_on(mode):
    c = shared(0)
    want = oracle_run(0, mode, True)
    b = make_bank(c, mode)
    assert b.agc is True
    worst, worst_state = 0.0, 0.0
    for x, y, w in zip(c["calls"], c["yc"], want):
        am = b.push(x)
        if y.shape[1] == 0:
            continue
        st = b.state()
        for k, wk in (("agc", "agc"), ("gain", "agc_gain"), ("maxbuf", "maxbuf")):
            worst_state = max(worst_state, float(rel(st[k], w[wk]).max()))
            assert rel(st[k], w[wk]).max() <= 1e-5, (k, y.shape, float(rel(st[k], w[wk]).max()))
        e = np.max(np.abs(am - w["am"]), axis=1) / (w["gain"].astype(np.float64) * w["scale"])
        worst = max(worst, float(e.max()))
        assert e.max() <= TOL, (y.shape, int(e.argmax()), float(e.max()))
        assert st["open"].all() and (w["gain"] != 1).any()
    print(f"{mode} AGC on: worst |am - want| / (gain scale) {worst:.2e}, worst state {worst_state:.2e}")
    b.close()


@pytest.mark.parametrize("mode", ["USB", "CW"])
def test_any_cut_gives_the_same_audio(mode):
    """The whole stream in one call against the case's cuts -- calls of 1, 3 and 0 outputs first, one of 2100: in CW the
    BFO phase follows the absolute output index, not the call -- and the same bits again after reset()."""
    c = shared(0)
    b = make_bank(c, mode, agc=False)
    one = b.push(c["x"])
    assert one.shape == (b.nk, c["y"].shape[1]) and np.isfinite(one).all() and np.abs(one).max() > 0
    for _ in range(2):
        b.reset()
        parts = [b.push(p) for p in c["calls"]]
        assert [p.shape[1] for p in parts] == [r.shape[1] for r in c["yc"]]
        assert np.array_equal(fbits(np.concatenate(parts, axis=1)), fbits(one))
    b.close()


def test_mode_switches_hold_for_the_whole_window():
    """NFM -> USB -> CW -> AM at call boundaries, the helper switched alike: each call is within its mode's bar from its
    first output, so the new mode owns the whole AF window (the row history is y, which no mode changes)."""
    c = shared(0)
    D, T, nk = c["D"], c["T"], len(c["rows"])
    edges = [0, 600, 1000, 1400, 1800]
    modes = ["NFM", "USB", "CW", "AM"]
    b = make_bank(c, "NFM")
    o = sbo.SidebandOracle(nk, c["fs_out"], sbo.taps("NFM", c["fs_out"], T), "NFM")
    pk = [0.0] * nk
    for j, mode in enumerate(modes):
        m0, m1 = edges[j], edges[j + 1]
        if j:
            b.set_mode(mode, af_bw=sbo.AF_BW[mode])
            o.set_mode(mode, sbo.taps(mode, c["fs_out"], T))
            assert b.mode == mode and b.af_bw == sbo.AF_BW[mode]
        am, w = b.push(c["x"][m0 * D:m1 * D]), o.process(c["y"][:, m0:m1])
        assert np.array_equal(cbits(b.iq()), cbits(c["y"][:, m0:m1]))
        st = b.state()
        if mode == "NFM":
            nfm_compare(c, o, c["y"][:, :m1], pk, am, w["am"], m0)
            assert np.array_equal(st["gain"], np.ones(nk, np.float32))
            continue
        for k, wk in (("agc", "agc"), ("gain", "agc_gain"), ("maxbuf", "maxbuf")):
            assert rel(st[k], w[wk]).max() <= 1e-5, (mode, k, float(rel(st[k], w[wk]).max()))
        if mode == "AM":
            e = np.max(np.abs(am - w["am"]), axis=1) / np.max(np.abs(w["am"]), axis=1)
        else:
            e = np.max(np.abs(am - w["am"]), axis=1) / (w["gain"].astype(np.float64) * w["scale"])
        assert e.max() <= TOL, (mode, int(e.argmax()), float(e.max()))
    b.close()


def test_squelch_is_inert():
    c = shared(0)
    nk = len(c["rows"])
    a, z, p = make_bank(c, "USB", squelch=bo.SQUELCH), make_bank(c, "USB", squelch=0.0), make_bank(c, "USB", squelch=bo.SQUELCH)
    assert a.squelch == bo.SQUELCH
    for x, y in zip(c["calls"][:6], c["yc"][:6]):
        am = a.push(x)
        assert np.array_equal(fbits(am), fbits(z.push(x)))
        rows, am_open = p.push_open(x)
        assert np.array_equal(rows, np.arange(nk)) and am_open.shape == am.shape
        assert np.array_equal(fbits(am_open), fbits(am))
        st = a.state()
        assert st["open"].all() and np.array_equal(st["level"], np.zeros(nk, np.float32))
    for v in (a, z, p):
        v.close()


def test_one_nan_frame_marks_exactly_the_windows_that_reach_it():
    """One input frame of NaN, AGC off, USB, 125 taps: an output is not finite exactly where its AF window d[m - T + 1 .. m]
    holds a row sample that is not finite (the rows of a channelizer on the same input say which), and once the window
    has passed every call is the clean run's, bit for bit."""
    from pysdr_amd.channelizer import Channelizer
    i = 1
    c = shared(i)
    D, T, nk = c["D"], c["T"], len(c["rows"])
    assert T == 125
    x = c["x"][:1500 * D].copy()
    x[420 * D + 3:421 * D + 3] = complex(np.nan, 0.25)
    cuts = [400 * D, 100 * D + 3, 300 * D - 3, 350 * D, 350 * D]
    ch = Channelizer(c["fs"], c["M"], D, max_in=len(x))
    y = ch.push(x)
    ch.close()
    bad_y = ~np.isfinite(y)
    assert bad_y.any() and not bad_y[:, :400].any() and not bad_y[:, 500:].any()
    # dilate by the window: output m is bad where any of y[m - T + 1 .. m] is
    csum = np.concatenate((np.zeros((nk, T), np.int64), np.cumsum(bad_y, axis=1)), axis=1)
    bad = (csum[:, T:] - csum[:, :-T]) > 0
    b, clean = make_bank(c, "USB", agc=False), make_bank(c, "USB", agc=False)
    for j, (p, pc, wb) in enumerate(zip(bo.split(x, cuts), bo.split(c["x"][:len(x)], cuts), bo.cut_rows(bad, cuts, D))):
        am, ref = b.push(p), clean.push(pc)
        assert np.array_equal(~np.isfinite(am), wb), j
        assert np.array_equal(b.state()["gain"], np.ones(nk, np.float32))
        if j == 0:
            assert not wb.any() and np.array_equal(fbits(am), fbits(ref))
        elif j == 1:
            assert wb.any() and not wb.all()
            assert np.array_equal(fbits(am[~wb]), fbits(ref[~wb]))          # nothing outside the windows is touched
        elif j >= 3:
            assert not wb.any() and np.array_equal(fbits(am), fbits(ref))
    b.close()
    clean.close()


def test_errors_leave_the_object_usable():
    from pysdr_amd import _lib
    from pysdr_amd.bank import SidebandBank
    c = shared(0)
    D = c["D"]
    x = np.array(c["x"][:200 * D])
    L = _lib.lib()
    b = make_bank(c, "USB", agc=False)
    want = b.push(x)
    b.reset()
    t = sbo.taps("CW", c["fs_out"], 255)
    re, im = np.ascontiguousarray(t.real), np.ascontiguousarray(t.imag)
    pr, pi = _lib.as_pd(re), _lib.as_pd(im)
    assert L.pysdr_bank_set_mode_cplx(b._h, 5, pr, pi, 254, 700.0) == -1                   # wrong tap count
    assert L.pysdr_bank_set_mode_cplx(b._h, 5, None, pi, 255, 700.0) == -1
    assert L.pysdr_bank_set_mode_cplx(b._h, 5, pr, None, 255, 700.0) == -1
    assert L.pysdr_bank_set_mode_cplx(None, 5, pr, pi, 255, 700.0) == -1
    for mode in (0, 9, 2, 6, 1, 10, 11, -1):                                               # AM, NFM, SSB, IQ, AM-Synch, RTTY, ...
        assert L.pysdr_bank_set_mode_cplx(b._h, mode, pr, pi, 255, 700.0) == -1, mode
    assert L.pysdr_bank_set_mode(b._h, 3, pr, 255) == -1                                   # real taps cannot say USB
    with pytest.raises(_lib.PysdrError):
        b.set_mode("IQ")
    with pytest.raises(_lib.PysdrError):
        SidebandBank(c["fs"], c["M"], D, mode="IQ")
    with pytest.raises(_lib.PysdrError):
        SidebandBank(c["fs"], c["M"], D, mode="USB", ntaps_af=2)
    assert b.mode == "USB"
    assert np.array_equal(fbits(b.push(x)), fbits(want))                  # nothing above advanced the stream or changed the mode
    b.close()
