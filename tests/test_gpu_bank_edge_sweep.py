"""The channel bank on the GPU at every AF tap count where its kernels' structure changes (tests/bank_edge_cases.py), in
AM, NFM, USB, LSB and CW, with taps that are no designed filter, against the FLOAT64 form of the helper
(tests/bank_sideband_oracle.py).  As in tests/test_gpu_bank.py the helper is fed the rows of an independent Channelizer
of the same shape on the same input, and that the bank's rows are those rows is asserted first: only the bank's own
arithmetic is judged.  tests/test_bank_edge_cases.py shows on any machine that the helper's float32 form is within
TOL / 4 of its float64 form on these inputs, and that a filter walked backwards, a dropped or misplaced last tap and a
lost history sample are at least 10 TOL away.

Every bar is one the project already holds: TOL on the audio, 1e-5 relative on the AGC state."""
import functools

import numpy as np
import pytest

from tests import bank_edge_cases as ec
from tests import bank_oracle as bo
from tests.test_gpu_bank import cbits, fbits, rel

pytestmark = pytest.mark.gpu

TOL = ec.TOL
STATE = (("agc", "agc"), ("gain", "agc_gain"), ("maxbuf", "maxbuf"))


def channelizer_rows(x):
    from pysdr_amd.channelizer import Channelizer
    c = ec.case()
    ch = Channelizer(c["fs"], ec.M, ec.D, channels=ec.CHANNELS, max_in=len(x))
    y = ch.push(x)
    ch.close()
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def shared():
    """the table's case with the rows of an independent channelizer, cut into calls; computed once, never changed"""
    c = dict(ec.case())
    c["y"] = channelizer_rows(c["x"])
    c["calls"], c["yc"] = bo.split(c["x"], c["cuts"]), bo.cut_rows(c["y"], c["cuts"], ec.D)
    assert [r.shape[1] for r in c["yc"]] == c["counts"]
    return c


@functools.lru_cache(maxsize=None)
def master(T, mode, agc):
    """the float64 helper's answers to every call of the table (read only)"""
    return ec.run_helper(T, mode, np.float64, shared()["yc"], agc)


@functools.lru_cache(maxsize=None)
def mirror(T, mode, agc):
    """the float32 helper's: what the AGC state is held to"""
    return ec.run_helper(T, mode, np.float32, shared()["yc"], agc)


def make_bank(T, mode, agc, n_in):
    """a SidebandBank of T taps whose taps are the table's, handed over through the raw ABI"""
    from pysdr_amd.bank import SidebandBank
    c = ec.case()
    b = SidebandBank(c["fs"], ec.M, ec.D, channels=ec.CHANNELS, mode="AM", af_bw=0.0, ntaps_af=T, max_in=n_in, bfo=ec.BFO, agc=agc)
    ec.install(b, T, mode)
    return b


@pytest.mark.parametrize("mode", ec.MODES)
@pytest.mark.parametrize("T", ec.LENGTHS)
def test_every_sample_against_the_float64_master(T, mode):
    c = shared()
    want = master(T, mode, False)
    b = make_bank(T, mode, False, len(c["x"]))
    nk, worst = len(c["rows"]), 0.0
    judge = ec.NfmJudge(ec.helper(T, mode, np.float64, False), c["y"], c["carrier_rows"]) if mode == "NFM" else None
    for j, (x, y, w) in enumerate(zip(c["calls"], c["yc"], want)):
        am = b.push(x)
        assert am.shape == w["a"].shape and am.dtype == np.float32
        if y.shape[1] == 0:
            continue
        assert np.array_equal(cbits(b.iq()), cbits(y))                    # the bank's rows are the channelizer's
        st = b.state()
        assert np.array_equal(st["gain"], np.ones(nk, np.float32)) and st["open"].all()
        if mode == "NFM":
            try:
                e = judge(am, w["a"])                                     # nfm_compare: the allowance, and the carrier row's plain bar
            except AssertionError as err:
                raise AssertionError(f"T={T} NFM call {j} ({y.shape[1]} outputs): (row, rule, error) = {err}") from None
        else:
            per_row = ec.audio_error(mode, am, w)
            e = float(per_row.max())
            assert e <= TOL, f"T={T} {mode} call {j} ({y.shape[1]} outputs) row {int(per_row.argmax())}: {e:.3e}"
        worst = max(worst, e)
    print(f"BANKSWEEP T={T} mode {mode} worst {worst:.2e}")
    b.close()


@pytest.mark.parametrize("T", ec.LENGTHS)
def test_agc_on_at_every_length(T):
    """AM and USB with the block AGC: agc, gain and maxbuf against the float32 helper after every call with outputs,
    the audio against the float64 helper at TOL x gain (AM: x the row's peak |a| in the call, USB: x scale)."""
    c = shared()
    for mode in ("AM", "USB"):
        want, w32 = master(T, mode, True), mirror(T, mode, True)
        b = make_bank(T, mode, True, len(c["x"]))
        assert b.agc is True
        worst, worst_state = 0.0, 0.0
        for j, (x, y, w, m) in enumerate(zip(c["calls"], c["yc"], want, w32)):
            am = b.push(x)
            if y.shape[1] == 0:
                continue
            st = b.state()
            for k, wk in STATE:
                e = float(rel(st[k], m[wk]).max())
                worst_state = max(worst_state, e)
                assert e <= 1e-5, f"T={T} {mode} call {j}: {k} {e:.3e}"
            assert (w["gain"] != 1).any() and st["open"].all()
            measure = np.max(np.abs(w["a"]), axis=1).astype(np.float64) if mode == "AM" else w["scale"]
            per_row = np.max(np.abs(am - w["am"]), axis=1) / (w["gain"].astype(np.float64) * measure)
            e = float(per_row.max())
            assert e <= TOL, f"T={T} {mode} call {j} ({y.shape[1]} outputs) row {int(per_row.argmax())}: {e:.3e}"
            worst = max(worst, e)
        print(f"BANKSWEEP T={T} mode {mode} AGC on: worst {worst:.2e}, state {worst_state:.2e}")
        b.close()


@pytest.mark.parametrize("mode", ["AM", "NFM", "USB", "CW"])
@pytest.mark.parametrize("T", ec.LENGTHS)
def test_one_call_equals_the_tables_calls(T, mode):
    """The whole stream in one call (three tiles, the last partly filled) gives the bits of the table's calls -- of 1, 3,
    0, 5, 9, one tile, a tile and nine, 7 and 270 outputs -- laid end to end: at every length, not only at 255 and 191."""
    c = shared()
    b = make_bank(T, mode, False, len(c["x"]))
    one = b.push(c["x"])
    assert one.shape == (b.nk, ec.FRAMES) and np.isfinite(one).all() and np.abs(one).max() > 0
    b.reset()
    parts = [b.push(p) for p in c["calls"]]
    assert [p.shape[1] for p in parts] == c["counts"]
    got = np.concatenate(parts, axis=1)
    same = fbits(got) == fbits(one)
    assert same.all(), f"T={T} {mode}: first differing (row, output) {tuple(int(v) for v in np.argwhere(~same)[0])}"
    b.close()


def test_agc_through_a_step_silence_and_the_return():
    """AM at 9 taps, 140 calls of 4 outputs: full level, 40 dB down from call 20, an all-zero input from call 40, full
    level again from call 100 (bank_edge_cases.agc_case).  bank_finish's one AGC step per call goes through the decay,
    the 1e4 clamp and the attack out of it; the conditions that make it do so are asserted
    on the helper (bank_edge_cases.agc_conditions), the bank is held to the helper in every call."""
    a = ec.agc_case()
    T = ec.AGC_T
    yc = bo.cut_rows(channelizer_rows(a["x"]), a["cuts"], ec.D)
    w32 = ec.run_helper(T, "AM", np.float32, yc, True)
    w64 = ec.run_helper(T, "AM", np.float64, yc, True)
    clamp_rows = ec.agc_conditions(w32)
    b = make_bank(T, "AM", True, len(a["x"]))
    worst, worst_state, zero_calls = 0.0, 0.0, 0
    for j, (x, y, m, w) in enumerate(zip(bo.split(a["x"], a["cuts"]), yc, w32, w64)):
        am = b.push(x)
        assert am.shape == (12, ec.AGC_OUTPUTS) and np.array_equal(cbits(b.iq()), cbits(y))
        st = b.state()
        for k, wk in STATE:
            e = float(rel(st[k], m[wk]).max())
            worst_state = max(worst_state, e)
            assert e <= 1e-5, f"call {j}: {k} {e:.3e} (row {int(rel(st[k], m[wk]).argmax())})"
        bar = TOL * w["gain"].astype(np.float64) * np.max(np.abs(w["a"]), axis=1)
        d = np.max(np.abs(am - w["am"]), axis=1)
        assert (d <= bar).all(), f"call {j} row {int((d - bar).argmax())}: |am - want| {d.max():.3e}"
        worst = max(worst, float(np.max(d[bar > 0] / bar[bar > 0] * TOL, initial=0.0)))
        if not m["maxbuf"].any():                                          # the prototype has flushed: silence in, silence out
            assert not am.any()
            zero_calls += 1
        if ec.AGC_BACK - 10 <= j < ec.AGC_BACK:                            # the clamp itself, not 1e4 to within 1e-5
            assert (st["gain"][clamp_rows] == np.float32(1e4)).all()
    assert zero_calls >= 40
    print(f"BANKSWEEP AGC step case: worst |am - want| / (gain peak) {worst:.2e}, state {worst_state:.2e}")
    b.close()
