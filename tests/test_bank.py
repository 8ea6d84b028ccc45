"""Channel bank without a GPU: the test helper is the oracle's receiver behind ``rx.iq``, the
device-free plan accepts exactly what the spec allows, and the shared input has the margins the GPU tests rely on."""
import ctypes as C

import numpy as np
import pytest

import pysdr_amd.bank as bank
from oracle import sdr_oracle as so
from pysdr_amd import _lib
from pysdr_amd.design import channelizer_taps
from tests import bank_oracle as bo
from tests import channelizer_oracle as co
from tests.test_gpu_parity import TOL


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("mode,squelch", [("AM", 0.0), ("NFM", bo.SQUELCH)])
def test_the_helper_is_the_oracles_receiver(mode, squelch):
    """so.Receiver at 800 kS/s -> 25 kS/s (UP = 1, DOWN = 32) on the base case's strongest carrier; the helper is fed the
    receiver's own rx.iq of every call and must repeat am, AGC and squelch state bit for bit"""
    fs, fs_out, T = 800e3, 25e3, 255
    c = bo.case(*bo.BASE[:2], frames=2200)
    rx = so.Receiver(fs, fs_out, 3 * fs / 64, mode, ntaps_af=T, af_bw=4e3)
    assert (rx.up, rx.down, rx.fs_out) == (1, 32, fs_out)
    rx.squelch = np.float32(squelch)
    taps = rx.demod.taps.real.astype(np.float64)
    assert np.array_equal(taps, bank.af_taps(fs_out, T, 4e3).astype(np.float32))     # the product designs the same filter
    h = bo.BankOracle(1, fs_out, taps, mode, squelch=squelch)
    calls = [x for x in bo.split(c["x"], c["cuts"]) if len(x) != 1]                   # (the receiver decays on an empty call)
    assert len(calls) >= 6
    opened = []
    for x in calls:
        am = rx.demod_data(x)
        assert len(am) >= 1
        got = h.process(np.asarray(rx.iq)[None, :])
        assert np.array_equal(bits(got["am"][0]), bits(am))
        assert bits(got["agc"])[0] == bits(rx.agc.agc) and bits(got["agc_gain"])[0] == bits(rx.agc.gain)
        assert bits(got["maxbuf"])[0] == bits(rx.agc.maxbuf)
        assert bits(got["level"])[0] == bits(rx.sq_level) and bool(got["open"][0]) == rx.sq_open
        opened.append(rx.sq_open)
    if mode == "NFM":
        assert not opened[1] and opened[-1]                     # the start-up transient closes the gate, the carrier opens it
    else:
        assert float(rx.agc.gain) > 1.0


def _plan(nk, T, max_out):
    out = (C.c_int32 * 8)()
    return _lib.lib().pysdr_bank_plan(nk, T, max_out, out), list(out)


def test_plan_rules(hiplib):
    for nk in (1, 12, 640, 4096):
        for T in (3, 4, 8, 63, 254, 255):
            rc, p = _plan(nk, T, 5000)
            assert rc == 0, (nk, T)
            tile, threads, lds, tiles, hist, tp = p[:6]
            assert tile == 8 * threads and threads % 64 == 0
            assert tiles == -(-5000 // tile)
            assert hist >= T + 1 and hist % 2 == 0 and hist <= threads            # rows stay 16-byte aligned; one sample per thread
            assert tp >= T and tp % 8 == 0 and lds == 4 * (tile + tp) <= 65536
    E = -1
    assert _plan(0, 255, 100)[0] == E and _plan(4097, 255, 100)[0] == E
    assert _plan(64, 2, 100)[0] == E and _plan(64, 256, 100)[0] == E and _plan(64, -1, 100)[0] == E
    assert _plan(64, 255, 0)[0] == E
    assert _lib.lib().pysdr_bank_plan(64, 255, 100, None) == E
    assert bank.plan(64, 255, 1)["history"] == 256
    with pytest.raises(_lib.PysdrError):
        bank.plan(64, 256, 1)


def test_null_handles_are_argument_errors(hiplib):
    L = _lib.lib()
    n = C.c_int(0)
    h = C.c_void_p()
    assert L.pysdr_bank_create(None, 25e3, 9, 255, C.byref(h)) == -1 and not h.value
    assert L.pysdr_bank_set_mode(None, 9, None, 255) == -1
    assert L.pysdr_bank_set_agc(None, 1, 0.5) == -1 and L.pysdr_bank_set_squelch(None, 0.0) == -1
    assert L.pysdr_bank_reset(None) == -1 and L.pysdr_bank_sync(None) == -1
    assert L.pysdr_bank_process(None, None, 0, 0, None, 0, 0, C.byref(n)) == -1
    assert L.pysdr_bank_state(None, None, None, None, None, None) == -1
    assert L.pysdr_bank_fetch(None, None, 0, None, None, 0) == -1
    L.pysdr_bank_destroy(None)


@pytest.mark.parametrize("M,D,channels,T", bo.SHAPES)
def test_input_conditions(M, D, channels, T):
    """What the GPU tests take for granted, on the oracle alone (rows from the float64 polyphase form): no squelch level
    within 1 % of the threshold, float32 and float64 gates equal, the NFM allowance exactly zero on the carrier channels
    from output 256 on, the float32 helper's audio within a quarter of the parity bar of the float64 helper's under the
    NFM rule of the GPU tests, and gates of both kinds at the end: open on the carrier channels, closed on all others."""
    c = bo.case(M, D, channels)
    fs_out = c["fs"] / D
    frames = len(c["x"]) // D
    assert frames >= 1200 and len(c["carrier_rows"]) >= 4
    counts = [-(-(s + n) // D) - -(-s // D) for s, n in zip(np.cumsum([0] + c["cuts"][:-1]), c["cuts"])]
    assert counts[:3] == [1, 3, 0] and len(counts) >= 6 and all(k % 2048 for k in counts[3:])
    if (M, D) == bo.BASE[:2]:         # one call of more than one tile of the kernel, the last of them partly filled
        assert max(counts) == bo.BIG and 2048 < bo.BIG < 4096
    y = co.polyphase(c["x"], channelizer_taps(M), M, D, 0, frames, c["rows"]).astype(np.complex64)
    taps = bank.af_taps(fs_out, T, bo.AF_BW)
    nk = len(c["rows"])
    o32 = bo.BankOracle(nk, fs_out, taps, "NFM", squelch=bo.SQUELCH)
    o64 = bo.BankOracle(nk, fs_out, taps, "NFM", squelch=bo.SQUELCH, dtype=np.float64)
    worst, margin, r32 = 0.0, np.inf, None
    pk, seen, own = [0.0] * nk, 0, 0.0
    for rows in bo.cut_rows(y, c["cuts"], D):
        r32, r64 = o32.process(rows), o64.process(rows)
        n = rows.shape[1]
        if n == 0:
            continue
        seen += n
        for a in range(nk):                   # the NFM parity rule of run_both, float32 helper against float64 helper
            allow = o32.allowance(a, y[a, :seen])[-n:]
            ok = allow == 0
            pk[a] = max(pk[a], float(np.max(np.abs(r32["a"][a][ok]))) if ok.any() else 0.0)
            excess = np.maximum(np.abs(r32["a"][a] - r64["a"][a]) - allow, 0.0)
            own = max(own, float(np.max(excess) / (pk[a] if pk[a] > 0 else 1.0)))
        assert np.array_equal(r32["open"], r64["open"])
        margin = min(margin, float(np.min(np.abs(r32["level"].astype(np.float64) - bo.SQUELCH) / bo.SQUELCH)))
        worst = max(worst, float(np.max(np.abs(r32["level"] - r64["level"]) / np.maximum(r64["level"], 1e-30))))
    print(f"M {M} D {D}: least |level - {bo.SQUELCH}| / {bo.SQUELCH} = {margin:.3f}, float32 vs float64 level {worst:.2e}, "
          f"{int(r32['open'].sum())} of {nk} gates open at the end")
    assert margin >= 0.01
    # the yardstick's own float32 rounding leaves a float32 implementation room under the bar: a factor 4, as for the squelch
    print(f"M {M} D {D}: float32 vs float64 helper audio, excess over the allowance / full scale {own:.2e}")
    assert 4 * own <= TOL
    for a in c["carrier_rows"]:
        assert np.all(o32.allowance(a, y[a])[256:] == 0.0), (a, c["rows"][a])
    # long enough for the start-up transient (levels in the hundreds) to decay
    assert r32["open"].sum() >= 3 and (~r32["open"]).sum() >= 3
    assert set(np.flatnonzero(r32["open"])) == set(c["carrier_rows"])
