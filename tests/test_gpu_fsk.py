"""The RTTY raster skimmer on the GPU (pysdr_amd/csrc/fsk.hip, api_fsk.hip) against the float32 oracle
of the definition (tests/fsk_oracle.py): counts, event words and every state field are EQUAL after every call, floats by
their bits.  The oracle side is fed the rows of an independent Channelizer of the same shape and prototype on the same
input, so only the decoders' own arithmetic is judged."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import channelizer_oracle as cz
from tests import fsk_oracle as fo
from tests.test_gpu_psk import call_lengths, cut_rows, fbits

pytestmark = pytest.mark.gpu

BAUD = fo.BAUD
SECONDS = 12
MAX_OUT = 256
MESSAGE = fo.MESSAGE                         # 4.3 s of characters at 1.5 stop bits behind 3 s of mark
# (fs, channels, stations (Hz from the band's centre, SNR dB in a baud of bandwidth))
SHAPES = [(8000.0, (3, 4), ((800.0, 20.0), (1100.3, 25.0), (1400.7, 30.0))),                # S = 22: half a workgroup of 8 rows
          (12000.0, (30, 4), ((-700.2, 30.0), (-100.0, 20.0), (300.4, 25.0))),              # S = 33, across the wrap: 4 of 7 rows
          (12000.0, (5, 9), ((2000.0, 25.0), (3000.3, 30.0), (4500.7, 20.0))),              # a whole workgroup and a partial one
          (8000.0, (28, 9), ((-900.0, 25.0), (-10.3, 20.0), (700.7, 30.0)))]                # S = 22: a whole workgroup, a partial one, the wrap
IDS = ["8000-3+4", "12000-30+4", "12000-5+9", "8000-28+9"]
STOPS = (1.0, 1.5, 2.0)


def make_input(i, bad=False):
    fs, channels, stations = SHAPES[i]
    n = int(SECONDS * fs)
    rng = np.random.default_rng(400 + i)
    sg = fo.noise_sigma(20.0, BAUD, fs)                                       # the noise is 20 dB under a station of power 1
    x = sg * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for j, (f, snr) in enumerate(stations):
        s = fo.rtty_baseband(fo.baudot_codes(MESSAGE), fs, f, stop=STOPS[j], preamble=3.0 + 0.3 * j, tail=1.0, phase=1.0 + j)
        s = s[:n] * 10 ** ((snr - 20.0) / 20)
        x[:len(s)] += s
    x = (0.05 * x).astype(np.complex64)
    if bad:
        x[int(4.0 * fs) + 7] = complex(np.nan, 0.25)
        x[int(5.6 * fs) + 1] = complex(-0.5, np.inf)               # more than max_out outputs later: another call
    return x


@functools.lru_cache(maxsize=None)
def base(i, bad=False):
    """case i: the input and the rows of an independent channelizer; computed once, never changed"""
    from pysdr_amd import fsk
    from pysdr_amd.channelizer import Channelizer
    fs, channels, stations = SHAPES[i]
    S, D, M = fsk.shape(fs)
    x = make_input(i, bad)
    if bad:
        x = x[:int(9 * fs)]
    ch = Channelizer(fs, M, D, fsk.prototype(fs, M, S), channels, max_in=len(x))
    y = ch.push(x)
    ch.close()
    for v in (x, y):
        v.setflags(write=False)
    return dict(i=i, fs=fs, S=S, D=D, M=M, channels=channels, stations=stations, x=x, y=y, nk=y.shape[0], nfine=y.shape[0] * S)


@functools.lru_cache(maxsize=None)
def shared(i, max_out=MAX_OUT, bad=False):
    """case i cut into calls, and the oracle's answer to every call (counts, words, state after it)"""
    from pysdr_amd import fsk
    c = dict(base(i, bad))
    S, D = c["S"], c["D"]
    tile = fsk.plan(c["nk"], S, max_out, fsk.params())["tile"]
    cuts = call_lengths(len(c["x"]), D, tile, max_out)
    yc = cut_rows(c["y"], cuts, D)
    counts = [r.shape[1] for r in yc]
    assert 0 in counts and 1 in counts and max(counts) == max_out
    if max_out >= tile + 1:
        assert {tile - 1, tile, tile + 1} <= set(counts)
    o = fo.Oracle(c["nk"], S, fo.params())
    want = []
    for r in yc:
        wc, ev = o.process(r)
        want.append((wc, ev, o.state()))
    calls, at = [], 0
    for n in cuts:
        calls.append(c["x"][at:at + n])
        at += n
    c.update(cuts=cuts, calls=calls, yc=yc, want=want, tile=tile, max_out=max_out)
    return c


def make(c, max_out=MAX_OUT):
    from pysdr_amd.fsk import RTTY_Raster_Skimmer
    sk = RTTY_Raster_Skimmer(c["fs"], channels=c["channels"], max_in=len(c["x"]), max_out=max_out)
    assert (sk.S, sk.D, sk.M, sk.nk, sk.nfine) == (c["S"], c["D"], c["M"], c["nk"], c["nfine"])
    return sk


def same_state(got, want, where):
    for k in fo.FLOATS:
        assert np.array_equal(fbits(got[k]), fbits(want[k])), (where, k, np.flatnonzero(fbits(got[k]) != fbits(want[k]))[:5])
    for k in fo.INTS:
        assert np.array_equal(got[k], want[k]), (where, k, np.flatnonzero(got[k] != want[k])[:5])


def run_calls(c, max_out):
    sk = make(c, max_out)
    assert sk.dec.cap == fo.cap_of(max_out, c["S"])
    total = 0
    for j, (x, r, (wc, wev, wst)) in enumerate(zip(c["calls"], c["yc"], c["want"])):
        got = sk.dec.decode_raw(x, events="all", squelch=True)
        assert got["n_out"] == r.shape[1], j
        assert np.array_equal(got["counts"], wc), (j, np.flatnonzero(got["counts"] != wc)[:5])
        for F in np.flatnonzero(wc):
            assert list(got["events"][F, :wc[F]]) == wev[F], (j, F)
        same_state(sk.dec.state(), wst, j)
        assert np.array_equal(fbits(got["qn"]), fbits(wst["qn"])) and np.array_equal(got["open"], wst["open"]), j
        total += int(wc.sum())
    sk.close()
    return total


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_every_call_equals_the_oracle(i):
    """ragged cuts: 1-sample calls, calls that complete no output, calls that end on the kernel's tile boundary and one
    output to either side of it"""
    assert run_calls(shared(i), MAX_OUT) > 100                                # the stations were read, not just noise compared


@pytest.mark.parametrize("i", (0, 1), ids=IDS[:2])
def test_every_call_of_at_most_16_outputs_equals_the_oracle(i):
    """max_out = 16: a cap of one slot, a quarter of a tile per call"""
    c = shared(i, 16)
    assert fo.cap_of(16, c["S"]) == 1 and len(c["calls"]) > 150
    assert run_calls(c, 16) > 100


@pytest.mark.parametrize("i", range(3), ids=IDS[:3])
def test_the_whole_stream_in_calls_of_max_out(i):
    """push cuts the stream itself; events and text are the oracle skimmer's (owners only), the end state the oracle's"""
    c = shared(i)
    sk = make(c)
    ev = sk.push(c["x"])
    ref = fo.Skimmer(c["nk"], c["S"], False, max_out=MAX_OUT)
    want = ref.push(c["y"])
    assert ev == want and len(ev) > 30
    assert {F: t for F, t in sk.text.items() if t} == ref.text
    same_state(sk.dec.state(), c["want"][-1][2], "end")
    sk.close()


def test_skimmer_reads_the_three_messages_on_their_owners():
    from pysdr_amd import fsk
    c = shared(0)
    sk = make(c)
    ev = sk.push(c["x"])
    st = sk.state()
    assert np.allclose(sk.freqs_fine, fo.fine_freqs(c["fs"], c["M"], c["S"], c["channels"])) and not sk.circular
    assert np.allclose(sk.freqs_mark - sk.freqs_fine, 15 * BAUD / 8) and np.allclose(np.diff(sk.freqs_fine), BAUD / 4)
    said = {F: t for F, t in sk.text.items() if t}
    home = []
    for f, snr in c["stations"]:
        near = [F for F in said if abs(sk.freqs_fine[F] - f) <= BAUD / 4]      # one raster step
        print(f"station {f} Hz {snr} dB:", {(F, round(float(sk.freqs_fine[F]), 2), round(float(st['contrast'][F]), 3)): said[F] for F in near})
        assert any(MESSAGE in said[F] for F in near), (f, said)
        home += near
    assert set(said) == set(home), said                                       # nothing on the neighbours, the images or the noise
    assert all(m2 >= m1 for (m1, _, _), (m2, _, _) in zip(ev, ev[1:]))
    assert st["open"].dtype == bool and st["freq"].shape == (c["nfine"],) and fsk.code_text(27) == "<FIGS>"
    sk.close()


def test_a_call_of_too_many_outputs_is_refused_and_changes_nothing():
    from pysdr_amd import _lib
    c = shared(0)
    D = c["D"]
    sk = make(c)
    L = _lib.lib()
    n1 = 3900 * D + 3
    sk.push(c["x"][:n1])
    before = sk.dec.state()
    x = np.array(c["x"][n1:n1 + (MAX_OUT + 1) * D])
    n_out = C.c_int(-1)
    assert sk.dec.chan.n_out_for(len(x)) == MAX_OUT + 1
    h, p = sk.dec._h, C.c_void_p(x.ctypes.data)
    rc = L.pysdr_fsk_process(h, p, len(x), 0, C.byref(n_out), None, None, 0, None, None)
    assert rc == -5 and n_out.value == 0 and b"max_out" in L.pysdr_last_error()
    ev = np.zeros((c["nfine"], 1), np.int32)
    cnt = np.zeros(c["nfine"], np.int32)
    pi32 = C.POINTER(C.c_int32)
    assert sk.dec.cap == 2
    assert L.pysdr_fsk_process(h, p, 64, 0, C.byref(n_out), cnt.ctypes.data_as(pi32), ev.ctypes.data_as(pi32), 1, None, None) == -5
    assert b"ev_pitch" in L.pysdr_last_error()
    assert L.pysdr_fsk_process(h, p, len(c["x"]) + 1, 0, C.byref(n_out), None, None, 0, None, None) == -5
    assert L.pysdr_fsk_process(h, None, 16, 0, C.byref(n_out), None, None, 0, None, None) == -1
    assert L.pysdr_fsk_process(h, p, -1, 0, C.byref(n_out), None, None, 0, None, None) == -1
    assert L.pysdr_fsk_process(h, p, 16, 0, None, None, None, 0, None, None) == -1
    rows = np.array([0, c["nfine"]], np.int32)
    big = np.zeros((2, sk.dec.cap), np.int32)
    assert L.pysdr_fsk_fetch(h, _lib.as_pi(rows), 2, big.ctypes.data_as(pi32), sk.dec.cap) == -1
    assert L.pysdr_fsk_fetch(h, _lib.as_pi(rows), 1, big.ctypes.data_as(pi32), sk.dec.cap - 1) == -5
    same_state(sk.dec.state(), before, "after the refused calls")
    # the stream did not advance: the rest equals an undisturbed twin's
    twin = make(c)
    twin.push(c["x"][:n1])
    rest = c["x"][n1:n1 + 3000 * D]
    got = sk.push(rest)
    assert got == twin.push(rest) and len(got) > 5
    same_state(sk.dec.state(), twin.dec.state(), "rest")
    sk.close()
    twin.close()


def test_a_call_without_outputs_changes_no_state_and_has_no_events():
    c = shared(0)
    D = c["D"]
    sk = make(c)
    sk.push(c["x"][:4500 * D + 1])
    before = sk.dec.state()
    got = sk.dec.decode_raw(c["x"][4500 * D + 1:4501 * D], events="all", squelch=True)   # ends one sample short of the next frame
    assert got["n_out"] == 0 and not got["counts"].any()
    assert np.array_equal(fbits(got["qn"]), fbits(before["qn"])) and np.array_equal(got["open"], before["open"]) and before["open"].any()
    assert not sk.dec.fetch([0, 1, 2, 5]).any()                              # nothing to fetch after it
    same_state(sk.dec.state(), before, "empty call")
    sk.close()


def test_one_nan_and_one_inf_blank_their_windows_and_nothing_else():
    """The rows of a channelizer on the same input carry each non-finite sample for as long as its window holds it; the
    decoders blank the outputs whose bit window reaches such a row sample (step 1: that it is exactly S outputs per row
    sample is shown on the oracle, tests/test_fsk_oracle.py), so events and state still equal the oracle's, every state
    float stays finite, and once the windows have passed the calls equal a run of the oracle from the state reached there."""
    c = shared(0, MAX_OUT, True)
    S, D = c["S"], c["D"]
    assert not np.isfinite(c["y"]).all() and np.isfinite(c["y"][:, -500:]).all()
    bad_calls = [j for j, r in enumerate(c["yc"]) if not np.isfinite(r).all()]
    assert len(bad_calls) >= 2
    sk = make(c)
    restart, m = None, 0
    for j, (x, r, (wc, wev, wst)) in enumerate(zip(c["calls"], c["yc"], c["want"])):
        got = sk.dec.decode_raw(x, events="all")
        st = sk.dec.state()
        assert np.array_equal(got["counts"], wc), j
        for F in np.flatnonzero(wc):
            assert list(got["events"][F, :wc[F]]) == wev[F], (j, F)
        same_state(st, wst, j)
        assert all(np.isfinite(st[k]).all() for k in fo.FLOATS), j
        m += r.shape[1]
        if restart is not None:
            wc2, wev2 = restart.process(r)
            assert np.array_equal(wc2, wc) and wev2 == wev, j
            same_state(st, restart.state(), ("restarted", j))
        elif j == bad_calls[-1] + 1:
            assert np.isfinite(c["y"][:, m - S + 1:m]).all()
            restart = fo.Oracle(c["nk"], S, fo.params())                      # from the device's state behind the windows
            restart.set_state(st, c["y"][:, m - (S - 1):m], m)
    assert restart is not None and sum(int(w[0].sum()) for w in c["want"]) > 10
    sk.close()


def test_reset_repeats_the_first_run():
    c = shared(0)
    sk = make(c)
    x = c["x"][:int(9 * c["fs"])]
    first = sk.push(x)
    st = sk.dec.state()
    text = dict(sk.text)
    assert len(first) > 5
    sk.reset()
    z = sk.dec.state()
    assert (z["cnt"] == c["S"]).all() and (z["prev"] == 1).all()
    assert not any(z[k].any() for k in ("st", "sh", "nb", "fig", "open", "seen")) and not any(fbits(z[k]).any() for k in fo.FLOATS)
    assert not any(sk.text.values()) and sk.chan.n_in == 0
    assert sk.push(x) == first and dict(sk.text) == text
    same_state(sk.dec.state(), st, "second run")
    sk.close()


def test_device_input_stays_on_the_device_until_fetched():
    """decode_raw with a device pointer and events=None only queues work; the rows fetched afterwards are the host-fed
    twin's"""
    from pysdr_amd import _lib
    c = shared(0)
    D, fs = c["D"], c["fs"]
    L = _lib.lib()
    at = int(5 * fs)
    x = np.array(c["x"][at:at + MAX_OUT * D])
    head = c["x"][:at]
    sk, twin = make(c), make(c)
    sk.push(head)
    twin.push(head)
    d = C.c_void_p()
    _lib.check(L.pysdr_dev_alloc(0, x.nbytes, C.byref(d)), "alloc")
    _lib.check(L.pysdr_dev_upload(0, d, C.c_void_p(x.ctypes.data), x.nbytes), "upload")
    got = sk.dec.decode_raw(d.value, len(x), on_device=True, events=None)
    sk.sync()
    want = twin.dec.decode_raw(x, events="all")
    assert got["n_out"] == want["n_out"] == MAX_OUT and got["counts"] is None and want["counts"].sum() > 0
    rows = np.flatnonzero(want["counts"])
    words = sk.dec.fetch(np.concatenate((rows, [0])))                        # runs of consecutive rows and a single one
    for k, F in enumerate(rows):
        assert np.array_equal(words[k, :want["counts"][F]], want["events"][F, :want["counts"][F]])
    same_state(sk.dec.state(), twin.dec.state(), "device input")
    _lib.check(L.pysdr_dev_free(0, d), "free")
    sk.close()
    twin.close()
