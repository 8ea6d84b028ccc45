"""The FT4 skimmer on the GPU (pysdr_amd/csrc/ft.hip, api_ft.hip) against the float32 oracle of the
definition (tests/ft4_oracle.py): counts, event words, scores, hit counts, the spectrum ring and the soft bits are EQUAL
after every call, floats by their bits.  The oracle side is fed the rows of an independent Channelizer of the same shape
and prototype on the same input, so only the skimmer's own arithmetic is judged.  Streams are 7 s: a frame with its ramps
is 5.04 s, it starts up to 0.9 s in, and the hold is 17 symbols."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import ft4_oracle as fo
from tests.test_ft4_oracle import SNR_CLEAN
from tests.test_gpu_psk import call_lengths, cut_rows, fbits

pytestmark = pytest.mark.gpu

BAUD = fo.BAUD
SECONDS = 7
MAX_OUT = 256
STEP = BAUD / 2                              # the raster's step, 10.4 Hz
# (fs, channels, stations (Hz of tone 0 from the band's centre, SNR dB in 2500 Hz, start of the ramp s)); a row's fine rows
# sit at its centre + (2 j - (NSUB + 5)) baud / 4
SHAPES = [(8000.0, (3, 3), ((750.0 - 9 * BAUD / 4, -5.0, 0.5),                 # S = 48, M = 32, rows 250 Hz apart: on the raster,
                            (1000.0 + 3 * BAUD / 4 + 0.3 * STEP, 3.0, 0.9),    # 0.3 steps off it
                            (1250.0 + 11 * BAUD / 4 + 0.5 * STEP, -8.0, 0.2))),  # and half way between two decoders
          (12000.0, (5, 2), ((1875.0 - 21 * BAUD / 4 + 0.5 * STEP, -6.0, 0.6),  # S = 72, rows 375 Hz apart
                             (2250.0 - 33 * BAUD / 4, -9.0, 0.3), (2250.0 + 15 * BAUD / 4 + 0.3 * STEP, 3.0, 0.8))),
          (8000.0, None, ((-156.25, 0.0, 0.4),                                 # all 32 rows: half way between the last fine row and fine row 0
                          (1750.0 + 5 * BAUD / 4, -7.0, 0.8), (-3000.0 - 17 * BAUD / 4 + 0.3 * STEP, -9.0, 0.6)))]
IDS = ["8000-3+3", "12000-5+2", "8000-all"]
RAMP = 0.048                                 # the frame's first Costas symbol begins one symbol behind the ramp's start


def station_bits(i, j):
    return np.random.default_rng(1000 + 10 * i + j).integers(0, 2, 174)


def make_input(i, bad=False):
    fs, channels, stations = SHAPES[i]
    n = int(SECONDS * fs)
    rng = np.random.default_rng(500 + i)
    x = fo.noise_sigma(0.0, fo.SNR_BW, fs) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))   # noise of power 1 in 2500 Hz
    for j, (f, snr, start) in enumerate(stations):
        s = fo.waveform(fo.tones(station_bits(i, j)), f, fs, gfsk=j != 1, phase=1.0 + j) * 10 ** (snr / 20)   # with its ramps
        at = int(start * fs)
        x[at:at + len(s)] += s[:n - at]
    x = (0.05 * x).astype(np.complex64)
    if bad:
        x[int(2.0 * fs) + 7] = complex(np.nan, 0.25)
        x[int(3.1 * fs) + 1] = complex(-0.5, np.inf)               # more than max_out outputs later: another call
    return x


@functools.lru_cache(maxsize=None)
def base(i, bad=False):
    """case i: the input and the rows of an independent channelizer; computed once, never changed"""
    from pysdr_amd import ft4
    from pysdr_amd.channelizer import Channelizer
    fs, channels, stations = SHAPES[i]
    S, D, M = ft4.shape(fs)
    x = make_input(i, bad)
    ch = Channelizer(fs, M, D, ft4.prototype(fs, M, S), channels, max_in=len(x))
    y = ch.push(x)
    ch.close()
    for v in (x, y):
        v.setflags(write=False)
    return dict(i=i, fs=fs, S=S, D=D, M=M, channels=channels, stations=stations, x=x, y=y, nk=y.shape[0], nfine=y.shape[0] * (S // 2))


@functools.lru_cache(maxsize=None)
def shared(i, max_out=MAX_OUT, bad=False):
    """case i cut into calls, and the oracle's answer to every call (counts, words, state after it)"""
    from pysdr_amd import ft4
    c = dict(base(i, bad))
    S, D = c["S"], c["D"]
    tile = ft4.plan(c["nk"], S, max_out, ft4.params())["tile"]
    assert tile == S
    cuts = call_lengths(len(c["x"]), D, tile, max_out)
    yc = cut_rows(c["y"], cuts, D)
    counts = [r.shape[1] for r in yc]
    assert 0 in counts and 1 in counts and max(counts) == max_out and any(0 < v < S // 4 for v in counts)
    if max_out >= tile + 1:
        assert {tile - 1, tile, tile + 1} <= set(counts)
    o = fo.Oracle(c["nk"], S, fo.params(), max_out)
    want = []
    for r in yc:
        t_first = o.t_done
        wc, ev = o.process(r)
        want.append((wc, ev, o.state(), o.events_of(t_first, ev)))
    calls, at = [], 0
    for n in cuts:
        calls.append(c["x"][at:at + n])
        at += n
    c.update(cuts=cuts, calls=calls, yc=yc, want=want, tile=tile, max_out=max_out)
    return c


def make(c, max_out=MAX_OUT):
    from pysdr_amd.ft4 import FT4_Skimmer
    sk = FT4_Skimmer(c["fs"], channels=c["channels"], max_in=len(c["x"]), max_out=max_out)
    assert (sk.S, sk.D, sk.M, sk.nk, sk.nfine) == (c["S"], c["D"], c["M"], c["nk"], c["nfine"])
    return sk


def same_state(got, want, where, ring=True):
    assert got["t_done"] == want["t_done"], where
    keys = ("sc", "ring") if ring else ("sc",)
    for k in keys:
        assert np.array_equal(fbits(got[k]), fbits(want[k])), (where, k, np.flatnonzero(fbits(got[k]) != fbits(want[k]))[:5])
    assert np.array_equal(got["hits"], want["hits"]), (where, "hits")


def words_of(ev):
    return [int(w) for pair in ev for w in pair]


def run_calls(c, max_out, every=1):
    """every call against the oracle: n_out, steps, counts, event words, scores, hits, and the ring on every `every`-th
    call; the soft bits of every event once its frame is whole.  -> the events seen"""
    sk = make(c, max_out)
    assert sk.dec.slots == fo.cap_of(max_out, c["S"]) and sk.dec.tr == fo.ring_steps(max_out, c["S"])
    o = fo.Oracle(c["nk"], c["S"], fo.params(), max_out)                       # a twin for the soft bits, stepped alongside
    seen, due = [], []
    for j, (x, r, (wc, wev, wst, wlist)) in enumerate(zip(c["calls"], c["yc"], c["want"])):
        got = sk.dec.decode_raw(x, events="all")
        o.process(r)
        assert got["n_out"] == r.shape[1] and got["t_first"] + got["n_steps"] == wst["t_done"], j
        assert np.array_equal(got["counts"], wc), (j, np.flatnonzero(got["counts"] != wc)[:5])
        for F in np.flatnonzero(wc):
            assert list(got["events"][F, :2 * wc[F]]) == words_of(wev[F]), (j, F)
        if r.shape[1]:
            assert sk.dec.events_of(got) == wlist, j
        ring = j % every == 0 or j == len(c["calls"]) - 1
        same_state(sk.dec.state(ring=ring), wst, j, ring)
        seen += wlist
        due += wlist
        ripe = [e for e in due if o.llr_ok(e[1], e[0])]
        if ripe:
            soft = sk.dec.llr([e[1] for e in ripe], [e[0] for e in ripe])
            for e, v in zip(ripe, soft):
                assert np.array_equal(fbits(v), fbits(o.llr(e[1], e[0]))), (j, e)
            due = [e for e in due if e not in ripe]
    sk.close()
    return seen


def step_of(c, start):
    """the step at which a station whose ramp starts at `start` s has its first Costas symbol: one symbol later, and the
    prototype delays a row by 8 outputs"""
    return ((start + RAMP) * c["fs"] / c["D"] + 8) / (c["S"] // 4)


def found(events, c, i):
    """every station has an event within a step and a fine row of where it was sent"""
    ff = fo.fine_freqs(c["fs"], c["M"], c["S"], c["channels"])
    for f, snr, start in c["stations"]:
        assert any(abs(e[0] - step_of(c, start)) <= 1.5 and abs(ff[e[1]] - f) <= STEP + 0.1 for e in events), (f, snr, events)
    return True


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_every_call_equals_the_oracle(i):
    """ragged cuts: 1-sample calls, calls that complete no output or fewer than a step's outputs, calls that end on the
    kernel's tile boundary (S outputs) and one output to either side of it, calls of max_out outputs"""
    c = shared(i)
    assert found(run_calls(c, MAX_OUT, every=1 if c["nk"] < 10 else 8), c, i)


@pytest.mark.parametrize("i", (0, 1), ids=IDS[:2])
def test_every_call_of_at_most_16_outputs_equals_the_oracle(i):
    """max_out = 16: at most a step (S = 72) or two (S = 48) per call, a cap of one slot"""
    c = shared(i, 16)
    assert fo.cap_of(16, c["S"]) == 1 and len(c["calls"]) > 300
    assert found(run_calls(c, 16, every=16), c, i)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_the_whole_stream_in_calls_of_max_out_and_the_records_of_three_stations(i):
    """push cuts the stream itself; the records are the oracle skimmer's (owners only, soft bits by their bits), the end
    state the oracle's; each station is one record on the fine row at or beside its frequency, with its bits where the
    SNR allows (SNR_CLEAN and above: DESIGN.md 3 item 23) and nothing else is reported"""
    from pysdr_amd import ft4
    c = shared(i)
    sk = make(c)
    recs = sk.push(c["x"])
    ref = fo.Skimmer(c["nk"], c["S"], c["channels"] is None, MAX_OUT)
    want = ref.push(c["y"])
    assert [(r["t0"], r["F"], r["hits"]) for r in recs] == [(r["t0"], r["F"], r["hits"]) for r in want] and len(recs) >= 3
    for a, b in zip(recs, want):
        assert fbits(np.float32(a["score"])) == fbits(np.float32(b["score"])) and np.array_equal(fbits(a["llr"]), fbits(b["llr"]))
    same_state(sk.dec.state(ring=True), c["want"][-1][2], "end")
    assert sk.circular == (c["channels"] is None) and np.allclose(sk.freqs_fine, fo.fine_freqs(c["fs"], c["M"], c["S"], c["channels"]))
    assert np.allclose(np.diff(sk.freqs_fine[:c["S"]]), STEP)
    home, asserted = [], 0
    for j, (f, snr, start) in enumerate(c["stations"]):
        near = [r for r in recs if abs(r["freq"] - f) <= STEP / 2 + 0.1 and abs(r["time"] - (start + RAMP + 0.008)) <= 0.03]
        errs = [int((ft4.hard_bits(r["llr"]) != station_bits(i, j)).sum()) for r in near]
        print(f"station {f:.2f} Hz {snr} dB at {start} s:", [(r["t0"], r["F"], round(r["freq"], 2), round(r["score"], 1), r["hits"]) for r in near], "bit errors", errs)
        assert len(near) == 1, (f, near)
        if snr >= SNR_CLEAN:
            assert errs == [0]
            asserted += 1
        home += near
    assert asserted >= 1 and len(recs) == len(home), [(r["t0"], r["F"], r["score"], r["hits"]) for r in recs]
    assert abs(float(np.std(ft4.unit_llr(recs[0]["llr"]))) - 1) < 1e-3
    sk.close()


def test_slot_and_dt_follow_t_first():
    from pysdr_amd.ft4 import FT4_Skimmer
    c = shared(0)
    sk = FT4_Skimmer(c["fs"], channels=c["channels"], max_in=len(c["x"]), t_first=1_700_000_000 * 7.5 + 7.5 - 0.1)
    recs = sk.push(c["x"])
    assert len(recs) == 3
    for r in recs:                                                              # the stream began 0.1 s before a slot: dt = time - 0.1 - 0.5
        assert r["slot"] == 1_700_000_001 and abs(r["dt"] - (r["time"] - 0.6)) < 1e-3
    sk.close()


def test_a_call_of_too_many_outputs_is_refused_and_changes_nothing():
    from pysdr_amd import _lib
    c = shared(0)
    D = c["D"]
    sk = make(c)
    L = _lib.lib()
    n1 = 5700 * D + 3                                                          # 5.7 s in: frames are being found
    first = sk.push(c["x"][:n1])
    before = sk.dec.state(ring=True)
    x = np.array(c["x"][n1:n1 + (MAX_OUT + 1) * D])
    n_out = C.c_int(-1)
    assert sk.dec.chan.n_out_for(len(x)) == MAX_OUT + 1
    h, p = sk.dec._h, C.c_void_p(x.ctypes.data)
    rc = L.pysdr_ft4_process(h, p, len(x), 0, C.byref(n_out), None, None, 0, None)
    assert rc == -5 and n_out.value == 0 and b"max_out" in L.pysdr_last_error()
    pi32 = C.POINTER(C.c_int32)
    words = 2 * sk.dec.slots
    ev = np.zeros((c["nfine"], words - 1), np.int32)
    cnt = np.zeros(c["nfine"], np.int32)
    assert L.pysdr_ft4_process(h, p, 64, 0, C.byref(n_out), cnt.ctypes.data_as(pi32), ev.ctypes.data_as(pi32), words - 1, None) == -5
    assert b"ev_pitch" in L.pysdr_last_error()
    assert L.pysdr_ft4_process(h, p, len(c["x"]) + 1, 0, C.byref(n_out), None, None, 0, None) == -5
    assert L.pysdr_ft4_process(h, None, 16, 0, C.byref(n_out), None, None, 0, None) == -1
    assert L.pysdr_ft4_process(h, p, -1, 0, C.byref(n_out), None, None, 0, None) == -1
    assert L.pysdr_ft4_process(h, p, 16, 0, None, None, None, 0, None) == -1
    rows = np.array([0, c["nfine"]], np.int32)
    big = np.zeros((2, words), np.int32)
    assert L.pysdr_ft4_fetch(h, _lib.as_pi(rows), 2, big.ctypes.data_as(pi32), words) == -1      # a fine row outside the raster
    assert L.pysdr_ft4_fetch(h, _lib.as_pi(rows), 1, big.ctypes.data_as(pi32), words - 1) == -5
    same_state(sk.dec.state(ring=True), before, "after the refused calls")
    # the stream did not advance: the rest equals an undisturbed twin's
    twin = make(c)
    assert [(r["t0"], r["F"]) for r in twin.push(c["x"][:n1])] == [(r["t0"], r["F"]) for r in first]
    rest = c["x"][n1:]
    got, want = sk.push(rest), twin.push(rest)
    assert [(r["t0"], r["F"], r["score"]) for r in got] == [(r["t0"], r["F"], r["score"]) for r in want] and len(first) + len(got) == 3
    assert 0 < len(first) < 3
    same_state(sk.dec.state(ring=True), twin.dec.state(ring=True), "rest")
    sk.close()
    twin.close()


def test_a_call_without_outputs_changes_no_state_and_has_no_events():
    c = shared(0)
    D = c["D"]
    sk = make(c)
    sk.push(c["x"][:6000 * D + 1])
    before = sk.dec.state(ring=True)
    got = sk.dec.decode_raw(c["x"][6000 * D + 1:6001 * D], events="all")       # ends one sample short of the next frame
    assert got["n_out"] == 0 and got["n_steps"] == 0 and not got["counts"].any() and before["sc"].any()
    assert not sk.dec.fetch([0, 1, 2, 5]).any()                                # nothing to fetch after it
    same_state(sk.dec.state(ring=True), before, "empty call")
    sk.close()


def test_one_nan_and_one_inf_change_only_the_steps_whose_windows_hold_them():
    """The rows of a channelizer on the same input carry each non-finite sample for as long as its window holds it; the
    spectrum blanks the bins of the steps whose window reaches such a row sample (step 1), so every call still equals the
    oracle and every float of the state stays finite; and against the clean stream's run the ring's history differs only
    in the steps whose S-sample windows hold a row sample that differs."""
    c, clean = shared(0, MAX_OUT, True), base(0)
    S = c["S"]
    assert not np.isfinite(c["y"]).all()
    sk = make(c)
    for j, (x, r, (wc, wev, wst, wlist)) in enumerate(zip(c["calls"], c["yc"], c["want"])):
        got = sk.dec.decode_raw(x, events="all")
        st = sk.dec.state(ring=True)
        assert np.array_equal(got["counts"], wc), j
        same_state(st, wst, j)
        assert np.isfinite(st["sc"]).all() and np.isfinite(st["ring"]).all(), j
    sk.close()
    o = fo.Oracle(c["nk"], S, fo.params())
    T = fo.steps_done(c["y"].shape[1], S)
    starts = (S // 4) * np.arange(T) + (S - 1)
    with np.errstate(all="ignore"):
        Pb = o.spectrum(np.concatenate((o.hist, c["y"]), axis=1), starts)
        Pc = o.spectrum(np.concatenate((o.hist, clean["y"]), axis=1), starts)
    differs = c["y"].view(np.uint64) != clean["y"].view(np.uint64)
    nonfinite = ~np.isfinite(c["y"])
    for a in range(c["nk"]):
        for t in range(T):
            w = slice((S // 4) * t, (S // 4) * t + S)
            if not differs[a, w].any():
                assert np.array_equal(fbits(Pb[a, t]), fbits(Pc[a, t])), (a, t)
            if nonfinite[a, w].any():
                assert not Pb[a, t].any(), (a, t)
    assert nonfinite.any(axis=1).all() and (~differs).all(axis=0).sum() > c["y"].shape[1] - 100


def test_reset_repeats_the_first_run():
    c = shared(0)
    sk = make(c)
    first = sk.push(c["x"])
    st = sk.dec.state(ring=True)
    assert len(first) == 3
    sk.reset()
    z = sk.dec.state(ring=True)
    assert z["t_done"] == 0 and not z["hits"].any() and not fbits(z["sc"]).any() and not fbits(z["ring"]).any()
    assert not sk.records and sk.chan.n_in == 0
    again = sk.push(c["x"])
    assert [(r["t0"], r["F"], r["score"], r["hits"]) for r in again] == [(r["t0"], r["F"], r["score"], r["hits"]) for r in first]
    assert all(np.array_equal(fbits(a["llr"]), fbits(b["llr"])) for a, b in zip(again, first))
    same_state(sk.dec.state(ring=True), st, "second run")
    sk.close()


def test_device_input_stays_on_the_device_until_fetched():
    """decode_raw with a device pointer and events=None only queues work; the rows fetched afterwards are the host-fed
    twin's"""
    from pysdr_amd import _lib
    c = shared(0)
    D, fs = c["D"], c["fs"]
    L = _lib.lib()
    at = int(5.1 * fs)                                                          # the call in which the 0.2 s station is emitted
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
    words = sk.dec.fetch(np.concatenate((rows, [0])))                          # runs of consecutive rows and a single one
    for k, F in enumerate(rows):
        assert np.array_equal(words[k, :2 * want["counts"][F]], want["events"][F, :2 * want["counts"][F]])
    same_state(sk.dec.state(ring=True), twin.dec.state(ring=True), "device input")
    _lib.check(L.pysdr_dev_free(0, d), "free")
    sk.close()
    twin.close()


def test_every_refusal_of_the_soft_bits():
    """before any launch and changing nothing: a frame not yet complete, one that has left the ring, a negative t0, an F
    outside the raster, too many candidates, NULL arguments"""
    from pysdr_amd import _lib
    c = shared(0)
    D, S = c["D"], c["S"]
    sk = make(c)
    L = _lib.lib()
    sk.push(c["x"][:4900 * D])                                                  # 4900 outputs: 405 steps, no frame is whole
    done, tr, nf = sk.dec.t_done, sk.dec.tr, c["nfine"]
    assert done == fo.steps_done(4900, S) == 405
    with pytest.raises(_lib.PysdrError):
        sk.dec.llr([3], [0])
    sk.push(c["x"][4900 * D:])
    done = sk.dec.t_done
    assert done == fo.steps_done(7000, S) == 580 and tr == 461
    before = sk.dec.state(ring=True)
    good = sk.dec.llr([3, nf - 1], [done - tr, done - 409])                     # the oldest frame in the ring and the newest whole one
    assert good.shape == (2, 174)
    h = sk.dec._h
    pi32, pll = C.POINTER(C.c_int32), C.POINTER(C.c_longlong)

    def call(F, t0, n=None, out=True):
        F, t0 = np.array(F, np.int32), np.array(t0, np.int64)
        o = np.full((max(len(F), 1), 174), 7.0, np.float32)
        rc = L.pysdr_ft4_llr(h, F.ctypes.data_as(pi32), t0.ctypes.data_as(pll), len(F) if n is None else n, _lib.as_pf(o) if out else None)
        assert (o == 7.0).all() or rc == 0
        return rc

    assert call([3, 3], [done - tr, done - 408]) == -5 and b"pysdr_ft4_llr" in L.pysdr_last_error()   # the second frame's last step is not in
    assert call([3], [-1]) == -5 and call([3], [0]) == -5 and call([3], [done - tr - 1]) == -5      # gone from the ring
    assert call([-1], [done - tr]) == -1 and call([3, nf], [done - tr, done - tr]) == -1
    assert call([3], [done - tr], n=-1) == -1 and call([3], [done - tr], n=4097) == -1 and call([3], [done - tr], out=False) == -1
    assert call([], [], n=0) == 0
    assert L.pysdr_ft4_llr(None, None, None, 0, None) == -1
    same_state(sk.dec.state(ring=True), before, "after the refusals")
    assert np.array_equal(fbits(sk.dec.llr([3, nf - 1], [done - tr, done - 409])), fbits(good))
    sk.close()
    # with max_out = 16 the ring holds 421 steps
    c16 = shared(0, 16)
    sk = make(c16, 16)
    for x in c16["calls"]:
        sk.dec.decode_raw(x, events=None)
    assert sk.dec.tr == 421 and sk.dec.state()["t_done"] == 580
    with pytest.raises(_lib.PysdrError):
        sk.dec.llr([3], [158])
    assert sk.dec.llr([3], [159]).shape == (1, 174)
    sk.close()
