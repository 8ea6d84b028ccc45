"""The SSTV skimmer on the GPU (pysdr_amd/csrc/sstv.hip, api_sstv.hip) against the float32 oracle of
the definition (tests/sstv_oracle.py): counts, event words, every state field, the ring and the line buffers are EQUAL
after every call.  The oracle side is fed the rows of an independent Channelizer of the same shape and prototype on the same
input, so only the decoders' own arithmetic is judged.  That the oracle reads what was sent is shown on the CPU
(tests/test_sstv_oracle.py); here the pictures are counted again so that no test passes on silence."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import sstv_oracle as so
from tests.test_gpu_psk import call_lengths, cut_rows

pytestmark = pytest.mark.gpu

MAX_OUT = 256
M, D = 16, 4
OMODES = so.MODES + [so.TINY, ("TINY2", 6, 1, 40, 4, 8.0, 1.5, 0.4, 0.0)]
# det, fs, channels, stations (channel, Hz off its centre, dB over the noise in the row bandwidth, mode, start s, pictures)
CASES = {
    "FM": (100000.0, (3, 9), ((4, 0.0, 30.0, "TINY", 0.02, 2), (9, 0.0, 25.0, "TINY2", 0.31, 1))),
    "USB": (48000.0, (3, 9), ((5, 0.0, 30.0, "TINY", 0.02, 2), (8, 60.0, 25.0, "TINY2", 0.31, 1))),
}


def modes():
    from pysdr_amd import sstv
    return sstv.MODES + (sstv.Mode("TINY", 5, 3, 32, 6, 5.0, 1.0, 0.5, 0.5, "GBR"), sstv.Mode("TINY2", 6, 1, 40, 4, 8.0, 1.5, 0.4, 0.0, "grey"))


def picture(mode, seed):
    """smooth: at most two sine periods per scan"""
    x = np.arange(mode.width)
    return np.array([[np.round(127.5 + 110.0 * np.sin(2 * np.pi * (1 + (l + j + seed) % 2) * x / mode.width + l + 2 * j + seed))
                      for j in range(mode.scans)] for l in range(mode.lines)]).astype(np.uint8)


def transmission(mode, pictures, short=False):
    """(Hz, ms) of `pictures` pictures back to back, each behind its header; short: only the header's second leader on"""
    from pysdr_amd import sstv
    t = []
    for k in range(pictures):
        t += sstv.tones(mode, picture(mode, k))[2 if short and k == 0 else 0:]
    return t + [(1900.0, 60.0)]


def scene(det, fs, n, stations, seed, floor_db=-40.0, short=False):
    """complex64 [n]: noise at floor_db in the row bandwidth fs / D and the stations"""
    from pysdr_amd import sstv
    rng = np.random.default_rng(seed)
    pn = 10 ** (floor_db / 10) * D
    x = np.sqrt(pn / 2) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for ch, off, db, name, t0, pics in stations:
        s = sstv.waveform(transmission(sstv.mode_named(name, modes()), pics, short), fs, ch * fs / M + off, det).astype(np.complex128)
        s = s[:max(0, n - int(t0 * fs))] * 10 ** ((floor_db + db) / 20)
        x[int(t0 * fs):int(t0 * fs) + len(s)] += s
    return x.astype(np.complex64)


def rows_of(fs, channels, x, det):
    """the rows of an independent channelizer"""
    from pysdr_amd import sstv
    from pysdr_amd.channelizer import Channelizer
    ch = Channelizer(fs, M, D, sstv.prototype(fs, M, D, det), channels, max_in=len(x))
    y, freqs = ch.push(x), ch.freqs.copy()
    ch.close()
    return y, freqs


def case_of(det, x, fs, channels):
    y, freqs = rows_of(fs, channels, x, det)
    for v in (x, y):
        v.setflags(write=False)
    return dict(det=det, fs=fs, channels=channels, x=x, y=y, nk=y.shape[0], fs_out=fs / D, freqs=freqs, k_first=channels[0])


@functools.lru_cache(maxsize=None)
def base(det, bad=False):
    """the case's input and the rows of an independent channelizer; computed once, never changed"""
    fs, channels, stations = CASES[det]
    n = int(2.75 * fs)
    x = scene(det, fs, n, stations, seed=700 + len(det))
    if bad:
        x = x[:int(1.5 * fs)].copy()
        x[int(1.0 * fs) + 7] = complex(np.nan, 0.25)                           # inside the first station's first picture
        x[int(1.1 * fs) + 1] = complex(-0.5, np.inf)                           # more than max_out outputs later: another call
    return case_of(det, x, fs, channels)


def oracle(c):
    return so.Oracle(c["nk"], c["fs_out"], c["det"], OMODES)


def answers(c, cuts):
    """the oracle's answer to every call (counts, words, state after it)"""
    yc = cut_rows(c["y"], cuts, D)
    o = oracle(c)
    want = []
    for r in yc:
        wc, ev = o.process(r)
        want.append((wc, ev, o.state()))
    calls, at = [], 0
    for n in cuts:
        calls.append(c["x"][at:at + n])
        at += n
    return dict(c, cuts=cuts, calls=calls, yc=yc, want=want)


@functools.lru_cache(maxsize=None)
def shared(det, max_out=MAX_OUT, bad=False):
    """the case cut into ragged calls"""
    from pysdr_amd import sstv
    c = base(det, bad)
    tile = sstv.plan(c["nk"], sstv.filter_length(c["fs_out"]), max_out, sstv.params(c["fs_out"], det, modes()))["tile"]
    cuts = call_lengths(len(c["x"]), D, tile, max_out)
    counts = [-(-sum(cuts[:k + 1]) // D) - -(-sum(cuts[:k]) // D) for k in range(len(cuts))]
    assert 0 in counts and 1 in counts and max(counts) == max_out and {tile - 1, tile, tile + 1} <= set(counts)
    return dict(answers(c, cuts), tile=tile, max_out=max_out)


def make(c, max_out=MAX_OUT, chan=None):
    from pysdr_amd.sstv import SSTV_Skimmer
    if chan is None:
        sk = SSTV_Skimmer(c["fs"], M, D, channels=c["channels"], max_in=len(c["x"]), max_out=max_out, det=c["det"], modes=modes())
    else:
        sk = SSTV_Skimmer(c["fs"], chan=chan, max_out=max_out, det=c["det"], modes=modes())
    assert (sk.nk, sk.fs_out, sk.L) == (c["nk"], c["fs_out"], so.tables(c["fs_out"])[0])
    assert sk.dec.cap == so.cap_of(max_out, so.params(c["fs_out"], c["det"], OMODES))
    return sk


def same_state(got, want, where):
    for k in so.INTS:
        assert np.array_equal(got[k], want[k]), (where, k, np.flatnonzero(got[k] != want[k])[:5], got[k], want[k])
    for k in so.FLOATS + ("ring",):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (where, k, np.argwhere(got[k] != want[k])[:5])
    assert np.array_equal(got["lines"], want["lines"]), (where, "lines", np.argwhere(got["lines"] != want["lines"])[:5])


def run_calls(c, max_out, every=1):
    """-> the records read, per row; the state is compared after every `every`-th call and the last"""
    sk = make(c, max_out)
    recs = {r: [] for r in range(c["nk"])}
    running = {}
    par_modes = so.params(c["fs_out"], c["det"], OMODES)["modes"]
    for j, (x, r, (wc, wev, wst)) in enumerate(zip(c["calls"], c["yc"], c["want"])):
        got = sk.dec.decode_raw(x, events="all")
        assert got["n_out"] == r.shape[1], j
        assert np.array_equal(got["counts"], wc), (j, np.flatnonzero(got["counts"] != wc)[:5], got["counts"], wc)
        for row in np.flatnonzero(wc):
            assert list(got["events"][row, :wc[row]]) == wev[row], (j, row)
            new = so.unpack(wev[row], par_modes, running.get(row))
            for rec in new:
                if rec[1] == "start":
                    running[row] = rec[2]
            recs[row] += new
        if j % every == 0 or j == len(c["calls"]) - 1:
            same_state(sk.dec.state(), wst, j)
    sk.close()
    return recs


def pictures_of(recs):
    """a row's records -> [(mode index, uint8 [lines][scans][width])] of the pictures that ended"""
    out, cur = [], None
    for rec in recs:
        if rec[1] == "start":
            cur = (rec[2], [])
        elif rec[1] == "line":
            assert rec[2] == len(cur[1])
            cur[1].append(rec[3])
        else:
            out.append((cur[0], np.array(cur[1])))
    return out


def all_read(c, recs):
    """every station's pictures are read on its home row, close to what was sent"""
    names = [m[0] for m in OMODES]
    for ch, off, db, name, t0, pics in CASES[c["det"]][2]:
        got = pictures_of(recs[ch - c["k_first"]])
        mode = next(m for m in modes() if m.name == name)
        assert [names[k] for k, _ in got] == [name] * pics, (ch, [names[k] for k, _ in got])
        for k, (_, img) in enumerate(got):
            err = np.abs(img.astype(int) - picture(mode, k).astype(int))
            assert err.mean() < 6.0, (ch, k, err.mean())


@pytest.mark.parametrize("det", ("FM", "USB"))
def test_every_call_equals_the_oracle(det):
    """ragged cuts: 1-sample calls, calls that complete no output, calls that end on the kernel's tile boundary and one
    output to either side of it, calls of max_out; 9 rows (one workgroup and one row of the next), two rows with
    different modes at once, two pictures back to back on one row"""
    c = shared(det)
    all_read(c, run_calls(c, MAX_OUT, every=3))


@pytest.mark.parametrize("det", ("FM", "USB"))
def test_calls_of_16_outputs_shorter_than_the_lag(det):
    """one row, the header from its second leader on and a TINY2 picture: VIS, anchor, every pixel and the end are decided
    in calls far shorter than the lag and the anchor's window"""
    fs = CASES[det][0]
    st = ((4, 0.0, 30.0, "TINY2", 0.005, 1),)
    n = int((0.005 + 0.6 + 0.102 + 0.09) * fs)
    c = case_of(det, scene(det, fs, n, st, seed=31, short=True), fs, (4, 1))
    cuts = [16 * D] * (n // (16 * D)) + ([n % (16 * D)] if n % (16 * D) else [])
    c = answers(c, cuts)
    assert so.params(c["fs_out"])["lag"] > 16
    recs = run_calls(c, 16, every=40)
    got = pictures_of(recs[0])
    assert len(got) == 1 and got[0][1].shape == (4, 1, 40)


@pytest.mark.parametrize("det", ("FM", "USB"))
def test_a_picture_ends_in_the_call_s_last_output(det):
    """calls of 4096 outputs, cut so that one ends with the output that completes the first station's last line"""
    c = base(det)
    wc, ev = oracle(c).process(c["y"])
    home = CASES[det][2][0][0] - c["k_first"]
    ends = [rec[0] for rec in so.unpack(ev[home], so.params(c["fs_out"], det, OMODES)["modes"]) if rec[1] == "end"]
    assert len(ends) == 2
    n, head = len(c["x"]), ((ends[0] + 1) % 4096) * D
    cuts = [head] + [4096 * D] * ((n - head) // (4096 * D)) + [(n - head) % (4096 * D)]
    c = answers(c, cuts)
    last = [j for j, (wc, wev, _) in enumerate(c["want"]) if wc[home] and (int(wev[home][-2]) & 0xFFFFFFFF) >> 12 == c["yc"][j].shape[1] - 1]
    assert last, "no call ends with the picture"
    all_read(c, run_calls(c, 4096))


@pytest.mark.parametrize("det", ("FM", "USB"))
def test_the_whole_stream_through_push(det):
    """push cuts the stream itself; records, images and pictures are what the oracle rebuilds"""
    c = base(det)
    sk = make(c, 4096)
    ev = sk.push(c["x"])
    o = oracle(c)
    want, running = [], {}
    for at in range(0, c["y"].shape[1], 4096):
        wc, wev = o.process(c["y"][:, at:at + 4096])
        for row in np.flatnonzero(wc):
            for rec in so.unpack(wev[row], o.par["modes"], running.get(row)):
                if rec[1] == "start":
                    running[row] = rec[2]
                want.append((at + rec[0], int(row)) + rec[1:])
    want.sort(key=lambda e: (e[0], e[1]))
    names = [m[0] for m in OMODES]
    assert len(ev) == len(want) and len(want) >= 3 * 2 + 16
    for a, b in zip(ev, want):
        assert a[:3] == b[:3]
        if a[2] == "start":
            assert a[3] == names[b[3]] and a[4] == b[4] and np.float32(a[5]) == np.float32(b[5]) and a[6] == b[6]
        elif a[2] == "line":
            assert a[3] == b[3] and np.array_equal(a[4], b[4])
        else:
            assert a[3] == b[3]
    by_row = {}
    for rec in want:
        by_row.setdefault(rec[1], []).append(rec[1:])
    for row, recs in by_row.items():
        pics = pictures_of([(0,) + r[1:] for r in recs])
        mine = [(names.index(m.name), img) for r, m, img in sk.pictures if r == row]
        assert len(pics) == len(mine) and all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(pics, mine))
    all_read(c, {r: [(0,) + rec[1:] for rec in by_row.get(r, [])] for r in range(c["nk"])})
    from pysdr_amd import sstv
    home = CASES[det][2][0][0] - c["k_first"]
    rgb = sstv.to_rgb(sk.mode_of[home], sk.images[home])
    assert rgb.shape == (6, 32, 3) and np.array_equal(rgb[..., 1], sk.images[home][:, 0]) and np.array_equal(rgb[..., 0], sk.images[home][:, 2])
    same_state(sk.dec.state(), o.state(), "end")
    sk.close()


def test_refused_calls_change_nothing():
    from pysdr_amd import _lib
    c = shared("FM")
    sk = make(c)
    L = _lib.lib()
    n1 = 27000 * D + 3                                                        # inside the first picture
    sk.push(c["x"][:n1])
    before = sk.dec.state()
    assert (before["phase"] == 2).any()
    x = np.array(c["x"][n1:n1 + (MAX_OUT + 1) * D])
    n_out = C.c_int(-1)
    assert sk.dec.chan.n_out_for(len(x)) == MAX_OUT + 1
    h, p = sk.dec._h, C.c_void_p(x.ctypes.data)
    rc = L.pysdr_sstv_process(h, p, len(x), 0, C.byref(n_out), None, None, 0)
    assert rc == -5 and n_out.value == 0 and b"max_out" in L.pysdr_last_error()
    cap = sk.dec.cap
    ev = np.zeros((c["nk"], cap - 1), np.int32)
    cnt = np.zeros(c["nk"], np.int32)
    pi32 = C.POINTER(C.c_int32)
    assert L.pysdr_sstv_process(h, p, 64, 0, C.byref(n_out), cnt.ctypes.data_as(pi32), ev.ctypes.data_as(pi32), cap - 1) == -5
    assert b"ev_pitch" in L.pysdr_last_error()
    assert L.pysdr_sstv_process(h, p, len(c["x"]) + 1, 0, C.byref(n_out), None, None, 0) == -5
    assert L.pysdr_sstv_process(h, None, 16, 0, C.byref(n_out), None, None, 0) == -1
    assert L.pysdr_sstv_process(h, p, -1, 0, C.byref(n_out), None, None, 0) == -1
    assert L.pysdr_sstv_process(h, p, 16, 0, None, None, None, 0) == -1
    rows = np.array([0, c["nk"]], np.int32)
    big = np.zeros((2, cap), np.int32)
    assert L.pysdr_sstv_fetch(h, _lib.as_pi(rows), 2, big.ctypes.data_as(pi32), cap) == -1
    assert L.pysdr_sstv_fetch(h, _lib.as_pi(rows), 1, big.ctypes.data_as(pi32), cap - 1) == -5
    same_state(sk.dec.state(), before, "after the refused calls")
    # the stream did not advance: the rest equals an undisturbed twin's
    twin = make(c)
    twin.push(c["x"][:n1])
    rest = c["x"][n1:]
    got, want = sk.push(rest), twin.push(rest)
    assert len(got) == len(want) >= 10 and all(a[:4] == b[:4] for a, b in zip(got, want))
    same_state(sk.dec.state(), twin.dec.state(), "rest")
    sk.close()
    twin.close()


def test_a_call_without_outputs_changes_no_state_and_has_no_events():
    c = shared("USB")
    sk = make(c)
    sk.push(c["x"][:13000 * D + 1])                                           # inside the first picture
    before = sk.dec.state()
    assert (before["phase"] == 2).any() and before["lines"].any()
    got = sk.dec.decode_raw(c["x"][13000 * D + 1:13001 * D], events="all")    # ends one sample short of the next output
    assert got["n_out"] == 0 and not got["counts"].any()
    assert not sk.dec.fetch([0, 1, 2, 5]).any()                               # nothing to fetch after it
    same_state(sk.dec.state(), before, "empty call")
    sk.close()


@pytest.mark.parametrize("det", ("FM", "USB"))
def test_one_nan_and_one_inf_blank_their_windows_and_nothing_else(det):
    """The rows of a channelizer on the same input carry each non-finite sample for as long as its window holds it; the
    decoders blank the lag products whose windows reach such a row sample (that it is exactly L + 1 per row sample, L + 2
    behind the discriminator, is shown on the oracle and in tests/sstv_plan), so events and state still equal the
    oracle's, and once the windows have passed the lag products are those of the finite rows again: the picture goes on"""
    c = shared(det, MAX_OUT, True)
    assert not np.isfinite(c["y"]).all() and np.isfinite(c["y"][:, -500:]).all()
    bad_calls = [j for j, r in enumerate(c["yc"]) if not np.isfinite(r).all()]
    assert len(bad_calls) >= 2
    recs = run_calls(c, MAX_OUT, every=1)
    home = CASES[det][2][0][0] - c["k_first"]
    lines = [rec for rec in recs[home] if rec[1] == "line"]
    assert len(lines) >= 6                                                    # the first picture ended, the row free-ran through the blanks
    o = oracle(c)
    o.process(c["y"])
    st = o.state()
    assert np.isfinite(st["ring"]).all() and all(np.isfinite(st[k]).all() for k in so.FLOATS)


def test_reset_repeats_the_first_run():
    c = shared("FM")
    sk = make(c)
    x = c["x"][:int(1.6 * c["fs"])]
    first = sk.push(x)
    st = sk.dec.state()
    assert len(first) >= 8 and len(sk.pictures) >= 1
    sk.reset()
    z = sk.dec.state()
    assert (z["mode"] == -1).all() and not any(z[k].any() for k in so.INTS if k != "mode") and not any(z[k].any() for k in so.FLOATS)
    assert not z["ring"].any() and not z["lines"].any() and not sk.images and not sk.pictures and sk.chan.n_in == 0
    again = sk.push(x)
    assert len(again) == len(first) and all(a[:4] == b[:4] and np.array_equal(a[-1], b[-1]) for a, b in zip(again, first))
    same_state(sk.dec.state(), st, "second run")
    sk.close()


def test_device_input_stays_on_the_device_until_fetched():
    """decode_raw with a device pointer and events=None only queues work; the rows fetched afterwards are the host-fed
    twin's"""
    from pysdr_amd import _lib
    c = base("FM")
    fs = c["fs"]
    L = _lib.lib()
    at = int(0.9 * fs)
    x = np.array(c["x"][at:at + 4096 * D])                                   # the first station's anchor and first lines are in it
    head = c["x"][:at]
    sk, twin = make(c, 4096), make(c, 4096)
    sk.push(head)
    twin.push(head)
    d = C.c_void_p()
    _lib.check(L.pysdr_dev_alloc(0, x.nbytes, C.byref(d)), "alloc")
    _lib.check(L.pysdr_dev_upload(0, d, C.c_void_p(x.ctypes.data), x.nbytes), "upload")
    got = sk.dec.decode_raw(d.value, len(x), on_device=True, events=None)
    sk.sync()
    want = twin.dec.decode_raw(x, events="all")
    assert got["n_out"] == want["n_out"] == 4096 and got["counts"] is None and want["counts"].sum() > 0
    rows = np.flatnonzero(want["counts"])
    words = sk.dec.fetch(np.concatenate((rows, [0])))                        # runs of consecutive rows and a single one
    for k, row in enumerate(rows):
        assert np.array_equal(words[k, :want["counts"][row]], want["events"][row, :want["counts"][row]])
    same_state(sk.dec.state(), twin.dec.state(), "device input")
    _lib.check(L.pysdr_dev_free(0, d), "free")
    sk.close()
    twin.close()


def test_a_fine_channelizer_is_adopted():
    """``chan=`` as a FineChannelizer: fs = 1.6 MS/s, rows at 25 kHz 6.25 kHz apart (M2 / D2 = 4), the shape fine.shape gives
    there; one FM station, read on its home row and equal to the oracle on the fine channelizer's own rows."""
    from pysdr_amd import fine, sstv
    fs, fs_out = 1600000.0, 25000.0
    M1, D1, M2, D2 = fine.shape(fs, fs_out, 4)
    f0 = 100000.0
    band = (f0 - 2 * 6250.0, f0 + 2 * 6250.0)
    g_first, ng = fine.channels_for(band, fs, M1, D1, M2)
    h1, h2 = fine.prototype1(fs, M1, D1, M2), sstv.prototype(fs / D1, M2, D2)
    tiny = sstv.mode_named("TINY", modes())
    s = sstv.waveform(transmission(tiny, 1), fs, f0, "FM")
    n = len(s) + int(0.02 * fs)
    rng = np.random.default_rng(91)
    x = 0.01 * np.sqrt(fs / fs_out / 2) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x[500:500 + len(s)] += 0.3 * s
    x = x.astype(np.complex64)
    twin = fine.FineChannelizer(fs, M1, M2, D1, D2, h1, h2, (g_first, ng), max_in=len(x))
    y, freqs = twin.push(x), twin.freqs.copy()
    twin.close()
    sk = sstv.SSTV_Skimmer(fs, chan=fine.FineChannelizer(fs, M1, M2, D1, D2, h1, h2, (g_first, ng), max_in=len(x)), max_out=4096, modes=modes())
    assert sk.fs_out == fs_out and sk.nk == ng == 5 and np.allclose(sk.freqs, freqs)
    ev = sk.push(x)
    o = so.Oracle(ng, fs_out, "FM", OMODES)
    for at in range(0, y.shape[1], 4096):
        o.process(y[:, at:at + 4096])
    home = int(np.argmin(np.abs(freqs - f0)))
    mine = [img for r, m, img in sk.pictures if r == home]
    assert len(mine) == 1 and np.abs(mine[0].astype(int) - picture(tiny, 0).astype(int)).mean() < 6.0
    assert [e[2] for e in ev if e[1] == home] == ["start"] + ["line"] * 6 + ["end"]
    same_state(sk.dec.state(), o.state(), "end")
    sk.close()
