"""The RDS skimmer on the GPU (pysdr_amd/csrc/rds.hip, api_rds.hip) against the float32 oracle of the
definition (tests/rds_oracle.py): counts, event words, every state field and the z ring are EQUAL after every call.  The
oracle side is fed the rows of an independent Channelizer of the same shape and prototype on the same input, so only the
decoders' own arithmetic is judged.  That the oracle reads every planted group is shown on the CPU
(tests/test_rds_oracle.py); here the groups are counted again so that no test passes on silence."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import rds_oracle as ro
from tests.test_gpu_psk import call_lengths, cut_rows

pytestmark = pytest.mark.gpu

MAX_OUT = 256
# (fs, M, D, channels, seconds, stations (channel, Hz off its centre, C/N dB in the row bandwidth, start s, name, text, version B))
# Where the rows lie closer than a station is wide (57 kHz apart at 228 kHz rows, 128 kHz at 512 kHz rows) the second
# station comes on when the first has gone off: two FM stations on one frequency are not what is tested here.
SHAPES = [
    (912000.0, 16, 4, (2, 3), 1.22, ((2, 10e3, 23.0, 0.02, "LOW EDGE", "a text", False), (4, -20e3, 40.0, 0.63, "VERSIONB", "bee", True))),
    (1600000.0, 16, 4, (14, 4), 0.78, ((14, -15e3, 20.0, 0.01, "WRAPS   ", "Hello RDS", False), (1, 25e3, 30.0, 0.12, "MIDSTRM ", "mid", True))),
    (2048000.0, 16, 4, (5, 2), 1.22, ((5, -25e3, 25.0, 0.02, "HIGHEDGE", "c text", False), (6, 10e3, 40.0, 0.63, "SECOND  ", "second", False))),
    (2000000.0, 20, 5, None, 0.78, ((3, 10e3, 20.0, 0.01, "KSON97.3", "Hello RDS", False), (11, -25e3, 40.0, 0.10, "PRIME B ", "yz!", True),
                                    (17, 20e3, 30.0, 0.14, "THIRD   ", "three", False))),
]
IDS = ["912k-16-2+3", "1600k-16-14+4", "2048k-16-5+2", "2000k-20-all"]


def groups_of(k, name, text, vb):
    from pysdr_amd import rds
    pi = 0x54A8 + 1000 + k
    return rds.ps_groups(pi, name, version_b=vb) + rds.rt_groups(pi, text, version_b=vb)


def planted(i):
    """[(home row, groups as the skimmer's words)]"""
    fs, M, D, channels, secs, stations = SHAPES[i]
    k_first = 0 if channels is None else channels[0]
    return [((ch - k_first) % M, [tuple(g) + (int(vb),) for g in groups_of(10 * i + k, name, text, vb)])
            for k, (ch, off, cn, t0, name, text, vb) in enumerate(stations)]


def make_input(i, bad=False):
    from pysdr_amd import rds
    fs, M, D, channels, secs, stations = SHAPES[i]
    n = int(secs * fs)
    sts = [(groups_of(10 * i + k, name, text, vb), ch * fs / M + off, cn, int(t0 * fs)) for k, (ch, off, cn, t0, name, text, vb) in enumerate(stations)]
    x = ro.scene(fs, n, sts, fs / D, rds.waveform, seed=700 + i)
    if bad:
        x[int(0.05 * fs) + 7] = complex(np.nan, 0.25)                         # inside the first station's first group
        x[int(0.09 * fs) + 1] = complex(-0.5, np.inf)                         # more than max_out outputs later: another call
    return x


def rows_of(fs, M, D, channels, x):
    """the rows of an independent channelizer"""
    from pysdr_amd import rds
    from pysdr_amd.channelizer import Channelizer
    ch = Channelizer(fs, M, D, rds.prototype(fs, M, D), channels, max_in=len(x))
    y, freqs = ch.push(x), ch.freqs.copy()
    ch.close()
    return y, freqs


@functools.lru_cache(maxsize=None)
def base(i, bad=False):
    """case i: the input and the rows of an independent channelizer; computed once, never changed"""
    fs, M, D, channels, secs, stations = SHAPES[i]
    nk = M if channels is None else channels[1]
    x = make_input(i, bad)
    y, freqs = rows_of(fs, M, D, channels, x)
    for v in (x, y):
        v.setflags(write=False)
    assert y.shape[0] == nk
    return dict(i=i, fs=fs, M=M, D=D, channels=channels, x=x, y=y, nk=nk, nd=nk * 16, fs_out=fs / D, freqs=freqs)


@functools.lru_cache(maxsize=None)
def shared(i, max_out=MAX_OUT, bad=False):
    """case i cut into ragged calls, and the oracle's answer to every call (counts, words, state after it)"""
    from pysdr_amd import rds
    c = base(i, bad)
    tile = rds.plan(c["nk"], rds.pulse_length(c["fs_out"]), max_out, rds.params(c["fs_out"]))["tile"]
    cuts = call_lengths(len(c["x"]), c["D"], tile, max_out)
    yc = cut_rows(c["y"], cuts, c["D"])
    counts = [r.shape[1] for r in yc]
    assert 0 in counts and 1 in counts and max(counts) == max_out and any(0 < n < c["D"] for n in cuts)
    if max_out >= tile + 1:
        assert {tile - 1, tile, tile + 1} <= set(counts)
    want = ro.Oracle(c["nk"], c["fs_out"]).replay(c["y"], counts)
    calls, at = [], 0
    for n in cuts:
        calls.append(c["x"][at:at + n])
        at += n
    return dict(c, cuts=cuts, calls=calls, yc=yc, want=want, tile=tile, max_out=max_out)


def make(c, max_out=MAX_OUT):
    from pysdr_amd.rds import RDS_Skimmer
    sk = RDS_Skimmer(c["fs"], c["M"], c["D"], channels=c["channels"], max_in=len(c["x"]), max_out=max_out)
    assert (sk.nk, sk.ndec, sk.fs_out, sk.L) == (c["nk"], c["nd"], c["fs_out"], ro.tables(c["fs_out"])[0])
    return sk


def run_calls(c, max_out, check=None):
    """-> the groups read, as (row, words); counts, words and the state are compared after every call"""
    sk = make(c, max_out)
    assert sk.dec.cap == ro.cap_of(max_out, ro.word19(c["fs_out"]))
    got_groups = []
    for j, (x, r, (wc, wev, wst)) in enumerate(zip(c["calls"], c["yc"], c["want"])):
        got = sk.dec.decode_raw(x, events="all")
        assert got["n_out"] == r.shape[1], j
        assert np.array_equal(got["counts"], wc), (j, np.flatnonzero(got["counts"] != wc)[:5])
        for d in np.flatnonzero(wc):
            assert list(got["events"][d, :wc[d]]) == wev[d], (j, d)
            got_groups += [(d // 16, w) for _, _, w in ro.unpack(wev[d])]
        ro.same_state(sk.dec.state(), wst, j)
        if check is not None:
            check(j, wst)
    sk.close()
    return got_groups


def all_read(i, got, least=3):
    for row, groups in planted(i):
        for g in groups:
            assert got.count((row, g)) >= least, (row, g, got.count((row, g)))
    sent = {g for _, groups in planted(i) for g in groups}
    assert {w for _, w in got} == sent                                        # and no group that was not sent


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_every_call_equals_the_oracle(i):
    """max_out = 256, so that chips, bits and groups straddle calls; ragged cuts: 1-sample calls, calls shorter than D,
    calls that complete no output, calls of max_out"""
    all_read(i, run_calls(shared(i), MAX_OUT))


@pytest.mark.parametrize("i", (1, 3), ids=[IDS[1], IDS[3]])
def test_calls_of_several_tiles_equal_the_oracle(i):
    """max_out = 4096: calls that end on the kernel's tile boundary and one output to either side of it, calls of four tiles"""
    all_read(i, run_calls(shared(i, 4096), 4096))


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_the_whole_stream_through_push(i):
    """push cuts the stream itself; the groups are the oracle skimmer's, one record per planted group, on its home row;
    every station is listed with its name and its text, once each"""
    c = base(i)
    sk = make(c, 65536)
    ev = sk.push(c["x"]) + sk.flush()
    ref = ro.Skimmer(c["nk"], c["fs"], c["fs_out"], c["freqs"], max_out=65536)
    want = ref.push(c["y"], flush=True)
    assert sk.groups == want == ref.groups
    assert [(m, row, w) for m, row, kind, w in ev if kind == "group"] == [(m, row, w) for m, row, w, _ in want]
    from pysdr_amd import packet
    near = packet.near_rows(c["freqs"], c["fs"], c["fs_out"])
    home = {g: row for row, groups in planted(i) for g in groups}
    assert sorted(w for _, _, w, _ in want) == sorted(home)                   # one record per planted group
    assert all(row in near[home[w]] for _, row, w, _ in want)                 # on its home row or the one beside it
    assert all(bin(mask).count("1") >= 3 for _, _, _, mask in sk.groups)
    raw = ro.Oracle(c["nk"], c["fs_out"]).process(c["y"])[0].reshape(c["nk"], 16).sum(axis=1)
    if i != 2:                                                               # (case 2 has no row but the two home rows)
        assert (raw > 0).sum() > len({row for row, _ in planted(i)})          # neighbour rows read the stations too: one record all the same
    fs, M, D, channels, secs, stations = SHAPES[i]
    texts = sorted((kind, v) for _, row, kind, v in ev if kind in ("ps", "rt"))
    assert texts == sorted(q for st in stations for q in (("ps", st[4]), ("rt", st[5])))
    listed = {pi: (row, s) for row in range(sk.nk) for pi, s in sk.stations[row].items()}
    assert len(listed) == sum(len(s) for s in sk.stations) == len(stations) == len(sk.band_list())
    for (row, groups), st in zip(planted(i), stations):
        at, s = listed[groups[0][0]]
        assert at in near[row] and (s.ps, s.rt) == (st[4], st[5]) and sum(s.rows.values()) == len(groups)
    ro.same_state(sk.dec.state(), ref.o.state(), "end")
    sk.close()


def test_refused_calls_change_nothing():
    from pysdr_amd import _lib
    c = shared(1)
    D = c["D"]
    sk = make(c)
    L = _lib.lib()
    n1 = 100000 * D + 3
    sk.push(c["x"][:n1])
    before = sk.dec.state()
    assert before["regs"].any() and before["ring"].any()
    x = np.array(c["x"][n1:n1 + (MAX_OUT + 1) * D])
    n_out = C.c_int(-1)
    assert sk.dec.chan.n_out_for(len(x)) == MAX_OUT + 1
    h, p = sk.dec._h, C.c_void_p(x.ctypes.data)
    rc = L.pysdr_rds_process(h, p, len(x), 0, C.byref(n_out), None, None, 0)
    assert rc == -5 and n_out.value == 0 and b"max_out" in L.pysdr_last_error()
    cap = sk.dec.cap
    ev = np.zeros((c["nd"], cap - 1), np.int32)
    cnt = np.zeros(c["nd"], np.int32)
    pi32 = C.POINTER(C.c_int32)
    assert L.pysdr_rds_process(h, p, 64, 0, C.byref(n_out), cnt.ctypes.data_as(pi32), ev.ctypes.data_as(pi32), cap - 1) == -5
    assert b"ev_pitch" in L.pysdr_last_error()
    assert L.pysdr_rds_process(h, p, len(c["x"]) + 1, 0, C.byref(n_out), None, None, 0) == -5
    assert L.pysdr_rds_process(h, None, 16, 0, C.byref(n_out), None, None, 0) == -1
    assert L.pysdr_rds_process(h, p, -1, 0, C.byref(n_out), None, None, 0) == -1
    assert L.pysdr_rds_process(h, p, 16, 0, None, None, None, 0) == -1
    rows = np.array([0, c["nd"]], np.int32)
    big = np.zeros((2, cap), np.int32)
    assert L.pysdr_rds_fetch(h, _lib.as_pi(rows), 2, big.ctypes.data_as(pi32), cap) == -1
    assert L.pysdr_rds_fetch(h, _lib.as_pi(rows), 1, big.ctypes.data_as(pi32), cap - 1) == -5
    ro.same_state(sk.dec.state(), before, "after the refused calls")
    # the stream did not advance: the rest equals an undisturbed twin's
    twin = make(c)
    twin.push(c["x"][:n1])
    rest = c["x"][n1:]
    got = sk.push(rest) + sk.flush()
    assert got == twin.push(rest) + twin.flush() and sum(1 for e in got if e[2] == "group") >= 6
    ro.same_state(sk.dec.state(), twin.dec.state(), "rest")
    sk.close()
    twin.close()


def test_a_call_without_outputs_changes_no_state_and_has_no_events():
    c = shared(1)
    D = c["D"]
    sk = make(c)
    groups = [e for e in sk.push(c["x"][:150000 * D + 1]) if e[2] == "group"]
    before = sk.dec.state()
    assert before["regs"].any() and before["ring"].any() and len(groups) >= 2
    got = sk.dec.decode_raw(c["x"][150000 * D + 1:150001 * D], events="all")  # ends one sample short of the next output
    assert got["n_out"] == 0 and not got["counts"].any()
    assert not sk.dec.fetch([0, 1, 2, 5]).any()                               # nothing to fetch after it
    ro.same_state(sk.dec.state(), before, "empty call")
    sk.close()


def test_one_nan_and_one_inf_zero_their_discriminator_outputs_and_nothing_else():
    """The rows of a channelizer on the same input carry each non-finite sample for as long as its window holds it; the
    discriminator gives 0 there (that it is exactly two products per row sample, and that every other product is bit for
    bit what it was, is shown on the oracle, tests/test_rds_oracle.py), so events and state still equal the oracle's, the
    z ring stays finite, and the groups behind are read."""
    c = shared(1, MAX_OUT, True)
    assert not np.isfinite(c["y"]).all() and np.isfinite(c["y"][:, -1000:]).all()
    bad_calls = [j for j, r in enumerate(c["yc"]) if not np.isfinite(r).all()]
    assert len(bad_calls) >= 2 and bad_calls[-1] - bad_calls[0] > 10

    def finite(j, st):
        assert np.isfinite(st["ring"]).all(), j

    got = run_calls(c, MAX_OUT, check=finite)
    (row, groups), _ = planted(1)
    assert all(got.count((row, g)) >= 3 for g in groups[2:])                  # the groups behind the two samples


def test_reset_repeats_the_first_run():
    c = shared(1)
    sk = make(c, 4096)
    x = c["x"][:int(0.5 * c["fs"])]
    first = sk.push(x)
    st = sk.dec.state()
    groups, names = list(sk.groups), [sorted(s) for s in sk.stations]
    assert sum(1 for e in first if e[2] == "group") >= 5 and any(e[2] == "ps" for e in first)
    sk.reset()
    z = sk.dec.state()
    assert not z["regs"].any() and not z["chips"].any() and not z["ring"].any()
    assert not sk.groups and not any(sk.stations) and sk.chan.n_in == 0
    assert sk.push(x) == first and sk.groups == groups and [sorted(s) for s in sk.stations] == names
    ro.same_state(sk.dec.state(), st, "second run")
    sk.close()


def test_device_input_stays_on_the_device_until_fetched():
    """decode_raw with a device pointer and events=None only queues work; the rows fetched afterwards are the host-fed
    twin's"""
    from pysdr_amd import _lib
    c = base(1)
    D, fs = c["D"], c["fs"]
    L = _lib.lib()
    at = int(0.06 * fs)
    x = np.array(c["x"][at:at + 65536 * D])                                  # the first station's first group ends in it
    head = c["x"][:at]
    sk, twin = make(c, 65536), make(c, 65536)
    sk.push(head)
    twin.push(head)
    d = C.c_void_p()
    _lib.check(L.pysdr_dev_alloc(0, x.nbytes, C.byref(d)), "alloc")
    _lib.check(L.pysdr_dev_upload(0, d, C.c_void_p(x.ctypes.data), x.nbytes), "upload")
    got = sk.dec.decode_raw(d.value, len(x), on_device=True, events=None)
    sk.sync()
    want = twin.dec.decode_raw(x, events="all")
    assert got["n_out"] == want["n_out"] == 65536 and got["counts"] is None and want["counts"].sum() > 0
    rows = np.flatnonzero(want["counts"])
    words = sk.dec.fetch(np.concatenate((rows, [0])))                        # runs of consecutive rows and a single one
    for k, dcd in enumerate(rows):
        assert np.array_equal(words[k, :want["counts"][dcd]], want["events"][dcd, :want["counts"][dcd]])
    ro.same_state(sk.dec.state(), twin.dec.state(), "device input")
    _lib.check(L.pysdr_dev_free(0, d), "free")
    sk.close()
    twin.close()


def test_a_fine_channelizer_is_adopted():
    """``chan=`` as a FineChannelizer: fs = 16 MS/s, rows at 250 kHz 62.5 kHz apart (M2 / D2 = 4), the shape fine.shape gives
    there; one station, four groups, read once each and equal to the oracle on the fine channelizer's own rows.  (The
    station is made at 2 MS/s and its phase interpolated to 16 MS/s: a test signal's privilege.)"""
    from pysdr_amd import fine, rds
    fs, fs_out = 16000000.0, 250000.0
    M1, D1, M2, D2 = fine.shape(fs, fs_out, 4)
    f0 = 1000000.0
    g_first, ng = fine.channels_for((f0 - 2 * 62500.0, f0 + 2 * 62500.0), fs, M1, D1, M2)
    h1, h2 = fine.prototype1(fs, M1, D1, M2), rds.prototype(fs / D1, M2, D2)
    groups = rds.ps_groups(rds.pi_of("KFMB"), "KFMB-FM ")
    low = np.angle(rds.waveform(groups, fs / 8, 0.0).astype(np.complex128))
    ph = np.interp(np.arange(8 * len(low)) / 8.0, np.arange(len(low)), np.unwrap(low))
    s = np.exp(1j * (ph + 2 * np.pi * (f0 + 10e3) * np.arange(len(ph)) / fs))
    rng = np.random.default_rng(91)
    n = len(s) + 16000
    x = np.sqrt(1e-4 * fs / fs_out / 2) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))   # 30 dB C/N in a row
    x[8000:8000 + len(s)] += 10 ** (-10 / 20) * s
    x = x.astype(np.complex64)
    twin = fine.FineChannelizer(fs, M1, M2, D1, D2, h1, h2, (g_first, ng), max_in=len(x))
    y, freqs = twin.push(x), twin.freqs.copy()
    twin.close()
    sk = rds.RDS_Skimmer(fs, chan=fine.FineChannelizer(fs, M1, M2, D1, D2, h1, h2, (g_first, ng), max_in=len(x)), max_out=65536)
    assert sk.fs_out == fs_out and sk.nk == ng == 5 and np.allclose(sk.freqs, freqs) and sk.L == 421
    ev = sk.push(x) + sk.flush()
    ref = ro.Skimmer(ng, fs, fs_out, freqs, max_out=65536)
    assert sk.groups == ref.push(y, flush=True)
    assert [w for _, _, w, _ in sk.groups] == [tuple(g) + (0,) for g in groups]
    assert [(kind, v) for _, _, kind, v in ev if kind != "group"] == [("ps", "KFMB-FM ")] and sk.band_list()[0][2:] == ("KFMB", "KFMB-FM ")
    ro.same_state(sk.dec.state(), ref.o.state(), "end")
    sk.close()
