"""The packet skimmer on the GPU (pysdr_amd/csrc/pkt.hip, api_pkt.hip) against the float32 oracle of
the definition (tests/pkt_oracle.py): counts, event words, every state field and the frame buffers are EQUAL after every
call.  The oracle side is fed the rows of an independent Channelizer of the same shape and prototype on the same input, so
only the decoders' own arithmetic is judged.  That the oracle reads every planted frame is shown on the CPU
(tests/test_pkt_oracle.py); here the frames are counted again so that no test passes on silence."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import pkt_oracle as po
from tests.test_gpu_psk import call_lengths, cut_rows

pytestmark = pytest.mark.gpu

SECONDS = 2.0
MAX_OUT = 256
# (fs, M, D, channels, stations (channel, Hz off its centre, C/N dB in the row bandwidth, 2200 Hz re 1200 Hz, start s, frames))
SHAPES = [
    (200000.0, 16, 8, (3, 4), ((3, 300.0, 20.0, 1.0, 0.03, (0, 1)), (5, -500.0, 12.0, 0.55, 0.40, (2,)), (6, 0.0, 30.0, 1.83, 1.00, (3,)))),
    (192000.0, 16, 8, (12, 9), ((13, -700.0, 25.0, 1.0, 0.03, (4,)), (0, 100.0, 12.0, 1.83, 0.50, (5,)), (3, 600.0, 30.0, 0.55, 1.00, (6, 7)))),
    (192000.0, 20, 10, None, ((2, 0.0, 30.0, 1.0, 0.03, (8,)), (11, 400.0, 15.0, 0.55, 0.45, (9,)), (19, -400.0, 20.0, 1.83, 1.00, (10,)))),
    (200000.0, 32, 8, (5, 9), ((8, 0.0, 20.0, 1.0, 0.03, (11,)), (11, 500.0, 30.0, 1.83, 0.55, (12,)), (6, -300.0, 12.0, 0.55, 1.05, (13,)))),
]
IDS = ["200k-16-3+4", "192k-16-12+9", "192k-20-all", "200k-32-5+9"]


def the_frame(k):
    from pysdr_amd import packet
    info = (f"!4903.50N/07201.75W-Test {k:06d} " + "abcdefghijklmnopqrstuvwxyz" * 2)[:22 + 3 * (k % 5)]
    if k in (1, 7):                                                           # the shortest frame, second of a pair that shares a flag
        return packet.ax25_frame("APRS", f"N0CALL-{k}", pid=None)
    return packet.ax25_frame("APRS", f"N0CALL-{k % 16}", ("WIDE1-1*", "WIDE2-1"), info)


def make_input(i, bad=False):
    from pysdr_amd import packet
    fs, M, D, channels, stations = SHAPES[i]
    n = int(SECONDS * fs)
    wf = functools.partial(packet.waveform, flags=(12, 2))
    sts = [([the_frame(k) for k in fr], ch * fs / M + off, cn, bal, int(t0 * fs)) for ch, off, cn, bal, t0, fr in stations]
    x = po.scene(fs, n, sts, fs / D, wf, seed=500 + i)
    if bad:
        x[int(0.2 * fs) + 7] = complex(np.nan, 0.25)                          # inside the first station's first frame
        x[int(0.33 * fs) + 1] = complex(-0.5, np.inf)                         # more than max_out outputs later: another call
    return x


def shape_of(i):
    fs, M, D, channels, stations = SHAPES[i]
    nk = M if channels is None else channels[1]
    k_first = 0 if channels is None else channels[0]
    return fs, M, D, channels, nk, k_first


def home_rows(i):
    fs, M, D, channels, nk, k_first = shape_of(i)
    return {(ch - k_first) % M: [the_frame(k) for k in fr] for ch, off, cn, bal, t0, fr in SHAPES[i][4]}


def rows_of(fs, M, D, channels, x):
    """the rows of an independent channelizer"""
    from pysdr_amd import packet
    from pysdr_amd.channelizer import Channelizer
    ch = Channelizer(fs, M, D, packet.prototype(fs, M, D), channels, max_in=len(x))
    y, freqs = ch.push(x), ch.freqs.copy()
    ch.close()
    return y, freqs


@functools.lru_cache(maxsize=None)
def base(i, bad=False):
    """case i: the input and the rows of an independent channelizer; computed once, never changed"""
    fs, M, D, channels, nk, k_first = shape_of(i)
    x = make_input(i, bad)
    if bad:
        x = x[:int(0.6 * fs)]
    y, freqs = rows_of(fs, M, D, channels, x)
    for v in (x, y):
        v.setflags(write=False)
    assert y.shape[0] == nk
    return dict(i=i, fs=fs, M=M, D=D, channels=channels, x=x, y=y, nk=nk, nd=nk * 8, fs_out=fs / D, freqs=freqs)


def answers(c, cuts):
    """the oracle's answer to every call (counts, words, state after it)"""
    yc = cut_rows(c["y"], cuts, c["D"])
    o = po.Oracle(c["nk"], c["fs_out"])
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
def shared(i, max_out=MAX_OUT, bad=False):
    """case i cut into ragged calls"""
    from pysdr_amd import packet
    c = base(i, bad)
    tile = packet.plan(c["nk"], packet.window_length(c["fs_out"]), max_out, packet.params(c["fs_out"]))["tile"]
    cuts = call_lengths(len(c["x"]), c["D"], tile, max_out)
    counts = [-(-sum(cuts[:k + 1]) // c["D"]) - -(-sum(cuts[:k]) // c["D"]) for k in range(len(cuts))]
    assert 0 in counts and 1 in counts and max(counts) == max_out
    if max_out >= tile + 1:
        assert {tile - 1, tile, tile + 1} <= set(counts)
    return dict(answers(c, cuts), tile=tile, max_out=max_out)


def make(c, max_out=MAX_OUT):
    from pysdr_amd.packet import Packet_Skimmer
    sk = Packet_Skimmer(c["fs"], c["M"], c["D"], channels=c["channels"], max_in=len(c["x"]), max_out=max_out)
    assert (sk.nk, sk.ndec, sk.fs_out, sk.L) == (c["nk"], c["nd"], c["fs_out"], po.tables(c["fs_out"])[0])
    return sk


def same_state(got, want, where):
    for k in po.INTS:
        assert np.array_equal(got[k], want[k]), (where, k, np.flatnonzero(got[k] != want[k])[:5])
    assert np.array_equal(got["frames"], want["frames"]), (where, "frames", np.argwhere(got["frames"] != want["frames"])[:5])


def run_calls(c, max_out, every=1):
    """-> the frames read, as a list of bytes; the state is compared after every `every`-th call and the last"""
    sk = make(c, max_out)
    assert sk.dec.cap == po.cap_of(max_out, po.params(c["fs_out"])["w_baud"])
    frames = []
    for j, (x, r, (wc, wev, wst)) in enumerate(zip(c["calls"], c["yc"], c["want"])):
        got = sk.dec.decode_raw(x, events="all")
        assert got["n_out"] == r.shape[1], j
        assert np.array_equal(got["counts"], wc), (j, np.flatnonzero(got["counts"] != wc)[:5])
        for d in np.flatnonzero(wc):
            assert list(got["events"][d, :wc[d]]) == wev[d], (j, d)
            frames += [data for _, data in po.unpack(wev[d])]
        if j % every == 0 or j == len(c["calls"]) - 1:
            same_state(sk.dec.state(), wst, j)
    sk.close()
    return frames


def all_read(i, frames, least=2):
    for fr in home_rows(i).values():
        for f in fr:
            assert frames.count(f) >= least, (len(f), frames.count(f))


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_every_call_equals_the_oracle(i):
    """ragged cuts: 1-sample calls, calls that complete no output, calls that end on the kernel's tile boundary and one
    output to either side of it, calls of max_out"""
    all_read(i, run_calls(shared(i), MAX_OUT))


def test_a_330_byte_frame_ends_in_a_call_of_16_outputs():
    """max_out = 16: the cap is the 84 words of a frame carried into the call, which the longest frame fills; one row"""
    from pysdr_amd import packet
    fs, M, D = 200000.0, 16, 8
    big = packet.ax25_frame("APRS", "N0CALL-1", info=bytes(range(256)) + b"\xff" * (330 - 16 - 256))
    assert len(big) == 330
    wf = functools.partial(packet.waveform, flags=(4, 2))
    n = len(wf(big, fs, 0.0)) + int(0.01 * fs)
    x = po.scene(fs, n, [([big], 4 * fs / M, 25.0, 1.0, 100)], fs / D, wf, seed=77)
    y, freqs = rows_of(fs, M, D, (4, 1), x)
    c = dict(i=None, fs=fs, M=M, D=D, channels=(4, 1), x=x, y=y, nk=1, nd=8, fs_out=fs / D, freqs=freqs)
    cuts = [16 * D] * (len(x) // (16 * D)) + [len(x) % (16 * D)]
    c = answers(c, cuts)
    assert po.cap_of(16, po.params(fs / D)["w_baud"]) == 84 and max(int(w[0].max()) for w in c["want"]) == 84
    frames = run_calls(c, 16, every=50)
    assert frames.count(big) >= 3 and set(frames) == {big}


def test_two_frames_end_in_one_call():
    """calls of 4096 outputs, cut so that one begins 300 outputs before the first frame of the pair that shares a flag
    ends: the 15-byte frame behind it (144 bits, 3000 outputs and a few stuffed bits) ends in the same call, on the same
    decoders"""
    c = base(0)
    D, n = c["D"], len(c["x"])
    wc, ev = po.Oracle(c["nk"], c["fs_out"]).process(c["y"])
    first = min(i for d in np.flatnonzero(wc) for i, data in po.unpack(ev[d]) if data == the_frame(0))
    head = ((first - 300) % 4096) * D
    cuts = [head] + [4096 * D] * ((n - head) // (4096 * D)) + [(n - head) % (4096 * D)]
    c = answers(c, cuts)
    both = [(j, d) for j, (wc, wev, _) in enumerate(c["want"]) for d in np.flatnonzero(wc) if len(po.unpack(wev[d])) >= 2]
    assert len(both) >= 2, "no two decoders closed two frames in one call"
    all_read(0, run_calls(c, 4096))


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_the_whole_stream_through_push(i):
    """push cuts the stream itself; frames and text are the oracle skimmer's, one record per frame, on its home row"""
    from pysdr_amd import packet
    c = base(i)
    sk = make(c, 4096)
    ev = sk.push(c["x"]) + sk.flush()
    ref = po.Skimmer(c["nk"], c["fs"], c["fs_out"], c["freqs"], packet.tnc2, max_out=4096)
    want = ref.push(c["y"], flush=True)
    assert ev == want and sk.frames == ref.frames
    assert {r: t for r, t in sk.text.items() if t} == ref.text
    home = home_rows(i)
    assert {r: sorted(t.splitlines()) for r, t in ref.text.items()} == {r: sorted(packet.tnc2(f) for f in fr) for r, fr in home.items()}
    assert all(bin(mask).count("1") >= 2 for _, _, _, mask in sk.frames)
    if i == 3:                                                               # a neighbour row read the station too: one record all the same
        raw = po.Oracle(c["nk"], c["fs_out"]).process(c["y"])[0].reshape(c["nk"], 8).sum(axis=1)
        assert (raw > 0).sum() > len(home)
    same_state(sk.dec.state(), ref.o.state(), "end")
    sk.close()


def test_refused_calls_change_nothing():
    from pysdr_amd import _lib
    c = shared(0)
    D = c["D"]
    sk = make(c)
    L = _lib.lib()
    n1 = 3000 * D + 3
    sk.push(c["x"][:n1])
    before = sk.dec.state()
    x = np.array(c["x"][n1:n1 + (MAX_OUT + 1) * D])
    n_out = C.c_int(-1)
    assert sk.dec.chan.n_out_for(len(x)) == MAX_OUT + 1
    h, p = sk.dec._h, C.c_void_p(x.ctypes.data)
    rc = L.pysdr_pkt_process(h, p, len(x), 0, C.byref(n_out), None, None, 0)
    assert rc == -5 and n_out.value == 0 and b"max_out" in L.pysdr_last_error()
    cap = sk.dec.cap
    ev = np.zeros((c["nd"], cap - 1), np.int32)
    cnt = np.zeros(c["nd"], np.int32)
    pi32 = C.POINTER(C.c_int32)
    assert L.pysdr_pkt_process(h, p, 64, 0, C.byref(n_out), cnt.ctypes.data_as(pi32), ev.ctypes.data_as(pi32), cap - 1) == -5
    assert b"ev_pitch" in L.pysdr_last_error()
    assert L.pysdr_pkt_process(h, p, len(c["x"]) + 1, 0, C.byref(n_out), None, None, 0) == -5
    assert L.pysdr_pkt_process(h, None, 16, 0, C.byref(n_out), None, None, 0) == -1
    assert L.pysdr_pkt_process(h, p, -1, 0, C.byref(n_out), None, None, 0) == -1
    assert L.pysdr_pkt_process(h, p, 16, 0, None, None, None, 0) == -1
    rows = np.array([0, c["nd"]], np.int32)
    big = np.zeros((2, cap), np.int32)
    assert L.pysdr_pkt_fetch(h, _lib.as_pi(rows), 2, big.ctypes.data_as(pi32), cap) == -1
    assert L.pysdr_pkt_fetch(h, _lib.as_pi(rows), 1, big.ctypes.data_as(pi32), cap - 1) == -5
    same_state(sk.dec.state(), before, "after the refused calls")
    # the stream did not advance: the rest equals an undisturbed twin's
    twin = make(c)
    twin.push(c["x"][:n1])
    rest = c["x"][n1:]
    got = sk.push(rest) + sk.flush()
    assert got == twin.push(rest) + twin.flush() and len(got) >= 3
    same_state(sk.dec.state(), twin.dec.state(), "rest")
    sk.close()
    twin.close()


def test_a_call_without_outputs_changes_no_state_and_has_no_events():
    c = shared(0)
    D = c["D"]
    sk = make(c)
    sk.push(c["x"][:4500 * D + 1])
    before = sk.dec.state()
    assert before["inframe"].any() and before["frames"].any()
    got = sk.dec.decode_raw(c["x"][4500 * D + 1:4501 * D], events="all")      # ends one sample short of the next output
    assert got["n_out"] == 0 and not got["counts"].any()
    assert not sk.dec.fetch([0, 1, 2, 5]).any()                               # nothing to fetch after it
    same_state(sk.dec.state(), before, "empty call")
    sk.close()


def test_one_nan_and_one_inf_blank_their_windows_and_nothing_else():
    """The rows of a channelizer on the same input carry each non-finite sample for as long as its window holds it; the
    decoders blank the outputs whose bit window reaches such a row sample (that it is exactly L + 1 outputs per row
    sample is shown on the oracle, tests/test_pkt_oracle.py), so events and state still equal the oracle's, and once the
    windows have passed the calls equal a run of the oracle from the state reached there."""
    c = shared(0, MAX_OUT, True)
    L = po.tables(c["fs_out"])[0]
    assert not np.isfinite(c["y"]).all() and np.isfinite(c["y"][:, -500:]).all()
    bad_calls = [j for j, r in enumerate(c["yc"]) if not np.isfinite(r).all()]
    assert len(bad_calls) >= 2
    sk = make(c)
    restart, m, frames = None, 0, []
    for j, (x, r, (wc, wev, wst)) in enumerate(zip(c["calls"], c["yc"], c["want"])):
        got = sk.dec.decode_raw(x, events="all")
        st = sk.dec.state()
        assert np.array_equal(got["counts"], wc), j
        for d in np.flatnonzero(wc):
            assert list(got["events"][d, :wc[d]]) == wev[d], (j, d)
            frames += [data for _, data in po.unpack(wev[d])]
        same_state(st, wst, j)
        m += r.shape[1]
        if restart is not None:
            wc2, wev2 = restart.process(r)
            assert np.array_equal(wc2, wc) and wev2 == wev, j
            same_state(st, restart.state(), ("restarted", j))
        elif j == bad_calls[-1] + 1:
            assert np.isfinite(c["y"][:, m - L:m]).all()
            restart = po.Oracle(c["nk"], c["fs_out"])                          # from the device's state behind the windows
            restart.set_state(st, c["y"][:, m - L:m], m)
    assert restart is not None and frames.count(the_frame(1)) >= 2            # the frame behind the windows is read
    sk.close()


def test_reset_repeats_the_first_run():
    c = shared(0)
    sk = make(c)
    x = c["x"][:int(1.2 * c["fs"])]
    first = sk.push(x)
    st = sk.dec.state()
    text, frames = dict(sk.text), list(sk.frames)
    assert len(first) >= 3
    sk.reset()
    z = sk.dec.state()
    assert (z["crc"] == 0xFFFF).all() and not any(z[k].any() for k in po.INTS if k != "crc") and not z["frames"].any()
    assert not any(sk.text.values()) and not sk.frames and sk.chan.n_in == 0
    assert sk.push(x) == first and dict(sk.text) == text and sk.frames == frames
    same_state(sk.dec.state(), st, "second run")
    sk.close()


def test_device_input_stays_on_the_device_until_fetched():
    """decode_raw with a device pointer and events=None only queues work; the rows fetched afterwards are the host-fed
    twin's"""
    from pysdr_amd import _lib
    c = base(0)
    D, fs = c["D"], c["fs"]
    L = _lib.lib()
    at = int(0.4 * fs)
    x = np.array(c["x"][at:at + 4096 * D])                                   # the first station's first frame ends in it
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
    for k, dcd in enumerate(rows):
        assert np.array_equal(words[k, :want["counts"][dcd]], want["events"][dcd, :want["counts"][dcd]])
    same_state(sk.dec.state(), twin.dec.state(), "device input")
    _lib.check(L.pysdr_dev_free(0, d), "free")
    sk.close()
    twin.close()


def test_a_fine_channelizer_is_adopted():
    """``chan=`` as a FineChannelizer: fs = 1.6 MS/s, rows at 25 kHz 6.25 kHz apart (M2 / D2 = 4), the shape fine.shape gives
    there; one station, read on its home row and equal to the oracle on the fine channelizer's own rows."""
    from pysdr_amd import fine, packet
    fs, fs_out = 1600000.0, 25000.0
    M1, D1, M2, D2 = fine.shape(fs, fs_out, 4)
    f0 = 100000.0
    band = (f0 - 2 * 6250.0, f0 + 2 * 6250.0)
    g_first, ng = fine.channels_for(band, fs, M1, D1, M2)
    h1, h2 = fine.prototype1(fs, M1, D1, M2), packet.prototype(fs / D1, M2, D2)
    f = the_frame(14)
    wf = functools.partial(packet.waveform, flags=(12, 2))
    n = len(wf(f, fs, f0)) + int(0.02 * fs)
    x = po.scene(fs, n, [([f], f0, 25.0, 1.0, 500)], fs_out, wf, seed=91)
    twin = fine.FineChannelizer(fs, M1, M2, D1, D2, h1, h2, (g_first, ng), max_in=len(x))
    y, freqs = twin.push(x), twin.freqs.copy()
    twin.close()
    sk = packet.Packet_Skimmer(fs, chan=fine.FineChannelizer(fs, M1, M2, D1, D2, h1, h2, (g_first, ng), max_in=len(x)), max_out=4096)
    assert sk.fs_out == fs_out and sk.nk == ng == 5 and np.allclose(sk.freqs, freqs)
    ev = sk.push(x) + sk.flush()
    ref = po.Skimmer(ng, fs, fs_out, freqs, packet.tnc2, max_out=4096)
    assert ev == ref.push(y, flush=True) and sk.frames == ref.frames
    home = int(np.argmin(np.abs(freqs - f0)))
    assert [(row, text) for _, row, text in ev] == [(home, packet.tnc2(f))]
    same_state(sk.dec.state(), ref.o.state(), "end")
    sk.close()
