"""The ACARS skimmer on the GPU (pysdr_amd/csrc/acars.hip, api_acars.hip) against the float32 oracle of
the definition (tests/acars_oracle.py): counts, event words, every state field and the frame buffers are EQUAL after every
call.  The oracle side is fed the rows of an independent Channelizer of the same shape and prototype on the same input, so
only the decoders' own arithmetic is judged.  That the oracle reads every planted block is shown on the CPU
(tests/test_acars_oracle.py); here the blocks are counted again so that no test passes on silence."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import acars_oracle as ao
from tests.test_gpu_psk import call_lengths, cut_rows

pytestmark = pytest.mark.gpu

SECONDS = 1.0
MAX_OUT = 256
# (fs, M, D, channels, stations (channel, Hz off its centre, C/N dB in the row bandwidth, AM depth, start s, frame, inverted))
SHAPES = [
    (400000.0, 16, 8, (3, 4), ((3, 300.0, 20.0, 0.8, 0.03, 0, False), (5, -500.0, 15.0, 0.5, 0.34, 1, True), (6, 0.0, 30.0, 0.9, 0.55, 2, False))),
    (200000.0, 16, 8, (12, 9), ((13, -700.0, 25.0, 0.8, 0.03, 3, True), (0, 100.0, 15.0, 0.9, 0.34, 4, False), (3, 600.0, 30.0, 0.5, 0.55, 5, False))),
    (153600.0, 16, 8, None, ((2, 0.0, 30.0, 0.8, 0.03, 6, False), (11, 400.0, 18.0, 0.9, 0.34, 7, True), (15, -400.0, 20.0, 0.6, 0.55, 8, False))),
    (384000.0, 32, 8, (5, 9), ((8, 0.0, 20.0, 0.8, 0.03, 9, False), (11, 500.0, 30.0, 0.5, 0.34, 10, False), (6, -300.0, 15.0, 0.9, 0.55, 11, True))),
]
IDS = ["400k-16-3+4", "200k-16-12+9", "153k6-16-all", "384k-32-5+9"]


def the_chars(k, prekey=16):
    """the characters of transmission k: blocks of 40 to 80 bytes, up- and downlinks, one ETB"""
    from pysdr_amd import acars
    n_text = 26 + (k * 7) % 41
    if k % 2:
        text = (f"M{k:02d}AXX{k:04d}" + "POS N49035W072017,KJFK,1234,350 " * 3)[:n_text]
        return acars.frame("2", f"N{100 + k}AB", None, "H1", str(k % 10), text, prekey=prekey)
    return acars.frame("2", f"G-AB{chr(65 + k % 26)}{chr(66 + k % 25)}", "A", "_d", chr(65 + k % 26), ("UPLINK " * 12)[:n_text], more=(k == 4), prekey=prekey)


def block_of(chars):
    """what the skimmer delivers of a transmission: the bytes behind SOH up to ETX / ETB"""
    at = chars.index(b"\x16\x16\x01") + 3
    return chars[at:-3]


def make_input(i, bad=False):
    from pysdr_amd import acars
    fs, M, D, channels, stations = SHAPES[i]
    n = int(SECONDS * fs)
    sts = [(the_chars(k), ch * fs / M + off, cn, depth, int(t0 * fs), inv) for ch, off, cn, depth, t0, k, inv in stations]
    x = ao.scene(fs, n, sts, fs / D, acars.waveform, seed=500 + i)
    if bad:
        x[int(0.2 * fs) + 7] = complex(np.nan, 0.25)                          # inside the first station's block
        x[int(0.33 * fs) + 1] = complex(-0.5, np.inf)                         # more than max_out outputs later: another call
    return x


def shape_of(i):
    fs, M, D, channels, stations = SHAPES[i]
    nk = M if channels is None else channels[1]
    k_first = 0 if channels is None else channels[0]
    return fs, M, D, channels, nk, k_first


def home_rows(i):
    fs, M, D, channels, nk, k_first = shape_of(i)
    return {(ch - k_first) % M: [block_of(the_chars(k))] for ch, off, cn, depth, t0, k, inv in SHAPES[i][4]}


def rows_of(fs, M, D, channels, x):
    """the rows of an independent channelizer"""
    from pysdr_amd import acars
    from pysdr_amd.channelizer import Channelizer
    ch = Channelizer(fs, M, D, acars.prototype(fs, M, D), channels, max_in=len(x))
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
    return dict(i=i, fs=fs, M=M, D=D, channels=channels, x=x, y=y, nk=nk, nd=nk, fs_out=fs / D, freqs=freqs)


def answers(c, cuts):
    """the oracle's answer to every call (counts, words, state after it)"""
    yc = cut_rows(c["y"], cuts, c["D"])
    o = ao.Oracle(c["nk"], c["fs_out"])
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
    from pysdr_amd import acars
    c = base(i, bad)
    tile = acars.plan(c["nk"], acars.window_length(c["fs_out"]), max_out, acars.params(c["fs_out"]))["tile"]
    cuts = call_lengths(len(c["x"]), c["D"], tile, max_out)
    counts = [-(-sum(cuts[:k + 1]) // c["D"]) - -(-sum(cuts[:k]) // c["D"]) for k in range(len(cuts))]
    assert 0 in counts and 1 in counts and max(counts) == max_out
    assert {tile - 1, tile, tile + 1} <= set(counts)
    return dict(answers(c, cuts), tile=tile, max_out=max_out)


def make(c, max_out=MAX_OUT):
    from pysdr_amd.acars import ACARS_Skimmer
    sk = ACARS_Skimmer(c["fs"], c["M"], c["D"], channels=c["channels"], max_in=len(c["x"]), max_out=max_out)
    assert (sk.nk, sk.ndec, sk.fs_out, sk.L) == (c["nk"], c["nd"], c["fs_out"], ao.tables(c["fs_out"])[0])
    return sk


def same_state(got, want, where):
    for k in ao.INTS:
        assert np.array_equal(got[k], want[k]), (where, k, np.flatnonzero(got[k] != want[k])[:5])
    assert np.array_equal(got["frames"], want["frames"]), (where, "frames", np.argwhere(got["frames"] != want["frames"])[:5])


def run_calls(c, max_out, every=1):
    """-> the blocks read, as a list of bytes; the state is compared after every `every`-th call and the last"""
    sk = make(c, max_out)
    assert sk.dec.cap == ao.cap_of(max_out, ao.params(c["fs_out"])["w_baud"])
    frames = []
    for j, (x, r, (wc, wev, wst)) in enumerate(zip(c["calls"], c["yc"], c["want"])):
        got = sk.dec.decode_raw(x, events="all")
        assert got["n_out"] == r.shape[1], j
        assert np.array_equal(got["counts"], wc), (j, np.flatnonzero(got["counts"] != wc)[:5])
        for d in np.flatnonzero(wc):
            assert list(got["events"][d, :wc[d]]) == wev[d], (j, d)
            frames += [data for _, data in ao.unpack(wev[d])]
        if j % every == 0 or j == len(c["calls"]) - 1:
            same_state(sk.dec.state(), wst, j)
    sk.close()
    return frames


def all_read(i, frames):
    for fr in home_rows(i).values():
        for f in fr:
            assert frames.count(f) >= 1, (len(f), frames.count(f))


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_every_call_equals_the_oracle(i):
    """ragged cuts: 1-sample calls, calls that complete no output, calls that end on the kernel's tile boundary and one
    output to either side of it, calls of max_out"""
    all_read(i, run_calls(shared(i), MAX_OUT))


def one_station(fs, M, D, chars, cn=25.0, seed=77):
    """one station on channel 4, alone in a channelizer of one row"""
    from pysdr_amd import acars
    n = len(acars.waveform(chars, fs, 0.0)) + int(0.02 * fs)
    x = ao.scene(fs, n, [(chars, 4 * fs / M, cn, 0.8, 100)], fs / D, acars.waveform, seed=seed)
    y, freqs = rows_of(fs, M, D, (4, 1), x)
    return dict(i=None, fs=fs, M=M, D=D, channels=(4, 1), x=x, y=y, nk=1, nd=1, fs_out=fs / D, freqs=freqs)


def test_a_238_byte_block_ends_in_a_call_of_16_outputs():
    """max_out = 16: the cap is the 61 words of a block carried into the call, which the longest block fills; one row"""
    from pysdr_amd import acars
    fs, M, D = 200000.0, 16, 8
    chars = acars.frame("2", "N123AB", None, "H1", "A", ("0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ" * 7)[:220], prekey=4)
    big = block_of(chars)
    assert len(big) == 234
    # the definition's limit is 238: four more characters than the 220 of text this helper writes
    body = bytes(b & 0x7F for b in big[:-1]) + b"WXYZ\x03"
    big = acars.parity(body)
    chars = chars[:chars.index(b"\x16\x16\x01") + 3] + big + int(acars.crc16(big)).to_bytes(2, "little") + acars.parity(b"\x7f")
    assert len(big) == 238
    c = one_station(fs, M, D, chars)
    x = c["x"]
    cuts = [16 * D] * (len(x) // (16 * D)) + [len(x) % (16 * D)]
    c = answers(c, cuts)
    assert ao.cap_of(16, ao.params(fs / D)["w_baud"]) == 61 and max(int(w[0].max()) for w in c["want"]) == 61
    frames = run_calls(c, 16, every=50)
    assert frames == [big]


def test_two_blocks_end_in_one_call():
    """calls of 4096 outputs at 19.2 kHz, cut so that one begins 300 outputs before the first of two 13-byte blocks sent
    back to back ends: the second (23 characters, 1472 outputs) ends in the same call, on the same decoder"""
    from pysdr_amd import acars
    fs, M, D = 153600.0, 16, 8
    a, b = acars.frame("2", "N1", None, "Q0", "1", prekey=8), acars.frame("2", "N2", "1", "Q0", "2", prekey=2)
    c = one_station(fs, M, D, a + b, seed=78)
    n = len(c["x"])
    wc, ev = ao.Oracle(1, c["fs_out"]).process(c["y"])
    got = ao.unpack(ev[0])
    assert [data for _, data in got] == [block_of(a), block_of(b)] and len(block_of(a)) == 13
    head = ((got[0][0] - 300) % 4096) * D
    cuts = [head] + [4096 * D] * ((n - head) // (4096 * D)) + [(n - head) % (4096 * D)]
    c = answers(c, cuts)
    assert any(len(ao.unpack(wev[0])) == 2 for _, wev, _ in c["want"]), "the two blocks did not end in one call"
    assert run_calls(c, 4096) == [block_of(a), block_of(b)]


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_the_whole_stream_through_push(i):
    """push cuts the stream itself; records and frames are the oracle skimmer's, one record per block, on its home row"""
    from pysdr_amd import acars
    c = base(i)
    ref = ao.Skimmer(c["nk"], c["fs"], c["fs_out"], c["freqs"], max_out=4096)
    want = ref.push(c["y"], flush=True)
    home = home_rows(i)
    assert sorted(data for _, _, data in want) == sorted(f for fr in home.values() for f in fr)
    for _, row, data in want:                                                # on its home row; where the rows lie fs_out / 4 apart (case 3)
        assert abs(row - [r for r, fr in home.items() if data in fr][0]) <= (1 if i == 3 else 0)   # a neighbour may have read it too
    for max_out in (4096, 1000):                                             # whatever the cut
        sk = make(c, max_out)
        ev = sk.push(c["x"]) + sk.flush()
        assert ev == [(m, row, acars.parse(data)) for m, row, data in want] and sk.frames == ref.frames
        assert {r: t for r, t in sk.text.items() if t} == {row: acars.line(acars.parse(data)) + "\n" for _, row, data in want}
        assert all(rec is not None and rec["address"] for _, _, rec in ev)
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
    rc = L.pysdr_acars_process(h, p, len(x), 0, C.byref(n_out), None, None, 0)
    assert rc == -5 and n_out.value == 0 and b"max_out" in L.pysdr_last_error()
    cap = sk.dec.cap
    ev = np.zeros((c["nd"], cap - 1), np.int32)
    cnt = np.zeros(c["nd"], np.int32)
    pi32 = C.POINTER(C.c_int32)
    assert L.pysdr_acars_process(h, p, 64, 0, C.byref(n_out), cnt.ctypes.data_as(pi32), ev.ctypes.data_as(pi32), cap - 1) == -5
    assert b"ev_pitch" in L.pysdr_last_error()
    assert L.pysdr_acars_process(h, p, len(c["x"]) + 1, 0, C.byref(n_out), None, None, 0) == -5
    assert L.pysdr_acars_process(h, None, 16, 0, C.byref(n_out), None, None, 0) == -1
    assert L.pysdr_acars_process(h, p, -1, 0, C.byref(n_out), None, None, 0) == -1
    assert L.pysdr_acars_process(h, p, 16, 0, None, None, None, 0) == -1
    rows = np.array([0, c["nd"]], np.int32)
    big = np.zeros((2, cap), np.int32)
    assert L.pysdr_acars_fetch(h, _lib.as_pi(rows), 2, big.ctypes.data_as(pi32), cap) == -1
    assert L.pysdr_acars_fetch(h, _lib.as_pi(rows), 1, big.ctypes.data_as(pi32), cap - 1) == -5
    same_state(sk.dec.state(), before, "after the refused calls")
    # the stream did not advance: the rest equals an undisturbed twin's
    twin = make(c)
    twin.push(c["x"][:n1])
    rest = c["x"][n1:]
    got = sk.push(rest) + sk.flush()
    assert got == twin.push(rest) + twin.flush() and len(got) == 3
    same_state(sk.dec.state(), twin.dec.state(), "rest")
    sk.close()
    twin.close()


def test_a_call_without_outputs_changes_no_state_and_has_no_events():
    c = shared(0)
    D = c["D"]
    sk = make(c)
    sk.push(c["x"][:7000 * D + 1])
    before = sk.dec.state()
    assert before["st"].any() and before["frames"].any()                      # inside the first station's block
    got = sk.dec.decode_raw(c["x"][7000 * D + 1:7001 * D], events="all")      # ends one sample short of the next output
    assert got["n_out"] == 0 and not got["counts"].any()
    assert not sk.dec.fetch([0, 1, 2, 3]).any()                               # nothing to fetch after it
    same_state(sk.dec.state(), before, "empty call")
    sk.close()


def test_one_nan_and_one_inf_blank_their_windows_and_nothing_else():
    """The rows of a channelizer on the same input carry each non-finite sample for as long as its window holds it; the
    decoders blank the outputs whose windows reach such a row sample (that it is exactly NT + L outputs per row sample is
    shown on the oracle, tests/test_acars_oracle.py), so events and state still equal the oracle's, and once the windows
    have passed the calls equal a run of the oracle from the state reached there."""
    c = shared(0, MAX_OUT, True)
    H = 5 * ao.tables(c["fs_out"])[0]
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
            frames += [data for _, data in ao.unpack(wev[d])]
        same_state(st, wst, j)
        m += r.shape[1]
        if restart is not None:
            wc2, wev2 = restart.process(r)
            assert np.array_equal(wc2, wc) and wev2 == wev, j
            same_state(st, restart.state(), ("restarted", j))
        elif j == bad_calls[-1] + 1:
            assert np.isfinite(c["y"][:, m - H:m]).all()
            restart = ao.Oracle(c["nk"], c["fs_out"])                          # from the device's state behind the windows
            restart.set_state(st, c["y"][:, m - H:m], m)
    assert restart is not None and frames.count(block_of(the_chars(1))) == 1  # the block behind the windows is read
    sk.close()


def test_reset_repeats_the_first_run():
    c = shared(0)
    sk = make(c)
    x = c["x"][:int(0.95 * c["fs"])]
    first = sk.push(x)
    st = sk.dec.state()
    text, frames = dict(sk.text), list(sk.frames)
    assert len(first) == 3
    sk.reset()
    z = sk.dec.state()
    assert not any(z[k].any() for k in ao.INTS) and not z["frames"].any()
    assert not any(sk.text.values()) and not sk.frames and sk.chan.n_in == 0
    assert sk.push(x) == first and dict(sk.text) == text and sk.frames == frames
    same_state(sk.dec.state(), st, "second run")
    sk.close()


def test_device_input_stays_on_the_device_until_fetched():
    """decode_raw with a device pointer and events=None only queues work; the rows fetched afterwards are the host-fed
    twin's"""
    from pysdr_amd import _lib
    c = base(0)
    D = c["D"]
    L = _lib.lib()
    wc, ev = ao.Oracle(c["nk"], c["fs_out"]).process(c["y"])
    m_end = min(i for d in np.flatnonzero(wc) for i, _ in ao.unpack(ev[d]))   # the first block's end
    at = (m_end - 2000) * D
    x = np.array(c["x"][at:at + 4096 * D])
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
    words = sk.dec.fetch(np.concatenate((rows, [0])))                        # the rows with a block and one more
    for k, dcd in enumerate(rows):
        assert np.array_equal(words[k, :want["counts"][dcd]], want["events"][dcd, :want["counts"][dcd]])
    same_state(sk.dec.state(), twin.dec.state(), "device input")
    _lib.check(L.pysdr_dev_free(0, d), "free")
    sk.close()
    twin.close()


def test_a_fine_channelizer_is_adopted():
    """``chan=`` as a FineChannelizer: fs = 1.6 MS/s, rows at 25 kHz 6.25 kHz apart (M2 / D2 = 4), the shape fine.shape gives
    there; one station, read once and equal to the oracle on the fine channelizer's own rows."""
    from pysdr_amd import acars, fine
    fs, fs_out = 1600000.0, 25000.0
    M1, D1, M2, D2 = fine.shape(fs, fs_out, 4)
    f0 = 100000.0
    band = (f0 - 2 * 6250.0, f0 + 2 * 6250.0)
    g_first, ng = fine.channels_for(band, fs, M1, D1, M2)
    h1, h2 = fine.prototype1(fs, M1, D1, M2), acars.prototype(fs / D1, M2, D2)
    chars = the_chars(14, prekey=8)
    n = len(acars.waveform(chars, fs, f0)) + int(0.02 * fs)
    x = ao.scene(fs, n, [(chars, f0, 25.0, 0.8, 500)], fs_out, acars.waveform, seed=91)
    twin = fine.FineChannelizer(fs, M1, M2, D1, D2, h1, h2, (g_first, ng), max_in=len(x))
    y, freqs = twin.push(x), twin.freqs.copy()
    twin.close()
    sk = acars.ACARS_Skimmer(fs, chan=fine.FineChannelizer(fs, M1, M2, D1, D2, h1, h2, (g_first, ng), max_in=len(x)), max_out=4096)
    assert sk.fs_out == fs_out and sk.nk == ng == 5 and np.allclose(sk.freqs, freqs)
    ev = sk.push(x) + sk.flush()
    ref = ao.Skimmer(ng, fs, fs_out, freqs, max_out=4096)
    want = ref.push(y, flush=True)
    assert sk.frames == ref.frames == want and [(m, row) for m, row, _ in ev] == [(m, row) for m, row, _ in want]
    home = int(np.argmin(np.abs(freqs - f0)))
    raw = ao.Oracle(ng, fs_out).process(y)[0]
    assert len(ev) == 1 and raw[home] > 0 and ev[0][2] == acars.parse(block_of(chars))   # rows 6.25 kHz apart overlap: copies, one record
    same_state(sk.dec.state(), ref.o.state(), "end")
    sk.close()
