"""The CW skimmer on the GPU (pysdr_amd/csrc/cw.hip, api_cw.hip) against the float32 oracle of the
definition (tests/cw_oracle.py): counts, event words and every state field are EQUAL after every call, floats by their
bits.  The oracle side is fed the rows of an independent Channelizer of the same shape on the same input, so only the
decoder's own arithmetic is judged."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import channelizer_oracle as cz
from tests import cw_oracle as co

pytestmark = pytest.mark.gpu

FS = 48000.0
SECONDS = 12
MAX_OUT = 1024
MESSAGE = "TT CQ K1ABC"                   # 114 dots: 9.1 s at 15 wpm
TAIL = "CQ K1ABC "
# (M, D, channels, carriers (channel k, fraction of a spacing off its centre, wpm, channel SNR dB), channel of the steady carrier)
SHAPES = [(64, 32, (60, 9), ((60, 0.1, 15, 25.0), (62, -0.2, 22, 30.0), (0, 0.3, 30, 35.0)), 2),       # circular range, one partial group
          (256, 128, (250, 70), ((252, 0.3, 15, 35.0), (3, 0.1, 22, 25.0), (40, -0.1, 30, 30.0)), 60),  # two groups, the second partial
          (64, 16, None, ((5, 0.2, 15, 30.0), (20, -0.3, 22, 35.0), (50, 0.1, 30, 25.0)), 33)]          # exactly one group, R = 3000
IDS = [f"{M}-{D}" for M, D, _, _, _ in SHAPES]
SIGMA = 0.01


def fbits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rows_of(M, channels):
    k0, nk = (0, M) if channels is None else channels
    return (k0 + np.arange(nk)) % M


def make_input(i, bad=False):
    from pysdr_amd.cw import morse_keying
    from pysdr_amd.design import channelizer_taps
    M, D, channels, carriers, steady = SHAPES[i]
    h = channelizer_taps(M)
    n = int(SECONDS * FS)
    rng = np.random.default_rng(100 + i)
    x = SIGMA * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    gain = 2 * SIGMA ** 2 * np.sum(h ** 2)                                   # noise power in a channel per unit carrier power
    for j, (k, off, wpm, snr) in enumerate(carriers):
        f = ((k - M if k >= (M + 1) // 2 else k) + off) * FS / M
        c = co.keyed_carrier(MESSAGE, wpm, FS, f, np.sqrt(gain * 10 ** (snr / 10)), 0.5 + 0.1 * j, 0.0, morse_keying, phase=1.0 + j)
        x[:len(c)] += c[:n]
    f = (steady - M if steady >= (M + 1) // 2 else steady) * FS / M
    x += np.sqrt(gain * 10 ** 3.0) * np.exp(2j * np.pi * f / FS * np.arange(n))
    x = x.astype(np.complex64)
    if bad:
        x[int(4.0 * FS) + 7] = complex(np.nan, 0.25)
        x[int(4.4 * FS) + 1] = complex(-0.5, np.inf)
    return x


def call_lengths(n, D, tile):
    """input lengths of the calls: random_cuts (0, 1, fewer than D samples, odd lengths) over the first 300 frames, then
    calls that complete exactly tile - 1, tile, tile + 1 and MAX_OUT outputs, then MAX_OUT outputs each to the end"""
    cuts = cz.random_cuts(300 * D + 5, D, 11)
    at = sum(cuts)

    def upto(frames):                     # the call that ends with the sample that completes `frames` more outputs
        m = -(-at // D)
        return (m + frames - 1) * D + 1 - at

    for fr in (tile - 1, tile, tile + 1, MAX_OUT):
        cuts.append(upto(fr))
        at += cuts[-1]
    while at < n:
        cuts.append(min(n - at, upto(MAX_OUT)))
        at += cuts[-1]
    assert sum(cuts) == n
    return cuts


def cut_rows(y, cuts, D):
    out, at = [], 0
    for c in cuts:
        m0, m1 = cz.frame_range(at, at + c, D)
        out.append(y[:, m0:m1])
        at += c
    return out


def settings(i):
    from pysdr_amd.design import channelizer_taps
    M, D = SHAPES[i][:2]
    return co.params(FS / D, settle=co.settle_samples(len(channelizer_taps(M)), D, FS / D))


@functools.lru_cache(maxsize=None)
def shared(i, bad=False):
    """case i: the input, the rows of an independent channelizer, the calls, and the oracle's answer to every call
    (counts, words, state after it); computed once, never changed"""
    from pysdr_amd import cw
    from pysdr_amd.channelizer import Channelizer
    M, D, channels, carriers, steady = SHAPES[i]
    x = make_input(i, bad)
    if bad:
        x = x[:int(7 * FS)]
    ch = Channelizer(FS, M, D, channels=channels, max_in=len(x))
    y = ch.push(x)
    ch.close()
    nk = y.shape[0]
    tile = cw.plan(nk, MAX_OUT, cw.params(FS / D))["tile"]
    cuts = call_lengths(len(x), D, tile)
    yc = cut_rows(y, cuts, D)
    counts = [r.shape[1] for r in yc]
    assert 0 in counts and 1 in counts and {tile - 1, tile, tile + 1, MAX_OUT} <= set(counts) and max(counts) == MAX_OUT
    o = co.Oracle(nk, settings(i))
    want = []
    for r in yc:
        c, ev = o.process(r)
        want.append((c, ev, o.state()))
    for v in (x, y):
        v.setflags(write=False)
    calls, at = [], 0
    for c in cuts:
        calls.append(x[at:at + c])
        at += c
    rows = list(rows_of(M, channels))
    return dict(M=M, D=D, channels=channels, x=x, y=y, cuts=cuts, calls=calls, yc=yc, want=want, nk=nk, tile=tile,
                home=[(rows.index(k), wpm) for k, _, wpm, _ in carriers], steady=rows.index(steady))


def make(c, **kw):
    from pysdr_amd.cw import CW_Skimmer
    return CW_Skimmer(FS, c["M"], c["D"], channels=c["channels"], max_in=len(c["x"]), max_out=MAX_OUT, **kw)


def same_state(got, want, where):
    for k in co.FLOATS:
        assert np.array_equal(fbits(got[k]), fbits(want[k])), (where, k, np.flatnonzero(fbits(got[k]) != fbits(want[k]))[:5])
    for k in co.INTS:
        assert np.array_equal(got[k], want[k]), (where, k, np.flatnonzero(got[k] != want[k])[:5])


def all_events(want, yc):
    """the oracle's events of a whole run as sorted (m, row, code)"""
    out, m0 = [], 0
    for (c, ev, _), r in zip(want, yc):
        for a, e in enumerate(ev):
            out += [(m0 + co.unpack(w)[0], a, co.unpack(w)[1]) for w in e]
        m0 += r.shape[1]
    return sorted(out)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_every_call_equals_the_oracle(i):
    c = shared(i)
    sk = make(c)
    assert sk.dec.cfg.n0 == settings(i)["n0"] and sk.dec.cap == co.cap_of(MAX_OUT) and sk.nk == c["nk"]
    total = 0
    for j, (x, r, (wc, wev, wst)) in enumerate(zip(c["calls"], c["yc"], c["want"])):
        got = sk.dec.decode_raw(x, events="all")
        assert got["n_out"] == r.shape[1], j
        assert np.array_equal(got["counts"], wc), (j, got["counts"], wc)
        for a in range(c["nk"]):
            assert list(got["events"][a, :wc[a]]) == wev[a], (j, a)
        same_state(sk.dec.state(), wst, j)
        total += int(wc.sum())
    assert total > 30                                                        # the carriers were read, not just silence compared
    sk.close()


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_the_whole_stream_in_calls_of_max_out(i):
    from pysdr_amd.cw import code_text
    c = shared(i)
    sk = make(c)
    ev = sk.push(c["x"])                                                     # cuts itself into calls of MAX_OUT outputs
    want = all_events(c["want"], c["yc"])
    assert ev == [(m, a, code_text(k)) for m, a, k in want]
    same_state(sk.dec.state(), c["want"][-1][2], "end")
    for a in range(c["nk"]):
        assert sk.text[a] == "".join(code_text(k) for _, b, k in want if b == a)
    sk.close()


def test_a_call_of_too_many_outputs_is_refused_and_changes_nothing():
    from pysdr_amd import _lib
    c = shared(0)
    D = c["D"]
    sk = make(c)
    L = _lib.lib()
    n1 = 700 * D + 3
    sk.push(c["x"][:n1])
    before = sk.dec.state()
    x = np.array(c["x"][n1:n1 + (MAX_OUT + 1) * D])
    n_out = C.c_int(-1)
    assert sk.dec.chan.n_out_for(len(x)) == MAX_OUT + 1
    rc = L.pysdr_cw_process(sk.dec._h, C.c_void_p(x.ctypes.data), len(x), 0, C.byref(n_out), None, None, 0)
    assert rc == -5 and n_out.value == 0 and b"max_out" in L.pysdr_last_error()
    ev = np.zeros((c["nk"], 4), np.int32)
    cnt = np.zeros(c["nk"], np.int32)
    pi32 = C.POINTER(C.c_int32)
    assert L.pysdr_cw_process(sk.dec._h, C.c_void_p(x.ctypes.data), 64, 0, C.byref(n_out), cnt.ctypes.data_as(pi32),
                              ev.ctypes.data_as(pi32), 4) == -5 and b"ev_pitch" in L.pysdr_last_error()
    assert L.pysdr_cw_process(sk.dec._h, C.c_void_p(x.ctypes.data), len(c["x"]) + 1, 0, C.byref(n_out), None, None, 0) == -5
    assert L.pysdr_cw_process(sk.dec._h, None, 16, 0, C.byref(n_out), None, None, 0) == -1
    assert L.pysdr_cw_process(sk.dec._h, C.c_void_p(x.ctypes.data), -1, 0, C.byref(n_out), None, None, 0) == -1
    assert L.pysdr_cw_process(sk.dec._h, C.c_void_p(x.ctypes.data), 16, 0, None, None, None, 0) == -1
    rows = np.array([0, c["nk"]], np.int32)
    big = np.zeros((2, sk.dec.cap), np.int32)
    assert L.pysdr_cw_fetch(sk.dec._h, _lib.as_pi(rows), 2, big.ctypes.data_as(pi32), sk.dec.cap) == -1
    assert L.pysdr_cw_fetch(sk.dec._h, _lib.as_pi(rows), 1, big.ctypes.data_as(pi32), sk.dec.cap - 1) == -5
    same_state(sk.dec.state(), before, "after the refused calls")
    # the stream did not advance: the rest equals an undisturbed twin's
    twin = make(c)
    twin.push(c["x"][:n1])
    rest = c["x"][n1:n1 + 1500 * D]
    assert sk.push(rest) == twin.push(rest)
    same_state(sk.dec.state(), twin.dec.state(), "rest")
    sk.close()
    twin.close()


def test_a_call_without_outputs_changes_no_state_and_has_no_events():
    c = shared(0)
    D = c["D"]
    sk = make(c)
    sk.push(c["x"][:500 * D + 1])
    before = sk.dec.state()
    got = sk.dec.decode_raw(c["x"][500 * D + 1:501 * D], events="all")       # ends one sample short of the next frame
    assert got["n_out"] == 0 and not got["counts"].any()
    assert not sk.dec.fetch([0, 1, 2, 5]).any()                              # nothing to fetch after it
    same_state(sk.dec.state(), before, "empty call")
    sk.close()


def test_one_nan_and_one_inf_hold_the_envelope_and_mark_nothing_else():
    """The rows of a channelizer on the same input carry the non-finite samples for as long as its window holds them; the
    decoder holds its envelope for those samples (step 1), so events and state still equal the oracle's, every state float
    stays finite, and once the window has passed the calls equal a run of the oracle from the state reached there."""
    c = shared(0, True)
    D = c["D"]
    assert not np.isfinite(c["y"]).all() and np.isfinite(c["y"][:, -2000:]).all()
    bad_calls = [j for j, r in enumerate(c["yc"]) if not np.isfinite(r).all()]
    assert len(bad_calls) >= 2
    sk = make(c)
    restart = None
    for j, (x, r, (wc, wev, wst)) in enumerate(zip(c["calls"], c["yc"], c["want"])):
        got = sk.dec.decode_raw(x, events="all")
        st = sk.dec.state()
        assert np.array_equal(got["counts"], wc), j
        for a in range(c["nk"]):
            assert list(got["events"][a, :wc[a]]) == wev[a], (j, a)
        same_state(st, wst, j)
        assert all(np.isfinite(st[k]).all() for k in co.FLOATS), j
        if restart is not None:
            wc2, wev2 = restart.process(r)
            assert np.array_equal(wc2, wc) and wev2 == wev, j
            same_state(st, restart.state(), ("restarted", j))
        elif j == bad_calls[-1] + 1:
            restart = co.Oracle(c["nk"], settings(0))                        # from the device's state behind the window
            restart.set_state(st)
    assert restart is not None and sum(int(w[0].sum()) for w in c["want"]) > 10
    sk.close()


def test_reset_repeats_the_first_run():
    c = shared(0)
    sk = make(c)
    x = c["x"][:int(5 * FS)]
    first = sk.push(x)
    st = sk.dec.state()
    text = dict(sk.text)
    assert len(first) > 5
    sk.reset()
    z = sk.dec.state()
    assert (z["dot"] == settings(0)["d0"]).all() and (z["code"] == 1).all() and not z["seen"].any() and not fbits(z["pk"]).any()
    assert all(t == "" for t in sk.text.values()) and sk.chan.n_in == 0
    assert sk.push(x) == first and sk.text == text
    same_state(sk.dec.state(), st, "second run")
    sk.close()


def test_skimmer_reads_the_carriers():
    """End to end on the first shape: the text of every home row holds the message's tail, its speed estimate is within
    15 % of the sent speed -- or, where the oracle's own estimate is outside that, within 15 % of the oracle's, which this
    run equals bit for bit anyway -- and the steady carrier and the noise rows say nothing."""
    c = shared(0)
    sk = make(c)
    ev = sk.push(c["x"])
    st = sk.state()
    ost = c["want"][-1][2]
    for row, wpm in c["home"]:
        assert TAIL in sk.text[row], (row, wpm, sk.text[row])
        est = float(st["wpm"][row])
        o_est = 19.2 * (FS / c["D"]) / float(ost["dot"][row])
        ref = wpm if abs(o_est - wpm) <= 0.15 * wpm else o_est               # the oracle's value where it is itself outside
        print(f"row {row}: {wpm} wpm sent, estimate {est:.2f} (oracle {o_est:.2f}), snr {st['snr_db'][row]:.1f} dB, text {sk.text[row]!r}")
        assert abs(est - ref) <= 0.15 * ref, (row, wpm, est, o_est)
        assert np.isfinite(st["snr_db"][row])
    assert sk.text[c["steady"]] == "" and st["key"].dtype == bool
    assert all(m2 >= m1 for (m1, _, _), (m2, _, _) in zip(ev, ev[1:]))
    assert np.array_equal(sk.freqs, np.where(rows_of(c["M"], c["channels"]) >= 32, rows_of(c["M"], c["channels"]) - 64, rows_of(c["M"], c["channels"])) * FS / 64)
    sk.close()


def test_device_input_stays_on_the_device_until_fetched():
    """decode_raw with a device pointer and events=None only queues work; the counts and rows fetched afterwards are the
    host-fed twin's"""
    from pysdr_amd import _lib
    c = shared(0)
    D = c["D"]
    L = _lib.lib()
    x = np.array(c["x"][int(2 * FS):int(2 * FS) + MAX_OUT * D])
    head = c["x"][:int(2 * FS)]
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
    for k, a in enumerate(rows):
        assert np.array_equal(words[k, :want["counts"][a]], want["events"][a, :want["counts"][a]])
    same_state(sk.dec.state(), twin.dec.state(), "device input")
    _lib.check(L.pysdr_dev_free(0, d), "free")
    sk.close()
    twin.close()
