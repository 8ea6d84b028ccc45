"""The LDPC(174,91) decoder on the GPU (pysdr_amd/csrc/ldpc.hip, ldpc_host.h) against the float32 oracle
of the definition (tests/ldpc_oracle.py): status, iterations, nerr, the packed bits and the bits of the final sums are
EQUAL -- from host soft bits in one and two chunks, and from the spectrum ring of an FT8 and an FT4 skimmer, where the
oracle is fed the skimmer's own soft bits.  Then the skimmers with ``decode=True``: the stations' texts come out, and
with ``decode=False`` a record is what it was."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import ft4_oracle as f4o
from tests import ft8_oracle as fo
from tests import ldpc_oracle as lo
from tests import test_gpu_ft4 as g4
from tests import test_gpu_ft8 as g8
from tests.test_gpu_psk import fbits

pytestmark = pytest.mark.gpu

F32 = np.float32
TEXTS = ("CQ K1ABC FN42", "K1ABC W9XYZ -12", "W9XYZ K1ABC RR73")
N_ALL = 4097                                                                    # two chunks, the last of one
pi32, pu8, pll = C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_longlong)


def messages():
    from pysdr_amd import ft8msg
    return [ft8msg.pack77(t) for t in TEXTS]


@functools.lru_cache(maxsize=None)
def soft_inputs():
    """4097 words: codewords at five noise levels, noise alone, a word with a broken CRC, zeros, and the same kinds scaled
    to near 1e18; shuffled, so that every prefix holds a mixture; computed once, never changed"""
    from pysdr_amd import ldpc
    rng = np.random.default_rng(24)
    out = np.zeros((N_ALL, 174), np.float64)
    kinds = rng.integers(0, 8, N_ALL)
    kinds[:8] = [1, 5, 6, 7, 3, 0, 2, 4]
    for i, k in enumerate(kinds):
        cw = ldpc.encode(rng.integers(0, 2, 77))
        if k < 5:
            out[i] = (2.0 * cw - 1) + (0.0, 0.4, 0.55, 0.643, 0.8)[k] * rng.standard_normal(174)
            if k == 0:
                out[i] *= rng.uniform(0.5, 2.0, 174)
        elif k == 5:
            out[i] = rng.standard_normal(174)
        elif k == 6:
            b91 = cw[:91].copy()
            b91[77 + i % 14] ^= 1
            out[i] = (2.0 * ldpc.encode91(b91) - 1) * rng.uniform(1.0, 2.0, 174)
        # k == 7: zeros
        if i % 3 == 0:
            out[i] *= 2.4e17                                                    # |llr| up to about 1e18
    out = out.astype(F32)
    assert np.isfinite(out).all() and np.abs(out).max() > 5e17 and np.abs(out).max() <= 2e18
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want(iters):
    st, bits, post = lo.decode(soft_inputs(), iters=iters)
    for v in (st, bits, post):
        v.setflags(write=False)
    return st, bits, post


def same(got, st, bits, post, where):
    from pysdr_amd import ldpc
    assert np.array_equal(got["status"], st[:, 0]), (where, np.flatnonzero(got["status"] != st[:, 0])[:5])
    assert np.array_equal(got["iterations"], st[:, 1]), (where, np.flatnonzero(got["iterations"] != st[:, 1])[:5])
    assert np.array_equal(got["nerr"], st[:, 2]), (where, np.flatnonzero(got["nerr"] != st[:, 2])[:5])
    assert np.array_equal(got["bits"], ldpc.unpack_bits(bits)), where
    assert np.array_equal(fbits(got["post"]), fbits(post)), (where, np.argwhere(fbits(got["post"]) != fbits(post))[:5])


@pytest.fixture(scope="module")
def small():
    """a skimmer of the smallest shape, for the calls that take soft bits from the host"""
    from pysdr_amd.ft8 import FT8_Skimmer
    sk = FT8_Skimmer(8000.0, channels=(3, 3), max_in=4096)
    yield sk
    sk.close()


@pytest.mark.parametrize("iters", (1, 30))
@pytest.mark.parametrize("n", (1, 3, 193, N_ALL))
def test_host_soft_bits_equal_the_oracle(small, n, iters):
    from pysdr_amd import ldpc
    st, bits, post = want(iters)
    if n == N_ALL and iters == 30:                                              # the mixture is one
        assert set(st[:, 0]) == {0, 1, 2} and len(set(st[:, 1])) > 8 and st[:, 1].max() == 30 and (st[st[:, 0] == 0, 1] == 30).all()
    got = small.dec.decode_llr(soft_inputs()[:n], ldpc.params(iters=iters), post=True)
    same(got, st[:n], bits[:n], post[:n], (n, iters))
    if n == 3:
        plain = small.dec.decode_llr(soft_inputs()[:n], ldpc.params(iters=iters))
        assert "post" not in plain and np.array_equal(plain["status"], got["status"]) and np.array_equal(plain["bits"], got["bits"])


def test_every_refusal_of_host_soft_bits_leaves_the_outputs_untouched(small):
    from pysdr_amd import _lib, ldpc
    L, h = _lib.lib(), small.dec._h
    llr = np.array(soft_inputs()[:4])
    st, bits, post = np.full((4, 4), 7, np.int32), np.full((4, 12), 7, np.uint8), np.full((4, 174), 7.0, F32)

    def call(x=llr, n=4, cfg=ldpc.params(), s=True, b=True):
        rc = L.pysdr_ft8_decode_llr(h, None if x is None else _lib.as_pf(x), n, None if cfg is None else C.byref(cfg),
                                    st.ctypes.data_as(pi32) if s else None, bits.ctypes.data_as(pu8) if b else None, _lib.as_pf(post))
        if rc != 0:
            assert (st == 7).all() and (bits == 7).all() and (post == 7.0).all()
        return rc

    assert call(n=-1) == -1 and call(n=4097) == -1 and b"pysdr_ft8_decode_llr" in L.pysdr_last_error()
    assert call(cfg=None) == -1 and call(x=None) == -1 and call(s=False) == -1 and call(b=False) == -1
    for k, v in (("iters", 0), ("iters", 201), ("alpha", 0.0), ("alpha", 1.25), ("alpha", float("nan"))):
        c = ldpc.params()
        setattr(c, k, v)
        assert call(cfg=c) == -1, (k, v)
    for v in (np.nan, np.inf, -np.inf):
        x = llr.copy()
        x[3, 173] = v
        assert call(x=x) == -1 and b"not finite" in L.pysdr_last_error()
        with pytest.raises(_lib.PysdrError):
            small.dec.decode_llr(x)
    assert call(n=0) == 0 and (st == 7).all()
    assert L.pysdr_ft8_decode_llr(None, _lib.as_pf(llr), 4, C.byref(ldpc.params()), st.ctypes.data_as(pi32), bits.ctypes.data_as(pu8), None) == -1
    assert call() == 0 and np.array_equal(st, want(30)[0][:4]) and np.array_equal(bits, want(30)[1][:4])


# ---- from the ring: case 0 of tests/test_gpu_ft8.py with codewords on the air ---------------------------------------------------

@functools.lru_cache(maxsize=None)
def coded_input():
    """test_gpu_ft8.make_input(0) with the stations re-made from encoded messages"""
    from pysdr_amd import ldpc
    fs, channels, stations = g8.SHAPES[0]
    n = int(g8.SECONDS * fs)
    rng = np.random.default_rng(500)
    x = fo.noise_sigma(0.0, fo.SNR_BW, fs) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for j, ((f, snr, start), msg) in enumerate(zip(stations, messages())):
        s = fo.waveform(fo.tones(ldpc.encode(msg)), f, fs, gfsk=j != 1, phase=1.0 + j) * 10 ** (snr / 20)
        at = int(start * fs)
        x[at:at + len(s)] += s[:n - at]
    x = (0.05 * x).astype(np.complex64)
    x.setflags(write=False)
    return x


def skimmer(**kw):
    from pysdr_amd.ft8 import FT8_Skimmer
    fs, channels, _ = g8.SHAPES[0]
    return FT8_Skimmer(fs, channels=channels, max_in=len(coded_input()), **kw)


@pytest.fixture(scope="module")
def pushed():
    """the decoding skimmer after the whole stream, and the records it gave"""
    sk = skimmer(decode=True)
    recs = sk.push(coded_input())
    yield sk, recs
    sk.close()


def test_candidates_from_the_ring_equal_the_oracle_on_the_skimmers_own_soft_bits(pushed):
    from pysdr_amd import ft8msg, ldpc
    sk, recs = pushed
    done, tr = sk.dec.t_done, sk.dec.tr
    assert (done, tr) == (347, 355) and len(recs) == 3
    rng = np.random.default_rng(7)
    F = np.array([r["F"] for r in recs] + list(rng.integers(0, sk.nfine, 60)) + [0, sk.nfine - 1], np.int32)
    t0 = np.array([r["t0"] for r in recs] + list(rng.integers(0, done - 312, 60)) + [0, done - 313], np.int64)
    soft = sk.dec.llr(F, t0)
    for iters in (1, 30):
        st, bits, post = lo.decode(soft, iters=iters)
        got = sk.dec.decode(F, t0, ldpc.params(iters=iters), post=True)
        same(got, st, bits, post, iters)
        if iters == 30:
            assert list(got["status"][:3]) == [2, 2, 2] and (got["status"][3:] != 2).all()
            assert sorted(ft8msg.unpack77(b[:77]) for b in got["bits"][:3]) == sorted(TEXTS)


def test_every_refusal_of_candidates_from_the_ring(pushed):
    """as pysdr_ft8_llr refuses them: a frame not yet complete, one gone from the ring, an F outside the raster; and n, the
    cfg and NULL arrays; nothing is launched and no output changes"""
    from pysdr_amd import _lib, ldpc
    sk, _ = pushed
    L, h, done, nf = _lib.lib(), sk.dec._h, sk.dec.t_done, sk.nfine
    st, bits, post = np.full((2, 4), 7, np.int32), np.full((2, 12), 7, np.uint8), np.full((2, 174), 7.0, F32)

    def call(F, t0, n=None, cfg=ldpc.params(), s=True):
        F, t0 = np.array(F, np.int32), np.array(t0, np.int64)
        rc = L.pysdr_ft8_decode(h, F.ctypes.data_as(pi32), t0.ctypes.data_as(pll), len(F) if n is None else n, None if cfg is None else C.byref(cfg),
                                st.ctypes.data_as(pi32) if s else None, bits.ctypes.data_as(pu8), _lib.as_pf(post))
        if rc != 0:
            assert (st == 7).all() and (bits == 7).all() and (post == 7.0).all()
        return rc

    assert call([3, 3], [0, done - 312]) == -5 and b"pysdr_ft8_decode" in L.pysdr_last_error()   # the second frame's last step is not in
    assert call([3], [-1]) == -5 and call([-1], [0]) == -1 and call([3, nf], [0, 0]) == -1
    assert call([3], [0], n=-1) == -1 and call([3], [0], n=4097) == -1 and call([3], [0], cfg=None) == -1 and call([3], [0], s=False) == -1
    bad = ldpc.params()
    bad.iters = 0
    assert call([3], [0], cfg=bad) == -1
    assert L.pysdr_ft8_decode(None, None, None, 0, C.byref(ldpc.params()), None, None, None) == -1
    with pytest.raises(_lib.PysdrError):
        sk.dec.decode([3], [done - 312])
    assert call([], [], n=0) == 0 and (st == 7).all()
    assert call([3, nf - 1], [0, done - 313]) == 0 and (st[:, 0] != 7).all()
    # gone from the ring: with max_out = 16 the ring holds 325 steps, and 347 are done
    sk16 = skimmer(max_out=16)
    sk16.push(coded_input())
    assert sk16.dec.tr == 325 and sk16.dec.t_done == 347
    with pytest.raises(_lib.PysdrError):
        sk16.dec.decode([3], [21])
    with pytest.raises(_lib.PysdrError):
        sk16.dec.llr([3], [21])
    assert sk16.dec.decode([3], [22])["status"].shape == (1,)
    sk16.close()


def test_the_skimmer_gives_the_three_texts_and_without_decode_the_records_of_today(pushed):
    from pysdr_amd import ft8, ldpc
    from pysdr_amd.channelizer import Channelizer
    sk, recs = pushed
    fs, channels, stations = g8.SHAPES[0]
    x = coded_input()
    assert len(recs) == 3
    for (f, snr, start), msg, text in zip(stations, messages(), TEXTS):
        near = [r for r in recs if abs(r["freq"] - f) <= 3.2 and abs(r["time"] - start) <= 0.25]
        assert len(near) == 1, (f, near)
        r = near[0]
        print(f"station {f} Hz {snr} dB: status {r['status']} after {r['iterations']} iterations, {r['nerr']} hard errors, text {r['text']!r}")
        assert r["ok"] and r["status"] == 2 and r["text"] == text and np.array_equal(r["bits77"], msg) and r["i3"] == 1
        assert r["nerr"] == int((ft8.hard_bits(r["llr"]) != ldpc.encode(msg)).sum())
    # decode off, the default: the records are the oracle skimmer's, key for key
    plain = skimmer()
    old = plain.push(x)
    plain.close()
    ch = Channelizer(fs, sk.M, sk.D, ft8.prototype(fs, sk.M, sk.S), channels, max_in=len(x))
    y = ch.push(x)
    ch.close()
    ref = fo.Skimmer(sk.nk, sk.S, False, 256).push(y)
    assert len(old) == len(ref) == 3
    for a, b, c in zip(old, ref, recs):
        assert sorted(a) == ["F", "freq", "hits", "llr", "score", "t0", "time"]
        assert (a["t0"], a["F"], a["hits"]) == (b["t0"], b["F"], b["hits"]) and fbits(F32(a["score"])) == fbits(F32(b["score"]))
        assert np.array_equal(fbits(a["llr"]), fbits(b["llr"]))
        for k in a:                                                             # and what decode=True adds sits beside them
            assert np.array_equal(a[k], c[k]), k
        assert sorted(set(c) - set(a)) == ["bits77", "i3", "iterations", "n3", "nerr", "ok", "status", "text"]
    # without the soft bits' download
    lean = skimmer(decode=True, keep_llr=False)
    got = lean.push(x)
    lean.close()
    assert [r["text"] for r in got] == [r["text"] for r in recs] and all("llr" not in r for r in got)
    assert [(r["t0"], r["F"], r["status"], r["iterations"], r["nerr"]) for r in got] == [(r["t0"], r["F"], r["status"], r["iterations"], r["nerr"]) for r in recs]


def test_ft4_frames_decode_from_their_ring():
    """tests/test_gpu_ft4.py's smallest shape with codewords on the air (this repository's FT4 has no scrambler: the bits
    decoded are the bits sent, and there is no text)"""
    from pysdr_amd import _lib, ldpc
    from pysdr_amd.ft4 import FT4_Skimmer
    fs, channels, stations = g4.SHAPES[0]
    n = int(g4.SECONDS * fs)
    rng = np.random.default_rng(500)
    x = f4o.noise_sigma(0.0, f4o.SNR_BW, fs) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for j, ((f, snr, start), msg) in enumerate(zip(stations, messages())):
        s = f4o.waveform(f4o.tones(ldpc.encode(msg)), f, fs, gfsk=j != 1, phase=1.0 + j) * 10 ** (snr / 20)
        at = int(start * fs)
        x[at:at + len(s)] += s[:n - at]
    x = (0.05 * x).astype(np.complex64)
    sk = FT4_Skimmer(fs, channels=channels, max_in=len(x), decode=True)
    # 470 steps in, the two earlier frames are whole, released and still in the ring (it holds 461 steps)
    recs = sk.push(x[:(sk.S + 469 * sk.qs) * sk.D])
    done, tr = sk.dec.t_done, sk.dec.tr
    assert (done, tr) == (470, 461)
    held = [r for r in recs if r["t0"] + 408 < done and done - r["t0"] <= tr]
    assert len(held) == len(recs) == 2
    rng = np.random.default_rng(4)
    F = np.array([r["F"] for r in held] + list(rng.integers(0, sk.nfine, 20)) + [0, sk.nfine - 1], np.int32)
    t0 = np.array([r["t0"] for r in held] + list(rng.integers(done - tr, done - 408, 20)) + [done - tr, done - 409], np.int64)
    st, bits, post = lo.decode(sk.dec.llr(F, t0))
    same(sk.dec.decode(F, t0, post=True), st, bits, post, "ft4")
    assert list(st[:2, 0]) == [2, 2] and (st[2:, 0] != 2).all()
    with pytest.raises(_lib.PysdrError):
        sk.dec.decode([0], [done - 408])
    with pytest.raises(_lib.PysdrError):
        sk.dec.decode([0], [done - tr - 1])
    recs = recs + sk.push(x[(sk.S + 469 * sk.qs) * sk.D:])
    assert len(recs) == 3
    for (f, snr, start), msg in zip(stations, messages()):
        near = [r for r in recs if abs(r["freq"] - f) <= g4.STEP / 2 + 0.1 and abs(r["time"] - (start + g4.RAMP + 0.008)) <= 0.03]
        assert len(near) == 1, (f, [(r["freq"], r["time"]) for r in recs])
        r = near[0]
        print(f"FT4 station {f:.1f} Hz {snr} dB: status {r['status']} after {r['iterations']} iterations, {r['nerr']} hard errors")
        assert r["ok"] and r["status"] == 2 and np.array_equal(r["bits77"], msg) and r["text"] is None
    sk.close()
