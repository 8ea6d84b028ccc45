"""Ordered-statistics decoding behind min-sum on the GPU (pysdr_amd/csrc/osd.hip, ldpc_host.h) against the
NumPy oracle of the definition (tests/osd_oracle.py): status (all four columns), the packed bits and detail -- the winner's
index, the last rank of the basis, the pattern's weight and the bits of its float32 distance -- are EQUAL, and post is
min-sum's: from host soft bits, across a chunk boundary, and from the spectrum ring of an FT8 and an FT4 skimmer, where the
oracle is fed the skimmer's own soft bits.  With ``osd=None`` the calls and the skimmer answer what they answered before.
Then the skimmer with ``osd=2`` on a stream whose weak stations only the second stage decodes."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import ft4_oracle as f4o
from tests import ft8_oracle as fo
from tests import ldpc_oracle as lo
from tests import osd_oracle as oo
from tests import test_ft8_oracle as t8
from tests import test_gpu_ft4 as g4
from tests import test_gpu_ldpc as gl
from tests.test_gpu_psk import fbits

pytestmark = pytest.mark.gpu

F32 = np.float32
pi32, pu8, pll = C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_longlong)
ORDERS = (0, 1, 2)


# ---- from host soft bits ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def soft_inputs():
    """313 words: clean codewords, codewords at sigma 0.8 / 0.9 / 1.0 / 1.1, noise alone, words with a broken CRC, zeros (and
    -0), words of +-1 only; every third one scaled to near 1e18; shuffled; computed once, never changed"""
    from pysdr_amd import ldpc
    rng = np.random.default_rng(25)
    out = []

    def cw():
        return 2.0 * ldpc.encode(rng.integers(0, 2, 77)) - 1

    out += [cw() * rng.uniform(0.5, 2.0, 174) for _ in range(20)]
    for sigma, count in ((0.8, 60), (0.9, 70), (1.0, 50), (1.1, 40)):
        out += [cw() + sigma * rng.standard_normal(174) for _ in range(count)]
    out += [rng.standard_normal(174) for _ in range(50)]
    for i in range(10):
        b91 = ldpc.encode(rng.integers(0, 2, 77))[:91]
        b91[77 + i] ^= 1
        out.append((2.0 * ldpc.encode91(b91) - 1) * rng.uniform(1.0, 2.0, 174))
    out += [np.zeros(174), -np.zeros(174), np.zeros(174)]
    for i in range(10):
        v = cw()
        v[rng.choice(174, 12 + 2 * i, replace=False)] *= -1
        out.append(v)
    out = np.array(out)[rng.permutation(len(out))]
    out[::3] *= 2.4e17                                                          # |llr| up to about 1e18
    out = out.astype(F32)
    assert np.isfinite(out).all() and 5e17 < np.abs(out).max() <= 2e18
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want(order):
    st, bits, post, detail = oo.decode(soft_inputs(), order=order)
    for v in (st, bits, post, detail):
        v.setflags(write=False)
    return st, bits, post, detail


@functools.lru_cache(maxsize=None)
def covered():
    """the oracle's answers hold every case there is -- asserted on the CPU, once"""
    st, _, _, de = want(2)
    ran, ok = st[:, 3] > 0, st[:, 0] == 2
    assert (~ran).sum() > 50 and (~ran == (de[:, 0] == -1)).all() and (st[~ran, 0] == 2).all()
    for s3 in (1, 2, 3):
        assert (ran & ok & (st[:, 3] == s3)).any(), s3                          # run and accepted: no, one and two rows flipped
    assert (ran & ~ok).sum() > 50                                               # run and rejected
    assert (de[ran, 1] == 90).any() and (de[ran, 1] > 100).any() and (de[ran, 1] >= 90).all()
    assert (want(0)[0][:, 3] <= 1).all() and (want(1)[0][:, 3] <= 2).all()
    assert (want(0)[0][:, 0] == 2).sum() < (want(1)[0][:, 0] == 2).sum() < ok.sum()
    return True


def same(got, st, bits, post, detail, where):
    from pysdr_amd import ldpc
    for col, key in enumerate(("status", "iterations", "nerr", "osd")):
        assert np.array_equal(got[key], st[:, col]), (where, key, np.flatnonzero(got[key] != st[:, col])[:5])
    assert np.array_equal(got["bits"], ldpc.unpack_bits(bits)), where
    assert np.array_equal(got["detail"], detail), (where, np.flatnonzero((got["detail"] != detail).any(axis=1))[:5],
                                                   got["detail"][(got["detail"] != detail).any(axis=1)][:3], detail[(got["detail"] != detail).any(axis=1)][:3])
    assert np.array_equal(fbits(got["post"]), fbits(post)), where


@pytest.fixture(scope="module")
def small():
    """a skimmer of the smallest shape, for the calls that take soft bits from the host"""
    from pysdr_amd.ft8 import FT8_Skimmer
    sk = FT8_Skimmer(8000.0, channels=(3, 3), max_in=4096)
    yield sk
    sk.close()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n", (1, 3, 193, None))
def test_host_soft_bits_equal_the_oracle(small, n, order):
    assert covered()
    n = len(soft_inputs()) if n is None else n
    st, bits, post, detail = want(order)
    got = small.dec.decode_llr(soft_inputs()[:n], post=True, osd=order, detail=True)
    same(got, st[:n], bits[:n], post[:n], detail[:n], (n, order))
    if n == 3:
        from pysdr_amd import ldpc
        lean = small.dec.decode_llr(soft_inputs()[:n], osd=ldpc.osd_params(order))
        assert sorted(lean) == ["bits", "iterations", "nerr", "osd", "status"]
        assert all(np.array_equal(lean[k], got[k]) for k in lean)


def test_a_candidate_behind_a_chunk_boundary():
    """4097 words in one ``decode_llr`` call: two calls of the C ABI, the last of one word, which needs the second stage"""
    from pysdr_amd import ldpc
    from pysdr_amd.ft8 import FT8_Skimmer
    rng = np.random.default_rng(26)
    x = np.array([(2.0 * ldpc.encode(rng.integers(0, 2, 77)) - 1) * rng.uniform(0.5, 2.0, 174) for _ in range(4097)])
    hard = np.concatenate((rng.choice(4096, 99, replace=False), [4096]))
    x[hard] += 1.0 * rng.standard_normal((100, 174))
    x = x.astype(F32)
    st, bits, post, detail = oo.decode(x, order=2)
    assert st[4096, 3] > 0 and 50 < (st[:, 3] > 0).sum() <= 100 and (st[:, 3] == 0).sum() >= 3997
    sk = FT8_Skimmer(8000.0, channels=(3, 3), max_in=4096)
    got = sk.dec.decode_llr(x, post=True, osd=2, detail=True)
    sk.close()
    same(got, st, bits, post, detail, "4097")


def test_with_osd_none_the_calls_answer_what_they_answered(small):
    x = soft_inputs()[:40]
    st, bits, post = lo.decode(x)
    a, b = small.dec.decode_llr(x), small.dec.decode_llr(x, post=True, osd=None, detail=False)
    assert sorted(a) == ["bits", "iterations", "nerr", "status"] and sorted(b) == ["bits", "iterations", "nerr", "post", "status"]
    gl.same(b, st, bits, post, "osd=None")
    assert all(np.array_equal(a[k], b[k]) for k in a)
    with pytest.raises(ValueError):
        small.dec.decode_llr(x, detail=True)                                    # detail is the second stage's


def test_every_refusal_of_host_soft_bits_leaves_the_outputs_untouched(small):
    from pysdr_amd import _lib, ldpc
    L, h = _lib.lib(), small.dec._h
    llr = np.array(soft_inputs()[:4])
    st, bits, post, de = np.full((4, 4), 7, np.int32), np.full((4, 12), 7, np.uint8), np.full((4, 174), 7.0, F32), np.full((4, 4), 7, np.int32)

    def call(x=llr, n=4, cfg=ldpc.params(), s=True, b=True, osd=ldpc.osd_params(), d=True):
        rc = L.pysdr_ft8_decode_llr_osd(h, None if x is None else _lib.as_pf(x), n, None if cfg is None else C.byref(cfg),
                                        st.ctypes.data_as(pi32) if s else None, bits.ctypes.data_as(pu8) if b else None, _lib.as_pf(post),
                                        None if osd is None else C.byref(osd), de.ctypes.data_as(pi32) if d else None)
        if rc != 0:
            assert (st == 7).all() and (bits == 7).all() and (post == 7.0).all() and (de == 7).all()
        return rc

    assert call(n=-1) == -1 and call(n=4097) == -1 and b"pysdr_ft8_decode_llr_osd" in L.pysdr_last_error()
    assert call(cfg=None) == -1 and call(x=None) == -1 and call(s=False) == -1 and call(b=False) == -1
    for k, v in (("iters", 0), ("iters", 201), ("alpha", 0.0), ("alpha", 1.25), ("alpha", float("nan"))):
        c = ldpc.params()
        setattr(c, k, v)
        assert call(cfg=c) == -1, (k, v)
    assert call(osd=None) == -1 and b"osd cfg" in L.pysdr_last_error()
    for order in (-1, 3, 1 << 20):
        assert call(osd=ldpc.osd_params(order)) == -1 and b"osd cfg" in L.pysdr_last_error()
        with pytest.raises(_lib.PysdrError):
            small.dec.decode_llr(llr, osd=ldpc.osd_params(order))
    for v in (np.nan, np.inf, -np.inf):
        x = llr.copy()
        x[3, 173] = v
        assert call(x=x) == -1 and b"not finite" in L.pysdr_last_error()
        with pytest.raises(_lib.PysdrError):
            small.dec.decode_llr(x, osd=2)
    assert call(n=0) == 0 and (st == 7).all() and (de == 7).all()
    assert L.pysdr_ft8_decode_llr_osd(None, _lib.as_pf(llr), 4, C.byref(ldpc.params()), st.ctypes.data_as(pi32), bits.ctypes.data_as(pu8), None,
                                      C.byref(ldpc.osd_params()), None) == -1
    w = want(2)
    assert call(d=False) == 0 and np.array_equal(st, w[0][:4]) and np.array_equal(bits, w[1][:4]) and (de == 7).all()   # detail may be NULL
    assert call() == 0 and np.array_equal(st, w[0][:4]) and np.array_equal(bits, w[1][:4]) and np.array_equal(de, w[3][:4])


# ---- from the ring ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pushed():
    """tests/test_gpu_ldpc.py's stream through a decoding skimmer with the second stage on"""
    sk = gl.skimmer(decode=True, osd=2)
    recs = sk.push(gl.coded_input())
    yield sk, recs
    sk.close()


def test_candidates_from_the_ft8_ring_equal_the_oracle_on_the_skimmers_own_soft_bits(pushed):
    sk, recs = pushed
    done, tr = sk.dec.t_done, sk.dec.tr
    assert (done, tr) == (347, 355) and len(recs) == 3
    rng = np.random.default_rng(7)                                              # tests/test_gpu_ldpc.py's 65 candidates
    F = np.array([r["F"] for r in recs] + list(rng.integers(0, sk.nfine, 60)) + [0, sk.nfine - 1], np.int32)
    t0 = np.array([r["t0"] for r in recs] + list(rng.integers(0, done - 312, 60)) + [0, done - 313], np.int64)
    soft = sk.dec.llr(F, t0)
    for order in ORDERS:
        st, bits, post, detail = oo.decode(soft, order=order)
        same(sk.dec.decode(F, t0, post=True, osd=order, detail=True), st, bits, post, detail, ("ft8", order))
        assert list(st[:3, 3]) == [0, 0, 0] and (st[3:, 3] > 0).sum() > 50
    assert all(r["osd"] == 0 and r["ok"] for r in recs) and sorted(r["text"] for r in recs) == sorted(gl.TEXTS)


def test_every_refusal_of_candidates_from_the_ring(pushed):
    from pysdr_amd import _lib, ldpc
    sk, _ = pushed
    L, h, done, nf = _lib.lib(), sk.dec._h, sk.dec.t_done, sk.nfine
    st, bits, post, de = np.full((2, 4), 7, np.int32), np.full((2, 12), 7, np.uint8), np.full((2, 174), 7.0, F32), np.full((2, 4), 7, np.int32)

    def call(F, t0, n=None, cfg=ldpc.params(), s=True, osd=ldpc.osd_params()):
        F, t0 = np.array(F, np.int32), np.array(t0, np.int64)
        rc = L.pysdr_ft8_decode_osd(h, F.ctypes.data_as(pi32), t0.ctypes.data_as(pll), len(F) if n is None else n, None if cfg is None else C.byref(cfg),
                                    st.ctypes.data_as(pi32) if s else None, bits.ctypes.data_as(pu8), _lib.as_pf(post),
                                    None if osd is None else C.byref(osd), de.ctypes.data_as(pi32))
        if rc != 0:
            assert (st == 7).all() and (bits == 7).all() and (post == 7.0).all() and (de == 7).all()
        return rc

    assert call([3, 3], [0, done - 312]) == -5 and b"pysdr_ft8_decode_osd" in L.pysdr_last_error()
    assert call([3], [-1]) == -5 and call([-1], [0]) == -1 and call([3, nf], [0, 0]) == -1
    assert call([3], [0], n=-1) == -1 and call([3], [0], n=4097) == -1 and call([3], [0], cfg=None) == -1 and call([3], [0], s=False) == -1
    bad = ldpc.params()
    bad.iters = 0
    assert call([3], [0], cfg=bad) == -1
    assert call([3], [0], osd=None) == -1 and call([3], [0], osd=ldpc.osd_params(3)) == -1 and call([3], [0], osd=ldpc.osd_params(-1)) == -1
    assert L.pysdr_ft8_decode_osd(None, None, None, 0, C.byref(ldpc.params()), None, None, None, C.byref(ldpc.osd_params()), None) == -1
    with pytest.raises(_lib.PysdrError):
        sk.dec.decode([3], [done - 312], osd=2)
    assert call([], [], n=0) == 0 and (st == 7).all() and (de == 7).all()
    assert call([3, nf - 1], [0, done - 313]) == 0 and (st[:, 0] != 7).all() and (de != 7).all()


def test_candidates_from_the_ft4_ring_equal_the_oracle():
    """the stream of tests/test_gpu_ldpc.py::test_ft4_frames_decode_from_their_ring"""
    from pysdr_amd import ldpc
    from pysdr_amd.ft4 import FT4_Skimmer
    fs, channels, stations = g4.SHAPES[0]
    n = int(g4.SECONDS * fs)
    rng = np.random.default_rng(500)
    x = f4o.noise_sigma(0.0, f4o.SNR_BW, fs) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for j, ((f, snr, start), msg) in enumerate(zip(stations, gl.messages())):
        s = f4o.waveform(f4o.tones(ldpc.encode(msg)), f, fs, gfsk=j != 1, phase=1.0 + j) * 10 ** (snr / 20)
        at = int(start * fs)
        x[at:at + len(s)] += s[:n - at]
    x = (0.05 * x).astype(np.complex64)
    sk = FT4_Skimmer(fs, channels=channels, max_in=len(x), decode=True, osd=ldpc.osd_params(2))
    recs = sk.push(x[:(sk.S + 469 * sk.qs) * sk.D])
    done, tr = sk.dec.t_done, sk.dec.tr
    assert (done, tr) == (470, 461) and len(recs) == 2 and all(r["ok"] and r["osd"] == 0 and r["text"] is None for r in recs)
    rng = np.random.default_rng(4)
    F = np.array([r["F"] for r in recs] + list(rng.integers(0, sk.nfine, 20)) + [0, sk.nfine - 1], np.int32)
    t0 = np.array([r["t0"] for r in recs] + list(rng.integers(done - tr, done - 408, 20)) + [done - tr, done - 409], np.int64)
    soft = sk.dec.llr(F, t0)
    for order in ORDERS:
        st, bits, post, detail = oo.decode(soft, order=order)
        same(sk.dec.decode(F, t0, post=True, osd=order, detail=True), st, bits, post, detail, ("ft4", order))
        assert list(st[:2, 3]) == [0, 0] and (st[2:, 3] > 0).sum() >= 15
    sk.close()


# ---- the skimmer: one strong station and four weak ones --------------------------------------------------------------------

FS, CHANNELS, SECONDS = 8000.0, (3, 3), 15.0
STREAM_SEED = 2                                  # of seeds 1 to 8, 2 and 7 leave two weak stations to the second stage alone
# (fine row of tone 0, SNR dB in 2500 Hz, start s, text): on different rows and starts, 60 Hz and more apart
STATIONS = ((4, 0.0, 0.5, "CQ K1ABC FN42"), (24, -18.0, 0.2, "K1ABC W9XYZ -12"), (43, -18.5, 0.8, "W9XYZ K1ABC RR73"),
            (62, -19.0, 1.1, "CQ DX W9XYZ EN52"), (81, -19.5, 0.35, "W9XYZ K1ABC 73"))


@functools.lru_cache(maxsize=None)
def weak_stream(seed=STREAM_SEED):
    """-> (complex64 stream, the stations' (Hz, dB, start, text, message bits))"""
    from pysdr_amd import ft8msg, ldpc
    S, D, M = 64, 20, 80
    ff = fo.fine_freqs(FS, M, S, CHANNELS)
    n = int(SECONDS * FS)
    rng = np.random.default_rng(seed)
    x = fo.noise_sigma(0.0, fo.SNR_BW, FS) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    sent = []
    for j, (F, snr, start, text) in enumerate(STATIONS):
        msg = ft8msg.pack77(text)
        s = fo.waveform(fo.tones(ldpc.encode(msg)), ff[F], FS, True, phase=0.7 * j) * 10 ** (snr / 20)
        at = int(start * FS)
        x[at:at + len(s)] += s[:n - at]
        sent.append((float(ff[F]), snr, start, text, msg))
    x = (0.05 * x).astype(np.complex64)
    x.setflags(write=False)
    return x, tuple(sent)


def judge(recs, sent):
    """records with status, osd and bits77 -> (texts decoded by min-sum, texts decoded only by the second stage, records that
    carry a message that was not sent)"""
    first, second, wrong = [], [], 0
    for r in recs:
        if r["status"] != 2:
            continue
        hit = [s for s in sent if np.array_equal(r["bits77"], s[4]) and abs(r["freq"] - s[0]) <= 3.2 and abs(r["time"] - s[2]) <= 0.25]
        if not hit:
            wrong += 1
        else:
            (second if r["osd"] > 0 else first).append(hit[0][3])
    return first, second, wrong


@functools.lru_cache(maxsize=None)
def oracle_chain(seed=STREAM_SEED):
    """the float64 channelizer, the oracle skimmer, min-sum and the second stage on the CPU -> ``judge``'s answer"""
    from pysdr_amd import ldpc
    x, sent = weak_stream(seed)
    rows = t8.rows_behind_the_channelizer(np.asarray(x, np.complex128), FS, 64, 20, 80, CHANNELS)
    sk = fo.Skimmer(3, 64, False)
    sk.push(rows)
    ff = fo.fine_freqs(FS, 80, 64, CHANNELS)
    st, bits, _, _ = oo.decode(np.array([r["llr"] for r in sk.records]), order=2)
    recs = [dict(status=int(s[0]), osd=int(s[3]), bits77=b[:77], freq=float(ff[r["F"]]), time=16 * r["t0"] / 400.0)
            for r, s, b in zip(sk.records, st, ldpc.unpack_bits(bits))]
    return judge(recs, sent)


def test_the_skimmer_decodes_weak_stations_only_through_the_second_stage():
    from pysdr_amd import ft8msg, ldpc
    from pysdr_amd.ft8 import FT8_Skimmer
    x, sent = weak_stream()
    first, second, wrong = oracle_chain()
    print(f"oracle chain, seed {STREAM_SEED}: min-sum {first}, only through the second stage {second}, not sent {wrong}")
    assert "CQ K1ABC FN42" in first and len(second) >= 2 and wrong == 0        # the choice of the seed
    sk = FT8_Skimmer(FS, channels=CHANNELS, max_in=len(x), decode=True, osd=2)
    recs = sk.push(x)
    sk.close()
    assert len(recs) >= 3
    st, bits, _, _ = oo.decode(np.array([r["llr"] for r in recs]), order=2)     # every record against the oracle on its own soft bits
    for r, s, b in zip(recs, st, ldpc.unpack_bits(bits)):
        assert (r["status"], r["iterations"], r["nerr"], r["osd"]) == tuple(int(v) for v in s), (r["t0"], r["F"], s)
        assert np.array_equal(r["bits77"], b[:77]) and r["ok"] == (s[0] == 2)
        assert r["text"] == (ft8msg.unpack77(b[:77]) if s[0] == 2 else None)
    got1, got2, gotw = judge(recs, sent)
    print(f"GPU: min-sum {got1}, only through the second stage {got2}, not sent {gotw}")
    assert gotw == 0 and len(got2) >= 1 and "CQ K1ABC FN42" in got1
    assert all(r["text"] in [s[3] for s in sent] for r in recs if r["text"] is not None)
    # osd=None: the records of today, key for key
    plain = FT8_Skimmer(FS, channels=CHANNELS, max_in=len(x), decode=True)
    old = plain.push(x)
    plain.close()
    assert len(old) == len(recs)
    st0, bits0, _ = lo.decode(np.array([r["llr"] for r in old]))
    for a, c, s, b in zip(old, recs, st0, ldpc.unpack_bits(bits0)):
        assert sorted(a) == ["F", "bits77", "freq", "hits", "i3", "iterations", "llr", "n3", "nerr", "ok", "score", "status", "t0", "text", "time"]
        assert sorted(set(c) - set(a)) == ["osd"]
        assert (a["status"], a["iterations"], a["nerr"]) == tuple(int(v) for v in s[:3]) and np.array_equal(a["bits77"], b[:77])
        for k in ("t0", "F", "freq", "time", "score", "hits", "iterations"):
            assert a[k] == c[k], k
        assert np.array_equal(fbits(a["llr"]), fbits(c["llr"]))
    with pytest.raises(ValueError):
        FT8_Skimmer(FS, channels=CHANNELS, osd=2)
