"""A-priori decoding on the GPU (pysdr_amd/csrc/ap.hip, ap_host.h, pysdr_amd/ap.py) against the oracle
of the definition (tests/ap_oracle.py): ap, bits and detail are EQUAL -- from host soft bits, and from the spectrum ring of
an FT8 and an FT4 skimmer at the weak levels tests/ap_cases.py records (picked on the CPU by tests/test_ap_oracle.py: min-sum
fails there and the right hypotheses rescue the frame), where the oracle is fed the skimmer's own soft bits.  Every refusal
leaves every output array as it was.  Then ``FT8_AP_Skimmer`` on 45 s: a CQ at a clean level and the same CQ two slots later
at the weak level."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import ap_cases as ac
from tests import ap_oracle as ao

pytestmark = pytest.mark.gpu

F32 = np.float32
pi32, pu8, pll = C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_longlong)


@pytest.fixture(scope="module")
def small():
    """a skimmer of the smallest shape, for the calls that take soft bits from the host"""
    from pysdr_amd.ft8 import FT8_Skimmer
    sk = FT8_Skimmer(8000.0, channels=(3, 3), max_in=4096)
    yield sk
    sk.close()


def hyps5():
    from pysdr_amd import ap
    return [ap.hyp_cq(), ap.hyp_from("K1ABC"), ap.hyp_cq_from("K1ABC"), ap.hyp_text(ac.CQ), ap.hyp_from("W9XYZ")]


@functools.lru_cache(maxsize=None)
def six():
    """6 candidates, 5 hypotheses, 13 pairs: a right hypothesis and a wrong one; two right ones that tie; a candidate with
    no pair; four kinds up to the full 77 bits, of which the last two decode; all-zero soft bits; noise.  Computed once, never changed."""
    from pysdr_amd import ldpc
    rng = np.random.default_rng(6)
    cw = 2.0 * ldpc.encode(ac.cq_bits()) - 1
    llr = np.array([cw + 1.0 * rng.standard_normal(174), 3.0 * cw, cw + 0.5 * rng.standard_normal(174), cw + 0.9 * rng.standard_normal(174),
                    np.zeros(174), rng.standard_normal(174)]).astype(F32)
    pairs = np.array([(0, 0), (0, 4), (1, 0), (1, 1), (3, 0), (3, 1), (3, 2), (3, 3), (4, 0), (4, 3), (4, 4), (5, 2), (5, 4)], np.int32)
    llr.setflags(write=False)
    pairs.setflags(write=False)
    return llr, pairs


@functools.lru_cache(maxsize=None)
def want_six(iters):
    llr, pairs = six()
    return ao.decode(llr, hyps5(), pairs, iters=iters)


def check_six(want):
    """the cases of ``six`` are what their names say (on the oracle's answer at iters 30)"""
    from pysdr_amd import ldpc
    ap_w, bits_w, d = want[0], want[1], want[2]
    assert list(d[:2, 0]) == [2, 0] and ap_w[0, 0] == 0                         # a right hypothesis, a wrong one
    assert list(d[2:4, 0]) == [2, 2] and d[2, 2] == d[3, 2] and list(ap_w[1]) == [2, 0, d[2, 2], 2]   # a tie goes to the lower pair
    assert list(ap_w[2]) == [-1, 0, 0, 0] and not bits_w[2].any()               # no pair
    assert list(d[4:8, 0]) == [0, 0, 2, 2] and d[7, 2] < d[6, 2] and list(ap_w[3]) == [7, d[7, 1], d[7, 2], 2]   # the least nerr wins: the full 77 bits
    assert list(d[8:11, 0]) == [1, 1, 1] and (d[8:11, 3] > 0).all() and ap_w[4, 0] == -1   # zeros: the zero codeword, which no value agrees with
    assert ap_w[5, 0] == -1
    assert np.array_equal(ldpc.unpack_bits(bits_w[[0, 1, 3]])[:, :77], np.tile(ac.cq_bits(), (3, 1)))


def same(got, want, pairs, where):
    from pysdr_amd import ldpc
    ap_w, bits_w, detail_w, _ = want
    assert np.array_equal(got["pair"], ap_w[:, 0]), (where, got["pair"], ap_w[:, 0])
    assert np.array_equal(got["iterations"], ap_w[:, 1]) and np.array_equal(got["nerr"], ap_w[:, 2]) and np.array_equal(got["count"], ap_w[:, 3]), where
    assert np.array_equal(got["bits"], ldpc.unpack_bits(bits_w)), where
    assert np.array_equal(got["detail"], detail_w), (where, np.argwhere(got["detail"] != detail_w)[:5])
    pairs = np.asarray(pairs).reshape(-1, 2)
    assert np.array_equal(got["hyp"], [pairs[p, 1] if p >= 0 else -1 for p in ap_w[:, 0]]), where


@pytest.mark.parametrize("iters", (1, 30))
def test_host_soft_bits_equal_the_oracle(small, iters):
    from pysdr_amd import ap, ldpc
    llr, pairs = six()
    want = want_six(iters)
    if iters == 30:
        check_six(want)
    got = ap.decode_llr(small.dec, llr, pairs, hyps5(), ldpc=ldpc.params(iters=iters), detail=True)
    same(got, want, pairs, iters)
    plain = ap.decode_llr(small.dec, llr, pairs, hyps5(), ldpc=ldpc.params(iters=iters))
    assert "detail" not in plain and np.array_equal(plain["pair"], got["pair"]) and np.array_equal(plain["bits"], got["bits"])


@functools.lru_cache(maxsize=None)
def many():
    """193 candidates of tests/test_gpu_ldpc.py's mixture, each with a random subset of eight hypotheses; every sixteenth
    also with its own hard bits under the masks of 61 and of 32 bits"""
    from tests.test_gpu_ldpc import soft_inputs
    rng = np.random.default_rng(193)
    llr = soft_inputs()[:193]
    hyps = hyps5() + [ao.hyp(rng.integers(0, 2, 77) | np.eye(77, dtype=np.int64)[k], rng.integers(0, 2, 77)) for k in (0, 40, 76)]
    pairs = [(c, h) for c in range(193) for h in range(8) if rng.random() < 0.3]
    for c in range(0, 193, 16):
        for k in (2, 1):
            pairs.append((c, len(hyps)))
            hyps.append(ao.hyp(ao.unword(hyps[k][0])[:77], llr[c, :77] > 0))
    pairs = np.array(sorted(pairs), np.int32)
    pairs.setflags(write=False)
    return llr, hyps, pairs


def test_more_candidates_than_a_workgroup_of_the_pick_and_the_settings(small):
    """193 candidates of tests/test_gpu_ldpc.py's mixture (codewords at five noise levels, noise, a broken CRC, zeros, some
    near 1e18), each with a random subset of eight hypotheses, under three settings"""
    from pysdr_amd import ap, ldpc
    llr, hyps, pairs = many()
    for mag, nerr_max, iters in ((1.0, 174, 30), (0.25, 20, 30), (16.0, 0, 5)):
        want = ao.decode(llr, hyps, pairs, mag=mag, nerr_max=nerr_max, iters=iters)
        got = ap.decode_llr(small.dec, llr, pairs, hyps, ap.params(mag, nerr_max), ldpc.params(iters=iters), detail=True)
        same(got, want, pairs, (mag, nerr_max, iters))
        if nerr_max == 174:
            assert set(want[2][:, 0]) == {0, 1, 2} and (want[0][:, 3] > 1).any() and (want[0][:, 0] == -1).any()
    none = ap.decode_llr(small.dec, llr[:3], np.zeros((0, 2), np.int32), hyps, detail=True)     # candidates, and not one pair
    assert list(none["pair"]) == [-1] * 3 and not none["bits"].any() and none["detail"].shape == (0, 4)


def test_every_refusal_of_host_soft_bits_leaves_the_outputs_untouched(small):
    from pysdr_amd import _lib, ap, ldpc
    L, h = _lib.lib(), small.dec._h
    llr, pairs = (np.array(v) for v in six())
    tab = ap.table(hyps5())
    out, bits, detail = np.full((6, 4), 7, np.int32), np.full((6, 12), 7, np.uint8), np.full((13, 4), 7, np.int32)

    def call(x=llr, n=6, t=tab, H=5, p=pairs, P=13, cfg=ldpc.params(), apc=ap.params(), o=True, b=True):
        rc = L.pysdr_ft8_decode_llr_ap(h, None if x is None else _lib.as_pf(x), n, None if t is None else t.ctypes.data_as(pu8), H,
                                       None if p is None else p.ctypes.data_as(pi32), P, None if cfg is None else C.byref(cfg),
                                       None if apc is None else C.byref(apc), out.ctypes.data_as(pi32) if o else None,
                                       bits.ctypes.data_as(pu8) if b else None, detail.ctypes.data_as(pi32))
        if rc != 0:
            assert (out == 7).all() and (bits == 7).all() and (detail == 7).all()
        return rc

    assert call(n=-1) == -1 and call(n=4097) == -1 and b"pysdr_ft8_decode_llr_ap" in L.pysdr_last_error()
    assert call(x=None) == -1 and call(cfg=None) == -1 and call(apc=None) == -1 and call(o=False) == -1 and call(b=False) == -1
    assert call(t=None) == -1 and call(p=None) == -1 and call(H=0) == -1 and call(H=4097) == -1 and call(P=-1) == -1 and call(P=65537) == -1
    for k, v in (("iters", 0), ("iters", 201), ("alpha", 0.0), ("alpha", float("nan"))):
        c = ldpc.params()
        setattr(c, k, v)
        assert call(cfg=c) == -1, (k, v)
    for mag, nerr_max in ((0.2, 174), (17.0, 174), (float("nan"), 174), (float("inf"), 174), (1.0, -1), (1.0, 175)):
        assert call(apc=ap.params(mag, nerr_max)) == -1 and b"ap cfg" in L.pysdr_last_error(), (mag, nerr_max)
    for byte, v in ((0, 0), (9, 0x04), (10, 0x80), (11, 0x01)):                 # an empty mask (hyp_cq's lies in bytes 0 to 3 and 9), bits 77, 80 and 95
        t = tab.copy()
        if v == 0:
            t[0, :12] = 0
            t[0, 12:] = 0
        else:
            t[2, byte] |= v
        assert call(t=t) == -1 and b"hypothesis" in L.pysdr_last_error(), (byte, v)
    t = tab.copy()
    t[4, 12 + 3] |= 0x10                                                        # a value bit outside hyp_from's mask (bits 29 .. 57, 74 .. 76)
    assert ao.unword(t[4, :12])[27] == 0 and call(t=t) == -1
    for bad in ([(0, 0), (0, 0)], [(1, 0), (0, 4)], [(0, 4), (0, 0)], [(6, 0), (6, 1)], [(0, 5), (1, 0)], [(-1, 0), (0, 0)], [(0, -1), (0, 0)]):
        p = pairs.copy()
        p[:2] = bad
        assert call(p=p) == -1 and b"pair" in L.pysdr_last_error(), bad
    assert call(H=4) == -1                                                      # the pairs name hypothesis 4
    for v in (np.nan, np.inf, -np.inf):
        x = llr.copy()
        x[5, 173] = v
        assert call(x=x) == -1 and b"not finite" in L.pysdr_last_error()
        with pytest.raises(_lib.PysdrError):
            ap.decode_llr(small.dec, x, pairs, hyps5())
    with pytest.raises(ValueError):
        ap.decode_llr(small.dec, llr, pairs[::-1], hyps5())
    assert call(n=0, P=0) == 0 and (out == 7).all() and (bits == 7).all()
    assert call(n=0) == -1                                                      # pairs without candidates
    assert L.pysdr_ft8_decode_llr_ap(None, _lib.as_pf(llr), 6, tab.ctypes.data_as(pu8), 5, pairs.ctypes.data_as(pi32), 13, C.byref(ldpc.params()),
                                     C.byref(ap.params()), out.ctypes.data_as(pi32), bits.ctypes.data_as(pu8), None) == -1
    want = want_six(30)
    assert call() == 0 and np.array_equal(out, want[0]) and np.array_equal(bits, want[1]) and np.array_equal(detail, want[2])


# ---- from the ring ------------------------------------------------------------------------------------------------------------

def at_station(recs, f, step):
    near = [r for r in recs if abs(r["freq"] - f) <= step / 2 + 0.1]
    assert len(near) == 1, [(r["freq"], r["t0"]) for r in recs]
    return near[0]


def ring_case(sk, rec, hyps, right):
    """the frame of ``rec`` and 12 other places of the ring, every one with every hypothesis, against the oracle on the
    skimmer's own soft bits, at iters 1 and 30; -> the answer at iters 30"""
    from pysdr_amd import ap, ldpc
    m = sk.DECODERS.MODE
    lag = m.STEPS_PER_SYMBOL * (m.SYMBOLS - 1)
    done, tr = sk.dec.t_done, sk.dec.tr
    rng = np.random.default_rng(9)
    F = np.array([rec["F"]] + list(rng.integers(0, sk.nfine, 10)) + [0, sk.nfine - 1], np.int32)
    t0 = np.array([rec["t0"]] + list(rng.integers(max(0, done - tr), done - lag - 1, 10)) + [max(0, done - tr), done - lag - 1], np.int64)
    pairs = np.array([(c, h) for c in range(len(F)) for h in range(len(hyps)) if c == 0 or (c + h) % 2], np.int32)
    soft = sk.dec.llr(F, t0)
    for iters in (1, 30):
        want = ao.decode(soft, hyps, pairs, iters=iters)
        got = ap.decode(sk.dec, F, t0, pairs, hyps, ldpc=ldpc.params(iters=iters), detail=True)
        same(got, want, pairs, (m.NAME, iters))
    assert list(got["detail"][:len(hyps), 0]) == [2] * right + [0] * (len(hyps) - right) and got["count"][0] == right
    return got


def test_ft8_candidates_from_the_ring_equal_the_oracle_and_the_weak_frame_is_rescued():
    from pysdr_amd import ft8, ldpc
    from pysdr_amd.ft8 import FT8_Skimmer
    x = ac.ft8_weak()
    sk = FT8_Skimmer(ac.FS, channels=ac.CHANNELS, max_in=len(x), decode=True)
    rec = at_station(sk.push(x), ac.FT8_F, ft8.BAUD / 2)
    assert (sk.dec.t_done, sk.dec.tr) == (347, 355) and not rec["ok"] and rec["status"] != 2       # min-sum fails at this level
    got = ring_case(sk, rec, hyps5(), 4)
    assert np.array_equal(got["bits"][0, :77], ac.cq_bits()) and got["hyp"][0] in (0, 1, 2, 3) and ldpc.crc_ok(got["bits"][0])
    print(f"FT8 {ac.FT8_WEAK} dB: min-sum status {rec['status']} after {rec['iterations']} iterations; pairs {got['detail'][:5].tolist()}")
    sk.close()


def test_ft4_candidates_from_the_ring_equal_the_oracle_and_the_weak_frame_is_rescued():
    from pysdr_amd import ap, ft4
    from pysdr_amd.ft4 import FT4_Skimmer
    from tests.test_ap_oracle import true_hyps
    x = ac.ft4_weak()
    sk = FT4_Skimmer(ac.FS, channels=ac.CHANNELS, max_in=len(x), decode=True)
    recs = sk.push(x[:(sk.S + 469 * sk.qs) * sk.D])                             # 470 steps in: the frame is whole, released and still in the ring
    assert (sk.dec.t_done, sk.dec.tr) == (470, 461)
    rec = at_station(recs, ac.FT4_F, ft4.BAUD)
    assert not rec["ok"] and rec["status"] != 2
    got = ring_case(sk, rec, true_hyps(ac.ft4_bits()) + [ap.hyp_text(ac.CQ)], 3)
    assert np.array_equal(got["bits"][0, :77], ac.ft4_bits())
    print(f"FT4 {ac.FT4_WEAK} dB: min-sum status {rec['status']} after {rec['iterations']} iterations; pairs {got['detail'][:4].tolist()}")
    sk.close()


def test_every_refusal_of_candidates_from_the_ring_leaves_the_outputs_untouched():
    from pysdr_amd import _lib, ap, ldpc
    from pysdr_amd.ft8 import FT8_Skimmer
    x = ac.ft8_weak()
    sk = FT8_Skimmer(ac.FS, channels=ac.CHANNELS, max_in=len(x))
    sk.push(x)
    L, h, done, nf = _lib.lib(), sk.dec._h, sk.dec.t_done, sk.nfine
    tab = ap.table(hyps5())
    out, bits, detail = np.full((2, 4), 7, np.int32), np.full((2, 12), 7, np.uint8), np.full((3, 4), 7, np.int32)

    def call(F, t0, n=None, p=((0, 0), (0, 3), (1, 1)), P=3, cfg=ldpc.params(), apc=ap.params(), o=True):
        F, t0, p = np.array(F, np.int32), np.array(t0, np.int64), np.array(p, np.int32)
        rc = L.pysdr_ft8_decode_ap(h, F.ctypes.data_as(pi32), t0.ctypes.data_as(pll), len(F) if n is None else n, tab.ctypes.data_as(pu8), 5,
                                   p.ctypes.data_as(pi32), P, None if cfg is None else C.byref(cfg), None if apc is None else C.byref(apc),
                                   out.ctypes.data_as(pi32) if o else None, bits.ctypes.data_as(pu8), detail.ctypes.data_as(pi32))
        if rc != 0:
            assert (out == 7).all() and (bits == 7).all() and (detail == 7).all()
        return rc

    assert call([3, 3], [0, done - 312]) == -5 and b"pysdr_ft8_decode_ap" in L.pysdr_last_error()   # the second frame's last step is not in
    assert call([3, 3], [-1, 0]) == -5 and call([-1, 3], [0, 0]) == -1 and call([3, nf], [0, 0]) == -1
    assert call([3, 3], [0, 0], n=-1) == -1 and call([3, 3], [0, 0], n=4097) == -1 and call([3, 3], [0, 0], cfg=None) == -1
    assert call([3, 3], [0, 0], apc=None) == -1 and call([3, 3], [0, 0], o=False) == -1 and call([3, 3], [0, 0], apc=ap.params(mag=0.1)) == -1
    assert call([3, 3], [0, 0], p=((0, 0), (2, 0), (2, 1))) == -1 and call([3, 3], [0, 0], p=((0, 3), (0, 0), (1, 1))) == -1
    assert call([3], [0]) == -1                                                 # a pair names candidate 1 of 1
    assert L.pysdr_ft8_decode_ap(None, None, None, 0, tab.ctypes.data_as(pu8), 5, None, 0, C.byref(ldpc.params()), C.byref(ap.params()), None, None, None) == -1
    with pytest.raises(_lib.PysdrError):
        ap.decode(sk.dec, [3], [done - 312], [(0, 0)], hyps5())
    assert call([], [], n=0, P=0) == 0 and (out == 7).all()
    assert call([3, nf - 1], [0, done - 313]) == 0 and (out[:, 0] != 7).all() and (detail[:, 0] != 7).all()
    sk.close()


# ---- the skimmer --------------------------------------------------------------------------------------------------------------

def test_the_skimmer_rescues_the_weak_cq_from_what_it_heard_two_slots_earlier():
    from pysdr_amd import ap, ft8
    from pysdr_amd.ft8 import FT8_Skimmer
    x = ac.skimmer_stream()
    kw = dict(channels=ac.CHANNELS, max_in=1 << 16, decode=True)
    runs = {}
    for name, make in (("ap", lambda: ap.FT8_AP_Skimmer(ac.FS, ap=ap.params(), **kw)), ("none", lambda: ap.FT8_AP_Skimmer(ac.FS, ap=None, **kw)),
                       ("plain", lambda: FT8_Skimmer(ac.FS, **kw))):
        sk = make()
        runs[name] = [r for i in range(0, len(x), 1 << 16) for r in sk.push(x[i:i + (1 << 16)])]
        sk.close()
    step = sk.qs * sk.D / ac.FS
    for name, recs in runs.items():
        cq = sorted((r for r in recs if abs(r["freq"] - ac.FT8_F) <= ft8.BAUD / 4 + 0.1 and min(abs(r["t0"] * step - s) for s in (0.5, 30.5)) <= 0.1),
                    key=lambda r: r["t0"])
        assert len(cq) == 2 and cq[1]["t0"] - cq[0]["t0"] == 750, (name, [(r["t0"], r["F"]) for r in recs])
        print(name, [(r["t0"], r["F"], r["ok"], r.get("ap"), r["text"]) for r in recs])
        if name == "ap":
            good = [r for r in recs if r["ok"]]
            assert [id(r) for r in good] == [id(r) for r in cq] and cq[0]["text"] == cq[1]["text"] == ac.CQ and cq[0]["ap"] == 0 and cq[1]["ap"] == 5
            assert cq[1]["status"] == 2 and np.array_equal(cq[1]["bits77"], ac.cq_bits()) and (cq[1]["i3"], cq[1]["n3"]) == (cq[0]["i3"], cq[0]["n3"])
            assert all(r["ap"] == -1 for r in recs if not r["ok"])              # the others were tried, with CQ ? ? at the least, in vain
        else:
            assert cq[0]["ok"] and cq[0]["text"] == ac.CQ and not cq[1]["ok"] and cq[1]["text"] is None and [id(r) for r in recs if r["ok"]] == [id(cq[0])]
            assert all("ap" not in r for r in recs)
    assert len(runs["none"]) == len(runs["plain"]) == len(runs["ap"])
    for a, b, c in zip(runs["none"], runs["plain"], runs["ap"]):                # ap=None is an FT8_Skimmer, key for key
        assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
        assert (a["t0"], a["F"]) == (c["t0"], c["F"]) and np.array_equal(a["llr"], c["llr"])
