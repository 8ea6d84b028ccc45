"""The second pass of the FT8 / FT4 skimmers on the GPU (pysdr_amd/csrc/pass.hip, pass_host.h) against the
NumPy model of the definition (tests/pass_oracle.py), which is fed the rows of an independent channelizer: the kept samples
and the residue ring, the four words of every job of a subtraction, the samples and the residue after it, and the events of
a rescan are EQUAL, floats by their bits -- on the 8000 Hz three-row FT8 shape with max_out = 64, whose stream wraps both
rings; for a frame inside one row, one whose tones spill into the next row, the first and the last row of the raster, a
frame that starts before sample 0, frames across the wrap of the sample ring, two overlapping frames of one row in both
orders, tied trials; on the full-circle raster of 80 rows with a frame on the last fine rows; on the 12000 Hz shape (S =
96) and on FT4.  Every refusal of the calls leaves outputs and rings untouched.  Then the skimmer with ``passes=2`` on a
weak station 9.4 Hz and 6 steps from a strong one: the weak one's text comes out with ``pass == 2``, the first pass's
records and ring are what they are without it, and two cuttings of the stream give the same records; and on a gaining pair
of tests/test_pass_oracle.py's grid the records are exactly the model skimmer's."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import ft4_oracle as f4o
from tests import ft8_oracle as fo
from tests import pass_oracle as po
from tests import test_gpu_ft4 as g4
from tests import test_gpu_ft8 as g8
from tests import test_gpu_ldpc as gl
from tests.test_gpu_psk import cut_rows, fbits

pytestmark = pytest.mark.gpu

F32 = np.float32
pi32, pu8, pll = C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_longlong)
SECONDS, REACH, MAX_OUT = 15.5, 16, 64
# (Hz of tone 0, dB in 2500 Hz, start s): a strong station, a weak one 3 fine rows above it and 6 steps later, a third apart
PAIR = ((300.0, 0.0, 0.5), (300.0 + 3 * 3.125, -12.0, 0.5 + 6 * 0.04), (455.0, -6.0, 0.7))


@functools.lru_cache(maxsize=None)
def pair_input():
    from pysdr_amd import ldpc
    fs = 8000.0
    n = int(SECONDS * fs)
    rng = np.random.default_rng(2700)
    x = fo.noise_sigma(0.0, fo.SNR_BW, fs) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for j, ((f, snr, start), msg) in enumerate(zip(PAIR, gl.messages())):
        s = fo.waveform(fo.tones(ldpc.encode(msg)), f, fs, phase=1.0 + j) * 10 ** (snr / 20)
        at = int(start * fs)
        x[at:at + len(s)] += s[:n - at]
    x = (0.05 * x).astype(np.complex64)
    x.setflags(write=False)
    return x


def cuts_of(n, D, max_out):
    cuts = [3, D * max_out - 3 - D + 1, 0, 1, D - 1]
    at = sum(cuts)
    while at < n:
        cuts.append(min(n - at, D * max_out))
        at += cuts[-1]
    return cuts


@functools.lru_cache(maxsize=None)
def stream(kind):
    """-> dict: the mode's modules, input, rows of an independent channelizer, shape; computed once, never changed"""
    from pysdr_amd import ft4, ft8
    from pysdr_amd.channelizer import Channelizer
    if kind == "pair":
        m, om, mode, fs, channels, x = ft8, fo, po.FT8, 8000.0, (3, 3), pair_input()
    elif kind == "circle":
        m, om, mode, (fs, channels, _), x = ft8, fo, po.FT8, g8.SHAPES[2], g8.make_input(2)
    elif kind == "s96":
        m, om, mode, (fs, channels, _), x = ft8, fo, po.FT8, g8.SHAPES[1], g8.make_input(1)
    else:
        m, om, mode, (fs, channels, _), x = ft4, f4o, po.FT4, g4.SHAPES[0], g4.make_input(0)
    S, D, M = m.shape(fs)
    ch = Channelizer(fs, M, D, m.prototype(fs, M, S), channels, max_in=len(x))
    y = ch.push(x)
    ch.close()
    y.setflags(write=False)
    return dict(m=m, om=om, mode=mode, fs=fs, channels=channels, x=x, y=y, S=S, D=D, M=M, nk=y.shape[0])


class Twin:
    """a skimmer that keeps, and the model beside it, fed the same calls"""

    def __init__(self, kind, reach=REACH, max_out=MAX_OUT, trials=9):
        c = stream(kind)
        self.c, m = c, c["m"]
        Sk = m.FT8_Skimmer if c["mode"] == po.FT8 else m.FT4_Skimmer
        self.sk = Sk(c["fs"], channels=c["channels"], max_in=len(c["x"]), max_out=max_out)
        self.plan = self.sk.dec.keep(reach, trials)
        self.p = po.PassOracle(c["mode"], c["om"].Oracle(c["nk"], c["S"], c["om"].params(), max_out), reach, c["nk"] == c["M"], trials)
        assert (self.plan["ty"], self.plan["tr2"]) == (self.p.ty, self.p.tr2)
        self.cuts = cuts_of(len(c["x"]), c["D"], max_out)
        self.rows = cut_rows(c["y"], self.cuts, c["D"])
        self.i = self.at = 0

    def feed(self, until=None):
        """calls until ``until`` steps are done (None: the whole stream)"""
        while self.i < len(self.cuts) and (until is None or self.p.o.t_done < until):
            n = self.cuts[self.i]
            self.sk.dec.decode_raw(self.c["x"][self.at:self.at + n], events=None)
            self.p.process(self.rows[self.i])
            self.at += n
            self.i += 1
        self.sk.dec.sync()
        return self

    def same(self, where):
        got, want = self.sk.dec.pass_state(), self.p.state()
        assert got["n_kept"] == want["n_kept"], where
        for k in ("yk", "ring2"):
            a, b = fbits(got[k].view(F32)) if k == "yk" else fbits(got[k]), fbits(want[k].view(F32)) if k == "yk" else fbits(want[k])
            assert a.shape == b.shape and np.array_equal(a, b), (where, k, np.argwhere(a != b)[:5])
        return got

    def subtract(self, F, t0, bits, trials, where):
        got = self.sk.dec.subtract(F, t0, bits, trials)
        want = self.p.subtract(F, t0, bits, trials)
        for k in ("before", "after"):
            assert np.array_equal(fbits(got[k]), fbits(want[k])), (where, k, got[k], want[k])
        for k in ("trial", "used"):
            assert np.array_equal(got[k], want[k]), (where, k, got[k], want[k])
        self.same(where)
        return got

    def rescan(self, F_lo, F_hi, t_lo, t_hi, cfg, p, where):
        got = self.sk.dec.rescan(F_lo, F_hi, t_lo, t_hi, cfg)
        want = self.p.rescan(F_lo, F_hi, t_lo, t_hi, p)
        assert [(e[0], e[1], e[3]) for e in got] == [(e[0], e[1], e[3]) for e in want], where
        assert np.array_equal(fbits([e[2] for e in got]), fbits([e[2] for e in want])), where
        return got

    def close(self):
        self.sk.close()


def words(rng, n):
    from pysdr_amd import ldpc
    return np.array([ldpc.encode(rng.integers(0, 2, 77))[:91] for _ in range(n)]).reshape(n, 91)


def grid(rng, n, qs, ntr=9):
    """random trials [n][ntr][2]: dn inside (-QS, QS), fw within about +-1 Hz of 400"""
    t = np.zeros((n, ntr, 2), np.int64)
    t[:, :, 0] = rng.integers(-(qs - 1), qs, (n, ntr))
    t[:, :, 1] = rng.integers(-(1 << 24), 1 << 24, (n, ntr))
    return (t & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def test_the_kept_rings_at_three_moments_of_a_stream_that_wraps_both():
    tw = Twin("pair")
    assert (tw.p.tr2, tw.p.ty, tw.sk.dec.tr) == (362, 5856, 331)
    for until in (120, 365, None):
        tw.feed(until)
        done = tw.p.o.t_done
        got = tw.same(done)
        ring = tw.sk.dec.state(ring=True)["ring"]
        t = np.arange(max(0, done - 331), done)                                   # the steps both rings hold
        assert np.array_equal(fbits(got["ring2"][:, t % 362]), fbits(ring[:, t % 331])), done
    assert done == 384 and got["n_kept"] == 6200 > 5856
    tw.close()


def test_subtractions_equal_the_model():
    rng = np.random.default_rng(271)
    from pysdr_amd import ft8, ldpc
    tw = Twin("pair").feed(340)
    done, nsub, qs = tw.p.o.t_done, 32, 16
    assert 340 <= done <= 344 and tw.p.first_step() == 0
    # a frame that starts before sample 0: every trial's dn is negative, the first symbol is left alone
    tr = grid(rng, 1, qs)
    tr[0, :, 0] = -rng.integers(1, qs, 9)
    got = tw.subtract([nsub + 15], [0], words(rng, 1), tr, "before sample 0")
    assert got["used"][0, 0] == 78 and got["used"][0, 1] == 0 and got["before"][0, 0] > got["after"][0, 0] > 0
    # the strong station itself, where its own bins hold most, with the skimmer's grid around the raster: most of it goes
    bits = np.array([ldpc.encode(gl.messages()[0])[:91]])
    Fs = int(np.argmin(np.abs(tw.sk.freqs_fine - PAIR[0][0])))
    tn = po.ro.frame_tones(po.FT8, bits[0])
    ts = max(range(0, 22), key=lambda t: po.frame_power(tw.p.ring2, tw.p.tr2, nsub, Fs, t, tn))
    got = tw.subtract([Fs], [ts], bits, ft8.trial_grid(ft8, 0.0, 0.0, qs, tw.sk.fs_out)[None], "the strong station")
    db = 10 * np.log10(got["after"][0, 0] / got["before"][0, 0])
    print(f"the strong station at F {Fs}, t0 {ts}: trial {got['trial'][0]}, {db:.1f} dB of its samples' power left (noise and two more stations stay)")
    assert db < -3.0
    tw.feed(None)
    done = tw.p.o.t_done
    lo, hi = tw.p.first_step() + 4, done - 312 - 4 - 1
    assert (done, lo, hi) == (384, 26, 67)
    # inside one row; tones that spill into the next row; into the row below; the first and the last row of the raster
    F = [nsub + 15, 20, 2 * nsub + 3, 5, 2 * nsub + 25, nsub + 31, nsub]
    t0 = [40, lo, hi, 50, 55, 60, 45]                                            # all of them cross the wrap of yk at sample 5856
    got = tw.subtract(F, t0, words(rng, len(F)), grid(rng, len(F), qs), "rows")
    assert [list(u) for u in got["used"]] == [[79, 0], [79, 79], [79, 79], [79, 0], [79, 0], [79, 79], [79, 79]]
    assert (got["before"][got["used"] > 0] > got["after"][got["used"] > 0]).all() and len(set(got["trial"][:, 0])) > 2
    # tied trials: the lowest index
    tr = grid(rng, 2, qs)
    tr[:, :, :] = tr[:, :1, :]
    got = tw.subtract([nsub + 9, 2 * nsub + 20], [33, 62], words(rng, 2), tr, "ties")
    assert (got["trial"] == 0).all()
    # a rescan of the whole raster over everything the residue holds, at settings that find plenty
    cfg, p = ft8.params(smin=1.2, hmin=6), fo.params(smin=1.2, hmin=6)
    ev = tw.rescan(0, 95, lo, hi, cfg, p, "rescan")
    assert len(ev) > 40 and min(e[0] for e in ev) <= lo + 4 and max(e[0] for e in ev) >= hi - 4
    assert tw.rescan(95, 95, hi, hi, cfg, p, "one place") is not None and tw.rescan(0, 0, lo, lo + 1, ft8.params(), fo.params(), "default") is not None
    # the residue decodes and gives soft bits as the model's residue says
    F, t0 = np.array([e[1] for e in ev[:20]], np.int32), np.array([e[0] for e in ev[:20]], np.int64)
    soft = tw.sk.dec.pass_llr(F, t0)
    assert np.array_equal(fbits(soft), fbits(np.array([tw.p.llr(int(f), int(t)) for f, t in zip(F, t0)])))
    a, b = tw.sk.dec.decode(F, t0, residual=True, post=True), tw.sk.dec.decode_llr(soft, post=True)
    for k in ("status", "iterations", "nerr", "bits"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(fbits(a["post"]), fbits(b["post"]))
    tw.close()


def test_two_frames_of_one_row_in_both_orders():
    rng = np.random.default_rng(272)
    bits, tr = words(rng, 2), grid(rng, 2, 16)
    F, t0 = [32 + 10, 32 + 12], [40, 41]
    out = []
    for order in ((0, 1), (1, 0)):
        tw = Twin("pair").feed(None)
        k = list(order)
        tw.subtract([F[i] for i in k], [t0[i] for i in k], bits[k], tr[k], order)
        out.append(tw.p.state())
        tw.close()
    assert not np.array_equal(out[0]["yk"], out[1]["yk"]) and not np.array_equal(out[0]["ring2"], out[1]["ring2"])


@pytest.mark.parametrize("kind", ("circle", "s96", "ft4"))
def test_the_other_shapes(kind):
    rng = np.random.default_rng(273)
    tw = Twin(kind, reach=8, max_out=256).feed(None)
    c, p = tw.c, tw.p
    nsub, qs, done, nfine = c["S"] // 2, c["S"] // 4, p.o.t_done, c["nk"] * (c["S"] // 2)
    lo, hi = max(0, p.first_step() + 4 if p.first_step() else 0), done - p.lag - 4 - 1
    assert hi >= lo + 4, (done, lo, hi)
    tw.same(kind)
    # the last fine rows (on the circle their tones spill into row 0), the first, a row's edge, and the ends in time
    F = [nfine - 1, nfine - 3, 0, nsub - 1, nsub, nfine // 2]
    t0 = [lo, hi, (lo + hi) // 2, lo + 1, hi - 1, lo + 2]
    got = tw.subtract(F, t0, words(rng, len(F)), grid(rng, len(F), qs), kind)
    if kind == "circle":
        assert (got["used"][:3] > 0).all() and p.circular                         # F = nfine - 1 and F = 0 both have a neighbour
    else:
        assert (got["used"][:3, 1] == 0).all() and (got["used"][3:5, 1] > 0).all()
    m, om = c["m"], c["om"]
    ev = tw.rescan(max(0, nfine - 40), nfine - 1, lo, hi, m.params(smin=1.2, hmin=5), om.params(smin=1.2, hmin=5), kind)
    ev += tw.rescan(0, 30, lo, hi, m.params(smin=1.2, hmin=5), om.params(smin=1.2, hmin=5), kind)
    assert len(ev) > 5
    tw.close()


def test_every_refusal_leaves_outputs_and_rings_untouched():
    from pysdr_amd import _lib, ft8, ldpc
    from pysdr_amd.ft8 import FT8_Skimmer
    L = _lib.lib()
    c = stream("pair")
    # without keep: ERR_STATE from every call; keep itself refuses a bad cfg, and a stream that has begun
    sk = FT8_Skimmer(c["fs"], channels=c["channels"], max_in=len(c["x"]), max_out=MAX_OUT)
    h = sk.dec._h
    out, cnt, ev = np.full((1, 2, 4), 7, np.int32), np.full(4, 7, np.int32), np.full((4, 52, 2), 7, np.int32)
    F, t0, bits, tr = np.array([40], np.int32), np.array([40], np.int64), np.zeros((1, 12), np.uint8), np.zeros((1, 9, 2), np.int32)
    st, b12 = np.full((1, 4), 7, np.int32), np.full((1, 12), 7, np.uint8)
    cfg, lc = ft8.params(), ldpc.params()
    pulse, lut = ft8.pass_pulse(ft8, 64), ft8.pass_lut()

    def keep(reach=16, trials=9, p=True, t=True):
        pc = _lib.PassCfg(reach_t=reach, trials=trials, pulse=pulse.ctypes.data_as(C.POINTER(C.c_uint32)) if p else None, lut=_lib.as_pf(lut) if t else None)
        return L.pysdr_ft8_keep(h, C.byref(pc))

    def sub(F=F, t0=t0, n=1, tr=tr, o=True, b=True):
        rc = L.pysdr_ft8_subtract(h, F.ctypes.data_as(pi32), t0.ctypes.data_as(pll), bits.ctypes.data_as(pu8) if b else None, tr.ctypes.data_as(pi32), n,
                                  out.ctypes.data_as(pi32) if o else None)
        assert rc == 0 or (out == 7).all()
        return rc

    def scan(F_lo=0, F_hi=3, t_lo=30, t_hi=40, cf=cfg, cn=True):
        rc = L.pysdr_ft8_rescan(h, F_lo, F_hi, C.c_longlong(t_lo), C.c_longlong(t_hi), C.byref(cf) if cf is not None else None,
                                cnt.ctypes.data_as(pi32) if cn else None, ev.ctypes.data_as(pi32))
        assert rc == 0 or ((cnt == 7).all() and (ev == 7).all())
        return rc

    def dec(F=F, t0=t0, n=1):
        rc = L.pysdr_ft8_pass_decode(h, F.ctypes.data_as(pi32), t0.ctypes.data_as(pll), n, C.byref(lc), st.ctypes.data_as(pi32), b12.ctypes.data_as(pu8),
                                     None, None, None)
        assert rc == 0 or ((st == 7).all() and (b12 == 7).all())
        return rc

    assert sub() == -5 and scan() == -5 and dec() == -5 and L.pysdr_ft8_pass_state(h, None, None, None) == -5 and b"keep" in L.pysdr_last_error()
    assert L.pysdr_ft8_pass_llr(h, F.ctypes.data_as(pi32), t0.ctypes.data_as(pll), 1, _lib.as_pf(np.zeros(174, F32))) == -5
    assert keep(0) == -1 and keep(121) == -1 and keep(16, 0) == -1 and keep(16, 10) == -1 and keep(p=False) == -1 and keep(t=False) == -1
    assert L.pysdr_ft8_keep(h, None) == -1 and L.pysdr_ft8_keep(None, None) == -1 and sub() == -5
    with pytest.raises(_lib.PysdrError):
        sk.dec.subtract([40], [40], np.zeros((1, 91)), np.zeros((1, 9, 2)))
    sk.dec.decode_raw(c["x"][:1000], events=None)
    assert keep() == -5                                                            # the stream has begun
    sk.dec.reset()
    assert keep() == 0 and keep() == 0                                             # after reset it may, and again
    sk.dec.kept = ft8.pass_plan(ft8, 3, 64, MAX_OUT, 16) | dict(trials=9)
    sk.push(c["x"])
    done = sk.dec.t_done
    assert done == 384
    before = sk.dec.pass_state()
    # frames not yet complete in, or gone from, what is kept; F outside the raster; n; a dn of a step or more; NULLs
    for t in (68, 25, -1, 400):
        assert sub(t0=np.array([t], np.int64)) == -5
    for t in (72, 21, -1):                                                         # (a decode needs the frame alone: t0 .. t0 + 312)
        assert dec(t0=np.array([t], np.int64)) == -5
    assert sub(F=np.array([-1], np.int32)) == -1 and sub(F=np.array([96], np.int32)) == -1 and sub(n=-1) == -1 and sub(n=257) == -1
    bad = tr.copy()
    bad[0, 8, 0] = 16
    assert sub(tr=bad) == -1 and sub(o=False) == -1 and sub(b=False) == -1 and L.pysdr_ft8_subtract(None, None, None, None, None, 0, None) == -1
    assert scan(t_lo=25) == -5 and scan(t_hi=68) == -5 and scan(t_lo=30, t_hi=30 + 248) == -1 and scan(t_lo=-1) == -1 and scan(t_lo=41) == -1
    assert scan(F_lo=-1) == -1 and scan(F_hi=96) == -1 and scan(F_lo=4, F_hi=3) == -1 and scan(cf=None) == -1 and scan(cn=False) == -1
    assert scan(cf=ft8.params(hmin=22)) == -1 and L.pysdr_ft8_rescan(None, 0, 3, C.c_longlong(30), C.c_longlong(40), C.byref(cfg), None, None) == -1
    assert dec(F=np.array([96], np.int32)) == -1 and dec(n=-1) == -1 and L.pysdr_ft8_pass_decode(None, None, None, 0, None, None, None, None, None, None) == -1
    after = sk.dec.pass_state()
    assert np.array_equal(before["yk"].view(F32).view(np.uint32), after["yk"].view(F32).view(np.uint32))
    assert np.array_equal(fbits(before["ring2"]), fbits(after["ring2"]))
    assert sub(n=0) == 0 and (out == 7).all() and scan() == 0 and (cnt[:4] != 7).all() and dec() == 0 and (st != 7).any()
    assert sub() == 0 and (out[0, 0, 3] == 79)
    sk.close()


def two_pass(cutting=None, **kw):
    from pysdr_amd.ft8 import FT8_Skimmer
    c = stream("pair")
    sk = FT8_Skimmer(c["fs"], channels=c["channels"], max_in=len(c["x"]), max_out=MAX_OUT, decode=True, **kw)
    recs, at = [], 0
    for n in (cutting or [len(c["x"])]):
        recs += sk.push(c["x"][at:at + n])
        at += n
    assert at == len(c["x"])
    ring = sk.dec.state(ring=True)["ring"]
    sk.close()
    return recs, ring


def same_records(a, b):
    assert len(a) == len(b)
    for r, s in zip(a, b):
        assert sorted(r) == sorted(s)
        for k in r:
            if isinstance(r[k], np.ndarray) and r[k].dtype == F32:
                assert np.array_equal(fbits(r[k]), fbits(s[k])), k
            else:
                assert np.array_equal(r[k], s[k]), k


def test_the_skimmer_finds_the_weak_station_under_the_strong_one():
    from pysdr_amd.ft8 import FT8_Skimmer
    n = len(pair_input())
    one, ring1 = two_pass()
    default, _ = two_pass(passes=1)
    two, ring2 = two_pass(passes=2, reach_t=REACH)
    cut, _ = two_pass([12345, 1, 40000, 7, 33333, n - 12345 - 1 - 40000 - 7 - 33333], passes=2, reach_t=REACH)
    for r in two + cut:
        print(r["pass"], r["t0"], r["F"], f"{r['score']:.2f}", r["hits"], r["status"], r["text"])
    same_records(one, default)
    assert all("pass" not in r for r in one)
    assert np.array_equal(fbits(ring1), fbits(ring2))                             # the first pass never sees a subtraction
    first = [r for r in two if r["pass"] == 1]
    same_records([{k: v for k, v in r.items() if k != "pass"} for r in first], one)
    texts1 = {r["text"] for r in one if r["ok"]}
    assert gl.TEXTS[0] in texts1 and gl.TEXTS[2] in texts1 and gl.TEXTS[1] not in texts1   # the weak station is lost to the strong one
    second = [r for r in two if r["pass"] == 2]
    assert [r["text"] for r in second] == [gl.TEXTS[1]] and second[0]["ok"] and second[0]["llr"].shape == (174,)
    assert abs(second[0]["freq"] - PAIR[1][0]) <= 3.2 and all(r["text"] in gl.TEXTS for r in two if r["ok"])
    key = lambda r: (r["t0"], r["F"], r["pass"])                                 # noqa: E731
    same_records(sorted(two, key=key), sorted(cut, key=key))
    # without passes=2 nothing is kept, so the process calls queue no pass kernel
    from pysdr_amd import _lib
    sk = FT8_Skimmer(8000.0, channels=(3, 3), decode=True, passes=1)
    sk.push(pair_input()[:20000])
    assert sk.dec.kept is None and _lib.lib().pysdr_ft8_pass_state(sk.dec._h, None, None, None) == -5
    sk.close()
    with pytest.raises(ValueError):
        FT8_Skimmer(8000.0, channels=(3, 3), passes=2)
    with pytest.raises(ValueError):
        FT8_Skimmer(8000.0, channels=(3, 3), decode=True, passes=3)
    with pytest.raises(ValueError):
        FT8_Skimmer(8000.0, channels=(3, 3), decode=True, passes=2, report=True)   # the report reads the first ring


def test_the_skimmer_gives_exactly_the_models_records_on_a_gaining_pair():
    """a pair of tests/test_pass_oracle.py's grid that gains there: the model skimmer on the rows of an independent
    channelizer against FT8_Skimmer(passes=2) on the same input, every record and every field the two share, floats by
    their bits -- the policy (order, trial grid, windows, the finder, the two filters) has a reference"""
    from pysdr_amd import ft8
    from pysdr_amd.channelizer import Channelizer
    from pysdr_amd.ft8 import FT8_Skimmer
    from tests import test_pass_oracle as tpo
    lvl, off = 12, 3
    assert (lvl, off) in tpo.GAINS
    x, msgs = tpo.pair_input(po.FT8, lvl, off)
    fs, channels = 8000.0, (3, 3)
    S, D, M = ft8.shape(fs)
    ch = Channelizer(fs, M, D, ft8.prototype(fs, M, S), channels, max_in=len(x))
    y = ch.push(x)
    ch.close()
    want = po.Skimmer(po.FT8, 3, S, False, MAX_OUT, 2).push(y)
    sk = FT8_Skimmer(fs, channels=channels, max_in=len(x), max_out=MAX_OUT, decode=True, passes=2)
    got = sk.push(x)
    sk.close()
    key = lambda r: (r["t0"], r["F"], r["pass"])                                 # noqa: E731
    got, want = sorted(got, key=key), sorted(want, key=key)
    for r in got:
        print(r["pass"], r["t0"], r["F"], f"{r['score']:.2f}", r["hits"], r["status"], r["text"])
    assert len(got) == len(want) and [key(r) for r in got] == [key(r) for r in want]
    for g, w in zip(got, want):
        assert set(w) <= set(g)
        for k in w:
            if k in ("score", "llr"):
                assert np.array_equal(fbits(g[k]), fbits(w[k])), (key(g), k)
            else:
                assert np.array_equal(g[k], w[k]), (key(g), k)
    second = [r for r in got if r["pass"] == 2]
    assert len(second) == 1 and np.array_equal(second[0]["bits77"], msgs[1]) and second[0]["text"] == gl.TEXTS[1]
    assert not any(r["pass"] == 1 and r["ok"] and np.array_equal(r["bits77"], msgs[1]) for r in got)
