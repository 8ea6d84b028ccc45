"""The channel bank on the GPU (pysdr_amd/csrc/bank.hip) against the oracle's demodulator, AGC and
squelch (tests/bank_oracle.py).  The oracle side is fed the rows of an independent Channelizer of the same shape on the
same input, so only the bank's own arithmetic is judged; that the bank's rows are those rows is asserted first."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import bank_oracle as bo
from tests.test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

IDS = [f"{M}-{D}" for M, D, _, _ in bo.SHAPES]


def fbits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cbits(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


@functools.lru_cache(maxsize=None)
def shared(i):
    """case i of bo.SHAPES with the rows of an independent channelizer, cut into calls; computed once, never changed"""
    from pysdr_amd.channelizer import Channelizer
    M, D, channels, T = bo.SHAPES[i]
    c = bo.case(M, D, channels)
    ch = Channelizer(c["fs"], M, D, channels=channels, max_in=len(c["x"]))
    y = ch.push(c["x"])
    ch.close()
    c["y"], c["calls"], c["yc"] = y, bo.split(c["x"], c["cuts"]), bo.cut_rows(y, c["cuts"], D)
    c["T"], c["channels"], c["fs_out"] = T, channels, c["fs"] / D
    counts = [r.shape[1] for r in c["yc"]]
    assert counts[:3] == [1, 3, 0] and len(counts) >= 6 and all(k % 2048 for k in counts[3:])
    if i == 0:                                                 # one call of two tiles of the kernel, the second partly filled
        assert max(counts) == bo.BIG and 2048 < bo.BIG < 4096
    for v in (c["x"], y):
        v.setflags(write=False)
    return c


def make_bank(c, mode, **kw):
    from pysdr_amd.bank import ChannelBank
    return ChannelBank(c["fs"], c["M"], c["D"], channels=c["channels"], mode=mode, af_bw=bo.AF_BW, ntaps_af=c["T"],
                       max_in=len(c["x"]), **kw)


@functools.lru_cache(maxsize=None)
def oracle_run(i, mode, squelch=0.0, agc=True, dtype=np.float32):
    """the helper's answers to every call of case i (a list of dicts), and the helper as it stands after them"""
    from pysdr_amd.bank import af_taps
    c = shared(i)
    o = bo.BankOracle(len(c["rows"]), c["fs_out"], af_taps(c["fs_out"], c["T"], bo.AF_BW), mode, squelch, agc, dtype)
    return [o.process(r) for r in c["yc"]], o


def rel(got, want):
    return np.abs(got - want) / np.maximum(np.abs(want), 1e-30)


@pytest.mark.parametrize("i", range(len(bo.SHAPES)), ids=IDS)
def test_parity_am(i):
    c = shared(i)
    want, _ = oracle_run(i, "AM")
    b = make_bank(c, "AM")
    assert np.array_equal(b.freqs, np.where(c["rows"] >= (c["M"] + 1) // 2, c["rows"] - c["M"], c["rows"]) * bo.SPACING)
    worst = 0.0
    for x, y, w in zip(c["calls"], c["yc"], want):
        am = b.push(x)
        assert am.shape == w["am"].shape and am.dtype == np.float32
        if y.shape[1] == 0:
            continue
        assert np.array_equal(cbits(b.iq()), cbits(y))                    # the bank's rows are the channelizer's
        e = np.max(np.abs(am - w["am"]), axis=1) / np.maximum(np.max(np.abs(w["am"]), axis=1), 1e-30)
        worst = max(worst, float(e.max()))
        assert e.max() <= TOL, (y.shape, int(e.argmax()), float(e.max()))
        st = b.state()
        for k, wk in (("agc", "agc"), ("gain", "agc_gain"), ("maxbuf", "maxbuf")):
            assert rel(st[k], w[wk]).max() <= 1e-5, (k, float(rel(st[k], w[wk]).max()))
        assert st["open"].all()
    print(f"AM M {c['M']} D {c['D']} T {c['T']}: worst |am - want| / peak of the channel's call {worst:.2e}")
    b.close()


def test_parity_am_255_taps_hard_start():
    """The shipped default of 255 AF taps (31 steps of eight and a tail of 7, one history sample per thread) at 640
    channels, the carriers at full amplitude from sample 0, 4000 frames: the stream has the call of more than one tile.
    AM has no ill-conditioned start-up, so the plain bar holds on every channel, call and sample."""
    from pysdr_amd.bank import ChannelBank, af_taps
    from pysdr_amd.channelizer import Channelizer
    M, D, T = 640, 320, 255
    c = bo.case(M, D, frames=4000, hard=True)
    ch = Channelizer(c["fs"], M, D, max_in=len(c["x"]))
    y = ch.push(c["x"])
    ch.close()
    yc = bo.cut_rows(y, c["cuts"], D)
    assert max(r.shape[1] for r in yc) == bo.BIG
    fs_out = c["fs"] / D
    o = bo.BankOracle(M, fs_out, af_taps(fs_out, T, bo.AF_BW), "AM")
    b = ChannelBank(c["fs"], M, D, mode="AM", af_bw=bo.AF_BW, ntaps_af=T, max_in=len(c["x"]))
    worst = 0.0
    for x, r in zip(bo.split(c["x"], c["cuts"]), yc):
        am, w = b.push(x), o.process(r)
        if r.shape[1] == 0:
            continue
        e = np.max(np.abs(am - w["am"]), axis=1) / np.maximum(np.max(np.abs(w["am"]), axis=1), 1e-30)
        worst = max(worst, float(e.max()))
        assert e.max() <= TOL, (r.shape, int(e.argmax()), float(e.max()))
        st = b.state()
        for k, wk in (("agc", "agc"), ("gain", "agc_gain"), ("maxbuf", "maxbuf")):
            assert rel(st[k], w[wk]).max() <= 1e-5, (k, float(rel(st[k], w[wk]).max()))
    print(f"AM M {M} D {D} T {T}, hard start: worst |am - want| / peak of the channel's call {worst:.2e}")
    b.close()


def nfm_compare(c, o, seen, pk, am, w, first):
    """run_both's rule (tests/test_gpu_parity.py) on every channel, plus the plain bar on the carrier channels from
    output 256 on; first = absolute index of the call's first output.  Returns the worst excess / full scale."""
    worst, n = 0.0, am.shape[1]
    for a in range(am.shape[0]):
        allow = o.allowance(a, seen[a])[-n:]
        ok = allow == 0
        pk[a] = max(pk[a], float(np.max(np.abs(w[a][ok]))) if ok.any() else 0.0)
        excess = np.maximum(np.abs(am[a] - w[a]) - allow, 0.0)
        e = float(np.max(excess) / (pk[a] if pk[a] > 0 else 1.0))
        assert e <= TOL, (a, "allowance", e)
        worst = max(worst, e)
        if a in c["carrier_rows"] and first + n > 256:
            s = max(256 - first, 0)
            assert not allow[s:].any()
            e = float(np.max(np.abs(am[a, s:] - w[a, s:])) / np.max(np.abs(w[a, s:])))
            assert e <= TOL, (a, "carrier", e)
            worst = max(worst, e)
    return worst


@pytest.mark.parametrize("i", range(len(bo.SHAPES)), ids=IDS)
def test_parity_nfm(i):
    c = shared(i)
    want, o = oracle_run(i, "NFM")
    b = make_bank(c, "NFM")
    nk = len(c["rows"])
    pk, first, worst = [0.0] * nk, 0, 0.0
    for x, y, w in zip(c["calls"], c["yc"], want):
        am = b.push(x)
        assert am.shape == w["am"].shape
        n = y.shape[1]
        if n == 0:
            continue
        assert np.array_equal(cbits(b.iq()), cbits(y))
        assert np.array_equal(b.state()["gain"], np.ones(nk, np.float32))          # NFM: gain 1, as in AGC_MODES
        worst = max(worst, nfm_compare(c, o, c["y"][:, :first + n], pk, am, w["am"], first))
        first += n
    print(f"NFM M {c['M']} D {c['D']} T {c['T']}: worst excess / full scale {worst:.2e}")
    b.close()


def test_squelch():
    """levels against the float32 helper within 4 x the helper's own float32 / float64 disagreement (a different but
    legitimate summation order), gates equal everywhere, closed channels silent, push_open = the open rows of push"""
    c = shared(0)
    w32, _ = oracle_run(0, "NFM", bo.SQUELCH)
    w64, _ = oracle_run(0, "NFM", bo.SQUELCH, True, np.float64)
    dis = max(float(rel(a["level"].astype(np.float64), b["level"]).max()) for a, b, y in zip(w32, w64, c["yc"]) if y.shape[1])
    bar = max(1e-5, 4 * dis)
    b, b2 = make_bank(c, "NFM", squelch=bo.SQUELCH), make_bank(c, "NFM", squelch=bo.SQUELCH)
    assert b.squelch == bo.SQUELCH
    worst, closed_seen, open_seen = 0.0, 0, 0
    for x, y, w in zip(c["calls"], c["yc"], w32):
        am = b.push(x)
        rows, am_open = b2.push_open(x)
        st = b.state()
        assert np.array_equal(st["open"], w["open"])
        assert np.array_equal(rows, np.flatnonzero(w["open"]))
        if y.shape[1] == 0:
            assert am_open.shape == (len(rows), 0)
            continue
        e = float(rel(st["level"].astype(np.float64), w["level"].astype(np.float64)).max())
        worst = max(worst, e)
        assert e <= bar, (e, bar)
        assert np.all(am[~w["open"]] == 0.0)
        assert np.array_equal(fbits(am_open), fbits(am[rows]))
        assert np.array_equal(fbits(b2.fetch(rows[:1])), fbits(am[rows[:1]]))
        closed_seen, open_seen = closed_seen + int((~w["open"]).sum()), open_seen + int(w["open"].sum())
    assert set(np.flatnonzero(b.open)) == set(c["carrier_rows"]) and closed_seen and open_seen
    assert np.array_equal(b.level, b.state()["level"]) and b.agc_state.shape == (len(c["rows"]),)
    print(f"squelch: float32 vs float64 helper {dis:.2e} -> bar {bar:.2e}; bank vs float32 helper {worst:.2e}")
    b.close()
    b2.close()


@pytest.mark.parametrize("i", [0, 3], ids=[IDS[0], IDS[3]])
@pytest.mark.parametrize("mode", ["AM", "NFM"])
def test_any_cut_gives_the_same_audio(i, mode):
    """One call of 2601 outputs -- two tiles of the kernel, the second partly filled -- against the same stream in pieces:
    lengths 0, 1, D - 1, D + 1; a piece that ends where the one call's first tile ends (output 2048), so that the next
    starts on that boundary with the halo in the history instead of in the previous tile; pieces of exactly one tile, of
    one tile and one output, and of two tiles cut inside the one call's tiles."""
    from pysdr_amd.bank import ChannelBank
    M, D, channels, T = bo.SHAPES[i]
    x = bo.case(M, D, channels, frames=2601)["x"][:D * 2600 + 3]
    b = ChannelBank(bo.SPACING * M, M, D, channels=channels, mode=mode, af_bw=bo.AF_BW, ntaps_af=T, max_in=len(x), agc=False)
    assert b.agc is False and b.squelch == 0.0
    one = b.push(x)
    assert one.shape == (b.nk, 2601) and np.isfinite(one).all() and np.abs(one).max() > 0
    heads = ([0, 1, D - 1, 0, D + 1, 7, 2048 * D - (2 * D + 8), 2 * D],         # ... | ends at output 2048 | two | the rest
             [2048 * D - D + 1, D + 1, 1, 1, 300 * D - 3, D - 1],               # exactly 2048 outputs: one full tile
             [D + 1, 2050 * D - 5, 3],                                          # 2 | 2049: one tile and one output | 0
             [200 * D + 9, 2300 * D])                                           # 201 | 2300: two tiles, offset from the one call's
    for head in heads:
        cuts = head + [len(x) - sum(head)]
        assert cuts[-1] > 0 and max(cuts) > 300 * D
        b.reset()
        parts = [b.push(p) for p in bo.split(x, cuts)]
        assert [p.shape[1] for p in parts] == [r.shape[1] for r in bo.cut_rows(one, cuts, D)]
        assert np.array_equal(fbits(np.concatenate(parts, axis=1)), fbits(one))
    b.close()


def test_a_call_without_outputs_changes_no_state():
    c = shared(0)
    D = c["D"]
    x = c["x"]
    a, t = make_bank(c, "AM"), make_bank(c, "AM")
    n1 = 40 * D + 5
    assert np.array_equal(fbits(a.push(x[:n1])), fbits(t.push(x[:n1])))
    before = a.state()
    empty = x[n1:n1 + D - 6]                                              # ends one sample short of the next frame
    assert a.n_out_for(len(empty)) == 0 and a.push(empty).shape == (len(c["rows"]), 0)
    assert a.iq().shape == (len(c["rows"]), 0) and a.fetch([0, 5]).shape == (2, 0)      # nothing to fetch after it
    after = a.state()
    for k in before:
        assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k
    nxt = x[n1 + len(empty):n1 + 90 * D]
    assert np.array_equal(fbits(a.push(nxt)), fbits(t.push(x[n1:n1 + 90 * D])))    # the twin never saw the empty call
    for k in before:
        assert np.array_equal(a.state()[k].view(np.uint8), t.state()[k].view(np.uint8)), k
    a.close()
    t.close()


def test_set_mode_between_calls():
    """AM -> NFM with another AF width: both hold for the whole AF window of the next call's outputs"""
    from pysdr_amd.bank import af_taps
    c = shared(0)
    D, T = c["D"], c["T"]
    n1, n2 = 600 * D, 400 * D
    b = make_bank(c, "AM")
    o = bo.BankOracle(len(c["rows"]), c["fs_out"], af_taps(c["fs_out"], T, bo.AF_BW), "AM")
    am1, w1 = b.push(c["x"][:n1]), o.process(c["y"][:, :600])
    assert (np.max(np.abs(am1 - w1["am"]), axis=1) <= TOL * np.max(np.abs(w1["am"]), axis=1)).all()
    b.set_mode("NFM", af_bw=2e3)
    o.set_mode("NFM", af_taps(c["fs_out"], T, 2e3))
    assert b.mode == "NFM" and b.af_bw == 2e3 and not np.array_equal(b.af, af_taps(c["fs_out"], T, bo.AF_BW))
    am2, w2 = b.push(c["x"][n1:n1 + n2]), o.process(c["y"][:, 600:1000])
    pk = [0.0] * len(c["rows"])
    nfm_compare(c, o, c["y"][:, :1000], pk, am2, w2["am"], 600)
    # not what the old taps, or a detector history of the old mode, would give in the first outputs
    old = bo.BankOracle(len(c["rows"]), c["fs_out"], af_taps(c["fs_out"], T, bo.AF_BW), "NFM")
    old.process(c["y"][:, :600])
    wo = old.process(c["y"][:, 600:1000])["am"]
    r = c["carrier_rows"][0]
    assert np.max(np.abs(am2[r, :8] - wo[r, :8])) > 100 * TOL * np.max(np.abs(w2["am"][r]))
    b.close()


@pytest.mark.parametrize("mode", ["AM", "NFM"])
def test_reset_repeats_the_first_run(mode):
    c = shared(0)
    b = make_bank(c, mode, squelch=bo.SQUELCH)
    calls = c["calls"][:6]
    first = [(b.push(x), b.state()) for x in calls]
    b.reset()
    assert b.n_out_for(7) == 1
    for x, (am, st) in zip(calls, first):
        assert np.array_equal(fbits(b.push(x)), fbits(am))
        s2 = b.state()
        for k in st:
            assert np.array_equal(st[k].view(np.uint8), s2[k].view(np.uint8)), k
    b.close()


@pytest.mark.parametrize("mode,agc", [("NFM", True), ("AM", False), ("AM", True)])
def test_one_nan_marks_what_the_definition_implies(mode, agc):
    """One NaN input sample: the helper, fed the rows of a channelizer on the same input, says which audio samples are
    not finite -- the AF windows of the detector outputs the bad frames reach.  The oracle's AGC is NaN-sticky: np.max
    hands the NaN to AGC.update, `peak > agc` is false ever after and the loop filter keeps the NaN, so agc and maxbuf
    stay NaN in every mode; the gain follows only where the AGC is active (AM, enabled) -- there the audio stays NaN --
    and is 1 otherwise, where every call after the window has passed is clean again, bit for bit."""
    from pysdr_amd.bank import af_taps
    from pysdr_amd.channelizer import Channelizer
    c = shared(0)
    D, T, nk = c["D"], c["T"], len(c["rows"])
    x = c["x"][:1500 * D].copy()
    where = 420 * D + 9
    x[where] = complex(np.nan, 0.25)
    cuts = [400 * D, 100 * D + 3, 300 * D - 3, 350 * D, 350 * D]
    ch = Channelizer(c["fs"], c["M"], D, max_in=len(x))
    yc = bo.cut_rows(ch.push(x), cuts, D)
    ch.close()
    o = bo.BankOracle(nk, c["fs_out"], af_taps(c["fs_out"], T, bo.AF_BW), mode, agc=agc)
    b = make_bank(c, mode, agc=agc)
    clean = make_bank(c, mode, agc=agc)
    for j, (p, pc, y) in enumerate(zip(bo.split(x, cuts), bo.split(c["x"][:len(x)], cuts), yc)):
        with np.errstate(invalid="ignore"):
            w = o.process(y)
        am, ref = b.push(p), clean.push(pc)
        bad = ~np.isfinite(w["am"])
        assert np.array_equal(~np.isfinite(am), bad), j
        st = b.state()
        for k, wk in (("agc", "agc"), ("gain", "agc_gain"), ("maxbuf", "maxbuf")):
            assert np.array_equal(np.isnan(st[k]), np.isnan(w[wk])), (j, k)
        if j == 0:
            assert not bad.any()
        elif j == 1:
            # frames 421 .. 436 hold the sample (8 M taps), so detector outputs 421 .. 436 (+ 2 in NFM) and T - 1 more
            n_bad = 16 + (2 if mode == "NFM" else 0) + T - 1
            first = 421 - 400
            if mode == "AM" and agc:
                assert bad.all()
            else:
                assert bad[:, first:first + min(n_bad, bad.shape[1] - first)].all() and not bad[:, :first].any()
                assert bad.sum(axis=1).max() == min(n_bad, bad.shape[1] - first)
        else:
            assert np.isnan(w["agc"]).all()                                # the helper's AGC state stays NaN ...
            if mode == "AM" and agc:
                assert bad.all()                                           # ... and with it the gain, where it is active
            elif j >= 3:
                assert not bad.any() and np.array_equal(fbits(am), fbits(ref))
    b.close()
    clean.close()


def test_errors_leave_the_object_usable():
    from pysdr_amd import _lib
    from pysdr_amd.bank import ChannelBank, af_taps
    from pysdr_amd.channelizer import Channelizer
    c = shared(0)
    D, nk = c["D"], len(c["rows"])
    x = np.array(c["x"][:200 * D])
    L = _lib.lib()
    n_out = C.c_int(-1)
    px = C.c_void_p(x.ctypes.data)
    am = np.zeros((nk, 200), np.float32)
    pa = C.c_void_p(am.ctypes.data)
    # a bank fresh from create has no mode
    ch = Channelizer(c["fs"], c["M"], D, max_in=len(x))
    h = C.c_void_p()
    assert L.pysdr_bank_create(ch._h, c["fs_out"], 5, 255, C.byref(h)) == -1 and not h.value          # CW
    assert L.pysdr_bank_create(ch._h, c["fs_out"], 9, 256, C.byref(h)) == -1 and not h.value
    assert L.pysdr_bank_create(ch._h, c["fs_out"], 9, 255, C.byref(h)) == 0 and h.value
    assert L.pysdr_bank_process(h, px, len(x), 0, pa, 200, 0, C.byref(n_out)) == -5 and n_out.value == 0
    assert b"no mode" in L.pysdr_last_error()
    L.pysdr_bank_destroy(h)
    ch.close()

    b = ChannelBank(c["fs"], c["M"], D, mode="NFM", af_bw=bo.AF_BW, ntaps_af=255, max_in=len(x))
    want = b.push(x)
    b.reset()
    af = af_taps(c["fs_out"], 255, bo.AF_BW)
    assert L.pysdr_bank_set_mode(b._h, 9, _lib.as_pd(af), 254) == -1                                  # wrong tap count
    assert L.pysdr_bank_set_mode(b._h, 3, _lib.as_pd(af), 255) == -1                                  # USB
    assert L.pysdr_bank_set_mode(b._h, 9, None, 255) == -1
    assert L.pysdr_bank_process(b._h, px, len(x), 0, pa, 199, 0, C.byref(n_out)) == -5                # am_pitch < 200 outputs
    assert b"pitch" in L.pysdr_last_error()
    assert L.pysdr_bank_process(b._h, px, len(x) + 1, 0, pa, 300, 0, C.byref(n_out)) == -5            # n > max_in
    assert L.pysdr_bank_process(b._h, px, -1, 0, pa, 200, 0, C.byref(n_out)) == -1
    assert L.pysdr_bank_process(b._h, None, 16, 0, pa, 200, 0, C.byref(n_out)) == -1
    assert L.pysdr_bank_process(b._h, px, len(x), 0, pa, 200, 0, None) == -1
    assert L.pysdr_bank_set_agc(b._h, 1, 0.0) == -1 and L.pysdr_bank_set_squelch(b._h, -1.0) == -1
    rows = np.array([0, nk], np.int32)
    assert L.pysdr_bank_fetch(b._h, _lib.as_pi(rows), 2, _lib.as_pf(am), None, 200) == -1
    assert n_out.value == 0
    with pytest.raises(_lib.PysdrError):
        b.set_mode("USB")
    with pytest.raises(_lib.PysdrError):
        ChannelBank(c["fs"], c["M"], D, mode="CW")
    with pytest.raises(_lib.PysdrError):
        ChannelBank(c["fs"], c["M"], D, ntaps_af=2)
    assert np.array_equal(fbits(b.push(x)), fbits(want))                  # nothing above advanced the stream or changed the mode
    b.close()
