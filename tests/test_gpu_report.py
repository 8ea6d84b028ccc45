"""The frame report and the row floor on the GPU (pysdr_amd/csrc/report.hip, report_host.h) against the
NumPy oracle of the definition (tests/report_oracle.py), which is fed the skimmer's own spectrum ring: every bit of power
and errs, and of every bin of a floor, is EQUAL -- on the 8000 Hz three-row FT8 shape with max_out = 64, whose 347-step
stream wraps its 331-step ring, at three moments of the stream; on the 12000 Hz shape (S = 96); on all 80 rows, where the
raster is a circle; on the FT4 shapes at S = 48 and 72; over 4097 candidates in two calls of the C ABI.  Every refusal of
both calls leaves the outputs untouched.  Then the skimmer with ``report=True``: the stations' SNR and fine frequency
within the bounds the CPU measurement set (tests/test_report_oracle.py), and with ``report=False`` the records of today."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import report_oracle as ro
from tests import test_gpu_ft4 as g4
from tests import test_gpu_ft8 as g8
from tests import test_gpu_ldpc as gl
from tests import test_report_oracle as tro
from tests.test_gpu_psk import fbits

pytestmark = pytest.mark.gpu

F32 = np.float32
pi32, pu8, pll = C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_longlong)


@functools.lru_cache(maxsize=None)
def stations():
    """(F, t0) of tests/test_gpu_ldpc.py's three stations, in the order of their messages: one decoding run, once"""
    sk = gl.skimmer(decode=True)
    recs = sk.push(gl.coded_input())
    sk.close()
    assert len(recs) == 3 and all(r["ok"] for r in recs)
    out = []
    for msg in gl.messages():
        r, = [r for r in recs if np.array_equal(r["bits77"], msg)]
        out.append((r["F"], r["t0"]))
    return tuple(out)


def words(rng, n):
    from pysdr_amd import ldpc
    return np.array([ldpc.encode(rng.integers(0, 2, 77))[:91] for _ in range(n)]).reshape(n, 91)


def same(sk, mode, F, t0, bits, where, ring=None):
    """the bank's answer against the oracle on the bank's own ring -> the answer"""
    ring = sk.dec.state(ring=True)["ring"] if ring is None else ring
    power, errs = ro.report(ring, sk.dec.t_done, sk.nsub, sk.circular, mode, F, t0, bits)
    got = sk.dec.report(F, t0, bits)
    assert got["sig9"].dtype == F32 and got["sig9"].shape == (len(F), 3, 3)
    bad = np.argwhere(fbits(got["sig9"].reshape(-1, 9)) != fbits(power[:, :9]))
    assert not len(bad), (where, bad[:5], got["sig9"].reshape(-1, 9)[bad[0][0]], power[bad[0][0]])
    assert np.array_equal(fbits(got["tot"]), fbits(power[:, 9])), where
    assert np.array_equal(got["nhard"], errs[:, 0]) and np.array_equal(got["nsync"], errs[:, 1]), where
    return got


def same_floor(sk, spans, where):
    ring = sk.dec.state(ring=True)["ring"]
    for t_end, nsym in spans:
        want = ro.floor(ring, sk.dec.t_done, t_end, nsym)
        assert want is not None, (where, t_end, nsym)
        got = sk.dec.floor(t_end, nsym)
        assert got.shape == want.shape and np.array_equal(fbits(got), fbits(want)), (where, t_end, nsym)


def push_to(sk, x, done):
    """the stream up to the sample that completes step done - 1 -> the records released on the way"""
    n = (sk.S + (done - 1) * sk.qs) * sk.D
    recs = sk.push(x[sk.chan.n_in:n])
    assert sk.dec.t_done == done
    return recs


def edge_candidates(sk, rng, lag, n_random):
    """random (F, t0), the raster's ends, a row's last decoder and the next row's first, the ring's ends"""
    done, tr = sk.dec.t_done, sk.dec.tr
    t_lo, t_hi = max(0, done - tr), done - lag - 1
    F = list(rng.integers(0, sk.nfine, n_random)) + [0, sk.nfine - 1, sk.nsub - 1, sk.nsub, 0, sk.nfine - 1, 3, 3]
    t0 = list(rng.integers(t_lo, t_hi + 1, n_random)) + [t_lo + 2, t_lo + 2, t_hi, t_lo, t_lo, t_hi, t_hi, t_lo]
    return np.array(F, np.int32), np.array(t0, np.int64)


def test_the_8000_hz_shape_at_three_moments_of_a_stream_that_wraps_its_ring():
    from pysdr_amd import ldpc
    x = gl.coded_input()
    sk = gl.skimmer(decode=True, max_out=64)
    rng = np.random.default_rng(26)
    own = np.array([ldpc.encode(m)[:91] for m in gl.messages()])
    assert sk.dec.tr == 331 and sk.nfine == 96 and not sk.circular
    STATIONS = stations()
    assert sorted(s[1] for s in STATIONS) == [5, 13, 23]             # whole and in the ring together only with 336 steps done
    # 320 steps in: nothing has left the ring, step 0 is a frame's first; t0 = done - 313 is the newest
    recs = push_to(sk, x, 320)
    F, t0 = edge_candidates(sk, rng, 312, 20)
    assert t0[-1] == 0 and t0[-2] == 320 - 313
    got = same(sk, ro.FT8, F, t0, words(rng, len(F)), "320")
    assert (got["sig9"][-1, 0] == -1).all() and (got["sig9"][-1, 1:] > 0).all() and (got["sig9"][-2, 2] == -1).all()
    same_floor(sk, ((319, 1), (319, 79), (0, 1), (312, 79), (319, 80)), "320")
    # 336 steps in: the ring has wrapped, and the three stations' frames are all whole and all still in it
    recs += push_to(sk, x, 336)
    F, t0 = edge_candidates(sk, rng, 312, 30)
    assert t0[-1] == 336 - 331 == 5 and t0[-2] == 336 - 313 == 23
    sF, st0 = np.array([s[0] for s in STATIONS], np.int32), np.array([s[1] for s in STATIONS], np.int64)
    F, t0 = np.concatenate((sF, sF, F)), np.concatenate((st0, st0, t0))
    bits = np.concatenate((own, own[[1, 2, 0]], words(rng, len(F) - 6)))
    got = same(sk, ro.FT8, F, t0, bits, "336")
    print("the stations with their own words: nhard", got["nhard"][:3], "nsync", got["nsync"][:3], "with another's:", got["nhard"][3:6], got["nsync"][3:6])
    assert (got["nhard"][:3] <= 4).all() and (got["nhard"][3:6] >= 30).all() and (got["nsync"][:6] <= 3).all()
    assert (got["sig9"][:3, 1, 1] > 3 * got["sig9"][3:6, 1, 1] / 2).all()
    miss = got["sig9"].reshape(-1, 9) == -1
    assert miss[:, [0, 3, 6]].all(axis=1).sum() >= 2 and miss[:, [2, 5, 8]].all(axis=1).sum() >= 2     # F = 0 and F = nfine - 1
    assert miss[:, :3].all(axis=1).sum() >= 3 and miss[:, 6:].all(axis=1).sum() >= 3 and not miss[:, 4].any()
    same_floor(sk, ((335, 1), (5, 1), (335, 79), (5 + 312, 79), (335, 83)), "336")
    # the whole stream: 347 steps
    recs += sk.push(x[sk.chan.n_in:])
    assert sk.dec.t_done == 347 and sorted((r["F"], r["t0"]) for r in recs) == sorted(STATIONS) and all(r["ok"] for r in recs)
    F, t0 = edge_candidates(sk, rng, 312, 30)
    assert t0[-1] == 16 and t0[-2] == 34
    same(sk, ro.FT8, F, t0, words(rng, len(F)), "347")
    same_floor(sk, ((346, 1), (16, 1), (346, 79), (16 + 312, 79), (346, 83)), "347")
    assert np.array_equal(fbits(sk.dec.floor()), fbits(sk.dec.floor(346, 79)))
    # 4097 candidates: two calls of the C ABI, the last of one candidate
    F = rng.integers(0, sk.nfine, 4097).astype(np.int32)
    t0 = rng.integers(16, 35, 4097).astype(np.int64)
    F[-1], t0[-1] = [s for s in STATIONS if s[1] == 23][0]
    got = same(sk, ro.FT8, F, t0, np.concatenate((words(rng, 4096), own[[s[1] for s in STATIONS].index(23)][None])), "4097")
    assert got["nhard"][-1] <= 4 and got["nhard"][:-1].min() > 20
    sk.close()


def test_every_refusal_of_both_calls_leaves_the_outputs_untouched():
    from pysdr_amd import _lib
    sk = gl.skimmer(decode=True, max_out=64)
    sk.push(gl.coded_input())
    L, h, done, nf = _lib.lib(), sk.dec._h, sk.dec.t_done, sk.nfine
    assert (done, sk.dec.tr) == (347, 331)
    power, errs, bits = np.full((2, 10), 7.0, F32), np.full((2, 2), 7, np.int32), np.zeros((2, 12), np.uint8)

    def call(F, t0, n=None, b=True, p=True, e=True):
        F, t0 = np.array(F, np.int32), np.array(t0, np.int64)
        rc = L.pysdr_ft8_report(h, F.ctypes.data_as(pi32), t0.ctypes.data_as(pll), bits.ctypes.data_as(pu8) if b else None, len(F) if n is None else n,
                                _lib.as_pf(power) if p else None, errs.ctypes.data_as(pi32) if e else None)
        if rc != 0:
            assert (power == 7.0).all() and (errs == 7).all()
        return rc

    assert call([3, 3], [20, done - 312]) == -5 and b"pysdr_ft8_report" in L.pysdr_last_error()   # the second frame's last step is not in
    assert call([3], [15]) == -5 and call([3], [-1]) == -5                       # gone from the ring; before the stream
    assert call([-1], [20]) == -1 and call([3, nf], [20, 20]) == -1
    assert call([3], [20], n=-1) == -1 and call([3], [20], n=4097) == -1
    assert call([3], [20], b=False) == -1 and call([3], [20], p=False) == -1 and call([3], [20], e=False) == -1
    assert L.pysdr_ft8_report(None, None, None, None, 0, None, None) == -1
    with pytest.raises(_lib.PysdrError):
        sk.dec.report([3], [done - 312], np.zeros((1, 91)))
    assert call([], [], n=0) == 0 and (power == 7.0).all() and (errs == 7).all()
    assert call([3, nf - 1], [16, done - 313]) == 0 and (power[:, 4] > 0).all() and (errs != 7).all()
    out = np.full((sk.nk, sk.dec.nb), 7.0, F32)

    def floor(t_end, nsym, o=True):
        rc = L.pysdr_ft8_floor(h, C.c_longlong(t_end), nsym, _lib.as_pf(out) if o else None)
        if rc != 0:
            assert (out == 7.0).all()
        return rc

    assert floor(346, 0) == -1 and floor(346, 129) == -1 and floor(346, -3) == -1 and b"pysdr_ft8_floor" in L.pysdr_last_error()
    assert floor(346, 79, o=False) == -1 and L.pysdr_ft8_floor(None, C.c_longlong(346), 79, _lib.as_pf(out)) == -1
    assert floor(347, 1) == -5 and floor(346, 84) == -5 and floor(15, 1) == -5 and floor(15 + 312, 79) == -5 and floor(-1, 1) == -5
    with pytest.raises(_lib.PysdrError):
        sk.dec.floor(347, 1)
    assert floor(346, 83) == 0 and (out > 0).all()
    sk.close()


@pytest.mark.parametrize("i", (1, 2), ids=g8.IDS[1:])
def test_the_12000_hz_shape_and_the_circular_raster_of_all_rows(i):
    from pysdr_amd.ft8 import FT8_Skimmer
    fs, channels, _ = g8.SHAPES[i]
    x = g8.make_input(i)
    sk = FT8_Skimmer(fs, channels=channels, max_in=len(x))
    sk.push(x)
    rng = np.random.default_rng(30 + i)
    assert sk.S == (96, 64)[i - 1] and sk.circular == (i == 2) and sk.dec.t_done == 347 and sk.dec.tr == (343, 355)[i - 1]
    F, t0 = edge_candidates(sk, rng, 312, 40)
    ring = sk.dec.state(ring=True)["ring"]
    got = same(sk, ro.FT8, F, t0, words(rng, len(F)), g8.IDS[i], ring)
    ends = got["sig9"][np.isin(F, (0, sk.nfine - 1))].reshape(-1, 9)
    if sk.circular:                                                             # F = 0 against nfine - 1: no fine row is missing
        assert not (ends[:, [3, 5]] == -1).any()
        a = sk.dec.report([0, sk.nfine - 1], [20, 20], words(np.random.default_rng(1), 1).repeat(2, axis=0))["sig9"]
        assert fbits(a[0, 1, 0]) == fbits(a[1, 1, 1]) and fbits(a[1, 1, 2]) == fbits(a[0, 1, 1])
    else:
        assert (ends[:, 3] == -1).sum() >= 2 and (ends[:, 5] == -1).sum() >= 2
    same_floor(sk, ((346, 79), (max(0, sk.dec.t_done - sk.dec.tr) + 312, 79), (346, 1)), g8.IDS[i])
    sk.close()


@pytest.mark.parametrize("i", (0, 1), ids=g4.IDS[:2])
def test_the_ft4_shapes(i):
    """S = 48 with a ring deep enough for a floor of 128 symbols across its wrap, and S = 72"""
    from pysdr_amd.ft4 import FT4_Skimmer
    fs, channels, _ = g4.SHAPES[i]
    x = g4.make_input(i)
    sk = FT4_Skimmer(fs, channels=channels, max_in=len(x), max_out=544 if i == 0 else 256)
    sk.push(x)
    done, tr = sk.dec.t_done, sk.dec.tr
    assert sk.S == (48, 72)[i] and done > tr and (i == 1 or tr == 509)
    rng = np.random.default_rng(40 + i)
    F, t0 = edge_candidates(sk, rng, 408, 40)
    got = same(sk, ro.FT4, F, t0, words(rng, len(F)), g4.IDS[i])
    assert (got["sig9"][:, 1, 1] > 0).all() and (got["nhard"] > 30).all()
    spans = [(done - 1, 103), (done - tr + 408, 103), (done - 1, 1), (done - tr, 1)]
    if i == 0:
        spans.append((done - 1, 128))                                           # 508 steps back: the oldest step of the ring
    same_floor(sk, spans, g4.IDS[i])
    assert np.array_equal(fbits(sk.dec.floor()), fbits(sk.dec.floor(done - 1, 103)))
    sk.close()


def test_the_skimmer_reports_snr_and_fine_frequency_and_without_report_the_records_of_today():
    from pysdr_amd import ft8
    fs, channels, sent = g8.SHAPES[0]
    x = gl.coded_input()
    B, Bf, _ = tro.BOUNDS[ro.FT8]
    sk = gl.skimmer(decode=True, report=True, max_out=64, t_first=1700000000.0 + 14.5)
    recs = sk.push(x)
    sk.close()
    plain = gl.skimmer(decode=True, max_out=64, t_first=1700000000.0 + 14.5)
    old = plain.push(x)
    plain.close()
    assert len(recs) == len(old) == 3
    new = ["dt_fine", "f_fine", "nhard", "noise", "nsync", "sig", "snr", "t_fine"]
    for a, c in zip(old, recs):
        assert sorted(a) == ["F", "bits77", "dt", "freq", "hits", "i3", "iterations", "llr", "n3", "nerr", "ok", "score", "slot", "status", "t0", "text", "time"]
        assert sorted(set(c) - set(a)) == new and set(a) <= set(c)
        for k in a:
            assert np.array_equal(a[k], c[k]), k
    for (f, snr, start), text in zip(sent, gl.TEXTS):
        r, = [r for r in recs if r["text"] == text]
        print(f"station {f} Hz {snr} dB at {start} s: snr {r['snr']:+.2f} f_fine {r['f_fine']:.2f} t_fine {r['t_fine']:.4f} dt_fine {r['dt_fine']:+.3f} "
              f"nhard {r['nhard']} nsync {r['nsync']} sig {r['sig']:.4g} noise {r['noise']:.4g}  |  {ft8.spot_line(r, 1500.0)}")
        assert abs(r["snr"] - snr) <= B, (f, r["snr"], snr, B)
        assert abs(r["f_fine"] - f) <= Bf, (f, r["f_fine"], Bf)
        assert abs(r["t_fine"] - r["time"]) <= 0.5 * sk.qs / sk.fs_out and abs(r["dt_fine"] - r["dt"]) <= 0.5 * sk.qs / sk.fs_out
        assert r["nhard"] <= 4 and r["nsync"] <= 3 and r["sig"] > r["noise"] > 0
    assert [id(r) for r in ft8.spots(recs)] == [id(r) for r in recs]
    twice = recs + [dict(r, F=r["F"] + 1, t0=r["t0"] + 1, sig=0.5 * r["sig"]) for r in recs]
    assert [id(r) for r in ft8.spots(twice)] == [id(r) for r in recs]          # one message seen on two fine rows is one spot
    with pytest.raises(ValueError):
        gl.skimmer(report=True)
    # a record that did not decode carries the keys as None: the stream of tests/test_gpu_ft8.py, whose frames are no codewords
    sk = gl.skimmer(decode=True, report=True)
    recs = sk.push(g8.make_input(0))
    sk.close()
    assert len(recs) == 3 and not any(r["ok"] for r in recs)
    assert all(r[k] is None for r in recs for k in new if k != "dt_fine") and not any("dt_fine" in r for r in recs)


def test_the_ft4_skimmer_reports_likewise():
    """tests/test_gpu_ldpc.py's FT4 stream: codewords on the air at -5, 3 and -8 dB"""
    from pysdr_amd import ft4, ldpc
    from pysdr_amd.ft4 import FT4_Skimmer
    from tests import ft4_oracle as f4o
    fs, channels, stations = g4.SHAPES[0]
    n = int(g4.SECONDS * fs)
    rng = np.random.default_rng(500)
    x = f4o.noise_sigma(0.0, f4o.SNR_BW, fs) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for j, ((f, snr, start), msg) in enumerate(zip(stations, gl.messages())):
        s = f4o.waveform(f4o.tones(ldpc.encode(msg)), f, fs, gfsk=j != 1, phase=1.0 + j) * 10 ** (snr / 20)
        at = int(start * fs)
        x[at:at + len(s)] += s[:n - at]
    x = (0.05 * x).astype(np.complex64)
    sk = FT4_Skimmer(fs, channels=channels, max_in=len(x), decode=True, report=True)
    recs = sk.push(x)
    sk.close()
    assert len(recs) == 3 and all(r["ok"] for r in recs)
    for (f, snr, start), msg in zip(stations, gl.messages()):
        r, = [r for r in recs if np.array_equal(r["bits77"], msg)]
        print(f"FT4 station {f:.1f} Hz {snr} dB: snr {r['snr']:+.2f} f_fine {r['f_fine']:.2f} t_fine {r['t_fine']:.4f} nhard {r['nhard']} nsync {r['nsync']}")
        assert abs(r["f_fine"] - f) <= ft4.BAUD / 4 and abs(r["t_fine"] - r["time"]) <= 0.5 * sk.qs / sk.fs_out
        assert r["nhard"] <= 6 and r["nsync"] <= 1 and r["sig"] > r["noise"] > 0 and np.isfinite(r["snr"])
    assert [id(r) for r in ft4.spots(recs)] == [id(r) for r in recs]
