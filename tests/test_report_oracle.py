"""The frame report's definition on the CPU: the oracle (tests/report_oracle.py) on planted rings --
every case of a missing place, the crossing from one row to the next, the wrap of a circular raster, a clean frame and a
wrong word of the same frame, the row floor and its refusals -- the host half's arithmetic (``ft8.delta``, ``refine``,
``noise_of``, ``snr_db``, ``spots``, ``spot_line``), and the ACCURACY MEASUREMENT: stations of known SNR, frequency and start
behind the float64 definition of the channelizer (tests/channelizer_oracle.py) on a raster of 13 rows, measured by the
oracle and the host half, against the generator's own numbers.  No GPU: the kernels are held against this oracle bit for
bit in tests/test_gpu_report.py."""
import functools

import numpy as np
import pytest

from tests import channelizer_oracle as cz
from tests import ft4_oracle as f4o
from tests import ft8_oracle as f8o
from tests import report_oracle as ro

F32 = np.float32


def fbits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def word(rng):
    """91 bits: a message and its CRC"""
    from pysdr_amd import ldpc
    return ldpc.encode(rng.integers(0, 2, 77))[:91]


# ---- the definition on planted rings ---------------------------------------------------------------------------------------

def planted(mode, nk, nsub, tr, t_done, seed):
    """a ring of random powers, every value different, as the state call delivers it"""
    rng = np.random.default_rng(seed)
    nb = nsub + (14 if mode == ro.FT8 else 6)
    ring = rng.uniform(0.5, 2.0, (nk, tr, nb)).astype(F32)
    ring.setflags(write=False)
    return ring


def plain(ring, t_done, nsub, circular, mode, F, t0, bits91):
    """the definition once more, one candidate, plain loops in float32"""
    nk, tr, nb = ring.shape
    nfine = nk * nsub
    tone = ro.frame_tones(mode, bits91)
    out = []
    for dt, dF in ro.PLACES:
        Fn = F + dF
        if circular:
            Fn %= nfine
        t = t0 + dt
        if not (0 <= Fn < nfine) or t < 0 or t + ro.lag(mode) >= t_done or t_done - t > tr:
            out.append(F32(-1.0))
            continue
        a, j = divmod(Fn, nsub)
        acc = None
        for k in range(len(tone)):
            p = ring[a, (t + 4 * k) % tr, j + 2 * tone[k]]
            acc = p if acc is None else F32(acc + p)
        out.append(acc)
    return out


@pytest.mark.parametrize("mode", (ro.FT8, ro.FT4), ids=["ft8", "ft4"])
def test_every_missing_place_row_crossing_and_circular_wrap(mode):
    rng = np.random.default_rng(3 + mode)
    nk, nsub, lag = 3, 8, ro.lag(mode)
    tr, t_done = lag + 30, lag + 50                                  # the ring has wrapped: steps 20 .. lag + 49 are in it
    ring = planted(mode, nk, nsub, tr, t_done, 10 + mode)
    nfine = nk * nsub
    t_lo, t_hi = t_done - tr, t_done - lag - 1                       # the oldest and the newest frame start a call takes
    cases = [(5, t_lo + 3), (0, t_lo + 3), (nfine - 1, t_lo + 3), (nsub - 1, t_lo + 5), (nsub, t_lo + 5), (2 * nsub - 1, t_hi), (7, t_lo),
             (0, t_lo), (nfine - 1, t_hi), (nsub, t_hi - 1), (nsub, t_lo + 1)]
    for circular in (False, True):
        F = np.array([c[0] for c in cases])
        t0 = np.array([c[1] for c in cases])
        bits = np.array([word(rng) for _ in cases])
        power, errs = ro.report(ring, t_done, nsub, circular, mode, F, t0, bits)
        for i, (f, t) in enumerate(cases):
            want = plain(ring, t_done, nsub, circular, mode, f, t, bits[i])
            assert np.array_equal(fbits(power[i, :9]), fbits(want)), (circular, f, t)
            miss = power[i, :9].reshape(3, 3) == -1
            assert not miss[1, 1]
            assert miss[0].all() == (t == t_lo) and miss[2].all() == (t == t_hi), (f, t, miss)      # a step too early, a step too late
            assert miss[:, 0].all() == (f == 0 and not circular) and miss[:, 2].all() == (f == nfine - 1 and not circular)
            assert (power[i][power[i] != -1] > 0).all()
        # the neighbour of a row's last decoder is decoder 0 of the next row; of the raster's last, fine row 0 on a circle
        k = cases.index((nsub - 1, t_lo + 5))
        again, _ = ro.report(ring, t_done, nsub, circular, mode, [nsub], [t_lo + 5], [bits[k]])
        assert fbits(power[k, 5]) == fbits(again[0, 4])
        if circular:
            k = cases.index((nfine - 1, t_lo + 3))
            again, _ = ro.report(ring, t_done, nsub, circular, mode, [0], [t_lo + 3], [bits[k]])
            assert fbits(power[k, 5]) == fbits(again[0, 4]) and fbits(power[k, 4]) == fbits(again[0, 3])
    # a ring that has not wrapped and a stream too short for step t0 - 1: t0 = 0
    young = planted(mode, nk, nsub, tr, lag + 2, 20 + mode)
    power, _ = ro.report(young, lag + 2, nsub, False, mode, [4], [0], [word(rng)])
    got = power[0, :9].reshape(3, 3)
    assert (got[0] == -1).all() and (got[1] > 0).all() and (got[2] > 0).all()
    power, _ = ro.report(young, lag + 2, nsub, False, mode, [4], [1], [word(rng)])
    assert (power[0, :3] > 0).all() and (power[0, 6:9] == -1).all()
    with pytest.raises(AssertionError):
        ro.report(young, lag + 2, nsub, False, mode, [4], [2], [word(rng)])     # not whole: pysdr_*_llr's refusal
    assert len(ro.report(young, lag + 2, nsub, False, mode, [], [], np.zeros((0, 91)))[0]) == 0


@pytest.mark.parametrize("mode", (ro.FT8, ro.FT4), ids=["ft8", "ft4"])
def test_a_clean_frame_has_no_lost_symbol_and_a_wrong_word_many(mode):
    rng = np.random.default_rng(30 + mode)
    nk, nsub, lag, T = 2, 8, ro.lag(mode), ro.NTONES[mode]
    tr = t_done = lag + 12
    ring = np.array(planted(mode, nk, nsub, tr, t_done, 40 + mode)) * F32(0.01)
    sent, other = word(rng), word(rng)
    F, t0 = nsub + 3, 5
    tone = ro.frame_tones(mode, sent)
    for k, c in enumerate(tone):
        ring[1, t0 + 4 * k, 3 + 2 * c] = F32(7.0) + F32(k) * F32(0.125)
    power, errs = ro.report(ring, t_done, nsub, False, mode, [F, F], [t0, t0], [sent, other])
    assert list(errs[0]) == [0, 0] and errs[1, 1] == 0               # the Costas symbols do not depend on the word
    differ = int((ro.frame_tones(mode, other) != tone).sum())
    assert errs[1, 0] == differ > 20, (errs, differ)
    want = F32(0)
    for k in range(len(tone)):
        want = F32(want + (F32(7.0) + F32(k) * F32(0.125))) if k else F32(7.0)
    assert fbits(power[0, 4]) == fbits(want) and power[0, 4] > 2 * power[1, 4]
    assert power[0, 9] == power[1, 9] and power[0, 9] > power[0, 4]   # tot does not depend on the word
    # a tie is a loss: the sent tone must be strictly greater
    ring[1, t0 + 4 * 10, 3 + 2 * ((tone[10] + 1) % T)] = ring[1, t0 + 4 * 10, 3 + 2 * tone[10]]
    _, errs = ro.report(ring, t_done, nsub, False, mode, [F], [t0], [sent])
    sync10 = 10 in ro.SYNC[mode]
    assert list(errs[0]) == ([0, 1] if sync10 else [1, 0])
    # the frame's tones: the Costas arrays in their places, the data symbols' bits MSB first through the Gray map
    from pysdr_amd import ft4, ft8, ldpc
    assert list(tone) == list((ft8 if mode == ro.FT8 else ft4).tones(ldpc.encode91(sent))) and len(tone) == ro.SYMS[mode]


def test_the_row_floor_and_its_refusals():
    ring = planted(ro.FT8, 3, 8, 340, 0, 50)
    t_done = 400                                                     # steps 60 .. 399 are in the ring
    for t_end, nsym in ((399, 1), (399, 79), (399, 85), (60, 1), (60 + 4 * 78, 79), (300, 20)):
        got = ro.floor(ring, t_done, t_end, nsym)
        want = np.zeros(ring.shape[::2], F32)
        for a in range(3):
            for b in range(ring.shape[2]):
                acc = None
                for i in range(nsym):
                    p = ring[a, (t_end - 4 * (nsym - 1 - i)) % 340, b]
                    acc = p if acc is None else F32(acc + p)
                want[a, b] = acc
        assert np.array_equal(fbits(got), fbits(want)), (t_end, nsym)
    for t_end, nsym in ((400, 1), (399, 0), (399, 129), (399, 86), (59, 1), (59 + 4 * 78, 79), (-1, 1)):
        assert ro.floor(ring, t_done, t_end, nsym) is None, (t_end, nsym)
    assert ro.floor(ring, 100, 99, 26) is None and ro.floor(ring, 100, 99, 25) is not None   # before step 0


# ---- the host half ------------------------------------------------------------------------------------------------------------

def test_delta_refine_and_snr():
    from pysdr_amd import ft8
    assert ft8.delta(-1.0, 5.0, 3.0) == 0.0 and ft8.delta(3.0, 5.0, -1.0) == 0.0          # a missing neighbour
    assert ft8.delta(3.0, 5.0, 3.0) == 0.0 and abs(ft8.delta(3.0, 5.0, 4.0) - 0.5 * (3 - 4) / (3 - 10 + 4)) < 1e-15
    assert ft8.delta(1.0, 5.0, 4.9) > 0 and ft8.delta(4.9, 5.0, 1.0) < 0
    assert ft8.delta(0.0, 5.0, 9.9) == 0.5 and ft8.delta(9.9, 5.0, 0.0) == -0.5              # concave, clipped: b is not the maximum
    assert ft8.delta(1.0, 2.0, 3.0) == 0.5 and ft8.delta(3.0, 2.0, 1.0) == -0.5              # a line: towards the greater
    assert ft8.delta(5.0, 2.0, 9.0) == 0.5 and ft8.delta(9.0, 2.0, 5.0) == -0.5 and ft8.delta(4.0, 2.0, 4.0) == 0.0   # convex
    # a parabola sampled at three points comes back exactly
    for x0, h in ((0.2, 7.0), (-0.45, 30.0), (0.0, 5.0)):
        y = [h - 2.0 * (x - x0) ** 2 for x in (-1, 0, 1)]
        s = np.full((3, 3), -1.0)
        s[1] = y
        df, dt, peak = ft8.refine(s)
        assert abs(df - x0) < 1e-12 and dt == 0.0 and abs(peak - h) < 1e-12
        df, dt, peak = ft8.refine(s.T)
        assert df == 0.0 and abs(dt - x0) < 1e-12 and peak == y[1]
    # snr: the signal's mean power over a bin's noise, moved to 2500 Hz
    assert abs(ft8.snr_db(79 * 101.0, 1.0, 79, 6.25, 0.0) - (20.0 - 10 * np.log10(400.0))) < 1e-12
    assert abs(ft8.snr_db(79 * 0.5, 1.0, 79, 6.25, 0.0) - (-30.0 - 10 * np.log10(400.0))) < 1e-12   # no signal left: the floor of -30 dB
    assert ft8.snr_db(79 * 3.0, 1.0, 79, 6.25, 1.0) - ft8.snr_db(79 * 3.0, 1.0, 79, 6.25, 0.0) == pytest.approx(1.0)


def test_the_noise_of_a_candidate():
    from pysdr_amd import ft8
    nsym, nb, nsub = 79, 46, 32
    rng = np.random.default_rng(8)
    floor = np.zeros((20, nb))
    for a in range(20):
        floor[a] = nsym * (a + 1) * rng.permutation(np.linspace(0.8, 1.2, nb))
    fl = ft8.noise_floor(floor, nsym)
    assert np.allclose(fl, np.arange(1, 21) * np.quantile(np.linspace(0.8, 1.2, nb), ft8.FLOOR_QUANTILE))
    assert ft8.noise_of(floor, nsym, 10 * nsub + 3, nsub, False) == pytest.approx(np.median(fl[[2, 3, 4, 5, 6, 14, 15, 16, 17, 18]]))
    assert ft8.noise_of(floor, nsym, 1 * nsub, nsub, False) == pytest.approx(np.median(fl[[5, 6, 7, 8, 9]]))
    assert ft8.noise_of(floor, nsym, 1 * nsub, nsub, True) == pytest.approx(np.median(fl[[5, 6, 7, 8, 9, 13, 14, 15, 16, 17]]))
    assert ft8.noise_of(floor[:3], nsym, 1 * nsub + 5, nsub, False) == pytest.approx(np.median(fl[[0, 2]]))      # none 4 away: all others
    one = floor[:1]
    b = np.arange(nb)
    assert ft8.noise_of(one, nsym, 10, nsub, False) == pytest.approx(np.quantile(one[0, (b < 8) | (b > 28)] / nsym, ft8.FLOOR_QUANTILE))


def test_spots_and_the_line():
    from pysdr_amd import ft4, ft8, ft8msg
    a, b = ft8msg.pack77("CQ K1ABC FN42"), ft8msg.pack77("K1ABC W9XYZ -12")
    recs = [dict(ok=True, bits77=a, t0=20, F=40, sig=5.0), dict(ok=True, bits77=a, t0=21, F=41, sig=7.0), dict(ok=True, bits77=a, t0=28, F=90, sig=6.0),
            dict(ok=True, bits77=a, t0=30, F=40, sig=7.0), dict(ok=True, bits77=b, t0=20, F=41, sig=1.0), dict(ok=False, bits77=a, t0=20, F=42, sig=None),
            dict(ok=True, bits77=a, t0=400, F=40, sig=0.5)]
    kept = ft8.spots(recs)
    # 21 beats 20 and 28; 30 ties with 21 nine steps away and loses to nobody within reach but 28, which it beats
    assert [(r["t0"], r["F"]) for r in kept] == [(21, 41), (30, 40), (20, 41), (400, 40)]
    assert [(r["t0"], r["F"]) for r in ft8.spots(recs, reach=9)] == [(21, 41), (20, 41), (400, 40)]      # the tie goes to the lower (t0, F)
    assert [(r["t0"], r["F"]) for r in ft8.spots(recs, reach=0)] == [(20, 40), (21, 41), (28, 90), (30, 40), (20, 41), (400, 40)]
    assert ft8.spots([]) == [] and ft4.spots is ft8.spots
    rec = dict(ok=True, text="CQ K1ABC FN42", snr=-12.4, f_fine=1234.6, t_fine=1.31, dt_fine=0.26, slot=4 * 3600 // 15 + 5 * 4 + 2)
    assert ft8.spot_line(rec) == "040530 -12  0.3 1235 ~  CQ K1ABC FN42"
    assert ft8.spot_line(rec, f_centre=-1000.0) == "040530 -12  0.3  235 ~  CQ K1ABC FN42"
    assert ft4.spot_line(dict(rec, slot=1 + 8 * 60)) == "010007 -12  0.3 1235 ~  CQ K1ABC FN42"
    del rec["slot"], rec["dt_fine"]
    assert ft8.spot_line(dict(rec, text=None)) == "       -12  1.3 1235 ~"


def test_report_needs_decode_without_a_device():
    from pysdr_amd.ft4 import FT4_Skimmer
    from pysdr_amd.ft8 import FT8_Skimmer
    for cls in (FT8_Skimmer, FT4_Skimmer):
        with pytest.raises(ValueError, match="decode=True"):
            cls(8000.0, channels=(3, 3), report=True)


# ---- the accuracy measurement ---------------------------------------------------------------------------------------------------
# A raster of 13 rows, the station in the seventh: the rows 4 to 6 away on either side give its noise.  The truth is the
# generator's: the SNR it scaled the frame by against noise of power 1 in 2500 Hz, tone 0's frequency, the sample the
# frame's first Costas symbol begins at.  Never the code under test.

CHANNELS = (3, 13)
HOME_ROW = 6
T0 = 20
PLACES = ("centre", "between", "+0.7 Hz", "first", "last")
SEEDS = (0, 1, 2)
SHIFT = (0.0, 0.3, -0.4)                         # the frame's start against step T0's window, in steps, by seed
MODES = {ro.FT8: dict(name="FT8", case=(8000.0, 64, 20, 80), seconds=14.0, o=f8o, asserted=(-18.0, -15.0, -10.0, 0.0), printed=(10.0, -20.0)),
         ro.FT4: dict(name="FT4", case=(8000.0, 48, 8, 32), seconds=7.0, o=f4o, asserted=(-12.0, -9.0, -6.0, 0.0), printed=(10.0, -15.0))}
MARGIN = (0.5, 0.1, 0.02)                        # dB, Hz, steps: for the seeds not drawn
# the bounds: the worst of the asserted runs as measured (the tables in DESIGN.md 3 item 26) plus the margins
BOUNDS = {ro.FT8: (1.2, 0.5, 0.38), ro.FT4: (1.05, 1.32, 0.31)}


def spectra(mode, x):
    """the complex spectrum of every step behind the float64 channelizer -> [nk][steps][NB] complex128 (linear in x)"""
    from pysdr_amd import ft4, ft8
    m = MODES[mode]
    fs, S, D, M = m["case"]
    h = (ft8 if mode == ro.FT8 else ft4).prototype(fs, M, S)
    rows = cz.polyphase(x, h, M, D, 0, -(-len(x) // D), m["o"].rows_of(M, CHANNELS))
    nb, qs = S // 2 + (14 if mode == ro.FT8 else 6), S // 4
    T = f8o.steps_done(rows.shape[1], S)
    q = 2 * np.arange(nb) - (nb - 1)
    E = np.exp(-2j * np.pi * np.outer(np.arange(S), q) / (4 * S))
    return rows[:, (qs * np.arange(T))[:, None] + np.arange(S)[None, :]] @ E


@functools.lru_cache(maxsize=None)
def noise_spectra(mode, seed):
    m = MODES[mode]
    fs = m["case"][0]
    n = int(m["seconds"] * fs)
    rng = np.random.default_rng(9000 + 10 * mode + seed)
    return spectra(mode, m["o"].noise_sigma(0.0, 2500.0, fs) * (rng.standard_normal(n) + 1j * rng.standard_normal(n)))


def station(mode, place, gfsk, seed):
    """-> (the unit frame's spectra, tone 0's Hz, the start in steps, the fine rows that may own it, the 91 bits)"""
    from pysdr_amd import ldpc
    m = MODES[mode]
    fs, S, D, M = m["case"]
    o, nsub, qs = m["o"], S // 2, S // 4
    ff = o.fine_freqs(fs, M, S, CHANNELS)
    F = HOME_ROW * nsub + {"centre": nsub // 2 + 2, "between": nsub // 2 + 2, "+0.7 Hz": nsub // 2 + 2, "first": 0, "last": nsub - 1}[place]
    f = ff[F] + {"between": o.BAUD / 4, "+0.7 Hz": 0.7}.get(place, 0.0)
    rng = np.random.default_rng(100 * PLACES.index(place) + 10 * seed + int(gfsk) + 1000 * mode)
    bits91 = ldpc.encode(rng.integers(0, 2, 77))[:91]
    at = int(round(((T0 + SHIFT[seed]) * qs - 8) * D))                # the first Costas symbol's first sample
    t_true = (at / D + 8) / qs
    w = o.waveform(o.tones(ldpc.encode91(bits91)), f, fs, gfsk, phase=rng.uniform(0, 6.28))
    if mode == ro.FT4:
        at -= S * D                                                  # the array begins with the ramp, one symbol before the frame
    x = np.zeros(int(m["seconds"] * fs), np.complex128)
    x[at:at + len(w)] = w[:len(x) - at]
    return spectra(mode, x), f, t_true, (F, F + 1) if place == "between" else (F,), bits91


def measure(mode, place, gfsk, seed, snrs):
    """-> [(snr, snr error dB, f_fine error Hz, t_fine error steps, nhard, nsync, F - home, t0 - T0)] by the oracle and the
    host half, on the owner the finder would crown: the greatest sync score within 2 fine rows and 4 steps of the truth"""
    from pysdr_amd import ft4, ft8
    m = MODES[mode]
    fs, S, D, M = m["case"]
    o, nsub, mod = m["o"], S // 2, (ft8 if mode == ro.FT8 else ft4)
    ff = o.fine_freqs(fs, M, S, CHANNELS)
    us, f, t_true, homes, bits91 = station(mode, place, gfsk, seed)
    un = noise_spectra(mode, seed)
    out = []
    for snr in snrs:
        ring = (np.abs(un + 10 ** (snr / 20) * us) ** 2).astype(F32)     # [nk][T][NB], nothing has left it
        t_done = ring.shape[1]
        t0s = np.arange(T0 - 4, T0 + 5)
        score, _ = o.sync_scores(ring[HOME_ROW - 1:HOME_ROW + 2], t0s, nsub, F32)
        score = score.transpose(1, 0, 2).reshape(len(t0s), -1)       # [t0][fine rows of the three rows]
        lo = homes[0] - 2 - (HOME_ROW - 1) * nsub
        near = score[:, lo:lo + len(homes) + 4]
        it, iF = np.unravel_index(np.argmax(near), near.shape)
        t0, F = int(t0s[it]), int(lo + iF + (HOME_ROW - 1) * nsub)
        power, errs = ro.report(ring, t_done, nsub, False, mode, [F], [t0], [bits91])
        floor = ro.floor(ring, t_done, t0 + ro.lag(mode), ro.SYMS[mode])
        df, dt, peak = mod.refine(power[0, :9])
        noise = mod.noise_of(floor, ro.SYMS[mode], F, nsub, False, mod.TONES, mod.FLOOR_ROWS, mod.FLOOR_QUANTILE)
        got = mod.snr_db(peak, noise, ro.SYMS[mode], mod.BAUD, mod.CAL)
        out.append((snr, got - snr, ff[F] + df * mod.BAUD / 2 - f, t0 + dt - t_true, int(errs[0, 0]), int(errs[0, 1]), F - homes[0], t0 - T0, noise))
    return out


@functools.lru_cache(maxsize=None)
def table(mode):
    """every run of the measurement: {(place, gfsk, snr): [one row per seed]}"""
    m = MODES[mode]
    snrs = m["asserted"] + m["printed"]
    out = {}
    for place in PLACES:
        for gfsk in (True, False):
            for seed in SEEDS:
                for row in measure(mode, place, gfsk, seed, snrs):
                    out.setdefault((place, gfsk, row[0]), []).append(row)
    return out


def show(mode, tab):
    m = MODES[mode]
    print(f"\n{m['name']}: error of snr (dB) / f_fine (Hz) / t_fine (steps), worst of {len(SEEDS)} seeds by magnitude; "
          f"[nhard, nsync] summed over the seeds")
    for place in PLACES:
        for gfsk in (True, False):
            cells = []
            for snr in sorted(m["asserted"] + m["printed"]):
                rows = tab[(place, gfsk, snr)]
                w = [max((r[c] for r in rows), key=abs) for c in (1, 2, 3)]
                cells.append(f"{snr:+5.0f}: {w[0]:+5.2f} {w[1]:+5.2f} {w[2]:+5.2f} [{sum(r[4] for r in rows)},{sum(r[5] for r in rows)}]")
            print(f"  {place:8s} {'gfsk' if gfsk else 'rect'}  " + "  ".join(cells))


@pytest.mark.parametrize("mode", (ro.FT8, ro.FT4), ids=["ft8", "ft4"])
def test_accuracy_of_snr_fine_frequency_and_fine_time(mode):
    m = MODES[mode]
    tab = table(mode)
    show(mode, tab)
    rows = [r for (place, gfsk, snr), v in tab.items() if snr in m["asserted"] for r in v]
    assert len(rows) == len(PLACES) * 2 * len(SEEDS) * len(m["asserted"])
    worst = [max(abs(r[c]) for r in rows) for c in (1, 2, 3)]
    mean = float(np.mean([r[1] for r in rows]))
    B, Bf, Bt = BOUNDS[mode]
    print(f"{m['name']}: worst |snr error| {worst[0]:.2f} dB (mean {mean:+.2f}), |f_fine error| {worst[1]:.3f} Hz, |t_fine error| {worst[2]:.3f} steps "
          f"over {len(rows)} runs; bounds {B} dB, {Bf} Hz, {Bt} steps")
    assert all(abs(r[6]) <= 2 and abs(r[7]) <= 1 for r in rows)                 # the owner is the station's
    assert B <= 2.5 and Bf < m["o"].BAUD / 4
    assert worst[0] <= B and worst[1] <= Bf and worst[2] <= Bt
    # the bounds are the measurement plus the margins, rounded up to the digits shown, not a loose guess
    assert worst[0] >= B - MARGIN[0] - 0.05 and worst[1] >= Bf - MARGIN[1] - 0.01 and worst[2] >= Bt - MARGIN[2] - 0.01
