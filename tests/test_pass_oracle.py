"""The definition of the FT8 / FT4 second pass on the CPU, through its NumPy model (tests/pass_oracle.py)
and the package's own tables and trial grid (pysdr_amd/ft8.py, ft4.py), which the model derives independently:

* the tables and the phase word of both derivations are equal, and the pulse table ends in exactly one turn;
* with nothing subtracted, recomputing any range of steps of any row from the kept samples gives the spectrum ring bit for
  bit, at three moments of a stream that wraps both rings, for FT8 and FT4;
* behind the float64 channelizer, one noiseless GFSK station on the raster and 0.7 Hz off it, at the time offsets of
  tests/test_report_oracle.py, with the skimmer's own trial grid around the refined place: the float64 model's table is
  printed, the float32 model is within 1 dB of it, and no case is worse than the float64 worst case
  less 3 dB;
* the oracle skimmer (``pass_oracle.Skimmer``) with ``passes=1`` and ``passes=2`` on a grid of 12 pairs in noise, on one FT4
  pair, and on three cuttings of one stream;
* the definition alone, without a channelizer: a noiseless GFSK station (``ft8.waveform`` / ``ft4.waveform``, ramps included) synthesised at the row rate is taken out of
  its own bins of the residue: on the raster, 0.7 Hz off it, and at time offsets of a fraction of a step, with the true
  offsets among nine trials.  The figures are printed (as found: -67 to -72 dB of the samples, -94 to -107 dB of the bins,
  -39.4 dB of the bins for the FT4 frame 5 samples early).  The bounds asserted are reasoned, not measured: the reference
  differs from the station only by the cos / sin table's phase step (2 pi / 4096: a residue of (pi / 4096)^2 / 3 =
  -67.1 dB of the samples, asserted with 1 dB for float32 rounding), the rounding of the phase word (2^-32 turns per
  sample: nothing) and, for FT4, by the ramps, which are not among the frame's symbols.  The true trial must win.

CPU only."""
import functools

import numpy as np
import pytest

from tests import channelizer_oracle as cz
from tests import ft4_oracle as f4o
from tests import ft8_oracle as f8o
from tests import pass_oracle as po
from tests import report_oracle as ro

F32 = np.float32


def fbits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def mode_of(mode):
    from pysdr_amd import ft4, ft8
    return ft8 if mode == po.FT8 else ft4


def oracle(mode, nk, S, max_out, reach_t):
    o = (f8o if mode == po.FT8 else f4o)
    return po.PassOracle(mode, o.Oracle(nk, S, o.params(), max_out), reach_t, False)


@pytest.mark.parametrize("mode,S", ((po.FT8, 64), (po.FT8, 96), (po.FT4, 48), (po.FT4, 72)))
def test_both_derivations_of_the_tables_agree(mode, S):
    from pysdr_amd import ft8
    m = mode_of(mode)
    pl = ft8.pass_pulse(m, S)
    assert pl.dtype == np.uint32 and len(pl) == po.PULSE_SYMS[mode] * S == m.PULSE_SYMBOLS * S
    assert [int(v) for v in pl] == po.pulse(mode, S)
    v = pl.astype(np.int64)
    v[len(v) // 2:][v[len(v) // 2:] == 0] = 1 << 32                                # a whole turn is stored as 0
    assert pl[-1] == 0 and pl[0] < 1 << 8 and (np.diff(v) >= 0).all() and v[-1] == 1 << 32   # one whole turn, rising
    assert abs(int(pl[len(pl) // 2 - 1]) - (1 << 31)) <= 1                               # the pulse is even about its middle: half a turn by then
    lut = ft8.pass_lut()
    c, s = po.lut()
    assert lut.shape == (4096, 2) and np.array_equal(fbits(lut[:, 0]), fbits(c)) and np.array_equal(fbits(lut[:, 1]), fbits(s))
    for q in (-(S // 2 + 13), -1, 0, 1, 5, S // 2 + 13, -3 * S):
        w = po.word(q, S)
        assert abs(w - (q * 2.0 ** 32 / (4 * S)) % 2.0 ** 32) <= 0.5 + 1e-3 or w == 0
    assert po.word(4 * S, S) == 0 and po.word(2, 64) == 1 << 25


def test_the_rows_of_a_frame():
    for mode, S, extra in ((po.FT8, 64, 14), (po.FT8, 96, 14), (po.FT4, 48, 6), (po.FT4, 72, 6)):
        nsub = S // 2
        for nk, circular in ((3, False), (4, True), (1, False), (1, True)):
            for F in range(nk * nsub):
                a, j = divmod(F, nsub)
                rows = po.frame_rows(mode, F, S, nk, circular)
                assert rows[0] == (a, 2 * j - (nsub + extra - 1)) and len(rows) <= 2
                up, down = j + extra >= nsub, j <= extra - 1
                assert not (up and down)
                want = a + 1 if up else (a - 1 if down else None)
                if want is not None and circular:
                    want %= nk
                if want is None or not 0 <= want < nk or want == a:
                    assert len(rows) == 1
                else:
                    # the same frequency seen from the neighbour's centre, nsub bins = 2 nsub quarter-bauds away
                    assert rows[1] == (want, rows[0][1] + (-2 * nsub if up else 2 * nsub))


@pytest.mark.parametrize("mode,S", ((po.FT8, 64), (po.FT4, 48)))
def test_respectrum_is_the_spectrum(mode, S):
    rng = np.random.default_rng(27 + S)
    nk, max_out, reach_t = 3, 64, 8
    p = oracle(mode, nk, S, max_out, reach_t)
    total = p.ty + 24 * S                                                         # both rings wrap
    rows = (rng.standard_normal((nk, total)) + 1j * rng.standard_normal((nk, total))).astype(np.complex64)
    at, moments, when = 0, 0, (40, p.tr2 + 3, p.tr2 + 60, 1 << 30)
    for n in list(rng.integers(0, max_out + 1, 600)):
        if at >= total:
            break
        n = min(int(n), total - at)
        p.process(rows[:, at:at + n])
        at += n
        done = p.o.t_done
        if done < when[moments]:
            continue
        moments += 1
        lo = p.first_step()
        both = np.arange(max(lo, done - p.o.tr), done)                            # the steps both rings hold
        assert np.array_equal(fbits(p.ring2[:, both % p.tr2]), fbits(p.o.ring[:, both % p.o.tr]))
        before = p.ring2.copy()
        for row in range(nk):
            for t_lo, t_hi in ((lo, lo), (done - 1, done - 1), (lo, done - 1), (lo + 7, lo + 29)):
                p.ring2[row, np.arange(t_lo, t_hi + 1) % p.tr2] = -1
                p.respectrum(row, t_lo, t_hi)
        assert np.array_equal(fbits(p.ring2), fbits(before)), (done, np.argwhere(fbits(p.ring2) != fbits(before))[:4])
        assert np.array_equal(p.yk[:, np.arange(max(0, at - p.ty), at) % p.ty], rows[:, max(0, at - p.ty):at])
    assert moments >= 3 and p.o.t_done > p.tr2 and p.n_abs > p.ty


SHIFT = (0, 3, -5)                                                               # whole row samples: fractions of a step (QS = 16, 12)
CASES = [(po.FT8, 64, 0.0, s) for s in SHIFT] + [(po.FT8, 64, 0.7, 0), (po.FT8, 96, 0.7, 3), (po.FT4, 48, 0.0, 0), (po.FT4, 48, 2.0, -5)]


@pytest.mark.parametrize("mode,S,off,shift", CASES)
def test_a_noiseless_station_leaves_its_bins(mode, S, off, shift):
    from pysdr_amd import ldpc
    m = mode_of(mode)
    rng = np.random.default_rng(5)
    nk, max_out, reach_t, t0, F = 3, 64, 8, 9, S // 2 + 8                         # row 1, j = 8: row 0 holds some of its tones too (FT8)
    p = oracle(mode, nk, S, max_out, reach_t)
    qs, fs_out = S // 4, S * m.BAUD
    bits91 = ldpc.encode(rng.integers(0, 2, 77))[:91]
    tones = ro.frame_tones(mode, bits91)
    q = po.frame_rows(mode, F, S, nk, False)[0][1]
    ramp = S if mode == po.FT4 else 0                                            # ft4.waveform starts a symbol early, at its ramp
    w = m.waveform(tones, q * m.BAUD / 4 + off, fs_out, phase=0.3)
    total = qs * (t0 + p.lag + 12) + S
    rows = np.zeros((nk, total), np.complex128)
    start = qs * t0 + shift - ramp
    rows[1, start:start + len(w)] = 0.25 * w
    rows = rows.astype(np.complex64)
    for at in range(0, total, max_out):
        p.process(rows[:, at:at + max_out])
    assert p.frame_ok(t0)
    before = po.frame_power(p.ring2, p.tr2, S // 2, F, t0, tones)
    fw = int(np.rint(off / fs_out * 2.0 ** 32))
    step = int(np.rint(0.3 / fs_out * 2.0 ** 32))
    trials = [(shift + dn, (fw + df * step) & po.MASK) for dn in (-qs // 2, 0, qs // 2) for df in (-1, 0, 1)]
    out = p.subtract([F], [t0], [bits91], np.array(trials, np.int64))
    after = po.frame_power(p.ring2, p.tr2, S // 2, F, t0, tones)
    db = 10 * np.log10(max(after, 1e-300) / before)
    sdb = 10 * np.log10(max(float(out["after"][0, 0]), 1e-300) / float(out["before"][0, 0]))
    print(f"mode {mode} S {S} off {off} Hz shift {shift}: trial {out['trial'][0]} used {out['used'][0]} bins {db:.1f} dB samples {sdb:.1f} dB")
    assert out["trial"][0, 0] == 4 and out["used"][0, 0] == len(tones)
    # FT4's ramps are not among the frame's symbols: |shift| samples of one lie in the window of the first or the last step,
    # at an amplitude of at most 1 on the held tone, against windows that hold S - |shift| samples of their own symbol
    leak = (abs(shift) / (S - abs(shift))) ** 2 / len(tones) if mode == po.FT4 else 0.0
    assert sdb <= -66.0 and db <= 10 * np.log10(leak + 10 ** -6.6)
    if mode == po.FT8:                                                           # the row below holds nothing: nothing is taken
        assert out["used"][0, 1] == len(tones) and out["before"][0, 1] == 0 and out["after"][0, 1] == 0


# ---- behind the float64 channelizer: the suppression of one noiseless station, float64 model against float32 model ---------
CHANNELS = (3, 3)
T0 = 20
STEP_SHIFT = (0.0, 0.3, -0.4)                                                    # tests/test_report_oracle.py's SHIFT, in steps
# the float64 model's figures as measured (printed below): dB left in the frame's own bins
WORST64 = -34.9                                                                  # the worst of them: +0.7 Hz, +0.3 step
BOUND = WORST64 + 3.0                                                            # no case may leave more than this (seed-to-seed margin)


def rows64(mode, x):
    """the rows of the float64 channelizer on the 8000 Hz three-row shape -> complex128 [3][n]"""
    from pysdr_amd import ft4, ft8
    fs, S, D, M = (8000.0, 64, 20, 80) if mode == po.FT8 else (8000.0, 48, 8, 32)
    o = f8o if mode == po.FT8 else f4o
    h = (ft8 if mode == po.FT8 else ft4).prototype(fs, M, S)
    return cz.polyphase(x, h, M, D, 0, -(-len(x) // D), o.rows_of(M, CHANNELS))


def suppression(off, shift):
    """one noiseless GFSK FT8 station -> (dB left by the float64 model, by the float32 model, the trial each chose)"""
    from pysdr_amd import ft8, ldpc
    mode, fs, S, D, M, nk = po.FT8, 8000.0, 64, 20, 80, 3
    nsub, qs, F = S // 2, S // 4, S // 2 + 18                                     # row 1, j = 18: row 2 holds its upper tones too
    rng = np.random.default_rng(int(10 * off) + int(100 * (shift + 1)))
    bits91 = ldpc.encode(rng.integers(0, 2, 77))[:91]
    tones = ro.frame_tones(mode, bits91)
    f = f8o.fine_freqs(fs, M, S, CHANNELS)[F] + off
    at = int(round(((T0 + shift) * qs - 8) * D))                                 # the first Costas symbol's first sample
    x = np.zeros(int(14.0 * fs), np.complex128)
    w = ft8.waveform(tones, f, fs, phase=0.7)
    x[at:at + len(w)] = 0.05 * w
    y = rows64(mode, x)
    p = oracle(mode, nk, S, 256, 40)
    for i0 in range(0, y.shape[1], 256):
        p.process(y[:, i0:i0 + 256].astype(np.complex64))
    power, _ = ro.report(p.o.ring, p.o.t_done, nsub, False, mode, [F], [T0], [bits91])
    df, dt = po.refine(power[0, :9])
    trials = po.trial_grid(mode, df, dt, qs, S * f8o.BAUD)
    b32 = po.frame_power(p.ring2, p.tr2, nsub, F, T0, tones)
    out = p.subtract([F], [T0], [bits91], np.array([trials], np.int64))
    a32 = po.frame_power(p.ring2, p.tr2, nsub, F, T0, tones)
    q = po.frame_rows(mode, F, S, nk, False)[0][1]
    z, trial = po.subtract64(mode, S, y[1], qs * T0, q, tones, trials)
    b64, a64 = po.bins64(mode, S, y[1], F - nsub, T0, tones), po.bins64(mode, S, z, F - nsub, T0, tones)
    return 10 * np.log10(a64 / b64), 10 * np.log10(a32 / b32), trial, int(out["trial"][0, 0]), df, dt


def test_suppression_behind_the_channelizer_float32_within_a_decibel_of_float64():
    tab = {}
    for off in (0.0, 0.7):
        for shift in STEP_SHIFT:
            tab[(off, shift)] = suppression(off, shift)
            d64, d32, t64, t32, df, dt = tab[(off, shift)]
            print(f"+{off} Hz, {shift:+.1f} step: float64 {d64:.1f} dB (trial {t64}), float32 {d32:.1f} dB (trial {t32}); refined df {df:+.3f} dt {dt:+.3f}")
    worst = max(v[0] for v in tab.values())
    print(f"the float64 model's worst case: {worst:.1f} dB")
    for k, (d64, d32, t64, t32, _, _) in tab.items():
        assert t64 == t32, k
        assert abs(d32 - d64) <= 1.0, (k, d32, d64)                              # rounding is all that separates the models
        assert d32 <= BOUND and d64 <= BOUND, (k, d32, d64, BOUND)
    assert abs(worst - WORST64) <= 0.5                                           # the figure recorded above is the one measured


# ---- the skimmer with a second pass, on the models ------------------------------------------------------------------------------
LEVELS, OFFSETS, STEPS_LATER = (6, 12, 18), (1, 3, 7, 16), 6
GRID = [(lvl, off) for lvl in LEVELS for off in OFFSETS]
F_STRONG = 22                                                                    # row 0, j = 22
# the pairs (dB under, fine rows above) whose weak station the first pass loses and the second gains, as found: ten of the
# twelve; at 16 fine rows and 6 or 12 dB under, the first pass decodes the weak station itself
GAINS = [(6, 1), (6, 3), (6, 7), (12, 1), (12, 3), (12, 7), (18, 1), (18, 3), (18, 7), (18, 16)]


def pair_texts():
    from tests.test_gpu_ldpc import TEXTS
    return TEXTS[0], TEXTS[1]


def pair_input(mode, lvl, off, seconds=None):
    """strong station at 0 dB in 2500 Hz on fine row F_STRONG, the weak one ``lvl`` dB under it, ``off`` fine rows above and 6
    steps later, in noise of power 1 in 2500 Hz; seeds fixed -> (complex64 input at 8000 Hz, the two messages' 77 bits)"""
    from pysdr_amd import ft8msg, ldpc
    o = f8o if mode == po.FT8 else f4o
    fs, S, D, M = (8000.0, 64, 20, 80) if mode == po.FT8 else (8000.0, 48, 8, 32)
    seconds = (15.5 if mode == po.FT8 else 7.5) if seconds is None else seconds
    n = int(seconds * fs)
    rng = np.random.default_rng(2700 + 100 * lvl + off + 1000 * mode)
    x = o.noise_sigma(0.0, 2500.0, fs) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    ff = o.fine_freqs(fs, M, S, CHANNELS)
    msgs = [ft8msg.pack77(t) for t in pair_texts()]
    for k, (F, db, later) in enumerate(((F_STRONG, 0.0, 0), (F_STRONG + off, -float(lvl), STEPS_LATER))):
        w = o.waveform(o.tones(ldpc.encode(msgs[k])), ff[F], fs, phase=1.0 + k) * 10 ** (db / 20)
        at = int(0.5 * fs) + later * (S // 4) * D
        x[at:at + len(w)] += w[:n - at]
    return (0.05 * x).astype(np.complex64), msgs


@functools.lru_cache(maxsize=None)
def pair_rows(mode, lvl, off):
    x, msgs = pair_input(mode, lvl, off)
    y = rows64(mode, x.astype(np.complex128)).astype(np.complex64)
    y.setflags(write=False)
    return y, msgs


def skim(mode, lvl, off, passes, max_out=256, cuts=None):
    y, msgs = pair_rows(mode, lvl, off)
    sk = po.Skimmer(mode, 3, 64 if mode == po.FT8 else 48, False, max_out, passes)
    return sk.push(y, cuts), msgs


def same_records(a, b, drop=()):
    assert len(a) == len(b), (len(a), len(b))
    for r, s in zip(a, b):
        assert sorted(r) == sorted(s)
        for k in r:
            if k in drop:
                continue
            if isinstance(r[k], np.ndarray) and r[k].dtype == F32:
                assert np.array_equal(fbits(r[k]), fbits(s[k])), k
            else:
                assert np.array_equal(r[k], s[k]), k


def run_pair(mode, lvl, off):
    """-> (the weak station decodes in pass 1, is gained by pass 2)"""
    one, msgs = skim(mode, lvl, off, 1)
    two, _ = skim(mode, lvl, off, 2)
    same_records([r for r in two if r["pass"] == 1], one)                        # every pass-1 record is unchanged
    second = [r for r in two if r["pass"] == 2]
    for r in second:
        assert any(np.array_equal(r["bits77"], m) for m in msgs), (lvl, off, r["t0"], r["F"])   # no false message
    in1 = any(r["ok"] and np.array_equal(r["bits77"], msgs[1]) for r in one)
    in2 = any(np.array_equal(r["bits77"], msgs[1]) for r in second)
    strong = any(r["ok"] and np.array_equal(r["bits77"], msgs[0]) for r in one)
    print(f"weak {lvl:2d} dB under, {off:2d} fine rows above: strong {'ok' if strong else '--'}, weak in pass 1 {'ok' if in1 else '--'}, "
          f"in pass 2 {'ok' if in2 else '--'} ({len(one)} + {len(second)} records)")
    return in1, in2


def test_the_gain_on_a_grid_of_twelve_pairs():
    got = {(lvl, off): run_pair(po.FT8, lvl, off) for lvl, off in GRID}
    gains = sorted(k for k, (in1, in2) in got.items() if in2 and not in1)
    print("gained by the second pass:", gains)
    assert len(gains) >= 1
    assert gains == GAINS


FT4_PAIR = (12, 3)


def test_the_gain_on_an_ft4_pair():
    in1, in2 = run_pair(po.FT4, *FT4_PAIR)
    assert in2 and not in1


def test_the_records_do_not_depend_on_how_the_stream_is_cut():
    lvl, off = GAINS[0]
    a, _ = skim(po.FT8, lvl, off, 2, 256)
    n = pair_rows(po.FT8, lvl, off)[0].shape[1]
    rng = np.random.default_rng(3)
    cuts = []
    while sum(cuts) < n:
        cuts.append(int(rng.integers(0, 257)))
    key = lambda r: (r["t0"], r["F"], r["pass"])                                 # noqa: E731
    assert any(r["pass"] == 2 for r in a)
    for b in (skim(po.FT8, lvl, off, 2, 64)[0], skim(po.FT8, lvl, off, 2, 256, cuts)[0]):
        same_records(sorted(a, key=key), sorted(b, key=key))
