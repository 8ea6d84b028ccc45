"""The SSTV skimmer's definition on the CPU: the float32 oracle of steps 1 to 8 (tests/sstv_oracle.py)
behind the float64 channelizer model (tests/channelizer_oracle.py) reads the header of every mode, at every phase of the
tick clock and off tune, refuses wrong parity, unknown codes and noise, and rebuilds the first lines of PD120 and Martin M1
pictures as well as the float64 form of the same definition does.  The GPU tests hold the kernel equal to this oracle; that
the oracle reads what was sent is shown here, so that they cannot pass on silence.  No device.

Noisy cases: USB at 15 dB in a 12 kHz row, FM at 20 dB C/N (deviation 3 kHz) in a 16 kHz row, fixed seeds."""
import functools

import numpy as np
import pytest

from tests import channelizer_oracle as cz
from tests import sstv_oracle as so

# det: (fs, M, D, channels between stations, SNR dB in the row bandwidth)
BANDS = {"USB": (96000.0, 32, 8, 2, 15.0), "FM": (256000.0, 64, 16, 4, 20.0)}
OMODES = so.MODES + [so.TINY]


def sv():
    from pysdr_amd import sstv
    return sstv


def all_modes():
    return sv().MODES + (sv().Mode("TINY", 5, 3, 32, 6, 5.0, 1.0, 0.5, 0.5, "GBR"),)


def smooth(mode, lines, seed=0):
    """at most two sine periods per scan"""
    x = np.arange(mode.width)
    return np.array([[np.round(127.5 + 110.0 * np.sin(2 * np.pi * (1 + (l + j + seed) % 2) * x / mode.width + l + 2 * j + seed))
                      for j in range(mode.scans)] for l in range(lines)]).astype(np.uint8)


def rows_of(det, stations, seconds, snr="band", seed=0, band=None):
    """stations: (slot, Hz off, start s, (Hz, ms) list); slot k sits on channel 1 + k * (channels between stations).
    -> the rows of the stations' channels behind the float64 channelizer model, complex64 [len(stations)][n], fs_out"""
    fs, M, D, step, db = BANDS[det] if band is None else band
    n = int(seconds * fs)
    rng = np.random.default_rng(seed)
    x = np.zeros(n, np.complex128)
    if snr is not None:
        pn = 10 ** (-db / 10) * D                                            # unit stations: noise power over the whole band
        x += np.sqrt(pn / 2) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    ks = []
    for slot, off, t0, tl in stations:
        k = 1 + slot * step
        ks.append(k)
        s = sv().waveform(tl, fs, k * fs / M + off, det).astype(np.complex128)
        at = int(t0 * fs)
        x[at:at + len(s)] += s[:n - at]
    y = cz.polyphase(0.1 * x, sv().prototype(fs, M, D, det), M, D, 0, -(-n // D), ks=np.array(ks)).astype(np.complex64)
    return y, fs / D


def records(y, fs_out, det, twin=False, modes=OMODES, chunk=1 << 16):
    o = so.Oracle(y.shape[0], fs_out, det, modes, twin=twin)
    out, running = [[] for _ in range(y.shape[0])], {}
    for at in range(0, y.shape[1], chunk):
        wc, ev = o.process(y[:, at:at + chunk])
        for r in np.flatnonzero(wc):
            for rec in so.unpack(ev[r], o.par["modes"], running.get(r)):
                if rec[1] == "start":
                    running[r] = rec[2]
                out[r].append((at + rec[0],) + rec[1:])
    return out, o


# ---- step 3 -------------------------------------------------------------------------------------------------------------
def test_the_polynomial_is_within_a_quarter_level_of_the_arctangent():
    """|phi(t) - arctan(t)| <= 1e-4 rad on |t| <= 1: one luminance level at 48 kHz is 2 pi (800 / 255) / 48000 = 4.1e-4 rad"""
    t = np.linspace(-1.0, 1.0, 200001).astype(np.float32)
    t2 = t * t
    s = t2 * so.A[4]
    for a in (so.A[3], so.A[2], so.A[1]):
        s = t2 * (a + s)
    phi = t * (so.A[0] + s)
    err = np.abs(phi.astype(np.float64) - np.arctan(t.astype(np.float64))).max()
    print("worst error of the polynomial:", err)
    assert err <= 1e-4
    for v in (-1.0, -0.3, 0.0, 0.77, 1.0):
        assert so.phi32(v) == phi[np.argmin(np.abs(t - np.float32(v)))] or abs(float(so.phi32(v)) - np.arctan(v)) <= 1e-4
    o = so.Oracle(1, 48000.0, "USB")
    assert o.hz(np.float32(0), np.float32(0)) == 0 and o.hz(np.float32(-1), np.float32(2)) == so.phi32(1) * o.par["k_hz"]
    assert o.hz(np.float32(1e-30), np.float32(-1)) == so.phi32(-1) * o.par["k_hz"]


# ---- step 5 -------------------------------------------------------------------------------------------------------------
def head(mode, parity_error=False, code=None):
    """a header and the start of line 0: sync, porch, 40 ms of mid grey"""
    s = sv()
    return [(1900.0, 40.0)] + s.vis_tones(mode.code if code is None else code, parity_error) + [(1200.0, mode.sync), (1500.0, mode.porch), (1900.0, 60.0)]


@pytest.mark.parametrize("det", ("USB", "FM"))
def test_every_code_is_recognised_wrong_parity_and_unknown_codes_are_not(det):
    modes = all_modes()
    st = [(k, 0.0, 0.003 * k, head(m)) for k, m in enumerate(modes)]
    st += [(len(modes), 0.0, 0.0, head(modes[2], parity_error=True)), (len(modes) + 1, 0.0, 0.0, head(modes[2], code=7)),
           (len(modes) + 2, 0.0, 0.0, head(modes[2], code=0x7F ^ modes[2].code))]
    y, fs_out = rows_of(det, st, 1.1, seed=3)
    recs, o = records(y, fs_out, det)
    for k, m in enumerate(modes):
        assert [(r[1], r[2], r[3]) for r in recs[k] if r[1] != "line"] == [("start", k, m.code)], (m.name, recs[k])
        assert abs(recs[k][0][4]) < 15.0, (m.name, recs[k][0][4])              # f_lead: the station is on tune
    for k in range(len(modes), len(modes) + 3):
        assert recs[k] == [], k
    st = o.state()
    assert list(st["phase"][:len(modes)]) == [2] * len(modes) and not st["phase"][len(modes):].any()


@pytest.mark.parametrize("det", ("USB", "FM"))
def test_tiny_is_recognised_at_seven_start_offsets_across_one_tick_and_off_tune(det):
    tiny = all_modes()[-1]
    offs = [0.010 * k / 7 for k in range(7)]
    st = [(k, 0.0, 0.02 + t, head(tiny)) for k, t in enumerate(offs)]
    if det == "USB":
        st += [(7, 100.0, 0.02, head(tiny)), (8, -100.0, 0.02, head(tiny))]
    y, fs_out = rows_of(det, st, 1.1, seed=5)
    recs, o = records(y, fs_out, det)
    rel = []
    for k in range(7):
        assert [(r[1], r[2], r[3]) for r in recs[k] if r[1] != "line"] == [("start", len(OMODES) - 1, tiny.code)], (k, recs[k])
        rel.append(recs[k][0][5] - (0.02 + offs[k]) * fs_out)
    print("e0 behind the transmission's start, row samples:", np.round(rel, 2))
    assert max(rel) - min(rel) <= 3.0                                        # the anchor follows the station, not the tick clock
    for k, f in ((7, 100.0), (8, -100.0)) if det == "USB" else ():
        assert [(r[1], r[3]) for r in recs[k] if r[1] != "line"] == [("start", tiny.code)] and abs(recs[k][0][4] - f) < 15.0, (k, recs[k])


@pytest.mark.parametrize("det,fs_out", (("USB", 12000.0), ("FM", 16000.0)))
def test_five_minutes_of_white_noise_give_no_start(det, fs_out):
    rng = np.random.default_rng(11 if det == "USB" else 12)
    o = so.Oracle(1, fs_out, det, OMODES)
    n, chunk = int(300 * fs_out), 1 << 19
    for at in range(0, n, chunk):
        k = min(chunk, n - at)
        y = (0.1 * (rng.standard_normal(k, np.float32) + 1j * rng.standard_normal(k, np.float32))).astype(np.complex64)
        wc, ev = o.process(y[None, :])
        assert not wc.any(), at
    st = o.state()
    assert st["phase"][0] == 0 and st["ticks"][0] in (29999, 30000)           # w_tick is 100 Hz rounded to 2^-32 turns


# ---- steps 6 to 8 -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def first_lines(name, det, noisy):
    s = sv()
    mode = s.mode_named(name)
    pic = smooth(mode, 3, seed=1)
    tl = [(1900.0, 30.0)] + s.tones(mode, pic) + [(1900.0, 80.0)]
    band = {"USB": (48000.0, 16, 4, 2, 15.0), "FM": (100000.0, 16, 4, 4, 20.0)}[det]     # rows at 12 and 25 kHz
    y, fs_out = rows_of(det, [(1, 0.0, 0.01, tl)], 0.01 + sum(t[1] for t in tl) * 1e-3, snr="band" if noisy else None, seed=21, band=band)
    out = {}
    for twin in (False, True):
        recs, o = records(y, fs_out, det, twin=twin, modes=so.MODES)
        lines = [r for r in recs[0] if r[1] == "line"]
        assert [r[1] for r in recs[0]] == ["start"] + ["line"] * len(lines) and len(lines) >= 3 and recs[0][0][3] == mode.code, (name, det, twin)
        err = np.abs(np.array([r[3] for r in lines[:3]]).astype(int) - pic.astype(int))
        out[twin] = (err.mean(), np.percentile(err, 99), recs[0][0][5])
    return out


@pytest.mark.parametrize("name", ("PD120", "Martin M1"))
@pytest.mark.parametrize("det", ("FM", "USB"))
def test_the_first_three_lines_are_as_good_as_the_float64_twin_s(name, det):
    """FM at 25 kHz rows, USB at 12 kHz rows, no noise.  The yardstick is the float64 form of the same definition (np.arctan2,
    float64 sums) on the same rows; the float32 oracle's mean absolute error and 99th percentile are asserted at twice the
    twin's (the margin is for the channelizer's ripple).  Measured here, in levels of 255 (mean, 99 %), twin = oracle to
    two digits: PD120 FM 0.46, 2; PD120 USB 0.12, 1; Martin M1 FM 0.22, 1; Martin M1 USB 0.08, 1 (LABNOTES 35)."""
    r = first_lines(name, det, False)
    (mae, p99, e0), (mae64, p99_64, e0_64) = r[False], r[True]
    print(f"{name} {det}: float32 mean {mae:.3f} p99 {p99:.1f} e0 {e0}; float64 twin mean {mae64:.3f} p99 {p99_64:.1f} e0 {e0_64}")
    assert e0 == e0_64
    assert mae <= 2 * mae64 and p99 <= 2 * p99_64
    assert mae64 < 3.0                                                       # the twin itself reads the picture


@pytest.mark.parametrize("name,det", (("Martin M1", "USB"), ("Martin M1", "FM")))
def test_the_first_three_lines_in_noise(name, det):
    """USB at 15 dB, FM at 20 dB C/N: header, anchor and lines are found; the error is measured against the twin's as above.
    Measured here (mean, 99 %), twin = oracle: USB 8.80, 30; FM 5.47, 17.2."""
    r = first_lines(name, det, True)
    (mae, p99, e0), (mae64, p99_64, e0_64) = r[False], r[True]
    print(f"{name} {det} in noise: float32 mean {mae:.3f} p99 {p99:.1f} e0 {e0}; float64 twin mean {mae64:.3f} p99 {p99_64:.1f} e0 {e0_64}")
    assert abs(e0 - e0_64) <= 1 and mae <= 2 * mae64 and p99 <= 2 * p99_64


# ---- the non-finite samples --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", ("USB", "FM"))
def test_a_non_finite_sample_blanks_its_windows_and_nothing_else(det):
    fs_out = 12000.0
    rng = np.random.default_rng(4)
    y = (0.1 * (rng.standard_normal(4000) + 1j * rng.standard_normal(4000))).astype(np.complex64)[None, :]
    bad = y.copy()
    bad[0, 1500] = complex(np.nan, 0.25)
    bad[0, 2500] = complex(-0.5, np.inf)
    o, ob = so.Oracle(1, fs_out, det), so.Oracle(1, fs_out, det)
    (cx, cy), (bx, by) = o.lag_products(y), ob.lag_products(bad)
    diff = np.flatnonzero((cx[0] != bx[0]) | (cy[0] != by[0])) - o.nq
    per = o.L + 1 + (1 if det == "FM" else 0)                                # behind the discriminator a sample is in two outputs
    assert list(diff) == list(range(1500, 1500 + per)) + list(range(2500, 2500 + per))
    assert not bx[0][diff + o.nq].any() and not by[0][diff + o.nq].any() and np.isfinite(bx).all() and np.isfinite(by).all()
    o.process(y)
    ob.process(bad)
    a, b = o.state(), ob.state()
    assert np.isfinite(b["ring"]).all() and a["ticks"][0] == b["ticks"][0] == 33
    changed = np.flatnonzero(a["ring"][0] != b["ring"][0])
    assert 1 <= len(changed) <= 6                                            # the ticks that hold the windows, and their neighbours' halves
