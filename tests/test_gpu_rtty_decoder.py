"""The RTTY decoder bank on the GPU (pysdr_amd/csrc/rtty.hip): the executed reference's fixture, cut independence,
all 2041 decoders against the CPU restatement, and the skimmer end to end (IQ -> device lines -> text), also behind
a Receiver in RTTY mode."""
import ctypes
import os

import numpy as np
import pytest

from oracle import rtty_oracle as ro
from tests import rtty_decoder_oracle as rdo
from tests.test_rtty_decoder import TOL_SCORE, compare_exactly, compare_with_fixture, load_fixture

pytestmark = pytest.mark.gpu


def raw_all(dec, lines, cuts, flipped=True):
    """decode_raw over the given cuts of host lines, concatenated"""
    parts = [dec.decode_raw(c, len(c), False, flipped, per_line=True) for c in np.split(lines, cuts) if len(c)]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def test_fixture_parity():
    from pysdr_amd import rtty
    f = load_fixture()
    dec = rtty.RTTY_Decoders(48000, bins=range(800, 1243), find_bins=(800, 1250), max_lines=512)
    r = raw_all(dec, f["lines"], [512])
    assert list(r["n"]) == list(range(30, 901, 30))
    ev = [(int(r["n"][j]), 800 + int(k), rtty.code_text(int(r["codes"][j, k]))) for j, k in zip(*np.nonzero(r["codes"] >= 0))]
    compare_with_fixture(f, r["codes"], r["t"], r["ndet"], ev)
    sel = f["sel"].astype(np.int64) - 800
    ok = f["sel_gap"] >= TOL_SCORE
    assert np.array_equal(r["isym"][:, sel][ok], f["sel_isym"][ok])
    assert np.array_equal(r["best"][:, sel], f["sel_best"])        # quantised lines: every score is exact
    compare_exactly(f, r["codes"], r["t"], ev, r["isym"][:, sel])
    # the public form: events ordered by (n, bin) and per-bin text
    dec.reset()
    got = dec.decode(f["lines"])
    assert got == sorted(got, key=lambda e: (e[0], e[1]))
    hz = dict(zip(f["bins"].tolist(), f["horizon"].tolist()))
    keep = lambda evs: [e for e in evs if e[0] <= 30 * hz[e[1]]]
    assert keep(got) == keep(f["events"])
    assert np.array_equal(dec.ndet, f["ndet"])
    for b, text in f["signals"]:
        assert dec.text[b] == "".join(c for n, bb, c in f["events"] if bb == b)
    dec.close()


def random_lines(nlines, seed, nsig=10):
    rng = np.random.default_rng(seed)
    sigs = [(int(b), "RYRY CQ TEST 599 DE AB1CD", float(rng.uniform(0.02, 0.2)), float(rng.uniform(0, 0.165)))
            for b in rng.choice(np.arange(30, 2000, 60), nsig, replace=False)]
    x = rdo.synth_band(48000, sigs, (nlines // 4 + 1) * 1056, 0.01, seed)
    return ro.RttyFilterbank(48000).push(x).astype(np.float32), sigs


def test_cut_independence_and_line_order():
    from pysdr_amd import _lib, rtty
    lines, _ = random_lines(700, 3)
    dec = rtty.RTTY_Decoders(48000, max_lines=256)
    whole = raw_all(dec, lines, [256, 512])
    rng = np.random.default_rng(9)
    for trial in range(2):
        dec.reset()
        cuts, c = [1, 2, 31], 31
        while c < len(lines):
            c += int(rng.integers(1, 256)) if trial else int(rng.choice([1, 29, 30, 59, 61]))
            cuts.append(min(c, len(lines)))
        got = raw_all(dec, lines, sorted(set(cuts)))
        for k in ("n", "codes", "t", "ndet", "isym", "best"):
            assert np.array_equal(got[k], whole[k]), k
        assert np.array_equal(got["snr2"], whole["snr2"], equal_nan=True)
    # the unflipped device order of pysdr_spectrum_batch, from device memory
    dec.reset()
    L = _lib.lib()
    d = ctypes.c_void_p()
    _lib.check(L.pysdr_dev_alloc(0, 256 * 2048 * 4, ctypes.byref(d)), "alloc")
    try:
        parts = []
        for a in range(0, len(lines), 256):
            blk = np.ascontiguousarray(lines[a:a + 256, ::-1])
            _lib.check(L.pysdr_dev_upload(0, d, ctypes.c_void_p(blk.ctypes.data), blk.nbytes), "upload")
            parts.append(dec.decode_raw(d.value, len(blk), True, False, per_line=True))
    finally:
        L.pysdr_dev_free(0, d)
    for k in ("codes", "t", "ndet", "isym", "best"):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k]), k
    dec.close()


def test_all_bins_agree_with_the_restatement():
    from pysdr_amd import rtty
    lines, sigs = random_lines(660, 4, nsig=14)
    dec = rtty.RTTY_Decoders(48000, max_lines=1024)
    assert dec.nb == 2041
    g = raw_all(dec, lines, [])
    c = rdo.DecoderBank(0, 2041, 800, 1243).decode(lines)
    hz = rdo.horizon(c["m_isym"], c["m_sc2"], c["m_snr"])
    nd = c["codes"].shape[0]
    assert g["codes"].shape == c["codes"].shape == (nd, 2041)
    assert hz.sum() >= 0.8 * nd * 2041
    mask = np.arange(nd)[:, None] < hz[None, :]
    assert np.array_equal(g["codes"][mask], c["codes"][mask])
    assert np.array_equal(g["t"][mask], c["t"][mask])
    s = mask & np.isfinite(c["snr2"])
    assert np.array_equal(np.isfinite(g["snr2"])[mask], np.isfinite(c["snr2"])[mask])
    assert np.array_equal(g["snr2"][s], c["snr2"][s])             # same float64 order
    ok = c["gap"] >= TOL_SCORE
    assert np.array_equal(g["isym"][ok], c["isym"][ok])
    assert np.allclose(g["best"], c["best"], rtol=1e-5, atol=1e-3)
    if c["m_find"].min() > 1e-6:
        assert np.array_equal(g["ndet"], c["ndet"])
    dec.close()


def snr_path_case(lines, b, lo, hi):
    """A line x and a decision jj such that, with line x's space at bin b + 7 set to -inf and nothing else changed,
    the restatement gates decision jj's held printable symbol with x on its SNR path at a mark bit (weight 1 on the
    mark, 0 on the space), where +-(mark - space) alone would give +inf; every margin up to jj is clear.
    -> (modified lines, jj, restatement output)"""
    k = b - lo
    nd = len(lines) // 30
    for j in range(3, nd):
        for q in range(2, 8):
            x = 30 * j - 88 + 4 * q
            mod = lines.copy()
            mod[x - 1, b + 7] = -np.inf
            r = rdo.DecoderBank(lo, hi, 0, 0).decode(mod)
            hz = rdo.horizon(r["m_isym"], r["m_sc2"], r["m_snr"])
            for jj in range(1, min(nd, hz[k])):
                tl, t = int(r["t"][jj - 1, k]), int(r["t"][jj, k])
                held = int(r["isym"][tl, k])
                path = tl - 28 + 4 * np.arange(8)
                bits = np.array([1, 0] + [(held >> i) & 1 for i in range(5)] + [1])
                if t - tl >= 25 and held not in (0, 27, 31) and x in path and bits[list(path).index(x)] == 1:
                    return mod, jj, r
    return None


def test_an_infinite_value_on_the_snr_path_emits_nothing():
    """rtty.py:657-665 weighs every mark and space of the SNR path by a bit and by 1 - bit, so one -inf dB value on it
    makes snr2 NaN and the decision emits nothing (NaN >= 8 is false) -- also where +-(mark - space) alone would give
    +inf.  Finite lines with one -inf mark on a gated decision's path."""
    from pysdr_amd import rtty
    lines, sigs = random_lines(480, 5, nsig=4)
    b = max(sigs, key=lambda s_: s_[2])[0]
    lo, hi = b - 2, b + 3
    case = snr_path_case(lines, b, lo, hi)
    assert case is not None
    mod, jj, c = case
    k = b - lo
    assert c["codes"][jj, k] == -1 and np.isnan(c["snr2"][jj, k])
    dec = rtty.RTTY_Decoders(48000, bins=range(lo, hi), max_lines=512)
    g = dec.decode_raw(mod, len(mod), False, True)
    assert g["t"][jj - 1, k] == c["t"][jj - 1, k] and g["t"][jj, k] == c["t"][jj, k]
    assert g["codes"][jj, k] == -1 and not np.isfinite(g["snr2"][jj, k])
    hz = rdo.horizon(c["m_isym"], c["m_sc2"], c["m_snr"])
    mask = np.arange(len(c["codes"]))[:, None] < hz[None, :]
    assert np.array_equal(g["codes"][mask], c["codes"][mask]) and np.array_equal(g["t"][mask], c["t"][mask])
    dec.close()


MSGS = [(850, "CQ DE K1ABC K"), (1000, "UR 599 TU"), (1150, "TEST W9XYZ")]


def skimmer_iq(fs, f0=0.0, seconds=5.0, seed=1):
    """MSGS in noise behind a preamble: the decoders take a character or two to find the timing, and the
    figures in it make sure a LTRS goes out after that"""
    sigs = [(b, text, 0.05, 0.011 * i) for i, (b, text) in enumerate(MSGS)]
    n = int(seconds * fs)
    rng = np.random.default_rng(seed)
    x = 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for b, text, amp, delay in sigs:
        x = x + rdo.baudot_fsk(fs, "RYRY 73 " + text, f0 + rdo.bin_hz(b), amp, delay + 0.2, n, phase=rng.uniform(0, 6.28))
    return x.astype(np.complex64)


def test_skimmer_end_to_end_and_device_hand_off():
    from pysdr_amd import rtty
    x = skimmer_iq(48000)
    sk = rtty.RTTY_Skimmer(48000, max_symbols=64)
    ev = []
    for c in np.array_split(x, 13):
        ev += sk.push(c)
    for b, text in MSGS:
        assert text in sk.text[b], (b, sk.text[b])
    # the same lines downloaded and flipped on the host (RTTY_Filterbank.push) give the same events
    fb = rtty.RTTY_Filterbank(48000, max_symbols=64)
    dec = rtty.RTTY_Decoders(48000, max_lines=256)
    ev2 = []
    for c in np.array_split(x, 5):
        ev2 += dec.decode(fb.push(c))
    assert ev == ev2 and len(ev) > 0
    with pytest.raises(ValueError):
        rtty.RTTY_Skimmer(44100)
    sk.close(), fb.close(), dec.close()


def test_skimmer_behind_a_receiver_in_rtty_mode():
    """receiver.py:286-290: the RTTY process is fed rx.iq of the receiver."""
    from oracle import sdr_oracle as so
    from pysdr_amd import rtty, sig_proc
    from pysdr_amd.params import RunTimeParams
    fs, frq = 2.048e6, 100e3
    L = so.chunk_sizes(fs, 48000)[3]
    x = skimmer_iq(fs, f0=frq, seed=2)
    P = RunTimeParams(fs=fs, fsout=48000, fc=[14.08e6], mode='RTTY', nfilt=1001)
    P.VIDEO_BW = 20e3
    rx = sig_proc.Receiver(P, frq, 0, '1')
    rx.mode, rx.af_bw = 'RTTY', 3e3
    sk = rtty.RTTY_Skimmer(48000, max_symbols=64)
    for k in range(len(x) // L):
        rx.demod_data(x[k * L:(k + 1) * L])
        sk.push(rx.iq)
    for b, text in MSGS:
        assert text in sk.text[b], (b, sk.text[b])
    sk.close()


def test_argument_errors():
    from pysdr_amd import _lib, rtty
    L = _lib.lib()
    dec = rtty.RTTY_Decoders(48000, bins=range(800, 900), max_lines=64)
    codes = np.zeros(4 * 100, np.int32)
    t = np.zeros(4 * 100, np.int64)
    snr = np.zeros(4 * 100)
    ndet = np.zeros(128, np.int32)
    nd = ctypes.c_int(0)
    lines = np.zeros((65, 2048), np.float32)
    pt = t.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))
    args = lambda n, c=_lib.as_pi(codes): (dec._h, ctypes.c_void_p(lines.ctypes.data), n, 0, 1, c, pt, _lib.as_pd(snr),
                                          ctypes.byref(nd), _lib.as_pi(ndet), None, None)
    assert L.pysdr_rtty_decode(*args(65)) == -1
    assert "max_lines" in L.pysdr_last_error().decode()
    assert L.pysdr_rtty_decode(*args(-1)) == -1
    assert L.pysdr_rtty_decode(*args(10, None)) == -1
    assert "NULL" in L.pysdr_last_error().decode()
    assert L.pysdr_rtty_decode(*args(64)) == 0 and nd.value == 2
    with pytest.raises(_lib.PysdrError, match="pysdr_rtty_create"):
        rtty.RTTY_Decoders(48000, bins=[2040, 2041])
    with pytest.raises(_lib.PysdrError, match="pysdr_rtty_create"):
        rtty.RTTY_Decoders(48000, find_bins=(1900, 2050))
    # lines that are not finite do not fault, and emit nothing where snr2 is not finite
    bad = np.full((64, 2048), np.nan, np.float32)
    bad[::3] = np.inf
    r = dec.decode_raw(bad, 64, False, True)
    assert (r["codes"] == -1).all()
    dec.close()
