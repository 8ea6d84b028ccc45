"""The RTTY decoder bank on the CPU: the restatement (tests/rtty_decoder_oracle.py) against the executed reference
(tests/golden/rtty_decoder_ref.npz, made by tests/golden/make_rtty_decoder_ref_golden.py), the product's Baudot
tables, and the product's refusal to run without a GPU."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests import rtty_decoder_oracle as rdo

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_SCORE, TOL_SNR = 1e-2, 1e-6


def load_fixture():
    g = np.load(os.path.join(HERE, "golden", "rtty_decoder_ref.npz"))
    f = {k: g[k] for k in g.files}
    lo = int(f["band_lo"])
    lines = np.zeros((len(f["band"]), 2048), np.float32)
    lines[:, lo:lo + f["band"].shape[1]] = f["band"].astype(np.float32) / 256.0      # exact: the values decoded
    f["lines"] = lines
    f["events"] = list(zip(f["ev_n"].tolist(), f["ev_bin"].tolist(), json.loads(str(f["ev_text"]))))
    f["horizon"] = rdo.horizon(f["m_isym"], f["m_sc2"], f["m_snr"], TOL_SCORE, TOL_SNR)
    f["signals"] = json.loads(str(f["signals"]))
    return f


def compare_with_fixture(f, codes, t, ndet, events):
    """The margin rule: decoder k is compared over its first horizon[k] decisions; ndet exactly."""
    bins = f["bins"].astype(np.int64)
    hz = f["horizon"]
    nd = f["codes"].shape[0]
    assert codes.shape == f["codes"].shape == t.shape
    assert np.array_equal(ndet, f["ndet"])
    for k in range(len(bins)):
        h = hz[k]
        assert np.array_equal(codes[:h, k], f["codes"][:h, k]), (bins[k], h)
        assert np.array_equal(t[:h, k], f["t"][:h, k]), (bins[k], h)
    lim = {int(b): 30 * (int(h) + 1) for b, h in zip(bins, hz)}      # decisions j < h are the lines n <= 30 h
    keep = lambda ev: [e for e in ev if e[0] <= lim[e[1]] - 30]
    assert keep(events) == keep(f["events"])
    # what the margin rule leaves out must stay small, and every transmitted signal compares in full
    assert hz.sum() >= 0.8 * nd * len(bins)
    for b, _ in f["signals"]:
        assert hz[b - bins[0]] == nd


def compare_exactly(f, codes, t, events, isym_sel):
    """On the fixture's quantised lines every score, sc2 and snr2 is exact in any order of addition, so a correct
    decoder equals the executed reference everywhere -- exact ties included, which go to the lowest index."""
    assert np.array_equal(codes, f["codes"]) and np.array_equal(t, f["t"])
    assert events == f["events"]
    assert np.array_equal(isym_sel, f["sel_isym"])
    assert (f["sel_gap"] == 0).any() and (f["m_sc2"] == 0).any()      # the fixture holds exact ties of both kinds


def events_from_codes(n, codes, bins):
    ev = []
    for j, k in zip(*np.nonzero(codes >= 0)):
        ev.append((int(n[j]), int(bins[k]), rdo.code_text(int(codes[j, k]))))
    return ev


def test_fixture_holds_the_band_signals_and_figs_traffic():
    f = load_fixture()
    assert f["band"].dtype == np.int16 and int(f["band_lo"]) == 800 and f["band"].shape[1] == 450
    assert list(f["bins"]) == list(range(800, 1243))
    assert len(f["signals"]) >= 4
    assert any(c >= 32 for c in f["codes"][:, 1002 - 800]), "FIGS traffic"
    assert os.path.getsize(os.path.join(HERE, "golden", "rtty_decoder_ref.npz")) < 1 << 20
    for b, text in f["signals"]:                   # the reference reads the transmitted text at the mark bins
        got = "".join(c for n, bb, c in f["events"] if bb == b)
        assert text[:8] in got or text[-8:] in got, (b, got)


def test_restatement_reproduces_the_executed_reference():
    f = load_fixture()
    bank = rdo.DecoderBank(800, 1243, 800, 1243)
    parts = [bank.decode(c) for c in np.split(f["lines"], [1, 47, 300, 301, 630])]     # cuts are free
    cat = lambda k: np.concatenate([p[k] for p in parts])
    codes, t, n = cat("codes"), cat("t"), cat("n")
    assert list(n) == list(range(30, 901, 30))
    compare_with_fixture(f, codes, t, cat("ndet"), events_from_codes(n, codes, f["bins"]))
    isym, best = cat("isym"), cat("best")
    sel = f["sel"].astype(np.int64) - 800
    ok = f["sel_gap"] >= TOL_SCORE
    assert ok.mean() > 0.9
    assert np.array_equal(isym[:, sel][ok], f["sel_isym"][ok])
    assert np.array_equal(best[:, sel], f["sel_best"])           # quantised lines: every score is exact in float32
    compare_exactly(f, codes, t, events_from_codes(n, codes, f["bins"]), isym[:, sel])


def test_product_baudot_tables_equal_the_recorded_ones():
    from pysdr_amd import rtty
    f = load_fixture()
    ltrs, figs = json.loads(str(f["ltrs"])), json.loads(str(f["figs"]))
    assert rtty.LTRS == ltrs == rdo.LTRS and rtty.FIGS == figs == rdo.FIGS
    assert figs[5] == "\\g" and ltrs[2] == "\n" and ltrs[8] == "\r"
    assert [rtty.code_text(c) for c in (1, 33, 37, 2, 40)] == ["E", "3", "\\g", "\n", "\r"]


def test_decoder_classes_refuse_without_a_gpu(monkeypatch):
    from pysdr_amd import _lib, rtty
    monkeypatch.setattr(_lib, "device_count", lambda: 0)
    with pytest.raises(_lib.PysdrError):
        rtty.RTTY_Decoders(48000)
    with pytest.raises(_lib.PysdrError):
        rtty.RTTY_Skimmer(48000)


def test_create_refuses_bad_ranges_before_any_device_work(hiplib):
    """Argument checks come before hipSetDevice: PYSDR_ERR_ARG with a text, GPU or not."""
    h = ctypes.c_void_p()
    for args in ((0, 2048, 7, 0, 2042, 800, 1243, 64), (0, 2048, 7, -1, 10, 800, 1243, 64),
                 (0, 2048, 7, 10, 10, 800, 1243, 64), (0, 2048, 7, 0, 100, 900, 800, 64),
                 (0, 2048, 7, 0, 100, 800, 2042, 64), (0, 2048, 7, 0, 100, 800, 1243, 0)):
        assert hiplib.pysdr_rtty_create(*args, ctypes.byref(h)) == -1, args
        assert hiplib.pysdr_last_error().decode().startswith("pysdr_rtty_create"), args
    assert hiplib.pysdr_rtty_create(0, 2048, 7, 0, 100, 800, 1243, 64, None) == -1
    assert hiplib.pysdr_rtty_decode(None, None, 0, 0, 1, None, None, None, None, None, None, None) == -1
    assert hiplib.pysdr_rtty_reset(None) == -1
    hiplib.pysdr_rtty_destroy(None)
