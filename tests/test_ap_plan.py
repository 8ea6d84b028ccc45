"""The pure half of a-priori decoding (pysdr_amd/csrc/ap_plan.h): pysdr_ap_plan through the library,
which needs no device for it, the argument checks of the four new decode calls that come before any device work, and the
stand-alone C++ program tests/ap_plan/plan_main.cpp, built and run by tests/plan_program.py under AddressSanitizer + UBSan
where they are usable: every refusal of the settings, a hypothesis table and a pair list, first[], the clamp, nerr / nap
and the pick, and the scalar transcription on a case this test writes to a file, compared with the NumPy oracle
(tests/ap_oracle.py) for equality.  CPU only; nothing that is loaded into Python runs under a sanitizer."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import ap_oracle as ao
from tests import plan_program

F32 = np.float32


def call(lib, cfg):
    out = (C.c_int32 * 4)(*([-7] * 4))
    rc = lib.pysdr_ap_plan(None if cfg is None else C.byref(cfg), out)
    return rc, list(out)


def test_plan_and_its_refusals(hiplib):
    from pysdr_amd import _lib, ap
    assert C.sizeof(_lib.ApCfg) == 8 and ap.params().mag == 1.0 and ap.params().nerr_max == ap.NERR_MAX == 174
    assert call(hiplib, ap.params()) == (0, [192, 4380, 65536, 4096])
    assert ap.plan(ap.params(0.25, 0)) == dict(threads=192, lds_bytes=4380, max_pairs=65536, max_hyps=4096)
    assert ap.plan(ap.params(16.0, 174))["threads"] == 192
    assert hiplib.pysdr_ap_plan(C.byref(ap.params()), None) == -1
    assert call(hiplib, None) == (-1, [-7] * 4)
    for mag, nerr_max in ((0.2, 174), (16.5, 174), (0.0, 174), (-1.0, 174), (float("nan"), 174), (float("inf"), 174), (1.0, -1), (1.0, 175)):
        assert call(hiplib, ap.params(mag, nerr_max)) == (-1, [-7] * 4), (mag, nerr_max)
        assert b"pysdr_ap_plan" in hiplib.pysdr_last_error()
        with pytest.raises(_lib.PysdrError):
            ap.plan(ap.params(mag, nerr_max))
    with pytest.raises(_lib.PysdrError):
        ap.plan(None)


def test_the_new_decode_calls_refuse_a_null_skimmer_before_any_device_work(hiplib):
    from pysdr_amd import ap, ldpc
    cfg, apc = ldpc.params(), ap.params()
    for kind in ("ft8", "ft4"):
        assert getattr(hiplib, f"pysdr_{kind}_decode_ap")(None, None, None, 0, None, 1, None, 0, C.byref(cfg), C.byref(apc), None, None, None) == -1
        assert f"pysdr_{kind}_decode_ap".encode() in hiplib.pysdr_last_error()
        assert getattr(hiplib, f"pysdr_{kind}_decode_llr_ap")(None, None, 0, None, 1, None, 0, C.byref(cfg), C.byref(apc), None, None, None) == -1
        assert f"pysdr_{kind}_decode_llr_ap".encode() in hiplib.pysdr_last_error()


def test_the_skimmer_refuses_ap_without_decode_or_with_report_or_a_second_pass_without_a_device():
    from pysdr_amd import _lib, ap
    kw = dict(channels=(3, 3), ap=ap.params())
    with pytest.raises(ValueError, match="decode=True"):
        ap.FT8_AP_Skimmer(8000.0, **kw)
    with pytest.raises(ValueError, match="report=True or passes=2"):
        ap.FT8_AP_Skimmer(8000.0, decode=True, report=True, **kw)
    with pytest.raises(ValueError, match="report=True or passes=2"):
        ap.FT8_AP_Skimmer(8000.0, decode=True, passes=2, **kw)
    with pytest.raises(_lib.PysdrError):
        ap.FT8_AP_Skimmer(8000.0, decode=True, channels=(3, 3), ap=ap.params(mag=0.1))


@functools.lru_cache(maxsize=None)
def case():
    """(llr float32 [n][174], hyps, pairs): clean, noisy and weak words of three messages, noise, zeros and -0, a coarse grid
    with ties; right, wrong and full hypotheses, a candidate with every hypothesis and candidates with none"""
    from pysdr_amd import ap, ft8msg, ldpc
    rng = np.random.default_rng(28)
    texts = ("CQ K1ABC FN42", "K1ABC W9XYZ -12", "W9XYZ K1ABC RR73")
    hyps = [ap.hyp_cq(), ap.hyp_from("K1ABC"), ap.hyp_pair("K1ABC", "W9XYZ"), ap.hyp_cq_from("K1ABC"), ap.hyp_text(texts[2]),
            ap.hyp_from("W9XYZ"), ap.hyp_pair("W9XYZ", "K1ABC"), ap.hyp_text("CQ DL1ABC JO62"),
            ao.hyp(np.eye(77, dtype=np.uint8)[76], np.ones(77, np.uint8)), ao.hyp(np.eye(77, dtype=np.uint8)[0], np.zeros(77, np.uint8))]
    llr = []
    for sigma in (0.0, 0.6, 0.9, 1.1, 1.3, 1.5):
        for t in texts:
            llr.append((2.0 * ldpc.encode(ft8msg.pack77(t)) - 1) + sigma * rng.standard_normal(174))
    llr += [rng.standard_normal(174) for _ in range(3)]
    llr += [np.zeros(174), -np.zeros(174), np.round(2 * ((2.0 * ldpc.encode(ft8msg.pack77(texts[0])) - 1) + 1.2 * rng.standard_normal(174))) / 2]
    llr.append(2.4e17 * ((2.0 * ldpc.encode(ft8msg.pack77(texts[1])) - 1) + 1.2 * rng.standard_normal(174)))
    llr = np.array(llr).astype(F32)
    pairs = []
    for c in range(len(llr)):
        if c % 5 == 4:
            continue                                                            # a candidate without pairs
        pairs += [(c, h) for h in range(len(hyps)) if c % 7 == 0 or (h + c) % 3 != 1]
    return llr, hyps, np.array(pairs, np.int32)


@pytest.mark.parametrize("iters,mag,nerr_max", ((30, 1.0, 174), (1, 0.25, 174), (30, 4.0, 12)))
def test_the_scalar_transcription_and_the_pick_equal_the_oracle(tmp_path, monkeypatch, iters, mag, nerr_max):
    from pysdr_amd import ap
    llr, hyps, pairs = case()
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        np.array([len(llr), len(hyps), len(pairs), iters, nerr_max], np.int32).tofile(f)
        np.array([mag, 0.8125], F32).tofile(f)
        llr.tofile(f)
        ap.table(hyps).tofile(f)
        pairs.tofile(f)
    monkeypatch.setenv("AP_PLAN_CASE", str(path))
    out = plan_program.run("tests/ap_plan/plan_main.cpp", "AP_PLAN_OK", tmp_path, extra_flags=("-ffp-contract=off",), includes=("pysdr_amd/csrc",))
    assert f"AP_PLAN_OK {len(llr)} candidates, {len(hyps)} hypotheses, {len(pairs)} pairs, lds 4380 bytes" in out
    want_ap, want_bits, want_detail, want_pbits = ao.decode(llr, hyps, pairs, mag=mag, nerr_max=nerr_max, iters=iters)
    got_p, got_c = {}, {}
    for line in out.splitlines():
        f = line.split()
        if f and f[0] == "PAIR":
            got_p[int(f[1])] = ([int(v) for v in f[2:6]], f[6])
        elif f and f[0] == "CAND":
            got_c[int(f[1])] = ([int(v) for v in f[2:6]], f[6])
    assert len(got_p) == len(pairs) and len(got_c) == len(llr)
    for p in range(len(pairs)):
        assert got_p[p] == ([int(v) for v in want_detail[p]], want_pbits[p].tobytes().hex()), (p, pairs[p], got_p[p], want_detail[p])
    for c in range(len(llr)):
        assert got_c[c] == ([int(v) for v in want_ap[c]], want_bits[c].tobytes().hex()), (c, got_c[c], want_ap[c])
    if (iters, mag, nerr_max) == (30, 1.0, 174):                               # the case is a mixture
        assert set(want_detail[:, 0]) == {0, 1, 2} and (want_ap[:, 0] == -1).any() and (want_ap[:, 3] > 1).any() and (want_detail[:, 3] > 0).any()
    print(f"iters {iters} mag {mag} nerr_max {nerr_max}: {len(pairs)} pairs, status 2 in {(want_detail[:, 0] == 2).sum()}, picked {(want_ap[:, 0] >= 0).sum()} of {len(llr)}")
