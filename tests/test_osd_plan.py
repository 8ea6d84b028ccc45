"""The pure half of ordered-statistics decoding (pysdr_amd/csrc/osd_plan.h): pysdr_osd_plan through the
library, which needs no device for it, the argument checks of the four new decode calls, and the scalar transcription in a
stand-alone C++ program (tests/osd_plan/plan_main.cpp) built and run by tests/plan_program.py, under AddressSanitizer +
UBSan where they are usable, on words this test writes to a file -- clean, noisy, noise, zeros and ties -- and whose
status, bits and detail it compares with the NumPy oracle (tests/osd_oracle.py) for equality.  CPU only; nothing that is
loaded into Python runs under a sanitizer."""
import ctypes as C

import numpy as np
import pytest

from tests import osd_oracle as oo
from tests import plan_program

F32 = np.float32


def call(lib, cfg):
    out = (C.c_int32 * 4)(*([-7] * 4))
    rc = lib.pysdr_osd_plan(None if cfg is None else C.byref(cfg), out)
    return rc, list(out)


def test_plan_and_its_refusals(hiplib):
    from pysdr_amd import _lib, ldpc
    assert C.sizeof(_lib.LdpcCfg) == 8 and C.sizeof(_lib.OsdCfg) == 4 and ldpc.osd_params().order == 2
    assert ldpc.OSD_PATTERNS == (1, 92, 4187) == oo.PATTERNS
    for order in (0, 1, 2):
        assert call(hiplib, ldpc.osd_params(order)) == (0, [64, 4502, ldpc.OSD_PATTERNS[order], 4096])
        assert ldpc.osd_plan(ldpc.osd_params(order)) == dict(threads=64, lds_bytes=4502, patterns=ldpc.OSD_PATTERNS[order], max_candidates=4096)
    assert hiplib.pysdr_osd_plan(C.byref(ldpc.osd_params()), None) == -1
    assert call(hiplib, None) == (-1, [-7] * 4)
    for order in (-1, 3):
        assert call(hiplib, ldpc.osd_params(order)) == (-1, [-7] * 4), order
        assert b"pysdr_osd_plan" in hiplib.pysdr_last_error()
        with pytest.raises(_lib.PysdrError):
            ldpc.osd_plan(ldpc.osd_params(order))
    with pytest.raises(_lib.PysdrError):
        ldpc.osd_plan(None)
    # what the Python layer takes for ``osd``
    assert ldpc.osd_cfg(None) is None and ldpc.osd_cfg(1).order == 1 and ldpc.osd_cfg(np.int64(2)).order == 2
    cfg = ldpc.osd_params(0)
    assert ldpc.osd_cfg(cfg) is cfg
    for bad in (True, 2.0, "2"):
        with pytest.raises(ValueError):
            ldpc.osd_cfg(bad)


def test_the_new_decode_calls_refuse_a_null_skimmer_before_any_device_work(hiplib):
    from pysdr_amd import ldpc
    cfg, osd = ldpc.params(), ldpc.osd_params()
    for kind in ("ft8", "ft4"):
        assert getattr(hiplib, f"pysdr_{kind}_decode_osd")(None, None, None, 0, C.byref(cfg), None, None, None, C.byref(osd), None) == -1
        assert f"pysdr_{kind}_decode_osd".encode() in hiplib.pysdr_last_error()
        assert getattr(hiplib, f"pysdr_{kind}_decode_llr_osd")(None, None, 0, C.byref(cfg), None, None, None, C.byref(osd), None) == -1
        assert f"pysdr_{kind}_decode_llr_osd".encode() in hiplib.pysdr_last_error()


def test_osd_without_decode_is_refused_without_a_device():
    from pysdr_amd.ft4 import FT4_Skimmer
    from pysdr_amd.ft8 import FT8_Skimmer
    for cls in (FT8_Skimmer, FT4_Skimmer):
        with pytest.raises(ValueError, match="decode=True"):
            cls(8000.0 if cls is FT8_Skimmer else 12000.0, channels=(3, 3), osd=2)


def words():
    """clean, noisy, noise, zeros and ties: float32 [n][174]"""
    from pysdr_amd import ldpc
    rng = np.random.default_rng(25)
    out = []
    for sigma in (0.0, 0.7, 0.8, 0.8, 0.8, 0.8, 0.8, 0.9, 0.9, 0.9, 0.9, 0.9, 1.0, 1.0, 1.1):
        for _ in range(2):
            cw = ldpc.encode(rng.integers(0, 2, 77))
            out.append((2.0 * cw - 1) + sigma * rng.standard_normal(174))
    out += [rng.standard_normal(174) for _ in range(6)]                         # noise
    out += [1e18 * rng.uniform(-1, 1, 174), 2.4e17 * ((2.0 * ldpc.encode(rng.integers(0, 2, 77)) - 1) + rng.standard_normal(174))]
    out.append(np.zeros(174))
    out.append(-np.zeros(174))                                                  # -0 everywhere
    cw = ldpc.encode(rng.integers(0, 2, 77))
    flip = 2.0 * cw - 1
    flip[rng.choice(174, 30, replace=False)] *= -1
    out.append(flip)                                                            # +-1 only: ranks are positions
    out.append(np.where(rng.integers(0, 2, 174) > 0, 1.0, -1.0))                # +-1 noise
    out.append(np.round(4 * ((2.0 * cw - 1) + rng.standard_normal(174))) / 4)   # a coarse grid: many ties in r and in distance
    out.append(np.round((2.0 * cw - 1) + 1.1 * rng.standard_normal(174)))       # with zeros among them
    return np.array(out).astype(F32)


def test_the_scalar_transcription_equals_the_oracle(tmp_path, monkeypatch):
    x = words()
    path = tmp_path / "words.f32"
    x.tofile(path)
    monkeypatch.setenv("OSD_PLAN_WORDS", str(path))
    out = plan_program.run("tests/osd_plan/plan_main.cpp", "OSD_PLAN_OK", tmp_path, extra_flags=("-ffp-contract=off",),
                           includes=("pysdr_amd/csrc",))
    assert f"OSD_PLAN_OK {len(x)} words, 4187 patterns" in out
    got = {}
    for line in out.splitlines():
        if line.startswith("WORD "):
            f = line.split()
            got[(int(f[1]), int(f[2]))] = ([int(v) for v in f[3:7]], f[7], [int(v) for v in f[8:12]])
    assert len(got) == 3 * len(x)
    ran = accepted = 0
    for order in (0, 1, 2):
        st, bits, _, detail = oo.decode(x, order=order)
        for i in range(len(x)):
            want = ([int(v) for v in st[i]], bits[i].tobytes().hex(), [int(v) for v in detail[i]])
            assert got[(i, order)] == want, (i, order, got[(i, order)], want)
        ran += int((st[:, 3] > 0).sum())
        accepted += int(((st[:, 3] > 0) & (st[:, 0] == 2)).sum())
        if order == 2:
            assert set(st[:, 3]) == {0, 1, 2, 3}, sorted(set(st[:, 3]))
    print(f"{len(x)} words, three orders: the second stage ran {ran} times and gave {accepted} messages")
    assert ran > 30 and accepted >= 3
