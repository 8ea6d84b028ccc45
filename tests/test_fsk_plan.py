"""The RTTY raster skimmer's plan (pysdr_fsk_plan, include/pysdr_hip.h; pysdr_amd/csrc/fsk_plan.h): what it refuses, the
event cap, the event word -- through the library, which needs no device for this -- the shape a fine channelizer takes
at 8 MS/s, and the tile walk, the LDS layout, both step functions and the event slots in a stand-alone C++ program
(tests/fsk_plan/plan_main.cpp) built and run by tests/plan_program.py, under AddressSanitizer + UBSan where they are usable.
CPU only; nothing that is loaded into Python runs under a sanitizer."""
import ctypes as C

import pytest

from tests import plan_program


def good():
    from pysdr_amd import fsk
    return fsk.params()


def call(lib, nk, S, max_out, cfg):
    out = (C.c_int32 * 8)(*([-7] * 8))
    rc = lib.pysdr_fsk_plan(nk, S, max_out, None if cfg is None else C.byref(cfg), out)
    return rc, list(out)


def test_plan_of_good_shapes(hiplib):
    from pysdr_amd import fsk
    from tests import fsk_oracle as fo
    cfg = good()
    for S, rows, threads, lds in ((22, 8, 192, 6936), (33, 7, 256, 7620)):
        for nk in (1, 2, 7, 8, 9, 15, 128, 512, (1 << 18) // S):
            for mo in (1, 143, 144, 145, 215, 216, 217, 63, 64, 65, 256, 1 << 20):
                rc, v = call(hiplib, nk, S, mo, cfg)
                assert rc == 0, (nk, S, mo, hiplib.pysdr_last_error())
                cap = mo // (6 * S + S // 2 + 1) + 1
                assert v == [rows, threads, lds, 64, cap, -(-nk // rows), S, 0]
                assert cap == fo.cap_of(mo, S)
                assert fsk.plan(nk, S, mo, cfg) == dict(rows=rows, threads=threads, lds_bytes=lds, tile=64, cap=cap, groups=-(-nk // rows), nsub=S)
    assert C.sizeof(fsk.FskCfg) == 28
    assert fsk.cfg_dict(cfg) == {k: (float(v) if k != "n0" else v) for k, v in fo.params().items()}


def test_plan_refuses_bad_shapes_and_settings(hiplib):
    from pysdr_amd import _lib, fsk
    cfg = good()
    assert hiplib.pysdr_fsk_plan(4, 22, 16, C.byref(cfg), None) == -1
    for nk, S, mo in ((0, 22, 16), (-1, 22, 16), (11916, 22, 16), (7944, 33, 16), (4, 22, 0), (4, 22, -1), (4, 22, (1 << 20) + 1),
                      (4, 0, 16), (4, 8, 16), (4, 12, 16), (4, 11, 16), (4, 44, 16), (4, -22, 16)):
        rc, v = call(hiplib, nk, S, mo, cfg)
        assert rc == -1 and v == [-7] * 8, (nk, S, mo)
        assert b"pysdr_fsk_plan" in hiplib.pysdr_last_error()
    assert call(hiplib, 4, 22, 16, None)[0] == -1
    bad = []
    for k in ("a_q", "a_b", "hi", "lo", "bal", "pmax"):
        bad += [(k, 0.0), (k, -0.5), (k, float("nan")), (k, float("inf")), (k, float("-inf"))]
    bad += [("a_q", 1.0000001), ("a_b", 2.0), ("lo", 0.85), ("hi", 1.5), ("bal", 1.0000001), ("pmax", 1.1e18), ("n0", 0), ("n0", -1),
            ("n0", (1 << 22) + 1)]
    for k, v in bad:
        c = good()
        setattr(c, k, v)
        assert call(hiplib, 4, 22, 16, c)[0] == -1, (k, v)
        with pytest.raises(_lib.PysdrError):
            fsk.plan(4, 22, 16, c)
    for k, v in (("a_q", 1.0), ("a_b", 1.0), ("n0", 1), ("n0", 1 << 22), ("lo", 0.8), ("hi", 1.0), ("bal", 1.0), ("pmax", 1e18)):
        c = good()
        setattr(c, k, v)
        assert call(hiplib, 4, 22, 16, c)[0] == 0, (k, v)
    # the handle-taking calls check their arguments before any device work
    h, n = C.c_void_p(), C.c_int(-1)
    tw, g = fsk.tables(22)
    assert hiplib.pysdr_fsk_create(None, 22, C.byref(cfg), _lib.as_pf(tw), _lib.as_pf(g), 16, C.byref(h)) == -1 and not h.value
    assert hiplib.pysdr_fsk_create(None, 22, C.byref(cfg), _lib.as_pf(tw), _lib.as_pf(g), 16, None) == -1
    assert hiplib.pysdr_fsk_process(None, None, 0, 0, C.byref(n), None, None, 0, None, None) == -1
    assert hiplib.pysdr_fsk_reset(None) == -1 and hiplib.pysdr_fsk_sync(None) == -1
    assert hiplib.pysdr_fsk_fetch(None, None, 0, None, 0) == -1 and hiplib.pysdr_fsk_state(None, None, None) == -1
    hiplib.pysdr_fsk_destroy(None)


def test_a_fine_channelizer_for_8_ms_per_second_has_the_shape_fine_plan_h_gives(hiplib):
    """fs = 8 MS/s, where fsk.shape finds no single stage (M = 32000 is beyond a channelizer): rows at 22 samples per bit
    need D1 D2 = 8000, and among M1 = 2 D1, M2 = 4 D2 >= 32 the largest valid M1 is 2000"""
    from pysdr_amd import fine, fsk
    fs = 8e6
    with pytest.raises(ValueError):
        fsk.shape(fs)
    M1, D1, M2, D2 = fine.shape(fs, 22 * fsk.BAUD, 4)
    assert (M1, D1, M2, D2) == (2000, 1000, 32, 8)
    band = (100e3, 100e3 + 7 * 250.0)
    g_first, ng = fine.channels_for(band, fs, M1, D1, M2)
    p = fine.plan(M1, D1, M2, D2, len(fine.prototype1(fs, M1, D1, M2)), len(fsk.prototype(fs / D1, M2, 22)), g_first, ng)
    assert (p["Q"], p["Mf"], p["D"], ng) == (16, 32000, 8000, 8) and fs / p["Mf"] == 250.0 and fs / p["D"] == 22 * fsk.BAUD
    assert fsk.plan(ng, 22, 256, fsk.params())["groups"] == 1


def test_tiles_cover_every_sample_once_the_steps_equal_the_transcription_and_the_slots_hold_the_cap(tmp_path):
    """the tile walk, both tones against the definition, the step against a plain transcription, the cap proof"""
    plan_program.run("tests/fsk_plan/plan_main.cpp", "FSK_PLAN_OK", tmp_path, extra_flags=("-ffp-contract=off",))
