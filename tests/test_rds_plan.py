"""The RDS skimmer's plan (pysdr_rds_plan, include/pysdr_hip.h; pysdr_amd/csrc/rds_plan.h): what it refuses, the event cap,
the struct -- through the library, which needs no device for this -- and the chip grid, the tile walk, every step against
a plain transcription of the definition, the cap and the code's constants in a stand-alone C++ program
(tests/rds_plan/plan_main.cpp) built and run by tests/plan_program.py, under AddressSanitizer + UBSan where they are usable.
CPU only; nothing that is loaded into Python runs under a sanitizer."""
import ctypes as C

import pytest

from tests import plan_program

EDGES = ((228000.0, 385, 7), (400000.0, 673, 11), (512000.0, 863, 14))


def good(fs_out=400000.0):
    from pysdr_amd import rds
    return rds.params(fs_out)


def call(lib, nk, L, max_out, cfg):
    out = (C.c_int32 * 8)(*([-7] * 8))
    rc = lib.pysdr_rds_plan(nk, L, max_out, None if cfg is None else C.byref(cfg), out)
    return rc, list(out)


def test_plan_of_good_shapes(hiplib):
    from pysdr_amd import rds
    from tests import rds_oracle as ro
    for fs_out, L, nseg in EDGES:
        cfg = good(fs_out)
        assert rds.pulse_length(fs_out) == L == ro.tables(fs_out)[0] and cfg.w19 == ro.word19(fs_out)
        for nk in (1, 2, 3, 16, 100, 1 << 14):
            for mo in (1, 11, 12, 13, 256, 1024, 4096, 65536, 1 << 20):
                rc, v = call(hiplib, nk, L, mo, cfg)
                assert rc == 0, (nk, L, mo, hiplib.pysdr_last_error())
                cap = 3 * -(-((mo * cfg.w19 >> 32) + 1) // 16)
                assert v == [2, 256, 53708, 1024, cap, -(-nk // 2), 16, nseg]
                assert cap == ro.cap_of(mo, cfg.w19)
                assert rds.plan(nk, L, mo, cfg) == dict(rows=2, threads=256, lds_bytes=53708, tile=1024, cap=cap, groups=-(-nk // 2),
                                                        phases=16, segments=nseg)
    assert C.sizeof(rds.RdsCfg) == 4
    assert 2 * 53708 <= 160 * 1024                                          # two workgroups on a CU's LDS
    assert ro.cap_of(256, good(228000.0).w19) == 6 and ro.cap_of(65536, good().w19) == 585


def test_plan_refuses_bad_shapes_and_settings(hiplib):
    from pysdr_amd import _lib, rds
    cfg = good()
    assert hiplib.pysdr_rds_plan(4, 673, 16, C.byref(cfg), None) == -1
    for nk, L, mo in ((0, 673, 16), (-1, 673, 16), ((1 << 14) + 1, 673, 16), (4, 673, 0), (4, 673, -1), (4, 673, (1 << 20) + 1),
                      (4, 671, 16), (4, 675, 16), (4, 672, 16), (4, 0, 16), (4, -673, 16), (4, 385, 16), (4, 863, 16)):
        rc, v = call(hiplib, nk, L, mo, cfg)
        assert rc == -1 and v == [-7] * 8, (nk, L, mo)
        assert b"pysdr_rds_plan" in hiplib.pysdr_last_error()
    assert call(hiplib, 4, 673, 16, None)[0] == -1
    assert call(hiplib, 1 << 14, 673, 1 << 20, cfg)[0] == 0
    for fs_out, L in ((227000.0, 383), (513000.0, 865), (200000.0, 337), (600000.0, 1011)):   # the rows' rates just outside, and far
        bad = rds.params(fs_out)
        assert call(hiplib, 4, L, 16, bad)[0] == -1 and call(hiplib, 4, 385, 16, bad)[0] == -1 and call(hiplib, 4, 863, 16, bad)[0] == -1
        with pytest.raises(_lib.PysdrError):
            rds.plan(4, L, 16, bad)
    assert call(hiplib, 4, 385, 16, rds.RdsCfg(w19=0))[0] == -1
    # the handle-taking calls check their arguments before any device work
    h, n = C.c_void_p(), C.c_int(-1)
    L, tw, g = rds.tables(400000.0)
    assert hiplib.pysdr_rds_create(None, L, C.byref(cfg), _lib.as_pf(tw), _lib.as_pf(g), 16, C.byref(h)) == -1 and not h.value
    assert hiplib.pysdr_rds_create(None, L, C.byref(cfg), _lib.as_pf(tw), _lib.as_pf(g), 16, None) == -1
    assert hiplib.pysdr_rds_process(None, None, 0, 0, C.byref(n), None, None, 0) == -1
    assert hiplib.pysdr_rds_reset(None) == -1 and hiplib.pysdr_rds_sync(None) == -1
    assert hiplib.pysdr_rds_fetch(None, None, 0, None, 0) == -1 and hiplib.pysdr_rds_state(None, None, None, None) == -1
    hiplib.pysdr_rds_destroy(None)


def test_the_skimmer_refuses_rows_outside_its_rates_before_it_needs_a_device():
    from pysdr_amd import rds
    with pytest.raises(ValueError):
        rds.RDS_Skimmer(1600000.0, 16, 8)                                   # rows at 200 kHz
    with pytest.raises(ValueError):
        rds.RDS_Skimmer(2400000.0, 16, 4)                                   # rows at 600 kHz
    with pytest.raises(ValueError):
        rds.RDS_Skimmer(100000.0)                                           # no 100 kHz raster with four rows' overlap


def test_chips_tiles_steps_cap_and_constants(tmp_path):
    """the chip grid's closed form, the tile walk, every step against a plain transcription of the definition, the slots
    at the cap, and the constants' cross-check"""
    plan_program.run("tests/rds_plan/plan_main.cpp", "RDS_PLAN_OK", tmp_path, extra_flags=("-ffp-contract=off",))
