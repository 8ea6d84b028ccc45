"""The ACARS skimmer's plan (pysdr_acars_plan, include/pysdr_hip.h; pysdr_amd/csrc/acars_plan.h): what it refuses, the
event cap, the struct -- through the library, which needs no device for this -- and the tile walk, all phases against a
plain transcription of the definition, the cap's proof, the frame machine and the event words in a stand-alone C++ program
(tests/acars_plan/plan_main.cpp) built and run by tests/plan_program.py, under AddressSanitizer + UBSan where they are
usable.  CPU only; nothing that is loaded into Python runs under a sanitizer."""
import ctypes as C

import pytest

from tests import plan_program

LDS = 1024 * 8 + 85 * 8 + 8 * 169 * 4 + 8 * 85 * 8 + 8 * 65 * 4


def good(fs_out=25000.0):
    from pysdr_amd import acars
    return acars.params(fs_out)


def call(lib, nk, L, max_out, cfg):
    out = (C.c_int32 * 8)(*([-7] * 8))
    rc = lib.pysdr_acars_plan(nk, L, max_out, None if cfg is None else C.byref(cfg), out)
    return rc, list(out)


def test_plan_of_good_shapes(hiplib):
    from pysdr_amd import acars
    from tests import acars_oracle as ao
    for fs_out, L_want in ((19200.0, 8), (20000.0, 8), (25000.0, 10), (48000.0, 20), (50000.0, 21)):
        cfg = good(fs_out)
        L = acars.window_length(fs_out)
        assert L == L_want == ao.tables(fs_out)[0]
        gap = 2 ** 31 // cfg.w_baud + 1
        for nk in (1, 7, 8, 9, 400):
            for mo in (1, 16, gap, gap + 1, 24 * gap, 24 * gap + 1, 256, 4096, 1 << 20):
                rc, v = call(hiplib, nk, L, mo, cfg)
                assert rc == 0, (nk, L, mo, hiplib.pysdr_last_error())
                cap = 61 + (-(-mo // gap) - 1) // 24
                assert v == [8, 256, LDS, 64, cap, -(-nk // 8), 4 * L + 1, 60]
                assert cap == ao.cap_of(mo, cfg.w_baud)
                assert acars.plan(nk, L, mo, cfg) == dict(rows=8, threads=256, lds_bytes=LDS, tile=64, cap=cap, groups=-(-nk // 8),
                                                          taps=4 * L + 1, frame_words=60)
    assert C.sizeof(acars.AcarsCfg) == 16 and LDS < 64 * 1024
    assert ao.cap_of(4096, good().w_baud) == 89 and ao.cap_of(16, good().w_baud) == 61


def test_plan_refuses_bad_shapes_and_settings(hiplib):
    from pysdr_amd import _lib, acars
    cfg = good()
    assert hiplib.pysdr_acars_plan(4, 10, 16, C.byref(cfg), None) == -1
    for nk, L, mo in ((0, 10, 16), (-1, 10, 16), ((1 << 15) + 1, 10, 16), (4, 10, 0), (4, 10, -1), (4, 10, (1 << 20) + 1),
                      (4, 7, 16), (4, 22, 16), (4, 0, 16), (4, -10, 16)):
        rc, v = call(hiplib, nk, L, mo, cfg)
        assert rc == -1 and v == [-7] * 8, (nk, L, mo)
        assert b"pysdr_acars_plan" in hiplib.pysdr_last_error()
    assert call(hiplib, 4, 10, 16, None)[0] == -1
    assert call(hiplib, 4, 8, 16, cfg)[0] == 0 and call(hiplib, 4, 21, 16, cfg)[0] == 0 and call(hiplib, 1 << 15, 10, 1 << 20, cfg)[0] == 0

    def changed(k, v):
        c = good()
        setattr(c, k, v)
        return c

    bad = [changed("pmax", v) for v in (0.0, -0.5, float("nan"), float("inf"), float("-inf"), 1.1e18)]
    bad += [changed("pll_shift", v) for v in (0, 5, -1)] + [changed(k, 0) for k in ("w_car", "w_baud")]
    bad += [changed("w_baud", (1 << 29) + 1)]
    for c in bad:
        assert call(hiplib, 4, 10, 16, c)[0] == -1, acars.cfg_dict(c)
        with pytest.raises(_lib.PysdrError):
            acars.plan(4, 10, 16, c)
    for c in (changed("pll_shift", 1), changed("pll_shift", 4), changed("pmax", 1e18), changed("w_baud", 1 << 29)):
        assert call(hiplib, 4, 10, 16, c)[0] == 0, acars.cfg_dict(c)
    # the handle-taking calls check their arguments before any device work
    h, n = C.c_void_p(), C.c_int(-1)
    L, tw, c = acars.tables(25000.0)
    assert hiplib.pysdr_acars_create(None, L, C.byref(cfg), _lib.as_pf(tw), _lib.as_pf(c), 16, C.byref(h)) == -1 and not h.value
    assert hiplib.pysdr_acars_create(None, L, C.byref(cfg), _lib.as_pf(tw), _lib.as_pf(c), 16, None) == -1
    assert hiplib.pysdr_acars_process(None, None, 0, 0, C.byref(n), None, None, 0) == -1
    assert hiplib.pysdr_acars_reset(None) == -1 and hiplib.pysdr_acars_sync(None) == -1
    assert hiplib.pysdr_acars_fetch(None, None, 0, None, 0) == -1 and hiplib.pysdr_acars_state(None, None, None) == -1
    hiplib.pysdr_acars_destroy(None)


def test_the_skimmer_refuses_rows_outside_its_rates_before_it_needs_a_device():
    from pysdr_amd import acars
    with pytest.raises(ValueError):
        acars.ACARS_Skimmer(200000.0, 16, 2)                                # rows at 100 kHz
    with pytest.raises(ValueError):
        acars.ACARS_Skimmer(153600.0, 16, 16)                               # rows at 9.6 kHz
    with pytest.raises(ValueError):
        acars.ACARS_Skimmer(408000.0, 16, 8)                                # rows at 51 kHz


def test_tiles_cover_every_sample_the_phases_equal_the_transcription_and_the_slots_hold_the_cap(tmp_path):
    """the tile walk, all phases against a plain transcription of the definition, the cap proof, the frame machine, the
    event words"""
    plan_program.run("tests/acars_plan/plan_main.cpp", "ACARS_PLAN_OK", tmp_path, extra_flags=("-ffp-contract=off",))
