"""The SSTV skimmer's plan (pysdr_sstv_plan, include/pysdr_hip.h; pysdr_amd/csrc/sstv_plan.h): what it refuses, the event
cap, the struct -- through the library, which needs no device for this -- and the tile walk, every step against a plain
transcription of the definition, the pixel boundaries of every mode, the cap's proof and the event words in a stand-alone
C++ program (tests/sstv_plan/plan_main.cpp) built and run by tests/plan_program.py, under AddressSanitizer + UBSan where
they are usable.  CPU only; nothing that is loaded into Python runs under a sanitizer."""
import ctypes as C

import pytest

from tests import plan_program
from tests import sstv_oracle as so

UNTOUCHED = [-7] * 8


def good(fs_out=25000.0, det="FM", modes=None):
    from pysdr_amd import sstv
    return sstv.params(fs_out, det, sstv.MODES if modes is None else modes)


def call(lib, nk, L, max_out, cfg):
    out = (C.c_int32 * 8)(*UNTOUCHED)
    rc = lib.pysdr_sstv_plan(nk, L, max_out, None if cfg is None else C.byref(cfg), out)
    return rc, list(out)


def test_plan_of_good_shapes(hiplib):
    from pysdr_amd import sstv
    assert C.sizeof(sstv.SstvMode) == 32 and C.sizeof(sstv.SstvCfg) == 552
    for fs_out in (8000.0, 12000.0, 16000.0, 25000.0, 48000.0):
        for det in ("FM", "USB"):
            cfg = good(fs_out, det)
            par = so.params(fs_out, det)
            L = sstv.filter_length(fs_out)
            assert L == so.tables(fs_out)[0] and 9 <= L <= 96
            H = 2 * cfg.R0 + 2 * cfg.W + L + 1
            for nk in (1, 7, 8, 9, 800):
                for mo in (1, 16, 64, 4096, 1 << 17):
                    rc, v = call(hiplib, nk, L, mo, cfg)
                    assert rc == 0, (fs_out, nk, mo, hiplib.pysdr_last_error())
                    cap = so.cap_of(mo, par)
                    assert v == [8, 256, v[2], 64, cap, -(-nk // 8), H, 800] and v[2] <= 65536
                    assert sstv.plan(nk, L, mo, cfg) == dict(rows=8, threads=256, lds_bytes=v[2], tile=64, cap=cap, groups=-(-nk // 8),
                                                             history=H, line_words=800)
    # a call of 4096 outputs at 25 kHz is shorter than any line: one line event, its end, two starts
    assert so.cap_of(4096, so.params(25000.0)) == (800 + 9) + 5


def test_the_settings_are_the_oracle_s(hiplib):
    from pysdr_amd import sstv
    import numpy as np
    tiny = sstv.Mode("TINY", 5, 3, 32, 6, 5.0, 1.0, 0.5, 0.5, "GBR")
    for fs_out in (8000.0, 12000.0, 25000.0, 48000.0):
        for det in ("FM", "USB"):
            c, par = sstv.cfg_dict(sstv.params(fs_out, det, sstv.MODES + (tiny,))), so.params(fs_out, det, so.MODES + [so.TINY])
            for k in ("w_sub", "w_tick", "W", "R0", "lag"):
                assert c[k] == par[k], (fs_out, det, k)
            assert np.float32(c["k_hz"]) == par["k_hz"] and np.float32(c["k_rho"]) == par["k_rho"] and np.float32(c["pmax"]) == par["pmax"]
            assert c["modes"] == [{k: v for k, v in md.items() if k != "name"} for md in par["modes"]]
        L, tw, g = sstv.tables(fs_out)
        L2, tw2, g2 = so.tables(fs_out)
        assert L == L2 and np.array_equal(tw.view(np.uint32), tw2.view(np.uint32)) and np.array_equal(g.view(np.uint32), g2.view(np.uint32))
    assert [(m.name, m.code) for m in sstv.MODES] == [(m[0], m[1]) for m in so.MODES]
    assert abs(sstv.line_ms(sstv.mode_named("PD120")) - 508.48) < 1e-9 and abs(sstv.line_ms(sstv.mode_named("Martin M1")) - 446.446) < 1e-9


def test_plan_refuses_bad_shapes_and_settings(hiplib):
    from pysdr_amd import _lib, sstv
    cfg = good()
    L = 37
    assert hiplib.pysdr_sstv_plan(4, L, 16, C.byref(cfg), None) == -1
    for nk, l, mo in ((0, L, 16), (-1, L, 16), ((1 << 15) + 1, L, 16), (4, L, 0), (4, L, -1), (4, L, (1 << 20) + 1), (4, 8, 16), (4, 97, 16),
                      (4, 0, 16), (4, -37, 16), (1 << 15, L, 1 << 20)):
        rc, v = call(hiplib, nk, l, mo, cfg)
        assert rc == -1 and v == UNTOUCHED, (nk, l, mo)
        assert b"pysdr_sstv_plan" in hiplib.pysdr_last_error()
    assert call(hiplib, 4, L, 16, None) == (-1, UNTOUCHED)
    assert call(hiplib, 4, 9, 16, cfg)[0] == 0 and call(hiplib, 4, 96, 16, cfg)[0] == 0 and call(hiplib, 1 << 15, L, 16, cfg)[0] == 0

    def changed(k, v):
        c = good()
        setattr(c, k, v)
        return c

    def mode_changed(i, k, v, **more):
        c = good()
        setattr(c.modes[i], k, v)
        for kk, vv in more.items():
            setattr(c.modes[i], kk, vv)
        return c

    bad = [changed("pmax", v) for v in (0.0, -0.5, float("nan"), float("inf"), float("-inf"), 1.1e18)]
    bad += [changed("det", 2), changed("det", -1), changed("nmodes", 0), changed("nmodes", 17)]
    bad += [changed("w_tick", 0), changed("w_tick", 2 * cfg.w_tick), changed("w_tick", cfg.w_tick // 2)]       # the fs-derived words
    bad += [changed("R0", cfg.R0 + 2), changed("R0", 79), changed("W", cfg.W + 1), changed("W", 0), changed("lag", cfg.lag + 1), changed("lag", cfg.lag - 1)]
    bad += [changed("k_hz", 1.1 * cfg.k_hz), changed("k_hz", float("nan")), changed("k_rho", 1.1 * cfg.k_rho), changed("k_rho", float("nan"))]
    bad += [mode_changed(2, "scan_q", (640 << 16) - 1),                      # a pixel under one sample
            mode_changed(2, "lines", 0), mode_changed(2, "lines", 4097), mode_changed(6, "width", 801, scan_q=0xF0000000), mode_changed(6, "width", 0),
            mode_changed(5, "code", cfg.modes[1].code), mode_changed(5, "code", 128), mode_changed(5, "code", -1),
            mode_changed(0, "scans", 0), mode_changed(0, "scans", 5), mode_changed(0, "sync_q", 0xFFFFFFFF)]
    for c in bad:
        assert call(hiplib, 4, L, 16, c) == (-1, UNTOUCHED), sstv.cfg_dict(c)
        with pytest.raises(_lib.PysdrError):
            sstv.plan(4, L, 16, c)
    for c in (changed("pmax", 1e18), changed("det", 1), changed("w_sub", 0), changed("nmodes", 1), mode_changed(2, "scan_q", 640 << 16)):
        assert call(hiplib, 4, L, 16, c)[0] == 0, sstv.cfg_dict(c)
    # the handle-taking calls check their arguments before any device work
    h, n = C.c_void_p(), C.c_int(-1)
    L, tw, g = sstv.tables(25000.0)
    assert hiplib.pysdr_sstv_create(None, L, C.byref(cfg), _lib.as_pf(tw), _lib.as_pf(g), 16, C.byref(h)) == -1 and not h.value
    assert hiplib.pysdr_sstv_create(None, L, C.byref(cfg), _lib.as_pf(tw), _lib.as_pf(g), 16, None) == -1
    assert hiplib.pysdr_sstv_process(None, None, 0, 0, C.byref(n), None, None, 0) == -1
    assert hiplib.pysdr_sstv_reset(None) == -1 and hiplib.pysdr_sstv_sync(None) == -1
    assert hiplib.pysdr_sstv_fetch(None, None, 0, None, 0) == -1 and hiplib.pysdr_sstv_state(None, None, None, None, None) == -1
    hiplib.pysdr_sstv_destroy(None)


def test_the_skimmer_refuses_rows_outside_its_rates_before_it_needs_a_device():
    from pysdr_amd import sstv
    with pytest.raises(ValueError):
        sstv.SSTV_Skimmer(200000.0, 16, 2)                                  # rows at 100 kHz
    with pytest.raises(ValueError):
        sstv.SSTV_Skimmer(48000.0, 16, 8)                                   # rows at 6 kHz
    with pytest.raises(ValueError):
        sstv.params(25000.0, modes=sstv.MODES * 2)
    with pytest.raises(KeyError):
        sstv.params(25000.0, det="AM")


def test_tiles_cover_every_sample_once_the_steps_equal_the_transcription_and_the_slots_hold_the_cap(tmp_path):
    """the tile walk, every step against a plain transcription of the definition, the pixel boundaries, the cap proof, the
    event words"""
    plan_program.run("tests/sstv_plan/plan_main.cpp", "SSTV_PLAN_OK", tmp_path, extra_flags=("-ffp-contract=off",))
