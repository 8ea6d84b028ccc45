"""The FT8 skimmer's plan (pysdr_ft8_plan, include/pysdr_hip.h; pysdr_amd/csrc/ft_plan.h): what it refuses, the event cap
and the ring depth -- through the library, which needs no device for this -- the shape a fine channelizer takes at
8 MS/s, and the tile walk, the spectrum, the sync score, the peak rule, the soft bits, the cap proof, the ring-depth rule
and pysdr_ft8_llr's validity window in a stand-alone C++ program (tests/ft_plan/plan_main.cpp, run for this mode) built and
run by tests/plan_program.py, under AddressSanitizer + UBSan where they are usable.  CPU only; nothing that is loaded into
Python runs under a sanitizer."""
import ctypes as C

import pytest

from tests import plan_program


def good():
    from pysdr_amd import ft8
    return ft8.params()


def call(lib, nk, S, max_out, cfg):
    out = (C.c_int32 * 8)(*([-7] * 8))
    rc = lib.pysdr_ft8_plan(nk, S, max_out, None if cfg is None else C.byref(cfg), out)
    return rc, list(out)


def test_plan_of_good_shapes(hiplib):
    from pysdr_amd import ft8
    from tests import ft8_oracle as fo
    cfg = good()
    for S, threads, lds in ((64, 192, 3064), (96, 256, 4600)):
        qs = S // 4
        for nk in (1, 2, 3, 80, 512, 2048):
            for mo in (1, qs - 1, qs, qs + 1, 4 * qs, 5 * qs - 1, 5 * qs, 63, 64, 65, 256, 1000):
                rc, v = call(hiplib, nk, S, mo, cfg)
                assert rc == 0, (nk, S, mo, hiplib.pysdr_last_error())
                spc = mo // qs + 1
                cap, tr = spc // 5 + 1, 321 + 2 * spc
                assert v == [1, threads, lds, S, cap, nk, S // 2, tr]
                assert cap == fo.cap_of(mo, S) and tr == fo.ring_steps(mo, S)
                assert ft8.plan(nk, S, mo, cfg) == dict(rows=1, threads=threads, lds_bytes=lds, tile=S, cap=cap, groups=nk, nsub=S // 2, tr=tr)
    assert C.sizeof(ft8.Ft8Cfg) == 12
    assert ft8.cfg_dict(cfg) == {k: (float(v) if k != "hmin" else v) for k, v in fo.params().items()}
    assert ft8.cfg_dict(cfg) == dict(smin=3.0, hmin=13, pmax=float(fo.F32(1e18)))
    assert (ft8.EMIT_LAG, ft8.HOLD, ft8.KEEP) == (fo.EMIT, fo.HOLD, fo.KEEP)
    for n in (0, 63, 64, 79, 80, 5600):
        assert ft8.steps_done(n, 64) == fo.steps_done(n, 64)


def test_plan_refuses_bad_shapes_and_settings(hiplib):
    from pysdr_amd import _lib, ft8
    cfg = good()
    assert hiplib.pysdr_ft8_plan(4, 64, 16, C.byref(cfg), None) == -1
    for nk, S, mo in ((0, 64, 16), (-1, 64, 16), (8193, 64, 16), (5462, 96, 16), (4, 64, 0), (4, 64, -1), (4, 64, (1 << 20) + 1),
                      (4, 0, 16), (4, 22, 16), (4, 32, 16), (4, 48, 16), (4, 128, 16), (4, -64, 16),
                      (8192, 64, 4096)):                                      # a ring of 1.26 GB
        rc, v = call(hiplib, nk, S, mo, cfg)
        assert rc == -1 and v == [-7] * 8, (nk, S, mo)
        assert b"pysdr_ft8_plan" in hiplib.pysdr_last_error()
    # the whole text of one refusal: the mode's numbers in it come from the traits of ft_plan.h
    assert call(hiplib, 8193, 64, 16, cfg)[0] == -1
    assert hiplib.pysdr_last_error() == (
        b"pysdr_ft8_plan: S 64 is neither 64 nor 96, nk 8193 < 1 or nk S / 2 > 262144, max_out 16 outside [1, 1048576], a spectrum ring "
        b"above 1073741824 bytes, or a cfg outside the rules (NULL; smin >= 0, 0 <= hmin <= 21, 0 < pmax <= 1e18, all finite)")
    assert call(hiplib, 8192, 64, 256, cfg)[0] == 0 and call(hiplib, 512, 64, 4096, cfg)[0] == 0
    assert call(hiplib, 4, 64, 16, None)[0] == -1
    bad = [("smin", -0.5), ("smin", float("nan")), ("smin", float("inf")), ("smin", float("-inf")), ("hmin", -1), ("hmin", 22)]
    bad += [("pmax", v) for v in (0.0, -0.5, float("nan"), float("inf"), float("-inf"), 1.1e18)]
    for k, v in bad:
        c = good()
        setattr(c, k, v)
        assert call(hiplib, 4, 64, 16, c)[0] == -1, (k, v)
        with pytest.raises(_lib.PysdrError):
            ft8.plan(4, 64, 16, c)
    for k, v in (("smin", 0.0), ("smin", 1e30), ("hmin", 0), ("hmin", 21), ("pmax", 1e18), ("pmax", 1e-30)):
        c = good()
        setattr(c, k, v)
        assert call(hiplib, 4, 64, 16, c)[0] == 0, (k, v)
    # the handle-taking calls check their arguments before any device work
    h, n = C.c_void_p(), C.c_int(-1)
    tw = ft8.tables(64)
    assert hiplib.pysdr_ft8_create(None, 64, C.byref(cfg), _lib.as_pf(tw), 16, C.byref(h)) == -1 and not h.value
    assert hiplib.pysdr_ft8_create(None, 64, C.byref(cfg), _lib.as_pf(tw), 16, None) == -1
    assert hiplib.pysdr_ft8_process(None, None, 0, 0, C.byref(n), None, None, 0, None) == -1
    assert hiplib.pysdr_ft8_reset(None) == -1 and hiplib.pysdr_ft8_sync(None) == -1
    assert hiplib.pysdr_ft8_fetch(None, None, 0, None, 0) == -1 and hiplib.pysdr_ft8_state(None, None, None, None, None) == -1
    assert hiplib.pysdr_ft8_llr(None, None, None, 0, None) == -1
    hiplib.pysdr_ft8_destroy(None)


def test_a_fine_channelizer_for_8_ms_per_second_is_valid_and_gives_rows_100_hz_apart(hiplib):
    """fs = 8 MS/s, where ft8.shape finds no single stage (M = 80000 is beyond a channelizer): fine.shape(8e6, 400, 4) is a
    valid two-stage shape whose rows are 100 Hz apart at 64 samples per symbol; so is 512 kS/s"""
    from pysdr_amd import fine, ft8
    for fs in (8e6, 512e3):
        M1, D1, M2, D2 = fine.shape(fs, 64 * ft8.BAUD, 4)
        assert M1 == 2 * D1 and M2 == 4 * D2 and D1 * D2 * 400 == fs
        band = (100e3, 100e3 + 7 * 100.0)
        g_first, ng = fine.channels_for(band, fs, M1, D1, M2)
        p = fine.plan(M1, D1, M2, D2, len(fine.prototype1(fs, M1, D1, M2)), len(ft8.prototype(fs / D1, M2, 64)), g_first, ng)
        assert ng == 8 and fs / p["Mf"] == 100.0 and fs / p["D"] == 400.0 and p["Mf"] == 4 * p["D"]
        assert ft8.plan(ng, 64, 256, ft8.params())["groups"] == 8
    for fs in (8e6, 512e3, 44100, 300.0):                                   # M = 5120 is beyond one stage too
        with pytest.raises(ValueError):
            ft8.shape(fs)
    assert ft8.shape(8000) == (64, 20, 80) and ft8.shape(12000) == (96, 20, 80) and ft8.shape(48000) == (96, 80, 320) and ft8.shape(16000) == (64, 40, 160)


def test_tiles_cover_every_sample_once_the_steps_equal_the_transcription_and_the_proofs_hold(tmp_path):
    """the tile walk over cut streams, spectrum, sync, peak and soft bits against plain transcriptions, the cap proof, the
    ring-depth rule and the validity window of the soft bits"""
    plan_program.run("tests/ft_plan/plan_main.cpp", "FT8_PLAN_OK", tmp_path, extra_flags=("-ffp-contract=off",), args=("ft8",))
