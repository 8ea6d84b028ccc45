"""The FT4 skimmer's plan (pysdr_ft4_plan, include/pysdr_hip.h; pysdr_amd/csrc/ft_plan.h): what it refuses, the event cap
and the ring depth -- through the library, which needs no device for this -- the shapes of the raster at one stage and
at two (8 MS/s, 512 kS/s), and the tile walk, the spectrum, the sync score with its symbol and tone tables, the soft
bits, the cap proof, the ring-depth rule and pysdr_ft4_llr's validity window in a stand-alone C++ program
(tests/ft_plan/plan_main.cpp, run for this mode) built and run by tests/plan_program.py, under AddressSanitizer + UBSan
where they are usable.  CPU only; nothing that is loaded into Python runs under a sanitizer."""
import ctypes as C

import pytest

from tests import plan_program


def good():
    from pysdr_amd import ft4
    return ft4.params()


def call(lib, nk, S, max_out, cfg):
    out = (C.c_int32 * 8)(*([-7] * 8))
    rc = lib.pysdr_ft4_plan(nk, S, max_out, None if cfg is None else C.byref(cfg), out)
    return rc, list(out)


def test_plan_of_good_shapes(hiplib):
    from pysdr_amd import ft4
    from tests import ft4_oracle as fo
    cfg = good()
    for S, threads, lds in ((48, 128, 2296), (72, 192, 3448)):
        qs = S // 4
        for nk in (1, 2, 3, 32, 512, 2048):
            for mo in (1, qs - 1, qs, qs + 1, 4 * qs, 5 * qs - 1, 5 * qs, 15, 16, 17, 255, 256, 257, 1000):
                rc, v = call(hiplib, nk, S, mo, cfg)
                assert rc == 0, (nk, S, mo, hiplib.pysdr_last_error())
                spc = mo // qs + 1
                cap, tr = spc // 5 + 1, 417 + 2 * spc
                assert v == [1, threads, lds, S, cap, nk, S // 2, tr]
                assert cap == fo.cap_of(mo, S) and tr == fo.ring_steps(mo, S)
                assert ft4.plan(nk, S, mo, cfg) == dict(rows=1, threads=threads, lds_bytes=lds, tile=S, cap=cap, groups=nk, nsub=S // 2, tr=tr)
    assert [ft4.plan(3, S, mo, cfg)["cap"] for S in (48, 72) for mo in (16, 256)] == [1, 5, 1, 4]
    assert [ft4.plan(3, S, mo, cfg)["tr"] for S in (48, 72) for mo in (16, 256)] == [421, 461, 419, 447]
    assert C.sizeof(ft4.Ft4Cfg) == 12
    assert ft4.cfg_dict(cfg) == {k: (float(v) if k != "hmin" else v) for k, v in fo.params().items()}
    assert (ft4.EMIT_LAG, ft4.HOLD, ft4.KEEP) == (fo.EMIT, fo.HOLD, fo.KEEP) == (412, 417, 9)
    for n in (0, 47, 48, 59, 60, 7000):
        assert ft4.steps_done(n, 48) == fo.steps_done(n, 48)
    assert ft4.steps_done(7000, 48) == 580 and ft4.steps_done(72, 72) == 1 and ft4.steps_done(89, 72) == 1 and ft4.steps_done(90, 72) == 2


def test_plan_refuses_bad_shapes_and_settings(hiplib):
    from pysdr_amd import _lib, ft4
    cfg = good()
    assert hiplib.pysdr_ft4_plan(4, 48, 16, C.byref(cfg), None) == -1
    for nk, S, mo in ((0, 48, 16), (-1, 48, 16), (10923, 48, 16), (7282, 72, 16), (4, 48, 0), (4, 48, -1), (4, 48, (1 << 20) + 1),
                      (4, 0, 16), (4, 24, 16), (4, 64, 16), (4, 96, 16), (4, 47, 16), (4, 144, 16), (4, -48, 16),
                      (10922, 48, 4096)):                                     # a ring of 1.44 GB
        rc, v = call(hiplib, nk, S, mo, cfg)
        assert rc == -1 and v == [-7] * 8, (nk, S, mo)
        assert b"pysdr_ft4_plan" in hiplib.pysdr_last_error()
    # the whole text of one refusal: the mode's numbers in it come from the traits of ft_plan.h
    assert call(hiplib, 10923, 48, 16, cfg)[0] == -1
    assert hiplib.pysdr_last_error() == (
        b"pysdr_ft4_plan: S 48 is neither 48 nor 72, nk 10923 < 1 or nk S / 2 > 262144, max_out 16 outside [1, 1048576], a spectrum ring "
        b"above 1073741824 bytes, or a cfg outside the rules (NULL; smin >= 0, 0 <= hmin <= 16, 0 < pmax <= 1e18, all finite)")
    assert call(hiplib, 10922, 48, 256, cfg)[0] == 0 and call(hiplib, 7281, 72, 16, cfg)[0] == 0 and call(hiplib, 512, 48, 4096, cfg)[0] == 0
    assert call(hiplib, 4, 48, 16, None)[0] == -1
    bad = [("smin", -0.5), ("smin", float("nan")), ("smin", float("inf")), ("smin", float("-inf")), ("hmin", -1), ("hmin", 17)]
    bad += [("pmax", v) for v in (0.0, -0.5, float("nan"), float("inf"), float("-inf"), 1.1e18)]
    for k, v in bad:
        c = good()
        setattr(c, k, v)
        assert call(hiplib, 4, 48, 16, c)[0] == -1, (k, v)
        with pytest.raises(_lib.PysdrError):
            ft4.plan(4, 48, 16, c)
    for k, v in (("smin", 0.0), ("smin", 1e30), ("hmin", 0), ("hmin", 16), ("pmax", 1e18), ("pmax", 1e-30)):
        c = good()
        setattr(c, k, v)
        assert call(hiplib, 4, 48, 16, c)[0] == 0, (k, v)
    # the handle-taking calls check their arguments before any device work
    h, n = C.c_void_p(), C.c_int(-1)
    tw = ft4.tables(48)
    assert hiplib.pysdr_ft4_create(None, 48, C.byref(cfg), _lib.as_pf(tw), 16, C.byref(h)) == -1 and not h.value
    assert hiplib.pysdr_ft4_create(None, 48, C.byref(cfg), _lib.as_pf(tw), 16, None) == -1
    assert hiplib.pysdr_ft4_process(None, None, 0, 0, C.byref(n), None, None, 0, None) == -1
    assert hiplib.pysdr_ft4_reset(None) == -1 and hiplib.pysdr_ft4_sync(None) == -1
    assert hiplib.pysdr_ft4_fetch(None, None, 0, None, 0) == -1 and hiplib.pysdr_ft4_state(None, None, None, None, None) == -1
    assert hiplib.pysdr_ft4_llr(None, None, None, 0, None) == -1
    hiplib.pysdr_ft4_destroy(None)


def test_the_shapes_of_one_stage_and_of_two(hiplib):
    """ft4.shape at the listed rates; at 8 MS/s and 512 kS/s the two-stage shape ft4.fine_channelizer takes, through
    fine.plan: rows 250 Hz apart at 48 samples per symbol"""
    from pysdr_amd import fine, ft4
    assert ft4.shape(8000) == (48, 8, 32) and ft4.shape(16000) == (48, 16, 64) and ft4.shape(12000) == (72, 8, 32) and ft4.shape(48000) == (72, 32, 128)
    for fs in (8e6, 44100, 300.0, 1000.0 * 3 / 7):
        with pytest.raises(ValueError):
            ft4.shape(fs)
    assert fine.shape(8e6, 48 * ft4.BAUD, 4) == (2000, 1000, 32, 8) and fine.shape(512e3, 48 * ft4.BAUD, 4) == (128, 64, 32, 8)
    for fs in (8e6, 512e3):
        M1, D1, M2, D2 = fine.shape(fs, 48 * ft4.BAUD, 4)
        assert M1 == 2 * D1 and M2 == 4 * D2 and D1 * D2 * 1000 == fs
        band = (100e3, 100e3 + 7 * 250.0)
        g_first, ng = fine.channels_for(band, fs, M1, D1, M2)
        p = fine.plan(M1, D1, M2, D2, len(fine.prototype1(fs, M1, D1, M2)), len(ft4.prototype(fs / D1, M2, 48)), g_first, ng)
        assert ng == 8 and fs / p["Mf"] == 250.0 and fs / p["D"] == 1000.0 and p["Mf"] == 4 * p["D"]
        assert ft4.plan(ng, 48, 256, ft4.params())["groups"] == 8


def test_tiles_cover_every_sample_once_the_steps_equal_the_transcription_and_the_proofs_hold(tmp_path):
    """the tile walk over cut streams, spectrum, sync, peak and soft bits against plain transcriptions, the symbol and tone
    tables against the lists written out, the cap proof, the ring-depth rule and the validity window of the soft bits"""
    plan_program.run("tests/ft_plan/plan_main.cpp", "FT4_PLAN_OK", tmp_path, extra_flags=("-ffp-contract=off",), args=("ft4",))
