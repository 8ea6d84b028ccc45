"""The PSK31 skimmer's plan (pysdr_psk_plan, include/pysdr_hip.h; pysdr_amd/csrc/psk_plan.h): what it refuses, the event
cap, the event word -- through the library, which needs no device for this -- and the tile walk, the LDS layout and the
event slots in a stand-alone C++ program (tests/psk_plan/plan_main.cpp) built and run by tests/plan_program.py, under
AddressSanitizer + UBSan where they are usable.
CPU only; nothing that is loaded into Python runs under a sanitizer."""
import ctypes as C

import pytest

from tests import plan_program


def good():
    from pysdr_amd import psk
    return psk.params()


def call(lib, nk, S, max_out, cfg):
    out = (C.c_int32 * 8)(*([-7] * 8))
    rc = lib.pysdr_psk_plan(nk, S, max_out, None if cfg is None else C.byref(cfg), out)
    return rc, list(out)


def test_plan_of_good_shapes(hiplib):
    from pysdr_amd import psk
    from tests import psk_oracle as po
    cfg = good()
    for S, rows, threads, lds in ((8, 2, 64, 5424), (12, 4, 192, 15168)):
        for nk in (1, 2, 3, 4, 5, 9, 128, 512, (1 << 18) // (4 * S)):
            for mo in (1, 11, 12, 13, 17, 18, 19, 63, 64, 65, 256, 1 << 20):
                rc, v = call(hiplib, nk, S, mo, cfg)
                assert rc == 0, (nk, S, mo, hiplib.pysdr_last_error())
                cap = mo // (3 * S // 2) + 1
                assert v == [rows, threads, lds, 64, cap, -(-nk // rows), 4 * S, 0]
                assert cap == po.cap_of(mo, S)
                assert psk.plan(nk, S, mo, cfg) == dict(rows=rows, threads=threads, lds_bytes=lds, tile=64, cap=cap, groups=-(-nk // rows), nsub=4 * S)
    assert C.sizeof(psk.PskCfg) == 28


def test_plan_refuses_bad_shapes_and_settings(hiplib):
    from pysdr_amd import _lib, psk
    cfg = good()
    assert hiplib.pysdr_psk_plan(4, 8, 16, C.byref(cfg), None) == -1
    for nk, S, mo in ((0, 8, 16), (-1, 8, 16), (8193, 8, 16), (5462, 12, 16), (4, 8, 0), (4, 8, -1), (4, 8, (1 << 20) + 1),
                      (4, 0, 16), (4, 4, 16), (4, 10, 16), (4, 16, 16), (4, -8, 16)):
        rc, v = call(hiplib, nk, S, mo, cfg)
        assert rc == -1 and v == [-7] * 8, (nk, S, mo)
        assert b"pysdr_psk_plan" in hiplib.pysdr_last_error()
    assert call(hiplib, 4, 8, 16, None)[0] == -1
    bad = []
    for k in ("a_t", "a_q", "hi", "lo", "hy", "pmax"):
        bad += [(k, 0.0), (k, -0.5), (k, float("nan")), (k, float("inf")), (k, float("-inf"))]
    bad += [("a_t", 1.0000001), ("a_q", 2.0), ("lo", 0.8), ("pmax", 1.1e18), ("n0", 0), ("n0", -1), ("n0", (1 << 22) + 1)]
    for k, v in bad:
        c = good()
        setattr(c, k, v)
        assert call(hiplib, 4, 8, 16, c)[0] == -1, (k, v)
        with pytest.raises(_lib.PysdrError):
            psk.plan(4, 8, 16, c)
    for k, v in (("a_t", 1.0), ("a_q", 1.0), ("n0", 1), ("n0", 1 << 22), ("lo", 0.75), ("pmax", 1e18), ("hy", 1.0)):
        c = good()
        setattr(c, k, v)
        assert call(hiplib, 4, 8, 16, c)[0] == 0, (k, v)
    # the handle-taking calls check their arguments before any device work
    h, n = C.c_void_p(), C.c_int(-1)
    tw, g = psk.tables(8)
    assert hiplib.pysdr_psk_create(None, 8, C.byref(cfg), _lib.as_pf(tw), _lib.as_pf(g), 16, C.byref(h)) == -1 and not h.value
    assert hiplib.pysdr_psk_create(None, 8, C.byref(cfg), _lib.as_pf(tw), _lib.as_pf(g), 16, None) == -1
    assert hiplib.pysdr_psk_process(None, None, 0, 0, C.byref(n), None, None, 0, None, None) == -1
    assert hiplib.pysdr_psk_reset(None) == -1 and hiplib.pysdr_psk_sync(None) == -1
    assert hiplib.pysdr_psk_fetch(None, None, 0, None, 0) == -1 and hiplib.pysdr_psk_state(None, None, None, None) == -1
    hiplib.pysdr_psk_destroy(None)


def test_tiles_cover_every_sample_once_and_the_slots_hold_the_cap(tmp_path):
    """the tile walk, the filter against the definition, the cap"""
    plan_program.run("tests/psk_plan/plan_main.cpp", "PSK_PLAN_OK", tmp_path, extra_flags=("-ffp-contract=off",))
