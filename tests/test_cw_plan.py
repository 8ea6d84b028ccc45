"""The CW skimmer's plan (pysdr_cw_plan, include/pysdr_hip.h; pysdr_amd/csrc/cw_plan.h): what it refuses, the event cap,
the event word -- through the library, which needs no device for this -- and the tile walk, the bank-conflict rule and the
event slots in a stand-alone C++ program (tests/cw_plan/plan_main.cpp) built and run by tests/plan_program.py, under
AddressSanitizer + UBSan where they are usable.
CPU only; nothing that is loaded into Python runs under a sanitizer."""
import ctypes as C

import numpy as np
import pytest

from tests import plan_program


def good():
    from pysdr_amd import cw
    return cw.params(375.0, settle=24)


def call(lib, nk, max_out, cfg):
    out = (C.c_int32 * 8)(*([-7] * 8))
    rc = lib.pysdr_cw_plan(nk, max_out, None if cfg is None else C.byref(cfg), out)
    return rc, list(out)


def test_plan_of_good_shapes(hiplib):
    from pysdr_amd import cw
    cfg = good()
    for nk in (1, 9, 63, 64, 65, 70, 4095, 4096):
        for mo in (1, 2, 3, 31, 32, 33, 1024, 1 << 21):
            rc, v = call(hiplib, nk, mo, cfg)
            assert rc == 0, (nk, mo, hiplib.pysdr_last_error())
            assert v == [64, 64, 64 * 33 * 8, 32, 2 * (mo // 3 + 1), -(-nk // 64), 0, 0]
            assert cw.plan(nk, mo, cfg) == dict(rows=64, threads=64, lds_bytes=16896, tile=32, cap=2 * (mo // 3 + 1), groups=-(-nk // 64))
    assert C.sizeof(cw.CwCfg) == 44


def test_plan_refuses_bad_shapes_and_settings(hiplib):
    from pysdr_amd import _lib, cw
    cfg = good()
    assert hiplib.pysdr_cw_plan(64, 16, C.byref(cfg), None) == -1
    for nk, mo in ((0, 16), (-1, 16), (4097, 16), (64, 0), (64, -1), (64, (1 << 21) + 1)):
        rc, v = call(hiplib, nk, mo, cfg)
        assert rc == -1 and v == [-7] * 8, (nk, mo)
        assert b"pysdr_cw_plan" in hiplib.pysdr_last_error()
    assert call(hiplib, 64, 16, None)[0] == -1
    bad = []
    for k in ("a_s", "a_p", "a_n", "snr_min", "hi", "lo", "fl"):
        bad += [(k, 0.0), (k, -0.5), (k, float("nan")), (k, float("inf"))]
    bad += [("a_s", 1.0000001), ("a_p", 2.0), ("a_n", 1.5), ("lo", 2.5),
            ("dmin", 15), ("dmin", 0), ("dmin", -4), ("d0", 119), ("d0", 1441), ("dmax", (1 << 22) + 1), ("dmax", 359),
            ("n0", 0), ("n0", -1), ("n0", (1 << 22) + 1)]
    for k, v in bad:
        c = good()
        setattr(c, k, v)
        assert call(hiplib, 64, 16, c)[0] == -1, (k, v)
        with pytest.raises(_lib.PysdrError):
            cw.plan(64, 16, c)
    for k, v in (("a_s", 1.0), ("dmin", 16), ("d0", 120), ("d0", 1440), ("dmax", 1 << 22), ("n0", 1), ("n0", 1 << 22), ("lo", 2.0)):
        c = good()
        setattr(c, k, v)
        assert call(hiplib, 64, 16, c)[0] == 0, (k, v)
    # the handle-taking calls check their arguments before any device work
    h, n = C.c_void_p(), C.c_int(-1)
    assert hiplib.pysdr_cw_create(None, C.byref(cfg), 16, C.byref(h)) == -1 and not h.value
    assert hiplib.pysdr_cw_create(None, C.byref(cfg), 16, None) == -1
    assert hiplib.pysdr_cw_process(None, None, 0, 0, C.byref(n), None, None, 0) == -1
    assert hiplib.pysdr_cw_reset(None) == -1 and hiplib.pysdr_cw_sync(None) == -1
    assert hiplib.pysdr_cw_fetch(None, None, 0, None, 0) == -1 and hiplib.pysdr_cw_state(None, None, None, None, None) == -1
    hiplib.pysdr_cw_destroy(None)


def test_cap_follows_the_bound_and_the_word_round_trips():
    """cap = 2 (max_out // 3 + 1): two character events are at least three samples apart and each is followed by at most
    its own word space (that no key sequence beats it is the C++ program's business)"""
    from pysdr_amd import cw
    from tests import cw_oracle as co
    cfg = good()
    for mo in list(range(1, 70)) + [1023, 1024, 1025, 4096]:
        assert cw.plan(7, mo, cfg)["cap"] == co.cap_of(mo) == 2 * (mo // 3 + 1) >= min(mo, 2)
    rng = np.random.default_rng(3)
    for i, c in [(0, 0), (0, 256), ((1 << 21) - 1, 255), ((1 << 21) - 1, 256)] + [(int(a), int(b)) for a, b in
                                                                                   zip(rng.integers(0, 1 << 21, 200), rng.integers(0, 257, 200))]:
        w = np.int32(co.pack(i, c))
        assert w >= 0 and cw.unpack(w) == (i, c) and co.unpack(w) == (i, c)
    assert cw.unpack(np.int32(-1)) == ((1 << 23) - 1, 511)          # the word is read as unsigned


def test_tiles_cover_every_sample_once_and_the_slots_hold_the_cap(tmp_path):
    plan_program.run("tests/cw_plan/plan_main.cpp", "CW_PLAN_OK", tmp_path)
