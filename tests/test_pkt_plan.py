"""The packet skimmer's plan (pysdr_pkt_plan, include/pysdr_hip.h; pysdr_amd/csrc/pkt_plan.h): what it refuses, the event
cap, the struct -- through the library, which needs no device for this -- and the tile walk, both phases against a plain
transcription of the definition, the cap's proof and the event words in a stand-alone C++ program
(tests/pkt_plan/plan_main.cpp) built and run by tests/plan_program.py, under AddressSanitizer + UBSan where they are usable.
CPU only; nothing that is loaded into Python runs under a sanitizer."""
import ctypes as C

import pytest

from tests import plan_program


def good(fs_out=25000.0):
    from pysdr_amd import packet
    return packet.params(fs_out)


def call(lib, nk, L, max_out, cfg):
    out = (C.c_int32 * 8)(*([-7] * 8))
    rc = lib.pysdr_pkt_plan(nk, L, max_out, None if cfg is None else C.byref(cfg), out)
    return rc, list(out)


def test_plan_of_good_shapes(hiplib):
    from pysdr_amd import packet
    from tests import pkt_oracle as po
    for fs_out in (9600.0, 19200.0, 24000.0, 25000.0, 48000.0):
        cfg = good(fs_out)
        L = packet.window_length(fs_out)
        gap = 2 ** 31 // cfg.w_baud + 1
        for nk in (1, 7, 8, 9, 16, 800, 1 << 15):
            for mo in (1, 16, gap, gap + 1, 24 * gap, 24 * gap + 1, 256, 4096, 1 << 20):
                rc, v = call(hiplib, nk, L, mo, cfg)
                assert rc == 0, (nk, L, mo, hiplib.pysdr_last_error())
                cap = 84 + (-(-mo // gap) - 1) // 24
                assert v == [8, 256, 32480, 64, cap, -(-nk // 8), 8, 83]
                assert cap == po.cap_of(mo, cfg.w_baud)
                assert packet.plan(nk, L, mo, cfg) == dict(rows=8, threads=256, lds_bytes=32480, tile=64, cap=cap, groups=-(-nk // 8),
                                                           slicers=8, frame_words=83)
    assert C.sizeof(packet.PktCfg) == 52
    assert po.cap_of(4096, good().w_baud) == 99 and po.cap_of(16, good().w_baud) == 84


def test_plan_refuses_bad_shapes_and_settings(hiplib):
    from pysdr_amd import _lib, packet
    cfg = good()
    assert hiplib.pysdr_pkt_plan(4, 21, 16, C.byref(cfg), None) == -1
    for nk, L, mo in ((0, 21, 16), (-1, 21, 16), ((1 << 15) + 1, 21, 16), (4, 21, 0), (4, 21, -1), (4, 21, (1 << 20) + 1),
                      (4, 7, 16), (4, 41, 16), (4, 0, 16), (4, -21, 16)):
        rc, v = call(hiplib, nk, L, mo, cfg)
        assert rc == -1 and v == [-7] * 8, (nk, L, mo)
        assert b"pysdr_pkt_plan" in hiplib.pysdr_last_error()
    assert call(hiplib, 4, 21, 16, None)[0] == -1
    assert call(hiplib, 4, 8, 16, cfg)[0] == 0 and call(hiplib, 4, 40, 16, cfg)[0] == 0 and call(hiplib, 1 << 15, 21, 1 << 20, cfg)[0] == 0

    def changed(k, v, s=None):
        c = good()
        if s is None:
            setattr(c, k, v)
        else:
            c.gain[s] = v
        return c

    bad = [changed("gain", v, s) for s in range(8) for v in (0.0, -0.5, float("nan"), float("inf"), float("-inf"))]
    bad += [changed("pmax", v) for v in (0.0, -0.5, float("nan"), float("inf"), float("-inf"), 1.1e18)]
    bad += [changed("pll_shift", v) for v in (0, 5, -1)] + [changed(k, 0) for k in ("w_mark", "w_space", "w_baud")]
    bad += [changed("w_baud", (1 << 29) + 1)]
    for c in bad:
        assert call(hiplib, 4, 21, 16, c)[0] == -1, packet.cfg_dict(c)
        with pytest.raises(_lib.PysdrError):
            packet.plan(4, 21, 16, c)
    for c in (changed("pll_shift", 1), changed("pll_shift", 4), changed("pmax", 1e18), changed("w_baud", 1 << 29), changed("gain", 1e30, 7)):
        assert call(hiplib, 4, 21, 16, c)[0] == 0, packet.cfg_dict(c)
    # the handle-taking calls check their arguments before any device work
    h, n = C.c_void_p(), C.c_int(-1)
    L, tw, g = packet.tables(25000.0)
    assert hiplib.pysdr_pkt_create(None, L, C.byref(cfg), _lib.as_pf(tw), _lib.as_pf(g), 16, C.byref(h)) == -1 and not h.value
    assert hiplib.pysdr_pkt_create(None, L, C.byref(cfg), _lib.as_pf(tw), _lib.as_pf(g), 16, None) == -1
    assert hiplib.pysdr_pkt_process(None, None, 0, 0, C.byref(n), None, None, 0) == -1
    assert hiplib.pysdr_pkt_reset(None) == -1 and hiplib.pysdr_pkt_sync(None) == -1
    assert hiplib.pysdr_pkt_fetch(None, None, 0, None, 0) == -1 and hiplib.pysdr_pkt_state(None, None, None) == -1
    hiplib.pysdr_pkt_destroy(None)


def test_the_skimmer_refuses_rows_outside_its_rates_before_it_needs_a_device():
    from pysdr_amd import packet
    with pytest.raises(ValueError):
        packet.Packet_Skimmer(200000.0, 16, 2)                              # rows at 100 kHz
    with pytest.raises(ValueError):
        packet.Packet_Skimmer(48000.0, 16, 8)                               # rows at 6 kHz
    with pytest.raises(ValueError):
        packet.params(25000.0, gain=[1.0] * 7)


def test_tiles_cover_every_sample_once_the_phases_equal_the_transcription_and_the_slots_hold_the_cap(tmp_path):
    """the tile walk, both phases against a plain transcription of the definition, the cap proof, the event words"""
    plan_program.run("tests/pkt_plan/plan_main.cpp", "PKT_PLAN_OK", tmp_path, extra_flags=("-ffp-contract=off",))
