"""The fine channelizer's plan (pysdr_chan_fine_plan, include/pysdr_hip.h; pysdr_amd/csrc/fine_plan.h): what it accepts and
refuses and what it reports -- through the library, which needs no device for this -- and the rules, the channel map, the
tiles, the tap reads and the roll of a stream of ragged calls against brute force in a stand-alone C++ program
(tests/fine_plan/plan_main.cpp) built and run by tests/plan_program.py, under AddressSanitizer + UBSan where they are usable.  The same program checks the pure half
of the FFT that both channelizer stages share (pysdr_amd/csrc/fft_plan.h): passes, digit reversal, multipliers, twiddles.  CPU only; nothing that is loaded into
Python runs under a sanitizer."""
import ctypes as C

import pytest

from tests import plan_program


def call(lib, *a):
    out = (C.c_int32 * 16)(*([-7] * 16))
    return lib.pysdr_chan_fine_plan(*a, out), list(out)


def test_plan_of_good_shapes(hiplib):
    from pysdr_amd import fine
    #        M1    D1    M2   D2  g_first ng        Q    Mf     D     C2 k1_first nk1 slots hist radices
    for (M1, D1, M2, D2, g, ng), want in (
            ((16, 8, 16, 8, 0, 128), (8, 128, 64, 2, 0, 16, 64, 128, [4, 4])),
            ((64, 16, 32, 32, 64 * 8 - 13, 37), (8, 512, 512, 1, 62, 6, 64, 256, [4, 4, 2])),
            ((256, 128, 20, 5, 705, 3), (10, 2560, 640, 4, 71, 1, 64, 160, [5, 4])),
            ((640, 320, 256, 128, 7000, 300), (128, 81920, 40960, 2, 55, 3, 32, 2048, [4, 4, 4, 4])),
            ((4096, 2048, 64, 16, 131072 - 500, 1000), (32, 131072, 32768, 4, 4080, 33, 64, 512, [4, 4, 4])),
            ((4000, 2000, 64, 16, 0, 48), (32, 128000, 32000, 4, 0, 2, 64, 512, [4, 4, 4])),
            ((64, 32, 1024, 256, 0, 9), (512, 32768, 8192, 4, 0, 1, 8, 8192, [4, 4, 4, 4, 4]))):
        rc, v = call(hiplib, M1, D1, M2, D2, 8 * M1, 8 * M2, g, ng)
        assert rc == 0, (M1, D1, M2, D2, hiplib.pysdr_last_error())
        Q, Mf, D, C2, k1, nk1, slots, hist, rad = want
        assert v[:11] == [Q, Mf, D, C2, k1, nk1, slots, slots * (M2 | 1) * 8, hist, 8, len(rad)] and v[11:11 + len(rad)] == rad
        p = fine.plan(M1, D1, M2, D2, g_first=g, ng=ng)
        assert (p["Q"], p["Mf"], p["D"], p["C2"], p["k1_first"], p["nk1"], p["frames_per_wg"], p["history"], p["radices"]) == want
    assert fine.shape(8e6, 250.0, 4) == (4000, 2000, 64, 16)
    assert fine.shape(512e3, 250.0, 4) == (512, 256, 32, 8) and fine.shape(192e3, 375.0, 2) == (64, 32, 32, 16)
    assert fine.channels_for((-100.0, 100.0), 8e6, 4000, 2000, 64) == (128000 - 1, 3)
    with pytest.raises(ValueError):
        fine.shape(8e6, 251.0, 4)
    with pytest.raises(ValueError):
        fine.shape(48e3, 24e3, 4)


def test_plan_refuses_bad_shapes(hiplib):
    from pysdr_amd import _lib, fine
    good = (64, 32, 32, 16, 512, 256, 0, 1024)
    assert call(hiplib, *good)[0] == 0
    assert hiplib.pysdr_chan_fine_plan(*good, None) == -1
    for i, vals in ((0, (8, 48, 8192)), (1, (64, 8, 0, 5)),           # M1 outside the rules; C1 = 1, 8; D1 not a divisor
                    (2, (8, 24, 2048, 50)), (3, (32, 4, 0, 5)),        # M2; M2 = 50: Q = 25 is odd; C2 = 1 with Q = 16 is fine, 8 is not
                    (4, (0, 16 * 64 + 1)), (5, (0, 16 * 32 + 1)), (6, (-1, 1024)), (7, (0, 1025))):
        for v in vals:
            a = list(good)
            a[i] = v
            if i == 3 and v == 32:
                assert call(hiplib, *a)[0] == 0
                continue
            rc, out = call(hiplib, *a)
            assert rc == -1 and out == [-7] * 16, a
            assert b"pysdr_chan_fine_plan" in hiplib.pysdr_last_error()
    assert call(hiplib, 64, 32, 16, 8, 512, 128, 0, 1)[0] == 0 and call(hiplib, 64, 16, 16, 8, 256, 128, 0, 1)[0] == -1   # Q = 8, Q = 4
    assert call(hiplib, 4096, 2048, 1024, 256, 4096, 1024, 0, 65536)[0] == 0
    assert call(hiplib, 4096, 2048, 1024, 256, 4096, 1024, 0, 65537)[0] == -1
    with pytest.raises(_lib.PysdrError):
        fine.plan(64, 64, 32, 16)
    # the handle-taking calls check their arguments before any device work
    h = C.c_void_p()
    assert hiplib.pysdr_chan_fine_create(0, 64, 64, 32, 16, 0, 8, 512, 256, 4096, C.byref(h)) == -1 and not h.value
    assert hiplib.pysdr_chan_fine_create(0, 64, 32, 32, 16, 0, 8, 512, 256, 0, C.byref(h)) == -1 and not h.value
    assert hiplib.pysdr_chan_fine_create(0, 64, 32, 32, 16, 0, 8, 512, 256, 4096, None) == -1
    assert hiplib.pysdr_chan_fine_set_taps(None, None, 0, None, 0) == -1


def test_rules_map_tiles_and_the_roll_against_brute_force(tmp_path):
    out = plan_program.run("tests/fine_plan/plan_main.cpp", "FINE_PLAN_OK", tmp_path, includes=("pysdr_amd/csrc",))
    assert "35 FFT sizes" in out, out[-1500:]     # every 2^a 5^b in [16, 4096] went through the shared FFT plan's checks
