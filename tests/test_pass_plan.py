"""The pure half of the second pass (pysdr_amd/csrc/pass_plan.h): pysdr_pass_plan through the library,
which needs no device for it, the refusals of the new calls that come before any device work, and the stand-alone C++
program (tests/pass_plan/plan_main.cpp) built and run by tests/plan_program.py, under AddressSanitizer + UBSan where they
are usable: the rows of a frame and their phase words at every fine row, which this test holds against the NumPy model
(tests/pass_oracle.py), the depth of both rings against a brute-force simulation of call sizes, and the rules' edges.  CPU
only; nothing that is loaded into Python runs under a sanitizer."""
import ctypes as C

import pytest

from tests import pass_oracle as po
from tests import plan_program


def call(lib, *args):
    out = (C.c_int32 * 8)(*([-7] * 8))
    return lib.pysdr_pass_plan(*args, out), list(out)


def test_plan_and_its_refusals(hiplib):
    from pysdr_amd import _lib, ft4, ft8
    rc, v = call(hiplib, 0, 3, 64, 64, 16)
    assert rc == 0 and v[0] == 256 and v[2:] == [5856, 362, 512, 256, 52, 3] and 0 < v[1] <= 65536
    assert ft8.pass_plan(ft8, 3, 64, 64, 16)["tr2"] == 362 == po.ring_steps2(po.FT8, 64, 64, 16) and po.ring_samples(362, 64) == 5856
    rc, v = call(hiplib, 1, 3, 48, 256, 40)
    assert rc == 0 and v[2:] == [po.ring_samples(v[3], 48), po.ring_steps2(po.FT4, 256, 48, 40), 512, 256, 52, 5] and 0 < v[1] <= 65536
    assert ft4.pass_plan(ft4, 3, 48, 256)["ty"] == v[2] and ft4.REACH_T == 40 == ft8.REACH_T
    for args in ((2, 3, 64, 64, 16), (-1, 3, 64, 64, 16), (0, 3, 48, 64, 16), (1, 3, 64, 64, 16), (0, 0, 64, 64, 16), (0, 3, 64, 0, 16),
                 (0, 3, 64, 64, 0), (0, 3, 64, 64, 121), (0, 8192, 64, 1 << 20, 16)):
        assert call(hiplib, *args) == (-1, [-7] * 8) and b"pysdr_pass_plan" in hiplib.pysdr_last_error(), args
    assert hiplib.pysdr_pass_plan(0, 3, 64, 64, 16, None) == -1
    with pytest.raises(_lib.PysdrError):
        ft8.pass_plan(ft8, 3, 64, 64, 121)


def test_the_new_calls_refuse_a_null_skimmer_before_any_device_work(hiplib):
    for kind in ("ft8", "ft4"):
        for what, args in (("keep", (None,)), ("subtract", (None, None, None, None, 0, None)), ("rescan", (0, 0, 0, 0, None, None, None)),
                           ("pass_decode", (None, None, 0, None, None, None, None, None, None)), ("pass_llr", (None, None, 0, None)),
                           ("pass_state", (None, None, None))):
            name = f"pysdr_{kind}_{what}"
            assert getattr(hiplib, name)(None, *args) == -1 and name.encode() in hiplib.pysdr_last_error(), name


def test_the_plan_program(tmp_path):
    out = plan_program.run("tests/pass_plan/plan_main.cpp", "PASS_PLAN_OK", tmp_path, includes=("pysdr_amd/csrc",))
    seen = 0
    for line in out.splitlines():
        if not line.startswith("ROWS "):
            continue
        f = [int(v) for v in line.split()[1:]]
        mode, S, nk, circular, F, n = f[:6]
        want = po.frame_rows(mode, F, S, nk, bool(circular))
        got = [(f[6 + 3 * i], f[7 + 3 * i]) for i in range(n)]
        assert got == want, line
        assert [f[8 + 3 * i] for i in range(n)] == [po.word(q, S) for _, q in want], line
        seen += 1
    assert seen == 2 * (1 + 3 + 4) * (32 + 48 + 24 + 36)
    assert int(out.split("PASS_PLAN_OK")[1].split()[0]) > 10000
