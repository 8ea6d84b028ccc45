"""The LDPC decoder's pure half (pysdr_amd/csrc/ldpc_plan.h): pysdr_ldpc_plan through the library, which
needs no device for it, the argument checks of the decode calls, and the tables, the CRC, every refusal, the check update
and the scalar decoder in a stand-alone C++ program (tests/ldpc_plan/plan_main.cpp) built and run by
tests/plan_program.py, under AddressSanitizer + UBSan where they are usable.  CPU only; nothing that is loaded into
Python runs under a sanitizer."""
import ctypes as C

import pytest

from tests import plan_program


def call(lib, cfg):
    out = (C.c_int32 * 4)(*([-7] * 4))
    rc = lib.pysdr_ldpc_plan(None if cfg is None else C.byref(cfg), out)
    return rc, list(out)


def test_plan_and_its_refusals(hiplib):
    from pysdr_amd import _lib, ldpc
    cfg = ldpc.params()
    assert C.sizeof(_lib.LdpcCfg) == 8 and ldpc.cfg_dict(cfg) == dict(iters=30, alpha=0.8125)
    assert call(hiplib, cfg) == (0, [192, 2 * 522 * 4 + 176 + 12, 4096, 30])
    assert ldpc.plan(cfg) == dict(threads=192, lds_bytes=4364, max_candidates=4096, iters=30)
    assert hiplib.pysdr_ldpc_plan(C.byref(cfg), None) == -1
    assert call(hiplib, None) == (-1, [-7] * 4)
    for k, v in (("iters", 0), ("iters", -3), ("iters", 201), ("alpha", 0.0), ("alpha", -0.5), ("alpha", 1.5), ("alpha", float("nan")),
                 ("alpha", float("inf")), ("alpha", float("-inf"))):
        c = ldpc.params()
        setattr(c, k, v)
        assert call(hiplib, c) == (-1, [-7] * 4), (k, v)
        assert b"pysdr_ldpc_plan" in hiplib.pysdr_last_error()
        with pytest.raises(_lib.PysdrError):
            ldpc.plan(c)
    for k, v in (("iters", 1), ("iters", 200), ("alpha", 1.0), ("alpha", 0.75), ("alpha", 1e-30)):
        c = ldpc.params()
        setattr(c, k, v)
        assert call(hiplib, c)[0] == 0, (k, v)


def test_the_decode_calls_check_their_arguments_before_any_device_work(hiplib):
    from pysdr_amd import ldpc
    cfg = ldpc.params()
    for kind in ("ft8", "ft4"):
        assert getattr(hiplib, f"pysdr_{kind}_decode")(None, None, None, 0, C.byref(cfg), None, None, None) == -1
        assert getattr(hiplib, f"pysdr_{kind}_decode_llr")(None, None, 0, C.byref(cfg), None, None, None) == -1
        assert f"pysdr_{kind}_decode_llr".encode() in hiplib.pysdr_last_error()


def test_tables_crc_refusals_check_update_and_the_scalar_decoder(tmp_path):
    out = plan_program.run("tests/ldpc_plan/plan_main.cpp", "LDPC_PLAN_OK", tmp_path, extra_flags=("-ffp-contract=off",),
                           includes=("pysdr_amd/csrc",))
    assert "522 edges, 59 + 24 checks" in out
