"""The pure half of the frame report (pysdr_amd/csrc/report_plan.h): pysdr_report_plan through the
library, which needs no device for it, the refusals of the four new calls that come before any device work, and the
scalar transcription in a stand-alone C++ program (tests/report_plan/plan_main.cpp) built and run by tests/plan_program.py,
under AddressSanitizer + UBSan where they are usable, on rings, candidates and floor spans this test writes to files --
both modes, a ring that has wrapped, a circular raster, the raster's and the ring's ends -- whose powers, counts and floors
it compares with the NumPy oracle (tests/report_oracle.py) for equality of every bit.  CPU only; nothing that is loaded into
Python runs under a sanitizer."""
import ctypes as C

import numpy as np
import pytest

from tests import plan_program
from tests import report_oracle as ro

F32 = np.float32


def call(lib, mode):
    out = (C.c_int32 * 4)(*([-7] * 4))
    return lib.pysdr_report_plan(mode, out), list(out)


def test_plan_and_its_refusals(hiplib):
    from pysdr_amd import _lib, ft4, ft8
    assert call(hiplib, 0) == (0, [128, 4400, 79, 4096]) and call(hiplib, 1) == (0, [128, 4400, 103, 4096])
    assert ft8.report_plan() == dict(threads=128, lds_bytes=4400, symbols=79, max_candidates=4096)
    assert ft4.report_plan() == dict(threads=128, lds_bytes=4400, symbols=103, max_candidates=4096)
    assert (ft8.REPORT_MODE, ft4.REPORT_MODE, ft8.REPORT_MAX) == (ro.FT8, ro.FT4, 4096)
    for mode in (-1, 2, 1 << 20):
        assert call(hiplib, mode) == (-1, [-7] * 4) and b"pysdr_report_plan" in hiplib.pysdr_last_error()
        with pytest.raises(_lib.PysdrError):
            ft8.report_plan(mode)
    assert hiplib.pysdr_report_plan(0, None) == -1


def test_the_new_calls_refuse_a_null_skimmer_before_any_device_work(hiplib):
    out = np.full(8, 7.0, F32)
    for kind in ("ft8", "ft4"):
        assert getattr(hiplib, f"pysdr_{kind}_report")(None, None, None, None, 0, None, None) == -1
        assert f"pysdr_{kind}_report".encode() in hiplib.pysdr_last_error()
        assert getattr(hiplib, f"pysdr_{kind}_floor")(None, 0, 1, out.ctypes.data_as(C.POINTER(C.c_float))) == -1
        assert f"pysdr_{kind}_floor".encode() in hiplib.pysdr_last_error() and (out == 7.0).all()


def cases():
    """(mode, ring, nsub, t_done, circular, F, t0, bits91 [n][91], floor spans) -- rings of random powers"""
    from pysdr_amd import ldpc
    rng = np.random.default_rng(26)
    out = []
    for mode, nk, nsub, tr, t_done, circular in ((ro.FT8, 3, 32, 331, 347, False), (ro.FT8, 4, 48, 340, 900, True), (ro.FT8, 2, 32, 355, 314, False),
                                                 (ro.FT4, 3, 24, 425, 470, False), (ro.FT4, 2, 36, 430, 2000, True)):
        nb = nsub + (14 if mode == ro.FT8 else 6)
        ring = (rng.uniform(0.0, 1.0, (nk, tr, nb)) ** 4 * 1e3).astype(F32)
        ring[rng.random(ring.shape) < 0.02] = 0                                # blanked steps give zeros, and ties
        nfine, lag = nk * nsub, ro.lag(mode)
        t_lo, t_hi = max(0, t_done - tr), t_done - lag - 1
        F = [0, nfine - 1, nsub - 1, nsub, 5, 0, nfine - 1, 7] + list(rng.integers(0, nfine, 12))
        t0 = [t_lo, t_hi, t_lo, t_hi, (t_lo + t_hi) // 2, t_hi, t_lo, t_lo + 1] + list(rng.integers(t_lo, t_hi + 1, 12))
        bits = np.array([ldpc.encode(rng.integers(0, 2, 77))[:91] for _ in F])
        bits[3] = 0
        bits[4] = 1
        spans = [(t_done - 1, 1), (t_done - 1, ro.SYMS[mode]), (t_lo + 4 * 78, 79), (t_done - 1, min(128, (tr - 1) // 4 + 1, (t_done - 1) // 4 + 1)),
                 (t_done, 1), (t_done - 1, 129), (t_lo - 1 + 4, 2) if t_lo else (3, 2)]
        out.append((mode, ring, nsub, t_done, circular, np.array(F), np.array(t0), bits, spans))
    return out


def test_the_scalar_transcription_equals_the_oracle(tmp_path, monkeypatch):
    cs = cases()
    paths = []
    for i, (mode, ring, nsub, t_done, circular, F, t0, bits, spans) in enumerate(cs):
        nk, tr, nb = ring.shape
        packed = np.packbits(np.concatenate((bits, np.zeros((len(F), 5), np.int64)), axis=1).astype(np.uint8), axis=1)
        assert packed.shape == (len(F), 12)
        path = tmp_path / f"case{i}.bin"
        with open(path, "wb") as f:
            f.write(np.array([mode, nk, tr, nb, nsub, t_done, int(circular), len(F), len(spans)], np.int32).tobytes())
            f.write(ring.tobytes())
            f.write(F.astype(np.int32).tobytes())
            f.write(t0.astype(np.int64).tobytes())
            f.write(packed.tobytes())
            f.write(np.array(spans, np.int32).tobytes())
        paths.append(str(path))
    monkeypatch.setenv("REPORT_PLAN_CASES", ":".join(paths))
    out = plan_program.run("tests/report_plan/plan_main.cpp", "REPORT_PLAN_OK", tmp_path, extra_flags=("-ffp-contract=off",),
                           includes=("pysdr_amd/csrc",))
    assert f"REPORT_PLAN_OK {len(cs)} cases, {sum(len(c[5]) for c in cs)} candidates, {sum(len(c[8]) for c in cs)} floors" in out
    cand, floors = {}, {}
    for line in out.splitlines():
        f = line.split()
        if line.startswith("CAND "):
            cand[(int(f[1]), int(f[2]))] = (int(f[3]), [int(v, 16) for v in f[4:14]], [int(f[14]), int(f[15])])
        elif line.startswith("FLOOR "):
            floors[(int(f[1]), int(f[2]))] = (int(f[3]), [int(v, 16) for v in f[4:]])
    missing = lost = 0
    for i, (mode, ring, nsub, t_done, circular, F, t0, bits, spans) in enumerate(cs):
        nk, tr, nb = ring.shape
        power, errs = ro.report(ring, t_done, nsub, circular, mode, F, t0, bits)
        for k in range(len(F)):
            mask, pw, er = cand[(i, k)]
            avail = ro.available(mode, int(F[k]), int(t0[k]), t_done, nk * nsub, tr, circular)
            assert mask == sum(1 << p for p in range(9) if avail[p]), (i, k)
            assert pw == [int(v) for v in power[k].view(np.uint32)], (i, k, pw, power[k])
            assert er == [int(v) for v in errs[k]], (i, k)
            missing += int((power[k] == -1).sum())
            lost += int(errs[k].sum())
        for k, (t_end, nsym) in enumerate(spans):
            want = ro.floor(ring, t_done, t_end, nsym)
            ok, got = floors[(i, k)]
            assert ok == (want is not None), (i, k, t_end, nsym)
            if ok:
                assert got == [int(v) for v in want.reshape(-1).view(np.uint32)], (i, k)
        assert [floors[(i, k)][0] for k in range(len(spans))] == [1, 1, 1, 1, 0, 0, 0], i
    print(f"{len(cs)} rings: {missing} missing places, {lost} lost symbols")
    assert missing > 60 and lost > 1000
