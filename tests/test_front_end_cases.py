"""The CPU side of the front end's sweep (tests/front_end_cases.py): the library's own account of its decision
(pysdr_front_end_plan / pysdr_front_end_shapes: pure arithmetic, no device) confirms that the case table reaches every compiled
instantiation, and the oracle's two precisions confirm that the table's signals make a 1e-5 bar against the float64 master
meaningful.  Nothing here measures a kernel: that is tests/test_gpu_front_end_sweep.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import sdr_oracle as so
from tests import front_end_cases as fc


def uncovered(cases):
    """Compiled entries that no case of ``cases`` selects under the default tuning."""
    vec, mm = fc.compiled()
    hit = {fc.selected(fc.query(c)) for c in cases}
    return (set(vec) | {('m', i) for i in mm}) - hit


def test_every_compiled_instantiation_has_a_case(hiplib):
    vec, mm = fc.compiled()
    assert len(vec) >= 30 and len(mm) >= 7 and len(set(vec)) == len(vec)
    assert uncovered(fc.CASES) == set()
    # ... and the check has teeth: any case taken out leaves its instantiation without one
    for drop in (fc.CASES[0], fc.CASES[12], fc.CASES[19], fc.CASES[-1]):
        assert uncovered([c for c in fc.CASES if c is not drop]) == {drop.expect}


@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.name)
def test_case_selects_the_instantiation_it_is_named_after(hiplib, case):
    p = fc.query(case)
    assert p.fits and fc.selected(p) == case.expect, p
    if case.expect[0] == 'v':
        assert p.form == fc.FORM_VECTOR and p.key[0] == case.nrx
        assert p.tile_out >= 2 and p.tile_out % 2 == 0 and p.yflush >= 1 and p.kpad % 16 == 0
        # the matrix-core instantiations run only with their taps held in registers
        assert p.taps_lds == (0 if p.key[3] else 1)
    else:
        _, mm = fc.compiled()
        up, down = so.chunk_sizes(case.fs, fc.FS_OUT)[:2]
        assert mm[p.mshape] == (up, down, -(-case.ntaps // up))


def test_the_query_follows_the_tuning(hiplib):
    """The switches that change the form: PYSDR_MIXDEC_MFMA=0 sends the matrix-core rates to the vector form; any thread count
    but 1024 and any tile whose outputs are no multiple of UP send the multi-RX matrix-core shapes to the generic
    instantiation with the taps in LDS; the small resampler takes a short single-RX prototype only where no raw peak is wanted."""
    for c in fc.MFMA_CASES:
        p = fc.query(c, mfma_enable=0)
        assert p.form == fc.FORM_VECTOR and p.fits and p.key[0] == 1 and p.key[2:] == (1024, 0) and p.taps_lds == 1, (c.name, p)
    ft8tri = fc.BY_NAME["8M1001x3-v3.21.768.1"]
    assert fc.query(ft8tri).key == (3, 21, 768, 1) and fc.query(ft8tri).taps_lds == 0
    for tuning in (dict(threads=768), dict(threads=256), dict(tile_bytes=12288)):
        p = fc.query(ft8tri, **tuning)
        assert p.key == (3, 0, 1024, 0) and p.taps_lds == 1 and p.fits, (tuning, p)
    assert fc.query(ft8tri, tile_bytes=12288).tile_out % 3 != 0
    # broadcast FM's audio stage, 250 kHz -> 48 kHz with 64 taps per branch: the small resampler without the raw peak
    assert fc.query((1, 24, 125, 24 * 64), want_peak=0).form == fc.FORM_SMALL
    assert fc.query((1, 24, 125, 24 * 64), want_peak=1).form == fc.FORM_VECTOR
    assert fc.query((1, 24, 125, 24 * 64), want_peak=1).key == (1, 4, 1024, 0)
    assert fc.query((2, 24, 125, 24 * 64), want_peak=0).form == fc.FORM_VECTOR
    # two workgroups per CU halve the LDS share: smaller tiles, same instantiation
    one, two = fc.query(fc.CASES[0]), fc.query(fc.CASES[0], wgs_per_cu=2)
    assert two.key == one.key and two.tile_out < one.tile_out
    assert fc.query(fc.CASES[0], yflush_cap=2).yflush == 2


def test_the_query_checks_its_arguments(hiplib):
    out = (C.c_int32 * 12)()
    ok = [1, 3, 500, 255, 0, 1024, 1, 0, 1, 1]
    assert hiplib.pysdr_front_end_plan(*ok, out) == 0
    for pos, bad in ((0, 0), (0, 9), (1, 0), (2, 0), (3, 0), (4, 100), (4, 200 * 1024), (5, 0), (5, 1000), (5, 2048), (6, 0), (7, -1)):
        args = list(ok)
        args[pos] = bad
        assert hiplib.pysdr_front_end_plan(*args, out) == -1, (pos, bad)
    assert hiplib.pysdr_front_end_plan(*ok, None) == -1
    n = C.c_int(0)
    o4 = (C.c_int32 * 4)()
    assert hiplib.pysdr_front_end_shapes(0, -1, None, C.byref(n)) == 0 and n.value >= 30
    assert hiplib.pysdr_front_end_shapes(0, n.value, o4, None) == -1
    assert hiplib.pysdr_front_end_shapes(2, 0, o4, None) == -1
    assert hiplib.pysdr_front_end_shapes(1, 0, None, None) == -1
    # a prototype that cannot fit the LDS of a workgroup is reported, not planned
    assert not fc.query((8, 1, 4, 4001)).fits


@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.name)
def test_float32_mirror_stays_within_a_quarter_of_the_bar_of_the_master(case):
    """The condition that makes ``TOL`` against the float64 master a statement about the kernels: on this case's signal
    the oracle's own float32 form is within TOL / 4 = 2.5e-6 of it, on the baseband IQ and on the audio of every call of the
    ragged list.  (A case that misses gets another input, not another bound.)"""
    cfg = fc.case_cfg(case)
    calls = fc.ragged_calls(fc.chunk_len(case))
    x = so.synth_iq(cfg, sum(calls), 57)
    m64, m32 = fc.run_oracle(cfg, x, calls, np.float64), fc.run_oracle(cfg, x, calls, np.float32)
    worst_iq = worst_am = 0.0
    for r in range(case.nrx):
        for (iq64, am64), (iq32, am32) in zip(m64[r], m32[r]):
            # per call and relative to the call's own peak, exactly as the GPU sweep judges the kernels
            worst_iq = max(worst_iq, fc.relerr(iq32, iq64))
            worst_am = max(worst_am, fc.relerr(am32, am64))
    print(f"{case.name}: float32 vs float64 oracle iq {worst_iq:.2e} am {worst_am:.2e}")
    assert worst_iq <= fc.COND and worst_am <= fc.COND, (worst_iq, worst_am)
