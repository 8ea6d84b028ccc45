"""Broadcast FM on ragged calls against the float64 master: every case of tests/wfm_cases.py, mono and stereo, on every kernel
of the audio resampler the case names.

tests/test_wfm_cases.py proves on any machine that the table covers every ratio of the rate tables, all three kernels and both
tap-staging branches, and that every call list holds a call without IF samples, a short call without output, a call of one
output, an odd start and a call above two chunks.  Here every (case, mode, kernel) runs on the GPU, and before it runs the
library is asked (pysdr_resamp_plan under the tuning the live context reports) that the context really launches the kernel the
test is named after: the test ids are the record of what ran.

The bar is the project's own, 1e-5, on EVERY sample of the resampler's output (``iq``) and of the audio from the first one,
over the whole stream with the master's peak over the stream as scale (a call of one to seven outputs has no peak of its own);
the float32 mirror follows the master to 1e-6 on these signals (the conditioning test of tests/test_wfm_cases.py).  Per-call
output counts equal the master's.  The kernels of a case sum every output in the same order: bit for bit the same; and the
overlapped form (pysdr_set_overlap) changes when kernels run, never what they compute: bit for bit the single-stream result."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import wfm_cases as wc

pytestmark = pytest.mark.gpu

TOL = wc.TOL

RUNS = [(c, m, k) for c in wc.CASES for m in wc.MODES for k in c.kernels]
CASE_MODES = [(c, m) for c in wc.CASES for m in wc.MODES]
OVERLAPPED = [(c, m) for c in wc.RATIO_CASES + wc.EXTRA_CASES for m in wc.MODES]


def run_id(r):
    return "-".join([r[0].name, r[1]] + [wc.KERNEL_NAMES[k] for k in r[2:]])


@functools.lru_cache(maxsize=4)
def case_data(name, mode):
    """The case's stream and what the float64 master makes of its calls (made once per case and mode)."""
    case = wc.BY_NAME[name]
    x, calls = wc.stream(case), wc.calls_of(case)
    master, counts = wc.run_oracle(case, mode, x, calls, np.float64)
    for _, am in master:
        am.setflags(write=False)
    return SimpleNamespace(case=case, mode=mode, x=x, calls=calls, master=master, counts=counts,
                           iq=wc.cat(master, 0), am=wc.cat(master, 1))


@functools.lru_cache(maxsize=None)
def gpu_run(name, mode, kernel, overlap=0, grid=None):
    """The case's calls through one context, one process_batch(x, 1, n) and a fetch per call.  -> per call (iq, am); the run is
    made once and shared by the tests that compare it (kept: a stream is about 6000 outputs).  ``grid`` overrides the case's."""
    from pysdr_amd import _lib
    d = case_data(name, mode)
    case = d.case
    want_grid = case.grid if grid is None else grid
    g, ctx = wc.make_gpu_receiver(case, mode, wc.plain_for(case, kernel), overlap, max(d.calls), grid=want_grid)
    try:
        plan, got_grid = wc.context_plan(ctx.h, case)
        assert plan.eligible and plan.kernel == kernel and got_grid == want_grid, (name, plan, got_grid)
        per, pos = [], 0
        for n in d.calls:
            ctx.process_batch(d.x[pos:pos + n], 1, n, on_device=False)
            assert _lib.lib().pysdr_last_call_overlapped(ctx.h) == (1 if overlap else 0)
            am, iq, cn, _ = ctx.fetch(0, 1)
            assert len(am) == len(iq) == int(cn.sum())
            per.append((iq.copy(), am.copy()))
            pos += n
    finally:
        ctx.close()
    return per


def check_against_master(d, per, what):
    """Counts per call, then every sample of the stream.  -> (worst iq, worst audio)."""
    assert [len(iq) for iq, _ in per] == [c.nout for c in d.counts], what
    assert [len(am) for _, am in per] == [c.nout for c in d.counts], what
    iq, am = wc.cat(per, 0), wc.cat(per, 1)
    assert am.dtype == (np.complex64 if d.mode == 'WFM2' else np.float32)
    e_iq, e_am = wc.relerr(iq, d.iq), wc.relerr(am, d.am)
    print(f"WFM-SWEEP {what}: iq {e_iq:.2e} am {e_am:.2e}")
    if e_iq > TOL or e_am > TOL:
        # where it went wrong: the first call whose own samples miss the bar
        s_iq, s_am = np.max(np.abs(d.iq)), np.max(np.abs(d.am))
        for j, ((giq, gam), (miq, mam)) in enumerate(zip(per, d.master)):
            if len(miq) and max(np.max(np.abs(giq - miq)) / s_iq, np.max(np.abs(gam - mam)) / s_am) > TOL:
                print(f"WFM-SWEEP {what}: first miss in call {j} {d.counts[j]}: iq {np.max(np.abs(giq - miq)) / s_iq:.2e} "
                      f"am {np.max(np.abs(gam - mam)) / s_am:.2e}, first sample {int(np.argmax(np.abs(giq - miq) / s_iq > TOL))}")
                break
    assert e_iq <= TOL, (what, 'iq', e_iq)
    assert e_am <= TOL, (what, 'am', e_am)
    return e_iq, e_am


def same_bits(a, b, what):
    assert len(a) == len(b), what
    for j, ((iq1, am1), (iq2, am2)) in enumerate(zip(a, b)):
        assert iq1.shape == iq2.shape and am1.shape == am2.shape, (what, j)
        assert np.array_equal(iq1.view(np.uint32), iq2.view(np.uint32)), (what, 'iq', j)
        assert np.array_equal(am1.view(np.uint32), am2.view(np.uint32)), (what, 'am', j)


@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_every_sample_against_the_float64_master(run):
    case, mode, kernel = run
    check_against_master(case_data(case.name, mode), gpu_run(case.name, mode, kernel), run_id(run))


@pytest.mark.parametrize("cm", [cm for cm in CASE_MODES if len(cm[0].kernels) > 1], ids=run_id)
def test_the_kernels_of_a_case_agree_bit_for_bit(cm):
    case, mode = cm
    first = gpu_run(case.name, mode, case.kernels[0])
    for k in case.kernels[1:]:
        same_bits(gpu_run(case.name, mode, k), first, f"{run_id(cm)}: {wc.KERNEL_NAMES[k]} against {wc.KERNEL_NAMES[case.kernels[0]]}")


def test_the_held_launch_agrees_with_the_free_one_bit_for_bit():
    """PYSDR_MIXDEC_GRID = 3 changes which workgroup walks which tile, never a sum: the same calls with the launch left free."""
    for mode in wc.MODES:
        for k in wc.BY_NAME["24_125-grid3"].kernels:
            same_bits(gpu_run("24_125-grid3", mode, k), gpu_run("24_125-grid3", mode, k, grid=0), f"grid3 {mode} {wc.KERNEL_NAMES[k]}")


@pytest.mark.parametrize("cm", OVERLAPPED, ids=run_id)
def test_overlapped_calls_equal_single_stream_bit_for_bit(cm):
    """pysdr_set_overlap 1 for WFM2 (the default of a batch context) and 2 for WFM (form 1 leaves mono single-stream): the
    buffer pairs flip on every call, so whatever a call hands to the next one must cross to the other buffer -- also from a
    call without a single IF sample, which starts no discriminator kernel (launch_wfm_disc carries the IF history then)."""
    case, mode = cm
    d = case_data(case.name, mode)
    kernel = case.kernels[0]
    over = gpu_run(case.name, mode, kernel, 1 if mode == 'WFM2' else 2)
    what = f"{run_id(cm)} overlapped"
    check_against_master(d, over, what)
    same_bits(over, gpu_run(case.name, mode, kernel), what)
