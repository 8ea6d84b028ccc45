"""The CPU side of broadcast FM's sweep (tests/wfm_cases.py): the library's own account of the resampler's choice of kernel
(pysdr_resamp_plan: pure arithmetic, no device) confirms that the case table covers every rate of the rate tables, reaches all
three kernels in production and both tap-staging branches of the one-output-per-thread kernel; the oracle's own counters confirm
that every call list holds the ragged calls the table promises; and the oracle's two precisions confirm that the table's
signals make a 1e-5 bar against the float64 master meaningful.  Nothing here measures a kernel: tests/test_gpu_wfm_sweep.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import sdr_oracle as so
from oracle import wfm_oracle as wo
from pysdr_amd.tables import RTLsrates, SDRplaysrates
from tests import wfm_cases as wc

CASE_MODES = [(c, m) for c in wc.CASES for m in wc.MODES]


def case_mode_id(cm):
    return f"{cm[0].name}-{cm[1]}"


def library_params(fs):
    d1, up2, down2 = C.c_int(0), C.c_int(0), C.c_int(0)
    from pysdr_amd import _lib
    _lib.check(_lib.lib().pysdr_wfm_params(float(fs), wc.FS_OUT, C.byref(d1), C.byref(up2), C.byref(down2)), "pysdr_wfm_params")
    return d1.value, up2.value, down2.value


def uncovered(cases):
    """(d1 == 1, UP2, DOWN2) of the rate tables that no ratio case of ``cases`` has."""
    have = {(wc.shape(c).d1 == 1, wc.shape(c).up2, wc.shape(c).down2) for c in cases}
    need = set()
    for mhz in RTLsrates + SDRplaysrates:
        d1, up2, down2 = library_params(mhz * 1e6)
        need.add((d1 == 1, up2, down2))
    return need - have


def test_every_rate_of_the_rate_tables_has_a_ratio_case(hiplib):
    for mhz in sorted(set(RTLsrates + SDRplaysrates + [c.fs / 1e6 for c in wc.CASES])):
        fs = mhz * 1e6
        d1, up2, down2 = library_params(fs)
        assert d1 == wo.wfm_if_decim(fs) and (up2, down2) == so.up_dn(fs / d1, so.chunk_sizes(fs, wc.FS_OUT)[2]), mhz
        assert (d1, up2, down2) == wc.shape(fs)[:1] + wc.shape(fs)[2:4]
    assert uncovered(wc.RATIO_CASES) == set()
    # ... and the check has teeth: a ratio of the tables taken out is missed (16/75 and 25/128 come from rates outside them)
    by = {c.name: c for c in wc.RATIO_CASES}
    for drop, miss in (("24_125", (False, 24, 125)), ("3_16", (False, 3, 16)), ("6_25", (False, 6, 25)), ("1_5", (False, 1, 5)),
                       ("24_125-d1_1", (True, 24, 125))):
        assert uncovered([c for c in wc.RATIO_CASES if c is not by[drop]]) == {miss}
    # the ratios the issue names, each under its own name
    assert {c.name: wc.shape(c)[2:4] for c in wc.RATIO_CASES} == {
        "24_125": (24, 125), "3_16": (3, 16), "6_25": (6, 25), "1_5": (1, 5), "16_75": (16, 75), "25_128": (25, 128),
        "24_125-d1_1": (24, 125)}
    assert wc.shape(by["24_125-d1_1"]).d1 == 1 and all(wc.shape(c).d1 > 1 for c in wc.RATIO_CASES if c.name != "24_125-d1_1")


@pytest.mark.parametrize("case", wc.CASES, ids=lambda c: c.name)
def test_case_reaches_the_kernels_it_names(hiplib, case):
    assert tuple(k for _, k in wc.reachable(case)) == case.kernels
    s = shape = wc.shape(case)
    kpad = -(-case.k // 16) * 16
    for plain, kernel in wc.reachable(case):
        p = wc.query(case, plain)
        assert (p.kernel, p.kpad, p.hist_len) == (kernel, kpad, kpad + 2), p
        # what the launch asks of the device, from the kernels' own indexing (resamp_small.hip)
        if kernel == wc.WAVE:
            assert p.threads == 64 * ((s.up2 + 1) // 2) <= 1024 and p.tile_out == 64 * s.up2
            assert p.lds == 8 * (p.span + p.tile_out) <= 78 * 1024
        elif kernel == wc.HALF:
            assert p.threads == 32 * s.up2 <= 1024 and p.tile_out == 32 * s.up2 and p.span <= 6 * p.threads
            assert p.lds == 8 * (p.span + p.tile_out + s.up2 * (kpad + 1)) <= 64 * 1024
        else:
            assert p.threads == 256 and p.tile_out == 256 and p.lds == 8 * (p.span + s.up2 * (kpad + 1)) <= 60 * 1024
        # a tile's input span fits: its outputs reach back kpad - 1 samples from floor((t0 + i DOWN) / UP), t0 < DOWN
        assert p.span >= ((p.tile_out - 1) * s.down2 + s.up2 - 1) // s.up2 + kpad
    assert shape.L <= 131072


def test_all_three_kernels_and_both_staging_branches_are_reached_in_production(hiplib):
    production = {}
    for c in wc.CASES:
        production.setdefault(wc.query(c, 0).kernel, []).append(c.name)
        assert wc.query(c, 0).kernel == c.kernels[0]
    # each of the three is some case's production kernel (PYSDR_RESAMP_PLAIN = 0) ...
    assert sorted(production) == [wc.WAVE, wc.THREAD, wc.HALF], production
    assert "1_5" in production[wc.THREAD] and "25_128-k192" in production[wc.THREAD] and production[wc.HALF] == ["25_131"]
    # ... and no rate of the rate tables is the half-wave form's: that takes the rate outside them
    for mhz in RTLsrates + SDRplaysrates:
        _, up2, down2 = library_params(mhz * 1e6)
        assert wc.query((up2, down2, 64 * up2), 0).kernel in (wc.WAVE, wc.THREAD), mhz
    # both tap-staging branches of resamp_small_kernel: 256 % kpad == 0 and != 0, in production and on request
    staging = {(256 % wc.query(c, wc.plain_for(c, wc.THREAD)).kpad == 0, wc.plain_for(c, wc.THREAD) == 0)
               for c in wc.CASES if wc.THREAD in c.kernels}
    assert staging == {(True, True), (True, False), (False, True), (False, False)}
    # the eligibility edges of 25/128 as the table's docstring states them
    assert [wc.query((25, 128, 25 * k), 0).kernel for k in (176, 177, 192)] == [wc.WAVE, wc.THREAD, wc.THREAD]
    assert wc.query((25, 128, 25 * 176), 0).lds == 79776 and not wc.query((25, 128, 25 * 256), 0).eligible
    assert wc.query((1, 5, 64), 0).kernel == wc.query((1, 5, 64), 2).kernel == wc.THREAD


def test_the_plan_checks_its_arguments(hiplib):
    out = (C.c_int32 * 8)()
    ok = [24, 125, 24 * 64, 0]
    assert hiplib.pysdr_resamp_plan(*ok, out) == 0 and list(out)[:3] == [1, wc.WAVE, 768]
    for pos, bad in ((0, 0), (1, 0), (2, 0), (3, -1), (3, 3)):
        args = list(ok)
        args[pos] = bad
        assert hiplib.pysdr_resamp_plan(*args, out) == -1, (pos, bad)
    assert hiplib.pysdr_resamp_plan(*ok, None) == -1
    assert hiplib.pysdr_get_resamp_tuning(None, (C.c_int32 * 2)()) == -1
    # a shape the form does not take is reported, not planned
    assert hiplib.pysdr_resamp_plan(3, 625, 255, 0, out) == 0 and list(out)[:2] == [0, -1]


def test_the_held_launch_walks_several_tiles_per_workgroup(hiplib):
    """PYSDR_MIXDEC_GRID = 3: in the case's longest call every workgroup of every kernel walks at least two tiles, so the
    half-wave form fetches a NEXT tile into registers (resamp_branch_kernel: nxt < ntiles) -- which the ragged list alone,
    2049 outputs at most, would not make it do."""
    held = [c for c in wc.CASES if c.grid]
    assert [c.name for c in held] == ["24_125-grid3"]
    for case in held:
        s = wc.shape(case)
        longest = max(c.nout for c in wc.count_calls(wc.calls_of(case), s)[0])
        ragged = max(c.nout for c in wc.count_calls(wc.ragged_calls(s.L), s)[0])
        for plain, kernel in wc.reachable(case):
            tile = wc.query(case, plain).tile_out
            assert -(-longest // tile) >= 2 * case.grid + 2, (kernel, longest, tile)
        assert -(-ragged // wc.query(case, wc.plain_for(case, wc.HALF)).tile_out) <= case.grid


@functools.lru_cache(maxsize=None)
def oracle_runs(name, mode):
    case = wc.BY_NAME[name]
    x, calls = wc.stream(case), wc.calls_of(case)
    return wc.run_oracle(case, mode, x, calls, np.float64), wc.run_oracle(case, mode, x, calls, np.float32)


@pytest.mark.parametrize("cm", CASE_MODES, ids=case_mode_id)
def test_call_list_holds_every_ragged_call(cm):
    """Counted with the oracle's own counters (its decimators' sample counts, the lengths it returns) in both precisions, and
    equal to the table's arithmetic."""
    case, mode = cm
    s, calls = wc.shape(case), wc.calls_of(case)
    hist_len = -(-case.k // 16) * 16 + 2
    nb = 7 + (1 if case.long_chunks else 0)                # the ragged list (and the long call of the held launch)
    assert calls[:7] == wc.ragged_calls(s.L) and 2 <= len(calls) - nb <= 5
    assert sum(calls) <= 6 * 131072
    for _, counts in oracle_runs(case.name, mode):
        assert counts == wc.count_calls(calls, s)[0]
        have = set().union(*(wc.properties_of(c, s, hist_len) for c in counts))
        assert have >= wc.wanted(s), (case.name, wc.wanted(s) - have)
        assert wc.wanted(s) == set(wc.PROPERTIES) - ({"n1_zero"} if s.d1 == 1 else set())
        # a call of one to five IF samples; a call without IF samples is followed by one with some (whose first
        # discriminator sample needs the history the empty call had to hand on)
        assert any(1 <= c.n1 <= 5 for c in counts)
        # the list closes on outputs, and (at the designed 64 taps per branch) their windows reach back over every added call
        assert counts[-1].nout >= wc.CLOSING_OUTPUTS and counts[-1].n1 > 0
        assert case.k < 64 or sum(c.n1 for c in counts[nb:-1]) < case.k
        if s.d1 > 1:
            assert any(a.n1 == 0 and b.n1 > 0 for a, b in zip(counts, counts[1:]))
            assert any(p.n1 > 0 and a.n1 == 0 for p, a in zip(counts, counts[1:]))


@pytest.mark.parametrize("cm", CASE_MODES, ids=case_mode_id)
def test_float32_mirror_stays_within_a_quarter_of_the_bar_of_the_master(cm):
    """The condition that makes ``TOL`` against the float64 master a statement about the kernels: on this case's signal the
    oracle's own float32 form is within TOL / 4 = 2.5e-6 of it, on the resampler's output and on the audio, over the
    concatenated stream with the stream's own peak as scale -- exactly as the GPU sweep judges the kernels."""
    case, mode = cm
    (m64, _), (m32, _) = oracle_runs(case.name, mode)
    e_iq = wc.relerr(wc.cat(m32, 0), wc.cat(m64, 0))
    e_am = wc.relerr(wc.cat(m32, 1), wc.cat(m64, 1))
    print(f"WFM-COND {case.name} {mode}: float32 vs float64 oracle iq {e_iq:.2e} am {e_am:.2e}")
    assert e_iq <= wc.COND and e_am <= wc.COND, (e_iq, e_am)
