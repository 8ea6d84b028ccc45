"""Every compiled instantiation of the mix + decimate front end against the float64 master of the oracle.

The case table (tests/front_end_cases.py) holds one operating point per entry of PYSDR_MIXDEC_SHAPES (30) and of
PYSDR_MFMA_SHAPES (7); tests/test_front_end_cases.py proves on any machine that the table is complete.  Here every case
runs on the GPU, and before it runs the library is asked (pysdr_front_end_plan, with the tuning the live context reports)
that the context really takes the instantiation the case is named after: the test ids are the record of what ran.

The bar is the project's own: 1e-5 of the output peak, per sub-receiver and per call, on EVERY sample of the baseband IQ
and of the audio -- against the float64 oracle, which the float32 mirror follows to 1e-6 on these signals (the conditioning
test of tests/test_front_end_cases.py)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import sdr_oracle as so
from tests import front_end_cases as fc
from tests import test_gpu_parity as tp

pytestmark = pytest.mark.gpu

TOL = fc.TOL
SEED = 57
BATCH = 5            # chunks of the bit-for-bit identities (the ragged list is 5 chunks + 1332 samples: one stream serves both)


@functools.lru_cache(maxsize=2)
def case_data(name):
    """The case's stream and what the float64 master makes of the ragged call list."""
    case = fc.BY_NAME[name]
    cfg = fc.case_cfg(case)
    L = fc.chunk_len(case)
    calls = fc.ragged_calls(L)
    assert BATCH * L <= sum(calls)
    x = so.synth_iq(cfg, sum(calls), SEED)
    master = fc.run_oracle(cfg, x, calls, np.float64)
    up, down = so.chunk_sizes(case.fs, fc.FS_OUT)[:2]
    n_batch = -(-BATCH * L * up // down)                  # outputs of the first BATCH chunks (output m exists once sample floor(m DOWN / UP) does)
    iq_batch = [np.concatenate([iq for iq, _ in per])[:n_batch] for per in master]
    return SimpleNamespace(case=case, cfg=cfg, L=L, calls=calls, x=x, master=master, iq_batch=iq_batch, up=up, down=down)


@pytest.fixture(scope="module", params=fc.CASES, ids=lambda c: c.name)
def data(request):
    # (module scope: pytest runs all tests of one case together, so its stream and master are made once)
    return case_data(request.param.name)


def hold_grid(monkeypatch, grid):
    """The existing idiom: the launch held to ``grid`` workgroups, so that each walks many tiles (the output stage's flush
    cadence, the add-only steady runs, peaks carried over chunk boundaries)."""
    if grid:
        monkeypatch.setenv("PYSDR_TUNING", "1")
        monkeypatch.setenv("PYSDR_MIXDEC_GRID", str(grid))


def assert_runs_on(P, case, expect, taps_lds=None):
    """The live context's tuning selects ``expect``, by the library's own account."""
    plan = fc.query(case, **fc.context_tuning(P._pysdr_stream.h))
    assert plan.fits and fc.selected(plan) == expect, (case.name, plan)
    if taps_lds is not None:
        assert plan.taps_lds == taps_lds, (case.name, plan)
    return plan


def run_against_master(d, expect=None, tile=None, taps_lds=None):
    """The ragged call list through one context: per sub-receiver and per call relerr(iq) and relerr(audio) <= TOL against the
    master, every sample; the raw chunk peak is NumPy's maximum.  -> (worst iq, worst audio, the plan that ran)."""
    from pysdr_amd import _lib
    P, g = tp.make_gpu_receivers(d.cfg, max_batch_chunks=-(-max(d.calls) // d.L))
    if tile:
        _lib.check(_lib.lib().pysdr_set_tile(P._pysdr_stream.h, *tile), "pysdr_set_tile")
    plan = assert_runs_on(P, d.case, d.case.expect if expect is None else expect, taps_lds)
    pos, w_iq, w_am = 0, 0.0, 0.0
    for k, c in enumerate(d.calls):
        xc = d.x[pos:pos + c]
        pos += c
        for i, rg in enumerate(g):
            am_g = rg.demod_data(xc)
            iq_m, am_m = d.master[i][k]
            e_iq, e_am = fc.relerr(rg.iq, iq_m), fc.relerr(am_g, am_m)
            w_iq, w_am = max(w_iq, e_iq), max(w_am, e_am)
            assert e_iq <= TOL, (d.case.name, i, k, 'iq', e_iq)
            assert e_am <= TOL, (d.case.name, i, k, 'am', e_am)
            want_pk = np.max(np.abs(xc.astype(np.complex128)) ** 2)
            assert abs(float(rg.peak_in) - want_pk) <= 1e-6 * want_pk, (d.case.name, i, k, rg.peak_in, want_pk)
    return w_iq, w_am, plan


@pytest.mark.parametrize("grid", [0, 3])
def test_every_sample_against_the_float64_master(data, grid, monkeypatch):
    hold_grid(monkeypatch, grid)
    w_iq, w_am, plan = run_against_master(data)
    print(f"SWEEP parity {data.case.name} grid {grid}: iq {w_iq:.2e} am {w_am:.2e} form {plan.form} key {plan.key} "
          f"mshape {plan.mshape} taps_lds {plan.taps_lds} tile_out {plan.tile_out} yflush {plan.yflush}")


@pytest.mark.parametrize("grid", [0, 3])
def test_one_batch_equals_chunk_by_chunk_equals_random_cuts(data, grid, monkeypatch):
    """The body of test_gpu_parity.test_multi_rx_long_prototype_does_not_depend_on_the_cut, for every instantiation."""
    hold_grid(monkeypatch, grid)
    P, worst = tp.check_does_not_depend_on_the_cut(data.cfg, B=BATCH, x=data.x[:BATCH * data.L], want_iq=data.iq_batch)
    assert_runs_on(P, data.case, data.case.expect)
    print(f"SWEEP cut {data.case.name} grid {grid}: iq {worst:.2e}")


def test_device_batch_at_an_odd_sample_offset(data):
    """The body of test_gpu_parity.test_device_batch_at_an_odd_sample_offset, for every instantiation: the vector form then
    stages every tile through its generic path (aligned16 = 0) instead of whole LDS-DMA pieces."""
    buf = np.concatenate((np.zeros(1, np.complex64), data.x[:BATCH * data.L]))     # the batch starts 8 bytes into the buffer
    P, worst = tp.check_device_batch_at_an_odd_sample_offset(data.cfg, buf, BATCH, want_iq=data.iq_batch)
    assert_runs_on(P, data.case, data.case.expect)
    print(f"SWEEP odd {data.case.name}: iq {worst:.2e}")


# ---- thread counts and the small tile -------------------------------------------------------------------------------------------
# (tile_bytes, threads) -> what the library says the combination runs: (instantiation, taps_lds).  The table documents the
# demotions: any thread count but 1024 sends a shape with a special instantiation at 1001 taps to the generic one (md_select
# keys them on threads == 1024), while the 255-tap, 63-tap and one-branch shapes keep theirs and only clamp their waves; the
# small tile leaves 4 outputs per tile at UP = 3 (no multiple of UP: the matrix-core shapes cannot hold their taps and take
# the generic instantiation) but 6 at UP = 6, where <R,11,768,1> stays.
SMALL_TILE = (12288, 1024)
THREADS = [(0, 256), (0, 512), (0, 768)]


def _same(case):
    return {t: (case.expect[1], 1) for t in THREADS + [SMALL_TILE]}


def _generic_below_1024(case, small):
    g = ((case.nrx, 0, 1024, 0), 1)
    return {**{t: g for t in THREADS}, SMALL_TILE: small}


TILE_SUBSET = {}
for _n in ["8M255x5-v5.6.1024.0", "8M255x6-v6.6.1024.0", "8M255x7-v7.6.1024.0", "8M255x8-v8.6.1024.0",          # every R >= 5 of the
           "3M1001x5-v5.0.1024.0", "3M1001x6-v6.0.1024.0", "3M1001x7-v7.0.1024.0", "3M1001x8-v8.0.1024.0",      # two 1024-thread families
           "8M1001x1-v1.21.1024.0", "2M4x255x1-v1.16.1024.0", "6M144x63x1-v1.4.1024.0"]:
    TILE_SUBSET[_n] = _same(fc.BY_NAME[_n])
TILE_SUBSET["7M1001x1-v1.11.1024.0"] = _generic_below_1024(fc.BY_NAME["7M1001x1-v1.11.1024.0"], ((1, 11, 1024, 0), 1))
TILE_SUBSET["7M1001x3-v3.11.768.1"] = _generic_below_1024(fc.BY_NAME["7M1001x3-v3.11.768.1"], ((3, 11, 768, 1), 0))
TILE_SUBSET["8M1001x5-v5.21.512.1"] = _generic_below_1024(fc.BY_NAME["8M1001x5-v5.21.512.1"], ((5, 0, 1024, 0), 1))


@pytest.mark.parametrize("tile", THREADS + [SMALL_TILE], ids=lambda t: f"tile{t[0]}-threads{t[1]}")
@pytest.mark.parametrize("name", sorted(TILE_SUBSET))
def test_thread_counts_and_the_small_tile(name, tile):
    d = case_data(name)
    key, taps_lds = TILE_SUBSET[name][tile]
    w_iq, w_am, plan = run_against_master(d, expect=('v', key), tile=tile, taps_lds=taps_lds)
    print(f"SWEEP tile {name} {tile}: iq {w_iq:.2e} am {w_am:.2e} key {plan.key} taps_lds {plan.taps_lds} tile_out {plan.tile_out}")


# ---- the matrix-core rates on the vector form ----------------------------------------------------------------------------------
MFMA_OFF = {0: (1, 21, 1024, 0), 1: (1, 16, 1024, 0), 2: (1, 21, 1024, 0), 3: (1, 21, 1024, 0), 4: (1, 21, 1024, 0),
            5: (1, 0, 1024, 0), 6: (1, 0, 1024, 0)}      # 1001 taps in ONE branch (kpad 1008) have no unrolled tap loop


@pytest.mark.parametrize("case", fc.MFMA_CASES, ids=lambda c: c.name)
def test_matrix_core_rates_on_the_vector_form(case, monkeypatch):
    monkeypatch.setenv("PYSDR_TUNING", "1")
    monkeypatch.setenv("PYSDR_MIXDEC_MFMA", "0")
    w_iq, w_am, plan = run_against_master(case_data(case.name), expect=('v', MFMA_OFF[case.expect[1]]), taps_lds=1)
    print(f"SWEEP mfma-off {case.name}: iq {w_iq:.2e} am {w_am:.2e} key {plan.key}")


# ---- a non-finite input sample on the multi-RX forms ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["8M255x5-v5.6.1024.0", "3M1001x3-v3.0.1024.0", "7M1001x3-v3.11.768.1", "8M1001x3-v3.21.768.1",
                                  "8M1001x5-v5.21.512.1"])
def test_non_finite_input_on_the_multi_rx_forms(name):
    """One NaN sample x[j] in the middle of a batch.  What it may reach, from the geometry (mixdec.hip):

      y[m] = rot(m) * sum_{k = 0 .. kpad-1} g[p_m][k] * x[n_m - k],   n_m = floor(m DOWN / UP),

    with the taps zero-padded from kdec = ceil(ntaps / UP) to kpad = 16 ceil(kdec / 16) per branch.  The kernels multiply the
    padding too (0 * NaN = NaN), so output m is non-finite iff  n_m - kpad < j <= n_m  -- the oracle's set is the same with
    kdec for kpad, hence a subset.  Nothing else can be reached: in the vector form a DPP row of 16 lanes IS one output and
    only its own sum is folded across the row; in the matrix-core form (v_mfma_f32_4x4x1, K = 1: sixteen independent outer
    products) row i of every block is fed by output i's window alone, and the fold (row rotations, permlane swaps) adds blocks,
    never rows -- so the other three outputs of a quad stay clean even though they share the instruction.  The LO rotation and
    the output stage are per output.  So: the non-finite outputs of every sub-receiver lie inside that window and
    contain the oracle's; everything else is bit-identical to the clean run; the next call on the same context is bit-identical
    to a clean context's (the history holds samples, not sums: once x[j] has left it, it is gone)."""
    d = case_data(name)
    cfg, L, B = d.cfg, d.L, 4
    x = d.x[:B * L]
    xn = x.copy()
    # the newest sample of an output in the middle of the third chunk (at 3/500 with 85 taps per branch most samples are in
    # no output's window at all)
    j = int(-(-(2 * L + 12345) * d.up // d.down) * d.down // d.up)
    xn[j] = np.complex64(complex(np.nan, 0.0))
    P1, g1 = tp.make_gpu_receivers(cfg, max_batch_chunks=B)
    plan = assert_runs_on(P1, d.case, d.case.expect)
    P2, g2 = tp.make_gpu_receivers(cfg, max_batch_chunks=B)
    P1._pysdr_stream.process_batch(x, B, L, on_device=False)
    clean = [P1._pysdr_stream.fetch(i, B)[1].copy() for i in range(len(g1))]
    P1._pysdr_stream.process_batch(x, B, L, on_device=False)
    clean2 = [P1._pysdr_stream.fetch(i, B)[1].copy() for i in range(len(g1))]
    P2._pysdr_stream.process_batch(xn, B, L, on_device=False)
    bad = [P2._pysdr_stream.fetch(i, B)[1].copy() for i in range(len(g2))]
    P2._pysdr_stream.process_batch(x, B, L, on_device=False)
    after = [P2._pysdr_stream.fetch(i, B)[1].copy() for i in range(len(g2))]
    kdec = -(-d.case.ntaps // d.up)
    assert plan.kpad == -(-kdec // 16) * 16
    m = np.arange(len(clean[0]), dtype=np.int64)
    n_m = m * d.down // d.up
    reach = (n_m >= j) & (n_m < j + plan.kpad)             # n_m - kpad < j <= n_m
    reach_oracle = (n_m >= j) & (n_m < j + kdec)
    assert reach.sum() >= reach_oracle.sum() > 0
    for i, o in enumerate(so.make_receivers(cfg, np.float64)):
        hit = ~np.isfinite(bad[i])
        # the oracle's own set on this stream (its window is kdec samples): computed, not assumed
        o.demod_data(xn[:2 * L]); o.demod_data(xn[2 * L:3 * L])
        lo = -(-2 * L * d.up // d.down)
        hit_o = np.zeros_like(hit)
        hit_o[lo:lo + len(o.iq)] = ~np.isfinite(o.iq)
        assert np.array_equal(hit_o, reach_oracle), i
        assert np.all(hit[hit_o]), i                                    # contains the oracle's set
        assert not np.any(hit & ~reach), (i, np.flatnonzero(hit)[[0, -1]], np.flatnonzero(reach)[[0, -1]])   # within the kpad window
        assert np.array_equal(bad[i][~hit], clean[i][~hit]), i          # every other output: the clean run's bits
        assert np.array_equal(after[i], clean2[i]), i                   # nothing of it is left in the context
