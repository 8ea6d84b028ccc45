"""The CPU side of the channel bank's edge sweep (tests/bank_edge_cases.py): the library's plan confirms what the table
claims about every length, the helper's two precisions confirm that the table's taps and rows make TOL against the
float64 helper a statement about the kernels, and four wrong filters -- the errors the table is there to see -- each
miss that bar by a factor of ten and more at every length and mode.  Nothing here measures a kernel: that is
tests/test_gpu_bank_edge_sweep.py."""
import numpy as np
import pytest

from tests import bank_edge_cases as ec
from tests import bank_oracle as bo


@pytest.mark.parametrize("T", ec.LENGTHS)
def test_the_plan_is_what_the_table_claims(T, hiplib):
    from pysdr_amd.bank import plan
    p = plan(ec.CHANNELS[1], T, 4096)
    tp, hpad, nfull, tail = ec.CLAIMS[T]
    assert (p["taps_padded"], p["history"]) == (tp, hpad), (T, p)
    assert (p["tile"], p["threads"], p["tiles_per_row"]) == (ec.TILE, 256, 2)
    # the kernels' own expressions (bank.hip): nstep = tp / 8 steps, nfull = T / 8 of them whole, the last takes T - 8 nfull
    assert (nfull, tail) == (T // 8, T - 8 * (T // 8)) and tp // 8 == nfull + (1 if tail else 0)
    assert hpad >= T + 1 and hpad % 8 == 0 and hpad - 8 < T + 1 and hpad <= p["threads"]
    assert p["lds_bytes"] == 4 * (ec.TILE + tp)


def test_the_lengths_hold_every_edge():
    assert set(ec.CLAIMS) == set(ec.LENGTHS) and len(set(ec.LENGTHS)) == len(ec.LENGTHS) == 12
    by = {T: ec.CLAIMS[T] for T in ec.LENGTHS}
    assert min(ec.LENGTHS) == 3 and max(ec.LENGTHS) == 255
    assert [T for T in ec.LENGTHS if by[T][2] == 0] == [3, 7]                         # nfull = 0: the guarded step alone
    assert {by[T][3] for T in ec.LENGTHS} >= {0, 1, 3, 6, 7}                          # no guarded step, left = 1, the longest
    assert [T for T in ec.LENGTHS if by[T][1] == T + 1] == [7, 15, 247, 255]          # NFM's y[i - 2] on the first history sample
    assert [T for T in ec.LENGTHS if by[T][1] < 64] == [3, 7, 8, 9, 15, 16, 17]       # a history shorter than a wave
    assert [T for T in ec.LENGTHS if by[T][1] == 256] == [248, 249, 254, 255]         # one sample per thread of bank_finish


def test_the_call_list_holds_what_it_is_there_for():
    c = ec.case()
    assert c["counts"][:8] == list(ec.CALL_OUTPUTS) == [1, 3, 0, 5, 9, 2048, 2057, 7]
    assert len(c["counts"]) == 9 and c["counts"][8] >= 150 and sum(c["counts"]) == ec.FRAMES
    assert {0, 1, 3, 5, 9, ec.TILE, ec.TILE + 8 + 1} <= set(c["counts"])
    assert [k for k in c["counts"] if k and k % ec.TILE == 0] == [ec.TILE]            # no other call is a multiple of the tile
    assert all(n % 2 == 1 for n in c["cuts"]) and sum(c["cuts"]) == len(c["x"])
    assert c["carrier_rows"] == [7] and list(c["rows"][6:9]) == [2, 3, 4]             # the carrier row and its neighbours
    assert list(c["rows"][:5]) == [60, 61, 62, 63, 0]                                  # the rows wrap k = 0
    y, yc = ec.model_rows_per_call()
    assert y.shape == (12, ec.FRAMES) and [r.shape[1] for r in yc] == c["counts"]


def taps_differ_everywhere(c):
    """no tap equals another or its mirror image: a wrong walk cannot pass"""
    mirrored = c == c[::-1]
    if len(c) % 2:
        mirrored[len(c) // 2] = False                          # the middle tap is its own mirror image
    return len(np.unique(c)) == len(c) and not mirrored.any()


@pytest.mark.parametrize("T", ec.LENGTHS)
def test_the_taps(T):
    for mode in ("AM", "NFM"):
        c = ec.taps(T, mode)
        assert c.dtype == np.float64 and c.shape == (T,) and (c > 0).all() and abs(c.sum() - 1.0) < 0.25
        assert taps_differ_everywhere(c.astype(np.float32))
        assert c.min() >= 0.2 / T                              # every tap matters
    u, l, w = ec.taps(T, "USB"), ec.taps(T, "LSB"), ec.taps(T, "CW")
    assert np.array_equal(l, np.conj(u)) and not np.array_equal(w, u)
    for c in (u, w):
        assert c.dtype == np.complex128 and abs(np.sum(np.abs(c)) - 1.0) < 1e-12
        assert taps_differ_everywhere(c.astype(np.complex64))
    assert np.array_equal(ec.taps(T, "AM"), ec.taps(T, "AM"))                          # seeded


# ---- conditioning ------------------------------------------------------------------------------------------------------
def helper_disagreement(T, mode):
    """float32 helper against float64 helper on the model's rows, on the GPU sweep's measure: the worst over the calls"""
    c = ec.case()
    y, yc = ec.model_rows_per_call()
    w32 = ec.run_helper(T, mode, np.float32, yc, False)
    o64 = ec.helper(T, mode, np.float64, False)
    judge = ec.NfmJudge(o64, y, c["carrier_rows"]) if mode == "NFM" else None
    worst = 0.0
    for j, (r, a) in enumerate(zip(yc, w32)):
        b = o64.process(r)
        assert a["a"].shape == b["a"].shape == r.shape
        if r.shape[1] == 0:
            continue
        e = judge(a["a"], b["a"]) if mode == "NFM" else float(ec.audio_error(mode, a["a"], b).max())
        assert e <= ec.COND, (T, mode, j, e)
        worst = max(worst, e)
    return worst


@pytest.mark.parametrize("T", ec.LENGTHS)
def test_float32_helper_stays_within_a_quarter_of_the_bar_of_the_float64_helper(T):
    """The condition that makes TOL against the float64 helper a statement about the kernels: at this length the helper's
    own float32 form is within COND = TOL / 4 of it in every mode, on every call, on the measure the GPU sweep uses.  (A
    length or mode that misses gets other taps or another signal, never another bound: bank_edge_cases says which.)"""
    for mode in ec.MODES:
        print(f"BANKEDGE helpers T={T} mode {mode} worst {helper_disagreement(T, mode):.2e}")


@pytest.mark.parametrize("T", ec.LENGTHS)
def test_agc_on_the_two_helpers_agree_on_state_and_audio(T):
    """What the GPU sweep's AGC test rests on, AM and USB: agc, gain and maxbuf of the float32 helper within a quarter of
    the 1e-5 they are held to of the float64 helper's, the audio within COND x gain on the mode's measure."""
    from tests.test_gpu_bank import rel
    _, yc = ec.model_rows_per_call()
    for mode in ("AM", "USB"):
        w32, w64 = ec.run_helper(T, mode, np.float32, yc, True), ec.run_helper(T, mode, np.float64, yc, True)
        for j, (p, q, r) in enumerate(zip(w32, w64, yc)):
            if r.shape[1] == 0:
                continue
            for k in ("agc", "agc_gain", "maxbuf"):
                assert rel(p[k].astype(np.float64), q[k]).max() <= 1e-5 / 4, (T, mode, j, k)
            measure = np.max(np.abs(q["a"]), axis=1) if mode == "AM" else q["scale"]
            e = np.max(np.abs(p["am"] - q["am"]), axis=1) / (q["gain"] * measure)
            assert e.max() <= ec.COND, (T, mode, j, float(e.max()))
            assert (q["gain"] != 1).all()


# ---- teeth -------------------------------------------------------------------------------------------------------------
def first_history_sample_zeroed(o, T, mode):
    """the sample a call's AF windows reach furthest back for, taken as 0 in every row: y[m0 - (T - 1)], in NFM
    y[m0 - (T + 1)] (the discriminator's y[i - 2] of the window's first output)"""
    back = T + 1 if mode == "NFM" else T - 1
    for d in o.demod:
        d.yhist = d.yhist.copy()
        d.yhist[len(d.yhist) - back] = 0


def mutants(T, mode):
    """name -> (helper, what to do to it before a call): the float64 helper with one thing wrong"""
    c = ec.taps(T, mode)
    dropped = c.copy()
    dropped[T - 1] = 0
    late = np.concatenate((c[:T - 1], [0], c[T - 1:]))                   # T + 1 taps: tap T - 1 meets d[m - T]
    mk = lambda t: ec.helper(T, mode, np.float64, False, t)              # noqa: E731
    return {"reversed": (mk(c[::-1].copy()), None), "tap T-1 dropped": (mk(dropped), None),
            "tap T-1 a sample late": (mk(late), None), "first history sample 0": (mk(c), first_history_sample_zeroed)}


def distance(mode, got, w, first, carrier):
    """how far ``got`` is from the master's answer w on the sweep's plain measures (NFM: the carrier row from output 256 on)"""
    if mode != "NFM":
        return float(ec.audio_error(mode, got, w).max())
    n = got.shape[1]
    if first + n <= 256:
        return 0.0
    s = max(256 - first, 0)
    return max(float(np.max(np.abs(got[a, s:] - w["a"][a, s:])) / np.max(np.abs(w["a"][a, s:]))) for a in carrier)


@pytest.mark.parametrize("T", ec.LENGTHS)
def test_the_cases_see_the_errors_they_are_there_for(T):
    """Taps walked backwards, the last tap dropped, the last tap one sample late, the first history sample of a call's
    window lost: each is at least 10 TOL from the float64 helper on at least one call, at this length in every mode --
    without a wrong kernel ever running on a GPU."""
    c = ec.case()
    _, yc = ec.model_rows_per_call()
    for mode in ec.MODES:
        master = ec.run_helper(T, mode, np.float64, yc, False)
        for name, (o, before) in mutants(T, mode).items():
            far, first = [], 0
            for r, w in zip(yc, master):
                if before is not None:
                    before(o, T, mode)
                got = o.process(r)["a"]
                if r.shape[1]:
                    far.append(distance(mode, got, w, first, c["carrier_rows"]))
                first += r.shape[1]
            print(f"BANKEDGE mutant T={T} mode {mode} {name}: {max(far):.2e}")
            assert max(far) >= 10 * ec.TOL, (T, mode, name, far)
            if name == "first history sample 0":            # only a call's first output can show it: each of the last three calls does
                assert c["counts"][-3:] == [2057, 7, 270] and min(far[-3:]) >= 10 * ec.TOL, (T, mode, far)


# ---- the AGC's step case ---------------------------------------------------------------------------------------------------
def test_the_agc_step_case_clamps_attacks_and_goes_silent():
    a = ec.agc_case()
    assert len(a["cuts"]) == ec.AGC_CALLS == 140 and sum(a["cuts"]) == len(a["x"])
    assert list(a["level"][[0, 19, 20, 39, 40, 99, 100, 139]]) == [1, 1, 0.01, 0.01, 0, 0, 1, 1]
    yc = bo.cut_rows(ec.model_rows(a["x"]), a["cuts"], ec.D)
    assert all(r.shape == (12, ec.AGC_OUTPUTS) for r in yc)
    w32 = ec.run_helper(ec.AGC_T, "AM", np.float32, yc, True)
    w64 = ec.run_helper(ec.AGC_T, "AM", np.float64, yc, True)
    rows = ec.agc_conditions(w32)
    assert len(rows) == 11
    # the two helpers agree on the audio as the GPU test measures it: |am - want| <= COND * gain * the row's peak |a|
    worst = 0.0
    for j, (p, q) in enumerate(zip(w32, w64)):
        bar = q["gain"] * np.max(np.abs(q["a"]), axis=1)
        d = np.max(np.abs(p["am"].astype(np.float64) - q["am"]), axis=1)
        assert (d <= ec.COND * bar).all(), (j, d, bar)
        worst = max(worst, float(np.max(d[bar > 0] / bar[bar > 0], initial=0.0)))
    print(f"BANKEDGE helpers AGC step case: worst |am32 - am64| / (gain peak) {worst:.2e}")
