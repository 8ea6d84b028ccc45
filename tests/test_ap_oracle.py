"""A-priori decoding on the CPU: the NumPy oracle (tests/ap_oracle.py: the clamp, tests/ldpc_oracle.py's
decoder, the pick) behind the float64 channelizer and the FT8 oracle skimmer, on item 24's twelve weak-station runs per
level at -18, -20, -22 and -24 dB, and on the noise-only stream of item 22 with the gates open.  The tables it prints are
the ones DESIGN.md 3 item 28 quotes; it asserts only what held in them.  No GPU: the kernels are held against this oracle
for equality in tests/test_gpu_ap.py, the scalar transcription in tests/test_ap_plan.py."""
import functools

import numpy as np

from tests import ap_oracle as ao
from tests import ft8_oracle as fo
from tests import ldpc_oracle as lo
from tests import test_ft8_oracle as t8
from tests import test_ldpc_oracle as tl

F32 = np.float32
LEVELS = (-18.0, -20.0, -22.0, -24.0)
MAGS = (0.5, 1.0, 2.0, 4.0)
CALLS = ("K1ABC", "W9XYZ", "DL1ABC", "JA1XYZ", "G4ABC", "VK2DEF", "PY2GH", "OH8X")


def masks():
    """the masks of ``CQ ? ?`` (29 + 3 bits), ``? call ?`` (32) and ``a b ?`` (61) as 77 bits each"""
    from pysdr_amd import ap
    return {name: ao.unword(h[0])[:77] for name, h in (("cq", ap.hyp_cq()), ("32", ap.hyp_from("K1ABC")), ("61", ap.hyp_pair("K1ABC", "W9XYZ")))}


def true_hyps(msg):
    """the three hypotheses that are right for a message: its own bits under each mask"""
    return [ao.hyp(m, msg) for m in masks().values()]


def wrong_hyps(rng):
    """eight hypotheses that a skimmer's history could offer and that are wrong for noise or for another station's frame"""
    from pysdr_amd import ap
    c = list(rng.permutation(CALLS))
    return [ap.hyp_cq(), ap.hyp_from(c[0]), ap.hyp_from(c[1]), ap.hyp_pair(c[2], c[3]), ap.hyp_pair(c[4], c[0]), ap.hyp_cq_from(c[5]),
            ap.hyp_cq_from(c[6]), ap.hyp_text(f"CQ {c[7]} FN42")]


@functools.lru_cache(maxsize=None)
def level(snr):
    """-> (runs, found, min-sum alone, {mag: rescues under the true cq / 32 / 61 hypothesis as bool [found][3]}, nerr of the rescues at mag 1)"""
    from pysdr_amd import ldpc
    runs, _ = tl.weak_runs(snr)
    found = [(v, m) for v, m in runs if v is not None]
    x = np.array([v for v, _ in found], F32).reshape(-1, 174)
    st = lo.decode(x)[0] if len(found) else np.zeros((0, 4), np.int32)
    first = np.array([s[0] == 2 and np.array_equal(ldpc.unpack_bits(b)[:77], m) for (v, m), s, b in zip(found, st, lo.decode(x)[1])], bool) \
        if len(found) else np.zeros(0, bool)
    hyps, pairs = [], []
    for c, (_, m) in enumerate(found):
        hyps += true_hyps(m)
        pairs += [(c, 3 * c + k) for k in range(3)]
    got, nerr = {}, []
    for mag in MAGS:
        _, _, detail, pbits = ao.decode(x, hyps, pairs, mag=mag) if len(found) else (None, None, np.zeros((0, 4), np.int32), np.zeros((0, 12), np.uint8))
        ok = np.array([d[0] == 2 and np.array_equal(ldpc.unpack_bits(b)[:77], found[p // 3][1]) for p, (d, b) in enumerate(zip(detail, pbits))], bool)
        wrong = int(((detail[:, 0] == 2) & ~ok).sum())
        assert wrong == 0                                                       # a right hypothesis never gives another message
        got[mag] = ok.reshape(-1, 3)
        if mag == 1.0:
            nerr = [int(d[2]) for d, o in zip(detail, ok) if o]
    return len(runs), len(found), first, got, nerr


@functools.lru_cache(maxsize=None)
def noise_candidates(least=2000):
    """the soft bits of the peaks of item 22's noise-only stream with the gates open: float32 [>= least][174]"""
    out = []
    for case in t8.CASES:
        sk, _, _, _ = t8.find(case, "centre", None, 60, seconds=60.0)
        loose = fo.Oracle(3, case[1], fo.params(smin=0.0, hmin=0))
        for i0 in range(0, sk.rows.shape[1], 256):
            t_first = loose.t_done
            for t0, F, _, _ in loose.events_of(t_first, loose.process(sk.rows[:, i0:i0 + 256])[1]):
                out.append(loose.llr(F, t0))
            if len(out) >= least:
                break
        if len(out) >= least:
            break
    x = np.array(out[:least], F32)
    x.setflags(write=False)
    return x


def test_the_weak_station_table_and_the_rule_for_mag():
    table = {}
    for snr in LEVELS:
        n, found, first, got, nerr = table[snr] = level(snr)
        print(f"{snr} dB: found {found} of {n}, min-sum alone {int(first.sum())}")
        for mag in MAGS:
            either = first[:, None] | got[mag]
            print(f"    mag {mag}: with the true CQ ? ? {int(either[:, 0].sum())}, the true 32 bits {int(either[:, 1].sum())}, the true 61 bits "
                  f"{int(either[:, 2].sum())} (the hypothesis alone: {[int(v) for v in got[mag].sum(axis=0)]})")
        print(f"    nerr of the rescues at mag 1.0: {sorted(nerr)}")
    # the weakest level where all twelve true 61-bit hypotheses rescue, at the default mag
    whole = [snr for snr in LEVELS if table[snr][1] == 12 and (table[snr][2] | table[snr][3][1.0][:, 2]).all()]
    print("all twelve decode with the true 61 bits at", whole)
    assert whole == [-18.0]
    snr = min(whole)
    assert table[snr][1] == 12 and (table[snr][2] | table[snr][3][1.0][:, 2]).all() and not table[snr][2].all()
    # -20 dB, where min-sum alone gives 1 of 12: the more bits are told, the more runs decode
    at20 = (table[-20.0][2][:, None] | table[-20.0][3][1.0]).sum(axis=0)
    assert int(table[-20.0][2].sum()) < at20[0] <= at20[1] < at20[2]
    # the default stays 1.0 unless another value decodes more at every level (alpha's rule)
    total = {mag: [int((table[s][2][:, None] | table[s][3][mag]).sum()) for s in LEVELS] for mag in MAGS}
    print("decodes per level, all three hypotheses together:", total)
    better = [mag for mag in MAGS if mag != 1.0 and all(a > b for a, b in zip(total[mag], total[1.0]))]
    print("values of mag that decode more than 1.0 at every level:", better)
    from pysdr_amd import ap
    assert ap.params().mag == 1.0 and not better


def test_the_price_on_noise_and_a_wrong_hypothesis_beside_a_right_one():
    from pysdr_amd import ap, ldpc
    x = noise_candidates()
    rng = np.random.default_rng(28)
    hyps, pairs = [], []
    for c in range(len(x)):
        hyps += wrong_hyps(rng)
        pairs += [(c, 8 * c + k) for k in range(8)]
    detail = np.concatenate([ao.decode(x[i:i + 256], hyps[8 * i:8 * (i + 256)], np.array(pairs[8 * i:8 * (i + 256)]) - (i, 8 * i))[2]
                             for i in range(0, len(x), 256)])
    false = detail[detail[:, 0] == 2]
    by_kind = detail[:, 0].reshape(-1, 8)
    print(f"{len(x)} noise candidates x 8 wrong hypotheses = {len(detail)} pairs, nerr_max off: status 2 in {len(false)} (expected "
          f"pairs * 2^-14 = {len(detail) / 16384:.2f}); by place in the eight: {[int(v) for v in (by_kind == 2).sum(axis=0)]}; "
          f"codewords of status 1: {int((detail[:, 0] == 1).sum())}")
    print(f"    nerr of those: {sorted(int(v) for v in false[:, 2])}")
    rescues = sorted(v for snr in LEVELS for v in level(snr)[4])
    print(f"    nerr of the true rescues at mag 1.0, all levels: {rescues}")
    if len(false) and rescues:
        print(f"    the two separate: {max(rescues) < min(false[:, 2])}")
    print(f"    false rate per pair {len(false) / len(detail):.2e}; the default nerr_max is {ap.NERR_MAX}")
    assert len(x) >= 2000
    # a wrong hypothesis never changes a pick that a right one wins: the weak runs again, every candidate with its three
    # right hypotheses and eight wrong ones
    for snr in LEVELS:
        runs, _ = tl.weak_runs(snr)
        found = [(v, m) for v, m in runs if v is not None]
        if not found:
            continue
        xs = np.array([v for v, _ in found], F32)
        hy, pr = [], []
        for c, (_, m) in enumerate(found):
            hy += true_hyps(m) + wrong_hyps(rng)
            pr += [(c, 11 * c + k) for k in range(11)]
        alone = ao.decode(xs, hy, [p for p in pr if p[1] % 11 < 3])
        both = ao.decode(xs, hy, pr)
        for c, (_, m) in enumerate(found):
            if alone[0][c, 0] >= 0:
                assert both[0][c, 0] >= 0 and pr[both[0][c, 0]][1] % 11 < 3 and np.array_equal(both[1][c], alone[1][c]), (snr, c)
                assert np.array_equal(ldpc.unpack_bits(both[1][c])[:77], m)


def disturbed(llr, hyps, rounds=10):
    """the soft bits a part in a thousand off, ``rounds`` times -> min-sum's status and every pair's status each time"""
    rng = np.random.default_rng(0)
    out = []
    for _ in range(rounds):
        y = (llr * (1 + 1e-3 * rng.standard_normal(174))).astype(F32)
        out.append((int(lo.decode(y[None])[0][0, 0]), [int(v) for v in ao.decode(y[None], hyps, [(0, h) for h in range(len(hyps))])[2][:, 0]]))
    return out


def test_the_weak_levels_of_the_device_tests():
    """tests/ap_cases.py's weak levels, which tests/test_gpu_ap.py runs on the device: min-sum gives no message on the oracle
    skimmer's soft bits, every right hypothesis rescues the frame and a wrong one does not, and all of that stays when the
    soft bits are a part in a thousand off (the device's channelizer is float32, this one float64)."""
    from pysdr_amd import ap, ldpc
    from tests import ap_cases as ac
    # FT8: the CQ alone
    recs = ac.near("ft8", ac.oracle_records("ft8", ac.ft8_weak()), ac.FT8_F, 0.5)
    assert len(recs) == 1
    llr = recs[0]["llr"]
    hyps = [ap.hyp_cq(), ap.hyp_from("K1ABC"), ap.hyp_cq_from("K1ABC"), ap.hyp_text(ac.CQ), ap.hyp_from("W9XYZ")]
    st = lo.decode(llr[None])[0][0]
    got = ao.decode(llr[None], hyps, [(0, h) for h in range(5)])
    print(f"FT8 {ac.FT8_WEAK} dB seed {ac.FT8_SEED}: t0 {recs[0]['t0']} F {recs[0]['F']}, min-sum {list(st[:3])}, pairs {got[2].tolist()}, pick {list(got[0][0])}")
    assert st[0] == 0 and list(got[2][:, 0]) == [2, 2, 2, 2, 0] and got[0][0, 0] == 3 and np.array_equal(ldpc.unpack_bits(got[1])[0, :77], ac.cq_bits())
    assert all(d == (0, [2, 2, 2, 2, 0]) for d in disturbed(llr, hyps))
    # FT4: 77 bits that mean nothing, and their own bits under the three masks
    recs = ac.near("ft4", ac.oracle_records("ft4", ac.ft4_weak()), ac.FT4_F, 0.5)
    assert len(recs) == 1
    llr = recs[0]["llr"]
    hyps = true_hyps(ac.ft4_bits()) + [ap.hyp_text(ac.CQ)]
    st = lo.decode(llr[None])[0][0]
    got = ao.decode(llr[None], hyps, [(0, h) for h in range(4)])
    print(f"FT4 {ac.FT4_WEAK} dB seed {ac.FT4_SEED}: t0 {recs[0]['t0']} F {recs[0]['F']}, min-sum {list(st[:3])}, pairs {got[2].tolist()}, pick {list(got[0][0])}")
    assert st[0] == 0 and list(got[2][:, 0]) == [2, 2, 2, 0] and np.array_equal(ldpc.unpack_bits(got[1])[0, :77], ac.ft4_bits())
    assert all(d == (0, [2, 2, 2, 0]) for d in disturbed(llr, hyps))
    # the skimmer's stream: the clean CQ decodes, the weak one two slots later does not, and the history's hypotheses rescue it
    recs = ac.oracle_records("ft8", ac.skimmer_stream())
    first, second = ac.near("ft8", recs, ac.FT8_F, 0.5), ac.near("ft8", recs, ac.FT8_F, 30.5)
    assert len(first) == len(second) == 1 and second[0]["t0"] - first[0]["t0"] == 750
    st = lo.decode(np.array([first[0]["llr"], second[0]["llr"]]))[0]
    assert list(st[:, 0]) == [2, 0]
    hist = ap.History()
    assert hist.note(dict(first[0], ok=True, text=ac.CQ))
    offered = hist.hypotheses(second[0]["F"], second[0]["t0"])
    assert [k for k, _ in offered] == [1, 2, 4, 5]
    hyps = [h for _, h in offered]
    got = ao.decode(second[0]["llr"][None], hyps, [(0, h) for h in range(4)])
    print(f"skimmer stream seed {ac.SKIM_SEED}: records {[(r['t0'], r['F']) for r in recs]}, the weak CQ's pairs {got[2].tolist()}, pick {list(got[0][0])}")
    assert got[0][0, 0] == 3 and list(got[2][1:, 0]) == [2, 2, 2]
    assert all(d[0] == 0 and d[1][1:] == [2, 2, 2] for d in disturbed(second[0]["llr"], hyps))
    for r in recs:                                                              # and nothing else in the stream decodes, with or without CQ ? ?
        if r is not first[0] and r is not second[0]:
            assert lo.decode(r["llr"][None])[0][0, 0] != 2 and ao.decode(r["llr"][None], [ap.hyp_cq()], [(0, 0)])[0][0, 0] == -1
