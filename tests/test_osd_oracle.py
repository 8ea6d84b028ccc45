"""Ordered-statistics decoding behind min-sum on the CPU: the NumPy oracle (tests/osd_oracle.py) on its
own definition -- the basis and the generator, the patterns' index, the edge inputs -- and behind the float64 channelizer
with the FT8 oracle skimmer on the weak-station runs of tests/test_ldpc_oracle.py.  No GPU: the kernel is held against
this oracle for equality in tests/test_gpu_osd.py, the scalar transcription in tests/test_osd_plan.py."""
import numpy as np

from tests import ldpc_oracle as lo
from tests import osd_oracle as oo
from tests import test_ldpc_oracle as tl

F32 = np.float32
NOISE_SEED = 400                                                                # the oracle gives no status 2 on this seed's 400 words


def noisy(rng, sigma):
    from pysdr_amd import ldpc
    cw = ldpc.encode(rng.integers(0, 2, 77))
    return cw, ((2.0 * cw - 1) + sigma * rng.standard_normal(174)).astype(F32)


def test_the_basis_the_generator_and_the_patterns_index():
    from pysdr_amd import ldpc
    rng = np.random.default_rng(3)
    assert oo.G.shape == (91, 174) and all(ldpc.check(row) for row in oo.G)
    lasts = []
    for sigma in (0.5, 1.0, 3.0):
        cw, x = noisy(rng, sigma)
        w = oo.osd_word(x, 2)
        perm, piv, Gp = w["perm"], w["piv"], w["Gp"]
        assert sorted(perm) == list(range(174)) and (np.diff(piv) > 0).all() and w["last"] == piv[90] >= 90
        r = np.abs(x)[perm]
        assert (np.diff(r) <= 0).all() and all(perm[p] < perm[p + 1] for p in np.flatnonzero(np.diff(r) == 0))
        assert np.array_equal(Gp[:, piv], np.eye(91, dtype=np.uint8))           # G' on the basis is the identity
        # a rank that was skipped depends on the basis ranks before it: its column is zero below them
        for p in sorted(set(range(piv[90])) - set(piv)):
            assert not Gp[np.searchsorted(piv, p):, p].any()
        assert len(w["pat"]) == 4187
        back = np.zeros((4187, 174), np.uint8)
        back[:, perm] = w["pat"] ^ w["h"][perm][None]                           # every pattern's word, in transmission order
        assert not ((back.astype(np.int64) @ ldpc.H.T.astype(np.int64)) % 2).any()
        for k in (0, 1, 91, 92, 93, 181, 182, 4186):
            assert ldpc.check(back[k])
            rows = oo.ij_of(k)
            want = w["pat"][0].copy()
            for i in rows:
                want ^= Gp[i]
            assert np.array_equal(w["pat"][k], want), k
        # the distance: every add rounded on its own, in rank order
        for k in (0, 50, 4000, w["k"]):
            d = F32(0)
            for p in np.flatnonzero(w["pat"][k]):
                d = F32(d + r[p])
            assert d.tobytes() == w["d"][k].tobytes()
        assert w["d"][w["k"]] == w["d"].min() and w["weight"] == w["pat"][w["k"]].sum()
        lasts.append(w["last"])
    print("last rank of the basis at sigma 0.5, 1.0, 3.0:", lasts)
    # k <-> (i, j) round-trips over all 4187, in lexicographic order
    assert oo.ij_of(0) == () and [oo.ij_of(k) for k in range(1, 92)] == [(i,) for i in range(91)]
    pairs = [oo.ij_of(k) for k in range(92, 4187)]
    assert pairs == sorted(pairs) and len(set(pairs)) == 4095 and all(i < j for i, j in pairs)
    assert all(oo.k_of(*oo.ij_of(k)) == k for k in range(1, 4187))


def test_edge_inputs():
    from pysdr_amd import ldpc
    rng = np.random.default_rng(4)
    # zeros, and -0: ranks are positions, the basis is the systematic one, k = 0, the status stays min-sum's 1
    for z in (np.zeros(174, F32), -np.zeros(174, F32)):
        for order in (0, 1, 2):
            st, bits, _, de = oo.decode(z[None], order=order)
            assert list(st[0]) == [1, 0, 0, 1] and not bits.any() and list(de[0]) == [0, 90, 0, 0]
    w = oo.osd_word(np.zeros(174, F32))
    assert np.array_equal(w["perm"], np.arange(174)) and np.array_equal(w["piv"], np.arange(91)) and np.array_equal(w["Gp"], oo.G)
    # a word of +-1 only: all r equal, ranks are positions; 12 errors among the parity bits are re-encoded away at k = 0
    cw = ldpc.encode(rng.integers(0, 2, 77))
    x = (2.0 * cw - 1).astype(F32)
    x[91 + rng.choice(83, 12, replace=False)] *= -1
    w = oo.osd_word(x)
    assert np.array_equal(w["perm"], np.arange(174)) and w["last"] == 90 and w["k"] == 0 and w["weight"] == 12 and w["dist"] == 12
    assert np.array_equal(w["word"], cw)
    # a status 2 is left alone
    st, _, _, de = oo.decode((2.0 * cw - 1).astype(F32)[None])
    assert list(st[0]) == [2, 0, 0, 0] and list(de[0]) == [-1, -1, -1, 0]
    # a tie of the two best patterns goes to the lower k: with equal magnitudes a distance is a weight, an integer, and
    # among 4187 words 25 errors away several often share the least
    ties = 0
    for _ in range(40):
        cw = ldpc.encode(rng.integers(0, 2, 77))
        x = (2.0 * cw - 1).astype(F32)
        x[rng.choice(174, 25, replace=False)] *= -1
        w = oo.osd_word(x)
        best = np.flatnonzero(w["d"] == w["d"].min())
        assert w["k"] == best[0] and float(w["dist"]) == w["weight"]
        ties += len(best) > 1
    assert ties >= 5, ties
    # the scale does not matter: a power of two changes no decision
    _, x = noisy(rng, 0.9)
    a, b = oo.decode(x[None]), oo.decode((x * F32(2.0 ** 50))[None])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3][:, :3], b[3][:, :3])


def osd_tally(snr, order):
    """-> (runs, found, decoded by min-sum, decoded with the second stage, wrong-but-accepted)"""
    from pysdr_amd import ldpc
    runs, others = tl.weak_runs(snr)
    found = [(v, m) for v, m in runs if v is not None]
    first = decoded = wrong = 0
    if found:
        x = np.array([v for v, _ in found])
        st0 = lo.decode(x)[0]
        st, bits, _, _ = oo.decode(x, order=order)
        for (v, m), s0, s, b in zip(found, st0, st, ldpc.unpack_bits(bits)):
            good = s[0] == 2 and np.array_equal(b[:77], m)
            first += s0[0] == 2
            decoded += good
            wrong += s[0] == 2 and not good
    if others:
        wrong += int((oo.decode(np.array(others), order=order)[0][:, 0] == 2).sum())
    return len(runs), len(found), int(first), int(decoded), int(wrong)


def test_the_weak_station_table():
    """-18 dB: all twelve runs decode to the transmitted bits with order 2.  -20 dB: strictly more than min-sum alone.  No
    word other than the transmitted one is accepted at any level, and 400 words of noise give no message."""
    got = {}
    for snr in (-18.0, -20.0, -21.0, -22.0):
        for order in (0, 1, 2):
            n, found, first, decoded, wrong = got[(snr, order)] = osd_tally(snr, order)
            print(f"{snr} dB order {order}: found {found} of {n}, min-sum alone {first}, with the second stage {decoded}, wrong-but-accepted {wrong}")
            assert wrong == 0 and decoded >= first
    assert got[(-18.0, 2)][1:4] == (12, 11, 12)
    assert got[(-20.0, 2)][1] == 12 and got[(-20.0, 2)][3] > got[(-20.0, 2)][2] == 1
    noise = np.random.default_rng(NOISE_SEED).standard_normal((400, 174)).astype(F32)
    st, _, _, de = oo.decode(noise, order=2)
    print(f"400 words of noise (seed {NOISE_SEED}): {(st[:, 0] == 2).sum()} status 2; weight of the best word {de[:, 2].min()} to {de[:, 2].max()}, "
          f"median {int(np.median(de[:, 2]))}; last rank {de[:, 1].min()} to {de[:, 1].max()}")
    assert (st[:, 3] > 0).all() and (st[:, 0] != 2).all()
