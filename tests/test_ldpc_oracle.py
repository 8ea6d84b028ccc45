"""LDPC(174,91), CRC-14 and the decoder's definition on the CPU: the sparse checks derived again from
the generator, the encoder, and the float32 oracle (tests/ldpc_oracle.py) on clean, damaged and hopeless words, and behind
the float64 channelizer with the FT8 oracle skimmer of tests/test_ft8_oracle.py in front of it.  No GPU: the kernel is held
against this oracle bit for bit in tests/test_gpu_ldpc.py."""
import functools

import numpy as np
import pytest

from tests import ft8_oracle as fo
from tests import ldpc_oracle as lo
from tests import test_ft8_oracle as t8

F32 = np.float32
SHA = "e524f34a5362d367a4437174bad02862c649975e8c1de3fd3ceebf413bc3ab38"
ALPHAS = (0.75, 0.8125, 0.875, 1.0)


def message(rng):
    return rng.integers(0, 2, 77).astype(np.uint8)


def soft(bits, rng, lo_=2.0, hi=4.0):
    """strong soft bits of a word: positive for bit 1"""
    return ((2.0 * np.asarray(bits, np.float64) - 1) * rng.uniform(lo_, hi, len(bits))).astype(F32)


def test_the_check_table_follows_from_the_generator():
    from pysdr_amd import ldpc
    rows = lo.derive_checks(seed=0, rounds=20)
    assert len(rows) == 83 and tuple(rows) == ldpc.CHECKS
    assert sorted(ldpc.CHECKS) == list(ldpc.CHECKS)
    assert lo.checks_sha256(ldpc.CHECKS) == SHA
    assert sorted(len(r) for r in rows) == [6] * 59 + [7] * 24
    assert (ldpc.H.sum(axis=0) == 3).all() and ldpc.H.sum() == 522
    # rank 83 over GF(2)
    A, r = ldpc.H.astype(bool).copy(), 0
    for c in range(174):
        p = np.flatnonzero(A[r:, c])
        if not len(p):
            continue
        A[[r, r + p[0]]] = A[[r + p[0], r]]
        others = np.flatnonzero(A[:, c])
        A[others[others != r]] ^= A[r]
        r += 1
        if r == 83:
            break
    assert r == 83
    # the two directions of the table
    for e in range(522):
        assert e in ldpc.COL_EDGES[ldpc.EDGE_COL[e]]
    assert (np.diff(ldpc.EDGE_CHECK[ldpc.COL_EDGES], axis=1) > 0).all()
    # a wrong hex digit destroys the structure
    bad = ldpc.GENERATOR.copy()
    bad[17, 40] ^= 1
    dual = np.concatenate((bad, np.eye(83, dtype=np.uint8)), axis=1)
    assert ((ldpc.H.astype(int) @ dual.T.astype(int)) % 2).any()


def test_encode_then_check_and_the_crc():
    from pysdr_amd import ldpc
    rng = np.random.default_rng(1)
    for _ in range(50):
        m = message(rng)
        cw = ldpc.encode(m)
        assert cw.shape == (174,) and np.array_equal(cw[:77], m) and np.array_equal(cw[77:91], ldpc.crc14(m))
        assert ldpc.check(cw) and ldpc.crc_ok(cw[:91])
        cw[rng.integers(0, 174)] ^= 1
        assert not ldpc.check(cw)
    assert not ldpc.crc14(np.zeros(77)).any() and ldpc.check(np.zeros(174))
    # long division of the 96-bit augmented word
    for _ in range(20):
        m = message(rng)
        w = np.concatenate((m, np.zeros(19, np.uint8))).astype(int)
        poly = [int(c) for c in format((1 << 14) | ldpc.CRC_POLY, "015b")]
        for i in range(82):
            if w[i]:
                w[i:i + 15] ^= poly
        assert list(w[82:]) == list(ldpc.crc14(m))
    with pytest.raises(ValueError):
        ldpc.crc14(np.zeros(76))
    with pytest.raises(ValueError):
        ldpc.check(np.zeros(173))
    assert np.array_equal(ldpc.unpack_bits(np.packbits(np.concatenate((cw[:91], np.zeros(5, np.uint8))))), cw[:91])


def test_clean_damaged_and_hopeless_words():
    from pysdr_amd import ldpc
    rng = np.random.default_rng(2)
    msgs = [message(rng) for _ in range(40)]
    cws = np.array([ldpc.encode(m) for m in msgs])
    clean = np.array([soft(c, rng) for c in cws])
    st, bits, post = lo.decode(clean)
    assert (st[:, 0] == 2).all() and not st[:, 1:].any()                       # noise-free: a codeword at k = 0
    assert np.array_equal(ldpc.unpack_bits(bits), cws[:, :91]) and np.array_equal(post.view(np.uint32), (-clean).view(np.uint32))
    flips = np.array([1 + i % 5 for i in range(40)])
    damaged = clean.copy()
    for i, k in enumerate(flips):
        where = rng.choice(174, k, replace=False)
        damaged[i, where] = -damaged[i, where]                                 # strong and wrong
    st, bits, _ = lo.decode(damaged)
    assert (st[:, 0] == 2).all() and (st[:, 1] >= 1).all() and np.array_equal(st[:, 2], flips), st[:, :3]
    assert np.array_equal(ldpc.unpack_bits(bits), cws[:, :91]) and not st[:, 3].any()
    assert (lo.decode(damaged, iters=1)[0][:, 1] == 1).all()
    # a word with a broken CRC is a codeword and no message; so is the zero word, which zero input produces
    b91 = cws[0, :91].copy()
    b91[80] ^= 1
    broken = ldpc.encode91(b91)
    assert ldpc.check(broken)
    st, bits, _ = lo.decode(np.stack((soft(broken, rng), np.zeros(174, F32), soft(np.zeros(174), rng))))
    assert list(st[:, 0]) == [1, 1, 1] and not st[:, 1:].any() and np.array_equal(ldpc.unpack_bits(bits)[0], b91) and not bits[1:].any()
    noise = rng.standard_normal((300, 174)).astype(F32)
    st, _, post = lo.decode(noise)
    print("noise: status counts", np.bincount(st[:, 0], minlength=3), "iterations of the rest", sorted(set(st[st[:, 0] > 0, 1])))
    assert (st[:, 0] <= 1).all() and (st[st[:, 0] == 0, 1] == 30).all() and np.isfinite(post).all()
    # the scale of the input does not matter: a power of two changes no decision
    a, b = lo.decode(damaged), lo.decode(damaged * F32(2.0 ** 40))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # a raw bit error rate of 6 %: about 10 errors of 174
    hard = 0
    for i in range(60):
        cw = ldpc.encode(message(rng))
        x = (2.0 * cw - 1) + 0.643 * rng.standard_normal(174)                 # Q(1 / 0.643) = 0.06
        hard += int(((x > 0) != cw).sum())
        s, bb, _ = lo.decode(x.astype(F32)[None])
        assert s[0, 0] == 2 and np.array_equal(ldpc.unpack_bits(bb)[0], cw[:91]), i
    print(f"6 % raw errors: 60 of 60 decoded, {hard / 60:.1f} hard errors per word")


# ---- behind the float64 channelizer ----------------------------------------------------------------------------------------

def find_coded(case, place, snr, seed, seconds=t8.SECONDS, t0=t8.T0, off=0.0):
    """tests/test_ft8_oracle.py's ``find`` with a codeword on the air: the same draws from the same generator, of which the
    first 77 bits are the message.  -> (oracle skimmer, the fine rows that may own the station, the message)"""
    from pysdr_amd import ldpc
    fs, S, D, M = case
    f, homes = t8.station_freq(place, fs, S, M)
    rng = np.random.default_rng(seed)
    msg = rng.integers(0, 2, 174)[:77].astype(np.uint8)
    bits = ldpc.encode(msg)
    n = int(seconds * fs)
    x = fo.noise_sigma(0.0, fo.SNR_BW, fs) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    at = t8.start_sample(t0, S, D, M)
    w = fo.waveform(fo.tones(bits), f + off, fs, True, phase=rng.uniform(0, 6.28)) * 10 ** (snr / 20)
    x[at:at + len(w)] += w[:n - at]
    rows = t8.rows_behind_the_channelizer(x, fs, S, D, M, t8.channels_of(place, M))
    sk = fo.Skimmer(3, S, False)
    sk.push(rows)
    return sk, homes, msg


@functools.lru_cache(maxsize=None)
def weak_runs(snr):
    """the twelve runs of test_weak_stations_are_reported_not_asserted at one level: (soft bits of the record at the
    station or None, message, hard errors), and the soft bits of every other record"""
    runs, others = [], []
    for case in t8.CASES:
        for seed in range(2):
            for place, off in (("centre", 0.0), ("between", 0.0), ("centre", 0.7)):
                sk, homes, msg = find_coded(case, place, snr, 7000 + 10 * seed + int(abs(snr)), off=off)
                near = [r for r in sk.records if abs(r["t0"] - t8.T0) <= 1 and min(abs(r["F"] - h) for h in homes) <= 1]
                others += [r["llr"] for r in sk.records if r not in near]
                runs.append((near[0]["llr"] if near else None, msg))
    return runs, others


def tally(snr, alpha):
    from pysdr_amd import ldpc
    runs, others = weak_runs(snr)
    found = [(v, m) for v, m in runs if v is not None]
    decoded = wrong = 0
    errs = []
    if found:
        st, bits, _ = lo.decode(np.array([v for v, _ in found]), alpha=alpha)
        for (v, m), s, b in zip(found, st, ldpc.unpack_bits(bits)):
            errs.append(int(((v > 0) != ldpc.encode(m)).sum()))
            good = s[0] == 2 and np.array_equal(b[:77], m)
            decoded += good
            wrong += s[0] == 2 and not good
    if others:
        wrong += int((lo.decode(np.array(others), alpha=alpha)[0][:, 0] == 2).sum())
    return len(runs), len(found), int(decoded), int(wrong), errs


def test_minus_15_db_decodes_every_run_and_weaker_ones_are_reported():
    """-15 dB in 2500 Hz: twelve of twelve found with few hard errors, every one status 2 with the transmitted bits.  -18 and
    -20 dB are measurements: printed for every alpha of the sweep, and no word that is not the transmitted one may come
    out status 2 at any level."""
    n, found, decoded, wrong, errs = tally(-15.0, 0.8125)
    print(f"-15.0 dB alpha 0.8125: found {found} of {n}, decoded {decoded}, wrong-but-status-2 {wrong}, hard errors {errs}")
    assert found == n == 12 and decoded == 12 and wrong == 0
    for snr in (-18.0, -20.0):
        for alpha in ALPHAS:
            n, found, decoded, wrong, errs = tally(snr, alpha)
            print(f"{snr} dB alpha {alpha}: found {found} of {n}, decoded {decoded}, wrong-but-status-2 {wrong}, hard errors {errs}")
            assert wrong == 0


def test_the_frame_of_the_26_s_stream_decodes_and_its_images_do_not():
    """DESIGN.md 3 item 22's images 144 steps from a frame are records; the decoder behind refuses them"""
    from pysdr_amd import ldpc
    sk, homes, msg = find_coded(t8.CASES[0], "centre", 0.0, 77, seconds=26.0, t0=160)
    st, bits, _ = lo.decode(np.array([r["llr"] for r in sk.records]))
    got = [(r["t0"] - 160, r["F"] - homes[0], int(s[0]), int(s[1]), int(s[2])) for r, s in zip(sk.records, st)]
    print(f"a 0 dB frame at step 160 of a 26 s stream: (steps, rows from it, status, iterations, nerr) {got}")
    frame = [k for k, g in enumerate(got) if g[:2] == (0, 0)]
    assert len(frame) == 1 and got[frame[0]][2] == 2 and np.array_equal(ldpc.unpack_bits(bits)[frame[0], :77], msg)
    assert len(got) > 1 and all(g[2] != 2 for g in got if g[:2] != (0, 0)) and all(g[0] in (-144, 0, 144) for g in got)
