"""NumPy model of a-priori decoding.  Test infrastructure only.

The rules of a hypothesis table and a pair list, the clamp, tests/ldpc_oracle.py's decoder on the clamped words, the
counting of nerr and nap, a pair's status and the pick, in the definition's order, so that the kernels
(pysdr_amd/csrc/ap.hip) and the scalar transcription (ap_plan.h) can be held against it for equality.  A hypothesis is
(mask, value), each uint8 [12], message bit i at bit 7 - (i & 7) of byte i >> 3."""
import numpy as np

from tests import ldpc_oracle as lo

F32 = np.float32
N, K, MSG = 174, 91, 77
HYP_MAX, PAIR_MAX, CAND_MAX = 4096, 65536, 4096


def word(bits):
    """bits (up to 96 of them, from bit 0 on) -> uint8 [12]"""
    b = np.zeros(96, np.uint8)
    b[:len(bits)] = np.asarray(bits, np.uint8) & 1
    return np.packbits(b)


def unword(w):
    """uint8 [12] -> its 96 bits"""
    return np.unpackbits(np.asarray(w, np.uint8).reshape(12))


def hyp(mask_bits, value_bits):
    """77 mask bits and 77 value bits -> (mask, value); the value is kept under the mask only"""
    m = np.asarray(mask_bits, np.uint8).reshape(MSG) & 1
    return word(m), word(m & np.asarray(value_bits, np.uint8).reshape(MSG))


def hyp_ok(mask, value):
    m, v = unword(mask), unword(value)
    return bool(m.any() and not m[MSG:].any() and not (v & ~m & 1).any())


def pairs_ok(pairs, n, H):
    """-> first int32 [n + 1], or None for a list outside the rule"""
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    if len(p) > PAIR_MAX or not 0 <= n <= CAND_MAX or not 1 <= H <= HYP_MAX:
        return None
    if len(p) and (p[:, 0].min() < 0 or p[:, 0].max() >= n or p[:, 1].min() < 0 or p[:, 1].max() >= H):
        return None
    key = p[:, 0] * (HYP_MAX + 1) + p[:, 1]
    if (np.diff(key) <= 0).any():
        return None
    return np.searchsorted(p[:, 0], np.arange(n + 1), "left").astype(np.int32)


def clamp(llr, hyps, pairs, mag=1.0):
    """llr float32 [n][174], hyps [(mask, value)], pairs [P][2] -> the clamped words float32 [P][174] and inside bool [P][174]"""
    llr = np.ascontiguousarray(llr, F32).reshape(-1, N)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    x = llr[pairs[:, 0]].copy()
    inside = np.zeros((len(pairs), N), bool)
    for p, (c, h) in enumerate(pairs):
        m, v = unword(hyps[h][0])[:MSG].astype(bool), unword(hyps[h][1])[:MSG].astype(bool)
        A = F32(F32(mag) * np.abs(llr[c]).max())                      # a maximum does not depend on order
        inside[p, :MSG] = m
        x[p, :MSG][m] = np.where(v[m], A, -A).astype(F32)             # -A is -0 where A is 0
    return x, inside


def decode(llr, hyps, pairs, n=None, mag=1.0, nerr_max=174, iters=30, alpha=0.8125):
    """-> (ap int32 [n][4], bits uint8 [n][12], detail int32 [P][4], pair bits uint8 [P][12])"""
    llr = np.ascontiguousarray(llr, F32).reshape(-1, N)
    n = len(llr) if n is None else n
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    first = pairs_ok(pairs, n, len(hyps))
    assert first is not None and all(hyp_ok(*h) for h in hyps)
    P = len(pairs)
    detail, pbits = np.zeros((P, 4), np.int32), np.zeros((P, 12), np.uint8)
    if P:
        x, inside = clamp(llr, hyps, pairs, mag)
        st, pbits, post = lo.decode(x, iters=iters, alpha=alpha)
        hard = post < 0
        value = np.zeros((P, N), bool)
        for p, (_, h) in enumerate(pairs):
            value[p, :MSG] = unword(hyps[h][1])[:MSG].astype(bool)
        nerr = (~inside & ((llr[pairs[:, 0]] > 0) != hard)).sum(axis=1)
        nap = (inside & (value != hard)).sum(axis=1)
        good = (st[:, 0] == 2) & (nap == 0) & (nerr <= nerr_max)
        detail[:, 0] = np.where(good, 2, np.minimum(st[:, 0], 1))
        detail[:, 1], detail[:, 2], detail[:, 3] = st[:, 1], nerr, nap
    ap, bits = pick(detail, pbits, first)
    return ap, bits, detail, pbits


def pick(detail, pbits, first):
    n = len(first) - 1
    ap, bits = np.zeros((n, 4), np.int32), np.zeros((n, 12), np.uint8)
    ap[:, 0] = -1
    for c in range(n):
        ok = [p for p in range(first[c], first[c + 1]) if detail[p, 0] == 2]
        if ok:
            best = min(ok, key=lambda p: (detail[p, 2], p))
            ap[c] = (best, detail[best, 1], detail[best, 2], len(ok))
            bits[c] = pbits[best]
    return ap, bits
