"""NumPy model of ordered-statistics decoding behind min-sum.  Test infrastructure only.

``osd_word``: one candidate, steps 1 to 8 of the definition in the definition's order, with everything a test may want to
look at (perm, piv, G', e0, the patterns).  ``decode``: min-sum (tests/ldpc_oracle.py) and then steps 1 to 11 on every
candidate it left without a message, so that the kernel (pysdr_amd/csrc/osd.hip) and the scalar transcription
(osd_plan.h) can be held against it for equality.  The distance is a loop over the 174 ranks with the patterns as a
vector, every add rounded in float32 on its own -- not ``np.sum``, whose pairwise order is not the definition's.
"""
import numpy as np

from pysdr_amd import ldpc
from tests import ldpc_oracle as lo

F32 = np.float32
N, K = 174, 91
PATTERNS = (1, 92, 4187)
G = np.concatenate((np.eye(K, dtype=np.uint8), ldpc.GENERATOR.T), axis=1)      # [91][174]: the systematic generator
G.setflags(write=False)
PAIRS = np.array([(i, j) for i in range(K) for j in range(i + 1, K)], np.int64)  # lexicographic
PAIRS.setflags(write=False)


def k_of(i, j=None):
    """(i,) or (i, j), i < j -> k"""
    if j is None:
        return 1 + i
    return 1 + K + i * (2 * K - 1 - i) // 2 + (j - i - 1)


def ij_of(k):
    """k -> (), (i,) or (i, j)"""
    if k == 0:
        return ()
    if k <= K:
        return (k - 1,)
    return tuple(int(v) for v in PAIRS[k - 1 - K])


def basis(x):
    """steps 1 to 4 -> (r float32 [174], h uint8 [174], perm, piv int [91], G' uint8 [91][174] in rank order)"""
    x = np.asarray(x, F32).reshape(N)
    r = np.abs(x)                                                               # step 1: -0 gives +0
    h = (x > 0).astype(np.uint8)
    perm = np.argsort(-r, kind="stable")                                        # step 2: descending r, ties by ascending n
    A = G[:, perm].astype(bool)                                                 # the generator in rank order
    free = np.ones(K, bool)                                                     # rows that hold no pivot yet
    piv, row_of = [], []
    for p in range(N):                                                          # step 3
        cand = np.flatnonzero(A[:, p] & free)
        if not len(cand):
            continue                                                            # dependent on the columns kept so far
        row = cand[0]
        others = np.flatnonzero(A[:, p])
        A[others[others != row]] ^= A[row]
        free[row] = False
        piv.append(p)
        row_of.append(row)
        if len(piv) == K:
            break
    assert len(piv) == K
    return r, h, perm, np.array(piv), A[row_of].astype(np.uint8)                # step 4: row i has its 1 at rank piv[i]


def patterns(h_ranked, piv, Gp, order):
    """steps 5 and 6 -> uint8 [patterns][174] in rank order, row k the pattern of index k"""
    c0 = (h_ranked[piv].astype(np.int64) @ Gp.astype(np.int64) % 2).astype(np.uint8)
    e0 = c0 ^ h_ranked
    out = [e0[None]]
    if order >= 1:
        out.append(e0[None] ^ Gp)
    if order >= 2:
        out.append(e0[None] ^ Gp[PAIRS[:, 0]] ^ Gp[PAIRS[:, 1]])
    return np.concatenate(out)


def distances(pat, r_ranked):
    """step 7: float32, one add per rank in rank order, only where the pattern's bit is set"""
    d = np.zeros(len(pat), F32)
    for p in range(N):
        on = pat[:, p] != 0
        d[on] = d[on] + r_ranked[p]
    return d


def osd_word(x, order=2):
    """-> dict of k, last, weight, dist (float32), word uint8 [174] in transmission order, and perm, piv, Gp, pat (the
    patterns, in rank order), d (their distances)"""
    r, h, perm, piv, Gp = basis(x)
    pat = patterns(h[perm], piv, Gp, order)
    assert len(pat) == PATTERNS[order]
    d = distances(pat, r[perm])
    k = int(np.flatnonzero(d == d.min())[0])                                    # step 8: the least, a tie to the lower k
    word = np.zeros(N, np.uint8)
    word[perm] = h[perm] ^ pat[k]                                               # step 9
    return dict(k=k, last=int(piv[-1]), weight=int(pat[k].sum()), dist=d[k], word=word, perm=perm, piv=piv, Gp=Gp, pat=pat, d=d,
                h=h, r=r)


def accept(word):
    return bool(word[:77].any() and ldpc.crc_ok(word[:K]))


def decode(llr, iters=30, alpha=0.8125, order=2):
    """llr float32 [B][174] -> (status int32 [B][4], bits uint8 [B][12], post float32 [B][174], detail int32 [B][4]): min-sum's
    answer, and on every candidate whose status is not 2, steps 1 to 11."""
    llr = np.ascontiguousarray(llr, F32).reshape(-1, N)
    status, bits, post = lo.decode(llr, iters=iters, alpha=alpha)
    status, bits = status.copy(), bits.copy()
    detail = np.zeros((len(llr), 4), np.int32)
    detail[:, :3] = -1
    for b in np.flatnonzero(status[:, 0] != 2):
        w = osd_word(llr[b], order)
        if accept(w["word"]):
            status[b, 0], status[b, 2] = 2, w["weight"]
            bits[b] = np.packbits(np.concatenate((w["word"][:K], np.zeros(5, np.uint8))))
        status[b, 3] = 1 if w["k"] == 0 else 2 if w["k"] <= K else 3
        detail[b] = (w["k"], w["last"], w["weight"], int(np.array([w["dist"]], F32).view(np.int32)[0]))
    return status, bits, post, detail
