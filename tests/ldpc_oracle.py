"""NumPy model of the LDPC(174,91) decoder.  Test infrastructure only.

``decode``: normalised min-sum on a flooding schedule, float32, every operation rounded on its own, vectorised over the
candidates; the definition's steps in the definition's order, so that the kernel (pysdr_amd/csrc/ldpc.hip) and the scalar
transcription (ldpc_plan.h) can be held against it bit for bit.  Zeros and signs: a message's magnitude is
f32(alpha * min) >= +0 and a negative sign negates it, so a zero minimum under a negative sign gives -0; -0 counts as
positive wherever a sign is taken (``v < 0`` is false) and as zero in every sum.
``derive_checks``: the sparse parity checks from the generator alone, by the search of the definition.
"""
import hashlib

import numpy as np

from pysdr_amd import ldpc

F32 = np.float32
N, K, M, EDGES = 174, 91, 83, 522
DEG = np.diff(ldpc.CHECK_BASE)
# edges of a check, padded to 7 with an edge that does not exist (index 522: a column of +inf / no sign)
PAD = np.full((M, 7), EDGES, np.int64)
for _m in range(M):
    PAD[_m, :DEG[_m]] = np.arange(ldpc.CHECK_BASE[_m], ldpc.CHECK_BASE[_m + 1])
E0, E1, E2 = (ldpc.COL_EDGES[:, s].astype(np.int64) for s in range(3))


def decode(llr, iters=30, alpha=0.8125):
    """llr float32 [B][174], positive for bit 1 -> (status int32 [B][4] = status, iterations, nerr, 0; bits uint8 [B][12];
    post float32 [B][174], the final tot)"""
    llr = np.ascontiguousarray(llr, F32).reshape(-1, N)
    B = llr.shape[0]
    alpha = F32(alpha)
    L = -llr
    c = np.zeros((B, EDGES), F32)
    post = np.zeros((B, N), F32)
    hard_out = np.zeros((B, N), np.uint8)
    status = np.zeros((B, 4), np.int32)
    act = np.arange(B)
    Ht = ldpc.H.T.astype(np.int64)
    for k in range(int(iters) + 1):
        if not len(act):
            break
        La, ca = L[act], c[act]
        c0, c1, c2 = ca[:, E0], ca[:, E1], ca[:, E2]
        tot = ((La + c0) + c1) + c2                                   # step 1
        hard = tot < 0                                                # step 2
        conv = ~((hard.astype(np.int64) @ Ht) % 2).any(axis=1)        # step 3
        stop = conv | (k == int(iters))                               # step 4
        if stop.any():
            idx = act[stop]
            post[idx], hard_out[idx] = tot[stop], hard[stop]
            status[idx, 0] = conv[stop]                               # 1: a codeword; the CRC is judged below
            status[idx, 1] = k
        keep = ~stop
        act = act[keep]
        if not len(act):
            break
        La, c0, c1, c2 = La[keep], c0[keep], c1[keep], c2[keep]
        v = np.empty((len(act), EDGES + 1), F32)                      # step 5
        v[:, E0] = (La + c1) + c2
        v[:, E1] = (La + c0) + c2
        v[:, E2] = (La + c0) + c1
        v[:, EDGES] = np.inf
        vm = v[:, PAD]                                                # [b][83][7]
        mag, neg = np.abs(vm), vm < 0
        order = np.argsort(mag, axis=2, kind="stable")
        first = order[:, :, :1]
        m1 = np.take_along_axis(mag, first, 2)
        m2 = np.take_along_axis(mag, order[:, :, 1:2], 2)
        others = np.where(np.arange(7)[None, None, :] == first, m2, m1)   # step 6: the minimum over the other edges
        out = alpha * others
        flip = (neg.sum(axis=2, keepdims=True) % 2).astype(bool) ^ neg    # the product of the other edges' signs
        out = np.where(flip, -out, out).astype(F32)
        cn = np.empty((len(act), EDGES + 1), F32)
        cn[:, PAD.reshape(-1)] = out.reshape(len(act), -1)
        c[act] = cn[:, :EDGES]
    nerr = ((llr > 0) != (hard_out > 0)).sum(axis=1)
    status[:, 2] = nerr
    bits = np.packbits(np.concatenate((hard_out[:, :K], np.zeros((B, 5), np.uint8)), axis=1), axis=1)
    for i in np.flatnonzero(status[:, 0]):
        b = hard_out[i, :K]
        if b[:77].any() and ldpc.crc_ok(b):
            status[i, 0] = 2
    return status, bits, post


def derive_checks(seed=0, rounds=20):
    """All words of weight <= 7 of the dual code that Gaussian elimination of [P^T | I] on random pivot sets and sums of two
    of its rows reach: -> sorted list of ascending column tuples"""
    rng = np.random.default_rng(seed)
    Hd = np.concatenate((ldpc.GENERATOR, np.eye(M, dtype=np.uint8)), axis=1).astype(bool)   # [83][174]: rows span the dual code
    found = set()
    for _ in range(rounds):
        A = Hd.copy()
        perm = rng.permutation(N)
        r = 0
        for col in perm:
            if r == M:
                break
            piv = np.flatnonzero(A[r:, col])
            if not len(piv):
                continue
            p = r + piv[0]
            if p != r:
                A[[r, p]] = A[[p, r]]
            rows = np.flatnonzero(A[:, col])
            rows = rows[rows != r]
            A[rows] ^= A[r]
            r += 1
        assert r == M
        w = A.sum(axis=1)
        for row in A[w <= 7]:
            found.add(tuple(int(v) for v in np.flatnonzero(row)))
        Ai = A.astype(np.int32)
        # weight of a sum of two rows: w_a + w_b - 2 overlap
        ov = Ai @ Ai.T
        w2 = w[:, None] + w[None, :] - 2 * ov
        for a, b in zip(*np.nonzero(np.triu(w2 <= 7, 1))):
            found.add(tuple(int(v) for v in np.flatnonzero(A[a] ^ A[b])))
    return sorted(found)


def checks_sha256(rows):
    text = "".join(" ".join(str(v) for v in r) + "\n" for r in rows)
    return hashlib.sha256(text.encode()).hexdigest()
