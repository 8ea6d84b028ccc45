"""NumPy model of the frame report and the row floor.  Test infrastructure only.

``report``: float32, every operation rounded on its own, vectorised over the candidates, the definition's sums in the
definition's order, so that the kernels (pysdr_amd/csrc/report.hip) and the scalar transcription (report_plan.h) can be held
against it bit for bit.  The ring is the one ``pysdr_ft8_state`` / ``pysdr_ft4_state`` deliver: P[nk][TR][NB], step t at
index t mod TR, with ``t_done`` steps complete.  ``available`` is the rule of a missing place, ``floor`` the row floor and its
refusal.  The frame's tones come from the encoder of ``pysdr_amd.ldpc`` and the oracles' own ``tones``.
"""
import numpy as np

from pysdr_amd import ldpc
from tests import ft4_oracle as f4o
from tests import ft8_oracle as f8o

F32 = np.float32
MISSING = F32(-1.0)
FT8, FT4 = 0, 1
SYMS = {FT8: 79, FT4: 103}
NTONES = {FT8: 8, FT4: 4}
SYNC = {FT8: sorted(f8o.SYNC_SYMS), FT4: [b + k for b in (0, 33, 66, 99) for k in range(4)]}
PLACES = [(dt, dF) for dt in (-1, 0, 1) for dF in (-1, 0, 1)]


def lag(mode):
    return 4 * (SYMS[mode] - 1)


def frame_tones(mode, bits91):
    """the 91 bits -> the codeword -> the frame's tones"""
    cw = ldpc.encode91(np.asarray(bits91).astype(np.uint8) & 1)
    return np.array((f8o if mode == FT8 else f4o).tones(cw), np.int64)


def time_ok(t, mode, t_done, tr):
    """a frame that begins at step t is whole, not before step 0 and still in the ring"""
    return t >= 0 and t + lag(mode) < t_done and t_done - t <= tr


def available(mode, F, t0, t_done, nfine, tr, circular):
    """-> bool [9], place (dt, dF) in ``PLACES`` order"""
    return np.array([time_ok(t0 + dt, mode, t_done, tr) and (circular or 0 <= F + dF < nfine) for dt, dF in PLACES])


def report(ring, t_done, nsub, circular, mode, F, t0, bits91):
    """-> (power float32 [n][10] = sig9 then tot, errs int32 [n][2] = nhard, nsync).  Every candidate obeys the rule of
    ``pysdr_*_llr`` (asserted)."""
    ring = np.asarray(ring)
    assert ring.dtype == F32
    nk, tr, nb = ring.shape
    nfine, nsym, T = nk * nsub, SYMS[mode], NTONES[mode]
    F, t0 = np.asarray(F, np.int64).reshape(-1), np.asarray(t0, np.int64).reshape(-1)
    n = len(F)
    bits91 = np.asarray(bits91).reshape(n, 91)
    tone = np.array([frame_tones(mode, b) for b in bits91]).reshape(n, nsym)
    sync = np.zeros(nsym, bool)
    sync[SYNC[mode]] = True
    power = np.full((n, 10), MISSING, F32)
    errs = np.zeros((n, 2), np.int32)
    for i in range(n):
        assert 0 <= F[i] < nfine and time_ok(int(t0[i]), mode, t_done, tr), (i, F[i], t0[i])
    if n == 0:
        return power, errs
    avail = np.array([available(mode, int(f), int(t), t_done, nfine, tr, circular) for f, t in zip(F, t0)])
    for place, (dt, dF) in enumerate(PLACES):
        ok = np.flatnonzero(avail[:, place])
        if not len(ok):
            continue
        Fn = (F[ok] + dF) % nfine                                              # in range wherever the place is available
        a, j = Fn // nsub, Fn % nsub
        acc = None
        for k in range(nsym):
            p = ring[a, (t0[ok] + dt + 4 * k) % tr, j + 2 * tone[ok, k]]
            acc = p if acc is None else acc + p                                 # float32 + float32, rounded once
        assert acc.dtype == F32
        power[ok, place] = acc
    a, j = F // nsub, F % nsub
    tot = None
    for k in range(nsym):
        P = ring[a[:, None], ((t0 + 4 * k) % tr)[:, None], j[:, None] + 2 * np.arange(T)[None, :]]   # [n][T]
        r = P[:, 0]
        for t in range(1, T):
            r = r + P[:, t]
        tot = r if tot is None else tot + r
        e = P[np.arange(n), tone[:, k]]
        miss = (~(e[:, None] > P) & (np.arange(T)[None, :] != tone[:, k][:, None])).any(axis=1)
        errs[:, 1 if sync[k] else 0] += miss
    assert tot.dtype == F32
    power[:, 9] = tot
    return power, errs


def floor_ok(t_end, nsym, t_done, tr):
    first = t_end - 4 * (nsym - 1)
    return 1 <= nsym <= 128 and first >= 0 and t_end < t_done and t_done - first <= tr


def floor(ring, t_done, t_end, nsym):
    """-> float32 [nk][NB]: every bin over the nsym steps, four apart, that end at t_end, ascending; None where refused"""
    ring = np.asarray(ring)
    tr = ring.shape[1]
    if not floor_ok(t_end, nsym, t_done, tr):
        return None
    acc = None
    for i in range(nsym):
        p = ring[:, (t_end - 4 * (nsym - 1 - i)) % tr, :]
        acc = p.copy() if acc is None else acc + p
    assert acc.dtype == F32
    return acc
