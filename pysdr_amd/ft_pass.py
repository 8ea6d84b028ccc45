"""The second pass of the FT8 and FT4 skimmers: its tables and trial grid, derived here in float64 and
rounded once, and its policy -- which decoded frames wait, when they are due, what of the residue becomes a record -- as one
object the skimmer holds.  ``mode`` is a mode's module (``ft8.py``, ``ft4.py``), read for its pulse, trial steps and holds."""
from __future__ import annotations

import math

import numpy as np

from . import _lib
from . import ldpc as _ldpc
from .ft_report import refine

PASS_TRIALS, PASS_MAX, PASS_LUT, PASS_EVENT_CAP, PASS_ROWS_MAX, PASS_WINDOW_MAX = 9, 256, 4096, 52, 256, 256


def pass_pulse(mode, S):
    """uint32 [PULSE_SYMBOLS S]: the phase one symbol of tone 1 has added by row sample i of the symbols its frequency
    pulse spans, 2^32 a turn: the cumulative sum of ``waveform``'s pulse at the samples' middles, scaled so that the
    whole pulse is exactly one turn (which the last entry holds as 0)."""
    P = mode.PULSE_SYMBOLS
    tau = (np.arange(P * S) + 0.5) / S - P / 2
    erf = np.vectorize(math.erf)
    g = 0.5 * (erf(mode.PULSE_K * (tau + 0.5)) - erf(mode.PULSE_K * (tau - 0.5)))
    c = np.cumsum(g)
    return np.ascontiguousarray((np.rint(c / c[-1] * 2.0 ** 32).astype(np.uint64) & 0xFFFFFFFF).astype(np.uint32))


def pass_lut():
    """float32 [4096][2] = (cos, sin)(2 pi i / 4096)"""
    t = 2 * np.pi * np.arange(PASS_LUT) / PASS_LUT
    return np.ascontiguousarray(np.stack((np.cos(t), np.sin(t)), axis=1), np.float32)


def pass_plan(mode, nk, S, max_out, reach_t=None):
    """What a second pass keeps and launches (no device needed): dict of threads, LDS bytes, ty (samples of a row kept),
    tr2 (steps kept), jobs and frames per subtract call, events per fine row of a rescan, symbols of the pulse."""
    v = _lib.plan_call("pysdr_pass_plan", 8, int(mode.REPORT_MODE), int(nk), int(S), int(max_out), int(mode.REACH_T if reach_t is None else reach_t))
    return dict(zip(("threads", "lds_bytes", "ty", "tr2", "max_jobs", "max_frames", "event_cap", "pulse_symbols"), v))


def trial_grid(mode, df, dt, qs, fs_out):
    """int32 [9][2] = (dn, fw): the refined offsets ``df`` (raster steps of baud / 2) and ``dt`` (steps) -> 3 times (outer)
    x 3 frequencies (inner) around them: dn in row samples, fw the phase word per row sample.  ``subtract`` refuses a dn of
    a step or more, so a trial time beyond QS - 1 samples is MOVED to QS - 1 (-(QS - 1)): that trial is then not the one the
    grid asked for.  ``refine`` leaves |dt| <= 0.5, so only the outer trials of a frame half a step off are moved, by at
    most QS / 4 - 1 samples."""
    out = np.zeros((9, 2), np.int64)
    for a, it in enumerate((-1, 0, 1)):
        dn = int(np.clip(np.rint((dt + it * mode.TRIAL_DN) * qs), -(qs - 1), qs - 1))
        for b, jf in enumerate((-1, 0, 1)):
            hz = df * mode.BAUD / 2 + jf * mode.TRIAL_DF
            out[3 * a + b] = dn, int(np.rint(hz / fs_out * 2.0 ** 32))
    return (out & 0xFFFFFFFF).astype(np.uint32).view(np.int32)              # (dn as its two's complement, which int32 reads back)


def pack91(bits91, n):
    """uint8 [n][91] -> [n][12], MSB first, as the decoder packs them"""
    b = np.ascontiguousarray(bits91, np.uint8).reshape(n, _ldpc.K) & 1
    return np.ascontiguousarray(np.packbits(np.concatenate((b, np.zeros((n, 5), np.uint8)), axis=1), axis=1))


class SecondPass:
    """The second pass of one skimmer ``sk``, in absolute steps.  ``hold`` takes a release's records: the decoded ones wait
    here, with their bits and refined place.  A waiting frame is due once step t0 + HOLD + reach_t - 1 is complete; ``run``
    takes the due frames in ascending t0, those of one t0 together: subtract them, rescan the residue around each (F -+ (2
    TONES + 2) fine rows inside the raster, t0 -+ reach_t), keep the owners among the new events that are not within (4
    steps, 2 fine rows) of a decoded record with t0' <= t0 + reach_t (every such record has been released by then, however
    the stream was cut), decode them from the residue and keep the messages that are not one of those records' within 8
    steps.  The skimmer is handed in with every call, not held: the two do not own each other."""

    def __init__(self, sk):
        sk.dec.keep(sk.reach_t)
        self.reset()

    def reset(self):
        self.waiting, self.ok = [], []                                   # (record, its 91 bits, df, dt) not yet due; every ok record still in reach

    def hold(self, sk, recs, bits):
        """pass-1 records gain ``pass``; the decoded ones wait until they are due"""
        for r in recs:
            r["pass"] = 1
        good = [k for k, r in enumerate(recs) if r["ok"]]
        if not good:
            return
        rep = sk.dec.report([recs[k]["F"] for k in good], [recs[k]["t0"] for k in good], bits[good])
        for i, k in enumerate(good):
            df, dt, _ = refine(rep["sig9"][i])
            self.waiting.append((recs[k], bits[k].copy(), df, dt))
            self.ok.append(recs[k])

    def run(self, sk):
        """-> the records of pass 2 that the frames now due uncover"""
        m, R, done, dec = sk.DECODERS.MODE, sk.reach_t, sk.dec.t_done, sk.dec
        due = [a for a in self.waiting if a[0]["t0"] + m.HOLD + R <= done]
        if not due:
            return []
        self.waiting = [a for a in self.waiting if a[0]["t0"] + m.HOLD + R > done]
        due.sort(key=lambda a: (a[0]["t0"], a[0]["F"]))
        out, W = [], 2 * m.TONES + 2
        for t0 in sorted({a[0]["t0"] for a in due}):
            grp = [a for a in due if a[0]["t0"] == t0]
            Fs = [a[0]["F"] for a in grp]
            trials = np.array([trial_grid(m, a[2], a[3], sk.qs, sk.fs_out) for a in grp], np.int32)
            dec.subtract(Fs, [t0] * len(grp), np.array([a[1] for a in grp]), trials)
            found = {}
            for F in Fs:
                for e in dec.rescan(max(0, F - W), min(sk.nfine - 1, F + W), max(0, t0 - R), t0 + R):
                    found[(e[0], e[1])] = e
            events = sorted(found.values())
            known = [r for r in self.ok if r["t0"] <= t0 + R]
            cand = [e for e, o in zip(events, sk._owners(events))
                    if o and not any(abs(e[0] - r["t0"]) <= 4 and sk._fdist(e[1], r["F"]) <= 2 for r in known)]
            if not cand:
                continue
            cF, ct = [e[1] for e in cand], [e[0] for e in cand]
            answer = dec.decode(cF, ct, sk.ldpc, osd=sk.osd, residual=True)
            llr = dec.pass_llr(cF, ct) if sk.keep_llr else None
            for k, e in enumerate(cand):
                rec = sk._decoded(sk._record(*e, None if llr is None else llr[k]), answer, k)
                if not rec["ok"] or any(abs(r["t0"] - rec["t0"]) <= 8 and np.array_equal(r["bits77"], rec["bits77"]) for r in known):
                    continue
                rec["pass"] = 2
                known.append(rec)
                self.ok.append(rec)
                out.append(rec)
            self.ok = [r for r in self.ok if r["t0"] >= t0 - R - 8]       # older ones meet no later group
        return out
