"""NumPy model of the FT8 / FT4 second pass.  Test infrastructure only.

``PassOracle`` wraps a float32 ``ft8_oracle.Oracle`` / ``ft4_oracle.Oracle`` and holds what ``pysdr_*_keep`` makes the library
hold, as ``pysdr_*_pass_state`` delivers it: the sample ring ``yk`` [nk][TY] (row sample n at n mod TY) and the residue ring
``ring2`` [nk][TR2][NB] (step t at t mod TR2).  ``process`` is the oracle's call plus the keeping; ``subtract`` the definition
of a subtraction -- the rows of a frame, the integer phase of the reference, the amplitudes of every trial, the choice, the
subtraction, the four words per job -- in float32 with every operation rounded on its own and every sum in the definition's
order, followed by the respectrum of the steps the frame touches (the wrapped oracle's own ``spectrum``); ``rescan`` the sync
score and the peak rule on the residue.  The tables (``pulse``, ``lut``) and the phase word are derived here from the
definition, independently of ``pysdr_amd.ft8``.  ``frame_power`` sums a frame's own bins of the residue.  ``subtract64`` / ``bins64`` are a float64 model of the same
definition on one row; ``Skimmer`` is the skimmer with ``passes``: ``FT8_Skimmer.push``'s policy written again on the models.
"""
import math

import numpy as np

from tests import ft4_oracle as f4o
from tests import ft8_oracle as f8o
from tests import report_oracle as ro

F32 = np.float32
FT8, FT4 = ro.FT8, ro.FT4
MASK = (1 << 32) - 1
LUT_BITS = 12
MARGIN = 4
EVENT_CAP = 52
PULSE_SYMS = {FT8: 3, FT4: 5}
PULSE_K = {FT8: 2 * math.pi * math.sqrt(2 / math.log(2)), FT4: math.pi * math.sqrt(2 / math.log(2))}
EXTRA = {FT8: 14, FT4: 6}
HOLD = {FT8: f8o.HOLD, FT4: 417}


def pulse(mode, S):
    """int [P S]: the phase of one symbol of tone 1 after row sample i of its pulse's span, 2^32 a turn, mod 2^32"""
    P = PULSE_SYMS[mode]
    g = []
    for i in range(P * S):
        tau = (i + 0.5) / S - P / 2
        g.append(0.5 * (math.erf(PULSE_K[mode] * (tau + 0.5)) - math.erf(PULSE_K[mode] * (tau - 0.5))))
    c = np.cumsum(np.array(g, np.float64))
    return [int(v) & MASK for v in np.rint(c / c[-1] * 2.0 ** 32)]


def lut():
    t = 2 * np.pi * np.arange(1 << LUT_BITS, dtype=np.float64) / (1 << LUT_BITS)
    return np.cos(t).astype(F32), np.sin(t).astype(F32)


def word(q, S):
    """round(q 2^32 / (4 S)), half up, mod 2^32"""
    return ((q * (1 << 31) + S) // (2 * S)) & MASK


def ring_steps2(mode, max_out, S, reach_t):
    return HOLD[mode] + 2 * reach_t + MARGIN + max_out // (S // 4) + 1


def ring_samples(tr2, S):
    return (S // 4 * tr2 + S + 15) & ~15


def frame_rows(mode, F, S, nk, circular):
    """the rows that hold tones of fine row F -> [(row, q of tone 0 in that row)]"""
    nsub, extra = S // 2, EXTRA[mode]
    a, j = divmod(int(F), nsub)
    out = [(a, 2 * j - (nsub + extra - 1))]
    if j + extra >= nsub:
        nbr, dq = a + 1, -2 * nsub
    elif j <= extra - 1:
        nbr, dq = a - 1, 2 * nsub
    else:
        return out
    if circular:
        nbr %= nk
    if 0 <= nbr < nk and nbr != a:
        out.append((nbr, out[0][1] + dq))
    return out


def phases(mode, S, tones, pl, w):
    """int64 [NS][S]: the reference's phase at sample m of symbol k, mod 2^32"""
    NS, H = len(tones), PULSE_SYMS[mode] // 2
    pl = np.array(pl, np.int64)
    k = np.arange(NS)[:, None]
    m = np.arange(S)[None, :]
    ph = ((S * k + m) * int(w)) & MASK
    tn = np.asarray(tones, np.int64)
    for d in range(-H, H + 1):
        kk = np.clip(k + d, 0, NS - 1)
        ph = (ph + tn[kk] * pl[(H - d) * S + m]) & MASK
    return ph


def lut_index(ph):
    return ((ph + (1 << (31 - LUT_BITS))) & MASK) >> (32 - LUT_BITS)


class PassOracle:
    def __init__(self, mode, o, reach_t, circular, trials=9):
        self.mode, self.o, self.reach_t, self.circular, self.ntr = mode, o, int(reach_t), bool(circular), int(trials)
        self.S, self.qs, self.nk = o.S, o.qs, o.nk
        self.lag = ro.lag(mode)
        self.tr2 = ring_steps2(mode, o.max_out, o.S, reach_t)
        self.ty = ring_samples(self.tr2, o.S)
        self.pulse, (self.cos, self.sin) = pulse(mode, o.S), lut()
        self.sync_scores = (f8o if mode == FT8 else f4o).sync_scores
        self.reset()

    def reset(self):
        self.o.reset()
        self.yk = np.zeros((self.nk, self.ty), np.complex64)
        self.ring2 = np.zeros((self.nk, self.tr2, self.o.nb), F32)
        self.n_abs = 0

    def process(self, rows):
        rows = np.asarray(rows, np.complex64)
        t_first, m0 = self.o.t_done, self.o.m
        out = self.o.process(rows)
        n = rows.shape[1]
        if n:
            self.yk[:, (m0 + np.arange(n)) % self.ty] = rows
            t = np.arange(t_first, self.o.t_done)
            self.ring2[:, t % self.tr2] = self.o.ring[:, t % self.o.tr]
            self.n_abs = m0 + n
        return out

    def state(self):
        return dict(yk=self.yk.copy(), ring2=self.ring2.copy(), n_kept=self.n_abs)

    def first_step(self):
        return max(0, self.o.t_done - self.tr2)

    def frame_ok(self, t0):
        return t0 >= 0 and t0 + self.lag + MARGIN < self.o.t_done and max(0, t0 - MARGIN) >= self.first_step()

    def window_ok(self, t_lo, t_hi):
        return t_hi + 4 + self.lag < self.o.t_done and max(0, t_lo - 4) >= self.first_step()

    def _symbols(self, row, n0):
        """the S samples of every symbol that starts at n0[k] -> (yr, yi float32 [NS][S], used bool [NS])"""
        n_lo, n_hi = max(0, self.n_abs - self.ty), self.n_abs
        idx = n0[:, None] + np.arange(self.S)[None, :]
        used = (n0 >= n_lo) & (n0 + self.S - 1 < n_hi)
        y = self.yk[row, idx % self.ty]
        return np.ascontiguousarray(y.real), np.ascontiguousarray(y.imag), used, idx % self.ty

    def job(self, row, q, t0, tones, trials):
        """one job -> (before, after, trial, used); ``yk`` of the row is changed"""
        S, NS = self.S, len(tones)
        inv = F32(1) / F32(S)
        amps, scores, refs, useds = [], [], [], []
        for dn, fw in trials:
            w = (word(q, S) + (int(fw) & MASK)) & MASK
            ix = lut_index(phases(self.mode, S, tones, self.pulse, w))
            c, s = self.cos[ix], self.sin[ix]
            yr, yi, used, _ = self._symbols(row, self.qs * t0 + int(dn) + S * np.arange(NS))
            vr, vi = yr * c + yi * s, yi * c - yr * s
            sr, si = vr[:, 0], vi[:, 0]
            for m in range(1, S):
                sr, si = sr + vr[:, m], si + vi[:, m]
            ar, ai = np.where(used, sr * inv, F32(0)), np.where(used, si * inv, F32(0))
            p = ar * ar + ai * ai
            acc = p[0]
            for k in range(1, NS):
                acc = acc + p[k]
            amps.append((ar, ai)), scores.append(acc), refs.append((c, s)), useds.append(used)
        best = 0
        for i in range(1, len(trials)):
            if scores[i] > scores[best]:
                best = i
        (ar, ai), (c, s), used = amps[best], refs[best], useds[best]
        yr, yi, _, at = self._symbols(row, self.qs * t0 + int(trials[best][0]) + S * np.arange(NS))
        zr = yr - (ar[:, None] * c - ai[:, None] * s)
        zi = yi - (ar[:, None] * s + ai[:, None] * c)
        b, a = yr * yr + yi * yi, zr * zr + zi * zi
        pb, pa = b[:, 0], a[:, 0]
        for m in range(1, S):
            pb, pa = pb + b[:, m], pa + a[:, m]
        before = after = F32(0)
        first = True
        for k in np.flatnonzero(used):
            before, after = (pb[k], pa[k]) if first else (before + pb[k], after + pa[k])
            first = False
            self.yk[row, at[k]] = (zr[k] + 1j * zi[k]).astype(np.complex64)
        assert np.asarray(before).dtype == F32 and zr.dtype == F32
        return F32(before), F32(after), best, int(used.sum())

    def respectrum(self, row, t_lo, t_hi):
        """the steps t_lo .. t_hi of ``ring2`` of a row from ``yk`` (those from step 0 on)"""
        t = np.arange(max(0, t_lo), t_hi + 1)
        n_a = self.qs * int(t[0])
        ext = self.yk[row, (n_a + np.arange(self.qs * (len(t) - 1) + self.S)) % self.ty][None, :]
        self.ring2[row, t % self.tr2] = self.o.spectrum(ext, self.qs * (t - t[0]))[0]

    def subtract(self, F, t0, bits91, trials):
        """-> dict of before, after float32 [n][2], trial, used int32 [n][2], as ``FT8_Decoders.subtract`` answers"""
        n = len(F)
        trials = np.asarray(trials).reshape(n, self.ntr, 2)
        assert all(self.frame_ok(int(t)) for t in t0) and (np.abs(trials[:, :, 0].astype(np.int64)) < self.qs).all()
        out = dict(before=np.zeros((n, 2), F32), after=np.zeros((n, 2), F32), trial=np.zeros((n, 2), np.int32), used=np.zeros((n, 2), np.int32))
        touched = []
        for i in range(n):
            tones = ro.frame_tones(self.mode, bits91[i])
            for r, (row, q) in enumerate(frame_rows(self.mode, F[i], self.S, self.nk, self.circular)):
                b, a, tr, u = self.job(row, q, int(t0[i]), tones, [(int(d), int(w)) for d, w in trials[i]])
                out["before"][i, r], out["after"][i, r], out["trial"][i, r], out["used"][i, r] = b, a, tr, u
                touched.append((row, int(t0[i])))
        for row, t in touched:
            self.respectrum(row, t - MARGIN, t + self.lag + MARGIN)
        return out

    def rescan(self, F_lo, F_hi, t_lo, t_hi, p=None):
        """-> events (t0, F, score, hits) sorted by (F, t0)"""
        p = self.o.p if p is None else p
        assert self.window_ok(t_lo, t_hi) and t_hi - t_lo + 9 <= 256
        ts = np.arange(max(0, t_lo - 4), t_hi + 5)
        score, hits = self.sync_scores(f8o._Unrolled(self.ring2, self.tr2), ts, self.o.nsub, F32)
        score, hits = score.transpose(1, 0, 2).reshape(len(ts), -1), hits.transpose(1, 0, 2).reshape(len(ts), -1)
        out = []
        for F in range(F_lo, F_hi + 1):
            sc = lambda t: score[t - ts[0], F] if t >= ts[0] else F32(0)     # noqa: E731
            hi = lambda t: hits[t - ts[0], F] if t >= ts[0] else 0          # noqa: E731
            for tc in range(t_lo, t_hi + 1):
                if f8o.is_peak(sc, hi, tc, p):
                    out.append((tc, F, float(sc(tc)), int(hi(tc))))
        return out

    def llr(self, F, t0):
        """the soft bits of (F, t0) from the residue"""
        ring, tr = self.o.ring, self.o.tr
        try:
            self.o.ring, self.o.tr = self.ring2, self.tr2
            return self.o.llr(F, t0)
        finally:
            self.o.ring, self.o.tr = ring, tr


def frame_power(ring2, tr2, nsub, F, t0, tones):
    """the sum of the residue's powers in the frame's own bins, float64"""
    a, j = divmod(int(F), nsub)
    return float(sum(float(ring2[a, (t0 + 4 * k) % tr2, j + 2 * int(tn)]) for k, tn in enumerate(tones)))


# ---- a float64 model of the same definition: the same integer phases, the table and every sum in float64 -----------------
def subtract64(mode, S, y, n0, q, tones, trials):
    """One job on one row in float64: y complex128 [n] (the row from sample 0, all of it held), n0 = QS t0 -> (the row
    after the subtraction, the trial chosen).  The phases are the definition's integers; the cos / sin table holds float64
    values; a symbol with a sample before sample 0 is left alone."""
    NS = len(tones)
    pl = pulse(mode, S)
    t = 2 * np.pi * np.arange(1 << LUT_BITS) / (1 << LUT_BITS)
    best = None
    for i, (dn, fw) in enumerate(trials):
        w = (word(q, S) + (int(fw) & MASK)) & MASK
        ix = lut_index(phases(mode, S, tones, pl, w))
        r = np.cos(t)[ix] + 1j * np.sin(t)[ix]                       # [NS][S]
        at = n0 + int(dn) + S * np.arange(NS)
        used = (at >= 0) & (at + S <= len(y))
        idx = np.clip(at[:, None] + np.arange(S)[None, :], 0, len(y) - 1)
        a = np.where(used, (y[idx] * np.conj(r)).sum(axis=1) / S, 0)
        score = float((np.abs(a) ** 2).sum())
        if best is None or score > best[0]:
            best = (score, i, a, r, idx, used)
    _, i, a, r, idx, used = best
    z = y.copy()
    for k in np.flatnonzero(used):
        z[idx[k]] = y[idx[k]] - a[k] * r[k]
    return z, i


def bins64(mode, S, y, F_j, t0, tones):
    """the power of row y in the frame's own bins, float64: sum over k of |step t0 + 4 k's bin j + 2 tone[k]|^2"""
    nb, qs = S // 2 + EXTRA[mode], S // 4
    out = 0.0
    i = np.arange(S)
    for k, tn in enumerate(tones):
        qb = 2 * (F_j + 2 * int(tn)) - (nb - 1)
        n = qs * (t0 + 4 * k)
        out += abs((y[n:n + S] * np.exp(-2j * np.pi * qb * i / (4 * S))).sum()) ** 2
    return out


# ---- the skimmer with a second pass: FT8_Skimmer.push's policy, written again on the models -------------------------------
TONES = {FT8: 8, FT4: 4}
BAUD = {FT8: f8o.BAUD, FT4: f4o.BAUD}
TRIAL_DN, TRIAL_DF = 0.25, {FT8: 0.3, FT4: 1.0}                      # steps, Hz between the trials


def delta(a, b, c):
    """the peak of the parabola through three points, from the middle one, within half a point; 0 where one is missing"""
    if a < 0 or c < 0:
        return 0.0
    d = a - 2 * b + c
    if d < 0:
        return min(0.5, max(-0.5, 0.5 * (a - c) / d))
    return 0.5 * float(np.sign(c - a))


def refine(sig9):
    s = np.asarray(sig9, np.float64).reshape(3, 3)
    return delta(s[1, 0], s[1, 1], s[1, 2]), delta(s[0, 1], s[1, 1], s[2, 1])


def trial_grid(mode, df, dt, qs, fs_out):
    """3 times (outer) x 3 frequencies around the refined offsets -> [(dn, fw)]"""
    out = []
    for it in (-1, 0, 1):
        dn = int(min(qs - 1, max(-(qs - 1), np.rint((dt + it * TRIAL_DN) * qs))))
        for jf in (-1, 0, 1):
            out.append((dn, int(np.rint((df * BAUD[mode] / 2 + jf * TRIAL_DF[mode]) / fs_out * 2.0 ** 32)) & MASK))
    return out


class Skimmer:
    """rows [nk][n] -> calls -> held events -> finder -> decoded records, and with ``passes=2`` the second pass: a decoded
    frame is due once step t0 + hold + reach_t - 1 is complete; due frames in ascending t0, those of one t0 together in
    ascending F; subtract, rescan, finder, drop what is within (4 steps, 2 fine rows) of a decoded record with t0' <= t0 +
    reach_t, decode the rest from the residue, keep the messages that are not one of those records' within 8 steps."""

    def __init__(self, mode, nk, S, circular, max_out=256, passes=1, reach_t=40, p=None, iters=30):
        om = f8o if mode == FT8 else f4o
        self.mode, self.om, self.passes, self.R, self.iters = mode, om, passes, int(reach_t), iters
        self.p = PassOracle(mode, om.Oracle(nk, S, om.params() if p is None else p, max_out), reach_t, circular)
        self.o, self.circular, self.max_out = self.p.o, circular, max_out
        self.fs_out = S * BAUD[mode]
        self.events, self.released, self.records, self.wait, self.ok = [], set(), [], [], []

    def decode(self, soft):
        from pysdr_amd import ldpc
        from tests import ldpc_oracle as lo
        st, bits, _ = lo.decode(np.array(soft, F32), iters=self.iters)
        return st, ldpc.unpack_bits(bits)

    def push(self, rows, cuts=None):
        """``cuts``: the outputs of each call (default: max_out each)"""
        out, at = [], 0
        cuts = [self.max_out] * (-(-rows.shape[1] // self.max_out)) if cuts is None else cuts
        for n in cuts:
            out += self.call(rows[:, at:at + n])
            at += n
        assert at >= rows.shape[1]
        self.records += out
        return out

    def call(self, rows):
        o, hold = self.o, HOLD[self.mode]
        t_first = o.t_done
        _, ev = self.p.process(rows)
        self.events += o.events_of(t_first, ev)
        ripe = [e for e in self.events if e[0] + hold <= o.t_done and e[:2] not in self.released]
        out = []
        if ripe:
            own = f8o.owners(self.events, nfine=o.nfine if self.circular else None)
            new = []
            for e, k in zip(self.events, own):
                if e in ripe:
                    self.released.add(e[:2])
                    if k:
                        new.append(e)
            new.sort(key=lambda e: (e[0], e[1]))
            if new:
                soft = [o.llr(e[1], e[0]) for e in new]
                st, bits = self.decode(soft)
                for k, e in enumerate(new):
                    rec = dict(t0=e[0], F=e[1], score=e[2], hits=e[3], llr=soft[k], status=int(st[k, 0]), ok=int(st[k, 0]) == 2, bits77=bits[k, :77].copy())
                    rec["pass"] = 1
                    out.append(rec)
                    if rec["ok"]:
                        power, _ = ro.report(o.ring, o.t_done, o.nsub, self.circular, self.mode, [e[1]], [e[0]], [bits[k]])
                        self.wait.append((rec, bits[k].copy()) + refine(power[0, :9]))
                        self.ok.append(rec)
            first = min(e[0] for e in ripe)
            self.events = [e for e in self.events if e[0] >= first - 16]
        if self.passes == 2:
            out += self.second()
        return out

    def fdist(self, a, b):
        d = abs(a - b)
        return min(d, self.o.nfine - d) if self.circular else d

    def second(self):
        o, R, hold = self.o, self.R, HOLD[self.mode]
        due = sorted((a for a in self.wait if a[0]["t0"] + hold + R <= o.t_done), key=lambda a: (a[0]["t0"], a[0]["F"]))
        self.wait = [a for a in self.wait if a[0]["t0"] + hold + R > o.t_done]
        out, W = [], 2 * TONES[self.mode] + 2
        for t0 in sorted({a[0]["t0"] for a in due}):
            grp = [a for a in due if a[0]["t0"] == t0]
            Fs = [a[0]["F"] for a in grp]
            trials = [trial_grid(self.mode, a[2], a[3], o.qs, self.fs_out) for a in grp]
            self.p.subtract(Fs, [t0] * len(grp), [a[1] for a in grp], np.array(trials, np.int64))
            found = {}
            for F in Fs:
                for e in self.p.rescan(max(0, F - W), min(o.nfine - 1, F + W), max(0, t0 - R), t0 + R):
                    found[(e[0], e[1])] = e
            ev = sorted(found.values())
            own = f8o.owners(ev, nfine=o.nfine if self.circular else None)
            known = [r for r in self.ok if r["t0"] <= t0 + R]
            cand = [e for e, k in zip(ev, own) if k and not any(abs(e[0] - r["t0"]) <= 4 and self.fdist(e[1], r["F"]) <= 2 for r in known)]
            if cand:
                soft = [self.p.llr(e[1], e[0]) for e in cand]
                st, bits = self.decode(soft)
                for k, e in enumerate(cand):
                    if int(st[k, 0]) != 2 or any(abs(r["t0"] - e[0]) <= 8 and np.array_equal(r["bits77"], bits[k, :77]) for r in known):
                        continue
                    rec = dict(t0=e[0], F=e[1], score=e[2], hits=e[3], llr=soft[k], status=2, ok=True, bits77=bits[k, :77].copy())
                    rec["pass"] = 2
                    known.append(rec)
                    self.ok.append(rec)
                    out.append(rec)
            self.ok = [r for r in self.ok if r["t0"] >= t0 - R - 8]          # older ones meet no later group
        return out
