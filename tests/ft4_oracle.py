"""NumPy models of the FT4 skimmer.  Test infrastructure only; the interface is tests/ft8_oracle.py's.

* ``params`` / ``tables``: the settings and the table, derived from the definition (independently of ``pysdr_amd.ft4``).
* ``Oracle``: float32, vectorised over rows, steps and decoders; ``process(rows)`` returns the counts and the event words
  of the call, and the state is held as the library holds it (``state()``: sc, hits, ring, t_done); ``llr`` the soft bits.
* ``plain64``: a plain float64 transcription of steps 1 to 3 over a whole stream, and ``plain_llr`` of the soft bits.
* ``Skimmer``: rows -> calls of max_out outputs -> held events -> finder -> records, as ``FT4_Skimmer.push`` does it, on
  the oracle.
* ``tones`` / ``waveform``: an FT4 frame, GFSK or rectangular, with or without its ramps, continuous phase.
What is not FT4's own -- the peak rule, the event words, the finder as a double loop, the ring read by absolute step --
is imported from tests/ft8_oracle.py.
"""
import math

import numpy as np

from tests.ft8_oracle import _Unrolled, is_peak, owners, pack, steps_done, tables                # noqa: F401  (item 22's, unchanged)
from tests.psk_oracle import noise_sigma, rows_of                            # noqa: F401  (shared with the other rasters)

F32 = np.float32
BAUD = 125.0 / 6.0
COSTAS = ((0, 1, 3, 2), (1, 0, 2, 3), (2, 3, 1, 0), (3, 2, 0, 1))
GRAY4 = (0, 1, 3, 2)
SYNC_SYMS = [b + k for b in (0, 33, 66, 99) for k in range(4)]              # the 16 Costas symbols in order
SYNC_TONES = [c for blk in COSTAS for c in blk]                              # and the tone each expects
DATA_SYMS = list(range(4, 33)) + list(range(37, 66)) + list(range(70, 99))  # the 87 data symbols in order
LAG, REACH, KEEP, EMIT, HOLD = 408, 4, 9, 412, 417
SNR_BW = 2500.0                                                              # the bandwidth FT4 reports its SNR in


def params(smin=4.0, hmin=12, pmax=1e18):
    return dict(smin=F32(smin), hmin=int(hmin), pmax=F32(pmax))


def steps_per_call(max_out, S):
    return max_out // (S // 4) + 1


def cap_of(max_out, S):
    return steps_per_call(max_out, S) // 5 + 1


def ring_steps(max_out, S):
    return HOLD + 2 * steps_per_call(max_out, S)


def sync_scores(P, t0s, nsub, dtype):
    """step 2 for the frame starts ``t0s`` on P[nk][t][NB] (absolute steps): -> score [nk][len(t0s)][nsub], hits likewise.
    Every operation is elementwise in ``dtype``, in the definition's order."""
    t0s = np.asarray(t0s, np.int64)
    j = np.arange(nsub)
    shape = (P.shape[0], len(t0s), nsub)
    sig, tot, hits = np.zeros(shape, dtype), np.zeros(shape, dtype), np.zeros(shape, np.int32)
    for sym, c in zip(SYNC_SYMS, SYNC_TONES):
        p = [P[:, t0s + 4 * sym, :][:, :, j + 2 * tone] for tone in range(4)]
        e = p[c]
        sig = sig + e
        r = p[0]
        for tone in range(1, 4):
            r = r + p[tone]
        tot = tot + r
        hit = np.ones(shape, bool)
        for tone in range(4):
            if tone != c:
                hit &= e > p[tone]
        hits += hit
    den = tot - sig
    with np.errstate(all="ignore"):
        score = np.where(den > 0, (dtype(3) * sig) / np.where(den > 0, den, dtype(1)), dtype(0)).astype(dtype)
    return score, hits


class Oracle:
    """nk rows x S / 2 decoders at once; fine row F = a NSUB + j; state arrays as ``pysdr_ft4_state`` delivers them."""

    def __init__(self, nk, S, p, max_out=256):
        self.nk, self.S, self.p, self.max_out = int(nk), int(S), p, int(max_out)
        self.nsub, self.nb, self.NT, self.qs = S // 2, S // 2 + 6, 4 * S, S // 4
        self.nfine = self.nk * self.nsub
        self.tr, self.cap = ring_steps(max_out, S), cap_of(max_out, S)
        tw = tables(S)
        q = 2 * np.arange(self.nb, dtype=np.int64) - (self.nb - 1)
        ix = (q[:, None] * np.arange(S, dtype=np.int64)[None, :]) % self.NT   # [NB][S], a mathematical mod
        self.twr, self.twi = tw[ix, 0], tw[ix, 1]
        self.reset()

    def reset(self):
        self.hist = np.zeros((self.nk, self.S - 1), np.complex64)
        self.m = self.t_done = 0
        self.ring = np.zeros((self.nk, self.tr, self.nb), F32)
        self.sc = np.zeros((KEEP, self.nfine), F32)
        self.hits = np.zeros((KEEP, self.nfine), np.int32)

    def state(self):
        return dict(sc=self.sc.copy(), hits=self.hits.copy(), ring=self.ring.copy(), t_done=self.t_done)

    def spectrum(self, ext, starts):
        """step 1 for the windows that begin at ext[:, starts[k]] -> P float32 [nk][len(starts)][NB]"""
        S = self.S
        W = ext[:, np.asarray(starts, np.int64)[:, None] + np.arange(S)[None, :]]            # [nk][ns][S]
        yr = np.ascontiguousarray(W.real)[:, :, None, :]
        yi = np.ascontiguousarray(W.imag)[:, :, None, :]
        with np.errstate(all="ignore"):
            vr = yr * self.twr - yi * self.twi                       # float32 arrays: every operation rounds on its own
            vi = yr * self.twi + yi * self.twr
            ur, ui = vr[..., 0], vi[..., 0]
            for i in range(1, S):
                ur, ui = ur + vr[..., i], ui + vi[..., i]
            P = ur * ur + ui * ui
        P[~(P <= self.p["pmax"])] = 0
        assert P.dtype == F32
        return P

    def process(self, rows):
        """complex64 [nk][n] -> (counts int32 [nfine], events: list of nfine lists of (word0, word1))"""
        rows = np.asarray(rows, np.complex64)
        assert rows.shape[0] == self.nk
        n, S = rows.shape[1], self.S
        events = [[] for _ in range(self.nfine)]
        if n == 0:
            return np.zeros(self.nfine, np.int32), events
        t_first, t1 = self.t_done, steps_done(self.m + n, S)
        ns = t1 - t_first
        assert ns <= steps_per_call(self.max_out, S)
        ext = np.concatenate((self.hist, rows), axis=1)              # outputs m - (S - 1) .. m + n - 1
        if ns:
            t = np.arange(t_first, t1)
            P = self.spectrum(ext, self.qs * t - self.m + (S - 1))
            self.ring[:, t % self.tr, :] = P
            t0s = t[t >= LAG] - LAG
            if len(t0s):
                full = _Unrolled(self.ring, self.tr)
                score, hits = sync_scores(full, t0s, self.nsub, F32)
                for k, t0 in enumerate(int(v) for v in t0s):
                    self.sc[t0 % KEEP] = score[:, k, :].reshape(-1)
                    self.hits[t0 % KEEP] = hits[:, k, :].reshape(-1)
                    tc = t0 - REACH
                    if tc < 0:
                        continue
                    v = self.sc[tc % KEEP]
                    cand = np.flatnonzero((v >= self.p["smin"]) & (self.hits[tc % KEEP] >= self.p["hmin"]))
                    for F in cand:
                        if is_peak(lambda s: self.sc[s % KEEP, F], lambda s: self.hits[s % KEEP, F], tc, self.p) and len(events[F]) < self.cap:
                            events[F].append(pack(t0 + LAG - t_first, self.hits[tc % KEEP, F], self.sc[tc % KEEP, F]))
        self.hist = ext[:, -(S - 1):].copy()
        self.m += n
        self.t_done = t1
        return np.array([len(v) for v in events], np.int32), events

    def events_of(self, t_first, events):
        """(t0, F, score, hits) of a call's event words"""
        out = []
        for F, ev in enumerate(events):
            for w0, w1 in ev:
                w = int(w0) & 0xFFFFFFFF
                out.append((t_first + (w >> 5) - EMIT, F, float(np.array([w1], np.int32).view(F32)[0]), w & 31))
        return out

    def llr_ok(self, F, t0):
        return 0 <= F < self.nfine and t0 >= 0 and t0 + LAG < self.t_done and self.t_done - t0 <= self.tr

    def llr(self, F, t0):
        """float32 [174] of the candidate, from the ring"""
        assert self.llr_ok(F, t0)
        a, j = divmod(int(F), self.nsub)
        out = np.zeros(174, F32)
        for d, sym in enumerate(DATA_SYMS):
            row = self.ring[a, (t0 + 4 * sym) % self.tr]
            p = [row[j + 2 * GRAY4[v]] for v in range(4)]
            for k, mask in enumerate((2, 1)):
                out[2 * d + k] = F32(max(p[v] for v in range(4) if v & mask) - max(p[v] for v in range(4) if not v & mask))
        return out


def plain64(rows, S, p):
    """Steps 1 to 3 over a whole stream in float64, written down plainly: rows complex [nk][n] -> (events: list of
    (t0, F, score, hits), P float64 [nk][steps][NB]).  The spectrum is a matrix product with exp(-2 pi i q_b i / NT)."""
    rows = np.asarray(rows, np.complex128)
    nk, n = rows.shape
    nsub, nb, NT, qs = S // 2, S // 2 + 6, 4 * S, S // 4
    T = steps_done(n, S)
    q = 2 * np.arange(nb) - (nb - 1)
    E = np.exp(-2j * np.pi * np.outer(np.arange(S), q) / NT)                                 # [S][NB]
    W = rows[:, (qs * np.arange(T))[:, None] + np.arange(S)[None, :]]                        # [nk][T][S]
    with np.errstate(all="ignore"):
        P = np.abs(W @ E) ** 2
    P[~(P <= float(p["pmax"]))] = 0
    nt0 = T - LAG
    if nt0 <= 0:
        return [], P
    score, hits = sync_scores(P, np.arange(nt0), nsub, np.float64)
    score, hits = score.transpose(1, 0, 2).reshape(nt0, -1), hits.transpose(1, 0, 2).reshape(nt0, -1)
    p64 = dict(smin=float(p["smin"]), hmin=p["hmin"])
    out = []
    for tc in range(nt0 - REACH):
        for F in np.flatnonzero((score[tc] >= p64["smin"]) & (hits[tc] >= p64["hmin"])):
            if is_peak(lambda s: score[s, F], lambda s: hits[s, F], tc, p64):
                out.append((tc, int(F), float(score[tc, F]), int(hits[tc, F])))
    return out, P


def plain_llr(P, S, F, t0):
    a, j = divmod(int(F), S // 2)
    out = np.zeros(174)
    for d, sym in enumerate(DATA_SYMS):
        p = [P[a, t0 + 4 * sym, j + 2 * GRAY4[v]] for v in range(4)]
        for k, mask in enumerate((2, 1)):
            out[2 * d + k] = max(p[v] for v in range(4) if v & mask) - max(p[v] for v in range(4) if not v & mask)
    return out


class Skimmer:
    """rows [nk][n] of the whole stream -> calls of max_out outputs -> events held until step t0 + 416 is complete -> the
    finder -> records (t0, F, score, hits, llr) of the owners, as ``FT4_Skimmer.push`` does it"""

    def __init__(self, nk, S, circular, max_out=256, p=None):
        self.o = Oracle(nk, S, params() if p is None else p, max_out)
        self.circular, self.max_out = circular, max_out
        self.all_events, self.records = [], []
        self.released = set()

    def push(self, rows):
        out = []
        for i0 in range(0, rows.shape[1], self.max_out):
            t_first = self.o.t_done
            counts, ev = self.o.process(rows[:, i0:i0 + self.max_out])
            self.all_events += self.o.events_of(t_first, ev)
            ripe = [e for e in self.all_events if e[0] + HOLD <= self.o.t_done and e[:2] not in self.released]
            if not ripe:
                continue
            own = owners(self.all_events, nfine=self.o.nfine if self.circular else None)
            for e, o in zip(self.all_events, own):
                if e in ripe:
                    self.released.add(e[:2])
                    if o:
                        out.append(dict(t0=e[0], F=e[1], score=e[2], hits=e[3], llr=self.o.llr(e[1], e[0])))
        out.sort(key=lambda r: (r["t0"], r["F"]))
        self.records += out
        return out


def fine_freqs(fs, M, S, channels):
    """Hz of tone 0 of every fine row: row centre + (2 j - (NB - 1)) baud / 4"""
    k = rows_of(M, channels)
    f = np.where(k >= (M + 1) // 2, k - M, k) * (fs / M)
    q = 2 * np.arange(S // 2) - (S // 2 + 5)
    return (f[:, None] + q[None, :] * (BAUD / 4)).reshape(-1)


def tones(bits):
    bits = [int(b) for b in bits]
    assert len(bits) == 174
    data = [GRAY4[2 * bits[2 * d] + bits[2 * d + 1]] for d in range(87)]
    return list(COSTAS[0]) + data[:29] + list(COSTAS[1]) + data[29:58] + list(COSTAS[2]) + data[58:] + list(COSTAS[3])


def waveform(tn, f0, fs, gfsk=True, ramps=True, phase=0.0):
    """the frame, sample by sample: instantaneous frequency f0 + baud sum_n tone_n pulse(t - n - 1/2), t in symbols at
    the sample's middle; pulse = (erf(k (t + 1/2)) - erf(k (t - 1/2))) / 2 with k = pi sqrt(2 / ln 2), or a rectangle; the
    first and the last tone are held beyond the frame.  With ramps the sequence gains a symbol at either end (the first
    and the last tone again) whose amplitude is (1 - cos(pi t)) / 2 and (1 + cos(pi t)) / 2, t in [0, 1) within the symbol:
    the array begins with the ramp, the frame one symbol later."""
    tn = list(tn)
    if ramps:
        tn = [tn[0]] + tn + [tn[-1]]
    sps = fs / BAUD
    n = int(round(len(tn) * sps))
    k = math.pi * math.sqrt(2 / math.log(2))
    erf = np.vectorize(math.erf)
    t = (np.arange(n) + 0.5) / sps
    ext = [tn[0]] * 3 + tn + [tn[-1]] * 3
    dev = np.zeros(n)
    if gfsk:
        for i, tone in enumerate(ext):                               # symbol i - 3
            tau = t - (i - 3) - 0.5
            near = np.abs(tau) < 3.5
            dev[near] += tone * 0.5 * (erf(k * (tau[near] + 0.5)) - erf(k * (tau[near] - 0.5)))
    else:
        dev = np.array(tn, np.float64)[np.minimum(np.floor(t).astype(int), len(tn) - 1)]
    ph = np.cumsum(f0 + BAUD * dev)
    w = np.exp(1j * (2 * np.pi / fs * ph + phase))
    if ramps:
        amp = np.ones(n)
        amp[t < 1] = 0.5 * (1 - np.cos(np.pi * t[t < 1]))
        last = t >= len(tn) - 1
        amp[last] = 0.5 * (1 + np.cos(np.pi * (t[last] - (len(tn) - 1))))
        w = w * amp
    return w
