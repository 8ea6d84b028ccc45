"""NumPy models of the RTTY raster skimmer's decoder.  Test infrastructure only.

* ``params`` / ``tables``: the settings and the two tables, derived from the definition (independently of ``pysdr_amd.fsk``).
* ``Oracle``: float32, vectorised over the fine rows; the tone powers of a call are array operations over all its outputs
  (they carry no state but the row's last S - 1 samples), the recurrences a Python loop over the outputs.
  ``process(rows)`` returns the counts and the packed event words of the call, and the state is held as the library
  holds it (``state()``: the same fields).
* ``Scalar``: a plain transcription of steps 1 to 3 for one decoder, one output at a time, NumPy float32 scalars.
* ``owners``: the finder as written (the loop of ``tests/psk_oracle.py`` with this raster's reach).  ``Skimmer``: rows ->
  calls of max_out outputs -> finder -> text, as ``RTTY_Raster_Skimmer.push`` does it, on the oracle.
* ``baudot_codes`` / ``rtty_baseband``: an RTTY signal: continuous-phase FSK, a given stop length.
* ``rows_of`` / ``fine_freqs`` / ``noise_sigma``: what the CPU and the GPU tests share about their inputs.
"""
import numpy as np

from tests.psk_oracle import KEEP, noise_sigma, rows_of                       # noqa: F401  (shared with the PSK raster)
from tests.psk_oracle import owners as _owners

F32 = np.float32
BAUD = 500.0 / 11                                                # the reference's T = 22 ms
FLOATS = ("qn", "qd", "bm", "bs")
INTS = ("st", "cnt", "sh", "nb", "prev", "fig", "open", "seen")
MESSAGE = "CQ CQ DE K1ABC K1ABC PSE K"
REACH = 16
SILENT = (0, 27, 31)                                             # code & 31 that text omits: null, FIGS, LTRS


def params(a_q=1.0 / 64, a_b=1.0 / 32, hi=0.8, lo=0.65, bal=0.25, pmax=1e18, n0=64):
    return dict(a_q=F32(a_q), a_b=F32(a_b), hi=F32(hi), lo=F32(lo), bal=F32(bal), pmax=F32(pmax), n0=int(n0))


def tables(S):
    NT = 8 * S
    t = np.arange(NT, dtype=np.float64)
    tw = np.stack((np.cos(2 * np.pi * t / NT), -np.sin(2 * np.pi * t / NT)), axis=1).astype(F32)
    g = np.kaiser(S, 8.6)
    return tw, (g / np.sum(g)).astype(F32)


def event_gap(S):
    return 6 * S + S // 2 + 1


def cap_of(max_out, S):
    return max_out // event_gap(S) + 1


def pack(i, code):
    return (int(i) << 6) | int(code)


def unpack(w):
    w = int(w) & 0xFFFFFFFF
    return w >> 6, w & 63


def code_text(code):
    """the character of a code, independent of the package's table lookup: ITA2, US figures as the reference has them"""
    from pysdr_amd.rtty import FIGS, LTRS
    return (FIGS if code >= 32 else LTRS)[code & 31]


class Scalar:
    """Decoder j of one row, steps 1 to 3 as written."""

    def __init__(self, S, j, p):
        self.S, self.p, self.NT = S, p, 8 * S
        self.q_s, self.q_m = 2 * j - S - 14, 2 * j - S + 16
        self.tw, self.g = tables(S)
        self.y = {}                                              # absolute index -> complex64
        self.qn = self.qd = self.bm = self.bs = F32(0)
        self.st = self.sh = self.nb = self.fig = self.open = self.seen = 0
        self.cnt, self.prev = S, 1
        self.m = 0

    def power(self, q):
        m, c = self.m, self.p
        ur = ui = None
        for i in range(self.S):
            k = m - i
            yk = self.y.get(k, np.complex64(0))
            yr, yi = F32(yk.real), F32(yk.imag)
            tr, ti = self.tw[(q * k) % self.NT]
            vr = F32(F32(yr * tr) - F32(yi * ti))
            vi = F32(F32(yr * ti) + F32(yi * tr))
            if i == 0:
                ur, ui = F32(self.g[0] * vr), F32(self.g[0] * vi)
            else:
                ur, ui = F32(ur + F32(self.g[i] * vr)), F32(ui + F32(self.g[i] * vi))
        P = F32(F32(ur * ur) + F32(ui * ui))
        return P if P <= c["pmax"] else F32(0)

    def step(self, y):
        """-> None or the event's code"""
        c, S = self.p, self.S
        self.y[self.m] = np.complex64(y)
        ev = None
        with np.errstate(all="ignore"):
            # 1
            PS, PM = self.power(self.q_s), self.power(self.q_m)
            d = int(bool(PM > PS))
            # 2
            self.cnt -= 1
            if self.st == 0 and self.prev == 1 and d == 0:
                self.st, self.cnt = 1, S // 2
            elif self.cnt == 0:
                # 3 (a)
                inch, framed = self.st != 0, False
                if self.st == 0:
                    pass
                elif self.st == 1:
                    if d == 0:
                        self.st, self.nb, self.sh = 2, 0, 0
                    else:
                        self.st, inch = 0, False
                elif self.st == 2:
                    self.sh |= d << self.nb
                    self.nb += 1
                    if self.nb == 5:
                        self.st = 3
                else:
                    framed, self.st = d == 1, 0
                self.cnt = S
                # (b)
                w, l = max(PM, PS), min(PM, PS)
                self.qn = F32(self.qn + F32(c["a_q"] * F32(F32(w - l) - self.qn)))
                self.qd = F32(self.qd + F32(c["a_q"] * F32(F32(w + l) - self.qd)))
                # (c)
                if inch and d:
                    self.bm = F32(self.bm + F32(c["a_b"] * F32(PM - self.bm)))
                if inch and not d:
                    self.bs = F32(self.bs + F32(c["a_b"] * F32(PS - self.bs)))
                # (d)
                if self.seen < c["n0"]:
                    self.seen += 1
                    self.open = 0
                else:
                    thr = F32((c["lo"] if self.open else c["hi"]) * self.qd)
                    self.open = int(bool(self.qd > 0 and self.qn >= thr
                                         and min(self.bm, self.bs) >= F32(c["bal"] * max(self.bm, self.bs))))
                # (e)
                if framed:
                    if self.open:
                        ev = self.sh + 32 * self.fig
                    if self.sh == 27:
                        self.fig = 1
                    if self.sh == 31:
                        self.fig = 0
            self.prev = d
        self.y.pop(self.m - self.S, None)
        self.m += 1
        return ev

    def state(self):
        return {k: getattr(self, k) for k in FLOATS + INTS}


class Oracle:
    """nk rows x S decoders at once; fine row F = a S + j; state arrays as ``pysdr_fsk_state`` delivers them."""

    def __init__(self, nk, S, p):
        self.nk, self.S, self.p = int(nk), int(S), p
        self.nsub, self.NT, self.ntone = self.S, 8 * self.S, self.S + 15
        self.nfine = self.nk * self.nsub
        self.tw, self.g = tables(self.S)
        self.q = 2 * np.arange(self.ntone, dtype=np.int64) - self.S - 14
        self.reset()

    def reset(self):
        nf = self.nfine
        self.hist = np.zeros((self.nk, self.S - 1), np.complex64)
        self.m = 0
        for k in FLOATS:
            setattr(self, k, np.zeros(nf, F32))
        for k in INTS:
            setattr(self, k, np.zeros(nf, np.int32))
        self.cnt[:] = self.S
        self.prev[:] = 1

    def state(self):
        return {k: getattr(self, k).copy() for k in FLOATS + INTS}

    def set_state(self, st, hist, m):
        """continue from a state, the rows' last S - 1 samples and the absolute index of the next output"""
        for k in FLOATS:
            setattr(self, k, np.array(st[k], F32))
        for k in INTS:
            setattr(self, k, np.array(st[k], np.int32))
        self.hist = np.array(hist, np.complex64)
        self.m = int(m)

    def powers(self, rows):
        """step 1 for every output of the call -> PS, PM float32 [nfine][n]"""
        S, n = self.S, rows.shape[1]
        ext = np.concatenate((self.hist, rows), axis=1)                          # outputs m - (S - 1) .. m + n - 1
        k = self.m - (S - 1) + np.arange(S - 1 + n, dtype=np.int64)
        t = (self.q[:, None] * k[None, :]) % self.NT                            # [ntone][S - 1 + n], a mathematical mod
        tr, ti = self.tw[t, 0][None, :, :], self.tw[t, 1][None, :, :]
        yr = np.ascontiguousarray(ext.real)[:, None, :]
        yi = np.ascontiguousarray(ext.imag)[:, None, :]
        vr = yr * tr - yi * ti                                                   # float32 arrays: every operation rounds on its own
        vi = yr * ti + yi * tr
        ur = ui = None
        for i in range(S):
            sl = slice(S - 1 - i, S - 1 - i + n)
            if i == 0:
                ur, ui = self.g[0] * vr[:, :, sl], self.g[0] * vi[:, :, sl]
            else:
                ur, ui = ur + self.g[i] * vr[:, :, sl], ui + self.g[i] * vi[:, :, sl]
        P = ur * ur + ui * ui
        P[~(P <= self.p["pmax"])] = 0
        assert P.dtype == F32
        nf = self.nfine
        return np.ascontiguousarray(P[:, :S, :]).reshape(nf, n), np.ascontiguousarray(P[:, 15:, :]).reshape(nf, n)

    def process(self, rows):
        """complex64 [nk][n] -> (counts int32 [nfine], events: list of nfine lists of packed words)"""
        rows = np.asarray(rows, np.complex64)
        assert rows.shape[0] == self.nk
        n, S, c = rows.shape[1], self.S, self.p
        events = [[] for _ in range(self.nfine)]
        if n == 0:
            return np.zeros(self.nfine, np.int32), events
        st, cnt, sh, nb, prev, fig = self.st, self.cnt, self.sh, self.nb, self.prev, self.fig
        with np.errstate(all="ignore"):
            PS, PM = self.powers(rows)
            D = (PM > PS).astype(np.int32)
            for i in range(n):
                d = D[:, i]
                cnt -= 1
                edge = (st == 0) & (prev == 1) & (d == 0)
                ix = np.flatnonzero(~edge & (cnt == 0))
                st[edge] = 1
                cnt[edge] = S // 2
                prev[:] = d
                if not len(ix):
                    continue
                s, dd, ps, pm = st[ix], d[ix], PS[ix, i], PM[ix, i]
                inch = (s != 0) & ~((s == 1) & (dd == 1))
                good = (s == 1) & (dd == 0)
                data = s == 2
                bits = np.where(data, sh[ix] | (dd << nb[ix]), np.where(good, 0, sh[ix]))
                nbs = np.where(data, nb[ix] + 1, np.where(good, 0, nb[ix]))
                framed = (s == 3) & (dd == 1)
                st[ix] = np.where(good, 2, np.where(data, np.where(nbs == 5, 3, 2), 0))
                sh[ix], nb[ix], cnt[ix] = bits, nbs, S
                w, l = np.maximum(pm, ps), np.minimum(pm, ps)
                qn = self.qn[ix] + c["a_q"] * ((w - l) - self.qn[ix])
                qd = self.qd[ix] + c["a_q"] * ((w + l) - self.qd[ix])
                self.qn[ix], self.qd[ix] = qn, qd
                bm, bs = self.bm[ix], self.bs[ix]
                bm = np.where(inch & (dd == 1), bm + c["a_b"] * (pm - bm), bm)
                bs = np.where(inch & (dd == 0), bs + c["a_b"] * (ps - bs), bs)
                self.bm[ix], self.bs[ix] = bm, bs
                settling = self.seen[ix] < c["n0"]
                self.seen[ix] += settling
                thr = np.where(self.open[ix] == 1, c["lo"], c["hi"]).astype(F32) * qd
                is_open = (~settling & (qd > 0) & (qn >= thr) & (np.minimum(bm, bs) >= c["bal"] * np.maximum(bm, bs))).astype(np.int32)
                self.open[ix] = is_open
                for a in np.flatnonzero(framed & (is_open == 1)):
                    events[ix[a]].append(pack(i, bits[a] + 32 * fig[ix[a]]))
                fig[ix] = np.where(framed & (bits == 27), 1, np.where(framed & (bits == 31), 0, fig[ix]))
                assert qn.dtype == F32 and bm.dtype == F32 and bs.dtype == F32 and thr.dtype == F32
        self.hist = np.concatenate((self.hist, rows), axis=1)[:, -(S - 1):].copy()
        self.m += n
        return np.array([len(v) for v in events], np.int32), events


def owners(qn, is_open, circular, prev=None, reach=REACH):
    """the finder as written: the loop of the PSK raster, 16 fine rows to either side"""
    return _owners(qn, is_open, circular, prev, reach)


class Skimmer:
    """rows [nk][n] of the whole stream -> calls of max_out outputs -> the finder on each call's end state -> text[F] of the
    owners, as ``RTTY_Raster_Skimmer.push`` does it"""

    def __init__(self, nk, S, circular, table=code_text, max_out=256, p=None, sticky=True, reach=REACH):
        self.o = Oracle(nk, S, params() if p is None else p)
        self.sticky, self.reach, self.owner = sticky, reach, np.zeros(nk * S, bool)
        self.circular, self.table, self.max_out = circular, table, max_out
        self.text = {}
        self.nevents = 0                                         # of all fine rows, owners or not
        self.nopen = 0                                           # decoders found open at the end of a call, summed over the calls

    def push(self, rows):
        out = []
        for i0 in range(0, rows.shape[1], self.max_out):
            m0 = self.o.m
            counts, ev = self.o.process(rows[:, i0:i0 + self.max_out])
            self.nevents += int(counts.sum())
            self.nopen += int(self.o.open.sum())
            own = self.owner = owners(self.o.qn, self.o.open, self.circular, self.owner if self.sticky else None, self.reach)
            for F in np.flatnonzero(own & (counts > 0)):
                out += [(m0 + unpack(w)[0], int(F), self.table(unpack(w)[1])) for w in ev[F]]
                for w in ev[F]:
                    if unpack(w)[1] & 31 not in SILENT:
                        self.text[F] = self.text.get(F, "") + self.table(unpack(w)[1])
        out.sort(key=lambda e: (e[0], e[1]))
        return out


def fine_freqs(fs, M, S, channels):
    """Hz of every fine row (the midpoint of its two tones): row centre + (2 j - S + 1) baud / 8"""
    k = rows_of(M, channels)
    f = np.where(k >= (M + 1) // 2, k - M, k) * (fs / M)
    q = 2 * np.arange(S) - S + 1
    return (f[:, None] + q[None, :] * (BAUD / 8)).reshape(-1)


def shift_events(events, base):
    """the words of a call with their index moved by base outputs: as tuples (absolute index, code)"""
    return [[(base + unpack(w)[0], unpack(w)[1]) for w in ev] for ev in events]


def baudot_codes(text):
    """ITA2 codes 0 .. 31 of ``text`` with the shifts it needs, starting in letters; characters outside both tables are
    skipped"""
    from pysdr_amd.rtty import FIGS, LTRS
    out, fig = [], 0
    for ch in text:
        if ch in LTRS and ch in FIGS and LTRS.index(ch) == FIGS.index(ch):   # space, CR, LF, null: the same code in both shifts
            out.append(LTRS.index(ch))
        elif ch in LTRS:
            if fig:
                out.append(31)
                fig = 0
            out.append(LTRS.index(ch))
        elif ch in FIGS:
            if not fig:
                out.append(27)
                fig = 1
            out.append(FIGS.index(ch))
    return out


def rtty_baseband(codes, fs, f, stop=1.5, preamble=2.0, tail=0.5, phase=0.0, baud=BAUD, shift=15 * BAUD / 4, dtype=None):
    """complex128 (or ``dtype``) test signal of power 1 at ``fs``: ``preamble`` seconds of steady mark, then every code as
    a start bit (space), five data bits LSB first (1 = mark) and ``stop`` bit lengths of mark, then ``tail`` seconds of mark;
    continuous-phase FSK around ``f`` Hz from the centre, mark the upper tone shift / 2 above it."""
    T = float(fs) / float(baud)                                  # samples per bit; need not be an integer
    lengths, levels = [preamble * baud], [1]
    for c in codes:
        lengths += [1.0] + [1.0] * 5 + [float(stop)]
        levels += [0] + [(int(c) >> b) & 1 for b in range(5)] + [1]
    lengths.append(tail * baud)
    levels.append(1)
    ends = np.ceil(np.cumsum(lengths) * T).astype(np.int64)      # piece k holds the samples n with ends[k - 1] <= n < ends[k]
    ph = np.repeat(float(f) + (np.asarray(levels) - 0.5) * float(shift), np.diff(ends, prepend=0))
    np.cumsum(ph, out=ph)                                        # cycles times fs, through sample n
    ph *= 2 * np.pi / float(fs)
    ph += phase
    out = np.empty(len(ph), np.complex128 if dtype is None else dtype)
    for i in range(0, len(ph), 1 << 22):                         # in pieces: a wideband test signal is long
        out[i:i + (1 << 22)] = np.exp(1j * ph[i:i + (1 << 22)])
    return out
