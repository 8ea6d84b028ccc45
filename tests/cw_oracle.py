"""NumPy models of the CW skimmer's decoder.  Test infrastructure only.

* ``params``: the settings, derived from the definition (independently of ``pysdr_amd.cw.params``).
* ``Oracle``: float32, vectorised over channels with a Python loop over samples; ``process(rows)`` returns the counts and
  the packed event words of the call, and the state is held as the library holds it (``state()``: the same fields).
* ``Scalar``: a plain per-channel transcription of steps 1 to 8, one sample at a time, NumPy float32 scalars.
* ``keyed_carrier`` / ``text_of``: the inputs and the read-out the CPU and the GPU tests share.
"""
import numpy as np

F = np.float32
WORD_SPACE = 256
RUN_MAX = 1 << 24
FLT_MAX = np.finfo(np.float32).max
INTS = ("key", "run", "dot", "last", "code", "nel", "sp", "seen")
FLOATS = ("s", "pk", "nf")
MESSAGE = "VVV CQ CQ DE K1ABC K1ABC TEST 599 73"
TAIL = "CQ CQ DE K1ABC K1ABC TEST 599 73 "


def settle_samples(ntaps, D, R):
    return -(-int(ntaps) // int(D)) + int(np.ceil(0.02 * float(R)))


def params(R, wpm0=20, settle=1):
    R = float(R)
    p = dict(a_s=F(min(1.0, 1.0 / (0.005 * R))), a_p=F(min(1.0, 1.0 / (1.5 * R))), a_n=F(min(1.0, 1.0 / (0.25 * R))),
             snr_min=F(16), hi=F(2), lo=F(0.5), fl=F(1.0 / 64),
             d0=int(round(16 * R * 1.2 / wpm0)), dmin=max(16, int(round(16 * R * 1.2 / 60))), dmax=int(round(16 * R * 1.2 / 5)),
             n0=int(settle))
    assert 1 <= p["n0"] <= 1 << 22
    assert p["dmin"] <= p["d0"] <= p["dmax"] <= 1 << 22
    return p


def cap_of(max_out):
    return 2 * (max_out // 3 + 1)


def pack(i, c):
    return (int(i) << 9) | int(c)


def unpack(w):
    w = int(w) & 0xFFFFFFFF
    return w >> 9, w & 511


class Scalar:
    """One channel, steps 1 to 8 as written."""

    def __init__(self, p):
        self.p = p
        self.s = self.pk = self.nf = F(0)
        self.key = self.run = self.last = self.nel = self.sp = self.seen = 0
        self.dot, self.code = p["d0"], 1
        self.m = 0

    def state(self):
        return {k: getattr(self, k) for k in FLOATS + INTS}

    def step(self, y):
        """-> None or the event's code"""
        c = self.p
        re, im = F(y.real), F(y.imag)
        with np.errstate(all="ignore"):
            # 1
            p = F(F(re * re) + F(im * im))
            if not p <= FLT_MAX:
                p = self.s
            # 2
            self.s = F(self.s + F(c["a_s"] * F(p - self.s)))
            # 3: the first n0 samples settle (n0 = 1: the floor is seeded by the first sample)
            settling = self.seen < c["n0"]
            if settling:
                self.seen += 1
            # 4
            if self.s > self.pk:
                self.pk = self.s
            else:
                self.pk = F(self.pk + F(c["a_p"] * F(self.s - self.pk)))
            if settling:
                self.nf = self.pk
            # 5
            A = F(self.nf * self.pk)
            B = F(F(self.pk * self.pk) * c["fl"])
            q = A if A > B else B
            u = F(self.s * self.s)
            pres = self.pk > F(c["snr_min"] * self.nf)
            new = int(bool(not settling and pres and (u >= F(q * c["lo"]) if self.key else u > F(q * c["hi"]))))
            # 6
            if new == 0 and not settling:
                cl = min(self.s, F(F(F(4) * self.nf) + F(1e-30)))
                self.nf = F(self.nf + F(c["a_n"] * F(cl - self.nf)))
        # 7
        if new != self.key:
            if self.key == 1:
                L = self.run
                if self.last > 0 and (L >= 2 * self.last or self.last >= 2 * L):
                    self.dot += (4 * (self.last + L) - self.dot) // 2
                    self.dot = min(max(self.dot, c["dmin"]), c["dmax"])
                self.last = L
                dash = int(16 * L >= 2 * self.dot)
                if self.code != 0:
                    if self.nel >= 7:
                        self.code = 0
                    else:
                        self.code = 2 * self.code + dash
                        self.nel += 1
            self.key, self.run = new, 1
        else:
            self.run = min(self.run + 1, RUN_MAX)
        # 8
        ev = None
        if self.key == 0:
            if self.code != 1 and 16 * self.run >= 2 * self.dot:
                ev = self.code
                self.code, self.nel, self.sp = 1, 0, 1
            elif self.sp and 16 * self.run >= 5 * self.dot:
                ev = WORD_SPACE
                self.sp = 0
        self.m += 1
        return ev

    def process(self, row):
        """-> [(index within the call, code)]"""
        out = []
        for i, y in enumerate(np.asarray(row, np.complex64)):
            e = self.step(y)
            if e is not None:
                out.append((i, e))
        return out


class Oracle:
    """nk channels at once; state arrays as the library's ``pysdr_cw_state`` delivers them."""

    def __init__(self, nk, p):
        self.nk, self.p = int(nk), p
        self.reset()

    def reset(self):
        nk = self.nk
        self.s, self.pk, self.nf = (np.zeros(nk, F) for _ in range(3))
        for k in INTS:
            setattr(self, k, np.zeros(nk, np.int32))
        self.dot[:] = self.p["d0"]
        self.code[:] = 1

    def state(self):
        return {k: getattr(self, k).copy() for k in FLOATS + INTS}

    def set_state(self, st):
        for k in FLOATS:
            setattr(self, k, np.array(st[k], F))
        for k in INTS:
            setattr(self, k, np.array(st[k], np.int32))

    def process(self, rows):
        """complex64 [nk][n] -> (counts int32 [nk], events: list of nk lists of packed words)"""
        rows = np.asarray(rows, np.complex64)
        assert rows.shape[0] == self.nk
        c = self.p
        re_all, im_all = np.ascontiguousarray(rows.real.T), np.ascontiguousarray(rows.imag.T)     # [n][nk]
        events = [[] for _ in range(self.nk)]
        s, pk, nf = self.s, self.pk, self.nf
        key, run, dot, last, code, nel, sp, seen = (getattr(self, k).astype(np.int64) for k in INTS)
        four, tiny = F(4), F(1e-30)
        with np.errstate(all="ignore"):
            for i in range(rows.shape[1]):
                re, im = re_all[i], im_all[i]
                p = re * re + im * im                                   # float32 arrays: every operation rounds on its own
                p = np.where(p <= FLT_MAX, p, s)
                s = s + c["a_s"] * (p - s)
                settling = seen < c["n0"]
                seen = np.where(settling, seen + 1, seen)
                pk = np.where(s > pk, s, pk + c["a_p"] * (s - pk))
                nf = np.where(settling, pk, nf)
                A, B = nf * pk, (pk * pk) * c["fl"]
                q = np.where(A > B, A, B)
                u = s * s
                pres = pk > c["snr_min"] * nf
                new = (~settling & pres & np.where(key == 1, u >= q * c["lo"], u > q * c["hi"])).astype(np.int64)
                cl = np.minimum(s, four * nf + tiny)
                nf = np.where((new == 0) & ~settling, nf + c["a_n"] * (cl - nf), nf)
                chg = new != key
                end = chg & (key == 1)
                if end.any():
                    L = run
                    adj = end & (last > 0) & ((L >= 2 * last) | (last >= 2 * L))
                    nd = np.clip(dot + (4 * (last + L) - dot) // 2, c["dmin"], c["dmax"])
                    dot = np.where(adj, nd, dot)
                    last = np.where(end, L, last)
                    dash = (16 * L >= 2 * dot).astype(np.int64)
                    live = end & (code != 0)
                    over = live & (nel >= 7)
                    app = live & (nel < 7)
                    code = np.where(over, 0, np.where(app, 2 * code + dash, code))
                    nel = np.where(app, nel + 1, nel)
                run = np.where(chg, 1, np.minimum(run + 1, RUN_MAX))
                key = new
                up = key == 0
                ch = up & (code != 1) & (16 * run >= 2 * dot)
                ws = up & ~ch & (sp == 1) & (16 * run >= 5 * dot)
                if ch.any():
                    for a in np.flatnonzero(ch):
                        events[a].append(pack(i, code[a]))
                    code = np.where(ch, 1, code)
                    nel = np.where(ch, 0, nel)
                    sp = np.where(ch, 1, sp)
                if ws.any():
                    for a in np.flatnonzero(ws):
                        events[a].append(pack(i, WORD_SPACE))
                    sp = np.where(ws, 0, sp)
        assert s.dtype == F and pk.dtype == F and nf.dtype == F
        self.s, self.pk, self.nf = s, pk, nf
        for k, v in zip(INTS, (key, run, dot, last, code, nel, sp, seen)):
            setattr(self, k, v.astype(np.int32))
        counts = np.array([len(e) for e in events], np.int32)
        return counts, events


def text_of(words, table):
    """packed words -> text through ``table(code)`` (``pysdr_amd.cw.code_text``)"""
    return "".join(table(unpack(w)[1]) for w in words)


def shift_events(events, base):
    """the words of a call with their index moved by base outputs: as tuples (absolute index, code)"""
    return [[(base + unpack(w)[0], unpack(w)[1]) for w in ev] for ev in events]


def shaped_keying(key01, fs, edge=0.008):
    """0 / 1 keying -> amplitude with raised-cosine edges of ``edge`` seconds (a Hann window of that length, unit sum)"""
    n = max(int(round(edge * fs)), 1)
    w = np.hanning(n + 2)[1:-1]
    return np.convolve(np.asarray(key01, np.float64), w / w.sum())


def keyed_carrier(text, wpm, fs, f_hz, amp, lead, tail, keying, phase=0.0):
    """complex128: ``lead`` seconds of nothing, the keyed carrier of ``text`` at f_hz, ``tail`` seconds of nothing"""
    k = shaped_keying(keying(text, wpm, fs), fs)
    a = np.concatenate((np.zeros(int(lead * fs)), k, np.zeros(int(tail * fs))))
    n = np.arange(len(a))
    return amp * a * np.exp(1j * (2 * np.pi * f_hz / fs * n + phase))
