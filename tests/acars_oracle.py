"""NumPy twin of the ACARS skimmer's definition, float32 with every operation rounded on its own, and
of the skimmer's de-duplication.  Test infrastructure only: it shares no code with pysdr_amd/acars.py beyond the numbers
of the definition, which it derives again.

* ``Oracle``: steps 1 to 8 on the rows of a channelizer, any cut into calls; ``process`` / ``state`` / ``set_state``.
* ``Skimmer``: the oracle behind the host's rule that makes one record of a frame's copies on neighbour rows.
* ``cap_of``: the event cap, as DESIGN.md derives it.
* ``scene``: stations with noise, the input the CPU and the GPU tests share.
"""
import numpy as np
from scipy.signal import firwin

FRAME_BYTES, FRAME_WORDS = 240, 60
MAX_BYTES, MIN_BYTES = 238, 13
INTS = ("clk", "xprev", "lev", "sr", "st", "byte", "nb", "nbytes", "crc")
SEARCH, SOH, TEXT, BCS1, BCS2 = range(5)


def tables(fs_out):
    L = int(np.floor(fs_out / 2400.0 + 0.5))
    k = np.arange(1024)
    tw = np.stack((np.cos(2 * np.pi * k / 1024), -np.sin(2 * np.pi * k / 1024)), axis=1).astype(np.float32)
    i = np.arange(4 * L + 1)
    c = firwin(4 * L + 1, 1500.0, window=("kaiser", 5.0), fs=fs_out) * np.exp(2j * np.pi * 1800.0 * (i - 2 * L) / fs_out)
    c = c - c.mean()
    return L, tw, np.stack((c.real, c.imag), axis=1).astype(np.float32)


def params(fs_out, pll_shift=2, pmax=1e18):
    return dict(pmax=np.float32(pmax), pll_shift=int(pll_shift), w_car=int(round(1800.0 / fs_out * 2 ** 32)),
                w_baud=int(round(2400.0 / fs_out * 2 ** 32)))


def cap_of(max_out, w_baud):
    """61 words for a frame carried into the call, then a word per 24 samplings; samplings are more than 2^31 / w_baud apart"""
    gap = 2 ** 31 // w_baud + 1
    return 61 + (-(-max_out // gap) - 1) // 24


def _odd(b):
    return bin(b).count("1") & 1


class Oracle:
    def __init__(self, nk, fs_out, par=None):
        self.nk = self.nd = int(nk)
        self.L, self.tw, self.c = tables(fs_out)
        self.H = 5 * self.L
        self.par = params(fs_out) if par is None else par
        self.hist = np.zeros((self.nk, self.H), np.complex64)
        self.m = 0
        self.s = {k: [0] * self.nd for k in INTS}
        self.frames = np.zeros((self.nd, FRAME_WORDS), np.uint32)
        self.bcs_checks = 0                                               # block checks reached, good or not

    # ---- steps 1 to 4: [nk][n] complex64 -> q float32 [nk][n]
    def detector(self, y):
        L, H, n = self.L, self.H, y.shape[1]
        yy = np.concatenate((self.hist, np.asarray(y, np.complex64)), axis=1)
        re, im = np.ascontiguousarray(yy.real), np.ascontiguousarray(yy.imag)
        with np.errstate(invalid="ignore", over="ignore"):
            p = re * re + im * im
            p = np.where(p <= self.par["pmax"], p, np.float32(0)).astype(np.float32)   # column j: the sample m0 - 5 L + j
            na = L + n                                                    # a of the outputs m0 - L ...: its newest power at 4 L + j
            br = bi = None
            for i in range(4 * L + 1):
                seg = p[:, 4 * L - i:4 * L - i + na]
                tr, ti = self.c[i, 0] * seg, self.c[i, 1] * seg
                br, bi = (tr, ti) if i == 0 else (br + tr, bi + ti)
            idx = ((self.m - L + np.arange(na)) % 2 ** 32).astype(np.uint64)   # only the low 32 bits matter
            k = (((idx * np.uint64(self.par["w_car"])) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)).astype(np.int64)
            tx, ty = self.tw[k, 0][None, :], self.tw[k, 1][None, :]
            ar, ai = br * tx - bi * ty, br * ty + bi * tx
            q = ai[:, L:] * ar[:, :-L] - ar[:, L:] * ai[:, :-L]
        return q.astype(np.float32)

    def process(self, y):
        """the rows' outputs of one call -> (counts int32 [nd], the event words of every decoder as lists)"""
        y = np.asarray(y, np.complex64)
        n = y.shape[1]
        counts, ev = np.zeros(self.nd, np.int32), [[] for _ in range(self.nd)]
        if n == 0:
            return counts, ev
        x = (self.detector(y) > 0).astype(np.int64)
        clk, xprev = np.array(self.s["clk"], np.int64), np.array(self.s["xprev"], np.int64)
        w, sh = self.par["w_baud"], self.par["pll_shift"]
        for j in range(n):
            xj = x[:, j]
            c = ((clk + w + 2 ** 31) & 0xFFFFFFFF) - 2 ** 31
            c = np.where(xj != xprev, c - (c >> sh), c)
            hit = (clk >= 0) & (c < 0)
            clk, xprev = c, xj
            if hit.any():
                for dcd in np.flatnonzero(hit):
                    self._sample(int(dcd), int(xj[dcd]), j, ev[dcd])
        self.s["clk"], self.s["xprev"] = [int(v) for v in clk], [int(v) for v in xprev]
        self.hist = np.concatenate((self.hist, y), axis=1)[:, -self.H:]
        self.m += n
        for dcd in range(self.nd):
            counts[dcd] = len(ev[dcd])
        return counts, ev

    # ---- steps 6 to 8
    def _store(self, d, b):
        s = self.s
        at = s["nbytes"][d]
        if at < FRAME_BYTES:                                               # a byte that opens a word clears the rest of it
            k, q = at >> 2, 8 * (at & 3)
            self.frames[d, k] = (int(self.frames[d, k]) & ((1 << q) - 1)) | (b << q)
        crc = s["crc"][d]
        for _ in range(8):
            crc = (crc >> 1) ^ (0x8408 if (crc ^ b) & 1 else 0)
            b >>= 1
        s["crc"][d], s["nbytes"][d] = crc, at + 1

    def _sample(self, d, x, j, ev):
        s = self.s
        s["lev"][d] ^= 1 - x
        bit = s["lev"][d]
        s["sr"][d] = (s["sr"][d] >> 1) | (bit << 15)
        st = s["st"][d]
        if st == SEARCH:
            if s["sr"][d] in (0x1616, 0xE9E9):
                if s["sr"][d] == 0xE9E9:
                    s["lev"][d] ^= 1
                s["st"][d], s["nb"][d], s["byte"][d] = SOH, 0, 0
            return
        s["byte"][d] |= bit << s["nb"][d]
        s["nb"][d] += 1
        if s["nb"][d] < 8:
            return
        b = s["byte"][d]
        s["nb"][d], s["byte"][d] = 0, 0
        if st == SOH:
            if b == 0x01:
                s["st"][d], s["crc"][d], s["nbytes"][d] = TEXT, 0, 0
            else:
                s["st"][d] = SEARCH
        elif st == TEXT:
            if not _odd(b):
                s["st"][d] = SEARCH
                return
            self._store(d, b)
            if b & 0x7F in (0x03, 0x17):
                s["st"][d] = BCS1
            elif s["nbytes"][d] >= MAX_BYTES:
                s["st"][d] = SEARCH
        elif st == BCS1:
            self._store(d, b)
            s["st"][d] = BCS2
        else:
            self._store(d, b)
            self.bcs_checks += 1
            n = s["nbytes"][d] - 2
            if s["crc"][d] == 0 and n >= MIN_BYTES:
                data = self.frames[d].astype("<u4").tobytes()[:n] + b"\0" * (-n % 4)
                ev.append(_i32((j << 10) | n))
                ev.extend(_i32(v) for v in np.frombuffer(data, "<u4"))
            s["st"][d] = SEARCH

    def state(self):
        out = {k: np.array(self.s[k], np.int32) for k in INTS}
        out["frames"] = self.frames.copy()
        return out

    def set_state(self, st, hist, m):
        """continue from a state: ``hist`` are the rows' last 5 L outputs, ``m`` the outputs complete so far"""
        self.s = {k: [int(v) for v in st[k]] for k in INTS}
        self.frames = np.array(st["frames"], np.uint32)
        self.hist = np.array(hist, np.complex64)
        assert self.hist.shape == (self.nk, self.H)
        self.m = int(m)


def _i32(v):
    v = int(v) & 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def unpack(words):
    """a decoder's event words of one call -> [(index within the call, bytes)]"""
    out, at = [], 0
    while at < len(words):
        h = int(words[at]) & 0xFFFFFFFF
        i, n = h >> 10, h & 1023
        nw = (n + 3) // 4
        data = b"".join((int(v) & 0xFFFFFFFF).to_bytes(4, "little") for v in words[at + 1:at + 1 + nw])
        assert len(data) == 4 * nw and not any(data[n:])
        out.append((i, data[:n]))
        at += 1 + nw
    return out


class Skimmer:
    """The oracle and the host's rule behind it.  Raw records (m, row, bytes) with equal bytes, at most 4 L outputs apart
    and on rows less than fs_out / 2 apart (on the circle of fs) are copies of one frame, and so are records that a chain
    of such pairs joins.  Once 4 L outputs lie behind the latest of a frame's records it becomes one record: the lowest of
    its rows, with that row's earliest m.  Kept here as a list of raw records per frame, joined by search."""

    def __init__(self, nk, fs, fs_out, freqs, max_out=4096, par=None):
        self.o = Oracle(nk, fs_out, par)
        self.fs, self.fs_out, self.freqs, self.max_out = fs, fs_out, np.asarray(freqs, np.float64), max_out
        self.reach = 4 * self.o.L
        self.sets, self.frames = [], []

    def _copies(self, a, b):
        d = abs(self.freqs[a[1]] - self.freqs[b[1]]) % self.fs
        return a[2] == b[2] and abs(a[0] - b[0]) <= self.reach and min(d, self.fs - d) < self.fs_out / 2 - 1e-6

    def push(self, y, flush=False):
        """rows [nk][N], cut into calls of max_out outputs -> [(m, row, bytes)]"""
        out = []
        for at in range(0, y.shape[1], self.max_out):
            m0 = self.o.m
            counts, ev = self.o.process(y[:, at:at + self.max_out])
            out += self.take([(m0 + i, d, data) for d in range(self.o.nd) for i, data in unpack(ev[d])], self.o.m)
        if flush:
            out += self._leave(lambda st: True)
        return out

    def take(self, raw, m_done):
        for rec in sorted(raw):
            joined = [st for st in self.sets if any(self._copies(rec, q) for q in st)]
            self.sets = [st for st in self.sets if not any(st is j for j in joined)] + [sum(joined, []) + [rec]]
        return self._leave(lambda st: m_done - 1 - max(q[0] for q in st) >= self.reach)

    def _leave(self, done):
        gone = sorted((st for st in self.sets if done(st)), key=lambda st: (max(q[0] for q in st), min(st)[:2]))
        self.sets = [st for st in self.sets if not done(st)]
        out = []
        for st in gone:
            best = min(q[1] for q in st)
            rec = (min(q[0] for q in st if q[1] == best), best, st[0][2])
            self.frames.append(rec)
            out.append(rec)
        return out


# ---- the input the tests share ---------------------------------------------------------------------------------------
def scene(fs, n, stations, fs_out, waveform, seed=0, floor_db=-40.0):
    """complex64 [n]: noise at ``floor_db`` (power in the row bandwidth fs_out, re full scale 1) and stations (characters,
    f0 Hz, C/N dB of the carrier in the row bandwidth, AM depth, start sample[, inverted]), each a ``waveform`` of the
    product's test-signal helper"""
    rng = np.random.default_rng(seed)
    pn = 10 ** (floor_db / 10) * fs / fs_out                              # noise power over the whole band
    x = np.sqrt(pn / 2) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for chars, f0, cn, depth, start, *inv in stations:
        s = waveform(chars, fs, f0, depth=depth, invert=bool(inv and inv[0])).astype(np.complex128) * 10 ** ((floor_db + cn) / 20)
        # the carrier's phase at sample 0 of the transmission is that of a free-running oscillator
        s = s[:max(0, n - start)] * np.exp(2j * np.pi * f0 * start / fs)
        x[start:start + len(s)] += s
    return x.astype(np.complex64)
