"""NumPy twin of the packet skimmer's definition, float32 with every operation rounded on its own,
and of the skimmer's de-duplication.  Test infrastructure only: it shares no code with pysdr_amd/packet.py beyond the
numbers of the definition, which it derives again.

* ``Oracle``: steps 1 to 6 on the rows of a channelizer, any cut into calls; ``process`` / ``state`` / ``set_state``.
* ``Skimmer``: the oracle behind the host's rule that makes one record of a frame's copies.
* ``cap_of``: the event cap, as DESIGN.md derives it.
* ``scene``: stations with noise, the input the CPU and the GPU tests share.
"""
import numpy as np

SLICERS = 8
FRAME_BYTES, FRAME_WORDS = 332, 83
INTS = ("clk", "xprev", "xlast", "sr", "ones", "inframe", "byte", "nb", "nbytes", "crc")


def tables(fs_out):
    L = int(np.floor(fs_out / 1200.0 + 0.5))
    k = np.arange(1024)
    tw = np.stack((np.cos(2 * np.pi * k / 1024), -np.sin(2 * np.pi * k / 1024)), axis=1).astype(np.float32)
    return L, tw, np.full(L, 1.0 / L).astype(np.float32)


def params(fs_out, pll_shift=2, pmax=1e18, gain=None):
    g = 10.0 ** (np.arange(-6, 10, 2) / 10.0) if gain is None else np.asarray(gain, np.float64)
    return dict(gain=g.astype(np.float32), pmax=np.float32(pmax), pll_shift=int(pll_shift),
                w_mark=int(round(1200.0 / fs_out * 2 ** 32)), w_space=int(round(2200.0 / fs_out * 2 ** 32)),
                w_baud=int(round(1200.0 / fs_out * 2 ** 32)))


def cap_of(max_out, w_baud):
    """84 words for a frame carried into the call, then a word per 24 samplings; samplings are more than 2^31 / w_baud apart"""
    gap = 2 ** 31 // w_baud + 1
    return 84 + (-(-max_out // gap) - 1) // 24


class Oracle:
    def __init__(self, nk, fs_out, par=None):
        self.nk, self.nd = int(nk), int(nk) * SLICERS
        self.L, self.tw, self.g = tables(fs_out)
        self.par = params(fs_out) if par is None else par
        self.hist = np.zeros((self.nk, self.L), np.complex64)
        self.m = 0
        self.s = {k: [0] * self.nd for k in INTS}
        self.s["crc"] = [0xFFFF] * self.nd
        self.frames = np.zeros((self.nd, FRAME_WORDS), np.uint32)
        self.fcs_checks = 0                                               # flags that closed 17 bytes or more, good or not

    # ---- steps 1 and 2: [nk][n] complex64 -> P_mark, P_space float32 [nk][n]
    def powers(self, y):
        L, n = self.L, y.shape[1]
        yy = np.concatenate((self.hist, np.asarray(y, np.complex64)), axis=1)
        re, im = np.ascontiguousarray(yy.real), np.ascontiguousarray(yy.imag)
        with np.errstate(invalid="ignore", over="ignore"):
            d = im[:, 1:] * re[:, :-1] - re[:, 1:] * im[:, :-1]           # d of the samples m0 - L + 1 ...
            idx = ((self.m - L + 1 + np.arange(L + n - 1)) % 2 ** 32).astype(np.uint64)   # only the low 32 bits matter
            out = []
            for w in (self.par["w_mark"], self.par["w_space"]):
                k = (((idx * np.uint64(w)) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)).astype(np.int64)
                vx, vy = d * self.tw[k, 0][None, :], d * self.tw[k, 1][None, :]
                ux = uy = None
                for i in range(L):                                       # output j's newest product sits at L - 1 + j
                    tx, ty = self.g[i] * vx[:, L - 1 - i:L - 1 - i + n], self.g[i] * vy[:, L - 1 - i:L - 1 - i + n]
                    ux, uy = (tx, ty) if i == 0 else (ux + tx, uy + ty)
                p = ux * ux + uy * uy
                out.append(np.where(p <= self.par["pmax"], p, np.float32(0)).astype(np.float32))
        return out

    def process(self, y):
        """the rows' outputs of one call -> (counts int32 [nd], the event words of every decoder as lists)"""
        y = np.asarray(y, np.complex64)
        n = y.shape[1]
        counts, ev = np.zeros(self.nd, np.int32), [[] for _ in range(self.nd)]
        if n == 0:
            return counts, ev
        pm, ps = self.powers(y)
        with np.errstate(invalid="ignore", over="ignore"):
            x = (self.par["gain"][None, :, None] * ps[:, None, :] > pm[:, None, :]).reshape(self.nd, n).astype(np.int64)
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
        self.hist = np.concatenate((self.hist, y), axis=1)[:, -self.L:]
        self.m += n
        for dcd in range(self.nd):
            counts[dcd] = len(ev[dcd])
        return counts, ev

    # ---- steps 5 and 6
    def _sample(self, d, x, j, ev):
        s = self.s
        bit = 1 if x == s["xlast"][d] else 0
        s["xlast"][d] = x
        s["sr"][d] = (s["sr"][d] >> 1) | (bit << 7)
        if s["sr"][d] == 0x7E:
            nbytes = s["nbytes"][d]
            if s["inframe"][d] and s["nb"][d] == 7 and nbytes >= 17:
                self.fcs_checks += 1
                if s["crc"][d] == 0xF0B8:
                    n = nbytes - 2
                    data = self.frames[d].astype("<u4").tobytes()[:n] + b"\0" * (-n % 4)
                    ev.append(_i32((j << 10) | n))
                    ev.extend(_i32(v) for v in np.frombuffer(data, "<u4"))
            s["inframe"][d], s["nb"][d], s["byte"][d], s["nbytes"][d], s["ones"][d], s["crc"][d] = 1, 0, 0, 0, 0, 0xFFFF
            return
        if bit:
            s["ones"][d] += 1
            if s["ones"][d] >= 7:
                s["inframe"][d] = 0
        else:
            stuffed = s["ones"][d] == 5
            s["ones"][d] = 0
            if stuffed:
                return
        if not s["inframe"][d]:
            return
        s["byte"][d] |= bit << s["nb"][d]
        s["nb"][d] += 1
        if s["nb"][d] < 8:
            return
        b, at = s["byte"][d], s["nbytes"][d]
        if at < FRAME_BYTES:                                               # a byte that opens a word clears the rest of it
            k, q = at >> 2, 8 * (at & 3)
            self.frames[d, k] = (int(self.frames[d, k]) & ((1 << q) - 1)) | (b << q)
        crc = s["crc"][d]
        for _ in range(8):
            crc = (crc >> 1) ^ (0x8408 if (crc ^ b) & 1 else 0)
            b >>= 1
        s["crc"][d], s["nbytes"][d], s["nb"][d], s["byte"][d] = crc, at + 1, 0, 0
        if at + 1 > FRAME_BYTES:
            s["inframe"][d] = 0

    def state(self):
        out = {k: np.array(self.s[k], np.int32) for k in INTS}
        out["frames"] = self.frames.copy()
        return out

    def set_state(self, st, hist, m):
        """continue from a state: ``hist`` are the rows' last L outputs, ``m`` the outputs complete so far"""
        self.s = {k: [int(v) for v in st[k]] for k in INTS}
        self.frames = np.array(st["frames"], np.uint32)
        self.hist = np.array(hist, np.complex64)
        assert self.hist.shape == (self.nk, self.L)
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
    """The oracle and the host's rule behind it.  Raw records (m, row, slicer, bytes) with equal bytes, at most 4 L
    outputs apart and on rows less than fs_out / 2 apart (on the circle of fs) are copies of one frame, and so are records
    that a chain of such pairs joins.  Once 4 L outputs lie behind the latest of a frame's records it becomes one record:
    of its rows the one with the most slicers, the lowest such, with that row's earliest m and slicer mask.  Kept here
    as a list of raw records per frame, joined by search."""

    def __init__(self, nk, fs, fs_out, freqs, tnc2, max_out=4096, par=None):
        self.o = Oracle(nk, fs_out, par)
        self.fs, self.fs_out, self.freqs, self.max_out, self.tnc2 = fs, fs_out, np.asarray(freqs, np.float64), max_out, tnc2
        self.reach = 4 * self.o.L
        self.sets, self.frames, self.text = [], [], {}

    def _copies(self, a, b):
        d = abs(self.freqs[a[1]] - self.freqs[b[1]]) % self.fs
        return a[3] == b[3] and abs(a[0] - b[0]) <= self.reach and min(d, self.fs - d) < self.fs_out / 2 - 1e-6

    def push(self, y, flush=False):
        """rows [nk][N], cut into calls of max_out outputs -> [(m, row, text)]"""
        out = []
        for at in range(0, y.shape[1], self.max_out):
            m0 = self.o.m
            counts, ev = self.o.process(y[:, at:at + self.max_out])
            out += self.take([(m0 + i, d // SLICERS, d % SLICERS, data) for d in range(self.o.nd) for i, data in unpack(ev[d])], self.o.m)
        if flush:
            out += self._leave(lambda st: True)
        return out

    def take(self, raw, m_done):
        """a call's raw records and the outputs complete behind it -> the frames that are final by then"""
        for rec in sorted(raw):
            joined = [st for st in self.sets if any(self._copies(rec, q) for q in st)]
            self.sets = [st for st in self.sets if not any(st is j for j in joined)] + [sum(joined, []) + [rec]]
        return self._leave(lambda st: m_done - 1 - max(q[0] for q in st) >= self.reach)

    def _leave(self, done):
        gone = sorted((st for st in self.sets if done(st)), key=lambda st: (max(q[0] for q in st), min(st)[:3]))
        self.sets = [st for st in self.sets if not done(st)]
        out = []
        for st in gone:
            rows = {}
            for m, row, s, _ in st:
                e = rows.setdefault(row, [m, 0])
                e[0], e[1] = min(e[0], m), e[1] | 1 << s
            best = sorted(rows, key=lambda r: (-bin(rows[r][1]).count("1"), r))[0]
            m, mask = rows[best]
            self.frames.append((m, best, st[0][3], mask))
            line = self.tnc2(st[0][3])
            self.text[best] = self.text.get(best, "") + line + "\n"
            out.append((m, best, line))
        return out


# ---- the input the tests share ---------------------------------------------------------------------------------------
def scene(fs, n, stations, fs_out, waveform, seed=0, floor_db=-40.0):
    """complex64 [n]: noise at ``floor_db`` (power in the row bandwidth fs_out, re full scale 1) and stations (frames, f0
    Hz, C/N dB in the row bandwidth, tone balance, start sample), each a ``waveform`` of the product's test-signal helper"""
    rng = np.random.default_rng(seed)
    pn = 10 ** (floor_db / 10) * fs / fs_out                              # noise power over the whole band
    x = np.sqrt(pn / 2) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for frames, f0, cn, bal, start in stations:
        s = waveform(frames, fs, f0, preemph=bal).astype(np.complex128) * 10 ** ((floor_db + cn) / 20)
        # the carrier's phase at sample 0 of the transmission is that of a free-running oscillator
        s = s[:max(0, n - start)] * np.exp(2j * np.pi * f0 * start / fs)
        x[start:start + len(s)] += s
    return x.astype(np.complex64)
