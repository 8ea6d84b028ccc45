"""NumPy twin of the RDS skimmer's definition, float32 with every operation rounded on its own, and
of the skimmer's de-duplication.  Test infrastructure only: it shares no code with pysdr_amd/rds.py beyond the numbers of
the definition, which it derives again.

* ``Oracle``: steps 1 to 6 on the rows of a channelizer, any cut into calls; ``process`` / ``state`` / ``set_state``.
* ``Skimmer``: the oracle behind the host's rule that makes one record of a group's copies.
* ``cap_of``: the event cap, as DESIGN.md derives it.
* ``scene``: stations with noise, the input the CPU and the GPU tests share.
"""
import numpy as np

PHASES, SEG = 16, 64
POLY = 0x5B9
OFF_A, OFF_B, OFF_C, OFF_C2, OFF_D = 0x0FC, 0x198, 0x168, 0x350, 0x1B4
A0, A1, A2, A3, A4 = (np.float32(v) for v in (0.9998660, -0.3302995, 0.1801410, -0.0851330, 0.0208351))
PI, HALF_PI, FLT_MAX = np.float32(np.pi), np.float32(np.pi / 2), np.finfo(np.float32).max
MASK26 = (1 << 26) - 1


def _shaping(t):
    return 2.0 * (np.sinc(0.5 + 4.0 * t) + np.sinc(0.5 - 4.0 * t))


def tables(fs_out):
    L = 2 * int(np.floor(fs_out / 1187.5)) + 1
    k = np.arange(1024)
    tw = np.stack((np.cos(2 * np.pi * k / 1024), -np.sin(2 * np.pi * k / 1024)), axis=1).astype(np.float32)
    t = (np.arange(L) - (L - 1) // 2) * (1187.5 / fs_out)
    g = _shaping(t + 0.25) - _shaping(t - 0.25)
    return L, tw, (g / np.abs(g).sum()).astype(np.float32)


def word19(fs_out):
    return int(round(19000.0 / fs_out * 2 ** 32))


def cap_of(max_out, w19):
    """three words per bit; a phase gets every sixteenth of the call's chips, which are at most floor(n w19 / 2^32) + 1"""
    return 3 * -(-((max_out * w19 >> 32) + 1) // 16)


def syndromes(b):
    """the remainders of 26-bit blocks (uint32 array) by g(x)"""
    b = np.array(b, np.uint32)
    for k in range(25, 9, -1):
        b = np.where((b >> np.uint32(k)) & np.uint32(1), b ^ np.uint32(POLY << (k - 10)), b)
    return b


def arg(y, y1):
    """step 1: d = arg(y conj(y1)), float32, every operation rounded on its own; 0 where the product is 0 or not finite"""
    f = np.float32
    yr, yi, pr, pi = (np.ascontiguousarray(v, np.float32) for v in (y.real, y.imag, y1.real, y1.imag))
    with np.errstate(all="ignore"):
        re = yr * pr + yi * pi
        im = yi * pr - yr * pi
        ax, ay = np.where(re < 0, -re, re), np.where(im < 0, -im, im)
        swap = ay > ax
        mx, mn = np.where(swap, ay, ax), np.where(swap, ax, ay)
        ok = (mx > 0) & (mx <= FLT_MAX) & (mn <= mx)
        t = np.where(ok, mn, f(0)) / np.where(ok, mx, f(1))
        t2 = t * t
        s = t2 * A4
        s = A3 + s; s = t2 * s
        s = A2 + s; s = t2 * s
        s = A1 + s; s = t2 * s
        s = A0 + s
        phi = t * s
        phi = np.where(swap, HALF_PI - phi, phi)
        phi = np.where(re < 0, PI - phi, phi)
        phi = np.where(im < 0, -phi, phi)
    return np.where(ok, phi, f(0)).astype(np.float32)


class Oracle:
    def __init__(self, nk, fs_out):
        self.nk, self.nd = int(nk), int(nk) * PHASES
        self.L, self.tw, self.g = tables(fs_out)
        self.w19 = word19(fs_out)
        self.hist = np.zeros((self.nk, self.L + 1), np.complex64)
        self.m = 0
        self.regs = np.zeros((4, self.nd), np.uint32)
        self.chips = np.zeros(self.nk, np.uint32)
        self.ring = np.zeros((self.nk, PHASES, 2), np.float32)

    # ---- steps 1 and 2: [nk][n] complex64 -> the products v (re, im) float32 [nk][L + n]: column c is call output c - L
    def products(self, y):
        L, n = self.L, y.shape[1]
        yy = np.concatenate((self.hist, np.asarray(y, np.complex64)), axis=1)
        d = arg(yy[:, 1:], yy[:, :-1])
        idx = ((self.m - L + np.arange(L + n)) % 2 ** 32).astype(np.uint64)   # only the low 32 bits matter
        k = (((idx * np.uint64(3 * self.w19)) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)).astype(np.int64)
        return d * self.tw[k, 0][None, :], d * self.tw[k, 1][None, :]

    def ticks(self, n):
        """the call's outputs that open a chip"""
        i = ((self.m + np.arange(n)) % 2 ** 32).astype(np.uint64)
        return np.flatnonzero(((i * np.uint64(self.w19)) & np.uint64(0xFFFFFFFF)) < np.uint64(self.w19))

    # ---- step 3: z (re, im) float32 [nk][chips] at the call's outputs jj
    def matched(self, vx, vy, jj):
        L, g = self.L, self.g
        zx = zy = None
        for lo in range(0, L, SEG):
            ux, uy = g[lo] * vx[:, L + jj - lo], g[lo] * vy[:, L + jj - lo]
            for i in range(lo + 1, min(L, lo + SEG)):
                ux, uy = ux + g[i] * vx[:, L + jj - i], uy + g[i] * vy[:, L + jj - i]
            zx, zy = (ux, uy) if lo == 0 else (zx + ux, zy + uy)
        return zx, zy

    def process(self, y):
        """the rows' outputs of one call -> (counts int32 [nd], the event words of every decoder as lists)"""
        y = np.asarray(y, np.complex64)
        n = y.shape[1]
        counts, ev = np.zeros(self.nd, np.int32), [[] for _ in range(self.nd)]
        if n == 0:
            return counts, ev
        jj = self.ticks(n)
        if len(jj):
            vx, vy = self.products(y)
            zx, zy = self.matched(vx, vy, jj)
            self._decide(zx, zy, jj, ev)
        self.hist = np.concatenate((self.hist, y), axis=1)[:, -(self.L + 1):]
        self.m += n
        self.chips = ((self.chips.astype(np.int64) + len(jj)) % 2 ** 32).astype(np.uint32)
        for d in range(self.nd):
            counts[d] = len(ev[d])
        return counts, ev

    def replay(self, y, lengths):
        """``process`` for a stream cut into calls of ``lengths`` outputs, with steps 1 to 3 run once over the whole of it:
        -> [(counts, event words, state after the call)].  The definition does not depend on the cut, so this equals call
        after call of ``process`` (tests/test_rds_oracle.py holds the two together); it is what makes a thousand calls of
        256 outputs affordable."""
        y = np.asarray(y, np.complex64)
        assert sum(lengths) == y.shape[1]
        jj = self.ticks(y.shape[1])
        zx, zy = self.matched(*self.products(y), jj) if len(jj) else (None, None)
        out, at = [], 0
        for n in lengths:
            a, b = np.searchsorted(jj, (at, at + n))
            ev = [[] for _ in range(self.nd)]
            if b > a:
                self._decide(zx[:, a:b], zy[:, a:b], jj[a:b] - at, ev)
            self.chips = ((self.chips.astype(np.int64) + (b - a)) % 2 ** 32).astype(np.uint32)
            self.m += n
            at += n
            out.append((np.array([len(e) for e in ev], np.int32), ev, self.state()))
        self.hist = np.concatenate((self.hist, y), axis=1)[:, -(self.L + 1):]
        return out

    # ---- steps 4 to 6, a bit of every phase at a time
    def _decide(self, zx, zy, jj, ev):
        nc = len(jj)
        first = (np.arange(PHASES)[None, :] - self.chips.astype(np.int64)[:, None]) % PHASES     # [nk][16]: each phase's first chip
        rows = np.arange(self.nk)[:, None]
        regs = self.regs.reshape(4, self.nk, PHASES)
        k = 0
        while True:
            ci = first + PHASES * k
            live = ci < nc
            if not live.any():
                break
            cc = np.minimum(ci, nc - 1)
            x, yv = zx[rows, cc], zy[rows, cc]
            with np.errstate(all="ignore"):
                q = x * self.ring[:, :, 0] + yv * self.ring[:, :, 1]
            bit = (q < 0).astype(np.uint32)
            self.ring[:, :, 0] = np.where(live, x, self.ring[:, :, 0])
            self.ring[:, :, 1] = np.where(live, yv, self.ring[:, :, 1])
            new = [((regs[b] << np.uint32(1)) | (regs[b + 1] >> np.uint32(25) if b < 3 else bit)) & np.uint32(MASK26) for b in range(4)]
            for b in range(4):
                regs[b] = np.where(live, new[b], regs[b])
            sc = syndromes(regs[2])
            hit = live & (syndromes(regs[0]) == OFF_A) & (syndromes(regs[1]) == OFF_B) & ((sc == OFF_C) | (sc == OFF_C2)) & (syndromes(regs[3]) == OFF_D)
            for a, p in np.argwhere(hit):
                w = [int(regs[b, a, p]) >> 10 for b in range(4)]
                ev[a * PHASES + p] += [_i32(int(jj[ci[a, p]]) << 5 | int(p) << 1 | int(sc[a, p] == OFF_C2)), _i32(w[0] << 16 | w[1]), _i32(w[2] << 16 | w[3])]
            k += 1

    def state(self):
        return dict(regs=self.regs.copy(), chips=self.chips.copy(), ring=self.ring.copy())

    def set_state(self, st, hist, m):
        """continue from a state: ``hist`` are the rows' last L + 1 outputs, ``m`` the outputs complete so far"""
        self.regs, self.chips = np.array(st["regs"], np.uint32), np.array(st["chips"], np.uint32)
        self.ring = np.array(st["ring"], np.float32)
        self.hist = np.array(hist, np.complex64)
        assert self.hist.shape == (self.nk, self.L + 1)
        self.m = int(m)


def _i32(v):
    v = int(v) & 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def unpack(words):
    """a decoder's event words of one call -> [(index within the call, phase, (a, b, c, d, C' flag))]"""
    out = []
    for at in range(0, len(words), 3):
        h, ab, cd = (int(v) & 0xFFFFFFFF for v in words[at:at + 3])
        out.append((h >> 5, h >> 1 & 15, (ab >> 16, ab & 0xFFFF, cd >> 16, cd & 0xFFFF, h & 1)))
    return out


def same_state(got, want, where=""):
    """every state field EQUAL, the floats bit for bit"""
    assert np.array_equal(got["regs"], want["regs"]), (where, "regs", np.argwhere(got["regs"] != want["regs"])[:5])
    assert np.array_equal(got["chips"], want["chips"]), (where, "chips", got["chips"][:4], want["chips"][:4])
    a, b = np.asarray(got["ring"], np.float32).view(np.uint32), np.asarray(want["ring"], np.float32).view(np.uint32)
    assert np.array_equal(a, b), (where, "ring", np.argwhere(a != b)[:5])


class Skimmer:
    """The oracle and the host's rule behind it.  Raw records (m, row, phase, words) with equal words, at most two bits
    of outputs apart and on rows less than fs_out / 2 apart (on the circle of fs) are copies of one group, and so are
    records that a chain of such pairs joins.  Once two bits of outputs lie behind the latest of a group's records it
    becomes one record: of its rows the one with the most phases, the lowest such, with that row's earliest m and phase
    mask.  Kept here as a list of raw records per group, joined by search."""

    def __init__(self, nk, fs, fs_out, freqs, max_out=65536):
        self.o = Oracle(nk, fs_out)
        self.fs, self.fs_out, self.freqs, self.max_out = fs, fs_out, np.asarray(freqs, np.float64), max_out
        self.reach = int(np.ceil(2 * fs_out / 1187.5))
        self.sets, self.groups = [], []

    def _copies(self, a, b):
        d = abs(self.freqs[a[1]] - self.freqs[b[1]]) % self.fs
        return a[3] == b[3] and abs(a[0] - b[0]) <= self.reach and min(d, self.fs - d) < self.fs_out / 2 - 1e-6

    def push(self, y, flush=False):
        """rows [nk][N], cut into calls of max_out outputs -> [(m, row, words, phases)]"""
        out = []
        for at in range(0, y.shape[1], self.max_out):
            m0 = self.o.m
            counts, ev = self.o.process(y[:, at:at + self.max_out])
            out += self.take([(m0 + i, d // PHASES, p, data) for d in range(self.o.nd) for i, p, data in unpack(ev[d])], self.o.m)
        if flush:
            out += self._leave(lambda st: True)
        return out

    def take(self, raw, m_done):
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
            for m, row, p, _ in st:
                e = rows.setdefault(row, [m, 0])
                e[0], e[1] = min(e[0], m), e[1] | 1 << p
            best = sorted(rows, key=lambda r: (-bin(rows[r][1]).count("1"), r))[0]
            out.append((rows[best][0], best, st[0][3], rows[best][1]))
        self.groups += out
        return out


# ---- the input the tests share ---------------------------------------------------------------------------------------
def scene(fs, n, stations, fs_out, waveform, seed=0, floor_db=-40.0):
    """complex64 [n]: noise at ``floor_db`` (power in the row bandwidth fs_out, re full scale 1) and stations (groups, f0
    Hz, C/N dB in the row bandwidth or None for no noise at all, start sample), each a ``waveform`` of the product's
    test-signal helper"""
    rng = np.random.default_rng(seed)
    pn = 10 ** (floor_db / 10) * fs / fs_out                              # noise power over the whole band
    x = np.sqrt(pn / 2) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    if any(cn is None for _, _, cn, _ in stations):
        x[:] = 0
    for groups, f0, cn, start in stations:
        s = waveform(groups, fs, f0).astype(np.complex128) * 10 ** ((floor_db + (30.0 if cn is None else cn)) / 20)
        s = s[:max(0, n - start)] * np.exp(2j * np.pi * f0 * start / fs)  # a free-running oscillator's phase at the start
        x[start:start + len(s)] += s
    return x.astype(np.complex64)
