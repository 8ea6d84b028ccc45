"""NumPy twin of the SSTV skimmer's definition, float32 with every operation rounded on its own.
Test infrastructure only: it shares no code with pysdr_amd/sstv.py beyond the numbers of the definition, which it derives
again.

* ``Oracle``: steps 1 to 8 on the rows of a channelizer, any cut into calls; ``process`` / ``state``.  ``twin=True`` is
  the float64 form of the same definition with ``np.arctan2`` and float64 sums, the yardstick of the accuracy tests.
* ``cap_of``: the event cap, as DESIGN.md derives it.
* ``unpack``: event words -> records.
"""
import numpy as np
from scipy.signal import firwin

INTS = ("ticks", "phase", "mode", "m_a", "e0", "line", "pix")
FLOATS = ("acc_re", "acc_im", "bprev_re", "bprev_im", "f_lead", "pacc_re", "pacc_im")
LINE_WORDS = 800
A = [np.float32(v) for v in (0.9998660, -0.3302995, 0.1801410, -0.0851330, 0.0208351)]
TOL, LEAD_MAX = np.float32(40.0), np.float32(150.0)
F32 = np.float32
U32 = 0xFFFFFFFF

# name, code, scans, width, sent lines, sync, porch, pixel, separator (ms)
MODES = [("PD50", 93, 4, 320, 128, 20.0, 2.08, 0.286, 0.0), ("PD90", 99, 4, 320, 128, 20.0, 2.08, 0.532, 0.0),
         ("PD120", 95, 4, 640, 248, 20.0, 2.08, 0.19, 0.0), ("PD160", 98, 4, 512, 200, 20.0, 2.08, 0.382, 0.0),
         ("PD180", 96, 4, 640, 248, 20.0, 2.08, 0.286, 0.0), ("PD240", 97, 4, 640, 248, 20.0, 2.08, 0.382, 0.0),
         ("PD290", 94, 4, 800, 308, 20.0, 2.08, 0.286, 0.0), ("Martin M1", 44, 3, 320, 256, 4.862, 0.572, 0.4576, 0.572),
         ("Martin M2", 40, 3, 320, 256, 4.862, 0.572, 0.2288, 0.572)]
TINY = ("TINY", 5, 3, 32, 6, 5.0, 1.0, 0.5, 0.5)                            # scan 16 ms


def tables(fs_out):
    L = 2 * int(np.floor(0.75 * fs_out / 1000.0)) + 1
    k = np.arange(1024)
    tw = np.stack((np.cos(2 * np.pi * k / 1024), -np.sin(2 * np.pi * k / 1024)), axis=1).astype(np.float32)
    return L, tw, firwin(L, 1900.0, window="hamming", fs=fs_out).astype(np.float32)


def q16(ms, fs_out):
    return int(round(ms * 1e-3 * fs_out * 65536.0))


def params(fs_out, det="FM", modes=MODES, offset=0.0, pmax=1e18):
    R0, W = int(round(0.010 * fs_out)), int(round(fs_out / 500.0))
    f_sub = (1900.0 if det == "FM" else 0.0) + offset
    return dict(det=det, w_sub=int(round(f_sub / fs_out * 2 ** 32)) & U32, w_tick=int(round(100.0 / fs_out * 2 ** 32)),
                k_hz=F32(fs_out / (2 * np.pi)), k_rho=F32(1024.0 / fs_out), pmax=F32(pmax), R0=R0, W=W, lag=2 * R0 + W + 1,
                modes=[dict(name=m[0], code=m[1], scans=m[2], width=m[3], lines=m[4], sync_q=q16(m[5], fs_out), porch_q=q16(m[6], fs_out),
                            scan_q=q16(m[7] * m[3], fs_out), sep_q=q16(m[8], fs_out)) for m in modes])


def line_q(md):
    return md["sync_q"] + md["porch_q"] + md["scans"] * (md["scan_q"] + md["sep_q"])


def cap_of(max_out, par):
    """two line events are never closer than the least ((line - separator) >> 16) - 2 outputs; each brings at most its line's
    words and 2, an end (2) and a start (5); one more start"""
    gap = min(((line_q(md) - md["sep_q"]) >> 16) - 2 for md in par["modes"])
    nw = max((md["scans"] * md["width"] + 3) // 4 for md in par["modes"])
    return -(-max_out // gap) * (nw + 9) + 5


def _i32(v):
    v = int(v) & U32
    return v - (1 << 32) if v >= 1 << 31 else v


def _s32(v):
    """the low 32 bits as a signed difference"""
    return _i32(v)


def seqsum(first, seg, dt):
    """first + seg[0] + seg[1] ... one addition at a time (first None: the first term is assigned)"""
    if first is not None:
        seg = np.concatenate((np.array([first], dt), seg))
    return np.cumsum(seg, dtype=dt)[-1]


def phi32(t):
    """the five-term arctangent of Abramowitz & Stegun 4.4.47 on |t| <= 1, every operation rounded to float32"""
    t = F32(t)
    t2 = t * t
    s = t2 * A[4]
    for a in (A[3], A[2], A[1]):
        s = a + s
        s = t2 * s
    s = A[0] + s
    return t * s


class Oracle:
    def __init__(self, nk, fs_out, det="FM", modes=MODES, par=None, twin=False):
        self.nk = int(nk)
        self.dt = np.float64 if twin else np.float32
        self.twin = twin
        self.L, self.tw, self.g = tables(fs_out)
        if twin:
            k = np.arange(1024)
            self.tw = np.stack((np.cos(2 * np.pi * k / 1024), -np.sin(2 * np.pi * k / 1024)), axis=1)
            self.g = firwin(self.L, 1900.0, window="hamming", fs=fs_out)
        self.par = params(fs_out, det, modes) if par is None else par
        p = self.par
        self.nq = 2 * p["R0"] + 2 * p["W"]
        self.H = self.nq + self.L + 1
        self.hist = np.zeros((self.nk, self.H), np.complex128 if twin else np.complex64)
        self.m = 0
        z = self.dt(0)
        self.rows = [dict(ticks=0, phase=0, mode=-1, m_a=0, e0=0, line=0, pix=0, acc=[z, z], bprev=[z, z], f_lead=z, pacc=[z, z])
                     for _ in range(self.nk)]
        self.ring = np.zeros((self.nk, 64), self.dt)
        self.lines = np.zeros((self.nk, LINE_WORDS), np.uint32)

    # ---- steps 1 and 2: the lag products of the samples -nq .. n - 1 from the call's first output: [nk][nq + n] re, im
    def lag_products(self, y):
        L, n, p, dt = self.L, y.shape[1], self.par, self.dt
        yy = np.concatenate((self.hist, y), axis=1)                       # column k is sample k - H
        re, im = np.ascontiguousarray(yy.real, dt), np.ascontiguousarray(yy.imag, dt)
        with np.errstate(invalid="ignore", over="ignore"):
            idx = ((self.m - self.H + 1 + np.arange(self.H + n - 1)) % 2 ** 32).astype(np.uint64)      # samples 1 - H ...
            k = (((idx * np.uint64(p["w_sub"])) & np.uint64(U32)) >> np.uint64(22)).astype(np.int64)
            tx, ty = self.tw[k, 0][None, :], self.tw[k, 1][None, :]
            if p["det"] == "FM":
                d = im[:, 1:] * re[:, :-1] - re[:, 1:] * im[:, :-1]
                vx, vy = d * tx, d * ty
            else:
                vx, vy = re[:, 1:] * tx - im[:, 1:] * ty, re[:, 1:] * ty + im[:, 1:] * tx
            # v column c is sample c + 1 - H; u for the samples -nq - 1 .. n - 1: nq + 1 + n of them, the newest product of the
            # first at column H - nq - 2 = L - 1
            nu = self.nq + 1 + n
            ux = uy = None
            for i in range(L):
                a, b = self.g[i] * vx[:, L - 1 - i:L - 1 - i + nu], self.g[i] * vy[:, L - 1 - i:L - 1 - i + nu]
                ux, uy = (a, b) if i == 0 else (ux + a, uy + b)
            pw = ux * ux + uy * uy
            ok = (pw <= p["pmax"])
            ok = ok[:, 1:] & ok[:, :-1]
            cx = ux[:, 1:] * ux[:, :-1] + uy[:, 1:] * uy[:, :-1]
            cy = uy[:, 1:] * ux[:, :-1] - ux[:, 1:] * uy[:, :-1]
            zero = dt(0)
            return np.where(ok, cx, zero).astype(dt), np.where(ok, cy, zero).astype(dt)

    # ---- step 3
    def hz(self, px, py):
        dt = self.dt
        if self.twin:
            return dt(np.clip(np.arctan2(py, px), -np.pi / 4, np.pi / 4)) * dt(self.par["k_hz"])
        px, py = F32(px), F32(py)
        with np.errstate(over="ignore", divide="ignore"):
            if px > 0:
                t = py / px
                t = F32(-1) if t < -1 else (F32(1) if t > 1 else t)
            else:
                t = F32(1) if py > 0 else (F32(-1) if py < 0 else F32(0))
        return phi32(t) * self.par["k_hz"]

    def vis(self, ring, k):
        dt = self.dt
        lead = [ring[(k - (34 + 6 * i)) & 63] for i in range(4)]
        s = lead[0]
        for v in lead[1:]:
            s = s + v
        f = s * dt(0.25)
        if not abs(f) <= LEAD_MAX or not all(abs(v - f) <= TOL for v in lead):
            return None
        code = ones = 0
        for b in range(10):
            x = ring[(k - (3 * b + 1)) & 63] - f
            if b in (0, 9):
                if not abs(x + dt(700)) <= TOL:
                    return None
                continue
            if abs(x + dt(800)) <= TOL:
                bit = 1
            elif abs(x + dt(600)) <= TOL:
                bit = 0
            else:
                return None
            ones += bit
            if b >= 2:
                code |= bit << (8 - b)
        if ones & 1:
            return None
        for i, md in enumerate(self.par["modes"]):
            if md["code"] == code:
                return i, f
        return None

    def pixel_start(self, md, e0, l, j, p):
        off = l * line_q(md) + md["porch_q"] + j * (md["scan_q"] + md["sep_q"]) + p * md["scan_q"] // md["width"]
        return (e0 + (off >> 16)) & U32

    def bounds(self, z):
        md = self.par["modes"][z["mode"]]
        j, p = divmod(z["pix"], md["width"])
        return self.pixel_start(md, z["e0"], z["line"], j, p), self.pixel_start(md, z["e0"], z["line"], j, p + 1)

    def anchor(self, z, cx, cy, ia):
        """cx, cy: the row's lag products, column k = sample k - nq of the call; ia: the index of m_a within the call"""
        p, dt, nq = self.par, self.dt, self.nq
        R0, W = p["R0"], p["W"]
        rho = self.tw[int(np.floor((z["f_lead"] - dt(550)) * dt(p["k_rho"]) + dt(0.5))) & 1023]
        a, b = cx[ia + 1:ia + 1 + nq], cy[ia + 1:ia + 1 + nq]                 # samples m_a - nq + 1 .. m_a
        im = a * dt(rho[1]) + b * dt(rho[0])
        q = np.where((a == 0) & (b == 0), 0, np.where(im < 0, 1, -1)).astype(np.int64)
        cs = np.concatenate(([0], np.cumsum(q)))
        t = np.arange(2 * R0 + 1)
        D = (cs[t + W] - cs[t]) - (cs[t + 2 * W] - cs[t + W])
        first = (z["m_a"] - (nq - 1)) & U32
        return (first + W + int(np.argmax(D))) & U32

    def process(self, y):
        """the rows' outputs of one call -> (counts int32 [nk], the event words of every row as lists)"""
        y = np.asarray(y, self.hist.dtype)
        n = y.shape[1]
        counts, ev = np.zeros(self.nk, np.int32), [[] for _ in range(self.nk)]
        if n == 0:
            return counts, ev
        cx, cy = self.lag_products(y)
        w = self.par["w_tick"]
        mm = (self.m + np.arange(n + 1)) % 2 ** 32                          # tick ends: output i with ((m + 1) w mod 2^32) < w
        ends = np.flatnonzero(((mm[1:] * w) % 2 ** 32) < w)
        for r in range(self.nk):
            self._row(r, cx[r], cy[r], n, ends, ev[r])
            counts[r] = len(ev[r])
        self.hist = np.concatenate((self.hist, y), axis=1)[:, -self.H:]
        self.m += n
        return counts, ev

    def _row(self, r, cx, cy, n, ends, ev):
        z, p, dt, nq = self.rows[r], self.par, self.dt, self.nq
        lag, m0 = p["lag"], self.m & U32
        ring = self.ring[r]
        at = 0                                                            # outputs of the call already in the tick sum
        te = 0                                                            # next tick end: ends[te]
        # the pixel sum covers lagged samples up to (not including) index `pat` of the call; a call begins at -lag
        pat = -lag
        while True:
            i_tick = int(ends[te]) if te < len(ends) else n
            i_other = n
            if z["phase"] == 1:
                d = _s32(z["m_a"] - m0)
                i_other = d if 0 <= d < n else n
            elif z["phase"] == 2:
                lo, hi = self.bounds(z)
                lo, hi = _s32(lo - m0), _s32(hi - m0)                     # the pixel's samples, as indices of the call
                i_other = min(hi - 1 + lag, n)
            if i_tick >= n and i_other >= n:
                break
            if i_tick <= i_other:                                         # a tick first, also at the same output
                first_new = ((((m0 + at) & U32) * p["w_tick"]) & U32) < p["w_tick"]
                sx, sy = cx[nq + at:nq + i_tick + 1], cy[nq + at:nq + i_tick + 1]
                z["acc"] = [seqsum(None if first_new else z["acc"][0], sx, dt), seqsum(None if first_new else z["acc"][1], sy, dt)]
                at = i_tick + 1
                te += 1
                P = (z["acc"][0] + z["bprev"][0], z["acc"][1] + z["bprev"][1])
                z["bprev"] = list(z["acc"])
                k = z["ticks"]
                ring[k & 63] = self.hz(*P)
                z["ticks"] = (k + 1) & U32
                if z["phase"] == 0:
                    hit = self.vis(ring, k)
                    if hit is not None:
                        md = p["modes"][hit[0]]
                        z["phase"], z["mode"], z["f_lead"] = 1, hit[0], hit[1]
                        z["m_a"] = (m0 + i_tick + (md["sync_q"] >> 16) + p["R0"] + p["W"]) & U32
                continue
            if z["phase"] == 1:
                e0 = self.anchor(z, cx, cy, i_other)
                z.update(phase=2, e0=e0, line=0, pix=0, pacc=[dt(0), dt(0)])
                md = p["modes"][z["mode"]]
                ev += [_i32(i_other << 12 | 1 << 10 | 4), z["mode"], md["code"], _i32(np.array([z["f_lead"]], np.float32).view(np.uint32)[0]), _i32(e0)]
                continue
            # a pixel ends at output i_other: its samples lo .. hi - 1, of which those before `pat` are in pacc already
            a = max(lo, pat)
            fresh = a == lo
            sx, sy = cx[nq + a:nq + hi], cy[nq + a:nq + hi]
            z["pacc"] = [seqsum(None if fresh else z["pacc"][0], sx, dt), seqsum(None if fresh else z["pacc"][1], sy, dt)]
            pat = hi
            self._pixel_done(r, z, i_other, ev)
        # the open tick and the open pixel at the end of the call
        if at < n:
            first_new = ((((m0 + at) & U32) * p["w_tick"]) & U32) < p["w_tick"]
            z["acc"] = [seqsum(None if first_new else z["acc"][0], cx[nq + at:nq + n], dt), seqsum(None if first_new else z["acc"][1], cy[nq + at:nq + n], dt)]
        if z["phase"] == 2:
            lo, hi = self.bounds(z)
            lo, hi = _s32(lo - m0), _s32(hi - m0)
            a, b = max(lo, pat), n - lag
            if a < b:
                fresh = a == lo
                z["pacc"] = [seqsum(None if fresh else z["pacc"][0], cx[nq + a:nq + b], dt), seqsum(None if fresh else z["pacc"][1], cy[nq + a:nq + b], dt)]

    def _pixel_done(self, r, z, i, ev):
        p, dt = self.par, self.dt
        md = p["modes"][z["mode"]]
        a = self.hz(z["pacc"][0], z["pacc"][1]) - z["f_lead"]
        a = a + dt(400)
        a = a * (dt(255) / dt(800))
        a = np.floor(a + dt(0.5))
        v = 0 if a < 0 else (255 if a > 255 else int(a))
        pix, nb = z["pix"], md["scans"] * md["width"]
        k, sh = pix >> 2, 8 * (pix & 3)
        self.lines[r, k] = (int(self.lines[r, k]) & ((1 << sh) - 1)) | (v << sh)   # a byte that opens a word clears the rest of it
        z["pix"] = pix + 1
        if z["pix"] == nb:
            nw = (nb + 3) // 4
            ev += [_i32(i << 12 | 2 << 10 | (1 + nw)), z["line"]] + [_i32(v) for v in self.lines[r, :nw]]
            z["pix"] = 0
            z["line"] += 1
            if z["line"] == md["lines"]:
                ev += [_i32(i << 12 | 3 << 10 | 1), md["lines"]]
                z["phase"] = 0

    def state(self):
        out = {k: np.array([_i32(z[k]) for z in self.rows], np.int32) for k in INTS}
        for k, (name, j) in zip(FLOATS, (("acc", 0), ("acc", 1), ("bprev", 0), ("bprev", 1), ("f_lead", None), ("pacc", 0), ("pacc", 1))):
            out[k] = np.array([z[name] if j is None else z[name][j] for z in self.rows], self.dt)
        out["ring"], out["lines"] = self.ring.copy(), self.lines.copy()
        return out


def unpack(words, modes, mode=None):
    """a row's event words -> [(i, "start", mode index, code, f_lead, e0) | (i, "line", number, uint8 [scans][width]) | (i, "end",
    lines)]; ``modes`` as in params()["modes"]; ``mode``: the index of the mode of a picture that began in an earlier call"""
    out, at = [], 0
    while at < len(words):
        h = int(words[at]) & U32
        i, kind, nw = h >> 12, h >> 10 & 3, h & 1023
        pl = [int(v) & U32 for v in words[at + 1:at + 1 + nw]]
        assert len(pl) == nw
        if kind == 1:
            mode = pl[0]
            out.append((i, "start", pl[0], pl[1], float(np.array([pl[2]], np.uint32).view(np.float32)[0]), pl[3]))
        elif kind == 2:
            md = modes[mode]
            nb = md["scans"] * md["width"]
            data = np.array(pl[1:], "<u4").view(np.uint8)
            assert len(pl) == 1 + (nb + 3) // 4 and not data[nb:].any()
            out.append((i, "line", pl[0], data[:nb].reshape(md["scans"], md["width"]).copy()))
        else:
            assert kind == 3
            out.append((i, "end", pl[0]))
        at += 1 + nw
    return out
