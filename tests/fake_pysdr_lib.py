"""A stand-in for the object ``pysdr_amd._lib.lib()`` returns, for tests of the Python layer that need no device
(tests/test_chan_py_trace.py).  The plan functions, ``pysdr_strerror`` and ``pysdr_last_error`` go through to the real
library, which needs no device for them.  The handle-taking calls of the channelizer, fine, bank, CW and PSK families are
answered from a tiny model: ``create`` hands out a token, a NULL or dead handle returns -1 as the C code does, ``process``
computes ``n_out`` from the model's own count of input samples and the D it was created with, and everything a call writes
(samples, counts, event words, qn, open, state) comes from a generator seeded by the call number, counts never above the cap.
The ``pysdr_ft8_*`` and ``pysdr_ft4_*`` handle calls (tests/test_ft_py_trace.py) have a model of their own further down: steps
by the quarter-symbol rule, two-word events, the refusals of the C code by call size, by ``keep`` and by the ring.

Every call is recorded in ``trace`` as one string: the name, every scalar argument, ``crc/bytes`` of what the function's
contract says it reads behind each input pointer (of the bytes; of ``quant`` of the values for taps and tables), and
``out`` or ``NULL`` for each output pointer."""
import ctypes as C
import zlib

import numpy as np


def crc(data):
    return "%08x" % (zlib.crc32(bytes(data)) & 0xFFFFFFFF)


def quant(a):
    """Floating-point data as integers on a grid of 2^-28 of the largest magnitude (non-finite values as marks), for a CRC
    that does not depend on the last bits of cos, sin, exp and log10, which differ between CPUs."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "c":
        a = a.view(a.real.dtype)
    a = a.astype(np.float64)
    fin = np.isfinite(a)
    m = np.abs(a[fin]).max() if fin.any() else 0.0
    q = np.zeros(a.shape, np.int64)
    if m > 0:
        q[fin] = np.rint(a[fin] * (2.0 ** 28 / m))
    q[~fin] = np.where(np.isnan(a[~fin]), 1 << 40, np.where(a[~fin] > 0, 1 << 41, -(1 << 41)))
    return q.tobytes()


def _addr(p):
    if p is None:
        return 0
    if isinstance(p, int):
        return p
    if hasattr(p, "_obj"):                       # C.byref(x)
        return C.addressof(p._obj)
    if isinstance(p, C.c_void_p):
        return p.value or 0
    return C.cast(p, C.c_void_p).value or 0


def _in(p, nbytes, dtype=None):
    """what is read behind an input pointer: the bytes, or (``dtype``: taps and tables, computed with cos and sin) ``quant`` of the values"""
    a = _addr(p)
    if not a:
        return "NULL"
    data = C.string_at(a, nbytes)
    return f"{crc(data if dtype is None else quant(np.frombuffer(data, dtype)))}/{nbytes}"


def _out(p):
    return "out" if _addr(p) else "NULL"


def _put(p, arr):
    a = _addr(p)
    arr = np.ascontiguousarray(arr)
    if a and arr.nbytes:
        C.memmove(a, arr.ctypes.data, arr.nbytes)


def _put_rows(p, arr, pitch):
    """arr [rows][n] -> row r at element r * pitch"""
    a = _addr(p)
    arr = np.ascontiguousarray(arr)
    if a and arr.shape[1]:
        for r in range(arr.shape[0]):
            C.memmove(a + r * pitch * arr.itemsize, arr[r].ctypes.data, arr[r].nbytes)


def _set(p, v):
    if _addr(p):
        p._obj.value = v


class _Obj:
    def __init__(self, kind, **kw):
        self.kind = kind
        self.__dict__.update(kw)


class FakeLib:
    def __init__(self, real):
        self._real = real
        self.trace = []
        self._objs = {}
        self._next = 1
        self._calls = 0
        self._failed = False

    def __getattr__(self, name):
        if name.startswith("pysdr_") and name.endswith("_plan"):
            self._failed = False
            return getattr(self._real, name)
        raise AttributeError(f"the fake library has no {name}")

    def pysdr_strerror(self, rc):
        return self._real.pysdr_strerror(rc)

    def pysdr_last_error(self):
        """the real library's message after a plan call; the model's own -1 has a fixed one (the real one would be stale)"""
        return b"fake: no such object" if self._failed else self._real.pysdr_last_error()

    # ---- helpers
    def _rec(self, name, *args):
        self._calls += 1
        self.trace.append(" ".join([name] + [a if isinstance(a, str) else repr(a) for a in args]))
        return np.random.default_rng(self._calls)

    def note(self, text):
        self.trace.append("= " + text)

    def _get(self, h, *kinds):
        o = self._objs.get(_addr(h))
        return o if o is not None and o.kind in kinds else None

    def _h(self, h):
        return "h%d" % _addr(h) if _addr(h) else "NULL"

    def _new(self, ph, obj):
        if not _addr(ph):
            return -1
        obj.token = self._next
        self._next += 1
        self._objs[obj.token] = obj
        _set(ph, obj.token)
        return 0

    def _destroy(self, name, h, *kinds):
        self._rec(name, self._h(h))
        if self._get(h, *kinds) is not None:
            del self._objs[_addr(h)]

    @staticmethod
    def _advance(ch, n):
        n_out = -(-(ch.n_in + n) // ch.D) - -(-ch.n_in // ch.D)
        ch.n_in += n
        return n_out

    @staticmethod
    def _samples(rng, rows, n):
        return (rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n))).astype(np.complex64)

    # ---- channelizer, both kinds
    def pysdr_chan_create(self, device, M, D, k_first, nk, max_taps, max_in, ph):
        self._rec("pysdr_chan_create", device, M, D, k_first, nk, max_taps, max_in, _out(ph))
        return self._new(ph, _Obj("chan", D=D, nk=nk, n_in=0))

    def pysdr_chan_fine_create(self, device, M1, D1, M2, D2, k_first, nk, mt1, mt2, max_in, ph):
        self._rec("pysdr_chan_fine_create", device, M1, D1, M2, D2, k_first, nk, mt1, mt2, max_in, _out(ph))
        return self._new(ph, _Obj("chan", D=D1 * D2, nk=nk, n_in=0))

    def pysdr_chan_destroy(self, h):
        self._destroy("pysdr_chan_destroy", h, "chan")

    def pysdr_chan_set_taps(self, h, taps, n):
        self._rec("pysdr_chan_set_taps", self._h(h), _in(taps, 8 * n, np.float64), n)
        return 0 if self._get(h, "chan") else -1

    def pysdr_chan_fine_set_taps(self, h, t1, n1, t2, n2):
        self._rec("pysdr_chan_fine_set_taps", self._h(h), _in(t1, 8 * n1, np.float64), n1, _in(t2, 8 * n2, np.float64), n2)
        return 0 if self._get(h, "chan") else -1

    def pysdr_chan_reset(self, h):
        self._rec("pysdr_chan_reset", self._h(h))
        ch = self._get(h, "chan")
        if ch is None:
            return -1
        ch.n_in = 0
        return 0

    def pysdr_chan_sync(self, h):
        self._rec("pysdr_chan_sync", self._h(h))
        return 0 if self._get(h, "chan") else -1

    def pysdr_chan_process(self, h, x, n, in_dev, out, pitch, out_dev, pn):
        rng = self._rec("pysdr_chan_process", self._h(h), _addr(x) if in_dev else _in(x, 8 * n), n, in_dev,
                        _addr(out) if out_dev else _out(out), pitch, out_dev, _out(pn))
        ch = self._get(h, "chan")
        if ch is None:
            return -1
        n_out = self._advance(ch, n)
        if not out_dev:
            _put_rows(out, self._samples(rng, ch.nk, n_out), pitch)
        _set(pn, n_out)
        return 0

    # ---- bank
    def pysdr_bank_create(self, hc, fs_out, mode, ntaps, ph):
        self._rec("pysdr_bank_create", self._h(hc), fs_out, mode, ntaps, _out(ph))
        ch = self._get(hc, "chan")
        if ch is None:
            return -1
        return self._new(ph, _Obj("bank", chan=ch, last=0))

    def pysdr_bank_destroy(self, h):
        self._destroy("pysdr_bank_destroy", h, "bank")

    def pysdr_bank_set_mode(self, h, mode, af, n):
        self._rec("pysdr_bank_set_mode", self._h(h), mode, _in(af, 8 * n, np.float64), n)
        return 0 if self._get(h, "bank") else -1

    def pysdr_bank_set_mode_cplx(self, h, mode, re, im, n, bfo):
        self._rec("pysdr_bank_set_mode_cplx", self._h(h), mode, _in(re, 8 * n, np.float64), _in(im, 8 * n, np.float64), n, bfo)
        return 0 if self._get(h, "bank") else -1

    def pysdr_bank_set_agc(self, h, on, a):
        self._rec("pysdr_bank_set_agc", self._h(h), on, a)
        return 0 if self._get(h, "bank") else -1

    def pysdr_bank_set_squelch(self, h, t):
        self._rec("pysdr_bank_set_squelch", self._h(h), t)
        return 0 if self._get(h, "bank") else -1

    def pysdr_bank_reset(self, h):
        self._rec("pysdr_bank_reset", self._h(h))
        b = self._get(h, "bank")
        if b is None:
            return -1
        b.chan.n_in = b.last = 0
        return 0

    def pysdr_bank_sync(self, h):
        self._rec("pysdr_bank_sync", self._h(h))
        return 0 if self._get(h, "bank") else -1

    def pysdr_bank_process(self, h, x, n, in_dev, am, pitch, out_dev, pn):
        rng = self._rec("pysdr_bank_process", self._h(h), _addr(x) if in_dev else _in(x, 8 * n), n, in_dev, _out(am), pitch,
                        out_dev, _out(pn))
        b = self._get(h, "bank")
        if b is None:
            return -1
        b.last = self._advance(b.chan, n)
        _put_rows(am, rng.standard_normal((b.chan.nk, b.last)).astype(np.float32), pitch)
        _set(pn, b.last)
        return 0

    def pysdr_bank_state(self, h, agc, gain, maxbuf, level, op):
        rng = self._rec("pysdr_bank_state", self._h(h), _out(agc), _out(gain), _out(maxbuf), _out(level), _out(op))
        b = self._get(h, "bank")
        if b is None:
            return -1
        for p in (agc, gain, maxbuf, level):
            _put(p, rng.random(b.chan.nk, np.float32))
        _put(op, rng.integers(0, 2, b.chan.nk).astype(np.uint8))
        return 0

    def pysdr_bank_fetch(self, h, rows, nrows, am, iq, pitch):
        rng = self._rec("pysdr_bank_fetch", self._h(h), _in(rows, 4 * nrows), nrows, _out(am), _out(iq), pitch)
        b = self._get(h, "bank")
        if b is None:
            return -1
        _put_rows(am, rng.standard_normal((nrows, b.last)).astype(np.float32), pitch)
        _put_rows(iq, self._samples(rng, nrows, b.last), pitch)
        return 0

    # ---- decoder banks: CW (9 code bits, codes 1 .. 256) and PSK (11 code bits)
    def _dec_create(self, hc, ph, kind, rows_per_row, max_out, cap, bits, codes):
        ch = self._get(hc, "chan")
        if ch is None:
            return -1
        ch.n_in = 0
        nrows = ch.nk * rows_per_row
        return self._new(ph, _Obj(kind, chan=ch, nrows=nrows, max_out=max_out, cap=cap, bits=bits, codes=codes,
                                  slots=np.zeros((nrows, cap), np.int32)))

    def _dec_process(self, d, rng, n, pn, counts, ev, cap):
        n_out = self._advance(d.chan, n)
        assert n_out <= d.max_out and cap == d.cap, (n_out, d.max_out, cap, d.cap)
        cnt = rng.integers(0, min(cap, n_out) + 1, d.nrows) * (rng.random(d.nrows) < 0.5)
        d.slots = np.zeros((d.nrows, cap), np.int32)
        for r in np.flatnonzero(cnt):
            idx = np.sort(rng.integers(0, n_out, cnt[r]))
            d.slots[r, :cnt[r]] = (idx << d.bits) | rng.choice(d.codes, cnt[r])
        _set(pn, n_out)
        _put(counts, cnt.astype(np.int32))
        _put(ev, d.slots)

    def _dec_fetch(self, name, kind, h, rows, nrows, ev, cap):
        self._rec(name, self._h(h), _in(rows, 4 * nrows), nrows, _out(ev), cap)
        d = self._get(h, kind)
        if d is None or cap != d.cap:
            return -1
        r = np.frombuffer(C.string_at(_addr(rows), 4 * nrows), np.int32) if nrows else np.zeros(0, np.int32)
        if len(r) and (r.min() < 0 or r.max() >= d.nrows):
            return -1
        _put(ev, d.slots[r])
        return 0

    def _dec_simple(self, name, kind, h, reset):
        self._rec(name, self._h(h))
        d = self._get(h, kind)
        if d is None:
            return -1
        if reset:
            d.chan.n_in = 0
        return 0

    def pysdr_cw_create(self, hc, cfg, max_out, ph):
        self._rec("pysdr_cw_create", self._h(hc), _in(cfg, 44), max_out, _out(ph))
        return self._dec_create(hc, ph, "cw", 1, max_out, 2 * (max_out // 3 + 1), 9, np.array([1, 2, 5, 6, 13, 31, 256]))

    def pysdr_cw_destroy(self, h):
        self._destroy("pysdr_cw_destroy", h, "cw")

    def pysdr_cw_reset(self, h):
        return self._dec_simple("pysdr_cw_reset", "cw", h, True)

    def pysdr_cw_sync(self, h):
        return self._dec_simple("pysdr_cw_sync", "cw", h, False)

    def pysdr_cw_process(self, h, x, n, on_dev, pn, counts, ev, cap):
        rng = self._rec("pysdr_cw_process", self._h(h), _addr(x) if on_dev else _in(x, 8 * n), n, on_dev, _out(pn),
                        _out(counts), _out(ev), cap)
        d = self._get(h, "cw")
        if d is None:
            return -1
        self._dec_process(d, rng, n, pn, counts, ev, cap)
        return 0

    def pysdr_cw_fetch(self, h, rows, nrows, ev, cap):
        return self._dec_fetch("pysdr_cw_fetch", "cw", h, rows, nrows, ev, cap)

    def pysdr_cw_state(self, h, s, pk, nf, ints):
        rng = self._rec("pysdr_cw_state", self._h(h), _out(s), _out(pk), _out(nf), _out(ints))
        d = self._get(h, "cw")
        if d is None:
            return -1
        for p in (s, pk, nf):
            _put(p, rng.random(d.nrows, np.float32))
        _put(ints, rng.integers(0, 1000, (d.nrows, 8)).astype(np.int32))
        return 0

    def pysdr_psk_create(self, hc, S, cfg, tw, g, max_out, ph):
        self._rec("pysdr_psk_create", self._h(hc), S, _in(cfg, 28), _in(tw, 32 * S * 2 * 4, np.float32), _in(g, 2 * S * 4, np.float32), max_out, _out(ph))
        rc = self._dec_create(hc, ph, "psk", 4 * S, max_out, max_out // (3 * S // 2) + 1, 11, np.array([1, 3, 5, 0x2f, 0x3ff, 0x55]))
        if rc == 0:
            self._objs[self._next - 1].S = S
        return rc

    def pysdr_psk_destroy(self, h):
        self._destroy("pysdr_psk_destroy", h, "psk")

    def pysdr_psk_reset(self, h):
        return self._dec_simple("pysdr_psk_reset", "psk", h, True)

    def pysdr_psk_sync(self, h):
        return self._dec_simple("pysdr_psk_sync", "psk", h, False)

    def pysdr_psk_process(self, h, x, n, on_dev, pn, counts, ev, cap, qn, is_open):
        rng = self._rec("pysdr_psk_process", self._h(h), _addr(x) if on_dev else _in(x, 8 * n), n, on_dev, _out(pn),
                        _out(counts), _out(ev), cap, _out(qn), _out(is_open))
        d = self._get(h, "psk")
        if d is None:
            return -1
        self._dec_process(d, rng, n, pn, counts, ev, cap)
        _put(qn, rng.random(d.nrows, np.float32))
        _put(is_open, (rng.random(d.nrows) < 0.8).astype(np.int32))
        return 0

    def pysdr_psk_fetch(self, h, rows, nrows, ev, cap):
        return self._dec_fetch("pysdr_psk_fetch", "psk", h, rows, nrows, ev, cap)

    def pysdr_psk_state(self, h, e, f, ints):
        rng = self._rec("pysdr_psk_state", self._h(h), _out(e), _out(f), _out(ints))
        d = self._get(h, "psk")
        if d is None:
            return -1
        _put(e, rng.random((d.S, d.nrows), np.float32))
        _put(f, rng.random((4, d.nrows), np.float32))
        _put(ints, rng.integers(0, 1000, (5, d.nrows)).astype(np.int32))
        return 0


    # ---- FT8 / FT4 decoder banks (tests/test_ft_py_trace.py): the numbers of include/pysdr_hip.h, written out here
    FT = {"ft8": dict(lag=316, hold=321, nb_extra=14, pulse=3, sync=21), "ft4": dict(lag=412, hold=417, nb_extra=6, pulse=5, sync=16)}
    FT_MAX, FT_FRAMES, FT_ROWS, FT_WINDOW, FT_EVENTS = 4096, 256, 256, 256, 52

    @staticmethod
    def _ft_steps(n_out, S):
        """steps complete once a row has n_out outputs: step t needs outputs QS t .. QS t + S - 1, QS = S / 4"""
        return (n_out - S) // (S // 4) + 1 if n_out >= S else 0

    @staticmethod
    def _ft_done(d):
        return FakeLib._ft_steps(-(-d.chan.n_in // d.chan.D), d.S)

    @staticmethod
    def _ft_words(rng, u, sync):
        """events at the ascending step indices ``u`` -> [len(u)][2]: (u << 5) | hits, the bits of a positive float32 score"""
        hits = rng.integers(sync // 2, sync + 1, len(u))
        score = (3.0 + 9.0 * rng.random(len(u))).astype(np.float32)
        return np.stack(((np.asarray(u, np.int64) << 5) | hits, score.view(np.int32).astype(np.int64)), axis=1).astype(np.int32)

    def _ft_cands(self, d, F, t0, n, ring2=False):
        """-> the candidates' CRCs for the trace, and whether the call stands: n in [0, 4096], every F on the raster and (first
        ring) every frame whole, not before step 0 and still in the ring"""
        text = (_in(F, 4 * max(n, 0)), _in(t0, 8 * max(n, 0)), n)
        if d is None or not 0 <= n <= self.FT_MAX or (ring2 and not d.kept):
            return text, False
        f = np.frombuffer(C.string_at(_addr(F), 4 * n), np.int32) if n else np.zeros(0, np.int32)
        t = np.frombuffer(C.string_at(_addr(t0), 8 * n), np.int64) if n else np.zeros(0, np.int64)
        ok = not (len(f) and (f.min() < 0 or f.max() >= d.nfine))
        if ok and not ring2 and len(t):
            done = self._ft_done(d)
            ok = bool((t >= 0).all() and (t + d.lag - 4 < done).all() and (done - t <= d.tr).all())
        return text, ok

    def _ft_create(self, kind, hc, S, cfg, tw, max_out, ph):
        self._rec(f"pysdr_{kind}_create", self._h(hc), S, _in(cfg, 12), _in(tw, 4 * S * 2 * 4, np.float32), max_out, _out(ph))
        ch = self._get(hc, "chan")
        if ch is None:
            return -1
        ch.n_in = 0
        k, qs = self.FT[kind], S // 4
        cap = (max_out // qs + 1) // 5 + 1
        return self._new(ph, _Obj(kind, chan=ch, S=S, qs=qs, nsub=S // 2, nb=S // 2 + k["nb_extra"], nfine=ch.nk * (S // 2), max_out=max_out,
                                  cap=cap, lag=k["lag"], hold=k["hold"], sync=k["sync"], pulse=k["pulse"], tr=k["hold"] + 2 * (max_out // qs + 1),
                                  slots=np.zeros((ch.nk * (S // 2), 2 * cap), np.int32), kept=False, trials=0, tr2=0, ty=0))

    def _ft_destroy(self, kind, h):
        self._destroy(f"pysdr_{kind}_destroy", h, kind)

    def _ft_reset(self, kind, h):
        return self._dec_simple(f"pysdr_{kind}_reset", kind, h, True)

    def _ft_sync(self, kind, h):
        return self._dec_simple(f"pysdr_{kind}_sync", kind, h, False)

    def _ft_process(self, kind, h, x, n, on_dev, pn, counts, ev, pitch, steps):
        rng = self._rec(f"pysdr_{kind}_process", self._h(h), _addr(x) if on_dev else _in(x, 8 * n), n, on_dev, _out(pn), _out(counts),
                        _out(ev), pitch, _out(steps))
        d = self._get(h, kind)
        if d is None or pitch < 2 * d.cap:
            return -1
        t_first = self._ft_done(d)
        n_out = self._advance(d.chan, n)
        assert n_out <= d.max_out, (n_out, d.max_out)
        ns = self._ft_done(d) - t_first
        first = max(0, d.lag - t_first)                                 # only events with t_first + u - lag >= 0, as the device does
        most = min(d.cap, max(ns - first, 0))
        cnt = rng.integers(0, most + 1, d.nfine) * (rng.random(d.nfine) < 1.0 / d.nfine)
        d.slots = np.zeros((d.nfine, 2 * d.cap), np.int32)
        for r in np.flatnonzero(cnt):
            u = np.sort(rng.choice(np.arange(first, ns), cnt[r], replace=False))
            d.slots[r, :2 * cnt[r]] = self._ft_words(rng, u, d.sync).reshape(-1)
        _set(pn, n_out)
        _put(counts, cnt.astype(np.int32))
        _put_rows(ev, d.slots, pitch)
        _put(steps, np.array([t_first, ns], np.int64))
        return 0

    def _ft_fetch(self, kind, h, rows, nrows, ev, pitch):
        self._rec(f"pysdr_{kind}_fetch", self._h(h), _in(rows, 4 * nrows), nrows, _out(ev), pitch)
        d = self._get(h, kind)
        if d is None or pitch < 2 * d.cap:
            return -1
        r = np.frombuffer(C.string_at(_addr(rows), 4 * nrows), np.int32) if nrows else np.zeros(0, np.int32)
        if len(r) and (r.min() < 0 or r.max() >= d.nfine):
            return -1
        _put_rows(ev, d.slots[r], pitch)
        return 0

    def _ft_state(self, kind, h, sc, hits, ring, done):
        rng = self._rec(f"pysdr_{kind}_state", self._h(h), _out(sc), _out(hits), _out(ring), _out(done))
        d = self._get(h, kind)
        if d is None:
            return -1
        _put(sc, rng.random((9, d.nfine), np.float32))
        _put(hits, rng.integers(0, d.sync + 1, (9, d.nfine)).astype(np.int32))
        _put(ring, rng.random((d.chan.nk, d.tr, d.nb), np.float32))
        _set(done, self._ft_done(d))
        return 0

    def _ft_llr(self, kind, h, F, t0, n, out, what="llr"):
        d = self._get(h, kind)
        text, ok = self._ft_cands(d, F, t0, n, what == "pass_llr")
        rng = self._rec(f"pysdr_{kind}_{what}", self._h(h), *text, _out(out))
        if not ok:
            return -1
        _put(out, rng.standard_normal((n, 174)).astype(np.float32))
        return 0

    def _ft_pass_llr(self, kind, h, F, t0, n, out):
        return self._ft_llr(kind, h, F, t0, n, out, "pass_llr")

    def _ft_answer(self, rng, n, st, bits, post, osd, detail):
        """what the four decode calls and pass_decode write: status 2 in about half the rows, 0 and 1 in a quarter each; the
        second stage, where asked for, runs on the rows without a message and decodes half of them"""
        s = np.zeros((n, 4), np.int32)
        s[:, 0] = rng.choice([0, 1, 2, 2], n)
        s[:, 1] = rng.integers(0, 30, n)
        s[:, 2] = rng.integers(0, 40, n)
        b = rng.integers(0, 256, (n, 12)).astype(np.uint8)
        b[:, 11] &= 0xE0                                                 # 91 bits, MSB first: the last 5 are padding
        det = np.tile(np.array([-1, -1, -1, 0], np.int32), (n, 1))
        if osd:
            ran = s[:, 0] != 2
            s[ran, 3] = rng.integers(1, 4, int(ran.sum()))
            s[ran & (rng.random(n) < 0.5), 0] = 2
            det[ran] = rng.integers(0, 4187, (int(ran.sum()), 4))
        _put(st, s)
        _put(bits, b)
        _put(post, rng.standard_normal((n, 174)).astype(np.float32))
        _put(detail, det)

    def _ft_decode(self, kind, h, F, t0, n, cfg, st, bits, post, osd=None, detail=None, what="decode"):
        d = self._get(h, kind)
        text, ok = self._ft_cands(d, F, t0, n, what == "pass_decode")
        more = () if what == "decode" else (_in(osd, 4), _out(detail))
        rng = self._rec(f"pysdr_{kind}_{what}", self._h(h), *text, _in(cfg, 8), _out(st), _out(bits), _out(post), *more)
        if not ok or not _addr(cfg) or not _addr(st) or not _addr(bits) or (what == "decode_osd" and not _addr(osd)) or (_addr(detail) and not _addr(osd)):
            return -1
        self._ft_answer(rng, n, st, bits, post, _addr(osd), detail)
        return 0

    def _ft_decode_osd(self, kind, h, F, t0, n, cfg, st, bits, post, osd, detail):
        return self._ft_decode(kind, h, F, t0, n, cfg, st, bits, post, osd, detail, "decode_osd")

    def _ft_pass_decode(self, kind, h, F, t0, n, cfg, st, bits, post, osd, detail):
        return self._ft_decode(kind, h, F, t0, n, cfg, st, bits, post, osd, detail, "pass_decode")

    def _ft_decode_llr(self, kind, h, llr, n, cfg, st, bits, post, osd=None, detail=None, what="decode_llr"):
        more = () if what == "decode_llr" else (_in(osd, 4), _out(detail))
        rng = self._rec(f"pysdr_{kind}_{what}", self._h(h), _in(llr, 174 * 4 * max(n, 0)), n, _in(cfg, 8), _out(st), _out(bits), _out(post), *more)
        if self._get(h, kind) is None or not 0 <= n <= self.FT_MAX or (what != "decode_llr" and not _addr(osd)):
            return -1
        if n and not np.isfinite(np.frombuffer(C.string_at(_addr(llr), 174 * 4 * n), np.float32)).all():
            return -1
        self._ft_answer(rng, n, st, bits, post, _addr(osd), detail)
        return 0

    def _ft_decode_llr_osd(self, kind, h, llr, n, cfg, st, bits, post, osd, detail):
        return self._ft_decode_llr(kind, h, llr, n, cfg, st, bits, post, osd, detail, "decode_llr_osd")

    def _ft_report(self, kind, h, F, t0, bits, n, power, errs):
        d = self._get(h, kind)
        text, ok = self._ft_cands(d, F, t0, n)
        rng = self._rec(f"pysdr_{kind}_report", self._h(h), text[0], text[1], _in(bits, 12 * max(n, 0)), n, _out(power), _out(errs))
        if not ok:
            return -1
        _put(power, (0.5 + rng.random((n, 10))).astype(np.float32) * np.float32(100.0))
        _put(errs, rng.integers(0, 8, (n, 2)).astype(np.int32))
        return 0

    def _ft_floor(self, kind, h, t_end, nsym, out):
        t_end = t_end.value if hasattr(t_end, "value") else t_end
        rng = self._rec(f"pysdr_{kind}_floor", self._h(h), t_end, nsym, _out(out))
        d = self._get(h, kind)
        if d is None or not 1 <= nsym <= 128:
            return -1
        done, t_lo = self._ft_done(d), t_end - 4 * (nsym - 1)
        if t_end >= done or t_lo < 0 or done - t_lo > d.tr:
            return -1
        _put(out, (0.5 + rng.random((d.chan.nk, d.nb))).astype(np.float32))
        return 0

    def _ft_keep(self, kind, h, cfg):
        c = cfg._obj if _addr(cfg) else None
        d = self._get(h, kind)
        size = d.pulse * d.S if d is not None else 0
        self._rec(f"pysdr_{kind}_keep", self._h(h), "NULL" if c is None else
                  f"reach_t={c.reach_t} trials={c.trials} pulse={crc((np.frombuffer(C.string_at(_addr(c.pulse), 4 * size), np.uint32) >> 8).tobytes())}/{4 * size} "
                  f"lut={_in(c.lut, 4096 * 2 * 4, np.float32)}")
        if d is None or c is None or d.chan.n_in > 0 or not 1 <= c.reach_t <= 120 or not 1 <= c.trials <= 9:
            return -1
        d.kept, d.trials = True, c.trials
        d.tr2 = d.hold + 2 * c.reach_t + 4 + d.max_out // d.qs + 1
        d.ty = -(-(d.qs * d.tr2 + d.S) // 16) * 16
        return 0

    def _ft_subtract(self, kind, h, F, t0, bits, trials, n, out):
        d = self._get(h, kind)
        nt = d.trials if d is not None else 0
        rng = self._rec(f"pysdr_{kind}_subtract", self._h(h), _in(F, 4 * max(n, 0)), _in(t0, 8 * max(n, 0)), _in(bits, 12 * max(n, 0)),
                        _in(trials, 8 * nt * max(n, 0)), n, _out(out))
        if d is None or not d.kept or not 0 <= n <= self.FT_FRAMES:
            return -1
        o = np.zeros((n, 2, 4), np.int32)
        o[:, :, :2] = (1.0 + rng.random((n, 2, 2))).astype(np.float32).view(np.int32)
        o[:, :, 2] = rng.integers(0, d.trials, (n, 2))
        o[:, :, 3] = rng.integers(1, 80, (n, 2))
        _put(out, o)
        return 0

    def _ft_rescan(self, kind, h, F_lo, F_hi, t_lo, t_hi, cfg, counts, ev):
        t_lo, t_hi = (t.value if hasattr(t, "value") else t for t in (t_lo, t_hi))
        rng = self._rec(f"pysdr_{kind}_rescan", self._h(h), F_lo, F_hi, t_lo, t_hi, _in(cfg, 12), _out(counts), _out(ev))
        d = self._get(h, kind)
        nF, nT = F_hi - F_lo + 1, t_hi - t_lo + 1
        if d is None or not d.kept or not 1 <= nF <= self.FT_ROWS or not 1 <= nT + 8 <= self.FT_WINDOW or F_lo < 0 or F_hi >= d.nfine or t_lo < 0:
            return -1
        cnt = rng.integers(1, min(3, nT, self.FT_EVENTS) + 1, nF) * (rng.random(nF) < 0.2)     # a few events in a few rows
        words = np.zeros((nF, self.FT_EVENTS, 2), np.int32)
        for r in np.flatnonzero(cnt):
            words[r, :cnt[r]] = self._ft_words(rng, np.sort(rng.choice(nT, cnt[r], replace=False)), d.sync)
        _put(counts, cnt.astype(np.int32))
        _put(ev, words)
        return 0

    def _ft_pass_state(self, kind, h, yk, ring2, info):
        rng = self._rec(f"pysdr_{kind}_pass_state", self._h(h), _out(yk), _out(ring2), _out(info))
        d = self._get(h, kind)
        if d is None or not d.kept:
            return -1
        _put(yk, self._samples(rng, d.chan.nk, d.ty))
        _put(ring2, rng.random((d.chan.nk, d.tr2, d.nb), np.float32))
        _put(info, np.array([-(-d.chan.n_in // d.chan.D), d.ty, d.tr2], np.int64))
        return 0


def _for_kind(fn, kind):
    def call(self, *a):
        return fn(self, kind, *a)
    return call


for _name, _fn in list(vars(FakeLib).items()):
    if _name.startswith("_ft_") and _name not in ("_ft_steps", "_ft_done", "_ft_words", "_ft_cands", "_ft_answer"):
        for _kind in FakeLib.FT:
            setattr(FakeLib, f"pysdr_{_kind}_{_name[4:]}", _for_kind(_fn, _kind))


def _noting_failure(fn):
    def call(self, *a):
        rc = fn(self, *a)
        self._failed = rc == -1
        if self._failed:
            self.trace[-1] += " -> -1"
        return rc
    return call


for _name, _fn in list(vars(FakeLib).items()):
    if _name.startswith("pysdr_") and _name not in ("pysdr_strerror", "pysdr_last_error"):
        setattr(FakeLib, _name, _noting_failure(_fn))
