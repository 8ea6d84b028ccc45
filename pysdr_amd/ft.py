"""What the FT8 and the FT4 skimmer share on the host (kernels ``ft.hip``, host half
``api_ft.hip``): the helpers that read a mode, the finder, and the decoder bank and the skimmer as classes that read
everything a mode differs in from ``MODE``, a mode's module (``ft8.py``, ``ft4.py``): NAME, BAUD, SHAPES, PLAN_CALL, the frame's
constants, ``params``, ``plan``, ``shape`` and ``prototype``.  The frame report's host maths is ``ft_report.py``, the second
pass's tables and policy ``ft_pass.py``.  The tables and settings are derived here, once, and handed to the library already
derived."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import channelizer as _chan
from . import ft8msg as _msg
from . import ft_pass as _pass
from . import ldpc as _ldpc
from .channelizer import Channelizer
from .ft_report import REPORT_MAX, noise_of, refine, snr_db
from .skimmer import DecoderBank, Skimmer

LLR_MAX = 4096                                   # candidates of one llr or decode call
KEEP = 9                                         # frame starts whose score the device keeps
_p32, _p64, _pu8 = C.POINTER(C.c_int32), C.POINTER(C.c_longlong), C.POINTER(C.c_uint8)


# ---- reading a mode ---------------------------------------------------------------------------------------------------------
def mode_shape(mode, fs):
    """``shape`` for ``mode``"""
    for S in mode.SHAPES:
        d = float(fs) / (S * mode.BAUD)
        D = int(round(d))
        if D < 1 or abs(d - D) > 1e-9 * max(d, 1.0):
            continue
        try:
            _chan.plan(4 * D, D, 16 * D)
        except _lib.PysdrError:
            continue
        return S, D, 4 * D
    r0, r1 = (f"{S * mode.BAUD:g}" for S in mode.SHAPES)
    raise ValueError(f"no {mode.NAME} raster for fs = {fs}: fs / {r0} or fs / {r1} must be an integer D with M = 4 D a channelizer size")


def mode_fine_channelizer(mode, fs, band, device=0, max_in=1 << 22):
    """``fine_channelizer`` for ``mode``"""
    from . import fine
    err = None
    for S in mode.SHAPES:
        try:
            M1, D1, M2, D2 = fine.shape(fs, S * mode.BAUD, 4)
        except ValueError as e:
            err = e
            continue
        h2 = mode.prototype(float(fs) / D1, M2, S)
        return fine.FineChannelizer(fs, M1, M2, D1, D2, fine.prototype1(fs, M1, D1, M2), h2,
                                    fine.channels_for(band, fs, M1, D1, M2), device, max_in)
    raise ValueError(f"no {mode.NAME} raster in two stages for fs = {fs}: {err}")


def mode_plan(mode, nk, S, max_out, cfg):
    """``plan`` for ``mode``"""
    v = _lib.plan_call(mode.PLAN_CALL, 8, int(nk), int(S), int(max_out), C.byref(cfg) if cfg is not None else None)
    return {"rows": v[0], "threads": v[1], "lds_bytes": v[2], "tile": v[3], "cap": v[4], "groups": v[5], "nsub": v[6], "tr": v[7]}


def tables(S):
    """-> tw float32 [4 S][2] = (cos, -sin)(2 pi i / NT): derived in float64, rounded once"""
    t = 2 * np.pi * np.arange(4 * S) / (4 * S)
    return np.ascontiguousarray(np.stack((np.cos(t), -np.sin(t)), axis=1), np.float32)


def cfg_dict(cfg):
    return {k: getattr(cfg, k) for k, _ in type(cfg)._fields_}


def steps_done(n_out, S):
    """steps complete once a row has n_out outputs: step t needs outputs QS t .. QS t + S - 1"""
    return (int(n_out) - S) // (S // 4) + 1 if n_out >= S else 0


# ---- events and soft bits ---------------------------------------------------------------------------------------------------
def unpack(words):
    """the two event words -> (index within the call of the emitting step, hits, score)"""
    w = int(words[0]) & 0xFFFFFFFF
    return w >> 5, w & 31, float(np.array([int(words[1]) & 0xFFFFFFFF], np.uint32).view(np.float32)[0])


def row_events(words, count):
    """a fine row's event words, two an event, and how many of them are events -> [(index, hits, score)]"""
    return [unpack(words[2 * i:2 * i + 2]) for i in range(int(count))]


def owners(events, reach_f=2, reach_t=4, nfine=None):
    """The finder.  ``events``: sequence of (t0, F, score, ...).  An event owns itself unless another event within
    ``reach_t`` steps and ``reach_f`` fine rows has a greater score; ties go to the lower (t0, F).  With ``nfine`` (the
    raster covers the whole circle, nk == M) the distance in F is circular.  -> bool [len(events)]"""
    n = len(events)
    own = np.ones(n, bool)
    if n < 2:
        return own
    t = np.array([e[0] for e in events], np.int64)
    F = np.array([e[1] for e in events], np.int64)
    s = np.array([e[2] for e in events], np.float64)
    order = np.argsort(t, kind="stable")
    lo = np.searchsorted(t[order], t - reach_t, "left")
    hi = np.searchsorted(t[order], t + reach_t, "right")
    for i in range(n):
        for k in order[lo[i]:hi[i]]:
            if k == i:
                continue
            d = abs(int(F[k] - F[i]))
            if nfine is not None:
                d = min(d, nfine - d)
            if d > reach_f:
                continue
            if s[k] > s[i] or (s[k] == s[i] and (t[k], F[k]) < (t[i], F[i])):
                own[i] = False
                break
    return own


def unit_llr(llr):
    """soft bits scaled to unit variance (what a decoder's channel model expects); zeros stay zeros"""
    llr = np.asarray(llr, np.float32)
    sd = float(np.std(llr.astype(np.float64)))
    return llr if sd == 0 else (llr / np.float32(sd)).astype(np.float32)


def hard_bits(llr):
    return (np.asarray(llr) > 0).astype(np.uint8)


# ---- what the bank's calls share --------------------------------------------------------------------------------------------
def _cands(F, t0):
    """candidates as the C ABI takes them -> F int32, t0 int64 and ``at(s)``: the two pointers for the candidates ``s``"""
    F, t0 = np.ascontiguousarray(F, np.int32), np.ascontiguousarray(t0, np.int64)
    return F, t0, lambda s=slice(None): (F[s].ctypes.data_as(_p32), t0[s].ctypes.data_as(_p64))


def _calls(n, size):
    """the slices that cut ``n`` candidates into calls of at most ``size``"""
    return [slice(i, min(i + size, n)) for i in range(0, n, size)]


class FT_Decoders(DecoderBank):
    """The decoder bank on a borrowed ``Channelizer`` (which it resets, and which must be fed only through it).  A mode
    file names KIND, DESTROY and MODE."""
    MODE = None                                                          # the mode's constants, settings, plan and tables

    def __init__(self, chan, S, max_out=256, cfg=None):
        super().__init__(chan, max_out)
        self.S, self.nsub, self.nb, self.qs = int(S), int(S) // 2, int(S) // 2 + self.MODE.NB_EXTRA, int(S) // 4
        self.nfine = self.nk * self.nsub
        self.cfg = self.MODE.params() if cfg is None else cfg
        self.plan = self.MODE.plan(self.nk, self.S, self.max_out, self.cfg)         # a bad shape fails here
        self.tr = self.plan["tr"]
        self.tw = self.MODE.tables(self.S)
        self._open(self.nfine, self.S, C.byref(self.cfg), _lib.as_pf(self.tw))
        self.slots = self.cap                                             # events per fine row and call
        self.cap = 2 * self.slots                                         # int32 words per fine row: what fetch and process move
        self.t_done = 0

    def reset(self):
        super().reset()
        self.t_done = 0

    def decode_raw(self, x, n=None, on_device=False, events="all"):
        """One call of the C ABI: host samples (complex64 [n]) or a device pointer.  -> dict of n_out, m0, counts [nfine]
        and events [nfine][2 slots] int32 words (``DecoderBank._decode``'s rules), and t_first, n_steps: the steps complete
        before the call and those it completed.  An event's t0 is ``t_first + unpack(words)[0] - EMIT_LAG``."""
        steps = (C.c_longlong * 2)()
        r = self._decode(x, n, on_device, events, steps)
        self.t_done = steps[0] + steps[1]
        return dict(r, t_first=int(steps[0]), n_steps=int(steps[1]))

    def events_of(self, r, rows=None, words=None):
        """the events of a call as (t0, F, score, hits), from ``decode_raw``'s answer (events="all") or from fetched rows"""
        if rows is None:
            rows, words = np.flatnonzero(r["counts"]), r["events"][np.flatnonzero(r["counts"])]
        first = r["t_first"] - self.MODE.EMIT_LAG
        return [(first + u, int(F), score, hits) for k, F in enumerate(rows) for u, hits, score in row_events(words[k], r["counts"][F])]

    def llr(self, F, t0):
        """float32 [n][174]: the soft bits of the candidates (F[i], t0[i]); PysdrError for a frame that is not complete yet
        or has left the ring, or an F outside the raster"""
        F, t0, at = _cands(F, t0)
        out = np.zeros((len(F), self.MODE.BITS), np.float32)
        for s in _calls(len(F), LLR_MAX):
            self._call("llr", *at(s), s.stop - s.start, _lib.as_pf(out[s]))
        return out

    def _decoder(self, what, n, head, cfg, post, osd, detail, residual=False):
        """``decode`` and ``decode_llr``: the LDPC decoder in calls of 4096 of ``what``, or of ``what + "_osd"`` with a second
        stage (``residual``: ``what`` takes the stage's arguments either way); ``head(s)``: the inputs of the candidates ``s``"""
        cfg = _ldpc.params() if cfg is None else cfg
        osd = _ldpc.osd_cfg(osd)
        if osd is None and detail:
            raise ValueError("detail is the second stage's: it needs osd")
        st, bits = np.zeros((n, 4), np.int32), np.zeros((n, 12), np.uint8)
        po = np.zeros((n, self.MODE.BITS), np.float32) if post else None
        de = np.zeros((n, 4), np.int32) if detail else None
        if residual:
            self._need_kept()
        for s in _calls(n, LLR_MAX):
            args = head(s) + (s.stop - s.start, C.byref(cfg), st[s].ctypes.data_as(_p32), bits[s].ctypes.data_as(_pu8),
                              None if po is None else _lib.as_pf(po[s]))
            if residual or osd is not None:
                args += (None if osd is None else C.byref(osd), None if de is None else de[s].ctypes.data_as(_p32))
            self._call(what if residual or osd is None else what + "_osd", *args)
        out = dict(status=st[:, 0].copy(), iterations=st[:, 1].copy(), nerr=st[:, 2].copy(), bits=_ldpc.unpack_bits(bits))
        for key, v in (("post", po), ("osd", None if osd is None else st[:, 3].copy()), ("detail", de)):
            if v is not None:                                             # only what was asked for
                out[key] = v
        return out

    def decode(self, F, t0, cfg=None, post=False, osd=None, detail=False, residual=False):
        """The candidates (F[i], t0[i]) of ``llr``, under its rules, through the LDPC decoder on the device, straight from
        the spectrum ring (``cfg``: ``ldpc.params()``).  -> dict of status int32 [n] (2: a codeword with
        a good CRC and a message that is not all zero, 1: any other codeword, 0: none), iterations, nerr (hard bits the
        decoder changed), bits uint8 [n][91] (the message's 77 and the CRC's 14, whatever the status) and, with ``post``,
        post float32 [n][174], the decoder's final sums.  With ``osd`` (an order 0 to 2 or ``ldpc.osd_params()``) the
        candidates min-sum left without a message go through ordered-statistics decoding in a second launch (DESIGN.md 3
        item 25) and the answer gains osd int32 [n] (0: the stage did not run; 1, 2, 3: it did and no, one or two rows of
        the basis were flipped) and, with ``detail``, detail int32 [n][4] (k, last, weight, the distance's bits).
        ``residual``: from the second pass's residue (``keep``) instead of the spectrum ring."""
        F, t0, at = _cands(F, t0)
        return self._decoder("pass_decode" if residual else "decode", len(F), at, cfg, post, osd, detail, residual)

    def decode_llr(self, llr, cfg=None, post=False, osd=None, detail=False):
        """Soft bits from the host, float32 [n][174], positive for bit 1, any scale -> ``decode``'s answer.  In calls of
        4096; a value that is not finite is refused."""
        llr = np.ascontiguousarray(llr, np.float32).reshape(-1, self.MODE.BITS)
        return self._decoder("decode_llr", len(llr), lambda s: (_lib.as_pf(llr[s]),), cfg, post, osd, detail)

    def report(self, F, t0, bits91):
        """The candidates (F[i], t0[i]) of ``llr``, under its rules, with the 91 bits of each as ``decode`` returns them
        (uint8 [n][91]; the CRC is not checked) -> dict of sig9 float32 [n][3][3] (the sum of the frame's sent tones at
        t0 - 1, t0, t0 + 1 outer and F - 1, F, F + 1 inner; -1 where a place is outside the raster or the ring), tot float32
        [n] (all tones at the candidate's own place), nhard and nsync int32 [n] (data and Costas symbols whose sent tone is
        not the strongest).  DESIGN.md 3 item 26; in calls of 4096."""
        F, t0, at = _cands(F, t0)
        packed = _pass.pack91(bits91, len(F))
        power = np.zeros((len(F), 10), np.float32)
        errs = np.zeros((len(F), 2), np.int32)
        for s in _calls(len(F), REPORT_MAX):
            self._call("report", *at(s), packed[s].ctypes.data_as(_pu8), s.stop - s.start, _lib.as_pf(power[s]), errs[s].ctypes.data_as(_p32))
        return dict(sig9=power[:, :9].reshape(-1, 3, 3).copy(), tot=power[:, 9].copy(), nhard=errs[:, 0].copy(), nsync=errs[:, 1].copy())

    def floor(self, t_end=None, nsym=None):
        """float32 [nk][NB]: every bin of every row summed over the ``nsym`` steps, four apart, that end at step ``t_end``
        (defaults: the newest complete step, the mode's symbol count); PysdrError unless 1 <= nsym <= 128 and every one of
        those steps is complete and still in the ring."""
        t_end = self.t_done - 1 if t_end is None else int(t_end)
        nsym = self.MODE.SYMBOLS if nsym is None else int(nsym)
        out = np.zeros((self.nk, self.nb), np.float32)
        self._call("floor", C.c_longlong(t_end), nsym, _lib.as_pf(out))
        return out

    # ---- the second pass ---------------------------------------------------------------------------
    kept = None                                                          # ``keep``'s plan once it was called

    def keep(self, reach_t=None, trials=_pass.PASS_TRIALS):
        """From now on -- allowed only before the stream begins, after create or ``reset`` -- every call also keeps its
        row samples and a second spectrum ring for ``subtract``, ``rescan`` and ``decode(residual=True)``.  ``reach_t``:
        steps a rescan will look to either side of a subtracted frame (default the mode's ``REACH_T``); ``trials``: the
        (dn, fw) pairs every frame of a ``subtract`` call carries.  -> the plan (``pass_plan``)."""
        m = self.MODE
        reach_t = m.REACH_T if reach_t is None else int(reach_t)
        plan = _pass.pass_plan(m, self.nk, self.S, self.max_out, reach_t)  # a bad reach_t fails here
        self._pulse, self._lut = _pass.pass_pulse(m, self.S), _pass.pass_lut()
        cfg = _lib.PassCfg(reach_t=reach_t, trials=int(trials), pulse=self._pulse.ctypes.data_as(C.POINTER(C.c_uint32)), lut=_lib.as_pf(self._lut))
        self._call("keep", C.byref(cfg))
        self.kept = dict(plan, reach_t=reach_t, trials=int(trials))
        return self.kept

    def _need_kept(self):
        if self.kept is None:
            raise _lib.PysdrError(f"{type(self).__name__}: nothing is kept for a second pass: call keep() first")

    def subtract(self, F, t0, bits91, trials):
        """Take the frames (F[i], t0[i]) with the 91 bits of each out of the kept row samples and recompute the steps they
        touch in the residue.  ``trials`` int32 [n][kept trials][2] = (dn, fw) (``trial_grid``).  -> dict of before, after
        float32 [n][2] (power of the frame's symbols in its own row and in the neighbour that holds some of its tones, 0
        where there is none), trial and used int32 [n][2].  At most 256 frames, in one call; PysdrError for a frame whose
        steps t0 - 4 .. t0 + lag + 4 are not all complete and held."""
        self._need_kept()
        F, t0, at = _cands(F, t0)
        packed = _pass.pack91(bits91, len(F))
        tr = np.ascontiguousarray(trials, np.int32).reshape(len(F), self.kept["trials"], 2)
        out = np.zeros((len(F), 2, 4), np.int32)
        self._call("subtract", *at(), packed.ctypes.data_as(_pu8), tr.ctypes.data_as(_p32), len(F), out.ctypes.data_as(_p32))
        pw = np.ascontiguousarray(out[:, :, :2]).view(np.float32)
        return dict(before=pw[:, :, 0].copy(), after=pw[:, :, 1].copy(), trial=out[:, :, 2].copy(), used=out[:, :, 3].copy())

    def rescan(self, F_lo, F_hi, t_lo, t_hi, cfg=None):
        """The sync score of the fine rows F_lo .. F_hi of the residue at the start steps t_lo - 4 .. t_hi + 4, judged at
        t_lo .. t_hi by the streaming peak rule under ``cfg`` (default the bank's) -> events (t0, F, score, hits) sorted by
        (F, t0).  At most 256 fine rows and 256 start steps."""
        self._need_kept()
        cfg = self.cfg if cfg is None else cfg
        nF = int(F_hi) - int(F_lo) + 1
        counts = np.zeros(max(nF, 1), np.int32)
        ev = np.zeros((max(nF, 1), 2 * _pass.PASS_EVENT_CAP), np.int32)
        self._call("rescan", int(F_lo), int(F_hi), C.c_longlong(int(t_lo)), C.c_longlong(int(t_hi)), C.byref(cfg), counts.ctypes.data_as(_p32),
                   ev.ctypes.data_as(_p32))
        return [(int(t_lo) + u, int(F_lo) + int(k), score, hits) for k in np.flatnonzero(counts[:nF]) for u, hits, score in row_events(ev[k], counts[k])]

    def pass_llr(self, F, t0):
        """``llr`` from the residue, in one call"""
        self._need_kept()
        F, t0, at = _cands(F, t0)
        out = np.zeros((len(F), self.MODE.BITS), np.float32)
        self._call("pass_llr", *at(), len(F), _lib.as_pf(out))
        return out

    def pass_state(self):
        """dict of yk complex64 [nk][TY] (row sample n at n mod TY), ring2 float32 [nk][TR2][NB] (step t at t mod TR2) and
        n_kept, the row samples since create / reset"""
        self._need_kept()
        yk = np.empty((self.nk, self.kept["ty"]), np.complex64)
        r2 = np.empty((self.nk, self.kept["tr2"], self.nb), np.float32)
        info = (C.c_longlong * 3)()
        self._call("pass_state", yk.ctypes.data_as(C.POINTER(C.c_float)), _lib.as_pf(r2), info)
        return dict(yk=yk, ring2=r2, n_kept=int(info[0]))

    def state(self, ring=False):
        """dict of sc float32 [9][nfine] and hits int32 [9][nfine] (frame start t at index t mod 9), t_done, and with
        ``ring`` the spectrum ring float32 [nk][TR][NB] (step t at index t mod TR)"""
        sc = np.empty((KEEP, self.nfine), np.float32)
        hits = np.empty((KEEP, self.nfine), np.int32)
        rg = np.empty((self.nk, self.tr, self.nb), np.float32) if ring else None
        done = C.c_longlong(0)
        self._call("state", _lib.as_pf(sc), hits.ctypes.data_as(_p32), None if rg is None else _lib.as_pf(rg), C.byref(done))
        return dict(sc=sc, hits=hits, t_done=int(done.value), **({"ring": rg} if ring else {}))


class FT_Skimmer(Skimmer):
    """Wideband IQ at ``fs`` -> a channelizer of M = 4 D rows S baud / 4 apart at S baud samples per second -> NSUB = S / 2
    sync decoders inside every row, fine row F with tone 0 at ``freqs_fine[F]`` Hz (signed) -> a record for every frame
    found: ``t0`` (steps of a quarter symbol since create / reset), ``F``, ``freq``, ``time`` (seconds into the stream),
    ``score``, ``hits`` and ``llr`` float32 [174]; with ``t_first`` (UTC seconds of sample 0) also ``slot`` and ``dt``.
    With ``decode=True`` the owners go through the LDPC decoder on the device (``ldpc``: ``ldpc.params()``) and a record
    gains ``status``, ``ok`` (status 2), ``iterations``, ``nerr``, ``bits77``, ``i3``, ``n3`` and ``text`` (None where the
    frame did not decode or its message type is not unpacked); ``keep_llr=False`` then skips the soft bits' download and
    the records carry no ``llr``.  ``passes=2`` (with ``decode=True``; ``reach_t`` steps, default the mode's ``REACH_T``) takes
    every decoded frame out of the kept row samples once it is due and searches the residue around it again
    (``ft_pass.SecondPass``): every record then carries ``pass``, 1 or 2, and a record of pass 2 is a
    frame found under a stronger one (its ``llr`` is the residue's); ``report=True`` is refused with it, for the report
    reads the first ring.  ``osd=2`` (an order 0 to 2, or ``ldpc.osd_params()``) sends the frames min-sum could not
    decode through ordered-statistics decoding and a record gains ``osd``: 0, the stage did not
    run; 1, 2, 3, it did.  Off by default: the CRC-14 is that stage's only guard, and a frame that reaches it comes out as
    a false message with probability about 2^-14.  ``report=True`` measures every decoded frame in the spectrum ring
    (DESIGN.md 3 item 26): one row-floor call per release and one report call for the records with ``ok``, which gain
    ``snr`` (dB in 2500 Hz), ``f_fine`` (Hz), ``t_fine`` (s), ``nhard``, ``nsync``, ``sig`` and ``noise`` (the mean power of
    the sent tones at the refined peak and the noise power per bin) and, with ``t_first``, ``dt_fine``; the other records
    carry the same keys as None.  ``spots`` then keeps one record per message and ``spot_line`` formats it.  A mode file
    names DECODERS."""

    DECODERS = None                                                      # the bank; its MODE is the skimmer's too
    REPORT_KEYS = ("snr", "f_fine", "t_fine", "nhard", "nsync", "sig", "noise")

    def __init__(self, fs, channels=None, device=0, max_in=1 << 22, max_out=256, chan=None, t_first=None, decode=False, ldpc=None,
                 keep_llr=True, osd=None, report=False, passes=1, reach_t=None):
        m = self.DECODERS.MODE
        self.passes = int(passes)
        if self.passes not in (1, 2):
            raise ValueError(f"{type(self).__name__}: passes is 1 or 2")
        if self.passes == 2 and not decode:
            raise ValueError(f"{type(self).__name__}: the second pass subtracts decoded frames: it needs decode=True")
        if self.passes == 2 and report:
            raise ValueError(f"{type(self).__name__}: the frame report reads the first spectrum ring, which a frame of the second pass "
                             f"may have left: passes=2 and report=True do not go together")
        self.reach_t = m.REACH_T if reach_t is None else int(reach_t)
        self.fs, self.baud, self.t_first = float(fs), m.BAUD, t_first
        self.decode, self.keep_llr = bool(decode), bool(keep_llr) or not decode
        self.ldpc = (_ldpc.params() if ldpc is None else ldpc) if decode else None
        self.osd = _ldpc.osd_cfg(osd)
        if self.osd is not None and not decode:
            raise ValueError(f"{type(self).__name__}: osd is a stage of the decoder: it needs decode=True")
        self.report = bool(report)
        if self.report and not decode:
            raise ValueError(f"{type(self).__name__}: report measures decoded frames: it needs decode=True")
        if decode:
            _ldpc.plan(self.ldpc)                                        # a bad setting fails here, with or without a device
        if self.osd is not None:
            _ldpc.osd_plan(self.osd)
        if chan is None:
            self.S, self.D, self.M = m.shape(fs)
            nk = self.M if channels is None else int(channels[1])
            m.plan(nk, self.S, max_out, m.params())                      # a bad shape fails here, with or without a device
            self.h = m.prototype(fs, self.M, self.S)
            self.chan = Channelizer(fs, self.M, self.D, self.h, channels, device, max_in)
        else:
            # a ready channelizer of either kind, adopted and owned: rows S baud / 4 apart at S baud samples per second
            self.chan = chan
            s = chan.fs_out / m.BAUD
            self.S, self.D, self.M = int(round(s)), chan.D, chan.M
            if abs(s - self.S) > 1e-9 * s or self.S not in m.SHAPES or chan.M != 4 * chan.D or float(fs) != chan.fs:
                raise ValueError(f"{type(self).__name__}: the channelizer's rows (fs {chan.fs}, fs_out {chan.fs_out}, M / D = "
                                 f"{chan.M / chan.D}) are not at {m.SHAPES[0]} or {m.SHAPES[1]} samples per symbol of {m.BAUD:.6g} baud "
                                 f"with M / D = 4 at fs = {fs}")
            self.h = chan.prototypes
        self.nsub, self.qs = self.S // 2, self.S // 4
        self.dec = self.DECODERS(self.chan, self.S, max_out)
        self.second = _pass.SecondPass(self) if self.passes == 2 else None   # it calls ``dec.keep``
        self.nk, self.nfine, self.fs_out = self.chan.nk, self.dec.nfine, self.chan.fs_out
        self.freqs = self.chan.freqs
        q = 2 * np.arange(self.nsub) - (self.dec.nb - 1)
        self.freqs_fine = (self.freqs[:, None] + q[None, :] * (m.BAUD / 4)).reshape(-1)
        self.circular = self.nk == self.M
        self.records = []
        self._pending, self._recent = [], []

    def reset(self):
        self.dec.reset()
        self.records = []
        self._pending, self._recent = [], []
        if self.second is not None:
            self.second.reset()

    def _events(self, x):
        """one call: the counts come off the device first, then only the rows that have events"""
        r = self.dec.decode_raw(x, events="counts")
        rows = np.flatnonzero(r["counts"])
        if r["n_out"] == 0 or r["n_steps"] == 0 or not len(rows):
            return []
        return self.dec.events_of(r, rows, self.dec.fetch(rows))

    def _owners(self, events):
        return owners(events, nfine=self.nfine if self.circular else None)

    def _fdist(self, a, b):
        d = abs(int(a) - int(b))
        return min(d, self.nfine - d) if self.circular else d

    def _record(self, t0, F, score, hits, llr=None):
        """an event as a record: its place in the band and the stream, and its soft bits where there are any"""
        m = self.DECODERS.MODE
        rec = dict(t0=t0, F=F, freq=float(self.freqs_fine[F]), time=self.qs * t0 / self.fs_out, score=score, hits=hits)
        if self.t_first is not None:
            T = float(self.t_first) + rec["time"]
            rec["slot"] = int(np.floor(T / m.SLOT_SECONDS))
            rec["dt"] = T - m.SLOT_SECONDS * rec["slot"] - m.NOMINAL_START
        if llr is not None:
            rec["llr"] = llr
        return rec

    def _decoded(self, rec, answer, k):
        """``rec`` with what row ``k`` of the bank's ``decode`` answer says about it"""
        m = self.DECODERS.MODE
        b77 = answer["bits"][k, :77].copy()
        i3, n3 = _msg.types(b77)
        ok = int(answer["status"][k]) == _ldpc.STATUS_OK
        rec.update(status=int(answer["status"][k]), ok=ok, iterations=int(answer["iterations"][k]), nerr=int(answer["nerr"][k]), bits77=b77,
                   i3=i3, n3=n3, text=m.UNPACK(b77) if ok and m.UNPACK is not None else None)
        if self.osd is not None:
            rec["osd"] = int(answer["osd"][k])
        return rec

    def _release(self):
        """the events whose rivals have all arrived: the owners among them, with their soft bits"""
        done, hold = self.dec.t_done, self.DECODERS.MODE.HOLD
        ripe = [e for e in self._pending if e[0] + hold <= done]
        if not ripe:
            return []
        pool = self._recent + self._pending
        out = [e for e, o in zip(pool, self._owners(pool)) if o and e in ripe and e[0] + hold <= done]
        first = min(e[0] for e in ripe)
        self._recent = [e for e in self._recent if e[0] >= first - 16] + ripe
        self._pending = [e for e in self._pending if e[0] + hold > done]
        out.sort(key=lambda e: (e[0], e[1]))
        if not out:
            return []
        Fs, ts = [e[1] for e in out], [e[0] for e in out]
        llr = self.dec.llr(Fs, ts) if self.keep_llr else None
        answer = self.dec.decode(Fs, ts, self.ldpc, osd=self.osd) if self.decode else None
        recs = [self._record(*e, None if llr is None else llr[k]) for k, e in enumerate(out)]
        if answer is not None:
            for k, rec in enumerate(recs):
                self._decoded(rec, answer, k)
        if self.report:
            self._measure(recs, answer["bits"])
        if self.second is not None:
            self.second.hold(self, recs, answer["bits"])
        return recs

    def _measure(self, recs, bits):
        """the frame report of a release: one floor over the newest frame's span, one report for the decoded records"""
        m = self.DECODERS.MODE
        keys = self.REPORT_KEYS + (("dt_fine",) if self.t_first is not None else ())
        for r in recs:
            r.update(dict.fromkeys(keys))
        good = [k for k, r in enumerate(recs) if r["ok"]]
        if not good:
            return
        lag = m.STEPS_PER_SYMBOL * (m.SYMBOLS - 1)
        floor = self.dec.floor(max(r["t0"] for r in recs) + lag, m.SYMBOLS)
        rep = self.dec.report([recs[k]["F"] for k in good], [recs[k]["t0"] for k in good], bits[good])
        for i, k in enumerate(good):
            r = recs[k]
            df, dt, peak = refine(rep["sig9"][i])
            noise = noise_of(floor, m.SYMBOLS, r["F"], self.nsub, self.circular, m.TONES, m.FLOOR_ROWS, m.FLOOR_QUANTILE)
            r.update(snr=float(snr_db(peak, noise, m.SYMBOLS, m.BAUD, m.CAL)), f_fine=float(self.freqs_fine[r["F"]] + df * m.BAUD / 2),
                     t_fine=(r["t0"] + dt) * self.qs / self.fs_out, nhard=int(rep["nhard"][i]), nsync=int(rep["nsync"][i]),
                     sig=peak / m.SYMBOLS, noise=noise)
            if self.t_first is not None:
                r["dt_fine"] = float(self.t_first) + r["t_fine"] - m.SLOT_SECONDS * r["slot"] - m.NOMINAL_START

    def push(self, x):
        """complex64 [n] -> the records of the frames whose step t0 + HOLD - 1 this input completes, owners only, sorted by
        (t0, F), and behind them what the second pass found.  ``records`` gains them.  The input goes through in calls of at
        most ``dec.max_samples()``."""
        x = np.ascontiguousarray(x, np.complex64)
        out, i = [], 0
        while i < len(x):
            n = min(len(x) - i, self.dec.max_samples())
            self._pending += self._events(x[i:i + n])
            out += self._release()
            if self.second is not None:
                out += self.second.run(self)
            i += n
        self.records += out
        return out
