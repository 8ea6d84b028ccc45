"""FT8 skimmer: Costas sync and soft bits on a fine raster of the band (kernels ``ft.hip``, host half
``api_ft.hip``).  8-FSK at 6.25 baud, tones 6.25 Hz apart, 79 symbols of which 21 are three Costas arrays.  A channelizer
with M / D = 4 delivers rows at ``S`` samples per symbol; inside every row ``NSUB = S / 2`` decoders run on the device, one
every 3.125 Hz, so that the fine rows ``F = a NSUB + j`` form one uniform raster over all rows.  The device finds every
frame by its sync score and hands out its 174 soft bits in transmission order; with ``decode=True`` the device also runs
the LDPC(174,91) decoder on them, straight from the spectrum ring, checks the CRC-14, and the record carries the message's
77 bits and its text (``ldpc.py``, ``ft8msg.py``); with ``report=True`` it measures every decoded frame
in the spectrum ring and the record carries its SNR, fine frequency and fine time (kernels ``report.hip``; DESIGN.md 3 item
26).  The tables and settings are derived here, once, and handed to the library already derived."""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np

from . import _lib
from . import channelizer as _chan
from . import ft8msg as _msg
from . import ldpc as _ldpc
from . import psk as _psk
from ._lib import Ft8Cfg
from .channelizer import Channelizer
from .skimmer import DecoderBank, Skimmer

BAUD = 6.25
COSTAS = (3, 1, 4, 0, 6, 5, 2)
GRAY = (0, 1, 3, 2, 5, 6, 4, 7)                  # value v is sent on tone GRAY[v]
SYMBOLS, DATA, BITS = 79, 58, 174
SYNC_AT = (0, 36, 72)                            # first symbol of the three Costas arrays
FRAME_SECONDS, SLOT_SECONDS, NOMINAL_START = SYMBOLS / BAUD, 15.0, 0.5
STEPS_PER_SYMBOL = 4
EMIT_LAG = 316                                   # an event t0 is emitted at step t0 + 316 ...
HOLD = 321                                       # ... and released once step t0 + 320 is complete: every rival has arrived
KEEP = 9
SHAPES = (64, 96)                                # row samples per symbol
NB_EXTRA = 14                                    # NB = NSUB + 14: decoder j uses bins j + 2 tone, tone 0 to 7
LLR_MAX = 4096
UNPACK = _msg.unpack77                           # the 77 decoded bits -> text (``ft4.py``: None, its scrambler is not here)


# ---- written once for both modes: ``mode`` is this module or ``ft4.py``, read for NAME, BAUD, SHAPES and PLAN_CALL ----------
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


# ---- this mode ------------------------------------------------------------------------------------------------------------
NAME, PLAN_CALL = "FT8", "pysdr_ft8_plan"
_MODE = sys.modules[__name__]


def shape(fs):
    """-> (S, D, M): S = 64 row samples per symbol if fs / (64 baud) is an integer D and the channelizer accepts M = 4 D,
    otherwise S = 96 likewise, otherwise ValueError."""
    return mode_shape(_MODE, fs)


def prototype(fs, M, S):
    """The channelizer's prototype for the FT8 raster, ``psk.prototype``'s form: Kaiser(8.0) windowed sinc of 4 M taps cut
    at fs_out / 2 = S baud / 2, sum 1.  A row's outer bin is (NB - 1) baud / 4 from its centre, a station up to a raster
    step beyond it, plus its own baud-wide tone: the response is flat within 0.1 dB out to fp = (NB + 1) baud / 4 + baud
    and at least 70 dB down from fs_out - fp on, where the aliases of that band begin."""
    return _psk.prototype(fs, M, BAUD, S)


def fine_channelizer(fs, band, device=0, max_in=1 << 22):
    """A ``fine.FineChannelizer`` for ``FT8_Skimmer(fs, chan=...)`` at a rate ``shape`` refuses: rows S baud / 4 apart whose
    centres lie in ``band = (f_lo, f_hi)`` Hz from the centre, S = 64 where ``fine.shape`` finds a shape, else 96; M2 / D2 =
    4, the second prototype is ``prototype`` at the first stage's output rate, the first ``fine.prototype1``."""
    return mode_fine_channelizer(_MODE, fs, band, device, max_in)


def params(smin=3.0, hmin=13, pmax=1e18):
    """The settings of DESIGN.md 3 item 22 as the ``_lib.Ft8Cfg`` the C ABI takes."""
    return Ft8Cfg(smin=float(np.float32(smin)), hmin=int(hmin), pmax=float(np.float32(pmax)))


def plan(nk, S, max_out, cfg):
    """What a skimmer of this shape launches (no device needed): dict of rows per workgroup, threads, LDS bytes, tile
    samples, event cap per decoder and call, workgroups, decoders per row, ring depth in steps.  Raises PysdrError
    outside the rules."""
    return mode_plan(_MODE, nk, S, max_out, cfg)


def unpack(words):
    """the two event words -> (index within the call of the emitting step, hits, score)"""
    w = int(words[0]) & 0xFFFFFFFF
    return w >> 5, w & 31, float(np.array([int(words[1]) & 0xFFFFFFFF], np.uint32).view(np.float32)[0])


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


def tones(bits):
    """174 bits in transmission order -> the frame's 79 tones: Costas arrays at symbols 0, 36 and 72, 2 x 29 data symbols
    of 3 bits, MSB first, Gray-mapped"""
    bits = np.asarray(bits, np.int64).reshape(DATA, 3)
    v = 4 * bits[:, 0] + 2 * bits[:, 1] + bits[:, 2]
    g = np.array(GRAY)[v]
    return np.concatenate((COSTAS, g[:29], COSTAS, g[29:], COSTAS)).astype(np.int64)


def waveform(tones, f0, fs, gfsk=True, phase=0.0):
    """complex128 frame of power 1 at ``fs``: tone 0 at ``f0`` Hz from the centre, continuous phase.  ``gfsk``: the
    frequency pulse of a symbol is (erf(k (t + 1/2)) - erf(k (t - 1/2))) / 2, k = 2 pi sqrt(2 / ln 2), t in symbols from the
    symbol's middle (BT = 2), the first and the last tone held beyond the frame; otherwise rectangular."""
    from scipy.special import erf
    tones = np.asarray(tones, np.float64)
    sps = float(fs) / BAUD
    n = int(round(len(tones) * sps))
    t = (np.arange(n) + 0.5) / sps                                       # symbols
    k0 = np.minimum(np.floor(t).astype(np.int64), len(tones) - 1)
    if gfsk:
        kk = 2 * np.pi * np.sqrt(2 / np.log(2))
        ext = np.concatenate((tones[:1], tones, tones[-1:]))
        dev = np.zeros(n)
        for d in (-1, 0, 1):                                             # the pulse is 0 to 1e-50 beyond a symbol and a half
            tau = t - (k0 + d) - 0.5
            dev += ext[k0 + d + 1] * 0.5 * (erf(kk * (tau + 0.5)) - erf(kk * (tau - 0.5)))
    else:
        dev = tones[k0]
    ph = np.cumsum(float(f0) + BAUD * dev)
    return np.exp(1j * (2 * np.pi / float(fs) * ph + phase))


# ---- the frame report on the host: float64, from the device's exact float32 numbers -----------------
REPORT_MODE = 0                                  # PYSDR_REPORT_FT8
REPORT_MAX = 4096
TONES = 8
SNR_BW = 2500.0                                  # the bandwidth an SNR is quoted in
FLOOR_QUANTILE = 0.02                            # a row's floor: this quantile of its NB bin means, all but the least of them
FLOOR_ROWS = (4, 8)                              # a candidate's noise: the median floor of the rows this far away, either side
CAL = -0.7                                       # dB: the bias of so low a quantile, measured (tests/test_report_oracle.py)


def report_plan(mode=None):
    """What a frame report launches (no device needed): dict of threads per candidate, LDS bytes, symbols of a frame and
    candidates per call.  Raises PysdrError for a mode that is neither."""
    v = _lib.plan_call("pysdr_report_plan", 4, int(REPORT_MODE if mode is None else mode))
    return {"threads": v[0], "lds_bytes": v[1], "symbols": v[2], "max_candidates": v[3]}


def delta(a, b, c):
    """Offset of a three-point parabola's peak from the middle point, in points, within +-0.5: 0 where ``a`` or ``c`` is
    missing (negative); with d = a - 2 b + c, clip(0.5 (a - c) / d) where d < 0, else half a point towards the greater
    neighbour.  ``b`` need not be the maximum."""
    a, b, c = float(a), float(b), float(c)
    if a < 0 or c < 0:
        return 0.0
    d = a - 2 * b + c
    if d < 0:
        return float(min(0.5, max(-0.5, 0.5 * (a - c) / d)))
    return 0.5 * float(np.sign(c - a))


def refine(sig9):
    """sig9 [3][3] (time outer, fine row inner) -> (delta_f in raster steps, delta_t in steps, peak): ``delta`` across the
    fine rows and across the steps through the candidate's own place; peak = b - 0.25 (a - c) delta_f, the parabola's
    height across the fine rows (b itself where a neighbour is missing)."""
    s = np.asarray(sig9, np.float64).reshape(3, 3)
    a, b, c = s[1, 0], s[1, 1], s[1, 2]
    df, dt = delta(a, b, c), delta(s[0, 1], b, s[2, 1])
    return df, dt, float(b - 0.25 * (a - c) * df)


def noise_floor(floor, nsym, quantile=None):
    """``FT8_Decoders.floor``'s sums [nk][NB] over ``nsym`` steps -> float64 [nk]: per row the lower quartile of its bins'
    mean powers"""
    q = FLOOR_QUANTILE if quantile is None else quantile
    return np.quantile(np.asarray(floor, np.float64) / float(nsym), q, axis=1)


def noise_of(floor, nsym, F, nsub, circular, tones=TONES, rows=None, quantile=None):
    """The noise power per bin for a candidate on fine row ``F``: the median of the floors of the rows 4 to 8 rows away
    on either side (circular where the raster is); of all other rows if there are none; and on a raster of one row the
    lower quartile of that row's own bins outside j - 2 .. j + 2 tones + 2."""
    floor = np.asarray(floor, np.float64)
    nk = floor.shape[0]
    lo, hi = FLOOR_ROWS if rows is None else rows
    q = FLOOR_QUANTILE if quantile is None else quantile
    a, j = divmod(int(F), int(nsub))
    if nk == 1:
        b = np.arange(floor.shape[1])
        out = floor[0, (b < j - 2) | (b > j + 2 * tones + 2)]
        return float(np.quantile((out if len(out) else floor[0]) / float(nsym), q))
    fl = noise_floor(floor, nsym, q)
    far = set()
    for d in range(lo, hi + 1):
        for r in (a - d, a + d):
            if circular:
                far.add(r % nk)
            elif 0 <= r < nk:
                far.add(r)
    far.discard(a)
    if not far:
        far = set(range(nk)) - {a}
    return float(np.median(fl[sorted(far)]))


def snr_db(peak, noise, nsym, baud=BAUD, cal=None):
    """10 log10(max(peak / nsym - noise, 1e-3 noise) / noise) - 10 log10(2500 / baud) + CAL: dB in 2500 Hz"""
    cal = CAL if cal is None else cal
    s = max(float(peak) / float(nsym) - float(noise), 1e-3 * float(noise))
    return 10 * np.log10(s / float(noise)) - 10 * np.log10(SNR_BW / baud) + cal


def spots(records, reach=8):
    """Among the ``ok`` records with equal ``bits77`` whose ``t0`` differ by at most ``reach`` steps keep the one of
    greatest ``sig`` (ties: the lower (t0, F)): one message seen on two fine rows, or a step apart, is one spot.  -> the
    records kept, in their order; records without ``ok`` are not spots."""
    ok = [r for r in records if r.get("ok")]
    keys = [bytes(np.asarray(r["bits77"], np.uint8)) for r in ok]
    out = []
    for i, r in enumerate(ok):
        beaten = False
        for k, o in enumerate(ok):
            if k == i or keys[k] != keys[i] or abs(o["t0"] - r["t0"]) > reach:
                continue
            if o["sig"] > r["sig"] or (o["sig"] == r["sig"] and (o["t0"], o["F"]) < (r["t0"], r["F"])):
                beaten = True
                break
        if not beaten:
            out.append(r)
    return out


def spot_line(rec, f_centre=0.0, slot_seconds=SLOT_SECONDS):
    """A reported record as the usual line ``HHMMSS snr dt freq ~ text``: the slot's UTC start, dB in 2500 Hz, seconds
    against the nominal start, Hz (``f_centre`` is the band centre's dial offset).  Without ``t_first`` the time is empty
    and dt is the frame's time into the stream."""
    if "slot" in rec:
        s = int(rec["slot"] * slot_seconds) % 86400
        when, dt = f"{s // 3600:02d}{s // 60 % 60:02d}{s % 60:02d}", rec["dt_fine"]
    else:
        when, dt = "", rec["t_fine"]
    return f"{when:6s} {int(round(rec['snr'])):3d} {dt:4.1f} {int(round(f_centre + rec['f_fine'])):4d} ~  {rec['text'] or ''}".rstrip()


# ---- the second pass: tables and the trial grid, derived here in float64 and rounded once ----------
PULSE_SYMBOLS = 3                                # symbols the frequency pulse of ``waveform`` spans (BT = 2)
PULSE_K = 2 * np.pi * np.sqrt(2 / np.log(2))
REACH_T = 40                                     # steps a rescan looks to either side of a subtracted frame
PASS_TRIALS, PASS_MAX, PASS_LUT, PASS_EVENT_CAP, PASS_ROWS_MAX, PASS_WINDOW_MAX = 9, 256, 4096, 52, 256, 256
# The trial grid: 3 times x 3 frequencies around the refined values.  ``refine`` leaves the time within 0.35 step and the
# frequency within 0.4 Hz, so a quarter step and 0.3 Hz to either side cover both, and the best
# trial is then within an eighth of a step and 0.15 Hz: about -27 dB of the frame left by the frequency error alone.
TRIAL_DN = 0.25                                  # steps between the trial times
TRIAL_DF = 0.3                                   # Hz between the trial frequencies


def pass_pulse(mode, S):
    """uint32 [PULSE_SYMBOLS S]: the phase one symbol of tone 1 has added by row sample i of the symbols its frequency
    pulse spans, 2^32 a turn: the cumulative sum of ``waveform``'s pulse at the samples' middles, scaled so that the
    whole pulse is exactly one turn (which the last entry holds as 0)."""
    import math
    P = mode.PULSE_SYMBOLS
    tau = (np.arange(P * S) + 0.5) / S - P / 2
    erf = np.vectorize(math.erf)
    g = 0.5 * (erf(mode.PULSE_K * (tau + 0.5)) - erf(mode.PULSE_K * (tau - 0.5)))
    c = np.cumsum(g)
    return np.ascontiguousarray((np.rint(c / c[-1] * 2.0 ** 32).astype(np.uint64) & 0xFFFFFFFF).astype(np.uint32))


def pass_lut():
    """float32 [4096][2] = (cos, sin)(2 pi i / 4096)"""
    t = 2 * np.pi * np.arange(PASS_LUT) / PASS_LUT
    return np.ascontiguousarray(np.stack((np.cos(t), np.sin(t)), axis=1), np.float32)


def pass_plan(mode, nk, S, max_out, reach_t=None):
    """What a second pass keeps and launches (no device needed): dict of threads, LDS bytes, ty (samples of a row kept),
    tr2 (steps kept), jobs and frames per subtract call, events per fine row of a rescan, symbols of the pulse."""
    v = _lib.plan_call("pysdr_pass_plan", 8, int(mode.REPORT_MODE), int(nk), int(S), int(max_out), int(mode.REACH_T if reach_t is None else reach_t))
    return dict(zip(("threads", "lds_bytes", "ty", "tr2", "max_jobs", "max_frames", "event_cap", "pulse_symbols"), v))


def trial_grid(mode, df, dt, qs, fs_out):
    """int32 [9][2] = (dn, fw): the refined offsets ``df`` (raster steps of baud / 2) and ``dt`` (steps) -> 3 times (outer)
    x 3 frequencies (inner) around them: dn in row samples, fw the phase word per row sample.  ``subtract`` refuses a dn of
    a step or more, so a trial time beyond QS - 1 samples is MOVED to QS - 1 (-(QS - 1)): that trial is then not the one the
    grid asked for.  ``refine`` leaves |dt| <= 0.5, so only the outer trials of a frame half a step off are moved, by at
    most QS / 4 - 1 samples."""
    out = np.zeros((9, 2), np.int64)
    for a, it in enumerate((-1, 0, 1)):
        dn = int(np.clip(np.rint((dt + it * mode.TRIAL_DN) * qs), -(qs - 1), qs - 1))
        for b, jf in enumerate((-1, 0, 1)):
            hz = df * mode.BAUD / 2 + jf * mode.TRIAL_DF
            out[3 * a + b] = dn, int(np.rint(hz / fs_out * 2.0 ** 32))
    return (out & 0xFFFFFFFF).astype(np.uint32).view(np.int32)              # (dn as its two's complement, which int32 reads back)


def pack91(bits91, n):
    """uint8 [n][91] -> [n][12], MSB first, as the decoder packs them"""
    b = np.ascontiguousarray(bits91, np.uint8).reshape(n, _ldpc.K) & 1
    return np.ascontiguousarray(np.packbits(np.concatenate((b, np.zeros((n, 5), np.uint8)), axis=1), axis=1))


class FT8_Decoders(DecoderBank):
    """The decoder bank on a borrowed ``Channelizer`` (which it resets, and which must be fed only through it)."""
    KIND, DESTROY = "ft8", "pysdr_ft8_destroy"
    MODE = sys.modules[__name__]                                         # the mode's constants, settings, plan and tables (``ft4.py`` has its own)

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
        out = []
        for k, F in enumerate(rows):
            for i in range(int(r["counts"][F])):
                u, hits, score = unpack(words[k, 2 * i:2 * i + 2])
                out.append((r["t_first"] + u - self.MODE.EMIT_LAG, int(F), score, hits))
        return out

    def llr(self, F, t0):
        """float32 [n][174]: the soft bits of the candidates (F[i], t0[i]); PysdrError for a frame that is not complete yet
        or has left the ring, or an F outside the raster"""
        F = np.ascontiguousarray(F, np.int32)
        t0 = np.ascontiguousarray(t0, np.int64)
        out = np.zeros((len(F), self.MODE.BITS), np.float32)
        for i in range(0, len(F), LLR_MAX):
            f, t, o = F[i:i + LLR_MAX], t0[i:i + LLR_MAX], out[i:i + LLR_MAX]
            self._call("llr", f.ctypes.data_as(C.POINTER(C.c_int32)), t.ctypes.data_as(C.POINTER(C.c_longlong)), len(f), _lib.as_pf(o))
        return out

    def _decoded(self, n, post):
        return (np.zeros((n, 4), np.int32), np.zeros((n, 12), np.uint8), np.zeros((n, self.MODE.BITS), np.float32) if post else None)

    @staticmethod
    def _answer(st, bits, post, osd=None, detail=None):
        out = dict(status=st[:, 0].copy(), iterations=st[:, 1].copy(), nerr=st[:, 2].copy(), bits=_ldpc.unpack_bits(bits))
        if post is not None:
            out["post"] = post
        if osd is not None:
            out["osd"] = st[:, 3].copy()
        if detail is not None:
            out["detail"] = detail
        return out

    @staticmethod
    def _osd(osd, detail, n):
        """-> (the OsdCfg or None, the detail array or None)"""
        osd = _ldpc.osd_cfg(osd)
        if osd is None and detail:
            raise ValueError("detail is the second stage's: it needs osd")
        return osd, np.zeros((n, 4), np.int32) if detail else None

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
        F = np.ascontiguousarray(F, np.int32)
        t0 = np.ascontiguousarray(t0, np.int64)
        cfg = _ldpc.params() if cfg is None else cfg
        osd, de = self._osd(osd, detail, len(F))
        st, bits, po = self._decoded(len(F), post)
        if residual:
            self._need_kept()
        for i in range(0, len(F), LLR_MAX):
            f, t = F[i:i + LLR_MAX], t0[i:i + LLR_MAX]
            args = (f.ctypes.data_as(C.POINTER(C.c_int32)), t.ctypes.data_as(C.POINTER(C.c_longlong)), len(f), C.byref(cfg),
                    st[i:].ctypes.data_as(C.POINTER(C.c_int32)), bits[i:].ctypes.data_as(C.POINTER(C.c_uint8)),
                    None if po is None else _lib.as_pf(po[i:]))
            if residual:
                self._call("pass_decode", *args, None if osd is None else C.byref(osd),
                           None if de is None else de[i:].ctypes.data_as(C.POINTER(C.c_int32)))
            elif osd is None:
                self._call("decode", *args)
            else:
                self._call("decode_osd", *args, C.byref(osd), None if de is None else de[i:].ctypes.data_as(C.POINTER(C.c_int32)))
        return self._answer(st, bits, po, osd, de)

    def decode_llr(self, llr, cfg=None, post=False, osd=None, detail=False):
        """Soft bits from the host, float32 [n][174], positive for bit 1, any scale -> ``decode``'s answer.  In calls of
        4096; a value that is not finite is refused."""
        llr = np.ascontiguousarray(llr, np.float32).reshape(-1, self.MODE.BITS)
        cfg = _ldpc.params() if cfg is None else cfg
        osd, de = self._osd(osd, detail, len(llr))
        st, bits, po = self._decoded(len(llr), post)
        for i in range(0, len(llr), LLR_MAX):
            v = llr[i:i + LLR_MAX]
            args = (_lib.as_pf(v), len(v), C.byref(cfg), st[i:].ctypes.data_as(C.POINTER(C.c_int32)),
                    bits[i:].ctypes.data_as(C.POINTER(C.c_uint8)), None if po is None else _lib.as_pf(po[i:]))
            if osd is None:
                self._call("decode_llr", *args)
            else:
                self._call("decode_llr_osd", *args, C.byref(osd), None if de is None else de[i:].ctypes.data_as(C.POINTER(C.c_int32)))
        return self._answer(st, bits, po, osd, de)

    def report(self, F, t0, bits91):
        """The candidates (F[i], t0[i]) of ``llr``, under its rules, with the 91 bits of each as ``decode`` returns them
        (uint8 [n][91]; the CRC is not checked) -> dict of sig9 float32 [n][3][3] (the sum of the frame's sent tones at
        t0 - 1, t0, t0 + 1 outer and F - 1, F, F + 1 inner; -1 where a place is outside the raster or the ring), tot float32
        [n] (all tones at the candidate's own place), nhard and nsync int32 [n] (data and Costas symbols whose sent tone is
        not the strongest).  DESIGN.md 3 item 26; in calls of 4096."""
        F = np.ascontiguousarray(F, np.int32)
        t0 = np.ascontiguousarray(t0, np.int64)
        b = np.ascontiguousarray(bits91, np.uint8).reshape(len(F), _ldpc.K) & 1
        packed = np.ascontiguousarray(np.packbits(np.concatenate((b, np.zeros((len(F), 5), np.uint8)), axis=1), axis=1))
        power = np.zeros((len(F), 10), np.float32)
        errs = np.zeros((len(F), 2), np.int32)
        for i in range(0, len(F), REPORT_MAX):
            f, t, p = F[i:i + REPORT_MAX], t0[i:i + REPORT_MAX], packed[i:i + REPORT_MAX]
            self._call("report", f.ctypes.data_as(C.POINTER(C.c_int32)), t.ctypes.data_as(C.POINTER(C.c_longlong)),
                       p.ctypes.data_as(C.POINTER(C.c_uint8)), len(f), _lib.as_pf(power[i:]), errs[i:].ctypes.data_as(C.POINTER(C.c_int32)))
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

    def keep(self, reach_t=None, trials=PASS_TRIALS):
        """From now on -- allowed only before the stream begins, after create or ``reset`` -- every call also keeps its
        row samples and a second spectrum ring for ``subtract``, ``rescan`` and ``decode(residual=True)``.  ``reach_t``:
        steps a rescan will look to either side of a subtracted frame (default the mode's ``REACH_T``); ``trials``: the
        (dn, fw) pairs every frame of a ``subtract`` call carries.  -> the plan (``pass_plan``)."""
        m = self.MODE
        reach_t = m.REACH_T if reach_t is None else int(reach_t)
        plan = pass_plan(m, self.nk, self.S, self.max_out, reach_t)          # a bad reach_t fails here
        self._pulse, self._lut = pass_pulse(m, self.S), pass_lut()
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
        where there is none), trial and used int32 [n][2].  At most 256 frames; PysdrError for a frame whose steps
        t0 - 4 .. t0 + lag + 4 are not all complete and held."""
        self._need_kept()
        F = np.ascontiguousarray(F, np.int32)
        t0 = np.ascontiguousarray(t0, np.int64)
        packed = pack91(bits91, len(F))
        tr = np.ascontiguousarray(trials, np.int32).reshape(len(F), self.kept["trials"], 2)
        out = np.zeros((len(F), 2, 4), np.int32)
        p32 = C.POINTER(C.c_int32)
        self._call("subtract", F.ctypes.data_as(p32), t0.ctypes.data_as(C.POINTER(C.c_longlong)), packed.ctypes.data_as(C.POINTER(C.c_uint8)),
                   tr.ctypes.data_as(p32), len(F), out.ctypes.data_as(p32))
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
        ev = np.zeros((max(nF, 1), PASS_EVENT_CAP, 2), np.int32)
        p32 = C.POINTER(C.c_int32)
        self._call("rescan", int(F_lo), int(F_hi), C.c_longlong(int(t_lo)), C.c_longlong(int(t_hi)), C.byref(cfg), counts.ctypes.data_as(p32),
                   ev.ctypes.data_as(p32))
        out = []
        for k in range(nF):
            for i in range(int(counts[k])):
                u, hits, score = unpack(ev[k, i])
                out.append((int(t_lo) + u, int(F_lo) + k, score, hits))
        return out

    def pass_llr(self, F, t0):
        """``llr`` from the residue"""
        self._need_kept()
        F = np.ascontiguousarray(F, np.int32)
        t0 = np.ascontiguousarray(t0, np.int64)
        out = np.zeros((len(F), self.MODE.BITS), np.float32)
        self._call("pass_llr", F.ctypes.data_as(C.POINTER(C.c_int32)), t0.ctypes.data_as(C.POINTER(C.c_longlong)), len(F), _lib.as_pf(out))
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
        self._call("state", _lib.as_pf(sc), hits.ctypes.data_as(C.POINTER(C.c_int32)), None if rg is None else _lib.as_pf(rg), C.byref(done))
        out = dict(sc=sc, hits=hits, t_done=int(done.value))
        if ring:
            out["ring"] = rg
        return out


class FT8_Skimmer(Skimmer):
    """Wideband IQ at ``fs`` -> a channelizer of M = 4 D rows S baud / 4 apart at S baud samples per second -> NSUB = S / 2
    sync decoders inside every row, fine row F with tone 0 at ``freqs_fine[F]`` Hz (signed) -> a record for every frame
    found: ``t0`` (steps of a quarter symbol since create / reset), ``F``, ``freq``, ``time`` (seconds into the stream),
    ``score``, ``hits`` and ``llr`` float32 [174]; with ``t_first`` (UTC seconds of sample 0) also ``slot`` and ``dt``.
    With ``decode=True`` the owners go through the LDPC decoder on the device (``ldpc``: ``ldpc.params()``) and a record
    gains ``status``, ``ok`` (status 2), ``iterations``, ``nerr``, ``bits77``, ``i3``, ``n3`` and ``text`` (None where the
    frame did not decode or its message type is not unpacked); ``keep_llr=False`` then skips the soft bits' download and
    the records carry no ``llr``.  ``passes=2`` (with ``decode=True``; ``reach_t`` steps, default the mode's ``REACH_T``) takes
    every decoded frame out of the kept row samples once it is due and searches the residue around it again (``_second``;
    DESIGN.md 3 item 27): every record then carries ``pass``, 1 or 2, and a record of pass 2 is a frame found under a
    stronger one (its ``llr`` is the residue's); ``report=True`` is refused with it, for the report reads the first ring.  ``osd=2`` (an order 0 to 2, or ``ldpc.osd_params()``) sends the frames min-sum could not
    decode through ordered-statistics decoding and a record gains ``osd``: 0, the stage did not
    run; 1, 2, 3, it did.  Off by default: the CRC-14 is that stage's only guard, and a frame that reaches it comes out as
    a false message with probability about 2^-14.  ``report=True`` measures every decoded frame in the spectrum ring
    (DESIGN.md 3 item 26): one row-floor call per release and one report call for the records with ``ok``, which gain
    ``snr`` (dB in 2500 Hz), ``f_fine`` (Hz), ``t_fine`` (s), ``nhard``, ``nsync``, ``sig`` and ``noise`` (the mean power of
    the sent tones at the refined peak and the noise power per bin) and, with ``t_first``, ``dt_fine``; the other records
    carry the same keys as None.  ``spots`` then keeps one record per message and ``spot_line`` formats it."""

    DECODERS = FT8_Decoders                                              # the bank; its MODE is the skimmer's too

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
        if self.passes == 2:
            self.dec.keep(self.reach_t)
        self.nk, self.nfine, self.fs_out = self.chan.nk, self.dec.nfine, self.chan.fs_out
        self.freqs = self.chan.freqs
        q = 2 * np.arange(self.nsub) - (self.dec.nb - 1)
        self.freqs_fine = (self.freqs[:, None] + q[None, :] * (m.BAUD / 4)).reshape(-1)
        self.circular = self.nk == self.M
        self.records = []
        self._pending, self._recent = [], []
        self._await, self._ok = [], []                                   # second pass: decoded frames not yet due; every ok record

    def reset(self):
        self.dec.reset()
        self.records = []
        self._pending, self._recent = [], []
        self._await, self._ok = [], []

    def _events(self, x):
        """one call: the counts come off the device first, then only the rows that have events"""
        r = self.dec.decode_raw(x, events="counts")
        if r["n_out"] == 0 or r["n_steps"] == 0:
            return []
        rows = np.flatnonzero(r["counts"])
        if not len(rows):
            return []
        return self.dec.events_of(r, rows, self.dec.fetch(rows))

    def _release(self):
        """the events whose rivals have all arrived: the owners among them, with their soft bits"""
        m = self.DECODERS.MODE
        done, hold = self.dec.t_done, m.HOLD
        ripe = [e for e in self._pending if e[0] + hold <= done]
        if not ripe:
            return []
        pool = self._recent + self._pending
        own = owners(pool, nfine=self.nfine if self.circular else None)
        out = [e for e, o in zip(pool, own) if o and e in ripe and e[0] + hold <= done]
        first = min(e[0] for e in ripe)
        self._recent = [e for e in self._recent if e[0] >= first - 16] + ripe
        self._pending = [e for e in self._pending if e[0] + hold > done]
        out.sort(key=lambda e: (e[0], e[1]))
        if not out:
            return []
        Fs, ts = [e[1] for e in out], [e[0] for e in out]
        llr = self.dec.llr(Fs, ts) if self.keep_llr else None
        dec = self.dec.decode(Fs, ts, self.ldpc, osd=self.osd) if self.decode else None
        recs = []
        for k, (t0, F, score, hits) in enumerate(out):
            rec = dict(t0=t0, F=F, freq=float(self.freqs_fine[F]), time=self.qs * t0 / self.fs_out, score=score, hits=hits)
            if llr is not None:
                rec["llr"] = llr[k]
            if dec is not None:
                b77 = dec["bits"][k, :77].copy()
                i3, n3 = _msg.types(b77)
                ok = int(dec["status"][k]) == _ldpc.STATUS_OK
                rec.update(status=int(dec["status"][k]), ok=ok, iterations=int(dec["iterations"][k]), nerr=int(dec["nerr"][k]), bits77=b77,
                           i3=i3, n3=n3, text=m.UNPACK(b77) if ok and m.UNPACK is not None else None)
                if self.osd is not None:
                    rec["osd"] = int(dec["osd"][k])
            if self.t_first is not None:
                T = float(self.t_first) + rec["time"]
                rec["slot"] = int(np.floor(T / m.SLOT_SECONDS))
                rec["dt"] = T - m.SLOT_SECONDS * rec["slot"] - m.NOMINAL_START
            recs.append(rec)
        if self.report:
            self._measure(recs, dec["bits"])
        if self.passes == 2:
            self._hold_for_second(recs, dec["bits"])
        return recs

    def _base_record(self, t0, F, score, hits):
        m = self.DECODERS.MODE
        rec = dict(t0=t0, F=F, freq=float(self.freqs_fine[F]), time=self.qs * t0 / self.fs_out, score=score, hits=hits)
        if self.t_first is not None:
            T = float(self.t_first) + rec["time"]
            rec["slot"] = int(np.floor(T / m.SLOT_SECONDS))
            rec["dt"] = T - m.SLOT_SECONDS * rec["slot"] - m.NOMINAL_START
        return rec

    def _hold_for_second(self, recs, bits):
        """pass-1 records gain ``pass``; the decoded ones wait, with their bits and refined place, until they are due"""
        for r in recs:
            r["pass"] = 1
        good = [k for k, r in enumerate(recs) if r["ok"]]
        if not good:
            return
        rep = self.dec.report([recs[k]["F"] for k in good], [recs[k]["t0"] for k in good], bits[good])
        for i, k in enumerate(good):
            df, dt, _ = refine(rep["sig9"][i])
            self._await.append((recs[k], bits[k].copy(), df, dt))
            self._ok.append(recs[k])

    def _fdist(self, a, b):
        d = abs(int(a) - int(b))
        return min(d, self.nfine - d) if self.circular else d

    def _second(self):
        """The second pass, in absolute steps: a decoded frame is due once step t0 + HOLD + reach_t - 1
        is complete; due frames go in ascending t0, those of one t0 together: subtract them, rescan the residue around each
        (F -+ (2 TONES + 2) fine rows inside the raster, t0 -+ reach_t), keep the owners among the new events that are not
        within (4 steps, 2 fine rows) of a decoded record with t0' <= t0 + reach_t (every such record has been released by
        then, however the stream was cut), decode them from the residue and keep the messages that are not one of those
        records' within 8 steps.  -> the new records, ``pass`` 2."""
        m, R, done = self.DECODERS.MODE, self.reach_t, self.dec.t_done
        due = [a for a in self._await if a[0]["t0"] + m.HOLD + R <= done]
        if not due:
            return []
        self._await = [a for a in self._await if a[0]["t0"] + m.HOLD + R > done]
        due.sort(key=lambda a: (a[0]["t0"], a[0]["F"]))
        out, W = [], 2 * m.TONES + 2
        for t0 in sorted({a[0]["t0"] for a in due}):
            grp = [a for a in due if a[0]["t0"] == t0]
            Fs = [a[0]["F"] for a in grp]
            trials = np.array([trial_grid(m, a[2], a[3], self.qs, self.fs_out) for a in grp], np.int32)
            self.dec.subtract(Fs, [t0] * len(grp), np.array([a[1] for a in grp]), trials)
            found = {}
            for F in Fs:
                for e in self.dec.rescan(max(0, F - W), min(self.nfine - 1, F + W), max(0, t0 - R), t0 + R):
                    found[(e[0], e[1])] = e
            events = sorted(found.values())
            own = owners(events, nfine=self.nfine if self.circular else None)
            known = [r for r in self._ok if r["t0"] <= t0 + R]
            cand = [e for e, o in zip(events, own)
                    if o and not any(abs(e[0] - r["t0"]) <= 4 and self._fdist(e[1], r["F"]) <= 2 for r in known)]
            if not cand:
                continue
            cF, ct = [e[1] for e in cand], [e[0] for e in cand]
            dec = self.dec.decode(cF, ct, self.ldpc, osd=self.osd, residual=True)
            llr = self.dec.pass_llr(cF, ct) if self.keep_llr else None
            for k, (et, eF, score, hits) in enumerate(cand):
                if int(dec["status"][k]) != _ldpc.STATUS_OK:
                    continue
                b77 = dec["bits"][k, :77].copy()
                if any(abs(r["t0"] - et) <= 8 and np.array_equal(r["bits77"], b77) for r in known):
                    continue
                rec = self._base_record(et, eF, score, hits)
                if llr is not None:
                    rec["llr"] = llr[k]
                i3, n3 = _msg.types(b77)
                rec.update(status=_ldpc.STATUS_OK, ok=True, iterations=int(dec["iterations"][k]), nerr=int(dec["nerr"][k]), bits77=b77, i3=i3,
                           n3=n3, text=m.UNPACK(b77) if m.UNPACK is not None else None)
                if self.osd is not None:
                    rec["osd"] = int(dec["osd"][k])
                rec["pass"] = 2
                known.append(rec)
                self._ok.append(rec)
                out.append(rec)
            self._ok = [r for r in self._ok if r["t0"] >= t0 - R - 8]      # older ones meet no later group
        return out

    REPORT_KEYS = ("snr", "f_fine", "t_fine", "nhard", "nsync", "sig", "noise")

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
        (t0, F).  ``records`` gains them.  The input goes through in calls of at most ``dec.max_samples()``."""
        x = np.ascontiguousarray(x, np.complex64)
        out, i = [], 0
        while i < len(x):
            n = min(len(x) - i, self.dec.max_samples())
            self._pending += self._events(x[i:i + n])
            out += self._release()
            if self.passes == 2:
                out += self._second()
            i += n
        self.records += out
        return out
