"""RTTY raster skimmer: a Baudot decoder on a fine raster of the band (kernel ``fsk.hip``, host half
``api_fsk.hip``).  45.45 baud, 170 Hz shift, mark the upper tone.  A ``Channelizer`` with M / D = 4 delivers rows at ``S``
samples per bit; inside every row a bank of ``NSUB = S`` decoders runs on the device, one every baud / 4, so that the fine
rows ``F = a NSUB + j`` form one uniform raster over all rows.  A finder on the host decides after every call which decoder
of a neighbourhood owns a station; only the owners' events are downloaded.  The tables and settings are derived here,
once, and handed to the library already derived.  (``rtty.RTTY_Skimmer`` is the reference's own decoder on one 48 kHz
line; this one runs behind either kind of channelizer at any rate they serve.)"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

from . import _lib
from . import channelizer as _chan
from . import psk as _psk
from ._lib import FskCfg
from .channelizer import Channelizer
from .rtty import code_text
from .skimmer import DecoderBank, Skimmer

BAUD = 500.0 / 11                        # the reference's T = 22 ms
TONE_STEPS = 15                          # mark is 15 raster steps of baud / 4 above space: 170.45 Hz
STATE_FLOATS = ("qn", "qd", "bm", "bs")
STATE_INTS = ("st", "cnt", "sh", "nb", "prev", "fig", "open", "seen")
NEIGHBOURHOOD = 16                       # fine rows on either side a station's owner beats: the window's main lobe, about
#                                          12 steps, and the images 15 steps away where one tone meets the other's filter
SHAPES = (22, 33)                        # row samples per bit


def unpack(word):
    """event word -> (index within the call, code = the five data bits + 32 in figures shift)"""
    w = int(word) & 0xFFFFFFFF
    return w >> 6, w & 63


def shape(fs):
    """-> (S, D, M): S = 22 row samples per bit if fs / (22 baud) is an integer D and the channelizer accepts M = 4 D,
    otherwise S = 33 likewise, otherwise ValueError."""
    for S in SHAPES:
        d = float(fs) / (S * BAUD)
        D = int(round(d))
        if D < 1 or abs(d - D) > 1e-9 * max(d, 1.0):
            continue
        try:
            _chan.plan(4 * D, D, 16 * D)
        except _lib.PysdrError:
            continue
        return S, D, 4 * D
    raise ValueError(f"no RTTY raster for fs = {fs}: fs / 1000 or fs / 1500 must be an integer D with M = 4 D a channelizer size")


def prototype(fs, M, S):
    """The channelizer's prototype for the RTTY raster, ``psk.prototype``'s form: Kaiser(8.0) windowed sinc of 4 M taps cut
    at fs_out / 2 = S baud / 2, sum 1.  The rows are S baud / 4 apart, so a decoder's outer tone is at most half a spacing
    plus 15 baud / 8 plus its own baud-wide spectrum from a row's centre: the response is flat within 0.1 dB out to fp =
    S baud / 8 + 15 baud / 8 + baud and at least 70 dB down from fs_out - fp on, where the aliases of that band begin."""
    return _psk.prototype(fs, M, BAUD, S)


def fine_channelizer(fs, band, device=0, max_in=1 << 22):
    """A ``fine.FineChannelizer`` for ``RTTY_Raster_Skimmer(fs, chan=...)`` at a rate ``shape`` refuses: rows S baud / 4
    apart whose centres lie in ``band = (f_lo, f_hi)`` Hz from the centre, S = 22 where ``fine.shape`` finds a shape, else
    33; M2 / D2 = 4, the second prototype is ``prototype`` at the first stage's output rate, the first ``fine.prototype1``."""
    from . import fine
    err = None
    for S in SHAPES:
        try:
            M1, D1, M2, D2 = fine.shape(fs, S * BAUD, 4)
        except ValueError as e:
            err = e
            continue
        h2 = prototype(float(fs) / D1, M2, S)
        return fine.FineChannelizer(fs, M1, M2, D1, D2, fine.prototype1(fs, M1, D1, M2), h2,
                                    fine.channels_for(band, fs, M1, D1, M2), device, max_in)
    raise ValueError(f"no RTTY raster in two stages for fs = {fs}: {err}")


def tables(S):
    """-> (tw float32 [8 S][2] = (cos, -sin)(2 pi t / NT), g float32 [S] = kaiser(S, 8.6), the reference's window over one
    bit, scaled to sum 1): derived in float64, rounded once"""
    t = 2 * np.pi * np.arange(8 * S) / (8 * S)
    tw = np.stack((np.cos(t), -np.sin(t)), axis=1)
    g = np.kaiser(S, 8.6)
    return np.ascontiguousarray(tw, np.float32), np.ascontiguousarray(g / g.sum(), np.float32)


def params(a_q=1.0 / 64, a_b=1.0 / 32, hi=0.8, lo=0.65, bal=0.25, pmax=1e18, n0=64):
    """The settings of DESIGN.md 3 item 21 as the ``_lib.FskCfg`` the C ABI takes."""
    def f(v):                                        # the float32 nearest to v, as the Python float ctypes takes
        return float(np.float32(v))

    return FskCfg(a_q=f(a_q), a_b=f(a_b), hi=f(hi), lo=f(lo), bal=f(bal), pmax=f(pmax), n0=int(n0))


def cfg_dict(cfg):
    return {k: getattr(cfg, k) for k, _ in FskCfg._fields_}


def plan(nk, S, max_out, cfg):
    """What a skimmer of this shape launches (no device needed): dict of rows per workgroup, threads, LDS bytes, tile
    samples, event cap per decoder and call, workgroups, decoders per row.  Raises PysdrError outside the rules."""
    v = _lib.plan_call("pysdr_fsk_plan", 8, int(nk), int(S), int(max_out), C.byref(cfg) if cfg is not None else None)
    return {"rows": v[0], "threads": v[1], "lds_bytes": v[2], "tile": v[3], "cap": v[4], "groups": v[5], "nsub": v[6]}


def owners(qn, is_open, circular, prev=None):
    """The finder: ``psk.owners``' rule with this raster's reach, 16 fine rows to either side.  -> bool [NF]"""
    return _psk.owners(qn, is_open, circular, prev, reach=NEIGHBOURHOOD)


class RTTY_Raster_Decoders(DecoderBank):
    """The decoder bank on a borrowed ``Channelizer`` (which it resets, and which must be fed only through it)."""
    KIND, DESTROY = "fsk", "pysdr_fsk_destroy"

    def __init__(self, chan, S, max_out=256, cfg=None):
        super().__init__(chan, max_out)
        self.S = self.nsub = int(S)
        self.nfine = self.nk * self.nsub
        self.cfg = params() if cfg is None else cfg
        self.plan = plan(self.nk, self.S, self.max_out, self.cfg)         # a bad shape fails here
        self.tw, self.g = tables(self.S)
        self._open(self.nfine, self.S, C.byref(self.cfg), _lib.as_pf(self.tw), _lib.as_pf(self.g))

    def decode_raw(self, x, n=None, on_device=False, events="all", squelch=False):
        """One call of the C ABI: host samples (complex64 [n]) or a device pointer.  -> dict of n_out, m0 (the absolute
        index of the call's first output), counts [nfine] and events: every fine row's slots [nfine][cap] ("all") or
        nothing ("counts": the counts alone; None: counts is None too, everything stays on the device and the call only
        queues work when the input is on the device).  ``squelch``: the end state's qn and open [nfine] as well."""
        qn = is_open = pq = po = None
        if squelch:
            qn, is_open = np.zeros(self.nfine, np.float32), np.zeros(self.nfine, np.int32)
            pq, po = _lib.as_pf(qn), is_open.ctypes.data_as(C.POINTER(C.c_int32))
        return dict(self._decode(x, n, on_device, events, pq, po), qn=qn, open=is_open)

    def state(self):
        """dict of float32 qn, qd, bm, bs [nfine] and int32 st, cnt, sh, nb, prev, fig, open, seen [nfine]"""
        f = np.empty((len(STATE_FLOATS), self.nfine), np.float32)
        ints = np.empty((len(STATE_INTS), self.nfine), np.int32)
        self._call("state", _lib.as_pf(f), ints.ctypes.data_as(C.POINTER(C.c_int32)))
        out = {k: f[i].copy() for i, k in enumerate(STATE_FLOATS)}
        out.update({k: ints[i].copy() for i, k in enumerate(STATE_INTS)})
        return out


class RTTY_Raster_Skimmer(Skimmer):
    """Wideband IQ at ``fs`` -> a channelizer of M = 4 D rows S baud / 4 apart at S baud samples per second -> NSUB = S
    decoders inside every row, fine row F centred at ``freqs_fine[F]`` Hz (signed; its mark tone at ``freqs_mark[F]``) ->
    the text of the stations, each on the fine row that owns it.  An event's text is the reference's (``rtty.LTRS`` /
    ``rtty.FIGS``); ``text`` leaves out nulls and the two shifts."""
    SILENT = ("\0", "<FIGS>", "<LTRS>")

    def __init__(self, fs, channels=None, device=0, max_in=1 << 22, max_out=256, chan=None):
        self.fs, self.baud = float(fs), BAUD
        if chan is None:
            self.S, self.D, self.M = shape(fs)
            nk = self.M if channels is None else int(channels[1])
            plan(nk, self.S, max_out, params())                          # a bad shape fails here, with or without a device
            self.h = prototype(fs, self.M, self.S)
            self.chan = Channelizer(fs, self.M, self.D, self.h, channels, device, max_in)
        else:
            # a ready channelizer of either kind, adopted and owned: rows S baud / 4 apart at S baud samples per second
            self.chan = chan
            s = chan.fs_out / BAUD
            self.S, self.D, self.M = int(round(s)), chan.D, chan.M
            if abs(s - self.S) > 1e-9 * s or self.S not in SHAPES or chan.M != 4 * chan.D or float(fs) != chan.fs:
                raise ValueError(f"RTTY_Raster_Skimmer: the channelizer's rows (fs {chan.fs}, fs_out {chan.fs_out}, M / D = "
                                 f"{chan.M / chan.D}) are not at 22 or 33 samples per bit of 45.45 baud with M / D = 4 at fs = {fs}")
            self.h = chan.prototypes
        self.nsub = self.S
        self.dec = RTTY_Raster_Decoders(self.chan, self.S, max_out)
        self.nk, self.nfine, self.fs_out = self.chan.nk, self.dec.nfine, self.chan.fs_out
        self.freqs = self.chan.freqs
        q = 2 * np.arange(self.nsub) - self.nsub + 1
        self.freqs_fine = (self.freqs[:, None] + q[None, :] * (BAUD / 8)).reshape(-1)
        self.freqs_mark = self.freqs_fine + TONE_STEPS * BAUD / 8
        self.circular = self.nk == self.M
        self.text = collections.defaultdict(str)
        self.owner = np.zeros(self.nfine, bool)                          # of the last call that completed an output

    def reset(self):
        self.dec.reset()
        self.text = collections.defaultdict(str)
        self.owner[:] = False

    def _events(self, x):
        """one call: the counts and the squelch state come off the device first, then only the owners that have events;
        ownership is decided per call, on the call's end state and the last call's owners"""
        r = self.dec.decode_raw(x, events="counts", squelch=True)
        if r["n_out"] == 0:
            return []
        self.owner = owners(r["qn"], r["open"], self.circular, self.owner)
        rows = np.flatnonzero(self.owner & (r["counts"] > 0))
        if not len(rows):
            return []
        words = self.dec.fetch(rows)
        return [(r["m0"] + j, int(F), code_text(c)) for k, F in enumerate(rows) for j, c in map(unpack, words[k, :r["counts"][F]])]

    def state(self):
        """The decoders' state: the raw fields of ``RTTY_Raster_Decoders.state`` plus contrast = qn / qd (1 for one tone at
        a time, 0.5 for noise), freq = freqs_fine and open as bool, [nfine] each."""
        st = self.dec.state()
        with np.errstate(divide="ignore", invalid="ignore"):
            st["contrast"] = st["qn"].astype(np.float64) / st["qd"].astype(np.float64)
        st["freq"] = self.freqs_fine.copy()
        st["open"] = st["open"].astype(bool)
        return st
