"""SSTV skimmer: a VIS and image decoder on every row of a raster (kernel ``sstv.hip``, host half
``api_sstv.hip``).  Analogue slow-scan television -- the ISS on 145.800 MHz (FM), 14.230 MHz and its neighbours (USB).  A
channelizer of either kind delivers rows at any ``fs_out`` from 8000 to 48000 Hz; on every row a detector, a mixer to the
1900 Hz subcarrier, a low-pass and lag products run on the device, and from their sums the 10 ms tick frequencies, the VIS
match, the anchor on the end of the first sync pulse and the pixels of a free-running line clock.  Pictures leave the
device line by line.  The tables and settings are derived here, once, and handed to the library already derived.  The
reference holds no SSTV decoder: the definition is our own."""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np
from scipy.signal import firwin

from . import _lib
from ._lib import SstvCfg, SstvMode
from .channelizer import Channelizer
from .skimmer import DecoderBank, Skimmer

SUBCARRIER = 1900.0
FS_OUT = (8000.0, 48000.0)
LINE_WORDS = 800
STATE_INTS = ("ticks", "phase", "mode", "m_a", "e0", "line", "pix")
STATE_FLOATS = ("acc_re", "acc_im", "bprev_re", "bprev_im", "f_lead", "pacc_re", "pacc_im")
DETECTORS = {"FM": 0, "USB": 1}
KINDS = {1: "start", 2: "line", 3: "end"}

Mode = collections.namedtuple("Mode", "name code scans width lines sync porch pixel sep colour")
Mode.__doc__ = """A mode as data: VIS code, scans of a sent line, pixels of a scan, sent lines, and the times in ms of the sync
pulse, the porch, one pixel and the separator behind every scan; ``colour`` names what the scans carry ("PD": Y0, R-Y,
B-Y, Y1, two picture lines per sent line; "GBR"; anything else: the scans as they are)."""


def _pd(name, code, pixel, width, height):
    return Mode(name, code, 4, width, height // 2, 20.0, 2.08, pixel, 0.0, "PD")


MODES = (
    _pd("PD50", 93, 0.286, 320, 256), _pd("PD90", 99, 0.532, 320, 256), _pd("PD120", 95, 0.19, 640, 496),
    _pd("PD160", 98, 0.382, 512, 400), _pd("PD180", 96, 0.286, 640, 496), _pd("PD240", 97, 0.382, 640, 496),
    _pd("PD290", 94, 0.286, 800, 616),
    Mode("Martin M1", 44, 3, 320, 256, 4.862, 0.572, 0.4576, 0.572, "GBR"),
    Mode("Martin M2", 40, 3, 320, 256, 4.862, 0.572, 0.2288, 0.572, "GBR"),
)


def mode_named(name, modes=MODES):
    return next(m for m in modes if m.name == name)


def line_ms(mode):
    return mode.sync + mode.porch + mode.scans * (mode.pixel * mode.width + mode.sep)


# ---- test signals -----------------------------------------------------------------------------------------------------
def vis_tones(code, parity_error=False):
    """the header as (Hz, ms): leader, break, leader, start bit, seven data bits LSB first (1100 Hz: 1, 1300 Hz: 0), even
    parity, stop bit"""
    bits = [code >> k & 1 for k in range(7)]
    bits.append((sum(bits) & 1) ^ (1 if parity_error else 0))
    return [(1900.0, 300.0), (1200.0, 10.0), (1900.0, 300.0), (1200.0, 30.0)] + [(1100.0 if b else 1300.0, 30.0) for b in bits] + [(1200.0, 30.0)]


def tones(mode, scans, header=True):
    """Header and picture as (Hz, ms) pairs.  ``scans``: uint8 [sent lines][mode.scans][mode.width], 0 = 1500 Hz, 255 =
    2300 Hz; fewer lines than the mode's send the top of the picture."""
    scans = np.asarray(scans)
    if scans.ndim != 3 or scans.shape[1:] != (mode.scans, mode.width) or scans.shape[0] > mode.lines:
        raise ValueError(f"scans {scans.shape} are not [<= {mode.lines}][{mode.scans}][{mode.width}]")
    out = vis_tones(mode.code) if header else []
    for ln in scans:
        out += [(1200.0, mode.sync), (1500.0, mode.porch)]
        for sc in ln:
            out += [(1500.0 + 800.0 * float(v) / 255.0, mode.pixel) for v in sc]
            if mode.sep:
                out.append((1500.0, mode.sep))
    return out


def audio_phase(tone_list, fs):
    """the audio's phase in radians at fs, continuous through every change of tone: float64 [floor(total ms fs / 1000)]"""
    f = np.array([t[0] for t in tone_list], np.float64)
    ends = np.cumsum([t[1] for t in tone_list]) * 1e-3
    n = int(np.floor(ends[-1] * fs + 1e-9))
    seg = np.minimum(np.searchsorted(ends, (np.arange(n) + 0.5) / fs, side="right"), len(f) - 1)
    return 2 * np.pi * np.cumsum(f[seg]) / fs


def audio(tone_list, fs):
    """the real audio, unit amplitude"""
    return np.cos(audio_phase(tone_list, fs))


def waveform(tone_list, fs, f0, det="FM", deviation=3000.0):
    """One transmission at ``f0`` Hz from the centre of a band sampled at ``fs``, complex64 of unit amplitude.  FM: the
    carrier at f0, peak deviation ``deviation`` Hz.  USB: f0 is where 1900 Hz of audio lands, the dial 1900 Hz below."""
    n = np.arange(len(audio_phase(tone_list, fs)))
    if det == "FM":
        ph = 2 * np.pi * float(deviation) * np.cumsum(audio(tone_list, fs)) / fs + 2 * np.pi * float(f0) * n / fs
    elif det == "USB":
        ph = audio_phase(tone_list, fs) + 2 * np.pi * (float(f0) - SUBCARRIER) * n / fs
    else:
        raise ValueError(f"det {det!r}")
    return np.exp(1j * ph).astype(np.complex64)


def to_rgb(mode, lines):
    """uint8 [sent lines][scans][width] -> the picture uint8 [rows][width][3]: YCbCr (BT.601, full range) for the PD family,
    two rows per sent line; G, B, R for Martin; the first scan as grey otherwise"""
    a = np.asarray(lines, np.float64)
    if mode.colour == "PD":
        y = np.stack((a[:, 0], a[:, 3]), axis=1).reshape(-1, a.shape[2])
        cr, cb = np.repeat(a[:, 1], 2, axis=0) - 128.0, np.repeat(a[:, 2], 2, axis=0) - 128.0
        rgb = np.stack((y + 1.402 * cr, y - 0.344136 * cb - 0.714136 * cr, y + 1.772 * cb), axis=-1)
    elif mode.colour == "GBR":
        rgb = np.stack((a[:, 2], a[:, 0], a[:, 1]), axis=-1)
    else:
        rgb = np.repeat(a[:, 0, :, None], 3, axis=-1)
    return np.clip(np.floor(rgb + 0.5), 0, 255).astype(np.uint8)


# ---- the bank's tables and settings ---------------------------------------------------------------------------------
def filter_length(fs_out):
    return 2 * int(np.floor(0.75 * float(fs_out) / 1000.0)) + 1


def tables(fs_out):
    """-> (L, tw float32 [1024][2] = (cos, -sin)(2 pi k / 1024), g float32 [L]: Hamming-windowed sinc cut at 1900 Hz, sum 1):
    derived in float64, rounded once"""
    L = filter_length(fs_out)
    t = 2 * np.pi * np.arange(1024) / 1024
    tw = np.stack((np.cos(t), -np.sin(t)), axis=1)
    g = firwin(L, SUBCARRIER, window="hamming", fs=float(fs_out))
    return L, np.ascontiguousarray(tw, np.float32), np.ascontiguousarray(g, np.float32)


def phase_word(f, fs_out):
    return int(round(float(f) / float(fs_out) * 2.0 ** 32)) & 0xFFFFFFFF


def _q16(ms, fs_out):
    return int(round(float(ms) * 1e-3 * float(fs_out) * 65536.0))


def params(fs_out, det="FM", modes=MODES, offset=0.0, pmax=1e18):
    """The settings of DESIGN.md 3 item 30 as the ``_lib.SstvCfg`` the C ABI takes.  ``det``: "FM" (the subcarrier at 1900 Hz
    of the discriminator's output) or "USB" (the subcarrier at the row's centre, or ``offset`` Hz above it)."""
    if len(modes) > 16:
        raise ValueError("at most 16 modes")
    fs_out = float(fs_out)
    R0, W = int(round(0.010 * fs_out)), int(round(fs_out / 500.0))
    c = SstvCfg(det=DETECTORS[det], nmodes=len(modes), w_sub=phase_word((SUBCARRIER if det == "FM" else 0.0) + offset, fs_out),
                w_tick=phase_word(100.0, fs_out), k_hz=float(np.float32(fs_out / (2 * np.pi))), k_rho=float(np.float32(1024.0 / fs_out)),
                pmax=float(np.float32(pmax)), W=W, R0=R0, lag=2 * R0 + W + 1)
    for i, m in enumerate(modes):
        c.modes[i] = SstvMode(code=m.code, scans=m.scans, width=m.width, lines=m.lines, sync_q=_q16(m.sync, fs_out),
                              porch_q=_q16(m.porch, fs_out), scan_q=_q16(m.pixel * m.width, fs_out), sep_q=_q16(m.sep, fs_out))
    return c


def cfg_dict(cfg):
    d = {k: getattr(cfg, k) for k in ("det", "nmodes", "w_sub", "w_tick", "k_hz", "k_rho", "pmax", "W", "R0", "lag")}
    d["modes"] = [{k: getattr(cfg.modes[i], k) for k in ("code", "scans", "width", "lines", "sync_q", "porch_q", "scan_q", "sep_q")}
                  for i in range(cfg.nmodes)]
    return d


def plan(nk, L, max_out, cfg):
    """What a skimmer of this shape launches (no device needed): dict of rows per workgroup, threads, LDS bytes, tile
    samples, event cap (words per row and call), workgroups, history samples, words of a line buffer.  Raises PysdrError
    outside the rules."""
    v = _lib.plan_call("pysdr_sstv_plan", 8, int(nk), int(L), int(max_out), C.byref(cfg) if cfg is not None else None)
    return {"rows": v[0], "threads": v[1], "lds_bytes": v[2], "tile": v[3], "cap": v[4], "groups": v[5], "history": v[6], "line_words": v[7]}


def unpack(words, modes=MODES):
    """A row's event words of one call -> records ``(i, "start", mode index, code, f_lead, e0)``, ``(i, "line", number,
    uint8 [scans][width])`` and ``(i, "end", lines)``; i the index within the call.  A line's shape is that of the mode
    of the start before it: ``Unpacker`` keeps it for a stream cut into calls."""
    return Unpacker(modes).feed(words)


class Unpacker:
    """``unpack`` for one row over many calls: remembers the mode of the picture that runs"""

    def __init__(self, modes=MODES, mode=None):
        self.modes, self.mode = modes, mode

    def feed(self, words):
        w = np.ascontiguousarray(words, np.int32).view(np.uint32)
        out, at = [], 0
        while at < len(w):
            i, kind, nw = int(w[at]) >> 12, int(w[at]) >> 10 & 3, int(w[at]) & 1023
            p = w[at + 1:at + 1 + nw]
            if kind == 1:
                self.mode = self.modes[int(p[0])]
                out.append((i, "start", int(p[0]), int(p[1]), float(p[2:3].view(np.float32)[0]), int(p[3])))
            elif kind == 2:
                m = self.mode
                data = p[1:].astype("<u4").view(np.uint8)[:m.scans * m.width].reshape(m.scans, m.width).copy()
                out.append((i, "line", int(p[0]), data))
            else:
                out.append((i, "end", int(p[0])))
            at += 1 + nw
        return out


def prototype(fs, M, D, det="FM"):
    """The channelizer's prototype for SSTV rows at fs_out = fs / D: Kaiser(8.0) windowed sinc of 32 D taps, sum 1, flat to
    0.08 fs_out below its cut and 80 dB down 0.08 fs_out above it.  USB: cut at 0.3 fs_out (12 kHz rows: the 800 Hz either
    side of the subcarrier with room for a station off tune).  FM: the row has to pass the whole transmission -- deviation
    3 kHz plus tones to 2.3 kHz, 5.3 kHz either side by Carson's rule -- so the cut is 6 kHz where 0.3 fs_out is less,
    though never above 0.38 fs_out (no aliasing): 16 kHz rows are cut at 6 kHz, 25 kHz rows at 7.5 kHz.  With a cut of
    4.8 kHz at 16 kHz rows half the headers at 20 dB C/N were lost to clicks (LABNOTES 35)."""
    fs_out = float(fs) / int(D)
    cut = 0.3 * fs_out if det != "FM" else max(0.3 * fs_out, min(6000.0, 0.38 * fs_out))
    return firwin(32 * int(D), cut, window=("kaiser", 8.0), fs=float(fs))


class SSTV_Decoders(DecoderBank):
    """The decoder bank on a borrowed channelizer of either kind (which it resets, and which must be fed only through it):
    one decoder per row."""
    KIND, DESTROY = "sstv", "pysdr_sstv_destroy"

    def __init__(self, chan, max_out=4096, cfg=None, det="FM", modes=MODES):
        super().__init__(chan, max_out)
        if not FS_OUT[0] <= self.fs_out <= FS_OUT[1]:
            raise ValueError(f"SSTV_Decoders: rows at {self.fs_out} Hz, outside {FS_OUT}")
        self.L, self.tw, self.g = tables(self.fs_out)
        self.modes = tuple(modes)
        self.cfg = params(self.fs_out, det, self.modes) if cfg is None else cfg
        self.plan = plan(self.nk, self.L, self.max_out, self.cfg)         # a bad shape fails here
        self._open(self.nk, self.L, C.byref(self.cfg), _lib.as_pf(self.tw), _lib.as_pf(self.g))

    def decode_raw(self, x, n=None, on_device=False, events="all"):
        """One call of the C ABI: host samples (complex64 [n]) or a device pointer.  -> dict of n_out, m0 (the absolute
        index of the call's first output), counts [nk] (event words) and events: every row's slots [nk][cap] ("all") or
        nothing ("counts": the counts alone; None: counts is None too, everything stays on the device and the call only
        queues work when the input is on the device)."""
        return self._decode(x, n, on_device, events)

    def state(self):
        """dict of int32 ticks, phase, mode, m_a, e0, line, pix [nk], float32 acc_re .. pacc_im [nk], ring float32 [nk][64]
        and lines uint32 [nk][800]"""
        ints = np.empty((len(STATE_INTS), self.nk), np.int32)
        fl = np.empty((len(STATE_FLOATS), self.nk), np.float32)
        ring = np.empty((self.nk, 64), np.float32)
        lines = np.empty((self.nk, LINE_WORDS), np.uint32)
        self._call("state", ints.ctypes.data_as(C.POINTER(C.c_int32)), _lib.as_pf(fl), _lib.as_pf(ring), lines.ctypes.data_as(C.POINTER(C.c_uint32)))
        out = {k: ints[i].copy() for i, k in enumerate(STATE_INTS)}
        out.update({k: fl[i].copy() for i, k in enumerate(STATE_FLOATS)})
        out["ring"], out["lines"] = ring, lines
        return out


class SSTV_Skimmer(Skimmer):
    """Wideband IQ at ``fs`` -> a channelizer of M rows fs / M apart at fs / D samples per second (D = M / 2 by default)
    -> an SSTV decoder on every row -> pictures.  ``push(x)`` returns records ``(m, row, "start", mode name, code, f_lead,
    e0)``, ``(m, row, "line", number, uint8 [scans][width])`` and ``(m, row, "end", lines)``, m the absolute index of the
    row output that completed the record; ``images[row]`` (uint8 [sent lines so far][scans][width], ``mode_of[row]`` its
    mode) grows line by line, and ``pictures`` gains ``(row, mode, lines)`` at every end.  ``det``: "FM" or "USB"."""

    def __init__(self, fs, M=None, D=None, h=None, channels=None, chan=None, max_out=4096, device=0, max_in=1 << 22, cfg=None, det="FM",
                 modes=MODES):
        self.fs = float(fs)
        if chan is None:
            self.M = int(M)
            self.D = self.M // 2 if D is None else int(D)
            fs_out = self.fs / self.D
            if not FS_OUT[0] <= fs_out <= FS_OUT[1]:
                raise ValueError(f"SSTV_Skimmer: rows at {fs_out} Hz, outside {FS_OUT}")
            nk = self.M if channels is None else int(channels[1])
            plan(nk, filter_length(fs_out), max_out, params(fs_out, det, modes) if cfg is None else cfg)   # with or without a device
            self.h = prototype(fs, self.M, self.D, det) if h is None else np.asarray(h, np.float64)
            self.chan = Channelizer(fs, self.M, self.D, self.h, channels, device, max_in)
        else:
            # a ready channelizer of either kind, adopted and owned
            if float(fs) != chan.fs or not FS_OUT[0] <= chan.fs_out <= FS_OUT[1]:
                raise ValueError(f"SSTV_Skimmer: the channelizer's rows (fs {chan.fs}, fs_out {chan.fs_out}) are not at {FS_OUT} Hz of fs = {fs}")
            self.chan, self.M, self.D, self.h = chan, chan.M, chan.D, chan.prototypes
        self.dec = SSTV_Decoders(self.chan, max_out, cfg, det, modes)
        self.nk, self.fs_out, self.L, self.modes = self.chan.nk, self.chan.fs_out, self.dec.L, self.dec.modes
        self.freqs = self.chan.freqs
        self._start()

    def _start(self):
        self.images, self.mode_of, self.pictures = {}, {}, []
        self._unpack = [Unpacker(self.modes) for _ in range(self.nk)]

    def reset(self):
        self.dec.reset()
        self._start()

    def _events(self, x):
        """one call: the counts come off the device first, then only the rows that have events"""
        r = self.dec.decode_raw(x, events="counts")
        if r["n_out"] == 0:
            return []
        rows = np.flatnonzero(r["counts"] > 0)
        out = []
        if len(rows):
            words = self.dec.fetch(rows)
            for k, row in enumerate(rows):
                row = int(row)
                for rec in self._unpack[row].feed(words[k, :r["counts"][row]]):
                    m = r["m0"] + rec[0]
                    if rec[1] == "start":
                        mode = self.modes[rec[2]]
                        self.mode_of[row] = mode
                        self.images[row] = np.zeros((0, mode.scans, mode.width), np.uint8)
                        out.append((m, row, "start", mode.name) + rec[3:])
                    elif rec[1] == "line":
                        self.images[row] = np.concatenate((self.images[row], rec[3][None]), axis=0)
                        out.append((m, row) + rec[1:])
                    else:
                        self.pictures.append((row, self.mode_of[row], self.images[row]))
                        out.append((m, row) + rec[1:])
        out.sort(key=lambda e: (e[0], e[1]))
        return out

    def push(self, x):
        """complex64 [n] -> the records of the outputs this input completes, sorted by (m, row); the input goes through in
        calls of at most ``dec.max_samples()``."""
        x = np.ascontiguousarray(x, np.complex64)
        ev, i = [], 0
        while i < len(x):
            n = min(len(x) - i, self.dec.max_samples())
            ev += self._events(x[i:i + n])
            i += n
        return ev
