"""CW skimmer: a Morse decoder on every channel of a raster (kernel ``cw.hip``, host half
``api_cw.hip``).  A ``Channelizer`` delivers the rows; every row then gets one decoder that works on the power of the
row's complex samples -- no audio, no BFO, no AF filter -- and emits ``(output index, row, text)`` events.  The settings
hold for the whole bank; they are derived here, once, and handed to the library already derived."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import CwCfg
from .channelizer import Channelizer
from .skimmer import DecoderBank, Skimmer

WORD_SPACE = 256
STATE_INTS = ("key", "run", "dot", "last", "code", "nel", "sp", "seen")

_ELEMENTS = {
    "A": ".-", "B": "-...", "C": "-.-.", "D": "-..", "E": ".", "F": "..-.", "G": "--.", "H": "....", "I": "..", "J": ".---",
    "K": "-.-", "L": ".-..", "M": "--", "N": "-.", "O": "---", "P": ".--.", "Q": "--.-", "R": ".-.", "S": "...", "T": "-",
    "U": "..-", "V": "...-", "W": ".--", "X": "-..-", "Y": "-.--", "Z": "--..",
    "0": "-----", "1": ".----", "2": "..---", "3": "...--", "4": "....-", "5": ".....", "6": "-....", "7": "--...",
    "8": "---..", "9": "----.",
    "/": "-..-.", "?": "..--..", "=": "-...-", ".": ".-.-.-", ",": "--..--",
}


def _code_of(elements):
    """the element string behind a leading 1: a dot appends 0, a dash appends 1"""
    c = 1
    for e in elements:
        c = 2 * c + (1 if e == "-" else 0)
    return c


MORSE = {_code_of(e): ch for ch, e in _ELEMENTS.items()}      # code -> character (International Morse)


def code_text(code):
    """The text of an event's code: the character, ' ' for a word space, '*' for anything the table does not hold (0: more
    than 7 elements)."""
    code = int(code)
    return " " if code == WORD_SPACE else MORSE.get(code, "*")


def unpack(word):
    """event word -> (index within the call, code)"""
    w = int(word) & 0xFFFFFFFF
    return w >> 9, w & 511


def settle_samples(ntaps, D, fs_out):
    """The settling samples n0 behind a channelizer whose prototype has ``ntaps`` taps: the outputs its run-in reaches plus
    20 ms, four time constants of the envelope."""
    return -(-int(ntaps) // int(D)) + int(np.ceil(0.02 * float(fs_out)))


def params(fs_out, wpm0=20, settle=1, snr_min=16.0, hi=2.0, lo=0.5, fl=1.0 / 64, wpm_min=5, wpm_max=60):
    """The settings of DESIGN.md 3 item 18 for channels at ``fs_out`` samples per second, as the ``_lib.CwCfg`` the C ABI
    takes: float32 smoothing constants of 5 ms (envelope), 1.5 s (peak decay) and 0.25 s (noise floor), dot lengths in
    1 / 16 sample, ``settle`` settling samples (1: the floor is seeded by the first sample alone)."""
    R = float(fs_out)
    def f(v):                                        # the float32 nearest to v, as the Python float ctypes takes
        return float(np.float32(v))

    return CwCfg(a_s=f(min(1.0, 1.0 / (0.005 * R))), a_p=f(min(1.0, 1.0 / (1.5 * R))), a_n=f(min(1.0, 1.0 / (0.25 * R))),
                 snr_min=f(snr_min), hi=f(hi), lo=f(lo), fl=f(fl),
                 d0=int(round(16 * R * 1.2 / wpm0)), dmin=max(16, int(round(16 * R * 1.2 / wpm_max))),
                 dmax=int(round(16 * R * 1.2 / wpm_min)), n0=int(settle))


def cfg_dict(cfg):
    return {k: getattr(cfg, k) for k, _ in CwCfg._fields_}


def plan(nk, max_out, cfg):
    """What a skimmer of this shape launches (no device needed): dict of rows per workgroup, threads, LDS bytes, tile
    samples, event cap per channel and call, workgroups.  Raises PysdrError outside the rules."""
    v = _lib.plan_call("pysdr_cw_plan", 8, int(nk), int(max_out), C.byref(cfg) if cfg is not None else None)
    return {"rows": v[0], "threads": v[1], "lds_bytes": v[2], "tile": v[3], "cap": v[4], "groups": v[5]}


def fine_channelizer(fs, band, fs_out, device=0, max_in=1 << 22):
    """A ``fine.FineChannelizer`` for ``CW_Skimmer(fs, chan=...)``: rows at ``fs_out`` samples per second, fs_out / 2 apart
    (M2 / D2 = 2), whose centres lie in ``band = (f_lo, f_hi)`` Hz from the centre; default prototypes."""
    from . import fine
    M1, D1, M2, D2 = fine.shape(fs, fs_out, 2)
    return fine.FineChannelizer(fs, M1, M2, D1, D2, channels=fine.channels_for(band, fs, M1, D1, M2), device=device, max_in=max_in)


def morse_keying(text, wpm, fs):
    """0 / 1 keying waveform (float32) of ``text`` at ``wpm`` words per minute and ``fs`` samples per second, timing
    1 : 3 : 1 : 3 : 7 (dot, dash, gap between elements, between characters, between words); a dot lasts 1.2 / wpm s.
    Characters the table does not hold are skipped.  The waveform ends with the last mark."""
    unit = 1.2 / float(wpm) * float(fs)
    marks, t = [], 0                                   # (start, end) in dot units
    words = text.upper().split(" ")
    for wi, word in enumerate(words):
        first = True
        for ch in word:
            el = _ELEMENTS.get(ch)
            if el is None:
                continue
            if not first:
                t += 3
            first = False
            for ei, e in enumerate(el):
                if ei:
                    t += 1
                n = 3 if e == "-" else 1
                marks.append((t, t + n))
                t += n
        if wi + 1 < len(words):
            t += 7
    k = np.zeros(int(round(t * unit)), np.float32)
    for a, b in marks:
        k[int(round(a * unit)):int(round(b * unit))] = 1.0
    return k


class CW_Decoders(DecoderBank):
    """The decoder bank on a borrowed ``Channelizer`` (which it resets, and which must be fed only through it)."""
    KIND, DESTROY = "cw", "pysdr_cw_destroy"

    def __init__(self, chan, wpm0=20, max_out=1024, cfg=None):
        super().__init__(chan, max_out)
        self.cfg = params(self.fs_out, wpm0, settle_samples(chan.run_in_taps, self.D, self.fs_out)) if cfg is None else cfg
        self.plan = plan(self.nk, self.max_out, self.cfg)               # a bad shape fails here
        self._open(self.nk, C.byref(self.cfg))

    def decode_raw(self, x, n=None, on_device=False, events="all"):
        """One call of the C ABI: host samples (complex64 [n]) or a device pointer.  -> dict of n_out, m0 (the absolute
        index of the call's first output), counts [nk] and events: every row's slots [nk][cap] ("all"), a dict
        {row: words} of the rows that have events, downloaded after the counts ("rows"), or nothing (None: counts is None
        too, everything stays on the device and the call only queues work when the input is on the device)."""
        out = self._decode(x, n, on_device, events)
        if events == "rows":
            counts = out["counts"]
            rows = np.flatnonzero(counts)
            words = self.fetch(rows) if len(rows) else np.zeros((0, self.cap), np.int32)
            out["events"] = {int(r): words[i, :counts[r]].copy() for i, r in enumerate(rows)}
        return out

    def state(self):
        """dict of float32 [nk] s, pk, nf and int32 [nk] key, run, dot, last, code, nel, sp, seen"""
        out = {k: np.empty(self.nk, np.float32) for k in ("s", "pk", "nf")}
        ints = np.empty((self.nk, 8), np.int32)
        self._call("state", _lib.as_pf(out["s"]), _lib.as_pf(out["pk"]), _lib.as_pf(out["nf"]), ints.ctypes.data_as(C.POINTER(C.c_int32)))
        for i, k in enumerate(STATE_INTS):
            out[k] = ints[:, i].copy()
        return out


class CW_Skimmer(Skimmer):
    """Wideband IQ at ``fs`` -> the channelizer's raster of M channels (row a at ``freqs[a]`` Hz, ``fs / D`` samples per
    second each) -> one Morse decoder per row, without taking the rows off the device."""

    def __init__(self, fs, M=None, D=None, h=None, channels=None, wpm0=20, device=0, max_in=1 << 22, max_out=1024, chan=None):
        if chan is None:
            nk = int(M) if channels is None else int(channels[1])
            D_ = int(M) // 2 if D is None else int(D)
            plan(nk, max_out, params(float(fs) / D_, wpm0))              # a bad shape fails here, with or without a device
            self.chan = Channelizer(fs, M, D, h, channels, device, max_in)
        else:
            self.chan = chan                                             # a ready channelizer of either kind, adopted and owned
        self.dec = CW_Decoders(self.chan, wpm0, max_out)
        self.fs, self.M, self.D, self.nk = self.chan.fs, self.chan.M, self.chan.D, self.chan.nk
        self.freqs, self.fs_out = self.chan.freqs, self.chan.fs_out
        self.text = {a: "" for a in range(self.nk)}

    def reset(self):
        self.dec.reset()
        self.text = {a: "" for a in range(self.nk)}

    def _events(self, x):
        """one call: the counts come off the device first, then only the rows that have events"""
        r = self.dec.decode_raw(x, events="rows")
        return [(r["m0"] + j, row, code_text(c)) for row, words in r["events"].items() for j, c in map(unpack, words)]

    def state(self):
        """The decoders' state: the raw fields of ``CW_Decoders.state`` plus wpm = 19.2 fs_out / dot, snr_db =
        10 log10(pk / nf) and key as bool, [nk] each."""
        st = self.dec.state()
        with np.errstate(divide="ignore", invalid="ignore"):
            st["wpm"] = 19.2 * self.fs_out / st["dot"].astype(np.float64)
            st["snr_db"] = 10.0 * np.log10(st["pk"].astype(np.float64) / st["nf"].astype(np.float64))
        st["key"] = st["key"].astype(bool)
        return st
