"""ACARS skimmer: an aircraft-message decoder on every row of an airband raster (kernel ``acars.hip``,
host half ``api_acars.hip``).  2400 bit/s MSK -- a bit that equals the one before it is a cycle of 2400 Hz, one that
differs half a cycle of 1200 Hz -- inside the envelope of an AM carrier, on a dozen or so channels of the 118 - 137 MHz
band that differ by region.  A channelizer of either kind delivers rows at any ``fs_out`` from 19200 to 50000 Hz; on every
row the envelope power, a band-pass at +1800 Hz, a differential detector over one bit, a bit clock and the frame machine
(SYN SYN, SOH, odd parity on every character, ETX or ETB, the block check) run on the device.  Only frames that check
completely leave the device.  The host removes the copies of a frame on overlapping neighbour rows and parses the fields.
The tables and settings are derived here, once, and handed to the library already derived.  The reference holds no ACARS
decoder: the definition is our own, and its protocol constants are written from memory (DESIGN.md says which)."""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np
from scipy.signal import firwin

from . import _lib
from ._lib import AcarsCfg
from .channelizer import Channelizer
from .packet import Dedup, near_rows, phase_word, unpack
from .skimmer import DecoderBank, Skimmer

BAUD, CARRIER, CUTOFF = 2400.0, 1800.0, 1500.0
FRAME_WORDS = 60
MIN_BYTES, MAX_BYTES, MAX_TEXT = 13, 238, 220
FS_OUT = (19200.0, 50000.0)
STATE_INTS = ("clk", "xprev", "lev", "sr", "st", "byte", "nb", "nbytes", "crc")
SYN, SOH, STX, ETX, ETB, NAK, DEL = 0x16, 0x01, 0x02, 0x03, 0x17, 0x15, 0x7F


# ---- characters and blocks ----------------------------------------------------------------------------------------------
def parity(data):
    """seven-bit characters -> bytes with bit 7 set so that every byte has an odd number of ones"""
    return bytes((b & 0x7F) | (0 if bin(b & 0x7F).count("1") & 1 else 0x80) for b in bytes(data))


def crc16(data, crc=0):
    """the block check: CRC-16 (reflected 0x1021), initial value 0, over the bytes as sent; 0 behind a block and its check"""
    for b in bytes(data):
        for _ in range(8):
            crc = (crc >> 1) ^ (0x8408 if (crc ^ b) & 1 else 0)
            b >>= 1
    return crc


def block(mode, address, ack, label, block_id, text="", more=False):
    """The bytes between SOH and the block check, parity bits set: mode, seven address characters (the registration,
    right-aligned, filled with '.'), the acknowledgement (a character, or None: NAK), two label characters, the block id,
    STX and the text if there is one, ETX (``more``: ETB).  What the skimmer delivers and ``parse`` reads."""
    text = text.encode("ascii") if isinstance(text, str) else bytes(text)
    address, label = str(address).upper().rjust(7, "."), str(label)
    if len(str(mode)) != 1 or len(address) != 7 or len(label) != 2 or len(str(block_id)) != 1 or len(text) > MAX_TEXT:
        raise ValueError("no ACARS block: one mode character, at most seven of address, two of label, one block id, at most 220 of text")
    ackc = bytes([NAK]) if ack is None else str(ack).encode("ascii")
    if len(ackc) != 1:
        raise ValueError("the acknowledgement is one character or None")
    body = str(mode).encode("ascii") + address.encode("ascii") + ackc + label.encode("ascii") + str(block_id).encode("ascii")
    if any(b > 0x7F for b in body + text):
        raise ValueError("seven-bit characters")
    return parity(body + (bytes([STX]) + text if text else b"") + bytes([ETB if more else ETX]))


def frame(mode, address, ack, label, block_id, text="", more=False, prekey=16):
    """The characters of one transmission, pre-key to DEL: ``prekey`` characters of all ones, '+' '*' for the bit clock,
    SYN SYN, SOH, the block, its check low byte first (no parity rule), DEL."""
    b = block(mode, address, ack, label, block_id, text, more)
    return b"\xff" * int(prekey) + parity(b"+*" + bytes([SYN, SYN, SOH])) + b + int(crc16(b)).to_bytes(2, "little") + parity(bytes([DEL]))


def parse(data):
    """A delivered block -> dict of mode, address (the registration without its fill), ack ('' for NAK), label, block_id,
    more (ETB), msn and flight (downlinks, whose block id is a digit, with a text of ten characters or more; else None)
    and text; None if it is shorter than a block or does not end in ETX / ETB."""
    c = bytes(b & 0x7F for b in bytes(data))
    if len(c) < MIN_BYTES or c[-1] not in (ETX, ETB) or (len(c) > MIN_BYTES and c[12] != STX):
        return None
    s = c.decode("ascii")
    text, msn, flight = s[13:-1], None, None
    if s[11].isdigit() and len(text) >= 10:
        msn, flight, text = text[:4], text[4:10], text[10:]
    return dict(mode=s[0], address=s[1:8].lstrip("."), ack="" if c[8] == NAK else s[8], label=s[9:11], block_id=s[11], more=c[-1] == ETB,
                msn=msn, flight=flight, text=text)


def line(rec):
    """one line of a record; a block that does not parse (``rec`` None) comes out as '?'"""
    if rec is None:
        return "?"
    head = f"{rec['address']:>7} {rec['mode']} {rec['label']} {rec['block_id']} {rec['ack'] or '!'}"
    if rec["msn"] is not None:
        head += f" {rec['msn']} {rec['flight']}"
    text = "".join(ch if " " <= ch <= "~" else "." for ch in rec["text"])
    return head + (" " + text if text else "") + (" +" if rec["more"] else "")


# ---- test signals -------------------------------------------------------------------------------------------------------
def bits(chars):
    """the characters' bits in the order sent, LSB first: uint8 [8 len(chars)]"""
    return np.unpackbits(np.frombuffer(bytes(chars), np.uint8), bitorder="little")


def audio(b, fs, first=1):
    """Continuous-phase MSK of the bits ``b`` at ``fs``: a bit that equals the one before it (``first`` before the first)
    is 2400 Hz, one that differs 1200 Hz.  float64 [len(b) fs / 2400], peak 1"""
    b = np.asarray(b, np.int64)
    same = b == np.concatenate(([int(first)], b[:-1]))
    n = int(np.floor(len(b) * fs / BAUD))
    k = np.minimum((np.arange(n) * BAUD / fs).astype(np.int64), len(b) - 1)
    f = np.where(same[k], 2400.0, 1200.0)
    return np.sin(2 * np.pi * np.cumsum(f) / fs)


def waveform(chars, fs, f0, depth=0.8, prekey=0, invert=False):
    """One transmission (the characters of ``frame``, behind ``prekey`` more characters of pre-key) as an AM carrier of
    amplitude 1 and modulation depth ``depth`` at ``f0`` Hz from the centre of a band sampled at ``fs``: complex64.
    ``invert``: the tone sequence starts from the other level, so that the receiver's bits come out inverted."""
    a = audio(bits(b"\xff" * int(prekey) + bytes(chars)), fs, first=0 if invert else 1)
    return ((1.0 + float(depth) * a) * np.exp(2j * np.pi * float(f0) * np.arange(len(a)) / fs)).astype(np.complex64)


# ---- the bank's tables and settings ---------------------------------------------------------------------------------------
def window_length(fs_out):
    return int(np.floor(float(fs_out) / BAUD + 0.5))


def tables(fs_out):
    """-> (L, tw float32 [1024][2] = (cos, -sin)(2 pi k / 1024), c float32 [4 L + 1][2]: a Kaiser(5.0) low-pass of 1500 Hz
    moved to +1800 Hz, its mean subtracted): derived in float64, rounded once"""
    L = window_length(fs_out)
    t = 2 * np.pi * np.arange(1024) / 1024
    tw = np.stack((np.cos(t), -np.sin(t)), axis=1)
    nt = 4 * L + 1
    c = firwin(nt, CUTOFF, window=("kaiser", 5.0), fs=float(fs_out)) * np.exp(2j * np.pi * CARRIER * (np.arange(nt) - 2 * L) / float(fs_out))
    c = c - c.mean()
    return L, np.ascontiguousarray(tw, np.float32), np.ascontiguousarray(np.stack((c.real, c.imag), axis=1), np.float32)


def params(fs_out, pll_shift=2, pmax=1e18):
    """The settings of DESIGN.md 3 item 32 as the ``_lib.AcarsCfg`` the C ABI takes: the blanking level, the phase words of
    1800 Hz and of the bit clock at ``fs_out``, the clock's pull."""
    return AcarsCfg(pmax=float(np.float32(pmax)), w_car=phase_word(CARRIER, fs_out), w_baud=phase_word(BAUD, fs_out), pll_shift=int(pll_shift))


def cfg_dict(cfg):
    return dict(pmax=cfg.pmax, w_car=cfg.w_car, w_baud=cfg.w_baud, pll_shift=cfg.pll_shift)


def plan(nk, L, max_out, cfg):
    """What a skimmer of this shape launches (no device needed): dict of rows per workgroup, threads, LDS bytes, tile
    samples, event cap (words per decoder and call), workgroups, taps, words of a frame buffer.  Raises PysdrError outside
    the rules."""
    v = _lib.plan_call("pysdr_acars_plan", 8, int(nk), int(L), int(max_out), C.byref(cfg) if cfg is not None else None)
    return {"rows": v[0], "threads": v[1], "lds_bytes": v[2], "tile": v[3], "cap": v[4], "groups": v[5], "taps": v[6], "frame_words": v[7]}


def prototype(fs, M, D):
    """The channelizer's prototype for ACARS rows at fs_out = fs / D: packet's, a Kaiser(8.0) windowed sinc of 32 D taps
    cut at 0.3 fs_out, sum 1: flat to 0.22 fs_out (4.2 kHz at 19.2 kHz rows: the tones' sidebands reach 3.6 kHz), 80 dB
    down from 0.38 fs_out on, so that a station one step away on a raster of fs_out / 2 is not read a second time."""
    return firwin(32 * int(D), 0.3 * float(fs) / int(D), window=("kaiser", 8.0), fs=float(fs))


class ACARS_Decoders(DecoderBank):
    """The decoder bank on a borrowed channelizer of either kind (which it resets, and which must be fed only through it):
    one decoder per row."""
    KIND, DESTROY = "acars", "pysdr_acars_destroy"

    def __init__(self, chan, max_out=4096, cfg=None):
        super().__init__(chan, max_out)
        if not FS_OUT[0] <= self.fs_out <= FS_OUT[1]:
            raise ValueError(f"ACARS_Decoders: rows at {self.fs_out} Hz, outside {FS_OUT}")
        self.L, self.tw, self.c = tables(self.fs_out)
        self.ndec = self.nk
        self.cfg = params(self.fs_out) if cfg is None else cfg
        self.plan = plan(self.nk, self.L, self.max_out, self.cfg)         # a bad shape fails here
        self._open(self.ndec, self.L, C.byref(self.cfg), _lib.as_pf(self.tw), _lib.as_pf(self.c))

    def decode_raw(self, x, n=None, on_device=False, events="all"):
        """One call of the C ABI: host samples (complex64 [n]) or a device pointer.  -> dict of n_out, m0 (the absolute
        index of the call's first output), counts [nk] (event words) and events: every row's slots [nk][cap] ("all") or
        nothing ("counts": the counts alone; None: counts is None too, everything stays on the device and the call only
        queues work when the input is on the device)."""
        return self._decode(x, n, on_device, events)

    def state(self):
        """dict of int32 clk, xprev, lev, sr, st, byte, nb, nbytes, crc [nk] and frames uint32 [nk][60]"""
        ints = np.empty((len(STATE_INTS), self.ndec), np.int32)
        frames = np.empty((self.ndec, FRAME_WORDS), np.uint32)
        self._call("state", ints.ctypes.data_as(C.POINTER(C.c_int32)), frames.ctypes.data_as(C.POINTER(C.c_uint32)))
        out = {k: ints[i].copy() for i, k in enumerate(STATE_INTS)}
        out["frames"] = frames
        return out


class ACARS_Skimmer(Skimmer):
    """Wideband IQ at ``fs`` -> a channelizer of M rows fs / M apart at fs / D samples per second (D = M / 2 by default: a
    12.5 kHz raster gives rows at 25 kHz) -> an ACARS decoder on every row -> the blocks heard, each once.  ``push(x)``
    returns ``(m, row, record)``: m the absolute index of the row output that completed the block check, record what
    ``parse`` makes of the block; ``text[row]`` gains the records' lines, ``frames`` the ``(m, row, bytes)``.  A block is
    final, and returned, once 4 L outputs lie behind it (``flush`` at the end of a stream)."""

    def __init__(self, fs, M=None, D=None, h=None, channels=None, chan=None, max_out=4096, device=0, max_in=1 << 22, cfg=None):
        self.fs = float(fs)
        if chan is None:
            self.M = int(M)
            self.D = self.M // 2 if D is None else int(D)
            fs_out = self.fs / self.D
            if not FS_OUT[0] <= fs_out <= FS_OUT[1]:
                raise ValueError(f"ACARS_Skimmer: rows at {fs_out} Hz, outside {FS_OUT}")
            nk = self.M if channels is None else int(channels[1])
            plan(nk, window_length(fs_out), max_out, params(fs_out) if cfg is None else cfg)   # a bad shape fails here, with or without a device
            self.h = prototype(fs, self.M, self.D) if h is None else np.asarray(h, np.float64)
            self.chan = Channelizer(fs, self.M, self.D, self.h, channels, device, max_in)
        else:
            # a ready channelizer of either kind, adopted and owned
            if float(fs) != chan.fs or not FS_OUT[0] <= chan.fs_out <= FS_OUT[1]:
                raise ValueError(f"ACARS_Skimmer: the channelizer's rows (fs {chan.fs}, fs_out {chan.fs_out}) are not at {FS_OUT} Hz of fs = {fs}")
            self.chan, self.M, self.D, self.h = chan, chan.M, chan.D, chan.prototypes
        self.dec = ACARS_Decoders(self.chan, max_out, cfg)
        self.nk, self.ndec, self.fs_out, self.L = self.chan.nk, self.dec.ndec, self.chan.fs_out, self.dec.L
        self.freqs = self.chan.freqs
        self._start()

    def _start(self):
        self.text = collections.defaultdict(str)
        self.frames = []
        self.dedup = Dedup(4 * self.L, near_rows(self.freqs, self.fs, self.fs_out))

    def reset(self):
        self.dec.reset()
        self._start()

    def _events(self, x):
        """one call: the counts come off the device first, then only the rows that closed a block"""
        r = self.dec.decode_raw(x, events="counts")
        if r["n_out"] == 0:
            return []
        rows = np.flatnonzero(r["counts"] > 0)
        raw = []
        if len(rows):
            words = self.dec.fetch(rows)
            raw = [(r["m0"] + i, int(d), 0, data) for k, d in enumerate(rows) for i, data in unpack(words[k, :r["counts"][d]])]
        return self._keep(self.dedup.add(raw, r["m0"] + r["n_out"]))

    def _keep(self, records):
        out = []
        for m, row, data, _ in records:
            rec = parse(data)
            self.frames.append((m, row, data))
            self.text[row] += line(rec) + "\n"
            out.append((m, row, rec))
        return out

    def push(self, x):
        """complex64 [n] -> the blocks (m, row, record) that became final with this input, in the order they were first
        heard; the input goes through in calls of at most ``dec.max_samples()``."""
        x = np.ascontiguousarray(x, np.complex64)
        ev, i = [], 0
        while i < len(x):
            n = min(len(x) - i, self.dec.max_samples())
            ev += self._events(x[i:i + n])
            i += n
        return ev

    def flush(self):
        """the blocks heard in the last 4 L outputs, at the end of a stream"""
        return self._keep(self.dedup.flush())
