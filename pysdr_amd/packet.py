"""Packet skimmer: an AX.25 decoder on every row of an NFM raster (kernel ``pkt.hip``, host half
``api_pkt.hip``).  1200 baud AFSK on narrow-band FM -- APRS on 144.390 and 144.800 MHz, the ISS and the satellite
digipeaters on 145.825 MHz.  A channelizer of either kind delivers rows at any ``fs_out`` from 9600 to 48000 Hz; on every
row a discriminator, a mark and a space tone filter over one bit and eight slicers run on the device, each slicer with a
bit clock, an HDLC receiver, the CRC and a frame buffer of its own.  Only frames with a good FCS leave the device.  The
host removes the copies of a frame (a row's other slicers, the neighbour rows that overlap it) and prints TNC2 lines.  The
tables and settings are derived here, once, and handed to the library already derived.  The reference holds no packet
decoder: the definition is our own."""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np
from scipy.signal import firwin

from . import _lib
from ._lib import PktCfg
from .channelizer import Channelizer
from .skimmer import DecoderBank, Skimmer

BAUD, MARK, SPACE = 1200.0, 1200.0, 2200.0
SLICERS = 8
FRAME_WORDS = 83
FS_OUT = (9600.0, 48000.0)
STATE_INTS = ("clk", "xprev", "xlast", "sr", "ones", "inframe", "byte", "nb", "nbytes", "crc")


# ---- AX.25 ------------------------------------------------------------------------------------------------------------
def crc_register(data, crc=0xFFFF):
    """the CRC-16 of AX.25 (reflected 0x1021) as the receiver runs it: no final inversion; 0xF0B8 behind a frame and its FCS"""
    for b in bytes(data):
        for _ in range(8):
            crc = (crc >> 1) ^ (0x8408 if (crc ^ b) & 1 else 0)
            b >>= 1
    return crc


def crc16(data):
    """CRC-16/X-25: ``crc16(b"123456789") == 0x906E``; a frame's FCS, sent low byte first"""
    return crc_register(data) ^ 0xFFFF


def fcs(frame):
    return int(crc16(frame)).to_bytes(2, "little")


def _address(call, last):
    call = call.strip().upper()
    h = call.endswith("*")
    name, _, ssid = call.rstrip("*").partition("-")
    ssid = int(ssid) if ssid else 0
    if not 1 <= len(name) <= 6 or not 0 <= ssid <= 15 or not name.isascii():
        raise ValueError(f"no AX.25 address: {call!r}")
    return bytes(ord(c) << 1 for c in name.ljust(6)) + bytes([0x60 | ssid << 1 | (0x80 if h else 0) | (1 if last else 0)])


def ax25_frame(dest, src, path=(), info=b"", control=3, pid=0xF0):
    """The bytes of a frame without its FCS: addresses (calls shifted left by one, SSID byte 0x60 | ssid << 1, H bit 0x80
    for a digipeater written with a trailing ``*``, the extension bit on the last address), control, PID (None: none) and
    info.  15 to 330 bytes are what the skimmer reads."""
    calls = [dest, src, *path]
    if len(calls) > 10:
        raise ValueError("at most 8 digipeaters")
    out = b"".join(_address(c, i == len(calls) - 1) for i, c in enumerate(calls)) + bytes([control])
    if pid is not None:
        out += bytes([pid])
    return out + (info.encode("latin-1") if isinstance(info, str) else bytes(info))


def _call(a):
    name = "".join(chr(b >> 1) for b in a[:6]).rstrip()
    ssid = a[6] >> 1 & 15
    return (name + (f"-{ssid}" if ssid else "")), bool(a[6] & 0x80)


def ax25_parse(frame):
    """-> dict of dest, src, path (digipeaters, a trailing ``*`` where the H bit is set), control, pid (None if the frame
    ends behind the control byte) and info; None if the address field is not one."""
    frame = bytes(frame)
    calls, at = [], 0
    while True:
        a = frame[at:at + 7]
        if len(a) < 7 or len(calls) == 10 or any(b & 1 for b in a[:6]):
            return None
        calls.append(_call(a))
        at += 7
        if a[6] & 1:
            break
    if len(calls) < 2 or at >= len(frame):
        return None
    path = tuple(c + ("*" if h else "") for c, h in calls[2:])
    return dict(dest=calls[0][0], src=calls[1][0], path=path, control=frame[at], pid=frame[at + 1] if at + 1 < len(frame) else None,
                info=frame[at + 2:])


def tnc2(frame):
    """``"N0CALL-7>APRS,WIDE1-1*:info"``: the star behind the last digipeater that has repeated the frame; a frame whose
    address field does not parse comes out as hex."""
    p = ax25_parse(frame)
    if p is None:
        return "?" + bytes(frame).hex()
    used = [i for i, c in enumerate(p["path"]) if c.endswith("*")]
    path = [c.rstrip("*") + ("*" if used and i == used[-1] else "") for i, c in enumerate(p["path"])]
    return f"{p['src']}>{','.join([p['dest'], *path])}:{p['info'].decode('latin-1')}"


# ---- test signals -----------------------------------------------------------------------------------------------------
def hdlc_bits(frame, flags=(30, 3)):
    """The line's levels, one per bit (1: mark, 0: space), of ``flags[0]`` flags, the frame and its FCS LSB first with a 0
    stuffed behind every five 1s, and ``flags[1]`` flags, NRZI (a 0 is a change of tone).  A list of frames goes out with
    one flag between neighbours."""
    frames = [frame] if isinstance(frame, (bytes, bytearray)) else list(frame)
    flag = [0, 1, 1, 1, 1, 1, 1, 0]
    bits = flag * flags[0]
    for k, f in enumerate(frames):
        ones = 0
        for b in bytes(f) + fcs(f):
            for i in range(8):
                bit = b >> i & 1
                bits.append(bit)
                ones = ones + 1 if bit else 0
                if ones == 5:
                    bits.append(0)
                    ones = 0
        bits += flag * (flags[1] if k == len(frames) - 1 else 1)
    level, out = 1, []
    for b in bits:
        if not b:
            level ^= 1
        out.append(level)
    return np.array(out, np.uint8)


def afsk_audio(bits, fs, preemph=1.0):
    """Continuous-phase AFSK of the levels ``bits`` at ``fs``: 1200 Hz for a 1, 2200 Hz for a 0, the 2200 Hz tone at
    ``preemph`` times the 1200 Hz tone's amplitude, the stronger of the two at 1.  float64 [len(bits) fs / 1200]"""
    n = int(np.floor(len(bits) * fs / BAUD))
    lv = np.asarray(bits)[np.minimum((np.arange(n) * BAUD / fs).astype(np.int64), len(bits) - 1)]
    f = np.where(lv == 1, MARK, SPACE)
    a = np.where(lv == 1, 1.0, float(preemph)) / max(1.0, float(preemph))
    ph = 2 * np.pi * np.cumsum(f) / fs
    return a * np.sin(ph)


def waveform(frame, fs, f0, deviation=3000.0, preemph=1.0, flags=(30, 3)):
    """One transmission (or a list of frames in one) as narrow-band FM at ``f0`` Hz from the centre of a band sampled at
    ``fs``: complex64, unit amplitude, peak deviation ``deviation`` Hz."""
    a = afsk_audio(hdlc_bits(frame, flags), fs, preemph)
    ph = 2 * np.pi * float(deviation) * np.cumsum(a) / fs + 2 * np.pi * float(f0) * np.arange(len(a)) / fs
    return np.exp(1j * ph).astype(np.complex64)


# ---- the bank's tables and settings ---------------------------------------------------------------------------------
def window_length(fs_out):
    return int(np.floor(float(fs_out) / BAUD + 0.5))


def tables(fs_out):
    """-> (L, tw float32 [1024][2] = (cos, -sin)(2 pi k / 1024), g float32 [L] = 1 / L): derived in float64, rounded once"""
    L = window_length(fs_out)
    t = 2 * np.pi * np.arange(1024) / 1024
    tw = np.stack((np.cos(t), -np.sin(t)), axis=1)
    return L, np.ascontiguousarray(tw, np.float32), np.full(L, 1.0 / L).astype(np.float32)


def phase_word(f, fs_out):
    return int(round(float(f) / float(fs_out) * 2.0 ** 32))


def params(fs_out, gain=None, pll_shift=2, pmax=1e18):
    """The settings of DESIGN.md 3 item 29 as the ``_lib.PktCfg`` the C ABI takes: the slicers' gains (default -6 to +8 dB
    of power in steps of 2 dB), the three phase words at ``fs_out``, the clock's pull and the blanking level."""
    gain = 10.0 ** (np.arange(-6, 10, 2) / 10.0) if gain is None else np.asarray(gain, np.float64)
    if gain.shape != (SLICERS,):
        raise ValueError(f"{SLICERS} gains")
    c = PktCfg(pmax=float(np.float32(pmax)), w_mark=phase_word(MARK, fs_out), w_space=phase_word(SPACE, fs_out),
               w_baud=phase_word(BAUD, fs_out), pll_shift=int(pll_shift))
    c.gain[:] = [float(np.float32(v)) for v in gain]
    return c


def cfg_dict(cfg):
    return dict(gain=[float(v) for v in cfg.gain], pmax=cfg.pmax, w_mark=cfg.w_mark, w_space=cfg.w_space, w_baud=cfg.w_baud,
                pll_shift=cfg.pll_shift)


def plan(nk, L, max_out, cfg):
    """What a skimmer of this shape launches (no device needed): dict of rows per workgroup, threads, LDS bytes, tile
    samples, event cap (words per decoder and call), workgroups, slicers per row, words of a frame buffer.  Raises
    PysdrError outside the rules."""
    v = _lib.plan_call("pysdr_pkt_plan", 8, int(nk), int(L), int(max_out), C.byref(cfg) if cfg is not None else None)
    return {"rows": v[0], "threads": v[1], "lds_bytes": v[2], "tile": v[3], "cap": v[4], "groups": v[5], "slicers": v[6], "frame_words": v[7]}


def unpack(words):
    """a decoder's event words of one call -> [(index within the call, the frame's bytes)]"""
    w = np.ascontiguousarray(words, np.int32).view(np.uint32)
    out, at = [], 0
    while at < len(w):
        i, n = int(w[at]) >> 10, int(w[at]) & 1023
        nw = (n + 3) // 4
        out.append((i, w[at + 1:at + 1 + nw].astype("<u4").tobytes()[:n]))
        at += 1 + nw
    return out


def prototype(fs, M, D):
    """The channelizer's prototype for packet rows at fs_out = fs / D: Kaiser(8.0) windowed sinc of 32 D taps cut at
    0.3 fs_out, sum 1: flat to 0.22 fs_out (5.5 kHz at 25 kHz rows: deviation 3 kHz, tones to 2.2 kHz), 80 dB down from
    0.38 fs_out on, so that a station one step away on a raster of fs_out / 2 is not read a second time."""
    return firwin(32 * int(D), 0.3 * float(fs) / int(D), window=("kaiser", 8.0), fs=float(fs))


# ---- de-duplication -----------------------------------------------------------------------------------------------------
class Dedup:
    """One frame, one record.  Two raw records (m, row, slicer, bytes) are copies of one frame if their bytes are equal,
    their m at most ``reach`` = 4 L outputs apart and their rows less than fs_out / 2 apart (``near[row]``: the rows that
    are); a group is all the records that a chain of such pairs joins.  ``add`` takes a call's raw records and the outputs
    complete behind the call, and returns the records (m, row, bytes, slicers) of the groups that are final by then: a
    group is final once ``reach`` outputs lie behind its latest record, and leaves as its row with the most slicers, then
    the lowest row, with that row's earliest m and slicer mask.  Groups leave ordered by their latest and then their first
    record, so the records do not depend on how the stream was cut."""

    def __init__(self, reach, near):
        self.reach, self.near = int(reach), near
        self.open = []                                                   # dicts: data, first (m, row, s), rows {row: [m first, m last, mask]}

    def add(self, records, m_done):
        for m, row, s, data in sorted(records):
            hit = [g for g in self.open if g["data"] == data and
                   any(r in self.near[row] and m - e[1] <= self.reach for r, e in g["rows"].items())]
            if not hit:
                self.open.append(dict(data=data, first=(m, row, s), rows={row: [m, m, 1 << s]}))
                continue
            g = hit[0]
            for other in hit[1:]:                                        # the record joins groups that were apart
                self.open.remove(other)
                g["first"] = min(g["first"], other["first"])
                for r, e in other["rows"].items():
                    mine = g["rows"].setdefault(r, list(e))
                    mine[0], mine[1], mine[2] = min(mine[0], e[0]), max(mine[1], e[1]), mine[2] | e[2]
            e = g["rows"].setdefault(row, [m, m, 0])
            e[1], e[2] = m, e[2] | 1 << s
        return self._leave(lambda g: m_done - 1 - self._last(g) >= self.reach)

    def flush(self):
        """what is still open, at the end of a stream"""
        return self._leave(lambda g: True)

    @staticmethod
    def _last(g):
        return max(e[1] for e in g["rows"].values())

    def _leave(self, final):
        out = sorted((g for g in self.open if final(g)), key=lambda g: (self._last(g), g["first"]))
        self.open = [g for g in self.open if not final(g)]
        res = []
        for g in out:
            row = min(g["rows"], key=lambda r: (-bin(g["rows"][r][2]).count("1"), r))
            res.append((g["rows"][row][0], row, g["data"], g["rows"][row][2]))
        return res


def near_rows(freqs, fs, fs_out):
    """near[a]: the rows whose centres are less than fs_out / 2 from row a's, on the circle of fs"""
    f = np.asarray(freqs, np.float64)
    d = np.abs((f[:, None] - f[None, :] + fs / 2) % fs - fs / 2)
    return [set(np.flatnonzero(d[a] < fs_out / 2 - 1e-6).tolist()) for a in range(len(f))]


class Packet_Decoders(DecoderBank):
    """The decoder bank on a borrowed channelizer of either kind (which it resets, and which must be fed only through it):
    decoder ``row * 8 + s`` is slicer s of row ``row``."""
    KIND, DESTROY = "pkt", "pysdr_pkt_destroy"

    def __init__(self, chan, max_out=4096, cfg=None):
        super().__init__(chan, max_out)
        if not FS_OUT[0] <= self.fs_out <= FS_OUT[1]:
            raise ValueError(f"Packet_Decoders: rows at {self.fs_out} Hz, outside {FS_OUT}")
        self.L, self.tw, self.g = tables(self.fs_out)
        self.ndec = self.nk * SLICERS
        self.cfg = params(self.fs_out) if cfg is None else cfg
        self.plan = plan(self.nk, self.L, self.max_out, self.cfg)         # a bad shape fails here
        self._open(self.ndec, self.L, C.byref(self.cfg), _lib.as_pf(self.tw), _lib.as_pf(self.g))

    def decode_raw(self, x, n=None, on_device=False, events="all"):
        """One call of the C ABI: host samples (complex64 [n]) or a device pointer.  -> dict of n_out, m0 (the absolute
        index of the call's first output), counts [ndec] (event words) and events: every decoder's slots [ndec][cap]
        ("all") or nothing ("counts": the counts alone; None: counts is None too, everything stays on the device and the
        call only queues work when the input is on the device)."""
        return self._decode(x, n, on_device, events)

    def state(self):
        """dict of int32 clk, xprev, xlast, sr, ones, inframe, byte, nb, nbytes, crc [ndec] and frames uint32 [ndec][83]"""
        ints = np.empty((len(STATE_INTS), self.ndec), np.int32)
        frames = np.empty((self.ndec, FRAME_WORDS), np.uint32)
        self._call("state", ints.ctypes.data_as(C.POINTER(C.c_int32)), frames.ctypes.data_as(C.POINTER(C.c_uint32)))
        out = {k: ints[i].copy() for i, k in enumerate(STATE_INTS)}
        out["frames"] = frames
        return out


class Packet_Skimmer(Skimmer):
    """Wideband IQ at ``fs`` -> a channelizer of M rows fs / M apart at fs / D samples per second (D = M / 2 by default: a
    12.5 kHz raster gives rows at 25 kHz) -> eight packet decoders on every row -> the frames heard, each once.
    ``push(x)`` returns ``(m, row, text)``: m the absolute index of the row output that completed the frame's closing
    flag, text its TNC2 line; ``text[row]`` gains the lines, ``frames`` the records ``(m, row, bytes, slicers)``, slicers
    a bit mask.  A frame is final, and returned, once 4 L outputs lie behind it (``flush`` at the end of a stream)."""

    def __init__(self, fs, M=None, D=None, h=None, channels=None, chan=None, max_out=4096, device=0, max_in=1 << 22, cfg=None):
        self.fs = float(fs)
        if chan is None:
            self.M = int(M)
            self.D = self.M // 2 if D is None else int(D)
            fs_out = self.fs / self.D
            if not FS_OUT[0] <= fs_out <= FS_OUT[1]:
                raise ValueError(f"Packet_Skimmer: rows at {fs_out} Hz, outside {FS_OUT}")
            nk = self.M if channels is None else int(channels[1])
            plan(nk, window_length(fs_out), max_out, params(fs_out) if cfg is None else cfg)   # a bad shape fails here, with or without a device
            self.h = prototype(fs, self.M, self.D) if h is None else np.asarray(h, np.float64)
            self.chan = Channelizer(fs, self.M, self.D, self.h, channels, device, max_in)
        else:
            # a ready channelizer of either kind, adopted and owned
            if float(fs) != chan.fs or not FS_OUT[0] <= chan.fs_out <= FS_OUT[1]:
                raise ValueError(f"Packet_Skimmer: the channelizer's rows (fs {chan.fs}, fs_out {chan.fs_out}) are not at {FS_OUT} Hz of fs = {fs}")
            self.chan, self.M, self.D, self.h = chan, chan.M, chan.D, chan.prototypes
        self.dec = Packet_Decoders(self.chan, max_out, cfg)
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
        """one call: the counts come off the device first, then only the decoders that closed a frame"""
        r = self.dec.decode_raw(x, events="counts")
        if r["n_out"] == 0:
            return []
        rows = np.flatnonzero(r["counts"] > 0)
        raw = []
        if len(rows):
            words = self.dec.fetch(rows)
            raw = [(r["m0"] + i, int(d) // SLICERS, int(d) % SLICERS, data) for k, d in enumerate(rows)
                   for i, data in unpack(words[k, :r["counts"][d]])]
        return self._keep(self.dedup.add(raw, r["m0"] + r["n_out"]))

    def _keep(self, records):
        self.frames += records
        out = [(m, row, tnc2(data)) for m, row, data, _ in records]
        for _, row, line in out:
            self.text[row] += line + "\n"
        return out

    def push(self, x):
        """complex64 [n] -> the frames (m, row, text) that became final with this input, in the order they were first
        heard; the input goes through in calls of at most ``dec.max_samples()``."""
        x = np.ascontiguousarray(x, np.complex64)
        ev, i = [], 0
        while i < len(x):
            n = min(len(x) - i, self.dec.max_samples())
            ev += self._events(x[i:i + n])
            i += n
        return ev

    def flush(self):
        """the frames heard in the last 4 L outputs, at the end of a stream"""
        return self._keep(self.dedup.flush())
