"""RDS skimmer: station names on every row of an FM broadcast raster (kernel ``rds.hip``, host half
``api_rds.hip``).  RDS / RBDS is the 1187.5 bit/s data on the 57 kHz subcarrier of a broadcast FM station: its PI code,
its eight-character name (PS), RadioText, programme type and clock time.  A channelizer of either kind delivers rows at
any ``fs_out`` from 228 to 512 kHz; on every row a four-quadrant discriminator, a mixer from 57 kHz, the matched filter
of the biphase symbol at sixteen timing phases per bit, a differential decision and sixteen block-check decoders run on
the device.  Only groups whose four blocks all check leave it.  The host removes the copies of a group (a row's other
phases, the neighbour rows that overlap it), parses the groups and assembles the stations' texts.  The tables and
settings are derived here, once, and handed to the library already derived.  The reference holds no RDS decoder: the
definition is our own."""
from __future__ import annotations

import ctypes as C

import numpy as np
from scipy.signal import firwin

from . import _lib
from ._lib import RdsCfg
from .channelizer import Channelizer
from .packet import Dedup, near_rows
from .skimmer import DecoderBank, Skimmer

BITRATE, PILOT, SUBCARRIER = 1187.5, 19000.0, 57000.0
PHASES = 16
FS_OUT = (228000.0, 512000.0)
POLY = 0x5B9                                                            # x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1
OFFSETS = {"A": 0x0FC, "B": 0x198, "C": 0x168, "C'": 0x350, "D": 0x1B4}


# ---- blocks and groups ----------------------------------------------------------------------------------------------------
def syndrome(b):
    """the remainder of a block of up to 26 bits by g(x), MSB first"""
    b = int(b)
    for k in range(25, 9, -1):
        if b >> k & 1:
            b ^= POLY << (k - 10)
    return b


def block(info, offset):
    """16 information bits -> the 26-bit block: the information, then its check word plus the offset word ("A" ... "D")"""
    info = int(info) & 0xFFFF
    return info << 10 | (syndrome(info << 10) ^ OFFSETS[offset])


def check_block(b):
    """the name of the offset word a 26-bit block checks with, or None"""
    s = syndrome(b)
    return next((k for k, v in OFFSETS.items() if v == s), None)


def group_bits(a, b, c, d, version_b=False):
    """the 104 bits of a group, in the order sent; the third block carries C' in a version B group (bit 11 of ``b``)"""
    third = "C'" if version_b or (int(b) >> 11 & 1) else "C"
    v = block(a, "A") << 78 | block(b, "B") << 52 | block(c, third) << 26 | block(d, "D")
    return np.array([v >> (103 - i) & 1 for i in range(104)], np.uint8)


def _second(code, version_b, tp, pty, low):
    return (int(code) & 15) << 12 | (1 if version_b else 0) << 11 | (int(tp) & 1) << 10 | (int(pty) & 31) << 5 | (int(low) & 31)


def _chars(text, n):
    raw = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    return raw.ljust(n)[:n]


def af_code(mhz):
    """87.6 .. 107.9 MHz -> 1 .. 204; None -> the filler code 205"""
    if mhz is None:
        return 205
    code = int(round((float(mhz) - 87.5) * 10))
    if not 1 <= code <= 204:
        raise ValueError(f"no AF: {mhz} MHz")
    return code


def group_0a(pi, ps, seg, tp=0, pty=0, ta=0, ms=1, di=0, af=(None, None)):
    """basic tuning, version A: characters ``2 seg`` and ``2 seg + 1`` of the name ``ps``, a pair of alternative
    frequencies (MHz or None), and bit ``3 - seg`` of the decoder identification as ``di``"""
    low = (ta & 1) << 4 | (ms & 1) << 3 | (di & 1) << 2 | (seg & 3)
    ch = _chars(ps, 8)[2 * seg:2 * seg + 2]
    return int(pi) & 0xFFFF, _second(0, False, tp, pty, low), af_code(af[0]) << 8 | af_code(af[1]), ch[0] << 8 | ch[1]


def group_0b(pi, ps, seg, tp=0, pty=0, ta=0, ms=1, di=0):
    """basic tuning, version B: the PI again in place of the alternative frequencies"""
    low = (ta & 1) << 4 | (ms & 1) << 3 | (di & 1) << 2 | (seg & 3)
    ch = _chars(ps, 8)[2 * seg:2 * seg + 2]
    return int(pi) & 0xFFFF, _second(0, True, tp, pty, low), int(pi) & 0xFFFF, ch[0] << 8 | ch[1]


def group_2a(pi, text, seg, ab, tp=0, pty=0):
    """RadioText, version A: characters ``4 seg`` .. ``4 seg + 3`` of ``text`` (the whole text, up to 64)"""
    ch = _chars(text, 64)[4 * seg:4 * seg + 4]
    return int(pi) & 0xFFFF, _second(2, False, tp, pty, (ab & 1) << 4 | (seg & 15)), ch[0] << 8 | ch[1], ch[2] << 8 | ch[3]


def group_2b(pi, text, seg, ab, tp=0, pty=0):
    """RadioText, version B: characters ``2 seg`` and ``2 seg + 1`` of ``text`` (up to 32)"""
    ch = _chars(text, 32)[2 * seg:2 * seg + 2]
    return int(pi) & 0xFFFF, _second(2, True, tp, pty, (ab & 1) << 4 | (seg & 15)), int(pi) & 0xFFFF, ch[0] << 8 | ch[1]


def group_4a(pi, mjd, hour, minute, offset=0, tp=0, pty=0):
    """clock time: modified Julian day, UTC hour and minute, local offset in half hours (signed)"""
    mjd, off = int(mjd) & 0x1FFFF, int(offset)
    c = (mjd & 0x7FFF) << 1 | (hour >> 4 & 1)
    d = (hour & 15) << 12 | (minute & 63) << 6 | (1 if off < 0 else 0) << 5 | (abs(off) & 31)
    return int(pi) & 0xFFFF, _second(4, False, tp, pty, mjd >> 15), c, d


def ps_groups(pi, ps, version_b=False, **kw):
    """the four groups that carry a station's name"""
    return [(group_0b if version_b else group_0a)(pi, ps, seg, **kw) for seg in range(4)]


def rt_groups(pi, text, ab=0, version_b=False, **kw):
    """the groups of a RadioText; one shorter than 64 (32) characters ends in 0x0D"""
    per, most = (2, 32) if version_b else (4, 64)
    raw = _chars(text, len(text))
    if len(raw) < most:
        raw += b"\r"
    make = group_2b if version_b else group_2a
    return [make(pi, raw.ljust(most), seg, ab, **kw) for seg in range(-(-len(raw) // per))]


def _text(raw):
    """bytes 0x20 to 0x7E are ASCII, the others '?' (the G0 / G1 / G2 tables are not done)"""
    return "".join(chr(b) if 0x20 <= b <= 0x7E else "?" for b in raw)


def _pair(w):
    return bytes([w >> 8 & 255, w & 255])


def parse_group(words):
    """(a, b, c, d) -> dict of pi, type ("0A" ...), tp, pty and what the type carries: 0A / 0B seg, ps (two characters),
    ta, ms, di, and af (a pair of MHz or None) in 0A; 2A / 2B seg, ab, text and raw (the bytes: 0x0D ends a text); 4A mjd,
    hour, minute, offset (half hours); anything else raw = (low five bits of b, c, d)."""
    a, b, c, d = (int(v) & 0xFFFF for v in words[:4])
    code, vb = b >> 12, b >> 11 & 1
    g = dict(pi=a, type=f"{code}{'AB'[vb]}", tp=b >> 10 & 1, pty=b >> 5 & 31)
    if code == 0:
        g.update(seg=b & 3, ps=_text(_pair(d)), ta=b >> 4 & 1, ms=b >> 3 & 1, di=b >> 2 & 1)
        if not vb:
            g["af"] = tuple(round(87.5 + 0.1 * k, 1) if 1 <= k <= 204 else None for k in (c >> 8, c & 255))
    elif code == 2:
        raw = _pair(d) if vb else _pair(c) + _pair(d)
        g.update(seg=b & 15, ab=b >> 4 & 1, raw=raw, text=_text(raw))
    elif code == 4 and not vb:
        off = d & 31
        g.update(mjd=(b & 3) << 15 | c >> 1, hour=(c & 1) << 4 | d >> 12, minute=d >> 6 & 63, offset=-off if d >> 5 & 1 else off)
    else:
        g["raw"] = (b & 31, c, d)
    return g


def callsign(pi):
    """The RBDS rule for a four-letter call: K or W and three letters in base 26, K from 0x1000, W from 0x54A8.  From
    memory of NRSC-4 and unpinned; the table of the three-letter calls (KGB, ...) is not here: None outside the rule."""
    pi = int(pi)
    if not 0x1000 <= pi < 0x54A8 + 17576:
        return None
    first, n = ("K", pi - 0x1000) if pi < 0x54A8 else ("W", pi - 0x54A8)
    return first + "".join(chr(65 + n // q % 26) for q in (676, 26, 1))


def pi_of(call):
    """the inverse of ``callsign``"""
    call = call.upper()
    if len(call) != 4 or call[0] not in "KW" or not call[1:].isalpha() or not call.isascii():
        raise ValueError(f"no four-letter K / W call: {call!r}")
    n = sum((ord(ch) - 65) * q for ch, q in zip(call[1:], (676, 26, 1)))
    return (0x1000 if call[0] == "K" else 0x54A8) + n


class Station:
    """What one PI code's groups add up to.  ``add(parsed group)`` returns the changes, a list of ("ps", name), ("rt",
    text) and ("ct", (mjd, hour, minute, offset)).

    PS: the eight characters are kept with a mark per segment.  A segment is kept and marked; one that differs from a
    marked one first clears every mark.  ``ps`` becomes the kept name once all four segments are marked, and that is a change if it
    differs from the name shown before.  A repeated segment changes nothing.

    RadioText: 64 (2A) or 32 (2B) characters are kept with a mark per segment; a group whose A/B flag differs from the last
    one's clears the characters, the marks and ``rt``.  ``rt`` becomes the characters up to the first 0x0D once every
    segment up to the one that holds it is marked, or all of them once every segment is marked."""

    def __init__(self, pi):
        self.pi, self.call = pi, callsign(pi)
        self.ps = self.rt = self.ct = None
        self.pty = self.tp = None
        self._ps, self._ps_got = bytearray(b" " * 8), 0
        self._rt, self._rt_got, self._ab = bytearray(64), 0, None
        self.rows = {}                                                    # the skimmer's: groups recorded per row

    def add(self, g):
        out = []
        self.pty, self.tp = g["pty"], g["tp"]
        if g["type"] in ("0A", "0B"):
            k, ch = g["seg"], g["ps"].encode("latin-1")
            if self._ps_got >> k & 1 and self._ps[2 * k:2 * k + 2] != ch:
                self._ps_got = 0
            self._ps[2 * k:2 * k + 2] = ch
            self._ps_got |= 1 << k
            name = self._ps.decode("latin-1")
            if self._ps_got == 15 and name != self.ps:
                self.ps = name
                out.append(("ps", name))
        elif g["type"] in ("2A", "2B"):
            per = 4 if g["type"] == "2A" else 2
            if g["ab"] != self._ab:
                self._rt, self._rt_got, self._ab, self.rt = bytearray(64), 0, g["ab"], None
            k = g["seg"]
            self._rt[per * k:per * k + per] = g["raw"]
            self._rt_got |= 1 << k
            end = self._rt.find(b"\r", 0, 16 * per)
            nseg = 16 if end < 0 else end // per + 1
            if self._rt_got & ((1 << nseg) - 1) == (1 << nseg) - 1:
                text = _text(self._rt[:16 * per if end < 0 else end])
                if text != self.rt:
                    self.rt = text
                    out.append(("rt", text))
        elif g["type"] == "4A":
            ct = (g["mjd"], g["hour"], g["minute"], g["offset"])
            if ct != self.ct:
                self.ct = ct
                out.append(("ct", ct))
        return out


# ---- test signals -----------------------------------------------------------------------------------------------------
def bits(groups):
    """the bits of the groups (a, b, c, d), in the order sent (the differential encoding is the waveform's business)"""
    return np.concatenate([group_bits(*g) for g in groups]) if len(groups) else np.zeros(0, np.uint8)


def _shaping(t):
    """the impulse response of the standard's shaping filter, cos(pi f t_d / 4) out to 2 / t_d, at t in bits"""
    return 2.0 * (np.sinc(0.5 + 4.0 * t) + np.sinc(0.5 - 4.0 * t))


def pulse(t):
    """a biphase symbol, centred at 0, at t in bits: an impulse a quarter bit early, its opposite a quarter bit late, shaped"""
    return _shaping(t + 0.25) - _shaping(t - 0.25)


def rds_baseband(groups, fs, lead=2):
    """The data signal at ``fs``, peak 1: ``lead`` bits of nothing, a reference symbol, the differentially encoded bits,
    ``lead`` bits of nothing.  float64"""
    b = bits(groups)
    e = np.concatenate(([0], np.cumsum(b) & 1))                          # the reference symbol, then e[k] = e[k - 1] ^ bit[k]
    a = np.concatenate((np.zeros(lead + 3), 2.0 * e - 1.0, np.zeros(lead + 3)))
    n = int(np.ceil((len(e) + 2 * lead) * fs / BITRATE))
    t = np.arange(n) * (BITRATE / fs) + 3.0                              # in bits; symbol k of ``a`` is centred at k + 0.5
    k0 = np.floor(t).astype(np.int64)
    s = np.zeros(n)
    for dk in range(-3, 4):                                              # the pulse beyond three bits is below 1e-3 of its peak
        s += a[k0 + dk] * pulse(t - (k0 + dk) - 0.5)
    return s / np.abs(s).max()


def mpx(groups, fs, left=1000.0, right=3100.0, audio_dev=30e3, pilot_dev=6.75e3, rds_dev=2e3, lead=2):
    """A stereo station's multiplex in Hz of deviation at ``fs``: tones ``left`` and ``right`` Hz at ``audio_dev`` in
    all, the 19 kHz pilot, L - R on 38 kHz, the groups' RDS on 57 kHz, both locked to the pilot.  float64"""
    s = rds_baseband(groups, fs, lead)
    th = 2 * np.pi * PILOT * np.arange(len(s)) / fs
    lt, rt = np.sin(2 * np.pi * left * np.arange(len(s)) / fs), np.sin(2 * np.pi * right * np.arange(len(s)) / fs)
    return audio_dev * (0.5 * (lt + rt) + 0.5 * (lt - rt) * np.sin(2 * th)) + pilot_dev * np.sin(th) + rds_dev * s * np.sin(3 * th)


def waveform(groups, fs, f0, deviation=75e3, rds_dev=2e3, **kw):
    """One station as FM at ``f0`` Hz from the centre of a band sampled at ``fs``: complex64, unit amplitude; the multiplex
    is limited to ``deviation`` Hz in all."""
    m = np.clip(mpx(groups, fs, rds_dev=rds_dev, **kw), -float(deviation), float(deviation))
    ph = 2 * np.pi * (np.cumsum(m) + float(f0) * np.arange(len(m))) / fs
    return np.exp(1j * ph).astype(np.complex64)


# ---- the bank's tables and settings ---------------------------------------------------------------------------------
def pulse_length(fs_out):
    return 2 * int(np.floor(float(fs_out) / BITRATE)) + 1


def tables(fs_out):
    """-> (L, tw float32 [1024][2] = (cos, -sin)(2 pi k / 1024), g float32 [L]: the symbol's pulse over a bit to either
    side of its centre, sum |g| = 1): derived in float64, rounded once"""
    L = pulse_length(fs_out)
    t = 2 * np.pi * np.arange(1024) / 1024
    tw = np.stack((np.cos(t), -np.sin(t)), axis=1)
    g = pulse((np.arange(L) - (L - 1) // 2) * (BITRATE / float(fs_out)))
    return L, np.ascontiguousarray(tw, np.float32), (g / np.abs(g).sum()).astype(np.float32)


def phase_word(f, fs_out):
    return int(round(float(f) / float(fs_out) * 2.0 ** 32))


def params(fs_out):
    """The settings of DESIGN.md 3 item 31 as the ``_lib.RdsCfg`` the C ABI takes: the one word, 19 kHz at ``fs_out``"""
    return RdsCfg(w19=phase_word(PILOT, fs_out))


def plan(nk, L, max_out, cfg):
    """What a skimmer of this shape launches (no device needed): dict of rows per workgroup, threads, LDS bytes, tile
    samples, event cap (words per decoder and call), workgroups, phases per row, segments of the matched filter.  Raises
    PysdrError outside the rules."""
    v = _lib.plan_call("pysdr_rds_plan", 8, int(nk), int(L), int(max_out), C.byref(cfg) if cfg is not None else None)
    return {"rows": v[0], "threads": v[1], "lds_bytes": v[2], "tile": v[3], "cap": v[4], "groups": v[5], "phases": v[6], "segments": v[7]}


def unpack(words):
    """a decoder's event words of one call -> [(index within the call, phase, (a, b, c, d, 1 if C' else 0))]"""
    w = np.ascontiguousarray(words, np.int32).view(np.uint32)
    return [(int(w[k]) >> 5, int(w[k]) >> 1 & 15, (int(w[k + 1]) >> 16, int(w[k + 1]) & 0xFFFF, int(w[k + 2]) >> 16, int(w[k + 2]) & 0xFFFF,
                                                   int(w[k]) & 1)) for k in range(0, len(w) - 2, 3)]


def prototype(fs, M, D):
    """The channelizer's prototype for RDS rows at fs_out = fs / D: Kaiser(8.0) windowed sinc of 48 D taps (16 M at the
    most) cut at 0.5 fs_out, sum 1: flat to 0.44 fs_out (100 kHz at 228 kHz rows, 176 kHz at 400 kHz rows: a station's
    deviation and the 57 kHz sidebands to either side of it), 80 dB down from 0.56 fs_out on; what folds lands outside
    0.44 fs_out."""
    return firwin(min(48 * int(D), 16 * int(M)), 0.5 * float(fs) / int(D), window=("kaiser", 8.0), fs=float(fs))


def reach(fs_out):
    """the outputs of two bits: copies of a group end no further apart"""
    return int(np.ceil(2 * float(fs_out) / BITRATE))


class RDS_Decoders(DecoderBank):
    """The decoder bank on a borrowed channelizer of either kind (which it resets, and which must be fed only through it):
    decoder ``row * 16 + p`` is timing phase p of row ``row``."""
    KIND, DESTROY = "rds", "pysdr_rds_destroy"

    def __init__(self, chan, max_out=65536, cfg=None):
        super().__init__(chan, max_out)
        if not FS_OUT[0] <= self.fs_out <= FS_OUT[1]:
            raise ValueError(f"RDS_Decoders: rows at {self.fs_out} Hz, outside {FS_OUT}")
        self.L, self.tw, self.g = tables(self.fs_out)
        self.ndec = self.nk * PHASES
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
        """dict of regs uint32 [4][ndec] (the registers' blocks, the oldest first), chips uint32 [nk] and ring float32
        [nk][16][2] (z of every phase's last chip)"""
        regs = np.empty((4, self.ndec), np.uint32)
        chips = np.empty(self.nk, np.uint32)
        ring = np.empty((self.nk, PHASES, 2), np.float32)
        pu = C.POINTER(C.c_uint32)
        self._call("state", regs.ctypes.data_as(pu), chips.ctypes.data_as(pu), _lib.as_pf(ring))
        return dict(regs=regs, chips=chips, ring=ring)


class RDS_Skimmer(Skimmer):
    """Wideband IQ at ``fs`` -> a channelizer of M rows fs / M apart at fs / D samples per second (by default a 100 kHz
    raster with rows at 400 kHz: M = fs / 100 kHz, D = M / 4, which serves the European grid and the odd 200 kHz channels
    of the US) -> sixteen RDS decoders on every row -> the groups heard, each once, and the stations' texts.
    ``push(x)`` returns records ``(m, row, "group", words)``: m the absolute index of the row output that completed the
    group, words (a, b, c, d, 1 if the third block carried C'); and ``(m, row, "ps" | "rt" | "ct", value)`` when a
    station's name, RadioText or clock time changes with that group.  ``groups`` gains ``(m, row, words, phases)``,
    phases a bit mask; ``stations[row]`` is a dict PI -> ``Station``, which lists a PI once it came in two groups on that
    row or the rows near it (``keep_groups``): a false group has a random PI.  A group is final, and returned, once two bits of outputs lie
    behind it (``flush`` at the end of a stream)."""

    def __init__(self, fs, M=None, D=None, h=None, channels=None, chan=None, max_out=65536, device=0, max_in=1 << 22, cfg=None):
        self.fs = float(fs)
        if chan is None:
            self.M = int(round(self.fs / 100e3)) if M is None else int(M)
            self.D = self.M // 4 if D is None else int(D)
            if self.M < 1 or self.D < 1:
                raise ValueError(f"RDS_Skimmer: no raster for fs = {fs}")
            fs_out = self.fs / self.D
            if not FS_OUT[0] <= fs_out <= FS_OUT[1]:
                raise ValueError(f"RDS_Skimmer: rows at {fs_out} Hz, outside {FS_OUT}")
            nk = self.M if channels is None else int(channels[1])
            plan(nk, pulse_length(fs_out), max_out, params(fs_out) if cfg is None else cfg)   # a bad shape fails here, with or without a device
            self.h = prototype(fs, self.M, self.D) if h is None else np.asarray(h, np.float64)
            self.chan = Channelizer(fs, self.M, self.D, self.h, channels, device, max_in)
        else:
            # a ready channelizer of either kind, adopted and owned
            if float(fs) != chan.fs or not FS_OUT[0] <= chan.fs_out <= FS_OUT[1]:
                raise ValueError(f"RDS_Skimmer: the channelizer's rows (fs {chan.fs}, fs_out {chan.fs_out}) are not at {FS_OUT} Hz of fs = {fs}")
            self.chan, self.M, self.D, self.h = chan, chan.M, chan.D, chan.prototypes
        self.dec = RDS_Decoders(self.chan, max_out, cfg)
        self.nk, self.ndec, self.fs_out, self.L = self.chan.nk, self.dec.ndec, self.chan.fs_out, self.dec.L
        self.freqs = self.chan.freqs
        self._start()

    def _start(self):
        self.groups = []
        self.stations = [dict() for _ in range(self.nk)]
        self._first = [dict() for _ in range(self.nk)]                    # a PI's first group on a row, until its second
        self.dedup = Dedup(reach(self.fs_out), near_rows(self.freqs, self.fs, self.fs_out))

    def reset(self):
        self.dec.reset()
        self._start()

    def _events(self, x):
        """one call: the counts come off the device first, then only the decoders that said something"""
        r = self.dec.decode_raw(x, events="counts")
        if r["n_out"] == 0:
            return []
        rows = np.flatnonzero(r["counts"] > 0)
        raw = []
        if len(rows):
            words = self.dec.fetch(rows)
            raw = [(r["m0"] + i, int(d) // PHASES, p, data) for k, d in enumerate(rows) for i, p, data in unpack(words[k, :r["counts"][d]])]
        return self._keep(self.dedup.add(raw, r["m0"] + r["n_out"]))

    def _keep(self, records):
        self.groups += records
        return keep_groups(records, self.stations, self._first, self.dedup.near)

    def push(self, x):
        """complex64 [n] -> the records that became final with this input; the input goes through in calls of at most
        ``dec.max_samples()``."""
        x = np.ascontiguousarray(x, np.complex64)
        ev, i = [], 0
        while i < len(x):
            n = min(len(x) - i, self.dec.max_samples())
            ev += self._events(x[i:i + n])
            i += n
        return ev

    def flush(self):
        """the groups heard in the last two bits, at the end of a stream"""
        return self._keep(self.dedup.flush())

    def band_list(self):
        """[(MHz offset from the band's centre of the row that recorded most of its groups, PI, call, PS)] of the stations
        listed so far"""
        return sorted((float(self.freqs[max(st.rows, key=lambda r: (st.rows[r], -r))]) / 1e6, pi, st.call, st.ps)
                      for row in range(self.nk) for pi, st in self.stations[row].items())


def keep_groups(records, stations, first, near=None):
    """Dedup's records (m, row, words, phases) -> push's records, and the rows' stations brought up to date.  Neighbour
    rows overlap, and which of them a group's record names depends on the noise; so a PI is looked up on the record's row,
    then on the rows near it (``near[row]``, lowest first) and then on the rows near those, and stays where it was first heard: its first group waits in
    ``first[row]`` until the PI comes again; then the station is listed on that row and takes both.  Text records carry
    the station's row."""
    out = []
    for m, row, words, _ in records:
        out.append((m, row, "group", words))
        g = parse_group(words)
        ring1 = set(near[row]) - {row} if near is not None else set()
        ring2 = {q for r in ring1 for q in near[r]} - ring1 - {row}
        around = [row] + sorted(ring1) + sorted(ring2)
        home = next((r for r in around if g["pi"] in stations[r]), None)
        todo = [g]
        if home is None:
            home = next((r for r in around if g["pi"] in first[r]), None)
            if home is None:
                first[row][g["pi"]] = g
                continue
            stations[home][g["pi"]] = Station(g["pi"])
            todo = [first[home].pop(g["pi"]), g]
        st = stations[home][g["pi"]]
        for r in [home] * (len(todo) - 1) + [row]:                        # the held group was recorded on the station's row
            st.rows[r] = st.rows.get(r, 0) + 1
        for q in todo:
            out += [(m, home, kind, value) for kind, value in st.add(q)]
    return out
