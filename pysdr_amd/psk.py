"""PSK31 skimmer: a Varicode decoder on a fine raster of the band (kernel ``psk.hip``, host half
``api_psk.hip``).  A ``Channelizer`` with M / D = 4 delivers rows at ``S`` samples per symbol; inside every row a bank of
``NSUB = 4 S`` differential BPSK decoders runs on the device, one every baud / 32, so that the fine rows ``F = a NSUB + j``
form one uniform raster of spacing baud / 16 over all rows.  A finder on the host decides after every call which decoder
of a neighbourhood owns a station; only the owners' events are downloaded.  The tables and settings are
derived here, once, and handed to the library already derived."""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np
from scipy.signal import firwin

from . import _lib
from . import channelizer as _chan
from ._lib import PskCfg
from .channelizer import Channelizer
from .skimmer import DecoderBank, Skimmer

STATE_FLOATS = ("qn", "qd", "cr", "ci")
STATE_INTS = ("pt", "cnt", "sh", "open", "seen")
NEIGHBOURHOOD = 9                        # fine rows on either side a station's owner beats: the image baud / 2 away is at 8
KEEP = 1.5                               # the finder's hysteresis: last call's owner competes with 1.5 times its qn

_VARICODE_HEX = """
2ab,2db,2ed,377,2eb,35f,2ef,2fd,2ff,ef,1d,36f,2dd,1f,375,3ab,2f7,2f5,3ad,3af,35b,36b,36d,357,37b,37d,3b7,355,35d,3bb,2fb,37f,
1,1ff,15f,1f5,1db,2d5,2bb,17f,fb,f7,16f,1df,75,35,57,1af,b7,bd,ed,ff,177,15b,16b,1ad,1ab,1b7,f5,1bd,1ed,55,1d7,2af,
2bd,7d,eb,ad,b5,77,db,fd,155,7f,1fd,17d,d7,bb,dd,ab,d5,1dd,af,6f,6d,157,1b5,15d,175,17b,2ad,1f7,1ef,1fb,2bf,16d,
2df,b,5f,2f,2d,3,3d,5b,2b,d,1eb,bf,1b,3b,f,7,3f,1bf,15,17,5,37,7b,6b,df,5d,1d5,2b7,1bb,2b5,2d7,3b5
"""
VARICODE = [int(v, 16) for v in _VARICODE_HEX.replace("\n", "").split(",")]      # ASCII 0 .. 127 -> bits, MSB first
CODE_CHAR = {c: chr(i) for i, c in enumerate(VARICODE)}


def code_text(code):
    """The text of an event's code: the character, '*' for anything the Varicode table does not hold."""
    return CODE_CHAR.get(int(code), "*")


def unpack(word):
    """event word -> (index within the call, code)"""
    w = int(word) & 0xFFFFFFFF
    return w >> 11, w & 2047


def varicode_bits(text):
    """The bit string of ``text``: every character's Varicode followed by 00 (characters beyond ASCII 127 are skipped)."""
    return "".join(format(VARICODE[ord(ch)], "b") + "00" for ch in text if ord(ch) < 128)


def psk_baseband(text, baud, fs, f, preamble=2.0, tail=0.5, phase=0.0):
    """complex128 test signal at ``fs``: ``preamble`` seconds of idle reversals, the characters of ``text`` separated by 00,
    ``tail`` seconds of idle, as a carrier ``f`` Hz from the centre.  A 0 reverses the phase, a 1 keeps it; the symbols are
    shaped with the raised-cosine pulse 0.5 (1 + cos(pi t / T)) over |t| < T, T = 1 / baud, so that the mean power is 1
    while the phase holds and the envelope goes through zero at a reversal."""
    T = float(fs) / float(baud)                                  # samples per symbol; need not be an integer
    bits = "0" * int(round(preamble * baud)) + varicode_bits(text) + "0" * int(round(tail * baud))
    a = np.cumprod(np.where(np.frombuffer(bits.encode(), np.uint8) == ord("1"), 1.0, -1.0))
    n = np.arange(int(np.ceil((len(a) + 1) * T)))
    s = np.zeros(len(n))
    k0 = np.floor(n / T).astype(np.int64)                        # the symbol whose centre is at or before n
    for dk in (0, 1):                                            # two pulses overlap everywhere
        k = k0 + dk
        t = n - k * T
        ok = k < len(a)
        s[ok] += a[k[ok]] * 0.5 * (1.0 + np.cos(np.pi * t[ok] / T))
    return s * np.exp(1j * (2 * np.pi * float(f) / float(fs) * n + phase))


def shape(fs, baud=31.25):
    """-> (S, D, M): S = 8 row samples per symbol if fs / (8 baud) is an integer D and the channelizer accepts M = 4 D,
    otherwise S = 12 likewise, otherwise ValueError."""
    for S in (8, 12):
        d = float(fs) / (S * float(baud))
        D = int(round(d))
        if D < 1 or abs(d - D) > 1e-9 * max(d, 1.0):
            continue
        try:
            _chan.plan(4 * D, D, 16 * D)
        except _lib.PysdrError:
            continue
        return S, D, 4 * D
    raise ValueError(f"no PSK raster for fs = {fs} and {baud} baud: fs / (8 baud) or fs / (12 baud) must be an integer D with "
                     f"M = 4 D a channelizer size")


def fine_channelizer(fs, band, baud=31.25, device=0, max_in=1 << 22):
    """A ``fine.FineChannelizer`` for ``PSK_Skimmer(fs, baud, chan=...)`` at a rate ``shape`` refuses: rows S baud / 4
    apart whose centres lie in ``band = (f_lo, f_hi)`` Hz from the centre, S = 8 where ``fine.shape`` finds a shape, else
    12; M2 / D2 = 4, the second prototype is ``prototype`` at the first stage's output rate, the first ``fine.prototype1``."""
    from . import fine
    err = None
    for S in (8, 12):
        try:
            M1, D1, M2, D2 = fine.shape(fs, S * float(baud), 4)
        except ValueError as e:
            err = e
            continue
        h2 = prototype(float(fs) / D1, M2, baud, S)
        return fine.FineChannelizer(fs, M1, M2, D1, D2, fine.prototype1(fs, M1, D1, M2), h2,
                                    fine.channels_for(band, fs, M1, D1, M2), device, max_in)
    raise ValueError(f"no PSK raster in two stages for fs = {fs} and {baud} baud: {err}")


def prototype(fs, M, baud, S):
    """The channelizer's prototype for the PSK raster: Kaiser(8.0) windowed-sinc low-pass of 4 M taps cut at fs_out / 2 =
    S baud / 2, sum 1 (the convention of ``design.channelizer_taps``).  The rows are S baud / 4 apart, so a station is
    at most half a spacing plus its own baud-wide spectrum from a row's centre: the response is flat within 0.1 dB out to
    fp = S baud / 8 + baud and at least 70 dB down from fs_out - fp on, where the aliases of that band begin."""
    return firwin(4 * int(M), 0.5 * S * float(baud), window=("kaiser", 8.0), fs=float(fs))


def tables(S):
    """-> (tw float32 [32 S][2] = (cos, -sin)(2 pi t / NT), g float32 [2 S]): derived in float64, rounded once"""
    NT, L = 32 * S, 2 * S
    t = 2 * np.pi * np.arange(NT) / NT
    tw = np.stack((np.cos(t), -np.sin(t)), axis=1)
    g = 0.5 * (1.0 - np.cos(2 * np.pi * (np.arange(L) + 0.5) / L))
    return np.ascontiguousarray(tw, np.float32), np.ascontiguousarray(g / g.sum(), np.float32)


def params(a_t=1.0 / 32, a_q=1.0 / 64, hi=0.75, lo=0.3, hy=1.125, pmax=1e18, n0=128):
    """The settings of DESIGN.md 3 item 19 as the ``_lib.PskCfg`` the C ABI takes."""
    def f(v):                                        # the float32 nearest to v, as the Python float ctypes takes
        return float(np.float32(v))

    return PskCfg(a_t=f(a_t), a_q=f(a_q), hi=f(hi), lo=f(lo), hy=f(hy), pmax=f(pmax), n0=int(n0))


def cfg_dict(cfg):
    return {k: getattr(cfg, k) for k, _ in PskCfg._fields_}


def plan(nk, S, max_out, cfg):
    """What a skimmer of this shape launches (no device needed): dict of rows per workgroup, threads, LDS bytes, tile
    samples, event cap per decoder and call, workgroups, decoders per row.  Raises PysdrError outside the rules."""
    v = _lib.plan_call("pysdr_psk_plan", 8, int(nk), int(S), int(max_out), C.byref(cfg) if cfg is not None else None)
    return {"rows": v[0], "threads": v[1], "lds_bytes": v[2], "tile": v[3], "cap": v[4], "groups": v[5], "nsub": v[6]}


def owners(qn, is_open, circular, prev=None, keep=KEEP, reach=NEIGHBOURHOOD):
    """The finder: fine row F owns its neighbourhood if it is open and beats every G with 0 < |F - G| <= ``reach`` (9) --
    qn[F] > qn[G], or equal and F < G.  The distance is circular where the rows cover the whole band, clipped otherwise.  The
    owners of the last call (``prev``, bool [NF]) compete with ``keep`` times their qn (float32 product): a station that
    sits between two decoders stays with the one that had it.  -> bool [NF]"""
    qn = np.asarray(qn, np.float32)
    if prev is not None:
        qn = np.where(np.asarray(prev, bool) & (qn > 0), np.float32(keep) * qn, qn).astype(np.float32)
    own = np.asarray(is_open).astype(bool).copy()
    NF = len(qn)
    F = np.arange(NF)
    for d in range(1, min(int(reach), NF - 1 if circular else NF) + 1):
        for sgn in (-1, 1):
            G = F + sgn * d
            if circular:
                G = G % NF
                valid = G != F
            else:
                valid = (G >= 0) & (G < NF)
                G = np.clip(G, 0, NF - 1)
            q = qn[G]
            own &= ~valid | (qn > q) | ((qn == q) & (F < G))
    return own


class PSK_Decoders(DecoderBank):
    """The decoder bank on a borrowed ``Channelizer`` (which it resets, and which must be fed only through it)."""
    KIND, DESTROY = "psk", "pysdr_psk_destroy"

    def __init__(self, chan, S, max_out=256, cfg=None):
        super().__init__(chan, max_out)
        self.S, self.nsub = int(S), 4 * int(S)
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
        """dict of float32 e [nfine][S], qn, qd, cr, ci [nfine] and int32 pt, cnt, sh, open, seen [nfine]"""
        e = np.empty((self.S, self.nfine), np.float32)
        f = np.empty((4, self.nfine), np.float32)
        ints = np.empty((5, self.nfine), np.int32)
        self._call("state", _lib.as_pf(e), _lib.as_pf(f), ints.ctypes.data_as(C.POINTER(C.c_int32)))
        out = {"e": np.ascontiguousarray(e.T)}
        for i, k in enumerate(STATE_FLOATS):
            out[k] = f[i].copy()
        for i, k in enumerate(STATE_INTS):
            out[k] = ints[i].copy()
        return out


class PSK_Skimmer(Skimmer):
    """Wideband IQ at ``fs`` -> a channelizer of M = 4 D rows S baud / 4 apart at S baud samples per second -> NSUB = 4 S
    decoders inside every row, fine row F at ``freqs_fine[F]`` Hz (signed) -> the text of the stations, each on the fine
    row that owns it."""

    def __init__(self, fs, baud=31.25, channels=None, device=0, max_in=1 << 22, max_out=256, chan=None):
        self.fs, self.baud = float(fs), float(baud)
        if chan is None:
            self.S, self.D, self.M = shape(fs, baud)
            self.nsub = 4 * self.S
            nk = self.M if channels is None else int(channels[1])
            plan(nk, self.S, max_out, params())                          # a bad shape fails here, with or without a device
            self.h = prototype(fs, self.M, baud, self.S)
            self.chan = Channelizer(fs, self.M, self.D, self.h, channels, device, max_in)
        else:
            # a ready channelizer of either kind, adopted and owned: rows S baud / 4 apart at S baud samples per second
            self.chan = chan
            s = chan.fs_out / self.baud
            self.S, self.D, self.M = int(round(s)), chan.D, chan.M
            if abs(s - self.S) > 1e-9 * s or self.S not in (8, 12) or chan.M != 4 * chan.D or float(fs) != chan.fs:
                raise ValueError(f"PSK_Skimmer: the channelizer's rows (fs {chan.fs}, fs_out {chan.fs_out}, M / D = {chan.M / chan.D}) "
                                 f"are not at 8 or 12 samples per symbol of {baud} baud with M / D = 4 at fs = {fs}")
            self.nsub = 4 * self.S
            self.h = chan.prototypes
        self.dec = PSK_Decoders(self.chan, self.S, max_out)
        self.nk, self.nfine, self.fs_out = self.chan.nk, self.dec.nfine, self.chan.fs_out
        self.freqs = self.chan.freqs
        q = 2 * np.arange(self.nsub) - self.nsub + 1
        self.freqs_fine = (self.freqs[:, None] + q[None, :] * (self.baud / 32)).reshape(-1)
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
        """The decoders' state: the raw fields of ``PSK_Decoders.state`` plus coh = qn / qd (1 for a BPSK signal on tune, 0
        for noise), freq = freqs_fine and open as bool, [nfine] each."""
        st = self.dec.state()
        with np.errstate(divide="ignore", invalid="ignore"):
            st["coh"] = st["qn"].astype(np.float64) / st["qd"].astype(np.float64)
        st["freq"] = self.freqs_fine.copy()
        st["open"] = st["open"].astype(bool)
        return st
