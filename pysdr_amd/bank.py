"""Channel bank: AM / NFM audio, AGC and squelch on every channel of a raster (kernels ``bank.hip``,
host half ``api_objects.hip``).  A
``Channelizer`` delivers the rows; every row then gets what a sub-receiver tuned there would do behind its ``rx.iq`` --
detector, real AF low-pass, block AGC (AM), noise squelch (NFM) -- with one call as the AGC block.  One mode, one AF
filter, one squelch threshold and one AGC setting hold for the whole bank.  ``SidebandBank`` adds the complex-tap modes
USB, LSB and CW."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .channelizer import Channelizer
from .design import af_bank_cmpx, af_bank_real, cw_taps
from .tables import AF_BWs, MODE_INDEX, index_of_bw

BANK_MODES = ("AM", "NFM")
SIDEBAND_MODES = ("USB", "LSB", "CW")
BFO_DEFAULT = 700.0        # Hz, the reference's CW pitch


def plan(nk, ntaps_af, max_out):
    """What a bank of this shape launches (no device needed): dict of outputs per workgroup, threads, LDS bytes,
    workgroups per row, history samples kept per row.  Raises PysdrError outside the rules."""
    v = _lib.plan_call("pysdr_bank_plan", 8, int(nk), int(ntaps_af), int(max_out))
    return {"tile": v[0], "threads": v[1], "lds_bytes": v[2], "tiles_per_row": v[3], "history": v[4], "taps_padded": v[5]}


def af_taps(fs_out, ntaps, af_bw):
    """The real AF low-pass of a sub-receiver in AM / NFM: the row of ``rx.demod.filter_bank_real`` whose label is af_bw
    Hz ('Max', a unit impulse, for 0 or a width without a label)."""
    idx = index_of_bw(af_bw, AF_BWs, 0) if af_bw else 0
    return af_bank_real(fs_out, ntaps, [AF_BWs[idx]])[0]


def sideband_taps(fs_out, ntaps, mode, af_bw, bfo=BFO_DEFAULT):
    """The complex AF taps (complex128) of a sub-receiver in USB / LSB -- the row of ``rx.demod.filter_bank_cmpx`` picked
    as ``af_taps`` picks its row ('Max' for 0 or a width without a label), conjugated for LSB -- or in CW: a band-pass of
    af_bw Hz (0: the widest) around the BFO pitch."""
    if mode == "CW":
        return cw_taps(fs_out, ntaps, af_bw, bfo)
    if mode not in ("USB", "LSB"):
        raise _lib.PysdrError(f"sideband_taps: mode {mode!r} is not one of {SIDEBAND_MODES}")
    idx = index_of_bw(af_bw, AF_BWs, 0) if af_bw else 0
    c = af_bank_cmpx(fs_out, ntaps, [AF_BWs[idx]])[0]
    return np.conj(c) if mode == "LSB" else c


class ChannelBank(_lib.Handle):
    """Row a of every output is channel ``(k_first + a) % M`` at ``freqs[a]`` Hz, as for ``Channelizer``."""
    MODES = BANK_MODES
    DESTROY = "pysdr_bank_destroy"
    chan = None

    def __init__(self, fs, M, D=None, h=None, channels=None, mode="NFM", af_bw=4e3, ntaps_af=255, squelch=0.0, agc=True,
                 device=0, max_in=1 << 22):
        self.ntaps_af = int(ntaps_af)
        if mode not in self.MODES:
            raise _lib.PysdrError(f"{type(self).__name__}: mode {mode!r} is not one of {self.MODES}")
        nk = int(M) if channels is None else int(channels[1])
        plan(nk, self.ntaps_af, 1)                                    # a bad shape fails here, with or without a device
        self.chan = Channelizer(fs, M, D, h, channels, device, max_in)
        self.fs, self.M, self.D, self.nk = self.chan.fs, self.chan.M, self.chan.D, self.chan.nk
        self.freqs, self.fs_out = self.chan.freqs, self.chan.fs_out
        start = mode if mode in BANK_MODES else BANK_MODES[0]        # create names a real-tap mode; set_mode below sets the real one
        self._create("pysdr_bank_create", self.chan._h, self.fs_out, MODE_INDEX[start], self.ntaps_af)
        self.mode, self.af_bw = mode, float(af_bw)
        self.set_mode(mode, af_bw)
        self._agc, self._squelch = True, 0.0
        self.agc = agc
        self.squelch = squelch
        self.last_n_out = 0

    def _release(self):
        if self.chan is not None:
            self.chan.close()                                         # after the bank, which holds a pointer into it

    def n_out_for(self, n):
        return self.chan.n_out_for(n)

    def set_mode(self, mode, af_bw=None):
        """Mode and AF filter from the next call on, for the whole AF window of that call's outputs."""
        if mode not in self.MODES:
            raise _lib.PysdrError(f"{type(self).__name__}: mode {mode!r} is not one of {self.MODES}")
        bw = self.af_bw if af_bw is None else float(af_bw)
        af = np.ascontiguousarray(af_taps(self.fs_out, self.ntaps_af, bw), np.float64)
        check(self._L.pysdr_bank_set_mode(self._h, MODE_INDEX[mode], _lib.as_pd(af), len(af)), "pysdr_bank_set_mode")
        self.mode, self.af_bw, self.af = mode, bw, af

    @property
    def agc(self):
        return self._agc

    @agc.setter
    def agc(self, on):
        check(self._L.pysdr_bank_set_agc(self._h, int(bool(on)), 0.5), "pysdr_bank_set_agc")
        self._agc = bool(on)

    @property
    def squelch(self):
        return self._squelch

    @squelch.setter
    def squelch(self, thresh):
        check(self._L.pysdr_bank_set_squelch(self._h, float(thresh)), "pysdr_bank_set_squelch")
        self._squelch = float(thresh)

    def reset(self):
        check(self._L.pysdr_bank_reset(self._h), "pysdr_bank_reset")
        self.chan.n_in = 0
        self.last_n_out = 0

    def _process(self, x, am):
        x = np.ascontiguousarray(x, np.complex64)
        n_out = C.c_int(0)
        pa, pitch = (None, 0) if am is None else (C.c_void_p(am.ctypes.data), max(am.shape[1], 1))
        check(self._L.pysdr_bank_process(self._h, C.c_void_p(x.ctypes.data), len(x), 0, pa, pitch, 0, C.byref(n_out)),
              "pysdr_bank_process")
        self.chan.n_in += len(x)
        self.last_n_out = n_out.value
        return n_out.value

    def push(self, x):
        """complex64 [n] -> float32 [nk, n_out]: the audio of every channel; the call is one AGC block"""
        am = np.empty((self.nk, self.n_out_for(len(x))), np.float32)
        n_out = self._process(x, am)
        assert n_out == am.shape[1], (n_out, am.shape)
        return am

    def push_device(self, d_x, n, sync=True):
        """n complex samples at the device pointer d_x; the results stay on the device (``fetch``).  Returns n_out."""
        n_out = C.c_int(0)
        check(self._L.pysdr_bank_process(self._h, C.c_void_p(d_x), int(n), 1, None, 0, 0, C.byref(n_out)), "pysdr_bank_process")
        self.chan.n_in += int(n)
        self.last_n_out = n_out.value
        if sync:
            self.sync()
        return n_out.value

    def fetch(self, rows, am=True, iq=False):
        """The last call's outputs of the named rows: float32 [len(rows), n_out] audio and / or complex64 channel samples
        (n_out = 0 after a call that completed no output)."""
        rows = np.ascontiguousarray(rows, np.int32)
        n = self.last_n_out
        a = np.empty((len(rows), n), np.float32) if am else None
        y = np.empty((len(rows), n), np.complex64) if iq else None
        check(self._L.pysdr_bank_fetch(self._h, _lib.as_pi(rows), len(rows), None if a is None else _lib.as_pf(a),
                                       None if y is None else y.ctypes.data_as(C.POINTER(C.c_float)), max(n, 1)),
              "pysdr_bank_fetch")
        return (a, y) if am and iq else (a if am else y)

    def push_open(self, x):
        """-> (rows, am[rows]): only the channels whose gate is open after this call are downloaded (the scanner's use)"""
        n_out = self._process(x, None)
        rows = np.flatnonzero(self.open).astype(np.int32)
        if n_out == 0:
            return rows, np.empty((len(rows), 0), np.float32)
        return rows, self.fetch(rows)

    def iq(self, rows=None):
        """The last call's channel samples of those rows (all rows: None), bit for bit the channelizer's."""
        return self.fetch(np.arange(self.nk) if rows is None else rows, am=False, iq=True)

    def state(self):
        """dict of float32 [nk] agc (smoothed block peak), gain, maxbuf (last block peak), level (squelch) and bool open"""
        out = {k: np.empty(self.nk, np.float32) for k in ("agc", "gain", "maxbuf", "level")}
        op = np.empty(self.nk, np.uint8)
        check(self._L.pysdr_bank_state(self._h, _lib.as_pf(out["agc"]), _lib.as_pf(out["gain"]), _lib.as_pf(out["maxbuf"]),
                                       _lib.as_pf(out["level"]), op.ctypes.data_as(C.POINTER(C.c_uint8))), "pysdr_bank_state")
        out["open"] = op.astype(bool)
        return out

    @property
    def open(self):
        return self.state()["open"]

    @property
    def level(self):
        return self.state()["level"]

    @property
    def agc_state(self):
        return self.state()["agc"]

    def sync(self):
        check(self._L.pysdr_bank_sync(self._h), "pysdr_bank_sync")


class SidebandBank(ChannelBank):
    """A ``ChannelBank`` that also runs USB, LSB and CW: complex AF taps, the real part of the filter output as audio, in
    CW behind a BFO of ``bfo`` Hz whose phase follows the absolute output index.  The block AGC is active in these modes
    as in AM; they have no squelch: a threshold is ignored, every gate stays open."""
    MODES = BANK_MODES + SIDEBAND_MODES

    def __init__(self, fs, M, D=None, h=None, channels=None, mode="USB", af_bw=3e3, ntaps_af=255, squelch=0.0, agc=True,
                 device=0, max_in=1 << 22, bfo=BFO_DEFAULT):
        self.bfo = float(bfo)
        super().__init__(fs, M, D, h, channels, mode, af_bw, ntaps_af, squelch, agc, device, max_in)

    def set_mode(self, mode, af_bw=None, bfo=None):
        """Mode, AF filter and (CW) BFO pitch from the next call on, for the whole AF window of that call's outputs."""
        if mode not in self.MODES:
            raise _lib.PysdrError(f"SidebandBank: mode {mode!r} is not one of {self.MODES}")
        if bfo is not None:
            self.bfo = float(bfo)
        if mode in BANK_MODES:
            return super().set_mode(mode, af_bw)
        bw = self.af_bw if af_bw is None else float(af_bw)
        af = np.ascontiguousarray(sideband_taps(self.fs_out, self.ntaps_af, mode, bw, self.bfo), np.complex128)
        re, im = np.ascontiguousarray(af.real), np.ascontiguousarray(af.imag)
        check(self._L.pysdr_bank_set_mode_cplx(self._h, MODE_INDEX[mode], _lib.as_pd(re), _lib.as_pd(im), len(af), self.bfo),
              "pysdr_bank_set_mode_cplx")
        self.mode, self.af_bw, self.af = mode, bw, af
