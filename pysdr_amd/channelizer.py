"""Polyphase channelizer: every channel of an M-channel raster in one pass over the wideband input (DESIGN.md 3 item 15;
kernels ``chan.hip``, host half ``api_objects.hip``).  Channel k is centred on k fs / M and comes out at fs / D, exactly as a sub-receiver tuned there with
UP = 1 and the prototype ``h`` would deliver its ``rx.iq`` -- but the input is read once for all of them."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .design import channelizer_taps


def plan(M, D, ntaps, k_first=0, nk=None):
    """What a channelizer of this shape launches (no device needed): dict of radices, frames per workgroup, frames per
    FIR work item, threads, LDS bytes, history length, taps per branch.  Raises PysdrError outside the rules."""
    v = _lib.plan_call("pysdr_chan_plan", 16, int(M), int(D), int(ntaps), int(k_first), int(M if nk is None else nk))
    return {"radices": v[1:1 + v[0]], "frames_per_wg": v[9], "frames_per_item": v[10], "threads": v[11],
            "lds_bytes": v[12], "history": v[13], "taps_per_branch": v[14]}


class ChannelizerCore(_lib.Handle):
    """What the one-stage and the two-stage channelizer have in common, and all that their clients (the bank, the CW and
    PSK decoders) know of them: ``fs``, the raster ``M``, ``D``, ``k_first``, ``nk``, ``freqs``, ``fs_out``, ``max_in``,
    the count ``n_in`` of samples taken since create / reset, the handle, and two things a kind declares: ``run_in_taps``,
    the length of its (equivalent) prototype in input samples, and ``prototypes``, ``h`` or ``(h1, h2)``."""
    DESTROY = "pysdr_chan_destroy"

    def _start(self, create, args, taps):
        """once the kind has its shape and has planned it: the C object, its taps, the raster of its rows"""
        _lib.require_gpu()
        self._create(create, *args)
        self.set_taps(*taps)
        self.fs_out = self.fs / self.D
        k = (self.k_first + np.arange(self.nk)) % self.M
        self.freqs = np.where(k >= (self.M + 1) // 2, k - self.M, k) * (self.fs / self.M)
        self.n_in = 0

    def reset(self):
        check(self._L.pysdr_chan_reset(self._h), "pysdr_chan_reset")
        self.n_in = 0

    def n_out_for(self, n):
        """Outputs the next call of n samples produces: those with s0 <= m D < s0 + n."""
        return -(-(self.n_in + n) // self.D) - -(-self.n_in // self.D)

    def push(self, x):
        """complex64 [n] -> complex64 [nk, n_out]"""
        x = np.ascontiguousarray(x, np.complex64)
        parts = []
        for i in range(0, max(len(x), 1), self.max_in):
            xi = x[i:i + self.max_in]
            cap = self.n_out_for(len(xi))
            y = np.empty((self.nk, cap), np.complex64)
            n_out = C.c_int(0)
            check(self._L.pysdr_chan_process(self._h, C.c_void_p(xi.ctypes.data), len(xi), 0, C.c_void_p(y.ctypes.data),
                                             max(cap, 1), 0, C.byref(n_out)), "pysdr_chan_process")
            assert n_out.value == cap, (n_out.value, cap)
            self.n_in += len(xi)
            parts.append(y)
        return parts[0] if len(parts) == 1 else np.concatenate(parts, axis=1)

    def push_device(self, d_x, n, d_out, pitch, sync=True):
        """Device pointers: n complex samples at d_x -> d_out[a * pitch + i]; returns n_out.  ``sync=False`` only queues
        the work on the channelizer's stream (``sync()`` waits for it)."""
        n_out = C.c_int(0)
        check(self._L.pysdr_chan_process(self._h, C.c_void_p(d_x), int(n), 1, C.c_void_p(d_out), int(pitch), 1,
                                         C.byref(n_out)), "pysdr_chan_process")
        self.n_in += int(n)
        if sync:
            self.sync()
        return n_out.value

    def sync(self):
        check(self._L.pysdr_chan_sync(self._h), "pysdr_chan_sync")


class Channelizer(ChannelizerCore):
    """``channels``: None = all M rows, or ``(k_first, nk)``: the circular range of channels k_first, k_first + 1, ...
    (mod M).  Row a of every output is channel ``(k_first + a) % M`` at ``freqs[a]`` Hz (signed)."""

    def __init__(self, fs, M, D=None, h=None, channels=None, device=0, max_in=1 << 22):
        self.fs, self.M = float(fs), int(M)
        self.D = self.M // 2 if D is None else int(D)
        h = channelizer_taps(self.M) if h is None else np.asarray(h, np.float64)
        self.k_first, self.nk = (0, self.M) if channels is None else (int(channels[0]), int(channels[1]))
        self.device, self.max_in = int(device), int(max_in)
        self.max_taps = max(len(h), 8 * self.M)                      # what a later set_taps may bring
        plan(self.M, self.D, len(h), self.k_first, self.nk)           # a bad shape fails here, with or without a device
        self._start("pysdr_chan_create", (self.device, self.M, self.D, self.k_first, self.nk, self.max_taps, self.max_in), (h,))

    run_in_taps = property(lambda self: len(self.h), doc="the prototype's length in input samples")
    prototypes = property(lambda self: self.h)

    def set_taps(self, h):
        """New prototype from the next call on, for the whole window of that call's outputs (``rx.dec.h``)."""
        h = np.ascontiguousarray(h, np.float64)
        check(self._L.pysdr_chan_set_taps(self._h, _lib.as_pd(h), len(h)), "pysdr_chan_set_taps")
        self.h = h
