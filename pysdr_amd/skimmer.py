"""What the CW, the PSK31 and the RTTY raster skimmer share on the host: a bank of decoders on a borrowed channelizer, and
the object that owns both and turns the bank's event words into text.  The event-word layouts, the settings and the
tables stay with ``cw.py``, ``psk.py`` and ``fsk.py``."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

_pi32 = C.POINTER(C.c_int32)


class DecoderBank(_lib.Handle):
    """A decoder bank on a borrowed channelizer (which it resets, and which must be fed only through it).  A kind names
    its entry points ``pysdr_<KIND>_*``, sets ``cfg`` and ``plan`` and then calls ``_open`` with its number of decoder rows."""
    KIND = None                                                          # and DESTROY, "pysdr_<KIND>_destroy"

    def __init__(self, chan, max_out):
        self.chan = chan
        self.nk, self.D, self.fs_out = chan.nk, chan.D, chan.fs_out
        self.max_out = int(max_out)

    def _call(self, what, *args):
        name = f"pysdr_{self.KIND}_{what}"
        check(getattr(self._L, name)(self._h, *args), name)

    def _open(self, nrows, *args):
        """the C object: ``args`` are what its create call takes between the channelizer and ``max_out``"""
        self.nrows, self.cap = nrows, self.plan["cap"]
        self._create(f"pysdr_{self.KIND}_create", self.chan._h, *args, self.max_out)
        self.chan.n_in = 0
        self._counts = np.zeros(nrows, np.int32)
        self.last_n_out = 0

    def reset(self):
        self._call("reset")
        self.chan.n_in = 0
        self.last_n_out = 0

    def sync(self):
        self._call("sync")

    def max_samples(self):
        """the longest next call: it completes at most max_out outputs and holds at most max_in samples"""
        return min(self.chan.max_in, (-self.chan.n_in) % self.D + self.max_out * self.D)

    def fetch(self, rows):
        """The last call's event slots [len(rows)][cap] of the named decoder rows (int32 words; only the first counts[row]
        of a row are events)."""
        rows = np.ascontiguousarray(rows, np.int32)
        ev = np.zeros((len(rows), self.cap), np.int32)
        self._call("fetch", _lib.as_pi(rows), len(rows), ev.ctypes.data_as(_pi32), self.cap)
        return ev

    def _decode(self, x, n, on_device, events, *more):
        """One process call: host samples (complex64 [n]) or a device pointer; ``more``: the kind's further outputs.
        -> dict of n_out, m0 (the absolute index of the call's first output), counts [nrows] and events [nrows][cap]
        ("all"); any other ``events`` but None brings the counts alone, None nothing at all."""
        self._check_open()
        if on_device:
            ptr, n = C.c_void_p(int(x)), int(n)
        else:
            x = np.ascontiguousarray(x, np.complex64)
            ptr, n = C.c_void_p(x.ctypes.data), len(x)
        m0 = -(-self.chan.n_in // self.D)
        n_out = C.c_int(0)
        counts = ev = pc = pe = None
        if events is not None:
            counts = self._counts
            pc = counts.ctypes.data_as(_pi32)
        if events == "all":
            ev = np.zeros((self.nrows, self.cap), np.int32)
            pe = ev.ctypes.data_as(_pi32)
        self._call("process", ptr, n, 1 if on_device else 0, C.byref(n_out), pc, pe, self.cap, *more)
        self.chan.n_in += n
        self.last_n_out = n_out.value
        return dict(n_out=n_out.value, m0=m0, counts=None if counts is None else counts.copy(), events=ev)


class Skimmer:
    """Owns a channelizer ``chan`` of either kind and the decoder bank ``dec`` on it; ``text[row]`` gains what ``push``
    returns.  A kind builds the two, and says in ``_events`` which of a call's events come off the device."""
    chan = dec = None
    SILENT = ()                                                          # event texts that ``text`` does not gain

    def close(self):
        if self.dec is not None:
            self.dec.close()                                             # the bank holds a pointer into the channelizer: it goes first
        if self.chan is not None:
            self.chan.close()

    __del__ = _lib.Handle.__del__

    def sync(self):
        self.dec.sync()

    def push(self, x):
        """complex64 [n] -> the events (m, row, text) of the outputs this input completes, sorted by (m, row); m is the
        absolute output index since create / reset.  ``text`` gains them.  The input goes through in calls of at most
        ``dec.max_samples()``."""
        x = np.ascontiguousarray(x, np.complex64)
        ev, i = [], 0
        while i < len(x):
            n = min(len(x) - i, self.dec.max_samples())
            ev += self._events(x[i:i + n])
            i += n
        ev.sort(key=lambda e: (e[0], e[1]))
        for _, row, ch in ev:
            if ch not in self.SILENT:
                self.text[row] += ch
        return ev
