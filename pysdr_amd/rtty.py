"""Wideband RTTY filterbank on the baseband-IQ tap: the FFT-heavy front of
the reference's RTTY process (``rtty.py:780-868``), fed with ``rx.iq`` like the reference feeds
its queue (``receiver.py:286-290``).  For every 22 ms symbol it produces four ``line``s, the
sliding Kaiser(8.6)-windowed, zero-padded FFT in dB, fftshifted and flipped
(``rtty.py:836-846``), computed in batches on the GPU through the spectrum entry points of the
C ABI (window / zero-pad / rocFFT / dB / fftshift kernels); ``mark_space`` picks the two bins a
decoder compares (``rtty.py:485-492``).

``RTTY_Decoders`` is the reference's bank of Baudot decoders (``RTTY_Decoder``, ``rtty.py:431-701``)
and its signal finder (``find_sigs``, ``:744-764``) on the GPU, one decoder on every bin of a range
(kernels ``rtty.hip``, host half ``api_objects.hip``); ``RTTY_Skimmer`` hands the filterbank's device lines to it without a download."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import check


class RTTY_Params:
    """``rtty.py:376-404``."""

    def __init__(self, FS_OUT, mark_bins=(559,)):
        self.T = 22e-3
        self.FSK_SHIFT = 170
        self.SAMPS_PER_BIT = 4
        STOP_BITS = 1.5
        self.M = int(4 * (1 + 5 + STOP_BITS))
        self.N = int(round(self.T * FS_OUT))
        self.NFFT = 1 << int(math.ceil(math.log2(self.N)))
        NSTEP = self.N / 4.
        self.NSTART = [int(NSTEP * i + 0.5) for i in range(4)]
        bin_size = FS_OUT / float(self.NFFT)
        self.NBINS = int(round(self.FSK_SHIFT / bin_size))
        self.frq = np.fft.fftshift(np.fft.fftfreq(self.NFFT, d=1000. / FS_OUT)) + 0
        self.mark_bins = np.array(mark_bins)


class RTTY_Filterbank(_lib.Handle):
    DESTROY = "pysdr_spectrum_destroy"
    _d_in = _d_out = None

    def __init__(self, FS_OUT, max_symbols=512, device=0, mark_bins=(559,)):
        _lib.require_gpu()
        self.RTTY = RTTY_Params(FS_OUT, mark_bins)
        p = self.RTTY
        self.device = device
        self.max_symbols = int(max_symbols)
        self.window = np.kaiser(p.N, 8.6)
        win = np.ascontiguousarray(self.window, np.float32)
        # the four quarter-symbol lines of a symbol start N/4 apart: when that is a whole number of
        # samples (48 kHz: N = 1056) all 4k lines of k symbols are ONE batch with hop N/4
        self._uniform = all(int(p.NSTART[i]) * 4 == i * p.N for i in range(4))
        self._create("pysdr_spectrum_create", device, p.N, p.NFFT, 4 * self.max_symbols, _lib.as_pf(win))
        self._d_in = C.c_void_p()
        self._d_out = C.c_void_p()
        check(self._L.pysdr_dev_alloc(device, (self.max_symbols + 1) * p.N * 8, C.byref(self._d_in)), "alloc")
        check(self._L.pysdr_dev_alloc(device, 4 * self.max_symbols * p.NFFT * 4, C.byref(self._d_out)), "alloc")
        self._fifo = np.zeros(0, np.complex64)
        self._prev = None

    def _release(self):
        for d in (self._d_in, self._d_out):                              # the two device buffers go after the spectrum object
            if d:
                self._L.pysdr_dev_free(self.device, d)
                d.value = None

    def _staged(self, iq):
        """Append baseband IQ; for every batch of k symbols it completes, upload [prev, k symbols] to the
        device input and yield k (the very first symbol only primes the overlap, ``rtty.py:826-829``)."""
        p = self.RTTY
        self._fifo = np.concatenate((self._fifo, np.ascontiguousarray(iq, np.complex64)))
        while True:
            k = len(self._fifo) // p.N
            if self._prev is None:
                if k == 0:
                    break
                self._prev, self._fifo = self._fifo[:p.N].copy(), self._fifo[p.N:]
                continue
            if k == 0:
                break
            k = min(k, self.max_symbols)
            cur, self._fifo = self._fifo[:k * p.N], self._fifo[k * p.N:]
            x = np.ascontiguousarray(np.concatenate((self._prev, cur)))
            check(self._L.pysdr_dev_upload(self.device, self._d_in, C.c_void_p(x.ctypes.data), x.nbytes), "upload")
            yield k
            self._prev = cur[-p.N:].copy()

    def _batch_uniform(self, k):
        # one launch sequence: frame 4 s + i starts at s N + i N/4; the unflipped lines stay at _d_out
        check(self._L.pysdr_spectrum_batch(self._h, self._d_in, 4 * k, self.RTTY.N // 4, self._d_out), "spectrum_batch")
        check(self._L.pysdr_spectrum_sync(self._h), "spectrum_sync")

    def push_device(self, iq, sink):
        """``push`` without the download, for rates with N % 4 == 0: ``sink(d_lines, nlines)`` gets each batch's
        lines [nlines][NFFT] in device memory, NOT flipped (valid until the next batch)."""
        if not self._uniform:
            raise ValueError(f"device lines need N % 4 == 0 (N = {self.RTTY.N})")
        for k in self._staged(iq):
            self._batch_uniform(k)
            sink(self._d_out.value, 4 * k)

    def push(self, iq):
        """Append baseband IQ; returns the lines [4*k, NFFT] of the k symbols completed by it
        (the very first symbol only primes the overlap, ``rtty.py:826-829``)."""
        p = self.RTTY
        out = []
        for k in self._staged(iq):
            lines = np.empty((4 * k, p.NFFT), np.float32)
            if self._uniform:
                # one launch sequence, one download
                self._batch_uniform(k)
                check(self._L.pysdr_dev_download(self.device, C.c_void_p(lines.ctypes.data), self._d_out, lines.nbytes),
                      "download")
                out.append(lines[:, ::-1].copy())                # np.flipud of the shifted spectrum
                continue
            tmp = np.empty((k, p.NFFT), np.float32)
            for i in range(4):
                # frames of quarter i: start NSTART[i] + s*N, s = 0..k-1
                src = C.c_void_p(self._d_in.value + p.NSTART[i] * 8)
                check(self._L.pysdr_spectrum_batch(self._h, src, k, p.N, self._d_out), "spectrum_batch")
                check(self._L.pysdr_spectrum_sync(self._h), "spectrum_sync")
                check(self._L.pysdr_dev_download(self.device, C.c_void_p(tmp.ctypes.data), self._d_out, tmp.nbytes),
                      "download")
                lines[i::4] = tmp[:, ::-1]                       # np.flipud of the shifted spectrum
            out.append(lines)
        if not out:
            return np.zeros((0, p.NFFT), np.float32)
        return np.concatenate(out)

    def mark_space(self, lines, mark_bin=None):
        """``rtty.py:485-492``: (mark, space) per line; ``signal = mark - space``."""
        mb = int(self.RTTY.mark_bins[0] if mark_bin is None else mark_bin)
        return lines[:, mb], lines[:, mb + self.RTTY.NBINS]


# RTTY_Decoder.baudot (rtty.py:573-582), as the reference has them: FIGS 5 is the two characters '\g'
LTRS = ['\0', 'E', '\n', 'A', ' ', 'S', 'I', 'U', '\r', 'D', 'R', 'J',
        'N', 'F', 'C', 'K', 'T', 'Z', 'L', 'W', 'H', 'Y', 'P', 'Q', 'O', 'B', 'G',
        '<FIGS>', 'M', 'X', 'V', '<LTRS>']
FIGS = ['\0', '3', '\n', '-', ' ', '\\g', '8', '7', '\r', '$', '4', "'",
        ',', '!', ':', '(', '5', '"', ')', '2', '#', '6', '0', '1', '9', '?', '&',
        '<FIGS>', '.', '/', ';', '<LTRS>']


def code_text(code):
    """A decoder's emitted code (sym + 32 * FIGS shift) -> the reference's character(s)."""
    return (FIGS if code >= 32 else LTRS)[code & 31]


class RTTY_Decoders(_lib.Handle):
    """The reference's RTTY decoders (``RTTY_Decoder``, ``rtty.py:431-701``) on every bin of a range, with its
    signal finder (``find_sigs``, ``:744-764``), driven as its executive drives them (``:847-853``).
    ``bins=None``: a decoder on every bin with a space bin, [0, NFFT - NBINS); otherwise the bins given (the
    decoders run on [min, max] and events are reported for the given ones).  ``find_bins`` is the reference's
    ``YLIM``: the finder scans the mark bins [lo, hi - NBINS).  Lines are numbered 1, 2, ... from construction
    or ``reset()``; characters are decided at lines n = 30 j."""
    DESTROY = "pysdr_rtty_destroy"

    def __init__(self, FS_OUT, bins=None, find_bins=(800, 1250), device=0, max_lines=2048):
        _lib.require_gpu()
        self.RTTY = RTTY_Params(FS_OUT)
        p = self.RTTY
        top = p.NFFT - p.NBINS
        if bins is None:
            self.bins = np.arange(0, top)
        else:
            self.bins = np.unique(np.asarray(list(bins), np.int64))
            if len(self.bins) == 0:
                raise ValueError("no decoder bins")
        self.bin_lo, self.bin_hi = int(self.bins[0]), int(self.bins[-1]) + 1
        self._sel = None if len(self.bins) == self.bin_hi - self.bin_lo else self.bins - self.bin_lo
        self.find_lo, self.find_hi = int(find_bins[0]), int(find_bins[1]) - p.NBINS
        self.device = device
        self.max_lines = int(max_lines)
        self._create("pysdr_rtty_create", device, p.NFFT, p.NBINS, self.bin_lo, self.bin_hi, self.find_lo, self.find_hi, self.max_lines)
        self.nb = self.bin_hi - self.bin_lo
        nd = self.max_lines // p.M + 1
        self._codes = np.empty((nd, self.nb), np.int32)
        self._t = np.empty((nd, self.nb), np.int64)
        self._snr = np.empty((nd, self.nb), np.float64)
        self._ndet = np.empty(self.max_lines, np.int32)
        self._reset_host()

    def _reset_host(self):
        self.n = 0                                   # lines decoded so far
        self.text = {int(b): '' for b in self.bins}  # per-bin accumulated text
        self.ndet = np.zeros(0, np.int32)            # the finder's count for every line of the last call

    def reset(self):
        check(self._L.pysdr_rtty_reset(self._h), "pysdr_rtty_reset")
        self._reset_host()

    def decode_raw(self, lines, nlines, on_device, flipped, per_line=False):
        """One call of the C ABI on at most ``max_lines`` lines: host lines (float32 [nlines][NFFT]) or a device
        pointer.  -> dict of n (decision lines), codes / t / snr2 [decision][bin - bin_lo], ndet [nlines] and, with
        ``per_line``, isym / best [nlines][bins]."""
        self._check_open()
        nlines = int(nlines)
        if on_device:
            ptr = C.c_void_p(int(lines))
        else:
            lines = np.ascontiguousarray(lines, np.float32)
            if lines.ndim != 2 or lines.shape[1] != self.RTTY.NFFT or lines.shape[0] != nlines:
                raise ValueError(f"lines must be [{nlines}][{self.RTTY.NFFT}]")
            ptr = C.c_void_p(lines.ctypes.data)
        isym = best = None
        if per_line:
            isym = np.empty((nlines, self.nb), np.int32)
            best = np.empty((nlines, self.nb), np.float32)
        nd = C.c_int(0)
        ndet = self._ndet[:nlines]
        check(self._L.pysdr_rtty_decode(self._h, ptr, nlines, 1 if on_device else 0, 1 if flipped else 0,
                                        _lib.as_pi(self._codes), self._t.ctypes.data_as(C.POINTER(C.c_longlong)),
                                        _lib.as_pd(self._snr), C.byref(nd), _lib.as_pi(ndet),
                                        None if isym is None else _lib.as_pi(isym),
                                        None if best is None else _lib.as_pf(best)), "pysdr_rtty_decode")
        M = self.RTTY.M
        j0 = self.n // M + 1
        self.n += nlines
        k = nd.value
        out = dict(n=M * np.arange(j0, j0 + k, dtype=np.int64), codes=self._codes[:k].copy(), t=self._t[:k].copy(),
                   snr2=self._snr[:k].copy(), ndet=ndet.copy())
        if per_line:
            out.update(isym=isym, best=best)
        return out

    def _events(self, r):
        codes = r['codes'] if self._sel is None else r['codes'][:, self._sel]
        bins = self.bins if self._sel is not None else np.arange(self.bin_lo, self.bin_hi)
        jj, kk = np.nonzero(codes >= 0)             # row-major: ordered by (n, bin)
        ev = []
        for j, k in zip(jj, kk):
            b, ch = int(bins[k]), code_text(int(codes[j, k]))
            self.text[b] += ch
            ev.append((int(r['n'][j]), b, ch))
        return ev

    def _run(self, lines, nlines, on_device, flipped):
        ev, ndet = [], []
        step = self.max_lines
        for a in range(0, nlines, step):
            m = min(step, nlines - a)
            src = (int(lines) + a * self.RTTY.NFFT * 4) if on_device else lines[a:a + m]
            r = self.decode_raw(src, m, on_device, flipped)
            ev += self._events(r)
            ndet.append(r['ndet'])
        self.ndet = np.concatenate(ndet) if ndet else np.zeros(0, np.int32)
        return ev

    def decode(self, lines):
        """Host lines [L][NFFT] in the reference's order (``RTTY_Filterbank.push``) -> events (n, bin, text)."""
        lines = np.ascontiguousarray(lines, np.float32)
        if lines.ndim != 2 or lines.shape[1] != self.RTTY.NFFT:
            raise ValueError(f"lines must be [L][{self.RTTY.NFFT}]")
        return self._run(lines, len(lines), False, True)

    def decode_device(self, d_lines, nlines, flipped=False):
        """Lines [nlines][NFFT] already in device memory (default: the unflipped order of
        ``pysdr_spectrum_batch``) -> events (n, bin, text)."""
        return self._run(d_lines, nlines, True, flipped)


class RTTY_Skimmer:
    """Baseband IQ at FS_OUT (``rx.iq`` of a Receiver in RTTY mode, ``receiver.py:286-290``) -> filterbank lines on
    the GPU -> the decoder bank, without taking the lines off the device.  Only rates where the four lines of a
    symbol are a whole number of samples apart (N % 4 == 0: 48, 96, 192 kHz)."""

    def __init__(self, FS_OUT, bins=None, find_bins=(800, 1250), device=0, max_symbols=512):
        _lib.require_gpu()
        p = RTTY_Params(FS_OUT)
        if p.N % 4:
            raise ValueError(f"RTTY_Skimmer needs N % 4 == 0 (FS_OUT = {FS_OUT}: N = {p.N})")
        self.fb = RTTY_Filterbank(FS_OUT, max_symbols=max_symbols, device=device)
        self.dec = RTTY_Decoders(FS_OUT, bins=bins, find_bins=find_bins, device=device, max_lines=4 * max_symbols)
        self.RTTY = self.dec.RTTY
        self.ndet = np.zeros(0, np.int32)            # the finder's count for every line of the last push

    @property
    def text(self):
        return self.dec.text

    def push(self, iq):
        """-> the events (n, bin, text) decided by the lines this IQ completes; ``self.ndet``: those lines' finder counts."""
        ev, ndet = [], []

        def sink(d_lines, nlines):
            ev.extend(self.dec.decode_device(d_lines, nlines, flipped=False))
            ndet.append(self.dec.ndet)

        self.fb.push_device(iq, sink)
        self.ndet = np.concatenate(ndet) if ndet else np.zeros(0, np.int32)
        return ev

    def close(self):
        self.dec.close()
        self.fb.close()
