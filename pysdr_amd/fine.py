"""Fine channelizer: two channelizer stages for bands wider than 4096 channels of the wanted width (DESIGN.md 3 item 20;
kernel ``fine.hip``, host half ``api_fine.hip``).  A first-stage ``Channelizer`` (M1, D1) cuts the band into coarse rows;
a second, batched stage runs an M2-channel channelizer on every coarse row that is needed, on the device and in the same
stream, and keeps the ``Q = M2 D1 / M1`` channels inside the row's own spacing.  The kept channels of all coarse rows form
one raster of ``Mf = M1 Q`` fine channels ``fs / Mf`` apart at ``fs / (D1 D2)`` samples per second.  Everything but the shape,
the create call and the taps is ``channelizer.ChannelizerCore``, which is also all that ``CW_Decoders``, ``PSK_Decoders`` and
the bank's C object know of a channelizer, so they run on this one unchanged."""
from __future__ import annotations

import numpy as np
from scipy.signal import firwin

from . import _lib
from ._lib import check
from .channelizer import ChannelizerCore
from .design import channelizer_taps

NG_MAX = 1 << 16


def plan(M1, D1, M2, D2, ntaps1=None, ntaps2=None, g_first=0, ng=None):
    """What a fine channelizer of this shape is and launches (no device needed): dict of Q, Mf, D, C2, the first coarse row
    and the number of coarse rows used, frames per workgroup, LDS bytes, history kept per row, taps per branch and radices
    of the second stage.  Raises PysdrError outside the rules."""
    M1, D1, M2, D2 = int(M1), int(D1), int(M2), int(D2)
    n1 = 8 * M1 if ntaps1 is None else int(ntaps1)
    n2 = 8 * M2 if ntaps2 is None else int(ntaps2)
    if ng is None:
        Mf = M1 * (M2 * D1 // M1) if M1 > 0 and D1 > 0 else 0
        ng = max(1, min(Mf, NG_MAX))
    v = _lib.plan_call("pysdr_chan_fine_plan", 16, M1, D1, M2, D2, n1, n2, int(g_first), int(ng))
    return {"Q": v[0], "Mf": v[1], "D": v[2], "C2": v[3], "k1_first": v[4], "nk1": v[5], "frames_per_wg": v[6], "lds_bytes": v[7],
            "history": v[8], "taps_per_branch": v[9], "radices": v[11:11 + v[10]]}


def prototype1(fs, M1, D1, M2=None):
    """The first stage's default prototype: Kaiser(8.0) windowed-sinc low-pass cut at fs1 / 2 = fs / (2 D1), of 8 M1 taps
    for M1 / D1 = 2 and 4 M1 for 4, sum 1.  A coarse row's kept channels reach half its spacing plus one fine spacing from
    its centre: the response is flat within 0.001 dB out to fp = fs / (2 M1) + df and at least 80 dB down from fs1 - fp
    on, where the aliases of that band begin (for Q >= 8)."""
    M1, D1 = int(M1), int(D1)
    return firwin((8 if M1 // D1 == 2 else 4) * M1, 0.5 * float(fs) / D1, window=("kaiser", 8.0), fs=float(fs))


def shape(fs, fs_out, C2):
    """-> (M1, D1, M2, D2): among D1 D2 = fs / fs_out with M1 = 2 D1 and M2 = C2 D2 >= 32 the valid shape with the largest
    M1; ValueError if there is none."""
    d = float(fs) / float(fs_out)
    D = int(round(d))
    best = None
    if D >= 1 and abs(d - D) <= 1e-9 * max(d, 1.0):
        for D1 in range(1, min(D, 2048) + 1):
            if D % D1:
                continue
            D2 = D // D1
            if int(C2) * D2 < 32:
                continue
            try:
                plan(2 * D1, D1, int(C2) * D2, D2, g_first=0, ng=1)
            except _lib.PysdrError:
                continue
            best = (2 * D1, D1, int(C2) * D2, D2)
    if best is None:
        raise ValueError(f"no fine channelizer for fs = {fs}, fs_out = {fs_out}, M2 / D2 = {C2}: fs / fs_out must be an integer "
                         f"D1 D2 with M1 = 2 D1 and M2 = C2 D2 >= 32 inside the rules of pysdr_chan_fine_plan")
    return best


def channels_for(band, fs, M1, D1, M2):
    """-> (g_first, ng): the fine channels whose centres lie in ``band = (f_lo, f_hi)`` Hz from the band's centre"""
    Q = int(M2) * int(D1) // int(M1)
    Mf = int(M1) * Q
    df = float(fs) / Mf
    lo, hi = int(np.ceil(band[0] / df - 1e-9)), int(np.floor(band[1] / df + 1e-9))
    if hi < lo:
        raise ValueError(f"no fine channel centre in {band} Hz (spacing {df} Hz)")
    return lo % Mf, hi - lo + 1


class FineChannelizer(ChannelizerCore):
    """``channels``: None = all Mf rows, or ``(g_first, ng)``: the circular range of fine channels g_first, g_first + 1, ...
    (mod Mf).  Row a of every output is fine channel ``(g_first + a) % Mf`` at ``freqs[a]`` Hz (signed)."""

    def __init__(self, fs, M1, M2, D1=None, D2=None, h1=None, h2=None, channels=None, device=0, max_in=1 << 22):
        self.fs, self.M1, self.M2 = float(fs), int(M1), int(M2)
        self.D1 = self.M1 // 2 if D1 is None else int(D1)
        self.D2 = self.M2 // 2 if D2 is None else int(D2)
        h1 = prototype1(fs, self.M1, self.D1, self.M2) if h1 is None else np.asarray(h1, np.float64)
        h2 = channelizer_taps(self.M2) if h2 is None else np.asarray(h2, np.float64)
        self.device, self.max_in = int(device), int(max_in)
        self.max_taps1, self.max_taps2 = max(len(h1), 8 * self.M1), max(len(h2), 8 * self.M2)   # what a later set_taps may bring
        g_first, ng = (0, None) if channels is None else (int(channels[0]), int(channels[1]))
        p = plan(self.M1, self.D1, self.M2, self.D2, len(h1), len(h2), g_first, ng)   # a bad shape fails here, with or without a device
        self.Q, self.M, self.D = p["Q"], p["Mf"], p["D"]
        self.k_first, self.nk = g_first, self.M if ng is None else ng
        self.k1_first, self.nk1 = p["k1_first"], p["nk1"]
        self.frames_per_wg = p["frames_per_wg"]
        self._start("pysdr_chan_fine_create", (self.device, self.M1, self.D1, self.M2, self.D2, self.k_first, self.nk, self.max_taps1,
                                               self.max_taps2, self.max_in), (h1, h2))

    run_in_taps = property(lambda self: len(self.h1) + self.D1 * (len(self.h2) - 1),
                           doc="the equivalent prototype length in input samples")
    prototypes = property(lambda self: (self.h1, self.h2))

    def set_taps(self, h1, h2):
        """New prototypes from the next call on; each stage applies its own to the whole window of that call's outputs."""
        h1, h2 = np.ascontiguousarray(h1, np.float64), np.ascontiguousarray(h2, np.float64)
        check(self._L.pysdr_chan_fine_set_taps(self._h, _lib.as_pd(h1), len(h1), _lib.as_pd(h2), len(h2)), "pysdr_chan_fine_set_taps")
        self.h1, self.h2 = h1, h2
