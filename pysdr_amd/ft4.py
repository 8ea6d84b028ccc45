"""FT4 skimmer: four Costas arrays and soft bits on a fine raster of the band (kernels ``ft.hip``, host
half ``api_ft.hip``).  4-GFSK at 125 / 6 baud, tones one baud apart, 103 symbols of which 16 are four different Costas
arrays.  A channelizer with M / D = 4 delivers rows at ``S`` samples per symbol; inside every row ``NSUB = S / 2`` decoders
run on the device, one every 10.4 Hz, so that the fine rows ``F = a NSUB + j`` form one uniform raster over all rows.  The
device finds every frame by its sync score and hands out its 174 soft bits in transmission order; with ``decode=True`` it
also runs the LDPC(174,91) decoder and the CRC-14 on them and a record carries ``ok`` and the 77
bits as decoded; the bit scrambler FT4 applies before the CRC is not here, so ``text`` is None.  This file is the mode: its
constants, settings and waveform.  The decoder bank and the skimmer are ``ft.py``'s, told this module as their ``MODE``;
``ft8.py`` is the other mode, and neither knows the other."""
from __future__ import annotations

import sys

import numpy as np

from . import ft as _ft
from . import ft_report as _report
from . import psk as _psk
from ._lib import Ft4Cfg
from .ft import KEEP, LLR_MAX, cfg_dict, hard_bits, owners, steps_done, tables, unit_llr, unpack  # noqa: F401  (importable from here, as they always were)
from .ft_report import CAL, FLOOR_QUANTILE, FLOOR_ROWS, delta, noise_floor, noise_of, refine, snr_db, spots  # noqa: F401
from .ft_pass import pack91, pass_lut, pass_plan, pass_pulse, trial_grid  # noqa: F401

NAME, PLAN_CALL = "FT4", "pysdr_ft4_plan"
_MODE = sys.modules[__name__]
BAUD = 125.0 / 6.0
COSTAS = ((0, 1, 3, 2), (1, 0, 2, 3), (2, 3, 1, 0), (3, 2, 0, 1))   # at symbols 0, 33, 66 and 99
GRAY4 = (0, 1, 3, 2)                             # value v is sent on tone GRAY4[v]
SYMBOLS, DATA, BITS = 103, 87, 174
SYNC_AT = (0, 33, 66, 99)                        # first symbol of the four Costas arrays
FRAME_SECONDS, SLOT_SECONDS, NOMINAL_START = SYMBOLS / BAUD, 7.5, 0.5
STEPS_PER_SYMBOL = 4
EMIT_LAG = 412                                   # an event t0 is emitted at step t0 + 412 ...
HOLD = 417                                       # ... and released once step t0 + 416 is complete: every rival has arrived
SHAPES = (48, 72)                                # row samples per symbol
NB_EXTRA = 6                                     # NB = NSUB + 6: decoder j uses bins j + 2 tone, tone 0 to 3
UNPACK = None                                    # FT4 XORs its 77 bits with a fixed scrambler before the CRC; that vector is not here
REPORT_MODE = 1                                  # PYSDR_REPORT_FT4
TONES = 4
PULSE_SYMBOLS = 5                                # symbols the frequency pulse of ``waveform`` spans (BT = 1)
PULSE_K = np.pi * np.sqrt(2 / np.log(2))
REACH_T = 40                                     # steps a rescan looks to either side of a subtracted frame
TRIAL_DN = 0.25                                  # steps between the trial times
TRIAL_DF = 1.0                                   # Hz between the trial frequencies: FT8's 0.3 Hz scaled by the baud


def report_plan():
    """``ft_report.report_plan`` for this mode: 103 symbols"""
    return _report.report_plan(REPORT_MODE)


def spot_line(rec, f_centre=0.0):
    """``ft_report.spot_line`` on this mode's 7.5 s slots"""
    return _report.spot_line(rec, f_centre, SLOT_SECONDS)


def shape(fs):
    """-> (S, D, M): S = 48 row samples per symbol if fs / (48 baud) is an integer D and the channelizer accepts M = 4 D,
    otherwise S = 72 likewise, otherwise ValueError."""
    return _ft.mode_shape(_MODE, fs)


def prototype(fs, M, S):
    """The channelizer's prototype for the FT4 raster, ``psk.prototype``'s form: cut at fs_out / 2 = S baud / 2, sum 1; flat
    within 0.1 dB out to fp = (NB + 1) baud / 4 + baud and at least 70 dB down from fs_out - fp on."""
    return _psk.prototype(fs, M, BAUD, S)


def fine_channelizer(fs, band, device=0, max_in=1 << 22):
    """A ``fine.FineChannelizer`` for ``FT4_Skimmer(fs, chan=...)`` at a rate ``shape`` refuses: rows S baud / 4 apart whose
    centres lie in ``band = (f_lo, f_hi)`` Hz from the centre, S = 48 where ``fine.shape`` finds a shape, else 72; M2 / D2 =
    4, the second prototype is ``prototype`` at the first stage's output rate, the first ``fine.prototype1``."""
    return _ft.mode_fine_channelizer(_MODE, fs, band, device, max_in)


def params(smin=4.0, hmin=12, pmax=1e18):
    """The settings of DESIGN.md 3 item 23 as the ``_lib.Ft4Cfg`` the C ABI takes."""
    return Ft4Cfg(smin=float(np.float32(smin)), hmin=int(hmin), pmax=float(np.float32(pmax)))


def plan(nk, S, max_out, cfg):
    """What a skimmer of this shape launches (no device needed): dict of rows per workgroup, threads, LDS bytes, tile
    samples, event cap per decoder and call, workgroups, decoders per row, ring depth in steps.  Raises PysdrError
    outside the rules."""
    return _ft.mode_plan(_MODE, nk, S, max_out, cfg)


def tones(bits):
    """174 bits in transmission order -> the frame's 103 tones: the four Costas arrays at symbols 0, 33, 66 and 99, 3 x 29
    data symbols of 2 bits, MSB first, Gray-mapped"""
    bits = np.asarray(bits, np.int64).reshape(DATA, 2)
    g = np.array(GRAY4)[2 * bits[:, 0] + bits[:, 1]]
    return np.concatenate((COSTAS[0], g[:29], COSTAS[1], g[29:58], COSTAS[2], g[58:], COSTAS[3])).astype(np.int64)


def waveform(tones, f0, fs, gfsk=True, ramps=True, phase=0.0):
    """complex128 frame at ``fs``: tone 0 at ``f0`` Hz from the centre, continuous phase, amplitude 1 over the frame's
    symbols.  ``gfsk``: the frequency pulse of a symbol is (erf(k (t + 1/2)) - erf(k (t - 1/2))) / 2, k = pi sqrt(2 / ln 2), t
    in symbols from the symbol's middle (BT = 1; it reaches two symbols to either side), the first and the last tone held
    beyond the frame; otherwise rectangular.  With ``ramps`` one more symbol before and one after the frame hold the first
    and the last tone under a raised-cosine amplitude, as on the air (105 symbols, 5.04 s): THE RETURNED ARRAY THEN STARTS
    AT THE RAMP, and the frame's first Costas symbol -- the skimmer's t0 -- begins one symbol (fs / baud samples) later."""
    from scipy.special import erf
    tones = np.asarray(tones, np.float64)
    if ramps:
        tones = np.concatenate((tones[:1], tones, tones[-1:]))
    sps = float(fs) / BAUD
    n = int(round(len(tones) * sps))
    t = (np.arange(n) + 0.5) / sps                                       # symbols
    k0 = np.minimum(np.floor(t).astype(np.int64), len(tones) - 1)
    if gfsk:
        kk = np.pi * np.sqrt(2 / np.log(2))
        ext = np.concatenate((tones[:1], tones[:1], tones, tones[-1:], tones[-1:]))
        dev = np.zeros(n)
        for d in (-2, -1, 0, 1, 2):                                      # the pulse is below 1e-13 beyond two symbols and a half
            tau = t - (k0 + d) - 0.5
            dev += ext[k0 + d + 2] * 0.5 * (erf(kk * (tau + 0.5)) - erf(kk * (tau - 0.5)))
    else:
        dev = tones[k0]
    ph = np.cumsum(float(f0) + BAUD * dev)
    w = np.exp(1j * (2 * np.pi / float(fs) * ph + phase))
    if ramps:
        first, last = t < 1, t >= len(tones) - 1
        w[first] *= 0.5 * (1 - np.cos(np.pi * t[first]))
        w[last] *= 0.5 * (1 + np.cos(np.pi * (t[last] - (len(tones) - 1))))
    return w


class FT4_Decoders(_ft.FT_Decoders):
    """The decoder bank on a borrowed ``Channelizer``: ``ft.FT_Decoders``' calls on ``pysdr_ft4_*`` with this module's
    constants (an event's t0 is ``t_first + unpack(words)[0] - 412``)."""
    KIND, DESTROY = "ft4", "pysdr_ft4_destroy"
    MODE = _MODE


class FT4_Skimmer(_ft.FT_Skimmer):
    """``ft.FT_Skimmer`` (which describes the records) on this mode: 103 symbols of 4 tones at 125 / 6 baud, rows at S baud =
    1000 or 1500 samples per second; ``t0`` is the first Costas symbol, one symbol behind the start of the transmission's
    ramp; 7.5 s slots, ``dt`` against 0.5 s; ``text`` is None."""
    DECODERS = FT4_Decoders
