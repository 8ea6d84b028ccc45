"""FT8 skimmer: Costas sync and soft bits on a fine raster of the band (kernels ``ft.hip``, host half
``api_ft.hip``).  8-FSK at 6.25 baud, tones 6.25 Hz apart, 79 symbols of which 21 are three Costas arrays.  A channelizer
with M / D = 4 delivers rows at ``S`` samples per symbol; inside every row ``NSUB = S / 2`` decoders run on the device, one
every 3.125 Hz, so that the fine rows ``F = a NSUB + j`` form one uniform raster over all rows.  The device finds every
frame by its sync score and hands out its 174 soft bits in transmission order; with ``decode=True`` the device also runs
the LDPC(174,91) decoder on them, straight from the spectrum ring, checks the CRC-14, and the record carries the message's
77 bits and its text (``ldpc.py``, ``ft8msg.py``); with ``report=True`` it measures every decoded frame
in the spectrum ring and the record carries its SNR, fine frequency and fine time (kernels ``report.hip``; DESIGN.md 3 item
26).  This file is the mode: its constants, settings and waveform.  The decoder bank and the skimmer are ``ft.py``'s, told this
module as their ``MODE``; ``ft4.py`` is the other mode, and neither knows the other.  The names of ``ft.py``, ``ft_report.py``
and ``ft_pass.py`` that a caller of this mode needs are importable from here."""
from __future__ import annotations

import sys

import numpy as np

from . import ft as _ft
from . import ft8msg as _msg
from . import psk as _psk
from ._lib import Ft8Cfg
from .channelizer import Channelizer  # noqa: F401  (the names below: importable from here, as they always were)
from .skimmer import DecoderBank, Skimmer  # noqa: F401
from .ft import KEEP, LLR_MAX, cfg_dict, hard_bits, mode_fine_channelizer, mode_plan, mode_shape, owners, steps_done, tables, unit_llr, unpack  # noqa: F401
from .ft_report import CAL, FLOOR_QUANTILE, FLOOR_ROWS, REPORT_MAX, SNR_BW  # noqa: F401
from .ft_report import delta, noise_floor, noise_of, refine, report_plan, snr_db, spot_line, spots  # noqa: F401
from .ft_pass import PASS_EVENT_CAP, PASS_LUT, PASS_MAX, PASS_ROWS_MAX, PASS_TRIALS, PASS_WINDOW_MAX  # noqa: F401
from .ft_pass import pack91, pass_lut, pass_plan, pass_pulse, trial_grid  # noqa: F401

NAME, PLAN_CALL = "FT8", "pysdr_ft8_plan"
_MODE = sys.modules[__name__]
BAUD = 6.25
COSTAS = (3, 1, 4, 0, 6, 5, 2)
GRAY = (0, 1, 3, 2, 5, 6, 4, 7)                  # value v is sent on tone GRAY[v]
SYMBOLS, DATA, BITS = 79, 58, 174
SYNC_AT = (0, 36, 72)                            # first symbol of the three Costas arrays
FRAME_SECONDS, SLOT_SECONDS, NOMINAL_START = SYMBOLS / BAUD, 15.0, 0.5
STEPS_PER_SYMBOL = 4
EMIT_LAG = 316                                   # an event t0 is emitted at step t0 + 316 ...
HOLD = 321                                       # ... and released once step t0 + 320 is complete: every rival has arrived
SHAPES = (64, 96)                                # row samples per symbol
NB_EXTRA = 14                                    # NB = NSUB + 14: decoder j uses bins j + 2 tone, tone 0 to 7
UNPACK = _msg.unpack77                           # the 77 decoded bits -> text (``ft4.py``: None, its scrambler is not here)
REPORT_MODE = 0                                  # PYSDR_REPORT_FT8
TONES = 8
PULSE_SYMBOLS = 3                                # symbols the frequency pulse of ``waveform`` spans (BT = 2)
PULSE_K = 2 * np.pi * np.sqrt(2 / np.log(2))
REACH_T = 40                                     # steps a rescan looks to either side of a subtracted frame
# The trial grid: 3 times x 3 frequencies around the refined values.  ``refine`` leaves the time within 0.35 step and the
# frequency within 0.4 Hz, so a quarter step and 0.3 Hz to either side cover both, and the best
# trial is then within an eighth of a step and 0.15 Hz: about -27 dB of the frame left by the frequency error alone.
TRIAL_DN = 0.25                                  # steps between the trial times
TRIAL_DF = 0.3                                   # Hz between the trial frequencies


def shape(fs):
    """-> (S, D, M): S = 64 row samples per symbol if fs / (64 baud) is an integer D and the channelizer accepts M = 4 D,
    otherwise S = 96 likewise, otherwise ValueError."""
    return _ft.mode_shape(_MODE, fs)


def prototype(fs, M, S):
    """The channelizer's prototype for the FT8 raster, ``psk.prototype``'s form: Kaiser(8.0) windowed sinc of 4 M taps cut
    at fs_out / 2 = S baud / 2, sum 1.  A row's outer bin is (NB - 1) baud / 4 from its centre, a station up to a raster
    step beyond it, plus its own baud-wide tone: the response is flat within 0.1 dB out to fp = (NB + 1) baud / 4 + baud
    and at least 70 dB down from fs_out - fp on, where the aliases of that band begin."""
    return _psk.prototype(fs, M, BAUD, S)


def fine_channelizer(fs, band, device=0, max_in=1 << 22):
    """A ``fine.FineChannelizer`` for ``FT8_Skimmer(fs, chan=...)`` at a rate ``shape`` refuses: rows S baud / 4 apart whose
    centres lie in ``band = (f_lo, f_hi)`` Hz from the centre, S = 64 where ``fine.shape`` finds a shape, else 96; M2 / D2 =
    4, the second prototype is ``prototype`` at the first stage's output rate, the first ``fine.prototype1``."""
    return _ft.mode_fine_channelizer(_MODE, fs, band, device, max_in)


def params(smin=3.0, hmin=13, pmax=1e18):
    """The settings of DESIGN.md 3 item 22 as the ``_lib.Ft8Cfg`` the C ABI takes."""
    return Ft8Cfg(smin=float(np.float32(smin)), hmin=int(hmin), pmax=float(np.float32(pmax)))


def plan(nk, S, max_out, cfg):
    """What a skimmer of this shape launches (no device needed): dict of rows per workgroup, threads, LDS bytes, tile
    samples, event cap per decoder and call, workgroups, decoders per row, ring depth in steps.  Raises PysdrError
    outside the rules."""
    return _ft.mode_plan(_MODE, nk, S, max_out, cfg)


def tones(bits):
    """174 bits in transmission order -> the frame's 79 tones: Costas arrays at symbols 0, 36 and 72, 2 x 29 data symbols
    of 3 bits, MSB first, Gray-mapped"""
    bits = np.asarray(bits, np.int64).reshape(DATA, 3)
    v = 4 * bits[:, 0] + 2 * bits[:, 1] + bits[:, 2]
    g = np.array(GRAY)[v]
    return np.concatenate((COSTAS, g[:29], COSTAS, g[29:], COSTAS)).astype(np.int64)


def waveform(tones, f0, fs, gfsk=True, phase=0.0):
    """complex128 frame of power 1 at ``fs``: tone 0 at ``f0`` Hz from the centre, continuous phase.  ``gfsk``: the
    frequency pulse of a symbol is (erf(k (t + 1/2)) - erf(k (t - 1/2))) / 2, k = 2 pi sqrt(2 / ln 2), t in symbols from the
    symbol's middle (BT = 2), the first and the last tone held beyond the frame; otherwise rectangular."""
    from scipy.special import erf
    tones = np.asarray(tones, np.float64)
    sps = float(fs) / BAUD
    n = int(round(len(tones) * sps))
    t = (np.arange(n) + 0.5) / sps                                       # symbols
    k0 = np.minimum(np.floor(t).astype(np.int64), len(tones) - 1)
    if gfsk:
        kk = 2 * np.pi * np.sqrt(2 / np.log(2))
        ext = np.concatenate((tones[:1], tones, tones[-1:]))
        dev = np.zeros(n)
        for d in (-1, 0, 1):                                             # the pulse is 0 to 1e-50 beyond a symbol and a half
            tau = t - (k0 + d) - 0.5
            dev += ext[k0 + d + 1] * 0.5 * (erf(kk * (tau + 0.5)) - erf(kk * (tau - 0.5)))
    else:
        dev = tones[k0]
    ph = np.cumsum(float(f0) + BAUD * dev)
    return np.exp(1j * (2 * np.pi / float(fs) * ph + phase))


class FT8_Decoders(_ft.FT_Decoders):
    """The decoder bank on a borrowed ``Channelizer``: ``ft.FT_Decoders``' calls on ``pysdr_ft8_*`` with this module's
    constants (an event's t0 is ``t_first + unpack(words)[0] - 316``)."""
    KIND, DESTROY = "ft8", "pysdr_ft8_destroy"
    MODE = _MODE


class FT8_Skimmer(_ft.FT_Skimmer):
    """``ft.FT_Skimmer`` (which describes the records) on this mode: 79 symbols of 8 tones at 6.25 baud, rows at S baud = 400
    or 600 samples per second, 15 s slots, ``text`` from ``ft8msg.unpack77``."""
    DECODERS = FT8_Decoders
