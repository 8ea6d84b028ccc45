"""Streams for the tests of a-priori decoding, shared by tests/test_ap_oracle.py, which picks the weak
level on the CPU, and tests/test_gpu_ap.py, which runs the same streams on the device: FT8 and FT4 frames of encoded
messages in white noise at the smallest shapes of tests/test_gpu_ft8.py and tests/test_gpu_ft4.py (8 kS/s, three rows), the
rows of the float64 channelizer behind them, and the oracle skimmer's record at a station."""
import functools

import numpy as np

from tests import channelizer_oracle as cz
from tests import ft4_oracle as f4o
from tests import ft8_oracle as f8o

FS, CHANNELS = 8000.0, (3, 3)
CQ = "CQ K1ABC FN42"
FT8_F, FT4_F = 260.0, 750.0 - 9 * f4o.BAUD / 4                                  # Hz of tone 0: on the raster in both modes
CLEAN = -8.0                                                                    # dB in 2500 Hz: decodes with no hard error
# The weak levels, picked on the CPU (tests/test_ap_oracle.py::test_the_weak_levels_of_the_device_tests): at these, with these
# seeds, min-sum gives no message on the oracle skimmer's soft bits, every right hypothesis rescues the frame, and both
# still hold when the soft bits are disturbed by a part in a thousand.
FT8_WEAK, FT8_SEED = -20.0, 31
FT4_WEAK, FT4_SEED = -15.5, 41
SKIM_SECONDS, SKIM_SEED = 45.0, 52                                              # the skimmer's stream: the CQ at 0.5 s, again at 30.5 s


def stream(oracle, frames, seconds, seed):
    """``frames``: (77 message bits, Hz of tone 0, dB in 2500 Hz, start s) -> complex64 [seconds FS], noise of power 1 in
    2500 Hz under the frames, scaled by 0.05"""
    from pysdr_amd import ldpc
    n = int(seconds * FS)
    rng = np.random.default_rng(seed)
    x = oracle.noise_sigma(0.0, oracle.SNR_BW, FS) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for j, (msg, f, snr, start) in enumerate(frames):
        s = oracle.waveform(oracle.tones(ldpc.encode(msg)), f, FS, True, phase=1.0 + j) * 10 ** (snr / 20)
        at = int(start * FS)
        x[at:at + len(s)] += s[:n - at]
    x = (0.05 * x).astype(np.complex64)
    x.setflags(write=False)
    return x


def cq_bits():
    from pysdr_amd import ft8msg
    return ft8msg.pack77(CQ)


def ft4_bits():
    return np.random.default_rng(4).integers(0, 2, 77).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def ft8_weak(snr=FT8_WEAK, seed=FT8_SEED):
    return stream(f8o, [(cq_bits(), FT8_F, snr, 0.5)], 14.0, seed)


@functools.lru_cache(maxsize=None)
def ft4_weak(snr=FT4_WEAK, seed=FT4_SEED):
    return stream(f4o, [(ft4_bits(), FT4_F, snr, 0.5)], 7.0, seed)


@functools.lru_cache(maxsize=None)
def skimmer_stream(snr=FT8_WEAK, seed=SKIM_SEED):
    return stream(f8o, [(cq_bits(), FT8_F, CLEAN, 0.5), (cq_bits(), FT8_F, snr, 30.5)], SKIM_SECONDS, seed)


def oracle_records(mode, x):
    """the float64 channelizer and the mode's oracle skimmer on the stream -> its records"""
    from pysdr_amd import ft4, ft8
    m, o = (ft8, f8o) if mode == "ft8" else (ft4, f4o)
    S, D, M = m.shape(FS)
    rows = cz.polyphase(np.asarray(x, np.complex128), m.prototype(FS, M, S), M, D, 0, -(-len(x) // D), o.rows_of(M, CHANNELS)).astype(np.complex64)
    sk = o.Skimmer(3, S, False)
    sk.push(rows)
    return sk.records


def near(mode, recs, f, start):
    """the records at the station: within a raster step and a step and a half of its place"""
    from pysdr_amd import ft4, ft8
    m = ft8 if mode == "ft8" else ft4
    S, D, M = m.shape(FS)
    ff = (f8o if mode == "ft8" else f4o).fine_freqs(FS, M, S, CHANNELS)
    qs_seconds = (S // 4) * D / FS
    lead = 0.0 if mode == "ft8" else 0.048 + 0.008                               # FT4: the ramp in front of the first symbol
    return [r for r in recs if abs(ff[r["F"]] - f) <= m.BAUD / 2 + 0.1 and abs(r["t0"] * qs_seconds - (start + lead)) <= 1.5 * qs_seconds + 0.03]
