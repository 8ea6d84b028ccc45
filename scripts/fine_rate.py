"""Rate probe of the fine channelizer (fine.hip behind chan.hip) at 8 MS/s, next to its first stage
alone.

    python scripts/fine_rate.py > profiles/fine_channelizer_rate.txt

Two shapes: the PSK31 raster (rows 62.5 Hz apart at 250 S/s, M2 / D2 = 4) over a 3 kHz band and a CW raster (rows 250 Hz
apart at 500 S/s, M2 / D2 = 2) over a 70 kHz band, both 100 kHz above the centre.  Three call lengths: 2^22 samples, the
256 D samples of a skimmer call of max_out = 256 outputs, and 2 D samples (two outputs per call: the many-rows-few-frames
split of the kernel's tile).  Device-resident input, outputs left on the device; at least 20 ms of warm-up, then at least
60 ms of queued calls ending in one synchronise.  Every figure stands next to ``Channelizer(8e6, M1, D1)`` with all M1 rows
on the same input and call length: what one object per band pays for repeating stage 1.  Nothing is asserted."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pysdr_amd import _lib, fine                              # noqa: E402
from pysdr_amd.channelizer import Channelizer                 # noqa: E402
from pysdr_amd.fine import FineChannelizer                    # noqa: E402

FS = 8e6
MAX_IN = 1 << 23
CASES = [("PSK31", 250.0, 4, (100e3, 103e3)), ("CW", 500.0, 2, (100e3, 170e3))]


def dev_noise(lib, n, seed=1):
    rng = np.random.default_rng(seed)
    blk = (0.1 * (rng.standard_normal(1 << 20) + 1j * rng.standard_normal(1 << 20))).astype(np.complex64)
    d = C.c_void_p()
    _lib.check(lib.pysdr_dev_alloc(0, n * 8, C.byref(d)), "alloc input")
    for off in range(0, n, len(blk)):
        k = min(len(blk), n - off)
        _lib.check(lib.pysdr_dev_upload(0, C.c_void_p(d.value + off * 8), C.c_void_p(blk.ctypes.data), k * 8), "upload")
    return d


def per_call(ch, d_x, n, d_y, pitch):
    def calls(k):
        t0 = time.perf_counter()
        for _ in range(k):
            ch.push_device(d_x.value, n, d_y.value, pitch, sync=False)
        ch.sync()
        return time.perf_counter() - t0

    warm, per = 0.0, 1.0
    while warm < 0.02:
        dt = calls(2)
        warm, per = warm + dt, dt / 2
    k = max(8, int(0.06 / per) + 1)
    return calls(k) / k


def main():
    lib = _lib.lib()
    _lib.require_gpu()
    d_x = dev_noise(lib, MAX_IN)
    for name, fs_out, C2, band in CASES:
        M1, D1, M2, D2 = fine.shape(FS, fs_out, C2)
        channels = fine.channels_for(band, FS, M1, D1, M2)
        fc = FineChannelizer(FS, M1, M2, D1, D2, channels=channels, max_in=MAX_IN)
        c1 = Channelizer(FS, M1, D1, max_in=MAX_IN)
        p = fine.plan(M1, D1, M2, D2, g_first=channels[0], ng=channels[1])
        pitch_f, pitch_1 = MAX_IN // fc.D + 16, MAX_IN // D1 + 16
        d_f, d_1 = C.c_void_p(), C.c_void_p()
        _lib.check(lib.pysdr_dev_alloc(0, fc.nk * pitch_f * 8, C.byref(d_f)), "alloc output")
        _lib.check(lib.pysdr_dev_alloc(0, M1 * pitch_1 * 8, C.byref(d_1)), "alloc output")
        print(f"{name} raster at 8 MS/s: M1 {M1} D1 {D1} M2 {M2} D2 {D2}, {fc.nk} fine rows {FS / fc.M:g} Hz apart at {fc.fs_out:g} S/s from "
              f"{fc.freqs[0]:g} Hz ({p['nk1']} coarse rows; second stage radices {p['radices']}, {p['frames_per_wg']} frames / workgroup, "
              f"256 threads, {p['lds_bytes']} B LDS)")
        for what, n in (("2^22 samples", 1 << 22), ("256 outputs", 256 * fc.D), ("2 outputs", 2 * fc.D)):
            tf = per_call(fc, d_x, n, d_f, pitch_f)
            t1 = per_call(c1, d_x, n, d_1, pitch_1)
            print(f"  calls of {what} ({n} samples, {n / FS * 1e3:.1f} ms of signal): fine {tf * 1e3:.3f} ms = {n / tf / 1e9:.2f} GS/s input = "
                  f"{n / tf / FS:.0f} x real time; Channelizer({M1}, {D1}) alone {t1 * 1e3:.3f} ms = {n / t1 / 1e9:.2f} GS/s; "
                  f"fine / first stage alone = {tf / t1:.2f}")
        fc.close()
        c1.close()
        lib.pysdr_dev_free(0, d_f)
        lib.pysdr_dev_free(0, d_1)
    lib.pysdr_dev_free(0, d_x)
    return 0


if __name__ == "__main__":
    sys.exit(main())
