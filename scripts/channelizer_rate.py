"""Rate probe of the polyphase channelizer (chan.hip) against the per-sub-receiver front end.

    python scripts/channelizer_rate.py [--one M D FS]        (--one: a single shape, a few calls: for a profiler run)

Device-resident input of 2^25 samples per call, default prototype, all M channels stored; at least 20 ms of warm-up,
then at least 60 ms of queued calls ending in one synchronise.  The time per call is the channelizer's kernel plus the
roll of its input history (one small launch).  Per shape: input GS/s, the algorithmic bytes 8 + 8 nk / D per sample
over that time, as a share of the 6.29 TB/s copy rate and of the 8 TB/s peak, and channel-samples per second (input
rate x nk).  In the same process: the 6-RX IQ-mode front end of the rx6 workload (8 MS/s, 3/500, 1001 taps), mix +
decimate kernel time from the context's own events, as input rate x 6.  Exit status 1 if the channelizer does not
exceed that figure at every shape."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pysdr_amd import _lib                                    # noqa: E402
from pysdr_amd.channelizer import Channelizer, plan           # noqa: E402

N_CALL = 1 << 25
COPY_TBPS, PEAK_TBPS = 6.29, 8.0
SHAPES = [(8e6, 256, 128), (8e6, 640, 320), (10e6, 4096, 2048)]


def dev_noise(lib, n, seed=1):
    rng = np.random.default_rng(seed)
    blk = (0.1 * (rng.standard_normal(1 << 20) + 1j * rng.standard_normal(1 << 20))).astype(np.complex64)
    d = C.c_void_p()
    _lib.check(lib.pysdr_dev_alloc(0, n * 8, C.byref(d)), "alloc input")
    for off in range(0, n, len(blk)):
        k = min(len(blk), n - off)
        _lib.check(lib.pysdr_dev_upload(0, C.c_void_p(d.value + off * 8), C.c_void_p(blk.ctypes.data), k * 8), "upload")
    return d


def chan_rate(lib, d_x, fs, M, D, quick=False):
    ch = Channelizer(fs, M, D, max_in=N_CALL)
    pitch = N_CALL // D + 16
    d_y = C.c_void_p()
    _lib.check(lib.pysdr_dev_alloc(0, M * pitch * 8, C.byref(d_y)), "alloc output")

    def calls(k):
        t0 = time.perf_counter()
        for _ in range(k):
            ch.push_device(d_x.value, N_CALL, d_y.value, pitch, sync=False)
        ch.sync()
        return time.perf_counter() - t0

    if quick:
        calls(4)
        per = calls(4) / 4
    else:
        warm, per = 0.0, 1.0
        while warm < 0.02:
            dt = calls(2)
            warm, per = warm + dt, dt / 2
        k = max(8, int(0.06 / per) + 1)
        per = calls(k) / k
    ch.close()
    lib.pysdr_dev_free(0, d_y)
    rate = N_CALL / per
    tbps = (8 + 8 * M / D) * rate / 1e12
    return dict(fs=fs, M=M, D=D, ms=per * 1e3, gsps=rate / 1e9, tbps=tbps, chan_sps=rate * M, plan=plan(M, D, 8 * M))


def rx6_rate(lib):
    """mix + decimate of six IQ-mode sub-receivers on one 8 MS/s stream, 1001-tap prototype"""
    import bench
    from pysdr_amd.synth import CONFIGS
    cfg = dict(CONFIGS['C3'], rx=[dict(r, mode='IQ') for r in bench.RX6[:6]], ntaps_dec=1001)
    B = 256
    P, rxs = bench.build_receivers(cfg, 0, B)
    ctx, L = P._pysdr_stream, P.IN_CHUNK_SIZE
    d_x = dev_noise(lib, B * L, seed=2)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.02:
        ctx.process_batch(d_x.value, B, L, on_device=True)
        _lib.check(lib.pysdr_sync(ctx.h), "sync")
    _lib.check(lib.pysdr_set_profile(ctx.h, 1), "profile")
    k = 0
    t0 = time.perf_counter()
    while k < 8 or time.perf_counter() - t0 < 0.06:
        ctx.process_batch(d_x.value, B, L, on_device=True)
        k += 1
    _lib.check(lib.pysdr_sync(ctx.h), "sync")
    ms, fe = C.c_float(0), []
    for back in range(min(k, 32)):
        _lib.check(lib.pysdr_get_elapsed_ms(ctx.h, 0, back, C.byref(ms)), "elapsed")
        fe.append(ms.value)
    lib.pysdr_dev_free(0, d_x)
    per = float(np.mean(fe)) * 1e-3
    return dict(samples=B * L, ms=per * 1e3, gsps=B * L / per / 1e9, chan_sps=B * L / per * 6)


def main():
    lib = _lib.lib()
    _lib.require_gpu()
    if "--one" in sys.argv:
        i = sys.argv.index("--one")
        M, D, fs = int(sys.argv[i + 1]), int(sys.argv[i + 2]), float(sys.argv[i + 3])
        d_x = dev_noise(lib, N_CALL)
        r = chan_rate(lib, d_x, fs, M, D, quick=True)
        print(f"M {M} D {D}: {r['ms']:.3f} ms per call of 2^25 samples, {r['gsps']:.2f} GS/s")
        return 0
    d_x = dev_noise(lib, N_CALL)
    rows = [chan_rate(lib, d_x, *s) for s in SHAPES]
    lib.pysdr_dev_free(0, d_x)
    ref = rx6_rate(lib)
    print(f"rx6 front end (8 MS/s, 6 RX IQ, 3/500, 1001 taps): {ref['ms']:.3f} ms per {ref['samples']} samples = "
          f"{ref['gsps']:.2f} GS/s input = {ref['chan_sps'] / 1e9:.1f} G channel-samples/s")
    ok = True
    for r in rows:
        p = r['plan']
        good = r['chan_sps'] > ref['chan_sps']
        ok = ok and good
        print(f"channelizer {r['fs'] / 1e6:g} MS/s M {r['M']} D {r['D']} (radices {p['radices']}, {p['frames_per_wg']} frames / "
              f"workgroup, {p['threads']} threads, {p['lds_bytes']} B LDS): {r['ms']:.3f} ms per call of 2^25 = {r['gsps']:.2f} GS/s "
              f"input, {8 + 8 * r['M'] / r['D']:g} B/sample = {r['tbps']:.3f} TB/s = {100 * r['tbps'] / COPY_TBPS:.1f} % of the copy "
              f"rate, {100 * r['tbps'] / PEAK_TBPS:.1f} % of peak; {r['chan_sps'] / 1e9:.1f} G channel-samples/s = "
              f"{r['chan_sps'] / ref['chan_sps']:.1f} x rx6 {'ok' if good else 'BELOW rx6'}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
