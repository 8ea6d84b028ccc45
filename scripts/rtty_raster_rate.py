"""Rate probe of the RTTY raster skimmer (fsk.hip) beside the channelizer pass it rides on.

    python scripts/rtty_raster_rate.py [--out FILE]            (default profiles/rtty_raster_rate.txt)

Two rasters, all M rows each: fs = 32 kHz (S = 22, M = 128, D = 32: 2816 decoders) and fs = 192 kHz (S = 33, M = 512, D =
128: 16896 decoders).  Device-resident input -- noise plus eight RTTY stations -- in calls that complete max_out = 256
outputs per row; at least 50 ms of warm-up, then three windows of at least 0.3 s of queued calls, each ending in one
synchronise (host clock; the median window is reported with the spread of the three).  In the same process, on the same
device: ``Channelizer.push_device`` alone (device output, the raster's prototype) and the skimmer (the same channelizer
pass with the decoders queued behind it, nothing downloaded).  Per shape: both times per call, their difference as the
decoders' share, the ratio decoders / channelizer, the input rate and how many times real time the skimmer runs; and the
same with what ``RTTY_Raster_Skimmer.push`` downloads per call (counts, qn and open of every fine row)."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pysdr_amd import _lib                                    # noqa: E402
from pysdr_amd import fsk                                     # noqa: E402
from pysdr_amd.channelizer import Channelizer                 # noqa: E402

MAX_OUT = 256
RATES = [32000.0, 192000.0]


def stations(fs, n):
    """eight stations sending RY without end, 1.5 stop bits: continuous-phase FSK, mark the upper tone"""
    t = np.arange(n) / fs
    bit = t * fsk.BAUD % 7.5                                  # start, five data bits, 1.5 stop bits
    ry = np.array([[0, 0, 1, 0, 1, 0, 1, 1], [0, 1, 0, 1, 0, 1, 1, 1]])   # R = 01010 and Y = 10101, LSB first
    lev = ry[(t * fsk.BAUD // 7.5).astype(np.int64) % 2, bit.astype(np.int64)]
    ph = 2 * np.pi * np.cumsum((lev - 0.5) * fsk.TONE_STEPS * fsk.BAUD / 4) / fs
    return sum(np.exp(1j * (ph + 2 * np.pi * (j - 3.6) * fs / 10 * t + j)) for j in range(8))


def dev_input(lib, fs, n, seed=1):
    rng = np.random.default_rng(seed)
    x = 0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + 0.05 * stations(fs, n)
    x = x.astype(np.complex64)
    d = C.c_void_p()
    _lib.check(lib.pysdr_dev_alloc(0, n * 8, C.byref(d)), "alloc input")
    _lib.check(lib.pysdr_dev_upload(0, d, C.c_void_p(x.ctypes.data), n * 8), "upload")
    return d


def timed(call, sync):
    """-> (median seconds per call of three windows, (min, max), calls per window)"""
    def calls(k):
        t0 = time.perf_counter()
        for _ in range(k):
            call()
        sync()
        return time.perf_counter() - t0

    warm, per = 0.0, 1.0
    while warm < 0.05:
        dt = calls(4)
        warm, per = warm + dt, dt / 4
    k = max(16, int(0.3 / per) + 1)
    t = sorted(calls(k) / k for _ in range(3))
    return t[1], (t[0], t[2]), k


def shape_rate(lib, fs):
    S, D, M = fsk.shape(fs)
    n = MAX_OUT * D
    d_x = dev_input(lib, fs, n)
    ch = Channelizer(fs, M, D, fsk.prototype(fs, M, S), max_in=n)
    pitch = MAX_OUT + 16
    d_y = C.c_void_p()
    _lib.check(lib.pysdr_dev_alloc(0, M * pitch * 8, C.byref(d_y)), "alloc output")
    t_ch = timed(lambda: ch.push_device(d_x.value, n, d_y.value, pitch, sync=False), ch.sync)
    ch.close()
    lib.pysdr_dev_free(0, d_y)
    sk = fsk.RTTY_Raster_Skimmer(fs, max_in=n, max_out=MAX_OUT)
    t_sk = timed(lambda: sk.dec.decode_raw(d_x.value, n, on_device=True, events=None), sk.sync)
    t_dl = timed(lambda: sk.dec.decode_raw(d_x.value, n, on_device=True, events="counts", squelch=True), sk.sync)
    r = sk.dec.decode_raw(d_x.value, n, on_device=True, events="counts", squelch=True)   # what the last call read, for the record
    res = dict(fs=fs, S=S, M=M, D=D, n=n, t_ch=t_ch, t_sk=t_sk, t_dl=t_dl, events=int(r["counts"].sum()), nopen=int(r["open"].sum()),
               plan=sk.dec.plan, nfine=sk.nfine)
    sk.close()
    lib.pysdr_dev_free(0, d_x)
    return res


def main():
    out = os.path.join(ROOT, "profiles", "rtty_raster_rate.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    lib = _lib.lib()
    _lib.require_gpu()
    lines = []
    for fs in RATES:
        r = shape_rate(lib, fs)
        p = r["plan"]
        (ch, chs, kc), (sk, sks, ks), (dl, dls, kd) = r["t_ch"], r["t_sk"], r["t_dl"]
        dec = sk - ch
        lines.append(
            f"rtty raster skimmer {r['fs'] / 1e3:g} kHz S {r['S']} M {r['M']} D {r['D']} ({r['M']} rows at {r['fs'] / r['D']:g} S/s, {r['nfine']} "
            f"decoders; {p['groups']} workgroups of {p['threads']} threads, {p['rows']} rows x {p['tile']} outputs per tile, "
            f"{p['lds_bytes']} B LDS, {p['cap']} event slots per decoder): call of {r['n']} samples = {MAX_OUT} outputs per row: "
            f"channelizer alone {ch * 1e6:.1f} us ({chs[0] * 1e6:.1f} .. {chs[1] * 1e6:.1f}, {kc} calls per window), skimmer "
            f"{sk * 1e6:.1f} us ({sks[0] * 1e6:.1f} .. {sks[1] * 1e6:.1f}, {ks} calls), decoders {dec * 1e6:.1f} us = "
            f"{dec / ch:.2f} x the channelizer's pass; skimmer {r['n'] / sk / 1e6:.2f} MS/s input = {r['n'] / sk / r['fs']:.0f} x real "
            f"time; with counts, qn and open downloaded every call {dl * 1e6:.1f} us ({dls[0] * 1e6:.1f} .. {dls[1] * 1e6:.1f}, {kd} "
            f"calls) = {r['n'] / dl / r['fs']:.0f} x real time; the last call read {r['events']} events, {r['nopen']} decoders open")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
