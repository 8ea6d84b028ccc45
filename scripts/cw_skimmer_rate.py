"""Rate probe of the CW skimmer (cw.hip) beside the channelizer pass it rides on.

    python scripts/cw_skimmer_rate.py [--out FILE]            (default profiles/cw_skimmer_rate.txt)

Two rasters of 187.5 Hz channels at 375 samples per second each: fs = 192 kHz, M = 1024, D = 512 and fs = 768 kHz,
M = 4096, D = 2048.  Device-resident input -- noise plus eight carriers keyed at 25 wpm -- in calls that complete
max_out = 1024 outputs per channel; at least 20 ms of warm-up, then at least 60 ms of queued calls ending in one
synchronise.  In the same process, on the same device: ``Channelizer.push_device`` alone (device output) and the skimmer
(the same channelizer pass with the decoder queued behind it, nothing downloaded).  Per shape: both times per call, their
difference as the decoder's share, the ratio decoder / channelizer, and how many times real time the skimmer runs."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pysdr_amd import _lib                                    # noqa: E402
from pysdr_amd import cw                                      # noqa: E402
from pysdr_amd.channelizer import Channelizer                 # noqa: E402

MAX_OUT = 1024
SHAPES = [(192e3, 1024, 512), (768e3, 4096, 2048)]


def dev_input(lib, fs, M, n, seed=1):
    rng = np.random.default_rng(seed)
    x = 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    key = cw.morse_keying("CQ K1ABC", 25, fs)
    key = np.resize(key, n)
    t = np.arange(n)
    for j in range(8):
        k = 5 + (M // 9) * j
        x += 0.02 * np.roll(key, 1000 * j) * np.exp(2j * np.pi * ((k + 0.2) / M) * t)
    x = x.astype(np.complex64)
    d = C.c_void_p()
    _lib.check(lib.pysdr_dev_alloc(0, n * 8, C.byref(d)), "alloc input")
    _lib.check(lib.pysdr_dev_upload(0, d, C.c_void_p(x.ctypes.data), n * 8), "upload")
    return d


def timed(call, sync):
    def calls(k):
        t0 = time.perf_counter()
        for _ in range(k):
            call()
        sync()
        return time.perf_counter() - t0

    warm, per = 0.0, 1.0
    while warm < 0.02:
        dt = calls(2)
        warm, per = warm + dt, dt / 2
    k = max(8, int(0.06 / per) + 1)
    return calls(k) / k, k


def shape_rate(lib, fs, M, D):
    n = MAX_OUT * D
    d_x = dev_input(lib, fs, M, n)
    ch = Channelizer(fs, M, D, max_in=n)
    pitch = MAX_OUT + 16
    d_y = C.c_void_p()
    _lib.check(lib.pysdr_dev_alloc(0, M * pitch * 8, C.byref(d_y)), "alloc output")
    t_ch, k_ch = timed(lambda: ch.push_device(d_x.value, n, d_y.value, pitch, sync=False), ch.sync)
    ch.close()
    lib.pysdr_dev_free(0, d_y)
    sk = cw.CW_Skimmer(fs, M, D, max_in=n, max_out=MAX_OUT)
    t_sk, k_sk = timed(lambda: sk.dec.decode_raw(d_x.value, n, on_device=True, events=None), sk.sync)
    r = sk.dec.decode_raw(d_x.value, n, on_device=True, events="rows")       # what the last call read, for the record
    nev = int(r["counts"].sum())
    plan = sk.dec.plan
    sk.close()
    lib.pysdr_dev_free(0, d_x)
    return dict(fs=fs, M=M, D=D, n=n, t_ch=t_ch, t_sk=t_sk, k_ch=k_ch, k_sk=k_sk, events=nev, rows=len(r["events"]), plan=plan)


def main():
    out = os.path.join(ROOT, "profiles", "cw_skimmer_rate.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    lib = _lib.lib()
    _lib.require_gpu()
    lines = []
    for fs, M, D in SHAPES:
        r = shape_rate(lib, fs, M, D)
        dec = r["t_sk"] - r["t_ch"]
        p = r["plan"]
        lines.append(
            f"cw skimmer {fs / 1e3:g} kHz M {M} D {D} ({fs / M:g} Hz channels at {fs / D:g} S/s; {p['groups']} workgroups of "
            f"{p['threads']} threads, {p['rows']} rows x {p['tile']} samples per tile, {p['lds_bytes']} B LDS, {p['cap']} event slots "
            f"per row): call of {r['n']} samples = {MAX_OUT} outputs per row: channelizer alone {r['t_ch'] * 1e6:.1f} us "
            f"({r['k_ch']} calls), skimmer {r['t_sk'] * 1e6:.1f} us ({r['k_sk']} calls), decoder {dec * 1e6:.1f} us = "
            f"{dec / r['t_ch']:.2f} x the channelizer's pass; skimmer {r['n'] / r['t_sk'] / 1e9:.3f} GS/s input = "
            f"{r['n'] / r['t_sk'] / fs:.0f} x real time; the last call read {r['events']} events on {r['rows']} rows")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
