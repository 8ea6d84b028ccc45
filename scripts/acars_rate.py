"""Rate probe of the ACARS skimmer (acars.hip) beside the channelizer pass it rides on.

    python scripts/acars_rate.py [--out FILE]            (default profiles/acars_rate.txt)

A 25 kHz raster of a 10 MS/s band, all M = 400 rows at 50 kHz (D = 200, L = 21, 85 taps: the most work per row sample the
definition allows).  Device-resident input -- noise plus eight stations that each send a 13-byte block inside the call --
in calls that complete max_out = 4096 outputs per row (82 ms of signal).  After at least 50 ms and four calls of warm-up,
25 calls are timed one by one, each ending in a synchronise (host clock); the median is reported with the least and the
most.  In the same process, on the same device: ``Channelizer.push_device`` alone (device output, the skimmer's
prototype) and the skimmer (the same channelizer pass with the decoders queued behind it, nothing downloaded).  One line:
both times per call, their difference as the decoders' share, the input rate and how many times real time the skimmer
runs; and the same with what ``ACARS_Skimmer.push`` downloads per call (the counts of every row)."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pysdr_amd import _lib                                    # noqa: E402
from pysdr_amd import acars                                   # noqa: E402
from pysdr_amd.channelizer import Channelizer                 # noqa: E402

MAX_OUT = 4096
FS, M, D = 10e6, 400, 200
CALLS = 25


def dev_input(lib, fs, M, n, seed=1):
    rng = np.random.default_rng(seed)
    x = 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for j in range(8):
        s = 0.03 * acars.waveform(acars.frame("2", f"N{j}", None, "Q0", str(j), prekey=2), fs, (3 + 11 * j) * fs / M + 100.0 * j)
        at = int(0.0005 * fs) * (j + 1)
        x[at:at + len(s)] += s[:n - at]
    x = x.astype(np.complex64)
    d = C.c_void_p()
    _lib.check(lib.pysdr_dev_alloc(0, n * 8, C.byref(d)), "alloc input")
    _lib.check(lib.pysdr_dev_upload(0, d, C.c_void_p(x.ctypes.data), n * 8), "upload")
    return d


def timed(call, sync):
    """-> (median seconds per call, (min, max), calls)"""
    def one():
        t0 = time.perf_counter()
        call()
        sync()
        return time.perf_counter() - t0

    warm, k = 0.0, 0
    while warm < 0.05 or k < 4:
        warm, k = warm + one(), k + 1
    t = sorted(one() for _ in range(CALLS))
    return t[len(t) // 2], (t[0], t[-1]), len(t)


def main():
    out = os.path.join(ROOT, "profiles", "acars_rate.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    lib = _lib.lib()
    _lib.require_gpu()
    n = MAX_OUT * D
    d_x = dev_input(lib, FS, M, n)
    ch = Channelizer(FS, M, D, acars.prototype(FS, M, D), max_in=n)
    pitch = MAX_OUT + 16
    d_y = C.c_void_p()
    _lib.check(lib.pysdr_dev_alloc(0, M * pitch * 8, C.byref(d_y)), "alloc output")
    (tc, tcs, kc) = timed(lambda: ch.push_device(d_x.value, n, d_y.value, pitch, sync=False), ch.sync)
    ch.close()
    lib.pysdr_dev_free(0, d_y)
    sk = acars.ACARS_Skimmer(FS, M, D, max_in=n, max_out=MAX_OUT)
    (ts, tss, ks) = timed(lambda: sk.dec.decode_raw(d_x.value, n, on_device=True, events=None), sk.sync)
    (td, tds, kd) = timed(lambda: sk.dec.decode_raw(d_x.value, n, on_device=True, events="counts"), sk.sync)
    r = sk.dec.decode_raw(d_x.value, n, on_device=True, events="counts")    # what the last call read, for the record
    heard = sum(len(acars.unpack(w[:c])) for w, c in zip(sk.dec.fetch(np.flatnonzero(r["counts"])), r["counts"][r["counts"] > 0]))
    p = sk.dec.plan
    text = (f"ACARS skimmer {FS / 1e6:g} MS/s M {M} D {D} ({M} rows at {FS / D:g} S/s, L {sk.L}, {p['taps']} taps, {sk.ndec} decoders; "
            f"{p['groups']} workgroups of {p['threads']} threads, {p['rows']} rows x {p['tile']} outputs per tile, {p['lds_bytes']} B LDS, "
            f"{p['cap']} event words per decoder): call of {n} samples = {MAX_OUT} outputs per row: channelizer alone {tc * 1e3:.3f} ms "
            f"({tcs[0] * 1e3:.3f} .. {tcs[1] * 1e3:.3f}, median of {kc} calls), skimmer {ts * 1e3:.3f} ms ({tss[0] * 1e3:.3f} .. {tss[1] * 1e3:.3f}, "
            f"{ks} calls), decoders {(ts - tc) * 1e3:.3f} ms = {(ts - tc) / tc:.2f} x the channelizer's pass; skimmer {n / ts / 1e6:.2f} MS/s "
            f"input = {n / ts / FS:.1f} x real time; with the counts downloaded every call {td * 1e3:.3f} ms ({tds[0] * 1e3:.3f} .. "
            f"{tds[1] * 1e3:.3f}, {kd} calls) = {n / td / FS:.1f} x real time; the last call read {heard} blocks in {int(r['counts'].sum())} "
            f"event words\n")
    sk.close()
    lib.pysdr_dev_free(0, d_x)
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
