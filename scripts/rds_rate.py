"""Rate probe of the RDS skimmer (rds.hip) beside the channelizer pass it rides on.

    python scripts/rds_rate.py [--out FILE]            (default profiles/rds_rate.txt)

One 100 kHz raster, all M rows: fs = 10 MS/s, M = 100, D = 25: 100 rows at 400 kHz, 1600 decoders, L = 673.  Device-resident
input -- noise plus eight stations that each send one group inside the call -- in calls that complete max_out = 65536
outputs per row (164 ms of signal).  After at least 60 ms and four calls of warm-up, 25 calls are timed one by one, each
ending in a synchronise (host clock); the median is reported with the least and the most.  In the same process, on the
same device: ``Channelizer.push_device`` alone (device output, the skimmer's prototype) and the skimmer (the same
channelizer pass with the decoders queued behind it, nothing downloaded).  Both times per call, their difference as the
decoders' share, the ratio decoders / channelizer, the input rate and how many times real time the skimmer runs; and the
same with what ``RDS_Skimmer.push`` downloads per call (the counts of every decoder)."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pysdr_amd import _lib                                    # noqa: E402
from pysdr_amd import rds                                     # noqa: E402
from pysdr_amd.channelizer import Channelizer                 # noqa: E402

MAX_OUT = 65536
SHAPES = [(10e6, 100, 25)]
CALLS = 25


def dev_input(lib, fs, M, n, seed=1):
    rng = np.random.default_rng(seed)
    x = 0.003 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for j in range(8):
        g = [rds.group_0a(rds.pi_of("KAAA") + j, "STATION%d" % j, j % 4)]
        s = 0.05 * rds.waveform(g, fs, ((3 + 11 * j) % M) * fs / M + 5000.0 * (j - 4))
        at = int(0.002 * fs) * (j + 1)
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
    while warm < 0.06 or k < 4:
        warm, k = warm + one(), k + 1
    t = sorted(one() for _ in range(CALLS))
    return t[len(t) // 2], (t[0], t[-1]), len(t)


def shape_rate(lib, fs, M, D):
    n = MAX_OUT * D
    d_x = dev_input(lib, fs, M, n)
    ch = Channelizer(fs, M, D, rds.prototype(fs, M, D), max_in=n)
    pitch = MAX_OUT + 16
    d_y = C.c_void_p()
    _lib.check(lib.pysdr_dev_alloc(0, M * pitch * 8, C.byref(d_y)), "alloc output")
    t_ch = timed(lambda: ch.push_device(d_x.value, n, d_y.value, pitch, sync=False), ch.sync)
    ch.close()
    lib.pysdr_dev_free(0, d_y)
    sk = rds.RDS_Skimmer(fs, M, D, max_in=n, max_out=MAX_OUT)
    sk.dec.reset()
    first = sk.dec.decode_raw(d_x.value, n, on_device=True, events="counts")    # the stream's first call, for the record: what it read
    heard = sum(len(rds.unpack(w[:c])) for w, c in zip(sk.dec.fetch(np.flatnonzero(first["counts"])), first["counts"][first["counts"] > 0]))
    t_sk = timed(lambda: sk.dec.decode_raw(d_x.value, n, on_device=True, events=None), sk.sync)
    t_dl = timed(lambda: sk.dec.decode_raw(d_x.value, n, on_device=True, events="counts"), sk.sync)
    res = dict(fs=fs, M=M, D=D, n=n, t_ch=t_ch, t_sk=t_sk, t_dl=t_dl, words=int(first["counts"].sum()), heard=heard, plan=sk.dec.plan, ndec=sk.ndec,
               L=sk.L)
    sk.close()
    lib.pysdr_dev_free(0, d_x)
    return res


def main():
    out = os.path.join(ROOT, "profiles", "rds_rate.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    lib = _lib.lib()
    _lib.require_gpu()
    lines = []
    for fs, M, D in SHAPES:
        r = shape_rate(lib, fs, M, D)
        p = r["plan"]
        (ch, chs, kc), (sk, sks, ks), (dl, dls, kd) = r["t_ch"], r["t_sk"], r["t_dl"]
        dec = sk - ch
        lines.append(
            f"RDS skimmer {r['fs'] / 1e6:g} MS/s M {r['M']} D {r['D']} ({r['M']} rows at {r['fs'] / r['D']:g} S/s, L {r['L']} in {p['segments']} "
            f"segments, {r['ndec']} decoders; {p['groups']} workgroups of {p['threads']} threads, {p['rows']} rows x {p['tile']} outputs per tile, "
            f"{p['lds_bytes']} B LDS, {p['cap']} event words per decoder): call of {r['n']} samples = {MAX_OUT} outputs per row: "
            f"channelizer alone {ch * 1e6:.1f} us ({chs[0] * 1e6:.1f} .. {chs[1] * 1e6:.1f}, median of {kc} calls), skimmer "
            f"{sk * 1e6:.1f} us ({sks[0] * 1e6:.1f} .. {sks[1] * 1e6:.1f}, {ks} calls), decoders {dec * 1e6:.1f} us = "
            f"{dec / ch:.2f} x the channelizer's pass; skimmer {r['n'] / sk / 1e6:.2f} MS/s input = {r['n'] / sk / r['fs']:.1f} x real "
            f"time; with the counts downloaded every call {dl * 1e6:.1f} us ({dls[0] * 1e6:.1f} .. {dls[1] * 1e6:.1f}, {kd} "
            f"calls) = {r['n'] / dl / r['fs']:.1f} x real time; the stream's first call read {r['heard']} copies of groups in {r['words']} event words")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
