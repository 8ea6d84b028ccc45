"""Rate probe of the SSTV skimmer (sstv.hip) beside the channelizer pass it rides on.

    python scripts/sstv_rate.py [--out FILE]            (default profiles/sstv_rate.txt)

A 12.5 kHz raster of a 10 MS/s band, all M = 800 rows at 25 kHz (D = 400), FM detector.  Device-resident input: noise
plus three PD120 stations that send their header and the first lines of a picture, 1.31 s in eight calls that complete
max_out = 4096 outputs per row each (164 ms of signal); behind them the three rows are inside their pictures, where they
stay for 126 s whatever they are fed.  The last of the eight calls is then repeated: after at least 50 ms and four calls
of warm-up, calls are timed one by one, each ending in a synchronise (host clock), until there are 25 of them and at least
60 ms; the median is reported with the least and the most.  In the same process, on the same device:
``Channelizer.push_device`` alone (device output, the skimmer's prototype) and the skimmer (the same channelizer pass with
the decoders queued behind it, nothing downloaded), and the same with what ``SSTV_Skimmer.push`` downloads per call (the
counts of every row)."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pysdr_amd import _lib                                    # noqa: E402
from pysdr_amd import sstv                                    # noqa: E402
from pysdr_amd.channelizer import Channelizer                 # noqa: E402

MAX_OUT = 4096
FS, M, D = 10e6, 800, 400
PREFIX = 8                                                    # calls that bring the stations into their pictures
CALLS, WINDOW = 25, 0.060
STATIONS = ((37, 0.0), (401, 0.004), (655, 0.009))            # (channel, start s)


def dev_input(lib, n, seed=1):
    rng = np.random.default_rng(seed)
    x = (0.01 * (rng.standard_normal(n, np.float32) + 1j * rng.standard_normal(n, np.float32))).astype(np.complex64)
    mode = sstv.mode_named("PD120")
    col = np.arange(mode.width)
    pic = np.array([[np.round(127.5 + 100.0 * np.sin(2 * np.pi * (3 + j) * col / mode.width + l)) for j in range(mode.scans)]
                    for l in range(1)]).astype(np.uint8)
    tones = sstv.tones(mode, pic)
    for ch, t0 in STATIONS:
        s = 0.05 * sstv.waveform(tones, FS, ch * FS / M, "FM")
        at = int(t0 * FS)
        x[at:at + len(s)] += s[:n - at]
    d = C.c_void_p()
    _lib.check(lib.pysdr_dev_alloc(0, n * 8, C.byref(d)), "alloc input")
    _lib.check(lib.pysdr_dev_upload(0, d, C.c_void_p(x.ctypes.data), n * 8), "upload")
    return d


def timed(call, sync):
    """-> (median seconds per call, (min, max), calls, seconds timed)"""
    def one():
        t0 = time.perf_counter()
        call()
        sync()
        return time.perf_counter() - t0

    warm, k = 0.0, 0
    while warm < 0.05 or k < 4:
        warm, k = warm + one(), k + 1
    t = []
    while len(t) < CALLS or sum(t) < WINDOW:
        t.append(one())
    total = sum(t)
    t.sort()
    return t[len(t) // 2], (t[0], t[-1]), len(t), total


def main():
    out = os.path.join(ROOT, "profiles", "sstv_rate.txt")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    lib = _lib.lib()
    _lib.require_gpu()
    n = MAX_OUT * D
    d_x = dev_input(lib, PREFIX * n)
    last = d_x.value + (PREFIX - 1) * n * 8
    ch = Channelizer(FS, M, D, sstv.prototype(FS, M, D), max_in=n)
    pitch = MAX_OUT + 16
    d_y = C.c_void_p()
    _lib.check(lib.pysdr_dev_alloc(0, M * pitch * 8, C.byref(d_y)), "alloc output")
    (t_ch, chs, kc, wc) = timed(lambda: ch.push_device(last, n, d_y.value, pitch, sync=False), ch.sync)
    ch.close()
    lib.pysdr_dev_free(0, d_y)
    sk = sstv.SSTV_Skimmer(FS, M, D, max_in=n, max_out=MAX_OUT, det="FM")
    words = 0
    for k in range(PREFIX):
        words += int(sk.dec.decode_raw(d_x.value + k * n * 8, n, on_device=True, events="counts")["counts"].sum())
    st = sk.dec.state()
    rows = np.flatnonzero(st["phase"] == 2)
    (t_sk, sks, ks, ws) = timed(lambda: sk.dec.decode_raw(last, n, on_device=True, events=None), sk.sync)
    (t_dl, dls, kd, wd) = timed(lambda: sk.dec.decode_raw(last, n, on_device=True, events="counts"), sk.sync)
    r = sk.dec.decode_raw(last, n, on_device=True, events="counts")
    st = sk.dec.state()
    p = sk.dec.plan
    dec = t_sk - t_ch
    text = (
        f"SSTV skimmer {FS / 1e6:g} MS/s M {M} D {D} ({M} rows at {FS / D:g} S/s, FM, L {sk.L}, {len(sk.modes)} modes; {p['groups']} workgroups of "
        f"{p['threads']} threads, {p['rows']} rows x {p['tile']} outputs per tile, {p['lds_bytes']} B LDS, {p['history']} samples of history, "
        f"{p['cap']} event words per row): {len(rows)} rows inside a PD120 picture (rows {', '.join(map(str, rows))}; {words} event words in the "
        f"{PREFIX} calls before), call of {n} samples = {MAX_OUT} outputs per row: channelizer alone {t_ch * 1e3:.3f} ms "
        f"({chs[0] * 1e3:.3f} .. {chs[1] * 1e3:.3f}, median of {kc} calls, {wc * 1e3:.0f} ms timed), skimmer {t_sk * 1e3:.3f} ms "
        f"({sks[0] * 1e3:.3f} .. {sks[1] * 1e3:.3f}, {ks} calls, {ws * 1e3:.0f} ms timed), decoders {dec * 1e3:.3f} ms = {dec / t_ch:.2f} x the "
        f"channelizer's pass; skimmer {n / t_sk / 1e6:.2f} MS/s input = {n / t_sk / FS:.1f} x real time; with the counts downloaded every call "
        f"{t_dl * 1e3:.3f} ms ({dls[0] * 1e3:.3f} .. {dls[1] * 1e3:.3f}, {kd} calls, {wd * 1e3:.0f} ms timed) = {n / t_dl / FS:.1f} x real time; "
        f"the last call brought {int(r['counts'].sum())} event words, {int((st['phase'] == 2).sum())} rows still inside their pictures at lines "
        f"{', '.join(str(int(v)) for v in st['line'][st['phase'] == 2])}\n")
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    sk.close()
    lib.pysdr_dev_free(0, d_x)
    return 0


if __name__ == "__main__":
    sys.exit(main())
