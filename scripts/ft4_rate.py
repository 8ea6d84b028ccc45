"""Time one queued FT4 skimmer call (max_out = 256 row outputs) on 512 rows with device input, at S = 48 and S = 72
(DESIGN.md 3 item 23, 4.9): the channelizer's pass, the spectrum kernel, the sync kernel.  The method is
scripts/ft8_rate.py's.  Writes profiles/ft4_rate.txt.

    python scripts/ft4_rate.py [--reps 20]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from pysdr_amd import _lib, ft4  # noqa: E402

ROWS, MAX_OUT = 512, 256


def run(fs, reps):
    S, D, M = ft4.shape(fs)
    sk = ft4.FT4_Skimmer(fs, channels=(0, ROWS), max_in=MAX_OUT * D, max_out=MAX_OUT)
    L = _lib.lib()
    rng = np.random.default_rng(1)
    n = MAX_OUT * D
    x = (0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    d = C.c_void_p()
    _lib.check(L.pysdr_dev_alloc(0, x.nbytes, C.byref(d)), "alloc")
    _lib.check(L.pysdr_dev_upload(0, d, C.c_void_p(x.ctypes.data), x.nbytes), "upload")
    warm = ft4.EMIT_LAG * (S // 4) // MAX_OUT + 5                       # past the 408 steps before the first score
    for _ in range(warm):
        sk.dec.decode_raw(d.value, n, on_device=True, events=None)
    sk.sync()
    assert sk.dec.t_done > ft4.HOLD
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        sk.dec.decode_raw(d.value, n, on_device=True, events=None)
        sk.sync()
        ts.append(time.perf_counter() - t)
    _lib.check(L.pysdr_dev_free(0, d), "free")
    sk.close()
    ts = np.array(ts) * 1e3
    macs = (S // 2 + 6) * S // (S // 4)
    secs = MAX_OUT / (S * ft4.BAUD)
    return (f"fs {fs:.0f} S {S} M {M} D {D}: {ROWS} rows x {S // 2} decoders, one call of {MAX_OUT} outputs per row ({secs:.3f} s of signal, "
            f"{n} input samples): median {np.median(ts):.3f} ms, min {ts.min():.3f} ms over {reps} calls, channelizer included; "
            f"spectrum {macs} complex MACs per row sample; {secs / (np.median(ts) * 1e-3):.0f} x real time")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    lines = [run(256 * 1000.0, a.reps), run(256 * 1500.0, a.reps)]
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "ft4_rate.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
