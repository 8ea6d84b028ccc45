"""Rate probe of the channel bank (bank.hip): AM / NFM audio of every channel of a raster, against
the only other way to the same result, six sub-receivers per context (``bench.py --workload rx6``).

    python scripts/bank_rate.py [--no-rx6] [--modes AM,USB] [--one M D FS MODE]
        (--one: a single shape, a few calls: for a profiler run; MODE may be NFM, AM, USB or CW.
         --modes: the modes of the table, default NFM,AM; USB and CW run ``SidebandBank``)

Device-resident input of 2^25 samples per call, default prototype, all M channels, 255 AF taps at 4 kHz; the results
stay on the device.  At least 20 ms of warm-up, then at least 60 ms of queued calls ending in one synchronise.  Per shape
and mode (NFM with the squelch armed, AM with the AGC on): input GS/s, demodulated channel-samples per second (input
rate x nk / D), and the share of the time a channelizer alone takes on the same input (timed the same way, in the same
process).  Then, in a child process, ``bench.py --workload rx6``: its input rate x 6 x fs_out / fs is what six
sub-receivers demodulate per second.  Exit status 1 if the bank does not exceed that figure at every shape."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pysdr_amd import _lib                                    # noqa: E402
from pysdr_amd.bank import BANK_MODES, ChannelBank, SidebandBank, plan      # noqa: E402
from pysdr_amd.channelizer import Channelizer                 # noqa: E402

N_CALL = 1 << 25
SHAPES = [(3.2e6, 256, 128), (8e6, 640, 320), (51.2e6, 4096, 2048)]        # 12.5 kHz rasters, fs_out = 25 kHz
MODES = [("NFM", dict(squelch=0.3)), ("AM", dict(agc=True))]
SIDEBAND = [("USB", dict(agc=True, af_bw=3e3)), ("CW", dict(agc=True, af_bw=500.0))]     # 255 complex taps; CW at 700 Hz
RX6_FS, RX6_FS_OUT = 8e6, 48e3


def dev_noise(lib, n, seed=1):
    rng = np.random.default_rng(seed)
    blk = (0.1 * (rng.standard_normal(1 << 20) + 1j * rng.standard_normal(1 << 20))).astype(np.complex64)
    d = C.c_void_p()
    _lib.check(lib.pysdr_dev_alloc(0, n * 8, C.byref(d)), "alloc input")
    for off in range(0, n, len(blk)):
        k = min(len(blk), n - off)
        _lib.check(lib.pysdr_dev_upload(0, C.c_void_p(d.value + off * 8), C.c_void_p(blk.ctypes.data), k * 8), "upload")
    return d


def timed(call, sync, quick):
    def calls(k):
        t0 = time.perf_counter()
        for _ in range(k):
            call()
        sync()
        return time.perf_counter() - t0

    if quick:
        calls(2)
        return calls(4) / 4
    warm, per = 0.0, 1.0
    while warm < 0.02:
        dt = calls(2)
        warm, per = warm + dt, dt / 2
    k = max(8, int(0.06 / per) + 1)
    return calls(k) / k


def chan_time(lib, d_x, fs, M, D, quick=False):
    ch = Channelizer(fs, M, D, max_in=N_CALL)
    pitch = N_CALL // D + 16
    d_y = C.c_void_p()
    _lib.check(lib.pysdr_dev_alloc(0, M * pitch * 8, C.byref(d_y)), "alloc output")
    per = timed(lambda: ch.push_device(d_x.value, N_CALL, d_y.value, pitch, sync=False), ch.sync, quick)
    ch.close()
    lib.pysdr_dev_free(0, d_y)
    return per


def bank_time(d_x, fs, M, D, mode, kw, quick=False):
    kw = dict(dict(af_bw=4e3), **kw)
    b = (ChannelBank if mode in BANK_MODES else SidebandBank)(fs, M, D, mode=mode, ntaps_af=255, max_in=N_CALL, **kw)
    per = timed(lambda: b.push_device(d_x.value, N_CALL, sync=False), b.sync, quick)
    b.close()
    return per


def rx6_rate():
    """bench.py --workload rx6 in a child process -> (input MS/s, demodulated channel-samples/s)"""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "rx6", "--no-cpu-baseline",
           "--no-cpu-mp", "--no-host-fed"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    if out.returncode != 0 or not line:
        raise RuntimeError(f"bench.py --workload rx6 failed ({out.returncode}): {out.stderr[-2000:]}")
    d = json.loads(line[-1])
    assert d["unit"] == "MS/s", d["unit"]
    return d["value"], d["value"] * 1e6 * 6 * RX6_FS_OUT / RX6_FS


def main():
    lib = _lib.lib()
    _lib.require_gpu()
    d_x = dev_noise(lib, N_CALL)
    if "--one" in sys.argv:
        i = sys.argv.index("--one")
        M, D, fs, mode = int(sys.argv[i + 1]), int(sys.argv[i + 2]), float(sys.argv[i + 3]), sys.argv[i + 4]
        per = bank_time(d_x, fs, M, D, mode, dict(MODES + SIDEBAND)[mode], quick=True)
        print(f"M {M} D {D} {mode}: {per * 1e3:.3f} ms per call of 2^25 samples, {N_CALL / per / 1e9:.2f} GS/s")
        return 0
    modes = MODES
    if "--modes" in sys.argv:
        want = sys.argv[sys.argv.index("--modes") + 1].split(",")
        modes = [(m, dict(MODES + SIDEBAND)[m]) for m in want]
    rows = []
    for fs, M, D in SHAPES:
        tc = chan_time(lib, d_x, fs, M, D)
        for mode, kw in modes:
            tb = bank_time(d_x, fs, M, D, mode, kw)
            rows.append(dict(fs=fs, M=M, D=D, mode=mode, kw=kw, ms=tb * 1e3, chan_ms=tc * 1e3, gsps=N_CALL / tb / 1e9,
                             demod_sps=N_CALL / tb * M / D))
    lib.pysdr_dev_free(0, d_x)
    ref = None
    if "--no-rx6" not in sys.argv:
        msps, ref = rx6_rate()
        print(f"rx6 (bench.py --workload rx6: 8 MS/s, 6 RX, 3/500): {msps:.1f} MS/s input x 6 x 48 kHz / 8 MHz = "
              f"{ref / 1e6:.2f} M demodulated channel-samples/s")
    ok = True
    for r in rows:
        p = plan(r["M"], 255, N_CALL // r["D"])
        txt = (f"bank {r['fs'] / 1e6:g} MS/s M {r['M']} D {r['D']} {r['mode']} {r['kw']} ({p['tile']} outputs / workgroup, "
               f"{p['threads']} threads, {p['lds_bytes'] * (1 if r['mode'] in BANK_MODES else 2)} B LDS): {r['ms']:.3f} ms per call of 2^25 = {r['gsps']:.2f} GS/s input, "
               f"{r['demod_sps'] / 1e9:.2f} G demodulated channel-samples/s; the channelizer alone {r['chan_ms']:.3f} ms = "
               f"{100 * r['chan_ms'] / r['ms']:.0f} % of the time")
        if ref is not None:
            good = r["demod_sps"] > ref
            ok = ok and good
            txt += f"; {r['demod_sps'] / ref:.0f} x rx6 {'ok' if good else 'BELOW rx6'}"
        print(txt)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
