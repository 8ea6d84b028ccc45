"""Rate of the RTTY decoder bank: all 2041 decoders of a 48 kHz line (bins [0, NFFT - NBINS)) plus the finder, on
lines resident on the device, from host lines, and the whole skimmer (IQ -> filterbank -> decoders), in lines/s and
times real time (4 lines per 22 ms symbol: 181.8 lines/s per receiver); beside the CPU restatement of the same
decoders (tests/rtty_decoder_oracle.py, NumPy on one core).

    python scripts/rtty_rate.py [LINES_PER_CALL]
"""
import ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[v] = "1"                          # the restatement on one core
import numpy as np
from oracle import rtty_oracle as ro
from pysdr_amd import _lib, rtty
from tests import rtty_decoder_oracle as rdo

RT = 4 / 22e-3
B = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
rng = np.random.default_rng(1)
sigs = [(int(b), "RYRY CQ TEST DE AB1CD 599", 0.05, float(rng.uniform(0, 0.165))) for b in range(40, 2000, 97)]
x = rdo.synth_band(48000, sigs, (B // 4 + 1) * 1056, 0.01, 1)
lines = ro.RttyFilterbank(48000).push(x).astype(np.float32)
assert lines.shape == (B, 2048)
lib = _lib.lib()
dec = rtty.RTTY_Decoders(48000, max_lines=B)


def rate(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


d = C.c_void_p()
_lib.check(lib.pysdr_dev_alloc(0, lines.nbytes, C.byref(d)), "alloc")
flip = np.ascontiguousarray(lines[:, ::-1])
_lib.check(lib.pysdr_dev_upload(0, d, C.c_void_p(flip.ctypes.data), flip.nbytes), "upload")
print(f"RTTY decoder bank, {dec.nb} decoders + the finder over {dec.find_hi - dec.find_lo} bins, {B} lines per call")
for what, fn in (("device lines", lambda: dec.decode_raw(d.value, B, True, False)),
                 ("host lines  ", lambda: dec.decode_raw(lines, B, False, True))):
    dt = rate(fn, 20)
    print(f"  {what}: {dt * 1e3:8.3f} ms per call = {B / dt:12.0f} lines/s = {B / dt / RT:9.0f} x real time")
for Bs in (B // 4, 16, 1):
    dt = rate(lambda: dec.decode_raw(d.value, Bs, True, False), 50)
    print(f"  device lines, {Bs:4d} per call: {dt * 1e3:8.3f} ms per call = {Bs / dt:12.0f} lines/s = {Bs / dt / RT:9.0f} x real time")
_lib.check(lib.pysdr_dev_free(0, d), "free")
dec.close()
sk = rtty.RTTY_Skimmer(48000, max_symbols=B // 4)
xs = np.ascontiguousarray(x[1056:])              # B/4 symbols after the priming one
sk.push(x[:1056])
dt = rate(lambda: sk.push(xs), 10)
print(f"  skimmer (IQ -> filterbank -> decoders, no download): {dt * 1e3:8.3f} ms per {B} lines = {B / dt:10.0f} lines/s = "
      f"{B / dt / RT:7.0f} x real time")
sk.close()
Lc = min(B, 600)
bank = rdo.DecoderBank(0, 2041, 800, 1243)
t0 = time.perf_counter()
bank.decode(lines[:Lc])
dt = time.perf_counter() - t0
print(f"  CPU restatement (NumPy, one core), {Lc} lines: {dt:8.3f} s = {Lc / dt:10.1f} lines/s = {Lc / dt / RT:7.2f} x real time")
