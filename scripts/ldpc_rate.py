"""Time the LDPC(174,91) decoder on 4096 candidates of an FT8 skimmer's spectrum ring, half decodable and half noise, at
iters = 30: ``decode`` straight from the ring, and the path it replaces the transfer of,
``llr`` with its download of 4096 x 174 floats (that call's code is what it was before the decoder came).  The two are timed
in one run, alternating.  The stream is 14 s at 8 kS/s on three rows with five stations; the decodable candidates are the
frames the skimmer found and decoded, repeated to 2048 -- a candidate's cost does not depend on its neighbours'.
Writes profiles/ldpc_rate.txt.

    python scripts/ldpc_rate.py [--reps 20]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from pysdr_amd import ft8, ft8msg, ldpc  # noqa: E402

FS, CHANNELS, SECONDS, N = 8000.0, (3, 3), 14.0, 4096
STATIONS = ((245.0, -8.0, 0.5, "CQ K1ABC FN42"), (351.3, 0.0, 0.9, "K1ABC W9XYZ -12"), (480.0, -12.0, 0.2, "W9XYZ K1ABC RR73"),
            (300.0, -10.0, 0.7, "CQ DX W9XYZ EN52"), (415.0, -5.0, 0.3, "HELLO WORLD"))


def stream():
    n = int(SECONDS * FS)
    rng = np.random.default_rng(11)
    sigma = np.sqrt(FS / 2500.0 / 2)                                 # noise of power 1 in 2500 Hz
    x = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for f, snr, start, text in STATIONS:
        s = ft8.waveform(ft8.tones(ldpc.encode(ft8msg.pack77(text))), f, FS, phase=f) * 10 ** (snr / 20)
        at = int(start * FS)
        x[at:at + len(s)] += s[:n - at]
    return (0.05 * x).astype(np.complex64)


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()                                                         # both calls end in a synchronise of the skimmer's stream
        ts.append(time.perf_counter() - t)
    return np.array(ts) * 1e3


def run(reps):
    x = stream()
    sk = ft8.FT8_Skimmer(FS, channels=CHANNELS, max_in=len(x), decode=True)
    recs = [r for r in sk.push(x) if r["ok"]]
    if not recs:
        raise RuntimeError("no frame decoded: nothing to time")
    done = sk.dec.t_done
    rng = np.random.default_rng(12)
    good = [(r["F"], r["t0"]) for r in recs]
    F = np.array([good[i % len(good)][0] for i in range(N // 2)] + list(rng.integers(0, sk.nfine, N // 2)), np.int32)
    t0 = np.array([good[i % len(good)][1] for i in range(N // 2)] + list(rng.integers(0, done - 312, N // 2)), np.int64)
    order = rng.permutation(N)                                       # decodable and noise interleaved, as a slot would bring them
    F, t0 = F[order], t0[order]
    cfg = ldpc.params(iters=30)
    for _ in range(5):                                               # warm up both paths
        got = sk.dec.decode(F, t0, cfg)
        sk.dec.llr(F, t0)
    a, b = [], []
    for _ in range(reps):                                            # alternating, in one run
        a += list(timed(lambda: sk.dec.decode(F, t0, cfg), 1))
        b += list(timed(lambda: sk.dec.llr(F, t0), 1))
    a, b = np.array(a), np.array(b)
    ok = int((got["status"] == 2).sum())
    its = got["iterations"]
    sk.close()
    head = (f"{N} candidates of a {SECONDS:.0f} s FT8 stream ({len(good)} frames decoded of {len(STATIONS)} sent, repeated to {N // 2}; {N // 2} noise), "
            f"iters 30, alpha 0.8125: {ok} status 2, mean iterations {its.mean():.1f}")
    return [f"decode from the ring, {head}: median {np.median(a):.3f} ms, min {a.min():.3f} ms over {reps} calls, results "
            f"downloaded (28 bytes per candidate); {N / (np.median(a) * 1e-3):.0f} candidates per second",
            f"llr and its download (696 bytes per candidate), the same {N} candidates: median {np.median(b):.3f} ms, min {b.min():.3f} ms "
            f"over {reps} calls"]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "ldpc_rate.txt"))
    a = ap.parse_args()
    lines = run(a.reps)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
