"""Time ``FT8_Skimmer.push`` of one slot with and without the second pass: 512 rows (51200
samples per second, the whole circle), 20 stations of which three lie 10 dB under and a few hertz from another, 16.5 s -- a 15 s slot and the
tail after which its frames are due -- with ``passes=1`` and ``passes=2``, alternating in one run, by 4.10's method: the
host clock around a ``reset`` and a ``push`` that ends in a synchronise.  There is no target.  Writes profiles/pass_rate.txt.

    python scripts/pass_rate.py [--reps 5]
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, ".."), HERE]

from pysdr_amd import ft8, ldpc  # noqa: E402

FS, SECONDS, NSTATIONS = 51200.0, 16.5, 20


def stream():
    """-> (x, the 77-bit messages sent)"""
    n = int(SECONDS * FS)
    rng = np.random.default_rng(27)
    sigma = np.sqrt(FS / 2500.0 / 2)                                 # noise of power 1 in 2500 Hz
    x = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    f = list(rng.uniform(-20000.0, 20000.0, NSTATIONS - 3))
    snr = list(rng.uniform(-14.0, 0.0, NSTATIONS - 3))
    start = list(rng.uniform(0.3, 1.0, NSTATIONS - 3))
    for k in range(3):                                               # a weaker station a few hertz from a stronger one
        f.append(f[k] + (3.125, 9.375, 21.875)[k])
        snr.append(snr[k] - 10.0)
        start.append(start[k] + 0.24)
    sent = []
    for fk, sk, tk in zip(f, snr, start):
        msg = rng.integers(0, 2, 77)
        sent.append(msg)
        s = ft8.waveform(ft8.tones(ldpc.encode(msg)), fk, FS, phase=fk) * 10 ** (sk / 20)
        at = int(tk * FS)
        x[at:at + len(s)] += s[:n - at]
    return (0.05 * x).astype(np.complex64), sent


def run(reps):
    x, sent = stream()
    keys = {bytes(np.asarray(m, np.uint8)) for m in sent}
    sks = {p: ft8.FT8_Skimmer(FS, max_in=len(x), decode=True, passes=p) for p in (1, 2)}
    ts, recs = {1: [], 2: []}, {}
    for rep in range(reps + 1):                                      # the first round warms both up
        for p, sk in sks.items():
            sk.reset()
            t = time.perf_counter()
            recs[p] = sk.push(x)
            sk.sync()
            if rep:
                ts[p].append((time.perf_counter() - t) * 1e3)
    lines = [f"{sks[1].nk} rows at {FS:.0f} samples per second, {SECONDS} s, {NSTATIONS} stations: {NSTATIONS - 3} at -14 to 0 dB in 2500 Hz and three 10 dB "
             f"under one of them, 3.1, 9.4 and 21.9 Hz and 6 steps away; max_out 256, reach_t {sks[2].reach_t}; host clock around reset + push + sync, "
             f"one warm-up round, {reps} timed rounds, passes=1 and passes=2 alternating; no trace and no counters were taken"]
    for p in (1, 2):
        ok = [r for r in recs[p] if r["ok"]]
        good = {bytes(np.asarray(r["bits77"], np.uint8)) for r in ok}
        t = np.array(ts[p])
        lines.append(f"passes={p}: median {np.median(t):.1f} ms, min {t.min():.1f} ms, max {t.max():.1f} ms; {len(recs[p])} records, {len(ok)} decoded, "
                     f"{len(good & keys)} of the {len(keys)} messages sent, {len(good - keys)} not sent"
                     + (f"; {sum(1 for r in ok if r['pass'] == 2)} records of pass 2" if p == 2 else ""))
    extra = np.median(ts[2]) - np.median(ts[1])
    lines.append(f"the second pass adds {extra:.1f} ms to the slot's {np.median(ts[1]):.1f} ms, {100 * extra / 15000:.2f} % of the 15 s the slot lasts")
    for sk in sks.values():
        sk.close()
    return lines


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "pass_rate.txt"))
    a = ap.parse_args()
    lines = run(a.reps)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
