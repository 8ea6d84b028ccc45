"""Time the frame report on the 4096 candidates of ``scripts/ldpc_rate.py``: an FT8 skimmer's
spectrum ring, half of the candidates the decoded frames repeated and half random points of the raster.  ``decode`` alone --
the path as it was before the report came -- against ``decode`` + ``floor`` + ``report`` on the words ``decode`` gave, and
the two new calls on their own, timed in one run, alternating.  There is no target.  Writes profiles/report_rate.txt.

    python scripts/report_rate.py [--reps 20]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, ".."), HERE]

from ldpc_rate import CHANNELS, FS, N, SECONDS, STATIONS, stream, timed  # noqa: E402  (the same stream and candidates)
from pysdr_amd import ft8, ldpc  # noqa: E402


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
    bits = sk.dec.decode(F, t0, cfg)["bits"]

    def both():
        d = sk.dec.decode(F, t0, cfg)
        sk.dec.floor(done - 1, ft8.SYMBOLS)
        return sk.dec.report(F, t0, d["bits"])

    paths = (("decode + floor + report", both), ("decode alone", lambda: sk.dec.decode(F, t0, cfg)),
             ("floor alone", lambda: sk.dec.floor(done - 1, ft8.SYMBOLS)), ("report alone", lambda: sk.dec.report(F, t0, bits)))
    got = {}
    for _ in range(5):                                               # warm up every path
        for name, fn in paths:
            got[name] = fn()
    ts = {name: [] for name, _ in paths}
    for _ in range(reps):                                            # alternating, in one run
        for name, fn in paths:
            ts[name] += list(timed(fn, 1))
    sk.close()
    rep = got["report alone"]
    okd = got["decode alone"]["status"] == 2
    lines = [f"{N} candidates of a {SECONDS:.0f} s FT8 stream ({len(good)} frames decoded of {len(STATIONS)} sent, repeated to {N // 2}; {N // 2} "
             f"random points of the raster), iters 30, alpha 0.8125; host clock around calls that each end in a synchronise, 5 warm-up "
             f"calls, {reps} timed calls of each path, alternating; the report's host half (packing 91 bits to 12 bytes in NumPy) is inside "
             f"the clock; no trace and no counters were taken"]
    for name, _ in paths:
        t = np.array(ts[name])
        lines.append(f"{name}: median {np.median(t):.3f} ms, min {t.min():.3f} ms, max {t.max():.3f} ms")
    extra = np.median(ts["decode + floor + report"]) - np.median(ts["decode alone"])
    lines.append(f"the report costs {extra:.3f} ms per call of {N} candidates over decode alone, {1e3 * extra / N:.3f} us per candidate")
    lines.append(f"decoded frames: nhard {int(rep['nhard'][okd].min())} to {int(rep['nhard'][okd].max())}, nsync {int(rep['nsync'][okd].min())} to "
                 f"{int(rep['nsync'][okd].max())}; the other candidates, with the words min-sum left: nhard {int(rep['nhard'][~okd].min())} to "
                 f"{int(rep['nhard'][~okd].max())} (median {int(np.median(rep['nhard'][~okd]))}), nsync {int(rep['nsync'][~okd].min())} to "
                 f"{int(rep['nsync'][~okd].max())} (median {int(np.median(rep['nsync'][~okd]))})")
    return lines


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "report_rate.txt"))
    a = ap.parse_args()
    lines = run(a.reps)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
