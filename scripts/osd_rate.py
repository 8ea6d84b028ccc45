"""Time ordered-statistics decoding behind min-sum on the 4096 candidates of
``scripts/ldpc_rate.py``: an FT8 skimmer's spectrum ring, half of the candidates the decoded frames repeated and half random
points of the raster, which min-sum leaves without a message -- so about 2048 runs of the second stage per call.  ``decode``
with ``osd=2``, with ``osd=1`` and without are timed in one run, alternating; the call without is the path as it was before
the second stage came.  There is no target.  Writes profiles/osd_rate.txt.

    python scripts/osd_rate.py [--reps 20]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, ".."), HERE]

from ldpc_rate import CHANNELS, FS, N, SECONDS, STATIONS, stream, timed  # noqa: E402  (the same stream and candidates)
from pysdr_amd import ft8, ft8msg, ldpc  # noqa: E402


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
    paths = (("osd=2", 2), ("osd=1", 1), ("without", None))
    got = {}
    for _ in range(5):                                               # warm up every path
        for name, osd in paths:
            got[name] = sk.dec.decode(F, t0, cfg, osd=osd)
    ts = {name: [] for name, _ in paths}
    for _ in range(reps):                                            # alternating, in one run
        for name, osd in paths:
            ts[name] += list(timed(lambda: sk.dec.decode(F, t0, cfg, osd=osd), 1))
    sk.close()
    base = np.median(ts["without"])
    sent = [s[3] for s in STATIONS]
    lines = [f"{N} candidates of a {SECONDS:.0f} s FT8 stream ({len(good)} frames decoded of {len(STATIONS)} sent, repeated to {N // 2}; {N // 2} "
             f"random points of the raster), iters 30, alpha 0.8125; host clock around one decode call that ends in a synchronise, "
             f"5 warm-up calls, {reps} timed calls of each path, alternating"]
    for name, osd in paths:
        t, g = np.array(ts[name]), got[name]
        ran = int((g["osd"] > 0).sum()) if osd is not None else 0
        more = ""
        if osd is not None:
            new = np.flatnonzero((g["osd"] > 0) & (g["status"] == 2))
            texts = [ft8msg.unpack77(g["bits"][i, :77]) for i in new]
            more = (f", the second stage ran on {ran} candidates ({ldpc.OSD_PATTERNS[osd]} patterns each) and gave {len(new)} messages "
                    f"({sum(v in sent for v in texts)} of them a station's text); {1e3 * (np.median(t) - base) / max(ran, 1):.3f} us per run over "
                    f"the call without")
        lines.append(f"decode {name}: median {np.median(t):.3f} ms, min {t.min():.3f} ms, max {t.max():.3f} ms; {int((g['status'] == 2).sum())} status 2{more}")
    return lines


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "osd_rate.txt"))
    a = ap.parse_args()
    lines = run(a.reps)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
