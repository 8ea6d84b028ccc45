"""Time a-priori decoding at the size of a whole call: 65536 pairs on the 4096 candidates of
``scripts/ldpc_rate.py`` (an FT8 skimmer's spectrum ring, half of the candidates the decoded frames repeated and half random
points of the raster), 16 hypotheses each out of a table of 64.  In the same run, alternating: the AP call on the
candidates' soft bits from the host, the AP call on the candidates straight from the ring, and 16 ``decode_llr`` calls of 4096
on the same soft bits -- the kernel as it was before AP came, doing the same number of decodes.  There is no target: the
file records the figures, their ratio, and the AP stage's share of a 15 s slot.  Writes profiles/ap_rate.txt.

    python scripts/ap_rate.py [--reps 10]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, ".."), HERE]

from ldpc_rate import CHANNELS, FS, N, SECONDS, STATIONS, stream, timed  # noqa: E402  (the same stream and candidates)
from pysdr_amd import ap, ft8, ldpc  # noqa: E402

PER = 16                                                             # hypotheses per candidate: 65536 pairs
CALLS = ("K1ABC", "W9XYZ", "DL1ABC", "JA1XYZ", "G4ABC", "VK2DEF", "PY2GH", "OH8X", "SM5XYZ", "F6ABC", "EA3DEF", "I2GHI", "ZL1JK", "VE3LM", "LU4NO")
SLOT_MS = 15000.0


def table():
    """64 hypotheses of every kind, of which those that name K1ABC and W9XYZ are right for some of the stream's frames"""
    hyps = [ap.hyp_cq()]
    hyps += [ap.hyp_from(c) for c in CALLS]
    hyps += [ap.hyp_cq_from(c) for c in CALLS]
    hyps += [ap.hyp_pair(a, b) for a, b in zip(CALLS, CALLS[1:] + CALLS[:1])]
    hyps += [ap.hyp_pair(b, a) for a, b in zip(CALLS, CALLS[1:] + CALLS[:1])]
    hyps += [ap.hyp_text(s[3]) for s in STATIONS[:3]]
    return hyps[:64]


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
    hyps = table()
    pairs = np.array([(c, h) for c in range(N) for h in sorted(rng.choice(len(hyps), PER, replace=False))], np.int32)
    assert len(hyps) == 64 and len(pairs) == N * PER == ap.PAIR_MAX
    soft = sk.dec.llr(F, t0)
    cfg, apc = ldpc.params(iters=30), ap.params()
    paths = (("AP, soft bits from the host", lambda: ap.decode_llr(sk.dec, soft, pairs, hyps, apc, cfg)),
             ("AP, candidates from the ring", lambda: ap.decode(sk.dec, F, t0, pairs, hyps, apc, cfg)),
             (f"{PER} decode_llr calls", lambda: [sk.dec.decode_llr(soft, cfg) for _ in range(PER)]))
    got = {}
    for _ in range(3):                                               # warm up every path
        for name, fn in paths:
            got[name] = fn()
    ts = {name: [] for name, _ in paths}
    for _ in range(reps):                                            # alternating, in one run
        for name, fn in paths:
            ts[name] += list(timed(fn, 1))
    sk.close()
    a, b = got[paths[0][0]], got[paths[1][0]]
    if not all(np.array_equal(a[k], b[k]) for k in ("pair", "iterations", "nerr", "count", "bits")):
        raise RuntimeError("the AP call from the ring and the one on its soft bits disagree")
    plain = got[paths[2][0]][0]
    lines = [f"{N} candidates of a {SECONDS:.0f} s FT8 stream ({len(good)} frames decoded of {len(STATIONS)} sent, repeated to {N // 2}; {N // 2} "
             f"random points of the raster), {PER} hypotheses each of a table of {len(hyps)}: {len(pairs)} pairs in one call; iters 30, alpha "
             f"0.8125, mag {apc.mag:g}, nerr_max {apc.nerr_max}; host clock around calls that end in a synchronise, 3 warm-up rounds, {reps} "
             f"timed rounds, the paths alternating",
             f"min-sum alone: {int((plain['status'] == 2).sum())} candidates with a message; AP: {int((a['pair'] >= 0).sum())} candidates with a pick, "
             f"{int(a['count'].sum())} pairs of status 2, {int(((a['pair'] >= 0) & (plain['status'] != 2)).sum())} picks where min-sum has no message"]
    med = {}
    for name, _ in paths:
        t = np.array(ts[name])
        med[name] = float(np.median(t))
        lines.append(f"{name}: median {np.median(t):.3f} ms, min {t.min():.3f} ms, max {t.max():.3f} ms; {1e3 * np.median(t) / len(pairs):.3f} us per decode")
    lines.append(f"AP (host soft bits) / {PER} decode_llr calls: {med[paths[0][0]] / med[paths[2][0]]:.3f}; AP (ring) / {PER} decode_llr calls: "
                 f"{med[paths[1][0]] / med[paths[2][0]]:.3f}")
    lines.append(f"the AP stage's share of a 15 s slot at this size: {100 * med[paths[1][0]] / SLOT_MS:.3f} % from the ring, "
                 f"{100 * med[paths[0][0]] / SLOT_MS:.3f} % from host soft bits")
    return lines


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "ap_rate.txt"))
    a = p.parse_args()
    lines = run(a.reps)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
