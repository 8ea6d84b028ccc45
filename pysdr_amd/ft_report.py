"""The frame report's host half: float64, from the device's exact float32 numbers.  What a mode
differs in -- its tones, baud, symbols and slots -- comes in as arguments; the defaults are FT8's.  The skimmer's
``_measure`` (``ft.py``) puts these together for the records of a release."""
from __future__ import annotations

import numpy as np

from . import _lib

REPORT_MAX = 4096                                # candidates of one report call
SNR_BW = 2500.0                                  # the bandwidth an SNR is quoted in
FLOOR_QUANTILE = 0.02                            # a row's floor: this quantile of its NB bin means, all but the least of them
FLOOR_ROWS = (4, 8)                              # a candidate's noise: the median floor of the rows this far away, either side: behind the prototype's stop band
CAL = -0.7                                       # dB: the bias of so low a quantile, measured (tests/test_report_oracle.py)


def report_plan(mode=None):
    """What a frame report launches (no device needed): dict of threads per candidate, LDS bytes, symbols of a frame and
    candidates per call; ``mode``: a mode's ``REPORT_MODE`` (default FT8's, 0).  Raises PysdrError for a mode that is neither."""
    v = _lib.plan_call("pysdr_report_plan", 4, int(0 if mode is None else mode))
    return {"threads": v[0], "lds_bytes": v[1], "symbols": v[2], "max_candidates": v[3]}


def delta(a, b, c):
    """Offset of a three-point parabola's peak from the middle point, in points, within +-0.5: 0 where ``a`` or ``c`` is
    missing (negative); with d = a - 2 b + c, clip(0.5 (a - c) / d) where d < 0, else half a point towards the greater
    neighbour.  ``b`` need not be the maximum."""
    a, b, c = float(a), float(b), float(c)
    if a < 0 or c < 0:
        return 0.0
    d = a - 2 * b + c
    if d < 0:
        return float(min(0.5, max(-0.5, 0.5 * (a - c) / d)))
    return 0.5 * float(np.sign(c - a))


def refine(sig9):
    """sig9 [3][3] (time outer, fine row inner) -> (delta_f in raster steps, delta_t in steps, peak): ``delta`` across the
    fine rows and across the steps through the candidate's own place; peak = b - 0.25 (a - c) delta_f, the parabola's
    height across the fine rows (b itself where a neighbour is missing)."""
    s = np.asarray(sig9, np.float64).reshape(3, 3)
    a, b, c = s[1, 0], s[1, 1], s[1, 2]
    df, dt = delta(a, b, c), delta(s[0, 1], b, s[2, 1])
    return df, dt, float(b - 0.25 * (a - c) * df)


def noise_floor(floor, nsym, quantile=None):
    """The bank's ``floor`` sums [nk][NB] over ``nsym`` steps -> float64 [nk]: per row the lower quartile of its bins'
    mean powers"""
    q = FLOOR_QUANTILE if quantile is None else quantile
    return np.quantile(np.asarray(floor, np.float64) / float(nsym), q, axis=1)


def noise_of(floor, nsym, F, nsub, circular, tones=8, rows=None, quantile=None):
    """The noise power per bin for a candidate on fine row ``F``: the median of the floors of the rows 4 to 8 rows away
    on either side (circular where the raster is); of all other rows if there are none; and on a raster of one row the
    lower quartile of that row's own bins outside j - 2 .. j + 2 tones + 2."""
    floor = np.asarray(floor, np.float64)
    nk = floor.shape[0]
    lo, hi = FLOOR_ROWS if rows is None else rows
    q = FLOOR_QUANTILE if quantile is None else quantile
    a, j = divmod(int(F), int(nsub))
    if nk == 1:
        b = np.arange(floor.shape[1])
        out = floor[0, (b < j - 2) | (b > j + 2 * tones + 2)]
        return float(np.quantile((out if len(out) else floor[0]) / float(nsym), q))
    fl = noise_floor(floor, nsym, q)
    far = set()
    for d in range(lo, hi + 1):
        for r in (a - d, a + d):
            if circular:
                far.add(r % nk)
            elif 0 <= r < nk:
                far.add(r)
    far.discard(a)
    if not far:
        far = set(range(nk)) - {a}
    return float(np.median(fl[sorted(far)]))


def snr_db(peak, noise, nsym, baud=6.25, cal=None):
    """10 log10(max(peak / nsym - noise, 1e-3 noise) / noise) - 10 log10(2500 / baud) + CAL: dB in 2500 Hz"""
    cal = CAL if cal is None else cal
    s = max(float(peak) / float(nsym) - float(noise), 1e-3 * float(noise))
    return 10 * np.log10(s / float(noise)) - 10 * np.log10(SNR_BW / baud) + cal


def spots(records, reach=8):
    """Among the ``ok`` records with equal ``bits77`` whose ``t0`` differ by at most ``reach`` steps keep the one of
    greatest ``sig`` (ties: the lower (t0, F)): one message seen on two fine rows, or a step apart, is one spot.  -> the
    records kept, in their order; records without ``ok`` are not spots."""
    ok = [r for r in records if r.get("ok")]
    keys = [bytes(np.asarray(r["bits77"], np.uint8)) for r in ok]
    out = []
    for i, r in enumerate(ok):
        beaten = False
        for k, o in enumerate(ok):
            if k == i or keys[k] != keys[i] or abs(o["t0"] - r["t0"]) > reach:
                continue
            if o["sig"] > r["sig"] or (o["sig"] == r["sig"] and (o["t0"], o["F"]) < (r["t0"], r["F"])):
                beaten = True
                break
        if not beaten:
            out.append(r)
    return out


def spot_line(rec, f_centre=0.0, slot_seconds=15.0):
    """A reported record as the usual line ``HHMMSS snr dt freq ~ text``: the slot's UTC start, dB in 2500 Hz, seconds
    against the nominal start, Hz (``f_centre`` is the band centre's dial offset).  Without ``t_first`` the time is empty
    and dt is the frame's time into the stream."""
    if "slot" in rec:
        s = int(rec["slot"] * slot_seconds) % 86400
        when, dt = f"{s // 3600:02d}{s // 60 % 60:02d}{s % 60:02d}", rec["dt_fine"]
    else:
        when, dt = "", rec["t_fine"]
    return f"{when:6s} {int(round(rec['snr'])):3d} {dt:4.1f} {int(round(f_centre + rec['f_fine'])):4d} ~  {rec['text'] or ''}".rstrip()
