"""The case table of the mix + decimate front end: one case per compiled instantiation.

Which kernel a context runs is decided by the decimator's shape alone (mixdec_plan.h: md_select, plan_mixdec,
plan_front_end).  Each case here is an operating point (input rate -> 48 kHz, prototype length, number of
sub-receivers) NAMED AFTER the instantiation it is meant to reach; tests/test_front_end_cases.py asks the library
(pysdr_front_end_plan, pysdr_front_end_shapes: no GPU needed) that every case reaches its instantiation and that every
compiled instantiation has a case, and tests/test_gpu_front_end_sweep.py runs every case against the float64 oracle.

Signals: every sub-receiver listens to a carrier of its own -- distinct offset, tone and amplitude, so that two
receivers swapped or one written twice cannot pass -- AM and USB alternating (audio comparable on every sample,
no NFM start-up allowance), amplitudes 0.12 .. 0.26 (6.7 dB: a receiver tuned 80 dB below its neighbours would
measure rounding noise against itself, bench.py RX6)."""
import ctypes as C
from collections import namedtuple

import numpy as np

from oracle import sdr_oracle as so

FS_OUT = 48e3
FORM_VECTOR, FORM_MFMA, FORM_SMALL = 0, 1, 2
TOL = 1e-5                      # the project's bar (BASELINE.json north star, test_gpu_parity.TOL)
COND = TOL / 4                  # float32 mirror vs float64 master: what makes TOL against the master meaningful

# name: what the case is called in test ids; expect: ('v', (R, NJ, TPB, MM)) or ('m', shape id)
Case = namedtuple("Case", "name fs ntaps nrx expect")


def _vec(tag, fs, ntaps, nrx, nj, tpb, mm):
    return Case(f"{tag}x{nrx}-v{nrx}.{nj}.{tpb}.{mm}", fs, ntaps, nrx, ('v', (nrx, nj, tpb, mm)))


CASES = (
    # 255 taps at UP = 3 (the BASELINE configurations): <R,6,1024,0>, unrolled taps; halves above 4 RX
    [_vec("8M255", 8e6, 255, r, 6, 1024, 0) for r in range(1, 9)]
    # 1001 taps at 2/125: nothing special-cased, the generic form with the taps in LDS
    + [_vec("3M1001", 3e6, 1001, r, 0, 1024, 0) for r in range(1, 9)]
    # 1001 taps at UP = 6: one RX holds its taps, 2 - 6 RX on the matrix cores (4x4x1)
    + [_vec("7M1001", 7e6, 1001, 1, 11, 1024, 0)]
    + [_vec("7M1001", 7e6, 1001, r, 11, 768, 1) for r in range(2, 7)]
    # 1001 taps at UP = 3: likewise; 5 and 6 RX with 512 threads of 256 registers
    + [_vec("8M1001", 8e6, 1001, 1, 21, 1024, 0)]
    + [_vec("8M1001", 8e6, 1001, r, 21, 768 if r <= 4 else 512, 1) for r in range(2, 7)]
    # the other single-RX compile-time tap loops: 255 taps in one branch, 63 taps in one branch
    + [_vec("2M4x255", 2.4e6, 255, 1, 16, 1024, 0), _vec("6M144x63", 6.144e6, 63, 1, 4, 1024, 0)]
    # one RX with a long prototype on the matrix cores: PYSDR_MFMA_SHAPES 0 .. 6
    + [Case(f"{tag}-mfma{sid}", fs, ntaps, 1, ('m', sid)) for sid, (tag, fs, ntaps) in enumerate(
        [("2M048x1001", 2.048e6, 1001), ("1M92x255", 1.92e6, 255), ("1M024x1001", 1.024e6, 1001), ("2M56x1001", 2.56e6, 1001),
         ("1M792x1001", 1.792e6, 1001), ("1M536x1001", 1.536e6, 1001), ("1M92x1001", 1.92e6, 1001)])]
)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
VECTOR_CASES = [c for c in CASES if c.expect[0] == 'v']
MFMA_CASES = [c for c in CASES if c.expect[0] == 'm']

# where the sub-receivers listen, as fractions of the input rate (inside the +-0.4 fs that every rate passes), in an order
# that puts neighbours in the table far apart in frequency
_OFFSETS = (0.06, -0.27, 0.39, -0.05, 0.17, -0.38, 0.28, -0.16)


def case_cfg(case):
    """The cfg dict ``synth_iq`` / ``make_receivers`` / ``make_gpu_receivers`` take."""
    carriers, rx = [], []
    for i in range(case.nrx):
        f = round(_OFFSETS[i] * case.fs / 1e3) * 1e3 + 100.0 * i
        amp = 0.12 + 0.02 * ((3 * i) % 8)                   # 0.12 .. 0.26, all different
        tone = 500.0 + 150.0 * i
        if i % 2 == 0:
            carriers.append(dict(f=f, kind='am', amp=amp, tone=tone, depth=0.5))
            rx.append(dict(frq=f, mode='AM', video_bw=10e3, af_bw=5e3))
        else:
            carriers.append(dict(f=f, kind='usb', amp=amp, tone=tone))
            rx.append(dict(frq=f, mode='USB', video_bw=10e3, af_bw=3e3))
    return dict(fs=case.fs, fs_out=FS_OUT, ntaps_dec=case.ntaps, noise=2e-3, carriers=carriers, rx=rx)


def chunk_len(case):
    return so.chunk_sizes(case.fs, FS_OUT)[3]


def ragged_calls(L):
    """Calls with no output, one that straddles several tiles, odd lengths that flip the parity of the staged image."""
    return [L, L, 1000, 7, L - 13, 2 * L + 5, 333]


# ---- what the library says ------------------------------------------------------------------------------------------
Plan = namedtuple("Plan", "form fits key mshape taps_lds tile_out yflush tile_cap kpad")
DEFAULT_TUNING = dict(tile_bytes=0, threads=1024, wgs_per_cu=1, yflush_cap=0, mfma_enable=1)


def query(case_or_shape, want_peak=1, **tuning):
    """pysdr_front_end_plan for a Case (or (nrx, up, down, ntaps)) under DEFAULT_TUNING overridden by ``tuning``."""
    from pysdr_amd import _lib
    if isinstance(case_or_shape, Case):
        up, down = so.chunk_sizes(case_or_shape.fs, FS_OUT)[:2]
        shape = (case_or_shape.nrx, up, down, case_or_shape.ntaps)
    else:
        shape = tuple(case_or_shape)
    t = dict(DEFAULT_TUNING, **tuning)
    out = (C.c_int32 * 12)()
    _lib.check(_lib.lib().pysdr_front_end_plan(*shape, t['tile_bytes'], t['threads'], t['wgs_per_cu'], t['yflush_cap'],
                                               t['mfma_enable'], want_peak, out), "pysdr_front_end_plan")
    o = list(out)
    return Plan(o[0], bool(o[1]), tuple(o[2:6]), o[6], o[7], o[8], o[9], o[10], o[11])


def context_tuning(ctx_handle):
    """The tuning a live context runs with (pysdr_get_tuning), as the keyword arguments of ``query``."""
    from pysdr_amd import _lib
    t = (C.c_int32 * 8)()
    _lib.check(_lib.lib().pysdr_get_tuning(ctx_handle, t), "pysdr_get_tuning")
    return dict(wgs_per_cu=t[2], yflush_cap=t[3], tile_bytes=t[4], threads=t[5], mfma_enable=t[7])


def selected(plan):
    """('v', key) / ('m', shape id) / ('s', key): comparable with Case.expect."""
    if plan.form == FORM_MFMA:
        return ('m', plan.mshape)
    return ('v' if plan.form == FORM_VECTOR else 's', plan.key)


def compiled():
    """Everything the library has compiled, in Case.expect's terms; MFMA entries also as {id: (up, down, taps per branch)}."""
    from pysdr_amd import _lib
    L = _lib.lib()
    vec, mm = [], {}
    for fam, sink in ((FORM_VECTOR, vec), (FORM_MFMA, mm)):
        n = C.c_int(0)
        _lib.check(L.pysdr_front_end_shapes(fam, -1, None, C.byref(n)), "pysdr_front_end_shapes")
        for i in range(n.value):
            o = (C.c_int32 * 4)()
            _lib.check(L.pysdr_front_end_shapes(fam, i, o, None), "pysdr_front_end_shapes")
            if fam == FORM_VECTOR:
                vec.append(('v', tuple(o)))
            else:
                mm[o[0]] = tuple(o[1:])
    return vec, mm


# ---- the float64 master ---------------------------------------------------------------------------------------------
def relerr(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.size == 0:
        return 0.0
    return float(np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-30))


def run_oracle(cfg, x, calls, dtype, ntaps_af=255):
    """-> per sub-receiver, per call: (iq, am) of the oracle in ``dtype`` (np.float64: the master)."""
    out = []
    for o in so.make_receivers(cfg, dtype, ntaps_af=ntaps_af):
        pos, per = 0, []
        for c in calls:
            am = o.demod_data(x[pos:pos + c])
            per.append((np.array(o.iq), np.array(am)))
            pos += c
        out.append(per)
    return out
