"""Polyphase channelizer without a GPU: the definition hangs on the existing float64 oracle, the
polyphase form and the float32 mirror of the kernel hang on the definition, the default prototype has the properties
the spec states, and the device-free plan accepts exactly the shapes the spec allows."""
import ctypes as C

import numpy as np
import pytest

import pysdr_amd.channelizer as chz
from pysdr_amd import _lib
from pysdr_amd.design import channelizer_taps
from tests import channelizer_oracle as co


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("D", [16, 32, 64])
def test_definition_equals_nco_plus_rational_decimator(D):
    """every channel of M = 64, over random cuts, against NCO(-k fs/M) + RationalDecimator(h, 1, D) in float64"""
    from oracle import sdr_oracle as so
    M, fs = 64, 8e6
    rng = np.random.default_rng(D)
    n = 3000
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    h = channelizer_taps(M)[:8 * M - 3]                      # (not a multiple of M long)
    cuts = co.random_cuts(n, D, seed=D)
    d = co.Definition(h, M, D)
    mine, i = [], 0
    for c in cuts:
        mine.append(d.process(x[i:i + c]))
        i += c
    mine = np.concatenate(mine, axis=1)
    assert mine.shape == (M, -(-n // D))
    worst = 0.0
    for k in range(M):
        nco = so.NCO(-k * fs / M, fs, dtype=np.float64)
        assert nco.fword == (-k * (1 << 32) // M) % (1 << 32)          # the phase word is exact for a power of two
        dec = so.RationalDecimator(h, 1, D, dtype=np.float64)
        ref, i = [], 0
        for c in cuts:
            ref.append(dec.process(nco.quad_mixer(x[i:i + c])))
            i += c
        worst = max(worst, _rel(mine[k], np.concatenate(ref)))
    print(f"M 64 D {D}: definition vs NCO + RationalDecimator {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("M,D", [(250, 125), (640, 320), (1024, 256), (4096, 2048)])
def test_polyphase_form_equals_definition(M, D):
    rng = np.random.default_rng(M)
    n = 10 * M + 77
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    ks = np.unique(np.concatenate(([0, 1, M // 2 - 1, M // 2, M // 2 + 1, M - 1], rng.integers(0, M, 6))))
    for h in (channelizer_taps(M), co.odd_taps(M)):
        ref = co.Definition(h, M, D, ks).process(x)
        m0, m1 = co.frame_range(0, n, D)
        got = co.polyphase(x, h, M, D, m0, m1, ks)
        e = _rel(got, ref)
        print(f"M {M} D {D} L {len(h)}: polyphase vs definition {e:.2e}")
        assert e <= 1e-12


@pytest.mark.parametrize("M,D", co.SHAPES)
def test_float32_mirror_is_well_conditioned(M, D):
    """the kernel's arithmetic, on exactly the signals the GPU tests use, within 1e-6 of the call's peak of the master"""
    for name, x in (("tones", co.signal(M)), ("noise", co.noise(M))):
        for h in (channelizer_taps(M), co.odd_taps(M)):
            m0, m1 = co.frame_range(0, len(x), D)
            ref = co.polyphase(x, h, M, D, m0, m1)
            got = co.mirror32(x, h, M, D, m0, m1, rad=chz.plan(M, D, len(h))["radices"])
            e = _rel(got, ref)
            print(f"M {M} D {D} L {len(h)} {name}: float32 mirror vs float64 master {e:.2e} of the call's peak")
            assert e <= 1e-6


@pytest.mark.parametrize("M", [64, 250, 640, 4096])
def test_default_taps(M):
    h = channelizer_taps(M)
    assert len(h) == 8 * M
    assert abs(np.sum(h) - 1.0) <= 1e-9
    i = np.arange(len(h))

    def H(f):                                                 # f in units of fs
        return np.abs(np.exp(-2j * np.pi * np.outer(np.atleast_1d(f), i)) @ h)

    half = 20 * np.log10(H(0.5 / M)[0])
    assert abs(half + 6.02) <= 0.05, half
    f = np.linspace(1.0 / M, 0.5, 1500)
    stop = 20 * np.log10(np.max(H(f)))
    print(f"M {M}: {half:.3f} dB at half a spacing, {stop:.1f} dB at worst from one spacing on")
    assert stop <= -80.0


def _plan(M, D, ntaps, k_first=0, nk=None):
    out = (C.c_int32 * 16)()
    rc = _lib.lib().pysdr_chan_plan(M, D, ntaps, k_first, M if nk is None else nk, out)
    return rc, list(out)


def test_plan_accepts_what_the_spec_allows(hiplib):
    shapes = [a * b for a in (1 << i for i in range(13)) for b in (5 ** i for i in range(6)) if 16 <= a * b <= 4096]
    assert 16 in shapes and 4096 in shapes and 3125 in shapes and 640 in shapes and len(shapes) == len(set(shapes))
    for M in shapes:
        for c in (1, 2, 4):
            if M % c:
                continue
            rc, p = _plan(M, M // c, 8 * M)
            assert rc == 0, (M, c)
            assert int(np.prod(p[1:1 + p[0]])) == M and set(p[1:1 + p[0]]) <= {2, 4, 5}
            assert 0 < p[12] <= 163840 and p[9] % p[10] == 0 and p[11] in (256, 1024)
            assert p[13] == 8 * M - 1 and p[14] == 8
            assert _plan(M, M // c, 16 * M)[0] == 0 and _plan(M, M // c, 1)[1][13] == M - 1


def test_plan_rejects_everything_else(hiplib):
    E = -1
    for M in (48, 8192, 12):
        assert _plan(M, M // 2, 8 * M)[0] == E
    assert _plan(64, 24, 512)[0] == E                         # D does not divide M
    assert _plan(64, 8, 512)[0] == E                          # M / D = 8
    assert _plan(64, 0, 512)[0] == E
    assert _plan(64, 32, 0)[0] == E and _plan(64, 32, 16 * 64 + 1)[0] == E
    assert _plan(64, 32, 512, 0, 0)[0] == E and _plan(64, 32, 512, 0, 65)[0] == E
    assert _plan(64, 32, 512, 64, 1)[0] == E and _plan(64, 32, 512, -1, 1)[0] == E
    assert _lib.lib().pysdr_chan_plan(64, 32, 512, 0, 64, None) == E
    with pytest.raises(_lib.PysdrError):
        chz.plan(48, 24, 384)


def test_null_handles_are_argument_errors(hiplib):
    L = _lib.lib()
    n = C.c_int(0)
    assert L.pysdr_chan_reset(None) == -1 and L.pysdr_chan_sync(None) == -1
    assert L.pysdr_chan_set_taps(None, None, 1) == -1
    assert L.pysdr_chan_process(None, None, 0, 0, None, 0, 0, C.byref(n)) == -1
    assert L.pysdr_chan_create(0, 48, 24, 0, 48, 384, 1024, C.byref(C.c_void_p())) == -1
    L.pysdr_chan_destroy(None)
