"""The polyphase channelizer on the GPU (pysdr_amd/csrc/chan.hip): every sample of every stored
channel against the float64 master, the frequency axis, bit-exact independence of cuts / channel range / buffer
placement, tap changes, reset, non-finite input and the error paths."""
import ctypes as C

import numpy as np
import pytest

from tests import channelizer_oracle as co

pytestmark = pytest.mark.gpu

FS = 8e6
BAR = 1e-5          # the project's parity bar, per call: of the call's peak over all channels


def bits(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


def run(ch, x, cuts=None):
    cuts = [len(x)] if cuts is None else cuts
    out, i = [], 0
    for c in cuts:
        out.append(ch.push(x[i:i + c]))
        i += c
    assert i == len(x)
    return np.concatenate(out, axis=1)


@pytest.mark.parametrize("M,D", co.SHAPES)
def test_parity_with_the_float64_master(M, D):
    from pysdr_amd.channelizer import Channelizer
    from pysdr_amd.design import channelizer_taps
    for h in (channelizer_taps(M), co.odd_taps(M)):
        ch = Channelizer(FS, M, D, h)
        for name, x in (("tones", co.signal(M)), ("noise", co.noise(M))):
            ch.reset()
            y = ch.push(x)
            m0, m1 = co.frame_range(0, len(x), D)
            ref = co.polyphase(x, h, M, D, m0, m1)
            assert y.shape == ref.shape == (M, m1 - m0) and y.dtype == np.complex64
            err = np.abs(y - ref)
            e_call = float(err.max() / np.abs(ref).max())
            e_own = float(np.max(err.max(axis=1) / np.abs(ref).max(axis=1)))
            print(f"M {M} D {D} L {len(h)} {name}: {e_call:.2e} of the call's peak, {e_own:.2e} of a channel's own peak")
            assert e_call <= BAR
            if name == "noise":
                assert e_own <= BAR
        ch.close()


@pytest.mark.parametrize("k,off", [(5, 0.2), (-7, -0.3), (31, 0.45), (-32, 0.1)])
def test_frequency_axis(k, off):
    """a pure tone lands in the row whose .freqs is nearest, with the prototype's gain there; rows two or more spacings
    away are at least 80 dB down"""
    from pysdr_amd.channelizer import Channelizer
    M, D = 64, 32
    ch = Channelizer(FS, M, D)
    f = (k + off) * FS / M
    n = np.arange(40 * M)
    x = np.exp(2j * np.pi * (f / FS) * n).astype(np.complex64)
    y = ch.push(x)[:, 8 * M // D:]                              # past the prototype's run-in
    level = np.abs(y).max(axis=1)
    row = int(np.argmin(np.abs(((ch.freqs - f) + FS / 2) % FS - FS / 2)))
    assert int(np.argmax(level)) == row
    delta = (f - ch.freqs[row]) / FS
    gain = abs(np.sum(ch.h * np.exp(-2j * np.pi * delta * np.arange(len(ch.h)))))
    assert abs(delta) <= 0.5 / M + 1e-12
    assert np.max(np.abs(np.abs(y[row]) - gain)) <= 1e-4, (np.abs(y[row]).min(), np.abs(y[row]).max(), gain)
    dist = np.abs(((ch.freqs - f) + FS / 2) % FS - FS / 2) / (FS / M)
    far = level[dist >= 2.0]
    assert len(far) >= M - 4 and 20 * np.log10(far.max()) <= -80.0, 20 * np.log10(far.max())
    assert ch.fs_out == FS / D and ch.freqs.min() == -FS / 2 and ch.freqs.max() == FS / 2 - FS / M
    ch.close()


@pytest.mark.parametrize("M,D", [(64, 16), (64, 64), (250, 125), (640, 320), (800, 400), (1024, 256), (4096, 2048)])
def test_any_cut_gives_the_same_bits(M, D):
    from pysdr_amd.channelizer import Channelizer
    x = co.signal(M, seed=1)
    h = co.odd_taps(M)
    ch = Channelizer(FS, M, D, h)
    one = run(ch, x)
    ch.reset()
    fixed = [1000] * (len(x) // 1000) + [len(x) % 1000]
    assert np.array_equal(bits(run(ch, x, fixed)), bits(one))
    for seed in (1, 2):
        cuts = co.random_cuts(len(x), D, seed)
        assert 0 in cuts and 1 in cuts and any(c % 2 for c in cuts) and (D <= 2 or any(0 < c < D for c in cuts))
        ch.reset()
        assert np.array_equal(bits(run(ch, x, cuts)), bits(one))
    ch.close()


@pytest.mark.parametrize("M,D", [(64, 32), (640, 320)])
def test_a_circular_channel_range_is_the_same_rows(M, D):
    from pysdr_amd.channelizer import Channelizer
    x = co.signal(M, seed=2)
    full = Channelizer(FS, M, D)
    y = full.push(x)
    part = Channelizer(FS, M, D, channels=(M - 3, 7))
    rows = (M - 3 + np.arange(7)) % M
    assert np.array_equal(part.freqs, full.freqs[rows])
    assert np.array_equal(bits(part.push(x)), bits(y[rows]))
    full.close()
    part.close()


def test_device_pointers_equal_the_host_path():
    from pysdr_amd import _lib
    from pysdr_amd.channelizer import Channelizer
    M, D = 256, 128
    x = co.signal(M, seed=3)
    ch = Channelizer(FS, M, D)
    want = ch.push(x)
    L = _lib.lib()
    d_x, d_y = C.c_void_p(), C.c_void_p()
    pitch = want.shape[1] + 9
    _lib.check(L.pysdr_dev_alloc(0, x.nbytes, C.byref(d_x)), "alloc")
    _lib.check(L.pysdr_dev_alloc(0, M * pitch * 8, C.byref(d_y)), "alloc")
    _lib.check(L.pysdr_dev_upload(0, d_x, C.c_void_p(x.ctypes.data), x.nbytes), "upload")
    ch.reset()
    half = 5431                                                 # odd, not a multiple of D, inside the signal
    assert 0 < half < len(x)
    n1 = ch.push_device(d_x.value, half, d_y.value, pitch)
    n2 = ch.push_device(d_x.value + 8 * half, len(x) - half, d_y.value + 8 * n1, pitch)
    assert n1 + n2 == want.shape[1]
    got = np.empty((M, pitch), np.complex64)
    _lib.check(L.pysdr_dev_download(0, C.c_void_p(got.ctypes.data), d_y, got.nbytes), "download")
    assert np.array_equal(bits(got[:, :n1 + n2]), bits(want))
    L.pysdr_dev_free(0, d_x)
    L.pysdr_dev_free(0, d_y)
    ch.close()


def test_set_taps_and_reset():
    from pysdr_amd.channelizer import Channelizer
    from pysdr_amd.design import channelizer_taps
    M, D = 64, 32
    x = co.signal(M, seed=4)
    h1, h2 = channelizer_taps(M), co.odd_taps(M) * 0.5
    cut = 2501
    ch = Channelizer(FS, M, D, h1)
    d = co.Definition(h1, M, D)
    a1, r1 = ch.push(x[:cut]), d.process(x[:cut])
    ch.set_taps(h2)
    d.set_taps(h2)
    a2, r2 = ch.push(x[cut:]), d.process(x[cut:])
    peak = max(np.abs(r1).max(), np.abs(r2).max())
    assert a1.shape == r1.shape and a2.shape == r2.shape
    assert np.abs(a1 - r1).max() <= BAR * peak and np.abs(a2 - r2).max() <= BAR * peak
    # the new taps hold for the whole window of the call's outputs: not what the old ones give
    assert np.abs(a2[:, :4] - co.Definition(h1, M, D).process(x)[:, r1.shape[1]:r1.shape[1] + 4]).max() > 100 * BAR * peak
    ch.reset()
    ch.set_taps(h1)
    again = ch.push(x[:cut])
    assert np.array_equal(bits(again), bits(a1))                # reset(): m = 0 again, empty history
    ch.close()


@pytest.mark.parametrize("M,D,where", [(64, 16, 3000), (250, 125, 4001), (4096, 2048, 60000)])
def test_one_nan_marks_exactly_its_frames(M, D, where):
    from pysdr_amd.channelizer import Channelizer
    h = co.odd_taps(M)
    P = -(-len(h) // M)
    x = co.signal(M, seed=5)
    ch = Channelizer(FS, M, D, h)
    clean = ch.push(x)
    bad = x.copy()
    bad[where] = complex(np.nan, 0.25)
    ch.reset()
    y = ch.push(bad)
    m = np.arange(clean.shape[1])
    hit = (m * D >= where) & (m * D - P * M < where)            # the padded window (mD - ceil(L/M) M, mD] holds it
    assert hit.sum() == P * M // D
    assert not np.isfinite(y[:, hit]).any()
    assert np.array_equal(bits(y[:, ~hit]), bits(clean[:, ~hit]))
    ch.close()


def test_errors_leave_the_object_usable():
    from pysdr_amd import _lib
    from pysdr_amd.channelizer import Channelizer
    M, D = 64, 32
    ch = Channelizer(FS, M, D, max_in=4096)
    x = co.signal(M, seed=6)[:4096]
    want = ch.push(x)
    ch.reset()
    L = _lib.lib()
    n_out = C.c_int(-1)
    y = np.zeros((M, 128), np.complex64)
    px, py = C.c_void_p(x.ctypes.data), C.c_void_p(y.ctypes.data)
    assert L.pysdr_chan_process(ch._h, px, 4097, 0, py, 129, 0, C.byref(n_out)) == -5       # n > max_in
    assert L.pysdr_chan_process(ch._h, px, 4096, 0, py, 127, 0, C.byref(n_out)) == -5       # pitch < 128 outputs
    assert b"pitch" in L.pysdr_last_error()
    assert L.pysdr_chan_process(ch._h, px, -1, 0, py, 128, 0, C.byref(n_out)) == -1
    assert L.pysdr_chan_process(ch._h, None, 16, 0, py, 128, 0, C.byref(n_out)) == -1
    assert L.pysdr_chan_process(ch._h, px, 4096, 0, None, 128, 0, C.byref(n_out)) == -1
    assert L.pysdr_chan_process(ch._h, px, 4096, 0, py, 128, 0, None) == -1
    assert L.pysdr_chan_set_taps(ch._h, _lib.as_pd(ch.h), 0) == -1
    assert L.pysdr_chan_set_taps(ch._h, _lib.as_pd(ch.h), ch.max_taps + 1) == -1
    h = C.c_void_p()
    assert L.pysdr_chan_create(0, 64, 32, 0, 64, 512, 0, C.byref(h)) == -1 and not h.value
    assert L.pysdr_chan_create(0, 64, 32, 0, 65, 512, 1024, C.byref(h)) == -1 and not h.value
    assert n_out.value == 0
    assert np.array_equal(bits(ch.push(x)), bits(want))         # nothing above advanced the stream
    ch.close()
    with pytest.raises(_lib.PysdrError):
        Channelizer(FS, 48, 24)
