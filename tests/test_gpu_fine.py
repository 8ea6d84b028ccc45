"""The fine channelizer on the GPU (pysdr_amd/csrc/fine.hip, api_fine.hip): every sample of every fine
row against the float64 cascade (tests/fine_oracle.py) call by call, bit-exact independence of cuts / channel range /
buffer placement, the frequency axis, tap changes, reset, non-finite input and the error paths."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import channelizer_oracle as cz
from tests import fine_oracle as fo

pytestmark = pytest.mark.gpu

FS = 8e6
BAR = 1e-5          # the project's parity bar, per call, of the scale fine_oracle.scale_of defines
# (M1, D1, M2, D2, g_first, ng)
SHAPES = [(16, 8, 16, 8, 0, 128),                       # all rows: the first coarse row serves both ends of the raster
          (64, 16, 32, 32, 64 * 8 - 13, 37),            # C1 = 4, C2 = 1, across the wrap, partial coarse rows at both ends
          (256, 128, 20, 5, 705, 3),                    # radix 5, C2 = 4, three rows inside one coarse row
          (640, 320, 256, 128, 7000, 300),              # 32 frames per workgroup
          (4096, 2048, 64, 16, 131072 - 500, 1000)]     # 33 coarse rows of the largest first stage, across the wrap
IDS = ["16-8-16-8", "64-16-32-32", "256-128-20-5", "640-320-256-128", "4096-2048-64-16"]


def bits(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


def taps(M1, D1, M2):
    from pysdr_amd import fine
    from pysdr_amd.design import channelizer_taps
    return fine.prototype1(FS, M1, D1, M2), channelizer_taps(M2)


def make(i, channels="shape", max_in=None, **kw):
    from pysdr_amd.fine import FineChannelizer
    M1, D1, M2, D2, g, ng = SHAPES[i]
    ch = (g, ng) if channels == "shape" else channels
    return FineChannelizer(FS, M1, M2, D1, D2, channels=ch, max_in=len(base(i)["x"]) if max_in is None else max_in, **kw)


def run(ch, x, cuts=None):
    cuts = [len(x)] if cuts is None else cuts
    out, i = [], 0
    for c in cuts:
        out.append(ch.push(x[i:i + c]))
        i += c
    assert i == len(x)
    return np.concatenate(out, axis=1)


@functools.lru_cache(maxsize=None)
def base(i):
    """shape i: the shared input and the float64 cascade's answer to the whole stream; computed once, never changed"""
    M1, D1, M2, D2, g, ng = SHAPES[i]
    h1, h2 = taps(M1, D1, M2)
    x = fo.signal(M1, D1, M2, D2, g, ng, h1, h2)
    m1 = -(-len(x) // (D1 * D2))
    want, y1 = fo.cascade64(x, h1, h2, M1, D1, M2, D2, g, ng, 0, m1)
    for v in (x, want, y1):
        v.setflags(write=False)
    return dict(x=x, want=want, y1=y1, h1=h1, h2=h2, D=D1 * D2, frames=m1)


@functools.lru_cache(maxsize=None)
def whole(i):
    """the device's answer to the whole stream in one call"""
    ch = make(i)
    y = ch.push(base(i)["x"])
    ch.close()
    y.setflags(write=False)
    return y


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_parity_with_the_float64_cascade_per_call(i):
    """the bar: the project's 1e-5, or four times what the float32 model of the kernels (fine_oracle.model32) measures
    against the same cascade on the same input, whichever is larger"""
    M1, D1, M2, D2, g, ng = SHAPES[i]
    b = base(i)
    x, want, D = b["x"], b["want"], b["D"]
    model = fo.model32(x, b["h1"], b["h2"], M1, D1, M2, D2, g, ng, 0, b["frames"])
    e_model = float(np.abs(model - want).max() / fo.scale_of(want, b["y1"], b["h2"], D2, 0, b["frames"]))
    bar = max(BAR, 4 * e_model)
    ch = make(i)
    assert (ch.M, ch.D, ch.nk, ch.Q) == (M1 * (M2 * D1 // M1), D, ng, M2 * D1 // M1) and ch.fs_out == FS / D
    assert ch.run_in_taps == fo.run_in_taps(b["h1"], b["h2"], D1) == len(x) - 40 * D - 1003
    third = len(x) // 3 + 1
    at, worst = 0, 0.0
    for n in (third, third, len(x) - 2 * third):
        m0, m1 = cz.frame_range(at, at + n, D)
        y = ch.push(x[at:at + n])
        at += n
        assert y.shape == (ng, m1 - m0) and y.dtype == np.complex64
        e = float(np.abs(y - want[:, m0:m1]).max() / fo.scale_of(want[:, m0:m1], b["y1"], b["h2"], D2, m0, m1))
        worst = max(worst, e)
        assert e <= bar, (m0, m1, e, bar)
    print(f"{IDS[i]}: device {worst:.2e}, float32 model {e_model:.2e} of the scale; bar {bar:.1e}")
    ch.close()


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_any_cut_gives_the_same_bits(i):
    """random cuts (0, 1, fewer than D samples, odd lengths), a call that completes a stage-1 output but no fine output,
    and first calls that complete one frame fewer than, exactly, and one frame more than a workgroup's tile"""
    M1, D1, M2, D2, g, ng = SHAPES[i]
    b = base(i)
    x, D = b["x"], b["D"]
    one = whole(i)
    ch = make(i)
    for seed in (1, 2):
        head = [1, D1]                                        # sample 0 completes frame 0 of both stages; D1 more: stage 1 alone
        cuts = head + cz.random_cuts(len(x) - sum(head), D, seed)
        ch.reset()
        assert ch.n_out_for(1) == 1
        ch.push(x[:1])
        assert ch.n_out_for(D1) == 0 and D2 > 1
        ch.reset()
        assert np.array_equal(bits(run(ch, x, cuts)), bits(one)), seed
    tile = ch.frames_per_wg
    ks = [k for t in (tile, tile // 2) for k in (t - 1, t, t + 1) if 1 <= k < b["frames"]]
    assert len(ks) >= 3
    for k in ks:
        first = (k - 1) * D + 1                               # ends with the sample that completes frame k - 1
        ch.reset()
        assert ch.n_out_for(first) == k
        assert np.array_equal(bits(run(ch, x, [first, D - 1, 1, len(x) - first - D])), bits(one)), k
    ch.close()


@pytest.mark.parametrize("G", [5 * 16 + 3, 7 * 16 + 8, 1024 - 2 * 16 - 8, 1024 - 1], ids=["inside", "seam", "negative-seam", "last"])
def test_frequency_axis(G):
    """a tone at freqs[a] peaks on row a with the cascade's gain 1 there -- inside a coarse row, on the seam between two, at
    a negative frequency"""
    from pysdr_amd.fine import FineChannelizer
    M1, D1, M2, D2 = 64, 32, 32, 16
    ch = FineChannelizer(FS, M1, M2, D1, D2, max_in=1 << 16)
    assert ch.M == 1024 and ch.nk == 1024 and ch.freqs.min() == -FS / 2 and ch.freqs.max() == FS / 2 - FS / 1024
    a = G
    assert ch.freqs[a] == (G - 1024 if G >= 512 else G) * FS / 1024
    n = np.arange(ch.run_in_taps + 12 * ch.D)
    x = (0.5 * np.exp(2j * np.pi * (ch.freqs[a] / FS) * n)).astype(np.complex64)
    y = ch.push(x)[:, -(-ch.run_in_taps // ch.D):]
    level = np.abs(y).max(axis=1)
    assert int(np.argmax(level)) == a
    assert np.abs(np.abs(y[a]) - 0.5).max() <= 1e-4 + BAR, (np.abs(y[a]).min(), np.abs(y[a]).max())
    others = np.delete(level, a)
    assert 20 * np.log10(others.max() / 0.5) <= -80.0, 20 * np.log10(others.max() / 0.5)
    ch.close()


@pytest.mark.parametrize("i,g,ng", [(0, 120, 13), (0, 3, 128), (1, 2, 9)], ids=["wrap", "all-from-3", "inside"])
def test_a_circular_range_is_the_same_rows_of_the_full_object(i, g, ng):
    M1, D1, M2, D2 = SHAPES[i][:4]
    x = base(i)["x"]
    full = make(i, channels=None)
    y = full.push(x)
    part = make(i, channels=(g, ng))
    rows = (g + np.arange(ng)) % full.M
    assert full.nk == full.M and np.array_equal(part.freqs, full.freqs[rows])
    assert np.array_equal(bits(part.push(x)), bits(y[rows]))
    full.close()
    part.close()


def test_device_pointers_equal_the_host_path():
    from pysdr_amd import _lib
    i = 2
    x = np.array(base(i)["x"])
    want = whole(i)
    ng = want.shape[0]
    ch = make(i)
    L = _lib.lib()
    d_x, d_y = C.c_void_p(), C.c_void_p()
    pitch = want.shape[1] + 9
    _lib.check(L.pysdr_dev_alloc(0, x.nbytes, C.byref(d_x)), "alloc")
    _lib.check(L.pysdr_dev_alloc(0, ng * pitch * 8, C.byref(d_y)), "alloc")
    _lib.check(L.pysdr_dev_upload(0, d_x, C.c_void_p(x.ctypes.data), x.nbytes), "upload")
    half = 25431                                                # odd, not a multiple of D, inside the signal
    assert 0 < half < len(x)
    n1 = ch.push_device(d_x.value, half, d_y.value, pitch)
    n2 = ch.push_device(d_x.value + 8 * half, len(x) - half, d_y.value + 8 * n1, pitch, sync=False)
    ch.sync()
    assert n1 + n2 == want.shape[1] and ch.n_in == len(x)
    got = np.empty((ng, pitch), np.complex64)
    _lib.check(L.pysdr_dev_download(0, C.c_void_p(got.ctypes.data), d_y, got.nbytes), "download")
    assert np.array_equal(bits(got[:, :n1 + n2]), bits(want))
    L.pysdr_dev_free(0, d_x)
    L.pysdr_dev_free(0, d_y)
    ch.close()


def test_set_taps_and_reset():
    from pysdr_amd import _lib
    from pysdr_amd.channelizer import Channelizer
    i = 1
    M1, D1, M2, D2, g, ng = SHAPES[i]
    b = base(i)
    x, h1, h2 = b["x"], b["h1"], b["h2"]
    k1, k2 = cz.odd_taps(M1) * 0.5, cz.odd_taps(M2)
    cut = 12501
    ch = make(i)
    ref = fo.Cascade(h1, h2, M1, D1, M2, D2, g, ng)
    a1, r1 = ch.push(x[:cut]), ref.process(x[:cut])
    ch.set_taps(k1, k2)
    ref.set_taps(k1, k2)
    a2, r2 = ch.push(x[cut:]), ref.process(x[cut:])
    # the scale: stage 1's rows hold the out-of-range tone at full strength
    scale = max(np.abs(r1).max(), np.abs(r2).max(), np.abs(ref.y1).max())
    assert a1.shape == r1.shape and a2.shape == r2.shape
    assert np.abs(a1 - r1).max() <= BAR * scale and np.abs(a2 - r2).max() <= BAR * scale
    assert np.abs(a2[:, :2] - b["want"][:, r1.shape[1]:r1.shape[1] + 2]).max() > 100 * BAR * scale   # not what the old taps give
    ch.reset()
    ch.set_taps(h1, h2)
    assert np.array_equal(bits(ch.push(x[:cut])), bits(a1))      # reset(): m = 0 again, empty history in both stages
    # each kind of handle refuses the other's set_taps and stays usable
    L = _lib.lib()
    assert L.pysdr_chan_set_taps(ch._h, _lib.as_pd(h2), len(h2)) == -5 and b"fine" in L.pysdr_last_error()
    plain = Channelizer(FS, 64, 32, max_in=4096)
    assert L.pysdr_chan_fine_set_taps(plain._h, _lib.as_pd(h1), len(h1), _lib.as_pd(h2), len(h2)) == -5
    assert np.array_equal(bits(ch.push(x[cut:])), bits(whole(i)[:, a1.shape[1]:]))
    plain.close()
    ch.close()


@pytest.mark.parametrize("i,where", [(1, 9000), (2, 30001), (4, 1500000)], ids=[IDS[1], IDS[2], IDS[4]])
def test_one_nan_and_one_inf_mark_exactly_their_frames(i, where):
    """non-finite: exactly the fine frames whose stage-2 window holds a stage-1 frame whose window holds the sample, all
    kept channels of them; every other output keeps its bits"""
    M1, D1, M2, D2, g, ng = SHAPES[i]
    b = base(i)
    clean = whole(i)
    L1, L2 = len(b["h1"]), len(b["h2"])
    assert L1 % M1 == 0 and L2 % M2 == 0                         # no padded taps: the windows are the prototypes' own
    bad = np.array(b["x"])
    spots = (where, where + 3 * b["D"] + 1)
    bad[spots[0]] = complex(np.nan, 0.25)
    bad[spots[1]] = complex(-0.5, np.inf)
    m1 = np.arange(-(-len(bad) // D1))
    hit1 = np.zeros(len(m1), bool)
    for w in spots:
        hit1 |= (m1 * D1 >= w) & (m1 * D1 - L1 < w)
    m = np.arange(clean.shape[1])
    c = np.concatenate(([0], np.cumsum(hit1)))                   # hit stage-1 frames in [lo, hi]: c[hi + 1] - c[lo]
    lo, hi = np.maximum(m * D2 - (L2 - 1), 0), m * D2
    hit = c[hi + 1] - c[lo] > 0
    assert 0 < hit.sum() < len(m)
    ch = make(i)
    y = ch.push(bad)
    assert not np.isfinite(y[:, hit]).any()
    assert np.array_equal(bits(y[:, ~hit]), bits(clean[:, ~hit]))
    ch.close()


def test_errors_leave_the_object_usable():
    from pysdr_amd import _lib
    from pysdr_amd.fine import FineChannelizer
    M1, D1, M2, D2 = 64, 32, 32, 16
    D = D1 * D2
    ch = FineChannelizer(FS, M1, M2, D1, D2, channels=(100, 20), max_in=8192)
    x = fo.signal(M1, D1, M2, D2, 100, 20, ch.h1, ch.h2, seed=6)[:8192]
    ch.push(x[:1000])
    want = ch.push(x[1000:])
    ch.reset()
    ch.push(x[:1000])
    L = _lib.lib()
    n_out = C.c_int(-1)
    y = np.zeros((20, 16), np.complex64)
    px, py = C.c_void_p(x.ctypes.data), C.c_void_p(y.ctypes.data)
    n = 8192 - 1000
    assert ch.n_out_for(n) == 14
    assert L.pysdr_chan_process(ch._h, px, 8193, 0, py, 16, 0, C.byref(n_out)) == -5         # n > max_in
    assert L.pysdr_chan_process(ch._h, px, n, 0, py, 13, 0, C.byref(n_out)) == -5            # pitch < 14 outputs
    assert b"pitch" in L.pysdr_last_error()
    assert L.pysdr_chan_process(ch._h, px, -1, 0, py, 16, 0, C.byref(n_out)) == -1
    assert L.pysdr_chan_process(ch._h, None, 16, 0, py, 16, 0, C.byref(n_out)) == -1
    assert L.pysdr_chan_process(ch._h, px, n, 0, None, 16, 0, C.byref(n_out)) == -1
    assert L.pysdr_chan_process(ch._h, px, n, 0, py, 16, 0, None) == -1
    pd = _lib.as_pd
    assert L.pysdr_chan_fine_set_taps(ch._h, pd(ch.h1), 0, pd(ch.h2), len(ch.h2)) == -1
    assert L.pysdr_chan_fine_set_taps(ch._h, pd(ch.h1), len(ch.h1), pd(ch.h2), ch.max_taps2 + 1) == -1
    assert L.pysdr_chan_fine_set_taps(ch._h, pd(ch.h1), ch.max_taps1 + 1, pd(ch.h2), len(ch.h2)) == -1
    assert L.pysdr_chan_fine_set_taps(ch._h, None, 8, pd(ch.h2), len(ch.h2)) == -1
    h = C.c_void_p()
    assert L.pysdr_chan_fine_create(0, 64, 32, 32, 16, 0, 1025, 512, 256, 1024, C.byref(h)) == -1 and not h.value
    assert L.pysdr_chan_fine_create(0, 64, 32, 48, 24, 0, 8, 512, 256, 1024, C.byref(h)) == -1 and not h.value
    assert n_out.value == 0
    assert np.array_equal(bits(ch.push(x[1000:])), bits(want))  # nothing above advanced the stream or touched the taps
    ch.close()
    with pytest.raises(_lib.PysdrError):
        FineChannelizer(FS, 64, 32, D1=64, D2=16)
