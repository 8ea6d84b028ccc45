"""The columns pass of the 64k PSD as a loop over frames (psdfft.hip psd_cols_pk_kernel; host_plan.h plan_psd_cols): a
workgroup keeps its column block, walks over the frames g, g + G, ... of the launch and loads the next frame's samples
while it transforms one.  The arithmetic of a frame is the unit kernel's, so EVERY frame must be bit for bit what
PYSDR_PSD_PATH=unit (one unit per workgroup, the form of every earlier round) gives: at every relation of the frame count
to the grid, at hops that move the frame starts, on the default path, and around frames whose block scale is degenerate.
At most 16 frames per call; frames differ by a scale of their own, so that a frame taken from the wrong index shows."""
import ctypes as C

import numpy as np
import pytest

from oracle import sdr_oracle as so
from tests.test_gpu_parity import psd_check

pytestmark = pytest.mark.gpu

CH, NF = 32768, 65536
PATH_VARS = ("PYSDR_PSD_PATH", "PYSDR_PSD_GROUP", "PYSDR_PSD_STREAMS", "PYSDR_PSD_PACKED", "PYSDR_PSD_ROCFFT")


@pytest.fixture(scope="module")
def base():
    """16 distinct frames' worth of the C3 signal with room for the widest hop, computed once and left unchanged"""
    x = so.synth_iq(so.CONFIGS['C3'], 6 * 40000 + CH + 16 * CH, 41)
    x.setflags(write=False)
    return x


def scaled_frames(base, nframes, seed):
    rng = np.random.default_rng(seed)
    scale = (0.25 + 0.75 * rng.random(nframes)).astype(np.float32)
    return (base[:nframes * CH].reshape(nframes, CH) * scale[:, None]).astype(np.complex64).reshape(-1)


def run_psd(monkeypatch, x, nframes, hop, path, calls=1):
    """-> [PSD of the call, (nframes, NF)] per call on ONE spectrum object created under PYSDR_PSD_PATH=path (None: nothing set)"""
    from pysdr_amd import _lib, design
    for k in PATH_VARS + ("PYSDR_TUNING",):
        monkeypatch.delenv(k, raising=False)
    if path is not None:
        monkeypatch.setenv("PYSDR_TUNING", "1")
        monkeypatch.setenv("PYSDR_PSD_PATH", path)
    assert x.dtype == np.complex64 and x.size >= (nframes - 1) * hop + CH
    lib = _lib.lib()
    d_x, d_o, sp = C.c_void_p(), C.c_void_p(), C.c_void_p()
    win = np.ascontiguousarray(design.psd_window(CH), np.float32)
    outs = []
    try:
        _lib.check(lib.pysdr_dev_alloc(0, x.nbytes, C.byref(d_x)), "alloc")
        _lib.check(lib.pysdr_dev_alloc(0, nframes * NF * 4, C.byref(d_o)), "alloc")
        _lib.check(lib.pysdr_dev_upload(0, d_x, C.c_void_p(x.ctypes.data), x.nbytes), "upload")
        _lib.check(lib.pysdr_spectrum_create(0, CH, NF, 16, _lib.as_pf(win), C.byref(sp)), "create")
        for _ in range(calls):
            _lib.check(lib.pysdr_spectrum_batch(sp, d_x, nframes, hop, d_o), "batch")
            _lib.check(lib.pysdr_spectrum_sync(sp), "sync")
            got = np.empty(nframes * NF, np.float32)
            _lib.check(lib.pysdr_dev_download(0, C.c_void_p(got.ctypes.data), d_o, got.nbytes), "dl")
            outs.append(got.reshape(nframes, NF))
    finally:
        if sp:
            lib.pysdr_spectrum_destroy(sp)
        for d in (d_x, d_o):
            if d:
                lib.pysdr_dev_free(0, d)
    return outs


def assert_frames_equal(got, want, what):
    assert got.shape == want.shape
    bad = [f for f in range(got.shape[0]) if not np.array_equal(got[f], want[f])]
    assert not bad, f"{what}: frames {bad} of {got.shape[0]} differ from the unit form"


def oracle_frame(x):
    return so.Spectrum(8000.0, CH, NF, 0.0, np.float64).periodogram(np.ascontiguousarray(x), True)


@pytest.mark.parametrize("nframes", [1, 2, 3, 4, 7, 10])
def test_every_frame_count_against_a_grid_of_three_rows(nframes, base, monkeypatch):
    """loop:3 = three workgroups per column block: fewer frames than workgroups (1, 2), exactly one round (3), a round
    plus one (4), uneven tails (7 = 3 + 2 + 2, 10 = 4 + 3 + 3)"""
    x = scaled_frames(base, nframes, 100 + nframes)
    unit, = run_psd(monkeypatch, x, nframes, CH, "unit")
    loop, = run_psd(monkeypatch, x, nframes, CH, "loop:3")
    assert_frames_equal(loop, unit, f"loop:3, {nframes} frames")
    for f in sorted({0, nframes - 1}):
        psd_check(loop[f], oracle_frame(x[f * CH:(f + 1) * CH]))
    if nframes == 1:                                       # (two frames against the oracle in every case)
        psd_check(unit[0], oracle_frame(x[:CH]))


@pytest.mark.parametrize("hop", [22937, 40000])
def test_frames_that_overlap_at_an_odd_hop_or_leave_gaps(hop, base, monkeypatch):
    """an odd hop (frame starts only 8-byte aligned) and a hop with gaps, 7 frames on three rows: a prefetch addressed from
    the wrong frame, or by the frame length instead of the hop, shows here"""
    nframes = 7
    x = np.ascontiguousarray(base[:(nframes - 1) * hop + CH])
    unit, = run_psd(monkeypatch, x, nframes, hop, "unit")
    loop, = run_psd(monkeypatch, x, nframes, hop, "loop:3")
    assert_frames_equal(loop, unit, f"hop {hop}")
    for f in (1, nframes - 1):
        psd_check(loop[f], oracle_frame(x[f * hop:f * hop + CH]))


def test_the_default_path_equals_the_unit_form_and_itself(base, monkeypatch):
    """nothing set: 16 frames, bit for bit the unit form's, and a second call on the same object repeats the first"""
    x = scaled_frames(base, 16, 7)
    unit, = run_psd(monkeypatch, x, 16, CH, "unit")
    first, second = run_psd(monkeypatch, x, 16, CH, None, calls=2)
    assert_frames_equal(first, unit, "default path")
    assert np.array_equal(first, second)
    for f in (0, 15):
        psd_check(first[f], oracle_frame(x[f * CH:(f + 1) * CH]))


def test_degenerate_frames_between_ordinary_ones(base, monkeypatch):
    """An impulse, a frame whose second half is silent and an all-zero frame (kinds of
    test_psd_24_bit_intermediate_on_hard_inputs) between ordinary frames of one 7-frame call on three rows: the block
    scale and the `live` test are per frame, so a value carried over from the workgroup's previous iteration (frames 0 and
    3 precede the zero frame 6 in workgroup 0, frame 1 the impulse 4 in workgroup 1) would show on them."""
    nframes = 7
    x = scaled_frames(base, nframes, 5).reshape(nframes, CH).copy()
    imp = np.zeros(CH, np.complex64); imp[12345] = 1.0 + 0.5j
    x[4] = imp
    x[2, CH // 2:] = 0
    x[6] = 0
    x = x.reshape(-1)
    unit, = run_psd(monkeypatch, x, nframes, CH, "unit")
    loop, = run_psd(monkeypatch, x, nframes, CH, "loop:3")
    assert_frames_equal(loop, unit, "hard frames")
    for f in (2, 4, 5):
        psd_check(loop[f], oracle_frame(x[f * CH:(f + 1) * CH]))
    po = oracle_frame(x[6 * CH:7 * CH])                    # the zero frame: the oracle's -300 dB on every bin
    assert np.all(np.isfinite(loop[6])) and np.max(np.abs(loop[6] - po)) <= 1e-3, (loop[6].min(), loop[6].max())
