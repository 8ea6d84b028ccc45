"""The rows pass of the 64k PSD as a loop over frames (psdfft.hip psd_rows_pk_kernel; host_plan.h plan_psd_rows): a workgroup
keeps its row block, walks over the frames r, r + R, ... of the launch and loads the next frame's intermediate -- HI and LO
planes through vector loads, the 16 block scales of each wave over the scalar path -- while it transforms one.  The
arithmetic of a frame is the unit kernel's, so EVERY frame must be bit for bit (as uint32) what PYSDR_PSD_PATH=rows=unit
(one unit per workgroup) gives with the SAME columns pass (the default loop): at every relation of the frame count to the
grid, at hops that move the frame starts, on the default plan, around frames whose block scales are degenerate or tiny,
and in linear power as well as in dB.  At most 16 frames per call; frames differ by a scale of their own, so that a frame
(or a frame's scales) taken from the wrong index shows."""
import ctypes as C

import numpy as np
import pytest

from oracle import sdr_oracle as so
from tests.test_gpu_parity import psd_check

pytestmark = pytest.mark.gpu

CH, NF = 32768, 65536
PATH_VARS = ("PYSDR_PSD_PATH", "PYSDR_PSD_GROUP", "PYSDR_PSD_STREAMS", "PYSDR_PSD_PACKED", "PYSDR_PSD_ROCFFT")
UNIT, LOOP3 = "rows=unit", "rows=loop:3"


@pytest.fixture(scope="module")
def base():
    """16 distinct frames' worth of the C3 signal with room for the widest hop, computed once and left unchanged"""
    x = so.synth_iq(so.CONFIGS['C3'], 6 * 40000 + CH + 16 * CH, 43)
    x.setflags(write=False)
    return x


def scaled_frames(base, nframes, seed):
    rng = np.random.default_rng(seed)
    scale = (0.25 + 0.75 * rng.random(nframes)).astype(np.float32)
    return (base[:nframes * CH].reshape(nframes, CH) * scale[:, None]).astype(np.complex64).reshape(-1)


def set_path(monkeypatch, path):
    for k in PATH_VARS + ("PYSDR_TUNING",):
        monkeypatch.delenv(k, raising=False)
    if path is not None:
        monkeypatch.setenv("PYSDR_TUNING", "1")
        monkeypatch.setenv("PYSDR_PSD_PATH", path)


def run_psd(monkeypatch, x, nframes, hop, path, calls=1):
    """-> [PSD of the call in dB, (nframes, NF)] per call on ONE spectrum object created under PYSDR_PSD_PATH=path (None: nothing set)"""
    from pysdr_amd import _lib, design
    set_path(monkeypatch, path)
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


def run_frame(monkeypatch, frame, db, path):
    """-> the PSD of one frame through pysdr_spectrum_frame, the entry point that offers linear power (db = 0)"""
    from pysdr_amd import _lib, design
    set_path(monkeypatch, path)
    lib = _lib.lib()
    sp, nout = C.c_void_p(), C.c_int(0)
    win = np.ascontiguousarray(design.psd_window(CH), np.float32)
    frame = np.ascontiguousarray(frame, np.complex64)
    out = np.empty(NF, np.float32)
    try:
        _lib.check(lib.pysdr_spectrum_create(0, CH, NF, 16, _lib.as_pf(win), C.byref(sp)), "create")
        _lib.check(lib.pysdr_spectrum_frame(sp, _lib.as_pf(frame.view(np.float32)), 1, db, _lib.as_pf(out), C.byref(nout)), "frame")
    finally:
        if sp:
            lib.pysdr_spectrum_destroy(sp)
    assert nout.value == NF
    return out


def assert_frames_equal(got, want, what):
    """bit for bit: the float32 outputs compared as uint32"""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = [f for f in range(got.shape[0]) if not np.array_equal(g[f], w[f])]
    assert not bad, f"{what}: frames {bad} of {got.shape[0]} differ from the unit form"


def oracle_frame(x):
    return so.Spectrum(8000.0, CH, NF, 0.0, np.float64).periodogram(np.ascontiguousarray(x), True)


@pytest.mark.parametrize("nframes", [1, 2, 3, 4, 7, 10])
def test_every_frame_count_against_a_grid_of_three_rows(nframes, base, monkeypatch):
    """rows=loop:3 = three workgroups per row block: fewer frames than workgroups (1, 2), exactly one round (3), a round
    plus one (4), uneven tails (7 = 3 + 2 + 2, 10 = 4 + 3 + 3)"""
    x = scaled_frames(base, nframes, 200 + nframes)
    unit, = run_psd(monkeypatch, x, nframes, CH, UNIT)
    loop, = run_psd(monkeypatch, x, nframes, CH, LOOP3)
    assert_frames_equal(loop, unit, f"{LOOP3}, {nframes} frames")
    for f in sorted({0, nframes - 1}):
        psd_check(loop[f], oracle_frame(x[f * CH:(f + 1) * CH]))
    if nframes == 1:                                       # (two frames against the oracle in every case)
        psd_check(unit[0], oracle_frame(x[:CH]))


@pytest.mark.parametrize("hop", [22937, 32768, 40000])
def test_frames_that_overlap_at_an_odd_hop_abut_or_leave_gaps(hop, base, monkeypatch):
    """7 frames on three rows.  The hop moves what the columns write, not where: a rows prefetch addressed by anything but
    the frame index times the intermediate's pitch shows as another frame's spectrum"""
    nframes = 7
    x = np.ascontiguousarray(base[:(nframes - 1) * hop + CH])
    unit, = run_psd(monkeypatch, x, nframes, hop, UNIT)
    loop, = run_psd(monkeypatch, x, nframes, hop, LOOP3)
    assert_frames_equal(loop, unit, f"hop {hop}")
    for f in (1, nframes - 1):
        psd_check(loop[f], oracle_frame(x[f * hop:f * hop + CH]))


def test_the_default_plan_equals_the_unit_form_and_itself(base, monkeypatch):
    """nothing set: 16 frames (R = 16, one frame per workgroup on a device of 64 CUs or more), bit for bit the rows unit's, and a
    second call on the same object repeats the first"""
    x = scaled_frames(base, 16, 9)
    unit, = run_psd(monkeypatch, x, 16, CH, UNIT)
    first, second = run_psd(monkeypatch, x, 16, CH, None, calls=2)
    assert_frames_equal(first, unit, "default plan")
    assert_frames_equal(second, first, "second call")
    for f in (0, 15):
        psd_check(first[f], oracle_frame(x[f * CH:(f + 1) * CH]))


def test_degenerate_and_tiny_frames_between_ordinary_ones(base, monkeypatch):
    """An impulse, a frame whose second half is silent, an all-zero frame (block scales stored as 0) and a frame at 1e-9 of
    full scale (block scales ~1e-16) between ordinary frames of one 9-frame call on three rows.  Workgroup 0 walks frames 0,
    3, 6 (ordinary, ordinary, zero), workgroup 1 frames 1, 4, 7 (ordinary, impulse, ordinary), workgroup 2 frames 2, 5, 8
    (half silent, tiny, ordinary): a scale or a plane word carried over from the iteration before, or read a frame early,
    changes a neighbour by many orders."""
    nframes = 9
    x = scaled_frames(base, nframes, 6).reshape(nframes, CH).copy()
    imp = np.zeros(CH, np.complex64); imp[12345] = 1.0 + 0.5j
    x[4] = imp
    x[2, CH // 2:] = 0
    x[6] = 0
    x[5] *= np.float32(1e-9)
    x = x.reshape(-1)
    unit, = run_psd(monkeypatch, x, nframes, CH, UNIT)
    loop, = run_psd(monkeypatch, x, nframes, CH, LOOP3)
    assert_frames_equal(loop, unit, "hard frames")
    for f in (2, 4, 5, 7):
        psd_check(loop[f], oracle_frame(x[f * CH:(f + 1) * CH]))
    po = oracle_frame(x[6 * CH:7 * CH])                    # the zero frame: the oracle's -300 dB on every bin
    assert np.all(np.isfinite(loop[6])) and np.max(np.abs(loop[6] - po)) <= 1e-3, (loop[6].min(), loop[6].max())


@pytest.mark.parametrize("db", [1, 0])
def test_one_frame_in_db_and_in_linear_power(db, base, monkeypatch):
    """pysdr_spectrum_frame is the entry point with a dB switch: one frame = a loop of one iteration per workgroup, whose
    output stage must be the unit's in both forms.  Two frames, each against the unit form and the oracle."""
    x = scaled_frames(base, 2, 11)
    for f in range(2):
        frame = x[f * CH:(f + 1) * CH]
        unit = run_frame(monkeypatch, frame, db, UNIT)
        loop = run_frame(monkeypatch, frame, db, None)
        assert_frames_equal(loop[None, :], unit[None, :], f"db={db}, frame {f}")
        if not db:
            assert np.all(loop >= 0)
        psd_check(loop if db else 10.0 * np.log10(loop.astype(np.float64) + 1e-300), oracle_frame(frame))
