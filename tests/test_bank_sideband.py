"""The complex-tap modes of the channel bank, what needs no GPU: the tap designs against the
oracle's, the new entry point's argument check, and the float32 helper against the float64 helper on the measure the GPU
tests use."""
import numpy as np
import pytest

from oracle import sdr_oracle as so
from tests import bank_oracle as bo
from tests import bank_sideband_oracle as sbo


@pytest.mark.parametrize("fs_out", [25e3, 6e3])
@pytest.mark.parametrize("T", [255, 125, 64])
def test_sideband_taps_are_the_oracles(fs_out, T):
    from pysdr_amd.bank import sideband_taps
    for mode in ("USB", "LSB"):
        for idx, lab in enumerate(so.AF_BWs):
            bw = so.parse_bw(lab) or 0.0
            got = sideband_taps(fs_out, T, mode, bw, sbo.BFO)
            assert got.dtype == np.complex128 and got.shape == (T,)
            assert np.max(np.abs(got - so.af_taps_for_mode(mode, idx, bw, sbo.BFO, fs_out, T))) <= 1e-12, (mode, lab)
        # a width without a label is 'Max'
        assert np.array_equal(sideband_taps(fs_out, T, mode, 1234.0), sideband_taps(fs_out, T, mode, 0.0))
    assert np.array_equal(sideband_taps(fs_out, T, "LSB", 3e3), np.conj(sideband_taps(fs_out, T, "USB", 3e3)))
    for bw in (0.0, 100.0, 500.0, 3e3):
        for bfo in (700.0, 450.0):
            got = sideband_taps(fs_out, T, "CW", bw, bfo)
            assert got.dtype == np.complex128
            assert np.max(np.abs(got - so.af_taps_for_mode("CW", 0, bw, bfo, fs_out, T))) <= 1e-12, (bw, bfo)


def test_sideband_taps_refuses_other_modes():
    from pysdr_amd import _lib
    from pysdr_amd.bank import ChannelBank, SidebandBank, sideband_taps
    for mode in ("AM", "NFM", "IQ", "SSB"):
        with pytest.raises(_lib.PysdrError):
            sideband_taps(25e3, 255, mode, 3e3)
    assert ChannelBank.MODES == ("AM", "NFM") and SidebandBank.MODES == ("AM", "NFM", "USB", "LSB", "CW")
    assert issubclass(SidebandBank, ChannelBank)


def test_set_mode_cplx_checks_its_arguments_before_any_device_work(hiplib):
    from pysdr_amd import _lib
    c = np.zeros(255)
    assert hiplib.pysdr_bank_set_mode_cplx(None, 3, _lib.as_pd(c), _lib.as_pd(c), 255, 0.0) == -1       # PYSDR_ERR_ARG
    assert b"pysdr_bank_set_mode_cplx" in hiplib.pysdr_last_error()
    assert hiplib.pysdr_bank_set_mode_cplx(None, 5, None, None, 255, 700.0) == -1


def test_float32_helper_is_ten_times_inside_the_bar_on_the_scale():
    """What the GPU tests' bar rests on: float32 helper against float64 helper on the start of the base case, rows from
    the float64 polyphase channelizer, normalised by the scale -- a carrier channel, its neighbour, a noise channel, the
    weakest carrier, in calls of 1, 3, 0 and 600 outputs.  Ten-fold room under TOL = 1e-5."""
    from pysdr_amd.design import channelizer_taps
    from tests import channelizer_oracle as co
    M, D, _, T = bo.BASE
    c = bo.case(M, D, frames=700)
    ks = [3, 4, 20, 59]
    y = co.polyphase(c["x"].astype(np.complex128), channelizer_taps(M), M, D, 0, 604, ks).astype(np.complex64)
    fs_out = c["fs"] / D
    for mode in ("USB", "LSB", "CW"):
        t = sbo.taps(mode, fs_out, T)
        o32 = sbo.SidebandOracle(len(ks), fs_out, t, mode, agc=False)
        o64 = sbo.SidebandOracle(len(ks), fs_out, t, mode, agc=False, dtype=np.float64)
        for m0, m1 in ((0, 1), (1, 4), (4, 4), (4, 604)):
            w32, w64 = o32.process(y[:, m0:m1]), o64.process(y[:, m0:m1])
            if m1 == m0:
                assert w32["a"].shape == (len(ks), 0) and not w32["scale"].any()
                continue
            assert (w64["scale"] > 0).all() and (w32["gain"] == 1).all()
            e = np.max(np.abs(w32["a"] - w64["a"]), axis=1) / w64["scale"]
            assert e.max() <= 1e-6, (mode, m0, float(e.max()))
