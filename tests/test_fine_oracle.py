"""The fine channelizer's definition on the CPU: the first stage's default prototype, the map between
fine channels and (coarse row, second-stage channel), a tone through the float64 cascade (tests/fine_oracle.py), the
float32 model of the kernels against it, and the PSK31 oracle behind the cascade at a rate one stage cannot serve.  No GPU;
the library is used for its plan alone."""
import numpy as np
import pytest

from tests import channelizer_oracle as cz
from tests import fine_oracle as fo
from tests import psk_oracle as po

BAR = 1e-5
FS = 8e6


def response_db(h, f, fs):
    n = np.arange(len(h))
    return 20 * np.log10(np.abs(np.exp(-2j * np.pi * np.outer(f, n) / fs) @ h) + 1e-300)


@pytest.mark.parametrize("C1,M1,Q", [(2, 64, 8), (2, 64, 16), (2, 1024, 16), (4, 64, 8), (4, 64, 16), (4, 1024, 16)])
def test_prototype1_passes_the_kept_channels_and_stops_their_aliases(C1, M1, Q, hiplib):
    """flat within 0.1 dB out to fp = half a coarse spacing plus one fine spacing, 70 dB down from fs1 - fp on (measured:
    +-0.0006 dB and 81 to 88 dB)"""
    from pysdr_amd import fine
    D1, M2 = M1 // C1, Q * C1
    h = fine.prototype1(FS, M1, D1, M2)
    assert len(h) == (8 if C1 == 2 else 4) * M1 and abs(h.sum() - 1) < 1e-9
    fs1, df = FS / D1, FS / (M1 * Q)
    fp = FS / M1 / 2 + df
    ps = response_db(h, np.linspace(0, fp, 400), FS)
    st = response_db(h, np.linspace(fs1 - fp, FS / 2, 4000), FS)
    print(f"C1 {C1} M1 {M1} Q {Q}: pass band {ps.min():+.5f} .. {ps.max():+.5f} dB, stop band {st.max():.1f} dB")
    assert np.abs(ps).max() <= 0.1 and st.max() <= -70.0


@pytest.mark.parametrize("M1,D1,M2", [(16, 8, 16), (64, 16, 32), (256, 128, 20), (64, 32, 32), (4096, 2048, 64)])
def test_fine_channels_map_one_to_one_onto_the_kept_channels(M1, D1, M2, hiplib):
    from pysdr_amd import fine
    Q = M2 // (M1 // D1)
    Mf = M1 * Q
    assert fine.plan(M1, D1, M2, M2 // 2, g_first=0, ng=min(Mf, fine.NG_MAX))["Mf"] == Mf
    G = np.arange(Mf)
    k1, q, k2 = fo.split(G, M1, D1, M2)
    assert q.min() == -Q // 2 and q.max() == Q // 2 - 1 and (0 <= k1).all() and (k1 < M1).all()
    assert len(set(zip(k1.tolist(), q.tolist()))) == Mf == M1 * Q                  # every (row, kept channel) exactly once
    assert np.array_equal((k1 * Q + q) % Mf, G) and np.array_equal(k2, q % M2)
    # channel G's centre G fs / Mf is q fine spacings from its coarse row's centre k1 fs / M1
    assert np.array_equal(((G - k1 * Q) + Mf // 2) % Mf - Mf // 2, q)
    assert list(fo.used_rows(M1, D1, M2, Mf - 3, 7)) == [0] and list(fo.used_rows(M1, D1, M2, Q // 2 - 1, 2)) == [0, 1]
    assert len(fo.used_rows(M1, D1, M2, 3, Mf)) == M1


def test_a_tone_lands_on_its_fine_row_also_on_a_seam(hiplib):
    """M1, D1, M2, D2 = 64, 32, 32, 16: 0.5 on row G (measured +-3e-5; asserted 1e-4: the first prototype's 0.001 dB ripple
    is 6e-5 of 0.5), at least 80 dB less on G +- 1 (the second prototype is 83 dB down from one spacing on)"""
    from pysdr_amd import fine
    from pysdr_amd.design import channelizer_taps
    M1, D1, M2, D2 = 64, 32, 32, 16
    g = fo.geometry(M1, D1, M2, D2)
    Q, Mf, D = g["Q"], g["Mf"], g["D"]
    h1, h2 = fine.prototype1(FS, M1, D1, M2), channelizer_taps(M2)
    n = np.arange(fo.run_in_taps(h1, h2, D1) + 12 * D)
    m0, m1 = -(-fo.run_in_taps(h1, h2, D1) // D), len(n) // D
    for G in (5 * Q + 3, 7 * Q + Q // 2, Mf - 2 * Q - Q // 2, 9 * Q - 1):          # inside a row, two seams (one negative), a row's last
        x = 0.5 * np.exp(2j * np.pi * (G / Mf) * n)
        y, _ = fo.cascade64(x, h1, h2, M1, D1, M2, D2, (G - 2) % Mf, 5, m0, m1)
        lev = np.abs(y)
        print(f"G {G}: own {lev[2].min():.6f} .. {lev[2].max():.6f}, neighbours {20 * np.log10(max(lev[1].max(), lev[3].max()) / 0.5):.1f} dB")
        assert np.abs(lev[2] - 0.5).max() <= 1e-4
        assert 20 * np.log10(lev[[0, 1, 3, 4]].max() / 0.5) <= -80.0


@pytest.mark.parametrize("M1,D1,M2,D2,g_first,ng", [(16, 8, 16, 8, 0, 128), (64, 16, 32, 32, 64 * 8 - 13, 37), (256, 128, 20, 5, 705, 3)])
def test_the_float32_model_is_within_a_quarter_of_the_bar(M1, D1, M2, D2, g_first, ng, hiplib):
    from pysdr_amd import fine
    from pysdr_amd.design import channelizer_taps
    h1, h2 = fine.prototype1(FS, M1, D1, M2), channelizer_taps(M2)
    x = fo.signal(M1, D1, M2, D2, g_first, ng, h1, h2)
    m1 = len(x) // (D1 * D2)
    want, y1 = fo.cascade64(x, h1, h2, M1, D1, M2, D2, g_first, ng, 0, m1)
    got = fo.model32(x, h1, h2, M1, D1, M2, D2, g_first, ng, 0, m1)
    e = float(np.abs(got - want).max() / fo.scale_of(want, y1, h2, D2, 0, m1))
    print(f"{(M1, D1, M2, D2)}: float32 model {e:.2e} of the scale")
    assert e <= BAR / 4


def test_the_stream_cascade_equals_the_whole_and_any_cut(hiplib):
    from pysdr_amd import fine
    from pysdr_amd.design import channelizer_taps
    M1, D1, M2, D2, g_first, ng = 16, 8, 16, 8, 120, 13
    h1, h2 = fine.prototype1(FS, M1, D1, M2), channelizer_taps(M2)
    x = fo.signal(M1, D1, M2, D2, g_first, ng, h1, h2)[:3001]
    want, _ = fo.cascade64(x, h1, h2, M1, D1, M2, D2, g_first, ng, 0, -(-len(x) // 64))
    c = fo.Cascade(h1, h2, M1, D1, M2, D2, g_first, ng)
    parts, at = [], 0
    for n in cz.random_cuts(len(x), D1 * D2, 3):
        parts.append(c.process(x[at:at + n]))
        at += n
    assert np.abs(np.concatenate(parts, axis=1) - want).max() <= 1e-12


def test_the_psk_oracle_reads_two_stations_either_side_of_a_coarse_seam(hiplib):
    """fs = 512 kS/s, where psk.shape refuses: (M1, D1, M2, D2) = (512, 256, 32, 8), eight fine rows from 20250 Hz, the
    stations at 20480.3 Hz / 20 dB and 20530.0 Hz / 25 dB either side of the seam at 20500 Hz"""
    from pysdr_amd import fine, psk
    from tests.test_gpu_psk import BAUD, MESSAGE
    fs, band, S = 512e3, (20250.0, 20690.0), 8
    with pytest.raises(ValueError):
        psk.shape(fs, BAUD)
    M1, D1, M2, D2 = fine.shape(fs, S * BAUD, 4)
    assert (M1, D1, M2, D2) == (512, 256, 32, 8)
    g_first, ng = fine.channels_for(band, fs, M1, D1, M2)
    assert (g_first * fs / (M1 * 16), ng) == (20250.0, 8)
    x, stations = psk_input(fs)
    h1, h2 = fine.prototype1(fs, M1, D1, M2), psk.prototype(fs / D1, M2, BAUD, S)
    y, _ = fo.cascade64(x, h1, h2, M1, D1, M2, D2, g_first, ng, 0, len(x) // (D1 * D2))
    ref = po.Skimmer(ng, S, False, psk.code_text, 256)
    ref.push(y.astype(np.complex64))
    freqs = ((g_first + np.arange(ng))[:, None] * 62.5 + (2 * np.arange(4 * S) - 4 * S + 1)[None, :] * (BAUD / 32)).reshape(-1)
    for f, snr in stations:
        near = {F: t for F, t in ref.text.items() if abs(freqs[F] - f) <= BAUD / 16}
        print(f"station {f} Hz {snr} dB:", near)
        assert any(MESSAGE in t for t in near.values()), (f, ref.text)
    assert all(min(abs(freqs[F] - f) for f, _ in stations) <= BAUD / 16 for F in ref.text)


def psk_input(fs, seconds=12):
    """the two stations of the 512 kS/s case, message and noise as in tests/test_gpu_psk.py"""
    from pysdr_amd import psk
    from tests.test_gpu_psk import BAUD, MESSAGE
    stations = ((20480.3, 20.0), (20530.0, 25.0))
    n = int(seconds * fs)
    rng = np.random.default_rng(512)
    sg = po.noise_sigma(20.0, BAUD, fs)
    x = sg * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for j, (f, snr) in enumerate(stations):
        s = psk.psk_baseband(MESSAGE, BAUD, fs, f, preamble=6.0 + 0.3 * j, tail=1.0, phase=1.0 + j)
        s = s[:n] * 10 ** ((snr - 20.0) / 20)
        x[:len(s)] += s
    return (0.05 * x).astype(np.complex64), stations
