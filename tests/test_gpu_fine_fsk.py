"""The RTTY raster skimmer on a fine channelizer: at 512 kS/s the decoders against their
float32 oracle (tests/fsk_oracle.py) -- counts, event words and every state field EQUAL after every call, floats by their
bits, the oracle fed the rows of an independent FineChannelizer of the same shape -- and the text of two stations, one
inside a coarse row and one on a seam between two; at 8 MS/s, which no single channelizer serves, one short station."""
import functools

import numpy as np
import pytest

from tests import fsk_oracle as fo
from tests.test_gpu_fsk import BAUD, MAX_OUT, MESSAGE, same_state
from tests.test_gpu_psk import call_lengths, cut_rows, fbits

pytestmark = pytest.mark.gpu

FS, BAND = 512e3, (21000.0, 22750.0)         # fine rows 84 .. 91 of 2048, 250 Hz apart; coarse row 5 ends with fine row 87
STATIONS = ((21300.0, 20.0), (21880.3, 25.0))        # inside coarse row 5; on the first decoder of fine row 88, its space tone 205 Hz below
SECONDS = 12


def chan():
    from pysdr_amd import fsk
    return fsk.fine_channelizer(FS, BAND, max_in=int(SECONDS * FS))


def make_input():
    n = int(SECONDS * FS)
    rng = np.random.default_rng(512)
    sg = np.float32(fo.noise_sigma(20.0, BAUD, FS))
    x = sg * (rng.standard_normal(n, np.float32) + 1j * rng.standard_normal(n, np.float32))
    for j, (f, snr) in enumerate(STATIONS):
        s = fo.rtty_baseband(fo.baudot_codes(MESSAGE), FS, f, stop=1.0 + 0.5 * j, preamble=3.0 + 0.3 * j, tail=1.0, phase=1.0 + j)
        x[:len(s)] += (s[:n] * 10 ** ((snr - 20.0) / 20)).astype(np.complex64)
    return (np.float32(0.05) * x).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def shared():
    """the input, the rows of an independent fine channelizer, the calls and the oracle's answer to every call"""
    from pysdr_amd import fsk
    x = make_input()
    ch = chan()
    assert (ch.M1, ch.D1, ch.M2, ch.D2, ch.k_first, ch.nk) == (128, 64, 32, 8, 84, 8) and abs(ch.fs_out - 22 * BAUD) < 1e-9
    y = ch.push(x)
    ch.close()
    S, D, nk = 22, ch.D, ch.nk
    tile = fsk.plan(nk, S, MAX_OUT, fsk.params())["tile"]
    cuts = call_lengths(len(x), D, tile, MAX_OUT)
    yc = cut_rows(y, cuts, D)
    o = fo.Oracle(nk, S, fo.params())
    want = []
    for r in yc:
        wc, ev = o.process(r)
        want.append((wc, ev, o.state()))
    for v in (x, y):
        v.setflags(write=False)
    calls, at = [], 0
    for n in cuts:
        calls.append(x[at:at + n])
        at += n
    return dict(x=x, y=y, S=S, D=D, nk=nk, cuts=cuts, calls=calls, yc=yc, want=want)


def test_decoders_on_a_fine_channelizer_equal_the_oracle_on_every_call():
    from pysdr_amd.fsk import RTTY_Raster_Skimmer
    c = shared()
    sk = RTTY_Raster_Skimmer(FS, chan=chan(), max_out=MAX_OUT)
    assert (sk.S, sk.D, sk.M, sk.nk, sk.nfine) == (22, 512, 2048, 8, 176) and not sk.circular
    counts = [r.shape[1] for r in c["yc"]]
    assert 0 in counts and 1 in counts and max(counts) == MAX_OUT
    total = 0
    for j, (x, r, (wc, wev, wst)) in enumerate(zip(c["calls"], c["yc"], c["want"])):
        got = sk.dec.decode_raw(x, events="all", squelch=True)
        assert got["n_out"] == r.shape[1], j
        assert np.array_equal(got["counts"], wc), (j, np.flatnonzero(got["counts"] != wc)[:5])
        for F in np.flatnonzero(wc):
            assert list(got["events"][F, :wc[F]]) == wev[F], (j, F)
        same_state(sk.dec.state(), wst, j)
        assert np.array_equal(fbits(got["qn"]), fbits(wst["qn"])) and np.array_equal(got["open"], wst["open"]), j
        total += int(wc.sum())
    assert total > 100                                                         # the stations were read, not just noise compared
    sk.close()


def test_skimmer_reads_both_stations_inside_a_coarse_row_and_on_a_seam():
    from pysdr_amd.fsk import RTTY_Raster_Skimmer
    c = shared()
    sk = RTTY_Raster_Skimmer(FS, chan=chan())
    assert np.array_equal(sk.freqs, 21000.0 + 250.0 * np.arange(8))
    sk.push(c["x"])
    said = {F: t for F, t in sk.text.items() if t}
    home = []
    for f, snr in STATIONS:
        near = [F for F in said if abs(sk.freqs_fine[F] - f) <= BAUD / 4]     # one raster step
        print(f"station {f} Hz {snr} dB:", {(F, round(float(sk.freqs_fine[F]), 2)): said[F] for F in near})
        assert any(MESSAGE in said[F] for F in near), (f, said)
        home += near
    assert set(said) == set(home), said                                       # nothing on the neighbours, the images or the noise
    assert 4 * 22 in home                                                     # the station on the seam: the first decoder of fine row 88
    sk.close()


def test_skimmer_without_a_channelizer_refuses_8_ms_per_second_and_a_foreign_channelizer():
    """(512 kS/s is within one stage's reach, M = 2048; the fine channelizer serves it with 8 rows instead)"""
    from pysdr_amd.fsk import RTTY_Raster_Skimmer
    with pytest.raises(ValueError):
        RTTY_Raster_Skimmer(8e6)
    ch = chan()
    with pytest.raises(ValueError):
        RTTY_Raster_Skimmer(2 * FS, chan=ch)
    ch.close()


def test_a_station_in_8_ms_per_second_is_read():
    """RTTY_Raster_Skimmer(8e6, chan=fsk.fine_channelizer(8e6, band)): 3.7 s of input, a station at 25 dB 800 Hz into a band
    of eight fine rows 100 kHz from the centre.  The call sign is asserted; the diddles in front of it give the two tone
    levels of the decoders their first updates (what a start transient costs)."""
    from pysdr_amd import fsk
    fs, text, call = 8e6, "RYRY CQ K1ABC", "CQ K1ABC"
    band = (100e3, 100e3 + 7 * 250.0)
    x = fo.rtty_baseband(fo.baudot_codes(text), fs, 100e3 + 800.0, stop=1.0, preamble=1.5, tail=0.15, dtype=np.complex64)
    rng = np.random.default_rng(8)
    sg = np.float32(fo.noise_sigma(25.0, BAUD, fs))
    for i in range(0, len(x), 1 << 22):
        n = len(x[i:i + (1 << 22)])
        x[i:i + n] += sg * (rng.standard_normal(n, np.float32) + 1j * rng.standard_normal(n, np.float32))
    x *= np.float32(0.01)
    sk = fsk.RTTY_Raster_Skimmer(fs, chan=fsk.fine_channelizer(fs, band))
    assert (sk.chan.M1, sk.chan.D1, sk.chan.M2, sk.chan.D2, sk.S, sk.D, sk.nk) == (2000, 1000, 32, 8, 22, 8000, 8)
    sk.push(x)
    said = {F: t for F, t in sk.text.items() if t}
    print({(F, round(float(sk.freqs_fine[F]), 1)): t for F, t in said.items()})
    assert len(said) == 1 and all(abs(sk.freqs_fine[F] - (100e3 + 800.0)) <= BAUD / 4 and call in t for F, t in said.items())
    sk.close()
