"""The FT4 skimmer on a fine channelizer: at 512 kS/s in two stages, rows 250 Hz apart, the
skimmer against its float32 oracle (tests/ft4_oracle.py) -- counts, event words, scores, hit counts, the ring and soft
bits EQUAL after every call, floats by their bits, the oracle fed the rows of an independent FineChannelizer of the same
shape -- and one station's record.  8 MS/s is covered by the CPU shape test (tests/test_ft4_plan.py) and the rate script
only: a 7 s stream there is 450 MB of host input."""
import functools

import numpy as np
import pytest

from tests import ft4_oracle as fo
from tests.test_gpu_ft4 import MAX_OUT, RAMP, same_state, words_of
from tests.test_gpu_psk import call_lengths, cut_rows, fbits

pytestmark = pytest.mark.gpu

FS, BAND = 512e3, (21000.0, 22000.0)         # fine rows 84 .. 88 of 2048, 250 Hz apart
STATION = (21500.0 - fo.BAUD / 4 - 0.4, 0.0, 0.5)   # tone 0 one raster point under a row's centre (and 0.4 Hz off it): its upper tones cross the centre
SECONDS = 7


def chan():
    from pysdr_amd import ft4
    return ft4.fine_channelizer(FS, BAND, max_in=int(SECONDS * FS))


def bits():
    return np.random.default_rng(512).integers(0, 2, 174)


def make_input():
    from pysdr_amd import ft4
    n = int(SECONDS * FS)
    rng = np.random.default_rng(513)
    sg = np.float32(fo.noise_sigma(0.0, fo.SNR_BW, FS))
    x = sg * (rng.standard_normal(n, np.float32) + 1j * rng.standard_normal(n, np.float32))
    f, snr, start = STATION
    s = ft4.waveform(ft4.tones(bits()), f, FS, phase=1.0) * 10 ** (snr / 20)          # (equal to the oracle's: tests/test_ft4_oracle.py)
    at = int(start * FS)                                                               # the ramp's first sample
    x[at:at + len(s)] += s[:n - at].astype(np.complex64)
    return (np.float32(0.05) * x).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def shared():
    """the input, the rows of an independent fine channelizer, the calls and the oracle's answer to every call"""
    x = make_input()
    ch = chan()
    assert (ch.M1, ch.D1, ch.M2, ch.D2, ch.nk) == (128, 64, 32, 8, 5) and abs(ch.fs_out - 1000.0) < 1e-9
    y = ch.push(x)
    ch.close()
    S, D, nk = 48, ch.D, ch.nk
    cuts = call_lengths(len(x), D, S, MAX_OUT)
    yc = cut_rows(y, cuts, D)
    o = fo.Oracle(nk, S, fo.params(), MAX_OUT)
    want = []
    for r in yc:
        t_first = o.t_done
        wc, ev = o.process(r)
        want.append((wc, ev, o.state(), o.events_of(t_first, ev)))
    for v in (x, y):
        v.setflags(write=False)
    calls, at = [], 0
    for n in cuts:
        calls.append(x[at:at + n])
        at += n
    return dict(x=x, y=y, S=S, D=D, nk=nk, calls=calls, yc=yc, want=want)


def test_the_skimmer_on_a_fine_channelizer_equals_the_oracle_on_every_call():
    from pysdr_amd.ft4 import FT4_Skimmer
    c = shared()
    sk = FT4_Skimmer(FS, chan=chan(), max_out=MAX_OUT)
    assert (sk.S, sk.D, sk.M, sk.nk, sk.nfine) == (48, 512, 2048, 5, 120) and not sk.circular
    assert np.array_equal(sk.freqs, 21000.0 + 250.0 * np.arange(5))
    o = fo.Oracle(c["nk"], 48, fo.params(), MAX_OUT)
    seen = []
    for j, (x, r, (wc, wev, wst, wlist)) in enumerate(zip(c["calls"], c["yc"], c["want"])):
        got = sk.dec.decode_raw(x, events="all")
        o.process(r)
        assert got["n_out"] == r.shape[1], j
        assert np.array_equal(got["counts"], wc), (j, np.flatnonzero(got["counts"] != wc)[:5])
        for F in np.flatnonzero(wc):
            assert list(got["events"][F, :2 * wc[F]]) == words_of(wev[F]), (j, F)
        same_state(sk.dec.state(ring=True), wst, j)
        for e in wlist:
            assert np.array_equal(fbits(sk.dec.llr([e[1]], [e[0]])[0]), fbits(o.llr(e[1], e[0]))), (j, e)
        seen += wlist
    assert len(seen) >= 1
    sk.close()


def test_the_station_is_one_record_with_its_bits():
    from pysdr_amd import ft4
    c = shared()
    sk = ft4.FT4_Skimmer(FS, chan=chan())
    recs = sk.push(c["x"])
    f, snr, start = STATION
    print([(r["t0"], r["F"], round(r["freq"], 2), round(r["time"], 3), round(r["score"], 1), r["hits"]) for r in recs])
    assert len(recs) == 1 and abs(recs[0]["freq"] - f) <= fo.BAUD / 4 + 0.1 and abs(recs[0]["time"] - (start + RAMP)) <= 0.03
    assert np.array_equal(ft4.hard_bits(recs[0]["llr"]), bits())
    ref = fo.Skimmer(c["nk"], 48, False, MAX_OUT)
    want = ref.push(c["y"])
    assert [(r["t0"], r["F"], r["hits"]) for r in want] == [(r["t0"], r["F"], r["hits"]) for r in recs]
    assert np.array_equal(fbits(recs[0]["llr"]), fbits(want[0]["llr"]))
    sk.close()


def test_a_foreign_channelizer_is_refused():
    """another rate than the channelizer's, and the FT8 raster's rows (400 Hz: 19.2 samples per FT4 symbol)"""
    from pysdr_amd import ft8
    from pysdr_amd.ft4 import FT4_Skimmer
    ch = chan()
    with pytest.raises(ValueError):
        FT4_Skimmer(2 * FS, chan=ch)
    ch.close()
    ch = ft8.fine_channelizer(FS, (21000.0, 21700.0), max_in=1 << 16)
    with pytest.raises(ValueError):
        FT4_Skimmer(FS, chan=ch)
    ch.close()
