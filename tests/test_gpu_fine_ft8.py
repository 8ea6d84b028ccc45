"""The FT8 skimmer on a fine channelizer: at 512 kS/s, which no single channelizer serves at
400 Hz rows, the skimmer against its float32 oracle (tests/ft8_oracle.py) -- counts, event words, scores, hit counts and
soft bits EQUAL after every call, floats by their bits, the oracle fed the rows of an independent FineChannelizer of the
same shape -- and one station's record.  8 MS/s is covered by the CPU shape test (tests/test_ft8_plan.py) and the rate
script only: a 14 s stream there is 900 MB of host input."""
import functools

import numpy as np
import pytest

from tests import ft8_oracle as fo
from tests.test_gpu_ft8 import MAX_OUT, same_state, words_of
from tests.test_gpu_psk import call_lengths, cut_rows, fbits

pytestmark = pytest.mark.gpu

FS, BAND = 512e3, (21000.0, 21700.0)         # fine rows 210 .. 217 of 5120, 100 Hz apart
STATION = (21398.4, -8.0, 0.5)               # tone 0 one raster step under a row's centre: its upper tones cross into the next row's decoders
SECONDS = 14


def chan():
    from pysdr_amd import ft8
    return ft8.fine_channelizer(FS, BAND, max_in=int(SECONDS * FS))


def bits():
    return np.random.default_rng(512).integers(0, 2, 174)


def make_input():
    from pysdr_amd import ft8
    n = int(SECONDS * FS)
    rng = np.random.default_rng(513)
    sg = np.float32(fo.noise_sigma(0.0, fo.SNR_BW, FS))
    x = sg * (rng.standard_normal(n, np.float32) + 1j * rng.standard_normal(n, np.float32))
    f, snr, start = STATION
    s = ft8.waveform(ft8.tones(bits()), f, FS, phase=1.0) * 10 ** (snr / 20)          # (equal to the oracle's: tests/test_ft8_oracle.py)
    at = int(start * FS)
    x[at:at + len(s)] += s[:n - at].astype(np.complex64)
    return (np.float32(0.05) * x).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def shared():
    """the input, the rows of an independent fine channelizer, the calls and the oracle's answer to every call"""
    x = make_input()
    ch = chan()
    assert (ch.M1, ch.D1, ch.M2, ch.D2, ch.nk) == (320, 160, 32, 8, 8) and abs(ch.fs_out - 400.0) < 1e-9
    y = ch.push(x)
    ch.close()
    S, D, nk = 64, ch.D, ch.nk
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
    from pysdr_amd.ft8 import FT8_Skimmer
    c = shared()
    sk = FT8_Skimmer(FS, chan=chan(), max_out=MAX_OUT)
    assert (sk.S, sk.D, sk.M, sk.nk, sk.nfine) == (64, 1280, 5120, 8, 256) and not sk.circular
    assert np.array_equal(sk.freqs, 21000.0 + 100.0 * np.arange(8))
    o = fo.Oracle(c["nk"], 64, fo.params(), MAX_OUT)
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
    from pysdr_amd import ft8
    c = shared()
    sk = ft8.FT8_Skimmer(FS, chan=chan())
    recs = sk.push(c["x"])
    f, snr, start = STATION
    print([(r["t0"], r["F"], round(r["freq"], 2), round(r["time"], 3), round(r["score"], 1), r["hits"]) for r in recs])
    assert len(recs) == 1 and abs(recs[0]["freq"] - f) <= 1.6 and abs(recs[0]["time"] - start) <= 0.08
    assert np.array_equal(ft8.hard_bits(recs[0]["llr"]), bits())
    ref = fo.Skimmer(c["nk"], 64, False, MAX_OUT)
    want = ref.push(c["y"])
    assert [(r["t0"], r["F"], r["hits"]) for r in want] == [(r["t0"], r["F"], r["hits"]) for r in recs]
    assert np.array_equal(fbits(recs[0]["llr"]), fbits(want[0]["llr"]))
    sk.close()


def test_skimmer_without_a_channelizer_refuses_512_ks_per_second_and_a_foreign_channelizer():
    from pysdr_amd.ft8 import FT8_Skimmer
    with pytest.raises(ValueError):
        FT8_Skimmer(FS)
    ch = chan()
    with pytest.raises(ValueError):
        FT8_Skimmer(2 * FS, chan=ch)
    ch.close()
