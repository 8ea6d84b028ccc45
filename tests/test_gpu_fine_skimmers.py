"""The PSK31 and the CW skimmer on a fine channelizer at rates a single channelizer cannot serve:
the decoders against their float32 oracles (tests/psk_oracle.py, tests/cw_oracle.py) -- counts, event words and every
state field EQUAL after every call, floats by their bits, the oracle fed the rows of an independent FineChannelizer of
the same shape -- and the text the skimmers read; and the channel bank's C object on the same handle."""
import functools

import numpy as np
import pytest

from tests import cw_oracle as co
from tests import psk_oracle as po
from tests.test_cw_oracle import ASSERTED_WPM, OFFSETS, SNRS
from tests.test_fine_oracle import psk_input
from tests.test_gpu_cw import call_lengths as cw_call_lengths, cut_rows, same_state as cw_same_state
from tests.test_gpu_psk import BAUD, MAX_OUT, MESSAGE, call_lengths as psk_call_lengths, fbits, same_state as psk_same_state

pytestmark = pytest.mark.gpu

PSK_FS, PSK_BAND = 512e3, (20250.0, 20690.0)
CW_FS, CW_BAND, CW_R = 192e3, (9000.0, 12000.0), 375.0
CW_MAX_OUT = 1024
# (fine channel, fraction of a fine spacing off its centre, wpm, channel SNR dB): inside a coarse row, and on the seam at 10500 Hz
CW_CARRIERS = ((50, OFFSETS[0], ASSERTED_WPM[-1], SNRS[0]), (56, OFFSETS[1], ASSERTED_WPM[-2], SNRS[1]))
CW_SIGMA = 0.01


def calls_of(x, cuts):
    out, at = [], 0
    for n in cuts:
        out.append(x[at:at + n])
        at += n
    return out


# ---- PSK31 at 512 kS/s ----------------------------------------------------------------------------------------------------
def psk_chan():
    from pysdr_amd import psk
    return psk.fine_channelizer(PSK_FS, PSK_BAND, BAUD, max_in=int(12 * PSK_FS))


@functools.lru_cache(maxsize=None)
def psk_shared():
    """the input, the rows of an independent fine channelizer, the calls and the oracle's answer to every call"""
    from pysdr_amd import psk
    x, stations = psk_input(PSK_FS)
    ch = psk_chan()
    assert (ch.M1, ch.D1, ch.M2, ch.D2, ch.k_first, ch.nk) == (512, 256, 32, 8, 324, 8) and ch.fs_out == 8 * BAUD
    y = ch.push(x)
    ch.close()
    S, D, nk = 8, ch.D, ch.nk
    tile = psk.plan(nk, S, MAX_OUT, psk.params())["tile"]
    cuts = psk_call_lengths(len(x), D, tile, MAX_OUT)
    yc = cut_rows(y, cuts, D)
    o = po.Oracle(nk, S, po.params())
    want = []
    for r in yc:
        wc, ev = o.process(r)
        want.append((wc, ev, o.state()))
    for v in (x, y):
        v.setflags(write=False)
    return dict(x=x, y=y, stations=stations, S=S, D=D, nk=nk, cuts=cuts, calls=calls_of(x, cuts), yc=yc, want=want)


def test_psk_decoders_on_a_fine_channelizer_equal_the_oracle_on_every_call():
    from pysdr_amd.psk import PSK_Skimmer
    c = psk_shared()
    sk = PSK_Skimmer(PSK_FS, BAUD, chan=psk_chan(), max_out=MAX_OUT)
    assert (sk.S, sk.D, sk.M, sk.nk, sk.nfine) == (8, 2048, 8192, 8, 256) and not sk.circular
    counts = [r.shape[1] for r in c["yc"]]
    assert 0 in counts and 1 in counts and max(counts) == MAX_OUT
    total = 0
    for j, (x, r, (wc, wev, wst)) in enumerate(zip(c["calls"], c["yc"], c["want"])):
        got = sk.dec.decode_raw(x, events="all", squelch=True)
        assert got["n_out"] == r.shape[1], j
        assert np.array_equal(got["counts"], wc), (j, np.flatnonzero(got["counts"] != wc)[:5])
        for F in np.flatnonzero(wc):
            assert list(got["events"][F, :wc[F]]) == wev[F], (j, F)
        psk_same_state(sk.dec.state(), wst, j)
        assert np.array_equal(fbits(got["qn"]), fbits(wst["qn"])) and np.array_equal(got["open"], wst["open"]), j
        total += int(wc.sum())
    assert total > 60                                                          # the stations were read, not just noise compared
    sk.close()


def test_psk_skimmer_reads_both_stations_either_side_of_the_seam():
    from pysdr_amd.psk import PSK_Skimmer
    c = psk_shared()
    sk = PSK_Skimmer(PSK_FS, chan=psk_chan())
    assert np.array_equal(sk.freqs, 20250.0 + 62.5 * np.arange(8))
    sk.push(c["x"])
    said = {F: t for F, t in sk.text.items() if t}
    home = []
    for f, snr in c["stations"]:
        near = [F for F in said if abs(sk.freqs_fine[F] - f) <= BAUD / 16]     # one raster step
        print(f"station {f} Hz {snr} dB:", {(F, round(float(sk.freqs_fine[F]), 2)): said[F] for F in near})
        assert any(MESSAGE in said[F] for F in near), (f, said)
        home += near
    assert set(said) == set(home), said                                       # nothing on the images, nothing on noise
    sk.close()


def test_psk_skimmer_without_a_channelizer_still_refuses_this_rate():
    from pysdr_amd.psk import PSK_Skimmer
    with pytest.raises(ValueError):
        PSK_Skimmer(PSK_FS)


# ---- CW at 192 kS/s, rows at 375 Hz ----------------------------------------------------------------------------------------
def cw_chan(n):
    from pysdr_amd import cw
    return cw.fine_channelizer(CW_FS, CW_BAND, CW_R, max_in=n)


def cw_input():
    """the message of tests/test_cw_oracle.py at two of its speeds and both of its SNRs, on two fine rows, in noise"""
    from pysdr_amd.cw import morse_keying
    from pysdr_amd.design import channelizer_taps
    D1, M2, df = 32, 32, CW_FS / 1024
    slowest = min(w for _, _, w, _ in CW_CARRIERS)
    n = int(len(morse_keying(co.MESSAGE, slowest, CW_FS)) + (0.8 + 12 * 1.2 / slowest) * CW_FS)
    rng = np.random.default_rng(192)
    x = CW_SIGMA * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    # noise power in a fine channel per unit carrier power: the input's density through the second prototype at fs / D1
    gain = 2 * CW_SIGMA ** 2 * np.sum(channelizer_taps(M2) ** 2) / D1
    for j, (G, off, wpm, snr) in enumerate(CW_CARRIERS):
        c = co.keyed_carrier(co.MESSAGE, wpm, CW_FS, (G + off) * df, np.sqrt(gain * 10 ** (snr / 10)), 0.5 + 0.1 * j, 0.0, morse_keying,
                             phase=1.0 + j)
        x[:len(c)] += c[:n]
    return x.astype(np.complex64)


@functools.lru_cache(maxsize=None)
def cw_shared():
    from pysdr_amd import cw
    x = cw_input()
    ch = cw_chan(len(x))
    assert (ch.M1, ch.D1, ch.M2, ch.D2, ch.k_first, ch.nk) == (64, 32, 32, 16, 48, 17) and ch.fs_out == CW_R
    run_in = ch.run_in_taps
    y = ch.push(x)
    ch.close()
    D, nk = 512, 17
    tile = cw.plan(nk, CW_MAX_OUT, cw.params(CW_R))["tile"]
    cuts = cw_call_lengths(len(x), D, tile)
    yc = cut_rows(y, cuts, D)
    o = co.Oracle(nk, co.params(CW_R, settle=co.settle_samples(run_in, D, CW_R)))
    want = []
    for r in yc:
        wc, ev = o.process(r)
        want.append((wc, ev, o.state()))
    for v in (x, y):
        v.setflags(write=False)
    return dict(x=x, y=y, D=D, nk=nk, run_in=run_in, calls=calls_of(x, cuts), yc=yc, want=want)


def test_cw_decoders_on_a_fine_channelizer_equal_the_oracle_and_read_the_message():
    from pysdr_amd.cw import CW_Skimmer, code_text
    c = cw_shared()
    sk = CW_Skimmer(CW_FS, chan=cw_chan(len(c["x"])), max_out=CW_MAX_OUT)
    assert (sk.M, sk.D, sk.nk, sk.fs_out) == (1024, 512, 17, CW_R)
    assert sk.dec.cfg.n0 == co.settle_samples(c["run_in"], c["D"], CW_R)      # the run-in of both stages, in outputs
    words = [[] for _ in range(c["nk"])]
    for j, (x, r, (wc, wev, wst)) in enumerate(zip(c["calls"], c["yc"], c["want"])):
        got = sk.dec.decode_raw(x, events="all")
        assert got["n_out"] == r.shape[1], j
        assert np.array_equal(got["counts"], wc), (j, got["counts"], wc)
        for a in range(c["nk"]):
            assert list(got["events"][a, :wc[a]]) == wev[a], (j, a)
            words[a] += wev[a]
        cw_same_state(sk.dec.state(), wst, j)
    for G, off, wpm, snr in CW_CARRIERS:
        text = co.text_of(words[G - 48], code_text)
        print(f"fine channel {G} ({sk.freqs[G - 48]} Hz), {off} off centre, {wpm} wpm, {snr} dB: {text!r}")
        assert co.TAIL in text, (G, text)
    sk.close()


# ---- the channel bank's C object on the same handle -------------------------------------------------------------------------
def test_the_banks_c_object_runs_on_a_fine_channelizer():
    """pysdr_bank_create takes the fine handle as it takes a plain one: AM audio, AGC state and the rows it keeps against
    the bank's oracle (tests/bank_oracle.py) fed the rows of an independent fine channelizer, at the bank's own 1e-5"""
    import ctypes as C

    from scipy.signal import firwin

    from pysdr_amd import _lib
    from pysdr_amd.tables import MODE_INDEX
    from tests import bank_oracle as bo
    c = cw_shared()
    x, D, nk = c["x"][:400 * 512 + 77], c["D"], c["nk"]
    af = np.ascontiguousarray(firwin(63, 60.0, fs=CW_R), np.float64)
    ch = cw_chan(len(c["x"]))
    L = _lib.lib()
    hd = C.c_void_p()
    _lib.check(L.pysdr_bank_create(ch._h, CW_R, MODE_INDEX["AM"], len(af), C.byref(hd)), "pysdr_bank_create")
    _lib.check(L.pysdr_bank_set_mode(hd, MODE_INDEX["AM"], _lib.as_pd(af), len(af)), "pysdr_bank_set_mode")
    o = bo.BankOracle(nk, CW_R, af, "AM")
    at, m, worst = 0, 0, 0.0
    for n in (1, 300, 100 * D + 5, len(x) - 100 * D - 306):                  # a call without outputs among them
        n_out = C.c_int(-1)
        cap = -(-(at + n) // D) - -(-at // D)
        am = np.empty((nk, max(cap, 1)), np.float32)
        xi = np.ascontiguousarray(x[at:at + n])
        _lib.check(L.pysdr_bank_process(hd, C.c_void_p(xi.ctypes.data), n, 0, C.c_void_p(am.ctypes.data), am.shape[1], 0,
                                        C.byref(n_out)), "pysdr_bank_process")
        at += n
        assert n_out.value == cap
        w = o.process(c["y"][:, m:m + cap])
        m += cap
        if cap == 0:
            continue
        e = np.max(np.abs(am[:, :cap] - w["am"]), axis=1) / np.maximum(np.max(np.abs(w["am"]), axis=1), 1e-30)
        worst = max(worst, float(e.max()))
        assert e.max() <= 1e-5, (cap, int(e.argmax()), float(e.max()))
    assert m > 390
    print(f"bank (AM, 63 taps) on a fine channelizer: worst |am - want| / peak of the channel's call {worst:.2e}")
    L.pysdr_bank_destroy(hd)
    ch.close()
