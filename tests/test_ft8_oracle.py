"""The FT8 skimmer's definition on the CPU: the channelizer prototype's response, the raster's shapes,
the frame and its waveform, the finder, and the float32 oracle (tests/ft8_oracle.py) -- against a plain float64
transcription, its invariance under cuts, the blanking of non-finite row samples -- and what the skimmer finds behind the
float64 definition of the channelizer (tests/channelizer_oracle.py): one station in every position of the raster that is
special, weak stations, noise alone, a very strong station, two stations 62.5 Hz apart, rectangular keying, and the images
36 symbols from a frame.  No GPU: the kernels are held against this oracle bit for bit in tests/test_gpu_ft8.py."""
import numpy as np
import pytest

from tests import channelizer_oracle as cz
from tests import ft8_oracle as fo

BAUD = fo.BAUD
CASES = [(8000.0, 64, 20, 80), (12000.0, 96, 20, 80)]            # fs, S, D, M
PLACES = ("centre", "between", "first", "last", "wrap")
SECONDS = 14.0
T0 = 20                                                          # the frame start of the asserted runs, steps


def fbits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_frame_and_its_waveform():
    from pysdr_amd import ft8
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 2, 174)
    tn = ft8.tones(bits)
    assert list(tn) == fo.tones(bits) and len(tn) == 79
    assert list(tn[:7]) == list(tn[36:43]) == list(tn[72:]) == [3, 1, 4, 0, 6, 5, 2]
    assert list(ft8.tones([0, 0, 0, 0, 0, 1, 0, 1, 0, 0, 1, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 1, 1, 1] + [0] * 150)[7:15]) == [0, 1, 3, 2, 5, 6, 4, 7]
    assert ft8.FRAME_SECONDS == 12.64 and ft8.BAUD == BAUD == 6.25
    for gfsk in (True, False):
        w = ft8.waveform(tn, 100.0, 8000.0, gfsk)
        assert len(w) == 79 * 1280 and np.allclose(np.abs(w), 1) and np.allclose(w, fo.waveform(fo.tones(bits), 100.0, 8000.0, gfsk), atol=1e-9)
        f = np.diff(np.unwrap(np.angle(w))) * 8000.0 / (2 * np.pi)                 # continuous phase: the frequency stays within the tones
        assert f.min() > 100.0 - 1e-6 and f.max() < 100.0 + 7 * BAUD + 1e-6
        mid = f[640::1280][:79]                                                    # a symbol's middle is on its tone
        assert np.allclose(mid, 100.0 + BAUD * tn, atol=1e-3 if gfsk else 1e-6)
    # the GFSK pulse: BT = 2, area one symbol
    from math import erf, log, pi, sqrt
    k = 2 * pi * sqrt(2 / log(2))
    t = (np.arange(-3 * 1280, 3 * 1280) + 0.5) / 1280
    pulse = np.array([(erf(k * (v + 0.5)) - erf(k * (v - 0.5))) / 2 for v in t])
    assert abs(pulse.sum() / 1280 - 1) < 1e-9 and abs(pulse[3 * 1280] - 1) < 1e-6
    llr = np.array([2.0, -2.0, 4.0, -4.0], np.float32)
    assert abs(np.std(ft8.unit_llr(llr)) - 1) < 1e-6 and not ft8.unit_llr(np.zeros(4)).any() and list(ft8.hard_bits(llr)) == [1, 0, 1, 0]


@pytest.mark.parametrize("fs, S", [(8000.0, 64), (16000.0, 64), (12000.0, 96), (48000.0, 96)])
def test_prototype_is_flat_over_a_row_and_down_where_the_aliases_begin(fs, S):
    from pysdr_amd import ft8
    fs_out = S * BAUD
    M = 4 * int(round(fs / fs_out))
    NB = S // 2 + 14
    h = ft8.prototype(fs, M, S)
    fp = (NB + 1) * BAUD / 4 + BAUD                                # the outer bin, a raster step beyond it, one baud
    assert 4 * M - 1 <= len(h) <= 4 * M + 1 and abs(np.sum(h) - 1) < 1e-12
    f = np.concatenate((np.linspace(0, fp, 400), np.linspace(fs_out - fp, fs / 2, 4000)))
    H = np.abs(np.exp(-2j * np.pi * np.outer(f, np.arange(len(h))) / fs) @ h)
    db = 20 * np.log10(np.maximum(H, 1e-30))
    print(f"fs {fs} S {S}: fp {fp:.1f} Hz, pass band {db[:400].min():+.4f} .. {db[:400].max():+.4f} dB, stop band {db[400:].max():.1f} dB")
    assert np.abs(db[:400]).max() <= 0.1
    assert db[400:].max() <= -70.0


def test_shapes_of_the_raster(hiplib):
    from pysdr_amd import ft8
    for fs in (4000, 8000, 16000, 20000, 32000):
        S, D, M = ft8.shape(fs)
        assert S == 64 and D * 400 == fs and M == 4 * D
    for fs in (6000, 12000, 24000, 48000, 96000):
        S, D, M = ft8.shape(fs)
        assert S == 96 and D * 600 == fs and M == 4 * D
    for fs in (44100, 11025, 9500, 300.0, 8e6):
        with pytest.raises(ValueError):
            ft8.shape(fs)
    for S in (64, 96):
        tw = ft8.tables(S)
        assert tw.dtype == np.float32 and tw.shape == (4 * S, 2) and np.array_equal(fbits(tw), fbits(fo.tables(S)))
    # the fine rows of all rows form one raster of baud / 2, tone 0 of decoder j on bin j
    for fs, S, D, M in CASES:
        ff = fo.fine_freqs(fs, M, S, (3, 3))
        assert np.allclose(np.diff(ff), BAUD / 2) and abs(ff[0] - (3 * fs / M - (S // 2 + 13) * BAUD / 4)) < 1e-9


def test_finder_equals_the_loop():
    from pysdr_amd import ft8
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 5, 40, 200):
        for nfine in (None, 96):
            for trial in range(4):
                ev = [(int(rng.integers(0, 30)), int(rng.integers(0, 96)), float(rng.integers(0, 5)) if trial % 2 else float(rng.random()), 21)
                      for _ in range(n)]
                ev = list({e[:2]: e for e in ev}.values())                          # one event per (t0, F)
                assert np.array_equal(ft8.owners(ev, nfine=nfine), fo.owners(ev, nfine=nfine)), (n, nfine, trial)
    ev = [(10, 5, 9.0, 21), (12, 7, 5.0, 15), (15, 5, 5.0, 15), (10, 8, 5.0, 15), (14, 3, 9.0, 21), (20, 95, 8.0, 20), (20, 1, 7.0, 20)]
    # (14, 3) ties with (10, 5) and (15, 5) with (12, 7): the lower (t0, F) wins; (10, 8) is out of (10, 5)'s reach and wins its tie
    assert list(ft8.owners(ev)) == [True, False, False, True, False, True, True]
    assert list(ft8.owners(ev, nfine=96)) == [True, False, False, True, False, True, False]   # 95 and 1 are two rows apart on the circle
    assert list(ft8.owners(ev, reach_f=0, reach_t=0)) == [True] * 7


def ideal_rows(S, nk, seconds, seed, snr=-8.0):
    """rows at S samples per symbol without a channelizer: a station per row and white noise"""
    fs = S * BAUD
    rng = np.random.default_rng(seed)
    rows, sent = [], []
    for a in range(nk):
        bits = rng.integers(0, 2, 174)
        j = (5 + 11 * a) % (S // 2)
        f = (2 * j - (S // 2 + 13)) * BAUD / 4 + 0.4 * a
        n = int(seconds * fs)
        x = fo.noise_sigma(snr, fo.SNR_BW, fs) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        at = int((0.3 + 0.37 * a) * fs)
        w = fo.waveform(fo.tones(bits), f, fs, phase=0.5 * a)
        x[at:at + len(w)] += w[:n - at]
        rows.append(x)
        sent.append((at / (S // 4), a * (S // 2) + j, bits))
    return np.array(rows).astype(np.complex64), sent


@pytest.mark.parametrize("S", (64, 96))
def test_the_oracle_equals_the_float64_transcription(S):
    """(t0, F) and hits of every event, and the hard bits of the stations' frames"""
    rows, sent = ideal_rows(S, 2, 14.0, 10 + S)
    sk = fo.Skimmer(2, S, False)
    sk.push(rows)
    ev64, P = fo.plain64(rows, S, fo.params())
    assert sorted(e[:2] + e[3:] for e in sk.all_events) == sorted(e[:2] + e[3:] for e in ev64) and len(ev64) >= 2
    for a, b in zip(sorted(sk.all_events), sorted(ev64)):
        assert abs(a[2] - b[2]) <= 1e-3 * b[2]
    for t0, F, bits in sent:
        rec = [r for r in sk.records if r["F"] == F and abs(r["t0"] - t0) <= 1]
        assert len(rec) == 1
        hard = (rec[0]["llr"] > 0).astype(int)
        assert list(hard) == list((fo.plain_llr(P, S, F, rec[0]["t0"]) > 0).astype(int)) == list(bits)
    assert len(sk.records) == 2


@pytest.mark.parametrize("S", (64, 96))
def test_any_cut_gives_the_same_events_state_bits_and_soft_bits(S):
    D = 8
    rows, sent = ideal_rows(S, 2, 14.0, 20 + S)
    n = rows.shape[1] * D                                          # input samples of a channelizer that decimates by D
    one = fo.Oracle(2, S, fo.params(), 1 << 20)
    t_first = one.t_done
    wc, wev = one.process(rows)
    want = sorted(one.events_of(t_first, wev))
    assert len(want) >= 2
    soft = [one.llr(e[1], e[0]) for e in want]
    rng = np.random.default_rng(S)
    for name, cuts in (("1", [1] * (40 * D)), ("D + 1", [D + 1] * (n // (D + 1)) + [n % (D + 1)]),
                       ("ragged", cz.random_cuts(n, D, 3)), ("long", [int(v) for v in rng.integers(1, 256 * D, 60)])):
        cuts = list(cuts)
        while sum(cuts) < n:
            cuts.append(min(256 * D, n - sum(cuts)))
        o = fo.Oracle(2, S, fo.params(), 256)
        got, at = [], 0
        for c in cuts:
            m0, m1 = cz.frame_range(at, min(at + c, n), D)
            at = min(at + c, n)
            t_first = o.t_done
            _, ev = o.process(rows[:, m0:m1])
            got += o.events_of(t_first, ev)
            if at == n:
                break
        assert at == n and sorted(got) == want, name
        a, b = o.state(), one.state()
        assert np.array_equal(fbits(a["sc"]), fbits(b["sc"])) and np.array_equal(a["hits"], b["hits"]) and a["t_done"] == b["t_done"], name
        for e, s in zip(want, soft):
            if o.llr_ok(e[1], e[0]):
                assert np.array_equal(fbits(o.llr(e[1], e[0])), fbits(s)), name
    gaps = [np.diff(sorted(e[0] for e in want if e[1] == F)).min() for F in {e[1] for e in want} if sum(e[1] == F for e in want) > 1]
    assert not gaps or min(gaps) >= 5


@pytest.mark.parametrize("S", (64, 96))
def test_a_non_finite_or_absurd_row_sample_blanks_exactly_the_steps_that_hold_it(S):
    rows, _ = ideal_rows(S, 2, 6.0, 30 + S)
    o = fo.Oracle(2, S, fo.params())
    T = fo.steps_done(rows.shape[1], S)
    starts = (S // 4) * np.arange(T) + (S - 1)
    P0 = o.spectrum(np.concatenate((o.hist, rows), axis=1), starts)
    dirty = rows.copy()
    spots = {(0, 300): complex(np.nan, 0.5), (1, 700): complex(0.5, -np.inf), (0, 1000): complex(3e19, 0), (0, 1300): complex(1e7, 0)}
    for (a, k), v in spots.items():
        dirty[a, k] = v
    P = o.spectrum(np.concatenate((o.hist, dirty), axis=1), starts)
    assert np.isfinite(P).all()
    for a in range(2):
        for t in range(T):
            held = [abs(v) for (b, k), v in spots.items() if a == b and (S // 4) * t <= k < (S // 4) * t + S]
            if not held:
                assert np.array_equal(fbits(P[a, t]), fbits(P0[a, t])), (a, t)
            elif held != [1e7]:                                     # 1e7: power about 1e14 < pmax, kept
                assert not P[a, t].any(), (a, t)
            else:
                assert P[a, t].all()


# ---- behind the channelizer --------------------------------------------------------------------------------------------

def channels_of(place, M):
    return (M - 1, 3) if place == "wrap" else (3, 3)


def station_freq(place, fs, S, M):
    """Hz of the station's tone 0 and the fine rows that may own it"""
    nsub = S // 2
    ff = fo.fine_freqs(fs, M, S, channels_of(place, M))
    F = {"centre": nsub + nsub // 2 + 2, "between": nsub + nsub // 2 + 2, "first": nsub, "last": 2 * nsub - 1, "wrap": nsub}[place]
    if place == "between":
        return ff[F] + BAUD / 4, (F, F + 1)
    return ff[F], (F,)


def rows_behind_the_channelizer(x, fs, S, D, M, channels):
    from pysdr_amd import ft8
    h = ft8.prototype(fs, M, S)
    m1 = -(-len(x) // D)
    return cz.polyphase(x, h, M, D, 0, m1, fo.rows_of(M, channels)).astype(np.complex64)


def start_sample(t0, S, D, M):
    """the input sample at which a frame begins so that its symbols fall on the windows of step t0: the prototype of 4 M
    taps delays a row by 2 M input samples, 8 row outputs"""
    return (t0 * (S // 4) - 8) * D


def find(case, place, snr, seed, gfsk=True, second=None, seconds=SECONDS, t0=T0, off=0.0, p=None):
    """one station (and a second one: (Hz above it, dB)) behind the float64 channelizer -> the oracle skimmer's records"""
    fs, S, D, M = case
    f, homes = station_freq(place, fs, S, M)
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, 174)
    n = int(seconds * fs)
    x = fo.noise_sigma(0.0, fo.SNR_BW, fs) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    if snr is not None:
        at = start_sample(t0, S, D, M)
        w = fo.waveform(fo.tones(bits), f + off, fs, gfsk, phase=rng.uniform(0, 6.28)) * 10 ** (snr / 20)
        x[at:at + len(w)] += w[:n - at]
    bits2 = rng.integers(0, 2, 174)
    if second is not None:
        at = start_sample(t0 + 6, S, D, M)
        w = fo.waveform(fo.tones(bits2), f + second[0], fs, gfsk, phase=1.0) * 10 ** (second[1] / 20)
        x[at:at + len(w)] += w[:n - at]
    rows = rows_behind_the_channelizer(x, fs, S, D, M, channels_of(place, M))
    sk = fo.Skimmer(3, S, False, p=p)
    sk.push(rows)
    sk.rows = rows
    return sk, homes, bits, bits2


def errors(rec, bits):
    return int(((rec["llr"] > 0).astype(int) != bits).sum())


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("case", CASES, ids=["8000", "12000"])
def test_one_station_is_found_on_its_owner_with_its_bits(case, place):
    """-10 dB and 0 dB in 2500 Hz, three seeds: on a decoder's centre, half way between two decoders, in the first and the
    last decoder of a row and across the wrap of the channel range.  One record: the station's owner, at exactly its step,
    with every hard bit as sent; nothing elsewhere."""
    for snr in (-10.0, 0.0):
        for seed in range(3):
            sk, homes, bits, _ = find(case, place, snr, 100 * PLACES.index(place) + 10 * seed + int(abs(snr)))
            got = [(r["t0"], r["F"], round(r["score"], 1), r["hits"], errors(r, bits)) for r in sk.records]
            print(f"fs {case[0]} {place} {snr} dB seed {seed}: homes {homes}", got)
            assert len(got) == 1 and got[0][0] == T0 and got[0][1] in homes and got[0][4] == 0, (snr, seed, homes, got)


@pytest.mark.parametrize("case", CASES, ids=["8000", "12000"])
def test_weak_stations_are_reported_not_asserted(case):
    for snr in (-15.0, -18.0, -20.0):
        hits = []
        for seed in range(2):
            for place, off in (("centre", 0.0), ("between", 0.0), ("centre", 0.7)):
                sk, homes, bits, _ = find(case, place, snr, 7000 + 10 * seed + int(abs(snr)), off=off)
                near = [r for r in sk.records if abs(r["t0"] - T0) <= 1 and min(abs(r["F"] - h) for h in homes) <= 1]
                hits.append((len(near), errors(near[0], bits) if near else None, len(sk.records) - len(near)))
        print(f"fs {case[0]} {snr} dB: found {sum(h[0] > 0 for h in hits)} of {len(hits)}, bit errors {[h[1] for h in hits]}, "
              f"other records {sum(h[2] for h in hits)}")


@pytest.mark.parametrize("case", CASES, ids=["8000", "12000"])
def test_sixty_seconds_of_noise_give_no_event(case):
    sk, _, _, _ = find(case, "centre", None, 60, seconds=60.0)
    o = sk.o
    print(f"fs {case[0]}: 60 s of noise x {o.nfine} decoders: events {sk.all_events}")
    assert not sk.all_events and not sk.records
    # what the settings keep out: the same noise with the gates open
    loose, peaks = fo.Oracle(3, case[1], fo.params(smin=0.0, hmin=0)), []
    for i0 in range(0, sk.rows.shape[1], 256):
        t_first = loose.t_done
        peaks += loose.events_of(t_first, loose.process(sk.rows[:, i0:i0 + 256])[1])
    print(f"  highest score {max(e[2] for e in peaks):.2f}, highest hit count {max(e[3] for e in peaks)} among {len(peaks)} peaks")
    assert max(e[2] for e in peaks) < 3.0 and max(e[3] for e in peaks) < 13


@pytest.mark.parametrize("case", CASES, ids=["8000", "12000"])
def test_a_30_db_station_leaves_no_second_owner(case):
    """the ghosts a symbol earlier or later and six tones off score high (the denominator is nearly empty there) but hit few
    symbols: hmin removes them; with hmin = 0 they are printed beside"""
    for seed in range(2):
        sk, homes, bits, _ = find(case, "centre", 30.0, 300 + seed)
        got = [(r["t0"], r["F"], round(r["score"], 1), r["hits"], errors(r, bits)) for r in sk.records]
        loose = fo.Skimmer(3, case[1], False, p=fo.params(hmin=0))
        loose.push(sk.rows)
        print(f"fs {case[0]} 30 dB: {got}; with hmin = 0: {[(r['t0'], r['F'], round(r['score'], 1), r['hits']) for r in loose.records]}")
        assert len(got) == 1 and got[0][0] == T0 and got[0][1] in homes and got[0][4] == 0


@pytest.mark.parametrize("gfsk", (True, False), ids=["gfsk", "rectangular"])
@pytest.mark.parametrize("case", CASES, ids=["8000", "12000"])
def test_two_stations_62_hz_apart_are_both_whole(case, gfsk):
    """-5 and -12 dB, 62.5 Hz = 20 raster steps apart, the weaker one six steps later; printed: 31.25 Hz apart, where the
    weaker station's tones lie among the stronger one's"""
    sk, homes, bits, bits2 = find(case, "first", -5.0, 900, gfsk=gfsk, second=(62.5, -12.0))
    got = [(r["t0"], r["F"], round(r["score"], 1), r["hits"]) for r in sk.records]
    print(f"fs {case[0]} gfsk {gfsk}: {got}")
    assert [(r["t0"], r["F"]) for r in sk.records] == [(T0, homes[0]), (T0 + 6, homes[0] + 20)]
    assert errors(sk.records[0], bits) == 0 and errors(sk.records[1], bits2) == 0
    near, _, b1, b2 = find(case, "first", -5.0, 900, gfsk=gfsk, second=(31.25, -12.0))
    print(f"  31.25 Hz apart: {[(r['t0'], r['F'], round(r['score'], 1), r['hits'], errors(r, b1), errors(r, b2)) for r in near.records]}")


@pytest.mark.parametrize("case", CASES, ids=["8000", "12000"])
def test_rectangular_keying_is_found_likewise(case):
    for snr in (-10.0, 0.0):
        sk, homes, bits, _ = find(case, "centre", snr, 500 + int(abs(snr)), gfsk=False)
        got = [(r["t0"], r["F"], round(r["score"], 1), r["hits"], errors(r, bits)) for r in sk.records]
        print(f"fs {case[0]} rectangular {snr} dB: {got}")
        assert len(got) == 1 and got[0][0] == T0 and got[0][1] in homes and got[0][4] == 0


def test_the_images_36_symbols_from_a_frame_are_reported():
    """Printed, DESIGN.md 3 item 22: 144 steps before and after a frame two of the three Costas arrays meet two of the
    frame's, 14 hits of 21; hmin = 13 lets them through where the stream holds them (a 14 s stream that begins with the
    frame holds neither).  Their soft bits are not a codeword: the LDPC decoder behind refuses them."""
    case = CASES[0]
    sk, homes, bits, _ = find(case, "centre", 0.0, 77, seconds=26.0, t0=160)
    got = [(r["t0"] - 160, r["F"] - homes[0], round(r["score"], 1), r["hits"], errors(r, bits)) for r in sk.records]
    print(f"a 0 dB frame at step 160 of a 26 s stream, records relative to it: {got}")
    assert (0, 0) in [g[:2] for g in got] and all(g[0] in (-144, 0, 144) for g in got)
