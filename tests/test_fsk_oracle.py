"""The RTTY raster skimmer's definition on the CPU: the channelizer prototype's response, the raster's
shapes, the finder, and the float32 oracle (tests/fsk_oracle.py) -- its two forms against each other, its invariance under
cuts, the blanking of non-finite row samples -- and what the decoder reads behind the float64 definition of the
channelizer (tests/channelizer_oracle.py): one station alone in every position of the raster that is special and with
1, 1.5 and 2 stop bits, two stations 250 Hz apart, figures, noise alone and a keyed carrier.  No GPU: the kernel is held
against this oracle bit for bit in tests/test_gpu_fsk.py."""
import numpy as np
import pytest

from tests import channelizer_oracle as cz
from tests import fsk_oracle as fo

BAUD = fo.BAUD
MESSAGE = fo.MESSAGE
CASES = [(8000.0, 22, 8, 32), (12000.0, 33, 8, 32)]              # fs, S, D, M
PLACES = ("centre", "between", "first", "last", "wrap")
STOPS = {15.0: 1.0, 20.0: 1.5, 30.0: 2.0}                        # the stop length that goes with an SNR in the asserted runs


def fbits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_baudot_codes_and_the_event_word():
    from pysdr_amd import fsk, rtty
    assert fo.baudot_codes("RY") == [10, 21] and fo.baudot_codes("A 1") == [3, 4, 27, 23]
    assert fo.baudot_codes("RST 599 K") == [10, 5, 16, 4, 27, 16, 24, 24, 4, 31, 15]
    assert [fo.code_text(c) for c in (3, 35, 27, 63, 4, 36)] == ["A", "-", "<FIGS>", "<LTRS>", " ", " "]
    assert fo.code_text is not rtty.code_text and all(fo.code_text(c) == rtty.code_text(c) for c in range(64))
    for i, c in [(0, 0), ((1 << 20) - 1, 63), (12345, 27)]:
        w = np.int32(fo.pack(i, c))
        assert w >= 0 and fsk.unpack(w) == (i, c) == fo.unpack(w)
    assert abs(fsk.BAUD - 1 / 0.022) < 1e-12 and fsk.BAUD == BAUD and abs(fsk.TONE_STEPS * BAUD / 4 - 170.0) < 0.5


@pytest.mark.parametrize("fs, S", [(8000.0, 22), (10000.0, 22), (12000.0, 33), (48000.0, 33)])
def test_prototype_is_flat_over_a_row_and_down_where_the_aliases_begin(fs, S):
    from pysdr_amd import fsk
    fs_out = S * BAUD
    M = 4 * int(round(fs / fs_out))
    h = fsk.prototype(fs, M, S)
    fp = fs_out / 8 + 15 * BAUD / 8 + BAUD                         # half a row spacing, the outer tone, one baud
    assert 4 * M - 1 <= len(h) <= 4 * M + 1 and abs(np.sum(h) - 1) < 1e-12
    f = np.concatenate((np.linspace(0, fp, 400), np.linspace(fs_out - fp, fs / 2, 4000)))
    H = np.abs(np.exp(-2j * np.pi * np.outer(f, np.arange(len(h))) / fs) @ h)
    db = 20 * np.log10(np.maximum(H, 1e-30))
    print(f"fs {fs} S {S}: pass band {db[:400].min():+.4f} .. {db[:400].max():+.4f} dB, stop band {db[400:].max():.1f} dB")
    assert np.abs(db[:400]).max() <= 0.1
    assert db[400:].max() <= -70.0


def test_shapes_of_the_raster(hiplib):
    from pysdr_amd import fsk
    for fs in (4000, 8000, 10000, 16000, 20000, 32000):
        S, D, M = fsk.shape(fs)
        assert S == 22 and D * 1000 == fs and M == 4 * D
    for fs in (6000, 12000, 24000, 48000, 96000):
        S, D, M = fsk.shape(fs)
        assert S == 33 and D * 1500 == fs and M == 4 * D
    for fs in (44100, 11025, 9500, 500.0, 8e6):
        with pytest.raises(ValueError):
            fsk.shape(fs)
    for S in (22, 33):
        tw, g = fsk.tables(S)
        otw, og = fo.tables(S)
        assert tw.dtype == np.float32 and tw.shape == (8 * S, 2) and np.array_equal(fbits(tw), fbits(otw))
        assert g.shape == (S,) and np.array_equal(fbits(g), fbits(og)) and abs(float(g.astype(np.float64).sum()) - 1) < 1e-6
        # decoder j: space 15 baud / 8 below its centre, mark as far above; tone t serves decoder t as space, t - 15 as mark
        j = np.arange(S)
        assert np.array_equal((2 * j - S - 14) + 15, 2 * j - S + 1) and np.array_equal((2 * j - S + 16) - 15, 2 * j - S + 1)
    assert fsk.cfg_dict(fsk.params()) == {k: (float(v) if k != "n0" else v) for k, v in fo.params().items()}


def test_finder_equals_the_loop():
    from pysdr_amd import fsk, psk
    rng = np.random.default_rng(5)
    for NF in (1, 2, 16, 17, 33, 34, 96, 500):
        for circular in (False, True):
            for trial in range(6):
                qn = rng.integers(0, 6, NF).astype(np.float32) if trial % 2 else rng.standard_normal(NF).astype(np.float32)   # ties
                is_open = (rng.random(NF) < 0.6).astype(np.int32)
                prev = None if trial < 3 else rng.random(NF) < 0.2
                got = fsk.owners(qn, is_open, circular, prev)
                assert np.array_equal(got, fo.owners(qn, is_open, circular, prev)), (NF, circular, trial)
                own = np.flatnonzero(got)
                if len(own) > 1 and not circular:
                    assert np.diff(own).min() > 16
    # an open image 15 or 16 rows away loses to the station, one 17 rows away does not; the PSK raster's reach is still 9
    qn = np.zeros(64, np.float32)
    qn[30], qn[45], qn[46], qn[13] = 1.0, 0.2, 0.2, 0.2
    op = (qn > 0).astype(np.int32)
    assert fsk.NEIGHBOURHOOD == fo.REACH == 16
    assert list(np.flatnonzero(fsk.owners(qn, op, False))) == [13, 30]
    assert list(np.flatnonzero(psk.owners(qn, op, False))) == [13, 30, 45]


def ideal_rows(S, nk, seconds, seed):
    """rows at S samples per bit without a channelizer: a station per row and white noise"""
    fs = S * BAUD
    rng = np.random.default_rng(seed)
    rows = []
    for a in range(nk):
        f = (-1) ** a * (2 * a + 1) * BAUD / 8 + 1.3 * a
        x = fo.rtty_baseband(fo.baudot_codes(MESSAGE + " 599 " + MESSAGE), fs, f, stop=1.0 + 0.5 * a, preamble=2.0, tail=seconds,
                             phase=0.5 * a)[:int(seconds * fs)]
        sg = fo.noise_sigma(20.0 - 4 * a, BAUD, fs)
        rows.append(x + sg * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x))))
    return np.array(rows).astype(np.complex64)


@pytest.mark.parametrize("S", (22, 33))
def test_the_vectorised_oracle_equals_the_transcription(S):
    rows = ideal_rows(S, 2, 7.0, 10 + S)
    p = fo.params(n0=24)
    o = fo.Oracle(2, S, p)
    n = rows.shape[1]
    c1, e1 = o.process(rows[:, :n // 3])
    c2, e2 = o.process(rows[:, n // 3:])
    ev = [a + [fo.pack(fo.unpack(w)[0] + n // 3, fo.unpack(w)[1]) for w in b] for a, b in zip(e1, e2)]
    st = o.state()
    checked = 0
    for a, j in ((0, 0), (0, S // 2 + 1), (1, S // 2 - 2), (1, S - 1)):
        sc = fo.Scalar(S, j, p)
        got = [fo.pack(i, e) for i, e in ((i, sc.step(y)) for i, y in enumerate(rows[a])) if e is not None]
        F = a * S + j
        assert got == ev[F], (a, j)
        s2 = sc.state()
        assert all(fbits(st[k][F]) == fbits(s2[k]) for k in fo.FLOATS) and all(st[k][F] == s2[k] for k in fo.INTS), (a, j)
        checked += len(got)
    assert checked >= 40                                           # events were compared, not just silence


@pytest.mark.parametrize("S", (22, 33))
def test_any_cut_gives_the_same_events_and_state_bits(S):
    D = 8
    rows = ideal_rows(S, 2, 9.0, 20 + S)
    n = rows.shape[1] * D                                          # input samples of a channelizer that decimates by D
    one = fo.Oracle(2, S, fo.params(n0=32))
    wc, wev = one.process(rows)
    want = fo.shift_events(wev, 0)
    assert wc.sum() > 100
    rng = np.random.default_rng(S)
    for name, cuts in (("1", [1] * (40 * D) + [n - 40 * D]), ("D - 1", [D - 1] * (n // (D - 1)) + [n % (D - 1)]),
                       ("D + 1", [D + 1] * (n // (D + 1)) + [n % (D + 1)]), ("ragged", cz.random_cuts(n, D, 3)),
                       ("long", [int(v) for v in rng.integers(1, 300 * D, 40)] + [n])):
        o = fo.Oracle(2, S, fo.params(n0=32))
        got = [[] for _ in range(o.nfine)]
        at = empty = 0
        for c in cuts:
            m0, m1 = cz.frame_range(at, min(at + c, n), D)
            at = min(at + c, n)
            empty += m1 == m0
            _, ev = o.process(rows[:, m0:m1])
            for F, e in enumerate(fo.shift_events(ev, m0)):
                got[F] += e
        assert at == n and (empty > 0 or name == "long")
        assert got == want, name
        a, b = o.state(), one.state()
        assert all(np.array_equal(fbits(a[k]), fbits(b[k])) for k in fo.FLOATS) and all(np.array_equal(a[k], b[k]) for k in fo.INTS), name
    # two events of a decoder are never closer than the cap's distance
    gaps = [np.diff([i for i, _ in e]).min() for e in want if len(e) > 1]
    assert min(gaps) >= fo.event_gap(S) and fo.cap_of(256, S) == 256 // (6 * S + S // 2 + 1) + 1


@pytest.mark.parametrize("S", (22, 33))
def test_a_non_finite_or_absurd_row_sample_blanks_exactly_the_outputs_that_reach_it(S):
    rows = ideal_rows(S, 2, 9.0, 30 + S)
    clean = fo.Oracle(2, S, fo.params())
    PS0, PM0 = clean.powers(rows)
    dirty = rows.copy()
    spots = {(0, 300): complex(np.nan, 0.5), (1, 700): complex(0.5, -np.inf), (0, 1000): complex(3e19, 0), (0, 1300): complex(1e9, 0)}
    for (a, k), v in spots.items():
        dirty[a, k] = v
    o = fo.Oracle(2, S, fo.params())
    with np.errstate(all="ignore"):
        PS, PM = o.powers(dirty)
    assert np.isfinite(PS).all() and np.isfinite(PM).all()
    for a in range(2):
        blank = np.zeros(rows.shape[1], bool)
        for (b, k), v in spots.items():
            if a == b and not abs(v) == 1e9:                      # 1e9: power 1e18 g^2 < pmax, not blanked
                blank[k:k + S] = True
        for F in range(a * S, (a + 1) * S):
            keep = ~blank
            keep[1300:1300 + S] = False
            for P, P0 in ((PS, PS0), (PM, PM0)):
                assert np.array_equal(P[F] == 0, blank), (a, F)
                assert np.array_equal(fbits(P[F][keep]), fbits(P0[F][keep]))
    # the state stays finite through the whole decoder, and what follows the last window equals a clean run from there
    with np.errstate(all="ignore"):
        o.process(dirty[:, :1400])
    st = o.state()
    assert all(np.isfinite(st[k]).all() for k in fo.FLOATS)
    twin = fo.Oracle(2, S, fo.params())
    twin.set_state(st, rows[:, 1400 - (S - 1):1400], 1400)
    c1, e1 = o.process(dirty[:, 1400:])
    c2, e2 = twin.process(rows[:, 1400:])
    assert e1 == e2 and c1.sum() > 50


# ---- behind the channelizer --------------------------------------------------------------------------------------------

def channels_of(place):
    return (31, 3) if place == "wrap" else (3, 3)


def station_freq(place, fs, S, M):
    """Hz of the station (the midpoint of its tones) and the fine rows that may own it"""
    ff = fo.fine_freqs(fs, M, S, channels_of(place))
    F = {"centre": S + S // 2 + 2, "between": S + S // 2 + 2, "first": S, "last": 2 * S - 1, "wrap": S}[place]
    if place == "between":
        return ff[F] + BAUD / 8, (F, F + 1)
    return ff[F], (F,)


def rows_behind_the_channelizer(x, fs, S, D, M, channels):
    from pysdr_amd import fsk
    h = fsk.prototype(fs, M, S)
    m1 = -(-len(x) // D)
    return cz.polyphase(x, h, M, D, 0, m1, fo.rows_of(M, channels)).astype(np.complex64)


def read(case, place, snr, seed, stop=1.5, text=MESSAGE, second=None, late=0.0, lead="", **how):
    """one station (and a second one `second` Hz above it) behind the float64 channelizer -> the oracle skimmer.  The
    station idles on mark from the stream's first sample, or from `late` seconds on, and sends `lead` in front of the text."""
    fs, S, D, M = case
    f, homes = station_freq(place, fs, S, M)
    rng = np.random.default_rng(seed)
    x = fo.rtty_baseband(fo.baudot_codes(lead + text), fs, f, stop=stop, preamble=3.0 + rng.uniform(0, 1 / BAUD), tail=0.5,
                         phase=rng.uniform(0, 6.28))                             # any bit phase against the frames
    if second is not None:
        s2 = fo.rtty_baseband(fo.baudot_codes(lead + text[::-1]), fs, f + second, stop=2.0, preamble=3.4, tail=0.5, phase=1.0)
        n = max(len(x), len(s2))
        x = np.pad(x, (0, n - len(x))) + np.pad(s2, (0, n - len(s2)))
    x = np.concatenate((np.zeros(int(late * fs)), x))
    sg = fo.noise_sigma(snr, BAUD, fs)
    x = x + sg * (rng.standard_normal(len(x)) + 1j * rng.standard_normal(len(x)))
    rows = rows_behind_the_channelizer(x, fs, S, D, M, channels_of(place))
    sk = fo.Skimmer(3, S, False, **how)
    sk.push(rows)
    sk.rows = rows
    return sk, homes, fo.fine_freqs(fs, M, S, channels_of(place))


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("case", CASES, ids=["8000", "12000"])
def test_one_station_is_read_whole_on_its_owner(case, place):
    """15 dB with 1 stop bit, 20 dB with 1.5, 30 dB with 2: on a decoder's centre, half way between two decoders, on the
    first and the last decoder of a row and across the wrap of the channel range.  Nothing but the owner speaks: the
    neighbours that frame the same text (up to 8 steps away) and the images 15 steps away lose to it in the finder."""
    for snr, stop in STOPS.items():
        sk, homes, ff = read(case, place, snr, int(snr) + PLACES.index(place), stop)
        said = {F: t for F, t in sk.text.items() if t}
        print(f"fs {case[0]} {place} {snr} dB, {stop} stop bits: homes {homes}", said)
        assert any(MESSAGE in said.get(F, "") for F in homes), (snr, homes, said)
        assert all(min(abs(F - H) for H in homes) <= 1 for F in said), (snr, homes, said)


@pytest.mark.parametrize("case", CASES, ids=["8000", "12000"])
def test_weak_stations_are_reported_not_asserted(case):
    for place in ("centre", "between"):
        for snr in (10.0, 12.0):
            got = []
            for trial in range(2):
                sk, homes, ff = read(case, place, snr, 100 * trial + int(snr))
                got.append(any(MESSAGE in sk.text.get(F, "") for F in homes))
            print(f"fs {case[0]} {place} {snr} dB: whole message read in {sum(got)} of {len(got)}")


@pytest.mark.parametrize("case", CASES, ids=["8000", "12000"])
def test_two_stations_250_hz_apart_are_both_read(case):
    """250 Hz is 22 steps of the raster, a reach of 16 ends short of the other station.  Both stations idle on mark for 3 s,
    send RYRY and then their texts, the upper one the lower one's backwards; both are read whole, RYRY included
    (asserted).  Printed, DESIGN.md 3 item 21: the same without RYRY, where the upper station's text begins with K, a
    character of one space bit, which the balance of a decoder that met the start of the stream refuses (5 of 8 runs);
    and both stations coming on half a second into the stream, where the upper one's idle image 15 steps up ties with
    its own decoder and the K was lost in 5 of 8 runs.  A reach of 12, which leaves the images out, runs beside each:
    it saves that K, and lets an image speak now and then."""
    fs, S, D, M = case
    for how in (dict(), dict(late=0.5)):
        plain, homes, ff = read(case, "first", 20.0, 77, second=250.0, **how)
        near = fo.Skimmer(3, S, False, reach=12)
        near.push(plain.rows)
        print(f"two stations, no RYRY, {how}: reach 16", {F: t for F, t in plain.text.items() if t}, "reach 12", {F: t for F, t in near.text.items() if t})
    sk, homes, ff = read(case, "first", 20.0, 77, second=250.0, lead="RYRY ")
    near = fo.Skimmer(3, S, False, reach=12)
    near.push(sk.rows)
    said = {F: t for F, t in sk.text.items() if t}
    print("two stations: reach 16", said, "reach 12", {F: t for F, t in near.text.items() if t})
    assert fo.REACH == 16 and any("RYRY " + MESSAGE in said.get(F, "") for F in homes)
    other = [F for F in said if abs(ff[F] - (ff[homes[0]] + 250.0)) <= BAUD / 8]
    assert other == [homes[0] + 22] and "RYRY " + MESSAGE[::-1] in said[other[0]], said
    assert set(said) == {homes[0], homes[0] + 22}


@pytest.mark.parametrize("case", CASES, ids=["8000", "12000"])
def test_figures_and_letters_make_the_round_trip(case):
    text = "RST 599 599 K"
    assert fo.baudot_codes(text).count(27) == 1 and fo.baudot_codes(text).count(31) == 1
    sk, homes, ff = read(case, "centre", 20.0, 9, text=text)
    assert sk.text.get(homes[0]) == text, sk.text
    shifts = fo.Skimmer(3, case[1], False)                        # the events carry the shifts, the text leaves them out
    said = [c for _, F, c in shifts.push(sk.rows) if F == homes[0]]
    assert said.count("<FIGS>") == 1 and said.count("<LTRS>") == 1 and "".join(c for c in said if c[0] != "<") == text


@pytest.mark.parametrize("case", CASES, ids=["8000", "12000"])
def test_sixty_seconds_of_noise_give_no_event(case):
    """No event on any fine row, owner or not, and no decoder found open at the end of any call."""
    fs, S, D, M = case
    rng = np.random.default_rng(int(fs))
    n = int(60 * fs)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    rows = rows_behind_the_channelizer(x, fs, S, D, M, (3, 3))
    sk = fo.Skimmer(3, S, False)
    sk.push(rows)
    st = sk.o.state()
    with np.errstate(all="ignore"):
        print(f"fs {fs}: {sk.nevents} events on {sk.o.nfine} fine rows, largest contrast at the end {np.max(st['qn'] / st['qd']):.3f}, "
              f"{sk.nopen} open decoders at the ends of the calls")
    assert sk.nevents == 0 and not sk.text and sk.nopen == 0


@pytest.mark.parametrize("case", CASES, ids=["8000", "12000"])
def test_a_keyed_carrier_on_the_mark_tone_gives_no_event(case):
    """A 25 dB carrier keyed at 8 Hz where a decoder's mark tone lies: its contrast is that of a station, but its space tone
    holds noise alone, which the balance of the two levels refuses -- on that decoder and on the skirts of the carrier."""
    fs, S, D, M = case
    f, homes = station_freq("centre", fs, S, M)
    rng = np.random.default_rng(8)
    n = np.arange(int(20 * fs))
    x = ((n * 8.0 / fs) % 1.0 < 0.5) * np.exp(2j * np.pi * (f + 15 * BAUD / 8) / fs * n)
    x = x + fo.noise_sigma(25.0, BAUD, fs) * (rng.standard_normal(len(n)) + 1j * rng.standard_normal(len(n)))
    rows = rows_behind_the_channelizer(x, fs, S, D, M, (3, 3))
    sk = fo.Skimmer(3, S, False)
    sk.push(rows)
    print(f"fs {fs}: {sk.nevents} events, {sk.nopen} open decoders at the ends of the calls")
    assert sk.nevents == 0 and not sk.text and sk.nopen == 0
