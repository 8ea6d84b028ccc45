"""The CW skimmer's definition on the CPU: the vectorised float32 oracle (tests/cw_oracle.py) against
the scalar transcription of steps 1 to 8, any cut of a stream against the whole stream, and what the definition reads:
keyed carriers behind the float64 channelizer (tests/channelizer_oracle.Definition) at 15 to 30 wpm and 25 / 35 dB, and
nothing at all in 60 s of noise.  No GPU, no library: the settings and the Morse table are pysdr_amd.cw's, pure Python."""
import functools

import numpy as np
import pytest

from tests import channelizer_oracle as cz
from tests import cw_oracle as co

FS = 48000.0
SHAPES = [(64, 32), (256, 128)]
HOME = {64: 5, 256: 219}                  # the second: a negative frequency, (219 - 256) fs / M
ASSERTED_WPM = (15, 20, 25, 30)
OFFSETS = (0.1, 0.3)
SNRS = (25.0, 35.0)


def taps(M):
    from pysdr_amd.design import channelizer_taps
    return channelizer_taps(M)


def sigma_for(snr_db, h):
    """per-component noise sigma that puts a unit-amplitude carrier snr_db above the channel's noise: channel SNR =
    carrier power / (noise power sum(h^2)), noise power = 2 sigma^2"""
    return float(np.sqrt(1.0 / (10 ** (snr_db / 10) * np.sum(np.asarray(h) ** 2) * 2.0)))


def home_row(M, D, wpm, off, snr, seed, total):
    """one keyed carrier `off` of a spacing above the centre of channel HOME[M], in noise, `total` samples: the home
    channel's complex64 row"""
    from pysdr_amd.cw import morse_keying
    h = taps(M)
    k = HOME[M]
    f = ((k - M if k >= M // 2 else k) + off) * FS / M
    x = co.keyed_carrier(co.MESSAGE, wpm, FS, f, 1.0, 0.5, 0.0, morse_keying, phase=0.3 * seed)
    assert len(x) <= total
    x = np.concatenate((x, np.zeros(total - len(x), np.complex128)))
    rng = np.random.default_rng(seed)
    x = x + sigma_for(snr, h) * (rng.standard_normal(total) + 1j * rng.standard_normal(total))
    return cz.Definition(h, M, D, ks=[k]).process(x)[0].astype(np.complex64)


@functools.lru_cache(maxsize=None)
def read(M, D, wpm, cases):
    """the text the oracle reads on the home channel of every (off, snr) of `cases`, and its speed estimate"""
    from pysdr_amd.cw import code_text, morse_keying
    total = int(len(morse_keying(co.MESSAGE, wpm, FS)) + (0.5 + 12 * 1.2 / wpm) * FS)      # the tail: 12 dots of key-up
    rows = np.stack([home_row(M, D, wpm, off, snr, 17 * i + wpm, total) for i, (off, snr) in enumerate(cases)])
    o = co.Oracle(len(cases), co.params(FS / D, settle=co.settle_samples(len(taps(M)), D, FS / D)))
    _, ev = o.process(rows)
    return [co.text_of(e, code_text) for e in ev], 19.2 * (FS / D) / o.dot


def small_case(R=375.0, n=3000, seed=5, settle=1):
    """six channel-rate rows: keyed envelopes at 18 / 27 / 40 wpm in noise, noise alone, a steady carrier, and a row with a
    NaN, an inf, an overflowing and a denormal sample"""
    from pysdr_amd.cw import morse_keying
    rng = np.random.default_rng(seed)
    rows = 0.01 * (rng.standard_normal((6, n)) + 1j * rng.standard_normal((6, n)))
    for a, wpm in enumerate((18, 27, 40)):
        k = co.shaped_keying(morse_keying("CQ TEST K1ABC 5NN", wpm, R), R)[:n - 200]
        rows[a, 200:200 + len(k)] += (0.3 + 0.4 * a) * k * np.exp(1j * 0.2 * np.arange(len(k)))
    rows[4] += 0.5
    k = co.shaped_keying(morse_keying("TEST TEST", 25, R), R)[:n - 300]
    rows[5, 300:300 + len(k)] += k
    rows = rows.astype(np.complex64)
    rows[5, 700] = complex(np.nan, 1.0)
    rows[5, 900] = complex(1.0, np.inf)
    rows[5, 1100] = complex(3e19, 3e19)               # re^2 + im^2 overflows float32
    rows[5, 1300] = complex(1e-30, 0.0)
    return rows, co.params(R, settle=settle)


def same_state(a, b):
    for k in co.FLOATS:
        assert np.array_equal(np.asarray(a[k], np.float32).view(np.uint32), np.asarray(b[k], np.float32).view(np.uint32)), k
    for k in co.INTS:
        assert np.array_equal(np.asarray(a[k], np.int64), np.asarray(b[k], np.int64)), k


def test_settings_and_table():
    from pysdr_amd import cw
    for R in (375.0, 1500.0, 3000.0, 187.5, 48000.0, 100.0):
        n0 = 1 if R < 200 else co.settle_samples(int(R), 7, R)
        assert n0 == cw.settle_samples(int(R), 7, R) or R < 200
        want, got = co.params(R, settle=n0), cw.cfg_dict(cw.params(R, settle=n0))
        assert set(want) == set(got)
        for k, v in want.items():
            if isinstance(v, np.float32):
                assert np.float32(got[k]).view(np.uint32) == v.view(np.uint32), (R, k)
            else:
                assert got[k] == v, (R, k)
    assert co.params(375.0)["d0"] == 360 and co.params(100.0)["dmin"] == 32 and co.params(20.0)["dmin"] == 16
    assert cw.code_text(0b101) == "A" and cw.code_text(0b11000) == "B" and cw.code_text(0b10) == "E" and cw.code_text(0b11) == "T"
    assert cw.code_text(0b101111) == "1" and cw.code_text(0b110010) == "/" and cw.code_text(0b1001100) == "?"
    assert cw.code_text(0) == "*" and cw.code_text(255) == "*" and cw.code_text(cw.WORD_SPACE) == " " and cw.code_text(1) == "*"
    assert len(cw.MORSE) == 26 + 10 + 5 and set("/?=.,") <= set(cw.MORSE.values())
    # 1 : 3 : 1 : 3 : 7 -- "EE T  E" style timing, 10 samples per dot
    k = cw.morse_keying("AE T", 12, 100.0)                # dot = 0.1 s = 10 samples
    runs = np.flatnonzero(np.diff(np.concatenate(([0], k, [0]))))
    assert list(np.diff(runs)) == [10, 10, 30, 30, 10, 70, 30]
    assert cw.unpack(co.pack(1023, 256)) == (1023, 256) and co.unpack(co.pack((1 << 21) - 1, 255)) == ((1 << 21) - 1, 255)


def test_one_settling_sample_is_the_first_sample_seed():
    """Steps 1 to 6 with the floor seeded by the first sample alone (`if seen == 0: nf = s, seen = 1`, then steps 4 to 6 on
    that sample as on any other) give, operation by operation, what n0 = 1 gives: floats by their bits and every key
    decision, on rows that start in noise, on a carrier, on zeros and on a non-finite sample."""
    f = np.float32
    rows, p = small_case(n=1500, settle=1)
    rows = rows.copy()
    rows[3, :4] = 0
    rows[5, 0] = complex(np.inf, 1.0)
    for a, row in enumerate(rows):
        ref = co.Scalar(p)
        s = pk = nf = f(0)
        seen = key = 0
        for y in row:
            with np.errstate(all="ignore"):
                re, im = f(y.real), f(y.imag)
                pw = f(f(re * re) + f(im * im))
                if not pw <= co.FLT_MAX:
                    pw = s
                s = f(s + f(p["a_s"] * f(pw - s)))
                if seen == 0:
                    nf, seen = s, 1
                pk = s if s > pk else f(pk + f(p["a_p"] * f(s - pk)))
                A, B = f(nf * pk), f(f(pk * pk) * p["fl"])
                q = A if A > B else B
                u = f(s * s)
                pres = pk > f(p["snr_min"] * nf)
                new = int(bool(pres and (u >= f(q * p["lo"]) if key else u > f(q * p["hi"]))))
                if new == 0:
                    c = min(s, f(f(f(4) * nf) + f(1e-30)))
                    nf = f(nf + f(p["a_n"] * f(c - nf)))
            key = new
            ref.step(y)
            got = ref.state()
            assert got["key"] == key and got["seen"] == 1, a
            assert [f(got[k]).view(np.uint32) for k in co.FLOATS] == [f(v).view(np.uint32) for v in (s, pk, nf)], a


@pytest.mark.parametrize("settle", [1, 24])
def test_vectorised_oracle_equals_the_scalar_transcription(settle):
    rows, p = small_case(settle=settle)
    o = co.Oracle(len(rows), p)
    counts, ev = o.process(rows)
    assert counts.sum() > 20 and counts[3] == 0
    st = o.state()
    assert all(np.isfinite(st[k]).all() for k in co.FLOATS)
    for a, row in enumerate(rows):
        s = co.Scalar(p)
        want = s.process(row)
        assert [co.unpack(w) for w in ev[a]] == want, a
        same_state({k: v[a:a + 1] for k, v in st.items()}, {k: [v] for k, v in s.state().items()})


def test_any_cut_gives_the_same_events_and_state():
    rows, p = small_case(settle=24)
    one = co.Oracle(len(rows), p)
    _, want = one.process(rows)
    want = co.shift_events(want, 0)
    for seed in (1, 2):
        o = co.Oracle(len(rows), p)
        got, at = [[] for _ in rows], 0
        for n in cz.random_cuts(rows.shape[1], 16, seed):
            c, ev = o.process(rows[:, at:at + n])
            assert list(c) == [len(e) for e in ev] and (n > 0 or c.sum() == 0)
            for a, e in enumerate(co.shift_events(ev, at)):
                got[a] += e
            at += n
        assert got == want
        same_state(o.state(), one.state())


@pytest.mark.parametrize("wpm", ASSERTED_WPM)
@pytest.mark.parametrize("M,D", SHAPES, ids=["64-32", "256-128"])
def test_the_oracle_reads_text(M, D, wpm):
    """One keyed carrier per case behind the float64 channelizer, 0.1 and 0.3 of a spacing off the centre, 25 and 35 dB:
    the home channel's text holds the message behind its preamble (the first character after silence may be garbled:
    the dot length and the noise floor are still settling, and that is the definition's behaviour)."""
    cases = tuple((off, snr) for off in OFFSETS for snr in SNRS)
    texts, est = read(M, D, wpm, cases)
    for (off, snr), t, w in zip(cases, texts, est):
        print(f"M {M} D {D} {wpm} wpm, {off} off centre, {snr} dB: {t!r}, estimate {w:.1f} wpm")
    for (off, snr), t in zip(cases, texts):
        assert co.TAIL in t, (off, snr, t)


@pytest.mark.parametrize("M,D", SHAPES, ids=["64-32", "256-128"])
def test_beyond_the_asserted_range_is_printed(M, D):
    """12 and 40 wpm, 15 and 45 dB: reported, not asserted (next to a very strong carrier the key clicks decode as dots, and
    at 15 dB the noise reaches the threshold)"""
    for wpm, cases in ((12, ((0.1, 25.0), (0.3, 35.0))), (40, ((0.1, 25.0), (0.3, 35.0))), (20, ((0.1, 15.0), (0.1, 45.0)))):
        texts, est = read(M, D, wpm, cases)
        for (off, snr), t, w in zip(cases, texts, est):
            print(f"M {M} D {D} {wpm} wpm, {off} off centre, {snr} dB: {'ok ' if co.TAIL in t else 'NOT'} {t!r}, estimate {w:.1f} wpm")


@pytest.mark.parametrize("M,D", SHAPES, ids=["64-32", "256-128"])
def test_noise_alone_gives_no_event(M, D):
    """60 s of complex noise through the channelizer, every row.  The rows come from the float64 polyphase form of
    tests/channelizer_oracle (the Definition's sum regrouped: one pass for all M rows, where the Definition convolves the
    whole stream once per row); that it gives the Definition's rows is checked first, on two rows of the first 20000
    samples."""
    h = taps(M)
    n = int(60 * FS)
    rng = np.random.default_rng(4242 + M)
    x = 0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    ks = [1, M - 3]
    want = cz.Definition(h, M, D, ks=ks).process(x[:20000])
    got = cz.polyphase(x[:20000], h, M, D, 0, want.shape[1], ks=ks)
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
    frames = -(-n // D)
    o = co.Oracle(M, co.params(FS / D, settle=co.settle_samples(len(h), D, FS / D)))
    total = 0
    step = 8192
    for m0 in range(0, frames, step):
        m1 = min(frames, m0 + step)
        lo = max(0, m0 * D - len(h))                                   # the samples these frames reach, from a multiple of M:
        lo -= lo % M                                                   # the channel phases count from sample 0
        rows = cz.polyphase(x[lo:m1 * D], h, M, D, m0 - lo // D, m1 - lo // D)
        counts, _ = o.process(rows.astype(np.complex64))
        total += int(counts.sum())
    st = o.state()
    print(f"M {M} D {D}: 60 s of noise, {total} events; rows ending key-down {int(st['key'].sum())}, with elements pending "
          f"{int((st['code'] != 1).sum())} of {M}; pk / nf at the end: median {np.median(st['pk'] / st['nf']):.2f}, "
          f"largest {np.max(st['pk'] / st['nf']):.2f} (presence needs 16)")
    assert total == 0, total
