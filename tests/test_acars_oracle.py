"""The ACARS skimmer's definition on the CPU: the helpers of pysdr_amd/acars.py, and the float32
oracle of steps 1 to 8 (tests/acars_oracle.py) reading every planted block -- behind the float64 channelizer model
(tests/channelizer_oracle.py), and on clean rows for the framing cases.  The GPU tests hold the kernel equal to this
oracle; that the oracle reads what was sent is shown here, so that they cannot pass on silence.  No device."""
import functools

import numpy as np
import pytest

from tests import acars_oracle as ao
from tests import channelizer_oracle as cz

# The lowest C/N of the carrier in the row bandwidth at which this oracle, behind the float64 channelizer, read every planted
# block (sensitivity(), below: 3 stations x 8 seeds per level in steps of 1 dB; every level from there up to 13 dB read all
# 24 too; one dB lower 23, 23 and 23 of 24), and the 2 dB above it that the test asserts: DESIGN.md 3 item 32 and the README carry the same figures.
MEASURED_DB = {19200.0: 13.0, 25000.0: 11.0, 50000.0: 8.0}
MARGIN_DB = 2.0


def ac():
    from pysdr_amd import acars
    return acars


def chars(k=0, n_text=40, **kw):
    a = ac()
    if k % 2:
        return a.frame("2", f"N{100 + k}AB", None, "H1", str(k % 10), (f"M{k:02d}AXX{k:04d}" + "POS N49035W072017,KJFK,1234,350 " * 8)[:n_text], **kw)
    return a.frame("2", f"G-AB{chr(65 + k % 26)}D", "A", "_d", chr(65 + k % 26), ("UPLINK " * 40)[:n_text], **kw)


def block_of(c):
    return c[c.index(b"\x16\x16\x01") + 3:-3]


def heard(o, ev, m0=0):
    """the oracle's events of one call -> {(row, absolute m): bytes}"""
    return {(d, m0 + i): data for d in range(o.nd) for i, data in ao.unpack(ev[d])}


def row_signal(c, fs_out, cn=None, depth=0.8, lead=0.02, tail=0.02, seed=0, invert=False, off=0.0):
    """one row at fs_out with one transmission `off` Hz from its centre: complex64 [1][n]; cn None: no noise"""
    s = ac().waveform(c, fs_out, off, depth=depth, invert=invert)
    n = len(s) + int((lead + tail) * fs_out)
    if cn is None:
        x = np.zeros(n, np.complex64)
        x[int(lead * fs_out):int(lead * fs_out) + len(s)] = 0.1 * s
        return x[None, :]
    return ao.scene(fs_out, n, [(c, off, cn, depth, int(lead * fs_out), invert)], fs_out, ac().waveform, seed)[None, :]


# ---- the helpers -------------------------------------------------------------------------------------------------------
def test_parity_crc_and_the_residue_of_every_block():
    a = ac()
    assert a.parity(b"\x16\x01+*\x7f\x03") == b"\x16\x01\xab\x2a\x7f\x83"
    assert all(bin(b).count("1") & 1 for b in a.parity(bytes(range(128))))
    assert a.crc16(b"123456789") == 0x2189                                  # CRC-16/KERMIT
    rng = np.random.default_rng(1)
    for k in range(40):
        b = a.block("2", f"N{k}", None, "H1", "1", bytes(rng.integers(32, 127, k * 5, dtype=np.uint8)))
        bcs = int(a.crc16(b)).to_bytes(2, "little")
        assert a.crc16(b + bcs) == 0 and a.crc16(b[:-1] + bytes([b[-1] ^ 1]) + bcs) != 0


def test_frame_parse_and_line_round_trip():
    a = ac()
    c = a.frame("2", "N123AB", None, "H1", "3", "M01AUA0123HELLO", prekey=4)
    assert c[:4] == b"\xff" * 4 and c[4:9] == b"\xab\x2a\x16\x16\x01" and c[-1] == 0x7F and len(c) == 4 + 5 + 29 + 3
    b = block_of(c)
    assert b == a.block("2", "N123AB", None, "H1", "3", "M01AUA0123HELLO") and a.crc16(b + c[-3:-1]) == 0
    rec = a.parse(b)
    assert rec == dict(mode="2", address="N123AB", ack="", label="H1", block_id="3", more=False, msn="M01A", flight="UA0123", text="HELLO")
    assert a.line(rec) == " N123AB 2 H1 3 ! M01A UA0123 HELLO"
    up = a.parse(a.block("2", "G-ABCD", "A", "_d", "B", "HI THERE", more=True))
    assert up == dict(mode="2", address="G-ABCD", ack="A", label="_d", block_id="B", more=True, msn=None, flight=None, text="HI THERE")
    assert a.line(up) == " G-ABCD 2 _d B A HI THERE +"
    short = a.block("2", "N1", None, "Q0", "1")
    assert len(short) == 13 and a.parse(short)["text"] == "" and a.parse(short)["address"] == "N1"
    assert len(a.block("2", "N1", None, "H1", "1", "x" * 220)) == 234 <= a.MAX_BYTES
    assert a.parse(short[:-1]) is None and a.parse(b"\x01" * 20) is None and a.line(None) == "?"
    for bad in (dict(mode="22"), dict(address="TOOLONGREG"), dict(label="H"), dict(block_id=""), dict(text="x" * 221), dict(ack="AA"), dict(text="\xe9")):
        kw = dict(mode="2", address="N1", ack=None, label="H1", block_id="1", text="")
        kw.update(bad)
        with pytest.raises(ValueError):
            a.block(**kw)


def test_bits_audio_and_waveform():
    a = ac()
    assert list(a.bits(b"\x16\x01")) == [0, 1, 1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0]
    b = a.bits(b"\xff\x2a")
    au = a.audio(b, 48000.0)
    assert len(au) == 16 * 20 and np.abs(au).max() <= 1.0
    # a bit that equals the one before is a whole cycle of 2400 Hz, one that differs half a cycle of 1200 Hz: every bit
    # ends on a zero of the sine, and the signs of the half cycles tell the changes of bit
    assert np.allclose(au[19::20], 0.0, atol=1e-9)
    same = b == np.concatenate(([1], b[:-1]))
    crossings = [int((np.diff(np.sign(au[20 * k:20 * k + 19])) != 0).sum()) for k in range(16)]
    assert crossings == [1 if s else 0 for s in same]
    assert np.allclose(a.audio(b, 48000.0, first=0)[20:], -au[20:], atol=1e-9)          # the other level: half a cycle more
    w = a.waveform(b"\xff" * 4, 96000.0, 5000.0, depth=0.5)
    assert w.dtype == np.complex64 and np.abs(w).max() <= 1.5 + 1e-6 and np.abs(w).min() >= 0.5 - 1e-6
    assert len(a.waveform(b"\xff", 96000.0, 0.0, prekey=3)) == 4 * 8 * 40


def test_tables_params_and_unpack():
    a = ac()
    for fs_out in (19200.0, 20000.0, 25000.0, 48000.0, 50000.0):
        L, tw, c = a.tables(fs_out)
        L2, tw2, c2 = ao.tables(fs_out)
        assert L == L2 == int(np.floor(fs_out / 2400 + 0.5)) and 8 <= L <= 21 and c.shape == (4 * L + 1, 2)
        assert np.array_equal(tw.view(np.uint32), tw2.view(np.uint32)) and np.array_equal(c.view(np.uint32), c2.view(np.uint32))
        assert abs(c.astype(np.float64).sum(axis=0)).max() < 1e-6                # the carrier's null
        resp = lambda f: abs(np.sum((c[:, 0] + 1j * c[:, 1]) * np.exp(-2j * np.pi * f * np.arange(len(c)) / fs_out)))
        assert resp(1200.0) > 0.7 and resp(2400.0) > 0.7 and resp(-1200.0) < 0.05 and resp(-2400.0) < 0.05
        cf, par = a.cfg_dict(a.params(fs_out)), ao.params(fs_out)
        assert (cf["w_car"], cf["w_baud"], cf["pll_shift"]) == (par["w_car"], par["w_baud"], par["pll_shift"]) and cf["pmax"] == float(par["pmax"])
    assert a.window_length(25000.0) == 10 and a.params(19200.0).w_baud == 1 << 29
    words = [(5 << 10) | 5, 0x04030201, 0x05, (9 << 10) | 4, 0x0D0C0B0A]
    assert a.unpack(np.array(words, np.int32)) == ao.unpack(words) == [(5, bytes([1, 2, 3, 4, 5])), (9, bytes([10, 11, 12, 13]))]


# ---- framing, on clean rows --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs_out", (19200.0, 25000.0, 50000.0))
def test_the_shortest_the_longest_an_etb_block_both_directions_and_an_inverted_start(fs_out):
    """the 13-byte block, a text of 220 characters, an ETB block, an uplink and a downlink, AM depth 0.5 and 0.9, one
    transmission whose tones start from the other level, all in one row, each read once and nothing else"""
    a = ac()
    sent = [(a.frame("2", "N1", None, "Q0", "1"), 0.8, False), (chars(2, 220), 0.5, False), (chars(4, 30, more=True), 0.9, False),
            (chars(6, 50), 0.9, True), (chars(7, 60), 0.5, False), (chars(9, 45, prekey=3), 0.8, True)]
    y = np.concatenate([row_signal(c, fs_out, depth=d, invert=inv, off=200.0 * k) for k, (c, d, inv) in enumerate(sent)], axis=1)
    o = ao.Oracle(1, fs_out)
    counts, ev = o.process(y)
    got = ao.unpack(ev[0])
    assert [data for _, data in got] == [block_of(c) for c, _, _ in sent]
    assert [len(d) for _, d in got][:2] == [13, 234] and got[2][1][-1] & 0x7F == 0x17
    assert a.parse(got[4][1])["flight"] == "XX0007" and a.parse(got[3][1])["msn"] is None
    assert counts.max() <= ao.cap_of(y.shape[1], o.par["w_baud"])
    assert o.state()["st"][0] == 0 and (o.state()["nbytes"] <= 240).all()


def test_blocks_outside_the_definition_are_not_read():
    """239 bytes, 12 bytes, a missing SOH, a character of even parity"""
    a = ac()
    fs_out = 25000.0
    good = a.block("2", "N1", None, "H1", "1", "x" * 220)

    def sent(body, soh=b"\x01"):
        return b"\xff" * 8 + a.parity(b"+*\x16\x16") + soh + body + int(a.crc16(body)).to_bytes(2, "little") + b"\x7f"

    long_ = good[:-1] + a.parity(b"abcde\x03")
    assert len(long_) == 239
    ok = good[:-1] + a.parity(b"abcd\x03")
    even = bytearray(good)
    even[50] ^= 0x80
    cases = [sent(ok), sent(long_), sent(a.parity(b"2.....N1\x15H1\x03")), sent(good, soh=b"\x02"), sent(bytes(even)), sent(good)]
    y = np.concatenate([row_signal(c, fs_out) for c in cases], axis=1)
    o = ao.Oracle(1, fs_out)
    counts, ev = o.process(y)
    assert [data for _, data in ao.unpack(ev[0])] == [ok, good]


@functools.lru_cache(maxsize=None)
def noisy_row(fs_out=25000.0):
    y = np.concatenate([row_signal(chars(k, 20 + 9 * k), fs_out, cn=16.0, depth=d, seed=k, invert=bool(k & 1))
                        for k, d in enumerate((0.8, 0.5, 0.9))], axis=1)
    y.setflags(write=False)
    o = ao.Oracle(1, fs_out)
    counts, ev = o.process(y)
    return y, heard(o, ev), o.state()


def test_any_cut_of_the_stream_gives_the_same_events_and_state():
    fs_out = 25000.0
    y, want, state = noisy_row(fs_out)
    assert sorted(want.values()) == sorted(block_of(chars(k, 20 + 9 * k)) for k in range(3))
    rng = np.random.default_rng(5)
    for trial in range(3):
        o, got, at = ao.Oracle(1, fs_out), {}, 0
        cuts = [0, 1, 1, 63, 64, 65, 0, 16] if trial == 0 else []
        while at < y.shape[1]:
            n = cuts.pop(0) if cuts else int(rng.integers(0, (40, 700, 5000)[trial]))
            m0 = o.m
            counts, ev = o.process(y[:, at:at + n])
            assert counts.max(initial=0) <= ao.cap_of(max(n, 1), o.par["w_baud"])
            got.update(heard(o, ev, m0))
            at += n
        assert got == want
        st = o.state()
        assert all(np.array_equal(st[k], state[k]) for k in st), trial


def test_one_flipped_bit_anywhere_means_the_block_is_not_read():
    """every bit of a 20-byte block and of its check, one at a time, as the sender's bit (two tones change) -- the parity
    rule or the check catches each -- and a sample of single tone errors, which invert every bit behind them"""
    a = ac()
    fs_out = 25000.0
    c = a.frame("2", "N77", "B", "H1", "4", "SEVENS", prekey=6)
    at = c.index(b"\x16\x16\x01") + 3
    assert len(block_of(c)) == 20
    rows, n = [], None
    for k in range(8 * 22):
        bad = bytearray(c)
        bad[at + k // 8] ^= 1 << (k % 8)
        rows.append(row_signal(bytes(bad), fs_out)[0])
    bits = a.bits(c)
    for k in range(8 * at, 8 * (at + 22), 5):                                  # a tone error at bit k: every later bit is inverted
        b = bits.copy()
        b[k:] ^= 1
        rows.append(row_signal(np.packbits(b, bitorder="little").tobytes(), fs_out)[0])
    rows.append(row_signal(c, fs_out)[0])
    o = ao.Oracle(len(rows), fs_out)
    counts, ev = o.process(np.stack(rows))
    assert counts[-1] == 1 + 5 and not counts[:-1].any()


def test_a_nan_and_an_inf_blank_only_their_windows():
    fs_out = 25000.0
    y, want, _ = noisy_row(fs_out)
    L = 10
    NT = 4 * L + 1
    bad = np.array(y)
    k1, k2 = 2000, 2400                                                   # inside the first block, and further on in it
    bad[0, k1] = complex(np.nan, 0.5)
    bad[0, k2] = complex(0.25, -np.inf)
    zeroed = np.array(y)
    zeroed[0, [k1, k2]] = 0
    a, b, z = ao.Oracle(1, fs_out), ao.Oracle(1, fs_out), ao.Oracle(1, fs_out)
    qa, qb, qz = a.detector(y), b.detector(bad), z.detector(zeroed)
    touched = np.zeros(y.shape[1], bool)
    for k in (k1, k2):
        touched[k:k + NT + L] = True                                      # a[k .. k + NT - 1], each in q at itself and L later
    assert np.isfinite(qb).all() and np.array_equal(qb.view(np.uint32), qz.view(np.uint32))   # blanked: the sample's power is 0
    assert np.array_equal(qa[0, ~touched].view(np.uint32), qb[0, ~touched].view(np.uint32))
    assert (qa[0, touched] != qb[0, touched]).sum() > 1.8 * (NT + L)                          # and the windows are NT + L long
    for k in (k1, k2):
        assert qa[0, k] != qb[0, k]
    counts, ev = b.process(bad)
    got = set(heard(b, ev).values())                                       # one sample's power is little to a window of four bits
    assert set(want.values()) - {block_of(chars(0, 20))} <= got <= set(want.values())


def test_an_unmodulated_carrier_a_voice_like_signal_and_noise_give_no_block():
    """a bare carrier keyed on and off, band-limited noise at AM depth 0.8 (300 - 3000 Hz), both at 30 dB C/N, and 60
    row-seconds of white noise: 8 rows of 7.5 s at 19.2 kHz.  A block check is reached only behind SYN SYN SOH, 13 or
    more characters of odd parity and an ETX, and then passes with probability 2^-16; the count is printed."""
    from scipy.signal import firwin
    fs_out, rows, secs = 19200.0, 8, 7.5
    rng = np.random.default_rng(77)
    n = int(secs * fs_out)
    y = (0.01 * (rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n)))).astype(np.complex64)
    t = np.arange(n) / fs_out
    car = 0.01 * np.sqrt(2) * 10 ** (30 / 20)
    y[1] += (car * (np.floor(t / 0.7) % 2) * np.exp(2j * np.pi * 300.0 * t)).astype(np.complex64)
    voice = np.convolve(rng.standard_normal(n), firwin(255, [300.0, 3000.0], pass_zero=False, fs=fs_out), "same")
    voice *= 0.8 / np.abs(voice).max()
    y[2] += (car * (1 + voice) * np.exp(-2j * np.pi * 500.0 * t)).astype(np.complex64)
    o = ao.Oracle(rows, fs_out)
    total = 0
    for at in range(0, n, 4096):
        counts, ev = o.process(y[:, at:at + 4096])
        total += int(counts.sum())
    print(f"noise: {rows * secs:.0f} row-seconds, {o.bcs_checks} block checks reached: {o.bcs_checks * 2.0 ** -16:.2e} false blocks expected")
    assert total == 0


# ---- behind the channelizer ----------------------------------------------------------------------------------------------
CASES = {19200.0: (153600.0, 16, 8), 25000.0: (200000.0, 16, 8), 50000.0: (400000.0, 16, 8)}


def planted(fs_out, cn, seed, off=0.0, sent=None):
    """three stations `off` Hz off the centres of channels 2, 5 and 8 at `cn` dB, through the float64 channelizer with the
    skimmer's prototype -> (the oracle's {(row, m): bytes} over channels 1 to 9, the blocks planted as (bytes, row));
    ``sent``: other transmissions, as (characters, channel, depth, inverted)"""
    a = ac()
    fs, M, D = CASES[fs_out]
    if sent is None:
        sent = [(chars(3 * k + seed % 5, 25 + 5 * k, prekey=12), ch, depth, inv) for k, (ch, depth, inv) in enumerate(((2, 0.5, False), (5, 0.8, True), (8, 0.9, False)))]
    n = int(0.02 * fs) + 777 * 3 + max(len(a.waveform(c, fs, 0.0)) for c, _, _, _ in sent) + int(0.01 * fs)
    stations = [(c, ch * fs / M + off, cn, depth, int(0.02 * fs) + 777 * k, inv) for k, (c, ch, depth, inv) in enumerate(sent)]
    x = ao.scene(fs, n, stations, fs_out, a.waveform, seed=seed)
    ks = np.arange(1, 10)
    y = cz.polyphase(x, a.prototype(fs, M, D), M, D, 0, -(-n // D), ks=ks).astype(np.complex64)
    o = ao.Oracle(len(ks), fs_out)
    counts, ev = o.process(y)
    return heard(o, ev), [(block_of(c), ch - 1) for c, ch, _, _ in sent]


def sensitivity(fs_out, levels=range(14, 3, -1), seeds=range(8)):
    """blocks read of those planted, per level: what MEASURED_DB was read from (python -c 'from tests.test_acars_oracle
    import *; print(sensitivity(25000.0))')"""
    out = {}
    for cn in levels:
        good = total = 0
        for seed in seeds:
            got, sent = planted(fs_out, float(cn), 1000 + seed)
            good += sum(1 for data, row in sent if (data, row) in {(v, d) for (d, m), v in got.items()})
            total += len(sent)
        out[cn] = (good, total)
    return out


@pytest.mark.parametrize("fs_out", (19200.0, 25000.0, 50000.0))
@pytest.mark.parametrize("off", (0.0, 800.0, -800.0))
def test_every_planted_block_is_read_on_its_home_row_only(fs_out, off):
    """depth 0.5, 0.8 and 0.9, one inverted, `off` Hz off their rows' centres, at 2 dB over the measured level"""
    cn = MEASURED_DB[fs_out] + MARGIN_DB
    got, sent = planted(fs_out, cn, int(fs_out + off) % 1000, off)
    print(f"fs_out {fs_out} off {off} C/N {cn} dB: {sorted((d, m) for d, m in got)}")
    assert sorted((v, d) for (d, m), v in got.items()) == sorted(sent)       # every block once, on its home row, and nothing else


def test_the_framing_cases_behind_the_channelizer():
    """the 13-byte block, a text of 220 characters on an inverted start and an ETB downlink, at depth 0.5, 0.9 and 0.8, on
    25 kHz rows at 20 dB (framing, not sensitivity: a block of 234 bytes has five times the bits of those the measured
    level was read from): each once, on its home row, and nothing else"""
    a = ac()
    sent = [(a.frame("2", "N1", None, "Q0", "1", prekey=12), 2, 0.5, False), (chars(2, 220, prekey=12), 5, 0.9, True),
            (chars(7, 60, more=True, prekey=12), 8, 0.8, False)]
    got, want = planted(25000.0, 20.0, 7, 300.0, sent)
    assert sorted((v, d) for (d, m), v in got.items()) == sorted(want) and sorted(len(v) for v, _ in want) == [13, 74, 234]


# ---- the host's rule -------------------------------------------------------------------------------------------------------
def test_copies_on_neighbour_rows_become_one_record_whatever_the_cut():
    """packet.Dedup, reused unchanged with one decoder per row, against the oracle skimmer's rule"""
    from pysdr_amd import packet
    fs, fs_out, L = 200000.0, 25000.0, 10
    freqs = (np.arange(12) - 3) * 6250.0                                  # rows 6.25 kHz apart: one to either side is near
    near = packet.near_rows(freqs, fs, fs_out)
    rng = np.random.default_rng(9)
    raw, m = [], 100
    for k in range(60):
        m += int(rng.integers(1, 400))
        data, row = bytes([k % 5]) * 20, int(rng.integers(0, 12))
        for r in range(max(0, row - 1), min(12, row + 2)):
            if rng.integers(0, 3):
                raw.append((m + int(rng.integers(0, 3)), r, data))
    raw.sort()
    end = raw[-1][0] + 200
    results = []
    for step in (1 << 30, 4096, 97, 16):
        a, b = packet.Dedup(4 * L, near), ao.Skimmer(12, fs, fs_out, freqs)
        got, want = [], []
        for m0 in range(0, end, min(step, end)):
            part = [q for q in raw if m0 <= q[0] < m0 + step]
            got += a.add([(m_, r, 0, d) for m_, r, d in part], min(m0 + step, end))
            want += b.take(part, min(m0 + step, end))
        got += a.flush()
        want += b._leave(lambda st: True)
        assert [(m_, r, d) for m_, r, d, _ in got] == want == b.frames
        results.append(got)
    assert all(r == results[0] for r in results) and 30 < len(results[0]) < len(raw)
