"""The packet skimmer's definition on the CPU: the AX.25 helpers of pysdr_amd/packet.py, and the
float32 oracle of steps 1 to 6 (tests/pkt_oracle.py) reading every planted frame -- behind the float64 channelizer model
(tests/channelizer_oracle.py) at 12 dB C/N, and on clean rows for the framing cases.  The GPU tests hold the kernel equal
to this oracle; that the oracle reads what was sent is shown here, so that they cannot pass on silence.  No device."""
import functools

import numpy as np
import pytest

from tests import channelizer_oracle as cz
from tests import pkt_oracle as po


def pk():
    from pysdr_amd import packet
    return packet


def frame(k=0, n_info=31):
    info = (f"!4903.50N/07201.75W-Test {k:06d} " + "abcdefghijklmnopqrstuvwxyz" * 13)[:n_info]
    return pk().ax25_frame("APRS", f"N0CALL-{k % 16}", ("WIDE1-1*", "WIDE2-1"), info)


def heard(o, ev, m0=0):
    """the oracle's events of one call -> {(decoder, absolute m): bytes}"""
    return {(d, m0 + i): data for d in range(o.nd) for i, data in po.unpack(ev[d])}


def row_signal(frames, fs_out, cn=None, bal=1.0, lead=0.02, tail=0.02, seed=0, flags=(30, 3)):
    """one row at fs_out with one transmission on its centre: complex64 [1][n]; cn None: no noise"""
    s = pk().waveform(frames, fs_out, 0.0, preemph=bal, flags=flags)
    n = len(s) + int((lead + tail) * fs_out)
    if cn is None:
        x = np.zeros(n, np.complex64)
        x[int(lead * fs_out):int(lead * fs_out) + len(s)] = 0.1 * s
        return x[None, :]
    return po.scene(fs_out, n, [(frames, 0.0, cn, bal, int(lead * fs_out))], fs_out, functools.partial(pk().waveform, flags=flags), seed)[None, :]


# ---- the helpers -------------------------------------------------------------------------------------------------------
def test_crc_check_value_and_the_residue_of_every_frame():
    p = pk()
    assert p.crc16(b"123456789") == 0x906E
    rng = np.random.default_rng(1)
    for k in range(40):
        f = p.ax25_frame("APRS", f"N0CALL-{k % 16}", ("WIDE1-1",) * (k % 3), bytes(rng.integers(0, 256, k * 7, dtype=np.uint8)))
        assert p.crc_register(f + p.fcs(f)) == 0xF0B8
        assert p.crc_register(f[:-1] + bytes([f[-1] ^ 1]) + p.fcs(f)) != 0xF0B8


def test_frame_parse_and_tnc2_round_trips():
    p = pk()
    f = p.ax25_frame("APRS", "N0CALL-7", ("WIDE1-1*",), b"info")
    assert f[:7] == bytes(ord(c) << 1 for c in "APRS  ") + bytes([0x60]) and f[13] == (0x60 | 7 << 1)
    assert f[20] == (0x60 | 1 << 1 | 0x80 | 1) and f[21:23] == b"\x03\xf0" and f[23:] == b"info"
    assert p.tnc2(f) == "N0CALL-7>APRS,WIDE1-1*:info"
    f = p.ax25_frame("APZ001", "DL1ABC-15", ("DB0XYZ*", "WIDE2*", "WIDE3-3"), "hello")
    q = p.ax25_parse(f)
    assert q == dict(dest="APZ001", src="DL1ABC-15", path=("DB0XYZ*", "WIDE2*", "WIDE3-3"), control=3, pid=0xF0, info=b"hello")
    assert p.ax25_frame(q["dest"], q["src"], q["path"], q["info"], q["control"], q["pid"]) == f
    assert p.tnc2(f) == "DL1ABC-15>APZ001,DB0XYZ,WIDE2*,WIDE3-3:hello"        # the star behind the last one that repeated
    short = p.ax25_frame("A", "B", pid=None)
    assert len(short) == 15 and len(short + p.fcs(short)) == 17 and p.tnc2(short) == "B>A:"
    assert p.ax25_parse(short) == dict(dest="A", src="B", path=(), control=3, pid=None, info=b"")
    longest = p.ax25_frame("APRS", "N0CALL", info=bytes(range(256)) + bytes(330 - 16 - 256))
    assert len(longest) == 330 and p.ax25_parse(longest)["info"][:256] == bytes(range(256))
    assert p.ax25_parse(b"\x01" * 20) is None and p.tnc2(b"\x01\x02").startswith("?")
    with pytest.raises(ValueError):
        p.ax25_frame("TOOLONGCALL", "B")
    with pytest.raises(ValueError):
        p.ax25_frame("A", "B-16")


def test_hdlc_bits_stuff_and_flag():
    p = pk()
    f = p.ax25_frame("A", "B", info=b"\xff\xff")
    lv = p.hdlc_bits(f, flags=(2, 1))
    bits = [1 if a == b else 0 for a, b in zip(lv, np.concatenate(([1], lv[:-1])))]    # NRZI back
    assert bits[:16] == [0, 1, 1, 1, 1, 1, 1, 0] * 2 and bits[-8:] == [0, 1, 1, 1, 1, 1, 1, 0]
    body = "".join(map(str, bits[16:-8]))
    assert "111111" not in body and body.count("111110") >= 3
    assert len(p.afsk_audio(lv, 48000.0)) == len(lv) * 40 and np.abs(p.afsk_audio(lv, 48000.0, 0.55)).max() <= 1.0
    w = p.waveform(f, 96000.0, 5000.0)
    assert w.dtype == np.complex64 and np.allclose(np.abs(w), 1.0, atol=1e-6)


def test_tables_params_and_unpack():
    p = pk()
    for fs_out in (9600.0, 12500.0, 19200.0, 24000.0, 25000.0, 48000.0):
        L, tw, g = p.tables(fs_out)
        L2, tw2, g2 = po.tables(fs_out)
        assert L == L2 == int(np.floor(fs_out / 1200 + 0.5)) and 8 <= L <= 40
        assert np.array_equal(tw.view(np.uint32), tw2.view(np.uint32)) and np.array_equal(g.view(np.uint32), g2.view(np.uint32))
        c, par = p.cfg_dict(p.params(fs_out)), po.params(fs_out)
        assert (c["w_mark"], c["w_space"], c["w_baud"], c["pll_shift"]) == (par["w_mark"], par["w_space"], par["w_baud"], par["pll_shift"])
        assert np.array_equal(np.array(c["gain"], np.float32).view(np.uint32), par["gain"].view(np.uint32)) and c["pmax"] == float(par["pmax"])
    assert p.window_length(25000.0) == 21 and p.phase_word(1200.0, 9600.0) == 1 << 29
    words = [(5 << 10) | 5, 0x04030201, 0x05, (9 << 10) | 4, 0x0D0C0B0A]
    assert p.unpack(np.array(words, np.int32)) == po.unpack(words) == [(5, bytes([1, 2, 3, 4, 5])), (9, bytes([10, 11, 12, 13]))]


# ---- framing, on clean rows --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs_out", (9600.0, 19200.0, 25000.0, 48000.0))
def test_stuffing_at_byte_boundaries_the_shortest_and_the_longest_frame(fs_out):
    """five ones that end on a byte boundary (0xF8 then a byte with a low 1 or 0), runs of 0xFF and of 0x7E, the 15-byte
    and the 330-byte frame, 331 bytes (not a frame), all in one row and read by every slicer that is not off balance"""
    p = pk()
    frames = [p.ax25_frame("A", "B", info=b"\xf8\x01\xf8\x00\x1f\x1f\xf8"), p.ax25_frame("A", "B", info=b"\xff" * 40),
              p.ax25_frame("A", "B", info=b"\x7e" * 40), p.ax25_frame("A", "B", pid=None),
              p.ax25_frame("A", "B", info=bytes(330 - 16)), p.ax25_frame("A", "B", info=b"\x55" * (331 - 16))]
    y = np.concatenate([row_signal(f, fs_out, flags=(8, 2)) for f in frames], axis=1)
    o = po.Oracle(1, fs_out)
    counts, ev = o.process(y)
    got = heard(o, ev)
    for k, f in enumerate(frames[:5]):
        assert sum(1 for v in got.values() if v == f) >= 4, (k, len(f))
    assert set(got.values()) == set(frames[:5])
    assert counts.max() <= po.cap_of(y.shape[1], o.par["w_baud"])
    assert (o.state()["nbytes"] <= 333).all()


def test_two_frames_that_share_one_flag_are_both_read():
    fs_out = 25000.0
    a, b = frame(1), frame(2, 50)
    o = po.Oracle(1, fs_out)
    counts, ev = o.process(row_signal([a, b], fs_out))
    got = heard(o, ev)
    assert set(got.values()) == {a, b}
    ma, mb = min(m for (d, m), v in got.items() if v == a), min(m for (d, m), v in got.items() if v == b)
    assert abs((mb - ma) - (len(b) + 3) * 8 * fs_out / 1200) < 0.05 * (len(b) + 3) * 8 * fs_out / 1200 + 2 * 21   # stuffed bits, jitter


@functools.lru_cache(maxsize=None)
def noisy_row(fs_out=24000.0):
    y = np.concatenate([row_signal(frame(k, 20 + 9 * k), fs_out, cn=15.0, bal=b, seed=k, flags=(10, 2))
                        for k, b in enumerate((1.0, 0.55, 1.83))], axis=1)
    y.setflags(write=False)
    o = po.Oracle(1, fs_out)
    counts, ev = o.process(y)
    return y, heard(o, ev), o.state()


def test_any_cut_of_the_stream_gives_the_same_events_and_state():
    fs_out = 24000.0
    y, want, state = noisy_row(fs_out)
    assert len(set(want.values())) == 3
    rng = np.random.default_rng(5)
    for trial in range(3):
        o, got, at = po.Oracle(1, fs_out), {}, 0
        cuts = [0, 1, 1, 63, 64, 65, 0, 16] if trial == 0 else []
        while at < y.shape[1]:
            n = cuts.pop(0) if cuts else int(rng.integers(0, (40, 700, 5000)[trial]))
            m0 = o.m
            counts, ev = o.process(y[:, at:at + n])
            assert counts.max(initial=0) <= po.cap_of(max(n, 1), o.par["w_baud"])
            got.update(heard(o, ev, m0))
            at += n
        assert got == want
        st = o.state()
        assert all(np.array_equal(st[k], state[k]) for k in st), trial


def test_a_nan_and_an_inf_blank_only_their_windows():
    fs_out = 24000.0
    y, want, _ = noisy_row(fs_out)
    L = 20
    bad = np.array(y)
    k1, k2 = 4000, 4100                                                   # inside the first frame's flags, and behind them
    bad[0, k1] = complex(np.nan, 0.5)
    bad[0, k2] = complex(0.25, -np.inf)
    a, b = po.Oracle(1, fs_out), po.Oracle(1, fs_out)
    pa, pb = a.powers(y), b.powers(bad)
    touched = np.zeros(y.shape[1], bool)
    for k in (k1, k2):
        touched[k:k + L + 1] = True                                       # d[k] and d[k + 1], each for L outputs
    for u, v in zip(pa, pb):
        assert np.isfinite(v).all() and not v[0, touched].any() and u[0, touched].all()
        assert np.array_equal(u[0, ~touched].view(np.uint32), v[0, ~touched].view(np.uint32))
    counts, ev = b.process(bad)
    got = heard(b, ev)
    assert set(got.values()) >= set(list(set(want.values()))) - {frame(0, 20)} and len(set(got.values())) >= 2


# ---- behind the channelizer ----------------------------------------------------------------------------------------------
CASES = [(192000.0, 20, 10), (192000.0, 16, 8), (200000.0, 16, 8)]       # rows at 19.2, 24 and 25 kHz


@pytest.mark.parametrize("fs,M,D", CASES, ids=["19200", "24000", "25000"])
@pytest.mark.parametrize("off", (0.0, 800.0, -800.0))
def test_every_planted_frame_is_read_on_two_slicers_at_12_db(fs, M, D, off):
    """three stations, 2200 Hz at 0.55, 1.0 and 1.83 of 1200 Hz, `off` Hz off their rows' centres, 12 dB C/N in the row
    bandwidth, through the float64 channelizer with the skimmer's prototype"""
    p = pk()
    fs_out = fs / D
    n = int(0.72 * fs)
    planted = [(frame(3 * k + int(abs(off)) % 7, 25 + 5 * k), ch, bal) for k, (ch, bal) in enumerate(((2, 0.55), (5, 1.0), (8, 1.83)))]
    stations = [([f], ch * fs / M + off, 12.0, bal, int(0.02 * fs) + 777 * k) for k, (f, ch, bal) in enumerate(planted)]
    x = po.scene(fs, n, stations, fs_out, p.waveform, seed=int(fs + off) % 1000)
    ks = np.arange(1, 10)
    y = cz.polyphase(x, p.prototype(fs, M, D), M, D, 0, -(-n // D), ks=ks).astype(np.complex64)
    o = po.Oracle(len(ks), fs_out)
    counts, ev = o.process(y)
    got = heard(o, ev)
    for f, ch, bal in planted:
        slicers = sorted({d % 8 for (d, m), v in got.items() if v == f and d // 8 == ch - 1})
        print(f"fs_out {fs_out} off {off} balance {bal}: slicers {slicers}")
        assert len(slicers) >= 2, (ch, bal, slicers)
    assert set(got.values()) == {f for f, _, _ in planted}                # and no frame that was not sent
    assert {d // 8 for d, m in got} == {1, 4, 7}                          # on their home rows, not on the neighbours


def test_noise_alone_gives_no_frame():
    """60 row-seconds of white noise: 8 rows of 7.5 s at 19.2 kHz.  A flag that closes 17 bytes or more reaches the CRC
    comparison and passes it with probability 2^-16; the count is printed for the README's false-frame rate."""
    fs_out, rows, secs = 19200.0, 8, 7.5
    rng = np.random.default_rng(77)
    n = int(secs * fs_out)
    y = (0.1 * (rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n)))).astype(np.complex64)
    o = po.Oracle(rows, fs_out)
    total = 0
    for at in range(0, n, 4096):
        counts, ev = o.process(y[:, at:at + 4096])
        total += int(counts.sum())
    print(f"noise: {rows * secs:.0f} row-seconds, {o.nd} decoders, {o.fcs_checks} flags behind 17 bytes or more reached the CRC comparison: "
          f"{o.fcs_checks * 2.0 ** -16:.2e} false frames expected")
    assert total == 0


# ---- the host's rule -------------------------------------------------------------------------------------------------------
def test_dedup_equals_the_oracle_rule_whatever_the_cut():
    p = pk()
    fs, fs_out, L = 200000.0, 25000.0, 21
    freqs = (np.arange(12) - 3) * 6250.0                                  # rows 6.25 kHz apart: two to either side are near
    near = p.near_rows(freqs, fs, fs_out)
    assert near[0] == {0, 1} and near[5] == {4, 5, 6} and p.near_rows(np.arange(16) * 12500.0, fs, fs_out)[3] == {3}
    assert p.near_rows((np.arange(32) * 6250.0 + 1e5) % 2e5 - 1e5, fs, fs_out)[0] == {31, 0, 1}      # the circle of fs
    rng = np.random.default_rng(9)
    raw, m = [], 100
    for k in range(60):
        m += int(rng.integers(1, 400))
        data, row = bytes([k % 5]) * 20, int(rng.integers(0, 12))
        for r in range(max(0, row - 2), min(12, row + 3)):
            for s in rng.choice(8, int(rng.integers(0, 6)), replace=False):
                raw.append((m + int(rng.integers(0, 5)), r, int(s), data))
    raw.sort()
    end = raw[-1][0] + 200
    results = []
    for step in (1 << 30, 4096, 97, 16):
        a, b = p.Dedup(4 * L, near), po.Skimmer(12, fs, fs_out, freqs, p.tnc2)
        got, want = [], []
        for m0 in range(0, end, min(step, end)):
            part = [q for q in raw if m0 <= q[0] < m0 + step]
            got += a.add(part, min(m0 + step, end))
            want += [(m, row) for m, row, _ in b.take(part, min(m0 + step, end))]
        got += a.flush()
        assert [(m, row) for m, row, _, _ in got] == want + [(m, row) for m, row, _ in b._leave(lambda st: True)]
        assert got == b.frames
        results.append(got)
    assert all(r == results[0] for r in results) and 40 < len(results[0]) < len(raw) / 3
