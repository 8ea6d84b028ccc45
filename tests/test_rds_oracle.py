"""The RDS skimmer's definition on the CPU: the protocol helpers of pysdr_amd/rds.py, and the float32
oracle of steps 1 to 6 (tests/rds_oracle.py) reading every planted group -- behind the float64 channelizer model
(tests/channelizer_oracle.py) at the asserted C/N, and on rows made at the row rate for the cuts, the non-finite samples,
silence and noise.  The GPU tests hold the kernel equal to this oracle; that the oracle reads what was sent is shown
here, so that they cannot pass on silence.  No device."""
import functools

import numpy as np
import pytest

from tests import channelizer_oracle as cz
from tests import rds_oracle as ro

# Sensitivity.  With the oracle behind the float64 channelizer, the station below 10 kHz off a row's centre, C/N in the row
# bandwidth in steps of 1 dB from 6 to 25 dB and three seeds, the lowest level from which every seed at every step read
# every planted group was 18 dB at 400 kHz rows (17 dB: 6, 6 and 5 of 7 groups) and 21 dB at 228 kHz rows (20 dB: 7, 6 and
# 6 of 7), the same noise density to within half a dB: wideband FM's threshold, with 2 kHz of deviation for the data.  The
# assertion is 2 dB above that -- the step, and the spread between the seeds, which was one step.
LEVEL_DB = {228000.0: 23.0, 400000.0: 20.0}


def rd():
    from pysdr_amd import rds
    return rds


def station_groups(pi=None, ps="KSON97.3", rt="Hello RDS", version_b=False):
    r = rd()
    pi = r.pi_of("KSON") if pi is None else pi
    return r.ps_groups(pi, ps, version_b=version_b) + r.rt_groups(pi, rt, version_b=version_b)


def heard(ev, m0=0):
    """the oracle's events of one call -> {(decoder, absolute m): words}"""
    return {(d, m0 + i): w for d in range(len(ev)) for i, p, w in ro.unpack(ev[d]) if p == d % 16}


def as_words(g):
    return tuple(g) + ((g[1] >> 11) & 1,)


# ---- the constants and the helpers -----------------------------------------------------------------------------------
def test_the_eleven_numbers_agree_with_the_decoder_syndromes_of_the_standard():
    """g has x of order 341 -- the (341, 331) code, shortened to (26, 16) -- and with the single exponent 325 every offset
    word o gives (o x^325) mod g = the syndrome the standard lists for it: a wrong digit in any of the eleven breaks this."""
    r = rd()

    def mulx(v):
        v <<= 1
        return (v ^ r.POLY) & 0x3FF if v & 0x400 else v

    v, order = mulx(1), 1
    while v != 1:
        v, order = mulx(v), order + 1
    assert order == 341
    want = {"A": 0x3D8, "B": 0x3D4, "C": 0x25C, "C'": 0x3CC, "D": 0x258}
    for name, o in r.OFFSETS.items():
        s = o
        for _ in range(325):
            s = mulx(s)
        assert s == want[name], (name, hex(s))
    assert (ro.POLY, ro.OFF_A, ro.OFF_B, ro.OFF_C, ro.OFF_C2, ro.OFF_D) == (r.POLY, *r.OFFSETS.values())
    assert r.syndrome(0) == 0 and 0 not in r.OFFSETS.values()              # a zeroed register matches nothing
    b = np.arange(0, 1 << 26, 4099, dtype=np.uint32)
    assert [r.syndrome(int(v)) for v in b[:500]] == list(ro.syndromes(b[:500]))


def test_every_block_of_every_group_maker_checks_with_its_offset_and_no_other():
    r = rd()
    pi = 0x54A8 + 4321
    groups = (r.ps_groups(pi, "ABCDEFGH", af=(97.3, 101.5)) + r.ps_groups(pi, "ABCDEFGH", version_b=True) + r.rt_groups(pi, "x" * 64, ab=1)
              + r.rt_groups(pi, "short", version_b=True) + [r.group_4a(pi, 60000, 23, 59, -3), r.group_4a(pi, 0x1FFFF, 0, 0, 31)])
    for g in groups:
        bits = r.group_bits(*g)
        assert bits.shape == (104,) and set(bits) <= {0, 1}
        blocks = [int("".join(map(str, bits[26 * k:26 * k + 26])), 2) for k in range(4)]
        names = ["A", "B", "C'" if g[1] >> 11 & 1 else "C", "D"]
        assert [r.check_block(b) for b in blocks] == names
        assert [b >> 10 for b in blocks] == list(g)
        for b, name in zip(blocks, names):
            assert b == r.block(b >> 10, name) and [k for k, o in r.OFFSETS.items() if r.syndrome(b) == o] == [name]
            assert all(r.check_block(b ^ 1 << k) is None or r.check_block(b ^ 1 << k) != name for k in range(26))
    assert len(r.bits(groups)) == 104 * len(groups) and np.array_equal(r.bits(groups[:1]), r.group_bits(*groups[0]))
    assert np.array_equal(r.group_bits(1, 2, 3, 4, version_b=True)[52:78], r.group_bits(1, 2 | 0x800, 3, 4)[52:78])


def test_parse_group_round_trips():
    r = rd()
    pi = r.pi_of("KFMB")
    g = r.parse_group(r.group_0a(pi, "KFMB-FM ", 2, tp=1, pty=9, ta=1, ms=0, di=1, af=(100.7, None)))
    assert g == dict(pi=pi, type="0A", tp=1, pty=9, seg=2, ps="-F", ta=1, ms=0, di=1, af=(100.7, None))
    assert r.parse_group(r.group_0a(pi, "ab", 0, af=(87.6, 107.9)))["af"] == (87.6, 107.9)
    g = r.parse_group(r.group_0b(pi, "KFMB-FM ", 3, pty=31))
    assert g == dict(pi=pi, type="0B", tp=0, pty=31, seg=3, ps="M ", ta=0, ms=1, di=0) and r.group_0b(pi, "x", 0)[2] == pi
    g = r.parse_group(r.group_2a(pi, "0123456789abcdef", 3, 1))
    assert (g["type"], g["seg"], g["ab"], g["text"], g["raw"]) == ("2A", 3, 1, "cdef", b"cdef")
    g = r.parse_group(r.group_2b(pi, "0123456789abcdef", 5, 0))
    assert (g["type"], g["seg"], g["ab"], g["text"]) == ("2B", 5, 0, "ab")
    assert r.parse_group(r.group_2a(pi, b"\x0d\x7f\x8e~", 0, 0))["text"] == "??" + "?~"   # only 0x20 to 0x7E are ASCII
    for mjd, hh, mm, off in ((60605, 13, 7, 2), (0x1FFFF, 23, 59, -31), (0, 0, 0, 0), (0x8000, 16, 32, -1)):
        g = r.parse_group(r.group_4a(pi, mjd, hh, mm, off))
        assert (g["type"], g["mjd"], g["hour"], g["minute"], g["offset"]) == ("4A", mjd, hh, mm, off)
    assert r.parse_group((pi, 0x3000 | 0x1F, 0xBEEF, 0xCAFE)) == dict(pi=pi, type="3A", tp=0, pty=0, raw=(0x1F, 0xBEEF, 0xCAFE))
    assert r.parse_group(as_words(r.group_0b(pi, "ab", 0)))["type"] == "0B"    # five words, as the skimmer hands them over
    with pytest.raises(ValueError):
        r.af_code(108.0)


def test_callsign_round_trip():
    """unpinned (from memory of NRSC-4): only that the two directions agree, and where the rule ends"""
    r = rd()
    for call in ("KAAA", "KSON", "KFMB", "KZZZ", "WAAA", "WXYZ", "WZZZ"):
        assert r.callsign(r.pi_of(call)) == call
    assert r.pi_of("KAAA") == 0x1000 and r.pi_of("WAAA") == 0x54A8 and r.pi_of("KZZZ") + 1 == r.pi_of("WAAA")
    assert r.callsign(0x0FFF) is None and r.callsign(r.pi_of("WZZZ") + 1) is None
    with pytest.raises(ValueError):
        r.pi_of("KGB")


def test_station_assembles_ps_and_radiotext():
    r = rd()
    pi = r.pi_of("KSON")
    st = r.Station(pi)
    assert st.call == "KSON"
    feed = lambda gs: [c for g in gs for c in st.add(r.parse_group(g))]
    ps = r.ps_groups(pi, "KSON97.3")
    assert feed(ps[:3]) == [] and st.ps is None
    assert feed([ps[1], ps[1]]) == []                                         # a repeated segment
    assert feed(ps[3:]) == [("ps", "KSON97.3")] and feed(ps) == []            # shown once
    new = r.ps_groups(pi, "KSON HD1")
    assert feed(new[2:]) == [] and st.ps == "KSON97.3"                        # two new segments: the marks start over
    assert feed(new[:1]) == [] and feed(new[1:2]) == [("ps", "KSON HD1")]
    rt = r.rt_groups(pi, "Now playing: a song", ab=0)
    assert len(rt) == 5 and feed(rt[1:]) == [] and st.rt is None
    assert feed(rt[:1]) == [("rt", "Now playing: a song")] and feed(rt) == []
    flip = r.rt_groups(pi, "Next", ab=1)
    assert len(flip) == 2 and feed(flip[:1]) == [] and st.rt is None          # the flip cleared it
    assert feed(flip[1:]) == [("rt", "Next")]
    full = r.rt_groups(pi, "0123456789abcdef" * 4, ab=0)
    assert len(full) == 16 and feed(full[:15]) == [] and feed(full[15:]) == [("rt", "0123456789abcdef" * 4)]
    short = r.rt_groups(pi, "2B text", ab=1, version_b=True)
    assert len(short) == 4 and feed(short) == [("rt", "2B text")]
    assert feed([r.group_4a(pi, 60605, 13, 7, 2)] * 2) == [("ct", (60605, 13, 7, 2))]
    # the skimmer's guard: a PI is listed at its second group, and then takes both
    stations, first = [dict()], [dict()]
    out = r.keep_groups([(100 * k, 0, as_words(g), 1) for k, g in enumerate(ps)] + [(999, 0, (0xDEAD, 0, 0, 0, 0), 1)], stations, first)
    assert [e[2] for e in out] == ["group"] * 4 + ["ps", "group"] and out[4] == (300, 0, "ps", "KSON97.3")
    assert list(stations[0]) == [pi] and list(first[0]) == [0xDEAD]
    # neighbour rows overlap: a PI stays on the row where it was first heard, two rows away at the most
    near = [{0, 1}, {0, 1, 2}, {1, 2, 3}, {2, 3, 4}, {3, 4}]
    stations, first = [dict() for _ in near], [dict() for _ in near]
    out = r.keep_groups([(100 * k, row, as_words(g), 1) for k, (g, row) in enumerate(zip(ps, (1, 2, 3, 1)))] + [(500, 4, as_words(ps[0]), 1)], stations, first, near)
    assert [len(s) for s in stations] == [0, 1, 0, 0, 0] and out[-2] == (300, 1, "ps", "KSON97.3") and stations[1][pi].rows == {1: 2, 2: 1, 3: 1}
    assert list(first[4]) == [pi]                                              # three rows away: another station


def test_tables_params_and_unpack():
    r = rd()
    for fs_out in (228000.0, 250000.0, 400000.0, 512000.0):
        L, tw, g = r.tables(fs_out)
        L2, tw2, g2 = ro.tables(fs_out)
        assert L == L2 == 2 * int(fs_out // 1187.5) + 1 and 385 <= L <= 863
        assert np.array_equal(tw.view(np.uint32), tw2.view(np.uint32)) and np.array_equal(g.view(np.uint32), g2.view(np.uint32))
        assert np.array_equal(g, -g[::-1]) and g[(L - 1) // 2] == 0 and g[(L - 1) // 2 - 1] > 0   # odd about its centre: a biphase symbol
        assert r.params(fs_out).w19 == ro.word19(fs_out)
    assert r.pulse_length(228000.0) == 385 and r.phase_word(19000.0, 304000.0) == 1 << 28
    words = [(5 << 5) | (9 << 1) | 1, (0x1234 << 16) | 0x0800, (0x1234 << 16) | 0x4142, (77 << 5) | (15 << 1), 0x00010002, -1]
    want = [(5, 9, (0x1234, 0x0800, 0x1234, 0x4142, 1)), (77, 15, (1, 2, 0xFFFF, 0xFFFF, 0))]
    assert r.unpack(np.array(words, np.int64).astype(np.int32)) == ro.unpack([ro._i32(v) for v in words]) == want
    h = r.prototype(1600000.0, 16, 4)
    assert len(h) == 192 <= 16 * 16 and abs(h.sum() - 1) < 1e-12
    H = np.abs(np.fft.rfft(h, 1 << 16))                                       # flat over +-100 kHz of a row at 400 kHz, and beyond
    f = np.fft.rfftfreq(1 << 16, 1 / 1600000.0)
    assert np.abs(20 * np.log10(H[f <= 170e3])).max() < 0.1 and 20 * np.log10(H[f >= 230e3].max()) < -75


# ---- on rows made at the row rate ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def noisy_row(fs_out=400000.0):
    """two rows: a station 10 kHz off the first's centre at 20 dB, a version B one -15 kHz off the second's, mid-stream"""
    r = rd()
    a, b = station_groups(), station_groups(r.pi_of("WXYZ"), "WXYZ-FM ", "B", version_b=True)
    na = len(r.waveform(a, fs_out, 0.0)) + 3000
    y = np.stack((ro.scene(fs_out, na, [(a, 10e3, 20.0, 1500)], fs_out, r.waveform, seed=1),
                  ro.scene(fs_out, na, [(b, -15e3, 25.0, 40000)], fs_out, r.waveform, seed=2)))
    y.setflags(write=False)
    o = ro.Oracle(2, fs_out)
    counts, ev = o.process(y)
    return y, heard(ev), o.state(), (a, b)


def test_the_oracle_reads_the_planted_groups_and_no_other():
    y, want, state, (a, b) = noisy_row()
    assert {w for (d, m), w in want.items() if d < 16} == {as_words(g) for g in a}
    assert {w for (d, m), w in want.items() if d >= 16} == {as_words(g) for g in b} and all(w[4] == 1 for (d, m), w in want.items() if d >= 16)
    for g in a + b:
        phases = {d % 16 for (d, m), w in want.items() if w == as_words(g)}
        assert len(phases) >= 4, (g, phases)


def test_any_cut_of_the_stream_gives_the_same_events_and_state():
    fs_out = 400000.0
    y, want, state, _ = noisy_row(fs_out)
    rng = np.random.default_rng(5)
    for trial in range(3):
        o, got, at = ro.Oracle(2, fs_out), {}, 0
        cuts = [0, 1, 1, 20, 21, 22, 0, 1023, 1024, 1025] if trial == 0 else []
        while at < y.shape[1]:
            n = cuts.pop(0) if cuts else int(rng.integers(0, 60 if trial == 0 and at < 3000 else (20000, 3000, 50000)[trial]))
            m0 = o.m
            counts, ev = o.process(y[:, at:at + n])
            assert counts.max(initial=0) <= ro.cap_of(max(n, 1), o.w19)
            got.update(heard(ev, m0))
            at += n
        assert got == want
        ro.same_state(o.state(), state, trial)
    # and the oracle's one-pass form, which the GPU tests use for their many short calls, is the same thing
    a, b = ro.Oracle(2, fs_out), ro.Oracle(2, fs_out)
    lengths = [0, 1, 255, 256, 257, 0, 1024, 5000]
    lengths += [256] * 40 + [y.shape[1] - sum(lengths) - 256 * 40]
    at = 0
    for n, (counts, ev, st) in zip(lengths, a.replay(y, lengths)):
        c2, ev2 = b.process(y[:, at:at + n])
        assert np.array_equal(counts, c2) and ev == ev2
        ro.same_state(st, b.state(), at)
        at += n
    ro.same_state(a.state(), state, "replay")
    assert np.array_equal(a.hist, b.hist) and a.m == b.m


def test_a_nan_and_an_inf_zero_two_products_each_and_nothing_else():
    """d is 0 at a non-finite sample and at the one behind it (both products of the discriminator hold it) and finite
    everywhere; every other product is bit for bit what it was, so only the chips within L of them move"""
    fs_out = 400000.0
    y, want, _, (a, b) = noisy_row(fs_out)
    L = 673
    bad = np.array(y)
    k1, k2 = 30011, 90007
    bad[0, k1] = complex(np.nan, 0.5)
    bad[0, k2] = complex(0.25, -np.inf)
    p, q = ro.Oracle(2, fs_out), ro.Oracle(2, fs_out)
    (vx, vy), (wx, wy) = p.products(y), q.products(bad)
    cols = np.array([L + k1, L + k1 + 1, L + k2, L + k2 + 1])
    assert ((vx[0, cols] != 0) | (vy[0, cols] != 0)).all()
    for u, v in ((vx, wx), (vy, wy)):
        assert np.isfinite(v).all() and not v[0, cols].any()
        keep = np.ones(u.shape[1], bool)
        keep[cols] = False
        assert np.array_equal(u[:, keep].view(np.uint32), v[:, keep].view(np.uint32))
    jj = p.ticks(y.shape[1])
    (zx, zy), (ux, uy) = p.matched(vx, vy, jj), q.matched(wx, wy, jj)
    near = ((jj >= k1) & (jj < k1 + 1 + L)) | ((jj >= k2) & (jj < k2 + 1 + L))
    assert np.array_equal(zx[:, ~near].view(np.uint32), ux[:, ~near].view(np.uint32)) and np.array_equal(zy[1].view(np.uint32), uy[1].view(np.uint32))
    assert (zx[0, near] != ux[0, near]).any() and np.isfinite(ux).all() and np.isfinite(uy).all()
    counts, ev = q.process(bad)
    got = heard(ev)
    assert np.isfinite(q.ring).all() and {w for w in got.values()} == {w for w in want.values()}   # two samples of 673 do not cost a group


def test_a_silent_row_emits_nothing_and_holds_d_at_zero():
    fs_out = 228000.0
    o = ro.Oracle(1, fs_out)
    y = np.zeros((1, 30000), np.complex64)
    vx, vy = o.products(y)
    assert not vx.any() and not vy.any()
    assert not ro.arg(np.zeros(4, np.complex64), np.ones(4, np.complex64)).any()
    counts, ev = o.process(y)
    st = o.state()
    assert not counts.any() and not st["regs"].any() and not st["ring"].any() and st["chips"][0] == 30000 // 12 == len(o.ticks(30000)) + 0
    # the four quadrants and the axes, against the library arctangent
    ang = np.linspace(-np.pi, np.pi, 2001)[1:-1]
    d = ro.arg(np.exp(1j * ang).astype(np.complex64), np.ones(len(ang), np.complex64))
    assert np.abs(d - ang).max() < 2e-5 and ro.arg(np.array([-1 + 0j], np.complex64), np.ones(1, np.complex64))[0] == np.float32(np.pi)


def test_noise_alone_gives_no_group():
    """16 row-seconds of white noise: 8 rows of 2 s at 228 kHz, 256 decoders.  A phase passes the check with probability
    2 x 2^-40 per bit: 5.6e-7 false groups are expected here."""
    fs_out, rows, secs = 228000.0, 8, 2.0
    rng = np.random.default_rng(77)
    n = int(secs * fs_out)
    o = ro.Oracle(rows, fs_out)
    total = 0
    for at in range(0, n, 65536):
        m = min(65536, n - at)
        y = (0.1 * (rng.standard_normal((rows, m)) + 1j * rng.standard_normal((rows, m)))).astype(np.complex64)
        total += int(o.process(y)[0].sum())
    bits = int(o.chips.astype(np.int64).sum())
    print(f"noise: {rows * secs:.0f} row-seconds, {o.nd} decoders, {bits} bits decided: {bits * 2.0 ** -39:.2e} false groups expected")
    assert total == 0 and bits == rows * len(np.arange(n)[::12]) and o.regs.any()


# ---- the host's rule -------------------------------------------------------------------------------------------------------
def test_dedup_yields_one_record_per_planted_group_whatever_the_cut():
    from pysdr_amd import packet
    r = rd()
    fs, fs_out = 2000000.0, 400000.0
    freqs = (np.arange(20) * 100e3 + 1e6) % 2e6 - 1e6
    near = packet.near_rows(freqs, fs, fs_out)
    assert near[5] == {4, 5, 6} and near[0] == {19, 0, 1} and r.reach(fs_out) == 674
    rng = np.random.default_rng(9)
    planted, raw, m = [], [], 1000
    for k in range(50):
        m += int(rng.integers(r.reach(fs_out) + 40, 5000))                  # the same words may come again after 104 bits, not sooner
        words, row = as_words(r.group_0a(0x5000 + k % 3, "ABCDEFGH", k % 4)), int(rng.integers(0, 20))
        planted.append((words, row))
        p0 = int(rng.integers(0, 16))
        for dr, nph in ((0, int(rng.integers(5, 12))), (1, int(rng.integers(0, 4))), (-1, int(rng.integers(0, 4)))):
            raw += [(m + 21 * j + dr, (row + dr) % 20, (p0 + j) % 16, words) for j in range(nph)]
    raw.sort()
    end = raw[-1][0] + 2000
    results = []
    for step in (1 << 30, 65536, 4096, 256, 21):
        a, b = packet.Dedup(r.reach(fs_out), near), ro.Skimmer(20, fs, fs_out, freqs)
        got, want = [], []
        for m0 in range(0, end, min(step, end)):
            part = [q for q in raw if m0 <= q[0] < m0 + step]
            got += a.add(part, min(m0 + step, end))
            want += b.take(part, min(m0 + step, end))
        got += a.flush()
        want += b._leave(lambda st: True)
        assert got == want == b.groups
        results.append(got)
    assert all(res == results[0] for res in results)
    assert [(w, row) for _, row, w, _ in results[0]] == planted           # one record each, on the row with the most phases
    assert all(bin(mask).count("1") >= 5 for _, _, _, mask in results[0])


# ---- behind the channelizer: sensitivity ----------------------------------------------------------------------------------
CASES = [(912000.0, 16, 4), (1600000.0, 16, 4)]                            # rows at 228 and 400 kHz


@pytest.mark.parametrize("fs,M,D", CASES, ids=["228k", "400k"])
def test_every_planted_group_is_read_at_the_asserted_level(fs, M, D):
    """the station of the issue's trial (L = 1 kHz, R = 3.1 kHz at 30 kHz, pilot 6.75 kHz, RDS 2 kHz), 10 kHz off a row's
    centre, LEVEL_DB[fs_out] C/N in the row bandwidth, through the float64 channelizer with the skimmer's prototype, three seeds"""
    r = rd()
    fs_out, ch = fs / D, 3
    groups = station_groups()
    s = r.waveform(groups, fs, ch * fs / M + 10e3).astype(np.complex128)
    n = len(s) + 4000
    pn = 10 ** (-40.0 / 10) * fs / fs_out
    for seed in range(3):
        rng = np.random.default_rng(1000 + seed)
        x = np.sqrt(pn / 2) * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
        x[2000:2000 + len(s)] += s * 10 ** ((-40.0 + LEVEL_DB[fs_out]) / 20)
        y = cz.polyphase(x.astype(np.complex64), r.prototype(fs, M, D), M, D, 0, -(-n // D), ks=np.array([ch])).astype(np.complex64)
        counts, ev = ro.Oracle(1, fs_out).process(y)
        got = {}
        for (d, m), w in heard(ev).items():
            got.setdefault(w, set()).add(d)
        print(f"fs_out {fs_out} seed {seed}: phases per group {[len(got.get(as_words(g), ())) for g in groups]}")
        assert set(got) == {as_words(g) for g in groups}, (seed, len(got))  # every planted group, and no other
