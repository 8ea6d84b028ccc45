"""The Python layer of the channelizer family -- Channelizer, FineChannelizer, the banks, the CW and PSK skimmers -- against a
recorded trace: every C call it makes (tests/fake_pysdr_lib.py stands in for the library and records name, scalars, a CRC of
what each input pointer is read for, NULL or not for each output pointer) and what every Python method returned, in order,
compared with tests/golden/chan_py_trace.json (written by tests/golden/make_chan_py_trace_golden.py).  CPU only."""
import json
import os

import numpy as np

from tests.fake_pysdr_lib import FakeLib, crc, quant

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chan_py_trace.json")


def enc(v):
    if isinstance(v, np.ndarray):
        return f"{v.dtype}{list(v.shape)}:{crc(quant(v) if v.dtype.kind in 'fc' else np.ascontiguousarray(v).tobytes())}"
    if isinstance(v, dict):
        return "{" + ", ".join(f"{k}: {enc(v[k])}" for k in sorted(v, key=str)) + "}"
    if isinstance(v, (list, tuple)):
        return "[" + ", ".join(enc(e) for e in v) + "]"
    if isinstance(v, (np.integer, np.floating, np.bool_)):
        return repr(v.item())
    return repr(v)


def samples(seed, n):
    rng = np.random.default_rng(1000 + seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


class Recorder:
    def __init__(self, fake):
        self.fake = fake

    def __call__(self, label, fn, *a, **kw):
        """runs fn, notes what it returned (or raised), returns it"""
        from pysdr_amd._lib import PysdrError
        try:
            r = fn(*a, **kw)
        except (PysdrError, AssertionError, ValueError) as e:
            self.fake.note(f"{label} raises {type(e).__name__}: {e}")
            return None
        self.fake.note(f"{label} -> {enc(r)}")
        return r

    def attrs(self, label, obj, names):
        self.fake.note(label + " " + ", ".join(f"{k}={enc(getattr(obj, k))}" for k in names))


CHAN_ATTRS = ("fs", "M", "D", "k_first", "nk", "device", "max_in", "fs_out", "freqs", "n_in")


def walk_channelizer(rec, ch, label, taps):
    for i, n in enumerate((0, 1, 7, 8, 9, 64, 150)):
        rec(f"{label}.n_out_for({n})", ch.n_out_for, n)
        rec(f"{label}.push({n})", ch.push, samples(i, n))
        rec.attrs(label, ch, ("n_in",))
    rec(f"{label}.push_device", ch.push_device, 0x10000, 21, 0x20000, 5)
    rec(f"{label}.push_device nosync", ch.push_device, 0x10000, 3, 0x20000, 1, sync=False)
    rec(f"{label}.sync", ch.sync)
    rec.attrs(label, ch, ("n_in",))
    rec(f"{label}.set_taps", ch.set_taps, *taps)
    rec(f"{label}.push(9)", ch.push, samples(20, 9))
    rec(f"{label}.reset", ch.reset)
    rec.attrs(label, ch, ("n_in",))
    rec(f"{label}.push(9)", ch.push, samples(21, 9))
    rec(f"{label}.close", ch.close)
    rec(f"{label}.close", ch.close)
    rec.attrs(label, ch, ("_h", "n_in"))
    rec(f"{label}.reset after close", ch.reset)


def scenario_channelizer(rec):
    from pysdr_amd import channelizer
    ch = channelizer.Channelizer(64e3, 16, 8, channels=(14, 5), max_in=64)
    rec.attrs("chan", ch, CHAN_ATTRS + ("max_taps", "h"))
    walk_channelizer(rec, ch, "chan", (np.arange(1, 49, dtype=np.float64) / 48,))
    rec.attrs("chan", ch, ("h",))
    rec("chan.plan bad", channelizer.plan, 16, 7, 128)


def scenario_fine(rec):
    from pysdr_amd import fine
    ch = fine.FineChannelizer(64e3, 16, 16, 8, 8, channels=(120, 16), max_in=64)
    rec.attrs("fine", ch, CHAN_ATTRS + ("M1", "M2", "D1", "D2", "Q", "k1_first", "nk1", "frames_per_wg", "max_taps1", "max_taps2",
                                        "h1", "h2", "run_in_taps"))
    walk_channelizer(rec, ch, "fine", (np.arange(1, 65, dtype=np.float64) / 64, np.arange(1, 33, dtype=np.float64) / 32))
    rec.attrs("fine", ch, ("h1", "h2", "run_in_taps"))
    full = fine.FineChannelizer(64e3, 16, 16)
    rec.attrs("fine full", full, CHAN_ATTRS)
    full.close()


def walk_bank(rec, b, label):
    rec.attrs(label, b, ("fs", "M", "D", "nk", "freqs", "fs_out", "mode", "af_bw", "af", "agc", "squelch", "last_n_out", "ntaps_af"))
    rec(f"{label}.push(21)", b.push, samples(30, 21))
    b.agc = False
    b.squelch = 0.25
    rec.attrs(label, b, ("agc", "squelch", "last_n_out"))
    rec(f"{label}.push(3)", b.push, samples(31, 3))
    rec(f"{label}.push_open(40)", b.push_open, samples(32, 40))
    rec(f"{label}.push_open(0)", b.push_open, samples(33, 0))
    rec(f"{label}.push_device", b.push_device, 0x10000, 17)
    rec(f"{label}.fetch am", b.fetch, [0, 3])
    rec(f"{label}.fetch iq", b.fetch, [4, 1], am=False, iq=True)
    rec(f"{label}.fetch both", b.fetch, [2], am=True, iq=True)
    rec(f"{label}.iq()", b.iq)
    rec(f"{label}.state", b.state)
    rec(f"{label}.open", lambda: b.open)
    rec(f"{label}.level", lambda: b.level)
    rec(f"{label}.agc_state", lambda: b.agc_state)
    rec(f"{label}.push_device nosync", b.push_device, 0x10000, 2, sync=False)
    rec(f"{label}.sync", b.sync)
    rec.attrs(label, b, ("last_n_out",))
    rec.attrs(label + ".chan", b.chan, ("n_in",))


def scenario_banks(rec):
    from pysdr_amd import bank
    b = bank.ChannelBank(64e3, 16, 8, channels=(14, 5), mode="NFM", af_bw=2e3, ntaps_af=31, squelch=0.1, max_in=64)
    walk_bank(rec, b, "bank")
    rec("bank.set_mode AM", b.set_mode, "AM", 1e3)
    rec("bank.set_mode USB", b.set_mode, "USB")
    rec("bank.reset", b.reset)
    rec.attrs("bank.chan", b.chan, ("n_in",))
    rec("bank.close", b.close)
    rec("bank.close", b.close)
    rec.attrs("bank", b, ("_h",))
    rec.attrs("bank.chan", b.chan, ("_h",))
    rec("bank bad mode", bank.ChannelBank, 64e3, 16, 8, mode="USB")
    s = bank.SidebandBank(64e3, 16, 8, channels=(14, 5), mode="USB", af_bw=2e3, ntaps_af=31, max_in=64)
    walk_bank(rec, s, "ssb")
    rec("ssb.set_mode CW", s.set_mode, "CW", 500.0, bfo=600.0)
    rec.attrs("ssb", s, ("mode", "af_bw", "af", "bfo"))
    rec("ssb.push(16)", s.push, samples(34, 16))
    rec("ssb.set_mode AM", s.set_mode, "AM")
    rec.attrs("ssb", s, ("mode", "af_bw", "af", "bfo"))
    rec("ssb.push(16)", s.push, samples(35, 16))
    rec("ssb.set_mode LSB", s.set_mode, "LSB", 1e3)
    rec("ssb.close", s.close)


def walk_cw(rec, sk, label):
    rec.attrs(label, sk, ("fs", "M", "D", "nk", "freqs", "fs_out", "text"))
    d = sk.dec
    rec.attrs(label + ".dec", d, ("nk", "D", "fs_out", "max_out", "cap", "plan", "last_n_out"))
    rec(label + ".dec.cfg", lambda: {k: getattr(d.cfg, k) for k, _ in type(d.cfg)._fields_})
    D = sk.D
    for i, n in enumerate((0, 1, D - 1, D, 2 * D + 1, 7 * D + 3, 3 * D, 11 * D - 2)):
        rec(f"{label}.dec.max_samples", d.max_samples)
        rec(f"{label}.push({n})", sk.push, samples(40 + i, n))
        rec.attrs(label, sk.chan, ("n_in",))
        rec.attrs(label, d, ("last_n_out",))
    rec.attrs(label, sk, ("text",))
    rec(f"{label}.sync", sk.sync)
    rec(f"{label}.state", sk.state)
    for ev in ("all", "rows", None):
        rec(f"{label}.decode_raw {ev}", d.decode_raw, samples(50, 2 * D + 1), events=ev)
        rec.attrs(label, sk.chan, ("n_in",))
    rec(f"{label}.decode_raw device", d.decode_raw, 0x10000, D + 2, on_device=True)
    rec(f"{label}.decode_raw device None", d.decode_raw, 0x10000, 2, on_device=True, events=None)
    rec(f"{label}.fetch", d.fetch, [sk.nk - 1, 0])
    rec.attrs(label, d, ("last_n_out",))
    rec(f"{label}.reset", sk.reset)
    rec.attrs(label, sk, ("text",))
    rec.attrs(label, sk.chan, ("n_in",))
    rec(f"{label}.push", sk.push, samples(51, 3 * D))
    rec(f"{label}.close", sk.close)
    rec(f"{label}.close", sk.close)
    rec.attrs(label, d, ("_h",))
    rec.attrs(label, sk.chan, ("_h",))
    rec(f"{label}.decode_raw after close", d.decode_raw, samples(52, 4))


def scenario_cw(rec):
    from pysdr_amd import cw, fine
    walk_cw(rec, cw.CW_Skimmer(64e3, 16, 8, channels=(14, 5), max_in=64, max_out=3), "cw")
    ch = fine.FineChannelizer(64e3, 16, 16, 8, 8, channels=(120, 16), max_in=300)
    walk_cw(rec, cw.CW_Skimmer(64e3, chan=ch, max_out=3), "cwf")
    rec("cw bad shape", cw.CW_Skimmer, 64e3, 16, 8, max_out=0)


def walk_psk(rec, sk, label):
    rec.attrs(label, sk, ("fs", "baud", "S", "D", "M", "nsub", "h", "nk", "nfine", "fs_out", "freqs", "freqs_fine", "circular",
                          "owner"))
    d = sk.dec
    rec.attrs(label + ".dec", d, ("S", "nsub", "nk", "D", "fs_out", "nfine", "max_out", "cap", "plan", "tw", "g", "last_n_out"))
    D = sk.D
    owners = []
    for i, n in enumerate((0, 1, D - 2, D, 25 * D + 1, 13 * D, 40 * D - 3)):
        rec(f"{label}.dec.max_samples", d.max_samples)
        rec(f"{label}.push({n})", sk.push, samples(60 + i, n))
        rec.attrs(label, sk.chan, ("n_in",))
        rec.attrs(label, sk, ("owner",))
        rec.attrs(label, d, ("last_n_out",))
        owners.append(sk.owner.copy())
    assert any((a != b).any() for a, b in zip(owners, owners[1:])) and owners[-1].any()    # the owner did change between calls
    rec(f"{label}.text", lambda: dict(sk.text))
    rec(f"{label}.sync", sk.sync)
    rec(f"{label}.state", sk.state)
    rec(f"{label}.decode_raw all", d.decode_raw, samples(70, 13 * D), events="all")
    rec(f"{label}.decode_raw counts squelch", d.decode_raw, samples(71, 2 * D + 1), events="counts", squelch=True)
    rec(f"{label}.decode_raw None", d.decode_raw, samples(72, D), events=None)
    rec(f"{label}.decode_raw device", d.decode_raw, 0x10000, 3 * D, on_device=True, squelch=True)
    rec(f"{label}.fetch", d.fetch, [d.nfine - 1, 0, 5])
    rec.attrs(label, sk.chan, ("n_in",))
    rec(f"{label}.reset", sk.reset)
    rec(f"{label}.text", lambda: dict(sk.text))
    rec.attrs(label, sk, ("owner",))
    rec.attrs(label, sk.chan, ("n_in",))
    rec(f"{label}.push", sk.push, samples(73, 14 * D))
    rec(f"{label}.close", sk.close)
    rec(f"{label}.close", sk.close)
    rec.attrs(label, d, ("_h",))
    rec.attrs(label, sk.chan, ("_h",))
    rec(f"{label}.decode_raw after close", d.decode_raw, samples(74, 4))


def scenario_psk(rec):
    from pysdr_amd import psk
    fs = next(f for f in range(250, 64001, 250) if _accepts(psk.shape, f))      # the smallest rate psk.shape accepts
    walk_psk(rec, psk.PSK_Skimmer(fs, channels=(6, 3), max_in=1 << 12, max_out=24), "psk")
    walk_psk(rec, psk.PSK_Skimmer(fs, max_in=1 << 12, max_out=24), "psk full")
    ffs = next(f for f in range(4000, 1024001, 4000) if _accepts(psk.fine_channelizer, f, (-100.0, 100.0)))
    ch = psk.fine_channelizer(ffs, (-100.0, 100.0), max_in=1 << 14)
    walk_psk(rec, psk.PSK_Skimmer(ffs, chan=ch, max_out=24), "pskf")
    ch = psk.fine_channelizer(ffs, (-100.0, 100.0))
    rec("psk bad chan", psk.PSK_Skimmer, 2 * ffs, chan=ch)
    ch.close()


def _accepts(fn, *a):
    try:
        r = fn(*a)
    except ValueError:
        return False
    if hasattr(r, "close"):
        r.close()
    return True


SCENARIOS = (scenario_channelizer, scenario_fine, scenario_banks, scenario_cw, scenario_psk)


def record(real, install):
    """-> {scenario name: [trace lines]}; ``install(fake)`` puts a fresh fake in place of the library before each scenario"""
    out = {}
    for sc in SCENARIOS:
        fake = FakeLib(real)
        install(fake)
        sc(Recorder(fake))
        out[sc.__name__] = fake.trace
    return out


def test_the_python_layer_makes_the_recorded_calls_and_returns_the_recorded_values(hiplib, monkeypatch):
    from pysdr_amd import _lib

    def install(fake):
        monkeypatch.setattr(_lib, "lib", lambda: fake)
        monkeypatch.setattr(_lib, "require_gpu", lambda: None)

    got = record(hiplib, install)
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    for name in want:
        for i, (g, w) in enumerate(zip(got[name], want[name])):
            assert g == w, f"{name}: line {i}: got {g!r}, recorded {w!r} (after {got[name][max(0, i - 3):i]})"
        assert len(got[name]) == len(want[name]), (name, len(got[name]), len(want[name]))
