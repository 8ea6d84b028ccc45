"""The Python layer of the FT8 and FT4 skimmers -- the decoder bank, the skimmer's release rule, owner filter, frame report
and second pass, and the public surface of ``pysdr_amd.ft8`` and ``pysdr_amd.ft4`` -- against a recorded trace, in the way of
tests/test_chan_py_trace.py, whose ``Recorder``, ``enc`` and ``samples`` it uses: every C call (tests/fake_pysdr_lib.py stands
in for the ``pysdr_ft8_*`` / ``pysdr_ft4_*`` handle calls) and what every Python method returned, in order, compared with
tests/golden/ft_py_trace.json (written by tests/golden/make_ft_py_trace_golden.py).  Records are noted exactly, but for
``snr``, which went through log10 and is noted to 12 significant digits.  A release cycle is a ``push`` that returned
records.  CPU only."""
import importlib
import inspect
import json
import os
import types

import numpy as np

from tests.fake_pysdr_lib import FakeLib
from tests.test_chan_py_trace import Recorder, _accepts, enc, samples

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ft_py_trace.json")
MODES = ("ft8", "ft4")
HANDLE_CALLS = ("create", "destroy", "reset", "sync", "process", "fetch", "state", "llr", "decode", "decode_osd", "decode_llr",
                "decode_llr_osd", "report", "floor", "keep", "subtract", "rescan", "pass_decode", "pass_llr", "pass_state")
T_FIRST = 1.7e9 + 3.25
RECORDS = []                                     # every record the skimmer runs returned (the golden's maker looks at them)

BANK_ATTRS = ("KIND", "DESTROY", "S", "nsub", "nb", "qs", "nk", "D", "fs_out", "nfine", "max_out", "cap", "slots", "plan", "tr", "tw",
              "t_done", "last_n_out", "kept")
SKIMMER_ATTRS = ("fs", "baud", "t_first", "decode", "keep_llr", "report", "passes", "reach_t", "S", "D", "M", "nsub", "qs", "h", "nk",
                 "nfine", "fs_out", "freqs", "freqs_fine", "circular", "records")


def mode(name):
    m = importlib.import_module("pysdr_amd." + name)
    return m, getattr(m, m.NAME + "_Decoders"), getattr(m, m.NAME + "_Skimmer")


def tidy(v):
    """records with ``snr`` at 12 significant digits"""
    if isinstance(v, dict):
        return {k: (float(f"{e:.12g}") if k == "snr" and e is not None else tidy(e)) for k, e in v.items()}
    if isinstance(v, (list, tuple)):
        return [tidy(e) for e in v]
    return v


def walk_bank(rec, name, fs, whole):
    """``whole``: every call of the bank; otherwise the constructor, one call and ``keep`` (the tables at the other S)"""
    from pysdr_amd.channelizer import Channelizer
    m, Dec, _ = mode(name)
    lb = f"{name}@{fs}"
    S, D, M = m.shape(fs)
    ch = Channelizer(fs, M, D, m.prototype(fs, M, S), (3, 3), 0, 1 << 16)
    d = Dec(ch, S, 64)
    rec.attrs(lb, d, BANK_ATTRS)
    rec(f"{lb}.cfg", m.cfg_dict, d.cfg)
    rec(f"{lb}.decode residual before keep", d.decode, [0], [0], residual=True)
    rec(f"{lb}.subtract before keep", d.subtract, [0], [0], np.zeros((1, 91), np.uint8), np.zeros((1, 9, 2), np.int32))
    rec(f"{lb}.keep", d.keep, 16)
    rec.attrs(lb, d, ("kept",))
    rec(f"{lb}.decode_raw all", d.decode_raw, samples(80, 40 * D), events="all")
    if not whole:
        rec(f"{lb}.close", d.close)
        ch.close()
        return
    rec(f"{lb}.decode_raw counts", d.decode_raw, samples(81, 17 * D + 3), events="counts")
    rec(f"{lb}.decode_raw None", d.decode_raw, samples(82, D), events=None)
    rec(f"{lb}.decode_raw empty", d.decode_raw, samples(83, 0))
    rec(f"{lb}.decode_raw device", d.decode_raw, 0x10000, 5 * D, on_device=True)
    rec.attrs(lb, d, ("t_done", "last_n_out"))
    rec.attrs(lb, ch, ("n_in",))
    ev = []
    while len(ev) < 3:                                                   # 64 outputs a call, until three frames are whole and in the ring
        r = d.decode_raw(0x10000, 64 * D, on_device=True)
        ev = [e for e in ev if d.t_done - e[0] <= d.tr - 8]
        if r["counts"].any():
            got = rec(f"{lb}.events_of", d.events_of, r)
            rows = np.flatnonzero(r["counts"])
            assert got == d.events_of(r, rows, rec(f"{lb}.fetch", d.fetch, rows))
            ev += got
    rec(f"{lb}.fetch ends", d.fetch, [d.nfine - 1, 0])
    rec.attrs(lb, d, ("t_done", "last_n_out"))
    F, t = [e[1] for e in ev], [e[0] for e in ev]
    F1, t1 = F[:1] * 4097, t[:1] * 4097
    rec(f"{lb}.llr 0", d.llr, [], [])
    rec(f"{lb}.llr 1", d.llr, F[:1], t[:1])
    rec(f"{lb}.llr 4097", d.llr, F1, t1)
    rec(f"{lb}.llr off the raster", d.llr, [d.nfine], t[:1])
    rec(f"{lb}.llr not whole yet", d.llr, F[:1], [d.t_done])
    rec(f"{lb}.decode", d.decode, F, t)
    rec(f"{lb}.decode post", d.decode, F, t, post=True)
    rec(f"{lb}.decode osd", d.decode, F, t, osd=1)
    full = rec(f"{lb}.decode post osd detail", d.decode, F, t, m_ldpc().params(20, 0.75), post=True, osd=m_ldpc().osd_params(2), detail=True)
    rec(f"{lb}.decode 4097", d.decode, F1, t1)
    rec(f"{lb}.decode detail without osd", d.decode, F, t, detail=True)
    llr = np.random.default_rng(7).standard_normal((5, 174)).astype(np.float32)
    rec(f"{lb}.decode_llr", d.decode_llr, llr)
    rec(f"{lb}.decode_llr post osd detail", d.decode_llr, llr, post=True, osd=0, detail=True)
    rec(f"{lb}.decode_llr 4097", d.decode_llr, np.zeros((4097, 174), np.float32))
    rec(f"{lb}.decode_llr not finite", d.decode_llr, np.full((1, 174), np.inf, np.float32))
    rep = rec(f"{lb}.report", d.report, F, t, full["bits"])
    rec(f"{lb}.report 4097", d.report, F1, t1, np.ones((4097, 91), np.uint8))
    rec(f"{lb}.floor", d.floor)
    rec(f"{lb}.floor explicit", d.floor, max(t) + 8, 3)
    rec(f"{lb}.floor 129", d.floor, None, 129)
    rec(f"{lb}.state", d.state)
    rec(f"{lb}.state ring", d.state, ring=True)
    grid = [rec(f"{lb}.trial_grid", m.trial_grid, m, *m.refine(s)[:2], d.qs, d.fs_out) for s in rep["sig9"]]
    rec(f"{lb}.subtract", d.subtract, F, t, full["bits"], grid)
    rec(f"{lb}.subtract 257", d.subtract, F[:1] * 257, t[:1] * 257, np.zeros((257, 91), np.uint8), grid[:1] * 257)
    rec(f"{lb}.rescan", d.rescan, 0, d.nfine - 1, max(0, t[0] - 16), t[0] + 16)
    rec(f"{lb}.rescan cfg", d.rescan, 2, 2, t[0], t[0], m.params(1.0, 2))
    rec(f"{lb}.rescan 257 steps", d.rescan, 0, 3, 0, 248)
    rec(f"{lb}.pass_llr", d.pass_llr, F, t)
    rec(f"{lb}.pass_llr 4097", d.pass_llr, F1, t1)
    rec(f"{lb}.pass_state", d.pass_state)
    rec(f"{lb}.decode residual", d.decode, F, t, residual=True)
    rec(f"{lb}.decode residual osd detail", d.decode, F, t, residual=True, osd=1, detail=True)
    rec(f"{lb}.keep late", d.keep)
    rec(f"{lb}.sync", d.sync)
    rec(f"{lb}.reset", d.reset)
    rec.attrs(lb, d, ("t_done", "last_n_out", "kept"))
    rec.attrs(lb, ch, ("n_in",))
    rec(f"{lb}.keep after reset", d.keep, None, 4)
    rec(f"{lb}.close", d.close)
    rec(f"{lb}.close", d.close)
    rec.attrs(lb, d, ("_h",))
    rec(f"{lb}.decode_raw after close", d.decode_raw, samples(84, 4))
    ch.close()


def m_ldpc():
    from pysdr_amd import ldpc
    return ldpc


def scenario_bank(rec):
    for name, (fs, other) in zip(MODES, ((8000, 12000), (8000, 12000))):
        walk_bank(rec, name, fs, True)
        walk_bank(rec, name, other, False)


def scenario_refusals(rec):
    from pysdr_amd.channelizer import Channelizer
    for name in MODES:
        m, _, Sk = mode(name)
        kw = dict(channels=(3, 3), max_out=256)
        rec(f"{name} passes=3", Sk, 8000, passes=3, **kw)
        rec(f"{name} passes=2 without decode", Sk, 8000, passes=2, **kw)
        rec(f"{name} passes=2 with report", Sk, 8000, passes=2, decode=True, report=True, **kw)
        rec(f"{name} osd without decode", Sk, 8000, osd=1, **kw)
        rec(f"{name} report without decode", Sk, 8000, report=True, **kw)
        rec(f"{name} no raster", Sk, 8001, **kw)
        S, D, M = m.shape(8000)
        ch = Channelizer(8000, M, D, m.prototype(8000, M, S), (3, 3))
        rec(f"{name} chan at the wrong rate", Sk, 16000, chan=ch, max_out=256)
        ch.close()


def run_skimmer(rec, lb, sk, seed):
    """three release cycles in ragged pieces, reset, one more, close"""
    rec.attrs(lb, sk, SKIMMER_ATTRS)
    rec.attrs(lb + ".dec", sk.dec, BANK_ATTRS)
    big = sk.dec.max_samples()
    sizes = (3 * big + 1, big - 3, 4 * big, 17, 2 * big + 7)
    i = 0
    for cycles in (3, 1):
        got = 0
        while got < cycles:
            assert i < 120, (lb, i)
            n = sizes[i % len(sizes)]
            out = rec(f"{lb}.push({n})", lambda x: tidy(sk.push(x)), samples(seed + i, n))
            RECORDS.extend(out)
            got += bool(out)
            i += 1
        rec.attrs(lb, sk.dec, ("t_done", "last_n_out"))
        rec.attrs(lb, sk.chan, ("n_in",))
        assert len(sk.records) >= cycles
        if cycles == 3:
            recs = sk.records
            rec(f"{lb}.reset", sk.reset)
            rec.attrs(lb, sk, ("records",))
    rec(f"{lb}.sync", sk.sync)
    rec(f"{lb}.close", sk.close)
    rec(f"{lb}.close", sk.close)
    rec.attrs(lb, sk.dec, ("_h",))
    rec.attrs(lb, sk.chan, ("_h",))
    return recs


def scenario_skimmers(rec):
    for k, name in enumerate(MODES):
        m, _, Sk = mode(name)
        kw = dict(channels=(3, 3), max_in=1 << 16, max_out=256)
        run_skimmer(rec, f"{name} plain", Sk(8000, **kw), 100 + 1000 * k)
        recs = run_skimmer(rec, f"{name} report", Sk(12000, decode=True, keep_llr=False, osd=2, report=True, t_first=T_FIRST, **kw), 200 + 1000 * k)
        spots = rec(f"{name} spots", lambda: tidy(m.spots(recs)))
        for r in spots:
            rec(f"{name} spot_line", m.spot_line, r, 1500.0)
        bare = {k: v for k, v in spots[0].items() if k not in ("slot", "dt", "dt_fine")}
        rec(f"{name} spot_line without t_first", m.spot_line, bare)
        run_skimmer(rec, f"{name} passes", Sk(8000, decode=True, passes=2, reach_t=16, **kw), 300 + 1000 * k)
        rate = int(round(m.SHAPES[0] * m.BAUD))                          # the rows' rate; their spacing is a quarter of it
        band = (-0.3 * rate, 0.3 * rate)                                 # three rows
        ffs = next(f for f in range(8 * rate, 4096 * rate, rate) if _accepts(m.fine_channelizer, f, band))
        ch = m.fine_channelizer(ffs, band, max_in=1 << 16)
        run_skimmer(rec, f"{name} passes fine", Sk(ffs, chan=ch, max_out=256, decode=True, passes=2, reach_t=16), 400 + 1000 * k)


def _public(obj):
    return [(k, getattr(obj, k)) for k in sorted(dir(obj)) if not k.startswith("_")]


def _sig(v):
    return str(inspect.signature(v))


def _value(v):
    if isinstance(v, types.ModuleType):
        return "module " + v.__name__
    if isinstance(v, type):
        return f"class {v.__module__}.{v.__qualname__}"
    if callable(v):
        return _sig(v)
    if isinstance(v, (float, np.floating)):
        return f"{v:.12g}"
    return repr(v)


def scenario_surface(rec):
    """every public name of the two mode files that is not a module, nor the language's own ``annotations``, nor a class of
    the other mode (``ft4.py`` held ``FT8_*`` only to derive from them, which it need not)"""
    for name in MODES:
        m, Dec, Sk = mode(name)
        for k, v in _public(m):
            if isinstance(v, types.ModuleType) or k == "annotations" or (isinstance(v, type) and v.__module__ in
                                                                        {"pysdr_amd." + o for o in MODES if o != name}):
                continue
            rec.fake.note(f"{name}.{k} {_value(v)}")
            if v is Dec or v is Sk:
                for a, w in _public(v):
                    rec.fake.note(f"{name}.{k}.{a} {_value(w)}")


SCENARIOS = (scenario_bank, scenario_refusals, scenario_skimmers, scenario_surface)


def record(real, install):
    """-> {scenario name: [trace lines]}; ``install(fake)`` puts a fresh fake in place of the library before each scenario"""
    out = {}
    del RECORDS[:]
    for sc in SCENARIOS:
        fake = FakeLib(real)
        install(fake)
        sc(Recorder(fake))
        out[sc.__name__] = fake.trace
    return out


def test_the_ft_python_layer_makes_the_recorded_calls_and_returns_the_recorded_values(hiplib, monkeypatch):
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
