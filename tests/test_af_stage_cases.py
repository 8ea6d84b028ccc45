"""The CPU side of the AF stage's sweep (tests/af_stage_cases.py): the oracle's two precisions confirm that the table's signals
make a 1e-5 bar against the float64 master meaningful at every filter length, the oracle accepts every length the library
accepts (1 tap and up) without moving a bit of what it computed at 63 taps and more, and it refuses the same combinations of AF
filter and squelch filters as the library.  Nothing here measures a kernel: that is tests/test_gpu_af_stage_sweep.py."""
import functools
import math

import numpy as np
import pytest

from oracle import sdr_oracle as so
from tests import af_stage_cases as ac


@pytest.mark.parametrize("ntaps_af", ac.LENGTHS)
def test_float32_mirror_stays_within_a_quarter_of_the_bar_of_the_master(ntaps_af):
    """The condition that makes ``TOL`` against the float64 master a statement about the kernels: at this filter length the
    oracle's own float32 form is within TOL / 4 = 2.5e-6 of it, for every sub-receiver, on the baseband IQ and on the audio of
    every call of the ragged list, relative to the call's own peak -- exactly as the GPU sweep judges the kernels.  (A mode that
    misses gets another signal, not another bound: af_stage_cases says which signal each mode ended up with.)"""
    m64, m32 = ac.run_oracle(ntaps_af, np.float64), ac.run_oracle(ntaps_af, np.float32)
    for r, mode in enumerate(ac.MODES):
        worst_iq = worst_am = 0.0
        for (iq64, am64), (iq32, am32) in zip(m64[r], m32[r]):
            worst_iq = max(worst_iq, ac.relerr(iq32, iq64))
            worst_am = max(worst_am, ac.relerr(am32, am64))
        print(f"AFSWEEP mirror T={ntaps_af} mode {mode} iq {worst_iq:.2e} am {worst_am:.2e}")
        assert worst_iq <= ac.COND and worst_am <= ac.COND, (ntaps_af, mode, worst_iq, worst_am)


def test_the_call_list_holds_what_it_is_there_for():
    assert ac.CALLS[:7] == ac.ragged_calls(ac.L)
    n = [len(iq) for iq in baseband()[0]]
    starts = [int(s) for s in ac.call_starts([(iq, None) for iq in baseband()[0]])]
    assert n == [1024, 1024, 24, 0, 1024, 2048, 8, 7, 2050, 1024, 3]
    assert 0 in n and any(0 < v < 8 for v in n)                          # a call without output, calls of fewer than 8
    odd = [(s, v) for s, v in zip(starts, n) if s % 2]                   # calls that start at an odd absolute output (par = 1)
    assert any(v > 2048 for _, v in odd) and any(v == 1024 for _, v in odd) and any(v < 8 for _, v in odd)
    assert 5 * ac.L <= sum(ac.CALLS) and max(ac.CALLS) <= 3 * ac.L       # the identities' five chunks; max_batch_chunks = 3


# ---- the oracle accepts what the library accepts ---------------------------------------------------------------------------------
class DemodulatorAsItWas:
    """Demodulator.process as it stood while its slices were anchored on hl = ntaps - 1 (ntaps >= 3 only; the ratio squelch's
    history right from 63 taps on): a copy of those expressions, the arrays the new form must reproduce bit for bit."""

    def __init__(self, fs_out, ntaps_af, dtype):
        self.fs_out, self.ntaps, self.rd = float(fs_out), int(ntaps_af), dtype
        self.cd = np.complex64 if dtype == np.float32 else np.complex128
        self.am_pll = so.CarrierPLL(fs_out, dtype)
        self.yhist = np.zeros(self.ntaps + 1, self.cd)
        self.vhist = np.zeros(self.ntaps - 1, self.cd)
        self.m_abs = 0

    def set_taps(self, c):
        self.taps = np.asarray(c, np.complex128).astype(self.cd)

    def process(self, y, mode, bfo):
        y = np.asarray(y, self.cd)
        n, hl = len(y), self.ntaps - 1
        ybuf = np.concatenate((self.yhist, y))
        if mode == "AM-Synch":
            v = self.am_pll.process(y).astype(self.cd)
            d = np.concatenate((self.vhist, v))
            self.vhist = d[len(d) - hl:]
        elif mode == "AM":
            d = np.abs(ybuf[2:]).astype(self.rd).astype(self.cd)
        elif mode == "NFM":
            scale = self.rd(self.fs_out / (2 * math.pi * so.NFM_FULL_SCALE_DEV))
            d = (so.nfm_discriminator(ybuf, self.rd) * scale).astype(self.cd)
        elif mode == "CW":
            fw, _ = so.freq_word(bfo, self.fs_out)
            idx = self.m_abs - hl + np.arange(hl + n, dtype=np.int64)
            ph = ((idx % so.TWO32) * fw) % so.TWO32
            d = (ybuf[2:] * so.phase_to_cplx(ph.astype(np.uint32), self.cd)).astype(self.cd)
        else:
            d = ybuf[2:]
        a = np.convolve(d, self.taps, mode='valid') if n else d[:0]
        dr = d.real.astype(self.rd)
        self.last_hp = np.abs(dr[hl:] - self.rd(2) * dr[hl - 1:-1] + dr[hl - 2:-2]).astype(self.rd) if n else dr[:0]
        self.last_det = dr[hl - (so.SQ_RATIO_TAPS - 1):] if n else dr[:0]
        self.yhist = ybuf[len(ybuf) - (hl + 2):]
        self.m_abs += n
        return a.astype(self.cd)


@functools.lru_cache(maxsize=1)
def baseband():
    """Per sub-receiver of the table, per call: the float32 oracle's baseband IQ (what the AF stage is fed)."""
    return [[iq for iq, _ in per] for per in ac.run_oracle(255, np.float32)]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("ntaps_af", [63, 64, 255, 1001])
def test_oracle_at_63_taps_and_more_is_bit_identical_to_what_it_was(ntaps_af):
    for r, rx in enumerate(ac.CFG['rx']):
        mode, bfo, af_bw = rx['mode'], rx.get('bfo', 0.0), rx.get('af_bw', 0.0)
        taps = so.af_taps_for_mode(mode, so.Receiver._af_index(af_bw), af_bw, bfo, ac.fc.FS_OUT, ntaps_af)
        new, old = so.Demodulator(ac.fc.FS_OUT, ntaps_af, np.float32), DemodulatorAsItWas(ac.fc.FS_OUT, ntaps_af, np.float32)
        new.set_taps(taps); old.set_taps(taps)
        for k, y in enumerate(baseband()[r]):
            a, b = new.process(y, mode, bfo), old.process(y, mode, bfo)
            assert same_bits(a, b), (ntaps_af, mode, k)
            assert same_bits(new.last_hp, old.last_hp), (ntaps_af, mode, k)
            assert same_bits(new.last_det, old.last_det), (ntaps_af, mode, k)
            assert len(new.last_hp) == len(y) and len(new.last_det) == (len(y) + so.SQ_RATIO_TAPS - 1 if len(y) else 0)


@pytest.mark.parametrize("ntaps_af", [1, 2, 3, 12, 62])
def test_oracle_runs_below_63_taps_with_real_detector_history(ntaps_af):
    """One long call == the ragged calls, for the outputs and for what the two squelches read -- which holds only if the detector
    history kept across calls is real (a wrapped negative index or a history of zeros would show at every cut)."""
    for r, rx in enumerate(ac.CFG['rx']):
        mode, bfo, af_bw = rx['mode'], rx.get('bfo', 0.0), rx.get('af_bw', 0.0)
        taps = so.af_taps_for_mode(mode, so.Receiver._af_index(af_bw), af_bw, bfo, ac.fc.FS_OUT, ntaps_af)
        cut, whole = so.Demodulator(ac.fc.FS_OUT, ntaps_af, np.float64), so.Demodulator(ac.fc.FS_OUT, ntaps_af, np.float64)
        cut.set_taps(taps); whole.set_taps(taps)
        ys = [y.astype(np.complex128) for y in baseband()[r]]
        a2 = whole.process(np.concatenate(ys), mode, bfo)
        assert len(a2) == sum(len(y) for y in ys)
        hist = so.SQ_RATIO_TAPS - 1
        det2 = whole.last_det                                        # the stream's detector output behind 62 zeros of history
        assert len(det2) == len(a2) + hist and not np.any(det2[:hist])
        a1, hp1, pos = [], [], 0
        for y in ys:
            a1.append(cut.process(y, mode, bfo)); hp1.append(cut.last_hp)
            if len(y):
                assert np.array_equal(cut.last_det, det2[pos:pos + len(y) + hist]), (mode, ntaps_af, pos)
            pos += len(y)
        # (float64; np.convolve may group an output's sum differently in a long call)
        assert np.allclose(np.concatenate(a1), a2, rtol=0, atol=1e-12 * np.max(np.abs(a2)))
        assert np.array_equal(np.concatenate(hp1), whole.last_hp)


# ---- the ratio squelch's bound -----------------------------------------------------------------------------------------------------
def test_squelch_bound_per_length_and_the_oracle_refuses_what_the_library_refuses():
    want = {1: 15, 12: 15, 13: 27, 40: 47, 41: 51, 48: 51, 49: 63, 60: 63, 61: 64, 255: 64, 2048: 64}
    for t, b in want.items():
        assert so.sq_ratio_taps_bound(t) == b, (t, so.sq_ratio_taps_bound(t))
    for t in range(1, 300):
        hy, H = so.af_history(t), -(-t // 12) * 12
        assert hy % 16 == 0 and hy >= -(-t // 8) * 8 + 5 and hy - 16 < -(-t // 8) * 8 + 5
        assert so.sq_ratio_taps_bound(t) == min(so.SQ_TAPS_MAX, H + 3, hy - 1)
        assert so.sq_ratio_taps_bound(t) <= so.sq_ratio_taps_bound(t + 1)
    cfg = ac.squelch_cfg()
    for t, ok in ((48, False), (49, True), (255, True)):
        o = so.make_receivers(cfg, np.float32, ntaps_af=t)[0]
        if ok:
            o.squelch_ratio = np.float32(2.0)
            assert o.squelch_ratio == np.float32(2.0)
        else:
            with pytest.raises(ValueError, match=r"63 taps.*48 taps"):
                o.squelch_ratio = np.float32(2.0)
            assert o.squelch_ratio == 0
            o.squelch_ratio = np.float32(0)          # disarming is always allowed


@pytest.mark.parametrize("ntaps_af", ac.RATIO_LENGTHS)
def test_ratio_squelch_case_crosses_its_threshold_with_a_margin(ntaps_af):
    """The GPU test holds the two envelopes to 1e-4 and asks for equal gates: every chunk's sq1 / sq2 is at least 1e-3 away from
    the threshold, and the gate takes both states within the accepted run."""
    c = ac.ratio_case(ntaps_af)
    assert c['K'] == so.sq_ratio_taps_bound(ntaps_af) == len(c['lp']) == len(c['hp']) == len(c['lp1']) - 1
    gate = [r >= c['thr'] for r in c['ratios']]
    assert all(abs(r / c['thr'] - 1.0) > 1e-3 for r in c['ratios']), (c['thr'], c['ratios'])
    assert any(gate[:ac.RATIO_CHUNKS]) and not all(gate[:ac.RATIO_CHUNKS])


def test_noise_squelch_case_opens_and_closes_in_the_oracle():
    """The GPU test's stream does what it is there for, at the shortest filter: the gate is open on the carrier and closed from
    the chunk in which it goes off the air (chunks 4 .. 7; the smoothed level, 2.5 there, decays by 0.36 per chunk and is still
    0.0503 behind chunk 11: the gate stays closed to the end), and no chunk's level is so close to the threshold that equal
    gates would be a matter of rounding (the GPU test holds the level to 1e-4)."""
    cfg = ac.squelch_cfg()
    x = ac.squelch_stream(cfg, 12, (4, 7))
    o = so.make_receivers(cfg, np.float32, ntaps_af=1)[0]
    o.squelch = np.float32(0.05)
    gate = []
    for k in range(12):
        o.demod_data(x[k * ac.L:(k + 1) * ac.L])
        gate.append(o.sq_open)
        assert abs(float(o.sq_level) / 0.05 - 1.0) > 5e-3, (k, o.sq_level)
    assert all(gate[:4]) and not any(gate[4:]), gate
