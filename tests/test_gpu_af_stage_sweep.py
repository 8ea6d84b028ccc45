"""The audio-rate tail (demod_fir_kernel<CPLX> and its epilogue, stage2.hip) at every AF filter length where its structure
changes, against the float64 master of the oracle.

The case table (tests/af_stage_cases.py) is one context of seven sub-receivers -- AM, NFM, AM-Synch, USB, LSB, CW and IQ: every
detector, all three arithmetic kinds of the inner product, both instantiations of the kernel -- on one stream cut into calls
without output, of 3, 7 and 8 outputs, of odd counts (later calls start at an odd absolute output) and of more than a workgroup
tile.  tests/test_af_stage_cases.py proves on any machine that the oracle's float32 form follows the master to a quarter of the
bar on these signals at every length.

The bar is the project's own: 1e-5 of the output peak, per sub-receiver and per call, on EVERY sample of the baseband IQ and of
the audio.  Two allowances, both the project's and neither new: AM-Synch is not compared over the first 1024 outputs of a stream
(tests/test_gpu_pll.py), and NFM gets nfm_rounding_allowance exactly as test_gpu_parity.run_both applies it.

The squelches depend on the AF filter's length through the staged image they read: the noise squelch two detector values back,
the ratio squelch its taps minus one -- more than a short AF filter stages or keeps, so pysdr_set_squelch_ratio refuses filters
longer than sq_taps_bound(ntaps_af) (common.h), and the oracle refuses the same."""
import functools

import numpy as np
import pytest

from oracle import sdr_oracle as so
from tests import af_stage_cases as ac
from tests import test_gpu_parity as tp

pytestmark = pytest.mark.gpu

TOL = ac.TOL
BATCH = 5                 # chunks of the bit-for-bit identities
AM_SYNCH_BATCH_BAR = 1e-5  # test_gpu_executive.test_am_synch_batched_slots_equal_the_chunked_run_within_the_parity_bar


@functools.lru_cache(maxsize=2)
def master(ntaps_af):
    return ac.run_oracle(ntaps_af, np.float64)


@pytest.mark.parametrize("ntaps_af", ac.LENGTHS)
def test_every_sample_against_the_float64_master(ntaps_af):
    m = master(ntaps_af)
    starts = [ac.call_starts(per) for per in m]
    x = ac.stream()
    P, g = tp.make_gpu_receivers(ac.CFG, af_filt_len=ntaps_af, max_batch_chunks=3)
    nfm = so.make_receivers(ac.CFG, np.float64, ntaps_af=ntaps_af)[ac.MODES.index("NFM")]    # (its taps: for the allowance)
    worst = {mode: [0.0, 0.0] for mode in ac.MODES}
    missed, iq_seen, pk, pos = [], [], 0.0, 0
    for k, c in enumerate(ac.CALLS):
        xc = x[pos:pos + c]
        pos += c
        for i, (rg, mode) in enumerate(zip(g, ac.MODES)):
            am_g = rg.demod_data(xc)
            iq_m, am_m = m[i][k]
            assert am_g.shape == am_m.shape and np.iscomplexobj(am_g) == (mode == "IQ"), (mode, k)
            e_iq = ac.relerr(rg.iq, iq_m)
            if mode == "AM-Synch":
                e_am = ac.relerr(ac.behind_pll_start(am_g, starts[i][k]), ac.behind_pll_start(am_m, starts[i][k]))
            elif mode == "NFM" and len(am_m):              # as run_both
                iq_seen.append(np.array(iq_m))
                allow = tp.nfm_rounding_allowance(nfm, np.concatenate(iq_seen))[-len(am_m):]
                pk = max(pk, float(np.max(np.abs(am_m[allow == 0]))) if np.any(allow == 0) else 0.0)
                excess = np.maximum(np.abs(am_g - am_m) - allow, 0.0)
                e_am = float(np.max(excess) / (pk if pk > 0 else 1.0))
            else:
                e_am = ac.relerr(am_g, am_m)
            worst[mode] = [max(worst[mode][0], e_iq), max(worst[mode][1], e_am)]
            if not (e_iq <= TOL and e_am <= TOL):
                missed.append((mode, k, len(am_m), e_iq, e_am))
    for mode in ac.MODES:
        print(f"AFSWEEP parity T={ntaps_af} mode {mode} iq {worst[mode][0]:.2e} am {worst[mode][1]:.2e}")
    assert not missed, missed


@pytest.mark.parametrize("ntaps_af", ac.LENGTHS)
def test_one_batch_equals_chunk_by_chunk(ntaps_af):
    """The first five chunks as one process_batch, as five demod_data calls and cut at random places: audio and IQ equal bit for
    bit for the six modes that promise it (under the random cuts the audio of the modes with an AGC has one gain per call: there
    the IQ, and the audio of NFM and IQ), AM-Synch's batch within the bar the project holds its segments to."""
    m = master(ntaps_af)
    x = ac.stream()[:BATCH * ac.L]
    n_batch = so.out_index_range(0, BATCH * ac.L, 3, 128)[1]
    iq_batch = [np.concatenate([iq for iq, _ in per])[:n_batch] for per in m]
    synch = ac.MODES.index("AM-Synch")
    P, worst = tp.check_does_not_depend_on_the_cut(ac.CFG, B=BATCH, x=x, want_iq=iq_batch, af_filt_len=ntaps_af,
                                                   am_bar={synch: AM_SYNCH_BATCH_BAR},
                                                   am_cut_rx=(ac.MODES.index("NFM"), ac.MODES.index("IQ")))
    print(f"AFSWEEP cut T={ntaps_af}: iq {worst:.2e}")


def zero_chunks(am, counts):
    pos = np.r_[0, np.cumsum(counts)]
    return [not np.any(am[pos[k]:pos[k + 1]]) for k in range(len(counts))]


@pytest.mark.parametrize("ntaps_af", [1, 3, 12, 13, 49])
def test_noise_squelch_at_short_af_filters(ntaps_af):
    """test_nfm_noise_squelch_mutes_when_the_carrier_drops at the filter lengths the oracle could not run or nothing ever ran:
    one NFM sub-receiver, 12 chunks, the carrier off the air for chunks 4 .. 7.  The gate equals the oracle's, the smoothed level
    is within 1e-4 of it, the audio within TOL or all zero while the gate is closed; the same chunks as one batch give the same
    gates and the same audio bits."""
    cfg, n, L = ac.squelch_cfg(), 12, ac.L
    x = ac.squelch_stream(cfg, n, (4, 7))
    P, g = tp.make_gpu_receivers(cfg, af_filt_len=ntaps_af)
    o = so.make_receivers(cfg, np.float32, ntaps_af=ntaps_af)
    g[0].squelch = 0.05
    o[0].squelch = np.float32(0.05)
    opened, am1, missed = [], [], []
    for k in range(n):
        xc = x[k * L:(k + 1) * L]
        ag, ao = g[0].demod_data(xc), o[0].demod_data(xc)
        am1.append(ag.copy())
        lvl, op = g[0].squelch_state
        opened.append(op)
        e_lvl = abs(lvl - float(o[0].sq_level)) / max(float(o[0].sq_level), 1e-3)
        e_am = ac.relerr(ag, ao)
        print(f"AFSWEEP squelch T={ntaps_af} chunk {k}: gate {int(op)} oracle {int(o[0].sq_open)} level {e_lvl:.2e} am {e_am:.2e}")
        if not (op == o[0].sq_open and e_lvl <= 1e-4 and (e_am <= TOL or (not op and not np.any(ag)))):
            missed.append((k, op, o[0].sq_open, e_lvl, e_am))
    assert not missed, missed
    assert all(opened[:4]) and not any(opened[4:8]), opened           # the gate really was open, and really closed
    P2, g2 = tp.make_gpu_receivers(cfg, af_filt_len=ntaps_af, max_batch_chunks=n)
    g2[0].squelch = 0.05
    ctx = P2._pysdr_stream
    ctx.process_batch(x, n, L, on_device=False)
    am, iq, cn, pk = ctx.fetch(0, n)
    assert list(cn) == [len(v) for v in am1]
    assert zero_chunks(am, cn) == [not np.any(v) for v in am1] == [not op for op in opened]
    assert np.array_equal(am.view(np.uint32), np.concatenate(am1).view(np.uint32))
    assert g2[0].squelch_state[1] == opened[-1]


def set_ratio(P, irx, thr, lp, hp):
    from pysdr_amd import _lib
    return _lib.lib().pysdr_set_squelch_ratio(P._pysdr_stream.h, irx, float(thr), _lib.as_pf(lp), _lib.as_pf(hp), len(lp))


@pytest.mark.parametrize("ntaps_af", ac.RATIO_LENGTHS)
def test_ratio_squelch_bound_follows_the_af_filter(ntaps_af):
    """Through the raw ABI, with squelch filters of exactly sq_taps_bound(ntaps_af) random taps (the oracle's _sq_taps the same):
    accepted, and over 10 chunks with the carriers off the air for chunks 4 .. 6 both envelopes are within 1e-4 of the oracle's
    per chunk and the gate is equal (the bars of test_ratio_squelch_follows_the_carrier_at_two_levels_20_db_apart); a batch of the
    same chunks gives the same gates and the same audio bits.  One tap more is refused -- for the other sub-receiver, with a
    message that names both lengths -- and the armed squelch goes on as if nothing had been asked: the next chunk still matches."""
    from pysdr_amd import _lib
    c = ac.ratio_case(ntaps_af)
    cfg, x, L, n = c['cfg'], c['x'], ac.L, ac.RATIO_CHUNKS
    P, g = tp.make_gpu_receivers(cfg, af_filt_len=ntaps_af)
    o = so.make_receivers(cfg, np.float32, ntaps_af=ntaps_af)
    assert set_ratio(P, 0, c['thr'], c['lp'], c['hp']) == 0, _lib.lib().pysdr_last_error()
    o[0]._sq_taps = (c['lp'], c['hp'])
    o[0].squelch_ratio = np.float32(c['thr'])
    opened, am1, missed, state = [], [], [], None

    def chunk(k):
        xc = x[k * L:(k + 1) * L]
        ag, ao = g[0].demod_data(xc), o[0].demod_data(xc)
        bg, bo = g[1].demod_data(xc), o[1].demod_data(xc)
        lo, hi, op = g[0].squelch_ratio_state
        e_lo, e_hi = abs(lo - float(o[0].sq_lp)) / float(o[0].sq_lp), abs(hi - float(o[0].sq_hp)) / float(o[0].sq_hp)
        e_am, e_bm = ac.relerr(ag, ao), ac.relerr(bg, bo)
        print(f"AFSWEEP ratio T={ntaps_af} K={c['K']} chunk {k}: gate {int(op)} oracle {int(o[0].sq_open)} sq1 {e_lo:.2e} sq2 {e_hi:.2e} "
              f"am {e_am:.2e} other rx {e_bm:.2e}")
        ok = op == o[0].sq_open and e_lo <= 1e-4 and e_hi <= 1e-4
        # (every chunk, the first included: a 63-tap decimator has filled within a few outputs)
        if not (ok and (e_am <= TOL or (not op and not np.any(ag))) and e_bm <= TOL):
            missed.append((k, op, o[0].sq_open, e_lo, e_hi, e_am, e_bm))
        return ag.copy(), (lo, hi, op)

    for k in range(n):
        ag, state = chunk(k)
        am1.append(ag)
        opened.append(state[2])
    assert not missed, missed
    assert any(opened) and not all(opened), opened
    # one tap more: refused, whichever sub-receiver asks, before anything of the context's is touched
    for irx in (1, 0):
        assert set_ratio(P, irx, c['thr'], c['lp1'], c['hp1']) == -1               # PYSDR_ERR_ARG
        msg = _lib.lib().pysdr_last_error().decode()
        assert f"{c['K'] + 1} taps" in msg and f"{ntaps_af} taps" in msg, msg
    o[1]._sq_taps = (c['lp1'], c['hp1'])
    with pytest.raises(ValueError):
        o[1].squelch_ratio = np.float32(c['thr'])
    chunk(n)
    assert not missed, missed
    # the accepted run's chunks as one batch
    P2, g2 = tp.make_gpu_receivers(cfg, af_filt_len=ntaps_af, max_batch_chunks=n)
    assert set_ratio(P2, 0, c['thr'], c['lp'], c['hp']) == 0
    ctx = P2._pysdr_stream
    ctx.process_batch(x[:n * L], n, L, on_device=False)
    am, iq, cn, pk = ctx.fetch(0, n)
    assert list(cn) == [len(v) for v in am1]
    assert zero_chunks(am, cn) == [not np.any(v) for v in am1] == [not op for op in opened]
    assert np.array_equal(am.view(np.uint32), np.concatenate(am1).view(np.uint32))
    s2 = g2[0].squelch_ratio_state
    assert s2[2] == state[2] and abs(s2[0] - state[0]) <= 1e-5 * state[0] and abs(s2[1] - state[1]) <= 1e-5 * state[1]


def test_ratio_squelch_bound_follows_the_af_filter_through_the_facade():
    """rx.squelch_ratio designs 63 taps: beside 48 AF taps the library refuses them and the attribute keeps its old value, beside
    49 it arms."""
    from pysdr_amd import _lib
    cfg = ac.squelch_cfg()
    P, g = tp.make_gpu_receivers(cfg, af_filt_len=48)
    with pytest.raises(_lib.PysdrError, match="63 taps.*48 taps"):
        g[0].squelch_ratio = 2.0
    assert g[0].squelch_ratio == 0.0
    x = ac.squelch_stream(cfg, 2, (1, 1))
    g[0].demod_data(x[:ac.L])
    assert np.any(g[0].demod_data(x[ac.L:]))                 # not armed: noise alone passes
    P, g = tp.make_gpu_receivers(cfg, af_filt_len=49)
    g[0].squelch_ratio = 2.0
    assert g[0].squelch_ratio == 2.0
