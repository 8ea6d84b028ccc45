"""The channel bank in terms of the oracle.  Test infrastructure only.

``BankOracle`` holds, per channel, one ``so.Demodulator`` with the AF taps set, one ``so.AGC`` and the block-noise squelch
lines of ``so.Receiver.demod_data``; a call without outputs skips AGC and squelch (the one deliberate difference from the
receiver, which decays its AGC on an empty chunk).  ``case`` builds the inputs the CPU and the GPU tests share."""
import copy
import types

import numpy as np

from oracle import sdr_oracle as so

SQUELCH = 0.3
SPACING = 12.5e3           # fs / M of every case: an NFM band plan

# (M, D, channels, AF taps): the shapes of the GPU parity tests; None = all rows.  255 = 31 steps of eight taps and a tail
# of 7, 125 = 15 and a tail of 5, 64 = whole steps only.  At M / D = 4 the decimator's run-in lasts 32 outputs, over which
# neighbouring carriers beat: the discriminator is ill-conditioned up to output 13 there, so with 255 taps the allowance
# would reach output 268 -- with 125 it ends at 138 and "carrier channels from output 256 on" holds as at the other shapes.
# At the larger shapes the carriers fade in over 32 frames (see case): their channels are noise until then, so the allowance
# of a carrier channel can reach output 32 + T - 1; 191 taps (23 steps and a tail of 7) keep that below 256.  (The default
# of 255 taps at 640 channels, carriers at full amplitude from sample 0, runs in AM: tests/test_gpu_bank.py.)
SHAPES = [(64, 32, None, 255), (64, 16, None, 125), (250, 125, (240, 20), 64), (640, 320, None, 191),
          (4096, 2048, (4090, 12), 191)]
BASE = SHAPES[0]
AF_BW = 4e3
FRAMES = 2400            # of the larger shapes (the base case: 4000)
BIG = 2100               # outputs of the one long call of a stream of at least 3944 frames; the kernel's tile is 2048


class BankOracle:
    def __init__(self, nk, fs_out, taps, mode, squelch=0.0, agc=True, dtype=np.float32):
        self.rd, self.nk, self.mode = dtype, int(nk), mode
        self.squelch, self.agc_on = dtype(squelch), bool(agc)
        proto = so.Demodulator(fs_out, len(taps), dtype)
        self.demod = []
        for _ in range(self.nk):
            d = copy.copy(proto)                      # (the constructor designs two filter banks: once is enough)
            d.yhist, d.vhist = proto.yhist.copy(), proto.vhist.copy()
            self.demod.append(d)
        self.agc = [so.AGC(dtype) for _ in range(self.nk)]
        self.level = np.zeros(self.nk, dtype)
        self.open = np.ones(self.nk, bool)
        self.set_mode(mode, taps)

    def set_mode(self, mode, taps=None):
        self.mode = mode
        if taps is not None:
            for d in self.demod:
                d.set_taps(taps)

    def process(self, rows):
        """rows [nk, n_out] of one call -> dict of a, am [nk, n_out], gain (as applied: 0 where closed), agc, maxbuf,
        level, open [nk]"""
        rd = self.rd
        rows = np.asarray(rows)
        n = rows.shape[1]
        a_all, am_all = np.zeros((self.nk, n), rd), np.zeros((self.nk, n), rd)
        gain = np.ones(self.nk, rd)
        for ch in range(self.nk):
            dm = self.demod[ch]
            a = dm.process(rows[ch], self.mode, 0.0).real.astype(rd)
            if n == 0:
                continue
            peak = np.max(np.abs(a))
            g = self.agc[ch].update(peak, self.agc_on and self.mode in so.AGC_MODES)
            if self.mode == 'NFM' and self.squelch > 0:            # so.Receiver.demod_data, the block-noise squelch
                noise = rd(np.sum(dm.last_hp.astype(np.float64)) / len(a))
                self.level[ch] = rd(self.level[ch] + rd(so.SQUELCH_ALPHA) * rd(noise - self.level[ch]))
                self.open[ch] = bool(self.level[ch] <= rd(self.squelch))
                if not self.open[ch]:
                    g = rd(0)
            a_all[ch], am_all[ch], gain[ch] = a, (a * g).astype(a.dtype), g
        return dict(a=a_all, am=am_all, gain=gain, agc=np.array([x.agc for x in self.agc], rd),
                    agc_gain=np.array([x.gain for x in self.agc], rd), maxbuf=np.array([x.maxbuf for x in self.agc], rd),
                    level=self.level.copy(), open=self.open.copy())

    def allowance(self, ch, iq_all):
        """tests.test_gpu_parity.nfm_rounding_allowance of channel ch, given all of its samples so far"""
        from tests.test_gpu_parity import nfm_rounding_allowance
        return nfm_rounding_allowance(types.SimpleNamespace(demod=self.demod[ch]), iq_all)


# ---- the shared input -------------------------------------------------------------------------------------------------
def carriers(M, base):
    """(k, amplitude, tone Hz, deviation Hz).  The base case is the one checked by hand.  The larger shapes put carriers on
    k = 0's two neighbours, on the Nyquist channel's neighbour, four channels off k = 0's neighbours (inside the circular
    ranges the tests store) and a weak one far from all of them: next to a carrier ten times stronger the decimator's
    run-in leaks enough of the neighbour to make the weak channel's first discriminator outputs ill-conditioned for
    longer than 256 outputs, which is a property of that input, not of any implementation."""
    if base:
        return [(3, 0.30, 1e3, 3e3), (10, 0.10, 400.0, 2.5e3), (59, 0.03, 700.0, 1.5e3), (31, 0.2, 300.0, 4e3)]
    return [(1, 0.30, 1e3, 3e3), (M - 1, 0.20, 400.0, 2.5e3), (M // 2 - 1, 0.2, 300.0, 4e3), (5, 0.10, 500.0, 2e3),
            (M - 5, 0.15, 600.0, 3.5e3), (M // 4 + 3, 0.03, 700.0, 1.5e3)]


def rows_of(M, channels):
    return np.arange(M) if channels is None else (channels[0] + np.arange(channels[1])) % M


def case(M, D, channels=None, frames=None, hard=None):
    """-> dict(fs, x complex64, cuts (call lengths), rows (channel of every stored row), carrier_rows).  hard: the carriers
    start at full amplitude at sample 0 (the base case's default); otherwise they fade in over the first 32 frames."""
    base = (M, D) == BASE[:2]
    frames = (4000 if base else FRAMES) if frames is None else frames
    hard = base if hard is None else hard
    fs = SPACING * M
    N = D * frames
    rng = np.random.default_rng(7)
    x = 1e-3 * np.sqrt(M / 64) * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    n = np.arange(N)
    cs = carriers(M, base)
    # base case: the carriers start at full amplitude at sample 0, as given.  Larger shapes: they fade in over the first 32
    # frames -- a hard start leaks through the partly filled prototype into every channel, and the more channels there
    # are, the more of them pass close to zero during the run-in with discriminator outputs in the hundreds, where float32
    # itself (the float32 against the float64 helper) is further than 1e-5 of full scale from the truth
    ramp = np.ones(N) if hard else 0.5 - 0.5 * np.cos(np.pi * np.minimum(n / (32.0 * D), 1.0))
    for k, A, fm, dev in cs:
        x += ramp * A * np.exp(1j * (2 * np.pi * ((k * n) % M) / M + (dev / fm) * np.sin(2 * np.pi * fm * n / fs)))
    # calls: one output (n < D), three, none (n = 1), then about 300 outputs each, odd lengths -- but the seventh of those
    # (the tenth call: the start-up transient of the squelch levels has decayed by then),
    # where the stream is long enough, completes BIG outputs: more than one tile of the kernel and no whole number of them
    cuts, pos, i = [7, 3 * D + 5 - 7, 1], 3 * D + 6, 0
    steps = [300 * D + 11, 297 * D - 5, 303 * D + 1]
    while N - pos > 0:
        c = BIG * D + 7 if i == 6 and N - pos >= (BIG + 40) * D else min(steps[i % 3], N - pos)
        if N - pos - c < 40 * D:                     # no stub at the end
            c = N - pos
        cuts.append(c)
        pos, i = pos + c, i + 1
    assert sum(cuts) == N
    rows = rows_of(M, channels)
    ck = [k for k, *_ in cs]
    return dict(fs=fs, M=M, D=D, x=x.astype(np.complex64), cuts=cuts, rows=rows,
                carrier_rows=[int(a) for a in range(len(rows)) if rows[a] in ck])


def split(x, cuts):
    out, i = [], 0
    for c in cuts:
        out.append(x[i:i + c])
        i += c
    return out


def cut_rows(y, cuts, D):
    """the full-stream rows [nk, n_frames] cut into what each call completes"""
    out, s = [], 0
    for c in cuts:
        m0, m1 = -(-s // D), -(-(s + c) // D)
        out.append(y[:, m0:m1])
        s += c
    return out
