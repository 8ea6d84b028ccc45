"""The channel bank's complex-tap modes USB / LSB / CW in terms of the oracle.  Test
infrastructure only.

``SidebandOracle`` is ``bank_oracle.BankOracle`` with the BFO handed to ``so.Demodulator.process`` (AM and NFM run as
in the base class, so one helper follows a bank through mode switches) and, per call and channel, the **scale** the
sideband comparisons are normalised by: max |y| over the call's outputs and the T - 1 row samples before them -- what
the call's AF windows hold.  The call's own max |a| is no measure here: a sideband filter cancels most of a strong
channel's input, and a call of one output can land on Re a ~ 0."""
import numpy as np

from oracle import sdr_oracle as so
from tests import bank_oracle as bo

BFO = 700.0
AF_BW = {"USB": 3e3, "LSB": 3e3, "CW": 500.0, "AM": bo.AF_BW, "NFM": bo.AF_BW}
AF_IDX = {3e3: so.AF_BWs.index("3 KHz"), 500.0: so.AF_BWs.index("500 Hz"), bo.AF_BW: so.AF_BWs.index("4 KHz")}


def taps(mode, fs_out, T, af_bw=None, bfo=BFO):
    """the oracle's own taps of a sub-receiver in that mode (complex128)"""
    bw = AF_BW[mode] if af_bw is None else af_bw
    return so.af_taps_for_mode(mode, AF_IDX[bw], bw, bfo, fs_out, T)


class SidebandOracle(bo.BankOracle):
    def __init__(self, nk, fs_out, taps, mode, bfo=BFO, squelch=0.0, agc=True, dtype=np.float32):
        self.bfo = float(bfo)
        super().__init__(nk, fs_out, taps, mode, squelch, agc, dtype)

    def set_mode(self, mode, taps=None, bfo=None):
        if bfo is not None:
            self.bfo = float(bfo)
        super().set_mode(mode, taps)

    def process(self, rows):
        """as BankOracle.process, plus scale [nk] (float64; 0 for a call without outputs)"""
        rd = self.rd
        rows = np.asarray(rows)
        n = rows.shape[1]
        a_all, am_all = np.zeros((self.nk, n), rd), np.zeros((self.nk, n), rd)
        gain, scale = np.ones(self.nk, rd), np.zeros(self.nk, np.float64)
        for ch in range(self.nk):
            dm = self.demod[ch]
            before = dm.yhist[len(dm.yhist) - (dm.ntaps - 1):]
            a = dm.process(rows[ch], self.mode, self.bfo).real.astype(rd)
            if n == 0:
                continue
            scale[ch] = float(np.max(np.abs(np.concatenate((before, rows[ch])).astype(np.complex128))))
            peak = np.max(np.abs(a))
            g = self.agc[ch].update(peak, self.agc_on and self.mode in so.AGC_MODES)
            if self.mode == 'NFM' and self.squelch > 0:
                noise = rd(np.sum(dm.last_hp.astype(np.float64)) / len(a))
                self.level[ch] = rd(self.level[ch] + rd(so.SQUELCH_ALPHA) * rd(noise - self.level[ch]))
                self.open[ch] = bool(self.level[ch] <= rd(self.squelch))
                if not self.open[ch]:
                    g = rd(0)
            a_all[ch], am_all[ch], gain[ch] = a, (a * g).astype(a.dtype), g
        return dict(a=a_all, am=am_all, gain=gain, scale=scale, agc=np.array([x.agc for x in self.agc], rd),
                    agc_gain=np.array([x.gain for x in self.agc], rd), maxbuf=np.array([x.maxbuf for x in self.agc], rd),
                    level=self.level.copy(), open=self.open.copy())
