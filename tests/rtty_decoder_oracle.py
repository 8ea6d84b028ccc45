"""CPU restatement of the reference's RTTY decoder bank and signal finder, vectorised over bins, and a Baudot FSK
synthesiser.  TEST INFRASTRUCTURE ONLY: the product is pysdr_amd/rtty.py + csrc/rtty.hip.

Restated from rtty.py (decoder :431-701, finder :744-764, executive :847-853), for every mark bin b of a range at once:
  :485-490  mark = line[b], space = line[b + NBINS] (kept as float32 in mark_buf / space_buf)
  :496      signal = FIFO(32).push(mark - space): d_n = f32(mark - space)
  :497-500  score = H @ signal (float32), isym = first argmax, sc_buf.push(score[isym])
  :519      sc2 = np.sum(sc_buf.x[-1::-M]) = best_n + best_{n-30} + ... + best_{n-120}
  :531-565  n % M == 0: i = argmax(sc3.x) over lines n-29..n, t = n + i - M; if t - tlast >= 25:
            snr2 = compute_snr(sym, tlast - n), ch = decode_symbol(sym, snr2); then tlast = t, sym = isyms.x[t - n]
  :612-653  H: 4 x stop (+1), 4 x start (-1), the 5 bits LSB first x4, 4 x stop (+1);  B: [1, 0, b0..b4, 1]
  :657-665  compute_snr: mean over the 8 bits of (signal - noise), marks/spaces at lines tlast - 28 + 4k (float64)
  :668-700  decode_symbol: snr2 >= THRESH = 8; 31 -> LTRS, 27 -> FIGS, 0 -> nothing, else figs/ltrs[sym]
  :744-764  find_sigs: det = FIFO2(21) of float32 lines; bins [YLIM[0], YLIM[1] - NBINS) with
            sum(|mark - space|) over the 21 lines > 20 * 21 are counted (ndet)
All FIFOs start zeroed: everything before line 1 is 0.  Besides what the reference computes, the bank records the
margins that decide each decision (see `decision margins` below) so that a float32 result computed in another order
can be compared with it."""
from __future__ import annotations

import numpy as np

M = 30                     # lines per character
NBINS = 7                  # 170 Hz at 48 kHz / 2048
THRESH = 8
LTRS = ['\0', 'E', '\n', 'A', ' ', 'S', 'I', 'U', '\r', 'D', 'R', 'J',
        'N', 'F', 'C', 'K', 'T', 'Z', 'L', 'W', 'H', 'Y', 'P', 'Q', 'O', 'B', 'G',
        '<FIGS>', 'M', 'X', 'V', '<LTRS>']
FIGS = ['\0', '3', '\n', '-', ' ', '\\g', '8', '7', '\r', '$', '4', "'",
        ',', '!', ':', '(', '5', '"', ')', '2', '#', '6', '0', '1', '9', '?', '&',
        '<FIGS>', '.', '/', ';', '<LTRS>']


def templates():
    """H [32][32] (+-1, float32) and B [32][8] (rtty.py:612-653)."""
    H = np.empty((32, 32), np.float32)
    B = np.empty((32, 8), np.int64)
    for s in range(32):
        bits = [(s >> b) & 1 for b in range(5)]
        B[s] = [1, 0] + bits + [1]
        h = [1] * 4 + [0] * 4 + [v for v in bits for _ in range(4)] + [1] * 4
        H[s] = 2 * np.asarray(h, np.float32) - 1
    return H, B


def code_text(code):
    return (FIGS if code >= 32 else LTRS)[code & 31]


class DecoderBank:
    """Decoders on the mark bins [bin_lo, bin_hi), the finder on [find_lo, find_hi); ``decode(lines)`` takes lines
    [L][nfft] in the reference's (flipped) order and may be called with any cut of a stream.

    Decision margins, per decision and bin (np.inf where a margin does not apply):
      m_isym  best - second-best score at the held symbol's line tlast + 1 (the symbol the decision gates)
      m_sc2   best - second-best sc2 in the decision's timing window
      m_snr   |snr2 - 8| when a symbol is gated (t - tlast >= 25)
    A decoder whose margins all clear the tolerances up to decision j decides 0..j as any correct float32
    evaluation does (`horizon`)."""

    def __init__(self, bin_lo, bin_hi, find_lo=800, find_hi=1243, nbins=NBINS):
        self.bin_lo, self.bin_hi, self.find_lo, self.find_hi, self.nsh = bin_lo, bin_hi, find_lo, find_hi, nbins
        self.nb = bin_hi - bin_lo
        self.H, self.B = templates()
        self.n = 0
        nb = self.nb
        z = lambda dt, w=nb: np.zeros((0, w), dt)
        self.mark, self.space, self.d = z(np.float32), z(np.float32), z(np.float32)
        self.best, self.isym, self.gap, self.sc2 = z(np.float32), z(np.int64), z(np.float32), z(np.float32)
        self.det = z(np.float32, max(find_hi - find_lo, 0) + nbins)
        self.tlast = np.zeros(nb, np.int64)
        self.sym = np.zeros(nb, np.int64)
        self.shift = np.zeros(nb, bool)

    @staticmethod
    def _at(a, idx):
        """rows idx (1-based line numbers) of a history array, 0 before line 1"""
        idx = np.asarray(idx)
        out = np.zeros(idx.shape + a.shape[1:], a.dtype)
        ok = idx >= 1
        out[ok] = a[idx[ok] - 1]
        return out

    def decode(self, lines):
        with np.errstate(invalid="ignore"):          # infinite dB values make NaN where the reference makes NaN
            return self._decode(lines)

    def _decode(self, lines):
        lines = np.asarray(lines)
        L = len(lines)
        n0 = self.n + 1
        cols = np.arange(self.bin_lo, self.bin_hi)
        m64, s64 = lines[:, cols].astype(np.float64), lines[:, cols + self.nsh].astype(np.float64)
        self.mark = np.concatenate((self.mark, m64.astype(np.float32)))
        self.space = np.concatenate((self.space, s64.astype(np.float32)))
        self.d = np.concatenate((self.d, (m64 - s64).astype(np.float32)))
        # scores of the new lines, in blocks of lines (the windows are [lines][bins][32])
        dpad = np.concatenate((np.zeros((31, self.nb), np.float32), self.d))   # row r + 31 = line r + 1
        best, isym, gap = [], [], []
        for a in range(0, L, 128):
            rows = np.arange(n0 + a, min(n0 + L, n0 + a + 128))                # line numbers
            win = dpad[(rows - 1)[:, None] + np.arange(32)[None, :]]           # [l][32][nb]: d_{n-31..n}
            sc = np.matmul(self.H[None, :, :], win)                            # [l][32 symbols][nb], float32
            i = np.argmax(sc, axis=1)
            b = np.take_along_axis(sc, i[:, None, :], axis=1)[:, 0, :]
            top2 = np.sort(sc, axis=1)[:, -2, :]
            isym.append(i)
            best.append(b)
            gap.append(b - top2)
        self.best = np.concatenate([self.best] + best)
        self.isym = np.concatenate([self.isym] + isym)
        self.gap = np.concatenate([self.gap] + gap)
        lines_n = np.arange(n0, n0 + L)
        sc2 = self._at(self.best, lines_n)
        for k in range(1, 5):
            sc2 = sc2 + self._at(self.best, lines_n - k * M)
        self.sc2 = np.concatenate((self.sc2, sc2))
        # decisions completed by these lines
        out = dict(n=[], codes=[], t=[], snr2=[], m_isym=[], m_sc2=[], m_snr=[])
        for n in range(M * (self.n // M + 1), self.n + L + 1, M):
            w = self.sc2[n - M:n]                                               # lines n-29..n
            i = np.argmax(w, axis=0)
            srt = np.sort(w, axis=0)
            t = n + i - M
            dt = t - self.tlast
            gate = dt >= 25
            # compute_snr(sym, tlast - n): lines tlast - 28 + 4k, float64
            path = self.tlast[None, :] - 28 + 4 * np.arange(8)[:, None]         # [8][nb]
            mk = np.where(path >= 1, self.mark[np.clip(path - 1, 0, None), np.arange(self.nb)], 0).astype(np.float64)
            sp = np.where(path >= 1, self.space[np.clip(path - 1, 0, None), np.arange(self.nb)], 0).astype(np.float64)
            bits = self.B[self.sym].T                                           # [8][nb]
            signal = bits * mk + (1 - bits) * sp
            noise = (1 - bits) * mk + bits * sp
            v = signal - noise                                                  # np.mean of 8: pairwise, / 8
            snr2 = np.where(gate, (((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))) / 8, np.nan)
            # the held symbol: the initial sym = 0 at the first decision, else isym at line tlast + 1
            held_gap = np.full(self.nb, np.inf) if n == M else self.gap[self.tlast, np.arange(self.nb)]
            codes = np.full(self.nb, -1, np.int64)
            ok = gate & (snr2 >= THRESH)
            self.shift[ok & (self.sym == 31)] = False
            self.shift[ok & (self.sym == 27)] = True
            emit = ok & ~np.isin(self.sym, (0, 27, 31))
            codes[emit] = self.sym[emit] + 32 * self.shift[emit]
            out['n'].append(n)
            out['codes'].append(codes)
            out['t'].append(t)
            out['snr2'].append(snr2)
            out['m_isym'].append(held_gap)
            out['m_sc2'].append(srt[-1] - srt[-2])
            out['m_snr'].append(np.where(gate, np.abs(snr2 - THRESH), np.inf))
            self.tlast = t
            self.sym = self.isym[t, np.arange(self.nb)]                          # isym_{t+1}: row t
        nd = len(out['n'])
        for k in ('codes', 't', 'snr2', 'm_isym', 'm_sc2', 'm_snr'):
            out[k] = np.array(out[k]).reshape(nd, self.nb)
        out['n'] = np.array(out['n'], np.int64)
        # the finder
        if self.find_hi > self.find_lo:
            fcols = np.arange(self.find_lo, self.find_hi + self.nsh)
            self.det = np.concatenate((self.det, lines[:, fcols].astype(np.float32)))
            nf = self.find_hi - self.find_lo
            ndet, fmin = [], []
            for n in lines_n:
                x = self._at(self.det, np.arange(n - 20, n + 1))               # [21][nf + nsh]
                a = np.abs(x[:, :nf] - x[:, self.nsh:]).astype(np.float64)
                r = a[:8] + a[8:16]                                             # np.sum of 21: pairwise, then the tail
                s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
                for q in range(16, 21):
                    s = s + a[q]
                ndet.append(int(np.sum(s > 20 * 21)))
                fmin.append(float(np.min(np.abs(s - 20 * 21))))
            out['ndet'] = np.array(ndet, np.int64)
            out['m_find'] = np.array(fmin)
        else:
            out['ndet'] = np.zeros(L, np.int64)
            out['m_find'] = np.full(L, np.inf)
        out['isym'] = self.isym[n0 - 1:]
        out['best'] = self.best[n0 - 1:]
        out['gap'] = self.gap[n0 - 1:]
        self.n += L
        return out


def horizon(m_isym, m_sc2, m_snr, tol_score=1e-2, tol_snr=1e-6):
    """Per bin: how many leading decisions have every margin at or above tolerance."""
    bad = (m_isym < tol_score) | (m_sc2 < tol_score) | (m_snr < tol_snr)
    nd = bad.shape[0]
    return np.where(bad.any(axis=0), np.argmax(bad, axis=0), nd)


# ---- Baudot FSK synthesiser ----------------------------------------------------------------------------------------

def bin_hz(b, fs=48000, nfft=2048):
    """Baseband frequency of bin b of a (flipped) filterbank line: index NFFT-1-(NFFT/2 + k) holds +k bins."""
    return (nfft // 2 - 1 - b) * fs / nfft


def baudot_codes(text):
    """Text -> 5-bit codes, LTRS first and a LTRS / FIGS code before every change of case (space, CR and LF
    exist in both cases and keep the current one)."""
    out, shift = [31], False
    for ch in text.upper():
        in_l = ch in LTRS and LTRS.index(ch) not in (0, 27, 31)
        in_f = ch in FIGS and FIGS.index(ch) not in (0, 27, 31)
        if in_l and not (shift and in_f):
            if shift:
                out.append(31)
                shift = False
            out.append(LTRS.index(ch))
        elif in_f:
            if not shift:
                out.append(27)
                shift = True
            out.append(FIGS.index(ch))
        else:
            raise ValueError(f"no Baudot code for {ch!r}")
    return out


def baudot_fsk(fs, text, mark_hz, amp=1.0, delay=0.0, nsamp=None, shift_hz=170.0, baud_t=22e-3, phase=0.0):
    """Continuous-phase FSK: idle mark for `delay` s, then each code as start (space), 5 bits LSB first
    (1 = mark), 1.5 stop bits (mark); idle mark after the text.  -> complex128 [nsamp]."""
    codes = baudot_codes(text)
    bits = []
    for c in codes:
        bits += [(0, 1.0)] + [((c >> b) & 1, 1.0) for b in range(5)] + [(1, 1.5)]
    edges = np.cumsum([0.0] + [w * baud_t for _, w in bits]) + delay
    if nsamp is None:
        nsamp = int(np.ceil((edges[-1] + 0.2) * fs))
    tt = np.arange(nsamp) / fs
    k = np.searchsorted(edges, tt, side='right') - 1
    val = np.ones(nsamp)
    inside = (k >= 0) & (k < len(bits))
    val[inside] = np.array([b for b, _ in bits], float)[k[inside]]
    f = np.where(val > 0, mark_hz, mark_hz - shift_hz)
    ph = phase + 2 * np.pi * np.cumsum(f) / fs
    return amp * np.exp(1j * ph)


def synth_band(fs, signals, nsamp, noise, seed):
    """sum of baudot_fsk(fs, text, bin_hz(bin), amp, delay) for (bin, text, amp, delay) + complex white noise"""
    rng = np.random.default_rng(seed)
    x = noise * (rng.standard_normal(nsamp) + 1j * rng.standard_normal(nsamp))
    for b, text, amp, delay in signals:
        x = x + baudot_fsk(fs, text, bin_hz(b, fs), amp, delay, nsamp, phase=rng.uniform(0, 2 * np.pi))
    return x.astype(np.complex64)
