"""NumPy models of the fine channelizer, built on ``tests/channelizer_oracle.py``.  Test
infrastructure only.

* ``split`` / ``used_rows``: fine channel G -> (coarse row k1, offset q, second-stage channel k2); the coarse rows a range uses.
* ``cascade64``: both stages in float64 (stage 2 on the unrounded float64 rows of stage 1) for the frames [m0, m1).
* ``model32``: the kernels' float32 arithmetic.  Stage 2 (fine.hip) sums in the order of chan.hip -- fma FIR with p
  ascending, in-place DIF passes of radix 5 / 4 / 2, digit-reversed read-out -- so both stages are
  ``channelizer_oracle.mirror32``, the second one fed the complex64 rows of the first.
* ``Cascade``: the float64 cascade as a stream (any cut into calls, taps swappable between calls).
* ``signal``: the input the GPU tests and the CPU tests share.
"""
import numpy as np

from tests import channelizer_oracle as co


def geometry(M1, D1, M2, D2):
    C1 = M1 // D1
    Q = M2 // C1
    return dict(C1=C1, C2=M2 // D2, Q=Q, Mf=M1 * Q, D=D1 * D2)


def split(G, M1, D1, M2):
    """fine channel(s) G in [0, Mf) -> (k1, q, k2)"""
    Q = M2 // (M1 // D1)
    G = np.asarray(G, np.int64)
    c = (G + Q // 2) // Q                       # floor
    q = G - c * Q
    return c % M1, q, q % M2


def used_rows(M1, D1, M2, g_first, ng):
    """the circular range of coarse rows that fine channels g_first .. g_first + ng - 1 run through, first occurrence order"""
    Q = M2 // (M1 // D1)
    c0, c1 = (g_first + Q // 2) // Q, (g_first + ng - 1 + Q // 2) // Q
    return (c0 + np.arange(min(c1 - c0 + 1, M1))) % M1


def run_in_taps(h1, h2, D1):
    return len(h1) + D1 * (len(h2) - 1)


def _rows_of(G, M1, D1, M2, g_first, ng):
    k1s = used_rows(M1, D1, M2, g_first, ng)
    k1, q, k2 = split(G, M1, D1, M2)
    j = np.array([int(np.flatnonzero(k1s == k)[0]) for k in k1])
    return k1s, j, k2


def cascade64(x, h1, h2, M1, D1, M2, D2, g_first, ng, m0, m1):
    """-> (y complex128 [ng, m1 - m0], y1 complex128 [nk1, n1]): the fine frames [m0, m1) and the used stage-1 rows from
    frame 0 to the last one frame m1 - 1 reads.  x: the whole stream from sample 0."""
    g = geometry(M1, D1, M2, D2)
    G = (g_first + np.arange(ng)) % g["Mf"]
    k1s, j, k2 = _rows_of(G, M1, D1, M2, g_first, ng)
    n1 = max((m1 - 1) * D2 + 1, 0)
    y1 = co.polyphase(x, h1, M1, D1, 0, n1, ks=k1s)
    y = np.zeros((ng, m1 - m0), np.complex128)
    for jj in range(len(k1s)):
        a = np.flatnonzero(j == jj)
        if len(a):
            y[a] = co.polyphase(y1[jj], h2, M2, D2, m0, m1, ks=k2[a])
    return y, y1


def model32(x, h1, h2, M1, D1, M2, D2, g_first, ng, m0, m1):
    """the kernels' arithmetic in float32 -> complex64 [ng, m1 - m0]"""
    g = geometry(M1, D1, M2, D2)
    G = (g_first + np.arange(ng)) % g["Mf"]
    k1s, j, k2 = _rows_of(G, M1, D1, M2, g_first, ng)
    n1 = max((m1 - 1) * D2 + 1, 0)
    y1 = co.mirror32(x, h1, M1, D1, 0, n1, ks=k1s)
    y = np.zeros((ng, m1 - m0), np.complex64)
    for jj in range(len(k1s)):
        a = np.flatnonzero(j == jj)
        if len(a):
            y[a] = co.mirror32(y1[jj], h2, M2, D2, m0, m1, ks=k2[a])
    return y


def scale_of(y, y1, h2, D2, m0, m1):
    """The scale of a call's parity bar: the larger of the call's fine peak and the peak of the used float64 stage-1 rows
    over the call's stage-2 windows (a coarse row can hold a strong signal that no kept fine channel passes)."""
    lo = max(m0 * D2 - (len(h2) - 1), 0)
    hi = (m1 - 1) * D2 + 1
    return max(float(np.abs(y).max()), float(np.abs(y1[:, lo:hi]).max()))


class Cascade:
    """The float64 cascade as a stream: ``process(x)`` returns [ng, n_out] for the fine frames the call completes, each
    stage applying the taps current at that call to the whole window of the call's outputs."""

    def __init__(self, h1, h2, M1, D1, M2, D2, g_first, ng):
        self.shape = (M1, D1, M2, D2)
        self.g_first, self.ng = g_first, ng
        self.h1, self.h2 = np.asarray(h1, np.float64), np.asarray(h2, np.float64)
        self.x = np.zeros(0, np.complex128)
        self.y1 = None                                      # stage-1 rows as the calls produced them

    def set_taps(self, h1, h2):
        self.h1, self.h2 = np.asarray(h1, np.float64), np.asarray(h2, np.float64)

    def process(self, x):
        M1, D1, M2, D2 = self.shape
        g = geometry(M1, D1, M2, D2)
        s0 = len(self.x)
        self.x = np.concatenate((self.x, np.asarray(x, np.complex128)))
        G = (self.g_first + np.arange(self.ng)) % g["Mf"]
        k1s, j, k2 = _rows_of(G, M1, D1, M2, self.g_first, self.ng)
        a0, a1 = co.frame_range(s0, len(self.x), D1)
        new = co.polyphase(self.x, self.h1, M1, D1, a0, a1, ks=k1s)
        self.y1 = new if self.y1 is None else np.concatenate((self.y1, new), axis=1)
        m0, m1 = co.frame_range(s0, len(self.x), g["D"])
        y = np.zeros((self.ng, m1 - m0), np.complex128)
        for jj in range(len(k1s)):
            a = np.flatnonzero(j == jj)
            if len(a) and m1 > m0:
                y[a] = co.polyphase(self.y1[jj], self.h2, M2, D2, m0, m1, ks=k2[a])
        return y


# ---- the shared input ---------------------------------------------------------------------------------------------------
def signal_length(h1, h2, D1, D2):
    return run_in_taps(h1, h2, D1) + 40 * D1 * D2 + 1003        # odd remainder


def tone_rows(M1, D1, M2, ng, g_first):
    """Output rows of the four in-range tones: centre, 0.3 off, 0.45 off, and the row on a coarse seam (q = -Q/2; None
    where the range holds no seam)."""
    Q = M2 // (M1 // D1)
    Mf = M1 * Q
    seam = [a for a in range(ng) if ((g_first + a) % Mf) % Q == Q // 2]
    return ng // 2, ng // 3, (2 * ng) // 3 if ng > 2 else 0, (seam[len(seam) // 2] if seam else None)


def signal(M1, D1, M2, D2, g_first, ng, h1, h2, seed=0):
    """Tones on a fine centre (0.2), 0.3 (0.1) and 0.45 (0.1) of df off a centre, one on the seam between two coarse rows
    (0.1; the nearest seam below the range where the range holds none), one outside the selected range at 0.25 (three rows
    past its end; inside where the range is the whole raster), complex noise at 0.01."""
    g = geometry(M1, D1, M2, D2)
    Mf, Q = g["Mf"], g["Q"]
    rng = np.random.default_rng(100003 * M1 + 1009 * M2 + 17 * D2 + seed)
    n = np.arange(signal_length(h1, h2, D1, D2))
    a_c, a_3, a_45, a_seam = tone_rows(M1, D1, M2, ng, g_first)
    G_seam = (g_first + a_seam) if a_seam is not None else ((g_first + Q // 2) // Q * Q - Q // 2)
    tones = [(0.2, g_first + a_c), (0.1, g_first + a_3 + 0.3), (0.1, g_first + a_45 - 0.45), (0.1, G_seam), (0.25, g_first + ng + 2)]
    ph = rng.uniform(0, 2 * np.pi, len(tones))
    x = np.zeros(len(n), np.complex128)
    for (amp, G), p in zip(tones, ph):
        x += amp * np.exp(1j * (2 * np.pi * ((G % Mf) / Mf) * n + p))
    x += 0.01 * (rng.standard_normal(len(n)) + 1j * rng.standard_normal(len(n)))
    return x.astype(np.complex64)
