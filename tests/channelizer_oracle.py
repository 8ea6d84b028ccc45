"""NumPy models of the polyphase channelizer.  Test infrastructure only.

    y_k[m] = sum_{i<L} h[i] x[mD - i] exp(-j 2 pi ((k (mD - i)) mod M) / M),   x[n] = 0 for n < 0

* ``Definition``: the sum as written, float64, streaming (any cut into calls, taps swappable between calls).
* ``polyphase``: float64 branch sums + ``np.fft.ifft``, for the large shapes.
* ``mirror32``: the kernel's float32 arithmetic (fma FIR with p ascending, in-place decimation-in-frequency passes of
  radix 5 / 4 / 2 with float32 twiddles from a float64 table, digit-reversed read-out).
* ``signal`` / ``noise`` / ``odd_taps``: the inputs the GPU tests and the CPU conditioning test share.
"""
import numpy as np
from scipy.signal import firwin


def frame_range(s0, s1, D):
    """frames m with s0 <= m D < s1 (out_index_range with UP = 1)"""
    return -(-s0 // D), -(-s1 // D)


def _phase(k, n, M):
    """exp(-j 2 pi ((k n) mod M) / M), exact integer phase"""
    return np.exp(-2j * np.pi * ((np.asarray(k, np.int64) * np.asarray(n, np.int64)) % M) / M)


class Definition:
    """The definition in float64, as a stream: ``process(x)`` returns [len(ks), n_out] for the frames the call completes,
    with the taps that are current at that call applied to the whole window of its outputs."""

    def __init__(self, h, M, D, ks=None):
        self.M, self.D = int(M), int(D)
        self.ks = np.arange(self.M) if ks is None else np.asarray(ks, np.int64)
        self.h = np.asarray(h, np.float64)
        self.x = np.zeros(0, np.complex128)

    def set_taps(self, h):
        self.h = np.asarray(h, np.float64)

    def reset(self):
        self.x = np.zeros(0, np.complex128)

    def process(self, x):
        s0 = len(self.x)
        self.x = np.concatenate((self.x, np.asarray(x, np.complex128)))
        m0, m1 = frame_range(s0, len(self.x), self.D)
        out = np.zeros((len(self.ks), m1 - m0), np.complex128)
        if m1 == m0:
            return out
        n = np.arange(len(self.x))
        idx = np.arange(m0, m1) * self.D
        for a, k in enumerate(self.ks):
            out[a] = np.convolve(self.x * _phase(k, n, self.M), self.h)[idx]
        return out


def branch_sums(x, h, M, D, m0, m1, dtype=np.float64, fma32=False):
    """v_m[r] = sum_p h[pM + r] x[mD - pM - r] for m in [m0, m1), p ascending -> (re, im) [m1 - m0, M]; x is the whole
    stream from sample 0.  fma32: float32 with one rounding per tap and component, as the kernel's fma."""
    P = -(-len(h) // M)
    hp = np.zeros(P * M, np.float64)
    hp[:len(h)] = h
    hp = hp.astype(dtype)
    xp = np.concatenate((np.zeros(P * M, np.complex128), np.asarray(x, np.complex128)))
    m = np.arange(m0, m1)[:, None]
    r = np.arange(M)[None, :]
    re = np.zeros((m1 - m0, M), dtype)
    im = np.zeros((m1 - m0, M), dtype)
    for p in range(P):
        xs = xp[m * D - p * M - r + P * M]
        t = hp[p * M:(p + 1) * M][None, :]
        if fma32:
            # the product of two float32 is exact in float64; the sum rounds to 53 bits, then to 24
            re = (t.astype(np.float64) * xs.real.astype(np.float32).astype(np.float64) + re.astype(np.float64)).astype(np.float32)
            im = (t.astype(np.float64) * xs.imag.astype(np.float32).astype(np.float64) + im.astype(np.float64)).astype(np.float32)
        else:
            re = re + t * xs.real.astype(dtype)
            im = im + t * xs.imag.astype(dtype)
    return re, im


def polyphase(x, h, M, D, m0, m1, ks=None):
    """float64 polyphase form: [len(ks), m1 - m0]"""
    ks = np.arange(M) if ks is None else np.asarray(ks, np.int64)
    re, im = branch_sums(x, h, M, D, m0, m1)
    Y = np.fft.ifft(re + 1j * im, axis=1) * M                      # sum_r v[r] e^{+j 2 pi k r / M}
    m = np.arange(m0, m1)[:, None]
    return (Y[:, ks] * _phase(ks[None, :], m * D, M)).T


def radices(M):
    """the kernel's pass order: fives, fours, then a two"""
    out = []
    while M % 5 == 0:
        out.append(5)
        M //= 5
    twos = 0
    while M % 2 == 0:
        twos += 1
        M //= 2
    assert M == 1
    return out + [4] * (twos // 2) + [2] * (twos % 2)


def _cmul32(ar, ai, wr, wi):
    return ar * wr - ai * wi, ar * wi + ai * wr


def _bfly32(R, vr, vi):
    f = np.float32
    if R == 2:
        return [vr[0] + vr[1], vr[0] - vr[1]], [vi[0] + vi[1], vi[0] - vi[1]]
    if R == 4:
        s02r, s02i, d02r, d02i = vr[0] + vr[2], vi[0] + vi[2], vr[0] - vr[2], vi[0] - vi[2]
        s13r, s13i, d13r, d13i = vr[1] + vr[3], vi[1] + vi[3], vr[1] - vr[3], vi[1] - vi[3]
        return ([s02r + s13r, d02r - d13i, s02r - s13r, d02r + d13i],
                [s02i + s13i, d02i + d13r, s02i - s13i, d02i - d13r])
    c1, c2 = f(np.cos(2 * np.pi / 5)), f(np.cos(4 * np.pi / 5))
    s1, s2 = f(np.sin(2 * np.pi / 5)), f(np.sin(4 * np.pi / 5))
    outr, outi = [None] * 5, [None] * 5
    t = {}
    for nm, v in (("r", vr), ("i", vi)):
        t1, t2, t3, t4 = v[1] + v[4], v[2] + v[3], v[1] - v[4], v[2] - v[3]
        t[nm] = ((v[0] + t1) + t2, (v[0] + c1 * t1) + c2 * t2, (v[0] + c2 * t1) + c1 * t2,
                 s1 * t3 + s2 * t4, s2 * t3 - s1 * t4)
    (y0r, m1r, m2r, n1r, n2r), (y0i, m1i, m2i, n1i, n2i) = t["r"], t["i"]
    outr[0], outi[0] = y0r, y0i
    outr[1], outi[1] = m1r - n1i, m1i + n1r
    outr[4], outi[4] = m1r + n1i, m1i - n1r
    outr[2], outi[2] = m2r - n2i, m2i + n2r
    outr[3], outi[3] = m2r + n2i, m2i - n2r
    return outr, outi


def mirror32(x, h, M, D, m0, m1, ks=None, rad=None):
    """The kernel's arithmetic in float32 -> complex64 [len(ks), m1 - m0].  x: the whole stream (complex64 values)."""
    ks = np.arange(M) if ks is None else np.asarray(ks, np.int64)
    rad = radices(M) if rad is None else list(rad)
    F = m1 - m0
    re, im = branch_sums(x, h, M, D, m0, m1, dtype=np.float32, fma32=True)
    # rotate: v[r] sits at (r - mD) mod M
    m = np.arange(m0, m1)[:, None]
    q = (np.arange(M)[None, :] - m * D) % M
    ar = np.empty_like(re)
    ai = np.empty_like(im)
    np.put_along_axis(ar, q, re, axis=1)
    np.put_along_axis(ai, q, im, axis=1)
    j = np.arange(M)
    twr = np.cos(2 * np.pi * j / M).astype(np.float32)
    twi = np.sin(2 * np.pi * j / M).astype(np.float32)
    nb = M
    for R in rad:
        nq = nb // R
        br = ar.reshape(F, M // nb, R, nq)
        bi = ai.reshape(F, M // nb, R, nq)
        yr, yi = _bfly32(R, [br[:, :, i, :] for i in range(R)], [bi[:, :, i, :] for i in range(R)])
        nr, ni = np.empty_like(br), np.empty_like(bi)
        n2 = np.arange(nq)
        for i in range(R):
            if i > 0 and nq > 1:
                t = n2 * i * (M // nb)
                yr[i], yi[i] = _cmul32(yr[i], yi[i], twr[t][None, None, :], twi[t][None, None, :])
            nr[:, :, i, :], ni[:, :, i, :] = yr[i], yi[i]
        ar, ai = nr.reshape(F, M), ni.reshape(F, M)
        nb = nq
    pos = np.zeros(len(ks), np.int64)
    k, nb = ks.copy(), M
    for R in rad:
        nb //= R
        pos += (k % R) * nb
        k //= R
    return (ar[:, pos] + 1j * ai[:, pos]).astype(np.complex64).T


# ---- the inputs the GPU tests and the conditioning test share ------------------------------------------------------
SHAPES = [(16, 16), (64, 16), (64, 32), (64, 64), (250, 125), (256, 128), (640, 320), (800, 400), (1024, 256), (4096, 2048),
          (625, 625), (2048, 512)]       # the last two: an odd M (LDS pitch M itself, radix 5 alone) and 8 frames per workgroup


def signal_length(M):
    return 24 * M + 5003          # odd; several workgroups at every shape, the first 8 M of it the filter's run-in


def signal(M, seed=0):
    """Tones at about 0.5 full scale in all -- one on a channel centre, one 0.3 of a spacing above another, one at a
    negative frequency 0.45 of a spacing off -- plus complex noise at 0.01."""
    rng = np.random.default_rng(1000 * M + seed)
    n = np.arange(signal_length(M))
    k1, k2, k3 = rng.integers(1, M // 2 - 1, 3)
    ph = rng.uniform(0, 2 * np.pi, 3)
    x = 0.25 * np.exp(1j * (2 * np.pi * k1 / M * n + ph[0]))
    x = x + 0.15 * np.exp(1j * (2 * np.pi * (k2 + 0.3) / M * n + ph[1]))
    x = x + 0.10 * np.exp(1j * (-2 * np.pi * (k3 + 0.45) / M * n + ph[2]))
    x = x + 0.01 * (rng.standard_normal(len(n)) + 1j * rng.standard_normal(len(n)))
    return x.astype(np.complex64)


def noise(M, seed=0):
    rng = np.random.default_rng(7000 * M + seed)
    n = signal_length(M)
    return (0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def odd_taps(M):
    """an odd-length prototype that is not a multiple of M taps long"""
    L = 5 * M + 3 if M % 2 == 0 else 5 * M + 2
    return firwin(L, 0.5 / M, window=('kaiser', 8.0), fs=1.0)


def random_cuts(n, D, seed):
    """cut lengths summing to n that include 0, 1, lengths shorter than D (where D > 2) and odd lengths"""
    rng = np.random.default_rng(seed)
    cuts = [0, 1, max(1, D - 1), 0, 3]
    while sum(cuts) < n:
        cuts.append(int(rng.integers(0, max(4 * D, 64))) | int(rng.integers(0, 2)))
    cuts[-1] -= sum(cuts) - n
    assert cuts[-1] >= 0 and sum(cuts) == n
    return cuts
