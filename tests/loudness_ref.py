"""The loudness normaliser's contract (pocket_tts_amd/loudness.py) restated in float64, for the tests: K-weighting in direct
form I, sub-block energies, the gated loudness and the gain per sub-block, the delayed and ramped output.  `Stream` is the
stage fed frame by frame; `reference` runs a whole signal through one `Stream` call.  Both do the same operations in the
same order, so they agree exactly.  Plain numpy and Python floats; nothing here imports the package's rule module except
for the coefficients, which `coefficients` recomputes on its own."""

from __future__ import annotations

import math

import numpy as np

MAX_BLOCKS = 1024


def coefficients(rate):
    """((b, a) of the shelf, (b, a) of the high-pass) at `rate` Hz, float64, a[0] = 1"""
    K = math.tan(math.pi * 1681.974450955533 / rate)
    Q = 0.7071752369554196
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = ([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0],
             [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    K = math.tan(math.pi * 38.13547087602444 / rate)
    Q = 0.5003270373238773
    a0 = 1.0 + K / Q + K * K
    hp = ([1.0, -2.0, 1.0], [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return shelf, hp


def lufs(Z):
    return -0.691 + 10.0 * math.log10(Z) if Z > 0.0 else -math.inf


def gated(Zs):
    """L over the gating-block energies `Zs` (absolute gate -70, relative gate -10), None when no block passes the absolute
    gate"""
    A = [Z for Z in Zs if lufs(Z) > -70.0]
    if not A:
        return None
    gamma = lufs(math.fsum(A) / len(A)) - 10.0
    R = [Z for Z in A if lufs(Z) > gamma]
    return lufs(math.fsum(R) / len(R))


class _Biquad:
    """direct form I, float64, zero initial state"""

    def __init__(self, b, a):
        self.b, self.a = [float(v) for v in b], [float(v) for v in a]
        self.x1 = self.x2 = self.y1 = self.y2 = 0.0

    def run(self, x):
        b0, b1, b2 = self.b
        _, a1, a2 = self.a
        x1, x2, y1, y2 = self.x1, self.x2, self.y1, self.y2
        out = [0.0] * len(x)
        for i, v in enumerate(x):
            y = b0 * v + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
            x2, x1, y2, y1 = x1, v, y1, y
            out[i] = y
        self.x1, self.x2, self.y1, self.y2 = x1, x2, y1, y2
        return out


class Stream:
    """One row of the stage at `rate` Hz with target `T`.  `frame(x)` takes the next samples of the row's input (any
    number; float32 values) and returns as many output samples in float64.  `c[m]`, `L[m]` (None while undefined), `Z[m]`
    (None for m < 3) are the gain, the loudness and the gating-block energy after sub-block m; `l[q]` the loudness of
    gating block q >= 3."""

    def __init__(self, rate, T):
        self.rate, self.T = int(rate), float(T)
        self.S = self.rate // 10
        self.D = 4 * self.S
        shelf, hp = coefficients(self.rate)
        self.f1, self.f2 = _Biquad(*shelf), _Biquad(*hp)
        self.open = []          # w^2 of the open sub-block
        self.z = []             # sub-block energies
        self.hist = []          # gating-block energies, at most MAX_BLOCKS
        self.c, self.L, self.Z, self.l = [], [], [], {}
        self.x = []             # every input sample so far
        self.pos = 0            # output samples so far

    def _complete(self, sq):
        m = len(self.z)
        self.z.append(math.fsum(sq) / self.S)
        prev = self.c[-1] if self.c else np.float32(1.0)
        if m < 3 or m - 3 >= MAX_BLOCKS:
            self.c.append(np.float32(1.0) if m < 3 else prev)
            self.L.append(self.L[-1] if self.L else None)
            self.Z.append(self.Z[-1] if self.Z else None)
            return
        Z = (((self.z[m - 3] + self.z[m - 2]) + self.z[m - 1]) + self.z[m]) / 4.0
        self.hist.append(Z)
        self.l[m] = lufs(Z)
        L = gated(self.hist)
        self.Z.append(Z)
        if L is None:
            self.c.append(prev)
            self.L.append(None)
        else:
            self.c.append(np.float32(min(max(10.0 ** ((self.T - L) / 20.0), 0.1), 10.0)))
            self.L.append(L)

    def knot(self, j):
        return float(self.c[max(j + 2, 3)])

    def frame(self, x):
        x = [float(v) for v in np.asarray(x, dtype=np.float32)]
        w = self.f2.run(self.f1.run(x))
        for v in w:
            self.open.append(v * v)
            if len(self.open) == self.S:
                self._complete(self.open)
                self.open = []
        self.x.extend(x)
        S, D = self.S, self.D
        y = np.zeros(len(x), dtype=np.float64)
        i = np.arange(self.pos, self.pos + len(x))
        on = i >= D
        if on.any():
            q = i[on] - D
            j = q // S
            knots = np.array([self.knot(v) for v in range(int(j[0]), int(j[-1]) + 2)], dtype=np.float64)
            k0, k1 = knots[j - j[0]], knots[j - j[0] + 1]
            xs = np.array(self.x[int(q[0]):int(q[-1]) + 1], dtype=np.float64)
            y[on] = (k0 + (k1 - k0) * (q % S) / S) * xs
        self.pos += len(x)
        return y

    def bound(self, lo, hi):
        """the fp32 error bound 16 * 2^-24 * max(k_j, k_{j+1}) * |x[i - D]| of output samples [lo, hi)"""
        S, D = self.S, self.D
        b = np.zeros(hi - lo, dtype=np.float64)
        for t, i in enumerate(range(lo, hi)):
            if i >= D:
                j = (i - D) // S
                b[t] = 16.0 * 2.0 ** -24 * max(self.knot(j), self.knot(j + 1)) * abs(self.x[i - D])
        return b


def reference(x, rate, T):
    """(y float64, the `Stream` after the whole signal `x`)"""
    s = Stream(rate, T)
    return s.frame(x), s


def integrated(x, rate):
    """the gated loudness of the whole signal `x` by BS.1770-4 (400 ms blocks every 100 ms), None for silence"""
    s = Stream(rate, -23.0)
    s.frame(np.asarray(x, dtype=np.float32))
    return gated(s.hist)
