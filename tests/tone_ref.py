"""The tone stage's contract (pocket_tts_amd/tone.py) restated in float64, for the tests: the audio-EQ-cookbook coefficients
from the issue's table with this file's own code, and a serial DIRECT FORM I filter, vectorised over rows - another
arrangement of the same transfer function than the transposed direct form II the stage runs, so the two share no rounding.
`Stream` is the stage fed frame by frame; `reference` runs a whole signal at once.  Both do the same operations in the same
order, so they agree exactly.  Plain numpy; nothing here imports the package."""

from __future__ import annotations

import math

import numpy as np

PRESETS = {
    "telephone": [("hp", 300.0, None, 0.5411961), ("hp", 300.0, None, 1.3065630), ("lp", 3400.0, None, 0.5411961),
                  ("lp", 3400.0, None, 1.3065630)],
    "warm": [("lowshelf", 200.0, 3.0, None), ("highshelf", 6000.0, -3.0, None)],
    "bright": [("highshelf", 5000.0, 4.0, None)],
    "presence": [("hp", 80.0, None, None), ("peak", 3000.0, 4.0, 1.0)],
    "small_speaker": [("hp", 180.0, None, None), ("peak", 2500.0, 3.0, 0.8)],
    "deess": [("peak", 6500.0, -6.0, 2.0)],
}


def parse(spec):
    """[(kind, f0, gain_db or None, q)] of a preset or a band list of valid syntax; q defaulted"""
    if spec in PRESETS:
        bands = PRESETS[spec]
    else:
        bands = []
        for band in spec.split(";"):
            kind, *nums = band.split(":")
            nums = [float(v) for v in nums]
            if kind in ("hp", "lp"):
                bands.append((kind, nums[0], None, nums[1] if len(nums) > 1 else None))
            else:
                bands.append((kind, nums[0], nums[1], nums[2] if len(nums) > 2 else None))
    return [(k, f, g, q if q is not None else (1.0 if k == "peak" else math.sqrt(0.5))) for k, f, g, q in bands]


def biquad(kind, f0, gain_db, q, rate):
    """(b [3], a [3]) with a[0] = 1, float64"""
    w = 2.0 * math.pi * f0 / rate
    c, s = math.cos(w), math.sin(w)
    al = s / (2.0 * q)
    if kind == "hp":
        b, a = [(1 + c) / 2, -(1 + c), (1 + c) / 2], [1 + al, -2 * c, 1 - al]
    elif kind == "lp":
        b, a = [(1 - c) / 2, 1 - c, (1 - c) / 2], [1 + al, -2 * c, 1 - al]
    else:
        A = 10.0 ** (gain_db / 40.0)
        r = 2.0 * math.sqrt(A) * al
        if kind == "peak":
            b, a = [1 + al * A, -2 * c, 1 - al * A], [1 + al / A, -2 * c, 1 - al / A]
        elif kind == "lowshelf":
            b = [A * ((A + 1) - (A - 1) * c + r), 2 * A * ((A - 1) - (A + 1) * c), A * ((A + 1) - (A - 1) * c - r)]
            a = [(A + 1) + (A - 1) * c + r, -2 * ((A - 1) + (A + 1) * c), (A + 1) + (A - 1) * c - r]
        elif kind == "highshelf":
            b = [A * ((A + 1) + (A - 1) * c + r), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - r)]
            a = [(A + 1) - (A - 1) * c + r, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - r]
        else:
            raise ValueError(kind)
    return np.array(b, dtype=np.float64) / a[0], np.array(a, dtype=np.float64) / a[0]


def coefficients(spec, rate):
    """[K, 5] float64: b0 b1 b2 a1 a2 of every section"""
    out = []
    for band in parse(spec):
        b, a = biquad(*band, rate)
        out.append([b[0], b[1], b[2], a[1], a[2]])
    return np.array(out, dtype=np.float64).reshape(-1, 5)


class Stream:
    """`rows` streams through the same cascade, frame by frame: direct form I, float64, zero initial state.  `frame(x)` takes
    [rows, n] (any float type) and returns the float64 output before the one rounding to fp32"""

    def __init__(self, coef, rows=1):
        self.coef = np.asarray(coef, dtype=np.float64).reshape(-1, 5)
        self.h = np.zeros((len(self.coef), 4, rows))  # per section: x[i-1], x[i-2], y[i-1], y[i-2]

    def frame(self, x):
        y = np.array(x, dtype=np.float64)
        if y.ndim == 1:
            y = y[None, :]
        for k, (b0, b1, b2, a1, a2) in enumerate(self.coef):
            x1, x2, y1, y2 = self.h[k]
            for i in range(y.shape[1]):
                xi = y[:, i].copy()
                yi = b0 * xi + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
                x2, x1, y2, y1 = x1, xi, y1, yi
                y[:, i] = yi
            self.h[k] = x1, x2, y1, y2
        return y


def reference(spec, rate, x):
    """the whole signal x [rows, N] or [N] through the tone `spec` at `rate` Hz: float64, not yet rounded"""
    x = np.asarray(x)
    y = Stream(coefficients(spec, rate), 1 if x.ndim == 1 else x.shape[0]).frame(x)
    return y[0] if x.ndim == 1 else y
