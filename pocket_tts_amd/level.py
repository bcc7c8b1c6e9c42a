"""Per-request output level: gain plus a streaming look-ahead peak limiter, the last stage of the output chain
codec -> resampler -> stretcher -> level (the kernel is csrc/ptts_level.hip; numpy only, nothing here touches the GPU).

A row's input stream `x` is whatever leaves the previous stage for that row, `n` samples per frame; x[i] = 0 for i < 0 and
for every i after the row is set to drain.  Per row there are two fp32 parameters, G = fp32(10^(gain_db / 20)) and
C = fp32(10^(peak_dbfs / 20)).  A plan is (n, LA, a, k), a function of the row's output rate and n only:

  LA = ceil(0.005 rate)                    the look-ahead: 40 / 120 / 240 samples at 8 / 24 / 48 kHz
  a  = fp32(exp(-1 / (0.100 rate)))        a 100 ms release
  k  = fp32(1 / LA)

The stage computes

  u[i] = G x[i]                                   (fp32 product)
  r[i] = |u[i]| > C ? C / |u[i]| : 1              (a NaN sample compares false: r = 1)
  m[i] = min over 0 <= t <= LA of r[i - t]        (r = 1 before the stream's start)
  d[i] = max(1 - m[i], a d[i - 1]),  d[-1] = 0    (the gain reduction; it decays by a per sample)
  e[i] = 1 - d[i]
  g[i] = k sum over 0 <= t < LA of e[i - t]       (e = 1 before the stream's start)
  y[i] = g[i] u[i - LA]                           (the output lags by LA samples)

Every e[j] with i - LA < j <= i has e[j] <= m[j] <= r[i - LA], because i - LA lies in the window of m[j]; so
g[i] <= r[i - LA] and |y[i]| <= C in exact arithmetic.  In fp32 the sum of LA terms and k add at most (LA + 8) 2^-24
relative.  The release is written on the reduction d and not as e = min(m, a e + 1 - a): that form drifts in fp32 by up to
2^-25 / (1 - a), and f(d) = max(c, A d) composes to the same shape, so a frame's d is an associative scan.

The first LA output samples of a row are pre-roll, and ceil(LA / n) frames of zeros flush its tail: one frame, since a plan
is admitted only with 1 <= LA <= 512 and LA <= n <= 8192.  `gain_db` None bypasses the stage: an exact copy, no lag, no
state.  `gain_db` 0 is not a bypass: it limits at the ceiling.
"""

from __future__ import annotations

import math
import numbers
import struct

import numpy as np

MAX_LA = 512          # PTTS_LV_MAX_LA in csrc/ptts_level.h
MAX_N = 8192          # PTTS_LV_MAX_N
GAIN_DB_MIN, GAIN_DB_MAX = -40.0, 24.0
PEAK_DBFS_MIN, PEAK_DBFS_MAX = -20.0, 0.0
PEAK_DBFS_DEFAULT = -1.0


class LevelPlan:
    """What the leveler needs for one (rate, n): `n`, `LA` and the fp32 `a` and `k`."""

    __slots__ = ("rate", "n", "LA", "a", "k")

    def __init__(self, rate, n, LA, a, k):
        self.rate, self.n, self.LA, self.a, self.k = rate, n, LA, a, k

    @property
    def preroll(self) -> int:
        """output samples at the start of a row's stream that precede its first input sample"""
        return self.LA

    @property
    def drain_frames(self) -> int:
        """frames of zeros that flush the row's tail"""
        return -(-self.LA // self.n)

    def ints(self):
        """the plan as the C ABI takes it: n, LA and the bit patterns of a and k"""
        a, k = struct.unpack("<ii", struct.pack("<ff", float(self.a), float(self.k)))
        return (self.n, self.LA, a, k)


def plan(rate: int, n: int) -> LevelPlan:
    """The `LevelPlan` of frames of `n` samples at `rate` Hz, or ValueError naming the rule it fails"""
    rate, n = int(rate), int(n)
    if rate < 1:
        raise ValueError(f"level at {rate} Hz: the rate must be positive")
    LA = -(-5 * rate // 1000)
    if not 1 <= LA <= MAX_LA:
        raise ValueError(f"level at {rate} Hz: the look-ahead of {LA} samples exceeds the {MAX_LA} the leveler carries")
    if n < LA:
        raise ValueError(f"level at {rate} Hz: a frame of {n} samples is shorter than the look-ahead of {LA}")
    if n > MAX_N:
        raise ValueError(f"level at {rate} Hz: a frame of {n} samples exceeds the kernel's {MAX_N}")
    return LevelPlan(rate, n, LA, np.float32(math.exp(-1.0 / (0.100 * rate))), np.float32(1.0 / LA))


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
        raise ValueError(f"{name} must be a finite number, got {v!r}")
    return float(v)


def check(gain_db, peak_dbfs=None):
    """(gain_db, peak_dbfs) as floats, peak_dbfs defaulting to -1; (None, None) for a request without a gain (bypass).
    ValueError for a value that is no finite number or out of range, and for a peak without a gain"""
    if gain_db is None:
        if peak_dbfs is not None:
            raise ValueError("peak_dbfs is only meaningful together with gain_db")
        return None, None
    g = _number("gain_db", gain_db)
    if not GAIN_DB_MIN <= g <= GAIN_DB_MAX:
        raise ValueError(f"gain_db {g}: must be in [{GAIN_DB_MIN:g}, {GAIN_DB_MAX:g}]")
    p = PEAK_DBFS_DEFAULT if peak_dbfs is None else _number("peak_dbfs", peak_dbfs)
    if not PEAK_DBFS_MIN <= p <= PEAK_DBFS_MAX:
        raise ValueError(f"peak_dbfs {p}: must be in [{PEAK_DBFS_MIN:g}, {PEAK_DBFS_MAX:g}]")
    return g, p


def linear(db: float) -> np.float32:
    """fp32(10^(db / 20)), computed in float64"""
    return np.float32(10.0 ** (float(db) / 20.0))


def params(gain_db, peak_dbfs=None):
    """(G, C) as fp32 of a checked (gain_db, peak_dbfs)"""
    g, p = check(gain_db, peak_dbfs)
    if g is None:
        raise ValueError("gain_db None is a bypass: it has no parameters")
    return linear(g), linear(p)


def table(pairs):
    """The plan table of the distinct (rate, n) among `pairs`, in their order.  Returns (plans, index) with index[(rate, n)]
    = the plan's position; ValueError for a pair the rule refuses"""
    plans, index = [], {}
    for rate, n in pairs:
        key = (int(rate), int(n))
        if key not in index:
            index[key] = len(plans)
            plans.append(plan(*key))
    return plans, index
