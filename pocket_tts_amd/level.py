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

True-peak mode.  A row whose ceiling is given as `peak_dbtp` instead of `peak_dbfs` (the two exclude each other; same range
and default) limits the peak of the reconstructed waveform as ITU-R BS.1770-4 Annex 2 reads it, by 4x oversampling.

  interpolator  h = resample.prototype(4, 1): 81 float64 taps, the filter the resampler would use for 4x, group delay 40
                upsampled samples = D = 10 input samples; its phase 0 is a pure delay up to normalisation.  Phase p in
                {1, 2, 3} has T = 21 taps h_p[j] = h[p + 4 j], zero past index 80, rounded to fp32 once: `TP_TAPS` [3][21].
  detector      v_p[i] = sum over j = 0 .. 20 of h_p[j] u[i - j], in ascending j   (the 4x signal at time i - 10 + p / 4)
                P[i] = fmax(|u[i - 10]|, |v_1[i]|, |v_2[i]|, |v_3[i]|)             (u = 0 before the start and past the drain)
                r[i] = P[i] > C ? C / P[i] : 1
  limiter       m, d, e, g exactly as above from this r;  y[i] = g[i] u[i - 10 - LA]
  meter         M = fmax(M, |y[i - 10]|, |w_1[i]|, |w_2[i]|, |w_3[i]|), w_p the same FIR over y, M = 0 at `set_row`

The row's pre-roll is LA + 10 and a plan is admitted in this mode only with LA + 10 <= n, so one drain frame still flushes the
tail; its zeros also push the last 10 samples of y through the meter, so M is what a 4x meter (`true_peak`) reads on
everything the row wrote.  fmax drops a NaN operand: a NaN sample u[s] makes v_p[i] NaN for s <= i <= s + 20, where P falls
back to |u[i - 10]|, the sample peak; at i = s + 10 that is NaN too, P is NaN, compares false and r = 1.  So a NaN costs one
output sample, y[s + 10 + LA], as in sample-peak mode, and the meter skips the 21 values of each w_p that hold it.

What holds.  P[i + 10] >= |u[i]|, so g[i + 10 + LA] <= r[i + 10] <= C / |u[i]| by the argument above and the sample-peak
bound |y| <= C still holds exactly.  The true-peak bound does not: g varies across the 21 taps, so w_p is not g v_p.  The excess
over C is measured on the float64 reference, not promised ("true peak", quotes it: hundredths of a dB).  A 4x meter
under-reads the continuous peak by design; a 16x meter reads +0.1 to +0.36 dB over the ceiling on the same outputs.  The
stage meets the standard's meter, not a finer one.

fp32 in this mode.  v_p is 21 products and 20 additions: |fp32(v_p) - v_p| <= 22 2^-24 sum |h_p[j]| |u[i - j]| <=
22 2^-24 S max|u| with S = `TP_S` = max over p of sum |h_p| (2.2414).  r moves by |C / P - C / P'| = C |P - P'| / (P P') <=
|P - P'| / C, since r < 1 only where P, P' > C; m, d, e and g are minima, maxima and averages of r and move by no more.  So y
moves by at most 22 2^-24 S (max|u| / C) max|u| on top of the (LA + 64) 2^-24 max|u| of sample-peak mode: `tp_error_bound`.
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
TP_DELAY = 10         # D: the interpolator's group delay in input samples (PTTS_LV_TP_D)
TP_NTAPS = 21         # T: taps per phase (PTTS_LV_TP_T)


def _tp_taps() -> np.ndarray:
    from . import resample

    h = resample.prototype(4, 1)
    t = np.zeros((3, TP_NTAPS), np.float64)
    for p in (1, 2, 3):
        hp = h[p::4]
        t[p - 1, :len(hp)] = hp
    return t.astype(np.float32)


TP_TAPS = _tp_taps()  # [3][21] fp32: phase p of the 4x interpolator at TP_TAPS[p - 1]
TP_TAPS.setflags(write=False)
TP_S = float(np.abs(TP_TAPS.astype(np.float64)).sum(axis=1).max())


def tp_error_bound(LA: int, umax: float, C: float) -> float:
    """the bound on |y - y64| / max|u| of a true-peak row (the docstring's last paragraph)"""
    return (LA + 64) * 2.0 ** -24 + 22 * 2.0 ** -24 * TP_S * max(1.0, float(umax) / float(C))


def true_peak(samples) -> float:
    """What a BS.1770-4 Annex 2 meter reads on `samples` (one channel, any float or int16 array, int16 scaled by 1 / 32768):
    the largest magnitude of the signal oversampled 4x with `TP_TAPS`, in float64, linear (1.0 = 0 dBTP); zeros follow the
    last sample, so its ringing counts.  NaN values are skipped, as the device meter skips them.  0.0 for no samples."""
    x = np.asarray(samples)
    x = x.astype(np.float64) / 32768.0 if x.dtype == np.int16 else x.astype(np.float64)
    x = x.reshape(-1)
    if x.size == 0:
        return 0.0
    peak = np.fmax.reduce(np.abs(x), initial=0.0)
    for hp in TP_TAPS.astype(np.float64):
        peak = max(peak, np.fmax.reduce(np.abs(np.convolve(x, hp)), initial=0.0))
    return float(peak)


def dbtp(linear_peak) -> float:
    """20 log10 of a linear true peak; -inf for 0"""
    return 20.0 * math.log10(linear_peak) if linear_peak > 0 else -math.inf


class LevelPlan:
    """What the leveler needs for one (rate, n): `n`, `LA` and the fp32 `a` and `k`."""

    __slots__ = ("rate", "n", "LA", "a", "k", "true_peak")

    def __init__(self, rate, n, LA, a, k, true_peak=False):
        self.rate, self.n, self.LA, self.a, self.k, self.true_peak = rate, n, LA, a, k, bool(true_peak)

    @property
    def preroll(self) -> int:
        """output samples at the start of a row's stream that precede its first input sample"""
        return self.LA + (TP_DELAY if self.true_peak else 0)

    @property
    def drain_frames(self) -> int:
        """frames of zeros that flush the row's tail"""
        return -(-self.preroll // self.n)

    def ints(self):
        """the plan as the C ABI takes it: n, LA and the bit patterns of a and k"""
        a, k = struct.unpack("<ii", struct.pack("<ff", float(self.a), float(self.k)))
        return (self.n, self.LA, a, k)


def plan(rate: int, n: int, true_peak: bool = False) -> LevelPlan:
    """The `LevelPlan` of frames of `n` samples at `rate` Hz, or ValueError naming the rule it fails.  `true_peak`: as a row in
    true-peak mode uses it, with the pre-roll LA + 10 and the rule LA + 10 <= n; the plan's n, LA, a and k are the same"""
    rate, n = int(rate), int(n)
    if rate < 1:
        raise ValueError(f"level at {rate} Hz: the rate must be positive")
    LA = -(-5 * rate // 1000)
    if not 1 <= LA <= MAX_LA:
        raise ValueError(f"level at {rate} Hz: the look-ahead of {LA} samples exceeds the {MAX_LA} the leveler carries")
    if n < LA:
        raise ValueError(f"level at {rate} Hz: a frame of {n} samples is shorter than the look-ahead of {LA}")
    if true_peak and n < LA + TP_DELAY:
        raise ValueError(f"level at {rate} Hz: a frame of {n} samples is shorter than the look-ahead of {LA} plus the "
                         f"true-peak detector's delay of {TP_DELAY}")
    if n > MAX_N:
        raise ValueError(f"level at {rate} Hz: a frame of {n} samples exceeds the kernel's {MAX_N}")
    return LevelPlan(rate, n, LA, np.float32(math.exp(-1.0 / (0.100 * rate))), np.float32(1.0 / LA), true_peak)


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
        raise ValueError(f"{name} must be a finite number, got {v!r}")
    return float(v)


def check(gain_db, peak_dbfs=None, peak_dbtp=None):
    """(gain_db, peak_dbfs) as floats, peak_dbfs defaulting to -1; (None, None) for a request without a gain (bypass).
    ValueError for a value that is no finite number or out of range, and for a peak without a gain.  With `peak_dbtp`, the
    ceiling as a true peak, the result is (gain_db, peak_dbtp): same range, same rules; ValueError for both ceilings together"""
    if peak_dbtp is not None:
        if peak_dbfs is not None:
            raise ValueError("peak_dbfs and peak_dbtp exclude each other: a ceiling is a sample peak or a true peak")
        if gain_db is None:
            raise ValueError("peak_dbtp is only meaningful together with gain_db")
        g = check(gain_db)[0]
        p = _number("peak_dbtp", peak_dbtp)
        if not PEAK_DBFS_MIN <= p <= PEAK_DBFS_MAX:
            raise ValueError(f"peak_dbtp {p}: must be in [{PEAK_DBFS_MIN:g}, {PEAK_DBFS_MAX:g}]")
        return g, p
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
