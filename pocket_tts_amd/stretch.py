"""Per-request speaking rate: the plan rule of the streaming WSOLA time-stretch (the kernel is csrc/ptts_stretch.hip;
numpy only, nothing here touches the GPU).

A row's input stream `x` is what leaves the previous output stage for that row - the codec's PCM, or the resampler's
output when the row has a rate of its own - at `n_in` samples per frame; x[i] = 0 for i < 0 and for every i after the row
is set to drain.  A plan is (n_in, Ha, Hs, D, L) with window W = 2 Hs and K = n_in / Ha hops per frame.  Hop k = 0, 1, ...:

  1. position   p_k = k Ha - L + delta_k; delta_0 = 0, and for k >= 1 delta_k in [-D, D] maximises
                s(delta) = sum_{i < Hs} x[p_{k-1} + Hs + i] * x[k Ha - L + delta + i]      (fp32, no normalisation);
                among equal maxima the smallest |delta|, then the negative one
  2. overlap-add  y[k Hs + n] += w[n] * x[p_k + n], n < W, w the periodic Hann window as an fp32 table
  3. emit       y[k Hs .. (k + 1) Hs) is final; a frame emits n_out = K Hs samples

With L = Ha * ceil((D + W + Hs) / Ha) nothing past the current frame's end is read, and the oldest sample a frame reads
lies L + D + Ha before its first one.  The first (L / Ha) Hs output samples of a row are pre-roll (`preroll`), and a row needs
ceil((L / Ha) / K) frames of zeros to flush its tail (`drain_frames`).  Ha == Hs is the identity plan: an exact copy.

The plan of a speed (`plan`): speed = p / q with q <= 20 in [0.5, 2]; Ha = p u, Hs = q u with n_in % Ha == 0 and
ceil(0.008 rate) <= Hs <= floor(0.032 rate); among those u the one with Hs nearest 0.020 rate, then the smaller Hs;
D = ceil(0.006 rate); L + D + Ha <= HIST and L + D + Ha + n_in <= WINDOW.  Whole hops per frame keep the output count of a
frame fixed; that is why e.g. 0.9 and 1.1 are refused at 24 kHz (9 and 11 do not divide 1920).
"""

from __future__ import annotations

import math
import numbers
from fractions import Fraction

import numpy as np

HIST = 8192          # most input samples a row carries from frame to frame (PTTS_TS_HIST in csrc/ptts_stretch.h)
WINDOW = 12288       # most floats of carried samples || frame the kernel stages (PTTS_TS_WINDOW)
SPEED_MIN, SPEED_MAX = 0.5, 2.0
MAX_DENOMINATOR = 20


def hann(W: int) -> np.ndarray:
    """fp32 table of the periodic Hann window 0.5 - 0.5 cos(2 pi n / W), computed in float64"""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(W, dtype=np.float64) / W)).astype(np.float32)


class StretchPlan:
    """What the stretcher needs for one (rate, speed): `n_in`, `Ha`, `Hs`, `D`, `L` and the fp32 `window` (W floats)."""

    __slots__ = ("speed", "rate", "n_in", "Ha", "Hs", "D", "L", "window")

    def __init__(self, speed, rate, n_in, Ha, Hs, D, L):
        self.speed, self.rate, self.n_in, self.Ha, self.Hs, self.D, self.L = speed, rate, n_in, Ha, Hs, D, L
        self.window = hann(2 * Hs)

    @property
    def identity(self) -> bool:
        return self.Ha == self.Hs

    @property
    def W(self) -> int:
        return 2 * self.Hs

    @property
    def K(self) -> int:
        return self.n_in // self.Ha

    @property
    def n_out(self) -> int:
        """output samples per frame"""
        return self.K * self.Hs

    @property
    def preroll(self) -> int:
        """output samples at the start of a row's stream that precede its first input sample (0 for the identity)"""
        return 0 if self.identity else self.L // self.Ha * self.Hs

    @property
    def drain_frames(self) -> int:
        """frames of zeros that flush the row's tail (0 for the identity)"""
        return 0 if self.identity else -(-(self.L // self.Ha) // self.K)

    def ints(self):
        return (self.n_in, self.Ha, self.Hs, self.D, self.L)


def identity(rate: int, n_in: int) -> StretchPlan:
    """the copy plan of a rate: what a request without a speed (or with speed 1.0) runs"""
    return StretchPlan(1.0, int(rate), int(n_in), int(n_in), int(n_in), 0, 0)


def fraction(speed) -> Fraction:
    """speed as p / q with q <= 20, or ValueError"""
    if isinstance(speed, bool) or not isinstance(speed, numbers.Real) or not math.isfinite(speed):
        raise ValueError(f"speed must be a finite number, got {speed!r}")
    f = Fraction(speed).limit_denominator(MAX_DENOMINATOR)
    if abs(float(f) - float(speed)) > 1e-9:
        raise ValueError(f"speed {speed}: must equal a fraction p / q with q <= {MAX_DENOMINATOR}")
    return f


def plan(speed, rate: int = 24000, n_in: int = 1920) -> StretchPlan:
    """The `StretchPlan` of `speed` for frames of `n_in` samples at `rate` Hz, or ValueError naming the rule it fails"""
    f = fraction(speed)
    if not SPEED_MIN <= f <= SPEED_MAX:
        raise ValueError(f"speed {speed}: must be in [{SPEED_MIN}, {SPEED_MAX}]")
    rate, n_in = int(rate), int(n_in)
    p, q = f.numerator, f.denominator
    us = [u for u in range(1, n_in // p + 1) if n_in % (p * u) == 0]
    if not us:
        raise ValueError(f"speed {speed} at {rate} Hz: a frame of {n_in} samples is not a whole number of hops "
                         f"(no multiple of {p} divides {n_in})")
    lo, hi = -(-8 * rate // 1000), 32 * rate // 1000
    us = [u for u in us if lo <= q * u <= hi]
    if not us:
        raise ValueError(f"speed {speed} at {rate} Hz: no synthesis hop of 8 to 32 ms ({lo} to {hi} samples, a multiple of "
                         f"{q}) gives whole hops per frame of {n_in} samples")
    u = min(us, key=lambda u: (abs(50 * q * u - rate), q * u))  # |Hs - 0.020 rate|, then the smaller Hs
    Ha, Hs = p * u, q * u
    D = -(-6 * rate // 1000)
    L = Ha * -(-(D + 3 * Hs) // Ha)
    if L + D + Ha > HIST:
        raise ValueError(f"speed {speed} at {rate} Hz: a frame reaches {L + D + Ha} samples back, more than the {HIST} the "
                         "stretcher carries")
    if L + D + Ha + n_in > WINDOW:
        raise ValueError(f"speed {speed} at {rate} Hz: the staged window of {L + D + Ha + n_in} samples exceeds the kernel's "
                         f"{WINDOW}")
    return StretchPlan(float(f), rate, n_in, Ha, Hs, D, L)


def normalise_speeds(speeds) -> list:
    """a configured speed list as floats of their fractions: 1.0 FIRST (index 0 is what a request without a speed gets),
    every other speed once, in the order given; ValueError for a speed that is no fraction in range"""
    out = [1.0]
    for s in speeds:
        f = fraction(s)
        if not SPEED_MIN <= f <= SPEED_MAX:
            raise ValueError(f"speed {s}: must be in [{SPEED_MIN}, {SPEED_MAX}]")
        if float(f) not in out:
            out.append(float(f))
    return out


def table(rates, speeds):
    """The plan table of (each rate served) x (each speed).  `rates`: [(rate, n_in)], index 0 the native rate; `speeds`: a
    list as `normalise_speeds` returns it.  Returns (plans, index) with index[r][s] = the plan's position in `plans`, or
    None where `plan` refuses the pair; speed 1.0 is each rate's identity plan.  ValueError for a speed that is admissible
    at none of the rates."""
    plans, index = [], []
    for rate, n_in in rates:
        row = []
        for s in speeds:
            if s == 1.0:
                pl = identity(rate, n_in)
            else:
                try:
                    pl = plan(s, rate, n_in)
                except ValueError:
                    pl = None
            row.append(None if pl is None else len(plans))
            if pl is not None:
                plans.append(pl)
        index.append(row)
    for j, s in enumerate(speeds):
        if all(row[j] is None for row in index):
            plan(s, *rates[0])  # raises with the rule the speed fails at the native rate
            raise ValueError(f"speed {s}: not admissible at any of the configured rates")
    return plans, index
