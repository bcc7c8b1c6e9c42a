"""Per-request pitch: the plan rule of the streaming pitch shifter (the kernel is csrc/ptts_pitch.hip; numpy only, nothing
here touches the GPU).

A pitch shift by the frequency ratio r = P / Q (reduced, P, Q <= 20, 0.5 <= r <= 2) is a time-stretch by r - the stream gets
r times as long and keeps its pitch - followed by a resampling by 1 / r, which brings it back to its length and moves every
frequency by r.  A row's input line has `n` samples per frame at `rate` Hz: whatever leaves the stage before it.  The plan
of (r, rate, n):

  WSOLA part  `sp = stretch.plan(Q / P, rate, n)`, unchanged: Ha = Q u, Hs = P u.  It turns a frame into n_mid = n P / Q "mid"
              samples, and its contract is word for word that of `stretch.py`: positions, score, tie-break, the periodic
              Hann window as an fp32 table, zero before the stream's start and after the row is set to drain.
  FIR part    the causal polyphase filter of `resample.py` with (up, down) = (Q, P) over the mid stream:
              h = resample.prototype(Q, P), T = ceil((20 max(P, Q) + 1) / Q) taps per phase (T - 1 <= 40 = HIST),
                  y[N] = sum_j table[(N P) % Q][j] * mid[(N P) // Q - j],        table[ph][j] = h[ph + j Q] as fp32,
              mid = 0 before the stream's start.  A frame yields exactly n outputs and the phase is 0 at every frame start,
              because n_mid Q % P == 0.

n_out = n.  The first `preroll` = sp.L output samples of a row precede its first input sample ((L / Ha) Hs mid samples times
Q / P is L exactly), and a row needs drain_frames = ceil(L / n) frames of zeros to flush its tail.  The FIR's own group delay,
10 max(P, Q) / P <= 20 output samples, is NOT compensated: the same convention as the resampler, whose output lags by its
filter's delay as well.  r == 1 is the identity plan: a bit-exact copy with no state and no lag.  A ratio that `stretch.plan`
refuses is refused with that rule's message, prefixed with the pitch.

The shift moves the formants with the pitch (it is a resampling of the whole spectrum): a voice shifted far sounds like a
smaller or larger speaker, not like the same speaker singing another note.
"""

from __future__ import annotations

import math
import numbers
from fractions import Fraction

import numpy as np

from . import resample, stretch

HIST = 40            # mid samples a row carries from frame to frame (PTTS_PT_HIST in csrc/ptts_pitch.h)
PITCH_MIN, PITCH_MAX = 0.5, 2.0
MAX_TERM = 20        # largest P and Q


def fraction(pitch) -> Fraction:
    """pitch, a number or a "P/Q" string, as P / Q with P, Q <= 20, or ValueError"""
    if isinstance(pitch, str):
        try:
            pitch = Fraction(pitch.strip())
        except (ValueError, ZeroDivisionError):
            try:
                pitch = float(pitch)  # "nan", "inf": numbers, refused as such below
            except ValueError:
                raise ValueError(f"pitch {pitch!r}: must be a number or a fraction \"P/Q\"") from None
    if isinstance(pitch, bool) or not isinstance(pitch, numbers.Real) or not math.isfinite(pitch):
        raise ValueError(f"pitch must be a finite number, got {pitch!r}")
    f = Fraction(pitch).limit_denominator(MAX_TERM)
    if abs(float(f) - float(pitch)) > 1e-9 or f.numerator > MAX_TERM:
        raise ValueError(f"pitch {pitch}: must equal a fraction P / Q with P, Q <= {MAX_TERM}")
    return f


def _in_range(pitch, f):
    if not PITCH_MIN <= f <= PITCH_MAX:
        raise ValueError(f"pitch {pitch}: must be in [{PITCH_MIN}, {PITCH_MAX}]")


def taps(P: int, Q: int) -> int:
    """T, the taps per phase of the FIR part"""
    return -(-(20 * max(P, Q) + 1) // Q)


class PitchPlan:
    """What the pitcher needs for one (pitch, rate, n): the WSOLA plan `sp`, `P`, `Q`, the taps per phase `T`, the float64
    prototype `h` and the fp32 polyphase table `table[ph][j] = h[ph + j Q]` ([Q, T], zero-padded)."""

    __slots__ = ("pitch", "frac", "rate", "n", "sp", "P", "Q", "T", "h", "table")

    def __init__(self, frac, rate, n, sp):
        self.frac, self.pitch, self.rate, self.n, self.sp = frac, float(frac), rate, n, sp
        self.P, self.Q = frac.numerator, frac.denominator
        if self.identity:
            self.T, self.h, self.table = 1, np.ones(1), np.ones((1, 1), np.float32)
        else:
            self.T = taps(self.P, self.Q)
            self.h = resample.prototype(self.Q, self.P)
            t = np.zeros(self.Q * self.T, np.float64)
            t[:len(self.h)] = self.h
            self.table = np.ascontiguousarray(t.reshape(self.T, self.Q).T).astype(np.float32)

    @property
    def identity(self) -> bool:
        return self.P == self.Q

    @property
    def n_mid(self) -> int:
        """mid samples per frame"""
        return self.sp.n_out

    @property
    def n_out(self) -> int:
        return self.n

    @property
    def K(self) -> int:
        return self.sp.K

    @property
    def L(self) -> int:
        return self.sp.L

    @property
    def preroll(self) -> int:
        """output samples at the start of a row's stream that precede its first input sample (0 for the identity)"""
        return 0 if self.identity else self.sp.L

    @property
    def drain_frames(self) -> int:
        """frames of zeros that flush the row's tail (0 for the identity)"""
        return 0 if self.identity else -(-self.sp.L // self.n)

    def ints(self):
        """the plan as the C ABI takes it: (n, Ha, Hs, D, L, P, Q, T)"""
        return (*self.sp.ints(), self.P, self.Q, self.T)


def identity(rate: int, n: int) -> PitchPlan:
    """the copy plan of a line: what a request without a pitch (or with pitch 1) runs"""
    return PitchPlan(Fraction(1), int(rate), int(n), stretch.identity(rate, n))


def plan(pitch, rate: int = 24000, n: int = 1920) -> PitchPlan:
    """The `PitchPlan` of `pitch` for frames of `n` samples at `rate` Hz, or ValueError naming the rule it fails"""
    f = fraction(pitch)
    _in_range(pitch, f)
    rate, n = int(rate), int(n)
    if f == 1:
        return identity(rate, n)
    try:
        sp = stretch.plan(1 / f, rate, n)
    except ValueError as e:
        raise ValueError(f"pitch {f}: {e}") from None
    assert sp.Ha // f.denominator == sp.Hs // f.numerator and taps(f.numerator, f.denominator) - 1 <= HIST
    return PitchPlan(f, rate, n, sp)


def normalise_pitches(pitches) -> list:
    """a configured pitch list as floats of their fractions: 1.0 FIRST (index 0 is what a request without a pitch gets),
    every other pitch once, in the order given; ValueError for a pitch that is no fraction in range"""
    out = [1.0]
    for p in pitches:
        f = fraction(p)
        _in_range(p, f)
        if float(f) not in out:
            out.append(float(f))
    return out


def table(lines, pitches):
    """The plan table of (each distinct (rate, n) among `lines`, in their order) x (each pitch).  `pitches`: a list as
    `normalise_pitches` returns it.  Returns (plans, index) with index[(rate, n)][pitch index] = the plan's position in
    `plans`, or None where `plan` refuses the pair; pitch 1.0 is each line's identity plan.  ValueError for a pitch that is
    admissible on none of the lines."""
    plans, index = [], {}
    for rate, n in lines:
        key = (int(rate), int(n))
        if key in index:
            continue
        row = []
        for p in pitches:
            try:
                pl = identity(*key) if p == 1.0 else plan(p, *key)
            except ValueError:
                pl = None
            row.append(None if pl is None else len(plans))
            if pl is not None:
                plans.append(pl)
        index[key] = row
    for j, p in enumerate(pitches):
        if all(row[j] is None for row in index.values()):
            plan(p, *next(iter(index)))  # raises with the rule the pitch fails on the first line
            raise ValueError(f"pitch {p}: not admissible on any of the configured lines")
    return plans, index


def admissible(rate: int, n: int) -> list:
    """every ratio P / Q the rule admits on the line (rate, n), ascending, 1 included"""
    out = []
    for q in range(1, MAX_TERM + 1):
        for p in range(1, MAX_TERM + 1):
            f = Fraction(p, q)
            if math.gcd(p, q) != 1 or not PITCH_MIN <= f <= PITCH_MAX:
                continue
            try:
                if f != 1:
                    stretch.plan(1 / f, rate, n)
            except ValueError:
                continue
            out.append(f)
    return sorted(out)


def nearest(semitones, rate: int = 24000, n: int = 1920):
    """(Fraction, error in cents): the admissible ratio closest to 2^(semitones / 12) on the line (rate, n), and how far
    it lies above (+) or below (-) that"""
    if isinstance(semitones, bool) or not isinstance(semitones, numbers.Real) or not math.isfinite(semitones):
        raise ValueError(f"semitones must be a finite number, got {semitones!r}")
    if not -12 <= semitones <= 12:
        raise ValueError(f"semitones {semitones}: must be in [-12, 12]")
    cents = lambda f: 1200.0 * math.log2(float(f)) - 100.0 * float(semitones)  # noqa: E731
    best = min(admissible(rate, n), key=lambda f: (abs(cents(f)), f))
    return best, cents(best)
