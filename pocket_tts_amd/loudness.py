"""Per-request loudness target: a streaming ITU-R BS.1770-4 normaliser, the stage of the output chain
(`output_chain.py` gives its order) that sits behind the toner and before the peak limiter (the kernel is
csrc/ptts_loud.hip; numpy only, nothing here touches the GPU).

A row's input stream `x` is whatever leaves the previous stage for that row, `n` samples per frame; x[i] = 0 for i < 0 and
for every i after the row is set to drain.  A plan is a function of (rate, n):

  S = rate // 10        the sub-block: 100 ms
  D = 4 S               the delay and the pre-roll: 400 ms, one gating block
  the two K-weighting biquads as ten float64 coefficients (b0 b1 b2 a1 a2 of the shelf, then of the high-pass), each the
  bilinear transform of its analog prototype with K = tan(pi f0 / rate) and a0 = 1 + K / Q + K^2 (`kweighting`).  At
  48 kHz they are the table of the standard.

Per row there is a target T in [-40, -10] LUFS.  The stage computes

  v = shelf(x), w = highpass(v)                direct form, float64, zero initial state
  z_m = (1/S) sum w[i]^2, mS <= i < (m+1)S     m = 0, 1, ..
  Z_m = (z_{m-3} + .. + z_m) / 4               m >= 3        l_m = -0.691 + 10 log10 Z_m
  A_m = {3 <= q <= m : l_q > -70}              Gamma_m = -0.691 + 10 log10 mean_{A_m} Z - 10
  R_m = {q in A_m : l_q > Gamma_m}             L_m = -0.691 + 10 log10 mean_{R_m} Z      (undefined when A_m is empty)
  c_m = fp32(clamp(10^((T - L_m) / 20), 0.1, 10)), or c_{m-1} when L_m is undefined;  c_2 = 1
  knots k_0 = c_3, k_j = c_{j+2} (j >= 1)
  y[i] = 0 for i < D;  else q = i - D, j = q // S:
  y[i] = (k_j + (k_{j+1} - k_j) (q % S) / S) x[i - D]            in fp32

Both knots of delayed sub-block j are complete at its first output sample: c_{j+3} ends at input sample (j + 4) S - 1.
So the stage is causal with exactly D samples of lag.  A row keeps at most MAX_BLOCKS gating-block energies (102 s);
past that the measurement freezes and c holds its last value.  The gain is clamped to +-20 dB, and at a target of -16
LUFS speech peaks above 1.0, so the stage is always followed by the limiter (`level.py`).  A row without a target is on
bypass: an exact copy of its whole line, no lag, no state.

The kernel walks a frame as one 4-state linear recurrence s' = A s + B x (both biquads in transposed direct form II,
`step`): each thread runs CHUNK = ceil(n / THREADS) samples from a zero state, the chunk end states are combined by a scan
with the powers A^(CHUNK 2^t) (`powers`), and each thread re-runs its chunk from its true state.  The high-pass poles are
nearly a double pole next to z = 1, so A^k v cancels by a factor of about k: a power rounded to float64 would put a relative
error of 1e-13 into every state, frame after frame, which shows once the signal has decayed far below its level (1e-8 in a
gating block of digital silence).  `powers` therefore computes them in integers, 1280 bits wide, and hands each over as a
high and a low float64 part; with both the scan stays at the error of the serial float64 recurrence itself.
"""

from __future__ import annotations

import functools
import math
import numbers
from fractions import Fraction

import numpy as np

RATE_MIN, RATE_MAX = 8000, 48000  # PTTS_LD_MIN_RATE, PTTS_LD_MAX_RATE in csrc/ptts_loud.h
MAX_N = 8192                      # PTTS_LD_MAX_N
THREADS = 1024                    # PTTS_LD_THREADS
SCAN_STEPS = 10                   # PTTS_LD_SCAN: 2^10 = THREADS
MAX_BLOCKS = 1024                 # PTTS_LD_HIST: gating-block energies a row keeps
TARGET_MIN, TARGET_MAX = -40.0, -10.0
GAIN_MIN, GAIN_MAX = 0.1, 10.0    # +-20 dB
ABS_GATE = -70.0
REL_GATE = -10.0
OFFSET = -0.691

SHELF_F0, SHELF_G_DB, SHELF_Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
SHELF_VB_EXP = 0.4996667741545416
HP_F0, HP_Q = 38.13547087602444, 0.5003270373238773


def kweighting(rate: int) -> np.ndarray:
    """the ten float64 coefficients at `rate` Hz: b0 b1 b2 a1 a2 of the shelf, then of the high-pass (a0 = 1)"""
    K = math.tan(math.pi * SHELF_F0 / rate)
    Vh = 10.0 ** (SHELF_G_DB / 20.0)
    Vb = Vh ** SHELF_VB_EXP
    a0 = 1.0 + K / SHELF_Q + K * K
    shelf = [(Vh + Vb * K / SHELF_Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / SHELF_Q + K * K) / a0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / SHELF_Q + K * K) / a0]
    K = math.tan(math.pi * HP_F0 / rate)
    a0 = 1.0 + K / HP_Q + K * K
    hp = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / HP_Q + K * K) / a0]
    return np.array(shelf + hp, dtype=np.float64)


def step(coef, s, x):
    """One sample of the 4-state recurrence (ld_step in csrc/ptts_loud.h): both biquads in transposed direct form II.
    `s` is a list of four floats, changed in place; returns w"""
    b0, b1, b2, a1, a2, c0, c1, c2, d1, d2 = coef
    v = b0 * x + s[0]
    s[0] = b1 * x - a1 * v + s[1]
    s[1] = b2 * x - a2 * v
    w = c0 * v + s[2]
    s[2] = c1 * v - d1 * w + s[3]
    s[3] = c2 * v - d2 * w
    return w


def chunk_of(n: int) -> int:
    """samples a thread runs: ceil(n / THREADS)"""
    return -(-int(n) // THREADS)


def _matmul(P, Q):
    return [[sum(P[i][k] * Q[k][j] for k in range(4)) for j in range(4)] for i in range(4)]


_KEEP = 1280  # bits of the largest entry kept after a product: the shelf block decays to 1e-277 of the high-pass block, and stays exact


def _trim(M, e):
    """M 2^-e with the largest entry cut to _KEEP bits (the entries of a power are of one magnitude)"""
    cut = max(abs(v).bit_length() for row in M for v in row) - _KEEP
    if cut <= 0:
        return M, e
    return [[v >> cut for v in row] for row in M], e - cut


@functools.lru_cache(maxsize=256)
def _powers(coef: tuple, chunk: int) -> np.ndarray:
    cols = []
    for j in range(4):
        s = [Fraction(int(i == j)) for i in range(4)]
        step([Fraction(c) for c in coef], s, Fraction(0))
        cols.append(s)
    E = max(v.denominator.bit_length() - 1 for col in cols for v in col)
    A = [[int(cols[j][i] * (1 << E)) for j in range(4)] for i in range(4)]  # A[i][j] 2^E, exactly
    M, e = [[int(i == j) for j in range(4)] for i in range(4)], 0
    for _ in range(chunk):
        M, e = _trim(_matmul(M, A), e + E)
    out = np.empty((SCAN_STEPS, 2, 4, 4), dtype=np.float64)
    for t in range(SCAN_STEPS):
        for i in range(4):
            for j in range(4):
                v = Fraction(M[i][j], 1 << e) if e >= 0 else Fraction(M[i][j] << -e)
                hi = float(v)
                out[t, 0, i, j], out[t, 1, i, j] = hi, float(v - Fraction(hi))
        M, e = _trim(_matmul(M, M), 2 * e)
    out.setflags(write=False)
    return out


def powers(coef, chunk: int) -> np.ndarray:
    """[SCAN_STEPS, 2, 4, 4]: A^(chunk 2^t), t = 0 .. SCAN_STEPS - 1, as a high and a low float64 part.  A is the exact
    linear map of `step` with the float64 coefficients; its entries are dyadic rationals, and the powers are computed in
    integers cut to _KEEP bits after every product (not exact, but 2^-1280 where two doubles hold 2^-106) and rounded once.  Read-only: the plans of one (rate, chunk) share it"""
    return _powers(tuple(float(c) for c in coef), int(chunk))


class LoudPlan:
    """What the normaliser needs for one (rate, n): `S`, `D`, the K-weighting `coef` [10] and the scan's `powers`
    [SCAN_STEPS, 2, 4, 4] (high and low parts), all float64."""

    __slots__ = ("rate", "n", "S", "D", "chunk", "coef", "powers")

    def __init__(self, rate, n):
        self.rate, self.n = rate, n
        self.S = rate // 10
        self.D = 4 * self.S
        self.chunk = chunk_of(n)
        self.coef = kweighting(rate)
        self.powers = powers(self.coef, self.chunk)

    @property
    def preroll(self) -> int:
        """output samples at the start of a row's stream that precede its first input sample"""
        return self.D

    @property
    def drain_frames(self) -> int:
        """frames of zeros that flush the row's tail"""
        return -(-self.D // self.n)

    def ints(self):
        """the plan's integers as the C ABI takes them; the library derives S, D and the chunk itself"""
        return (self.rate, self.n)

    def doubles(self) -> np.ndarray:
        """the plan's float64 values as the C ABI takes them: coef, then powers"""
        return np.concatenate([self.coef, self.powers.reshape(-1)])


DOUBLES_PER_PLAN = 10 + SCAN_STEPS * 32


def plan(rate: int, n: int) -> LoudPlan:
    """The `LoudPlan` of frames of `n` samples at `rate` Hz, or ValueError naming the rule it fails"""
    rate, n = int(rate), int(n)
    if not RATE_MIN <= rate <= RATE_MAX:
        raise ValueError(f"loudness at {rate} Hz: the rate must be in [{RATE_MIN}, {RATE_MAX}]")
    if not 1 <= n <= MAX_N:
        raise ValueError(f"loudness at {rate} Hz: a frame of {n} samples is not in [1, {MAX_N}]")
    return LoudPlan(rate, n)


def check(loudness_lufs):
    """the target as a float, None for a request without one (bypass).  ValueError for a value that is no finite number
    or outside [TARGET_MIN, TARGET_MAX]"""
    if loudness_lufs is None:
        return None
    v = loudness_lufs
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
        raise ValueError(f"loudness_lufs must be a finite number, got {v!r}")
    if not TARGET_MIN <= float(v) <= TARGET_MAX:
        raise ValueError(f"loudness_lufs {float(v)}: must be in [{TARGET_MIN:g}, {TARGET_MAX:g}]")
    return float(v)


def check_with(loudness_lufs, gain_db):
    """`check(loudness_lufs)`, and ValueError for a target together with a gain: the one place that states the rule"""
    target = check(loudness_lufs)
    if target is not None and gain_db is not None:
        raise ValueError("loudness_lufs and gain_db exclude each other: the normaliser sets the gain")
    return target


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
