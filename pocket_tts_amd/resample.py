"""Per-request output sample rates: the filter design and the admission rules of the streaming polyphase resampler
(the kernel is csrc/ptts_resample.hip; numpy only, nothing here touches the GPU).

The codec produces `frame_samples` (1920) samples per frame at its native rate (24 kHz).  A request may ask for another
rate; its frames then go through the causal polyphase FIR

    y[N] = sum_k h[k] * x_up[N * down - k],        x_up = x with up - 1 zeros between samples, (up, down) = ratio(rate, native)

which is `scipy.signal.upfirdn(h, x, up, down)`.  `h` is the prototype `scipy.signal.resample_poly` designs by default:
L = 20 * max(up, down) + 1 taps of a windowed sinc with cutoff 1 / max(up, down) and a Kaiser window (beta = 5), scaled by
`up`; it is computed here with `np.sinc` and `np.kaiser` in float64, so the product does not need scipy for it.  Input
before the stream's start counts as zero, the convention of the streaming convolutions' zero carries.  The native rate
(up = down = 1) is an exact copy, not a filter.

A rate is admitted only when
  * RATE_MIN <= rate <= RATE_MAX,
  * frame_samples * up % down == 0: every frame yields a whole number out_n = frame_samples * up / down of output samples
    and the filter's phase is 0 at each frame start, so a frame needs nothing from its predecessor but input samples,
  * the taps per phase T = ceil(L / up) satisfy T - 1 <= HIST: a frame's first output reaches T - 1 samples back, and HIST
    is what the kernel carries from one frame to the next.
At 24 kHz that admits, among others, 8000 (640 samples per frame), 11025 (882), 12000, 16000 (1280), 22050 (1764), 32000
(2560), 44100 (3528) and 48000 (3840).

Consequence of the causal form: the output lags the input by the filter's group delay, (L - 1) / 2 = 10 * max(up, down)
samples at the upsampled rate = 10 * max(up, down) / up input samples (30 samples = 1.25 ms at 8 kHz, 10 samples = 0.42 ms
at 48 kHz).  That tail of each text chunk is not flushed: a chunk's last 10 * max(up, down) / up input samples shape no
output (chunks restart the codec from zero state anyway, and the resampler's history with it).
"""

from __future__ import annotations

import math
import numbers

import numpy as np

HIST = 64            # input samples carried from one frame to the next (PTTS_RS_HIST in csrc/ptts_resample.h)
RATE_MIN, RATE_MAX = 8000, 48000


def ratio(rate: int, native: int) -> tuple[int, int]:
    """(up, down) of `rate` / `native`, reduced by the gcd"""
    g = math.gcd(int(rate), int(native))
    return int(rate) // g, int(native) // g


def prototype(up: int, down: int) -> np.ndarray:
    """float64 taps of the prototype low-pass: `firwin(L, 1 / max(up, down), window=("kaiser", 5.0)) * up`"""
    m = max(up, down)
    L = 20 * m + 1
    c = 1.0 / m
    k = np.arange(L, dtype=np.float64) - 0.5 * (L - 1)
    h = c * np.sinc(c * k) * np.kaiser(L, 5.0)
    return h / h.sum() * up


class RatePlan:
    """What the resampler needs for one rate: `up`, `down`, the taps per phase `taps` (T), the output samples per frame
    `out_n`, the float64 prototype `h` and the fp32 polyphase table `table[ph][j] = h[ph + j * up]` (zero-padded to
    [up, T]).  `native` is True for up = down = 1 (a copy: the table is [[1.0]] and never read)."""

    __slots__ = ("rate", "up", "down", "taps", "out_n", "h", "table")

    def __init__(self, rate, up, down, taps, out_n, h, table):
        self.rate, self.up, self.down, self.taps, self.out_n, self.h, self.table = rate, up, down, taps, out_n, h, table

    @property
    def native(self) -> bool:
        return self.up == 1 and self.down == 1

    @property
    def delay_input_samples(self) -> float:
        """the group delay in input samples (0 for the native rate)"""
        return 0.0 if self.native else 10.0 * max(self.up, self.down) / self.up


def plan(rate, native: int = 24000, frame_samples: int = 1920) -> RatePlan:
    """The `RatePlan` of `rate`, or ValueError naming the admission rule it fails"""
    if isinstance(rate, bool) or not isinstance(rate, numbers.Integral):
        raise ValueError(f"sample rate must be an integer, got {rate!r}")
    rate = int(rate)
    if not RATE_MIN <= rate <= RATE_MAX:
        raise ValueError(f"sample rate {rate}: must be in [{RATE_MIN}, {RATE_MAX}]")
    up, down = ratio(rate, native)
    if frame_samples * up % down != 0:
        raise ValueError(f"sample rate {rate}: a frame of {frame_samples} samples at {native} Hz is not a whole number of "
                         f"output samples ({frame_samples} * {up} / {down})")
    if up == 1 and down == 1:
        return RatePlan(rate, 1, 1, 1, frame_samples, np.ones(1), np.ones((1, 1), np.float32))
    L = 20 * max(up, down) + 1
    T = -(-L // up)
    if T - 1 > HIST:
        raise ValueError(f"sample rate {rate}: the filter needs {T - 1} samples of history per frame, more than the "
                         f"{HIST} the resampler carries")
    h = prototype(up, down)
    table = np.zeros(up * T, np.float64)
    table[:L] = h
    table = np.ascontiguousarray(table.reshape(T, up).T)  # [ph][j] = h[ph + j * up]
    return RatePlan(rate, up, down, T, frame_samples * up // down, h, table.astype(np.float32))


def plans(sample_rates, native: int = 24000, frame_samples: int = 1920) -> list:
    """The plans of a configured rate list with the native rate FIRST (index 0 is what a request without a rate gets) and
    every other rate once, in the order given"""
    out = [plan(native, native, frame_samples)] if RATE_MIN <= native <= RATE_MAX else \
        [RatePlan(native, 1, 1, 1, frame_samples, np.ones(1), np.ones((1, 1), np.float32))]
    for r in sample_rates:
        p = plan(r, native, frame_samples)
        if all(p.rate != q.rate for q in out):
            out.append(p)
    return out
