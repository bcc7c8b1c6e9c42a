"""ITU-T G.711 in numpy, written from the Recommendation's tables: the two compressors on 16-bit linear samples and the two
expanders back to 16 bits.  The reference of tests/test_encoding_cpu.py and tests/test_gpu_encode.py.

mu-law (Table 2): the input is the 14-bit value s >> 2.  Its magnitude, clipped to 8158, plus the bias 33 lies in
[33, 8191]; chord e = 0 .. 7 holds [2^(e + 5), 2^(e + 6)) in 16 steps of 2^(e + 1).  The character is sign, chord, step with
every bit inverted; a positive value has the sign bit 1 before the inversion of the other seven.

A-law (Table 1): the input is the 13-bit value s >> 3.  A negative value v has the magnitude -v - 1, so that 0 and -1 share
the first step.  Chords 0 and 1 hold [0, 32) and [32, 64) in 16 steps of 2; chord e >= 2 holds [2^(e + 4), 2^(e + 5)) in 16
steps of 2^e.  The character is sign, chord, step with the even bits inverted (XOR 0x55); a positive value has the sign bit 1.

The expanders return the middle of a step on the 16-bit scale.
"""

from __future__ import annotations

import numpy as np

MU_CLIP, MU_BIAS = 8158, 33
MU_CHORDS = 64 << np.arange(7)   # first biased magnitude of chords 1 .. 7: 64, 128, .. 4096
A_CHORDS = 32 << np.arange(7)    # first magnitude of chords 1 .. 7: 32, 64, .. 2048


def s16(x) -> np.ndarray:
    """the 16-bit sample of fp32 x as every stage converts it: clamp to [-1, 1] (a NaN becomes -1), times 32767 in fp32,
    truncated towards zero"""
    x = np.asarray(x, np.float32)
    c = np.where(np.isnan(x), np.float32(-1), np.clip(x, np.float32(-1), np.float32(1))).astype(np.float32)
    return np.trunc(c * np.float32(32767.0)).astype(np.int16)


def lin2ulaw(s) -> np.ndarray:
    v = np.asarray(s).astype(np.int64) >> 2
    m = np.minimum(np.abs(v), MU_CLIP) + MU_BIAS
    e = (m[..., None] >= MU_CHORDS).sum(-1)
    step = (m >> (e + 1)) & 15
    char = (e << 4) | step
    return np.where(v >= 0, 0xFF ^ char, 0x7F ^ char).astype(np.uint8)


def lin2alaw(s) -> np.ndarray:
    v = np.asarray(s).astype(np.int64) >> 3
    m = np.where(v >= 0, v, -v - 1)
    e = (m[..., None] >= A_CHORDS).sum(-1)
    step = np.where(e == 0, m >> 1, m >> np.maximum(e, 1)) & 15
    char = (e << 4) | step
    return np.where(v >= 0, 0xD5 ^ char, 0x55 ^ char).astype(np.uint8)


def ulaw2lin(codes) -> np.ndarray:
    u = ~np.asarray(codes).astype(np.int64) & 0xFF
    e, step = (u >> 4) & 7, u & 15
    mag = (((2 * step + MU_BIAS) << e) - MU_BIAS) * 4  # the middle of the step, 14 bits -> 16
    return np.where(u & 0x80, -mag, mag).astype(np.int16)


def alaw2lin(codes) -> np.ndarray:
    a = np.asarray(codes).astype(np.int64) ^ 0x55
    e, step = (a >> 4) & 7, a & 15
    mag = np.where(e == 0, 2 * step + 1, (2 * step + 33) << np.maximum(e - 1, 0)) * 8  # 13 bits -> 16
    return np.where(a & 0x80, mag, -mag).astype(np.int16)


def ramp() -> tuple:
    """(s, x): s = -32767 .. 32767 and the fp32 x = (s +- 0.5) / 32767 that `s16` truncates back to exactly s"""
    s = np.arange(-32767, 32768, dtype=np.int64)
    x = (np.where(s >= 0, s + 0.5, s - 0.5) / 32767.0).astype(np.float32)
    return s.astype(np.int16), x
