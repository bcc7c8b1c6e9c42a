"""fp64 reference of the streaming polyphase resampler (pocket_tts_amd/resample.py, csrc/ptts_resample.hip): frame by
frame, a history of HIST input samples carried between frames, zero before the stream's start.  Shared by the CPU tests
(against scipy.signal.upfirdn) and the GPU tests (against the kernel)."""

import numpy as np

from pocket_tts_amd.resample import HIST

RATES = (8000, 11025, 12000, 16000, 22050, 32000, 44100, 48000)  # the rates the admission rules are documented with
NATIVE, FRAME = 24000, 1920


def poly_table(h, up: int, T: int) -> np.ndarray:
    """float64 [up, T] polyphase table of the prototype taps h: table[ph][j] = h[ph + j * up], zero-padded"""
    t = np.zeros(up * T, np.float64)
    t[:len(h)] = h
    return np.ascontiguousarray(t.reshape(T, up).T)


class StreamRef:
    """One sequence.  `table`: [up, T] (any float dtype; used as float64, so the kernel's own fp32 taps can be given)."""

    def __init__(self, table, up: int, down: int, frame_samples: int = FRAME):
        self.table = np.asarray(table, np.float64)
        self.up, self.down, self.T = up, down, self.table.shape[1]
        self.fs = frame_samples
        assert frame_samples * up % down == 0 and self.T - 1 <= HIST
        self.out_n = frame_samples * up // down
        self.hist = np.zeros(HIST, np.float64)

    def frame(self, x):
        """x [frame_samples] -> (y float64 [out_n], bound [out_n]); bound = the standard bound of a length-T fp32 dot
        product accumulated in any order, with or without FMA, of exactly representable operands:
        |fl(sum) - sum| <= (T + 2) * 2^-24 * sum_j |h_j x_j|, plus 2^-24 absolute for the final rounding near zero."""
        x = np.asarray(x, np.float64)
        assert x.shape == (self.fs,)
        w = np.concatenate([self.hist, x])
        n = np.arange(self.out_n)
        i0, ph = (n * self.down) // self.up, (n * self.down) % self.up
        if self.up == 1 and self.down == 1:
            y, bound = x.copy(), np.zeros(self.fs)
        else:
            idx = HIST + i0[:, None] - np.arange(self.T)[None, :]
            assert idx.min() >= 0 and idx.max() < HIST + self.fs
            prod = self.table[ph] * w[idx]
            y = prod.sum(axis=1)
            bound = (self.T + 2) * 2.0 ** -24 * np.abs(prod).sum(axis=1) + 2.0 ** -24
        self.hist = w[-HIST:].copy()
        return y, bound


def to_i16(y) -> np.ndarray:
    """the codec's 16-bit conversion: (clamp(y, -1, 1) * 32767) truncated toward zero"""
    return np.trunc(np.clip(np.asarray(y, np.float64), -1.0, 1.0) * 32767.0).astype(np.int16)


def to_i16_f32(y) -> np.ndarray:
    """the same in fp32 arithmetic, as the kernel computes it from its own fp32 output"""
    v = np.clip(np.asarray(y, np.float32), np.float32(-1), np.float32(1)) * np.float32(32767)
    return np.trunc(v).astype(np.int16)
