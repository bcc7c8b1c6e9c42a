"""float64 reference of the streaming WSOLA time-stretch (pocket_tts_amd/stretch.py states the contract; the kernel is
csrc/ptts_stretch.hip).  numpy only.

`x` is a row's input stream; x[i] = 0 for i < 0 and for i >= len(x) (the row drains).  A plan `p` has n_in, Ha, Hs, D, L and
the fp32 `window` table.  Everything but the window table (which the kernel is handed as fp32) is float64.
"""

from __future__ import annotations

import numpy as np


def _at(x, start, n):
    """x[start .. start + n) as float64, zeros outside x"""
    out = np.zeros(n, np.float64)
    lo, hi = max(start, 0), min(start + n, len(x))
    if hi > lo:
        out[lo - start:hi - start] = x[lo:hi]
    return out


def scores(x, p, k, p_prev):
    """(s, a): s[d + D] = sum_i t[i] x[k Ha - L + d + i] and a[d + D] = sum_i |t[i] x[..]| for d in [-D, D], with the template
    t = x[p_prev + Hs .. p_prev + 2 Hs), all in float64"""
    t = _at(x, p_prev + p.Hs, p.Hs)
    seg = _at(x, k * p.Ha - p.L - p.D, 2 * p.D + p.Hs)
    win = np.lib.stride_tricks.sliding_window_view(seg, p.Hs)  # [2 D + 1, Hs]
    return win @ t, np.abs(win) @ np.abs(t)


def choose(s, D):
    """the delta of the largest score; among equal maxima the smallest |delta|, then the negative one"""
    best = np.flatnonzero(s == s.max()) - D
    return int(min(best, key=lambda d: (abs(d), d)))


def overlap_add(x, p, deltas):
    """y[0 .. len(deltas) Hs) of the hops 0 .. len(deltas) - 1 placed at the given deltas"""
    W, Hs = 2 * p.Hs, p.Hs
    w = p.window.astype(np.float64)
    y = np.zeros((len(deltas) + 1) * Hs, np.float64)
    for k, d in enumerate(deltas):
        y[k * Hs:k * Hs + W] += w * _at(x, k * p.Ha - p.L + d, W)
    return y[:len(deltas) * Hs]


def wsola(x, p, frames):
    """(y, deltas) of `frames` frames of the stream x: y has frames * n_out samples (pre-roll included)"""
    x = np.asarray(x, np.float64)
    if p.identity:
        return _at(x, 0, frames * p.n_in), []
    deltas, prev = [], None
    for k in range(frames * p.K):
        d = 0 if k == 0 else choose(scores(x, p, k, prev)[0], p.D)
        prev = k * p.Ha - p.L + d
        deltas.append(d)
    return overlap_add(x, p, deltas), deltas


class Stream:
    """The same computation with the state a streaming implementation keeps: the last L + D + Ha input samples, the second
    half of the last segment, the last delta and whether a hop has happened.  `feed(frame)` returns the frame's n_out
    samples and appends its deltas to `deltas`.  Reads outside carried || frame raise: the plan's causality claim."""

    def __init__(self, p):
        self.p = p
        self.reach = p.L + p.D + p.Ha
        self.hist = np.zeros(self.reach, np.float64)
        self.carry = np.zeros(p.Hs, np.float64)
        self.dprev, self.started = 0, False
        self.deltas: list = []

    def feed(self, frame):
        p = self.p
        frame = np.asarray(frame, np.float64)
        assert len(frame) == p.n_in
        if p.identity:
            return frame.copy()
        w = np.concatenate([self.hist, frame])
        win = p.window.astype(np.float64)
        out = np.zeros(p.n_out, np.float64)

        def cut(a, n):
            assert 0 <= a and a + n <= len(w), "read outside carried || frame"
            return w[a:a + n]

        for j in range(p.K):
            d = 0
            if self.started:
                t = cut(self.reach + (j - 1) * p.Ha - p.L + self.dprev + p.Hs, p.Hs)
                seg = cut(self.reach + j * p.Ha - p.L - p.D, 2 * p.D + p.Hs)
                d = choose(np.lib.stride_tricks.sliding_window_view(seg, p.Hs) @ t, p.D)
            s = cut(self.reach + j * p.Ha - p.L + d, 2 * p.Hs)
            out[j * p.Hs:(j + 1) * p.Hs] = self.carry + win[:p.Hs] * s[:p.Hs]
            self.carry = win[p.Hs:] * s[p.Hs:]
            self.dprev, self.started = d, True
            self.deltas.append(d)
        self.hist = w[p.n_in:].copy()
        return out


def pcm16(v):
    """the library's 16-bit conversion of float32 samples: (clamp(v, -1, 1) * 32767) truncated, in float32"""
    v = np.asarray(v, np.float32)
    return (np.clip(v, np.float32(-1), np.float32(1)) * np.float32(32767)).astype(np.int16)
