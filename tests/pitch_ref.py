"""float64 reference of the streaming pitch shifter (pocket_tts_amd/pitch.py states the contract; the kernel is
csrc/ptts_pitch.hip): the composition of the two references the project already has - `stretch_ref` for the mid stream,
`resample_ref.StreamRef` with (up, down) = (Q, P) over frames of n_mid samples for the FIR, with its error bound.  numpy only.
"""

from __future__ import annotations

import numpy as np

import stretch_ref
from resample_ref import StreamRef, poly_table


def _signal(n, period, seed):
    """band-limited noise plus an impulse train (9-sample Hann pulses every `period` samples), float32, |x| < 1"""
    rng = np.random.default_rng(seed)
    h = np.hanning(33)
    x = np.convolve(rng.standard_normal(n + 32), h / h.sum(), mode="valid")[:n] * 0.3
    for s in range(period // 2, n - 9, period):
        x[s:s + 9] += 0.8 * np.hanning(9)
    return x.astype(np.float32)


def table64(p) -> np.ndarray:
    """the plan's polyphase table [Q, T] in float64, from its float64 prototype"""
    return poly_table(p.h, p.Q, p.T)


def fir(mid, p, table):
    """(y, bound, gain) of the FIR part over a whole mid stream (a whole number of frames of n_mid samples, zero before its
    start): y float64, bound = `StreamRef`'s bound of an fp32 evaluation with `table`, gain[N] = sum_j |table[phase(N)][j]|"""
    mid = np.asarray(mid, np.float64)
    frames = len(mid) // p.n_mid
    assert frames * p.n_mid == len(mid)
    if p.identity:
        return mid.copy(), np.zeros(len(mid)), np.ones(len(mid))
    ref = StreamRef(table, p.Q, p.P, frame_samples=p.n_mid)
    assert ref.out_n == p.n and ref.T == p.T
    parts = [ref.frame(mid[f * p.n_mid:(f + 1) * p.n_mid]) for f in range(frames)]
    ph = (np.arange(p.n) * p.P) % p.Q
    gain = np.tile(np.abs(np.asarray(table, np.float64)).sum(axis=1)[ph], frames)
    return np.concatenate([y for y, _ in parts]), np.concatenate([b for _, b in parts]), gain


class Stream:
    """One row, frame by frame, with the state a streaming implementation keeps: `stretch_ref.Stream` for the WSOLA part, a
    `StreamRef` for the FIR.  `feed(frame)` returns the frame's n samples; `deltas` and `mid` collect the taps."""

    def __init__(self, p, table=None):
        self.p = p
        self.ws = stretch_ref.Stream(p.sp)
        self.fir = None if p.identity else StreamRef(table64(p) if table is None else table, p.Q, p.P, frame_samples=p.n_mid)
        self.mid: list = []

    @property
    def deltas(self):
        return self.ws.deltas

    def feed(self, frame):
        if self.p.identity:
            return np.asarray(frame, np.float64).copy()
        m = self.ws.feed(frame)
        self.mid.append(m)
        return self.fir.frame(m)[0]


def pitch(x, p, frames, table=None):
    """(y, bound, gain, mid, deltas) of `frames` frames of the stream x (zeros behind its end): the whole-signal WSOLA of
    `stretch_ref.wsola`, then `fir` with `table` (None: the float64 table)"""
    mid, deltas = stretch_ref.wsola(x, p.sp, frames)
    y, bound, gain = fir(mid, p, table64(p) if table is None else table)
    return y, bound, gain, mid, deltas
