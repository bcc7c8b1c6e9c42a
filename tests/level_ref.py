"""float64 restatement of the output-level contract (pocket_tts_amd/level.py), for the tests: the whole signal at once
(`level`) and frame by frame with carried state (`Stream`).  Both are fed the fp32 G, C, a, k of a row and its plan and do
every operation in float64."""

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def _stages(u, r_hist, e_hist, d_prev, C, LA, a, k):
    """u: the new samples (float64); r_hist / e_hist: the LA values before them.  Returns (r, m, d, e, g) of the new samples."""
    au = np.abs(u)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(au > C, C / au, 1.0)  # a NaN compares false
    m = sliding_window_view(np.concatenate([r_hist, r]), LA + 1).min(axis=1)
    c = 1.0 - m
    d = np.empty(len(u))
    prev = d_prev
    for i in range(len(u)):
        prev = max(c[i], a * prev)
        d[i] = prev
    e = 1.0 - d
    g = k * sliding_window_view(np.concatenate([e_hist[1:], e]), LA).sum(axis=1)
    return r, m, d, e, g


def level(x, G, C, LA, a, k, full=False):
    """y of the whole stream x (len(x) samples: y[i] = g[i] u[i - LA]); with `full` also (u, r, g)"""
    G, C, a, k = float(G), float(C), float(a), float(k)
    u = G * np.asarray(x, np.float64)
    r, m, d, e, g = _stages(u, np.ones(LA), np.ones(LA), 0.0, C, LA, a, k)
    y = g * np.concatenate([np.zeros(LA), u])[:len(u)]
    return (y, u, r, g) if full else y


class Stream:
    """the same, one frame at a time: carries the last LA samples of u, r and e and the last d"""

    def __init__(self, G, C, LA, a, k):
        self.G, self.C, self.LA, self.a, self.k = float(G), float(C), int(LA), float(a), float(k)
        self.u = np.zeros(LA)
        self.r = np.ones(LA)
        self.e = np.ones(LA)
        self.d = 0.0

    def feed(self, frame):
        LA = self.LA
        u = self.G * np.asarray(frame, np.float64)
        r, m, d, e, g = _stages(u, self.r, self.e, self.d, self.C, LA, self.a, self.k)
        y = g * np.concatenate([self.u, u])[:len(u)]
        self.u = np.concatenate([self.u, u])[-LA:]
        self.r = np.concatenate([self.r, r])[-LA:]
        self.e = np.concatenate([self.e, e])[-LA:]
        self.d = float(d[-1])
        return y


def level_f32(x, G, C, LA, a, k):
    """the contract in fp32, sample by sample (numpy scalars): what the kernel's arithmetic amounts to up to the order of the
    scan's combines; for the CPU checks of the ceiling and of the error bound"""
    f = np.float32
    G, C, a, k = f(G), f(C), f(a), f(k)
    u = (G * np.asarray(x, f)).astype(f)
    au = np.abs(u)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(au > C, (C / au).astype(f), f(1))
    m = sliding_window_view(np.concatenate([np.ones(LA, f), r]), LA + 1).min(axis=1)
    c = (f(1) - m).astype(f)
    e = np.empty(len(u), f)
    prev = f(0)
    for i in range(len(u)):
        prev = max(c[i], f(a * prev))
        e[i] = f(1) - prev
    ee = np.concatenate([np.ones(LA - 1, f), e])
    s = np.zeros(len(u), f)
    for t in range(LA):  # ascending index within each window, one fp32 addition per term
        s = (s + ee[t:t + len(u)]).astype(f)
    g = (k * s).astype(f)
    return (g * np.concatenate([np.zeros(LA, f), u])[:len(u)]).astype(f)


def signal(n_total, seed=0, env_period=9000, spikes=()):
    """band-limited noise under a slow envelope (float32), with full-scale single samples at `spikes`"""
    rng = np.random.default_rng(seed)
    w = np.hanning(33)
    x = np.convolve(rng.standard_normal(n_total + 32), w / np.sqrt((w ** 2).sum()), mode="valid")[:n_total]
    env = 0.06 + 0.22 * (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_total) / env_period))
    x = np.clip(x * env, -0.95, 0.95)
    for i, s in enumerate(spikes):
        x[s] = 1.0 if i % 2 == 0 else -1.0
    return x.astype(np.float32)


# the limiting rows of the GPU test, (rate, n, gain_db): three share one launch with a bypass row, the 48 kHz row (two tiles)
# has a launch of its own
GPU_ROWS = [(24000, 1920, 12.0), (8000, 640, 12.0), (24000, 960, -6.0), (48000, 3840, 12.0)]
GPU_FRAMES = 4


def gpu_signal(rate, n, frames=GPU_FRAMES):
    """the input of a GPU-test row: noise under an envelope plus full-scale single samples at a frame's last sample, the next
    frame's first, index 5 of the stream and, where the frame has two tiles, on both sides of a tile boundary (2047 | 2048)"""
    spikes = [n - 1, 2 * n, 5] + ([n + 2047, 2 * n + 2048] if n > 2048 else [])
    return signal(frames * n, seed=n, env_period=int(2.2 * n), spikes=spikes)


def pcm16(y):
    """the int16 conversion of the output kernels, on an fp32 array"""
    y = np.asarray(y, np.float32)
    with np.errstate(invalid="ignore"):
        return (np.minimum(np.maximum(y, np.float32(-1)), np.float32(1)) * np.float32(32767)).astype(np.int16)
