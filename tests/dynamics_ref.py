"""The dynamics stage's contract (pocket_tts_amd/dynamics.py) restated in float64, for the tests, with this file's own code:
`Serial` is the definition, one Python loop per sample, fed frame by frame and carrying (p, s) between frames; `Chunked` is
the kernel's chunk / scan / re-run scheme over 1024 threads with the same carried state, used only to measure E, the largest
|s_chunked - s_serial| in dB.  `ROWS`, `F` and `signal` are the rows of tests/test_gpu_dynamics.py, shared with the CPU test
that measures E over them.  Plain numpy; nothing here imports the package."""

from __future__ import annotations

import math

import numpy as np

K = math.log(10.0) / 20.0
KEYS = ("threshold", "ratio", "knee", "attack", "release", "makeup")
PRESETS = {  # T, R, W, attack ms, release ms, M
    "speech": (-20.0, 3.0, 6.0, 5.0, 100.0, 4.0),
    "gentle": (-16.0, 2.0, 10.0, 10.0, 200.0, 2.0),
    "broadcast": (-24.0, 4.0, 8.0, 3.0, 150.0, 8.0),
    "telephone": (-18.0, 6.0, 4.0, 2.0, 60.0, 6.0),
}

CORNER = "threshold=-60;ratio=20;knee=0;attack=0.1;release=10;makeup=24"
F = 8  # frames: gated noise, digital silence in frames 3 and 4 (the release rings out), a full-scale sample in frame 5
# (rate, n, setting); None: bypass.  chunk 2; fewer threads than the block; the last thread holds one sample (1025 = 512 * 2
# + 1) at the corner of the grammar; less than one wave; chunk 8
ROWS = [None, (24000, 1920, "speech"), (8000, 640, "telephone"), (24000, 1025, CORNER), (24000, 63, "gentle"),
        (48000, 7680, "broadcast")]
WIDTH = 7680
ODD = 2  # the row with a NaN and an Inf sample


def parse(setting):
    """(T, R, W, attack, release, M) of a preset or a pair list of valid syntax; keys left out are those of `speech`"""
    if setting in PRESETS:
        return PRESETS[setting]
    v = dict(zip(KEYS, PRESETS["speech"]))
    for pair in setting.split(";"):
        key, value = pair.split("=")
        v[key.strip()] = float(value)
    return tuple(v[k] for k in KEYS)


def signal(n, seed, odd=False):
    """F frames of n samples, fp32: noise gated between -12 dBFS and -50 dBFS peaks every max(16, n // 3) samples, so that
    it crosses every threshold in both directions; frames 3 and 4 digital silence; one full-scale sample in frame 5; `odd`:
    a NaN in frame 1 and an Inf in frame 6"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(F * n)
    gate = (np.arange(F * n) // max(16, n // 3)) % 2 == 0
    x *= np.where(gate, 0.25, 0.003)
    x[3 * n:5 * n] = 0.0
    x[5 * n + n // 2] = -1.0
    if odd:
        x[n + n // 3] = np.nan
        x[6 * n + n // 4] = np.inf
    return x.astype(np.float32)


def curve(L, T, k, W):
    d = L - T
    if 2.0 * d <= -W:
        return 0.0
    if 2.0 * d < W:
        return k * (d + W / 2.0) * (d + W / 2.0) / (2.0 * W)
    return k * d


class Serial:
    """one stream through the setting at `rate` Hz, frame by frame: `frame(x)` returns (y float64, not yet rounded; s)"""

    def __init__(self, setting, rate):
        self.T, R, self.W, attack, release, self.M = parse(setting)
        self.k = 1.0 - 1.0 / R
        self.aA = math.exp(-1.0 / (attack * rate / 1000.0))
        self.aR = math.exp(-1.0 / (release * rate / 1000.0))
        self.p = self.s = 0.0

    def frame(self, x):
        x = np.asarray(x, dtype=np.float64)
        y, ss = np.empty_like(x), np.empty_like(x)
        p, s = self.p, self.s
        for i in range(x.shape[0]):
            xi = float(x[i])
            a = abs(xi)
            a = a if a > 1e-6 else 1e-6
            a = a if a < 1e6 else 1e6
            c = curve(math.log(a) / K, self.T, self.k, self.W)
            q = self.aR * p
            p = c if c > q else q
            s = self.aA * s + (1.0 - self.aA) * p
            ss[i] = s
            y[i] = math.exp((self.M - s) * K) * xi
        self.p, self.s = p, s
        return y, ss


class Chunked:
    """the same stream by the kernel's scheme: THREADS chunks of ceil(n / THREADS) samples, each run from 0 (the first from
    the carried state), the chunk ends combined in log steps with the powers exp(-chunk 2^j / tau), each chunk re-run from
    its true start.  `frame(x)` returns (y, s) as `Serial.frame` does"""

    THREADS = 1024

    def __init__(self, setting, rate):
        self.T, R, self.W, attack, release, self.M = parse(setting)
        self.k = 1.0 - 1.0 / R
        self.tau_a, self.tau_r = attack * rate / 1000.0, release * rate / 1000.0
        self.aA, self.aR = math.exp(-1.0 / self.tau_a), math.exp(-1.0 / self.tau_r)
        self.p = self.s = 0.0

    def _scan(self, v, carry, step, combine, tau, chunk):
        """v [nT, chunk] (NaN behind the frame's end): the recurrence `step(value, state)` over every chunk; returns the
        values of every sample and the state after the last one"""
        nT = v.shape[0]
        live = ~np.isnan(v)
        a = np.zeros(nT)
        a[0] = carry
        for q in range(chunk):
            a = np.where(live[:, q], step(v[:, q], a), a)
        j = 0
        while (1 << j) < nT:
            off, pw = 1 << j, math.exp(-(chunk << j) / tau)
            nxt = a.copy()
            nxt[off:] = combine(a[off:], pw * a[:-off])
            a, j = nxt, j + 1
        start = np.concatenate([[carry], a[:-1]])
        out = np.full(v.shape, np.nan)
        for q in range(chunk):
            start = np.where(live[:, q], step(v[:, q], start), start)
            out[:, q] = np.where(live[:, q], start, np.nan)
        return out, float(start[-1])

    def frame(self, x):
        x = np.asarray(x, dtype=np.float64)
        n = x.shape[0]
        chunk = -(-n // self.THREADS)
        nT = -(-n // chunk)
        with np.errstate(invalid="ignore"):
            a = np.abs(x)
            a = np.where(a > 1e-6, a, 1e-6)
            a = np.where(a < 1e6, a, 1e6)
        c = np.array([curve(math.log(v) / K, self.T, self.k, self.W) for v in a])
        grid = np.full(nT * chunk, np.nan)
        grid[:n] = c
        aA, aR = self.aA, self.aR
        with np.errstate(invalid="ignore"):
            p, self.p = self._scan(grid.reshape(nT, chunk), self.p, lambda c_, s_: np.where(c_ > aR * s_, c_, aR * s_),
                                   lambda e_, d_: np.where(e_ > d_, e_, d_), self.tau_r, chunk)
            s, self.s = self._scan(p, self.s, lambda p_, s_: aA * s_ + (1.0 - aA) * p_, lambda e_, d_: e_ + d_, self.tau_a,
                                   chunk)
        s = s.reshape(-1)[:n]
        return np.exp((self.M - s) * K) * x, s


def reference(setting, rate, x, n=None):
    """the whole signal x through `Serial`, in frames of n samples (None: at once): (y float64, s)"""
    st = Serial(setting, rate)
    x = np.asarray(x)
    n = x.shape[0] if n is None else n
    parts = [st.frame(x[i:i + n]) for i in range(0, x.shape[0], n)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
