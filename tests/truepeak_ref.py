"""float64 restatement of the leveler's true-peak mode (pocket_tts_amd/level.py, "True-peak mode"), for the tests: the whole
signal at once, serial, every operation in float64, fed the fp32 G, C, a, k of a row and its plan and the fp32 taps.  Also the
test signals of the property the mode is for, and a 16x meter to say what the 4x one under-reads."""

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

D, T = 10, 21


def fir(u, taps):
    """v[p][i] = sum over j of taps[p][j] u[i - j] in ascending j, u = 0 before the start: [3, len(u)].  A NaN in u reaches the
    21 values whose window holds it and no other"""
    u = np.asarray(u, np.float64)
    taps = np.asarray(taps, np.float64)
    up = np.concatenate([np.zeros(T - 1), u])
    v = np.zeros((taps.shape[0], len(u)))
    for j in range(T):
        v += taps[:, j:j + 1] * up[T - 1 - j:T - 1 - j + len(u)][None, :]
    return v


def detector(u, taps):
    """P[i] = fmax(|u[i - 10]|, |v_1[i]|, |v_2[i]|, |v_3[i]|)"""
    u = np.asarray(u, np.float64)
    centre = np.abs(np.concatenate([np.zeros(D), u])[:len(u)])
    return np.fmax(centre, np.fmax.reduce(np.abs(fir(u, taps)), axis=0))


def meter(y, taps):
    """M after the samples y: the largest P of y, NaN skipped; 0.0 for none"""
    if len(y) == 0:
        return 0.0
    return float(np.fmax.reduce(detector(y, taps), initial=0.0))


def limiter(r, LA, a, k):
    """g of level.py from r: m, d, e and the box average, r = e = 1 before the stream's start"""
    m = sliding_window_view(np.concatenate([np.ones(LA), r]), LA + 1).min(axis=1)
    c = 1.0 - m
    d = np.empty(len(r))
    prev = 0.0
    for i in range(len(r)):
        prev = max(c[i], a * prev)
        d[i] = prev
    e = 1.0 - d
    return k * sliding_window_view(np.concatenate([np.ones(LA - 1), e]), LA).sum(axis=1)


def level_tp(x, G, C, LA, a, k, taps, full=False):
    """y of the whole stream x in true-peak mode (y[i] = g[i] u[i - 10 - LA]); with `full` also (u, P, r, g, M), M the meter
    after len(x) samples"""
    G, C, a, k = float(G), float(C), float(a), float(k)
    u = G * np.asarray(x, np.float64)
    P = detector(u, taps)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(P > C, C / P, 1.0)  # a NaN compares false
    g = limiter(r, LA, a, k)
    y = g * np.concatenate([np.zeros(LA + D), u])[:len(u)]
    return (y, u, P, r, g, meter(y, taps)) if full else y


def level_sp(x, G, C, LA, a, k):
    """the sample-peak mode of level.py on the same limiter, for the comparison of the two: y[i] = g[i] u[i - LA]"""
    G, C, a, k = float(G), float(C), float(a), float(k)
    u = G * np.asarray(x, np.float64)
    au = np.abs(u)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(au > C, C / au, 1.0)
    return limiter(r, LA, a, k) * np.concatenate([np.zeros(LA), u])[:len(u)]


def meter_16x(y):
    """the same reading through a 16x interpolator of the same family (`resample.prototype(16, 1)`), in float64"""
    from pocket_tts_amd import resample

    h = resample.prototype(16, 1)
    y = np.asarray(y, np.float64)
    return float(max(np.abs(np.convolve(y, h[p::16])).max() for p in range(16)))


# ---- the inputs of the property test: `n` samples of float32, a quarter second of lead-out of zeros behind them ------------
def sine(n):
    """fs / 4 at 45 degrees, amplitude 0.5: every sample is 0.354, the waveform between them reaches 0.5"""
    return (0.5 * np.sin(0.5 * np.pi * np.arange(n) + 0.25 * np.pi)).astype(np.float32)


def sweep(n):
    """a linear sweep from 0.2 fs to 0.25 fs, amplitude 0.5"""
    t = np.arange(n) / n
    return (0.5 * np.sin(2 * np.pi * n * (0.2 * t + 0.025 * t * t) + 0.3)).astype(np.float32)


def noise(n, seed=7):
    return (0.3 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def pulses(n, rate, seed=11):
    """a pulse train at about 120 Hz with jitter through three two-pole formants (700, 1200 and 2600 Hz), peak 0.5"""
    rng = np.random.default_rng(seed)
    x = np.zeros(n)
    i = 0
    while i < n:
        x[i] = 1.0
        i += int(rate / 120 * (1 + 0.04 * rng.standard_normal()))
    y = np.zeros(n)
    for f0, bw, gain in ((700, 90, 1.0), (1200, 110, 0.7), (2600, 160, 0.4)):
        rad = np.exp(-np.pi * bw / rate)
        a1, a2 = -2 * rad * np.cos(2 * np.pi * f0 / rate), rad * rad
        s = np.zeros(n)
        for j in range(n):
            s[j] = x[j] - a1 * (s[j - 1] if j >= 1 else 0.0) - a2 * (s[j - 2] if j >= 2 else 0.0)
        y += gain * s
    return (0.5 * y / np.abs(y).max()).astype(np.float32)


PROPERTY_INPUTS = ("sine", "sweep", "noise", "pulses")


def property_input(name, rate, n):
    return {"sine": sine, "sweep": sweep, "noise": noise, "pulses": lambda m: pulses(m, rate)}[name](n)
