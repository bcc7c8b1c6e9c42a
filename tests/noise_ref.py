"""numpy restatement of the FlowLM step's device noise generator (ptts_kernels.h: mix64, counter_normal,
counter_trunc_normal): the draws of row m, column k at step counter `ctr` use idx = m * ldim + k."""

import math

import numpy as np

_M = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _hash(seed: int, ctr: int, idx):
    idx = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        key = (np.uint64(ctr) << np.uint64(32)) | idx
        return _mix64(np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * key)


def counter_normal(seed: int, ctr: int, idx) -> np.ndarray:
    """N(0, 1) by Box-Muller on two 24-bit uniforms of the splitmix64 hash (float64 evaluation of the fp32 kernel)"""
    z = _hash(seed, ctr, idx)
    u1 = (((z >> np.uint64(40)) & np.uint64(0xFFFFFF)).astype(np.float64) + 1.0) / 16777216.0
    u2 = ((z >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.float64) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def trunc_params(temp: float, clamp: float):
    """(std, lo, width) as ptts_lm_state_set_row_sampling stores them (fp32): u in [2l - 1, 2h - 1] = [-a, a]"""
    sd = np.float32(math.sqrt(np.float32(temp)))
    a = np.float32(math.erf(float(np.float32(clamp)) / (float(sd) * math.sqrt(2.0))))
    return sd, np.float32(-a), np.float32(2.0 * a)


def counter_trunc_normal(seed: int, ctr: int, idx, temp: float, clamp: float) -> np.ndarray:
    """truncated N(0, temp) on [-clamp, clamp] by the inverse CDF (torch.nn.init.trunc_normal_), in float64 after the
    fp32 uniform the kernel forms"""
    from scipy.special import erfinv

    sd, lo, width = trunc_params(temp, clamp)
    z = _hash(seed, ctr, idx)
    u01 = (2.0 * (z >> np.uint64(41)).astype(np.float64) + 1.0) / 16777216.0
    u = (float(width) * u01 + float(lo)).astype(np.float32).astype(np.float64)
    return np.clip(float(sd) * math.sqrt(2.0) * erfinv(u), -clamp, clamp)


def row_noise(seed: int, ctr: int, row: int, ldim: int, temp: float, clamp: float | None = None) -> np.ndarray:
    """the LSD start point of one row at one step"""
    idx = row * ldim + np.arange(ldim)
    if temp == 0:
        return np.zeros(ldim)
    if clamp is not None and clamp > 0:
        return counter_trunc_normal(seed, ctr, idx, temp, clamp)
    return float(np.float32(math.sqrt(np.float32(temp)))) * counter_normal(seed, ctr, idx)
