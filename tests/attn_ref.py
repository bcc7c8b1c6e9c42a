"""float64 reference of ONE attention launch of the hot path (attn_kernel / attn_decode_kernel / attn_decode2_kernel /
attn_cascade_kernel + attn_combine_kernel, ptts_kernels.h), on the fp32 operands the kernel consumed (Engine.debug_attn):

    y[b][t][h] = sum_p softmax_p(q[b][t][h] . K[b][p][h] / 8) V[b][p][h],
    over the keys p with pos_k(p) >= 0 and 0 <= pos_q - pos_k(p) < context (reference transformer.py:22-29)

The scale 1/8 = 1/sqrt(64) is a power of two, so the kernel's scaled query is exact in fp32: kernel and reference differ
only by fp32 rounding in the dot products, the exponentials and the sums.  NumPy, host only."""

from __future__ import annotations

import numpy as np

F64 = np.float64


def histories(k, v, pk=None, pv=None, pre_len=None, pre_id=None):
    """[B][T][H][64] float64 key / value histories of the rows: position p of row b is pk / pv[pre_id[b]][p] when row b
    has a prefix and p < its length (the shared voice prefix), else k / v[b][p]"""
    K, V = np.array(k, dtype=F64), np.array(v, dtype=F64)
    if pk is not None:
        for b, j in enumerate(pre_id):
            if j >= 0 and pre_len[j] > 0:
                K[b, : pre_len[j]] = pk[j, : pre_len[j]]
                V[b, : pre_len[j]] = pv[j, : pre_len[j]]
    return K, V


def attend(q, K, V, pos_q, pos_k, context=0):
    """one row: q [Tq][H][64], K / V [S][H][64] (S key slots), pos_q [Tq], pos_k [S] (< 0: an empty slot).
    Returns y [Tq][H][64], the score scale s1 [Tq][H] = max over attended keys of sum_e |q_e k_e| / 8 and the value
    magnitude vmax [Tq][H] = max over attended keys of max_e |v_e|."""
    q, K, V = (np.asarray(x, dtype=F64) for x in (q, K, V))
    delta = np.asarray(pos_q)[:, None] - np.asarray(pos_k)[None, :]
    mask = (np.asarray(pos_k)[None, :] >= 0) & (delta >= 0)
    if context and context > 0:
        mask &= delta < context
    assert mask.any(axis=1).all(), "a query without keys"
    s = np.einsum("thd,khd->htk", q, K) / 8.0
    s = np.where(mask[None], s, -np.inf)
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    p /= p.sum(axis=-1, keepdims=True)
    y = np.einsum("htk,khd->thd", p, V)
    s1 = np.einsum("thd,khd->htk", np.abs(q), np.abs(K)) / 8.0
    s1 = np.where(mask[None], s1, 0.0).max(axis=-1).T
    va = np.abs(V).max(axis=-1).T  # [H][S]
    vmax = np.where(mask[None], va[:, None, :], 0.0).max(axis=-1).T
    return y, s1, vmax


def attn_ref(q, K, V, offset, context=0):
    """q [B][Tq][H][64], histories K / V [B][T][H][64] (histories()), offset [B] = position of each row's first query.
    Returns y [B][Tq][H * 64], s1 [B][Tq][H], vmax [B][Tq][H] (see attend)."""
    q = np.asarray(q, dtype=F64)
    B, Tq, H, _ = q.shape
    T = K.shape[1]
    y = np.empty((B, Tq, H, 64))
    s1 = np.empty((B, Tq, H))
    vmax = np.empty((B, Tq, H))
    for b in range(B):
        off = int(offset[b])
        n = off + Tq  # keys after the last query are never attended
        assert n <= T, "a row's queries lie past its history"
        lo = max(0, off - context + 1) if context and context > 0 else 0
        y[b], s1[b], vmax[b] = attend(q[b], K[b, lo:n], V[b, lo:n], off + np.arange(Tq), np.arange(lo, n), context)
    return y.reshape(B, Tq, H * 64), s1, vmax


def bound(s1, vmax, tol=2.0 ** -18):
    """the per-(row, query, head) error bound of the fp32 kernels: tol * max|v| * (1 + S), S = s1 (see
    tests/test_gpu_attn_matrix.py)"""
    return tol * vmax * (1.0 + s1)


def bf16_round(x):
    """fp32 -> bf16 round-to-nearest-even, as float64 (the h16 output's rounding, via float32 bit patterns)"""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).astype(F64)


def bf16_ulp(x):
    """the spacing of bf16 numbers at |x| (8 significant bits)"""
    x = np.abs(np.asarray(x, dtype=F64))
    e = np.floor(np.log2(np.maximum(x, 2.0 ** -126)))
    return 2.0 ** (e - 7)
