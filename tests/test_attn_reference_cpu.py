"""Pins tests/attn_ref.py (the float64 reference of tests/test_gpu_attn_matrix.py) against torch's float64
scaled_dot_product_attention with an explicit boolean mask (the reference model's mask: pos_k >= 0, 0 <= delta < context),
against a ring-buffer arrangement of the same keys, and against the numpy oracle's attention_core."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from attn_ref import attend, attn_ref, bf16_round, bf16_ulp, bound, histories
from oracle import np_oracle as O


def rnd(*shape, seed=0, scale=1.0):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape) * scale


def sdpa(q, K, V, pos_q, pos_k, context):
    """torch float64 SDPA of one row with the reference model's mask (transformer.py:22-29)"""
    delta = pos_q[:, None] - pos_k[None, :]
    mask = (pos_k[None, :] >= 0) & (delta >= 0)
    if context:
        mask = mask & (delta < context)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).permute(1, 0, 2)[None]  # [1][H][L][64]
    y = F.scaled_dot_product_attention(t(q), t(K), t(V), attn_mask=torch.from_numpy(mask)[None, None], scale=0.125)
    return y[0].permute(1, 0, 2).numpy()


@pytest.mark.parametrize("Tq,off,context", [(1, 0, 0), (1, 37, 0), (7, 16, 0), (17, 31, 0), (16, 300, 250), (1, 260, 250),
                                            (39, 5, 20), (40, 0, 16)])
def test_matches_sdpa(Tq, off, context):
    B, H, T = 2, 3, off + Tq + 5
    q, k, v = rnd(B, Tq, H, 64, seed=1), rnd(B, T, H, 64, seed=2), rnd(B, T, H, 64, seed=3)
    offs = [off, max(0, off - 3)]
    y, s1, vmax = attn_ref(q, k, v, offs, context)
    for b in range(B):
        want = sdpa(q[b], k[b], v[b], offs[b] + np.arange(Tq), np.arange(T), context)
        np.testing.assert_allclose(y[b].reshape(Tq, H, 64), want, rtol=1e-12, atol=1e-12)
    # the bound's ingredients are the attended keys' magnitudes
    assert (s1 > 0).all() and (vmax <= 1.0).all() and (vmax > 0.5).all()
    assert (bound(s1, vmax) > 0).all()


@pytest.mark.parametrize("frame_off", [0, 16, 256, 272, 288, 1600])
def test_ring_arrangement_matches_history(frame_off):
    """a codec frame (16 queries) on a ring of 272 slots, context 250: the slots hold the newest position of their class
    (never-written slots position -1), which is the history's last 265 keys"""
    ring, Tq, H, context = 272, 16, 2, 250
    T = frame_off + Tq
    q, k, v = rnd(1, Tq, H, 64, seed=4), rnd(1, T, H, 64, seed=5), rnd(1, T, H, 64, seed=6)
    y, _, _ = attn_ref(q, k, v, [frame_off], context)
    top = frame_off + Tq - 1
    pos_k = np.array([top - ((top - s) % ring) for s in range(ring)])
    Kr, Vr = np.zeros((ring, H, 64)), np.zeros((ring, H, 64))
    ok = pos_k >= 0
    Kr[ok], Vr[ok] = k[0, pos_k[ok]], v[0, pos_k[ok]]
    pos_k[~ok] = -1
    yr, _, _ = attend(q[0], Kr, Vr, frame_off + np.arange(Tq), pos_k, context)
    np.testing.assert_allclose(y[0].reshape(Tq, H, 64), yr, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(yr, sdpa(q[0], Kr, Vr, frame_off + np.arange(Tq), pos_k, context), rtol=1e-12, atol=1e-12)


def test_prefix_substitution():
    """rows that borrow a prefix see its keys below its length and their own above"""
    B, T, H = 3, 50, 2
    k, v = rnd(B, T, H, 64, seed=7), rnd(B, T, H, 64, seed=8)
    pk, pv = rnd(2, 40, H, 64, seed=9), rnd(2, 40, H, 64, seed=10)
    K, V = histories(k, v, pk, pv, [33, 16], [1, -1, 0])
    np.testing.assert_array_equal(K[0, :16], pk[1, :16])
    np.testing.assert_array_equal(K[0, 16:], k[0, 16:])
    np.testing.assert_array_equal(K[1], k[1])
    np.testing.assert_array_equal(V[2, :33], pv[0, :33])
    np.testing.assert_array_equal(V[2, 33:], v[2, 33:])


@pytest.mark.parametrize("scale", [1.0, 100.0])
def test_large_scores_and_equal_scores(scale):
    """|s| ~ 100 overflows exp without the running max; all-equal scores give the values' mean"""
    Tq, H, T = 4, 2, 40
    q = rnd(1, Tq, H, 64, seed=11) * np.sqrt(8 * scale / 64) * 2
    k = rnd(1, T, H, 64, seed=12) * np.sqrt(8 * scale / 64) * 2
    v = rnd(1, T, H, 64, seed=13, scale=1e3)
    y, _, _ = attn_ref(q, k, v, [T - Tq])
    assert np.isfinite(y).all()
    want = sdpa(q[0], k[0], v[0], T - Tq + np.arange(Tq), np.arange(T), 0)
    np.testing.assert_allclose(y[0].reshape(Tq, H, 64), want, rtol=1e-10, atol=1e-9)
    y, _, _ = attn_ref(np.ones((1, 1, H, 64)), np.ones((1, T, H, 64)), v, [T - 1])
    np.testing.assert_allclose(y[0, 0].reshape(H, 64), v[0].mean(axis=0), rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("T,off,context", [(1, 0, None), (5, 0, None), (3, 20, None), (16, 40, 30), (9, 7, 8)])
def test_matches_oracle_attention_core(T, off, context):
    """the oracle's fp32 attention_core (RoPE applied to q and k first, then the cache write): attn_ref on the same
    rotated operands agrees to fp32 rounding"""
    B, H = 2, 2
    C = 64 * H
    proj = rnd(B, T, 3 * C, seed=14).astype(np.float32)
    cache = np.full((2, B, off + T + 3, H, 64), np.nan, np.float32)
    cache[:, :, :off] = rnd(2, B, off, H, 64, seed=15).astype(np.float32)
    state = {"offset": off, "cache": cache.copy()}
    got = O.attention_core(proj, state, H, context, 10000.0)
    p = proj.reshape(B, T, 3, H, 64)
    q, k = O.apply_rope(p[:, :, 0], p[:, :, 1], off, 10000.0)
    kh = np.concatenate([cache[0, :, :off], k], axis=1)
    vh = np.concatenate([cache[1, :, :off], p[:, :, 2]], axis=1)
    y, _, _ = attn_ref(q, kh, vh, [off] * B, context or 0)
    np.testing.assert_allclose(np.asarray(got).reshape(B, T, C), y, rtol=0, atol=2e-6)


def test_bf16_helpers():
    x = np.array([1.0, 1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, -3.14159, 1e3], np.float32)
    r = bf16_round(x)
    np.testing.assert_array_equal(r, torch.from_numpy(x).to(torch.bfloat16).double().numpy())
    np.testing.assert_array_equal(bf16_ulp([1.0, 1.5, 2.0, 1e3]), [2 ** -7, 2 ** -7, 2 ** -6, 2 ** 2])
