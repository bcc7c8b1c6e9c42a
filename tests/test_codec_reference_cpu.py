"""Pins tests/codec_ref.py (the float64 reference of the reduced-precision codec's GEMMs) against independent
formulations: torch conv1d / conv_transpose1d streamed over two frames, layer_norm + linear, complex-number RoPE, the
OCP e4m3 grid, and the numpy oracle's bf16 model helpers."""

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from codec_ref import (E4M3_MAX, EPI_CONVTR, EPI_QKV, EPI_RES, EPI_STORE, PRE_LNFOLD, codec_gemm_ref, convtr_weight, e4m3,
                       e4m3_grid, e4m3_neighbours, layer_stats, pcm_ref, quant_weight_f8, rope_apply)
from gemm_ref import ACT_ELU, ACT_GELU, ACT_NONE, bf16_round

F64 = torch.float64


def rn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


@pytest.mark.parametrize("k,halo", [(7, 6), (3, 2), (3, 0), (3, 1), (1, 0)])
def test_streamed_conv1d(k, halo):
    """two frames of B sequences: the reference over the second frame (x_prev = the first) equals conv1d over both frames
    with left padding, for the causal halo; a smaller halo shifts the window right (rows past the end are zero)"""
    B, T, C, N = 3, 16, 32, 8
    f0, f1, w, b = rn(B, T, C, seed=1), rn(B, T, C, seed=2), rn(N, C, k, seed=3), rn(N, seed=4)
    full = torch.cat((f0, f1), dim=1).transpose(1, 2)  # [B][C][2T]
    ypad = F.conv1d(F.pad(full, (halo, k)), w, b)  # output t reads input rows t - halo .. t - halo + k - 1
    want = ypad[:, :, T:2 * T].transpose(1, 2).reshape(B * T, N)
    if halo < k - 1:  # the hook's rows past a sequence's end belong to the NEXT sequence of x (zero after the last)
        x_next = torch.cat((f1[1:], torch.zeros(1, T, C, dtype=F64)))
        full2 = torch.cat((f0, f1, x_next), dim=1).transpose(1, 2)
        want = F.conv1d(F.pad(full2, (halo, 0)), w, b)[:, :, T:2 * T].transpose(1, 2).reshape(B * T, N)
    w_eff = w.permute(0, 2, 1).reshape(N, k * C)
    _, y, scale = codec_gemm_ref(f1.reshape(B * T, C), w_eff, M=B * T, ntaps=k, T=T, halo=halo,
                                 xp_eff=f0.reshape(B * T, C), bias=b)
    torch.testing.assert_close(y, want, rtol=1e-12, atol=1e-12)
    assert (scale >= y.abs() - 1e-12).all()


@pytest.mark.parametrize("stride,cout", [(6, 32), (5, 64), (4, 32)])
def test_streamed_conv_transpose(stride, cout):
    """mode-1 packing + CONVTR interleave over the second of two frames == conv_transpose1d over both frames"""
    B, T, C = 2, 16, 64
    f0, f1 = rn(B, T, C, seed=5), rn(B, T, C, seed=6)
    w, b = rn(C, cout, 2 * stride, seed=7), rn(cout, seed=8)
    full = torch.cat((f0, f1), dim=1).transpose(1, 2)
    ct = F.conv_transpose1d(full, w, b, stride=stride)  # [B][cout][(2T - 1) s + 2 s]
    want = ct[:, :, T * stride:2 * T * stride].transpose(1, 2).reshape(B * T * stride, cout)
    _, y, _ = codec_gemm_ref(f1.reshape(B * T, C), convtr_weight(w, stride), M=B * T, ntaps=2, T=T, halo=1,
                             xp_eff=f0.reshape(B * T, C), bias=b, epi=EPI_CONVTR, stride=stride)
    torch.testing.assert_close(y, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("mean", [0.0, 4.0, 30.0])
def test_lnfold_equals_layer_norm(mean):
    M, C, N = 32, 64, 48
    x, w, b = rn(M, C, seed=9) + mean, rn(N, C, seed=10) / 8, rn(N, seed=11)
    g, beta = 1 + rn(C, seed=12) / 5, rn(C, seed=13) / 10
    want = F.linear(F.layer_norm(x, (C,), g, beta, eps=1e-5), w, b)
    wp = w * g
    _, y, scale = codec_gemm_ref(x, wp, M=M, pre=PRE_LNFOLD, ln_s=wp.sum(1), ln_c=w @ beta + b)
    torch.testing.assert_close(y, want, rtol=1e-9, atol=1e-9)
    mu, var, dmu, dvar = layer_stats(x)
    # the statistics bound grows with (E[x^2] + mu^2) / var, i.e. with the row mean
    ratio = (dvar / (var * (C / 4 + 5) * 2.0 ** -24)).mean().item()
    assert ratio == pytest.approx(1 + 2 * mean ** 2, rel=0.5)


def test_lnfold_matches_oracle_bf16_model():
    from oracle.np_oracle import bf16_round as np_bf16, lnfold_linear_bf16

    M, C, N = 16, 64, 32
    x = bf16_round(rn(M, C, seed=14).float()).numpy().astype(np.float32)
    w = (rn(N, C, seed=15) / 8).float().numpy()
    g, beta, bias = (1 + rn(C, seed=16) / 5).float().numpy(), (rn(C, seed=17) / 10).float().numpy(), rn(N, seed=18).float().numpy()
    want = lnfold_linear_bf16(x, w, g, beta, bias, 1e-5)
    wr = torch.from_numpy(np_bf16(w * g[None, :]))
    _, y, scale = codec_gemm_ref(torch.from_numpy(x), wr, M=M, pre=PRE_LNFOLD, ln_s=wr.double().sum(1),
                                 ln_c=torch.from_numpy((w @ beta + bias).astype(np.float32)))
    assert ((y - torch.from_numpy(want).double()).abs() <= 2.0 ** -18 * scale + 1e-6).all()


def test_bf16_round_matches_oracle():
    from oracle.np_oracle import bf16_round as np_bf16

    v = torch.cat((rn(4096, seed=19).float() * 100, torch.tensor([1 + 2 ** -8, 1 + 3 * 2 ** -8, -0.0, 3.0e38])))
    assert torch.equal(bf16_round(v), torch.from_numpy(np_bf16(v.numpy())).double())


def test_rope_matches_complex_rotation():
    M, H = 8, 2
    v = rn(M, H * 64, seed=20)
    ang = rn(M, 32, seed=21)
    tab = torch.stack((torch.cos(ang), torch.sin(ang)), -1)
    z = torch.view_as_complex(v.reshape(M, H, 32, 2).contiguous()) * torch.polar(torch.ones_like(ang), ang)[:, None, :]
    torch.testing.assert_close(rope_apply(v, tab, H), torch.view_as_real(z).reshape(M, H * 64))
    # QKV: q and k rotated, v not
    x, w = rn(M, 64, seed=22), rn(3 * H * 64, 64, seed=23)
    _, y, _ = codec_gemm_ref(x, w, M=M, epi=EPI_QKV, rope=tab, H=H)
    plain = x @ w.T
    D = H * 64
    torch.testing.assert_close(y[:, :D], rope_apply(plain[:, :D], tab, H))
    torch.testing.assert_close(y[:, D:2 * D], rope_apply(plain[:, D:2 * D], tab, H))
    torch.testing.assert_close(y[:, 2 * D:], plain[:, 2 * D:])


def test_e4m3_grid_and_rounding():
    g = e4m3_grid()
    assert len(g) == 253 and g.max() == E4M3_MAX and g.min() == -E4M3_MAX  # 256 codes - 2 NaN - (-0)
    assert g[g > 0].min() == 2.0 ** -9  # smallest subnormal
    v = torch.tensor([500.0, -1e9, 0.0, 2.0 ** -9 * 0.49, 2.0 ** -9 * 0.51, 1.0625, 1.1875, 17.0])
    assert e4m3(v).tolist() == [448.0, -448.0, 0.0, 0.0, 2.0 ** -9, 1.0, 1.25, 16.0]  # ties to even
    x = rn(10000, seed=24) * 100
    lo, hi = e4m3_neighbours(x)
    q = e4m3(x)
    assert ((q == lo) | (q == hi)).all() and (lo <= x.clamp(-448, 448)).all() and (hi >= x.clamp(-448, 448)).all()


def test_quant_weight_f8():
    w = torch.cat((rn(4, 64, seed=25), torch.zeros(1, 64)))
    w[0, 3] = 7.0
    deq, scale = quant_weight_f8(w)
    assert scale[0].item() == np.float32(7.0) / np.float32(448.0)
    assert scale[4].item() == 1.0 and (deq[4] == 0).all()
    assert deq[0, 3].item() == pytest.approx(7.0, rel=2 ** -20)
    assert ((deq - w).abs() <= 2 ** -4 * w.abs() + 2 ** -9 * scale[:, None]).all()


def test_pcm_ref_and_residual():
    M, T, C = 32, 16, 64
    x, xp, w, b = rn(M, C, seed=26), rn(M, C, seed=27), rn(1, C, 3, seed=28) / 4, rn(1, seed=29)
    y, scale, i16 = pcm_ref(x, w, M=M, T=T, halo=2, xp_eff=xp, bias=b)
    want = F.conv1d(F.pad(torch.cat((xp.reshape(2, T, C), x.reshape(2, T, C)), 1).transpose(1, 2), (2, 0)), w, b)
    torch.testing.assert_close(y, want[:, 0, T:2 * T].reshape(M))
    assert (i16.abs() <= 32767).all() and (i16 == torch.trunc(y.clamp(-1, 1) * 32767)).all()
    r, ls = rn(M, 32, seed=30), rn(32, seed=31)
    w2 = rn(32, C, seed=32)
    pre, y2, _ = codec_gemm_ref(x, w2, M=M, epi=EPI_RES, r=r, ls=ls, act=ACT_ELU)
    torch.testing.assert_close(pre, (x @ w2.T) * ls)
    torch.testing.assert_close(y2, F.elu(bf16_round(r) + pre))
    _, y3, _ = codec_gemm_ref(x, w2, M=M, epi=EPI_STORE, act=ACT_GELU)
    torch.testing.assert_close(y3, F.gelu(x @ w2.T))
    assert ACT_NONE == 0 and math.isfinite(scale.sum().item())
