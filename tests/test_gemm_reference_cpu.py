"""Pins tests/gemm_ref.py (the float64 reference of tests/test_gpu_gemm_matrix.py) against torch's own float64 Linear,
Conv1d and LayerNorm, and against the numpy oracle's rounding models of the int8 and bf16 weight formats."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gemm_ref import (ACT_ELU, ACT_GELU, ACT_NONE, ACT_SILU, EPI_GATE, EPI_RES, EPI_STORE, PRE_ADDSILU, PRE_ELU,
                      PRE_LNFOLD, PRE_LNMOD, bf16_round, gemm_ref)
from oracle import np_oracle as O

D = torch.float64


def rnd(*shape, seed=0, mean=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=D) + mean


@pytest.mark.parametrize("act", [ACT_NONE, ACT_GELU, ACT_SILU, ACT_ELU])
def test_linear_matches_torch(act):
    x, w, b = rnd(37, 48, seed=1), rnd(24, 48, seed=2), rnd(24, seed=3)
    y, scale = gemm_ref(x, w, M=37, bias=b, act=act)
    z = F.linear(x, w, b)
    want = {ACT_NONE: z, ACT_GELU: F.gelu(z), ACT_SILU: F.silu(z), ACT_ELU: F.elu(z)}[act]
    torch.testing.assert_close(y, want, rtol=1e-12, atol=1e-12)
    assert torch.allclose(scale, x.abs() @ w.abs().T + b.abs())


def test_prologues_and_epilogues_match_torch():
    x, w, b = rnd(20, 32, seed=4), rnd(16, 32, seed=5), rnd(16, seed=6)
    r, g, ls, pv = rnd(20, 16, seed=7), rnd(20, 16, seed=8), rnd(16, seed=9), rnd(32, seed=10)
    y, _ = gemm_ref(x, w, M=20, bias=b, pre=PRE_ELU)
    torch.testing.assert_close(y, F.linear(F.elu(x), w, b), rtol=1e-12, atol=1e-12)
    y, _ = gemm_ref(x, w, M=20, bias=b, pre=PRE_ADDSILU, prevec=pv)
    torch.testing.assert_close(y, F.linear(F.silu(x + pv), w, b), rtol=1e-12, atol=1e-12)
    lw, lb, sh, sc = rnd(32, seed=11), rnd(32, seed=12), rnd(20, 32, seed=13), rnd(20, 32, seed=14)
    y, _ = gemm_ref(x, w, M=20, bias=b, pre=PRE_LNMOD, lnm_w=lw, lnm_b=lb, mod_shift=sh, mod_scale=sc)
    xm = F.layer_norm(x, (32,), lw, lb, eps=1e-5) * (1 + sc) + sh
    torch.testing.assert_close(y, F.linear(xm, w, b), rtol=1e-12, atol=1e-12)
    y, _ = gemm_ref(x, w, M=20, bias=b, epi=EPI_RES, r=r, ls=ls, act=ACT_GELU)
    torch.testing.assert_close(y, F.gelu(r + ls * F.linear(x, w, b)), rtol=1e-12, atol=1e-12)
    y, _ = gemm_ref(x, w, M=20, bias=b, epi=EPI_GATE, r=r, g=g)
    torch.testing.assert_close(y, r + g * F.linear(x, w, b), rtol=1e-12, atol=1e-12)
    rows = torch.tensor([0, 7, 19])
    y2, _ = gemm_ref(x, w, M=20, bias=b, epi=EPI_GATE, r=r, g=g, rows=rows)
    torch.testing.assert_close(y2, y[rows], rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("mean", [0.0, 3.0])
def test_lnfold_matches_layer_norm(mean):
    """the fold (sum x w' - s mu) rs + c with w' = W diag(g), s = sum_k w', c = W beta + bias is LayerNorm + Linear"""
    x = rnd(9, 64, seed=20, mean=mean)
    w, gam, bet, b = rnd(32, 64, seed=21), rnd(64, seed=22), rnd(64, seed=23), rnd(32, seed=24)
    wp = w * gam
    y, scale = gemm_ref(x, wp, M=9, pre=PRE_LNFOLD, ln_s=wp.sum(1), ln_c=w @ bet + b)
    torch.testing.assert_close(y, F.linear(F.layer_norm(x, (64,), gam, bet, eps=1e-5), w, b), rtol=1e-10, atol=1e-10)
    assert (scale >= y.abs() - (w @ bet + b).abs() - 1e-9).all()


def conv_torch(x, xp, w, b, T, xstride, halo, halo_mode):
    """torch.nn.functional.conv1d of each sequence, its `halo` left-context rows from xp / zeros / its first row"""
    B = x.shape[0] // (T * xstride)
    out = []
    for s in range(B):
        seq = x[s * T * xstride:(s + 1) * T * xstride]
        if halo_mode == 0:
            left = xp[(s + 1) * T * xstride - halo:(s + 1) * T * xstride]
        elif halo_mode == 1:
            left = torch.zeros(halo, x.shape[1], dtype=D)
        else:
            left = seq[:1].expand(halo, -1)
        full = torch.cat([left, seq]).T[None]
        out.append(F.conv1d(full, w, b, stride=xstride)[0].T[:T])
    return torch.cat(out)


@pytest.mark.parametrize("halo_mode", [0, 1, 2])
@pytest.mark.parametrize("ntaps,xstride,T,B", [(3, 1, 16, 1), (7, 1, 32, 3), (4, 2, 16, 2)])
def test_conv_matches_conv1d(halo_mode, ntaps, xstride, T, B):
    C, N = 32, 24
    halo = ntaps - xstride
    x, xp = rnd(B * T * xstride, C, seed=30), rnd(B * T * xstride, C, seed=31)
    w, b = rnd(N, C, ntaps, seed=32), rnd(N, seed=33)
    w_eff = w.permute(0, 2, 1).reshape(N, ntaps * C)  # k = tap * C + c
    y, _ = gemm_ref(x, w_eff, M=B * T, ntaps=ntaps, T=T, xstride=xstride, halo=halo, halo_mode=halo_mode, x_prev=xp, bias=b)
    torch.testing.assert_close(y, conv_torch(x, xp, w, b, T, xstride, halo, halo_mode), rtol=1e-12, atol=1e-12)
    # the previous-frame rows matter (halo_mode 0) / do not (1, 2)
    y2, _ = gemm_ref(x, w_eff, M=B * T, ntaps=ntaps, T=T, xstride=xstride, halo=halo, halo_mode=halo_mode, x_prev=xp + 1, bias=b)
    assert (not torch.equal(y, y2)) == (halo_mode == 0)


def test_bf16_round_matches_oracle():
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32) * 7
    x[:4] = [1.00390625, 1.01171875, -1.00390625, 3.0]  # exact ties round to even
    np.testing.assert_array_equal(bf16_round(torch.from_numpy(x)).numpy().astype(np.float32), O.bf16_round(x))


def test_bf16_lnfold_matches_oracle():
    """wfmt 2 + PRE_LNFOLD: the oracle's rounding model of the bf16 LM path"""
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((5, 128)) + 3).astype(np.float32)
    w, gam, bet, b = (rng.standard_normal(s).astype(np.float32) for s in ((48, 128), 128, 128, 48))
    want = O.lnfold_linear_bf16(O.bf16_round(x), w, gam, bet, b, 1e-5, stats_from=x)
    wr = O.bf16_round(w * gam[None, :])
    y, _ = gemm_ref(torch.from_numpy(x), torch.from_numpy(wr), M=5, wfmt=2, pre=PRE_LNFOLD,
                    ln_s=torch.from_numpy(wr.sum(axis=1, dtype=np.float32)), ln_c=torch.from_numpy((w @ bet + b).astype(np.float32)))
    np.testing.assert_allclose(y.numpy(), want, rtol=2e-5, atol=2e-5)


def test_int8_matches_oracle():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((7, 64)).astype(np.float32)
    w = rng.standard_normal((32, 64)).astype(np.float32)
    wdq = O.quantize_dequantize_int8(w)
    y, _ = gemm_ref(torch.from_numpy(x), torch.from_numpy(wdq), M=7, wfmt=1)
    np.testing.assert_allclose(y.numpy(), x.astype(np.float64) @ wdq.astype(np.float64).T, rtol=1e-12, atol=1e-12)
    # folded LayerNorm: gain on x, fold vectors of the dequantised matrix
    gam, bet = rng.standard_normal(64).astype(np.float32), rng.standard_normal(64).astype(np.float32)
    y, _ = gemm_ref(torch.from_numpy(x), torch.from_numpy(wdq), M=7, wfmt=1, pre=PRE_LNFOLD, ln_g=torch.from_numpy(gam),
                    ln_s=torch.from_numpy(wdq.astype(np.float64) @ gam), ln_c=torch.from_numpy(wdq.astype(np.float64) @ bet))
    xd = torch.from_numpy(x).double()
    want = F.linear(F.layer_norm(xd, (64,), torch.from_numpy(gam).double(), torch.from_numpy(bet).double(), eps=1e-5),
                    torch.from_numpy(wdq).double())
    torch.testing.assert_close(y, want, rtol=1e-5, atol=1e-5)  # x * gain rounds to fp32 on load


def test_split_products_are_exact():
    """wfmt 3: hi*hi + hi*lo + lo*hi of the split operands, i.e. x w up to the dropped lo*lo term (~2^-16 relative)"""
    x, w = rnd(6, 64, seed=40).float(), rnd(16, 64, seed=41).float()
    wh = bf16_round(w)
    wl = bf16_round(w.double() - wh)
    y, scale = gemm_ref(x, wh, w_lo=wl, M=6, wfmt=3)
    exact = x.double() @ w.double().T
    assert ((y - exact).abs() <= 2.0 ** -15 * scale).all()
    xh = bf16_round(x)
    xl = bf16_round(x.double() - xh)
    torch.testing.assert_close(y, xh @ wh.T + xl @ wh.T + xh @ wl.T, rtol=0, atol=0)
