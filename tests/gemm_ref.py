"""float64 reference of ONE GEMM of the hot path's kernel family (gemm_kernel / gemm_lds_kernel, ptts_kernels.h), on exactly
the operands the kernel consumes (Engine.debug_gemm returns the effective weight image and the LayerNorm fold vectors):

    y[m][n] = epilogue( sum_tap sum_c pre(x[row(m, tap)][c]) * w[n][tap * C + c] )

with the activation rounded as the weight format rounds it (bf16 round-to-nearest-even for wfmt 2, the hi / lo split
for wfmt 3, x * ln_g for int8 with a folded LayerNorm).  bf16 x bf16 and split products are exact in fp32, so the kernel
and this reference then differ only by the order of the fp32 summation, in every format.

Enumerations as in ptts_kernels.h / include/ptts.h.  Device-agnostic torch: the tensors' device is used throughout.
The epilogues behind EPI_GATE are tested where they run: EPI_QKV in test_gpu_lm_matrix.py (the fp32 FlowLM),
test_gpu_mimi_matrix.py and test_gpu_codec_matrix.py (the codec), EPI_HEAD and EPI_LATENT in test_gpu_flow_matrix.py,
EPI_CONVTR in test_gpu_mimi_matrix.py and test_gpu_codec_matrix.py, EPI_PCM in test_gpu_mimi_matrix.py."""

from __future__ import annotations

import math

import torch

PRE_NONE, PRE_ELU, PRE_ADDSILU, PRE_LNFOLD, PRE_LNMOD = range(5)
EPI_STORE, EPI_RES, EPI_GATE = range(3)
ACT_NONE, ACT_GELU, ACT_SILU, ACT_ELU = range(4)

# mirror of kCfgName / kCfgShape in ptts_dispatch.hip: {TN, TM, WK, WN, WM} of the register-staged configurations,
# {BNT, BMT, 0, 0, 0} of the LDS-staged ones
CFG_NAME = ["gemm<1,1,8,1,1>", "gemm<1,2,4,1,1>", "gemm<1,4,4,1,1>", "gemm<2,4,1,2,2>", "gemm<2,4,1,1,4>", "gemm<1,4,1,1,4>",
            "gemm<1,1,1,1,4>", "gemm<2,4,4,1,1>", "gemm_lds<4,8,2>", "gemm_lds<4,4,2>", "gemm<2,2,4,1,1>", "gemm<1,1,4,1,1>",
            "gemm_lds<4,2,2>", "gemm<1,2,1,2,2>", "gemm<2,4,2,2,1>", "gemm_lds<8,8,2>", "gemm_lds<8,4,2>", "gemm_lds<8,2,2>"]
CFG_SHAPE = [(1, 1, 8, 1, 1), (1, 2, 4, 1, 1), (1, 4, 4, 1, 1), (2, 4, 1, 2, 2), (2, 4, 1, 1, 4), (1, 4, 1, 1, 4),
             (1, 1, 1, 1, 4), (2, 4, 4, 1, 1), (8, 4, 0, 0, 0), (4, 4, 0, 0, 0), (2, 2, 4, 1, 1), (1, 1, 4, 1, 1),
             (2, 4, 0, 0, 0), (1, 2, 1, 2, 2), (2, 4, 2, 2, 1), (8, 8, 0, 0, 0), (4, 8, 0, 0, 0), (2, 8, 0, 0, 0)]

F64 = torch.float64


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 round-to-nearest-even (v_cvt_pk_bf16_f32), as float64"""
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def gather_rows(x, M, ntaps=1, T=16, xstride=1, halo=0, halo_mode=1, x_prev=None, rows=None):
    """[len(rows)][ntaps][C] float64: input row of every (output row, tap).  Output row m = b * T + t reads
    x[b * T * xstride + t * xstride + tap - halo]; rows before the sequence's start come from x_prev (halo_mode 0,
    the previous frame: same offset from the END of the sequence's rows), are zero (1) or repeat its first row (2)."""
    x = x.to(F64)
    m = torch.arange(M, device=x.device) if rows is None else rows.to(x.device)
    if ntaps == 1:
        return x[m][:, None, :]
    b, t = m // T, m % T
    base = b * T * xstride
    out = []
    for tap in range(ntaps):
        ts = t * xstride + tap - halo
        inside = ts >= 0
        v = x[(base + ts.clamp(min=0))].clone()
        before = ~inside
        if before.any():
            if halo_mode == 0:
                v[before] = x_prev.to(F64)[(base + T * xstride + ts)[before]]
            elif halo_mode == 1:
                v[before] = 0.0
            else:
                v[before] = x[base[before]]
        out.append(v)
    return torch.stack(out, dim=1)


def _act(v, act):
    if act == ACT_GELU:
        return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    if act == ACT_SILU:
        return v * torch.sigmoid(v)
    if act == ACT_ELU:
        return torch.where(v > 0, v, torch.expm1(v))
    return v


def gemm_ref(x, w_eff, *, M, ntaps=1, T=16, xstride=1, halo=0, halo_mode=1, x_prev=None, wfmt=0, w_lo=None,
             pre=PRE_NONE, ln_g=None, ln_s=None, ln_c=None, prevec=None, lnm_w=None, lnm_b=None, mod_shift=None,
             mod_scale=None, bias=None, epi=EPI_STORE, act=ACT_NONE, r=None, g=None, ls=None, rows=None, eps=1e-5):
    """Returns (y, scale) as float64 [len(rows)][N] (rows: subset of output rows, default all M).  `scale` is what an
    fp32 summation error of y is measured against: rs * sum_k |x_k w_k| + |b| (rs = the LayerNorm's 1 / std, else 1),
    carried through the epilogue's multiplications, plus |r| where a residual is added.
    w_eff: [N][ntaps * C] (k = tap * C + c); for wfmt 3 the hi image, w_lo the lo image.  For PRE_LNFOLD: ln_s, ln_c
    = the fold vectors the kernel uses (bias included in ln_c), ln_g = the LayerNorm gain applied to x on load (int8)."""
    w = w_eff.to(F64)
    N, K = w.shape
    C = K // ntaps
    X = gather_rows(x, M, ntaps, T, xstride, halo, halo_mode, x_prev, rows)  # [R][ntaps][C]
    sel = torch.arange(M, device=X.device) if rows is None else rows.to(X.device)
    if pre == PRE_ELU:
        X = torch.where(X > 0, X, torch.expm1(X))
    elif pre == PRE_ADDSILU:
        X = X + prevec.to(F64)
        X = X * torch.sigmoid(X)
    elif pre == PRE_LNMOD:
        mu = X.mean(dim=-1, keepdim=True)
        var = ((X - mu) ** 2).mean(dim=-1, keepdim=True)
        X = (X - mu) / torch.sqrt(var + eps)
        if lnm_w is not None:
            X = X * lnm_w.to(F64) + lnm_b.to(F64)
        X = X * (1.0 + mod_scale.to(F64)[sel][:, None, :]) + mod_shift.to(F64)[sel][:, None, :]
    rs = torch.ones(X.shape[0], 1, dtype=F64, device=X.device)
    if pre == PRE_LNFOLD:
        # statistics of the unrounded fp32 row (ntaps == 1)
        mu = X[:, 0].mean(dim=-1, keepdim=True)
        var = (X[:, 0] * X[:, 0]).mean(dim=-1, keepdim=True) - mu * mu
        rs = 1.0 / torch.sqrt(var.clamp(min=0) + eps)
        if ln_g is not None:
            X = (X.to(torch.float32) * ln_g.to(torch.float32)).to(F64)  # int8: x * gain on load, in fp32
    X = X.reshape(X.shape[0], K)
    if wfmt == 2:
        X = bf16_round(X)
    if wfmt == 3:
        xh = bf16_round(X)
        xl = bf16_round(X - xh)
        wl = w_lo.to(F64)
        acc = xh @ w.T + xl @ w.T + xh @ wl.T
        mag = X.abs() @ (w + wl).abs().T
    else:
        acc = X @ w.T
        mag = X.abs() @ w.abs().T
    if pre == PRE_LNFOLD:
        s, c = ln_s.to(F64), ln_c.to(F64)
        v = (acc - s * mu) * rs + c
        scale = rs * mag + c.abs()
    else:
        b = bias.to(F64) if bias is not None else torch.zeros(N, dtype=F64, device=X.device)
        v = acc + b
        scale = mag + b.abs()
    if epi == EPI_STORE:
        y = _act(v, act)
    elif epi == EPI_RES:
        rr = r.to(F64)[sel]
        if ls is not None:
            v = v * ls.to(F64)
            scale = scale * ls.to(F64).abs()
        y = _act(rr + v, act)
        scale = scale + rr.abs()
    else:
        rr, gg = r.to(F64)[sel], g.to(F64)[sel]
        y = rr + gg * v
        scale = scale * gg.abs() + rr.abs()
    return y, scale
