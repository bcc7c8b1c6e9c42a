"""Every tile x format x prologue x epilogue of the reduced-precision codec (gemm_h_kernel on bf16, gemm_f8_kernel on e4m3)
and its last conv (pcm_conv_h_kernel), one launch at a time through the production launchers (Engine.debug_codec_gemm ->
ptts_debug_codec_gemm), against the float64 reference of tests/codec_ref.py on the operands the kernel consumed.

Bound.  bf16 x bf16 and e4m3 x e4m3 products are exact in fp32 (8 + 8 and 4 + 4 significand bits), so the kernel's
accumulator differs from the reference only by the order of the fp32 summation: K products, in at most K / 32 MFMA steps
per output, each step adding a 32-term dot product into the accumulator.  Bounding every addition by one rounding gives
|acc - ref| <= (K / 32 + 5) u sum |x w| with u = 2^-24; the e4m3 epilogue adds two roundings (wscale * xs, then the
product).  Hence, before output rounding,

    |y - ref| <= tol_sum(K) * (xs * wscale * sum |x w| + |b|)   (scaled by the epilogue's |ls|, plus |r| for a residual)

with tol_sum(K) = max(2^-18, (K / 32 + 5) u): 2^-18 up to K = 1888, the worst case above (ff2, K = 2048; K = 2080 edge),
and the LayerNorm fold's fp32 statistics added as layer_stats in codec_ref.py states them.  The e4m3 MFMA does not sum its
32 products as fp32 does; test_fp8_mfma_step_model pins how, and codec_ref.f8_mfma_bound adds what that model drops.
pcm_conv_h_kernel sums its K = C * ntaps products in one fp32 chain (worst case (K + 1) u, 2^-16.4 at K = 192); it is
held to 2^-18, tighter than that worst case, which data of random sign meets (the chain's error grows like sqrt(K) u).
Output rounding on top: a bf16 output lies within half a bf16 ulp of the bounded interval (round to nearest even), an e4m3
output is one of the two e4m3 neighbours of its ends times yinv (exactly +-448 when saturated), int16 PCM within one step."""

import math
from collections import defaultdict

import pytest
import torch

from codec_ref import (E4M3_MAX, EPI_CONVTR, EPI_QKV, EPI_RES, EPI_STORE, PRE_LNFOLD, PRE_NONE, codec_gemm_ref, e4m3,
                       e4m3_neighbours, f32_div, f8_mfma_bound, pcm_ref, quant_weight_f8)
from gemm_ref import ACT_ELU, ACT_GELU, ACT_NONE, F64, bf16_round

pytestmark = pytest.mark.gpu

TOL = 2.0 ** -18
DEV = "cuda:0"
TILES = [(2, 4, 2, 2), (2, 2, 2, 2), (1, 2, 2, 2), (1, 1, 2, 2)]
NAMES = ["gemm_h<2,4,2,2>", "gemm_h<2,2,2,2>", "gemm_h<1,2,2,2>", "gemm_h<1,1,2,2>"]
EPI_NAME = {EPI_STORE: "store", EPI_RES: "res", EPI_QKV: "qkv", EPI_CONVTR: "convtr"}
STATS = defaultdict(lambda: [0.0, 0])  # (fmt, cfg, epilogue) -> [worst scaled error, cases]


def tol_sum(K, fmt=0):
    """relative bound of the accumulator's summation error over K products (see the module docstring)"""
    return max(TOL, (K / 32 + 5) * 2.0 ** -24)


def cdiv(a, b):
    return (a + b - 1) // b


def prod_tile(NT, MT):
    """mirror of choose_h_tile (ptts_dispatch.hip) / choose_f8_tile (ptts_fp8.hip)"""
    for i, t in enumerate(TILES):
        if t[0] * t[2] > 2 * NT and i < 3:
            continue
        if cdiv(NT, t[0] * t[2]) * cdiv(MT, t[1] * t[3]) >= 512 or i == 3:
            return i
    return 3


def label_of(fmt, cfg, pre, NT, MT):
    if fmt == 1:
        return f"gemm_f8@{NT * MT}"
    t = TILES[cfg]
    return f"{NAMES[cfg]}{'+ln' if pre == PRE_LNFOLD else ''}@{cdiv(NT, t[0] * t[2]) * cdiv(MT, t[1] * t[3]) * 256}"


@pytest.fixture(scope="module")
def eng():
    from pocket_tts_amd.config import named_config
    from pocket_tts_amd.engine import Engine
    from pocket_tts_amd.weights import generate_state_dict

    cfg = named_config("tiny")
    e = Engine(cfg, generate_state_dict(cfg, 0), DEV)
    yield e
    e.close()


def make(M, N, C, ntaps=1, *, fmt=0, pre=PRE_NONE, epi=EPI_STORE, act=ACT_NONE, T=16, halo=None, par=0, mode=0, cout=0,
         stride=0, yf8=0, yinv=1.0, xs=1.0, ls=True, bias=True, yraw=False, mean=0.0, wmul=1.0, zero_rows=0, H=0, Tq=16,
         ring=0, cap=0, offset=None, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)

    def rn(*shape, s=1.0, m=0.0):
        return torch.randn(*shape, generator=g, device=DEV, dtype=torch.float32) * s + m

    K = C * ntaps
    kw = dict(fmt=fmt, pre=pre, epi=epi, act=act, T=T, halo=(ntaps - 1 if halo is None else halo), par=par, mode=mode,
              cout=cout, stride=stride, yf8=yf8, yinv=yinv, xs=xs, yraw=yraw, ntaps=ntaps, H=H, Tq=Tq, ring=ring, cap=cap,
              offset=offset)
    kw["x"] = rn(M, C, m=mean) * xs
    kw["x_prev"] = rn(M, C) * xs if ntaps > 1 else None
    kw["w"] = rn(C, cout, 2 * stride, s=wmul / math.sqrt(K)) if mode == 1 else rn(N, C, ntaps, s=wmul / math.sqrt(K))
    if zero_rows:
        kw["w"][:zero_rows] = 0.0
    kw["bias"] = rn(cout if mode == 1 else N, s=0.1) if bias else None
    if pre == PRE_LNFOLD:
        kw["ln_w"], kw["ln_b"] = rn(C, s=0.2, m=1.0), rn(C, s=0.1)
    if epi == EPI_RES:
        kw["r"] = rn(M, N)
        kw["ls"] = rn(N, s=0.1, m=0.5) if ls else None
    return kw


def run(eng, kw, cfg):
    kw = dict(kw)
    x, w = kw.pop("x"), kw.pop("w")
    return eng.debug_codec_gemm(x, w, cfg=cfg, want_operands=True, **kw)


def bf16_ulp(v):
    _, e = torch.frexp(v.abs().clamp(min=2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), e - 8)


def check(kw, out, M, N, cfg_key, repeat=None):
    fmt, pre, epi = kw["fmt"], kw["pre"], kw["epi"]
    ntaps = kw["ntaps"]
    x, xp, w_eff = out["x_eff"].to(F64), out["xp_eff"].to(F64), out["w_eff"].to(F64)
    # the consumed operands are the production conversions of the case's operands
    if fmt == 0:
        assert torch.equal(x, bf16_round(kw["x"]))
    else:
        xs = torch.tensor(kw["xs"], dtype=torch.float32).item()
        inv = f32_div(1.0, xs).item()
        q = e4m3((kw["x"].to(F64) * inv).to(torch.float32))
        assert torch.equal(x, (q * xs).to(torch.float32).to(F64))  # fp32 products, as the kernel and the hook form them
    if kw.get("mode") == 1:
        from codec_ref import convtr_weight
        w2 = convtr_weight(kw["w"], kw["stride"])
    else:
        w2 = kw["w"].permute(0, 2, 1).reshape(N, -1).to(F64)
        if pre == PRE_LNFOLD:
            w2 = (kw["w"][:, :, 0] * kw["ln_w"]).to(F64)
    if fmt == 0:
        assert torch.equal(w_eff, bf16_round(w2))
    else:
        deq, scale = quant_weight_f8(w2)
        assert torch.equal(out["wscale"].to(F64), scale)
        assert torch.equal(w_eff, deq)
    if pre == PRE_LNFOLD:
        K = w_eff.shape[1]
        s_ref = w_eff.sum(1)
        assert ((out["ln_s"].to(F64) - s_ref).abs() <= (K / 64 + 8) * 2.0 ** -24 * w_eff.abs().sum(1)).all()
    pre_act, ref, scale = codec_gemm_ref(x, w_eff, M=M, ntaps=ntaps, T=kw["T"], halo=kw["halo"], xp_eff=xp,
                                         bias=kw["bias"], pre=pre, ln_s=out.get("ln_s"), ln_c=out.get("ln_c"), epi=epi,
                                         act=kw["act"], r=kw.get("r"), ls=kw.get("ls"), stride=kw["stride"] or 1,
                                         rope=out.get("rope"), H=kw["H"])
    y = out["y"].to(F64)
    assert torch.isfinite(y).all()
    if repeat is not None:
        assert torch.equal(out["y"], repeat["y"])
    tol = tol_sum(ntaps * x.shape[1]) * scale + 2.0 ** -22 * ref.abs()  # + the activation's fp32 evaluation
    if fmt == 1:  # + what the e4m3 MFMA drops (test_fp8_mfma_step_model), through the layer scale of a residual
        sx = torch.tensor(kw["xs"], dtype=torch.float32).item()
        tol = tol + f8_mfma_bound(x, w_eff, out["wscale"].to(F64) * sx, M=M, ntaps=ntaps, T=kw["T"], halo=kw["halo"],
                                  xp_eff=xp, stride=kw["stride"] or 1, convtr=epi == EPI_CONVTR)
    if epi == EPI_QKV:
        err = ((y - ref).abs() / tol).max().item()
    elif kw["yf8"]:
        yinv = kw["yinv"]
        lo, _ = e4m3_neighbours((ref - tol) * yinv)
        _, hi = e4m3_neighbours((ref + tol) * yinv)
        assert ((y >= lo) & (y <= hi)).all(), "e4m3 output outside the neighbours of ref * yinv"
        sat = (ref - tol) * yinv >= E4M3_MAX
        assert (y[sat] == E4M3_MAX).all() and (y[(ref + tol) * yinv <= -E4M3_MAX] == -E4M3_MAX).all()
        assert (y[ref == 0] == 0).all()
        # distance to the clamped reference over the interval's width (zero where the interval is a single point: exact)
        d = (y / yinv - ref.clamp(-E4M3_MAX / yinv, E4M3_MAX / yinv)).abs()
        w = tol + (hi - lo) / yinv
        err = torch.where(w > 0, d / w.clamp(min=1e-300), torch.zeros_like(d)).max().item()
    else:
        # round to nearest: |y - acc| <= ulp(y) / 2 (RNE never leaves acc's binade downwards, so ulp(acc) <= ulp(y))
        err = (((y - ref).abs() - 0.5 * bf16_ulp(y)).clamp(min=0) / tol).max().item()
    if kw["yraw"]:
        yr = out["yraw"].to(F64)
        assert (((yr - pre_act).abs() - 0.5 * bf16_ulp(yr)).clamp(min=0) <= tol).all(), "Yraw"
    st = STATS[cfg_key]
    st[0] = max(st[0], err)
    st[1] += 1
    assert err <= 1.0, f"scaled error {err}"


# ---- cases ----------------------------------------------------------------------------------------------------------
# en100m's codec: transformer width 512, ff 2048, heads 8; SEANet n_filters 64, ratios 6 / 5 / 4, rows per sequence per
# frame 16 / 96 / 480 / 1920
def prod_cases(B):
    r0, r1, r2, r3 = 16, 96, 480, 1920
    M = B * 16
    out = [
        ("qkv", M, 1536, 512, dict(pre=PRE_LNFOLD, epi=EPI_QKV, H=8, Tq=16, ring=272, cap=272, offset=[37 * b % 250 for b in range(B)])),
        ("out", M, 512, 512, dict(epi=EPI_RES)),
        ("ff1", M, 2048, 512, dict(pre=PRE_LNFOLD, act=ACT_GELU)),
        ("ff2", M, 512, 2048, dict(epi=EPI_RES)),
        ("conv0", B * r0, 512, 512, dict(ntaps=7, T=r0, act=ACT_ELU)),
    ]
    for (cin, cout, s, Tin, Tout) in ((512, 256, 6, r0, r1), (256, 128, 5, r1, r2), (128, 64, 4, r2, r3)):
        out.append((f"convtr{s}", B * Tin, s * cout, cin, dict(ntaps=2, T=Tin, mode=1, cout=cout, stride=s, epi=EPI_CONVTR,
                                                               act=ACT_ELU, yraw=True)))
        out.append((f"res{cout}a", B * Tout, cout // 2, cout, dict(ntaps=3, T=Tout, act=ACT_ELU)))
        out.append((f"res{cout}b", B * Tout, cout, cout // 2, dict(epi=EPI_RES, ls=False, act=ACT_ELU)))
    return out


# the fp8 codec runs the transformer and conv0 in bf16 (conv0 with an e4m3 output) and the SEANet blocks on e4m3
PROD = [(fmt, B, *c) for B in (1, 3, 64) for c in prod_cases(B) for fmt in (0, 1)
        if fmt == 0 or c[0].startswith(("convtr", "res"))]
PROD += [(0, B, "conv0_f8out", B * 16, 512, 512, dict(ntaps=7, T=16, act=ACT_ELU, yf8=1, yinv=30.0)) for B in (1, 3, 64)]


@pytest.mark.parametrize("case", PROD, ids=lambda c: f"{'bf16' if c[0] == 0 else 'e4m3'}-B{c[1]}-{c[2]}")
def test_production_shapes(eng, case):
    fmt, B, name, M, N, C, extra = case
    extra = dict(extra)
    ntaps = extra.pop("ntaps", 1)
    if fmt == 1:
        extra.setdefault("xs", 0.05)
        if name != "res64b":  # the last residual block's output feeds the bf16-input last conv
            extra.update(yf8=1, yinv=20.0)
    kw = make(M, N, C, ntaps, fmt=fmt, seed=B, **extra)
    out = run(eng, kw, -1)
    assert out is not None
    NT, MT = cdiv(N, 16), cdiv(M, 16)
    assert out["cfg"] == prod_tile(NT, MT)
    assert out["label"] == label_of(fmt, out["cfg"], kw["pre"], NT, MT)
    check(kw, out, M, N, (fmt, out["cfg"], EPI_NAME[kw["epi"]] + ("->e4m3" if kw["yf8"] else "")))


def edge_cases():
    cs = []
    for C in (32, 64, 96, 2048, 2080):  # KF 1, 2, 3, large even, large odd
        cs.append((f"kf{C // 32}", 32, 64, C, {}))
    for N in (32, 64, 96, 160):
        for M in (1, 15, 16, 17, 33, 63, 64, 65, 112, 129, 145, 272):  # MT 1 .. 17 around TM * WM = 2, 4, 8
            cs.append((f"n{N}m{M}", M, N, 64, dict(act=ACT_GELU)))
    for k in (3, 7):
        for halo in range(k):
            for par in (0, 1):
                cs.append((f"k{k}h{halo}p{par}", 96, 64, 64, dict(ntaps=k, T=48, halo=halo, par=par, act=ACT_ELU, yraw=True)))
    cs.append(("k3T32", 64, 32, 32, dict(ntaps=3, T=32)))
    for mean in (0.0, 4.0, 30.0):
        cs.append((f"ln{int(mean)}", 48, 96, 512, dict(pre=PRE_LNFOLD, mean=mean)))
    cs.append(("lnqkv", 48, 3 * 2 * 64, 512, dict(pre=PRE_LNFOLD, epi=EPI_QKV, H=2, Tq=16, ring=64, cap=64, offset=[0, 50, 63])))
    cs.append(("qkvwrap", 32, 3 * 64, 64, dict(epi=EPI_QKV, H=1, Tq=16, ring=32, cap=48, offset=[20, 31])))
    cs.append(("qkvlin", 48, 3 * 64, 64, dict(epi=EPI_QKV, H=1, Tq=48, ring=0, cap=112, offset=[60])))
    cs.append(("res_ls", 33, 64, 64, dict(epi=EPI_RES, act=ACT_ELU)))
    cs.append(("res", 33, 64, 64, dict(epi=EPI_RES, ls=False)))
    cs.append(("ctr", 32, 3 * 32, 64, dict(ntaps=2, T=16, mode=1, cout=32, stride=3, epi=EPI_CONVTR, par=1, yraw=True)))
    # e4m3 outputs: saturated, subnormal, exactly zero (zero weight rows, no bias)
    cs.append(("f8sat", 32, 64, 64, dict(yf8=1, yinv=800.0, yraw=True)))
    cs.append(("f8sub", 32, 64, 64, dict(yf8=1, yinv=2.0 ** -6)))
    cs.append(("f8zero", 32, 64, 64, dict(yf8=1, yinv=4.0, bias=False, zero_rows=8)))
    cs.append(("f8res", 33, 64, 64, dict(epi=EPI_RES, ls=False, act=ACT_ELU, yf8=1, yinv=16.0)))
    cs.append(("f8res_sat", 48, 96, 64, dict(epi=EPI_RES, ls=False, yf8=1, yinv=300.0)))
    cs.append(("f8ctr_sat", 32, 3 * 32, 64, dict(ntaps=2, T=16, mode=1, cout=32, stride=3, epi=EPI_CONVTR, yf8=1, yinv=300.0,
                                                 yraw=True)))
    return cs


EDGE = edge_cases()


@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("case", EDGE, ids=lambda c: c[0])
def test_edge_shapes(eng, fmt, cfg, case):
    name, M, N, C, extra = case
    extra = dict(extra)
    ntaps = extra.pop("ntaps", 1)
    if fmt == 1:
        extra.setdefault("xs", 0.25)
    kw = make(M, N, C, ntaps, fmt=fmt, seed=cfg + 7, **extra)
    out = run(eng, kw, cfg)
    refused = fmt == 1 and (kw["pre"] == PRE_LNFOLD or kw["epi"] == EPI_QKV or (kw["epi"] == EPI_RES and kw.get("ls") is not None))
    refused |= fmt == 0 and kw["yf8"] and kw["epi"] != EPI_STORE
    if refused:
        assert out is None
        return
    assert out is not None and out["cfg"] == cfg
    assert out["label"] == label_of(fmt, cfg, kw["pre"], cdiv(N, 16), cdiv(M, 16))
    again = run(eng, kw, cfg)
    check(kw, out, M, N, (fmt, cfg, EPI_NAME[kw["epi"]] + ("->e4m3" if kw["yf8"] else "")), repeat=again)


@pytest.mark.parametrize("big_k", [0, 17, 31])
def test_fp8_mfma_step_model(eng, big_k):
    """One 16x16x32 e4m3 step on operands built so that fp32 accumulation would be exact: row m holds one product
    448 * 2^a at k = big_k and 31 products 448 * 2^-b (gap a + b up to 17 binades, every partial sum fits in fp32).  A
    residual of -1.75 * 2^a cancels the large product, so the bf16 output shows what the step kept of the small ones.
    The MFMA keeps the 24 small products outside big_k's group of 8 exactly and truncates each of the 7 inside it to a
    multiple of 2^(E - 13), E = the large product's exponent: the model codec_ref.f8_mfma_bound charges.  The bf16 MFMA
    on the same operands keeps everything."""
    from codec_ref import F8_GROUP, F8_KEEP

    M, N, C = 16, 32, 32
    x, r = torch.zeros(M, C), torch.zeros(M, N)
    ab = [(min(8, m + 2), m + 2 - min(8, m + 2)) for m in range(M)]
    for m, (a, b) in enumerate(ab):
        x[m, :] = 2.0 ** -b
        x[m, big_k] = 2.0 ** a
        r[m, :] = -1.75 * 2.0 ** a
    w = torch.full((N, C), 1.75)  # amax 1.75: wscale 2^-8 exactly, every weight the e4m3 code 448
    for fmt in (0, 1):
        out = eng.debug_codec_gemm(x.to(DEV), w.to(DEV), fmt=fmt, epi=EPI_RES, xs=1.0, r=r.to(DEV), want_operands=True)
        y = out["y"].cpu().to(F64)
        for m, (a, b) in enumerate(ab):
            small = 448.0 * 2.0 ** -b
            if fmt == 0:
                kept = 31 * small
            else:
                q = 2.0 ** (math.floor(math.log2(448.0 * 2.0 ** a)) - F8_KEEP)
                kept = (31 - (F8_GROUP - 1)) * small + (F8_GROUP - 1) * math.floor(small / q) * q
            assert (y[m] == kept * 2.0 ** -8).all(), (fmt, a, b, y[m, 0].item(), kept * 2.0 ** -8)


def test_admitted_sets(eng):
    """every tile runs for both formats; combinations no kernel implements launch nothing"""
    for fmt in (0, 1):
        for cfg in range(4):
            assert run(eng, make(32, 64, 64, fmt=fmt, xs=0.5), cfg) is not None
    assert run(eng, make(32, 64, 64, fmt=1, pre=PRE_LNFOLD), -1) is None
    assert run(eng, make(32, 192, 64, fmt=1, epi=EPI_QKV, H=1, Tq=16, ring=0, cap=32, offset=[0, 0]), -1) is None
    assert run(eng, make(32, 64, 64, fmt=1, epi=EPI_RES), -1) is None  # layer scale on fp8 RES
    assert run(eng, make(32, 64, 48), -1) is None  # C % 32
    assert run(eng, make(32, 64, 64, fmt=0, epi=EPI_RES, yf8=1, yinv=2.0), -1) is None  # gemm_h's RES stores bf16 only
    assert run(eng, make(32, 64, 64, 3, fmt=0, T=16, pre=PRE_LNFOLD), -1) is None  # the fold is for Linear layers


@pytest.mark.parametrize("B,T,halo,scale", [(1, 1920, 2, 1.0), (3, 16, 2, 1.0), (2, 32, 0, 1.0), (2, 32, 1, 1.0), (4, 48, 2, 8.0)])
@pytest.mark.parametrize("par", [0, 1])
def test_pcm_conv(eng, B, T, halo, scale, par):
    M, C = B * T, 64
    g = torch.Generator(device=DEV).manual_seed(B * 100 + T + par)
    x, xp = (torch.randn(M, C, generator=g, device=DEV) for _ in range(2))
    w = torch.randn(1, C, 3, generator=g, device=DEV) * scale / math.sqrt(3 * C)
    b = torch.randn(1, generator=g, device=DEV) * 0.1
    out = eng.debug_codec_gemm(x, w, kind=1, T=T, halo=halo, par=par, x_prev=xp, bias=b, want_operands=True)
    assert out["label"] == "pcm_conv_h"
    y, scale_ref, i16 = pcm_ref(out["x_eff"], w, M=M, T=T, halo=halo, xp_eff=out["xp_eff"], bias=b)
    err = ((out["y"].to(F64) - y).abs() / (TOL * scale_ref)).max().item()
    STATS[(0, 0, "pcm")][0] = max(STATS[(0, 0, "pcm")][0], err)
    STATS[(0, 0, "pcm")][1] += 1
    assert err <= 1.0
    assert ((out["y_i16"].to(F64) - i16).abs() <= 1).all()
    if scale > 1:
        assert (y.abs() > 1).any() and (out["y_i16"].abs().max() == 32767)


def test_zz_error_tables():
    print("\nworst |y - ref| / bound per (fmt, cfg, epilogue) [cases]")
    for key in sorted(STATS):
        worst, n = STATS[key]
        print(f"  {'bf16' if key[0] == 0 else 'e4m3'} cfg {key[1]} {key[2]:13s}: {worst:.3e}  [{n}]")
    assert STATS, "no case ran"


@pytest.mark.parametrize("groups", [None, "codec_split", "codec_bf16", "codec_fp8"])
def test_reset_row_bitwise(groups):
    """ptts_mimi_state_reset_row in every codec format (per-format element sizes of the double buffers): after a reset, row
    r's PCM is bitwise that of a fresh state of the same batch fed the same latents, and the other rows are bitwise those of
    a twin that was not reset (GEMM and attention results are per-row independent at a fixed batch)."""
    import numpy as np

    from conftest import synth_weights
    from pocket_tts_amd.engine import Engine

    cfg, W = synth_weights("en100m")
    B, r, warm, k = 3, 1, 3, 3
    rng = np.random.default_rng(21)
    lat = [torch.from_numpy(rng.standard_normal((B, cfg.mimi.quantizer.dimension)).astype(np.float32)).to(DEV)
           for _ in range(warm + k)]
    eng = Engine(cfg, W, DEV, quantize_groups={groups} if groups else None)
    try:
        a, twin, fresh = eng.new_mimi_state(B), eng.new_mimi_state(B), eng.new_mimi_state(B)
        for f in range(warm):
            eng.mimi_decode(a, lat[f])
            eng.mimi_decode(twin, lat[f])
        a.reset_row(r)
        for f in range(warm, warm + k):
            pa = eng.mimi_decode(a, lat[f]).cpu()
            pt = eng.mimi_decode(twin, lat[f]).cpu()
            pf = eng.mimi_decode(fresh, lat[f]).cpu()
            assert torch.isfinite(pa).all()
            assert torch.equal(pa[r], pf[r]), f"frame {f - warm} after the reset: row {r} differs from a fresh state"
            others = [i for i in range(B) if i != r]
            assert torch.equal(pa[others], pt[others]), f"frame {f - warm}: the reset changed another row"
            assert not torch.equal(pa[r], pt[r])
    finally:
        eng.close()
