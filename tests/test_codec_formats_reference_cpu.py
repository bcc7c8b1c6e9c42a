"""CPU checks of the format stages of tests/mimi_ref.py (the reference of tests/test_gpu_codec_formats.py); no GPU.

  * identity roundings: with every rounding replaced by the identity, each format stage IS the fp64 stage of mimi_ref
    (bitwise, but for the two +ln stages, which restate LayerNorm + Linear as the folded GEMM: the same number to 1e-12);
  * the rounding model: the bf16 chain agrees with `oracle.np_oracle.MimiDecoderBF16` to the accuracy
    tests/test_oracle_bf16_model.py establishes for two evaluations of one rounding model (their SNR exceeds the format's
    price, the model's SNR against the fp32 oracle, which lies in 38 .. 50 dB);
  * seeded defects: every defect moves an element of its designated stage out of the bounded, rounded interval of the GPU
    test by at least 4 x the bound, on the taps of the reference chain of that test's cases (`nf64` / `nf64x2`, B = 3;
    the saturating case for the e4m3 wrap).  A defect that does not reach 4 gets a better-aimed case, never a lower factor."""

import numpy as np
import pytest

import mimi_ref as R
from test_gpu_codec_formats import FACTOR, seed_of

F64 = np.float64
POW2_SCALES = np.full(16, 2.0 ** -7, np.float32)  # exact products code * scale: the identity check is then bitwise


def _frames(name, fmt, B, nf, scales=None, scale=1.0, seed=None):
    cfg, W = R.codec_weights(name)
    ch = R.FChain(cfg, W, B, fmt, scales)
    lat = R.seeded_latents(cfg, nf, B, seed_of(name, fmt, B, (), ()) if seed is None else seed, scale)
    return cfg, W, [ch.decode(x) for x in lat]


_REF_SCALES = {}


def ref_scales(name):
    if name not in _REF_SCALES:
        cfg, W = R.codec_weights(name)
        _REF_SCALES[name] = R.calibrate(cfg, W, R.seeded_latents(cfg, 6, 8, 5))
    return _REF_SCALES[name]


@pytest.mark.parametrize("fmt", R.FMTS)
def test_identity_roundings_give_the_fp64_stages(fmt):
    cfg, W, fr = _frames("nf64", fmt, 2, 2, POW2_SCALES)
    cur, prev = fr[1], fr[0]
    sc = POW2_SCALES
    kw = dict(cfg=cfg, W=W, fmt=fmt, ident=True)
    val = lambda name, k: cur[name] * float(sc[k]) if fmt == "fp8" else cur[name]  # noqa: E731  (the operand's value)
    tl = lambda a, n: a[:, -n:]  # noqa: E731
    eq = lambda a, b: np.array_equal(a, b) and a.dtype == F64  # noqa: E731
    x = cur["upsample"]
    assert eq(R.fstage_B(l=0, attn=cur["tr_attn0"], x=x, **kw)["resid"], R.stage_B(cfg, W, cur["tr_attn0"], x))
    assert eq(R.fstage_D(l=0, ff=cur["tr_ff0"], resid=cur["tr_resid0"], **kw)["out"], R.stage_D(cfg, W, cur["tr_ff0"], cur["tr_resid0"]))
    c, c64 = R.fstage_C(l=0, resid=cur["tr_resid0"], **kw)["ff"], R.stage_C(cfg, W, cur["tr_resid0"])
    assert np.abs(c - c64).max() <= 1e-12 * np.abs(c64).max()
    # Q and A on a first frame against the fp64 transformer's attention output
    pos = np.tile(np.arange(16), (2, 1))
    q = R.fstage_Q(l=0, x=x, pos=pos, **kw)
    ring = R.engine_ring(cfg)
    K, V = np.zeros((2, ring, q["k"].shape[2])), np.zeros((2, ring, q["k"].shape[2]))
    K[:, :16], V[:, :16] = q["k"], q["v"]
    a, a64 = R.fstage_A(q=q["q"], K=K, V=V, pos0=np.zeros(2, np.int64), **kw)["attn"], R.stage_A(cfg, W, [x])
    assert np.abs(a - a64).max() <= 1e-12 * np.abs(a64).max()
    assert eq(R.fstage_S0(x=cur["dec_tr"], tail=tl(prev["dec_tr"], 6), scales=sc, **kw)["a0"],
              R.stage_S0(cfg, W, cur["dec_tr"], tl(prev["dec_tr"], 6)))
    src, ks = "seanet0", 0
    for i in (1, 2, 3):
        cv = R.fstage_Cv(i=i, x=cur[src], tail=tl(prev[src], 1), scales=sc, **kw)
        k_in = R.SC_IN[("convtr", i)]
        raw64 = R.stage_Cv(cfg, W, i, val(src, k_in), tl(prev[src], 1) * (float(sc[k_in]) if fmt == "fp8" else 1.0))
        assert eq(cv["raw"], raw64) and eq(cv["elu"], R._elu(raw64, False)), i
        # the block on a RAW input of bf16 values, its ELU'd copy handed to Ra as the operand's value / scale
        raw, rawp = cur[f"seanet{3 * i - 1}"], tl(prev[f"seanet{3 * i - 1}"], 2)
        s_c = float(sc[R.SC_IN[("res_a", i)]]) if fmt == "fp8" else 1.0
        h = R.fstage_Ra(i=i, x=R._elu(raw, False) / s_c, tail=R._elu(rawp, False) / s_c, scales=sc, **kw)["h"]
        s_h = float(sc[R.SC_IN[("res_b", i)]]) if fmt == "fp8" else 1.0
        out = R.fstage_Rb(i=i, h=h / s_h, skip=raw, scales=sc, **kw)["out"]
        assert eq(out, R.stage_R(cfg, W, i, raw, rawp)), i
        src = f"seanet{3 * i}"
    assert eq(R.fstage_L(x=cur["seanet9"], tail=tl(prev["seanet9"], 2), **kw)["pcm"], R.stage_L(cfg, W, cur["seanet9"], tl(prev["seanet9"], 2)))
    assert eq(R.fstage_P(lat=cur["latent"], lat_prev=prev["latent"], live=np.ones(2, bool), **kw)["upsample"],
              R.stage_P(cfg, W, cur["latent"], prev["latent"], np.ones(2, bool)))


def _snr(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return 10 * np.log10((a ** 2).sum() / ((a - b) ** 2).sum())


def test_bf16_chain_is_the_oracles_rounding_model():
    from conftest import synth_weights
    from oracle import np_oracle as O

    cfg, W = synth_weights("en100m")
    B, nf = 1, 2
    lat = np.random.default_rng(11).standard_normal((nf, B, cfg.mimi.quantizer.dimension)).astype(np.float32)

    def run(dec):
        st = dec.init_state(B, nf)
        return np.stack([dec.decode(st, lat[f]) for f in range(nf)])

    r32, r16 = run(O.MimiDecoder(cfg, W)), run(O.MimiDecoderBF16(cfg, W))
    ch = R.FChain(cfg, W, B, "bf16")
    mine = np.stack([ch.decode(lat[f])["pcm"] for f in range(nf)])
    price, agreement = _snr(r32, r16), _snr(r16, mine)
    print(f"bf16 model vs fp32 oracle {price:.1f} dB; format chain vs the oracle's model {agreement:.1f} dB")
    assert 38.0 < price < 50.0
    assert agreement > price


# ---- seeded defects ---------------------------------------------------------------------------------------------------------
def _moved(cfg, W, fmt, scales, fn, kw, out, site, mutate, rounding_only=False, wrong_kw=None, cols=None):
    """how far the defect moves output `out` of the launch out of the GPU test's bounded, rounded interval, in units of
    that bound (inf: an e4m3 code outside the interval's neighbours, or a non-finite value)"""
    com = dict(cfg=cfg, W=W, fmt=fmt)
    y64, e32 = R.fstage_e32(fn, {**com, **kw})
    tol = FACTOR * e32[out]
    if cols is not None:  # an e4m3 GEMM: the extra terms of the GPU test's bound
        first = y64[next(iter(y64))]
        tol = tol + R.f8_extra(cfg, W, site, cols, scales, first.reshape(cols.shape[:-1] + (-1,))).reshape(first.shape)
    kind, k = R.out_kind(fmt, site) if out != "raw" else ("bf16", None)
    if site in ("q", "pcm"):
        kind, k = "f32", None
    yinv = None if k is None else R.yinv_of(scales, k)
    pre = y64[out] if rounding_only else fn(**{**com, **kw, **(wrong_kw or {})}, **({} if wrong_kw else dict(mutate=mutate)))[out]
    got = R.out_round(pre, kind, yinv, mutate if rounding_only else None)
    return R.ratio_of(got, y64[out], tol, kind, yinv)


def _cols(fmt, cur, prev, site):
    """the operand rows of an fp8 launch, as the GPU test hands them to f8_extra; None for a bf16 GEMM"""
    if fmt != "fp8" or site not in R.SC_IN:
        return None
    kind, i = site
    if kind == "convtr":
        src = "seanet0" if i == 1 else f"seanet{3 * i - 3}"
        xx = np.concatenate([prev[src][:, -1:], cur[src]], axis=1)
        return np.concatenate([xx[:, 1:], xx[:, :-1]], axis=-1)
    if kind == "res_a":
        return R._im2col(np.concatenate([prev[f"seanet_c{i}"][:, -2:], cur[f"seanet_c{i}"]], axis=1), 3)
    return cur[f"seanet_h{i}"]


def _conv_kw(cur, prev, stage, i, scales):
    """(function, keyword arguments, site, output) of a SEANet launch on the chain's taps"""
    tl = lambda name, n: prev[name][:, -n:]  # noqa: E731
    src = "seanet0" if i == 1 else f"seanet{3 * i - 3}"
    if stage == "S0":
        return R.fstage_S0, dict(x=cur["dec_tr"], tail=tl("dec_tr", 6), scales=scales), ("conv0",), "a0"
    if stage == "Cv":
        return R.fstage_Cv, dict(i=i, x=cur[src], tail=tl(src, 1), scales=scales), ("convtr", i), "elu"
    if stage == "Ra":
        return R.fstage_Ra, dict(i=i, x=cur[f"seanet_c{i}"], tail=tl(f"seanet_c{i}", 2), scales=scales), ("res_a", i), "h"
    if stage == "Rb":
        return R.fstage_Rb, dict(i=i, h=cur[f"seanet_h{i}"], skip=cur[f"seanet{3 * i - 1}"], scales=scales), ("res_b", i), "out"
    return R.fstage_L, dict(x=cur["seanet9"], tail=tl("seanet9", 2)), "pcm", "pcm"


CONV_DEFECTS = [("parity", "S0", 0), ("parity", "Cv", 2), ("parity", "Ra", 3), ("parity", "L", 0), ("seqcut", "Ra", 1),
                ("no_carry", "L", 0), ("taps_rev", "L", 0), ("skip_elu", "Rb", 1), ("skip_elu", "Rb", 3),
                ("no_bias2", "Rb", 2), ("elu_twice", "Cv", 1), ("elu_twice", "Ra", 2),
                ("sc_in_next", "Cv", 2), ("sc_in_next", "Cv", 3), ("tensor_scale", "Cv", 1), ("tensor_scale", "Ra", 2),
                ("tensor_scale", "Rb", 3), ("no_yinv", "S0", 0), ("no_yinv", "Ra", 2), ("no_yinv", "Rb", 1), ("trunc", "Rb", 3),
                ("trunc", "S0", 0)]


def _applies(fmt, mutate, stage):
    """the bf16 codec has no scales; conv0's output is e4m3 on the fp8 codec, so it cannot be truncated to bf16"""
    if fmt == "bf16":
        return mutate not in ("sc_in_next", "tensor_scale", "no_yinv")
    return not (mutate == "trunc" and stage == "S0")


@pytest.mark.parametrize("fmt,mutate,stage,i", [(f, *d) for d in CONV_DEFECTS for f in R.FMTS if _applies(f, d[0], d[1])],
                         ids=lambda v: str(v))
def test_seeded_conv_defects_reach_four_times_the_bound(fmt, mutate, stage, i):
    sc = ref_scales("nf64") if fmt == "fp8" else None
    cfg, W, fr = _frames("nf64", fmt, 3, 2, sc)
    fn, kw, site, out = _conv_kw(fr[1], fr[0], stage, i, sc)
    moved = _moved(cfg, W, fmt, sc, fn, kw, out, site, mutate, rounding_only=mutate in ("no_yinv", "trunc"),
                   cols=_cols(fmt, fr[1], fr[0], site))
    print(f"{fmt} {stage}{i or ''} {mutate}: {moved:.3g} x the bound")
    assert moved >= 4


def test_e4m3_wrap_shows_on_the_saturating_case():
    cfg, W = R.codec_weights("nf64")
    sc = ref_scales("nf64")
    cfg, W, fr = _frames("nf64", "fp8", 3, 3, sc, scale=6.0, seed=seed_of("nf64", "fp8", 3, (), ("sat",)))
    hit = 0
    for f in (1, 2):
        for stage, i in (("S0", 0), ("Cv", 1), ("Ra", 1), ("Rb", 1), ("Cv", 2), ("Ra", 2), ("Rb", 2), ("Cv", 3), ("Ra", 3)):
            fn, kw, site, out = _conv_kw(fr[f], fr[f - 1], stage, i, sc)
            kind, k = R.out_kind("fp8", site)
            if kind != "e4m3":
                continue
            pre = fn(cfg=cfg, W=W, fmt="fp8", **kw)[out]
            if (np.abs(pre) * float(R.yinv_of(sc, k)) >= 480.0).any():  # past e4m3's top by a whole step: no code is near
                hit += 1
                assert _moved(cfg, W, "fp8", sc, fn, kw, out, site, "wrap", rounding_only=True,
                              cols=_cols("fp8", fr[f], fr[f - 1], site)) >= 4, (stage, i)
    assert hit > 0, "no output of the reference chain passes e4m3's top by a step: scale the latents further"


TR_DEFECTS = [("up_swap", "P"), ("no_mean", "P"), ("rope_ring", "Q"), ("ln_s_unrounded", "Q"), ("window", "A"), ("k_layer0", "A"),
              ("no_ls", "B"), ("tanh_gelu", "C"), ("ln_s_unrounded", "C"), ("no_ls", "D"), ("trunc", "D")]


@pytest.mark.parametrize("mutate,stage", TR_DEFECTS, ids=lambda v: str(v))
def test_seeded_transformer_defects_reach_four_times_the_bound(mutate, stage):
    """the transformer is the same launches in both formats: judged on the bf16 chain of `nf64x2`, last layer, frame 5 (the
    ring has wrapped, so `rope_ring` shows)"""
    cfg, W, fr = _frames("nf64x2", "bf16", 3, 6)
    cur, prev, l = fr[5], fr[4], 1
    pos0 = cur["pos0"]
    pos = pos0[:, None] + np.arange(16)[None, :]
    wrong = None
    if stage == "P":
        fn, kw, out, site = R.fstage_P, dict(lat=cur["latent"], lat_prev=prev["latent"], live=np.ones(3, bool)), "upsample", ("p",)
    elif stage == "Q":
        fn, kw, out, site = R.fstage_Q, dict(l=l, x=cur["tr_in1"], pos=pos), "q", "q"
    elif stage == "A":
        fn, kw, out, site = R.fstage_A, dict(q=cur["tr_q1"], K=cur["tr_k1"], V=cur["tr_v1"], pos0=pos0), "attn", ("a",)
        if mutate == "k_layer0":
            wrong = dict(K=cur["tr_k0"])
    elif stage == "B":
        fn, kw, out, site = R.fstage_B, dict(l=l, attn=cur["tr_attn1"], x=cur["tr_in1"]), "resid", ("out", l)
    elif stage == "C":
        fn, kw, out, site = R.fstage_C, dict(l=l, resid=cur["tr_resid1"]), "ff", ("ff1", l)
    else:
        fn, kw, out, site = R.fstage_D, dict(l=l, ff=cur["tr_ff1"], resid=cur["tr_resid1"]), "out", ("ff2", l)
    moved = _moved(cfg, W, "bf16", None, fn, kw, out, site, mutate, rounding_only=mutate == "trunc", wrong_kw=wrong)
    print(f"{stage} {mutate}: {moved:.3g} x the bound")
    assert moved >= 4


def test_reference_calibration_and_saturation():
    """the reference's own calibration gives one positive scale per used index and 1 elsewhere; with the latents of the GPU
    test's saturating case the reference chain saturates at least one element of a SEANet tap"""
    cfg, W = R.codec_weights("nf64")
    sc = ref_scales("nf64")
    assert all(0 < sc[k] < 1 for k in R.SC_USED) and all(sc[k] == 1 for k in range(16) if k not in R.SC_USED)
    assert sorted(R.SCALE_TAP) == R.SC_USED
    _, _, fr = _frames("nf64", "fp8", 3, 3, sc, scale=6.0, seed=seed_of("nf64", "fp8", 3, (), ("sat",)))
    assert sum(int((np.abs(t[n]) == 448.0).sum()) for t in fr for n in R.SCALE_TAP.values()) > 0


# ---- one rounding model ------------------------------------------------------------------------------------------------
def _edge_values():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal(4096) * 3, rng.standard_normal(4096) * 300, rng.standard_normal(1024) * 1e-3,
                        [0.0, -0.0, 1.0, 1.00390625, 1.001953125, 447.9, 448.0, 463.9, 464.0, 480.0, 1e4, -1e4, 2.0 ** -9, 2.0 ** -10,
                         1.5 * 2.0 ** -10, 2.0 ** -6, 0.0019, 65504.0, 1e-30]])
    return x.astype(np.float32)


def test_the_reference_roundings_are_the_shared_ones():
    """mimi_ref's bf16 / e4m3 / weight quantisation against gemm_ref.bf16_round, codec_ref.e4m3 and
    codec_ref.quant_weight_f8, bit for bit, on random and edge inputs and on every fp8 weight site"""
    import torch

    import codec_ref as CR
    from gemm_ref import bf16_round

    x = _edge_values()
    t = torch.from_numpy(x)
    assert np.array_equal(R.bf16(x), bf16_round(t).numpy())
    assert np.array_equal(R.e4m3(x), CR.e4m3(t).numpy())
    assert np.array_equal(R.e4m3(x), t.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).to(torch.float64).numpy())
    assert R.is_e4m3(R.e4m3(x)) and R.is_bf16(R.bf16(x))
    cfg, W = R.codec_weights("nf64")
    for site in R.SC_IN:
        codes, _, ws = R.site_weights(cfg, W, site, "fp8")
        deq, scale = CR.quant_weight_f8(torch.from_numpy(R.site_weights(cfg, W, site, "f32")[0]))
        assert np.array_equal(ws.astype(np.float64), scale.numpy()), site
        assert np.array_equal((codes * ws.astype(np.float64)[:, None]).astype(np.float32).astype(np.float64), deq.numpy()), site
    for site in (("qkv", 0), ("ff2", 0), ("conv0",), ("convtr", 2)):
        assert np.array_equal(R.site_weights(cfg, W, site, "bf16")[0], bf16_round(torch.from_numpy(R.site_weights(cfg, W, site, "f32")[0])).numpy())


def test_fast_fp8_bound_is_codec_refs():
    """f8_bound_codes never lies below codec_ref.f8_mfma_bound and exceeds it by at most 1 + K 2^-22"""
    import torch

    import codec_ref as CR

    rng = np.random.default_rng(9)
    grid = CR.e4m3_grid().numpy()
    for M, N, K, xs in ((33, 32, 64, 0.0071), (16, 48, 256, 1.0), (7, 16, 32, 3e-4)):
        cx, cw = rng.choice(grid, (M, K)), rng.choice(grid, (N, K))
        cx[0] = 0.0
        cx[1, 8:] = 0.0
        ws = (rng.random(N) * 0.01 + 1e-4).astype(np.float32)
        s = ws.astype(np.float64) * xs
        ref = CR.f8_mfma_bound(torch.from_numpy(cx * xs), torch.from_numpy(cw * ws.astype(np.float64)[:, None]), torch.from_numpy(s), M=M).numpy()
        fast = R.f8_bound_codes(cx, cw, s)
        assert (fast >= ref).all() and (fast <= ref * (1 + K * 2.0 ** -22) + 1e-300).all(), (M, N, K)
