"""Pins the split-bf16 model of tests/mimi_ref.py (`split=""` on the stage functions, `_mms`, `_ln_mm`) and proves that the
bounds of tests/test_gpu_codec_split_matrix.py discriminate.  No GPU.  The stage inputs are the taps of the reference's own
float32 split chain (`Chain(.., split="", split_res=(1,))`) on 6 frames of seeded latents, for the configurations ("nf64",
"nf64x2") and batch sizes (1, 3, 5) the GPU cases use.

1. THE MODE'S PROMISE, from the reference alone.  For every GEMM stage of every frame,
   |y64s - y64| <= 2^-14 scale (`mimi_ref.split_scale`): y64s the float64 evaluation of the split formulas, y64 the fp32
   model's.  With |v - hi| <= 2^-8 |v| and |(v - hi) - lo| <= 2^-16 |v| each of the three dropped terms wl xl,
   (w - wh - wl) x and w (x - xh - xl) is at most 2^-16 |w| |x|, their sum below 2^-14 |w| |x|.  Worst observed ratio per
   stage, over both configurations, the three batch sizes and all frames (1 = the promise):
     Q 0.034   B 0.031   C 0.035   D 0.036   S0 0.031   C1 0.018   C2 0.026   C3 0.037
     Ra1 0.019   Rb1 0.051   Ra2 0.033   Rb2 0.078   Ra3 0.035   Rb3 0.135
   i.e. the products err at about 2^-19 of their scale (random signs), 7 to 50 times inside the promise.

2. THE +ln FOLD'S OWN SHARE.  A split +ln site subtracts mu * ln_s with ln_s summed from the fp32 image while it multiplies
   by hi + lo, which leaves rs |mu| |sum_k (w_k - wh_k - wl_k)|.  Measured on these taps (B = 3, all frames): at most 2.2e-3
   of the promise's 2^-14 scale and 0.09 of the observed max |y64s - y64| at Q, 2.4e-3 and 0.09 at C (|w - wh - wl| <=
   2^-17 |w| with random signs).  The term is small, a tenth of the product's own split error and 400 times inside the
   promise: nothing is changed in the engine, ln_s stays the fp32 codec's.

3. SEEDED DEFECTS (`mimi_ref.SPLIT_MUTANTS`), each on the smallest case the GPU matrix runs for its stage (B = 1, frame 1).
   Each listed (defect, stage) moves the float64 split result by at least 32 E32s, 4 times the GPU bound of 8 E32s; the
   32 is a condition that keeps the GPU bound meaningful, not a measurement:
     no_wlo, no_xlo   every GEMM stage (Q, B, C, D, T, S0, C1..C3, Ra1, Rb1): a product at 2^-9 instead of 2^-17
     lo_of_x_trunc    every GEMM stage: half of the elements get xl from a hi one bf16 ulp off, an error of 2^-8 |x| there
     lns_hi           Q, C and T: ln_s off by sum_k wl, times mu rs
   NOT detectable by the bound, and not listed as detected:
     fp32_w           a site on the fp32 matrix (the fp32 kernel): it moves a stage by |y64 - y64s|, which is 2.5 .. 24 E32s
                      on these taps: the split model and the fp32 model are closer to each other than 32 E32s, at T and S0
                      closer than the GPU bound itself.  No bound on values can tell the two kernels apart; the profiler's
                      "+split" label at every site is what does (test_gpu_codec_split_matrix.check_kernels).

4. AGREEMENT with the single-GEMM reference: the split product equals `gemm_ref.gemm_ref(.., wfmt=3)` on the hi / lo images
   and fold vectors of the reference, on conv0's k7 shape (with the halo from the previous frame) and on linear1's +ln shape."""

import numpy as np
import pytest
import torch

import gemm_ref as G
import mimi_ref as R

GPU_FACTOR = 8  # test_gpu_codec_split_matrix.FACTOR
MUTANT_FACTOR = 4 * GPU_FACTOR
NAMES = ("nf64", "nf64x2")
BATCHES = (1, 3, 5)
FRAMES = 6
GEMM_STAGES = ("Q", "B", "C", "D", "S0", "C1", "C2", "C3", "Ra1", "Rb1", "Ra2", "Rb2", "Ra3", "Rb3")
PROMISE_WORST = {}
MUTANT_RATIOS = {}
_FRAMES = {}


def frames_of(name, B):
    """the taps of 6 frames of the float32 split chain (stage 1's block as the unfused pair, as the engine runs it), plus the
    taps an engine with `fuse_res` 0 adds: the ELU'd copies and hidden activations of stages 2 and 3"""
    if (name, B) not in _FRAMES:
        cfg, W = R.codec_weights(name)
        chain = R.Chain(cfg, W, B, np.float32, split="", split_res=(1,))
        frames = []
        for lat in R.seeded_latents(cfg, FRAMES, B, 200 + B):
            t = chain.decode(lat)
            for i in (1, 2, 3):
                c = f"seanet_c{i}"
                t.setdefault(c, R._elu(t[f"seanet{3 * i - 1}"], False))
                tail = np.zeros_like(t[c][:, :2]) if not frames else frames[-1][c][:, -2:]
                t[f"seanet_h{i}"] = R.stage_Ra(cfg, W, i, t[c], tail, np.float32, split="")
            frames.append(t)
        _FRAMES[(name, B)] = frames
    return _FRAMES[(name, B)]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", NAMES)
def test_split_model_keeps_the_promise(name, B):
    """|y64s - y64| <= 2^-14 scale for every GEMM stage of every frame, on the input the stage consumed"""
    cfg, W = R.codec_weights(name)
    frames = frames_of(name, B)
    for f in range(FRAMES):
        for stage in GEMM_STAGES:
            inputs = R.split_inputs(stage, cfg, W, frames, f)
            y64s, y64 = R.SSTAGES[stage](**inputs, split=""), R.SSTAGES[stage](**inputs)
            scale = R.split_scale(stage, inputs)
            assert scale.shape == y64.shape and (scale > 0).all(), stage
            ratio = float((np.abs(y64s - y64) / (R.PROMISE * scale)).max())
            PROMISE_WORST[stage] = max(PROMISE_WORST.get(stage, 0.0), ratio)
            assert 0 < ratio <= 1, (name, B, f, stage, ratio)
    print(f"  {name} B={B}: worst |y64s - y64| / (2^-14 scale):", {k: round(v, 3) for k, v in PROMISE_WORST.items()})


@pytest.mark.parametrize("name", NAMES)
def test_fold_vector_share(name):
    """rs |mu| |sum_k (w - wh - wl)| of the +ln sites Q and C beside the promise's 2^-14 scale and the observed split error:
    a small share (docstring, 2), so `ln_s` stays summed from the fp32 image"""
    cfg, W = R.codec_weights(name)
    frames = frames_of(name, 3)
    L = cfg.mimi.transformer.num_layers
    for stage, kind, key in (("Q", "qkv", "x"), ("C", "ff1", "resid")):
        worst_p = worst_o = 0.0
        for f in range(FRAMES):
            inputs = R.split_inputs(stage, cfg, W, frames, f)
            x = np.asarray(inputs[key], np.float64)
            wf = R.fold_image(cfg, W, (kind, L - 1), np.float64)
            wh, wl = R._wsplit(wf)
            mu, rs = R._stats(x, False)
            term = (rs * np.abs(mu))[..., 0][..., None] * np.abs((wf - wh - wl).sum(axis=1))[None, None, :]  # [B, T, N]
            scale = R.split_scale("C", inputs) if stage == "C" else None
            if stage == "Q":  # before RoPE, which only mixes pairs: compare with the unrotated scale
                scale = (rs.reshape(-1, 1) * (R._mag(x, wf) + np.abs(mu).reshape(-1, 1) * np.abs(wf).sum(axis=1)[None, :])).reshape(term.shape)
            seen = np.abs(R.SSTAGES[stage](**inputs, split="") - R.SSTAGES[stage](**inputs)).max()
            worst_p = max(worst_p, float((term / (R.PROMISE * scale)).max()))
            worst_o = max(worst_o, float(term.max() / seen))
        print(f"  {name} {stage}: fold term <= {worst_p:.2e} of 2^-14 scale, <= {worst_o:.2e} of the observed max |y64s - y64|")
        # |w - wh - wl| <= 2^-17 |w| bounds the term by 2^-3 of the promise even with every sign aligned; it must also stay
        # below the split error of the product itself (the issue's condition for leaving the engine's ln_s alone)
        assert worst_p <= 2.0 ** -3 and worst_o < 1, (stage, worst_p, worst_o)


ALL = [("nf64", s) for s in ("Q", "B", "C", "D", "S0", "C1", "C2", "C3", "Ra1", "Rb1")] + [("nf64x2", "T")]
DESIGNATED = {
    "no_wlo": ALL,
    "no_xlo": ALL,
    "lo_of_x_trunc": ALL,
    "lns_hi": [("nf64", "Q"), ("nf64", "C"), ("nf64x2", "T")],
}
NOT_DETECTED = {"fp32_w": ALL}  # docstring, 3


def moved_by(mutant, name, stage, B=1, f=1):
    cfg, W = R.codec_weights(name)
    inputs = R.split_inputs(stage, cfg, W, frames_of(name, B), f)
    y64s, e32s = R.split_e32(stage, inputs)
    moved = float(np.abs(R.SSTAGES[stage](**inputs, split=mutant) - y64s).max())
    MUTANT_RATIOS[(mutant, name, stage)] = (e32s, moved)
    print(f"mutant {mutant} {name} {stage}: E32s {e32s:.2e}, moved {moved:.2e} = {moved / e32s:.3g} x E32s")
    return moved, e32s


def test_every_mutant_is_accounted_for():
    assert sorted(list(DESIGNATED) + list(NOT_DETECTED)) == sorted(R.SPLIT_MUTANTS)


@pytest.mark.parametrize("mutant,name,stage", [(m, *d) for m, ds in sorted(DESIGNATED.items()) for d in ds])
def test_mutant_moves_the_result(mutant, name, stage):
    moved, e32s = moved_by(mutant, name, stage)
    assert moved >= MUTANT_FACTOR * e32s, (moved, e32s, moved / e32s)


def test_fp32_fallback_is_inside_the_bounds():
    """`fp32_w`, a site that silently runs on the fp32 matrix: the bounds on values do NOT catch it.  It moves every stage by
    |y64 - y64s|, under 32 E32s everywhere on these taps (measured 2.5 .. 24 E32s) and inside the promise by construction, so it
    is not listed as detected; the GPU tests catch it by the profiler's "+split" label at every site instead"""
    for name, stage in NOT_DETECTED["fp32_w"]:
        moved, e32s = moved_by("fp32_w", name, stage)
        assert 0 < moved < MUTANT_FACTOR * e32s, (name, stage, moved / e32s)  # if this fails the defect IS detectable: list it


def test_split_product_is_gemm_ref_wfmt3():
    cfg, W = R.codec_weights("nf64")
    frames = frames_of("nf64", 3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    # conv0: k7, the halo rows from the previous frame
    cur, prev = frames[2]["dec_tr"], frames[1]["dec_tr"]
    B, T, C = cur.shape
    w, b = R.params(cfg, W, np.float64).conv(f"mimi.decoder.model.{R._layer_of(cfg, 'conv', 0)[0]}.conv")
    wh, wl = R._wsplit(w)
    want, _ = G.gemm_ref(t(cur.reshape(B * T, C)), t(wh), M=B * T, ntaps=7, T=T, halo=6, halo_mode=0, x_prev=t(prev.reshape(B * T, C)),
                         wfmt=3, w_lo=t(wl), bias=t(b), act=G.ACT_ELU)
    got = R.stage_S0(cfg, W, cur, prev[:, -6:], split="")
    assert np.abs(got.reshape(B * T, -1) - want.numpy()).max() <= 1e-12 * np.abs(got).max()
    # linear1: the +ln fold with ln_s from the fp32 image
    x = frames[2]["tr_resid"]
    wf = R.fold_image(cfg, W, ("ff1", 0), np.float64)
    fh, fl = R._wsplit(wf)
    P = R.params(cfg, W, np.float64)
    ln_c = P.vec(R._lp(0) + ".linear1.weight") @ P.vec(R._lp(0) + ".norm2.bias")
    want, _ = G.gemm_ref(t(x.reshape(B * T, C)), t(fh), M=B * T, wfmt=3, w_lo=t(fl), pre=G.PRE_LNFOLD, ln_s=t(wf.sum(axis=1)), ln_c=t(ln_c),
                         act=G.ACT_GELU)
    got = R.stage_C(cfg, W, x, alt=True, split="")  # gemm_ref's variance is the one-pass form
    assert np.abs(got.reshape(B * T, -1) - want.numpy()).max() <= 1e-12 * np.abs(got).max()
    # and the parts are what the packer's arithmetic gives: hi = bf16(w), lo = bf16(w - hi), bit for bit gemm_ref.bf16_round
    w32 = w.astype(np.float32)
    assert np.array_equal(wh, G.bf16_round(torch.from_numpy(w32)).numpy())
    assert np.array_equal(wl, G.bf16_round(torch.from_numpy((w32.astype(np.float64) - wh).astype(np.float32))).numpy())


def test_split_chain_is_the_stages_chained():
    """the split `Chain` hands each stage the taps the stage functions are judged on: its float64 PCM is reproduced by
    walking the stages on its own taps"""
    cfg, W = R.codec_weights("nf64")
    chain = R.Chain(cfg, W, 2, split="", split_res=(1,))
    frames = [chain.decode(lat) for lat in R.seeded_latents(cfg, 2, 2, 11)]
    for stage, tap in (("S0", "seanet0"), ("D", "dec_tr"), ("Rb1", "seanet3")):
        inputs = R.split_inputs(stage, cfg, W, [dict(fr, seanet_h1=None) for fr in frames], 1)
        if stage == "Rb1":
            inputs["h"] = R.stage_Ra(cfg, W, 1, frames[1]["seanet_c1"], frames[0]["seanet_c1"][:, -2:], split="")
        assert np.array_equal(R.SSTAGES[stage](**inputs, split=""), frames[1][tap]), stage
    assert np.array_equal(R.stage_R(cfg, W, 2, frames[1]["seanet5"], frames[0]["seanet5"][:, -2:]), frames[1]["seanet6"])  # fp32 block


def test_zz_tables():
    print("\nsplit model: worst |y64s - y64| / (2^-14 scale) per stage")
    print("  " + "   ".join(f"{k} {v:.3f}" for k, v in PROMISE_WORST.items()))
    print(f"seeded defects of the split product (required: >= {MUTANT_FACTOR} x E32s; fp32_w: not detectable)")
    for (m, name, stage), (e, moved) in sorted(MUTANT_RATIOS.items()):
        print(f"  {m:14s} {name:7s} {stage:4s} E32s {e:.2e}  moved {moved:.2e}  = {moved / e:9.3g} x E32s   {R.SPLIT_MUTANTS[m]}")
