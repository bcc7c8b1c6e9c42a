"""fp64 reference of the voice-prompt encoder (`ptts_encode_voice`), ONE STATELESS FUNCTION PER STAGE, for
tests/test_voice_reference_cpu.py and tests/test_gpu_voice_matrix.py.  Plain numpy, no GPU.  The arithmetic pieces, the
weight matrices and the meaning of E32 are those of tests/mimi_ref.py.

A stage is what lies between two buffers the engine can read back (`Engine.debug_read_encoder` after an `encode_voice` with
the option `debug_taps`): it takes the stage's input tap and returns its output tap, so a kernel is judged on the very input
it consumed.  Formulas are those of `oracle.np_oracle.VoiceEncoder` and of the reference lines it cites (`mimi.py:96-119`,
`tts_model.py:379-388`, `seanet.py:33-41,63-104`, `conv.py:22-33,84-115`, `resample.py:7-29`, `transformer.py:22-29,63-75,
135-158`, `mimi_transformer.py:39-54`, `rope.py:7-58`), evaluated in `dtype` from the float32 operands.

Layout: one sequence, activations [T, C] (time-major, channels last), as the engine's taps.  The taps hold what the NEXT
kernel reads.  RAW: `conv0_raw`, `down<i>_raw` (the residual blocks' skip inputs), `final`, `tr_*`, `enc_tr`, `latent`, `cond`.
ELU'd by their producer: `conv0`, `rb<i>`, `se<i>` (the block's output; its raw sum is stored nowhere), `down<i>`.

  stage        input taps                 output tap            what it computes
  E0 / E0e     the audio, n samples       conv0_raw / conv0     zero tail up to a whole frame, k7 conv, 6 zeros on the left
  Ra<i>        conv0 | down<i-1>          rb<i>                 ELU(k3 conv of the ELU'd input), 2 zeros on the left
  Rb<i>        rb<i>, conv0_raw |         se<i>                 ELU(raw skip + 1x1 conv)
               down<i-1>_raw
  Dn<i>/Dn<i>e se<i>                      down<i>_raw / down<i> kernel 2r, stride r, r zeros on the left; r = 4, 5, 6 for i = 1, 2, 3
  F            down3                      final                 k3 conv, 2 zeros on the left
  Q            final                      tr_qkv                one-layer configurations: LayerNorm, in_proj, RoPE of q and k: what
                                                                the attention kernel reads, [q | k | v] per position
  A            final                      tr_attn               one-layer configurations: the same, then attention
  B            tr_attn, final             tr_resid              x + layer_scale_1 * out_proj
  C            tr_resid                   tr_ff                 GELU(linear1(norm2(x))) of the last layer
  D            tr_ff, tr_resid            enc_tr                x + layer_scale_2 * linear2
  T            final                      enc_tr                the whole transformer
  DS           enc_tr                     latent                kernel 32, stride 16, the first position 16 times on the left, no bias
  SP           latent                     cond                  the speaker projection

The transformer is the non-streaming form: positions 0 .. M2 - 1, keys 0 <= q - k < context, the RoPE angle the FLOAT32
product freq * pos (as the model defines it), sine, cosine and everything after them in `dtype`.  freq is the correctly
rounded float32 exp (`mimi_ref._rope`): one ulp in a frequency is 4e-6 rad at position 271, more than stage Q's E32.

`stage_e32(stage, inputs) -> (y64, E32)`, `chain_e32(cfg, W, audio)`: E32 is the largest max|y32 - y64| over the float32
evaluations `mimi_ref.F32_VARIANTS` ("np" and "seq" summation orders, both elementwise forms).  It comes from the reference
alone.  MUTANTS are seeded defects: each moves its designated stage by >= 32 E32 (tests/test_voice_reference_cpu.py), 4 x
the GPU bound of 8 E32."""

from __future__ import annotations

import math
import zlib

import numpy as np

import mimi_ref as R
from mimi_ref import F32, F64, F32_VARIANTS, _elu, _gelu, _in, _layer_norm, _mm, _rope, codec_weights, params  # noqa: F401
from pocket_tts_amd.weights import seanet_encoder_layers

MUTANTS = {
    "tail_repeat": "the tail padded by repeating the last sample instead of zeros",
    "ctx_2r1": "left context 2r - 1 instead of r on a strided conv",
    "phase": "the stride phase off by one input row",
    "ratios_rev": "the ratios applied as 6, 5, 4",
    "skip_elu": "the resblock skip taken from the ELU'd copy instead of the raw value",
    "elu_twice": "ELU applied twice on the operand",
    "ds_zero": "the downsample zero-padded instead of replicate-padded",
    "ds_swap": "the downsample's two half-kernels exchanged",
    "window": "the window one key too long",
    "rope_pos1": "RoPE started at position 1 (attention scores depend on q - k only, so it shows in stage Q, not in A or T)",
    "no_ls": "the layer scale left out of a residual add",
    "tanh_gelu": "the tanh approximation of GELU instead of the erf form",
    "proj_prev": "the speaker projection applied to frame t - 1",
}

CONFIG_NAMES = R.CONFIG_NAMES
_TR = "mimi.encoder_transformer.transformer.layers"


def _check(mutate, allowed):
    assert mutate is None or mutate in allowed, (mutate, allowed)


def _layer(cfg, kind, i):
    """(ModuleList index, cin, cout, kernel, stride) of the encoder's i-th layer of `kind` (conv: 0 first, 1 last)"""
    idx, _, cin, cout, k, stride = [l for l in seanet_encoder_layers(cfg) if l[1] == kind][i]
    return idx, cin, cout, k, stride


def _conv(x, w, b, K, stride, left, n_out, order, replicate=False):
    """out[t] = sum_k x[t * stride - left + k] w[:, k] + b for t < n_out; rows before the start are zero, or row 0 with
    `replicate`; rows past the end are zero.  x [T, C], w [N, K * C] with column k * C + c"""
    T = x.shape[0]
    idx = np.arange(n_out)[:, None] * stride - left + np.arange(K)[None, :]
    ok = (idx < T) & ((idx >= 0) | replicate)
    cols = x[np.clip(idx, 0, T - 1)] * ok[:, :, None].astype(x.dtype)
    return _mm(cols.reshape(n_out, K * x.shape[1]), w, b, order)


def padded_audio(cfg, audio, mutate=None):
    """the samples behind a zero tail up to a whole number of frames (`pad_for_conv1d`)"""
    a = np.asarray(audio).reshape(-1)
    pad = (-len(a)) % cfg.frame_samples
    return np.concatenate([a, np.full(pad, a[-1] if mutate == "tail_repeat" else 0, a.dtype)])


# ---- the stages --------------------------------------------------------------------------------------------------------
def stage_E0(cfg, W, audio, act=False, dtype=F64, order="np", alt=False, mutate=None):
    _check(mutate, ("tail_repeat",))
    P = params(cfg, W, dtype)
    idx, _, _, K, _ = _layer(cfg, "conv", 0)
    w, b = P.conv(f"mimi.encoder.model.{idx}.conv")
    x = _in(padded_audio(cfg, audio, mutate), dtype)[:, None]
    y = _conv(x, w, b, K, 1, K - 1, len(x), order)
    return _elu(y, alt) if act else y


def stage_Ra(cfg, W, i, x, dtype=F64, order="np", alt=False, mutate=None):
    _check(mutate, ("elu_twice",))
    P = params(cfg, W, dtype)
    idx, _, _, K, _ = _layer(cfg, "res", i - 1)
    w, b = P.conv(f"mimi.encoder.model.{idx}.block.1.conv")
    x = _in(x, dtype)
    if mutate == "elu_twice":
        x = _elu(x, alt)
    return _elu(_conv(x, w, b, K, 1, K - 1, len(x), order), alt)


def stage_Rb(cfg, W, i, rb, skip, dtype=F64, order="np", alt=False, mutate=None):
    _check(mutate, ("skip_elu",))
    P = params(cfg, W, dtype)
    idx = _layer(cfg, "res", i - 1)[0]
    w, b = P.conv(f"mimi.encoder.model.{idx}.block.3.conv")
    skip = _in(skip, dtype)
    if mutate == "skip_elu":
        skip = _elu(skip, alt)
    return _elu(skip + _mm(_in(rb, dtype), w, b, order), alt)


def stage_Dn(cfg, W, i, x, act=False, dtype=F64, order="np", alt=False, mutate=None):
    _check(mutate, ("ctx_2r1", "phase", "ratios_rev", "elu_twice"))
    P = params(cfg, W, dtype)
    idx, _, _, K, r = _layer(cfg, "down", i - 1)
    assert K == 2 * r
    w, b = P.conv(f"mimi.encoder.model.{idx}.conv")
    x = _in(x, dtype)
    n_out = len(x) // r
    stride, left = r, r
    if mutate == "ctx_2r1":
        left = 2 * r - 1
    elif mutate == "phase":
        left = r - 1
    elif mutate == "ratios_rev":
        stride = left = _layer(cfg, "down", 3 - i)[4]
    elif mutate == "elu_twice":
        x = _elu(x, alt)
    y = _conv(x, w, b, K, stride, left, n_out, order)
    return _elu(y, alt) if act else y


def stage_F(cfg, W, x, dtype=F64, order="np", alt=False, mutate=None):
    _check(mutate, ("elu_twice",))
    P = params(cfg, W, dtype)
    idx, _, _, K, _ = _layer(cfg, "conv", 1)
    w, b = P.conv(f"mimi.encoder.model.{idx}.conv")
    x = _in(x, dtype)
    if mutate == "elu_twice":
        x = _elu(x, alt)
    return _conv(x, w, b, K, 1, K - 1, len(x), order)


def _transformer(cfg, W, x, dtype, order, alt, mutate):
    """the encoder transformer on the whole sequence x [T, C] at once -> the last layer's taps"""
    P = params(cfg, W, dtype)
    tr = cfg.mimi.transformer
    H, Dh, ctx = tr.num_heads, tr.d_model // tr.num_heads, tr.context
    dt = np.dtype(dtype).type
    x = _in(x, dtype)[None]  # [1, T, C]
    T, C = x.shape[1], x.shape[2]
    pos = np.arange(T)[None, :]
    rp = pos + 1 if mutate == "rope_pos1" else pos
    delta = pos[0][:, None] - pos[0][None, :]
    mask = (delta >= 0) & (delta < ctx + (1 if mutate == "window" else 0))
    for l in range(tr.num_layers):
        p = f"{_TR}.{l}"
        h = _layer_norm(x, P.vec(p + ".norm1.weight"), P.vec(p + ".norm1.bias"), alt)
        qkv = _mm(h, P.vec(p + ".self_attn.in_proj.weight"), None, order).reshape(1, T, 3, H, Dh)
        q = _rope(qkv[:, :, 0], rp, float(tr.max_period), dtype)
        k = _rope(qkv[:, :, 1], rp, float(tr.max_period), dtype)
        sc = np.einsum("bqhd,bkhd->bhqk", q, k) * dt(1.0 / math.sqrt(Dh))
        sc = np.where(mask[None, None], sc, dt(-np.inf))
        sc = sc - sc.max(axis=-1, keepdims=True)
        pr = np.exp(sc)
        pr = pr / pr.sum(axis=-1, keepdims=True)
        ao = np.einsum("bhqk,bkhd->bqhd", pr, qkv[:, :, 2]).reshape(1, T, C)
        packed = np.concatenate([q.reshape(T, C), k.reshape(T, C), qkv[0, :, 2].reshape(T, C)], axis=1)
        resid = x + P.vec(p + ".layer_scale_1.scale") * _mm(ao, P.vec(p + ".self_attn.out_proj.weight"), None, order)
        ff = _gelu(_mm(_layer_norm(resid, P.vec(p + ".norm2.weight"), P.vec(p + ".norm2.bias"), alt),
                       P.vec(p + ".linear1.weight"), None, order))
        x = resid + P.vec(p + ".layer_scale_2.scale") * _mm(ff, P.vec(p + ".linear2.weight"), None, order)
    taps = dict(qkv=packed, attn=ao[0], resid=resid[0], ff=ff[0], out=x[0])
    assert all(v.dtype == dt for v in taps.values())
    return taps


def stage_Q(cfg, W, x, dtype=F64, order="np", alt=False, mutate=None):
    _check(mutate, ("rope_pos1",))
    assert cfg.mimi.transformer.num_layers == 1, "stage Q is defined on the one-layer configurations"
    return _transformer(cfg, W, x, dtype, order, alt, mutate)["qkv"]


def stage_A(cfg, W, x, dtype=F64, order="np", alt=False, mutate=None):
    _check(mutate, ("window",))
    assert cfg.mimi.transformer.num_layers == 1, "stage A is defined on the one-layer configurations"
    return _transformer(cfg, W, x, dtype, order, alt, mutate)["attn"]


def stage_T(cfg, W, x, dtype=F64, order="np", alt=False, mutate=None):
    _check(mutate, ("window",))
    return _transformer(cfg, W, x, dtype, order, alt, mutate)["out"]


def _last(cfg):
    return f"{_TR}.{cfg.mimi.transformer.num_layers - 1}"


def stage_B(cfg, W, attn, x, dtype=F64, order="np", alt=False, mutate=None):
    _check(mutate, ("no_ls",))
    assert cfg.mimi.transformer.num_layers == 1, "stage B's input x is the transformer's input on one layer only"
    P, p = params(cfg, W, dtype), _last(cfg)
    ls = 1 if mutate == "no_ls" else P.vec(p + ".layer_scale_1.scale")
    return _in(x, dtype) + ls * _mm(_in(attn, dtype), P.vec(p + ".self_attn.out_proj.weight"), None, order)


def stage_C(cfg, W, resid, dtype=F64, order="np", alt=False, mutate=None):
    _check(mutate, ("tanh_gelu",))
    P, p = params(cfg, W, dtype), _last(cfg)
    h = _layer_norm(_in(resid, dtype), P.vec(p + ".norm2.weight"), P.vec(p + ".norm2.bias"), alt)
    return _gelu(_mm(h, P.vec(p + ".linear1.weight"), None, order), mutate == "tanh_gelu")


def stage_D(cfg, W, ff, resid, dtype=F64, order="np", alt=False, mutate=None):
    _check(mutate, ("no_ls",))
    P, p = params(cfg, W, dtype), _last(cfg)
    ls = 1 if mutate == "no_ls" else P.vec(p + ".layer_scale_2.scale")
    return _in(resid, dtype) + ls * _mm(_in(ff, dtype), P.vec(p + ".linear2.weight"), None, order)


def stage_DS(cfg, W, x, dtype=F64, order="np", alt=False, mutate=None):
    _check(mutate, ("ds_zero", "ds_swap"))
    P = params(cfg, W, dtype)
    s = cfg.upsample_stride
    name = "mimi.downsample.conv.conv.weight"
    w = P.get(name + "#m", lambda: (lambda v: v.transpose(0, 2, 1).reshape(v.shape[0], -1))(W[name]))
    x = _in(x, dtype)
    if mutate == "ds_swap":
        C = x.shape[1]
        w = np.ascontiguousarray(np.concatenate([w[:, s * C:], w[:, : s * C]], axis=1))
    return _conv(x, w, None, 2 * s, s, s, len(x) // s, order, replicate=mutate != "ds_zero")


def stage_SP(cfg, W, lat, dtype=F64, order="np", alt=False, mutate=None):
    _check(mutate, ("proj_prev",))
    P = params(cfg, W, dtype)
    lat = _in(lat, dtype)
    if mutate == "proj_prev":
        lat = np.concatenate([np.zeros_like(lat[:1]), lat[:-1]], axis=0)
    return _mm(lat, P.vec("flow_lm.speaker_proj_weight"), None, order)


def _bind(fn, **fixed):
    def run(cfg, W, *a, **kw):
        return fn(cfg, W, *a, **fixed, **kw)

    return run


STAGES = {"E0": stage_E0, "E0e": _bind(stage_E0, act=True), "F": stage_F, "Q": stage_Q, "A": stage_A, "B": stage_B, "C": stage_C,
          "D": stage_D, "T": stage_T, "DS": stage_DS, "SP": stage_SP}
OUTPUT_TAP = {"E0": "conv0_raw", "E0e": "conv0", "F": "final", "Q": "tr_qkv", "A": "tr_attn", "B": "tr_resid", "C": "tr_ff", "D": "enc_tr",
              "T": "enc_tr", "DS": "latent", "SP": "cond"}
for _i in (1, 2, 3):
    STAGES.update({f"Ra{_i}": _bind(stage_Ra, i=_i), f"Rb{_i}": _bind(stage_Rb, i=_i), f"Dn{_i}": _bind(stage_Dn, i=_i),
                   f"Dn{_i}e": _bind(stage_Dn, i=_i, act=True)})
    OUTPUT_TAP.update({f"Ra{_i}": f"rb{_i}", f"Rb{_i}": f"se{_i}", f"Dn{_i}": f"down{_i}_raw", f"Dn{_i}e": f"down{_i}"})
TAPS = ("audio",) + tuple(dict.fromkeys(OUTPUT_TAP.values()))


def stages_of(cfg):
    """the stages judged on a configuration: A and B need the transformer's input to be the last layer's"""
    one = cfg.mimi.transformer.num_layers == 1
    conv = ["E0", "E0e"] + [f"{s}{i}{e}" for i in (1, 2, 3) for s, e in (("Ra", ""), ("Rb", ""), ("Dn", ""), ("Dn", "e"))]
    return conv + ["F"] + (["Q", "A", "B"] if one else ["T"]) + ["C", "D", "DS", "SP"]


def stage_inputs(stage, cfg, W, taps, audio):
    """keyword arguments of `STAGES[stage]` from the taps of one encode (engine names) and the audio it was given"""
    kw = dict(cfg=cfg, W=W)
    if stage in ("E0", "E0e"):
        return dict(kw, audio=audio)
    if stage[:2] in ("Ra", "Rb", "Dn"):
        i = int(stage[2])
        if stage[:2] == "Dn":
            return dict(kw, x=taps[f"se{i}"])
        src = "conv0" if i == 1 else f"down{i - 1}"
        return dict(kw, x=taps[src]) if stage[:2] == "Ra" else dict(kw, rb=taps[f"rb{i}"], skip=taps[src + "_raw"])
    return {"F": lambda: dict(kw, x=taps["down3"]), "A": lambda: dict(kw, x=taps["final"]), "Q": lambda: dict(kw, x=taps["final"]), "T": lambda: dict(kw, x=taps["final"]),
            "B": lambda: dict(kw, attn=taps["tr_attn"], x=taps["final"]), "C": lambda: dict(kw, resid=taps["tr_resid"]),
            "D": lambda: dict(kw, ff=taps["tr_ff"], resid=taps["tr_resid"]), "DS": lambda: dict(kw, x=taps["enc_tr"]),
            "SP": lambda: dict(kw, lat=taps["latent"])}[stage]()


def stage_e32(stage, inputs):
    """-> (y64, E32) of `STAGES[stage](**inputs)`: the fp64 result and the worst float32 error of the same formulas on the
    same inputs over F32_VARIANTS.  From the reference alone; positive."""
    fn = STAGES[stage]
    y64 = fn(**inputs)
    assert y64.dtype == np.float64
    e32 = 0.0
    for order, alt in F32_VARIANTS:
        y32 = fn(**inputs, dtype=F32, order=order, alt=alt)
        assert y32.dtype == np.float32 and y32.shape == y64.shape, (stage, y32.dtype)
        e32 = max(e32, float(np.abs(y32.astype(np.float64) - y64).max()))
    assert e32 > 0, stage
    return y64, e32


# ---- the stages chained ------------------------------------------------------------------------------------------------
def encode(cfg, W, audio, dtype=F64, order="np", alt=False):
    """audio [n] -> every tap of the path (engine names), each stage fed the one before it"""
    kw = dict(dtype=dtype, order=order, alt=alt)
    t = {"audio": padded_audio(cfg, audio)}
    t["conv0_raw"] = stage_E0(cfg, W, audio, **kw)
    t["conv0"] = _elu(t["conv0_raw"], alt)
    raw, act = "conv0_raw", "conv0"
    for i in (1, 2, 3):
        t[f"rb{i}"] = stage_Ra(cfg, W, i, t[act], **kw)
        t[f"se{i}"] = stage_Rb(cfg, W, i, t[f"rb{i}"], t[raw], **kw)
        raw, act = f"down{i}_raw", f"down{i}"
        t[raw] = stage_Dn(cfg, W, i, t[f"se{i}"], **kw)
        t[act] = _elu(t[raw], alt)
    t["final"] = stage_F(cfg, W, t["down3"], **kw)
    tr = _transformer(cfg, W, t["final"], dtype, order, alt, None)
    t.update(tr_qkv=tr["qkv"], tr_attn=tr["attn"], tr_resid=tr["resid"], tr_ff=tr["ff"], enc_tr=tr["out"])
    t["latent"] = stage_DS(cfg, W, t["enc_tr"], **kw)
    t["cond"] = stage_SP(cfg, W, t["latent"], **kw)
    return t


def chain_taps_e32(cfg, W, audio):
    """-> (taps64, {tap: E32}): the fp64 chain and, per tap, the worst float32 error of the same chain over F32_VARIANTS"""
    t64 = encode(cfg, W, audio)
    e32 = {}
    for order, alt in F32_VARIANTS:
        t32 = encode(cfg, W, audio, F32, order, alt)
        for k in t64:
            if k != "audio":
                e32[k] = max(e32.get(k, 0.0), float(np.abs(t32[k].astype(np.float64) - t64[k]).max()))
    return t64, e32


def chain_e32(cfg, W, audio):
    """the whole path: -> ((latent64, E32), (cond64, E32))"""
    t64, e32 = chain_taps_e32(cfg, W, audio)
    assert e32["latent"] > 0 and e32["cond"] > 0
    return (t64["latent"], e32["latent"]), (t64["cond"], e32["cond"])


def seeded_audio(n, seed, amplitude=0.2):
    """[n] float32 ~ amplitude * N(0, 1)"""
    return (np.random.default_rng(seed).standard_normal(n) * amplitude).astype(np.float32)


# The lengths the GPU matrix runs, in samples.  A frame is 1920 samples = 16 transformer positions: the frame boundary
# (1, 1, 2 frames); 3 frames = 48 positions, above the context of 40, the golden's length; 6 frames = 96 positions, query
# blocks whose window excludes whole leading key tiles; 16 and 17 frames = one and two row tiles in the downsample and the
# speaker projection, 272 positions
FRAME = 1920
LENGTHS = (FRAME - 1, FRAME, FRAME + 1, 2 * FRAME + 700, 6 * FRAME, 16 * FRAME, 16 * FRAME + 1)


def case_audio(name, n):
    """the audio of the matrix's case (configuration, length): another seed per case"""
    return seeded_audio(n, zlib.crc32(repr((name, n)).encode()))
