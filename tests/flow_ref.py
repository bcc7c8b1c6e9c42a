"""fp64 reference of the FlowLM flow head (everything from the `flow.head` site to the end of a decode step) for
tests/test_flow_reference_cpu.py and tests/test_gpu_flow_matrix.py.  Plain numpy, no GPU.

The head as ONE operation: transformer output x [B, d_model] + LSD start point (noise) -> next latent, EOS logit and the
conditioning buffer `ce`.  Formulas are those of `oracle.np_oracle.FlowLM` (`time_embed`, `flow_net`, `decode_step`),
evaluated in `dtype` from the float32 operands the kernels consume (weights, x, noise, the float32-rounded times i / n).

  E32(case) = the larger of max|y32 - y64| over two float32 evaluations of the same formulas (two-pass LayerNorm
              variance, and the kernels' one-pass max(E[x^2] - mu^2, 0)), per output (latent, eos_logit, ce).
              One documented exception, for the logit of fewer than 16 rows: see `flow_head_e32`.

E32 is the yardstick of the GPU matrix: it is what a plain float32 evaluation of the head loses on this very case, so a
kernel that only sums in another order stays within a small multiple of it, and a kernel with a wrong constant or
formula (the MUTANTS below) does not.  It never comes from the code under test."""

from __future__ import annotations

import numpy as np

from pocket_tts_amd.config import make_config, named_config, NAMED_CONFIGS
from pocket_tts_amd.weights import generate_state_dict

# seeded defects (`mutate=`): each is one plausible slip in a kernel or in the host code of the head
MUTANTS = {
    "a": "flow LayerNorm eps 1e-5 instead of 1e-6",
    "b": "time-embedding RMSNorm eps 1e-6 instead of 1e-5",
    "c": "biased variance (ddof 0) in the time-embedding RMSNorm",
    "d": "s and t exchanged between the two time embedders",
    "e": "a row with its own count uses the step's 1 / n in the Euler update",
    "f": "a row past its count keeps integrating",
    "g": "AdaLN scale used without the 1 +",
    "h": "EOS logit taken from the un-normalised x",
}

# "tiny" everywhere except flow_dim (FDF = flow_dim / 16 column tiles, KPW = ceil(FDF / 8) k-fragments per worker wave)
FLOW_DIMS = {"F64": 64, "F192": 192, "F256": 256, "F320": 320}
CONFIG_NAMES = ("F64", "F192", "F256", "F320", "F512")
VARIANTS = ("plain", "smallvar", "smallte", "bigmean")

_CFG = {}
_WEIGHTS = {}
_CAST = {}


def flow_config(name):
    """F64 (= "tiny"): KPW 1; F192: KPW 2 with worker waves 6 and 7 idle; F256: KPW 2, all busy; F320: kpw 3, no cluster
    kernel; F512 = "en100m": KPW 4"""
    if name not in _CFG:
        _CFG[name] = named_config("en100m") if name == "F512" else make_config(**{**NAMED_CONFIGS["tiny"], "flow_dim": FLOW_DIMS[name]})
    return _CFG[name]


def flow_weights(name, variant="plain", seed=0):
    """(cfg, W): `generate_state_dict(cfg, seed)` with the variant's edits
    smallvar: input_proj x 0.01 -> rows of variance ~5e-5 enter the first block's LayerNorm, where eps decides the result
    smallte:  the time embedders' last Linear x 0.01 -> the same for the RMSNorm's eps
    bigmean:  input_proj.bias + 4 -> row mean ~4, variance ~0.4: the cancellation case of the one-pass variance"""
    key = (name, variant, seed)
    if key not in _WEIGHTS:
        cfg = flow_config(name)
        base = (name, "plain", seed)
        if base not in _WEIGHTS:
            _WEIGHTS[base] = (cfg, generate_state_dict(cfg, seed))
        W = dict(_WEIGHTS[base][1])
        p = "flow_lm.flow_net."
        if variant == "smallvar":
            for k in ("weight", "bias"):
                W[p + "input_proj." + k] = (W[p + "input_proj." + k] * np.float32(0.01)).astype(np.float32)
        elif variant == "smallte":
            for i in (0, 1):
                for k in ("weight", "bias"):
                    n = f"{p}time_embed.{i}.mlp.2.{k}"
                    W[n] = (W[n] * np.float32(0.01)).astype(np.float32)
        elif variant == "bigmean":
            W[p + "input_proj.bias"] = (W[p + "input_proj.bias"] + np.float32(4.0)).astype(np.float32)
        elif variant != "plain":
            raise KeyError(variant)
        _WEIGHTS[key] = (cfg, W)
    return _WEIGHTS[key]


def _cast(W, dtype):
    """the head's tensors of W in `dtype`, converted once per weight dict"""
    key = (id(W), np.dtype(dtype).str)
    if key not in _CAST:
        keep = ("flow_lm.flow_net.", "flow_lm.out_norm.", "flow_lm.out_eos.")
        _CAST[key] = (W, {k: np.asarray(v).astype(dtype) for k, v in W.items() if k.startswith(keep)})
    return _CAST[key][1]


def _silu(x):
    with np.errstate(over="ignore"):  # exp(-x) = inf for very negative x: x / inf = -0, the limit
        return x / (1 + np.exp(-x))


def _linear(x, w, b):
    return x @ w.T + b


def _layer_norm(x, w, b, eps, onepass):
    dt = x.dtype.type
    mu = x.mean(axis=-1, keepdims=True)
    if onepass:  # the kernels' formula (not their summation order)
        var = np.maximum((x * x).mean(axis=-1, keepdims=True) - mu * mu, dt(0))
    else:
        var = ((x - mu) * (x - mu)).mean(axis=-1, keepdims=True)
    y = (x - mu) / np.sqrt(var + dt(eps))
    return y if w is None else y * w + b


def _time_embed(P, k, t, dt, mutate):
    """TimestepEmbedder k at the scalar time t (float32-rounded, as the host hands it to the kernel) -> [flow_dim]"""
    p = f"flow_lm.flow_net.time_embed.{k}."
    args = dt(np.float32(t)) * P[p + "freqs"]
    e = np.concatenate([np.cos(args), np.sin(args)])
    h = _silu(_linear(e, P[p + "mlp.0.weight"], P[p + "mlp.0.bias"]))
    h = _linear(h, P[p + "mlp.2.weight"], P[p + "mlp.2.bias"])
    var = h.var(ddof=0 if mutate == "c" else 1) + dt(1e-6 if mutate == "b" else 1e-5)
    return h * (P[p + "mlp.3.alpha"] / np.sqrt(var))


def _t_comb(P, i, n, dt, mutate):
    s, t = i / n, (i + 1) / n
    if mutate == "d":
        s, t = t, s
    return (_time_embed(P, 0, s, dt, mutate) + _time_embed(P, 1, t, dt, mutate)) / dt(2)


def _flow_dir(P, depth, cond, tc, cur, onepass, mutate):
    """SimpleMLPAdaLN.forward on rows `cur` with the conditioning `cond` (= cond_embed(c)) and the time embedding `tc`"""
    dt = cur.dtype.type
    p = "flow_lm.flow_net."
    eps = 1e-5 if mutate == "a" else 1e-6
    one = dt(0 if mutate == "g" else 1)
    x = _linear(cur, P[p + "input_proj.weight"], P[p + "input_proj.bias"])
    sy = _silu(tc + cond)
    for r in range(depth):
        q = f"{p}res_blocks.{r}."
        shift, scale, gate = np.split(_linear(sy, P[q + "adaLN_modulation.1.weight"], P[q + "adaLN_modulation.1.bias"]), 3, axis=-1)
        h = _layer_norm(x, P[q + "in_ln.weight"], P[q + "in_ln.bias"], eps, onepass) * (one + scale) + shift
        h = _silu(_linear(h, P[q + "mlp.0.weight"], P[q + "mlp.0.bias"]))
        x = x + gate * _linear(h, P[q + "mlp.2.weight"], P[q + "mlp.2.bias"])
    q = p + "final_layer."
    shift, scale = np.split(_linear(sy, P[q + "adaLN_modulation.1.weight"], P[q + "adaLN_modulation.1.bias"]), 2, axis=-1)
    h = _layer_norm(x, None, None, eps, onepass) * (one + scale) + shift
    return _linear(h, P[q + "linear.weight"], P[q + "linear.bias"])


def flow_head_ref(cfg, W, x, noise, lsd_steps, row_n=None, dtype=np.float64, onepass=False, mutate=None):
    """x [B, d_model]: transformer output before out_norm; noise [B, ldim]: LSD start point; row_n[m]: row m's own Euler
    count (0: lsd_steps).  `row_n=None` is a state without row schedules, an array (all zero included) one with them:
    only the former folds silu(t_comb + .) into `ce` at lsd_steps == 1.
    -> latent [B, ldim], eos_logit [B], ce [B, flow_dim]"""
    assert mutate is None or mutate in MUTANTS
    dt = np.dtype(dtype).type
    P = _cast(W, dtype)
    depth = cfg.flow_lm.flow.depth
    x = np.asarray(x).astype(dtype)
    B = x.shape[0]
    c = _layer_norm(x, P["flow_lm.out_norm.weight"], P["flow_lm.out_norm.bias"], 1e-5, onepass)
    eos = _linear(x if mutate == "h" else c, P["flow_lm.out_eos.weight"], P["flow_lm.out_eos.bias"])[:, 0]
    cond = _linear(c, P["flow_lm.flow_net.cond_embed.weight"], P["flow_lm.flow_net.cond_embed.bias"])
    own = np.zeros(B, np.int64) if row_n is None else np.asarray(row_n, np.int64)
    eff = np.where(own > 0, own, lsd_steps)
    lat = np.asarray(noise).astype(dtype).copy()
    run_to = int(eff.max())
    for n in sorted(set(eff.tolist())):
        for overridden in (False, True):
            rows = (eff == n) & ((own > 0) == overridden)
            if not rows.any():
                continue
            inv = dt(1) / dt(lsd_steps if (mutate == "e" and overridden) else n)
            cur = lat[rows]
            for i in range(run_to if mutate == "f" else n):  # mutant f: on with the row's own schedule, extrapolated
                cur = cur + _flow_dir(P, depth, cond[rows], _t_comb(P, i, n, dt, mutate), cur, onepass, mutate) * inv
            lat[rows] = cur
    ce = _silu(_t_comb(P, 0, 1, dt, mutate) + cond) if (lsd_steps == 1 and row_n is None) else cond
    return lat, eos, ce


OUTPUTS = ("latent", "eos_logit", "ce")


MIN_SAMPLES = 16  # fewest float32 errors an E32 may be the worst of


def _logit_e32_reordered(W, x, eos64, orders):
    """max|logit32 - logit64| over `orders` further float32 evaluations of the SAME logit: out_norm and the out_eos dot
    product with the d_model axis in another (seeded) order, both variance forms.  The value is the same in exact
    arithmetic; only the float32 roundings differ."""
    P = _cast(W, np.float32)
    x = np.asarray(x, np.float32)
    g, beta = P["flow_lm.out_norm.weight"], P["flow_lm.out_norm.bias"]
    w, b = P["flow_lm.out_eos.weight"], P["flow_lm.out_eos.bias"]
    rng = np.random.default_rng(x.shape[1])
    worst = 0.0
    for _ in range(orders):
        idx = rng.permutation(x.shape[1])
        for onepass in (False, True):
            c = _layer_norm(np.ascontiguousarray(x[:, idx]), g[idx], beta[idx], 1e-5, onepass)
            e = _linear(c, np.ascontiguousarray(w[:, idx]), b)[:, 0]
            assert e.dtype == np.float32
            worst = max(worst, float(np.abs(e.astype(np.float64) - eos64).max()))
    return worst


def flow_head_e32(cfg, W, x, noise, lsd_steps, row_n=None):
    """-> (y64, E32): the fp64 reference (latent, eos_logit, ce) and E32 per output as {name: float}.

    E32 is meant as the worst of many random-sign float32 errors.  The logit has one element per row, so with fewer than
    MIN_SAMPLES rows it is the rounding error of a few numbers and can lie anywhere below half an ulp of the logit (8.9e-9
    was met at B = 1, where |logit| ~ 4.5 has an ulp of 4.8e-7).  Then, and only then, the logit's E32 also takes
    ceil(MIN_SAMPLES / B) - 1 further float32 evaluations of the same logits with the d_model sums in other orders
    (`_logit_e32_reordered`), so that it is the worst of >= MIN_SAMPLES errors like every other figure.  Nothing here
    comes from the code under test."""
    y64 = flow_head_ref(cfg, W, x, noise, lsd_steps, row_n)
    e32 = dict.fromkeys(OUTPUTS, 0.0)
    for onepass in (False, True):
        y32 = flow_head_ref(cfg, W, x, noise, lsd_steps, row_n, dtype=np.float32, onepass=onepass)
        for name, a, b in zip(OUTPUTS, y32, y64):
            assert a.dtype == np.float32, name
            e32[name] = max(e32[name], float(np.abs(a.astype(np.float64) - b).max()))
    B = y64[1].shape[0]
    if B < MIN_SAMPLES:
        e32["eos_logit"] = max(e32["eos_logit"], _logit_e32_reordered(W, x, y64[1], -(-MIN_SAMPLES // B) - 1))
    return y64, e32


def random_inputs(cfg, B, seed):
    """the CPU experiments' stand-in for a transformer output: x ~ N(0, 1), noise ~ 0.8 N(0, 1)"""
    rng = np.random.default_rng(seed)
    D, ldim = cfg.flow_lm.transformer.d_model, cfg.mimi.quantizer.dimension
    return rng.standard_normal((B, D)).astype(np.float32), (rng.standard_normal((B, ldim)) * 0.8).astype(np.float32)
