"""fp64 reference of the FlowLM transformer backbone (the layer stack that turns embeddings or latents into the residual
stream x and the KV cache) for tests/test_lm_reference_cpu.py and tests/test_gpu_lm_matrix.py and, with a weight format,
tests/test_lm_formats_reference_cpu.py and tests/test_gpu_lm_formats.py.  Plain numpy, no GPU.

Formulas are those of `oracle.np_oracle.FlowLM.backbone`, `prefill`, `transformer_layer`, `apply_rope` and the input
side of `decode_step` (BOS for NaN element by element, then input_linear), evaluated in `dtype` from the float32
operands the kernels consume: weights, embeddings or latents, BOS and the cache already present.  The state is explicit
(`LMRef`): per-row offsets, an active flag per row, and per layer K (after RoPE) and V in the reference layout
[2, B, T, H, 64] of `export_layer` / `import_layer`.

RoPE: the fp64 evaluation uses the formula in fp64 (frequencies exp(-ln(max_period) * 2 i / 64), angle freq * pos); the
float32 evaluation does everything in float32, as the reference's rope.py does.  The float32 rounding of the frequency
table and of the angle (3e-5 at position 1000) is thereby part of E32, not of the reference.

  E32(call, output) = the larger of max|y32 - y64| over two float32 evaluations of the same call (two-pass LayerNorm
                      variance, and the kernels' one-pass max(E[x^2] - mu^2, 0)), per output: the residual stream x of
                      the real rows and, for every layer l, the rows of K and V the call wrote ("x", "K<l>", "V<l>").
                      Every output has at least 128 numbers (one row of x, or one position of one layer), so the
                      small-sample exception of flow_ref.flow_head_e32 is not needed and `lm_e32` asserts that.

E32 is the yardstick of the GPU matrix and never comes from the code under test: a kernel that only sums in another
order stays within a small multiple of it, a kernel with one of the seeded defects below (MUTANTS) does not.

Parked rows follow the library's contract (include/ptts.h, ptts_lm_state_set_row_active): parking pins the row to
position 0; it keeps flowing through the kernels there, so each step rewrites slot 0 of its own cache and nothing else,
and its position never advances.  `copy_row` un-parks.

The cases of the GPU matrix are written once, here (CASES), against a small driver interface; `RefDriver` runs them on
the reference alone (for the mutation test), tests/test_gpu_lm_matrix.py runs the same functions on the engine.

Weight formats (`fmt`, for tests/test_lm_formats_reference_cpu.py and tests/test_gpu_lm_formats.py).  None is the fp32
model above and changes nothing.  The images are computed in numpy float32 as the load-time kernels state them and then
widened (`format_weights`):

  "q8a" / "q8f" / "q8"  int8 weights for in_proj and out_proj / linear1 and linear2 / all four: per output row
                        scale = max|w| / 127 (1 for a zero row), q = clip(rint(w / scale), -127, 127), and the weight is
                        q * scale formed in fp64.  LayerNorm stays a plain LayerNorm.  No activation is rounded; the bound
                        is FACTOR * E32 with E32 from the dequantised weights.
  "b16"                 in_proj and linear1: W' = bf16_rne(fp32(w * g)), g the preceding norm's gain, evaluated in folded
                        form ((x~ W'^T) - mu s) rs + c with s = rowsum(W'), c = w beta from the unrounded w, and mu, rs
                        from the unrounded x; out_proj and linear2: W' = bf16_rne(w).  Four operands per layer are
                        rounded to bf16 (SITES): x before in_proj, the attention output before out_proj, x before
                        linear1 and GELU(linear1) before linear2.

The kernels round their own fp32 intermediate, the reference an fp64 one; an element next to a rounding midpoint can land
on the other side, which moves outputs by about |w| ulp_bf16(x), three orders above fp32 noise.  So rounding decisions
are explicit (`Rounding`, `lm_judge`):

  master     the fp64 pass rounds to nearest even and records, per rounded element, the value it chose, the other
             neighbour and the distance to the nearest midpoint.
  forced     the two float32 passes of E32 take the master's chosen values instead of rounding their own, so E32 measures
             summation and transcendental error only; they also give e_site = max|x32 - x64| per operand tensor.
  A          the ambiguous set: every element whose distance to a midpoint is at most FACTOR * e_site (an operand the
             call was given, e_site = 0, has none: both sides round the same number).
  F          per a in A one more fp64 pass with that element on its other neighbour and everything downstream of it
             rounded to nearest even again, so the pass carries the flip's consequences, later roundings that follow it
             included; F(output) = sum_a |y64(flip a) - y64| elementwise, accumulated only where the output is downstream
             of a (a later site of the same row, a later position of the same sequence), exactly 0 elsewhere.
  bound      |gpu - y64| <= FACTOR * E32(output) + F(output), elementwise.

A few percent of the rounded operands are ambiguous (an element below about 2e-3 always is: half its bf16 spacing is less
than 8 e_site), most of them small, with allowances near E32; the few of ordinary size carry allowances of 1e-2 on outputs
of order 1, since what follows a flipped operand rounds differently too.  F therefore grows with everything upstream: it
is exactly 0 for layer 0's K and V of a prefill, around 1e-2 for the residual stream of a decode step, and past the first
positions of a long prefill it reaches a tenth of the outputs' size.  Every position is judged by this bound; for the few
calls whose flip passes do not fit a test (JUDGE_ROWS) `lm_judge(rows=)` works F out for the first positions a sequence
gets in the call, which is exact for them, and holds the later ones to FACTOR times the deviation of a float32 evaluation
that rounds its own operands (E32nat).

Nothing in E32, A or F comes from the code under test."""

from __future__ import annotations

import math
import zlib

import numpy as np
from scipy.special import erf as _erf

from pocket_tts_amd.config import named_config
from pocket_tts_amd.weights import generate_state_dict

# seeded defects (`mutate=`): each is one plausible slip in a kernel or in the host code around the layer stack
MUTANTS = {
    "eps": "LayerNorm eps 1e-6 instead of 1e-5",
    "rope_half": "half-split RoPE pairs (i, i + 32) instead of interleaved (2 i, 2 i + 1)",
    "rope_t": "RoPE position t instead of offset[b] + t",
    "rope_row0": "every row rotated with row 0's offset",
    "rope_v": "RoPE also applied to V",
    "noscale": "attention scale 1 / sqrt(64) missing",
    "noself": "a query does not see its own key",
    "future": "a query also sees key pos + 1",
    "ragged_pad": "a ragged row's padding keys are stored and its position moves past them: the next chunk attends them",
    "bos_row": "BOS replaces the whole row when any element is NaN",
    "nan_zero": "NaN replaced by 0 instead of BOS",
    "gelu_tanh": "tanh-GELU instead of erf",
    "res2_norm": "second residual taken from the normalised stream",
    "park_adv": "a parked row advances its position",
}

CONFIG_NAMES = ("tiny", "en100m")
VARIANTS = ("plain", "smallvar", "bigmean")
MIN_SAMPLES = 16  # fewest float32 errors an E32 may be the worst of (flow_ref.MIN_SAMPLES)

_WEIGHTS = {}
_CAST = {}


def lm_weights(name, seed=0):
    """(cfg, W) of `generate_state_dict(named_config(name), seed)`, built once"""
    if (name, seed) not in _WEIGHTS:
        cfg = named_config(name)
        _WEIGHTS[(name, seed)] = (cfg, generate_state_dict(cfg, seed))
    return _WEIGHTS[(name, seed)]


def _cast(W, dtype):
    """the backbone's tensors of W in `dtype`, converted once per weight dict"""
    key = (id(W), np.dtype(dtype).str)
    if key not in _CAST:
        keep = ("flow_lm.transformer.", "flow_lm.bos_emb", "flow_lm.input_linear.")
        _CAST[key] = (W, {k: np.asarray(v).astype(dtype) for k, v in W.items() if k.startswith(keep)})
    return _CAST[key][1]


FORMATS = ("q8a", "q8f", "q8", "b16")
FACTOR = 8  # the project's figure: the bound on outputs and the width of the ambiguous set in units of e_site
SITES = ("x1", "ao", "x2", "gelu")  # the operands a b16 layer rounds, in the order it meets them
_Q8 = {"q8a": ("self_attn.in_proj", "self_attn.out_proj"), "q8f": ("linear1", "linear2"),
       "q8": ("self_attn.in_proj", "self_attn.out_proj", "linear1", "linear2")}
_FMT = {}
FLIP_ROWS = 4096  # rows of one batched flip pass


def q8_image(w):
    """int8 image of a Linear weight [N, K] as the quantiser states it, in float32: (q as float32 integers, scale [N, 1])"""
    w = np.asarray(w, np.float32)
    mx = np.abs(w).max(axis=1, keepdims=True)
    scale = np.where(mx > 0, mx / np.float32(127.0), np.float32(1.0)).astype(np.float32)
    q = (np.clip(np.rint(w / scale), -127, 127) + np.float32(0.0)).astype(np.float32)  # + 0: an int8 has no -0
    return q, scale


def b16_image(w, g=None):
    """bf16 image of a Linear weight as float32: bf16_rne(fp32(w * g)) behind a LayerNorm of gain g, else bf16_rne(w)"""
    from oracle.np_oracle import bf16_round

    w = np.asarray(w, np.float32)
    return bf16_round(w if g is None else (w * np.asarray(g, np.float32)[None, :]).astype(np.float32))


def format_weights(W, L, fmt, dtype):
    """what `fmt` puts in the place of the backbone's Linear weights, in `dtype`: for q8* the dequantised weight under the
    weight's own name; for b16 the bf16 images under the weights' names and, for in_proj and linear1, the fold vectors
    under "<linear>.s" and "<linear>.c".  Built once per (weight dict, format, dtype)."""
    key = (id(W), fmt, np.dtype(dtype).str)
    if key in _FMT:
        return _FMT[key][1]
    out = {}
    for l in range(L):
        p = f"flow_lm.transformer.layers.{l}."
        if fmt in _Q8:
            for lin in _Q8[fmt]:
                q, scale = q8_image(W[p + lin + ".weight"])
                out[p + lin + ".weight"] = (q.astype(np.float64) * scale.astype(np.float64)).astype(dtype)
        else:
            for lin, norm in (("self_attn.in_proj", "norm1"), ("linear1", "norm2")):
                w = np.asarray(W[p + lin + ".weight"], np.float32)
                img = b16_image(w, W[p + norm + ".weight"]).astype(dtype)
                out[p + lin + ".weight"] = img
                out[p + lin + ".s"] = img.sum(axis=1)
                out[p + lin + ".c"] = w.astype(dtype) @ np.asarray(W[p + norm + ".bias"]).astype(dtype)
            for lin in ("self_attn.out_proj", "linear2"):
                out[p + lin + ".weight"] = b16_image(W[p + lin + ".weight"]).astype(dtype)
    _FMT[key] = (W, out)
    return out


def bf16_rne64(v):
    """fp64 -> bf16, round to nearest even, without a detour over float32: (the value chosen, the other neighbour, the
    distance to the midpoint between them), all fp64.  bf16 has 8 significant bits: with v = m 2^e, 0.5 <= |m| < 1, the
    spacing is 2^(e - 8) and v / 2^(e - 8) has its integer part in [128, 256) (subnormals and overflow do not occur at
    the backbone's magnitudes)."""
    v = np.asarray(v, np.float64)
    _, e = np.frexp(v)
    q = np.ldexp(1.0, e - 8)
    t = v / q
    lo = np.floor(t)
    chosen = np.rint(t)  # ties to the even integer = the even mantissa
    other = 2.0 * lo + 1.0 - chosen
    assert np.array_equal(chosen * q, bf16_rne64_fast(v))
    return chosen * q, other * q, np.abs(t - lo - 0.5) * q


def bf16_rne64_fast(v):
    """the value `bf16_rne64` chooses, on the bits: fp64 keeps 52 mantissa bits, bf16 7, so 45 are rounded away"""
    u = np.ascontiguousarray(v, np.float64).view(np.uint64)
    r = ((u + np.uint64((1 << 44) - 1) + ((u >> np.uint64(45)) & np.uint64(1))) >> np.uint64(45)) << np.uint64(45)
    return r.view(np.float64)


class Rounding:
    """The operand roundings of the `_segments` passes of one b16 call.  Without arguments: round to nearest even (the
    natural evaluation in the pass's dtype).  `forced` = another pass's `chosen`: take those values instead.  `override` =
    {(layer, site): (rows, columns, values)}: those elements of the (only) pass get `values` whatever they round to.  `record`
    keeps, per (pass k, layer, site), the unrounded operand `raw` and, when rounding fp64, `chosen`, `other` and `dist`;
    per (k, layer) the layer's input `xin`; per k the segments' (row, first position, rows) as `layout`."""

    def __init__(self, forced=None, override=None, record=False):
        self.forced, self.override, self.record = forced, override, record
        self.k = -1
        self.raw, self.chosen, self.other, self.dist, self.xin, self.layout = {}, {}, {}, {}, {}, {}

    def operand(self, l, site, v):
        from oracle.np_oracle import bf16_round

        key = (self.k, l, site)
        if self.forced is not None:
            r = self.forced[key].astype(v.dtype)
            assert r.shape == v.shape
        elif v.dtype == np.float64 and self.record:
            r, self.other[key], self.dist[key] = bf16_rne64(v)
            self.chosen[key] = r
        elif v.dtype == np.float64:
            r = bf16_rne64_fast(v)
        else:
            r = bf16_round(v)
            if self.record:
                self.chosen[key] = r
        if self.record:
            self.raw[key] = v
        if self.override is not None and (l, site) in self.override:
            rows, cols, vals = self.override[(l, site)]
            r = r.copy()
            r[rows, cols] = vals
        return r


def input_variant(emb, variant):
    """plain; smallvar: scaled so that the row variance is ~1e-5 and eps decides the first LayerNorm; bigmean: + 4, row
    mean ~4 against a deviation of ~0.3, the cancellation case of the one-pass variance"""
    emb = np.asarray(emb, np.float32)
    if variant == "smallvar":
        return (emb * np.float32(math.sqrt(1e-5) / float(emb.std()))).astype(np.float32)
    if variant == "bigmean":
        return (emb + np.float32(4.0)).astype(np.float32)
    if variant != "plain":
        raise KeyError(variant)
    return emb


def _layer_norm(x, w, b, eps, onepass):
    dt = x.dtype.type
    mu = x.mean(axis=-1, keepdims=True)
    if onepass:  # the kernels' formula (not their summation order)
        var = np.maximum((x * x).mean(axis=-1, keepdims=True) - mu * mu, dt(0))
    else:
        var = ((x - mu) * (x - mu)).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + dt(eps)) * w + b


def _ln_stats(x, eps, onepass):
    """(mu, 1 / sqrt(var + eps)) of the rows of x, the variance as in `_layer_norm`"""
    dt = x.dtype.type
    mu = x.mean(axis=-1, keepdims=True)
    if onepass:
        var = np.maximum((x * x).mean(axis=-1, keepdims=True) - mu * mu, dt(0))
    else:
        var = ((x - mu) * (x - mu)).mean(axis=-1, keepdims=True)
    return mu, dt(1) / np.sqrt(var + dt(eps))


def _gelu(x, tanh):
    dt = x.dtype.type
    if tanh:
        return dt(0.5) * x * (dt(1) + np.tanh(dt(math.sqrt(2.0 / math.pi)) * (x + dt(0.044715) * x * x * x)))
    return x * dt(0.5) * (dt(1) + _erf(x * dt(1.0 / math.sqrt(2.0))))


def _rope(x, pos, max_period, half):
    """x [n, H, 64], pos int [n] -> rotated; float32: every step in float32 (reference rope.py), fp64: the formula"""
    dt = x.dtype.type
    D = x.shape[-1]
    if x.dtype == np.float32:
        freqs = np.exp(np.arange(D // 2, dtype=np.float32) * np.float32(-math.log(max_period) * 2 / D)).astype(np.float32)
        ang = (freqs[None, :] * pos.astype(np.float32)[:, None]).astype(np.float32)
    else:
        freqs = np.exp(-math.log(max_period) * 2.0 * np.arange(D // 2, dtype=np.float64) / D)
        ang = freqs[None, :] * pos.astype(np.float64)[:, None]
    c, s = np.cos(ang).astype(dt)[:, None, :], np.sin(ang).astype(dt)[:, None, :]
    if half:
        xr, xi = x[..., : D // 2], x[..., D // 2:]
        return np.concatenate([xr * c - xi * s, xr * s + xi * c], axis=-1)
    xr, xi = x[..., 0::2], x[..., 1::2]
    out = np.empty_like(x)
    out[..., 0::2] = xr * c - xi * s
    out[..., 1::2] = xr * s + xi * c
    return out


class Written:
    """what one call computed: per row b the residual stream of its real rows x[b] [n_b, D], the first position it
    wrote start[b], and per layer l the K / V rows it wrote kv[l][b] [2, n_b, H, 64]"""

    def __init__(self, x, kv, start):
        self.x, self.kv, self.start = x, kv, np.asarray(start, np.int64)
        self.n = np.array([len(r) for r in x], np.int64)

    def outputs(self):
        """{"x", "K0", "V0", "K1", ...} -> all real rows of the call, concatenated and flattened"""
        out = {"x": np.concatenate([r.reshape(-1) for r in self.x])}
        for l, rows in enumerate(self.kv):
            for j, name in enumerate("KV"):
                out[f"{name}{l}"] = np.concatenate([r[j].reshape(-1) for r in rows])
        return out


class LMRef:
    """The backbone's state and entry points in `dtype`.  `onepass`: LayerNorm variance as max(E[x^2] - mu^2, 0).
    `fmt`: the weight format (module docstring); under "b16" the operand roundings of a call go through `self.R`
    (a `Rounding`; None: a fresh natural one per call)."""

    def __init__(self, cfg, W, B, cap, dtype=np.float64, onepass=False, mutate=None, fmt=None):
        assert mutate is None or mutate in MUTANTS
        assert fmt is None or fmt in FORMATS
        t = cfg.flow_lm.transformer
        self.cfg, self.W = cfg, W
        self.D, self.H, self.L = t.d_model, t.num_heads, t.num_layers
        self.max_period = float(t.max_period)
        self.ldim = cfg.mimi.quantizer.dimension
        self.B, self.cap = B, cap
        self.dtype, self.onepass, self.mutate = np.dtype(dtype), onepass, mutate
        self.P = _cast(W, dtype)
        self.fmt, self.R = fmt, None
        if fmt is not None:
            self.P = {**self.P, **format_weights(W, self.L, fmt, dtype)}
        self.kv = [np.zeros((2, B, cap, self.H, 64), dtype) for _ in range(self.L)]
        self.off = np.zeros(B, np.int64)
        self.active = np.ones(B, bool)

    # ---- bookkeeping: what import / reset / copy / park do to a state (include/ptts.h)
    def load(self, kv, off, active=None):
        """operands as the kernels find them: float32 caches [2, B, cap, H, 64] per layer, offsets, active flags"""
        for l in range(self.L):
            self.kv[l][...] = np.asarray(kv[l]).astype(self.dtype)
        self.off[:] = off
        self.active[:] = True if active is None else active
        return self

    def snapshot(self):
        return dict(kv=[k.copy() for k in self.kv], off=self.off.copy(), active=self.active.copy())

    def round32(self):
        """the cache as float32 numbers: what a later call finds as its operand"""
        for l in range(self.L):
            self.kv[l] = self.kv[l].astype(np.float32).astype(self.dtype)

    def import_cache(self, layer, cache, t):
        """cache [2, 1 | B, >= t, H, 64]: a batch of 1 goes to every row; every row's offset becomes t"""
        self.kv[layer][:, :, :t] = np.asarray(cache)[:, :, :t].astype(self.dtype)
        self.off[:] = t

    def reset(self):
        self.off[:] = 0
        self.active[:] = True

    def copy_row(self, row, src, src_row=0):
        """row <- sequence src_row of src, at its own length; the row is active afterwards"""
        T = int(src.off[src_row])
        for l in range(self.L):
            self.kv[l][:, row, :T] = src.kv[l][:, src_row, :T].astype(self.dtype)
        self.off[row] = T
        self.active[row] = True

    def copy_from(self, src):
        for b in range(self.B):
            sb = 0 if src.B == 1 else b
            T = int(src.off[sb])
            for l in range(self.L):
                self.kv[l][:, b, :T] = src.kv[l][:, sb, :T].astype(self.dtype)
            self.off[b] = T

    def set_row_active(self, row, active):
        """parking pins the row to position 0; un-parking by flag leaves it there (copy_row gives it a sequence)"""
        self.active[row] = bool(active)
        if not active:
            self.off[row] = 0

    # ---- the layer stack
    def _segments(self, segs, off0, first_layer=0, R=None, scratch=False):
        """segs = [(row b, inputs x [m, D], first position p0)]: every segment's rows run at positions p0 .. p0 + m and
        their K / V are stored there.  The row-wise parts run on all segments at once, attention per segment.
        `first_layer`: x is the input of that layer and only the layers from there on run; `scratch`: the cache is read
        (positions before p0) but not written, so that segments of one row do not see each other (the flip passes).
        -> [(x out [m, D], [[K, V] per layer that ran])] per segment"""
        b16 = self.fmt == "b16"
        if b16:
            R = R if R is not None else self.R if self.R is not None else Rounding()
            R.k += 1
        P, dt, mu = self.P, self.dtype.type, self.mutate
        eps = 1e-6 if mu == "eps" else 1e-5
        scale = dt(1.0) if mu == "noscale" else dt(1.0 / math.sqrt(64.0))
        ms = [x.shape[0] for _, x, _ in segs]
        lo = np.concatenate([[0], np.cumsum(ms)])
        M = int(lo[-1])
        for (b, _, p0), m in zip(segs, ms):
            assert p0 + m <= self.cap, "KV cache capacity exceeded"
        x = np.concatenate([np.asarray(x).astype(self.dtype) for _, x, _ in segs])
        rp = np.concatenate([(0 if mu == "rope_t" else off0 if mu == "rope_row0" else p0) + np.arange(m) for (_, _, p0), m in zip(segs, ms)])
        wrote = [[] for _ in segs]
        if b16 and R.record:
            R.layout[R.k] = ([(b, p0, m) for (b, _, p0), m in zip(segs, ms)], lo)
        for l in range(first_layer, self.L):
            p = f"flow_lm.transformer.layers.{l}."
            if b16:
                if R.record:
                    R.xin[(R.k, l)] = x
                mean, rs = _ln_stats(x, eps, self.onepass)
                proj = R.operand(l, "x1", x) @ P[p + "self_attn.in_proj.weight"].T
                proj = ((proj - mean * P[p + "self_attn.in_proj.s"]) * rs + P[p + "self_attn.in_proj.c"]).reshape(M, 3, self.H, 64)
            else:
                h = _layer_norm(x, P[p + "norm1.weight"], P[p + "norm1.bias"], eps, self.onepass)
                proj = (h @ P[p + "self_attn.in_proj.weight"].T).reshape(M, 3, self.H, 64)
            q = _rope(proj[:, 0], rp, self.max_period, mu == "rope_half")
            k = _rope(proj[:, 1], rp, self.max_period, mu == "rope_half")
            v = _rope(proj[:, 2], rp, self.max_period, False) if mu == "rope_v" else proj[:, 2]
            ao = np.empty((M, self.D), self.dtype)
            for i, ((b, _, p0), m) in enumerate(zip(segs, ms)):
                sl, nk = slice(lo[i], lo[i + 1]), p0 + m
                wrote[i].append(np.stack([k[sl], v[sl]]))
                if scratch:
                    K, V = np.concatenate([self.kv[l][0, b, :p0], k[sl]]), np.concatenate([self.kv[l][1, b, :p0], v[sl]])
                else:
                    self.kv[l][0, b, p0:nk], self.kv[l][1, b, p0:nk] = k[sl], v[sl]
                    K, V = self.kv[l][0, b, :nk], self.kv[l][1, b, :nk]
                delta = (p0 + np.arange(m))[:, None] - np.arange(nk)[None, :]
                mask = delta > 0 if mu == "noself" else delta >= -1 if mu == "future" else delta >= 0
                s = np.einsum("qhd,khd->hqk", q[sl], K) * scale
                s = np.where(mask[None], s, dt(-np.inf))
                s = s - np.maximum(s.max(axis=-1, keepdims=True), dt(-1e30))  # a query without a key: all weights 0
                w = np.exp(s)
                w = w / np.maximum(w.sum(axis=-1, keepdims=True), dt(1e-30))
                ao[sl] = np.einsum("hqk,khd->qhd", w, V).reshape(m, self.D)
            a = (R.operand(l, "ao", ao) if b16 else ao) @ P[p + "self_attn.out_proj.weight"].T
            ls1, ls2 = P.get(p + "layer_scale_1.scale"), P.get(p + "layer_scale_2.scale")
            x = x + (a if ls1 is None else ls1 * a)
            if b16:
                mean, rs = _ln_stats(x, eps, self.onepass)
                f = R.operand(l, "x2", x) @ P[p + "linear1.weight"].T
                f = (f - mean * P[p + "linear1.s"]) * rs + P[p + "linear1.c"]
                f = R.operand(l, "gelu", _gelu(f, mu == "gelu_tanh")) @ P[p + "linear2.weight"].T
                h = _layer_norm(x, P[p + "norm2.weight"], P[p + "norm2.bias"], eps, self.onepass) if mu == "res2_norm" else None
            else:
                h = _layer_norm(x, P[p + "norm2.weight"], P[p + "norm2.bias"], eps, self.onepass)
                f = _gelu(h @ P[p + "linear1.weight"].T, mu == "gelu_tanh") @ P[p + "linear2.weight"].T
            x = (h if mu == "res2_norm" else x) + (f if ls2 is None else ls2 * f)
        assert x.dtype == self.dtype, x.dtype
        return [(x[lo[i]:lo[i + 1]], wrote[i]) for i in range(len(segs))]

    def _run(self, xs, lens, ragged=False):
        """xs[b] [T_b, D]: row b's inputs, the first lens[b] of them real.  Real rows are computed at positions
        off[b] .. off[b] + lens[b], their K / V stored there; nothing else of the cache changes (a row without a real
        position is not touched at all)."""
        off0, start = int(self.off[0]), self.off.copy()
        real = [b for b in range(self.B) if int(lens[b]) > 0]
        done = dict(zip(real, self._segments([(b, xs[b][:int(lens[b])], int(self.off[b])) for b in real], off0))) if real else {}
        for b in real:
            self.off[b] += int(lens[b])
        if self.mutate == "ragged_pad" and ragged:  # the padding runs on as if it were real
            pad = [b for b in real if xs[b].shape[0] > int(lens[b])]
            if pad:
                self._segments([(b, xs[b][int(lens[b]):], int(self.off[b])) for b in pad], off0)
            for b in pad:
                self.off[b] = start[b] + xs[b].shape[0]
        none_x, none_kv = np.zeros((0, self.D), self.dtype), np.zeros((2, 0, self.H, 64), self.dtype)
        out_x = [done[b][0] if b in done else none_x for b in range(self.B)]
        out_kv = [[done[b][1][l] if b in done else none_kv for b in range(self.B)] for l in range(self.L)]
        return Written(out_x, out_kv, start)

    def prefill(self, emb, lengths=None):
        """emb [B, T, D]; `lengths`: ragged prefill, row b's first lengths[b] positions are real, the rest is ignored"""
        emb = np.asarray(emb)
        assert emb.shape[0] == self.B and emb.shape[2] == self.D and self.active.all()
        lens = np.full(self.B, emb.shape[1]) if lengths is None else np.asarray(lengths)
        return self._run(list(emb), lens, ragged=lengths is not None)

    def decode(self, latent_in):
        """one step from latent_in [B, ldim]: BOS for NaN element by element, input_linear, the layers.  A parked row runs
        at its pinned position and does not advance."""
        P, mu = self.P, self.mutate
        lat = np.asarray(latent_in).astype(self.dtype)
        nan = np.isnan(lat)
        if mu == "bos_row":
            nan = np.broadcast_to(nan.any(axis=1, keepdims=True), nan.shape)
        fill = np.zeros_like(P["flow_lm.bos_emb"]) if mu == "nan_zero" else P["flow_lm.bos_emb"]
        seq = np.where(nan, fill[None, :], lat)
        x0 = seq @ P["flow_lm.input_linear.weight"].T
        before = self.off.copy()
        res = self._run([x0[b:b + 1] for b in range(self.B)], np.ones(self.B, np.int64))
        if mu != "park_adv":
            self.off[~self.active] = before[~self.active]
        return res


# ------------------------------------------------------------------------------------------------
# one call judged on its own operands
def evaluate(cfg, W, snap, op, dtype=np.float64, onepass=False, mutate=None, fmt=None, R=None):
    """`op` = ("prefill", emb, lengths | None) or ("decode", latent_in) on the state `snap` (LMRef.snapshot, or the
    float32 caches, offsets and flags read back from an engine) -> (Written, the LMRef after the call).  `R`: the
    `Rounding` of a b16 call (None: round to nearest even)."""
    B, cap = snap["kv"][0].shape[1], snap["kv"][0].shape[2]
    ref = LMRef(cfg, W, B, cap, dtype, onepass, mutate, fmt).load(snap["kv"], snap["off"], snap.get("active"))
    ref.R = R
    res = ref.prefill(op[1], op[2]) if op[0] == "prefill" else ref.decode(op[1])
    return res, ref


def lm_e32(cfg, W, snap, op, fmt=None, master=None, e_site=None):
    """-> (Written in fp64, {output: E32}, the fp64 LMRef after the call).  Nothing here comes from the code under test.
    Under "b16" the fp64 pass is the master (`master`, a recording Rounding, is filled when given) and the float32 passes
    are forced to its roundings; `e_site` (a dict) receives max|x32 - x64| per (pass, layer, site)."""
    if fmt == "b16" and master is None:
        master = Rounding(record=True)
    res64, ref64 = evaluate(cfg, W, snap, op, fmt=fmt, R=master)
    y64 = res64.outputs()
    e32 = dict.fromkeys(y64, 0.0)
    for onepass in (False, True):
        R = Rounding(forced=master.chosen, record=True) if fmt == "b16" else None
        y32 = evaluate(cfg, W, snap, op, np.float32, onepass, fmt=fmt, R=R)[0].outputs()
        for name, a in y32.items():
            assert a.dtype == np.float32 and a.size >= MIN_SAMPLES, (name, a.dtype, a.size)
            e32[name] = max(e32[name], float(np.abs(a.astype(np.float64) - y64[name]).max()))
        if R is not None and e_site is not None:
            for key, raw in R.raw.items():
                assert raw.dtype == np.float32
                e_site[key] = max(e_site.get(key, 0.0), float(np.abs(raw.astype(np.float64) - master.raw[key]).max()))
    return res64, e32, ref64


class Judged:
    """a call's reference and bound: `res64` (Written), `e32` {output: E32}, `F` {output: flip allowance, flattened like
    Written.outputs()} (zeros without b16), `ref64` the fp64 state after the call, `nA` the size of the ambiguous set,
    `outputs` the names that are judged"""

    def __init__(self, res64, e32, F, ref64, nA, outputs, late=None):
        self.res64, self.e32, self.F, self.ref64, self.nA, self.outputs = res64, e32, F, ref64, nA, outputs
        self.late = late or {}  # output -> (mask of the elements under the late rule, their E32nat)

    def bound(self, name, factor=FACTOR):
        """elementwise: factor * E32 + F, and factor * E32nat where F was not worked out (lm_judge, `rows`)"""
        b = factor * self.e32[name] + self.F[name]
        if name in self.late:
            mask, enat = self.late[name]
            b = np.where(mask, factor * enat, b)
        return b


def lm_judge(cfg, W, snap, op, fmt=None, flips=True, rows=None, cascade=True):
    """The reference of one call with its elementwise bound FACTOR * E32 + F (module docstring).  `flips=False` (b16): no
    flip pass is run and only the outputs that have no ambiguous element upstream by construction are judged, the K and
    V rows of layer 0, whose only rounded operand is the layer's input; where the call was given that input (a prefill)
    its e_site is 0 and the set is empty, which is asserted.
    `rows` (b16): F is worked out for the first `rows` positions each sequence gets in this call, from the ambiguous
    elements of those positions alone, which is exact (attention is causal: a later position is upstream of none of them);
    it is for the calls whose flip passes do not fit a test (judge_args).  At the later positions F is not worked out (it
    reads infinity) and, except where nothing is upstream at all (layer 0's K and V when the layer's input is the call's
    own operand: F = 0), the bound is the project's rule for a kernel that differs from a float32 evaluation in summation
    order, taken with the evaluation that does what the kernel does: FACTOR * E32nat, E32nat(output) = the largest
    |y32 - y64| over the output's late elements and over the two float32 evaluations that round their OWN operands (flips
    and what follows them included).  It is of the order 1e-2 .. 1e-1 on outputs of order 1: no match for a subtle defect,
    which the judged positions are for, but a wrong, stale or unwritten row or tile fails it.
    `cascade=False` is the flip pass read literally, only that element moved and every later rounding kept as the master
    chose it; tests/test_lm_formats_reference_cpu.py shows that this F does not cover a float32 evaluation."""
    master, e_site = (Rounding(record=True), {}) if fmt == "b16" else (None, None)
    res64, e32, ref64 = lm_e32(cfg, W, snap, op, fmt, master, e_site)
    y64 = res64.outputs()
    F = Written([np.zeros_like(r) for r in res64.x], [[np.zeros_like(r) for r in rows] for rows in res64.kv], res64.start)
    if fmt != "b16":
        return Judged(res64, e32, F.outputs(), ref64, 0, list(y64))
    A = []
    for key, dist in master.dist.items():
        assert key[0] == 0  # the true call is one pass
        if e_site[key] > 0:  # an operand both sides hold bit for bit rounds the same on both
            A += [(key[1], key[2], int(r), int(c)) for r, c in np.argwhere(dist <= FACTOR * e_site[key])]
    if not flips:
        assert not [a for a in A if a[:2] == (0, "x1")], "layer 0's input is not the call's own operand"
        return Judged(res64, e32, F.outputs(), ref64, len(A), ["K0", "V0"])
    segs, lo = master.layout[0]

    def run(l, batch):
        """the flip passes of `batch`, all from layer l on, as the segments of one pass: each is its sequence from the
        flipped row on, over the cache and the master's rows before it"""
        fsegs, ov, at, spans = [], {}, 0, []
        for _, site, r, c in batch:
            i = int(np.searchsorted(lo, r, side="right")) - 1
            b, p0, m = segs[i]
            rr = r - int(lo[i])
            end = int(lo[i]) + min(m, rows or m)
            fsegs.append((b, master.xin[(0, l)][r:end], p0 + rr))
            ov.setdefault((l, site), []).append((at, c, master.other[(0, l, site)][r, c]))
            at += end - r
            spans.append((r, end))
        ov = {k: tuple(np.array(col) for col in zip(*v)) for k, v in ov.items()}
        ov = {k: (v[0].astype(np.int64), v[1].astype(np.int64), v[2]) for k, v in ov.items()}
        # the rows before a flipped row are the master's: the cache must hold them, and it does (ref64 is the master's state)
        forced = None
        if not cascade:  # every rounding of the pass as the master chose it, the flipped element aside
            forced = {(0, ll, site): np.concatenate([master.chosen[(0, ll, site)][r:end] for r, end in spans])
                      for ll in range(l, ref64.L) for site in SITES}
        out = ref64._segments(fsegs, 0, first_layer=l, R=Rounding(forced=forced, override=ov), scratch=True)
        for (_, site, r, c), (b, _, p), (xo, kvo) in zip(batch, fsegs, out):
            rr = p - int(res64.start[b])
            end = rr + len(xo)
            F.x[b][rr:end] += np.abs(xo - res64.x[b][rr:end])
            for j, ll in enumerate(range(l, ref64.L)):
                if ll > l or site == "x1":  # layer l's K and V are downstream of its first operand only
                    F.kv[ll][b][:, rr:end] += np.abs(kvo[j] - res64.kv[ll][b][:, rr:end])

    def seq_row(a):
        i = int(np.searchsorted(lo, a[2], side="right")) - 1
        return a[2] - int(lo[i])

    late = [a for a in A if rows is not None and seq_row(a) >= rows]
    for l in range(ref64.L):
        batch, n = [], 0
        for a in (a for a in A if a[0] == l and not (rows is not None and seq_row(a) >= rows)):
            batch.append(a)
            n += int(lo[int(np.searchsorted(lo, a[2], side="right"))]) - a[2]
            if n >= FLIP_ROWS:
                run(l, batch)
                batch, n = [], 0
        if batch:
            run(l, batch)
    if rows is None:
        return Judged(res64, e32, F.outputs(), ref64, len(A), list(y64))
    for b in range(len(F.x)):
        F.x[b][rows:] = np.inf
        for l in range(ref64.L):
            if l > 0 or any(a[:2] == (0, "x1") for a in late):
                F.kv[l][b][:, rows:] = np.inf
    F = F.outputs()
    nat = [evaluate(cfg, W, snap, op, np.float32, onepass, fmt=fmt)[0].outputs() for onepass in (False, True)]
    rule = {}
    for name, f in F.items():
        mask = np.isinf(f)
        if mask.any():
            assert int(mask.sum()) >= MIN_SAMPLES
            rule[name] = (mask, max(float(np.abs(y[name].astype(np.float64) - y64[name])[mask].max()) for y in nat))
    return Judged(res64, e32, F, ref64, len(A), list(y64), rule)


# ------------------------------------------------------------------------------------------------
# The cases of the GPU matrix, written against a driver `d`:
#   d.cfg, d.W, d.D, d.H, d.L, d.ldim
#   d.new(B, cap) -> state                     d.close(state)
#   d.prefill(s, emb, lengths=None, judge=True, attn="attn")      d.decode(s, latent_in, attn="attn_decode")
#   d.import_cache(s, caches, t)   d.reset(s)   d.copy_from(s, src)   d.copy_row(s, row, src, src_row=0)
#   d.park(s, row)
#   d.options(share_prefix=.., prefix_cascade=.., lm_cluster=..)   engine options until the case ends (no-op on the reference)
# `attn`: the attention kernel family the engine must use at lm.attn ("lm_cluster": the single-launch stack instead).
def seed_of(*case):
    return zlib.crc32(repr(case).encode())


def _emb(rng, B, T, D):
    return (rng.standard_normal((B, T, D)) * 0.3).astype(np.float32)


def _latent(rng, B, ldim, first):
    """a decode step's input: finite; at `first`, row 0 is all NaN (BOS) and row 1 NaN in some elements only"""
    lat = (rng.standard_normal((B, ldim)) * 0.8).astype(np.float32)
    if first:
        lat[0, :] = np.nan
        if B > 1:
            lat[1, 1::3] = np.nan
    return lat


def case_prefill(d, B, T, variant="plain"):
    rng = np.random.default_rng(seed_of("prefill", B, T, variant))
    s = d.new(B, -(-T // 16) * 16)
    d.prefill(s, input_variant(_emb(rng, B, T, d.D), variant), attn="attn_decode" if T == 1 else "attn")
    d.close(s)


def case_chunked(d, t1, t2, B=2):
    rng = np.random.default_rng(seed_of("chunked", t1, t2, B))
    s = d.new(B, -(-(t1 + t2) // 16) * 16)
    d.prefill(s, _emb(rng, B, t1, d.D))
    d.prefill(s, _emb(rng, B, t2, d.D))
    d.close(s)


RAGGED_1 = [0, 1, 16, 17, 20]
RAGGED_2 = [3, 0, 17, 1, 16]


def _pad(emb, lengths, rng):
    """padding embeddings around +-1e6"""
    for b, n in enumerate(lengths):
        emb[b, n:] = (rng.standard_normal(emb[b, n:].shape) * 1e6).astype(np.float32)
    return emb


def case_ragged(d):
    """every layer's cache holds a recognisable pattern, offsets 0; two ragged chunks, the second on top of the first, so
    that a padding key stored by the first would be attended by the second"""
    rng = np.random.default_rng(seed_of("ragged"))
    B, cap = 5, 48
    s = d.new(B, cap)
    pattern = [(100.0 + l + 0.001 * np.arange(2 * B * cap * d.H * 64)).reshape(2, B, cap, d.H, 64).astype(np.float32) for l in range(d.L)]
    d.import_cache(s, pattern, cap)
    d.reset(s)
    d.prefill(s, _pad(_emb(rng, B, 20, d.D), RAGGED_1, rng), RAGGED_1)
    d.prefill(s, _pad(_emb(rng, B, 17, d.D), RAGGED_2, rng), RAGGED_2)
    d.close(s)


def case_decode(d, B, cluster=0):
    """context 20, then 3 decode steps"""
    rng = np.random.default_rng(seed_of("decode", B))
    if cluster:
        d.options(lm_cluster=1)
    s = d.new(B, 32)
    d.prefill(s, _emb(rng, B, 20, d.D), judge=False)
    for k in range(3):
        d.decode(s, _latent(rng, B, d.ldim, k == 0), attn="lm_cluster" if cluster else "attn_decode")
    d.close(s)


MIXED = [7, 40, 19, 33, 12]


def case_mixed(d, cluster=0):
    """five rows from batch-1 states of different lengths, row 3 parked; 3 steps; un-park by copy_row; one more step"""
    rng = np.random.default_rng(seed_of("mixed"))
    attn = "lm_cluster" if cluster else "attn_decode"
    if cluster:
        d.options(lm_cluster=1)
    singles = []
    for n in MIXED:
        s1 = d.new(1, 48)
        d.prefill(s1, _emb(rng, 1, n, d.D), judge=False)
        singles.append(s1)
    big = d.new(len(MIXED), 48)
    for i, s1 in enumerate(singles):
        d.copy_row(big, i, s1)
    d.park(big, 3)
    for k in range(3):
        d.decode(big, _latent(rng, len(MIXED), d.ldim, k == 0), attn=attn)
    d.copy_row(big, 3, singles[3])
    d.decode(big, _latent(rng, len(MIXED), d.ldim, False), attn=attn)
    d.close(big)
    for s1 in singles:
        d.close(s1)


def case_bigpos(d):
    """seeded N(0, 1) caches at t = 1000 in a capacity of 1040: two decode steps at positions 1000 and 1001, then, on a
    fresh import, a prefill of positions 1000 .. 1016"""
    rng = np.random.default_rng(seed_of("bigpos"))
    B, cap, t = 3, 1040, 1000
    caches = [rng.standard_normal((2, B, t, d.H, 64)).astype(np.float32) for _ in range(d.L)]
    s = d.new(B, cap)
    d.import_cache(s, caches, t)
    for k in range(2):
        d.decode(s, _latent(rng, B, d.ldim, k == 0))
    d.import_cache(s, caches, t)
    d.prefill(s, _emb(rng, B, 17, d.D))
    d.close(s)


def case_borrowed(d, B, share, cascade):
    """a batch-1 voice state of 37 positions cloned into B rows, 5 text positions, 3 decode steps"""
    rng = np.random.default_rng(seed_of("borrowed", B))
    d.options(share_prefix=share, prefix_cascade=cascade)
    voice = d.new(1, 48)
    d.prefill(voice, _emb(rng, 1, 37, d.D), judge=False)
    s = d.new(B, 48)
    d.copy_from(s, voice)
    d.prefill(s, _emb(rng, B, 5, d.D))
    for k in range(3):
        d.decode(s, _latent(rng, B, d.ldim, k == 0), attn="attn_cascade" if (share and cascade and B >= 16) else "attn_decode")
    d.close(s)
    d.close(voice)


PREFILL_SHAPES = {"tiny": [(1, 1), (1, 16), (1, 17), (3, 33), (17, 5), (2, 100)], "en100m": [(1, 17), (3, 20)]}
DECODE_BATCHES = {"tiny": [1, 3, 16, 17, 37], "en100m": [1, 17]}
CLUSTER_BATCHES = {"tiny": [3, 17], "en100m": [3]}
BORROWED = [(B, share, cascade) for B in (3, 16) for share, cascade in ((1, 0), (1, 423), (0, 423))]

# family -> [(id, config, function, arguments)]: the whole GPU matrix
CASES = {
    "prefill": [(f"{name}-B{B}-T{T}-{v}", name, case_prefill, (B, T, v))
                for name in CONFIG_NAMES for B, T in PREFILL_SHAPES[name] for v in VARIANTS],
    "chunked": [(f"tiny-{a}+{b}", "tiny", case_chunked, (a, b)) for a, b in ((37, 5), (16, 16))],
    "ragged": [("tiny", "tiny", case_ragged, ())],
    "decode": [(f"{name}-B{B}", name, case_decode, (B,)) for name in CONFIG_NAMES for B in DECODE_BATCHES[name]],
    "mixed": [("tiny", "tiny", case_mixed, ())],
    "bigpos": [("tiny", "tiny", case_bigpos, ())],
    "borrowed": [(f"tiny-B{B}-share{s}-cascade{c}", "tiny", case_borrowed, (B, s, c)) for B, s, c in BORROWED],
    "cluster": [(f"{name}-B{B}", name, case_decode, (B, 1)) for name in CONFIG_NAMES for B in CLUSTER_BATCHES[name]]
               + [("tiny-mixed", "tiny", case_mixed, (1,))],
}


# The reduced-format matrix: (family, case id) of CASES per config.  A borrowed prefix at B = 16 with and without the
# cascade kernel; "cluster" asks for the single-launch stack, which a reduced-format engine must not run.
# b16: the calls whose flip passes do not fit a test (one pass per ambiguous element, each over the rest of its sequence),
# and the positions per sequence that get them (lm_judge, `rows`).  Everything else is judged at every position.  Measured
# reference work of the full judgement on 8 CPU cores: (1, 17) 0.2 s, bigmean 6 s; (3, 33) 6 s, bigmean (48488 ambiguous
# elements) about a minute; (2, 100) 90 s, bigmean (124384) many minutes.
JUDGE_ROWS = {"tiny-B3-T33-bigmean": 8, "tiny-B2-T100-plain": 32, "tiny-B2-T100-smallvar": 32, "tiny-B2-T100-bigmean": 8}
FORMAT_CASES = {
    "tiny": [("prefill", f"tiny-B{B}-T{T}-{v}") for B, T in ((1, 1), (1, 17), (3, 33), (2, 100)) for v in VARIANTS]
            + [("chunked", "tiny-37+5"), ("ragged", "tiny")] + [("decode", f"tiny-B{B}") for B in (1, 3, 16, 17, 37)]
            + [("mixed", "tiny"), ("borrowed", "tiny-B16-share1-cascade423"), ("borrowed", "tiny-B16-share1-cascade0"),
               ("cluster", "tiny-B3")],
    "en100m": [("prefill", "en100m-B1-T17-plain"), ("decode", "en100m-B1"), ("decode", "en100m-B17")],
}


def format_cases(name, fmt):
    """the cases of config `name` under `fmt`.  en100m runs all-int8 and bf16 only, and bf16 leaves out decode B = 17
    (17 rows of 7168 rounded operands per layer: one fp64 pass of 1024-wide layers per ambiguous element)."""
    if name == "en100m":
        if fmt not in ("q8", "b16"):
            return []
        return [c for c in FORMAT_CASES[name] if not (fmt == "b16" and c[1] == "en100m-B17")]
    return FORMAT_CASES[name]


def judge_args(fmt, family, cid):
    """how `lm_judge` is asked for a case: the en100m bf16 prefill is judged on layer 0's K and V only.  Downstream of
    layer 0 it has tens of thousands of ambiguous elements (17 x 7168 operands per layer, a few percent of them within 8
    e_site of a midpoint), each a pass through 1024-wide fp64 layers, and an allowance that adds up to the size of the
    outputs: unaffordable and void.  Layer 0's K and V have nothing ambiguous upstream and are held to 8 E32."""
    if fmt != "b16":
        return {}
    if cid.startswith("en100m") and family == "prefill":
        return dict(flips=False)
    return dict(rows=JUDGE_ROWS[cid]) if family == "prefill" and cid in JUDGE_ROWS else {}


def find_case(family, cid):
    return next(c for c in CASES[family] if c[0] == cid)


class RefDriver:
    """Runs a case on the reference alone and records every judged call: `calls` = [(op, snapshot before, Written,
    offsets after)].  The cache is rounded to float32 after every call, so that each call finds float32 operands as on
    the engine and two drivers that have computed the same so far hold the same bits.  `mutate` applies to the judged
    calls only."""

    def __init__(self, name, mutate=None, fmt=None):
        self.cfg, self.W = lm_weights(name)
        t = self.cfg.flow_lm.transformer
        self.D, self.H, self.L, self.ldim = t.d_model, t.num_heads, t.num_layers, self.cfg.mimi.quantizer.dimension
        self.mutate, self.fmt = mutate, fmt
        self.calls = []

    def new(self, B, cap):
        return LMRef(self.cfg, self.W, B, cap, mutate=self.mutate, fmt=self.fmt)

    def close(self, s):
        pass

    def options(self, **kw):
        pass

    def _call(self, s, op, judge):
        snap = s.snapshot() if judge else None
        keep = s.mutate
        if not judge:  # a call the matrix does not judge only makes operands: whatever it leaves is what the next call finds
            s.mutate = None
        res = s.prefill(op[1], op[2]) if op[0] == "prefill" else s.decode(op[1])
        s.mutate = keep
        s.round32()
        if judge:
            self.calls.append((op, snap, res, s.off.copy()))

    def prefill(self, s, emb, lengths=None, judge=True, attn="attn"):
        self._call(s, ("prefill", emb, lengths), judge)

    def decode(self, s, latent_in, attn="attn_decode"):
        self._call(s, ("decode", latent_in), True)

    def import_cache(self, s, caches, t):
        for l, c in enumerate(caches):
            s.import_cache(l, c, t)

    def reset(self, s):
        s.reset()

    def copy_from(self, s, src):
        s.copy_from(src)

    def copy_row(self, s, row, src, src_row=0):
        s.copy_row(row, src, src_row)

    def park(self, s, row):
        s.set_row_active(row, False)
