"""fp64 reference of the fp32 Mimi decoder, ONE STATELESS FUNCTION PER STAGE, for tests/test_mimi_reference_cpu.py and
tests/test_gpu_mimi_matrix.py.  Plain numpy, no GPU.

A stage is what lies between two buffers the engine can read back (`Engine.debug_read`): it takes the stage's input tap of
this frame plus the tail of the same tap from the previous frame (zeros on a sequence's first frame and after `reset_row`)
and returns the stage's output tap, so a kernel is judged on the very input it consumed.  Formulas are those of
`oracle.np_oracle.MimiDecoder.decode` and of the reference lines it cites (`tts_model.py:449-455`, `mimi.py:89-94`,
`dummy_quantizer.py:17-18`, `resample.py:40-51`, `mimi_transformer.py:39-54,140-150`, `transformer.py:22-29,135-158`,
`rope.py:7-58`, `seanet.py:33-41,141-180`, `conv.py:84-163`), evaluated in `dtype` from the float32 operands.

Layout: activations are [B, T, C] (time-major, channels last); the engine's taps are [B * T, C], row b * T + t.  The taps
hold what the next kernel reads: `seanet0/3/6/9` are ELU'd by their producer, `seanet2/5/8` (the residual blocks' skip
inputs) are raw, `tr_attn` is the attention output before out_proj, `tr_ff` is GELU(linear1).

  stage  inputs                                       output tap     kernels judged
  P      latent[f], latent[f-1]                       upsample       mimi_prologue_kernel
  A      upsample of every frame <= f                 tr_attn        +ln GEMM with EPI_QKV, RoPE table, ring, attention
  B      tr_attn, upsample                            tr_resid       EPI_RES + layer scale
  C      tr_resid                                     tr_ff          +ln GEMM, GELU
  D      tr_ff, tr_resid                              dec_tr         EPI_RES into the parity-buffered output
  T      upsample of every frame <= f                 dec_tr         the whole transformer
  S0     dec_tr, last 6 rows of the previous frame    seanet0        k7 streaming conv
  Ci     stage input, last row of the previous frame  seanet2/5/8    EPI_CONVTR
  Ri     seanet2/5/8, last 2 rows of the prev. frame  seanet3/6/9    fused resblock<..> or the gemm(+elu) / EPI_RES pair
  L      seanet9, last 2 rows of the previous frame   PCM            pcm_conv, EPI_PCM, or pcm_part + pcm_carry + pcm_fix
  R3L    seanet8, last 4 rows of the previous frame   PCM            R3 and L in one launch, the block's output kept on chip

In stage A the RoPE angle is the FLOAT32 product freq * pos, as the model defines it (`np_oracle.apply_rope`, reference
`rope.py:28-50`); sine, cosine and everything after them are `dtype`.  The key window is 0 <= pos_q - pos_k < context.

The yardstick, `stage_e32(stage, inputs) -> (y64, E32)`: E32 is the largest max|y32 - y64| over float32 evaluations of the
same formulas on the same inputs, in two summation orders and two equivalent forms of the elementwise formulas:

  "np"   numpy's own matrix product; two-pass LayerNorm variance; ELU by expm1
  "seq"  a plain sequential sum over k (the least accurate order a kernel may legitimately use); the one-pass variance
         max(E[x^2] - mu^2, 0) and ELU as exp(x) - 1, the forms the kernels use (not their summation order).  The
         sequential sum runs on an evenly spaced subset of the output rows (>= 32 rows, about SEQ_ELEMS outputs) and
         numpy's product on the others: E32 is a maximum, so the subset can only make it smaller, i.e. the bound tighter.

E32 comes from the reference alone, never from a kernel.  MUTANTS are seeded defects: each moves its designated stage's
result by >= 32 E32 (tests/test_mimi_reference_cpu.py), 4 x the GPU bound of 8 E32."""

from __future__ import annotations

import math

import numpy as np
from scipy.special import erf as _erf

from pocket_tts_amd.config import NAMED_CONFIGS, make_config
from pocket_tts_amd.weights import generate_state_dict, seanet_decoder_layers

F32, F64 = np.float32, np.float64

MUTANTS = {
    "parity": "the previous frame's halo rows read from the current frame (wrong parity)",
    "seqcut": "the halo not cut at a sequence boundary (rows of sequence b - 1 used for b)",
    "skip_elu": "the resblock skip taken from the ELU'd copy instead of the raw value",
    "elu_twice": "ELU applied twice on the operand",
    "up_swap": "the two taps of the upsample exchanged",
    "no_mean": "emb_mean dropped",
    "rope_ring": "the RoPE position taken as pos % ring",
    "window": "the window one key too long",
    "no_carry": "the tile carry of rows 0/1 dropped at a sequence's first tile of a frame > 0",
    "taps_rev": "the last conv's taps reversed",
    "no_bias2": "the 1x1 conv's bias dropped",
    "no_ls": "the layer scale left out of a residual add",
    "tanh_gelu": "the tanh approximation of GELU instead of the erf form",
}

# seeded defects of the split-bf16 matrix product (`_mms`, `_ln_mm`; tests/test_codec_split_reference_cpu.py)
SPLIT_MUTANTS = {
    "no_wlo": "the xh.wl term dropped (the weight's lo image never multiplied)",
    "no_xlo": "the xl.wh term dropped (the activation's residual never multiplied)",
    "fp32_w": "the site multiplies by the fp32 matrix instead of hi + lo (a silent fall-back to the fp32 kernel)",
    "lns_hi": "the LayerNorm fold's ln_s summed from the hi image alone",
    "lo_of_x_trunc": "xl formed from a truncated xh while the product uses the rounded xh",
}

CONFIG_NAMES = ("tiny", "tiny1", "nf64")
_CONFIG_EDITS = {"tiny": {}, "tiny1": dict(mimi_layers=1), "nf64": dict(n_filters=64, mimi_layers=1)}
SEQ_ELEMS = 16384  # outputs the sequential-order evaluation covers per GEMM (at least 32 rows)

_WEIGHTS = {}
_PARAMS = {}


def codec_weights(name, seed=0):
    """(cfg, W) of "tiny" (two layers, n_filters 32: stages 1 and 2 fuse, stage 3 does not, the last conv is the generic
    EPI_PCM), "tiny1" (tiny with one transformer layer) or "nf64" (tiny dimensions with n_filters 64 and one layer: the
    SEANet of the 100M model, 512 -> 256 -> 128 -> 64 channels on 16 / 96 / 480 / 1920 rows per sequence)"""
    if (name, seed) not in _WEIGHTS:
        cfg = make_config(**{**NAMED_CONFIGS["tiny"], **_CONFIG_EDITS[name]})
        _WEIGHTS[(name, seed)] = (cfg, generate_state_dict(cfg, seed))
    return _WEIGHTS[(name, seed)]


def ring_of(cfg):
    """slots of the K / V ring: the context rounded up to whole 16-row frames, plus the frame being written"""
    return ((cfg.mimi.transformer.context - 1 + 15) // 16 + 1) * 16


class _Params:
    """the decoder's tensors of one weight dict in one dtype, as the matrices the stage functions multiply by"""

    def __init__(self, cfg, W, dtype):
        self.cfg, self.W, self.dt = cfg, W, np.dtype(dtype).type
        self.layers = seanet_decoder_layers(cfg)
        self._m = {}

    def get(self, key, make):
        if key not in self._m:
            self._m[key] = np.ascontiguousarray(make()).astype(self.dt)
        return self._m[key]

    def vec(self, name):
        return self.get(name, lambda: self.W[name])

    def conv(self, p):
        """Conv1d weight [O, C, K] -> [O, K * C] with k = tap * C + c, and its bias"""
        return self.get(p + ".weight#m", lambda: (lambda w: w.transpose(0, 2, 1).reshape(w.shape[0], -1))(self.W[p + ".weight"])), \
            self.vec(p + ".bias")

    def convtr(self, p, s):
        """ConvTranspose1d weight [C, O, 2s] -> [s * O, 2 * C]: output column j * O + o of input row t is sample t * s + j;
        k < C multiplies row t (kernel index j), k >= C row t - 1 (kernel index j + s): overlap-add as a 2-tap causal conv"""

        def make():
            w = self.W[p + ".weight"]
            C, O = w.shape[0], w.shape[1]
            cur = w[:, :, :s].transpose(2, 1, 0).reshape(s * O, C)
            prev = w[:, :, s:].transpose(2, 1, 0).reshape(s * O, C)
            return np.concatenate([cur, prev], axis=1)

        return self.get(p + ".weight#m", make), self.vec(p + ".bias")


def params(cfg, W, dtype):
    key = (id(W), np.dtype(dtype).str)
    if key not in _PARAMS:
        _PARAMS[key] = (W, _Params(cfg, W, dtype))
    return _PARAMS[key][1]


# ---- arithmetic pieces ----------------------------------------------------------------------------------------------------
def _seq_rows(M, N):
    n = min(M, max(32, SEQ_ELEMS // max(N, 1)))
    return np.unique(np.linspace(0, M - 1, n).astype(np.int64))


def _mm(x, w, b, order, split=None):
    """x [..., K] @ w[N, K]^T + b in x's dtype; order "seq": rows `_seq_rows` by a plain sequential sum over k.
    split: None, or the product in the split-bf16 model (`_mms`)"""
    if split is not None:
        return _mms(x, w, b, order, split)
    lead, K = x.shape[:-1], x.shape[-1]
    X = np.ascontiguousarray(x.reshape(-1, K))
    y = X @ w.T
    if order == "seq":
        rows = _seq_rows(X.shape[0], w.shape[0])
        xs, wt = np.ascontiguousarray(X[rows].T), np.ascontiguousarray(w.T)  # [K, R], [K, N]
        acc = np.zeros((len(rows), w.shape[0]), X.dtype)
        tmp = np.empty_like(acc)
        for k in range(K):
            np.multiply(xs[k][:, None], wt[k][None, :], out=tmp)
            np.add(acc, tmp, out=acc)
        y[rows] = acc
    if b is not None:
        y = y + b
    assert y.dtype == x.dtype
    return y.reshape(lead + (w.shape[0],))


def split_parts(v, lo_of_trunc=False):
    """fp32 v -> (hi, lo) as float64: hi = bf16(v), lo = bf16(v - hi), round to nearest even (v - hi is exact in fp32:
    to_bf16x4(a - from_bf16x4(ah)), ptts_split.hip / ptts_kernels.h).  lo_of_trunc (a seeded defect): lo formed from the
    TRUNCATED hi while the rounded hi is returned"""
    v32 = np.ascontiguousarray(v, dtype=np.float32)
    hi = bf16(v32)
    base = bf16(v32, trunc=True) if lo_of_trunc else hi
    return hi, bf16((v32.astype(np.float64) - base).astype(np.float32))


_WSPLIT = {}


def _wsplit(w):
    """the hi / lo images of a weight matrix in its own dtype (remembered per array)"""
    if id(w) not in _WSPLIT:
        hi, lo = split_parts(w)
        _WSPLIT[id(w)] = (w, hi.astype(w.dtype), lo.astype(w.dtype))
    return _WSPLIT[id(w)][1:]


def _mms(x, w, b, order, split=""):
    """the matrix product of gemm_kernel<.., WF = 3> (include/ptts.h PTTS_CODEC_SPLIT, the header of ptts_split.hip): with
    xh = bf16(x), xl = bf16(x - xh), wh = bf16(w), wl = bf16(w - wh):  xh.wh + xl.wh + xh.wl  (no xl.wl term), summed in x's
    dtype; every product of two bf16 values is exact in float32.  split: "" or a SPLIT_MUTANTS name"""
    assert split == "" or split in SPLIT_MUTANTS, split
    if split == "fp32_w":
        return _mm(x, w, b, order)
    xh, xl = (a.astype(x.dtype) for a in split_parts(x, split == "lo_of_x_trunc"))
    wh, wl = _wsplit(w)
    acc = _mm(xh, wh, None, order)
    if split != "no_xlo":
        acc = acc + _mm(xl, wh, None, order)
    if split != "no_wlo":
        acc = acc + _mm(xh, wl, None, order)
    return acc if b is None else acc + b


def _ln_site(cfg, W, site, dtype):
    """(in-projection or linear1 weight, LayerNorm gain, LayerNorm bias) of the +ln site ("qkv" | "ff1", layer)"""
    P, p = params(cfg, W, dtype), f"mimi.decoder_transformer.transformer.layers.{site[1]}"
    wn, nn = (".self_attn.in_proj.weight", ".norm1") if site[0] == "qkv" else (".linear1.weight", ".norm2")
    return P, p + wn, P.vec(p + wn), P.vec(p + nn + ".weight"), P.vec(p + nn + ".bias")


def _stats(x, alt):
    dt = x.dtype.type
    mu = x.mean(axis=-1, keepdims=True)
    if alt:
        var = np.maximum((x * x).mean(axis=-1, keepdims=True) - mu * mu, dt(0))
    else:
        var = ((x - mu) * (x - mu)).mean(axis=-1, keepdims=True)
    return mu, dt(1) / np.sqrt(var + dt(1e-5))


def fold_image(cfg, W, site, dtype):
    """the matrix a +ln site multiplies by: the FLOAT32 product w * ln_w (pack_lin), in `dtype`"""
    _, key, w0, g, _ = _ln_site(cfg, W, site, F32)
    return params(cfg, W, dtype).get(key + "#fold", lambda: w0 * g[None, :])


def _ln_mm(cfg, W, site, x, dtype, order, alt, split):
    """linear(norm(x)) of a +ln site, no bias.  split None: LayerNorm, then the product.  Else what a split engine's +ln
    launch evaluates: statistics mu, rs of the UNROUNDED row, the split product of the raw row with the folded image, then
    (acc - ln_s mu) rs + ln_c with ln_s = sum_k of the fp32 image and ln_c = W ln_b (fold_ln_kernel; build_engine leaves
    both as the fp32 codec has them).  "lns_hi" (a seeded defect): ln_s summed from the hi image alone"""
    _, _, w0, g, beta = _ln_site(cfg, W, site, dtype)
    if split is None:
        return _mm(_layer_norm(x, g, beta, alt), w0, None, order)
    wf = fold_image(cfg, W, site, dtype)
    mu, rs = _stats(x, alt)
    acc = _mms(x, wf, None, order, "" if split == "lns_hi" else split)
    s = (_wsplit(wf)[0] if split == "lns_hi" else wf).sum(axis=1)
    c = _mm(beta[None, :], w0, None, order)[0]
    return (acc - mu * s) * rs + c


def _elu(x, alt):
    neg = np.minimum(x, 0)
    return np.where(x > 0, x, np.exp(neg) - 1 if alt else np.expm1(neg))


def _gelu(x, tanh=False):
    dt = x.dtype.type
    if tanh:
        return dt(0.5) * x * (dt(1) + np.tanh(dt(math.sqrt(2.0 / math.pi)) * (x + dt(0.044715) * x * x * x)))
    return x * dt(0.5) * (dt(1) + _erf(x * dt(1.0 / math.sqrt(2.0))).astype(x.dtype))


def _layer_norm(x, w, b, alt):
    dt = x.dtype.type
    mu = x.mean(axis=-1, keepdims=True)
    if alt:
        var = np.maximum((x * x).mean(axis=-1, keepdims=True) - mu * mu, dt(0))
    else:
        var = ((x - mu) * (x - mu)).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + dt(1e-5)) * w + b


def _halo(x, tail, n, mutate):
    """[B, n + T, C]: the frame behind the last n rows of the previous one"""
    tail = np.asarray(tail)[:, -n:]
    assert tail.shape == (x.shape[0], n, x.shape[2]), (tail.shape, x.shape, n)
    tail = tail.astype(x.dtype)
    if mutate == "parity":
        tail = x[:, -n:]
    elif mutate == "seqcut":
        tail = np.concatenate([tail[:1], x[:-1, -n:]], axis=0)
    elif mutate == "no_carry":
        tail = np.zeros_like(tail)
    return np.concatenate([tail, x], axis=1)


def _im2col(xx, K):
    T = xx.shape[1] - K + 1
    return np.concatenate([xx[:, k : k + T] for k in range(K)], axis=-1)


def _check(mutate, allowed):
    assert mutate is None or mutate in allowed, (mutate, allowed)


def _in(x, dtype):
    return np.asarray(x).astype(dtype)


# ---- the stages --------------------------------------------------------------------------------------------------------
def stage_P(cfg, W, lat, lat_prev, live, dtype=F64, order="np", alt=False, mutate=None):
    """de-normalisation, quantizer projection and the depthwise x16 transposed conv (kernel 32, stride 16) on one input
    step: out[b, t, c] = zq[b, c] w[c, t] + zq_prev[b, c] w[c, 16 + t].  live[b] False: no previous frame (zq_prev = 0)"""
    _check(mutate, ("up_swap", "no_mean"))
    P = params(cfg, W, dtype)
    s = cfg.upsample_stride
    std, mean = P.vec("flow_lm.emb_std"), P.vec("flow_lm.emb_mean")
    wq = P.get("quant#m", lambda: W["mimi.quantizer.output_proj.weight"][:, :, 0])
    wu = P.get("up#m", lambda: W["mimi.upsample.convtr.convtr.weight"][:, 0, :])  # [C, 2s]

    def zq(z):
        z = _in(z, dtype) * std
        return _mm(z if mutate == "no_mean" else z + mean, wq, None, order)

    zc = zq(lat)
    zp = zq(lat_prev) * np.asarray(live, bool)[:, None].astype(dtype)
    w_cur, w_prev = wu[:, :s], wu[:, s:]
    if mutate == "up_swap":
        w_cur, w_prev = w_prev, w_cur
    return zc[:, None, :] * w_cur.T[None] + zp[:, None, :] * w_prev.T[None]


def _rope(x, pos, max_period, dtype):
    """interleaved-pair rotary embedding of x [B, T, H, D] at the integer positions pos [B, T]; float32 angle"""
    D = x.shape[-1]
    ds = np.arange(D // 2, dtype=F32)
    # the correctly rounded float32 exp of the float32 argument.  numpy's own float32 exp is one ulp off in 13 of the 32
    # entries at max_period 10000 (torch's in one, glibc's expf in none), which moves an angle by 4e-6 at position 271: more
    # than a stage's E32 once it multiplies a query (tests/test_gpu_voice_matrix.py, stage Q)
    freqs = np.exp((ds * F32(-math.log(max_period) * 2 / D)).astype(F64)).astype(F32)
    ang = (freqs[None, None, :] * pos.astype(F32)[:, :, None]).astype(F32).astype(dtype)  # the float32 product
    c, s = np.cos(ang)[:, :, None, :], np.sin(ang)[:, :, None, :]
    xr, xi = x[..., 0::2], x[..., 1::2]
    out = np.empty_like(x)
    out[..., 0::2] = xr * c - xi * s
    out[..., 1::2] = xr * s + xi * c
    return out


_TR_MEMO = {}


def _transformer(cfg, W, ups, start, dtype, order, alt, mutate, n_layers=None, split=None):
    """the decoder transformer on the frames `ups` (upsample taps [B, 16, C] of frames 0 .. f), streaming: every frame
    attends to the keys of the frames before it.  start[b]: the frame sequence b's utterance began at (position 0; keys
    of earlier frames are not its own).  -> the last layer's taps of frame f.
    A pure function of its arguments; the K / V of a prefix of frames it has already seen (the same arrays at the same
    positions) are remembered, so that judging frame after frame costs one frame each.
    split: None, or the four GEMMs of every layer in the split-bf16 model (`_mms`, `_fold_split`; "" or a SPLIT_MUTANTS name)"""
    P = params(cfg, W, dtype)
    tr = cfg.mimi.transformer
    H, Dh, ctx = tr.num_heads, tr.d_model // tr.num_heads, tr.context
    L = tr.num_layers if n_layers is None else n_layers
    B, T, C = np.asarray(ups[0]).shape
    start = np.zeros(B, np.int64) if start is None else np.asarray(start, np.int64)
    dt = np.dtype(dtype).type
    key = (id(W), np.dtype(dtype).str, order, alt, mutate, L, split)
    done = []  # per frame: dict(pos, kv = [(k, v) per layer], taps)
    for f, u in enumerate(ups):
        new = f >= start  # [B]: the frame belongs to the sequence's current utterance (else to the one before it)
        pos = (16 * np.where(new, f - start, f))[:, None] + np.arange(T)[None, :]  # [B, T]
        key = key + (id(u), pos[:, 0].tobytes())
        if key in _TR_MEMO:
            done = _TR_MEMO[key][1]
            continue
        x = _in(u, dtype)
        rp = pos % ring_of(cfg) if mutate == "rope_ring" else pos
        fr = dict(pos=pos, kv=[])
        for l in range(L):
            p = f"mimi.decoder_transformer.transformer.layers.{l}"
            x_in = x
            qkv = _ln_mm(cfg, W, ("qkv", l), x, dtype, order, alt, split).reshape(B, T, 3, H, Dh)
            q = _rope(qkv[:, :, 0], rp, float(tr.max_period), dtype)
            fr["kv"].append((_rope(qkv[:, :, 1], rp, float(tr.max_period), dtype), qkv[:, :, 2]))
            hist = done + [fr]
            K = np.concatenate([g["kv"][l][0] for g in hist], axis=1)
            V = np.concatenate([g["kv"][l][1] for g in hist], axis=1)
            pk = np.concatenate([g["pos"] for g in hist], axis=1)
            own = np.concatenate([np.repeat((n >= start)[:, None], T, axis=1) for n in range(len(hist))], axis=1)
            delta = pos[:, :, None] - pk[:, None, :]  # [B, Tq, Tk]
            mask = (delta >= 0) & (delta < ctx + (1 if mutate == "window" else 0))
            mask &= own[:, None, :] == new[:, None, None]  # keys of the same utterance only
            sc = np.einsum("bqhd,bkhd->bhqk", q, K) * dt(1.0 / math.sqrt(Dh))
            sc = np.where(mask[:, None], sc, dt(-np.inf))
            sc = sc - sc.max(axis=-1, keepdims=True)
            pr = np.exp(sc)
            pr = pr / pr.sum(axis=-1, keepdims=True)
            ao = np.einsum("bhqk,bkhd->bqhd", pr, V).reshape(B, T, C)
            resid = x + P.vec(p + ".layer_scale_1.scale") * _mm(ao, P.vec(p + ".self_attn.out_proj.weight"), None, order, split)
            ff = _gelu(_ln_mm(cfg, W, ("ff1", l), resid, dtype, order, alt, split))
            x = resid + P.vec(p + ".layer_scale_2.scale") * _mm(ff, P.vec(p + ".linear2.weight"), None, order, split)
        fr["taps"] = dict(attn=ao, resid=resid, ff=ff, out=x, inp=x_in)
        done = done + [fr]
        if len(_TR_MEMO) > 256:
            _TR_MEMO.clear()
        _TR_MEMO[key] = (list(ups[: f + 1]), done)  # the arrays stay alive with their ids
    taps = done[-1]["taps"]
    assert all(v.dtype == dt for v in taps.values())
    return taps


def stage_A(cfg, W, ups, start=None, dtype=F64, order="np", alt=False, mutate=None, split=None):
    """one-layer configurations: LayerNorm + in_proj + RoPE + the K / V history + attention -> attention output"""
    _check(mutate, ("rope_ring", "window"))
    assert cfg.mimi.transformer.num_layers == 1, "stage A is defined on the one-layer configurations"
    return _transformer(cfg, W, ups, start, dtype, order, alt, mutate, split=split)["attn"]


def stage_T(cfg, W, ups, start=None, dtype=F64, order="np", alt=False, mutate=None, split=None):
    """the whole decoder transformer: upsample history -> dec_tr"""
    _check(mutate, ("rope_ring", "window"))
    return _transformer(cfg, W, ups, start, dtype, order, alt, mutate, split=split)["out"]


def _last(cfg):
    return f"mimi.decoder_transformer.transformer.layers.{cfg.mimi.transformer.num_layers - 1}"


def stage_B(cfg, W, attn, x, dtype=F64, order="np", alt=False, mutate=None, split=None):
    """x + layer_scale_1 * out_proj(attention output) of the last layer (one-layer configurations: x = upsample)"""
    _check(mutate, ("no_ls",))
    P, p = params(cfg, W, dtype), _last(cfg)
    return _in(x, dtype) + (1 if mutate == "no_ls" else P.vec(p + ".layer_scale_1.scale")) * _mm(_in(attn, dtype), P.vec(p + ".self_attn.out_proj.weight"), None, order, split)


def stage_C(cfg, W, resid, dtype=F64, order="np", alt=False, mutate=None, split=None):
    """GELU(linear1(norm2(x))) of the last layer"""
    _check(mutate, ("tanh_gelu",))
    l = cfg.mimi.transformer.num_layers - 1
    return _gelu(_ln_mm(cfg, W, ("ff1", l), _in(resid, dtype), dtype, order, alt, split), mutate == "tanh_gelu")


def stage_D(cfg, W, ff, resid, dtype=F64, order="np", alt=False, mutate=None, split=None):
    """x + layer_scale_2 * linear2(ff) of the last layer: the transformer's output"""
    _check(mutate, ("no_ls",))
    P, p = params(cfg, W, dtype), _last(cfg)
    return _in(resid, dtype) + (1 if mutate == "no_ls" else P.vec(p + ".layer_scale_2.scale")) * _mm(_in(ff, dtype), P.vec(p + ".linear2.weight"), None, order, split)


def _layer_of(cfg, kind, i):
    """(ModuleList index, cin, cout, kernel, stride) of SEANet stage i's layer of `kind` (i = 0: first / last conv)"""
    found = [l for l in seanet_decoder_layers(cfg) if l[1] == kind]
    idx, _, cin, cout, k, stride = found[i - 1] if kind != "conv" else found[i]
    return idx, cin, cout, k, stride


def stage_S0(cfg, W, x, tail, dtype=F64, order="np", alt=False, mutate=None, split=None):
    """ELU(k7 streaming conv of the transformer's output); tail: the last 6 rows of the previous frame's dec_tr"""
    _check(mutate, ("parity", "seqcut"))
    P = params(cfg, W, dtype)
    idx, _, _, K, _ = _layer_of(cfg, "conv", 0)
    w, b = P.conv(f"mimi.decoder.model.{idx}.conv")
    return _elu(_mm(_im2col(_halo(_in(x, dtype), tail, K - 1, mutate), K), w, b, order, split), alt)


def stage_Cv(cfg, W, i, x, tail, dtype=F64, order="np", alt=False, mutate=None, split=None):
    """stage i's transposed conv (kernel 2s, stride s) of the ELU'd input: raw output [B, T * s, cout]; tail: the last
    row of the previous frame's input"""
    _check(mutate, ("parity", "seqcut", "elu_twice"))
    P = params(cfg, W, dtype)
    idx, _, cout, _, s = _layer_of(cfg, "convtr", i)
    w, b = P.convtr(f"mimi.decoder.model.{idx}.convtr", s)
    xx = _halo(_in(x, dtype), tail, 1, mutate)
    if mutate == "elu_twice":
        xx = _elu(xx, alt)
    B, T = x.shape[0], x.shape[1]
    y = _mm(np.concatenate([xx[:, 1:], xx[:, :-1]], axis=-1), w, np.tile(b, s), order, split)
    return y.reshape(B, T * s, cout)


def _resblock(P, cfg, i, xx, alt, order, mutate):
    """ELU(x + conv1x1(ELU(conv3(ELU(x))))) on the rows behind the 2 halo rows of xx"""
    idx = _layer_of(cfg, "res", i)[0]
    p = f"mimi.decoder.model.{idx}.block"
    w1, b1 = P.conv(p + ".1.conv")
    w2, b2 = P.conv(p + ".3.conv")
    h = _elu(_mm(_im2col(_elu(xx, alt), 3), w1, b1, order), alt)
    v = _mm(h, w2, None if mutate == "no_bias2" else b2, order)
    skip = xx[:, 2:]
    return _elu((_elu(skip, alt) if mutate == "skip_elu" else skip) + v, alt)


def stage_R(cfg, W, i, x, tail, dtype=F64, order="np", alt=False, mutate=None):
    """stage i's residual block on the RAW transposed-conv output; tail: the last 2 rows of the previous frame's"""
    _check(mutate, ("parity", "seqcut", "skip_elu", "no_bias2"))
    P = params(cfg, W, dtype)
    return _resblock(P, cfg, i, _halo(_in(x, dtype), tail, 2, mutate), alt, order, mutate)


def _last_conv(P, cfg, xx, order, mutate):
    idx, _, _, K, _ = _layer_of(cfg, "conv", 1)
    w, b = P.conv(f"mimi.decoder.model.{idx}.conv")
    if mutate == "taps_rev":
        C = w.shape[1] // K
        w = np.ascontiguousarray(w.reshape(1, K, C)[:, ::-1].reshape(1, K * C))
    return _mm(_im2col(xx, K), w, b, order)[..., 0]


def stage_L(cfg, W, x, tail, dtype=F64, order="np", alt=False, mutate=None):
    """the last conv (k3, n_filters -> 1 sample) of the ELU'd block output -> PCM [B, T]; tail: last 2 rows of the
    previous frame's"""
    _check(mutate, ("parity", "seqcut", "no_carry", "taps_rev"))
    P = params(cfg, W, dtype)
    return _last_conv(P, cfg, _halo(_in(x, dtype), tail, 2, mutate), order, mutate)


def stage_R3L(cfg, W, x, tail, live, dtype=F64, order="np", alt=False, mutate=None):
    """stage 3's residual block and the last conv as one operation: seanet8 -> PCM.  tail: the last 4 rows of the previous
    frame's seanet8 (2 for the block's halo + 2 block outputs for the last conv's); live[b] False: no previous frame, the
    last conv's halo is zero (not the block applied to zeros)"""
    _check(mutate, ("no_carry", "taps_rev", "skip_elu", "no_bias2"))
    P = params(cfg, W, dtype)
    ext = _resblock(P, cfg, 3, _halo(_in(x, dtype), tail, 4, None), alt, order, mutate)  # [B, 2 + T, C]
    keep = np.asarray(live, bool)[:, None, None].astype(dtype)
    if mutate == "no_carry":
        keep = np.zeros_like(keep)
    xx = np.concatenate([ext[:, :2] * keep, ext[:, 2:]], axis=1)
    return _last_conv(P, cfg, xx, order, mutate)


def _conv_stage(fn, i):
    def run(cfg, W, *a, **kw):
        return fn(cfg, W, i, *a, **kw)

    run.__doc__ = fn.__doc__
    return run


STAGES = {"P": stage_P, "A": stage_A, "B": stage_B, "C": stage_C, "D": stage_D, "T": stage_T, "S0": stage_S0,
          "C1": _conv_stage(stage_Cv, 1), "C2": _conv_stage(stage_Cv, 2), "C3": _conv_stage(stage_Cv, 3),
          "R1": _conv_stage(stage_R, 1), "R2": _conv_stage(stage_R, 2), "R3": _conv_stage(stage_R, 3),
          "L": stage_L, "R3L": stage_R3L}
# the engine's tap each stage produces ("pcm": the decode's output) and the one the conv stages read
OUTPUT_TAP = {"P": "upsample", "A": "tr_attn", "B": "tr_resid", "C": "tr_ff", "D": "dec_tr", "T": "dec_tr", "S0": "seanet0",
              "C1": "seanet2", "R1": "seanet3", "C2": "seanet5", "R2": "seanet6", "C3": "seanet8", "R3": "seanet9",
              "L": "pcm", "R3L": "pcm"}
CONV_CHAIN = (("S0", "dec_tr", 6), ("C1", "seanet0", 1), ("R1", "seanet2", 2), ("C2", "seanet3", 1), ("R2", "seanet5", 2),
              ("C3", "seanet6", 1), ("R3", "seanet8", 2), ("L", "seanet9", 2))  # (stage, input tap, halo rows)
F32_VARIANTS = (("np", False), ("seq", True))  # (summation order, the kernels' forms of variance and ELU)


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


def stage_inputs(stage, cfg, W, frames, f, start=None):
    """keyword arguments of `STAGES[stage]` at frame f.  frames[g]: the taps of frame g as [B, T, C] arrays under the
    engine's tap names, plus "latent" [B, ldim]; start[b]: the frame sequence b's utterance began at (default 0).  Tails
    come from frames[f - 1] and are zero for the sequences that have no previous frame."""
    cur = frames[f]
    B = np.asarray(cur["latent"]).shape[0]
    start = np.zeros(B, np.int64) if start is None else np.asarray(start, np.int64)
    live = start < f
    kw = dict(cfg=cfg, W=W)

    def tail(name, n):
        x = np.asarray(cur[name])
        if f == 0:
            return np.zeros_like(x[:, :n])
        return np.asarray(frames[f - 1][name])[:, -n:] * live[:, None, None].astype(x.dtype)

    if stage == "P":
        return dict(kw, lat=cur["latent"], lat_prev=frames[f - 1]["latent"] if f else cur["latent"], live=live)
    if stage in ("A", "T"):
        return dict(kw, ups=[frames[g]["upsample"] for g in range(f + 1)], start=start)
    if stage == "B":
        return dict(kw, attn=cur["tr_attn"], x=cur["upsample"])
    if stage == "C":
        return dict(kw, resid=cur["tr_resid"])
    if stage == "D":
        return dict(kw, ff=cur["tr_ff"], resid=cur["tr_resid"])
    if stage == "R3L":
        return dict(kw, x=cur["seanet8"], tail=tail("seanet8", 4), live=live)
    src, n = {st: (tap, rows) for st, tap, rows in CONV_CHAIN}[stage]
    return dict(kw, x=cur[src], tail=tail(src, n))


# ---- the stages chained: a decoder that carries the taps of the previous frame ----------------------------------------
class Chain:
    """The stage functions chained on their own outputs: latent -> taps and PCM of a frame, frame after frame.  In float32
    it is `np_oracle.MimiDecoder.decode` (tests/test_mimi_reference_cpu.py); in float64 the reference of the decodes
    whose intermediate buffers stay on chip."""

    def __init__(self, cfg, W, B, dtype=F64, order="np", alt=False, fused_tail=False, split=None, split_res=()):
        self.cfg, self.W, self.B = cfg, W, B
        self.kw = dict(dtype=dtype, order=order, alt=alt)
        self.fused_tail = fused_tail  # PCM through stage R3L instead of R3 and L
        # a split-bf16 engine: the transformer's GEMMs, conv0, the transposed convs and the residual blocks of the stages
        # in split_res (the unfused Ra / Rb pair) in the split model, everything else as the fp32 stages
        self.split, self.split_res = split, tuple(split_res)
        assert split is None or not fused_tail
        self.frame = 0
        self.start = np.zeros(B, np.int64)
        self.ups, self.lat_prev, self.prev = [], None, None

    def reset_row(self, row):
        """a new utterance joins in `row`: zero tails, position 0"""
        self.start[row] = self.frame

    def decode(self, lat):
        cfg, W, kw = self.cfg, self.W, self.kw
        live = self.start < self.frame
        t = {"latent": np.asarray(lat)}
        t["upsample"] = stage_P(cfg, W, lat, lat if self.lat_prev is None else self.lat_prev, live, **kw)
        self.ups.append(t["upsample"])
        tr = _transformer(cfg, W, self.ups, self.start, mutate=None, split=self.split, **kw)  # stage T, with the last layer's taps
        t.update(tr_attn=tr["attn"], tr_resid=tr["resid"], tr_ff=tr["ff"], dec_tr=tr["out"])
        if cfg.mimi.transformer.num_layers > 1:
            t[f"tr_in{cfg.mimi.transformer.num_layers - 1}"] = tr["inp"]  # the last layer's input
        keep = live[:, None, None].astype(t["dec_tr"].dtype)

        def tail(name, n):
            cur = t[name]
            return np.zeros_like(cur[:, :n]) if self.prev is None else self.prev[name][:, -n:] * keep

        for stage, src, n in CONV_CHAIN[:-2] if self.fused_tail else CONV_CHAIN:
            if self.split is not None and stage[0] == "R" and int(stage[1]) in self.split_res:
                i, c = int(stage[1]), f"seanet_c{stage[1]}"
                t[c] = _elu(t[src], kw["alt"])  # the ELU'd copy the transposed conv stores beside the raw one
                h = stage_Ra(cfg, W, i, t[c], tail(c, 2), split=self.split, **kw)
                t[OUTPUT_TAP[stage]] = stage_Rb(cfg, W, i, h, t[src], split=self.split, **kw)
            elif self.split is not None and stage in ("S0", "C1", "C2", "C3"):
                t[OUTPUT_TAP[stage]] = STAGES[stage](cfg, W, t[src], tail(src, n), split=self.split, **kw)
            else:
                t[OUTPUT_TAP[stage]] = STAGES[stage](cfg, W, t[src], tail(src, n), **kw)
        if self.fused_tail:
            t["pcm"] = stage_R3L(cfg, W, t["seanet8"], tail("seanet8", 4), live, **kw)
        self.prev, self.lat_prev = t, np.asarray(lat)
        self.frame += 1
        return t


def chain_e32(cfg, W, latents, fused_tail=False, resets=(), **split_kw):
    """latents [F, B, ldim] -> per frame (pcm64, E32): the fp64 chain's PCM and the worst float32 error of the same chain
    over F32_VARIANTS.  resets: (frame, row) pairs of `reset_row` calls issued before that frame; split_kw: `Chain`'s
    split / split_res"""
    B = latents.shape[1]
    chains = [Chain(cfg, W, B, fused_tail=fused_tail, **split_kw)] + \
        [Chain(cfg, W, B, F32, o, a, fused_tail, **split_kw) for o, a in F32_VARIANTS]
    out = []
    for f, lat in enumerate(latents):
        for fr, row in resets:
            if fr == f:
                for c in chains:
                    c.reset_row(row)
        pcm = [c.decode(lat)["pcm"] for c in chains]
        e32 = max(float(np.abs(p.astype(np.float64) - pcm[0]).max()) for p in pcm[1:])
        assert e32 > 0
        out.append((pcm[0], e32))
    return out


def seeded_latents(cfg, F, B, seed, scale=1.0):
    """[F, B, ldim] float32 ~ scale * N(0, 1): different latents per frame and sequence"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((F, B, cfg.mimi.quantizer.dimension)) * scale).astype(np.float32)


# ---- the reduced-precision codecs (codec_bf16, codec_fp8): one stateless function per LAUNCH ----------------------------
# mimi_enqueue_h (csrc/ptts_codec.hip) launches, per transformer layer l, Q (+ln GEMM with EPI_QKV), A (attention), B
# (out_proj + residual), C (+ln GEMM, GELU), D (linear2 + residual), after the prologue P; then S0 (conv0), per SEANet stage
# i = 1..3 Cv (transposed conv, raw and ELU'd outputs), Ra (k3 conv), Rb (1x1 conv + skip), and L (the last conv).
#
# Every input is what was read back from the device (`Engine.debug_read`), so it is exactly representable: bf16 values, or
# for the operands of the fp8 convolutions e4m3 CODES (value = code * scales[k], k from SC_IN).  A function returns the
# launch's outputs BEFORE the output rounding (`OUT_KIND`, `out_round`), in `dtype`.  The only roundings inside are the ones
# the kernels make:
#   * the weight image: bf16 RNE of the fp32 weight (pack_weight_h_kernel, ptts_bf16.h:40), for a +ln site of the fp32
#     product w * ln_w (ptts_bf16.h:34); or e4m3 of w * (1 / scale) with scale = amax / 448 per output row, all fp32
#     (pack_weight_f8_kernel, ptts_fp8.hip:46,53-55);
#   * +ln sites: y = rs * (W' x - mu * sum_k W'[n][k]) + c with the sum over the ROUNDED image (fold_s_h_kernel,
#     ptts_bf16.h:44-55; restated as W' ((x - mu) rs) + c, which is the same number when the two sums agree), c = W ln_b from
#     the unrounded weights (fold_ln_kernel), and fp32 statistics mu, E[x^2] - mu^2 of the bf16 operand (ptts_bf16.h:171-179,
#     207-210);
#   * fp8 sites: acc * (wscale * xs), the fp32 product wscale * xs first (gemm_f8_epilogue, ptts_fp8.hip:90);
#   * the output: bf16 RNE (to_bf16x4, ptts_bf16.h:70,75,108); or v * yinv, yinv = 1 / scales[k] in fp32, clamped to +-448 and
#     rounded to e4m3 (to_f8x4, ptts_kernels.h:37; ptts_bf16.h:69, ptts_fp8.hip:83); the PCM stays fp32.
# `ident=True` replaces every one of these roundings by the identity: the functions are then the fp64 stages above.
import torch  # noqa: E402  (bf16 / e4m3 conversions)

import codec_ref as _CR  # noqa: E402
from gemm_ref import bf16_round as _bf16_round  # noqa: E402

FMTS = ("bf16", "fp8")
E4M3_MAX = 448.0
FMT_MUTANTS = {
    "sc_in_next": "sc_in of a transposed conv read from the next scale index",
    "no_yinv": "yinv left at 1 on one conv",
    "wrap": "an e4m3 output converted without the clamp to +-448 (magnitudes past the format's top come out as 0x7f, NaN)",
    "skip_elu": "the residual block's skip taken from the ELU'd copy instead of the raw one",
    "elu_twice": "ELU applied again on the operand of a transposed or k3 conv",
    "no_bias2": "the 1x1 conv's bias dropped",
    "tensor_scale": "one weight scale per tensor instead of one per output channel",
    "trunc": "a bf16 output truncated instead of rounded to nearest even",
    "ln_s_unrounded": "the LayerNorm fold's ln_s summed from the unrounded weights",
    "parity": "the halo read from the current frame's parity slot",
    "k_layer0": "layer 1 attending over layer 0's K ring",
}
# index of the activation scale an fp8 convolution reads its operand with / writes its e4m3 output with (ptts_host.h:142:
# 0 conv0's output, 3 i - 2 stage i's transposed conv (ELU'd), 3 i - 1 its hidden activation, 3 i its block output, i < 3)
SC_IN = {("convtr", 1): 0, ("convtr", 2): 3, ("convtr", 3): 6, **{("res_a", i): 3 * i - 2 for i in (1, 2, 3)},
         **{("res_b", i): 3 * i - 1 for i in (1, 2, 3)}}
SC_OUT = {("conv0",): 0, **{("convtr", i): 3 * i - 2 for i in (1, 2, 3)}, **{("res_a", i): 3 * i - 1 for i in (1, 2, 3)},
          ("res_b", 1): 3, ("res_b", 2): 6}
SC_USED = sorted(set(SC_OUT.values()))
_CONFIG_EDITS["nf64x2"] = dict(n_filters=64, mimi_layers=2)  # nf64 with two layers: the layer-to-layer hand-over


def bf16(x, trunc=False):
    """fp32 -> bf16 values (float64): round to nearest even, or (a seeded defect) truncation"""
    x32 = np.ascontiguousarray(x, dtype=np.float32)
    if trunc:
        return (x32.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)
    return _bf16_round(torch.from_numpy(x32)).numpy()  # gemm_ref's


def e4m3(x, clamp=True):
    """fp32 -> OCP e4m3fn codes (float64), after the kernels' clamp to +-448"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if clamp:
        return _CR.e4m3(t).numpy()  # codec_ref's
    return t.to(torch.float8_e4m3fn).to(torch.float64).numpy()  # the seeded defect: no clamp


def f32_div(a, b):
    return (np.asarray(a, np.float64) / np.asarray(b, np.float64)).astype(np.float32)


def is_bf16(x):
    x = np.asarray(x, np.float32)
    return bool(np.array_equal(bf16(x), x.astype(np.float64)))


def is_e4m3(x):
    x = np.asarray(x, np.float32)
    return bool(np.isfinite(x).all() and np.array_equal(e4m3(x), x.astype(np.float64)))


def yinv_of(scales, k):
    """1.0f / f8s[k] (ptts_codec.hip, f8_conv)"""
    return f32_div(1.0, np.float32(scales[k]))


def out_round(pre, kind, yinv=None, mutate=None):
    """the output rounding of a launch: kind "bf16", "e4m3" (codes of pre * yinv) or "f32" -> float64"""
    if kind == "f32":
        return np.asarray(pre, np.float32).astype(np.float64)
    if kind == "bf16":
        return bf16(pre, trunc=mutate == "trunc")
    y = np.asarray(pre, np.float32) * (np.float32(1) if mutate == "no_yinv" else np.float32(yinv))
    return e4m3(y, clamp=mutate != "wrap")


_SITES = {}


def _lp(l):
    return f"mimi.decoder_transformer.transformer.layers.{l}"


def site_weights(cfg, W, site, mode, mutate=None):
    """(w [N, K] float64, bias or ln_c [N] float64 or None, wscale [N] float32 or None) of one GEMM site; mode "ident"
    (the unrounded weights), "f32" (what the packer rounds), "bf16" or "fp8" (e4m3 CODES and their per-row scale; the same
    arithmetic as codec_ref.quant_weight_f8, which returns the codes times the scale: compared bitwise on the CPU).  K runs tap-major, oldest input row first;
    a transposed conv's rows are j * cout + o, its first C columns multiply the current input row"""
    key = (id(W), site, mode, mutate)
    if key in _SITES:
        return _SITES[key][1:]
    P = params(cfg, W, F32)
    kind = site[0]
    bias = None
    if kind in ("qkv", "ff1"):
        p = _lp(site[1])
        wn, nn = (".self_attn.in_proj.weight", ".norm1") if kind == "qkv" else (".linear1.weight", ".norm2")
        w0 = P.vec(p + wn)
        w32 = w0 * P.vec(p + nn + ".weight")[None, :]  # the fp32 product
        if mode == "ident":
            w32 = w0.astype(F64) * P.vec(p + nn + ".weight").astype(F64)[None, :]
        bias = w0.astype(F64) @ P.vec(p + nn + ".bias").astype(F64)
    elif kind in ("out", "ff2"):
        w32 = P.vec(_lp(site[1]) + (".self_attn.out_proj.weight" if kind == "out" else ".linear2.weight"))
    elif kind == "conv0":
        w32, b = P.conv(f"mimi.decoder.model.{_layer_of(cfg, 'conv', 0)[0]}.conv")
        bias = b.astype(F64)
    elif kind == "convtr":
        idx, _, _, _, s = _layer_of(cfg, "convtr", site[1])
        w32, b = P.convtr(f"mimi.decoder.model.{idx}.convtr", s)
        bias = np.tile(b, s).astype(F64)
    else:
        p = f"mimi.decoder.model.{_layer_of(cfg, 'res', site[1])[0]}.block" + (".1.conv" if kind == "res_a" else ".3.conv")
        w32, b = P.conv(p)
        bias = b.astype(F64)
    ws = None
    if mode in ("ident", "f32"):  # "f32": the fp32 matrix the packer rounds (a +ln site's fp32 product)
        w = w32.astype(F64)
    elif mode == "bf16":
        w = bf16(w32)
    else:
        amax = np.abs(w32).max(axis=1)
        if mutate == "tensor_scale":
            amax = np.full_like(amax, amax.max())
        ws = np.where(amax > 0, f32_div(amax, 448.0), np.float32(1)).astype(F32)
        inv = f32_div(1.0, ws)
        w = e4m3((w32.astype(F64) * inv.astype(F64)[:, None]).astype(F32))
    _SITES[key] = (W, w, bias, ws)
    return w, bias, ws


def _fmode(fmt, site, ident):
    return "ident" if ident else "fp8" if fmt == "fp8" and site in SC_IN else "bf16"


def _fgemm(cfg, W, fmt, site, x, scales, dtype, order, ident, mutate):
    """x [..., K] times the site's weight image, plus its bias: x holds bf16 values, or at an fp8 site e4m3 codes"""
    w, b, ws = site_weights(cfg, W, site, _fmode(fmt, site, ident), mutate if mutate == "tensor_scale" else None)
    x = _in(x, dtype)
    dt = np.dtype(dtype).type
    if fmt == "fp8" and site in SC_IN:
        k = SC_IN[site] + (1 if mutate == "sc_in_next" and site[0] == "convtr" else 0)
        xs = np.float32(scales[k])
        if ws is None:  # identity roundings: the operand's value times the unrounded weight
            acc = _mm(x * dt(xs), w.astype(dtype), None, order)
        else:
            acc = _mm(x, w.astype(dtype), None, order) * (ws * xs).astype(dtype)  # the fp32 product wscale * xs first
    else:
        acc = _mm(x, w.astype(dtype), None, order)
    return acc if b is None else acc + b.astype(dtype)


def _fold(cfg, W, fmt, site, x, dtype, order, alt, ident, mutate):
    """the +ln GEMM: fp32 statistics of the operand, the folded image, ln_c"""
    x = _in(x, dtype)
    dt = np.dtype(dtype).type
    mu = x.mean(axis=-1, keepdims=True)
    if alt:
        var = np.maximum((x * x).mean(axis=-1, keepdims=True) - mu * mu, dt(0))
    else:
        var = ((x - mu) * (x - mu)).mean(axis=-1, keepdims=True)
    rs = dt(1) / np.sqrt(var + dt(1e-5))
    if mutate == "ln_s_unrounded":
        w, c, _ = site_weights(cfg, W, site, _fmode(fmt, site, ident))
        s = site_weights(cfg, W, site, "ident")[0].sum(axis=1).astype(dtype)
        return (_mm(x, w.astype(dtype), None, order) - mu * s) * rs + c.astype(dtype)
    return _fgemm(cfg, W, fmt, site, (x - mu) * rs, None, dtype, order, ident, None)


def _tr_cfg(cfg):
    tr = cfg.mimi.transformer
    return tr, tr.num_heads, tr.d_model // tr.num_heads


def fstage_P(cfg, W, fmt, lat, lat_prev, live, dtype=F64, order="np", alt=False, mutate=None, ident=False):
    """mimi_prologue_kernel (last argument 1): fp32 weights and arithmetic, bf16 output"""
    return {"upsample": stage_P(cfg, W, lat, lat_prev, live, dtype, order, alt, mutate)}


def fstage_Q(cfg, W, fmt, l, x, pos, dtype=F64, order="np", alt=False, mutate=None, ident=False):
    """layer l's +ln GEMM with EPI_QKV on its bf16 input x [B, T, C] at the positions pos [B, T]: the queries and the K / V
    rows it writes, after RoPE, [B, T, H * 64] each; fp32 outputs (no output rounding)"""
    _check(mutate, ("ln_s_unrounded", "rope_ring"))
    tr, H, Dh = _tr_cfg(cfg)
    B, T, _ = np.asarray(x).shape
    qkv = _fold(cfg, W, fmt, ("qkv", l), x, dtype, order, alt, ident, mutate).reshape(B, T, 3, H, Dh)
    rp = pos % engine_ring(cfg) if mutate == "rope_ring" else pos
    q = _rope(qkv[:, :, 0], rp, float(tr.max_period), dtype)
    k = _rope(qkv[:, :, 1], rp, float(tr.max_period), dtype)
    return {"q": q.reshape(B, T, H * Dh), "k": k.reshape(B, T, H * Dh), "v": np.ascontiguousarray(qkv[:, :, 2]).reshape(B, T, H * Dh)}


def engine_ring(cfg):
    """slots of the engine's K / V ring (build_engine): the context in whole 16-row frames plus two frames being written"""
    return ((cfg.mimi.transformer.context - 1 + 15) // 16 + 2) * 16


def ring_positions(ring, pos0, T=16):
    """[B, ring]: the position whose key slot s holds once the frame at positions pos0 .. pos0 + T - 1 is written (the
    newest position of the slot's class), negative where the sequence has not written the slot"""
    top = np.asarray(pos0, np.int64)[:, None] + T - 1
    s = np.arange(ring)[None, :]
    return top - ((top - s) % ring)


def fstage_A(cfg, W, fmt, q, K, V, pos0, dtype=F64, order="np", alt=False, mutate=None, ident=False):
    """attention of the queries q [B, T, H * 64] (positions pos0[b] + t) over the rings K, V [B, ring, H * 64] as read back
    after the Q launch: key position p is attended when 0 <= pos_q - p < context; -> attention output (bf16 output)"""
    _check(mutate, ("window",))
    tr, H, Dh = _tr_cfg(cfg)
    B, T, C = np.asarray(q).shape
    dt = np.dtype(dtype).type
    q, K, V = (_in(a, dtype).reshape(B, -1, H, Dh) for a in (q, K, V))
    pk = ring_positions(K.shape[1], pos0, T)  # [B, ring]
    pq = np.asarray(pos0, np.int64)[:, None] + np.arange(T)[None, :]
    delta = pq[:, :, None] - pk[:, None, :]
    mask = (delta >= 0) & (delta < tr.context + (1 if mutate == "window" else 0)) & (pk >= 0)[:, None, :]
    sc = np.einsum("bqhd,bkhd->bhqk", q, K) * dt(1.0 / math.sqrt(Dh))
    sc = np.where(mask[:, None], sc, dt(-np.inf))
    sc = sc - sc.max(axis=-1, keepdims=True)
    pr = np.exp(sc)
    pr = pr / pr.sum(axis=-1, keepdims=True)
    Vz = np.where(np.isfinite(V), V, dt(0))  # slots never written may hold anything: their weight is exactly 0
    out = np.einsum("bhqk,bkhd->bqhd", pr, Vz).reshape(B, T, C)
    assert out.dtype == dt
    return {"attn": out}


def fstage_B(cfg, W, fmt, l, attn, x, dtype=F64, order="np", alt=False, mutate=None, ident=False):
    """x + layer_scale_1 * out_proj(attention output): EPI_RES with the layer scale, bf16 output"""
    _check(mutate, ("no_ls",))
    ls = 1 if mutate == "no_ls" else params(cfg, W, dtype).vec(_lp(l) + ".layer_scale_1.scale")
    return {"resid": _in(x, dtype) + ls * _fgemm(cfg, W, fmt, ("out", l), attn, None, dtype, order, ident, None)}


def fstage_C(cfg, W, fmt, l, resid, dtype=F64, order="np", alt=False, mutate=None, ident=False):
    """GELU(+ln GEMM of linear1), bf16 output"""
    _check(mutate, ("tanh_gelu", "ln_s_unrounded"))
    return {"ff": _gelu(_fold(cfg, W, fmt, ("ff1", l), resid, dtype, order, alt, ident, mutate), mutate == "tanh_gelu")}


def fstage_D(cfg, W, fmt, l, ff, resid, dtype=F64, order="np", alt=False, mutate=None, ident=False):
    """x + layer_scale_2 * linear2(ff): the layer's output, bf16"""
    _check(mutate, ("no_ls",))
    ls = 1 if mutate == "no_ls" else params(cfg, W, dtype).vec(_lp(l) + ".layer_scale_2.scale")
    return {"out": _in(resid, dtype) + ls * _fgemm(cfg, W, fmt, ("ff2", l), ff, None, dtype, order, ident, None)}


def _elu_again(xx, fmt, scales, site, alt):
    """the seeded defect "elu_twice": ELU applied once more to the (already ELU'd) operand's value"""
    xs = xx.dtype.type(np.float32(scales[SC_IN[site]])) if fmt == "fp8" else xx.dtype.type(1)
    return _elu(xx * xs, alt) / xs


def fstage_S0(cfg, W, fmt, x, tail, scales=None, dtype=F64, order="np", alt=False, mutate=None, ident=False):
    """ELU(k7 conv of the transformer's bf16 output), gemm_h in both formats; output bf16 or e4m3 (scale 0)"""
    _check(mutate, ("parity", "seqcut", "no_yinv", "wrap", "trunc"))
    K = _layer_of(cfg, "conv", 0)[3]
    cols = _im2col(_halo(_in(x, dtype), tail, K - 1, mutate), K)
    return {"a0": _elu(_fgemm(cfg, W, fmt, ("conv0",), cols, scales, dtype, order, ident, None), alt)}


def fstage_Cv(cfg, W, fmt, i, x, tail, scales=None, dtype=F64, order="np", alt=False, mutate=None, ident=False):
    """stage i's transposed conv of the ELU'd input (bf16 values or e4m3 codes): the raw output (bf16, the block's skip) and
    ELU of it (bf16 or e4m3), [B, T * s, cout]"""
    _check(mutate, ("parity", "seqcut", "elu_twice", "sc_in_next", "tensor_scale", "no_yinv", "wrap", "trunc"))
    _, _, cout, _, s = _layer_of(cfg, "convtr", i)
    xx = _halo(_in(x, dtype), tail, 1, mutate)
    if mutate == "elu_twice":
        xx = _elu_again(xx, fmt, scales, ("convtr", i), alt)
    B, T = np.asarray(x).shape[:2]
    v = _fgemm(cfg, W, fmt, ("convtr", i), np.concatenate([xx[:, 1:], xx[:, :-1]], axis=-1), scales, dtype, order, ident, mutate)
    v = v.reshape(B, T * s, cout)
    return {"raw": v, "elu": _elu(v, alt)}


def fstage_Ra(cfg, W, fmt, i, x, tail, scales=None, dtype=F64, order="np", alt=False, mutate=None, ident=False):
    """stage i's k3 conv of the ELU'd transposed-conv output (tail: its last 2 rows of the previous frame), ELU'd: the
    block's hidden activation (bf16 or e4m3)"""
    _check(mutate, ("parity", "seqcut", "elu_twice", "tensor_scale", "no_yinv", "wrap", "trunc"))
    xx = _halo(_in(x, dtype), tail, 2, mutate)
    if mutate == "elu_twice":
        xx = _elu_again(xx, fmt, scales, ("res_a", i), alt)
    cols = _im2col(xx, 3)
    return {"h": _elu(_fgemm(cfg, W, fmt, ("res_a", i), cols, scales, dtype, order, ident, mutate), alt)}


def fstage_Rb(cfg, W, fmt, i, h, skip, scales=None, dtype=F64, order="np", alt=False, mutate=None, ident=False):
    """ELU(raw skip + 1x1 conv of the hidden activation): the block's output (bf16; e4m3 for i < 3 on the fp8 codec)"""
    _check(mutate, ("skip_elu", "no_bias2", "tensor_scale", "no_yinv", "wrap", "trunc"))
    skip = _in(skip, dtype)
    v = _fgemm(cfg, W, fmt, ("res_b", i), h, scales, dtype, order, ident, mutate)
    if mutate == "no_bias2":
        v = v - site_weights(cfg, W, ("res_b", i), "ident")[1].astype(dtype)
    return {"out": _elu((_elu(skip, alt) if mutate == "skip_elu" else skip) + v, alt)}


def fstage_L(cfg, W, fmt, x, tail, dtype=F64, order="np", alt=False, mutate=None, ident=False):
    """pcm_conv_h_kernel: the last conv with its fp32 weights on the bf16 block output -> fp32 PCM [B, T]"""
    return {"pcm": stage_L(cfg, W, x, tail, dtype, order, alt, mutate)}


def out_kind(fmt, site):
    """(kind, scale index or None) of the output rounding of the launch at `site` ("raw": a transposed conv's skip copy)"""
    if fmt == "fp8" and site in SC_OUT:
        return "e4m3", SC_OUT[site]
    return "bf16", None


def fstage_e32(fn, kw):
    """-> ({name: y64}, {name: E32}) of a format stage: the fp64 result and the worst float32 error of the same formulas
    on the same inputs over F32_VARIANTS, per output.  From the reference alone."""
    y64 = fn(**kw)
    e32 = {k: 0.0 for k in y64}
    for order, alt in F32_VARIANTS:
        y32 = fn(**kw, dtype=F32, order=order, alt=alt)
        for k, v in y32.items():
            assert v.dtype == np.float32 and y64[k].dtype == np.float64 and v.shape == y64[k].shape, (k, v.dtype)
            e32[k] = max(e32[k], float(np.abs(v.astype(np.float64) - y64[k]).max()))
    return y64, e32


class FChain:
    """the format stages chained on their own ROUNDED outputs: the whole decoder on the CPU in the format's arithmetic.
    decode(lat) -> the taps of the frame as the device holds them (bf16 values, e4m3 codes) under the engine's tap names.
    fmt "fp8" takes `scales` (16 floats), e.g. from `calibrate`"""

    def __init__(self, cfg, W, B, fmt, scales=None, mutate=None, mutate_at=None):
        assert fmt in FMTS and (fmt == "bf16" or scales is not None)
        self.cfg, self.W, self.B, self.fmt, self.scales = cfg, W, B, fmt, scales
        self.mutate, self.mutate_at = mutate, mutate_at  # a seeded defect at one launch (stage name)
        tr, H, Dh = _tr_cfg(cfg)
        self.L, self.ring = tr.num_layers, engine_ring(cfg)
        self.K = [np.zeros((B, self.ring, H * Dh)) for _ in range(self.L)]
        self.V = [np.zeros((B, self.ring, H * Dh)) for _ in range(self.L)]
        self.frame, self.start = 0, np.zeros(B, np.int64)
        self.lat_prev, self.prev = None, None

    def reset_row(self, row):
        self.start[row] = self.frame

    def _m(self, stage):
        return self.mutate if stage == self.mutate_at else None

    def _rnd(self, pre, site, stage):
        kind, k = out_kind(self.fmt, site)
        return out_round(pre, kind, None if k is None else yinv_of(self.scales, k), self._m(stage))

    def decode(self, lat):
        cfg, W, fmt, sc = self.cfg, self.W, self.fmt, self.scales
        live = self.start < self.frame
        pos0 = 16 * (self.frame - self.start)
        pos = pos0[:, None] + np.arange(16)[None, :]
        t = {"latent": np.asarray(lat), "pos0": pos0}
        x = bf16(fstage_P(cfg, W, fmt, lat, lat if self.lat_prev is None else self.lat_prev, live)["upsample"])
        t["upsample"] = t["tr_in0"] = x
        for l in range(self.L):
            qkv = fstage_Q(cfg, W, fmt, l, x, pos, mutate=self._m(f"Q{l}"))
            slots = pos % self.ring
            for b in range(self.B):
                self.K[l][b, slots[b]] = out_round(qkv["k"][b], "f32")
                self.V[l][b, slots[b]] = out_round(qkv["v"][b], "f32")
            t[f"tr_q{l}"] = out_round(qkv["q"], "f32")
            t[f"tr_k{l}"], t[f"tr_v{l}"] = self.K[l].copy(), self.V[l].copy()
            Kr = self.K[0] if self._m(f"A{l}") == "k_layer0" else self.K[l]
            t[f"tr_attn{l}"] = bf16(fstage_A(cfg, W, fmt, t[f"tr_q{l}"], Kr, self.V[l], pos0)["attn"])
            t[f"tr_resid{l}"] = bf16(fstage_B(cfg, W, fmt, l, t[f"tr_attn{l}"], x)["resid"])
            t[f"tr_ff{l}"] = bf16(fstage_C(cfg, W, fmt, l, t[f"tr_resid{l}"], mutate=self._m(f"C{l}"))["ff"])
            x = bf16(fstage_D(cfg, W, fmt, l, t[f"tr_ff{l}"], t[f"tr_resid{l}"])["out"], trunc=self._m(f"D{l}") == "trunc")
            t[f"tr_in{l + 1}" if l < self.L - 1 else "dec_tr"] = x
        keep = live[:, None, None].astype(np.float64)

        def tail(name, n):
            return np.zeros_like(t[name][:, :n]) if self.prev is None else self.prev[name][:, -n:] * keep

        kw = dict(scales=sc)
        t["seanet0"] = self._rnd(fstage_S0(cfg, W, fmt, t["dec_tr"], tail("dec_tr", 6), mutate=self._m("S0"), **kw)["a0"], ("conv0",), "S0")
        src = "seanet0"
        for i in (1, 2, 3):
            c = fstage_Cv(cfg, W, fmt, i, t[src], tail(src, 1), mutate=self._m(f"Cv{i}"), **kw)
            t[f"seanet{3 * i - 1}"] = bf16(c["raw"])
            t[f"seanet_c{i}"] = self._rnd(c["elu"], ("convtr", i), f"Cv{i}")
            h = fstage_Ra(cfg, W, fmt, i, t[f"seanet_c{i}"], tail(f"seanet_c{i}", 2), mutate=self._m(f"Ra{i}"), **kw)["h"]
            t[f"seanet_h{i}"] = self._rnd(h, ("res_a", i), f"Ra{i}")
            o = fstage_Rb(cfg, W, fmt, i, t[f"seanet_h{i}"], t[f"seanet{3 * i - 1}"], mutate=self._m(f"Rb{i}"), **kw)["out"]
            t[f"seanet{3 * i}"] = self._rnd(o, ("res_b", i), f"Rb{i}")
            src = f"seanet{3 * i}"
        t["pcm"] = out_round(fstage_L(cfg, W, fmt, t["seanet9"], tail("seanet9", 2))["pcm"], "f32")
        self.prev, self.lat_prev = t, np.asarray(lat)
        self.frame += 1
        return t


# the tap whose amax fixes each activation scale of the fp8 codec (calibrate_fp8_codec scans the bf16 codec's buffers)
SCALE_TAP = {0: "seanet0", 1: "seanet_c1", 2: "seanet_h1", 3: "seanet3", 4: "seanet_c2", 5: "seanet_h2", 6: "seanet6",
             7: "seanet_c3", 8: "seanet_h3"}


def scales_from_amax(amax):
    """2.0f * amax / 448.0f in fp32 per used index, 1 elsewhere (calibrate_fp8_codec)"""
    out = np.ones(16, np.float32)
    for k, a in amax.items():
        if a > 0:
            out[k] = f32_div(np.float32(2.0) * np.float32(a), 448.0)
    return out


def calibrate(cfg, W, latents):
    """the reference's own calibration: the bf16 chain on latents [F, B, ldim], amax of every SCALE_TAP over all frames,
    scale = 2 amax / 448"""
    ch = FChain(cfg, W, latents.shape[1], "bf16")
    amax = {k: 0.0 for k in SCALE_TAP}
    for lat in latents:
        t = ch.decode(lat)
        for k, name in SCALE_TAP.items():
            amax[k] = max(amax[k], float(np.abs(t[name]).max()))
    return scales_from_amax(amax)


# ---- the bound of tests/test_gpu_codec_formats.py, shared with the seeded defects of the CPU test ----------------------
def bf16_ulp(v):
    _, e = np.frexp(np.maximum(np.abs(v), 2.0 ** -126))
    return np.ldexp(1.0, e - 8)


def ratio_of(got, y64, tol, kind, yinv=None):
    """worst distance of `got` from the bounded interval [y64 - tol, y64 + tol] after the output rounding, in units of the
    bound (<= 1 passes); inf for an e4m3 code outside the neighbours of the interval's ends"""
    got = np.asarray(got).astype(np.float64)
    assert got.shape == y64.shape, (got.shape, y64.shape)
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - y64)
    if kind == "f32":
        return float((err / tol).max())
    if kind == "bf16":
        return float((np.maximum(err - 0.5 * bf16_ulp(got), 0) / tol).max())
    yinv = float(yinv)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    lo, _ = _CR.e4m3_neighbours(t((y64 - tol) * yinv))
    _, hi = _CR.e4m3_neighbours(t((y64 + tol) * yinv))
    lo, hi = lo.numpy(), hi.numpy()
    if not ((got >= lo) & (got <= hi)).all():
        return float("inf")
    sat_hi, sat_lo = (y64 - tol) * yinv >= _CR.E4M3_MAX, (y64 + tol) * yinv <= -_CR.E4M3_MAX
    if not ((got[sat_hi] == _CR.E4M3_MAX).all() and (got[sat_lo] == -_CR.E4M3_MAX).all()):
        return float("inf")
    d = np.abs(got / yinv - np.clip(y64, -_CR.E4M3_MAX / yinv, _CR.E4M3_MAX / yinv))
    w = tol + (hi - lo) / yinv
    return float(np.where(w > 0, d / np.maximum(w, 1e-300), 0.0).max())


def f8_bound_codes(cx, cw, s):
    """codec_ref.f8_mfma_bound on the raw e4m3 codes cx [M][K], cw [N][K] and the operands' scale s [N], in float32: a
    product of two codes has at most 8 significant bits and the group quantum is a power of two, so every term is exact
    in float32; only the sum over K terms rounds, which the factor 1 + K 2^-23 covers (an upper bound of that function's
    float64 result, within 1 + K 2^-22 of it: tests/test_codec_formats_reference_cpu.py).  Half the memory traffic and no
    logarithm: the GPU test visits every product of every fp8 GEMM."""
    G, KEEP = _CR.F8_GROUP, _CR.F8_KEEP
    X = torch.from_numpy(np.ascontiguousarray(np.abs(cx), dtype=np.float32))
    Wc = torch.from_numpy(np.ascontiguousarray(np.abs(cw), dtype=np.float32))
    M, K = X.shape
    N = Wc.shape[0]
    wg = Wc.reshape(1, N, K // G, G)
    out = torch.empty(M, N, dtype=torch.float32)
    step = max(1, (1 << 25) // (N * K))
    for r0 in range(0, M, step):
        p = X[r0:r0 + step].reshape(-1, 1, K // G, G) * wg
        mx = p.amax(dim=-1, keepdim=True)
        _, e = torch.frexp(mx)  # mx = m 2^e, 0.5 <= m < 1: floor(log2 mx) = e - 1
        q = torch.where(mx > 0, torch.ldexp(torch.ones_like(mx), e - 1 - KEEP), torch.zeros_like(mx))
        out[r0:r0 + step] = torch.minimum(p, q).sum(dim=(-1, -2))
    return out.to(torch.float64).numpy() * (1 + K * 2.0 ** -23) * np.asarray(s, np.float64)[None, :]


def f8_extra(cfg, W, site, cols, scales, y64, mutate=None):
    """what the e4m3 MFMA drops at this site (codec_ref.f8_mfma_bound's model on the codes of the launch's operands, see
    f8_bound_codes) plus the fp8 epilogue's two fp32 roundings, shaped as the site's output before any reshape"""
    w, _, ws = site_weights(cfg, W, site, "fp8")
    xs = float(np.float32(scales[SC_IN[site]]))
    b = f8_bound_codes(cols.reshape(-1, cols.shape[-1]), w, ws.astype(np.float64) * xs)
    return b.reshape(y64.shape) + 2 * 2.0 ** -24 * np.abs(y64)


# ---- the split-bf16 codec (codec_split, gemm_kernel<.., WF = 3>): the fp32 stages with a split matrix product ------------
# A split engine runs the fp32 codec's launches on fp32 buffers; only the matrix product of its GEMM launches differs
# (`_mms`: xh.wh + xl.wh + xh.wl, hi = bf16(v), lo = bf16(v - hi), include/ptts.h and the header of ptts_split.hip).  The
# stage functions above take `split=""` for that product (or a SPLIT_MUTANTS name); the prologue P, the attention proper,
# the fused residual block R (fp32 weights, mimi_seanet_enqueue) and the last conv L stay the fp32 stages.  Launches the
# fp32 stages lump together are judged apart here, on the taps between them:
#   Q    the last layer's input, positions          tr_q / tr_k / tr_v   the +ln GEMM with EPI_QKV alone ([3, B, T, H 64])
#   Ci   as above                                   seanet(3i-1), seanet_c<i>   raw and ELU'd copies ([2, B, T s, cout])
#   Rai  seanet_c<i>, its last 2 rows before         seanet_h<i>          the k3 conv of an unfused block
#   Rbi  seanet_h<i>, seanet(3i-1)                   seanet(3i)           the 1x1 conv + raw skip
# E32s (`split_e32`) is E32 of the same split formulas: the float32 evaluations differ from the float64 one by the
# summation and the epilogue only, since every bf16 x bf16 product is exact in float32.
def stage_Q(cfg, W, x, pos, dtype=F64, order="np", alt=False, mutate=None, split=None):
    """the last layer's in-projection of norm1(x) with RoPE at the positions pos [B, T]: queries, key rows and value rows
    as the launch writes them, stacked [3, B, T, H * 64]"""
    _check(mutate, ())
    tr, H, Dh = _tr_cfg(cfg)
    x = _in(x, dtype)
    B, T, _ = x.shape
    qkv = _ln_mm(cfg, W, ("qkv", tr.num_layers - 1), x, dtype, order, alt, split).reshape(B, T, 3, H, Dh)
    q = _rope(qkv[:, :, 0], pos, float(tr.max_period), dtype)
    k = _rope(qkv[:, :, 1], pos, float(tr.max_period), dtype)
    return np.stack([q.reshape(B, T, H * Dh), k.reshape(B, T, H * Dh), np.ascontiguousarray(qkv[:, :, 2]).reshape(B, T, H * Dh)])


def stage_Cv2(cfg, W, i, x, tail, dtype=F64, order="np", alt=False, mutate=None, split=None):
    """stage i's transposed conv as a launch without "single_store" writes it: the raw output (the block's skip) and its
    ELU'd copy (the k3 conv's operand), stacked [2, B, T * s, cout]"""
    raw = stage_Cv(cfg, W, i, x, tail, dtype, order, alt, mutate, split)
    return np.stack([raw, _elu(raw, alt)])


def _res_convs(cfg, W, i, dtype):
    P = params(cfg, W, dtype)
    p = f"mimi.decoder.model.{_layer_of(cfg, 'res', i)[0]}.block"
    return P.conv(p + ".1.conv"), P.conv(p + ".3.conv")


def stage_Ra(cfg, W, i, x, tail, dtype=F64, order="np", alt=False, mutate=None, split=None):
    """the k3 conv of stage i's unfused residual block on the ELU'd transposed-conv output (tail: its last 2 rows of the
    previous frame), ELU'd: the hidden activation"""
    _check(mutate, ("parity", "seqcut"))
    (w1, b1), _ = _res_convs(cfg, W, i, dtype)
    return _elu(_mm(_im2col(_halo(_in(x, dtype), tail, 2, mutate), 3), w1, b1, order, split), alt)


def stage_Rb(cfg, W, i, h, skip, dtype=F64, order="np", alt=False, mutate=None, split=None):
    """ELU(raw skip + 1x1 conv of the hidden activation): the unfused block's output (EPI_RES from craw)"""
    _check(mutate, ("skip_elu", "no_bias2"))
    _, (w2, b2) = _res_convs(cfg, W, i, dtype)
    skip = _in(skip, dtype)
    v = _mm(_in(h, dtype), w2, None if mutate == "no_bias2" else b2, order, split)
    return _elu((_elu(skip, alt) if mutate == "skip_elu" else skip) + v, alt)


SSTAGES = {"Q": stage_Q, "A": stage_A, "T": stage_T, "B": stage_B, "C": stage_C, "D": stage_D, "S0": stage_S0,
           **{f"C{i}": _conv_stage(stage_Cv2, i) for i in (1, 2, 3)},
           **{f"Ra{i}": _conv_stage(stage_Ra, i) for i in (1, 2, 3)}, **{f"Rb{i}": _conv_stage(stage_Rb, i) for i in (1, 2, 3)}}
SPLIT_TAPS = {"Q": ("tr_q", "tr_krows", "tr_vrows"), "A": ("tr_attn",), "T": ("dec_tr",), "B": ("tr_resid",), "C": ("tr_ff",),
              "D": ("dec_tr",), "S0": ("seanet0",), **{f"C{i}": (f"seanet{3 * i - 1}", f"seanet_c{i}") for i in (1, 2, 3)},
              **{f"Ra{i}": (f"seanet_h{i}",) for i in (1, 2, 3)}, **{f"Rb{i}": (f"seanet{3 * i}",) for i in (1, 2, 3)}}


def split_e32(stage, inputs, split=""):
    """-> (y64s, E32s) of `SSTAGES[stage](**inputs, split=split)`: the float64 evaluation of the split formulas and the
    worst float32 error of the same formulas on the same inputs over F32_VARIANTS.  From the reference alone."""
    fn = SSTAGES[stage]
    y64 = fn(**inputs, split=split)
    assert y64.dtype == np.float64
    e32 = 0.0
    for order, alt in F32_VARIANTS:
        y32 = fn(**inputs, dtype=F32, order=order, alt=alt, split=split)
        assert y32.dtype == np.float32 and y32.shape == y64.shape, (stage, y32.dtype)
        e32 = max(e32, float(np.abs(y32.astype(np.float64) - y64).max()))
    assert e32 > 0, stage
    return y64, e32


def split_inputs(stage, cfg, W, frames, f, start=None):
    """keyword arguments of `SSTAGES[stage]` at frame f; frames[g] as for `stage_inputs`, with the taps of SPLIT_TAPS and,
    for more than one layer, "tr_in<last>" (the last layer's input)"""
    cur = frames[f]
    L = cfg.mimi.transformer.num_layers
    B = np.asarray(cur["latent"]).shape[0]
    st = np.zeros(B, np.int64) if start is None else np.asarray(start, np.int64)
    live = st < f

    def x_last():
        return cur["upsample"] if L == 1 else cur[f"tr_in{L - 1}"]

    def tail(name, n):
        x = np.asarray(cur[name])
        return np.zeros_like(x[:, :n]) if f == 0 else np.asarray(frames[f - 1][name])[:, -n:] * live[:, None, None].astype(x.dtype)

    if stage == "Q":
        return dict(cfg=cfg, W=W, x=x_last(), pos=(16 * (f - st))[:, None] + np.arange(16)[None, :])
    if stage == "B":
        return dict(cfg=cfg, W=W, attn=cur["tr_attn"], x=x_last())
    if stage[:2] == "Ra":
        return dict(cfg=cfg, W=W, x=cur[f"seanet_c{stage[2]}"], tail=tail(f"seanet_c{stage[2]}", 2))
    if stage[:2] == "Rb":
        return dict(cfg=cfg, W=W, h=cur[f"seanet_h{stage[2]}"], skip=cur[f"seanet{3 * int(stage[2]) - 1}"])
    return stage_inputs(stage, cfg, W, frames, f, start)


def _mag(x, w):
    x = np.abs(np.asarray(x, np.float64))
    return x.reshape(-1, x.shape[-1]) @ np.abs(w).T


def split_scale(stage, inputs):
    """what the mode's promise is measured against, shaped as the stage's output: rs * sum_k |x_k| |w_k| over the GEMM's
    operands (x after any prologue, w the fp32 matrix; a +ln site adds rs |mu| sum_k |w_k|, the fold's second product),
    carried through the epilogue's multiplications (the layer scale; RoPE's cosine and sine, in magnitude) as
    gemm_ref.gemm_ref carries its `scale`, without the bias and the residual, which the split leaves exact.  The
    activations' slopes are taken as 1 (ELU's is at most 1; GELU's reaches 1.13, inside the slack between the three
    dropped terms' 3 x 2^-16 and the promise's 2^-14).  Stages A and T have none: their GEMMs' errors pass through a
    softmax and further layers."""
    cfg, W = inputs["cfg"], inputs["W"]
    P = params(cfg, W, F64)
    tr, H, Dh = _tr_cfg(cfg)
    l = tr.num_layers - 1
    if stage in ("Q", "C"):
        x = np.asarray(inputs["x" if stage == "Q" else "resid"], np.float64)
        wf = fold_image(cfg, W, ("qkv" if stage == "Q" else "ff1", l), F64)
        mu, rs = _stats(x, False)
        sc = (rs.reshape(-1, 1) * (_mag(x, wf) + np.abs(mu).reshape(-1, 1) * np.abs(wf).sum(axis=1)[None, :])).reshape(x.shape[:2] + (-1,))
        if stage == "C":
            return sc
        B, T = x.shape[:2]
        sc = sc.reshape(B, T, 3, H, Dh)
        ds = np.arange(Dh // 2, dtype=F32)
        freqs = np.exp((ds * F32(-math.log(float(tr.max_period)) * 2 / Dh)).astype(F64)).astype(F32)
        ang = (freqs[None, None, :] * inputs["pos"].astype(F32)[:, :, None]).astype(F32).astype(F64)
        c, s = np.abs(np.cos(ang))[:, :, None, :], np.abs(np.sin(ang))[:, :, None, :]
        out = []
        for j in (0, 1):
            r, im = sc[:, :, j, :, 0::2], sc[:, :, j, :, 1::2]
            o = np.empty_like(sc[:, :, j])
            o[..., 0::2] = r * c + im * s
            o[..., 1::2] = r * s + im * c
            out.append(o.reshape(B, T, H * Dh))
        return np.stack(out + [sc[:, :, 2].reshape(B, T, H * Dh)])
    if stage in ("B", "D"):
        x = inputs["attn" if stage == "B" else "ff"]
        w = P.vec(_lp(l) + (".self_attn.out_proj.weight" if stage == "B" else ".linear2.weight"))
        ls = np.abs(P.vec(_lp(l) + (".layer_scale_1.scale" if stage == "B" else ".layer_scale_2.scale")))
        return (_mag(x, w) * ls[None, :]).reshape(np.asarray(x).shape[:2] + (-1,))
    x, tl = np.asarray(inputs["h" if stage[:2] == "Rb" else "x"], np.float64), inputs.get("tail")
    B, T = x.shape[:2]
    if stage == "S0":
        idx, _, _, K, _ = _layer_of(cfg, "conv", 0)
        return _mag(_im2col(_halo(x, tl, K - 1, None), K), P.conv(f"mimi.decoder.model.{idx}.conv")[0]).reshape(B, T, -1)
    i = int(stage[-1])
    if stage[0] == "C":
        idx, _, cout, _, s = _layer_of(cfg, "convtr", i)
        xx = _halo(x, tl, 1, None)
        m = _mag(np.concatenate([xx[:, 1:], xx[:, :-1]], axis=-1), P.convtr(f"mimi.decoder.model.{idx}.convtr", s)[0]).reshape(B, T * s, cout)
        return np.stack([m, m])
    (w1, _), (w2, _) = _res_convs(cfg, W, i, F64)
    if stage[:2] == "Ra":
        return _mag(_im2col(_halo(x, tl, 2, None), 3), w1).reshape(B, T, -1)
    return _mag(x, w2).reshape(B, T, -1)


PROMISE = 2.0 ** -14  # include/ptts.h: about 2^-16 per product; wl xl, (w - wh - wl) x and w (x - xh - xl) are each <= 2^-16 |w| |x|
