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


def _mm(x, w, b, order):
    """x [..., K] @ w[N, K]^T + b in x's dtype; order "seq": rows `_seq_rows` by a plain sequential sum over k"""
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


def _transformer(cfg, W, ups, start, dtype, order, alt, mutate, n_layers=None):
    """the decoder transformer on the frames `ups` (upsample taps [B, 16, C] of frames 0 .. f), streaming: every frame
    attends to the keys of the frames before it.  start[b]: the frame sequence b's utterance began at (position 0; keys
    of earlier frames are not its own).  -> the last layer's taps of frame f.
    A pure function of its arguments; the K / V of a prefix of frames it has already seen (the same arrays at the same
    positions) are remembered, so that judging frame after frame costs one frame each."""
    P = params(cfg, W, dtype)
    tr = cfg.mimi.transformer
    H, Dh, ctx = tr.num_heads, tr.d_model // tr.num_heads, tr.context
    L = tr.num_layers if n_layers is None else n_layers
    B, T, C = np.asarray(ups[0]).shape
    start = np.zeros(B, np.int64) if start is None else np.asarray(start, np.int64)
    dt = np.dtype(dtype).type
    key = (id(W), np.dtype(dtype).str, order, alt, mutate, L)
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
            h = _layer_norm(x, P.vec(p + ".norm1.weight"), P.vec(p + ".norm1.bias"), alt)
            qkv = _mm(h, P.vec(p + ".self_attn.in_proj.weight"), None, order).reshape(B, T, 3, H, Dh)
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
            resid = x + P.vec(p + ".layer_scale_1.scale") * _mm(ao, P.vec(p + ".self_attn.out_proj.weight"), None, order)
            ff = _gelu(_mm(_layer_norm(resid, P.vec(p + ".norm2.weight"), P.vec(p + ".norm2.bias"), alt),
                           P.vec(p + ".linear1.weight"), None, order))
            x = resid + P.vec(p + ".layer_scale_2.scale") * _mm(ff, P.vec(p + ".linear2.weight"), None, order)
        fr["taps"] = dict(attn=ao, resid=resid, ff=ff, out=x)
        done = done + [fr]
        if len(_TR_MEMO) > 256:
            _TR_MEMO.clear()
        _TR_MEMO[key] = (list(ups[: f + 1]), done)  # the arrays stay alive with their ids
    taps = done[-1]["taps"]
    assert all(v.dtype == dt for v in taps.values())
    return taps


def stage_A(cfg, W, ups, start=None, dtype=F64, order="np", alt=False, mutate=None):
    """one-layer configurations: LayerNorm + in_proj + RoPE + the K / V history + attention -> attention output"""
    _check(mutate, ("rope_ring", "window"))
    assert cfg.mimi.transformer.num_layers == 1, "stage A is defined on the one-layer configurations"
    return _transformer(cfg, W, ups, start, dtype, order, alt, mutate)["attn"]


def stage_T(cfg, W, ups, start=None, dtype=F64, order="np", alt=False, mutate=None):
    """the whole decoder transformer: upsample history -> dec_tr"""
    _check(mutate, ("rope_ring", "window"))
    return _transformer(cfg, W, ups, start, dtype, order, alt, mutate)["out"]


def _last(cfg):
    return f"mimi.decoder_transformer.transformer.layers.{cfg.mimi.transformer.num_layers - 1}"


def stage_B(cfg, W, attn, x, dtype=F64, order="np", alt=False, mutate=None):
    """x + layer_scale_1 * out_proj(attention output) (one-layer configurations: x = upsample)"""
    _check(mutate, ("no_ls",))
    P, p = params(cfg, W, dtype), _last(cfg)
    return _in(x, dtype) + (1 if mutate == "no_ls" else P.vec(p + ".layer_scale_1.scale")) * _mm(_in(attn, dtype), P.vec(p + ".self_attn.out_proj.weight"), None, order)


def stage_C(cfg, W, resid, dtype=F64, order="np", alt=False, mutate=None):
    """GELU(linear1(norm2(x))) of the last layer"""
    _check(mutate, ("tanh_gelu",))
    P, p = params(cfg, W, dtype), _last(cfg)
    h = _layer_norm(_in(resid, dtype), P.vec(p + ".norm2.weight"), P.vec(p + ".norm2.bias"), alt)
    return _gelu(_mm(h, P.vec(p + ".linear1.weight"), None, order), mutate == "tanh_gelu")


def stage_D(cfg, W, ff, resid, dtype=F64, order="np", alt=False, mutate=None):
    """x + layer_scale_2 * linear2(ff) of the last layer: the transformer's output"""
    _check(mutate, ("no_ls",))
    P, p = params(cfg, W, dtype), _last(cfg)
    return _in(resid, dtype) + (1 if mutate == "no_ls" else P.vec(p + ".layer_scale_2.scale")) * _mm(_in(ff, dtype), P.vec(p + ".linear2.weight"), None, order)


def _layer_of(cfg, kind, i):
    """(ModuleList index, cin, cout, kernel, stride) of SEANet stage i's layer of `kind` (i = 0: first / last conv)"""
    found = [l for l in seanet_decoder_layers(cfg) if l[1] == kind]
    idx, _, cin, cout, k, stride = found[i - 1] if kind != "conv" else found[i]
    return idx, cin, cout, k, stride


def stage_S0(cfg, W, x, tail, dtype=F64, order="np", alt=False, mutate=None):
    """ELU(k7 streaming conv of the transformer's output); tail: the last 6 rows of the previous frame's dec_tr"""
    _check(mutate, ("parity", "seqcut"))
    P = params(cfg, W, dtype)
    idx, _, _, K, _ = _layer_of(cfg, "conv", 0)
    w, b = P.conv(f"mimi.decoder.model.{idx}.conv")
    return _elu(_mm(_im2col(_halo(_in(x, dtype), tail, K - 1, mutate), K), w, b, order), alt)


def stage_Cv(cfg, W, i, x, tail, dtype=F64, order="np", alt=False, mutate=None):
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
    y = _mm(np.concatenate([xx[:, 1:], xx[:, :-1]], axis=-1), w, np.tile(b, s), order)
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

    def __init__(self, cfg, W, B, dtype=F64, order="np", alt=False, fused_tail=False):
        self.cfg, self.W, self.B = cfg, W, B
        self.kw = dict(dtype=dtype, order=order, alt=alt)
        self.fused_tail = fused_tail  # PCM through stage R3L instead of R3 and L
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
        tr = _transformer(cfg, W, self.ups, self.start, mutate=None, **kw)  # stage T, with the last layer's taps
        t.update(tr_attn=tr["attn"], tr_resid=tr["resid"], tr_ff=tr["ff"], dec_tr=tr["out"])
        keep = live[:, None, None].astype(t["dec_tr"].dtype)

        def tail(name, n):
            cur = t[name]
            return np.zeros_like(cur[:, :n]) if self.prev is None else self.prev[name][:, -n:] * keep

        for stage, src, n in CONV_CHAIN[:-2] if self.fused_tail else CONV_CHAIN:
            t[OUTPUT_TAP[stage]] = STAGES[stage](cfg, W, t[src], tail(src, n), **kw)
        if self.fused_tail:
            t["pcm"] = stage_R3L(cfg, W, t["seanet8"], tail("seanet8", 4), live, **kw)
        self.prev, self.lat_prev = t, np.asarray(lat)
        self.frame += 1
        return t


def chain_e32(cfg, W, latents, fused_tail=False, resets=()):
    """latents [F, B, ldim] -> per frame (pcm64, E32): the fp64 chain's PCM and the worst float32 error of the same chain
    over F32_VARIANTS.  resets: (frame, row) pairs of `reset_row` calls issued before that frame"""
    B = latents.shape[1]
    chains = [Chain(cfg, W, B, fused_tail=fused_tail)] + [Chain(cfg, W, B, F32, o, a, fused_tail) for o, a in F32_VARIANTS]
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
