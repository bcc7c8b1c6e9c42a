"""The decoder a `codec_split` engine runs (PTTS_CODEC_SPLIT: the fp32 codec's launches with gemm_kernel<.., WF = 3> at the GEMM
sites, csrc/ptts_split.hip) against the fp64 stage references of tests/mimi_ref.py, LAUNCH BY LAUNCH, through the public
`Engine.mimi_decode` (one case through `mimi_decode_tr(lat, lat_b)` + `mimi_decode_seanet`: frame pairs).  `-m gpu`.

Per case: a fresh state decodes 6 frames of seeded latents with the engine option `debug_taps` 1: the zero-carry first
frame, the window dropping keys (context 40, from frame 2) and the ring wrapping.  After each frame every tap is read back
(`Engine.debug_read`) and every stage is judged ON THE INPUT THE KERNELS CONSUMED, for every element of every frame:

    split GEMM stages   |gpu - y64s| <= FACTOR * E32s                      the model bound       FACTOR = 8
                        |gpu - y64|  <= FACTOR * E32s + 2^-14 * scale      the promise bound
    fp32 stages         |gpu - y64|  <= FACTOR * E32                       as tests/test_gpu_mimi_matrix.py

y64s is the float64 evaluation of the split model xh.wh + xl.wh + xh.wl (hi = bf16(v), lo = bf16(v - hi), include/ptts.h and
the header of ptts_split.hip; a +ln site: statistics of the unrounded row, ln_s and ln_c of the fp32 image), E32s the loss of
a float32 evaluation of the same formulas on the same inputs (`mimi_ref.split_e32`), y64 the fp32 model, scale
rs sum_k |x_k| |w_k| through the epilogue (`mimi_ref.split_scale`).  FACTOR as in tests/test_gpu_mimi_matrix.py and for its
reason (the kernels split K over waves and sum in MFMA chains, another order than numpy's).  None of these figures is fitted
to what the kernels return; tests/test_codec_split_reference_cpu.py shows the promise holding in the reference alone and
every seeded defect of `mimi_ref.SPLIT_MUTANTS` but the fp32 fall-back moving its stage by >= 32 E32s.

The split GEMM stages are Q (the last layer's +ln GEMM with EPI_QKV alone: queries, key rows, value rows), B, C, D, S0,
C1..C3 (raw and ELU'd copies) and the unfused pair Ra / Rb; A (one layer) and T (two layers) run the whole transformer in the
split model and carry the model bound only (no scale passes a softmax).  P, the attention proper (At, `mimi_ref.fstage_A`
on the queries and rings read back), the fused resblock<..> (fp32 weights) and the last conv L are fp32 stages.

WHAT MUST HAVE RUN is asserted from the profiler's (site, kernel) records, which is what catches a silent fall-back to fp32
weights (the bounds on values cannot: the two models differ by less than 32 E32s): `+ln+split` at mimi.qkv / ff1, `+split`
at mimi.out / ff2, seanet.conv0 and convtr1..3, no `+elu` anywhere (no single store), resblock<hid/16,cout/16> without
`+split` at the fusable stages (2 and 3 on nf64) and gemm..+split at res1a / res1b, all six residual sites `+split` with
`fuse_res` 0, seanet.conv_last = pcm_conv (never pcm_fix), no gemm_lds kernel with `+split`.

MEASURED on an MI355X, all 35 tests of this module passing: worst ratio to the model bound 8 E32s (fp32 stages P, At, R2,
R3, L and the chain: to 8 E32) and, second column, to the promise bound 8 E32s + 2^-14 scale (0.000: the stage has none), per
(configuration, stage, kernel) over every case of the module ("pair": the frame-pair case; "chain": the PCM without taps).
Every kernel sits at <= 0.37 of the model bound and <= 0.13 of the promise bound; nothing was found wrong in the dispatcher,
the codec host code or the kernels, and no site fell back to fp32 weights or an LDS-staged tile.  Tile configurations that
ran with `+split` at some site of the sweep: 1, 2, 3, 4, 5, 6, 7, 10, 11, 13, 14 (all that split_cfg admits); for the others
(0, 8, 9, 12, 15, 16, 17) every site showed choose_cfg's register-staged `+split` fall-back.  Slowest case: 3.7 s
(test_every_tile_configuration[4-B9]); the module takes 77 s, nearly all of it the numpy reference.  The hi and lo images
of all 17 matrices of nf64x2 were bit-equal to bf16(w) and bf16(w - bf16(w)), ln_s and ln_c of qkv and ff1 within the bound.

  nf64   A        0.159  0.000  gemm<1,1,1,1,4>+ln+split attn
  nf64   A        0.151  0.000  gemm<1,1,4,1,1>+ln+split attn
  nf64   A        0.244  0.000  gemm<1,2,1,2,2>+ln+split attn
  nf64   A        0.129  0.000  gemm<1,2,4,1,1>+ln+split attn
  nf64   A        0.233  0.000  gemm<1,4,1,1,4>+ln+split attn
  nf64   A        0.126  0.000  gemm<1,4,4,1,1>+ln+split attn
  nf64   A        0.134  0.000  gemm<2,2,4,1,1>+ln+split attn
  nf64   A        0.236  0.000  gemm<2,4,1,1,4>+ln+split attn
  nf64   A        0.204  0.000  gemm<2,4,1,2,2>+ln+split attn
  nf64   A        0.101  0.000  gemm<2,4,2,2,1>+ln+split attn
  nf64   A        0.119  0.000  gemm<2,4,4,1,1>+ln+split attn
  nf64   At       0.197  0.000  attn
  nf64   B        0.180  0.030  gemm<1,1,1,1,4>+split
  nf64   B        0.125  0.029  gemm<1,1,4,1,1>+split
  nf64   B        0.192  0.031  gemm<1,2,1,2,2>+split
  nf64   B        0.125  0.029  gemm<1,2,4,1,1>+split
  nf64   B        0.175  0.029  gemm<1,4,1,1,4>+split
  nf64   B        0.137  0.033  gemm<1,4,4,1,1>+split
  nf64   B        0.146  0.029  gemm<2,2,4,1,1>+split
  nf64   B        0.183  0.031  gemm<2,4,1,1,4>+split
  nf64   B        0.286  0.031  gemm<2,4,1,2,2>+split
  nf64   B        0.141  0.029  gemm<2,4,2,2,1>+split
  nf64   B        0.131  0.033  gemm<2,4,4,1,1>+split
  nf64   C        0.202  0.034  gemm<1,1,1,1,4>+ln+split
  nf64   C        0.114  0.030  gemm<1,1,4,1,1>+ln+split
  nf64   C        0.191  0.036  gemm<1,2,1,2,2>+ln+split
  nf64   C        0.095  0.029  gemm<1,2,4,1,1>+ln+split
  nf64   C        0.149  0.031  gemm<1,4,1,1,4>+ln+split
  nf64   C        0.083  0.033  gemm<1,4,4,1,1>+ln+split
  nf64   C        0.091  0.029  gemm<2,2,4,1,1>+ln+split
  nf64   C        0.163  0.032  gemm<2,4,1,1,4>+ln+split
  nf64   C        0.219  0.034  gemm<2,4,1,2,2>+ln+split
  nf64   C        0.126  0.031  gemm<2,4,2,2,1>+ln+split
  nf64   C        0.081  0.031  gemm<2,4,4,1,1>+ln+split
  nf64   C1       0.199  0.018  gemm<1,1,1,1,4>+split
  nf64   C1       0.068  0.016  gemm<1,1,4,1,1>+split
  nf64   C1       0.214  0.020  gemm<1,2,1,2,2>+split
  nf64   C1       0.084  0.019  gemm<1,2,4,1,1>+split
  nf64   C1       0.188  0.017  gemm<1,4,1,1,4>+split
  nf64   C1       0.068  0.018  gemm<1,4,4,1,1>+split
  nf64   C1       0.061  0.017  gemm<2,2,4,1,1>+split
  nf64   C1       0.265  0.019  gemm<2,4,1,1,4>+split
  nf64   C1       0.189  0.016  gemm<2,4,1,2,2>+split
  nf64   C1       0.116  0.016  gemm<2,4,2,2,1>+split
  nf64   C1       0.077  0.016  gemm<2,4,4,1,1>+split
  nf64   C2       0.286  0.026  gemm<1,1,1,1,4>+split
  nf64   C2       0.075  0.025  gemm<1,1,4,1,1>+split
  nf64   C2       0.274  0.025  gemm<1,2,1,2,2>+split
  nf64   C2       0.100  0.026  gemm<1,2,4,1,1>+split
  nf64   C2       0.260  0.029  gemm<1,4,1,1,4>+split
  nf64   C2       0.085  0.024  gemm<1,4,4,1,1>+split
  nf64   C2       0.095  0.026  gemm<2,2,4,1,1>+split
  nf64   C2       0.308  0.027  gemm<2,4,1,1,4>+split
  nf64   C2       0.271  0.024  gemm<2,4,1,2,2>+split
  nf64   C2       0.190  0.026  gemm<2,4,2,2,1>+split
  nf64   C2       0.116  0.027  gemm<2,4,4,1,1>+split
  nf64   C3       0.218  0.036  gemm<1,1,1,1,4>+split
  nf64   C3       0.069  0.033  gemm<1,1,4,1,1>+split
  nf64   C3       0.184  0.033  gemm<1,2,1,2,2>+split
  nf64   C3       0.068  0.034  gemm<1,2,4,1,1>+split
  nf64   C3       0.242  0.037  gemm<1,4,1,1,4>+split
  nf64   C3       0.062  0.033  gemm<1,4,4,1,1>+split
  nf64   C3       0.068  0.032  gemm<2,2,4,1,1>+split
  nf64   C3       0.270  0.034  gemm<2,4,1,1,4>+split
  nf64   C3       0.221  0.034  gemm<2,4,1,2,2>+split
  nf64   C3       0.108  0.034  gemm<2,4,2,2,1>+split
  nf64   C3       0.069  0.034  gemm<2,4,4,1,1>+split
  nf64   D        0.186  0.029  gemm<1,1,1,1,4>+split
  nf64   D        0.081  0.028  gemm<1,1,4,1,1>+split
  nf64   D        0.241  0.031  gemm<1,2,1,2,2>+split
  nf64   D        0.070  0.028  gemm<1,2,4,1,1>+split
  nf64   D        0.208  0.029  gemm<1,4,1,1,4>+split
  nf64   D        0.077  0.028  gemm<1,4,4,1,1>+split
  nf64   D        0.094  0.031  gemm<2,2,4,1,1>+split
  nf64   D        0.228  0.029  gemm<2,4,1,1,4>+split
  nf64   D        0.262  0.032  gemm<2,4,1,2,2>+split
  nf64   D        0.107  0.027  gemm<2,4,2,2,1>+split
  nf64   D        0.076  0.028  gemm<2,4,4,1,1>+split
  nf64   L        0.051  0.000  pcm_conv
  nf64   P        0.119  0.000  mimi_prologue
  nf64   Q        0.169  0.030  gemm<1,1,1,1,4>+ln+split
  nf64   Q        0.098  0.030  gemm<1,1,4,1,1>+ln+split
  nf64   Q        0.188  0.030  gemm<1,2,1,2,2>+ln+split
  nf64   Q        0.085  0.031  gemm<1,2,4,1,1>+ln+split
  nf64   Q        0.179  0.033  gemm<1,4,1,1,4>+ln+split
  nf64   Q        0.081  0.029  gemm<1,4,4,1,1>+ln+split
  nf64   Q        0.080  0.032  gemm<2,2,4,1,1>+ln+split
  nf64   Q        0.210  0.033  gemm<2,4,1,1,4>+ln+split
  nf64   Q        0.210  0.034  gemm<2,4,1,2,2>+ln+split
  nf64   Q        0.102  0.035  gemm<2,4,2,2,1>+ln+split
  nf64   Q        0.076  0.031  gemm<2,4,4,1,1>+ln+split
  nf64   R2       0.161  0.000  resblock<4,8>
  nf64   R3       0.166  0.000  resblock<2,4>
  nf64   Ra1      0.240  0.019  gemm<1,1,1,1,4>+split
  nf64   Ra1      0.069  0.022  gemm<1,1,4,1,1>+split
  nf64   Ra1      0.228  0.018  gemm<1,2,1,2,2>+split
  nf64   Ra1      0.070  0.016  gemm<1,2,4,1,1>+split
  nf64   Ra1      0.242  0.018  gemm<1,4,1,1,4>+split
  nf64   Ra1      0.078  0.018  gemm<1,4,4,1,1>+split
  nf64   Ra1      0.071  0.015  gemm<2,2,4,1,1>+split
  nf64   Ra1      0.244  0.020  gemm<2,4,1,1,4>+split
  nf64   Ra1      0.364  0.021  gemm<2,4,1,2,2>+split
  nf64   Ra1      0.156  0.020  gemm<2,4,2,2,1>+split
  nf64   Ra1      0.088  0.019  gemm<2,4,4,1,1>+split
  nf64   Ra2      0.194  0.031  gemm<1,1,1,1,4>+split
  nf64   Ra3      0.210  0.034  gemm<1,1,1,1,4>+split
  nf64   Rb1      0.213  0.056  gemm<1,1,1,1,4>+split
  nf64   Rb1      0.110  0.046  gemm<1,1,4,1,1>+split
  nf64   Rb1      0.174  0.048  gemm<1,2,1,2,2>+split
  nf64   Rb1      0.085  0.048  gemm<1,2,4,1,1>+split
  nf64   Rb1      0.253  0.048  gemm<1,4,1,1,4>+split
  nf64   Rb1      0.089  0.055  gemm<1,4,4,1,1>+split
  nf64   Rb1      0.094  0.049  gemm<2,2,4,1,1>+split
  nf64   Rb1      0.182  0.046  gemm<2,4,1,1,4>+split
  nf64   Rb1      0.231  0.053  gemm<2,4,1,2,2>+split
  nf64   Rb1      0.098  0.047  gemm<2,4,2,2,1>+split
  nf64   Rb1      0.096  0.047  gemm<2,4,4,1,1>+split
  nf64   Rb2      0.153  0.065  gemm<1,1,1,1,4>+split
  nf64   Rb3      0.099  0.121  gemm<2,4,1,2,2>+split
  nf64   S0       0.214  0.026  gemm<1,1,1,1,4>+split
  nf64   S0       0.066  0.025  gemm<1,1,4,1,1>+split
  nf64   S0       0.206  0.026  gemm<1,2,1,2,2>+split
  nf64   S0       0.075  0.022  gemm<1,2,4,1,1>+split
  nf64   S0       0.188  0.025  gemm<1,4,1,1,4>+split
  nf64   S0       0.066  0.025  gemm<1,4,4,1,1>+split
  nf64   S0       0.065  0.027  gemm<2,2,4,1,1>+split
  nf64   S0       0.223  0.030  gemm<2,4,1,1,4>+split
  nf64   S0       0.219  0.027  gemm<2,4,1,2,2>+split
  nf64   S0       0.105  0.022  gemm<2,4,2,2,1>+split
  nf64   S0       0.062  0.024  gemm<2,4,4,1,1>+split
  nf64   chain    0.149  0.000  pcm_conv
  nf64x2 At       0.122  0.000  attn
  nf64x2 B        0.125  0.026  gemm<1,1,4,1,1>+split
  nf64x2 B        0.183  0.027  gemm<1,2,1,2,2>+split
  nf64x2 B        0.259  0.029  gemm<2,4,1,2,2>+split
  nf64x2 C        0.102  0.033  gemm<1,1,4,1,1>+ln+split
  nf64x2 C        0.183  0.027  gemm<1,2,1,2,2>+ln+split
  nf64x2 C        0.163  0.030  gemm<2,4,1,2,2>+ln+split
  nf64x2 C1       0.063  0.014  gemm<1,1,4,1,1>+split
  nf64x2 C1       0.181  0.016  gemm<1,2,1,2,2>+split
  nf64x2 C1       0.073  0.016  gemm<1,2,4,1,1>+split
  nf64x2 C2       0.120  0.025  gemm<1,2,4,1,1>+split
  nf64x2 C2       0.232  0.024  gemm<2,4,1,2,2>+split
  nf64x2 C2       0.094  0.024  gemm<2,4,4,1,1>+split
  nf64x2 C3       0.207  0.036  gemm<1,1,1,1,4>+split
  nf64x2 C3       0.201  0.031  gemm<2,4,1,2,2>+split
  nf64x2 D        0.077  0.028  gemm<1,1,4,1,1>+split
  nf64x2 D        0.172  0.027  gemm<1,2,1,2,2>+split
  nf64x2 D        0.166  0.029  gemm<2,4,1,2,2>+split
  nf64x2 L        0.041  0.000  pcm_conv
  nf64x2 P        0.094  0.000  mimi_prologue
  nf64x2 P pair   0.086  0.000  mimi_prologue
  nf64x2 Q        0.086  0.029  gemm<1,1,4,1,1>+ln+split
  nf64x2 Q        0.199  0.029  gemm<1,2,1,2,2>+ln+split
  nf64x2 Q        0.156  0.031  gemm<2,4,1,2,2>+ln+split
  nf64x2 R2       0.133  0.000  resblock<4,8>
  nf64x2 R3       0.149  0.000  resblock<2,4>
  nf64x2 Ra1      0.263  0.021  gemm<2,4,1,2,2>+split
  nf64x2 Rb1      0.206  0.046  gemm<2,4,1,2,2>+split
  nf64x2 S0       0.066  0.019  gemm<1,1,4,1,1>+split
  nf64x2 S0       0.208  0.028  gemm<1,2,1,2,2>+split
  nf64x2 S0       0.207  0.022  gemm<2,4,1,2,2>+split
  nf64x2 T        0.154  0.000  gemm<1,1,4,1,1>+ln+split attn
  nf64x2 T        0.155  0.000  gemm<1,2,1,2,2>+ln+split attn
  nf64x2 T        0.164  0.000  gemm<2,4,1,2,2>+ln+split attn
  nf64x2 T pair   0.201  0.000  gemm<2,4,1,2,2>+ln+split attn

Seeded defects, each seeded once in a local build that is not committed, each run once on the MI355X and caught:
  * the `wl * xb` MFMA dropped in the SPL branch of gemm_kernel (the weight's lo image never multiplied):
    test_batches[nf64-1] fails at every split stage and only there: the model bound at Q 968 x, A 981 x, B 1449 x, C 903 x,
    D 775 x, S0 390 x, C1 470 x, Ra1 514 x, Rb1 1482 x, C2 796 x, C3 873 x; the promise bound at 5.3 .. 15.7 x; the fp32
    stages P, At, R2, R3, L stay at <= 0.18;
  * the `wh * xr` MFMA dropped (the activation's residual never multiplied): test_batches[nf64-1] fails at the same
    eleven stages, the model bound at 320 x (S0) .. 1266 x (Rb1), the promise bound at 5.8 .. 15.7 x;
  * `mk_gemm` handing out the split images at every site but res_b (a silent fp32 fall-back): test_batches[nf64-3] fails in
    check_kernels at seanet.res1b, which showed `gemm<1,1,8,1,1>@147456` without `+split`.  Only the profiler's record can
    catch this one: the fp32 result is inside both bounds (tests/test_codec_split_reference_cpu.py, `fp32_w`);
  * the lo image packed from a - trunc_bf16(a) instead of a - bf16(a): test_weight_images_bit_for_bit fails at `wl_qkv0`, the
    first image it reads (half of the elements differ)."""

import time
import zlib

import numpy as np
import pytest
import torch

import mimi_ref as R
from gemm_ref import CFG_NAME, CFG_SHAPE
from pocket_tts_amd._lib import PttsError
from test_gpu_mimi_matrix import at, cdiv, fusable, pre_of, seanet_dims

pytestmark = pytest.mark.gpu

FACTOR = 8
FRAMES = 6
NCFG = len(CFG_NAME)
SPLIT_CFGS = (1, 2, 3, 4, 5, 6, 7, 10, 11, 13, 14)  # split_cfg (csrc/ptts_split.hip)
DEFAULTS = dict(fuse_res=1, single_store=1, fuse_pcm=1, debug_taps=0)  # opt_* in csrc/ptts_host.h
STATS = {}  # (config, stage, kernel label) -> [worst ratio to the model / fp32 bound, worst ratio to the promise bound]
TIMES = {}
SWEPT = {}  # config -> tile configurations that ran at some site of the sweep
SWEEP_CASES = {}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def seed_of(*case):
    return zlib.crc32(repr(case).encode())


@pytest.fixture(scope="module")
def engines():
    """one split engine per configuration for the whole module"""
    from pocket_tts_amd.engine import Engine

    cache = {}

    def get(name):
        if name not in cache:
            cfg, W = R.codec_weights(name)
            cache[name] = (Engine(cfg, W, "cuda:0", quantize_groups={"codec_split"}), cfg, W)
        return cache[name]

    yield get
    for eng, _, _ in cache.values():
        eng.close()


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.time()
    yield
    TIMES[request.node.name] = time.time() - t0


# ---- what must have run ----------------------------------------------------------------------------------------------
def split_gemm(k, pre):
    """a register-staged gemm<..> with exactly the suffixes `pre`"""
    return k.startswith("gemm<") and pre_of(k) == pre


def check_common(prof):
    for s, k in prof:
        p = pre_of(k)
        assert "elu" not in p and not {"q8", "b16"} & set(p), (s, k)
        assert not (k.startswith("gemm_lds") and "split" in p), (s, k)
        assert not (k.startswith("gemm") and "split" not in p), (s, k)  # no GEMM of a split engine's codec runs on fp32 weights


def check_tr(prof, cfg):
    check_common(prof)
    L = cfg.mimi.transformer.num_layers
    assert at(prof, "mimi.prologue") == ["mimi_prologue"], prof
    for site, pre in (("mimi.qkv", ["ln", "split"]), ("mimi.out", ["split"]), ("mimi.ff1", ["ln", "split"]), ("mimi.ff2", ["split"])):
        got = at(prof, site)
        assert len(got) == L and all(split_gemm(k, pre) for k in got), (site, got)
    assert len(at(prof, "mimi.attn")) >= L, prof


def check_seanet(prof, cfg, B, opts):
    """-> the stages whose residual block ran as the unfused split pair"""
    check_common(prof)
    c0 = at(prof, "seanet.conv0")
    assert len(c0) == 1 and split_gemm(c0[0], ["split"]), c0
    unfused = []
    for i in (1, 2, 3):
        _, cout, hid, _, _, rows = seanet_dims(cfg)[i - 1]
        ct, ra, rb = (at(prof, f"seanet.{s}{i}{x}") for s, x in (("convtr", ""), ("res", "a"), ("res", "b")))
        assert len(ct) == 1 and split_gemm(ct[0], ["split"]), (i, ct)
        if opts["fuse_res"] and fusable(cfg, i, B):
            want = f"resblock<{hid // 16},{cout // 16}>@{cdiv(B * rows // 16, 4) * 256}"
            assert ra == [want] and rb == [], (i, want, ra, rb)
        else:
            assert len(ra) == 1 and split_gemm(ra[0], ["split"]), (i, ra)
            assert len(rb) == 1 and split_gemm(rb[0], ["split"]), (i, rb)
            unfused.append(i)
    assert at(prof, "seanet.conv_last") == ["pcm_conv"], prof
    return unfused


def check_kernels(prof, cfg, B, opts):
    check_tr([r for r in prof if r[0].startswith("mimi.")], cfg)
    return check_seanet([r for r in prof if not r[0].startswith("mimi.")], cfg, B, opts)


STAGE_SITES = {"P": ("mimi.prologue",), "Q": ("mimi.qkv",), "At": ("mimi.attn",), "A": ("mimi.qkv", "mimi.attn"),
               "T": ("mimi.qkv", "mimi.attn"), "B": ("mimi.out",), "C": ("mimi.ff1",), "D": ("mimi.ff2",), "S0": ("seanet.conv0",),
               "L": ("seanet.conv_last",), **{f"C{i}": (f"seanet.convtr{i}",) for i in (1, 2, 3)},
               **{f"R{i}": (f"seanet.res{i}a",) for i in (1, 2, 3)}, **{f"Ra{i}": (f"seanet.res{i}a",) for i in (1, 2, 3)},
               **{f"Rb{i}": (f"seanet.res{i}b",) for i in (1, 2, 3)}}


def label_of_stage(prof, stage):
    return " ".join(at(prof, s)[-1].split("@")[0] for s in STAGE_SITES[stage] if at(prof, s))


# ---- running ---------------------------------------------------------------------------------------------------------
def tap_names(cfg, unfused, taps):
    L = cfg.mimi.transformer.num_layers
    if not taps:
        return ["upsample"]
    return ["upsample", "tr_q", f"tr_k{L - 1}", f"tr_v{L - 1}", "tr_attn", "tr_resid", "tr_ff", "dec_tr", "seanet0"] + \
        ([f"tr_in{L - 1}"] if L > 1 else []) + [f"seanet{k}" for k in (2, 3, 5, 6, 8, 9)] + [f"seanet_c{i}" for i in (1, 2, 3)] + \
        [f"seanet_h{i}" for i in unfused]


def read_taps(eng, ms, B, names):
    t = {}
    for name in names:
        x = eng.debug_read(ms, name).cpu().numpy()
        t[name] = x.reshape(B, x.shape[0] // B, x.shape[1])
    return t


def decode_frames(eng, cfg, B, latents, opts, resets=()):
    """-> one dict per frame: latent, PCM, every readable tap as [B, T, C], the profiler's (site, kernel) records.  A HIP
    error ends the session: the device may be in any state, nothing more is started"""
    unfused = [i for i in (1, 2, 3) if not (opts["fuse_res"] and fusable(cfg, i, B))]
    names = tap_names(cfg, unfused, opts["debug_taps"])
    for k, v in opts.items():
        eng.set_option(k, v)
    ms = eng.new_mimi_state(B)
    frames = []
    try:
        for f, lat in enumerate(latents):
            for fr, row in resets:
                if fr == f:
                    ms.reset_row(row)
            eng.profile_start()
            pcm = eng.mimi_decode(ms, dev(lat))
            prof = eng.profile_stop()
            torch.cuda.synchronize()
            t = dict(latent=lat, pcm=pcm.cpu().numpy(), prof=[(r["site"], r["kernel"]) for r in prof for _ in range(r["count"])])
            t.update(read_taps(eng, ms, B, names))
            frames.append(t)
    except (PttsError, RuntimeError) as e:
        pytest.exit(f"GPU error in the split codec matrix, session ended: {e}", returncode=3)
    ms.close()
    for k, v in DEFAULTS.items():
        eng.set_option(k, v)
    return frames


# ---- judging ---------------------------------------------------------------------------------------------------------
def starts_of(B, f, resets):
    start = np.zeros(B, np.int64)
    for fr, row in resets:
        if fr <= f:
            start[row] = fr
    return start


def note(worst, key, model, promise, f):
    w = worst.setdefault(key, [0.0, 0.0])
    w[0], w[1] = max(w[0], model), max(w[1], promise)
    print(f"  frame {f} {key[1]:4s} model / fp32 bound {model:6.3f}  promise bound {promise:6.3f}  {key[2]}")


def judge_split(name, cfg, W, frames, f, stage, start, worst, got=None):
    """one split stage of frame f against both bounds (A and T: the model bound alone)"""
    inputs = R.split_inputs(stage, cfg, W, frames, f, start)
    y64s, e32s = R.split_e32(stage, inputs)
    if got is None:
        taps = [frames[f][t] for t in R.SPLIT_TAPS[stage]]
        got = taps[0] if len(taps) == 1 else np.stack(taps)
    assert got.shape == y64s.shape and np.isfinite(got).all(), (stage, f, got.shape, y64s.shape)
    got = got.astype(np.float64)
    model = float(np.abs(got - y64s).max() / (FACTOR * e32s))
    promise = 0.0
    if stage not in ("A", "T"):
        y64, scale = R.SSTAGES[stage](**inputs), R.split_scale(stage, inputs)
        promise = float((np.abs(got - y64) / (FACTOR * e32s + R.PROMISE * scale)).max())
    note(worst, (name, stage, label_of_stage(frames[f]["prof"], stage)), model, promise, f)


def judge_f32(name, cfg, W, frames, f, stage, start, worst):
    got = frames[f][R.OUTPUT_TAP[stage]]
    y64, e32 = R.stage_e32(stage, R.stage_inputs(stage, cfg, W, frames, f, start))
    assert got.shape == y64.shape and np.isfinite(got).all(), (stage, f, got.shape, y64.shape)
    note(worst, (name, stage, label_of_stage(frames[f]["prof"], stage)), float(np.abs(got.astype(np.float64) - y64).max() / (FACTOR * e32)), 0.0, f)


def judge_attention(name, cfg, W, frames, f, start, worst):
    """the attention proper, fp32: the queries and the rings as read back after the Q launch -> tr_attn"""
    cur, L = frames[f], cfg.mimi.transformer.num_layers
    y64, e32 = R.fstage_e32(R.fstage_A, dict(cfg=cfg, W=W, fmt=None, q=cur["tr_q"], K=cur[f"tr_k{L - 1}"], V=cur[f"tr_v{L - 1}"], pos0=16 * (f - start)))
    got = cur["tr_attn"].astype(np.float64)
    assert got.shape == y64["attn"].shape and np.isfinite(got).all()
    note(worst, (name, "At", label_of_stage(cur["prof"], "At")), float(np.abs(got - y64["attn"]).max() / (FACTOR * e32["attn"])), 0.0, f)


def finish(worst):
    for key, v in worst.items():
        s = STATS.setdefault(key, [0.0, 0.0])
        s[0], s[1] = max(s[0], v[0]), max(s[1], v[1])
    bad = {k: [round(x, 2) for x in v] for k, v in worst.items() if not (v[0] <= 1 and v[1] <= 1)}
    assert not bad, bad


def judge(name, cfg, W, frames, unfused, resets=()):
    """finiteness and the bounds for every stage of every frame, each against its OWN E32 / E32s; records STATS"""
    B = frames[0]["latent"].shape[0]
    L = cfg.mimi.transformer.num_layers
    ring = frames[0][f"tr_k{L - 1}"].shape[1]
    worst = {}
    for f, cur in enumerate(frames):
        start = starts_of(B, f, resets)
        slots = ((16 * (f - start))[:, None] + np.arange(16)[None, :]) % ring
        cur["tr_krows"] = np.stack([cur[f"tr_k{L - 1}"][b, slots[b]] for b in range(B)])
        cur["tr_vrows"] = np.stack([cur[f"tr_v{L - 1}"][b, slots[b]] for b in range(B)])
        judge_f32(name, cfg, W, frames, f, "P", start, worst)
        judge_split(name, cfg, W, frames, f, "Q", start, worst)
        judge_attention(name, cfg, W, frames, f, start, worst)
        for stage in ["A" if L == 1 else "T", "B", "C", "D", "S0"]:
            judge_split(name, cfg, W, frames, f, stage, start, worst)
        for i in (1, 2, 3):
            judge_split(name, cfg, W, frames, f, f"C{i}", start, worst)
            if i in unfused:
                judge_split(name, cfg, W, frames, f, f"Ra{i}", start, worst)
                judge_split(name, cfg, W, frames, f, f"Rb{i}", start, worst)
            else:
                judge_f32(name, cfg, W, frames, f, f"R{i}", start, worst)
        judge_f32(name, cfg, W, frames, f, "L", start, worst)
    finish(worst)


def run_case(engines, name, B, opts=None, resets=(), case=()):
    eng, cfg, W = engines(name)
    opts = {**DEFAULTS, "debug_taps": 1, **(opts or {})}
    latents = R.seeded_latents(cfg, FRAMES, B, seed_of(name, B, sorted(opts.items()), resets, case))
    frames = decode_frames(eng, cfg, B, latents, opts, resets)
    unfused = [check_kernels(fr["prof"], cfg, B, opts) for fr in frames]
    assert all(u == unfused[0] for u in unfused), unfused
    assert unfused[0] == ([1, 2, 3] if not opts["fuse_res"] else [i for i in (1, 2, 3) if not fusable(cfg, i, B)]), unfused[0]
    judge(name, cfg, W, frames, unfused[0], resets)
    return frames


# one row tile; partial row tiles; MT 5
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("name", ["nf64", "nf64x2"])
def test_batches(engines, name, B):
    frames = run_case(engines, name, B)
    if name == "nf64":  # stage 1 is not fusable (hid 64, cout 256: 4 x 16 tiles), stages 2 and 3 keep the fused fp32 block
        assert all(at(fr["prof"], "seanet.res1b") and not at(fr["prof"], "seanet.res2b") for fr in frames)


def test_fuse_res_off(engines):
    """`fuse_res` 0: every residual conv runs on split, the 1x1 conv with the EPI_RES skip from craw"""
    frames = run_case(engines, "nf64", 3, dict(fuse_res=0))
    assert all(len([k for s, k in fr["prof"] if s.startswith("seanet.res") and "split" in pre_of(k)]) == 6 for fr in frames)


def test_production_launch_without_taps(engines):
    """`debug_taps` 0, what production runs.  Only the latents go in and the PCM comes out, so the PCM is judged against the
    fp64 CHAIN: the split stages where the profiler shows split, the fp32 stages elsewhere, and that chain's own float32 loss
    times 8, as tests/test_gpu_mimi_matrix.py::test_production_launch_without_taps"""
    eng, cfg, W = engines("nf64")
    B = 3
    latents = R.seeded_latents(cfg, FRAMES, B, seed_of("nf64", "no taps"))
    frames = decode_frames(eng, cfg, B, latents, DEFAULTS)
    unfused = [check_kernels(fr["prof"], cfg, B, DEFAULTS) for fr in frames]
    assert all(u == [1] for u in unfused), unfused
    worst = 0.0
    for f, (pcm64, e32) in enumerate(R.chain_e32(cfg, W, latents, split="", split_res=(1,))):
        got = frames[f]["pcm"]
        assert got.shape == pcm64.shape and np.isfinite(got).all()
        err = float(np.abs(got.astype(np.float64) - pcm64).max())
        worst = max(worst, err / (FACTOR * e32))
        print(f"  frame {f} chain err {err:.3e}  E32 {e32:.3e}  ratio to the bound {err / (FACTOR * e32):.3f}")
    STATS[("nf64", "chain", label_of_stage(frames[0]["prof"], "L"))] = [worst, 0.0]
    assert worst <= 1, worst


def test_reset_row(engines):
    """`reset_row` on the last row before frame 3: the reference restarts that row with zero tails at position 0"""
    run_case(engines, "nf64", 3, resets=((3, 2),))


def test_frame_pairs(engines):
    """the plan P, P, P on nf64x2 at B = 3: `mimi_decode_tr(lat, lat_b)` runs the split transformer on 32 rows per sequence
    (tr_in0), its outputs land in slots f & 3 of the hand-over ring; two `mimi_decode_seanet` calls follow.  Stage P and stage
    T (split model) for both frames of each pair, the SEANet stages as usual"""
    eng, cfg, W = engines("nf64x2")
    B, opts = 3, {**DEFAULTS, "debug_taps": 1}
    latents = R.seeded_latents(cfg, FRAMES, B, seed_of("nf64x2", "pairs"))
    unfused = [i for i in (1, 2, 3) if not fusable(cfg, i, B)]
    names = ["dec_tr", "seanet0"] + [f"seanet{k}" for k in (2, 3, 5, 6, 8, 9)] + [f"seanet_c{i}" for i in (1, 2, 3)] + [f"seanet_h{i}" for i in unfused]
    for k, v in opts.items():
        eng.set_option(k, v)
    ms = eng.new_mimi_state(B)
    frames = []
    try:
        for f in range(0, FRAMES, 2):
            eng.profile_start()
            eng.mimi_decode_tr(ms, dev(latents[f]), dev(latents[f + 1]))
            prof_tr = [(r["site"], r["kernel"]) for r in eng.profile_stop() for _ in range(r["count"])]
            torch.cuda.synchronize()
            u = read_taps(eng, ms, B, ["tr_in0"])["tr_in0"]
            assert u.shape[1] == 32, u.shape
            slots = [read_taps(eng, ms, B, [f"dec_tr_slot{g & 3}"])[f"dec_tr_slot{g & 3}"] for g in (f, f + 1)]
            for j in (0, 1):
                eng.profile_start()
                pcm = eng.mimi_decode_seanet(ms)
                prof = [(r["site"], r["kernel"]) for r in eng.profile_stop() for _ in range(r["count"])]
                torch.cuda.synchronize()
                t = dict(latent=latents[f + j], pcm=pcm.cpu().numpy(), prof=prof_tr + prof, upsample=u[:, 16 * j:16 * j + 16], tr_out=slots[j])
                t.update(read_taps(eng, ms, B, names))
                frames.append(t)
    except (PttsError, RuntimeError) as e:
        pytest.exit(f"GPU error in the split codec matrix, session ended: {e}", returncode=3)
    ms.close()
    for k, v in DEFAULTS.items():
        eng.set_option(k, v)
    worst = {}
    start = np.zeros(B, np.int64)
    for f, cur in enumerate(frames):
        assert check_kernels(cur["prof"], cfg, B, opts) == unfused
        assert np.array_equal(cur["tr_out"], cur["dec_tr"]), f  # the slot SEANet read is the one the pair wrote for this frame
        judge_f32("nf64x2", cfg, W, frames, f, "P", start, worst)
        judge_split("nf64x2", cfg, W, frames, f, "T", start, worst)
        judge_split("nf64x2", cfg, W, frames, f, "S0", start, worst)
        for i in (1, 2, 3):
            judge_split("nf64x2", cfg, W, frames, f, f"C{i}", start, worst)
            for stage in ((f"Ra{i}", f"Rb{i}") if i in unfused else ()):
                judge_split("nf64x2", cfg, W, frames, f, stage, start, worst)
            if i not in unfused:
                judge_f32("nf64x2", cfg, W, frames, f, f"R{i}", start, worst)
        judge_f32("nf64x2", cfg, W, frames, f, "L", start, worst)
    finish({(n, s + " pair" if s in ("P", "T") else s, k): v for (n, s, k), v in worst.items()})


# ---- every tile configuration at every split GEMM site ----------------------------------------------------------------
def split_sites(cfg, B):
    """site -> (NT, KF, MT, +ln) of a split engine's GEMM launches under the default options"""
    tr, sn = cfg.mimi.transformer, cfg.mimi.seanet
    C, FF = tr.d_model, tr.dim_feedforward
    s = {"mimi.qkv": (3 * C // 16, C // 16, B, True), "mimi.out": (C // 16, C // 16, B, False),
         "mimi.ff1": (FF // 16, C // 16, B, True), "mimi.ff2": (C // 16, FF // 16, B, False),
         "seanet.conv0": (8 * sn.n_filters // 16, sn.kernel_size * sn.dimension // 16, B, False)}
    for i, (cin, cout, hid, r, rin, rout) in enumerate(seanet_dims(cfg), 1):
        s[f"seanet.convtr{i}"] = (r * cout // 16, 2 * cin // 16, B * rin // 16, False)
        if not fusable(cfg, i, B):
            s[f"seanet.res{i}a"] = (hid // 16, 3 * cout // 16, B * rout // 16, False)
            s[f"seanet.res{i}b"] = (cout // 16, hid // 16, B * rout // 16, False)
    return s


def admitted(c, NT, KF, MT):
    """cfg_valid (csrc/ptts_dispatch.hip) for wfmt 3: split_cfg(c), whole pairs of k-fragments per wave, the shape rules"""
    s = CFG_SHAPE[c]
    if c not in SPLIT_CFGS or KF % (2 * s[2]):
        return False
    tn, tm = s[0] * s[3], s[1] * s[4]
    if (tm > 1 and tm > 2 * MT) or (tn > 1 and tn > 2 * NT):
        return False
    return not (s[2] > 1 and KF < 2)


def label_of(c, ln, NT, MT):
    s = CFG_SHAPE[c]
    threads = cdiv(NT, s[0] * s[3]) * cdiv(MT, s[1] * s[4]) * 64 * s[2] * s[3] * s[4]
    return f"{CFG_NAME[c]}{'+ln' if ln else ''}+split@{threads}"


_TABLES = {}


def tuned_table(eng, name, B):
    """the tuner's table of the split engine at batch B, measured once: its lines without the configuration column"""
    if (name, B) not in _TABLES:
        eng.tune(B, force=True)
        lines = [ln.split() for ln in eng._tune_table()]
        assert lines and all(len(f) == 14 for f in lines), "the tuner measured nothing (PTTS_NO_TUNE set?)"
        _TABLES[(name, B)] = [" ".join(f[:13]) for f in lines]
        eng.tune_clear()
    return _TABLES[(name, B)]


SWEEP = [(c, 5) for c in range(NCFG)] + [(c, 9) for c in (4, 5, 6)]  # 4, 5, 6: 16-row tile groups, transformer sites from MT 8


@pytest.mark.parametrize("c,B", SWEEP, ids=[f"{c}-B{B}" for c, B in SWEEP])
def test_every_tile_configuration(engines, c, B):
    """every line of the table tuned for B is rewritten to configuration c.  Where cfg_valid's wfmt-3 rule admits c the
    profiler must show EXACTLY c with `+split`; elsewhere a register-staged `+split` kernel other than c (choose_cfg's
    fall-back), never an fp32 or an LDS-staged one; every stage meets the bounds"""
    name = "nf64"
    eng, cfg, W = engines(name)
    keys = tuned_table(eng, name, B)
    sites = split_sites(cfg, B)
    SWEEP_CASES.setdefault(name, set()).add((c, B))
    try:
        assert eng.tune_import("".join(f"{k} {c}\n" for k in keys)) == len(keys)
        frames = run_case(engines, name, B, case=("cfg", c))
    finally:
        eng.tune_clear()
    for fr in frames:
        gemms = {s for s, k in fr["prof"] if k.startswith("gemm")}
        assert gemms == set(sites), (sorted(gemms), sorted(sites))
        for site, (NT, KF, MT, ln) in sites.items():
            for k in at(fr["prof"], site):
                if admitted(c, NT, KF, MT):
                    assert k == label_of(c, ln, NT, MT), (site, c, k)
                    SWEPT.setdefault(name, set()).add(c)
                else:
                    assert k.startswith("gemm<") and "split" in pre_of(k) and k.split("+")[0] != CFG_NAME[c], (site, c, k)


# ---- weight images, refusals, the packed file ----------------------------------------------------------------------
def weight_sites(cfg):
    L = cfg.mimi.transformer.num_layers
    return [(k, l) for l in range(L) for k in ("qkv", "out", "ff1", "ff2")] + [("conv0",)] + \
        [(k, i) for i in (1, 2, 3) for k in ("convtr", "res_a", "res_b")]


def test_weight_images_bit_for_bit(engines):
    """the hi and lo images every split launch multiplies by, as the engine packed them, against bf16(w) and
    bf16(w - bf16(w)) of the reference's own fp32 matrices (a +ln site: of the fp32 product w * ln_w); ln_s and ln_c of qkv and
    ff1 against the fold of the fp32 image within the bound tests/test_gpu_codec_matrix.py uses for ln_s, (K / 64 + 8) u of the
    absolute sum (fold_ln_kernel sums K / 64 terms per lane, then 6 shuffle steps)"""
    eng, cfg, W = engines("nf64x2")
    ms = eng.new_mimi_state(1)
    try:
        for site in weight_sites(cfg):
            tag = site[0] + (str(site[1]) if len(site) > 1 else "")
            f32 = R.site_weights(cfg, W, site, "f32")[0]
            want = R.split_parts(f32)
            assert np.any(want[1] != 0)
            for part, ref in zip(("wh_", "wl_"), want):
                got = eng.debug_read(ms, part + tag).cpu().numpy().astype(np.float64)
                if site[0] == "convtr":  # the packer's tap 0 is the previous input row, the reference's first half the current one
                    C = got.shape[1] // 2
                    got = np.concatenate([got[:, C:], got[:, :C]], axis=1)
                assert got.shape == ref.shape and np.array_equal(got, ref), (part, site)
            if site[0] in ("qkv", "ff1"):
                _, _, w0, g, beta = R._ln_site(cfg, W, site, np.float64)
                K = f32.shape[1]
                for vec, ref, mag in (("lns_", f32.sum(axis=1), np.abs(f32).sum(axis=1)), ("lnc_", w0 @ beta, np.abs(w0) @ np.abs(beta))):
                    got = eng.debug_read(ms, vec + tag).cpu().numpy().astype(np.float64)[0]
                    assert got.shape == ref.shape and (np.abs(got - ref) <= (K / 64 + 8) * 2.0 ** -24 * mag).all(), (vec, site)
        for name in ("wh_qkv2", "wl_convtr0", "wh_res_a4", "wh_conv1", "lns_out0", "lns_conv0"):
            with pytest.raises(PttsError, match="unknown buffer|folds no LayerNorm"):
                eng.debug_read(ms, name)
        with pytest.raises(PttsError, match="no reduced-precision weight image"):
            eng.debug_read(ms, "w_conv0")
    finally:
        ms.close()


def test_other_engines_refuse_the_split_images():
    from pocket_tts_amd.engine import Engine

    cfg, W = R.codec_weights("nf64")
    for groups in (None, {"codec_bf16"}):
        eng = Engine(cfg, W, "cuda:0", quantize_groups=groups)
        try:
            ms = eng.new_mimi_state(1)
            for name in ("wh_conv0", "wl_qkv0"):
                with pytest.raises(PttsError, match="only a split-bf16 engine"):
                    eng.debug_read(ms, name)
            ms.close()
        finally:
            eng.close()


def test_odd_fragment_counts_are_refused(engines):
    """"tiny" has 16-channel layers, so matrices with an odd number of k-fragments: the mode refuses the configuration at
    build time, and an engine created afterwards in the same process works"""
    from pocket_tts_amd.engine import Engine

    cfg, W = R.codec_weights("tiny")
    with pytest.raises(PttsError, match="even number of 16-wide k-fragments"):
        Engine(cfg, W, "cuda:0", quantize_groups={"codec_split"})
    cfg, W = R.codec_weights("nf64")
    eng = Engine(cfg, W, "cuda:0", quantize_groups={"codec_split"})
    try:
        ms = eng.new_mimi_state(2)
        lat = R.seeded_latents(cfg, 1, 2, 3)[0]
        pcm = eng.mimi_decode(ms, dev(lat)).cpu().numpy()
        want = engines("nf64")[0]
        ms2 = want.new_mimi_state(2)
        assert np.array_equal(pcm, want.mimi_decode(ms2, dev(lat)).cpu().numpy())
        ms.close()
        ms2.close()
    finally:
        eng.close()


def test_zz_error_table():
    """worst ratio to the bounds per (configuration, stage, kernel) of this session, the tile configurations that ran and the
    slowest tests; every admitted configuration ran at some site of a complete sweep"""
    print(f"\nsplit codec: worst ratio to the model bound {FACTOR} E32s (fp32 stages: {FACTOR} E32) and to the promise bound")
    for (name, stage, label), (m, p) in sorted(STATS.items()):
        print(f"  {name:6s} {stage:7s} {m:6.3f} {p:6.3f}  {label}")
    assert STATS and all(m <= 1 and p <= 1 for m, p in STATS.values())
    for name, ran in SWEPT.items():
        print(f"  {name}: tile configurations that ran: {sorted(ran)}")
    for name, forced in SWEEP_CASES.items():
        if forced == set(SWEEP):  # a complete sweep
            assert SWEPT.get(name) == set(SPLIT_CFGS), (name, SWEPT.get(name))
    for n, t in sorted(TIMES.items(), key=lambda kv: -kv[1])[:5]:
        print(f"  {t:6.1f} s  {n}")
