"""The FlowLM backbone built with reduced-precision weights (int8 attention, int8 FFN, both, bf16) against the fp64 reference
of tests/lm_ref.py, call by call, through the public engine calls: the driver, the cases and the per-call invariants are
those of tests/test_gpu_lm_matrix.py, the reference carries the format (`fmt`).  `-m gpu`.

Every judged call is judged on its own operands (caches, offsets and active flags read back before the call).  For the
residual stream of the real rows and the K and V rows the call wrote at every layer, elementwise

    |gpu - y64| <= FACTOR * E32(call, output) + F(call, element)          FACTOR = 8

E32: the loss of a float32 evaluation of the same model (dequantised int8 weights; for bf16 the stated weight images, fold
vectors and the fp64 master's operand roundings).  F: 0 for int8, which rounds no activation; for bf16 the flip allowance
of lm_ref.lm_judge: the sum, over the operand elements that lie within 8 e_site of a bf16 rounding midpoint and are
upstream of the output element, of what putting that element on its other neighbour does to the output.  Neither comes
from the kernels.  tests/test_lm_formats_reference_cpu.py shows that every seeded defect of lm_ref.MUTANTS moves a judged
element of one of these cases by >= 4 x this bound under each format.

bf16: every position of every call is judged by this bound, except in the four tiny prefills whose flip passes (one per
ambiguous element, each over the rest of its sequence) do not fit a test: (3, 33) bigmean and (2, 100) in its three
variants (lm_ref.JUDGE_ROWS).  There F is worked out for the first 8 or 32 positions of each sequence, exactly; layer 0's
K and V, which have no rounded intermediate upstream, have F = 0 at every position; and x and the later layers' K and V
at the later positions are held to FACTOR * E32nat, the deviation of the float32 evaluations that round their own
operands (lm_ref.lm_judge): of the order 1e-1 on outputs of order 1, which a wrong, stale or unwritten row or tile
fails.  The en100m prefill is judged on layer 0's K and V only (lm_ref.judge_args says why); en100m decode B = 1 in full.

Besides the bound every call asserts what the fp32 matrix asserts (finite outputs, exact offsets, every cache position
the call did not write bit-identical, `st.error()` false) and, from the profiler's records: `+q8` / `+b16` on exactly the
sites the format covers and on none it does not, `+ln` on lm.qkv and lm.ff1 only, the expected attention family at
lm.attn, and never an lm.cluster site, `lm_cluster=1` included: the single-launch stack is fp32 only.

The tile sweep forces every configuration the int8 / bf16 kernels admit (ADMITTED of tests/test_gpu_gemm_matrix.py) at
the four LM sites through the tuner's table; the last tests check the weight images bit for bit and the LayerNorm fold
vectors against their stated rule, and print the table below.

Measured worst |gpu - y64| / (8 E32 + F) per (config, format, family, kernel at lm.attn) on an MI355X (bound 1):
  config  fmt  family    lm.attn            x      K      V
  en100m  b16  decode    attn_decode     0.01   0.07   0.07
  en100m  b16  prefill   attn               -   0.12   0.07
  en100m  q8   decode    attn_decode     0.11   0.17   0.11
  en100m  q8   prefill   attn            0.08   0.09   0.08
  tiny    b16  borrowed  attn            0.47   0.55   0.62
  tiny    b16  borrowed  attn_cascade    0.59   0.86   0.85
  tiny    b16  borrowed  attn_decode     0.59   0.86   0.85
  tiny    b16  chunked   attn            0.11   0.21   0.22
  tiny    b16  cluster   attn_decode     0.00   0.13   0.15
  tiny    b16  decode    attn_decode     0.39   0.73   0.73
  tiny    b16  mixed     attn_decode     0.23   0.12   0.12
  tiny    b16  prefill   attn            0.15   0.82   0.85
  tiny    b16  prefill   attn_decode     0.00   0.12   0.17
  tiny    b16  ragged    attn            0.08   0.12   0.14
  tiny    q8   borrowed  attn            0.10   0.17   0.14
  tiny    q8   borrowed  attn_cascade    0.11   0.13   0.16
  tiny    q8   borrowed  attn_decode     0.08   0.14   0.15
  tiny    q8   chunked   attn            0.12   0.15   0.19
  tiny    q8   cluster   attn_decode     0.16   0.18   0.35
  tiny    q8   decode    attn_decode     0.23   0.18   0.35
  tiny    q8   mixed     attn_decode     0.16   0.13   0.17
  tiny    q8   prefill   attn            0.16   0.16   0.17
  tiny    q8   prefill   attn_decode     0.44   0.49   0.47
  tiny    q8   ragged    attn            0.12   0.14   0.13
  tiny    q8a  borrowed  attn            0.11   0.17   0.14
  tiny    q8a  borrowed  attn_cascade    0.11   0.15   0.15
  tiny    q8a  borrowed  attn_decode     0.11   0.14   0.15
  tiny    q8a  chunked   attn            0.11   0.15   0.19
  tiny    q8a  cluster   attn_decode     0.13   0.18   0.35
  tiny    q8a  decode    attn_decode     0.21   0.18   0.35
  tiny    q8a  mixed     attn_decode     0.15   0.15   0.17
  tiny    q8a  prefill   attn            0.16   0.16   0.17
  tiny    q8a  prefill   attn_decode     0.44   0.54   0.46
  tiny    q8a  ragged    attn            0.09   0.13   0.13
  tiny    q8f  borrowed  attn            0.10   0.14   0.08
  tiny    q8f  borrowed  attn_cascade    0.11   0.13   0.08
  tiny    q8f  borrowed  attn_decode     0.10   0.13   0.09
  tiny    q8f  chunked   attn            0.08   0.13   0.08
  tiny    q8f  cluster   attn_decode     0.15   0.14   0.18
  tiny    q8f  decode    attn_decode     0.18   0.15   0.20
  tiny    q8f  mixed     attn_decode     0.12   0.16   0.11
  tiny    q8f  prefill   attn            0.14   0.24   0.21
  tiny    q8f  prefill   attn_decode     0.15   0.16   0.14
  tiny    q8f  ragged    attn            0.08   0.11   0.07

(K, V: the worst layer; the tile sweep's runs included.  int8: 1 is 8 E32, so the kernels stay within 4.4 E32.  "cluster":
decode B = 3 with lm_cluster = 1, which ran the per-layer launches.  "-": not judged.  The ratio is against the bound the
element has, the late rule's included.)
bf16: 543744 of the 1513216 elements under 8 E32 + F on tiny and 34816 of 74752 on en100m have F = 0 and are held to 8 E32
alone; the worst among them is 0.33 x that on tiny, 0.12 on en100m.  203904 elements of the four long prefills are under
the late rule; the worst is 0.13 x 8 E32nat.
The sweep ran configurations [0, 1, 2, 3, 7, 10, 11] under int8 and [1, 2, 3, 7, 10, 11] under bf16 at an LM site.  The
slowest case takes 2.2 s (b16 prefill tiny-B3-T33-plain, nearly all of it the reference's flip passes).

Seeded, one at a time, in a local build that was not committed; each made tests of this module fail: the bf16 ln_s summed
from the unrounded rows (the six bf16 fold-vector tests, and K0 / V0 of a b16 prefill at 112 / 221 x the bound); the int8
ln_c without the bias (the six int8 fold-vector tests, 0.37 against 3.8e-6); layer 1 reading layer 0's ln_s (K1 / V1 at
2e3 .. 6e4 x the bound under q8 and b16); the attention-output operand of out_proj cut off instead of rounded under b16
(19 of the 23 tiny b16 cases, K1 / V1 at 18 .. 170 x, x at 2.6 .. 21 x the bound); lm_cluster = 1 honoured on an int8 engine
(the q8 and q8a cluster cases: an lm.cluster record).
"""

import hashlib
import time

import numpy as np
import pytest
import torch

from gemm_ref import CFG_SHAPE, PRE_LNFOLD, PRE_NONE
from lm_ref import FACTOR, b16_image, find_case, format_cases, judge_args, lm_judge, lm_weights, q8_image
from test_gpu_gemm_matrix import ADMITTED, cdiv
from test_gpu_gemm_matrix import label_of as gemm_label
from test_gpu_lm_matrix import GpuDriver, check_kernels

pytestmark = pytest.mark.gpu

GROUPS = {"q8a": {"attention"}, "q8f": {"ffn"}, "q8": {"attention", "ffn"}, "b16": {"lm_bf16"}}
# weight-format suffix of the attention Linears (lm.qkv, lm.out) and of the FFN Linears (lm.ff1, lm.ff2)
SUFFIX = {"q8a": ("q8", None), "q8f": (None, "q8"), "q8": ("q8", "q8"), "b16": ("b16", "b16")}
WFMT = {"q8": 1, "b16": 2}
TOL_FOLD = 2.0 ** -18  # fp32 accumulation, the bound of tests/test_gpu_gemm_matrix.py
STATS = {}   # (config, fmt, family, kernel at lm.attn, output kind) -> worst err / bound
ZERO = {}    # (config, fmt) -> [elements under 8 E32 + F, of them with F = 0, worst err / (8 E32) among those,
             #                    elements under the late rule, worst err / (8 E32nat) among those]
SLOWEST = [0.0, ""]
SWEPT = {}   # fmt -> configurations a sweep case ran at some LM site
FORCED = set()  # (fmt, configuration) the sweep forced in this session


@pytest.fixture(scope="module")
def engines():
    """one engine per (config, format) for the whole module"""
    from pocket_tts_amd.engine import Engine

    cache = {}

    def get(name, fmt):
        if (name, fmt) not in cache:
            cfg, W = lm_weights(name)
            cache[(name, fmt)] = Engine(cfg, W, "cuda:0", quantize_groups=GROUPS[fmt] if fmt else None)
        return cache[(name, fmt)]

    yield get
    for eng in cache.values():
        eng.close()


def site_kernels(prof, site):
    return [(k, n) for s, k, n in prof if s == site]


_REFERENCE = {}


def reference(cfg, W, snap, op, fmt, name, family, cid):
    """lm_judge of the call.  A tiny b16 prefill's reference is kept for the module: the tile sweep runs prefill (3, 33) once
    per configuration on the same operands (an empty cache and the case's embeddings), which the digest of all of them checks"""
    kw = judge_args(fmt, family, cid)
    if not (fmt == "b16" and name == "tiny" and family == "prefill"):
        return lm_judge(cfg, W, snap, op, fmt, **kw)
    h = hashlib.sha1(repr((cid, op[0], None if op[2] is None else list(op[2]))).encode())
    for a in [op[1], snap["off"], snap["active"], *snap["kv"]]:
        h.update(np.ascontiguousarray(a).tobytes())
    if h.digest() not in _REFERENCE:
        _REFERENCE[h.digest()] = lm_judge(cfg, W, snap, op, fmt, **kw)
    return _REFERENCE[h.digest()]


class FormatDriver(GpuDriver):
    """test_gpu_lm_matrix's driver on an engine of format `fmt`: the kernels a call must run and the bound it must meet"""

    def __init__(self, eng, name, family, cid, fmt):
        super().__init__(eng, name, family)
        self.cid, self.fmt = cid, fmt
        self.profs = []

    def check_kernels(self, prof, kind, attn):
        """the fp32 matrix's check with this format's suffixes; "lm_cluster" asked for: the per-layer launches all the same"""
        self.profs.append((kind, prof))
        assert not site_kernels(prof, "lm.cluster"), prof  # fp32 only: also with lm_cluster = 1
        check_kernels(prof, kind, "attn_decode" if attn == "lm_cluster" else attn, self.L, SUFFIX[self.fmt])

    def judge(self, s, snap, op, attn, got, start, n):
        kind = op[0]
        J = reference(self.cfg, self.W, snap, op, self.fmt, self.name, self.family, self.cid)
        assert list(J.ref64.off) == list(s.off) and list(J.res64.start) == list(start) and list(J.res64.n) == list(n)
        y64 = J.res64.outputs()
        attn = "attn_decode" if attn == "lm_cluster" else attn
        ratios = {}
        for name, ref in y64.items():
            g = got[name]
            assert g.shape == ref.shape and np.isfinite(g).all(), name
            if name not in J.outputs:
                continue
            assert J.e32[name] > 0
            err = np.abs(g.astype(np.float64) - ref)
            ratios[name] = float((err / J.bound(name)).max())
            z = ZERO.setdefault((self.name, self.fmt), [0, 0, 0.0, 0, 0.0])
            tight = J.F[name] == 0
            z[0] += int(np.isfinite(J.F[name]).sum())
            z[1] += int(tight.sum())
            if tight.any():
                z[2] = max(z[2], float(err[tight].max()) / (FACTOR * J.e32[name]))
            if name in J.late:
                mask, enat = J.late[name]
                z[3] += int(mask.sum())
                z[4] = max(z[4], float(err[mask].max()) / (FACTOR * enat))
        line = " ".join(f"{k} {v:.2f}" for k, v in ratios.items())
        print(f"  {self.name} {self.fmt} {self.family} {kind} B={s.B} n={int(n.max())} at {int(start.max())} [{attn}] |A|={J.nA}: {line}")
        for name, r in ratios.items():
            key = (self.name, self.fmt, self.family, attn, name[0])
            STATS[key] = max(STATS.get(key, 0.0), r)
            self.worst[name] = max(self.worst.get(name, 0.0), r)


def run_case(engines, fmt, family, cid):
    """-> [(call kind, profiler records)] of the case's calls"""
    _, name, fn, args = find_case(family, cid)
    t0 = time.perf_counter()
    d = FormatDriver(engines(name, fmt), name, family, cid, fmt)
    try:
        fn(d, *args)
    finally:
        d.finish()
    sec = time.perf_counter() - t0
    if sec > SLOWEST[0]:
        SLOWEST[:] = [sec, f"{fmt} {family} {cid}"]
    assert d.worst and all(v <= 1.0 for v in d.worst.values()), {k: round(v, 2) for k, v in d.worst.items() if v > 1.0}
    return d.profs


MATRIX = [(fmt, name, family, cid) for name in ("tiny", "en100m") for fmt in GROUPS for family, cid in format_cases(name, fmt)]


@pytest.mark.parametrize("fmt,name,family,cid", MATRIX, ids=[f"{m[0]}-{m[2]}-{m[3]}" for m in MATRIX])
def test_call_by_call(engines, fmt, name, family, cid):
    run_case(engines, fmt, family, cid)


# ---- every tile configuration the format admits, at the four LM sites -----------------------------------------------------
SWEEP_CASES = [("prefill", "tiny-B3-T33-plain"), ("decode", "tiny-B17")]


def lm_sites(eng, M):
    """site -> (NT, KF, MT, prologue) of the backbone's four GEMMs at M rows"""
    D, FF = eng.D, eng.D * eng.cfg.flow_lm.transformer.hidden_scale
    MT = cdiv(M, 16)
    return {"lm.qkv": (3 * D // 16, D // 16, MT, PRE_LNFOLD), "lm.out": (D // 16, D // 16, MT, PRE_NONE),
            "lm.ff1": (FF // 16, D // 16, MT, PRE_LNFOLD), "lm.ff2": (D // 16, FF // 16, MT, PRE_NONE)}


def admitted(c, wfmt, NT, KF, MT):
    """cfg_valid (csrc/ptts_dispatch.hip) for int8 / bf16 weights: whole groups of four / two k-fragments per wave"""
    s = CFG_SHAPE[c]
    if c not in ADMITTED[wfmt] or KF % ((4 if wfmt == 1 else 2) * s[2]):
        return False
    tn, tm = s[0] * s[3], s[1] * s[4]
    if (tm > 1 and tm > 2 * MT) or (tn > 1 and tn > 2 * NT):
        return False  # mostly padding
    return not (s[2] > 1 and KF < 2)


_TABLES = {}


def tuned_keys(eng, fmt):
    """the table lines (without the configuration) the tuner measures for the sweep's two shapes, this format's GEMMs only"""
    if fmt not in _TABLES:
        from pocket_tts_amd import _lib

        eng.tune(17, force=True)
        eng._pre()
        _lib.check(eng.lib.ptts_tune_prefill(eng.handle, 3, 33, eng._sp))
        eng.sync()
        lines = [ln.split() for ln in eng._tune_table()]
        assert lines and all(len(f) == 14 for f in lines), "the tuner measured nothing (PTTS_NO_TUNE set?)"
        _TABLES[fmt] = [" ".join(f[:13]) for f in lines if int(f[12]) == WFMT[fmt]]
        eng.tune_clear()
        assert len(_TABLES[fmt]) >= 8, _TABLES[fmt]  # four sites at two row counts
    return _TABLES[fmt]


_BASE = {}


def heuristic_labels(engines, fmt, family, cid):
    """site -> the labels the case runs with an empty table: what the dispatcher falls back to where it does not admit a
    forced configuration"""
    if (fmt, cid) not in _BASE:
        engines("tiny", fmt).tune_clear()
        profs = run_case(engines, fmt, family, cid)
        _BASE[(fmt, cid)] = {site: {k for kind, p in profs if kind == family for k, _ in site_kernels(p, site)}
                             for site in ("lm.qkv", "lm.out", "lm.ff1", "lm.ff2")}
    return _BASE[(fmt, cid)]


@pytest.mark.parametrize("fmt,c", [(fmt, c) for fmt, wf in WFMT.items() for c in sorted(ADMITTED[wf])])
def test_every_admitted_tile_configuration(engines, fmt, c):
    """every line of the tuner's table for this format is rewritten to configuration c; a prefill (3, 33) and decode steps at
    B = 17 then meet the same bound, and each LM site shows c where cfg_valid admits it for the site's shape and the
    label of the untuned run where it does not (choose_cfg's documented fall-back: the heuristic's choice, else tile 3 or
    11, which at a single row tile may be the very tile cfg_valid calls mostly padding)"""
    wf = WFMT[fmt]
    eng = engines("tiny", fmt)
    keys = tuned_keys(eng, fmt)
    base = {cid: heuristic_labels(engines, fmt, family, cid) for family, cid in SWEEP_CASES}
    try:
        assert eng.tune_import("".join(f"{k} {c}\n" for k in keys)) == len(keys)
        profs = {cid: run_case(engines, fmt, family, cid) for family, cid in SWEEP_CASES}
    finally:
        eng.tune_clear()
    FORCED.add((fmt, c))
    for (family, cid), M in zip(SWEEP_CASES, (3 * 33, 17)):
        calls = [prof for kind, prof in profs[cid] if kind == family]  # not the prefill that gives the decode steps a context
        assert calls
        for prof in calls:
            for site, (NT, KF, MT, pre) in lm_sites(eng, M).items():
                labels = {k for k, _ in site_kernels(prof, site)}
                if admitted(c, wf, NT, KF, MT):
                    assert labels == {gemm_label(c, pre, wf, NT, MT)}, (site, c, labels)
                    SWEPT.setdefault(fmt, set()).add(c)
                else:
                    assert labels == base[cid][site], (site, c, labels, base[cid][site])


# ---- weight images and fold vectors against their stated rule ---------------------------------------------------------------
def linear_shapes():
    """(config, layer, Linear, its norm) of tiny's four Linear shapes and en100m's in_proj and linear2"""
    tiny = [("tiny", 1, lin, norm) for lin, norm in (("self_attn.in_proj", "norm1"), ("self_attn.out_proj", "norm1"),
                                                    ("linear1", "norm2"), ("linear2", "norm2"))]
    return tiny + [("en100m", 0, "self_attn.in_proj", "norm1"), ("en100m", 1, "linear2", "norm2")]


@pytest.mark.parametrize("pre", [PRE_NONE, PRE_LNFOLD], ids=["plain", "lnfold"])
@pytest.mark.parametrize("wfmt", [0, 1, 2], ids=["fp32", "int8", "bf16"])
@pytest.mark.parametrize("name,layer,lin,norm", linear_shapes(), ids=lambda v: str(v))
def test_weight_image_and_fold_vectors(engines, name, layer, lin, norm, wfmt, pre):
    """the load-time kernels (pack_weight, fold_ln, quantize_packed, pack_weight_b16) on the model's own matrices: w_eff
    bit for bit the numpy rule of lm_ref, ln_s and ln_c within 2^-18 sum|terms| of the fp64 sums of their definition.
    The norm's gain and bias are the checkpoint's where it follows that norm; a bias is added to exercise ln_c's."""
    _, W = lm_weights(name)
    p = f"flow_lm.transformer.layers.{layer}."
    w = np.asarray(W[p + lin + ".weight"], np.float32)
    N, K = w.shape
    rng = np.random.default_rng(N + K + wfmt)
    g = np.asarray(W[p + norm + ".weight"], np.float32) if K == len(W[p + norm + ".weight"]) else (1 + 0.2 * rng.standard_normal(K)).astype(np.float32)
    beta = np.asarray(W[p + norm + ".bias"], np.float32) if K == len(W[p + norm + ".bias"]) else (0.1 * rng.standard_normal(K)).astype(np.float32)
    if not np.abs(beta).max() > 0:  # a synthetic checkpoint with zero norm biases would leave ln_c = bias
        beta = (0.1 * rng.standard_normal(K)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(N)).astype(np.float32)
    x = rng.standard_normal((16, K)).astype(np.float32)
    fold = pre == PRE_LNFOLD
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")  # noqa: E731
    out = engines("tiny", None).debug_gemm(t(x), t(w), want_weights=True, wfmt=wfmt, pre=pre, bias=t(bias),
                                           ln_w=t(g) if fold else None, ln_b=t(beta) if fold else None)
    assert out is not None
    if wfmt == 0:
        rule = (w * g[None, :]).astype(np.float32) if fold else w
    elif wfmt == 1:
        q, scale = q8_image(w)
        rule = (q * scale).astype(np.float32)  # exact in fp64, rounded once: what the unpacker's float product gives
        assert np.array_equal(rule, (q.astype(np.float64) * scale.astype(np.float64)).astype(np.float32))
    else:
        rule = b16_image(w, g if fold else None)
    w_eff = out["w_eff"].cpu().numpy()
    bad = np.argwhere(w_eff.view(np.uint32) != np.ascontiguousarray(rule).view(np.uint32))
    assert not len(bad), (len(bad), bad[:4], w_eff[tuple(bad[0])], rule[tuple(bad[0])])
    if not fold:
        return
    w64, r64, g64, b64 = w.astype(np.float64), rule.astype(np.float64), g.astype(np.float64), beta.astype(np.float64)
    if wfmt == 0:    # sum_k W g, sum_k W beta + bias
        ts, tc = w64 * g64, w64 * b64
    elif wfmt == 1:  # both from the dequantised rows
        ts, tc = r64 * g64, r64 * b64
    else:            # s from the rounded rows (the gain is in them), c from the fp32 rows
        ts, tc = r64, w64 * b64
    for what, got, terms, add in (("ln_s", out["ln_s"], ts, 0.0), ("ln_c", out["ln_c"], tc, bias.astype(np.float64))):
        want = terms.sum(axis=1) + add
        scale = np.abs(terms).sum(axis=1) + np.abs(add)
        err = np.abs(got.cpu().numpy().astype(np.float64) - want) / scale
        print(f"  {name} {lin} wfmt {wfmt} {what}: worst |got - fp64| / sum|terms| = {err.max():.2e} (bound {TOL_FOLD:.2e})")
        assert err.max() <= TOL_FOLD, (what, int(err.argmax()), float(err.max()))


# ---- the table ------------------------------------------------------------------------------------------------------------
def test_zz_error_table_and_coverage():
    """worst err / bound per (config, format, family, kernel at lm.attn) of this session; every (format, admitted
    configuration) pair seen by a complete sweep"""
    print(f"\nFlowLM backbone, reduced formats: worst |gpu - y64| / ({FACTOR} E32 + F) (bound 1)")
    print(f"  {'config':7s} {'fmt':4s} {'family':9s} {'lm.attn':13s} {'x':>6s} {'K':>6s} {'V':>6s}")
    for key in sorted({k[:4] for k in STATS}):
        print(f"  {key[0]:7s} {key[1]:4s} {key[2]:9s} {key[3]:13s}" + "".join(f" {STATS[key + (o,)]:6.2f}" if key + (o,) in STATS else f" {'-':>6s}" for o in "xKV"))
    for (name, fmt), (judged, tight, worst, late, worst_late) in sorted(ZERO.items()):
        if fmt == "b16":
            print(f"  {name} b16: {tight} of {judged} elements under {FACTOR} E32 + F ({tight / max(judged, 1):.3f}) have F = 0; worst |gpu - y64| / "
                  f"({FACTOR} E32) among them {worst:.2f}; {late} elements under the late rule, worst |gpu - y64| / ({FACTOR} E32nat) {worst_late:.2f}")
    print(f"  slowest case: {SLOWEST[0]:.1f} s ({SLOWEST[1]})")
    for fmt, ran in SWEPT.items():
        print(f"  {fmt}: tile configurations that ran at an LM site: {sorted(ran)}")
    assert all(v <= 1.0 for v in STATS.values())
    for fmt, wf in WFMT.items():
        if {c for f, c in FORCED if f == fmt} == ADMITTED[wf]:  # a complete sweep: every admitted configuration ran somewhere
            assert SWEPT.get(fmt) == ADMITTED[wf], (fmt, SWEPT.get(fmt))
