"""Every compiled attention instantiation of the hot path (attn_kernel, attn_decode_kernel, attn_decode2_kernel,
attn_cascade_kernel, + attn_combine_kernel on split keys), one launch at a time through the production dispatcher
(Engine.debug_attn -> ptts_debug_attn), against the float64 reference of tests/attn_ref.py on the operands the kernel
consumed, at the mask, tile, split, ring and prefix edges production produces.

Bound.  With u = 2^-24, a score is a 64-term fp32 dot product: its error is at most ~64 u * S, where S = sum_e |q_e k_e| / 8
(the worst attended key).  An error d in every score moves the softmax weights by a relative ~2d, hence the output by
~2d * max|v|; the exponentials (a few ulp each), the online rescales and the sums over keys, waves and splits add a few
hundred u * max|v| at the key counts tested (<= ~700).  Together, per (row, query, head):

    |y - ref| <= 2^-18 * max|v| * (1 + S)          (2^-18 = 64 u; max|v|, S over the query's attended keys)

h16 (bf16 output): |y - bf16(ref)| <= one bf16 ulp + that bound.  Every slot a row must not read holds poison K = 0,
V = 1e6: one key included by mistake moves the output by ~1e6 / n_keys * e^(-|s|), far past the bound on unit-range
inputs.  Every case also asserts finite output, untouched guards (the hook checks them) and bitwise-equal repeats."""

import math
import os
from collections import defaultdict

import numpy as np
import pytest
import torch

from attn_ref import attn_ref, bf16_round, bf16_ulp, bound, histories

pytestmark = pytest.mark.gpu

# mirror of kAttn in ptts_dispatch.hip: (family, nw or R, pw, depth, ns, cascade code); family 0 attn_kernel, 1 attn_decode_kernel,
# 2 attn_decode2_kernel, 3 attn_cascade_kernel
KERNELS = [
    ("attn<4,3>", 0, 4, 0, 3, 0, 0), ("attn<2,3>", 0, 2, 0, 3, 0, 0), ("attn<1,3>", 0, 1, 0, 3, 0, 0),
    ("attn<1,2>", 0, 1, 0, 2, 0, 0), ("attn_decode<1>", 1, 1, 0, 3, 0, 0), ("attn_decode2<1,2>", 2, 1, 0, 2, 0, 0),
    ("attn_decode2<1,3>", 2, 1, 0, 3, 0, 0), ("attn_decode2<2,3>", 2, 2, 0, 3, 0, 0), ("attn_decode2<4,3>", 2, 4, 0, 3, 0, 0),
    ("attn_decode2<8,3>", 2, 8, 0, 3, 0, 0), ("attn_cascade<4,2,3,1>", 3, 4, 2, 3, 1, 423),
    ("attn_cascade<4,4,2,2>", 3, 4, 4, 2, 2, 442), ("attn_cascade<2,2,2,2>", 3, 2, 2, 2, 2, 222),
    ("attn_cascade<4,2,2,1>", 3, 4, 2, 2, 1, 42), ("attn_cascade<4,4,2,1>", 3, 4, 4, 2, 1, 44),
    ("attn_cascade<8,4,2,1>", 3, 8, 4, 2, 1, 84), ("attn_cascade<2,2,2,1>", 3, 2, 2, 2, 1, 22),
]
NK = len(KERNELS)
IDX = {k[0]: i for i, k in enumerate(KERNELS)}
KNOBS = ("PTTS_ATTN_NW", "PTTS_ATTN_KERNEL_NW", "PTTS_ATTN_DEPTH", "PTTS_ATTN_V", "PTTS_ATTN_WAVES")
POISON_K, POISON_V = 0.0, 1e6

STATS = defaultdict(lambda: [0.0, 0])  # (kernel, h16) -> [worst |y - ref| / bound, cases]
PROD_LABELS = []


def cdiv(a, b):
    return (a + b - 1) // b


# ---- Python mirror of the dispatcher's rules (ptts_dispatch.hip: decode_attn_waves, attn_nw, attn_splits, choose_attn, attn_valid)
def decode_attn_waves(BH):
    nw = 1
    while nw < 8 and BH * nw * 2 <= 1024:
        nw *= 2
    return nw


def attn_nw(base):
    return 4 if base <= 128 else (2 if base <= 256 else 1)


def attn_splits(base, max_tiles):
    nw = attn_nw(base)
    s = max(1, cdiv(1024, max(1, base * nw)))
    return max(1, min(s, cdiv(max_tiles, nw)))


def prod_splits(B, H, Tq, cap, ring, ctx):
    QB = cdiv(Tq, 16)
    if Tq == 1 and not ring:
        return 1  # FlowLM decode step
    if ring:
        return attn_splits(B * H, ring // 16)  # codec state
    if ctx > 0:
        return attn_splits(B * H * QB, min(QB, cdiv(ctx, 16) + 2))  # encoder transformer
    return attn_splits(B * H * QB, cdiv(cap, 16))  # FlowLM prefill


def choose(B, H, Tq, splits, ring, ctx, has_pre, cascade):
    BH, QB = B * H, cdiv(Tq, 16)
    if Tq == 1 and cascade and has_pre and splits == 1 and not ring and ctx <= 0 and B >= 16:
        return next((i for i, k in enumerate(KERNELS) if k[6] == cascade), IDX["attn_cascade<4,2,3,1>"])
    if Tq == 1:
        nw = decode_attn_waves(BH)
        return IDX[{8: "attn_decode2<8,3>", 4: "attn_decode2<4,3>", 2: "attn_decode2<2,3>"}.get(nw, "attn_decode2<1,2>")]
    nw = attn_nw(BH * QB)
    return IDX[{4: "attn<4,3>", 2: "attn<2,3>"}.get(nw, "attn<1,2>")]


def label_of(k, B, H, Tq, splits):
    _, fam, nw, pw, _, ns, _ = KERNELS[k]
    if fam == 3:
        return f"attn_cascade@{cdiv(B, nw) * H * 64 * (nw * ns + pw)}"
    if fam == 0:
        return f"attn@{B * H * cdiv(Tq, 16) * splits * 64 * nw}"
    return f"attn_decode@{B * H * splits * 64 * nw}"


def admitted(k, case):
    """attn_valid on the (valid) cases of this file: decode and cascade kernels take one query and fp32 output; the
    cascade kernel one split, a linear cache without window and a prefix table"""
    fam = KERNELS[k][1]
    if fam != 0 and (case["Tq"] != 1 or case["h16"]):
        return False
    if fam == 3 and (case["splits"] != 1 or case["ring"] or case["ctx"] > 0 or case["pk"] is None):
        return False
    return True


@pytest.fixture(scope="module")
def eng():
    from pocket_tts_amd.config import named_config
    from pocket_tts_amd.engine import Engine
    from pocket_tts_amd.weights import generate_state_dict

    cfg = named_config("tiny")
    e = Engine(cfg, generate_state_dict(cfg, 0), "cuda:0")
    yield e
    e.close()


def make_case(offsets, *, Tq=1, H=4, cap=None, T=None, ring=0, ctx=0, splits=-1, h16=0, layer=0, banks=None, pre_id=None,
              pre_cap=0, numerics="unit", seed=0):
    """operands of one launch (numpy float32) and their float64 reference.  banks: prefix lengths [n_pre]; pre_id [B].
    numerics: "unit" U(-1, 1); "big" scores up to |s| ~ 100; "equal" every score equal; "bigv" values ~ 1e3"""
    rng = np.random.default_rng(seed)
    B = len(offsets)
    T = T or max(offsets) + Tq
    cap = cap or cdiv(T, 16) * 16
    u = lambda *s: rng.uniform(-1.0, 1.0, s).astype(np.float32)
    q, k, v = u(B, Tq, H, 64), u(B, T, H, 64), u(B, T, H, 64)
    pk = pv = None
    if banks is not None:
        pT = max(max(banks), 1)
        pk, pv = u(len(banks), pT, H, 64), u(len(banks), pT, H, 64)
    if numerics == "big":  # |s| = |q.k| / 8 up to ~100
        a = np.float32(math.sqrt(300.0))
        q, k = q * a, k * a
        pk = pk * a if pk is not None else None
    elif numerics == "equal":
        q, k = np.full_like(q, 0.5), np.full_like(k, 0.5)
        pk = np.full_like(pk, 0.5) if pk is not None else None
    elif numerics == "bigv":
        v = v * np.float32(1e3)
        pv = pv * np.float32(1e3) if pv is not None else None
    K, V = histories(k, v, pk, pv, banks, pre_id)
    ref = attn_ref(q, K, V, offsets, ctx)
    return dict(q=torch.from_numpy(q), k=torch.from_numpy(k), v=torch.from_numpy(v), offset=list(offsets),
                pk=None if pk is None else torch.from_numpy(pk), pv=None if pv is None else torch.from_numpy(pv),
                pre_len=banks, pre_id=pre_id, B=B, Tq=Tq, H=H, cap=cap, ring=ring, ctx=ctx, splits=splits, h16=h16,
                layer=layer, pre_cap=pre_cap, ref=ref)


def run(eng, case, kernel=-1, cascade=0):
    ints = {f: case[f] for f in ("cap", "ring", "ctx", "splits", "h16", "layer", "pre_cap")}
    return eng.debug_attn(case["q"], case["k"], case["v"], case["offset"], pk=case["pk"], pv=case["pv"],
                          pre_len=case["pre_len"], pre_id=case["pre_id"], poison_k=POISON_K, poison_v=POISON_V,
                          kernel=kernel, cascade=cascade, **ints)


def check(case, out, k, what=""):
    """output against the reference within the docstring's bound; the same launch again is bitwise equal"""
    y = out["y"].cpu().numpy().astype(np.float64)
    name = KERNELS[k][0]
    assert np.isfinite(y).all(), f"{name} {what}: non-finite output (unwritten queries read back as NaN)"
    ref, s1, vmax = case["ref"]
    tol = np.repeat(bound(s1, vmax), 64, axis=-1)
    want = ref
    if case["h16"]:
        want = bf16_round(ref)
        tol = tol + bf16_ulp(np.abs(ref) + tol)
    ratio = np.abs(y - want) / tol
    worst = float(ratio.max())
    st = STATS[(k, case["h16"])]
    st[0], st[1] = max(st[0], worst), st[1] + 1
    if worst > 1.0:
        b, t, n = np.unravel_index(int(ratio.argmax()), ratio.shape)
        raise AssertionError(f"{name} {what}: |y - ref| = {abs(y[b, t, n] - want[b, t, n]):.3e} at row {b} (offset "
                             f"{case['offset'][b]}) query {t} col {n}, {worst:.2f}x the bound {tol[b, t, n]:.3e}")


def run_all(eng, case, what=""):
    """every kernel of the table on `case`: the hook runs exactly the admitted ones, each within the bound, repeatably"""
    ran = set()
    for k in range(NK):
        out = run(eng, case, k)
        if out is None:
            continue
        ran.add(k)
        assert out["kernel"] == k
        check(case, out, k, what)
        again = run(eng, case, k)
        assert torch.equal(out["y"], again["y"]), f"{KERNELS[k][0]} {what}: two launches differ"
    want = {k for k in range(NK) if admitted(k, case)}
    assert ran == want, f"{what}: ran {sorted(ran)}, the validity rules admit {sorted(want)}"


EDGE_OFFSETS = [0, 1, 14, 15, 16, 17, 31, 32, 33, 111, 112, 113, 159, 160, 161, 221, 281, 282, 283]


def spread(cap, Tq, n, seed):
    """n offsets across [0, cap - Tq] with duplicates"""
    r = np.random.default_rng(seed).integers(0, cap - Tq + 1, n).tolist()
    return r + r[:3]


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tq", [1, 16])
def test_offsets(eng, Tq):
    """queries at the tile edges, at position 0 and at cap - 1: every row of one launch at its own offset"""
    cap = 304
    offs = [o for o in EDGE_OFFSETS if o + Tq <= cap] + [cap - Tq]
    run_all(eng, make_case(offs, Tq=Tq, cap=cap, splits=1, seed=Tq), f"offsets Tq={Tq}")
    run_all(eng, make_case(spread(cap, Tq, 13, Tq), Tq=Tq, cap=cap, splits=1, seed=Tq + 1), f"spread Tq={Tq}")


@pytest.mark.parametrize("splits", [2, 3, 5, 8, 19, 40])
def test_splits(eng, splits):
    """keys split over workgroups + the combine kernel; 19 tiles at most, so from 19 splits on some own no tiles"""
    cap = 304
    offs = [0, 1, 15, 16, 47, 160, 221, 283, cap - 1]
    run_all(eng, make_case(offs, cap=cap, splits=splits, seed=splits), f"splits={splits} Tq=1")
    offs = [0, 17, 100, 281, cap - 16]
    run_all(eng, make_case(offs, Tq=16, cap=cap, splits=splits, seed=splits + 1), f"splits={splits} Tq=16")


@pytest.mark.parametrize("h16", [0, 1])
@pytest.mark.parametrize("splits", [1, 3, -1])
def test_ring(eng, splits, h16):
    """the codec's ring: 272 slots, context 250, frames at offsets that wrap it"""
    offs = [0, 16, 240, 256, 272, 288, 1600]
    run_all(eng, make_case(offs, Tq=16, H=8, cap=272, T=1616, ring=272, ctx=250, splits=splits, h16=h16, seed=7),
            f"ring frame splits={splits} h16={h16}")
    if not h16:
        offs = [0, 15, 249, 250, 271, 272, 273, 1615]
        run_all(eng, make_case(offs, Tq=1, H=8, cap=272, T=1616, ring=272, ctx=250, splits=splits, seed=8),
                f"ring decode splits={splits}")


@pytest.mark.parametrize("ctx", [0, 40])
@pytest.mark.parametrize("Tq", [1, 7, 16, 17, 39, 158])
def test_query_blocks(eng, Tq, ctx):
    """partial and multiple query blocks, with and without a window"""
    cap = 336
    offs = [0, 5, 33, 100, cap - Tq]
    run_all(eng, make_case(offs, Tq=Tq, H=2, cap=cap, ctx=ctx, splits=1, seed=Tq + ctx), f"Tq={Tq} ctx={ctx}")
    if Tq > 1:
        run_all(eng, make_case(offs, Tq=Tq, H=2, cap=cap, ctx=ctx, splits=3, h16=1, seed=Tq + ctx + 1),
                f"Tq={Tq} ctx={ctx} h16 splits=3")


@pytest.mark.parametrize("layer", [0, 5])
@pytest.mark.parametrize("Tq", [1, 7])
def test_prefix_lengths(eng, Tq, layer):
    """prefixes of 0, 16, 112, 113 and 127 keys, queries at len and at len + 40, a row without a prefix; owner caches of
    another capacity, the prefix in plane `layer` of layers 0 .. layer + 1"""
    banks = [0, 16, 112, 113, 127]
    pre_id, offs = [], []
    for j, n in enumerate(banks):
        pre_id += [j, j]
        offs += [n, n + 40]
    pre_id.append(-1)
    offs.append(77)
    for splits in (1, 2):
        case = make_case(offs, Tq=Tq, cap=192, splits=splits, banks=banks, pre_id=pre_id, pre_cap=144, layer=layer,
                         seed=layer + Tq + splits)
        run_all(eng, case, f"prefix Tq={Tq} layer={layer} splits={splits}")


@pytest.mark.parametrize("nseq", [17, 63])
def test_cascade_groups(eng, nseq):
    """groups of R rows that mix a prefix row with a non-prefix row, two owners with equal len, one owner with another
    len, a partial last group"""
    banks = [112, 112, 128, 113]
    pattern = [0, 0, 0, 0, 0, -1, 0, 0, 0, 1, 0, 1, 2, 0, 0, 0, 3, 3, 0, 0, -1, -1, -1, -1]
    pre_id = [pattern[b % len(pattern)] for b in range(nseq)]
    rng = np.random.default_rng(nseq)
    offs = [(banks[j] if j >= 0 else 0) + int(rng.integers(0, 120)) for j in pre_id]
    offs[0] = banks[0]  # the query at the prefix's length
    run_all(eng, make_case(offs, H=2, cap=256, splits=1, banks=banks, pre_id=pre_id, seed=nseq), f"cascade nseq={nseq}")


@pytest.mark.parametrize("numerics", ["unit", "big", "equal", "bigv"])
def test_numerics(eng, numerics):
    """scores up to |s| ~ 100 (fp32 exp overflows without the running max), all-equal scores, values ~ 1e3"""
    run_all(eng, make_case([0, 16, 100, 221, 283], cap=304, splits=1, numerics=numerics, seed=3), f"{numerics} Tq=1")
    run_all(eng, make_case([0, 16, 100, 221, 283], cap=304, splits=4, numerics=numerics, seed=4), f"{numerics} splits=4")
    run_all(eng, make_case([0, 272, 1600], Tq=16, H=8, cap=272, T=1616, ring=272, ctx=250, numerics=numerics, seed=5),
            f"{numerics} ring")
    banks, pre_id = [112], [0] * 8 + [-1]
    run_all(eng, make_case([112, 130, 200, 112, 150, 160, 170, 180, 90], cap=256, splits=1, banks=banks, pre_id=pre_id,
                           numerics=numerics, seed=6), f"{numerics} prefix")


# ---------------------------------------------------------------------------------------------------------------------
def prod_cases():
    """the production launch shapes: (id, make_case kwargs, cascade option)"""
    out = []
    for B in (1, 4, 8, 16, 32, 64):  # en100m FlowLM decode step
        offs = [221 + (b * 31) % 63 for b in range(B)]
        for pre in (False, True):
            for casc in ((0, 423) if pre else (0,)):
                kw = dict(offsets=offs, H=16, cap=400)
                if pre:
                    kw.update(banks=[112], pre_id=[0] * B)
                out.append((f"decode-B{B}-{'pre' if pre else 'nopre'}-casc{casc}", kw, casc))
    out.append(("prefill-Tq158", dict(offsets=[0], Tq=158, H=16, cap=176), 0))
    out.append(("prefill-Tq158-pre", dict(offsets=[112], Tq=158, H=16, cap=272, banks=[112], pre_id=[0]), 0))
    for B in (1, 64):  # codec frame
        for h16 in (0, 1):
            offs = [1600 + 16 * (b % 5) for b in range(B)]
            out.append((f"codec-B{B}-h16{h16}", dict(offsets=offs, Tq=16, H=8, cap=272, T=1700, ring=272, ctx=250, h16=h16), 0))
    out.append(("encoder-720", dict(offsets=[0], Tq=720, H=8, cap=720, ctx=250), 0))
    return out


@pytest.mark.parametrize("pid,kw,cascade", prod_cases(), ids=[c[0] for c in prod_cases()])
def test_production_choice(eng, pid, kw, cascade):
    """the dispatcher's kernel, splits and label for each production launch shape, and its output"""
    if any(os.environ.get(k) for k in KNOBS):
        pytest.skip("an attention A/B knob is set")
    kw = dict(kw)
    offs = kw.pop("offsets")
    case = make_case(offs, seed=len(offs), **kw)
    B, H, Tq = case["B"], case["H"], case["Tq"]
    splits = prod_splits(B, H, Tq, case["cap"], case["ring"], case["ctx"])
    k = choose(B, H, Tq, splits, case["ring"], case["ctx"], case["pk"] is not None, cascade)
    out = run(eng, case, -1, cascade)
    assert out is not None
    assert (out["kernel"], out["splits"]) == (k, splits), (KERNELS[out["kernel"]][0], out["splits"], KERNELS[k][0], splits)
    assert out["label"] == label_of(k, B, H, Tq, splits)
    check(case, out, k, pid)
    PROD_LABELS.append((pid, out["label"], KERNELS[k][0]))


def test_zz_error_tables():
    """worst scaled error per kernel and output type; every kernel of the table ran"""
    if not STATS:
        pytest.skip("no case ran in this session")
    print("\nworst max|y - ref| / bound per attention kernel (fp32: bound 2^-18 * max|v| * (1 + S); bf16: + one bf16 ulp)")
    for k in range(NK):
        for h16, kind in ((0, "fp32"), (1, "bf16")):
            if (k, h16) in STATS:
                e, n = STATS[(k, h16)]
                print(f"  {k:2d} {KERNELS[k][0]:24s} {kind}  {e:.3e}  ({n} cases)")
    for pid, label, name in PROD_LABELS:
        print(f"  production {pid:28s} {label:24s} {name}")
    missing = [KERNELS[k][0] for k in range(NK) if (k, 0) not in STATS]
    assert not missing, f"kernels no case ran: {missing}"
