"""Every tile configuration x weight format x prologue x epilogue of the hot path's GEMM kernel family, one GEMM at a time
through the production dispatcher (Engine.debug_gemm -> ptts_debug_gemm), against the float64 reference of
tests/gemm_ref.py on the operands the kernel consumed.  Kernel and reference differ only by the fp32 summation order, so
the bound is fp32-accumulation tight: max |y - ref| <= 2^-18 * max(rs * sum_k |x_k w_k| + |b|), per case."""

import math
from collections import defaultdict
from pathlib import Path

import pytest
import torch

from gemm_ref import (ACT_ELU, ACT_GELU, ACT_NONE, ACT_SILU, CFG_NAME, CFG_SHAPE, EPI_GATE, EPI_RES, EPI_STORE, PRE_ADDSILU,
                      PRE_ELU, PRE_LNFOLD, PRE_LNMOD, PRE_NONE, gemm_ref)

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
TOL = 2.0 ** -18
REF_MACS = 2 ** 28  # above this many multiply-adds the reference covers a fixed subset of row tiles

NCFG = len(CFG_NAME)
# the configurations the library admits per weight format (fp32, int8, bf16, split bf16) on a shape every one of them fits
ADMITTED = {
    0: set(range(NCFG)),
    1: {0, 1, 2, 3, 7, 10, 11},
    2: {1, 2, 3, 7, 10, 11},  # no 8-wave bf16 kernel (b16_cfg in ptts_dispatch.hip)
    3: {1, 2, 3, 4, 5, 6, 7, 10, 11, 13, 14},
}
PRE_SFX = {PRE_NONE: "", PRE_LNFOLD: "+ln", PRE_LNMOD: "+lnmod", PRE_ELU: "+elu", PRE_ADDSILU: "+addsilu"}
WF_SFX = {0: "", 1: "+q8", 2: "+b16", 3: "+split"}

# worst scaled error and case count per (format, cfg); production-shape coverage per (format, cfg)
STATS = defaultdict(lambda: [0.0, 0])
PROD_SEEN = set()


def cdiv(a, b):
    return (a + b - 1) // b


def label_of(cfg, pre, wfmt, NT, MT):
    s = CFG_SHAPE[cfg]
    if s[2] == 0:
        threads = cdiv(NT, s[0]) * cdiv(MT, s[1]) * 256
    else:
        threads = cdiv(NT, s[0] * s[3]) * cdiv(MT, s[1] * s[4]) * 64 * s[2] * s[3] * s[4]
    return f"{CFG_NAME[cfg]}{PRE_SFX[pre]}{WF_SFX[wfmt]}@{threads}"


def packable(wfmt, C, ntaps, pre):
    """what the engine's packers accept: int8 and bf16 images are for Linear layers (in_features % 64 / % 32), the
    split image needs an even number of k-fragments; only fp32 kernels exist for the other prologues"""
    if wfmt and pre not in (PRE_NONE, PRE_LNFOLD):
        return False
    if wfmt == 1:
        return ntaps == 1 and C % 64 == 0
    if wfmt == 2:
        return ntaps == 1 and C % 32 == 0
    if wfmt == 3:
        return (C // 16 * ntaps) % 2 == 0
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


def make_case(M, N, C, ntaps=1, *, wfmt=0, pre=PRE_NONE, epi=EPI_STORE, act=ACT_NONE, T=16, xstride=1, halo=None,
              halo_mode=0, krot=0, lds_target=0, mean=0.0, bias=True, seed=0):
    """operands of one GEMM on cuda:0 (weights ~ 1/sqrt(K), activations ~ N(mean, 1))"""
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    dev = "cuda:0"

    def rn(*shape, s=1.0, m=0.0):
        return torch.randn(*shape, generator=g, device=dev, dtype=torch.float32) * s + m

    rows = M * xstride if ntaps > 1 else M
    K = C * ntaps
    c = dict(M=M, N=N, C=C, ntaps=ntaps, wfmt=wfmt, pre=pre, epi=epi, act=act, T=T, xstride=xstride,
             halo=(ntaps - xstride if halo is None else halo) if ntaps > 1 else 0, halo_mode=halo_mode if ntaps > 1 else 1,
             krot=krot, lds_target=lds_target)
    c["x"] = rn(rows, C, m=mean)
    c["x_prev"] = rn(rows, C) if ntaps > 1 and halo_mode == 0 else None
    c["w"] = rn(N, C, ntaps, s=1.0 / math.sqrt(K))
    c["bias"] = rn(N, s=0.1) if bias else None
    if pre in (PRE_LNFOLD, PRE_LNMOD):
        c["ln_w"], c["ln_b"] = rn(C, s=0.2, m=1.0), rn(C, s=0.1)
    if pre == PRE_ADDSILU:
        c["prevec"] = rn(C)
    if pre == PRE_LNMOD:
        c["mod_shift"], c["mod_scale"] = rn(M, C, s=0.1), rn(M, C, s=0.1)
    if epi in (EPI_RES, EPI_GATE):
        c["r"] = rn(M, N)
    if epi == EPI_RES:
        c["ls"] = rn(N, s=0.1, m=0.5)
    if epi == EPI_GATE:
        c["g"] = rn(M, N)
    return c


def ref_rows(M, N, K):
    if M * N * K <= REF_MACS:
        return None
    MT = cdiv(M, 16)
    tiles = sorted({0, MT - 1, *range(0, MT, max(1, MT // 14))})
    rows = torch.cat([torch.arange(16 * t, min(16 * t + 16, M)) for t in tiles])
    return rows.to("cuda:0")


def run(eng, case, cfg, *, production=False):
    """runs `case` with configuration `cfg` (-1: the dispatcher's choice); None when no kernel exists for it"""
    ints = {k: case[k] for k in ("T", "xstride", "halo", "halo_mode", "wfmt", "pre", "epi", "act", "krot", "lds_target")}
    ins = {k: case.get(k) for k in ("x_prev", "bias", "ln_w", "ln_b", "prevec", "mod_shift", "mod_scale", "r", "g", "ls")}
    out = eng.debug_gemm(case["x"], case["w"], want_weights=True, cfg=cfg, **ints, **ins)
    if out is None:
        return None
    M, N, C, ntaps, wfmt, pre = case["M"], case["N"], case["C"], case["ntaps"], case["wfmt"], case["pre"]
    used = out["cfg"]
    if cfg >= 0:
        assert used == cfg
    tag = f"wfmt {wfmt} cfg {used} M {M} N {N} C {C} taps {ntaps} pre {pre} epi {case['epi']} act {case['act']}"
    assert out["label"] == label_of(used, pre, wfmt, cdiv(N, 16), cdiv(M, 16)), (tag, out["label"])
    y = out["y"]
    assert torch.isfinite(y).all(), f"{tag}: {int((~torch.isfinite(y)).sum())} non-finite outputs"
    rows = ref_rows(M, N, C * ntaps)
    ref, scale = gemm_ref(case["x"], out["w_eff"], M=M, ntaps=ntaps, T=case["T"], xstride=case["xstride"], halo=case["halo"],
                          halo_mode=case["halo_mode"], x_prev=case.get("x_prev"), wfmt=wfmt, w_lo=out.get("w_eff_lo"),
                          pre=pre, ln_g=case.get("ln_w") if (wfmt == 1 and pre == PRE_LNFOLD) else None,
                          ln_s=out.get("ln_s"), ln_c=out.get("ln_c"), prevec=case.get("prevec"),
                          lnm_w=case.get("ln_w") if pre == PRE_LNMOD else None, lnm_b=case.get("ln_b") if pre == PRE_LNMOD else None,
                          mod_shift=case.get("mod_shift"), mod_scale=case.get("mod_scale"), bias=case.get("bias"),
                          epi=case["epi"], act=case["act"], r=case.get("r"), g=case.get("g"), ls=case.get("ls"), rows=rows)
    yy = y if rows is None else y[rows]
    err = float((yy.double() - ref).abs().max() / scale.max())
    assert err <= TOL, f"{tag}: scaled error {err:.3e} > 2^-18 ({out['label']})"
    # the same request again (cfg -1 may name a configuration cfg_valid does not admit for the shape: the int8 / bf16
    # fall-back to the 2-D tile 3 at a single row tile, correct but mostly padding)
    again = eng.debug_gemm(case["x"], case["w"], cfg=cfg, **ints, **ins)
    assert torch.equal(again["y"], y), f"{tag}: two launches differ"
    st = STATS[(wfmt, used)]
    st[0], st[1] = max(st[0], err), st[1] + 1
    if production:
        PROD_SEEN.add((wfmt, used))
    return err


def run_all_cfgs(eng, case, production=False):
    ran = [c for c in range(NCFG) if run(eng, case, c, production=production) is not None]
    assert run(eng, case, -1, production=production) is not None, "the dispatcher found no configuration"
    return ran


# ---- admission and unsupported combinations --------------------------------------------------------------------------
@pytest.mark.parametrize("wfmt", [0, 1, 2, 3])
def test_admitted_configurations(eng, wfmt):
    """MT = 8, NT = 4, KF = 32: every configuration of the table fits; the admitted set per format is exactly ADMITTED"""
    case = make_case(128, 64, 512, wfmt=wfmt, seed=1)
    assert set(run_all_cfgs(eng, case)) == ADMITTED[wfmt]


@pytest.mark.parametrize("wfmt", [1, 2, 3])
@pytest.mark.parametrize("pre", [PRE_ELU, PRE_ADDSILU, PRE_LNMOD])
def test_unsupported_prologue(eng, wfmt, pre):
    """int8 / bf16 / split kernels exist for plain and LN-folded operands only: other prologues are refused, never run
    by a kernel that would drop them"""
    case = make_case(64, 64, 128, wfmt=0, pre=pre, seed=2)
    case["wfmt"] = wfmt
    for cfg in [-1, *range(NCFG)]:
        assert run(eng, case, cfg) is None, (wfmt, pre, cfg)


# ---- production shapes ---------------------------------------------------------------------------------------------------
def production_keys():
    """distinct (NT, KF, CF, ntaps, MT, epi, pre, act, wfmt) of the committed tile table, site-specific epilogues excluded"""
    keys = set()
    for line in (REPO / "profiles" / "tune_cache_mi355x.txt").read_text().splitlines():
        f = line.split()
        if len(f) != 14 or not f[0].isdigit():
            continue
        NT, KF, CF, ntaps, MT, epi, pre, act, xstride, halo_mode, yraw, has_r, wfmt, _ = map(int, f)
        if epi <= EPI_GATE:
            keys.add((NT, KF, CF, ntaps, MT, epi, pre, act, wfmt))
    return sorted(keys)


@pytest.mark.parametrize("wfmt", [0, 1, 2, 3])
def test_production_shapes(eng, wfmt):
    """every GEMM shape of the committed tile table with every configuration; the int8 / bf16 / split formats take the
    table's shapes their packers accept"""
    n = 0
    for NT, KF, CF, ntaps, MT, epi, pre, act, kw in production_keys():
        if not packable(wfmt, CF * 16, ntaps, pre) or (wfmt == 0 and kw != 0):
            continue
        case = make_case(MT * 16, NT * 16, CF * 16, ntaps, wfmt=wfmt, pre=pre, epi=epi, act=act, seed=NT * 131 + MT)
        run_all_cfgs(eng, case, production=True)
        n += 1
    assert n > 0


# ---- edge shapes ----------------------------------------------------------------------------------------------------------
def linear_edges():
    out = []
    for M in (1, 15, 17, 130):  # clamped row tiles (mt = MT - 1)
        for N in (16, 200):  # clamped column tiles (nt = NT - 1)
            out.append(dict(M=M, N=N, C=256))
    out += [dict(M=32, N=64, C=32), dict(M=32, N=64, C=96)]  # KF = 2, 6 < WK: waves with empty K ranges
    out += [dict(M=16, N=48, C=16 * kf) for kf in (34, 66, 68, 130)]  # KF just off multiples of WK * U: tail loops
    out += [dict(M=64, N=1024, C=1024), dict(M=64, N=256, C=4096)]  # the LM's K
    out += [dict(M=16, N=256, C=4096, krot=1), dict(M=48, N=128, C=1024, krot=1)]  # rotated K chunks, several per wave
    out += [dict(M=1008, N=64, C=64), dict(M=1024, N=64, C=64)]  # either side of swz_for (MT >= 64)
    out += [dict(M=256, N=128, C=256, lds_target=44 * 1024)]  # LDS-staged tiles under the occupancy cap
    return out


@pytest.mark.parametrize("wfmt", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", linear_edges(), ids=lambda s: "-".join(f"{k}{v}" for k, v in s.items()))
def test_linear_edges(eng, wfmt, shape):
    if not packable(wfmt, shape["C"], 1, PRE_NONE):
        pytest.skip("no weight image of this format for this in_features")
    run_all_cfgs(eng, make_case(**shape, wfmt=wfmt, seed=shape["M"] + shape["C"]))


CONVS = [(3, 16, 1, 1), (7, 32, 3, 1), (3, 32, 3, 1), (7, 16, 1, 1), (4, 16, 2, 2)]  # (ntaps, T, B, xstride)


@pytest.mark.parametrize("wfmt", [0, 3])
@pytest.mark.parametrize("halo_mode", [0, 1, 2])
@pytest.mark.parametrize("conv", CONVS, ids=lambda c: f"k{c[0]}-T{c[1]}-B{c[2]}-s{c[3]}")
def test_conv_edges(eng, wfmt, halo_mode, conv):
    ntaps, T, B, xs = conv
    case = make_case(B * T, 64, 64, ntaps, wfmt=wfmt, T=T, xstride=xs, halo_mode=halo_mode, seed=ntaps * 7 + T + B)
    run_all_cfgs(eng, case)


@pytest.mark.parametrize("wfmt", [0, 1, 2, 3])
@pytest.mark.parametrize("mean", [0.0, 3.0])
def test_lnfold(eng, wfmt, mean):
    """mean 3, std 1: the fold (sum x w' - s mu) rs + c cancels most of its two terms"""
    for M, N, C in ((64, 192, 1024), (17, 64, 256)):
        run_all_cfgs(eng, make_case(M, N, C, wfmt=wfmt, pre=PRE_LNFOLD, mean=mean, seed=M + int(mean)))


@pytest.mark.parametrize("pre", [PRE_ELU, PRE_ADDSILU, PRE_LNMOD])
def test_fp32_prologues(eng, pre):
    for M, N, C in ((64, 128, 512), (130, 32, 64)):
        run_all_cfgs(eng, make_case(M, N, C, pre=pre, seed=M + pre))
    if pre == PRE_ELU:  # the codec's transposed conv -> k3 conv with ELU on the operand read
        run_all_cfgs(eng, make_case(48, 64, 64, 3, pre=pre, T=16, halo_mode=0, seed=5))


@pytest.mark.parametrize("wfmt", [0, 1, 2, 3])
@pytest.mark.parametrize("epi,act", [(EPI_STORE, ACT_GELU), (EPI_STORE, ACT_SILU), (EPI_STORE, ACT_ELU),
                                     (EPI_RES, ACT_NONE), (EPI_GATE, ACT_NONE)])
def test_epilogues(eng, wfmt, epi, act):
    run_all_cfgs(eng, make_case(64, 96, 256, wfmt=wfmt, epi=epi, act=act, seed=epi * 4 + act))


def test_zz_error_tables():
    """worst scaled error per (format, configuration), and every admitted pair met on a production shape"""
    if not STATS:
        pytest.skip("no case ran in this session")
    for wfmt, name in ((0, "fp32"), (1, "int8"), (2, "bf16"), (3, "split bf16")):
        print(f"\nweights {name}: worst max|y - ref| / scale per configuration (bound 2^-18 = {TOL:.2e})")
        for cfg in range(NCFG):
            if (wfmt, cfg) in STATS:
                e, n = STATS[(wfmt, cfg)]
                print(f"  {cfg:2d} {CFG_NAME[cfg]:16s} {e:.3e}  ({n} cases)")
    if PROD_SEEN:
        formats = {w for w, _ in PROD_SEEN}
        missing = sorted((w, c) for w in formats for c in ADMITTED[w] if (w, c) not in PROD_SEEN)
        assert not missing, f"admitted (format, cfg) pairs no production shape exercised: {missing}"
