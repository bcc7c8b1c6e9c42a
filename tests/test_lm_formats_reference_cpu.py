"""Pins the weight-format side of tests/lm_ref.py (`fmt` in "q8a", "q8f", "q8", "b16") and proves that the bound of the GPU
matrix of the reduced formats (tests/test_gpu_lm_formats.py: 8 E32 + F, elementwise) discriminates.  No GPU.

a. Weight rules: the int8 image is `oracle.np_oracle.quantize_dequantize_int8` to the last float32 bit once q * scale is
   rounded to float32 (the sign of a zero aside: the oracle's float rint keeps it, an int8 q has none); the bf16 images
   are `bf16_round` of the stated products, the fold vectors the stated sums; the fp64 bf16 rounding of the reference
   agrees with `bf16_round` on float32 inputs and names the right neighbour and midpoint.
b. Every seeded defect of `lm_ref.MUTANTS`, under each of the four formats, moves at least one judged output ELEMENT of at
   least one case of the reduced-format matrix by >= 4 times the bound that element gets: 32 E32 under q8*, 4 (8 E32 + F)
   under b16.  This is what keeps the flip allowance F from hiding a defect.  A condition on the cases, not a measurement.
c. The flip machinery against a float32 evaluation that rounds its own intermediates (what a kernel does):
   - the plain float32 evaluation (two-pass variance) stays within E32 + F elementwise on every judged call, factor 1, and
     leaves E32 alone on most calls (it does flip elements, and a flip is worth thousands of E32);
   - for both float32 evaluations of E32, the fp64 pass forced to the roundings the float32 pass made differs from the
     master by <= F elementwise: the machinery's own claim, free of float32 noise;
   - the one-pass evaluation stays within N + F, N = the larger of E32 and its own float32 noise max|y32 - y64'| measured
     against the fp64 pass forced to ITS roundings.  E32 is the worst noise under the master's roundings over an output's
     few hundred numbers; the noise under other roundings is of that size, not below it (where one ambiguous element of
     5e-4 flips in V0 of a decode step, 4.2e-7 against an E32 of 3.1e-7), so E32 + F with factor 1 does not bound it;
   - with the flip pass read literally (only the element moved, every later rounding kept: lm_judge(cascade=False)) the
     plain float32 evaluation is NOT within E32 + F: what follows a flipped operand rounds differently too, and those
     later flips are worth more than the first.  Hence F's passes round again downstream.
d. Per case: |A|, the shares of elements under 8 E32 + F, with F = 0 and under the late rule, and the reference's time; F by
   position on prefill (3, 33), and that restricting the flip passes to the first positions is exact for them.

The four calls whose flip passes do not fit a test (lm_ref.JUDGE_ROWS) take 4 to 6 s of reference work on 8 CPU cores, the
en100m decode B = 1 case 2.7 s for its three steps (|A| = 2395), the en100m prefill 0.7 s (|A| = 23386, no flip pass)."""

import time

import numpy as np
import pytest

from lm_ref import (FACTOR, FORMATS, MUTANTS, RefDriver, Rounding, b16_image, bf16_rne64, bf16_rne64_fast, evaluate,
                    find_case, format_cases, format_weights, judge_args, lm_judge, lm_weights, q8_image)
from oracle import np_oracle as O

MUTANT_FACTOR = 4          # times the bound of the GPU matrix
RATIOS = {}                # (fmt, mutant, family) -> best ratio over the family's cases
REPORT = {}                # (fmt, case) -> [|A|, elements, under 8 E32 + F, of them with F = 0, under the late rule, seconds]
_TRUE = {}


# ------------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize("name", ["tiny", "en100m"])
def test_weight_images_follow_their_rule(name):
    cfg, W = lm_weights(name)
    L = cfg.flow_lm.transformer.num_layers
    P8 = format_weights(W, L, "q8", np.float64)
    P16 = format_weights(W, L, "b16", np.float64)
    for l in range(L):
        p = f"flow_lm.transformer.layers.{l}."
        for lin in ("self_attn.in_proj", "self_attn.out_proj", "linear1", "linear2"):
            w = np.asarray(W[p + lin + ".weight"], np.float32)
            q, scale = q8_image(w)
            assert np.array_equal(q, np.rint(q)) and np.abs(q).max() == 127 and scale.dtype == np.float32
            assert np.array_equal(P8[p + lin + ".weight"], q.astype(np.float64) * scale.astype(np.float64))
            # to the last bit; the oracle's float rint keeps the sign of a weight that rounds to 0, the int8 image has no -0
            assert np.array_equal(P8[p + lin + ".weight"].astype(np.float32).view(np.uint32),
                                  (O.quantize_dequantize_int8(w) + np.float32(0.0)).view(np.uint32)), (l, lin)
        for lin, norm in (("self_attn.in_proj", "norm1"), ("linear1", "norm2")):
            w = np.asarray(W[p + lin + ".weight"], np.float32)
            g, beta = np.asarray(W[p + norm + ".weight"], np.float32), np.asarray(W[p + norm + ".bias"], np.float32)
            img = O.bf16_round((w * g[None, :]).astype(np.float32))
            assert np.array_equal(P16[p + lin + ".weight"], img.astype(np.float64))
            assert np.array_equal(P16[p + lin + ".s"], img.astype(np.float64).sum(axis=1))
            assert np.array_equal(P16[p + lin + ".c"], w.astype(np.float64) @ beta.astype(np.float64))
        for lin in ("self_attn.out_proj", "linear2"):
            w = np.asarray(W[p + lin + ".weight"], np.float32)
            assert np.array_equal(P16[p + lin + ".weight"], O.bf16_round(w).astype(np.float64))
            assert np.array_equal(b16_image(w), O.bf16_round(w))
    for fmt, touched in (("q8a", ("self_attn.in_proj", "self_attn.out_proj")), ("q8f", ("linear1", "linear2"))):
        P = format_weights(W, L, fmt, np.float64)
        assert sorted(P) == sorted(f"flow_lm.transformer.layers.{l}.{lin}.weight" for l in range(L) for lin in touched)
        assert all(np.array_equal(P[k], P8[k]) for k in P)


def test_zero_row_and_clipping_of_the_int8_image():
    w = np.zeros((3, 64), np.float32)
    w[1, :] = np.linspace(-1, 1, 64)
    w[2, 5] = -3.0
    q, scale = q8_image(w)
    assert scale[0, 0] == 1 and (q[0] == 0).all() and q[1, 0] == -127 and q[1, -1] == 127 and q[2, 5] == -127


def test_fp64_bf16_rounding():
    rng = np.random.default_rng(0)
    v32 = np.concatenate([(rng.standard_normal(4096) * s).astype(np.float32) for s in (1e-3, 1.0, 50.0)] + [np.zeros(1, np.float32)])
    chosen, other, dist = bf16_rne64(v32.astype(np.float64))
    assert np.array_equal(chosen, O.bf16_round(v32).astype(np.float64)) and np.array_equal(chosen, bf16_rne64_fast(v32.astype(np.float64)))
    # both neighbours are bf16 numbers, the value lies between them, the midpoint is where the distance says
    for a in (chosen, other):
        assert np.array_equal(a, O.bf16_round(a.astype(np.float32)).astype(np.float64))
    v = v32.astype(np.float64)
    assert (np.minimum(chosen, other) <= v).all() and (v <= np.maximum(chosen, other)).all()
    assert np.allclose(np.abs(v - (chosen + other) / 2), dist, rtol=0, atol=1e-18)
    assert (np.abs(v - chosen) <= np.abs(v - other)).all()
    # ties go to the even mantissa: 1 + 2^-8 is the midpoint of 1 and 1 + 2^-7, 1 + 3 * 2^-8 that of 1 + 2^-7 and 1 + 2^-6
    c, o, d = bf16_rne64(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -40]))
    assert list(c) == [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7] and list(o) == [1 + 2.0 ** -7, 1 + 2.0 ** -7, 1.0]
    assert d[0] == 0 and d[1] == 0 and d[2] == 2.0 ** -40


def test_reference_b16_in_float32_is_the_oracles_rounding_model():
    """LMRef(fmt="b16") in float32 against `oracle.np_oracle.FlowLMBF16` (the CPU statement of where the build rounds) on a
    prefill: both are float32 evaluations that round their own intermediates, so they agree up to summation order and the
    flips that follows; layer 0's K and V, which have no rounded intermediate upstream, agree to a few float32 ulps"""
    cfg, W = lm_weights("tiny")
    rng = np.random.default_rng(5)
    B, T, cap = 2, 11, 16
    lm = O.FlowLMBF16(cfg, W)
    emb = (rng.standard_normal((B, T, lm.D)) * 0.5).astype(np.float32)
    ost = lm.init_state(B, cap)
    lm.backbone(ost, emb, np.zeros((B, 0, lm.ldim), np.float32))
    empty = dict(kv=[np.zeros((2, B, cap, lm.H, 64), np.float32) for _ in range(lm.L)], off=np.zeros(B, np.int64))
    op = ("prefill", emb, None)
    _, ref32 = evaluate(cfg, W, empty, op, np.float32, onepass=True, fmt="b16")
    J = lm_judge(cfg, W, empty, op, "b16", flips=False)
    for j, kv in enumerate("KV"):
        err = float(np.abs(ref32.kv[0][j][:, :T].astype(np.float64) - ost[0]["cache"][j][:, :T]).max())
        print(f"  layer 0 {kv}: |ref32 - oracle| {err:.3e} = {err / J.e32[kv + '0']:.2f} x E32")
        assert err <= 4 * J.e32[kv + "0"]
    last = float(np.abs(ref32.kv[lm.L - 1][1][:, :T].astype(np.float64) - ost[lm.L - 1]["cache"][1][:, :T]).max())
    print(f"  layer {lm.L - 1} V: |ref32 - oracle| {last:.3e} (flips included)")
    assert last < 0.1


# ------------------------------------------------------------------------------------------------ b
def true_chain(fmt, family, cid):
    """the case on the unmutated reference: [(op, outputs, Judged)] of its judged calls, and the report line of the case"""
    key = (fmt, family, cid)
    if key not in _TRUE:
        _, name, fn, args = find_case(family, cid)
        d = RefDriver(name, fmt=fmt)
        fn(d, *args)
        out, t0, nA, n, judged, zero, late = [], time.perf_counter(), 0, 0, 0, 0, 0
        for op, snap, res, off in d.calls:
            J = lm_judge(d.cfg, d.W, snap, op, fmt, **judge_args(fmt, family, cid))
            y, y64 = res.outputs(), J.res64.outputs()
            assert all(np.array_equal(y[k], y64[k]) for k in y)  # the chain's call IS the call judged on its operands
            assert list(J.ref64.off) == list(off)
            out.append((op, y, J))
            nA += J.nA
            for k in y:
                n += y[k].size
                if k in J.outputs:
                    judged += int(np.isfinite(J.F[k]).sum())
                    zero += int((J.F[k] == 0).sum())
                    late += int(J.late[k][0].sum()) if k in J.late else 0
        REPORT[(fmt, f"{family}:{cid}")] = [nA, n, judged, zero, late, time.perf_counter() - t0]
        _TRUE[key] = out
    return _TRUE[key]


def mutant_ratio(fmt, mutant, family, cid):
    """worst moved / bound over the judged elements of the first judged call whose outputs the defect moves (0: none)"""
    _, name, fn, args = find_case(family, cid)
    d = RefDriver(name, mutate=mutant, fmt=fmt)
    fn(d, *args)
    truth = true_chain(fmt, family, cid)
    assert len(d.calls) == len(truth)
    for (_, _, res, _), (_, y, J) in zip(d.calls, truth):
        ym = res.outputs()
        if any(np.abs(ym[k] - y[k]).max() > 0 for k in y):
            return max(float((np.abs(ym[k] - y[k]) / J.bound(k)).max()) for k in J.outputs)
    return 0.0


TINY = format_cases("tiny", "q8")
FAMILIES = sorted({f for f, _ in TINY})


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_mutants_on_family(fmt, family):
    for mutant in MUTANTS:
        RATIOS[(fmt, mutant, family)] = max(mutant_ratio(fmt, mutant, f, cid) for f, cid in TINY if f == family)
        print(f"  {fmt:4s} {mutant:11s} {family:9s} {RATIOS[(fmt, mutant, family)]:12.4g} x bound")


@pytest.mark.parametrize("fmt", FORMATS)
def test_zz_every_mutant_moves_a_judged_element(fmt):
    """the mutant x case-family table of one format; every defect reaches 4 x the bound in at least one family"""
    assert sorted({m for f, m, _ in RATIOS if f == fmt}) == sorted(MUTANTS)
    assert sorted({fam for f, _, fam in RATIOS if f == fmt}) == FAMILIES
    print(f"\n{fmt}: seeded defects, worst moved / bound ({FACTOR} E32" + (" + F" if fmt == "b16" else "")
          + f") over the elements of the first call moved (required: >= {MUTANT_FACTOR} in a family)")
    print(f"  {'mutant':11s}" + "".join(f" {f:>10s}" for f in FAMILIES))
    for m in MUTANTS:
        print(f"  {m:11s}" + "".join(f" {RATIOS[(fmt, m, f)]:10.3g}" for f in FAMILIES) + f"   {MUTANTS[m]}")
    escaped = {m: max(RATIOS[(fmt, m, f)] for f in FAMILIES) for m in MUTANTS}
    escaped = {m: round(v, 3) for m, v in escaped.items() if v < MUTANT_FACTOR}
    assert not escaped, escaped


# ------------------------------------------------------------------------------------------------ c
_SELF = []


def selfcheck():
    """[(case, call, one-pass?, output, worst |y32 - y64| / (E32 + F), any element beyond E32?, worst |y64' - y64| / F,
    worst |y32 - y64| / (max(E32, N) + F))] over the judged calls of the tiny matrix and the elements F was worked out for:
    y32 a float32 evaluation that rounds its own intermediates, y64' the fp64 evaluation forced to the roundings y32 made,
    N = max|y32 - y64'| the float32 noise of y32"""
    if _SELF:
        return _SELF
    for family, cid in TINY:
        _, name, fn, args = find_case(family, cid)
        cfg, W = lm_weights(name)
        d = RefDriver(name, fmt="b16")
        fn(d, *args)
        for i, ((op, snap, _, _), (_, y64, J)) in enumerate(zip(d.calls, true_chain("b16", family, cid))):
            for onepass in (False, True):
                R = Rounding(record=True)
                y32 = evaluate(cfg, W, snap, op, np.float32, onepass, fmt="b16", R=R)[0].outputs()
                y64f = evaluate(cfg, W, snap, op, fmt="b16", R=Rounding(forced=R.chosen))[0].outputs()
                for k in J.outputs:
                    ok = np.isfinite(J.F[k])
                    err = np.abs(y32[k].astype(np.float64) - y64[k])[ok]
                    moved = np.abs(y64f[k] - y64[k])[ok]
                    noise = max(J.e32[k], float(np.abs(y32[k].astype(np.float64) - y64f[k])[ok].max()))
                    F = J.F[k][ok]
                    with np.errstate(divide="ignore", invalid="ignore"):
                        rounding = float(np.where(moved > 0, moved / F, 0.0).max())
                    _SELF.append((f"{family}:{cid}", i, onepass, k, float((err / (J.e32[k] + F)).max()), bool((err > J.e32[k]).any()),
                                  rounding, float((err / (noise + F)).max())))
    return _SELF


def test_float32_evaluation_stays_within_e32_plus_f():
    """the float32 evaluation of the b16 model (`evaluate(..., np.float32, fmt="b16")`, which rounds its own intermediates)
    against the master: within E32 + F on every judged element of every judged call of the tiny matrix (factor 1), and
    not within E32 alone on at least one call"""
    rows = [r for r in selfcheck() if not r[2]]
    beyond = sorted({r[:2] for r in rows if r[5]})
    print(f"  {len({r[:2] for r in rows})} judged calls, {len(beyond)} with an element beyond E32 alone (a flip happened)")
    over = [r for r in rows if r[4] > 1.0]
    for r in over:
        print(f"  beyond E32 + F: {r[0]} call {r[1]} {r[3]}: {r[4]:.3f}")
    print(f"  worst |y32 - y64| / (E32 + F) = {max(r[4] for r in rows):.3f}")
    assert beyond, "no call of the matrix has a flip in its float32 evaluation: pick a seed that has one"
    assert not over, [(r[0], r[1], r[3], round(r[4], 3)) for r in over]


def test_one_pass_evaluation_stays_within_its_noise_plus_f():
    """the one-pass-variance float32 evaluation: within max(E32, its own float32 noise under its own roundings) + F,
    elementwise, factor 1 (module docstring, c)"""
    rows = [r for r in selfcheck() if r[2]]
    over = [r for r in rows if r[7] > 1.0]
    print(f"  worst |y32 - y64| / (max(E32, N) + F) = {max(r[7] for r in rows):.3f}; against E32 + F: {max(r[4] for r in rows):.3f}")
    assert not over, [(r[0], r[1], r[3], round(r[7], 3)) for r in over]


def test_rounding_differences_stay_within_f():
    """the flip machinery's own claim, for both float32 evaluations of E32: the fp64 evaluation forced to the roundings the
    float32 evaluation made differs from the master by at most F, elementwise (no float32 noise on either side)"""
    rows = selfcheck()
    over = [r for r in rows if r[6] > 1.0]
    for r in over:
        print(f"  beyond F: {r[0]} call {r[1]} one-pass {r[2]} {r[3]}: {r[6]:.3f}")
    print(f"  worst |y64(float32's roundings) - y64| / F = {max(r[6] for r in rows):.3f}")
    assert not over, [(r[0], r[1], r[3], round(r[6], 3)) for r in over]


def test_literal_flip_pass_does_not_cover_a_float32_evaluation():
    """F from flip passes that keep every later rounding as the master chose it (the flip pass read literally) against the
    plain float32 evaluation.  Where the float32 evaluation flips only small elements the literal F suffices (prefill
    (1, 17): ratio 1.0); where it flips one of ordinary size the later flips that follow are not in it (decode B = 17: 235
    times E32 + F).  The F whose passes round again downstream holds on all of them."""
    worst = {}
    for family, cid in (("prefill", "tiny-B1-T17-plain"), ("decode", "tiny-B17"), ("decode", "tiny-B37")):
        _, name, fn, args = find_case(family, cid)
        cfg, W = lm_weights(name)
        d = RefDriver(name, fmt="b16")
        fn(d, *args)
        w = worst[cid] = {True: 0.0, False: 0.0}
        for (op, snap, _, _), (_, y64, J) in zip(d.calls, true_chain("b16", family, cid)):
            lit = lm_judge(cfg, W, snap, op, "b16", cascade=False)
            assert lit.nA == J.nA and lit.e32 == J.e32
            y32 = evaluate(cfg, W, snap, op, np.float32, fmt="b16")[0].outputs()
            for k in y64:
                err = np.abs(y32[k].astype(np.float64) - y64[k])
                for cascade, judged in ((True, J), (False, lit)):
                    w[cascade] = max(w[cascade], float((err / (judged.e32[k] + judged.F[k])).max()))
        print(f"  {cid}: worst |y32 - y64| / (E32 + F): {w[True]:.3f} with F's passes rounding again downstream, {w[False]:.1f} read literally")
    assert all(w[True] <= 1.0 for w in worst.values())
    assert worst["tiny-B17"][False] > 1.0 and sum(w[False] > 1.0 for w in worst.values()) >= 1


# ------------------------------------------------------------------------------------------------ d
@pytest.mark.parametrize("fmt", ["q8", "b16"])
def test_en100m_reference_work(fmt):
    """the en100m cases of the GPU matrix on the reference alone: the time of the reference's work per case"""
    for family, cid in format_cases("en100m", fmt):
        t0 = time.perf_counter()
        true_chain(fmt, family, cid)
        print(f"  {fmt} {cid}: {time.perf_counter() - t0:.1f} s (with the case's own chain)")


def test_allowance_by_position():
    """F(x) of prefill (3, 33), worked out for every position, grows with every position upstream (measured: median 2.5e-2 at
    position 0, 6.8e-2 at 8, 1.8e-1 at 32 on outputs of order 1, E32 = 9.5e-7); and flip passes for the first 8 positions
    alone give those positions the same F to the bit, with a finite late rule behind them"""
    _, name, fn, args = find_case("prefill", "tiny-B3-T33-plain")
    d = RefDriver(name, fmt="b16")
    fn(d, *args)
    (op, snap, _, _), = d.calls
    full = true_chain("b16", "prefill", "tiny-B3-T33-plain")[0][2]
    part = lm_judge(d.cfg, d.W, snap, op, "b16", rows=8)
    assert not full.late and np.isfinite(full.F["x"]).all()
    Fx, Px = full.F["x"].reshape(3, 33, -1), part.F["x"].reshape(3, 33, -1)
    assert np.array_equal(Fx[:, :8], Px[:, :8]) and np.isinf(Px[:, 8:]).all()  # exact where worked out
    assert sorted(part.late) == ["K1", "V1", "x"] and np.isfinite(part.bound("x")).all()
    assert (part.F["K0"] == 0).all() and (part.F["V0"] == 0).all()
    med = [float(np.median(Fx[:, t])) for t in (0, 8, 32)]
    print(f"  median F(x) at positions 0, 8, 32: {med[0]:.2e} {med[1]:.2e} {med[2]:.2e} (E32 {full.e32['x']:.2e}, |A| {full.nA}); "
          f"late rule 8 x {part.late['x'][1]:.2e}")
    assert med[0] < med[1] < med[2]


def test_zzz_report():
    """|A|, the shares of elements under 8 E32 + F, of those with F = 0, under the late rule, and the reference time, per case"""
    print("\nreference work per case")
    print(f"  {'fmt':4s} {'case':34s} {'|A|':>7s} {'E32 + F':>7s} {'F = 0':>7s} {'late':>7s} {'seconds':>8s}")
    for (fmt, cid), (nA, n, judged, zero, late, sec) in sorted(REPORT.items()):
        print(f"  {fmt:4s} {cid:34s} {nA:7d} {judged / n:7.3f} {zero / max(judged, 1):7.3f} {late / n:7.3f} {sec:8.2f}")
