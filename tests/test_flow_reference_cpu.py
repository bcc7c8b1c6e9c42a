"""Pins tests/flow_ref.py and proves that the GPU matrix's bound (tests/test_gpu_flow_matrix.py: 8 E32) discriminates.
No GPU.

1. `flow_head_ref` in float32 agrees with `oracle.np_oracle.FlowLM` (itself tied to the reference project's goldens by
   test_oracle_golden.py) on the same x and noise.
2. Every seeded defect of `flow_ref.MUTANTS` moves the fp64 result by at least 32 E32 on its designated case: 4 times
   the GPU tolerance.  The 32 is a condition that keeps the GPU bound meaningful, not a measurement."""

import numpy as np
import pytest

from flow_ref import MUTANTS, flow_head_e32, flow_head_ref, flow_weights, random_inputs
from oracle import np_oracle as O

GPU_FACTOR = 8            # test_gpu_flow_matrix.FACTOR
MUTANT_FACTOR = 4 * GPU_FACTOR
B = 17
RATIOS = {}


@pytest.mark.parametrize("lsd", [1, 3])
@pytest.mark.parametrize("name", ["F64", "F512"])
def test_float32_reference_is_the_oracle(name, lsd):
    cfg, W = flow_weights(name)
    x, noise = random_inputs(cfg, B, 7)
    lm = O.FlowLM(cfg, W)
    c = O.layer_norm(x, W["flow_lm.out_norm.weight"], W["flow_lm.out_norm.bias"], 1e-5)
    want_eos = O.linear(c, W["flow_lm.out_eos.weight"], W["flow_lm.out_eos.bias"])[:, 0]
    cur = noise.copy()
    for i in range(lsd):  # the flow part of FlowLM.decode_step
        s = np.full((B, 1), i / lsd, np.float32)
        t = np.full((B, 1), (i + 1) / lsd, np.float32)
        cur = (cur + lm.flow_net(c, s, t, cur) / np.float32(lsd)).astype(np.float32)
    lat, eos, ce = flow_head_ref(cfg, W, x, noise, lsd, dtype=np.float32)
    assert lat.dtype == eos.dtype == ce.dtype == np.float32
    assert np.abs(lat - cur).max() <= 1e-5
    assert np.abs(eos - want_eos).max() <= 1e-5
    p = "flow_lm.flow_net."
    cond = O.linear(c, W[p + "cond_embed.weight"], W[p + "cond_embed.bias"])
    if lsd == 1:  # a state without schedules folds silu(t_comb + .) into the buffer
        z = np.zeros((1, 1), np.float32)
        cond = O.silu((lm.time_embed(0, z) + lm.time_embed(1, z + 1)) / np.float32(2) + cond)
    assert np.abs(ce - cond).max() <= 1e-5
    # a scheduled state with no override computes the same latent and keeps the plain cond_embed(c)
    lat_s, _, ce_s = flow_head_ref(cfg, W, x, noise, lsd, row_n=np.zeros(B, int), dtype=np.float32)
    assert np.array_equal(lat_s, lat)
    assert np.abs(ce_s - O.linear(c, W[p + "cond_embed.weight"], W[p + "cond_embed.bias"])).max() <= 1e-5


def test_row_schedules_are_per_row_runs():
    """row m of a scheduled batch = row m of a plain run at its own count; un-overridden rows take the step's"""
    cfg, W = flow_weights("F64")
    x, noise = random_inputs(cfg, 33, 3)
    row_n = np.array([0 if m % 5 == 0 else 1 + m % 4 for m in range(33)])
    lat, eos, _ = flow_head_ref(cfg, W, x, noise, 3, row_n=row_n)
    for n in (1, 2, 3, 4):
        want, want_eos, _ = flow_head_ref(cfg, W, x, noise, n)
        rows = np.where(row_n > 0, row_n, 3) == n
        assert rows.any()
        assert np.abs(lat[rows] - want[rows]).max() <= 1e-12
        assert np.array_equal(eos, want_eos)


def schedule_case(cfg):
    x, noise = random_inputs(cfg, 33, 11)
    return x, noise, 3, np.array([0 if m % 5 == 0 else 1 + m % 4 for m in range(33)])


def plain_case(cfg):
    x, noise = random_inputs(cfg, B, 11)
    return x, noise, 2, None


# mutant -> (weight variant, configs, case, output the defect must move)
DESIGNATED = {
    "a": ("smallvar", ("F64", "F256"), plain_case, "latent"),
    "b": ("smallte", ("F64", "F256"), plain_case, "latent"),
    "c": ("plain", ("F64", "F256", "F512"), plain_case, "latent"),
    "d": ("plain", ("F64", "F256", "F512"), plain_case, "latent"),
    "e": ("plain", ("F64", "F256", "F512"), schedule_case, "latent"),
    "f": ("plain", ("F64", "F256", "F512"), schedule_case, "latent"),
    "g": ("plain", ("F64", "F256", "F512"), plain_case, "latent"),
    "h": ("plain", ("F64", "F256", "F512"), plain_case, "eos_logit"),
}
_REF = {}


def reference(variant, name, case):
    key = (variant, name, case.__name__)
    if key not in _REF:
        cfg, W = flow_weights(name, variant)
        x, noise, lsd, row_n = case(cfg)
        _REF[key] = (cfg, W, x, noise, lsd, row_n) + flow_head_e32(cfg, W, x, noise, lsd, row_n)
    return _REF[key]


def test_every_mutant_is_designated():
    assert sorted(DESIGNATED) == sorted(MUTANTS)


@pytest.mark.parametrize("mutant,name", [(m, n) for m, d in sorted(DESIGNATED.items()) for n in d[1]])
def test_mutant_moves_the_result(mutant, name):
    variant, _, case, output = DESIGNATED[mutant]
    cfg, W, x, noise, lsd, row_n, y64, e32 = reference(variant, name, case)
    got = flow_head_ref(cfg, W, x, noise, lsd, row_n, mutate=mutant)
    k = ("latent", "eos_logit", "ce").index(output)
    moved = float(np.abs(got[k] - y64[k]).max())
    ratio = moved / e32[output]
    RATIOS[(mutant, name)] = (variant, output, e32[output], moved, ratio)
    print(f"mutant {mutant} {name} {variant}: E32 {e32[output]:.2e}, moved {moved:.2e} = {ratio:.3g} x E32")
    assert e32[output] > 0
    assert moved >= MUTANT_FACTOR * e32[output], (moved, e32[output], ratio)


def test_few_row_logit_e32_is_the_worst_of_16_and_still_discriminates():
    """the one exception to E32's definition (flow_ref.flow_head_e32): below 16 rows the logit's E32 also takes the same
    sums in other orders.  It only ever grows, stays a float32 rounding error (within the 1e-5 that ties float32 to the oracle), leaves the other
    outputs and every B >= 16 alone, and mutant h stays >= 32 x above it."""
    for name in ("F64", "F192", "F512"):
        cfg, W = flow_weights(name)
        for seed in range(4):
            x, noise = random_inputs(cfg, 1, seed)
            y64, e32 = flow_head_e32(cfg, W, x, noise, 2)
            plain = dict.fromkeys(("latent", "eos_logit", "ce"), 0.0)
            for onepass in (False, True):
                y32 = flow_head_ref(cfg, W, x, noise, 2, dtype=np.float32, onepass=onepass)
                for k, a, b in zip(plain, y32, y64):
                    plain[k] = max(plain[k], float(np.abs(a.astype(np.float64) - b).max()))
            assert e32["latent"] == plain["latent"] and e32["ce"] == plain["ce"]
            assert plain["eos_logit"] <= e32["eos_logit"] <= 1e-5, (name, seed, e32["eos_logit"])
            moved = abs(flow_head_ref(cfg, W, x, noise, 2, mutate="h")[1][0] - y64[1][0])
            assert moved >= MUTANT_FACTOR * e32["eos_logit"], (name, seed, moved, e32["eos_logit"])
    cfg, W = flow_weights("F64")
    x, noise = random_inputs(cfg, 16, 0)
    y64, e32 = flow_head_e32(cfg, W, x, noise, 2)
    y32 = [flow_head_ref(cfg, W, x, noise, 2, dtype=np.float32, onepass=o)[1] for o in (False, True)]
    assert e32["eos_logit"] == max(float(np.abs(a.astype(np.float64) - y64[1]).max()) for a in y32)


def test_zz_mutation_table():
    print(f"\nseeded defects against the fp64 reference (required: >= {MUTANT_FACTOR} x E32)")
    for (m, name), (variant, output, e, moved, ratio) in sorted(RATIOS.items()):
        print(f"  {m} {name:5s} {variant:9s} {output:9s} E32 {e:.2e}  moved {moved:.2e}  = {ratio:9.3g} x E32   {MUTANTS[m]}")
