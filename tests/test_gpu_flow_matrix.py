"""The flow head (everything from the `flow.head` site to the end of a decode step) against the fp64 reference of
tests/flow_ref.py, as ONE operation through the public step, on both of its paths: the single-launch cluster
(csrc/ptts_flow.h) and the per-layer launches.  `-m gpu`.

Per case: a state of capacity 8, 4 prefilled positions, two decode steps with explicit noise (the second feeds the
first latent back, so the cluster's flag epoch is non-zero and x differs).  After each step the transformer output x and
the conditioning buffer `ce` are read back (`debug_read`), the reference is evaluated on that x, and for latent, EOS
logit and ce

    max|gpu - y64| <= FACTOR * E32(case)            FACTOR = 8

with E32 the loss of a plain float32 evaluation of the same formulas on the same case (flow_ref.flow_head_e32); it is
computed here from the reference, never from the kernels.  8: the kernels split K over 8 waves with 4-wide MFMA chains,
another summation order than numpy's; both sides are the worst of B * ldim random-sign float32 errors.  Every seeded
defect of flow_ref.MUTANTS moves the result by >= 32 E32 (tests/test_flow_reference_cpu.py), 4 x this bound.

Every step is judged against its own E32.  One documented exception to E32's definition (flow_ref.flow_head_e32): the
EOS logit has one element per row, so with fewer than 16 rows (here: B = 1) its plain E32 is the rounding error of ONE
number and was met as low as 8.9e-9, far below half an ulp of the float32 logit (|logit| ~ 4.5, ulp 4.8e-7); against it
a GPU error of at most one ulp gave ratios of 9.5 and 25.9 (flow_dim 192), and 2.2e-6 at K = 1024 gave 23.3 (en100m, where
17 rows give E32 2e-6 .. 4e-6).  For that class the logit's E32 also takes float32 evaluations of the same logit with the
d_model sums in 15 other orders, i.e. it is the worst of 16 errors like every other figure; latent, ce and the logits of
B >= 16 use the plain definition.

The kernels that ran are asserted from the profiler's (site, kernel) records, so a silent fall-back to the other path
fails the case instead of passing it there."""

import json
import os
import subprocess
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

from flow_ref import OUTPUTS, flow_head_e32, flow_weights

pytestmark = pytest.mark.gpu

FACTOR = 8
THR = -4.0
FLOW_THREADS = 64 * 9
STATS = {}  # (config, path, variant, output) -> worst err / E32


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


@pytest.fixture(scope="module")
def engines():
    """one engine per (config, variant) for the whole module"""
    from pocket_tts_amd.engine import Engine

    cache = {}

    def get(name, variant="plain"):
        if (name, variant) not in cache:
            cfg, W = flow_weights(name, variant)
            cache[(name, variant)] = (Engine(cfg, W, "cuda:0"), cfg, W)
        return cache[(name, variant)]

    yield get
    for eng, _, _ in cache.values():
        eng.close()


def run_head(eng, B, lsd, seed, reserve=0, row_n=None):
    """-> one dict per decode step: the step's noise, x, ce, latent, logit, EOS flag and profiler records"""
    rng = np.random.default_rng(seed)
    st = eng.new_lm_state(B, 8)
    steps = []
    try:
        if reserve:
            st.reserve_row_lsd(reserve)
            for m, n in enumerate(row_n if row_n is not None else ()):
                if n:
                    st.set_row_lsd(m, int(n))
        eng.lm_prefill(st, dev((rng.standard_normal((B, 4, eng.D)) * 0.3).astype(np.float32)))
        for _ in range(2):
            noise = (rng.standard_normal((B, eng.ldim)) * 0.8).astype(np.float32)
            eng.profile_start()
            try:
                o, lg, fl = eng.lm_decode_step(st, None, dev(noise), lsd, THR)
            finally:
                prof = eng.profile_stop()
            torch.cuda.synchronize()
            steps.append(dict(noise=noise, prof=[(r["site"], r["kernel"]) for r in prof],
                              x=eng.debug_read(st, "x").cpu().numpy(), ce=eng.debug_read(st, "ce").cpu().numpy(),
                              latent=o.cpu().numpy(), eos_logit=lg.cpu().numpy(), flag=fl.cpu().numpy()))
        assert not st.error()
    finally:
        st.close()
    return steps


def pre_of(kernel):
    """prologue / weight-format suffixes of a GEMM label "<cfg>+a+b@threads" """
    return kernel.split("@")[0].split("+")[1:]


def check_path(prof, cluster, lsd, scheduled):
    """the kernels of the head that ran are those of the expected path (fp32 weights everywhere)"""
    at = lambda site: [k for s, k in prof if s == site]  # noqa: E731
    for s, k in prof:
        if s.startswith("flow."):
            assert not {"q8", "b16", "split"} & set(pre_of(k)), (s, k)
    assert [pre_of(k) for k in at("flow.head")] == [["ln"]], prof
    adaln = ["addsilu_row"] if scheduled else [] if lsd == 1 else ["addsilu"]
    assert at("flow.adaln") and all(pre_of(k) == adaln for k in at("flow.adaln")), (adaln, prof)
    if cluster:
        want = "flow_cluster_rowlsd@" if scheduled else "flow_cluster@"
        assert len(at("flow.cluster")) == 1 and at("flow.cluster")[0].startswith(want), prof
        assert not at("flow.final") and not at("flow.res.l0") and not at("flow.input_proj"), prof
    else:
        assert not at("flow.cluster"), prof
        assert at("flow.final") and all(pre_of(k) == (["lnmod_row"] if scheduled else ["lnmod"]) for k in at("flow.final")), prof
        assert at("flow.res.l0") and all(pre_of(k) == ["lnmod"] for k in at("flow.res.l0")), prof
        assert at("flow.input_proj") and at("flow.res.l2"), prof


def compare(steps, cfg, W, lsd, row_ref, key):
    """-> {output: worst err / E32 over the case's steps}, each step judged against its OWN E32 (the reference evaluated on
    that step's x and noise).  Asserts finiteness and each step's EOS flags, records STATS."""
    worst = dict.fromkeys(OUTPUTS, 0.0)
    for k, s in enumerate(steps):
        assert np.isfinite(s["x"]).all()
        y64, e32 = flow_head_e32(cfg, W, s["x"], s["noise"], lsd, row_ref)
        for name, ref in zip(OUTPUTS, y64):
            got = s[name]
            assert got.shape == ref.shape and np.isfinite(got).all(), (name, k)
            assert e32[name] > 0
            err = float(np.abs(got.astype(np.float64) - ref).max())
            worst[name] = max(worst[name], err / e32[name])
            print(f"  step {k} {name:9s} err {err:.3e}  E32 {e32[name]:.3e}  ratio {err / e32[name]:.2f}")
        sure = np.abs(y64[1] - THR) > FACTOR * e32["eos_logit"]
        assert np.array_equal(s["flag"][sure] != 0, (y64[1] > THR)[sure]), k
    for name in OUTPUTS:
        STATS[key + (name,)] = max(STATS.get(key + (name,), 0.0), worst[name])
    return worst


def seed_of(*case):
    return zlib.crc32(repr(case).encode())


def run_case(engines, name, B, lsd, cluster, variant="plain", reserve=0, row_n=None, max_cus=None):
    eng, cfg, W = engines(name, variant)
    scheduled = reserve > 0
    eng.set_option("flow_cluster", cluster)
    if max_cus:
        eng.set_option("flow_max_cus", max_cus)
    try:
        steps = run_head(eng, B, lsd, seed_of(name, B, lsd, variant, reserve, max_cus), reserve, row_n)
    finally:
        eng.set_option("flow_cluster", 1)
        if max_cus:
            eng.set_option("flow_max_cus", 128)  # the engine's default (opt_flow_max_cus in csrc/ptts_host.h)
    expect_cluster = bool(cluster) and name != "F320"  # kpw 3: no cluster kernel, the per-layer launches must show
    for s in steps:
        check_path(s["prof"], expect_cluster, lsd, scheduled)
    row_ref = None if not scheduled else np.zeros(B, int) if row_n is None else np.asarray(row_n)
    path = ("cluster" if expect_cluster else "layers") + ("+rows" if scheduled else "")
    worst = compare(steps, cfg, W, lsd, row_ref, (name, path, variant))
    assert all(v <= FACTOR for v in worst.values()), worst
    return steps


CLUSTER = pytest.mark.parametrize("cluster", [1, 0])


# partial last tile, the clamped duplicate tile, one or many clusters; F192: worker waves 6 and 7 idle
@CLUSTER
@pytest.mark.parametrize("lsd", [1, 2, 4])
@pytest.mark.parametrize("B", [1, 16, 17, 33])
@pytest.mark.parametrize("name", ["F64", "F192", "F256"])
def test_shapes(engines, name, B, lsd, cluster):
    run_case(engines, name, B, lsd, cluster)


# B = 100: 7 row groups on 4 resident clusters, the row-group loop at the real size
@CLUSTER
@pytest.mark.parametrize("lsd", [1, 2])
@pytest.mark.parametrize("B", [1, 17, 100])
def test_shapes_en100m(engines, B, lsd, cluster):
    steps = run_case(engines, "F512", B, lsd, cluster)
    if cluster:
        ncl = min(-(-B // 16), 4)
        assert [k for s, k in steps[0]["prof"] if s == "flow.cluster"] == [f"flow_cluster@{ncl * 32 * FLOW_THREADS}"]


@CLUSTER
def test_row_group_loop_small(engines, cluster):
    """8 workgroups = 2 resident clusters of F64 for 7 row groups: uneven groups per cluster"""
    steps = run_case(engines, "F64", 100, 2, cluster, max_cus=8)
    if cluster:
        assert [k for s, k in steps[0]["prof"] if s == "flow.cluster"] == [f"flow_cluster@{2 * 4 * FLOW_THREADS}"]


@CLUSTER
def test_no_cluster_kernel_falls_back_to_the_layers(engines, cluster):
    run_case(engines, "F320", 17, 2, cluster)


SCHEDULED = pytest.mark.parametrize("name", ["F64", "F256", "F512"])


@CLUSTER
@SCHEDULED
def test_row_schedules_mixed_within_a_tile(engines, name, cluster):
    run_case(engines, name, 33, 3, cluster, reserve=4, row_n=[0 if m % 5 == 0 else 1 + m % 4 for m in range(33)])


@CLUSTER
@SCHEDULED
def test_row_schedules_group_finished_early(engines, name, cluster):
    """rows 0..15 stop after one Euler step (their group's later phases never run), 16..31 run four, row 32 the step's two"""
    run_case(engines, name, 33, 2, cluster, reserve=4, row_n=[1] * 16 + [4] * 16 + [0])


@CLUSTER
@SCHEDULED
def test_single_step_on_a_scheduled_state(engines, name, cluster):
    """lsd_steps 1 with reserved schedules: silu(t_comb + .) is NOT folded into the head GEMM, ce stays cond_embed(c)"""
    run_case(engines, name, 33, 1, cluster, reserve=4)


# smallvar / smallte: the LayerNorm / RMSNorm eps decides the result; bigmean: cancellation in the one-pass variance
@CLUSTER
@pytest.mark.parametrize("variant", ["smallvar", "smallte", "bigmean"])
@pytest.mark.parametrize("name", ["F64", "F256"])
def test_variants(engines, name, variant, cluster):
    run_case(engines, name, 17, 2, cluster, variant=variant)


def test_two_row_tiles_per_cluster_in_a_fresh_process(tmp_path):
    """PTTS_FLOW_RT=2 is read once per process: a child runs F256 at B = 33 (2 row groups, the second half filled) and
    F64 at B = 17 and writes its err / E32 ratios; the same bound holds"""
    out = tmp_path / "rt2.json"
    r = subprocess.run([sys.executable, str(Path(__file__).with_name("_flow_rt2_worker.py")), str(out)],
                       env={**os.environ, "PTTS_FLOW_RT": "2"}, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    res = json.loads(out.read_text())
    assert sorted(res) == ["F256", "F64"]
    # row groups of 32 rows: B = 33 -> 2 clusters of 16 workgroups (RT 1: 3), B = 17 -> 1 cluster of 4 (RT 1: 2)
    assert res["F256"]["cluster_kernel"] == f"flow_cluster@{2 * 16 * FLOW_THREADS}"
    assert res["F64"]["cluster_kernel"] == f"flow_cluster@{1 * 4 * FLOW_THREADS}"
    for name, r in res.items():
        for output in OUTPUTS:
            STATS[(name, "cluster RT=2", "plain", output)] = r["ratio"][output]
            assert r["ratio"][output] <= FACTOR, (name, r["ratio"])


def test_zz_error_table():
    """worst err / E32 per (config, path, variant, output) of this session"""
    print(f"\nflow head: worst max|gpu - y64| / E32 (bound {FACTOR})")
    print(f"  {'config':6s} {'path':13s} {'variant':9s}" + "".join(f" {o:>10s}" for o in OUTPUTS))
    for key in sorted({k[:3] for k in STATS}):
        print(f"  {key[0]:6s} {key[1]:13s} {key[2]:9s}" + "".join(f" {STATS.get(key + (o,), float('nan')):10.2f}" for o in OUTPUTS))
    assert all(v <= FACTOR for v in STATS.values())
