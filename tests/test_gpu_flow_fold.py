"""The flow fold (`ptts_lm_state_set_flow_fold`, csrc/ptts_flow.h: flow_cluster_mod_kernel): the flow cluster computes the
AdaLN modulations inside its hand-off waits and the `flow.adaln` launch goes.  `-m gpu`.

The cases, the fp64 reference, E32 and FACTOR = 8 are those of tests/test_gpu_flow_matrix.py (imported, not copied): every
output of every step within FACTOR x E32 of the reference evaluated on that step's own x and noise, EOS flags exact where
the reference is sure.  On top of that: the launches that ran (one `flow.head`, no `flow.adaln`, one `flow.cluster` with
the label `flow_cluster_mod@<threads>`), the state's error word, the latents against the same steps with the switch off
(test_gpu_parity.ATOL: another summation order of the same fp32 products), the fall-backs, bitwise repeatability, batch
invariance, repeatability under load and the refusals.  No case provokes the spin limit."""

import numpy as np
import pytest
import torch

from test_gpu_flow_matrix import FACTOR, FLOW_THREADS, THR, compare, dev, engines, seed_of  # noqa: F401  (engines: fixture)
from test_gpu_parity import ATOL, _maxerr

pytestmark = pytest.mark.gpu


def run_head(eng, B, lsd, seed, fold, reserve=0, n_steps=2, busy=None):
    """the `run_head` of test_gpu_flow_matrix.py with the state's fold switch: one dict per decode step"""
    rng = np.random.default_rng(seed)
    st = eng.new_lm_state(B, 4 + n_steps + 2)
    steps = []
    try:
        if reserve:
            st.reserve_row_lsd(reserve)
        st.set_flow_fold(fold)
        eng.lm_prefill(st, dev((rng.standard_normal((B, 4, eng.D)) * 0.3).astype(np.float32)))
        for _ in range(n_steps):
            noise = (rng.standard_normal((B, eng.ldim)) * 0.8).astype(np.float32)
            if busy is not None:
                busy()
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


def at(prof, site):
    return [k for s, k in prof if s == site]


def check_folded(prof, wgs=None):
    assert len(at(prof, "flow.head")) == 1 and not at(prof, "flow.adaln"), prof
    cl = at(prof, "flow.cluster")
    assert len(cl) == 1 and cl[0].startswith("flow_cluster_mod@"), prof
    if wgs is not None:
        assert cl[0] == f"flow_cluster_mod@{wgs * FLOW_THREADS}", prof
    assert not at(prof, "flow.final") and not at(prof, "flow.res.l0") and not at(prof, "flow.input_proj"), prof


def run_case(engines, name, B, lsd, max_cus=None, wgs=None):
    eng, cfg, W = engines(name)
    if max_cus:
        eng.set_option("flow_max_cus", max_cus)
    try:
        seed = seed_of("fold", name, B, lsd, max_cus)
        on = run_head(eng, B, lsd, seed, True)
        off = run_head(eng, B, lsd, seed, False)
    finally:
        if max_cus:
            eng.set_option("flow_max_cus", 128)  # the engine's default
    for s, s0 in zip(on, off):
        check_folded(s["prof"], wgs)
        assert at(s0["prof"], "flow.adaln") and at(s0["prof"], "flow.cluster")[0].startswith("flow_cluster@"), s0["prof"]
        assert np.array_equal(s["noise"], s0["noise"])
        d = _maxerr(s["latent"], s0["latent"])
        print(f"  fold on vs off: max|latent diff| {d:.3e} (ATOL {ATOL:.1e})")
        assert d < ATOL
    worst = compare(on, cfg, W, lsd, None, (name, "cluster+fold", "plain"))
    assert all(v <= FACTOR for v in worst.values()), worst
    return on


# partial last tile, the clamped duplicate tile, one or many clusters; F64: KPW 1, F192: KPW 2 with worker waves 6 and 7
# idle, F256: KPW 2
@pytest.mark.parametrize("lsd", [1, 2, 4])
@pytest.mark.parametrize("B", [1, 16, 17, 33])
@pytest.mark.parametrize("name", ["F64", "F192", "F256"])
def test_shapes(engines, name, B, lsd):
    run_case(engines, name, B, lsd)


# KPW 4; B = 100: 7 row groups on 4 resident clusters
@pytest.mark.parametrize("lsd", [1, 2])
@pytest.mark.parametrize("B", [1, 17, 100])
def test_shapes_en100m(engines, B, lsd):
    run_case(engines, "F512", B, lsd, wgs=min(-(-B // 16), 4) * 32)


def test_row_group_loop_small(engines):
    """8 workgroups = 2 resident clusters of F64 for 7 row groups: the modulation operand is reloaded per group"""
    run_case(engines, "F64", 100, 2, max_cus=8, wgs=2 * 4)


def test_kpw3_takes_todays_launches(engines):
    """F320 has no cluster kernel: the switch changes nothing, the per-layer launches with `flow.adaln` run"""
    eng, cfg, W = engines("F320")
    steps = run_head(eng, 17, 2, seed_of("fold", "F320"), True)
    for s in steps:
        assert at(s["prof"], "flow.adaln") and not at(s["prof"], "flow.cluster") and at(s["prof"], "flow.final"), s["prof"]
    worst = compare(steps, cfg, W, 2, None, ("F320", "layers+fold", "plain"))
    assert all(v <= FACTOR for v in worst.values()), worst


def test_row_schedules_take_todays_launches(engines):
    """a state with a per-row LSD capacity: `flow.adaln` and the scheduled cluster kernel, as without the switch"""
    eng, cfg, W = engines("F256")
    steps = run_head(eng, 33, 2, seed_of("fold", "rows"), True, reserve=4)
    for s in steps:
        assert at(s["prof"], "flow.adaln"), s["prof"]
        assert [k.split("@")[0] for k in at(s["prof"], "flow.cluster")] == ["flow_cluster_rowlsd"], s["prof"]
    worst = compare(steps, cfg, W, 2, np.zeros(33, int), ("F256", "cluster+rows+fold", "plain"))
    assert all(v <= FACTOR for v in worst.values()), worst


@pytest.mark.parametrize("name,lsd", [("F64", 2), ("F512", 1)])
def test_repeatable_and_batch_invariant(engines, name, lsd):
    """two runs of the same seeded steps are bitwise equal; a row's latent does not depend on the batch it runs in (rows
    0..16 of B = 33 against B = 17 on the same inputs), where the GEMMs in front of the cluster use the same tiles"""
    eng, _, _ = engines(name)

    def run(B):
        rng = np.random.default_rng(seed_of("inv", name))
        emb = (rng.standard_normal((33, 4, eng.D)) * 0.3).astype(np.float32)[:B]
        noise = (rng.standard_normal((2, 33, eng.ldim)) * 0.8).astype(np.float32)[:, :B]
        st = eng.new_lm_state(B, 8)
        try:
            st.set_flow_fold(True)
            eng.lm_prefill(st, dev(emb))
            out = []
            for k in range(2):
                eng.profile_start()
                try:
                    o, _, _ = eng.lm_decode_step(st, None, dev(noise[k]), lsd, THR)
                finally:
                    prof = eng.profile_stop()
                check_folded([(r["site"], r["kernel"]) for r in prof])
                out.append((o.cpu().numpy(), eng.debug_read(st, "ce").cpu().numpy()))
            assert not st.error()
        finally:
            st.close()
        return out

    a, b, c = run(17), run(17), run(33)
    for k in range(2):
        assert np.array_equal(a[k][0], b[k][0]), k
        same_in = np.array_equal(a[k][1], c[k][1][:17])
        print(f"  step {k}: cluster input bitwise equal at B = 17 and B = 33: {same_in}")
        if same_in:  # the cluster's input is batch-independent: so must its output be
            assert np.array_equal(a[k][0], c[k][0][:17]), k
        else:  # (the GEMMs in front of the cluster picked other tiles for the other batch)
            assert _maxerr(a[k][0], c[k][0][:17]) < ATOL, k


def test_repeatable_under_load(engines):
    """40 steps at batch 64 while a second stream keeps HBM and the CUs busy, against the quiet run: bitwise equal"""
    eng, _, _ = engines("F512")
    side = torch.cuda.Stream()
    big = torch.randn(32 * 1024 * 1024, device="cuda:0")
    mats = torch.randn(2048, 2048, device="cuda:0")
    k = [0]

    def busy():
        k[0] += 1
        with torch.cuda.stream(side):
            if k[0] % 3 == 0:
                big.mul_(1.0000001)
            elif k[0] % 3 == 1:
                torch.mm(mats, mats)

    def run(load):
        rng = np.random.default_rng(5)
        st = eng.new_lm_state(64, 20 + 41)
        try:
            st.set_flow_fold(True)
            eng.lm_prefill(st, dev((rng.standard_normal((64, 20, eng.D)) * 0.3).astype(np.float32)))
            out = []
            for _ in range(40):
                noise = dev((rng.standard_normal((64, eng.ldim)) * 0.8).astype(np.float32))
                if load:
                    busy()
                o, _, _ = eng.lm_decode_step(st, None, noise, 1, THR)
                out.append(o.clone())
            torch.cuda.synchronize()
            assert not st.error()
        finally:
            st.close()
        return np.stack([o.cpu().numpy() for o in out])

    a, b = run(True), run(False)
    side.synchronize()
    assert np.isfinite(a).all() and np.array_equal(a, b)


def test_switch_is_refused_under_captured_graphs_and_mod_is_not_handed_out(engines):
    from pocket_tts_amd._lib import PttsError

    eng, _, _ = engines("F64")
    B = 17
    rng = np.random.default_rng(3)
    st = eng.new_lm_state(B, 8)
    try:
        eng.lm_prefill(st, dev((rng.standard_normal((B, 4, eng.D)) * 0.3).astype(np.float32)))
        eng.lm_decode_step(st, None, dev(np.zeros((B, eng.ldim), np.float32)), 1, THR)
        mod = eng.debug_read(st, "mod")  # an unfolded step materialises the modulations
        assert mod.shape == (B, (3 * 2 + 2) * 64) and torch.isfinite(mod).all()
        out, lg = torch.zeros(B, eng.ldim, device="cuda:0"), torch.zeros(B, device="cuda:0")
        fl = torch.zeros(B, dtype=torch.uint8, device="cuda:0")
        eng.sync()
        g = eng.capture_lm_step(st, None, 1, THR, out, lg, fl)  # captured without the fold: it cannot be turned on now
        try:
            with pytest.raises(PttsError, match="captured graphs"):
                st.set_flow_fold(True)
            st.set_flow_fold(False)  # no change: accepted
        finally:
            eng.graph_destroy(g)
        st.set_flow_fold(True)
        eng.lm_decode_step(st, None, dev(np.zeros((B, eng.ldim), np.float32)), 1, THR)
        with pytest.raises(PttsError, match="flow fold"):
            eng.debug_read(st, "mod")
        eng.sync()
        g = eng.capture_lm_step(st, None, 1, THR, out, lg, fl)
        try:
            with pytest.raises(PttsError, match="captured graphs"):
                st.set_flow_fold(False)
            st.set_flow_fold(True)  # no change: accepted
        finally:
            eng.graph_destroy(g)
        st.set_flow_fold(False)
        assert not st.error()
    finally:
        st.close()
