"""Per-row LSD schedules of a FlowLM state (ptts_lm_state_reserve_row_lsd / set_row_lsd): every row runs its own number of
Euler steps of the flow head inside one batched step.  Checked against the numpy oracle run per row with that row's
count, bitwise against a state without the capacity stepped with the same count, inside a captured graph, on both flow
paths (the single-launch cluster and the per-layer launches), and through ContinuousBatcher against single-request
generation with a model loaded at that count."""

from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import synth_weights
from test_gpu_parity import _maxerr, dev, get_engine

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"

B = 37  # three row groups of 16: 0-15, 16-31, 32-36
CTX = 12
STEPS = 6


def _prefilled(eng, seed, Bn=B, K=None, steps=STEPS):
    rng = np.random.default_rng(seed)
    emb = (rng.standard_normal((Bn, CTX, eng.D)) * 0.3).astype(np.float32)
    st = eng.new_lm_state(Bn, CTX + steps + 2)
    if K is not None:
        st.reserve_row_lsd(K)
    eng.lm_prefill(st, dev(emb))
    return st, emb


def _noise(eng, seed, Bn=B, steps=STEPS):
    rng = np.random.default_rng(seed + 1000)
    return [(rng.standard_normal((Bn, eng.ldim)) * 0.8).astype(np.float32) for _ in range(steps)]


def _run(eng, st, noise, lsd):
    lat, lg = [], []
    for z in noise:
        o, l, _ = eng.lm_decode_step(st, None, dev(z), lsd, -4.0)
        lat.append(o.clone())
        lg.append(l.clone())
    torch.cuda.synchronize()
    assert not st.error()
    return np.stack([o.cpu().numpy() for o in lat]), np.stack([l.cpu().numpy() for l in lg])


# per-row counts (0: no override, the step's lsd_steps = 2)
def _mixed():
    pat = [1, 2, 3, 5, 0, 1, 3, 0, 5, 2, 1]
    return [pat[r % len(pat)] for r in range(B)]


def _grouped():
    n = [1] * 16 + [0] * 16 + [3, 0, 2, 1, 0]  # group 0: all n = 1; group 1: one row at 5; group 2: mixed
    n[21] = 5
    return n


@pytest.mark.parametrize("cfg_name", ["tiny", "en100m"])
@pytest.mark.parametrize("cluster", [1, 0])
@pytest.mark.parametrize("pattern", ["mixed", "grouped"])
def test_per_row_counts_match_oracle(cfg_name, cluster, pattern):
    from oracle import np_oracle as O

    eng = get_engine(cfg_name)
    cfg, W = synth_weights(cfg_name)
    eng.set_option("flow_cluster", cluster)
    lsd_def = 2
    ns = _mixed() if pattern == "mixed" else _grouped()
    st, emb = _prefilled(eng, 3, K=5)
    for r, n in enumerate(ns):
        if n:
            st.set_row_lsd(r, n)
    noise = _noise(eng, 3)
    try:
        lat, lg = _run(eng, st, noise, lsd_def)
    finally:
        eng.set_option("flow_cluster", 1)
        st.close()
    eff = np.array([n or lsd_def for n in ns])
    # one oracle state per count: every row is fed its own history, the row with that count is read from it
    lm = O.FlowLM(cfg, W)
    ref_lat = np.zeros_like(lat)
    ref_lg = np.zeros_like(lg)
    for n in sorted(set(eff.tolist())):
        ost = lm.init_state(B, CTX + STEPS + 2)
        lm.prefill(ost, emb)
        x = np.full((B, eng.ldim), np.nan, np.float32)
        rows = eff == n
        for k in range(STEPS):
            o, l, _ = lm.decode_step(ost, x, noise[k], n, -4.0)
            ref_lat[k][rows] = o[rows]
            ref_lg[k][rows] = l[rows]
            x = lat[k]  # the batch's own history (GPU latents) for every row
    assert np.isfinite(lat).all()
    err = np.abs(lat.astype(np.float64) - ref_lat).reshape(STEPS, B, -1).max(axis=(0, 2))
    assert err.max() <= 1e-4, {int(r): float(err[r]) for r in np.argsort(err)[-5:]}
    assert _maxerr(lg, ref_lg) <= 1e-3


@pytest.mark.parametrize("cluster", [1, 0])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_overridden_rows_equal_a_plain_state(cluster, n):
    """every row overridden to n (even rows) or running the step's count n (odd rows, no override) against a state
    without the capacity stepped with lsd_steps = n: bitwise for n >= 2 (same kernels, same summation order)"""
    eng = get_engine("en100m")
    eng.set_option("flow_cluster", cluster)
    try:
        plain, _ = _prefilled(eng, 5)
        ref, ref_lg = _run(eng, plain, _noise(eng, 5), n)
        plain.close()
        st, _ = _prefilled(eng, 5, K=5)
        for r in range(0, B, 2):
            st.set_row_lsd(r, n)
        got, got_lg = _run(eng, st, _noise(eng, 5), n)
        st.close()
    finally:
        eng.set_option("flow_cluster", 1)
    if n >= 2:
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    else:  # n = 1: the plain state folds the time embedding + SiLU into the head GEMM, the reserved one does not
        assert _maxerr(got, ref) <= 1e-6
    assert _maxerr(got_lg, ref_lg) <= 1e-6


def test_rows_overridden_against_the_step_count():
    """rows overridden to n = 1 and 4 in a step whose own count is 3: each matches a plain state at its count"""
    eng = get_engine("en100m")
    refs = {}
    for n in (1, 3, 4):
        plain, _ = _prefilled(eng, 8)
        refs[n], _ = _run(eng, plain, _noise(eng, 8), n)
        plain.close()
    st, _ = _prefilled(eng, 8, K=4)
    ns = [(1, 4, 0)[r % 3] for r in range(B)]
    for r, n in enumerate(ns):
        if n:
            st.set_row_lsd(r, n)
    got, _ = _run(eng, st, _noise(eng, 8), 3)
    st.close()
    for r, n in enumerate(ns):
        ref = refs[n or 3][:, r]
        if n == 1:
            assert _maxerr(got[:, r], ref) <= 1e-6, r
        else:
            assert np.array_equal(got[:, r].view(np.uint32), ref.view(np.uint32)), (r, n)


@pytest.mark.parametrize("cluster", [1, 0])
def test_captured_step_reads_overrides_set_after_capture(cluster):
    eng = get_engine("en100m")
    eng.set_option("flow_cluster", cluster)
    steps = 4
    noise = _noise(eng, 9, steps=steps)
    plans = [{}, {r: 1 + r % 4 for r in range(0, B, 3)}, {r: 4 for r in range(16, 32)}, {0: 2, 36: 3}]
    g = None
    try:
        cap, _ = _prefilled(eng, 9, K=4, steps=steps)
        ref, _ = _prefilled(eng, 9, K=4, steps=steps)
        zbuf = dev(noise[0])
        out_lat = torch.empty((B, eng.ldim), device="cuda:0")
        out_logit = torch.empty((B,), device="cuda:0")
        out_eos = torch.empty((B,), dtype=torch.uint8, device="cuda:0")
        g = eng.capture_lm_step(cap, zbuf, 2, -4.0, out_lat, out_logit, out_eos)
        for k in range(steps):
            for st in (cap, ref):
                for r in range(B):
                    if r in plans[k]:
                        st.set_row_lsd(r, plans[k][r])
                    elif k and r in plans[k - 1]:
                        st.clear_row_lsd(r)
            zbuf.copy_(dev(noise[k]))
            torch.cuda.synchronize()  # the copy runs on torch's stream, the graph on the engine's
            eng.graph_launch(g)
            o, l, _ = eng.lm_decode_step(ref, None, dev(noise[k]), 2, -4.0)
            torch.cuda.synchronize()
            assert np.array_equal(out_lat.cpu().numpy().view(np.uint32), o.cpu().numpy().view(np.uint32)), k
            assert np.array_equal(out_logit.cpu().numpy(), l.cpu().numpy()), k
        assert not cap.error() and not ref.error()
        # the capacity cannot change under a captured graph
        with pytest.raises(Exception):
            cap.reserve_row_lsd(8)
        assert eng.lib.ptts_lm_state_reserve_row_lsd(cap.handle, 2, None) < 0
    finally:
        if g is not None:
            eng.graph_destroy(g)
        eng.set_option("flow_cluster", 1)
    cap.close()
    ref.close()


def test_error_codes():
    from pocket_tts_amd._lib import PttsError

    eng = get_engine("tiny")
    st = eng.new_lm_state(4, 16)
    lib = eng.lib
    with pytest.raises(PttsError):
        st.set_row_lsd(0, 2)  # no capacity
    assert lib.ptts_lm_state_set_row_lsd(st.handle, 0, 1, None) < 0
    for K in (0, 65, -1):
        assert lib.ptts_lm_state_reserve_row_lsd(st.handle, K, None) < 0
    st.reserve_row_lsd(3)
    for row, n in ((0, 4), (0, 0), (0, -1), (4, 2), (-1, 2)):
        with pytest.raises(PttsError):
            st.set_row_lsd(row, n)
        assert lib.ptts_lm_state_set_row_lsd(st.handle, row, n, None) < 0
    for row in (4, -1):
        assert lib.ptts_lm_state_clear_row_lsd(st.handle, row, None) < 0
    assert lib.ptts_lm_state_set_row_lsd(st.handle, 3, 3, None) == 0
    st.reserve_row_lsd(2)  # never shrinks: 3 stays allowed
    assert lib.ptts_lm_state_set_row_lsd(st.handle, 1, 3, None) == 0
    assert lib.ptts_lm_state_clear_row_lsd(st.handle, 1, None) == 0
    st.close()


def test_reset_clears_overrides():
    eng = get_engine("en100m")
    plain, _ = _prefilled(eng, 12, steps=2)
    ref, _ = _run(eng, plain, _noise(eng, 12, steps=2), 2)
    plain.close()
    st, _ = _prefilled(eng, 12, K=5, steps=2)
    for r in range(B):
        st.set_row_lsd(r, 1 + r % 5)
    _run(eng, st, _noise(eng, 12, steps=1), 2)
    st.reset()
    rng = np.random.default_rng(12)
    eng.lm_prefill(st, dev((rng.standard_normal((B, CTX, eng.D)) * 0.3).astype(np.float32)))
    got, _ = _run(eng, st, _noise(eng, 12, steps=2), 2)
    st.close()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


# ---- the continuous batcher ----------------------------------------------------------------------------------------
TEXTS = ["Hello world.", "The quick brown fox jumps over the lazy dog.", "One two three.", "Good morning to you all."]


def test_batcher_per_request_lsd_matches_single_generation():
    from pocket_tts_amd import TTSModel
    from pocket_tts_amd.batching import ContinuousBatcher

    counts = [1, 2, 4, None, 2, 4, None, 1]
    m = TTSModel.load_model(config=G / "e2e_tiny.yaml", temp=0.0)
    voice_path = G / "e2e_voice.safetensors"
    try:
        state = m.get_state_for_audio_prompt(voice_path)
        cb = ContinuousBatcher(m, slots=8, capacity=512, max_lsd_decode_steps=4)
        try:
            with pytest.raises(ValueError):
                cb.submit(state, "hi", lsd_decode_steps=5)
            with pytest.raises(ValueError):
                cb.submit(state, "hi", lsd_decode_steps=0)
            with pytest.raises(ValueError):
                cb.submit(state, "hi", lsd_decode_steps=2.0)
            reqs = [cb.submit(state, TEXTS[i % len(TEXTS)], lsd_decode_steps=n) for i, n in enumerate(counts)]
            cb.run_until_idle()
            outs = [r.result() for r in reqs]
        finally:
            cb.close()
        plain = ContinuousBatcher(m, slots=2, capacity=512)  # no capacity: only the model's own count
        try:
            with pytest.raises(ValueError):
                plain.submit(state, "hi", lsd_decode_steps=m.lsd_decode_steps + 1)
        finally:
            plain.close()
    finally:
        m.engine.close()
    for n in sorted(set(c or 1 for c in counts)):
        single = TTSModel.load_model(config=G / "e2e_tiny.yaml", temp=0.0, lsd_decode_steps=n)
        try:
            st1 = single.get_state_for_audio_prompt(voice_path)
            for i, c in enumerate(counts):
                if (c or 1) != n:
                    continue
                ref = single.generate_audio(st1, TEXTS[i % len(TEXTS)])
                assert outs[i].shape == ref.shape, (i, n, outs[i].shape, ref.shape)
                assert np.abs(outs[i].numpy() - ref.numpy()).max() < 5e-4, (i, n)
        finally:
            single.engine.close()
