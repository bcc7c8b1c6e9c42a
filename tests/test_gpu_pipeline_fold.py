"""StepPipeline with the flow fold (`flow_fold`, PTTS_FLOW_FOLD): in the throughput mode its FlowLM graphs carry the folded
flow cluster (csrc/ptts_flow.h: flow_cluster_mod_kernel).  Every frame it hands out must be the frame the unfolded pipeline
hands out and the frame eager steps give, within test_gpu_parity.ATOL (the modulations sum in another order), across
restart(); small batches keep the latency path and the unfolded kernels.  `-m gpu`."""

import numpy as np
import pytest
import torch

from test_gpu_parity import ATOL, _maxerr, dev, get_engine

pytestmark = pytest.mark.gpu

B, TP, NS = 9, 23, 7  # "events" is the default mode from batch 9 on


def _emb(eng, b=B):
    rng = np.random.default_rng(22)
    return dev((rng.standard_normal((b, TP, eng.D)) * 0.5).astype(np.float32))


def run_pipeline(eng, emb, fold_env, monkeypatch):
    """two utterances of NS frames with restart() between them -> [utterance][frame] host copies of the PCM"""
    from pocket_tts_amd.engine import StepPipeline

    monkeypatch.setenv("PTTS_FLOW_FOLD", fold_env)
    st, ms = eng.new_lm_state(B, TP + NS), eng.new_mimi_state(B)
    pipe = StepPipeline(eng, st, ms, None, 1, float("inf"))
    assert pipe.mode == "events" and pipe.flow_fold == (fold_env == "1")
    out = []
    for rep in range(2):
        st.reset()
        eng.lm_prefill(st, emb)
        pipe.restart()
        got = {}
        for i in range(NS + 1):
            f = pipe.step() if i < NS else pipe.flush()
            if f is None:
                continue
            for g in ([f - 1, f] if pipe.codec_pair and i < NS else [f]):
                pipe.done_event(g).synchronize()
                got[g] = pipe.pcm_of(g).numpy().copy()
        assert sorted(got) == list(range(NS)), sorted(got)
        out.append([got[i] for i in range(NS)])
    assert not st.error()
    pipe.close()
    ms.close()
    st.close()
    return out


def test_fold_pipeline_matches_unfolded_pipeline_and_eager_frames(monkeypatch):
    eng = get_engine("tiny")
    emb = _emb(eng)
    eng.tune(B)
    st, ms = eng.new_lm_state(B, TP + NS), eng.new_mimi_state(B)
    eng.lm_prefill(st, emb)
    ref = []
    for _ in range(NS):
        o, _, _ = eng.lm_decode_step(st, None, None, 1, float("inf"))
        pcm = eng.mimi_decode(ms, o)
        torch.cuda.synchronize()
        ref.append(pcm.cpu().numpy().copy())
    ms.close()
    st.close()
    off = run_pipeline(eng, emb, "0", monkeypatch)
    on = run_pipeline(eng, emb, "1", monkeypatch)
    for u in range(2):
        for f in range(NS):
            assert np.abs(off[u][f]).max() > 0
            assert _maxerr(on[u][f], off[u][f]) < ATOL, (u, f)
            assert _maxerr(on[u][f], ref[f]) < ATOL, (u, f)


def test_graphs_of_a_fold_pipeline_carry_the_folded_kernel(monkeypatch):
    """a state the pipeline has switched on runs `flow_cluster_mod` in an eager step too, and no `flow.adaln`"""
    from pocket_tts_amd.engine import StepPipeline

    monkeypatch.setenv("PTTS_FLOW_FOLD", "1")
    eng = get_engine("tiny")
    st, ms = eng.new_lm_state(B, TP + 2), eng.new_mimi_state(B)
    pipe = StepPipeline(eng, st, ms, None, 1, float("inf"))
    assert pipe.flow_fold
    pipe.close()  # its graphs are gone; the state keeps the switch
    eng.lm_prefill(st, _emb(eng))
    eng.profile_start()
    try:
        eng.lm_decode_step(st, None, None, 1, float("inf"))
    finally:
        prof = [(r["site"], r["kernel"]) for r in eng.profile_stop()]
    torch.cuda.synchronize()
    assert not [k for s, k in prof if s == "flow.adaln"], prof
    assert [k.split("@")[0] for s, k in prof if s == "flow.cluster"] == ["flow_cluster_mod"], prof
    assert not st.error()
    ms.close()
    st.close()


def test_small_batches_keep_the_unfolded_path(monkeypatch):
    from pocket_tts_amd.engine import StepPipeline

    monkeypatch.setenv("PTTS_FLOW_FOLD", "1")
    eng = get_engine("tiny")
    st, ms = eng.new_lm_state(3, TP + 2), eng.new_mimi_state(3)
    pipe = StepPipeline(eng, st, ms, None, 1, float("inf"), mode="events")
    assert pipe.mode == "events" and pipe.flow_fold is False
    pipe.close()
    ms.close()
    st.close()
