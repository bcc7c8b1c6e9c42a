"""StepPipeline with frame pairs through the codec transformer (`codec_pair`, PTTS_CODEC_PAIR): every frame it hands out must be
the frame the single-frame pipeline hands out, within test_gpu_parity.ATOL (a pair sums in another order than two singles), at
an odd utterance length, across restart(), with and without an output chain; and its graph replays must give what eager
whole-frame decodes give.  `-m gpu`."""

import numpy as np
import pytest
import torch

from test_gpu_parity import ATOL, _maxerr, dev, get_engine

pytestmark = pytest.mark.gpu

B, TP, NS = 9, 23, 7  # "events" is the default mode from batch 9 on; 7 frames: three pairs and an odd tail


def _emb(eng):
    rng = np.random.default_rng(21)
    return dev((rng.standard_normal((B, TP, eng.D)) * 0.5).astype(np.float32))


def run_pipeline(eng, emb, pair_env, monkeypatch, read, **chain):
    """two utterances of NS frames with restart() between them -> [utterance][frame] host copies of read(pipe, frame),
    taken when done_event(frame) has fired"""
    from pocket_tts_amd.engine import StepPipeline

    monkeypatch.setenv("PTTS_CODEC_PAIR", pair_env)
    st, ms = eng.new_lm_state(B, TP + NS), eng.new_mimi_state(B)
    pipe = StepPipeline(eng, st, ms, None, 1, float("inf"), **chain)
    assert pipe.mode == "events" and pipe.codec_pair == (pair_env == "1")
    routes = [pipe.chain.table.route(sample_rate=8000 if b % 2 else None) for b in range(B)] if chain else None
    out = []
    for rep in range(2):
        st.reset()
        eng.lm_prefill(st, emb)
        pipe.restart(routes)
        got = {}
        for i in range(NS + 1):
            f = pipe.step() if i < NS else pipe.flush()
            if f is None:
                continue
            # a pair's second frame is handed out with its first complete before it
            for g in ([f - 1, f] if pipe.codec_pair and i < NS else [f]):
                pipe.done_event(g).synchronize()
                got[g] = read(pipe, g).numpy().copy()
        assert sorted(got) == list(range(NS)), sorted(got)
        out.append([got[i] for i in range(NS)])
    pipe.close()
    ms.close()
    st.close()
    return out


def test_pair_pipeline_matches_single_pipeline(monkeypatch):
    eng = get_engine("tiny")
    emb = _emb(eng)
    read = lambda pipe, f: pipe.pcm_of(f)
    single = run_pipeline(eng, emb, "0", monkeypatch, read)
    pair = run_pipeline(eng, emb, "1", monkeypatch, read)
    for u in range(2):
        for f in range(NS):
            assert np.abs(single[u][f]).max() > 0
            assert _maxerr(pair[u][f], single[u][f]) < ATOL, (u, f)
    # the second utterance repeats the first (same prefill, restart() zeroes the codec): a frame read from the wrong ring
    # slot would not
    for f in range(NS):
        assert _maxerr(pair[1][f], pair[0][f]) < ATOL, f


def test_pair_pipeline_with_output_chain(monkeypatch):
    eng = get_engine("tiny")
    emb = _emb(eng)
    read = lambda pipe, f: pipe.out_of(f)
    single = run_pipeline(eng, emb, "0", monkeypatch, read, sample_rates=[8000])
    pair = run_pipeline(eng, emb, "1", monkeypatch, read, sample_rates=[8000])
    for u in range(2):
        for f in range(NS):
            assert np.abs(single[u][f]).max() > 0
            assert _maxerr(pair[u][f], single[u][f]) < ATOL, (u, f)


def test_pair_pipeline_matches_eager_frames(monkeypatch):
    """graph replays of the parts against eager ptts_mimi_decode, one call per frame, on the eager FlowLM step's latents"""
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
    pair = run_pipeline(eng, emb, "1", monkeypatch, lambda pipe, f: pipe.pcm_of(f))
    for f in range(NS):
        assert _maxerr(pair[0][f], ref[f]) < ATOL, f
