"""The device half of the output chain (pocket_tts_amd/output_chain.py) on the GPU: an `OutputChain` built from a
`ChainTable`, attached to a codec state and captured in one graph, with two rows on different routes, against the same
stages driven one by one (tiny model, batch 2)."""

import itertools
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"
FRAMES = 3
REQUEST = dict(sample_rate=16000, speed=0.8, gain_db=6.0)
SUBSETS = [c for n in (1, 2, 3) for c in itertools.combinations(REQUEST, n)]


@pytest.fixture(scope="module")
def eng():
    from pocket_tts_amd import TTSModel

    m = TTSModel.load_model(config=G / "e2e_tiny.yaml", temp=0.0)
    yield m.engine
    m.engine.close()


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("subset", SUBSETS, ids="+".join)
def test_two_routes_in_one_graph_equal_the_stages_one_by_one(eng, subset):
    """row 0 on the subset's route, row 1 on the default route, 3 frames and the route's drain frames: the pinned ring
    equals, bitwise, a resampler, a stretcher and a leveler of their own run one by one on the same PCM; row 1 is the PCM"""
    from pocket_tts_amd.output_chain import ChainTable, OutputChain

    B, fs, dev = 2, eng.frame_samples, eng.device
    req = {k: REQUEST[k] for k in subset}
    table = ChainTable(eng.sample_rate, fs, [req["sample_rate"]] if "sample_rate" in req else None,
                       [req["speed"]] if "speed" in req else None, "gain_db" in req)
    route, plain = table.route(**req), table.route()
    assert plain.n_out == fs and plain.preroll == 0 and (route.drain_frames == 0) == (subset == ("sample_rate",))
    ms = eng.new_mimi_state(B)
    chain = OutputChain(eng, B, table, 1)
    # the same stages on their own, dealt the same rows by hand
    rs = eng.new_resampler(B, table.sample_rates) if chain.rs is not None else None
    ts = eng.new_stretcher(B, table.stretch_plans) if chain.ts is not None else None
    lv = eng.new_leveler(B, table.level_plans) if chain.lv is not None else None
    twins = [s for s in (rs, ts, lv) if s is not None]
    bufs = [torch.zeros(B, s.width if s is lv else s.out_max, device=dev) for s in twins]  # what each of them writes
    g = None
    try:
        assert [type(s) for s in chain.stages()] == [type(s) for s in twins] and chain.out[0].shape == bufs[-1].shape
        lat = torch.randn(B, eng.ldim, device=dev, generator=torch.Generator(dev).manual_seed(4))
        pcm = torch.zeros(B, fs, device=dev)
        chain.attach(ms, 0)
        g = eng.capture_mimi(ms, lat, pcm)
        chain.detach(ms)
        chain.set_row(0, route)
        chain.set_row(1, plain)
        if rs is not None:
            rs.set_row(0, route.rate_index)
        if ts is not None:
            ts.set_row(0, route.stretch_plan)
        if route.level is not None:
            lv.set_row(0, *route.level)
        got, want, pos = [], [], 0
        for f in range(FRAMES + route.drain_frames):
            if f == FRAMES:  # the row's job has ended: what follows are its drain frames
                chain.drain_row(0, route)
                {"stretch": ts, "level": lv}[route.drain_stage].set_row_drain(0, True)
            eng.graph_launch(g)
            eng.sync()
            x = pcm
            for stage, y in zip(twins, bufs):
                stage.frame(x, y)
                x = y
            torch.cuda.synchronize()
            line, ref, p = chain.out[0].numpy().copy(), x.cpu().numpy(), pcm.cpu().numpy()
            assert np.array_equal(_bits(line[0, :route.n_out]), _bits(ref[0, :route.n_out])), f
            assert np.array_equal(_bits(line[1, :fs]), _bits(p[1])) and p[1].any(), f  # the default route is an exact copy
            if rs is not None:  # ... and what the resampler makes of the row at the native rate
                assert np.array_equal(_bits(line[1, :fs]), _bits(bufs[0].cpu().numpy()[1, :fs])), f
            lo, hi = route.take(pos, None if f < FRAMES else FRAMES)
            got.append(line[0, lo:hi])
            want.append(ref[0, lo:hi])
            pos += route.n_out
        got = np.concatenate(got)
        assert got.size == FRAMES * route.n_out and np.array_equal(_bits(got), _bits(np.concatenate(want)))
        assert np.isfinite(got).all() and got.any()
    finally:
        if g is not None:
            eng.graph_destroy(g)
        for s in reversed(twins):
            s.close()
        chain.close()
        ms.close()
