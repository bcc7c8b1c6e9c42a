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


# ---- all seven stages ---------------------------------------------------------------------------------------------------------
FULL = dict(sample_rate=16000, speed=0.8, pitch="5/4", tone="warm", loudness_lufs=-16.0, gain_db=6.0, encoding="mulaw")
FULL_SUBSETS = [c for n in range(1, len(FULL) + 1) for c in itertools.combinations(FULL, n)
                if not {"loudness_lufs", "gain_db"} <= set(c)]
DRAINS = {"stretch": "ts", "pitch": "ps", "loud": "ln", "level": "lv"}


def _table(eng, fields):
    """the `ChainTable` of exactly the stages the request fields `fields` name"""
    from pocket_tts_amd.output_chain import ChainTable

    return ChainTable(eng.sample_rate, eng.frame_samples, [FULL["sample_rate"]] if "sample_rate" in fields else None,
                      [FULL["speed"]] if "speed" in fields else None, "gain_db" in fields,
                      [FULL["pitch"]] if "pitch" in fields else None, "loudness_lufs" in fields,
                      [FULL["encoding"]] if "encoding" in fields else None, [FULL["tone"]] if "tone" in fields else None)


def _twins(eng, B, table):
    """{name: stage} in chain order: stages of their own for the table, to be driven one by one"""
    t = {}
    if table.has_rates:
        t["rs"] = eng.new_resampler(B, table.sample_rates)
    if table.speeds is not None:
        t["ts"] = eng.new_stretcher(B, table.stretch_plans)
    if table.pitches is not None:
        t["ps"] = eng.new_pitcher(B, table.pitch_plans)
    if table.tone_plans is not None:
        t["tn"] = eng.new_toner(B, table.tone_plans, table.width)
    if table.loud_plans is not None:
        t["ln"] = eng.new_normalizer(B, table.loud_plans)
    if table.level_plans is not None:
        t["lv"] = eng.new_leveler(B, table.level_plans)
    if table.encodings is not None:
        t["en"] = eng.new_encoder(B, table.width)
    return t


def _deal(t, row, r):
    """what `OutputChain.set_row` deals a row on the route `r`, by hand"""
    for name, args in (("rs", (r.rate_index,)), ("ts", (r.stretch_plan,)), ("ps", (r.pitch_plan,)), ("tn", (r.tone_plan,)),
                       ("ln", r.loud or (None, None)), ("lv", r.level or (None, None, None)), ("en", (r.n_out, r.encoding))):
        if name in t:
            t[name].set_row(row, *args)


@pytest.mark.parametrize("subset", FULL_SUBSETS, ids="+".join)
def test_every_stage_subset_in_one_graph_equals_the_stages_one_by_one(eng, subset):
    """A table of exactly the subset's stages, row 0 on the subset's route, row 1 on the default route, 3 frames and the
    route's drain frames: after every frame both rows of the pinned ring equal, bit for bit (with an encoder: byte for byte
    over n_out * bytes_per_sample), stages of their own run one by one through f32 device buffers on the same PCM; what
    `Route.take` selects over the run is 3 * n_out samples, finite and not silent; without an encoder row 1 is the PCM"""
    from pocket_tts_amd.output_chain import OutputChain

    B, fs, dev = 2, eng.frame_samples, eng.device
    table = _table(eng, subset)
    routes = [table.route(**{k: FULL[k] for k in subset}), table.route()]
    route, enc = routes[0], "encoding" in subset
    assert routes[1].n_out == fs and routes[1].preroll == 0
    bps = [r.bytes_per_sample if enc else 4 for r in routes]
    ms = eng.new_mimi_state(B)
    chain = OutputChain(eng, B, table, 1)
    t = _twins(eng, B, table)
    g = None
    try:
        assert [type(s) for s in chain.stages()] == [type(s) for s in t.values()]
        # what each twin writes: f32 on the device, the encoder bytes
        bufs = [torch.zeros(B, s.pitch, dtype=torch.uint8, device=dev) if n == "en" else
                torch.zeros(B, s.out_max if n in ("rs", "ts") else s.width, device=dev) for n, s in t.items()]
        assert chain.out[0].shape == bufs[-1].shape and chain.out[0].dtype == bufs[-1].dtype and chain.out[0].is_pinned()
        lat = torch.randn(B, eng.ldim, device=dev, generator=torch.Generator(dev).manual_seed(4))
        pcm = torch.zeros(B, fs, device=dev)
        chain.attach(ms, 0)
        g = eng.capture_mimi(ms, lat, pcm)
        chain.detach(ms)
        for b, r in enumerate(routes):
            chain.set_row(b, r)
            _deal(t, b, r)
        got, want, fed, pos = [], [], [], 0
        for f in range(FRAMES + route.drain_frames):
            if f == FRAMES:  # the row's job has ended: what follows are its drain frames
                chain.drain_row(0, route)
                t[DRAINS[route.drain_stage]].set_row_drain(0, True)
            eng.graph_launch(g)
            eng.sync()
            x = last_f32 = pcm
            for stage, y in zip(t.values(), bufs):
                stage.frame(x, y)
                last_f32, x = x, y
            if not enc:
                last_f32 = x
            torch.cuda.synchronize()
            line = chain.out[0].numpy().copy().view(np.uint8)
            ref = x.cpu().numpy().view(np.uint8)
            for b, r in enumerate(routes):
                assert np.array_equal(line[b, :r.n_out * bps[b]], ref[b, :r.n_out * bps[b]]), (f, b)
            p = pcm.cpu().numpy()
            assert p[1].any(), f
            if not enc:  # the default route is an exact copy
                assert np.array_equal(line[1, :4 * fs], p[1].view(np.uint8)), f
            lo, hi = route.take(pos, None if f < FRAMES else FRAMES)
            got.append(line[0, lo * bps[0]:hi * bps[0]])
            want.append(ref[0, lo * bps[0]:hi * bps[0]])
            fed.append(last_f32.cpu().numpy()[0, lo:hi])  # the same samples as f32, before the encoder if there is one
            pos += route.n_out
        got, fed = np.concatenate(got), np.concatenate(fed)
        assert got.size == FRAMES * route.n_out * bps[0] and np.array_equal(got, np.concatenate(want))
        assert fed.size == FRAMES * route.n_out and np.isfinite(fed).all() and fed.any()
        if enc:
            assert (got != 0xFF).any()  # mu-law: FF is silence
        else:
            assert np.array_equal(got, fed.view(np.uint8))
    finally:
        if g is not None:
            eng.graph_destroy(g)
        for s in reversed(list(t.values())):
            s.close()
        chain.close()
        ms.close()


def _codec_launches(eng, ms):
    """(site, kernel) of every launch of one eager codec frame, in launch order"""
    lat = torch.zeros(ms.batch, eng.ldim, device=eng.device)
    pcm = torch.zeros(ms.batch, eng.frame_samples, device=eng.device)
    eng.sync()
    eng.profile_start()
    eng.mimi_decode(ms, lat, pcm)
    return [(r["site"], r["kernel"]) for r in eng.profile_stop()]


# what the commit before the chain's links records behind the codec's last launch with all seven stages attached
FULL_TAIL = [("resample", "resample"), ("resample", "resample_carry"), ("stretch", "stretch"), ("pitch", "pitch"),
             ("tone", "tone"), ("loudnorm", "loudnorm"), ("level", "level"), ("encode", "encode")]


def test_the_launch_tail_of_the_full_chain(eng):
    """all seven stages attached: one eager frame records the codec's launches and then, literally, `FULL_TAIL`; after
    `detach` the list is the codec's alone again"""
    from pocket_tts_amd.output_chain import OutputChain

    ms = eng.new_mimi_state(2)
    chain = OutputChain(eng, 2, _table(eng, FULL), 1)
    try:
        assert len(chain.stages()) == 7
        codec = _codec_launches(eng, ms)
        assert codec and codec[-1] == ("mimi.tail", "step_tail")
        chain.attach(ms, 0)
        got = _codec_launches(eng, ms)
        assert got[:len(codec)] == codec and got[len(codec):] == FULL_TAIL
        chain.detach(ms)
        assert _codec_launches(eng, ms) == codec
    finally:
        chain.close()
        ms.close()
