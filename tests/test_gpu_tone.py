"""Per-request tone on the GPU: the toner kernel against the float64 direct-form-I reference (tests/tone_ref.py) under the
bound of one fp32 rounding plus the float64 scheme's own error, exactness and isolation, streaming state, captured graphs,
the whole output chain - and the path through the continuous batcher, `TTSModel.generate_audio_stream` and the HTTP server
(tiny model).

E64 is the largest |chunked - serial| / (running peak of |serial|) of the float64 chunk / scan / re-run scheme over the five
shapes below, measured on the CPU by tests/cpp/tone_sweep.cpp (tests/test_tone_cpu.py::test_e64_of_the_gpu_tests_shapes prints
it and holds it against this file): 3.0e-14, 2.8e-15, 7.0e-15, 1.9e-13 and, for (48000, 7680), 1.067e-12."""

import asyncio
import io
import json
import re
import shutil
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

import g711_ref
import level_ref
import tone_ref

E64 = 1.1e-12

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"
SENTINEL_F = -77.0
GUARD = 4096
TEXT = "Hello world. This is a test."
F = 8  # frames: noise, digital silence in frames 3 and 4 (the ring-out), noise again
EIGHT = "hp:40;peak:200:6:4;peak:500:-6:2;peak:1000:3;peak:2000:-3:8;lowshelf:300:4;highshelf:3000:-4;lp:3500"
# (rate, n, tone); None: bypass.  chunk 2; one sample per thread; fewer threads than the block; eight sections with the last
# thread holding one sample (1025 = 512 * 2 + 1); chunk 8
ROWS = [None, (24000, 1920, "telephone"), (8000, 640, "telephone"), (11025, 882, "lowshelf:200:6"), (24000, 1025, EIGHT),
        (48000, 7680, "hp:40;peak:3000:6:4;highshelf:8000:-6")]
WIDTH = 7680


def _plans():
    from pocket_tts_amd.tone import plan

    return [plan(*r) for r in ROWS if r is not None]


def _plan_index(b):
    return None if ROWS[b] is None else sum(1 for r in ROWS[:b] if r is not None)


def _signal(n, seed):
    x = np.random.default_rng(seed).standard_normal(F * n)
    x = np.convolve(x, np.ones(3) / 3.0, mode="same") * 0.25
    x[3 * n:5 * n] = 0.0
    return x.astype(np.float32)


@pytest.fixture(scope="module")
def ref():
    """the rows' input streams and, for each toned row, the float64 reference; computed once and left unchanged"""
    streams, refs = [], []
    for b, r in enumerate(ROWS):
        if r is None:
            streams.append(np.random.default_rng(100 + b).standard_normal(F * WIDTH).astype(np.float32))
            refs.append(None)
            continue
        rate, n, spec = r
        x = _signal(n, 200 + b)
        y64 = tone_ref.reference(spec, rate, x)
        assert np.isfinite(y64).all() and np.abs(y64[:3 * n]).max() > 0.01
        assert y64[3 * n + 2:5 * n].any()  # the ring-out of the silence is no silence
        streams.append(x)
        refs.append(y64)
    for y in refs:
        if y is not None:
            y.setflags(write=False)
    return streams, refs


def _lines(streams, order=None, frames=F):
    """[frames, B, WIDTH] input lines: row b's frame at the front of its line, NaN behind it (nothing may read it)"""
    order = list(range(len(ROWS))) if order is None else order
    x = np.full((frames, len(order), WIDTH), np.nan, np.float32)
    for j, b in enumerate(order):
        n = WIDTH if ROWS[b] is None else ROWS[b][1]
        x[:, j, :n] = streams[b][:frames * n].reshape(frames, n)
    return x


def _guarded(eng, shape, fill, dtype=torch.float32):
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=eng.device)
    return big[GUARD:GUARD + n].view(*shape), big


def _run(eng, x, order=None, events=None):
    """x [frames, B, WIDTH] through a fresh Toner whose row j runs row `order[j]`; `events` = {frame: [j]}: set_row of row j
    again before that frame.  The output and the guard bands around it are pre-filled with sentinels before every frame.
    Returns outs [frames][B, WIDTH]"""
    order = list(range(len(ROWS))) if order is None else order
    B = len(order)
    tn = eng.new_toner(B, _plans(), WIDTH)
    try:
        assert tn.width == WIDTH and tn.row_plan == [-1] * B
        for j, b in enumerate(order):
            tn.set_row(j, _plan_index(b))
        outs = []
        for f in range(x.shape[0]):
            for j in (events or {}).get(f, ()):
                tn.set_row(j, tn.row_plan[j])
            out, out_big = _guarded(eng, (B, WIDTH), SENTINEL_F)
            xin, _ = _guarded(eng, (B, WIDTH), float("nan"))
            xin.copy_(torch.from_numpy(x[f]))
            tn.frame(xin, out)
            torch.cuda.synchronize()
            g = out_big.cpu().numpy()
            assert (g[:GUARD] == SENTINEL_F).all() and (g[-GUARD:] == SENTINEL_F).all(), "a write outside the buffer"
            assert np.array_equal(xin.cpu().numpy().view(np.uint32), x[f].view(np.uint32)), "the input was written"
            outs.append(out.cpu().numpy())
        return outs
    finally:
        tn.close()


def _stream_of(outs, j, n):
    return np.concatenate([o[j, :n] for o in outs])


def _bound(y64):
    """one fp32 rounding of the sample, plus ten times the float64 scheme's own error at the running peak (ten: the
    reference is direct form I, the stage transposed direct form II)"""
    return 2.0 ** -24 * np.abs(y64) + 10.0 * E64 * np.maximum.accumulate(np.abs(y64))


@pytest.fixture(scope="module")
def model():
    """a model of this file's own: the toned contexts it leaves in the model's cache reach no other file's tests"""
    from pocket_tts_amd import TTSModel

    m = TTSModel.load_model(config=G / "e2e_tiny.yaml", temp=0.0)
    yield m
    m.engine.close()


@pytest.fixture(scope="module")
def eng(model):
    return model.engine


@pytest.fixture(scope="module")
def base(eng, ref):
    return _run(eng, _lines(ref[0]))


def test_against_the_reference(ref, base):
    streams, refs = ref
    worst = 0.0
    for b, r in enumerate(ROWS):
        if r is None:
            got = np.stack([o[b] for o in base])
            assert np.array_equal(got.view(np.uint32), streams[b].reshape(F, WIDTH).view(np.uint32))  # bypass: the whole line
            continue
        rate, n, spec = r
        for o in base:
            assert (o[b, n:] == SENTINEL_F).all(), (b, "written past the row's n")
        y, y64 = _stream_of(base, b, n), refs[b]
        assert y.shape == y64.shape and np.isfinite(y).all()
        err, bound = np.abs(y.astype(np.float64) - y64), _bound(y64)
        k = int(np.argmax(err / np.maximum(bound, 1e-300)))
        share = err[k] / bound[k]
        print(f"tone row {b} {r}: largest |y - y64| = {err.max():.3g}; largest share of the bound {share:.3f} at sample {k}")
        worst = max(worst, share)
        assert (err <= bound).all(), (b, k, err[k], bound[k])
    print(f"tone: worst share of the bound {worst:.3f}")


def test_a_row_is_bitwise_the_same_in_any_slot_and_any_batch(eng, ref, base):
    streams, _ = ref
    order = [5, 4, 4, 0, 3, 2, 1, 1, 5]
    outs = _run(eng, _lines(streams, order), order)
    for j, b in enumerate(order):
        n = WIDTH if ROWS[b] is None else ROWS[b][1]
        assert np.array_equal(_stream_of(outs, j, n).view(np.uint32), _stream_of(base, b, n).view(np.uint32)), (j, b)
    for b in (1, 4, 5):  # alone in a batch of one
        outs = _run(eng, _lines(streams, [b]), [b])
        n = ROWS[b][1]
        assert np.array_equal(_stream_of(outs, 0, n).view(np.uint32), _stream_of(base, b, n).view(np.uint32)), b


def test_set_row_restarts_a_row_from_zero_state(eng, ref, base):
    """rows that have run three frames and are set again: from there on they are fresh rows fed frames 3 ..; the others go on"""
    streams, _ = ref
    x = _lines(streams)
    x2 = np.concatenate([x[:3], x[:F - 3]])  # every row sees its first frames again from frame 3 on
    outs = _run(eng, x2, events={3: [1, 4, 5]})
    for b in (1, 4, 5):
        n = ROWS[b][1]
        assert np.array_equal(_stream_of(outs[3:], b, n).view(np.uint32), _stream_of(base[:F - 3], b, n).view(np.uint32)), b
    n = ROWS[2][1]  # a row that was not set again carries its state over: its frames 3 .. differ from a fresh row's
    assert not np.array_equal(_stream_of(outs[3:], 2, n), _stream_of(base[:F - 3], 2, n))


def _frame_plans():
    from pocket_tts_amd.tone import plan

    return [plan(24000, 1920, "telephone"), plan(24000, 1920, "lowshelf:200:6"), plan(24000, 1920, EIGHT)]


def test_captured_graph_follows_set_row(eng):
    """a codec graph captured with a toner and a leveler: a later set_row to another plan and to bypass changes what its
    replays compute, without recapture, exactly as it changes stages of their own fed the same PCM frame by frame"""
    from pocket_tts_amd import level

    B = 3
    assert eng.frame_samples == 1920
    plans, lplans = _frame_plans(), [level.plan(24000, 1920)]
    ms = eng.new_mimi_state(B)
    tn, twin = eng.new_toner(B, plans), eng.new_toner(B, plans)
    lv, lv2 = eng.new_leveler(B, lplans), eng.new_leveler(B, lplans)
    g = None
    try:
        lat = torch.randn(B, eng.ldim, device=eng.device, generator=torch.Generator(eng.device).manual_seed(3))
        pcm = torch.zeros(B, 1920, device=eng.device)
        mid, mid2 = torch.full((B, 1920), SENTINEL_F, device=eng.device), torch.full((B, 1920), SENTINEL_F, device=eng.device)
        out, want = torch.full((B, 1920), SENTINEL_F, device=eng.device), torch.full((B, 1920), SENTINEL_F, device=eng.device)
        for s, v in ((tn, lv), (twin, lv2)):
            s.set_row(1, 0)
            s.set_row(2, 2)
            for b in range(B):
                v.set_row(b, 0, 0.0)
        ms.set_tone(tn, mid)
        ms.set_leveler(lv, out, mid)
        g = eng.capture_mimi(ms, lat, pcm)
        ms.set_leveler(None)
        ms.set_tone(None)
        u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731

        def step(tag):
            eng.graph_launch(g)
            eng.sync()
            twin.frame(pcm, mid2)
            lv2.frame(mid2, want)
            torch.cuda.synchronize()
            assert pcm.abs().max().item() > 0
            assert np.array_equal(u32(mid), u32(mid2)), tag
            assert np.array_equal(u32(out), u32(want)), tag
            return mid.cpu().numpy().copy(), pcm.cpu().numpy().copy()

        for f in range(3):
            a, x = step(("plain", f))
        assert np.array_equal(a[0], x[0]) and not np.array_equal(a[1], x[1]) and not np.array_equal(a[2], x[2])
        for s in (tn, twin):
            s.set_row(1, 1)   # another plan
            s.set_row(2, -1)  # to bypass
            s.set_row(0, 0)   # from bypass to a plan
        for f in range(3):
            b_, x = step(("set_row", f))
        assert np.array_equal(b_[2], x[2]) and not np.array_equal(b_[0], x[0]) and not np.array_equal(b_[1], x[1])
        # an eager decode on a state with the two stages appends the same launches
        ms.set_tone(tn, mid)
        ms.set_leveler(lv, out, mid)
        eng.mimi_decode(ms, lat, pcm)
        eng.sync()
        twin.frame(pcm, mid2)
        lv2.frame(mid2, want)
        torch.cuda.synchronize()
        assert np.array_equal(u32(out), u32(want))
        ms.set_leveler(None)
        ms.set_tone(None)
    finally:
        if g is not None:
            eng.graph_destroy(g)
        for s in (lv, lv2, tn, twin):
            s.close()
        ms.close()


def test_the_chain_in_one_graph_equals_its_stages_one_by_one(eng):
    """codec -> pitcher (5/4) -> tone -> normaliser -> leveler -> encoder in one captured graph, against stages of their own
    run one by one on the recorded intermediate buffers: bitwise"""
    from pocket_tts_amd import level, loudness, pitch

    B = 2
    ms = eng.new_mimi_state(B)
    pplans = [pitch.identity(24000, 1920), pitch.plan("5/4", 24000, 1920)]
    made = [(eng.new_pitcher(B, pplans), eng.new_toner(B, _frame_plans()), eng.new_normalizer(B, [loudness.plan(24000, 1920)]),
             eng.new_leveler(B, [level.plan(24000, 1920)]), eng.new_encoder(B, 1920)) for _ in range(2)]
    (ps, tn, ln, lv, en), (ps2, tn2, ln2, lv2, en2) = made
    g = None
    try:
        for p, t, n_, v, e in made:
            p.set_row(0, 1)
            t.set_row(0, 0)
            n_.set_row(0, 0, -16.0)
            v.set_row(0, 0, 0.0, -3.0)
            e.set_row(0, 1920, "mulaw")
            p.set_row(1, 0)  # row 1: pitch 1, eight sections, no target, its own gain
            t.set_row(1, 2)
            v.set_row(1, 0, 3.0)
            e.set_row(1, 1920, "pcm_f32le")
        lat = torch.randn(B, eng.ldim, device=eng.device, generator=torch.Generator(eng.device).manual_seed(4))
        pcm = torch.zeros(B, 1920, device=eng.device)
        m1, m2, m3, m4 = (torch.full((B, 1920), SENTINEL_F, device=eng.device) for _ in range(4))
        out = torch.zeros(B, en.pitch, dtype=torch.uint8, device=eng.device)
        w1, w2, w3, w4 = (torch.full((B, 1920), SENTINEL_F, device=eng.device) for _ in range(4))
        w5 = torch.zeros_like(out)
        ms.set_pitcher(ps, m1)
        ms.set_tone(tn, m2, m1)
        ms.set_loudnorm(ln, m3, m2)
        ms.set_leveler(lv, m4, m3)
        ms.set_encoder(en, out, m4)
        g = eng.capture_mimi(ms, lat, pcm)
        for off in (ms.set_encoder, ms.set_leveler, ms.set_loudnorm, ms.set_tone, ms.set_pitcher):
            off(None)
        u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
        for f in range(7):  # D = 9600 samples of the normaliser are over after five frames
            eng.graph_launch(g)
            eng.sync()
            for stage, src, dst, got in ((ps2, pcm, w1, m1), (tn2, m1, w2, m2), (ln2, m2, w3, m3), (lv2, m3, w4, m4)):
                stage.frame(src, dst)
                torch.cuda.synchronize()
                assert np.array_equal(u32(dst), u32(got)), (f, type(stage).__name__)
            en2.frame(m4, w5)
            torch.cuda.synchronize()
            assert np.array_equal(w5.cpu().numpy(), out.cpu().numpy()), f
        assert m4.cpu().numpy()[0].any() and m4.cpu().numpy()[1].any() and np.isfinite(m4.cpu().numpy()).all()
    finally:
        if g is not None:
            eng.graph_destroy(g)
        for stages in made:
            for s in reversed(stages):
                s.close()
        ms.close()


def test_cabi_error_codes(eng):
    import ctypes as C

    from pocket_tts_amd import level, tone

    plans = _frame_plans()
    tn = eng.new_toner(2, plans)
    try:
        lib, sp = eng.lib, eng._sp
        for row, idx in ((-1, 0), (2, 0), (0, -2), (0, 3), (0, 1 << 20)):  # bad row, bad plan index
            assert lib.ptts_tone_set_row(tn.handle, row, idx, sp) == -1, (row, idx)
            assert b"out of range" in lib.ptts_last_error()
        assert lib.ptts_tone_set_row(None, 0, 0, sp) == -1
        with pytest.raises(ValueError, match="plan index"):
            tn.set_row(0, 3)
        assert tn.row_plan == [-1, -1]
        x = torch.zeros(2, tn.width, device=eng.device)
        out = torch.zeros(2, tn.width, device=eng.device)
        px, po = C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr())
        assert lib.ptts_tone_frame(tn.handle, None, po, sp) == -1 and lib.ptts_tone_frame(tn.handle, px, None, sp) == -1
        assert lib.ptts_tone_frame(None, px, po, sp) == -1
        assert lib.ptts_tone_frame(tn.handle, px, px, sp) == -1 and b"in place" in lib.ptts_last_error()  # in == out
        for bad in (torch.zeros(2, tn.width - 1, device=eng.device), torch.zeros(3, tn.width, device=eng.device),
                    torch.zeros(2, tn.width, dtype=torch.float64, device=eng.device), torch.zeros(2, tn.width)):
            with pytest.raises(ValueError, match="toner input"):  # width mismatch and friends, before the library is called
                tn.frame(bad, out)
            with pytest.raises(ValueError, match="toner input"):
                tn.frame(x, bad)
        h = C.c_void_p()
        d = np.ascontiguousarray(plans[0].doubles())
        pd = d.ctypes.data_as(C.POINTER(C.c_double))
        for rate, n, K in ((7999, 640, 1), (48001, 1920, 1), (24000, 0, 1), (24000, 8193, 1), (24000, 1920, 0), (24000, 1920, 9)):
            arr = (C.c_int32 * 3)(rate, n, K)  # a plan that breaks a rule never reaches the device
            assert lib.ptts_tone_create(eng.handle, 2, 0, arr, 1, pd, d.size, C.byref(h)) == -1
            assert b"not admissible" in lib.ptts_last_error()
        arr = (C.c_int32 * 3)(24000, 1920, 4)
        assert lib.ptts_tone_create(eng.handle, 2, 0, arr, 1, pd, d.size - 1, C.byref(h)) == -1
        assert lib.ptts_tone_create(eng.handle, 2, 1919, arr, 1, pd, d.size, C.byref(h)) == -1  # a line narrower than a plan
        assert b"longer than the line" in lib.ptts_last_error()
        assert lib.ptts_tone_create(eng.handle, 2, 8193, arr, 1, pd, d.size, C.byref(h)) == -1
        bad = d.copy()
        bad[50] = np.inf
        assert lib.ptts_tone_create(eng.handle, 2, 0, arr, 1, bad.ctypes.data_as(C.POINTER(C.c_double)), d.size, C.byref(h)) == -1
        assert b"not finite" in lib.ptts_last_error()
        assert tone.DOUBLES_PER_PLAN == d.size
        ms = eng.new_mimi_state(3)
        assert lib.ptts_mimi_set_tone(ms.handle, tn.handle, None, po) == -1 and b"batch" in lib.ptts_last_error()  # 3 vs 2
        ms.close()
        ms = eng.new_mimi_state(2)
        assert lib.ptts_mimi_set_tone(None, tn.handle, None, po) == -1
        assert lib.ptts_mimi_set_tone(ms.handle, tn.handle, None, None) == -1 and b"null output" in lib.ptts_last_error()
        assert lib.ptts_mimi_set_tone(ms.handle, tn.handle, po, po) == -1 and b"in place" in lib.ptts_last_error()
        # an input buffer means "behind an earlier stage": refused on a state that has none
        assert lib.ptts_mimi_set_tone(ms.handle, tn.handle, px, po) == -1 and b"input buffer" in lib.ptts_last_error()
        wide = eng.new_toner(2, plans, 2048)  # width mismatch: the toner's line is not the state's frame
        wo = torch.zeros(2, 2048, device=eng.device)
        assert lib.ptts_mimi_set_tone(ms.handle, wide.handle, None, C.c_void_p(wo.data_ptr())) == -1
        assert b"frame length" in lib.ptts_last_error()
        wide.close()
        # a frame with a toner but no leveler fails, and nothing of the toner is enqueued before the check
        lat = torch.zeros(2, eng.ldim, device=eng.device)
        pcm = torch.zeros(2, eng.frame_samples, device=eng.device)
        assert lib.ptts_mimi_set_tone(ms.handle, tn.handle, None, po) == 0
        assert lib.ptts_mimi_decode(eng.handle, ms.handle, C.c_void_p(lat.data_ptr()), C.c_void_p(pcm.data_ptr()), sp) == -1
        assert b"followed by a leveler" in lib.ptts_last_error()
        # the leveler accepts an input buffer on a state whose only earlier stage is the toner
        lv = eng.new_leveler(2, [level.plan(24000, 1920)])
        out2 = torch.zeros(2, lv.width, device=eng.device)
        assert lib.ptts_mimi_set_leveler(ms.handle, lv.handle, po, C.c_void_p(out2.data_ptr()), 0) == 0
        assert lib.ptts_mimi_set_leveler(ms.handle, None, None, None, 0) == 0
        assert lib.ptts_mimi_set_tone(ms.handle, None, None, None) == 0
        eng.sync()
        lv.close()
        ms.close()
    finally:
        tn.close()


# ---- through the batcher, the model and the server -------------------------------------------------------------------------
def _toned_and_limited(wav_p, spec, rate=24000, n=1920, peak_dbfs=None):
    """the untoned waveform through `tone_ref`, rounded to fp32 once as the stage does, then `level_ref` at gain 0 dB: (what
    the request delivers, the float64 output of the tone alone).  The limiter must be idle on the reference (asserted): its
    gain is then exactly 1 and the leveler a delay, so the bound of the stage test holds for the chain"""
    from pocket_tts_amd import level

    y64 = tone_ref.reference(spec, rate, wav_p)
    lp = level.plan(rate, n)
    Gl, Cl = level.params(0.0, peak_dbfs)
    assert np.abs(y64).max() < 0.99 * float(Cl), "the reference engages the limiter"
    x = np.concatenate([y64.astype(np.float32).astype(np.float64), np.zeros(lp.LA)])
    y = level_ref.level(x, Gl, Cl, lp.LA, lp.a, lp.k)
    return y[lp.LA:lp.LA + wav_p.shape[0]], y64


def _within(wav, want, y64, what):
    err, bound = np.abs(wav.astype(np.float64) - want), _bound(y64)
    k = int(np.argmax(err / np.maximum(bound, 1e-300)))
    print(f"{what}: largest |y - y64| = {err.max():.3g}; largest share of the bound {err[k] / bound[k]:.3f}")
    assert (err <= bound).all(), (what, k, err[k], bound[k])


@pytest.fixture(scope="module")
def alone(model):
    """(frames, waveform) of TEXT as the only request of a fresh batcher with the leveler alone (2 slots), without a gain:
    the leveler's bypass, the model's own samples"""
    from pocket_tts_amd.batching import ContinuousBatcher

    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    cb = ContinuousBatcher(model, slots=2, capacity=512, level=True)
    try:
        assert cb.tn is None
        r = cb.submit(state, TEXT)
        cb.run_until_idle()
        return r.frames, r.result().numpy()
    finally:
        cb.close()


def test_batcher_end_to_end(model, eng, alone):
    from pocket_tts_amd.batching import ContinuousBatcher

    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    frames, wav_p = alone
    assert wav_p.shape[0] == frames * 1920 and wav_p.any()
    cb = ContinuousBatcher(model, slots=2, capacity=512, tones=["telephone", "hp:120;peak:3000:-4"])
    try:
        assert cb.tn is not None and cb.lv is not None and cb.ln is None and cb.lagging
        with pytest.raises(ValueError, match="is not configured"):
            cb.submit(state, TEXT, tone="warm")
        with pytest.raises(ValueError, match="needs a gain"):
            cb.submit(state, TEXT, tone="peak:100")
        with pytest.raises(ValueError, match="frames_after_eos >= 1"):
            cb.submit(state, TEXT, frames_after_eos=0, tone="telephone")
        r = cb.submit(state, TEXT, tone="telephone")
        cb.run_until_idle()
        wav = r.result().numpy()
        assert r.frames == frames and wav.shape[0] == frames * 1920
        want, y64 = _toned_and_limited(wav_p, "telephone")
        _within(wav, want, y64, "batcher, telephone at 24 kHz")
        assert not np.array_equal(wav, wav_p)
        # then, in the slot the toned request has left: an untoned request is bitwise the one of a plain levelled batcher
        r = cb.submit(state, TEXT)
        cb.run_until_idle()
        assert np.array_equal(r.result().numpy().view(np.uint32), wav_p.view(np.uint32))
        # and a band list, under its canonical form (a cut: the tiny model is loud, and a boost would engage the limiter)
        r = cb.submit(state, TEXT, tone="HP:120 ; peak:3000:-4:1")
        cb.run_until_idle()
        want, y64 = _toned_and_limited(wav_p, "hp:120;peak:3000:-4")
        _within(r.result().numpy(), want, y64, "batcher, hp:120;peak:3000:-4")
    finally:
        cb.close()
    cb = ContinuousBatcher(model, slots=2, capacity=512, level=True)
    try:
        with pytest.raises(ValueError, match="no tone stage"):
            cb.submit(state, TEXT, tone="telephone")
    finally:
        cb.close()


def test_generate_audio_stream_tone_and_the_server_field(model, eng, tmp_path):
    import httpx

    from pocket_tts_amd.server import create_app

    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    try:
        # 8 kHz through the leveler's bypass... gain 0 dB limits, so the untoned stream is read in float32 at 8 kHz as it is
        wav8 = np.concatenate([c.numpy() for c in model.generate_audio_stream(state, TEXT, sample_rate=8000)])
        chunks = [c.numpy() for c in model.generate_audio_stream(state, TEXT, tone="telephone", sample_rate=8000, encoding="mulaw")]
        assert all(c.dtype == np.uint8 and 0 < c.shape[0] <= 640 for c in chunks)
        mu = np.concatenate(chunks)
        f32 = np.concatenate([c.numpy() for c in model.generate_audio_stream(state, TEXT, tone="telephone", sample_rate=8000,
                                                                             encoding="pcm_f32le")])
        assert mu.shape == f32.shape == wav8.shape
        want, y64 = _toned_and_limited(wav8, "telephone", 8000, 640)
        _within(f32, want, y64, "model, telephone at 8 kHz")
        assert np.array_equal(mu, g711_ref.lin2ulaw(g711_ref.s16(f32)).astype(np.uint8))  # the same samples, as G.711
        with pytest.raises(ValueError, match="not admissible at 8000 Hz"):
            model.generate_audio(state, TEXT, tone="bright", sample_rate=8000)
        with pytest.raises(ValueError, match="neither a preset"):
            model.generate_audio(state, TEXT, tone="loud")
        assert any("tone" in k[4:] and "level" in k[4:] for k in model._ctx_cache)
    finally:
        model._drop_rate_contexts(0)
    assert not any("tone" in k[4:] for k in model._ctx_cache)

    shutil.copy(G / "e2e_voice.safetensors", tmp_path / "e2e_voice.safetensors")
    app = create_app(model, slots=2, capacity=512, voices_dir=tmp_path, default_voice="e2e_voice", sample_rates=[8000],
                     tones=["telephone", "bright"])
    plain = create_app(model, slots=2, capacity=512, voices_dir=tmp_path, default_voice="e2e_voice")

    async def go(app, forms):
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t", timeout=600) as cl:
                return [await cl.post("/tts", data=d) for d in forms]

    ok, other, refused = asyncio.run(go(app, [{"text": TEXT, "tone": "telephone", "sample_rate": "8000"},
                                              {"text": TEXT, "tone": "warm"},
                                              {"text": TEXT, "tone": "bright", "sample_rate": "8000"}]))
    (without,) = asyncio.run(go(plain, [{"text": TEXT, "tone": "telephone"}]))
    assert other.status_code == 400 and "['telephone', 'bright']" in other.json()["detail"]
    assert refused.status_code == 400 and "admissible there: ['telephone']" in refused.json()["detail"]
    assert without.status_code == 400 and "without tones" in without.json()["detail"]
    assert ok.status_code == 200, ok.text[:200]
    with wave.open(io.BytesIO(ok.content), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 8000)
    pcm = np.frombuffer(ok.content[44:], np.int16)[:f32.shape[0]]
    assert np.abs(pcm.astype(np.int64) - g711_ref.s16(f32).astype(np.int64)).max() <= 1  # the same stream, as 16-bit samples


# ---- feature off ------------------------------------------------------------------------------------------------------------
def _step_launches(eng, st, ms):
    """(site, kernel) of every launch of one eager FlowLM step followed by one eager codec frame, in launch order"""
    lat = torch.zeros(ms.batch, eng.ldim, device=eng.device)
    pcm = torch.zeros(ms.batch, eng.frame_samples, device=eng.device)
    eng.sync()
    eng.profile_start()
    if st is not None:
        eng.lm_decode_step(st, None, None, 1, float("inf"))
    eng.mimi_decode(ms, lat, pcm)
    return [(r["site"], r["kernel"]) for r in eng.profile_stop()]


def _untuned(rows):
    """the launch list with what the tuner chooses per process taken out of the names: the template arguments and the
    '@threads' of the GEMM and attention kernels (their family and prologue suffix stay); every other name stays whole"""
    return [(s, re.sub(r"<[^>]*>", "", k).split("@")[0] if k.startswith(("gemm", "attn")) else k) for s, k in rows]


def test_without_tones_the_launches_are_those_of_the_parent_commit(model, eng):
    """tests/golden/stretch_noop_launches.json holds what the commit before the output chain records for one eager FlowLM
    step and one codec frame, on the batcher's states and on the `TTSModel` context: built without `tones`, both still record
    the same launches at the same sites in the same order"""
    from pocket_tts_amd.batching import ContinuousBatcher

    want = json.loads((G / "stretch_noop_launches.json").read_text())
    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    cb = ContinuousBatcher(model, slots=2, capacity=512)
    try:
        cb.submit(state, "ok")
        cb.run_until_idle()
        assert cb.tn is None and cb.lv is None and not cb.lagging and cb.pipe.out is None and cb.pipe.pcm[0].is_pinned()
        got = _step_launches(eng, cb.st, cb.ms)
    finally:
        cb.close()
    assert len(got) == len(want["batcher"]) == 25
    assert [s for s, _ in got] == [s for s, _ in want["batcher"]]
    assert _untuned(got) == _untuned(map(tuple, want["batcher"]))
    model._drop_rate_contexts(0)
    model.generate_audio(state, "ok")
    ctxs = [c for k, c in model._ctx_cache.items() if len(k) == 4]
    assert ctxs and all(c["pipe"].tn is None and c["pipe"].lv is None and c["pipe"].out is None for c in ctxs)
    for c in ctxs:
        got = _step_launches(eng, c["st"], c["ms"])
        assert len(got) == len(want["model"]) == 25
        assert [s for s, _ in got] == [s for s, _ in want["model"]]
        assert _untuned(got) == _untuned(map(tuple, want["model"]))


def test_a_toner_set_and_cleared_leaves_the_launches_of_before(eng):
    from pocket_tts_amd import level, loudness, pitch

    fresh, used = eng.new_mimi_state(2), eng.new_mimi_state(2)
    ps = eng.new_pitcher(2, [pitch.identity(24000, 1920)])
    tn = eng.new_toner(2, _frame_plans())
    ln = eng.new_normalizer(2, [loudness.plan(24000, 1920)])
    lv = eng.new_leveler(2, [level.plan(24000, 1920)])
    try:
        want = _step_launches(eng, None, fresh)
        assert want and not any("tone" in s or "tone" in k for s, k in want)
        m1, m2, m3, out = (torch.zeros(2, 1920, device=eng.device) for _ in range(4))
        used.set_tone(tn, m2)
        used.set_leveler(lv, out, m2)
        assert _step_launches(eng, None, used) == want + [("tone", "tone"), ("level", "level")]
        used.set_leveler(None)
        used.set_tone(None)
        assert _step_launches(eng, None, used) == want
        # between the pitcher's launch and the normaliser's
        used.set_pitcher(ps, m1)
        used.set_loudnorm(ln, m3, m1)
        used.set_leveler(lv, out, m3)
        without = _step_launches(eng, None, used)
        used.set_leveler(None)
        used.set_loudnorm(None)
        used.set_tone(tn, m2, m1)
        used.set_loudnorm(ln, m3, m2)
        used.set_leveler(lv, out, m3)
        with_tone = _step_launches(eng, None, used)
        i = [s for s, _ in without].index("loudnorm")
        assert without[i - 1][0] == "pitch" and with_tone == without[:i] + [("tone", "tone")] + without[i:]
        for off in (used.set_leveler, used.set_loudnorm, used.set_tone, used.set_pitcher):
            off(None)
        assert _step_launches(eng, None, used) == want
    finally:
        for s in (lv, ln, tn, ps):
            s.close()
        fresh.close()
        used.close()
