"""Per-request output sample rates on the GPU: the resampler kernels against the fp64 streaming reference
(tests/resample_ref.py), row independence, `set_row`, the C ABI's error codes, and the path through the continuous batcher,
`TTSModel.generate_audio` and the HTTP server (tiny model)."""

import asyncio
import ctypes as C
import io
import shutil
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

from resample_ref import StreamRef, to_i16, to_i16_f32

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"
ROW_RATES = [24000, 8000, 16000, 22050, 32000, 44100, 48000]  # one row per rate, the native one first
N_FRAMES = 3
SENTINEL_F, SENTINEL_I = -77.0, -12345
TEXTS = ["Hello world. This is a test.", "ok", "How are you today?", "Short one.", "And one more."]


@pytest.fixture(scope="module")
def model():
    from pocket_tts_amd import TTSModel

    m = TTSModel.load_model(config=G / "e2e_tiny.yaml", temp=0.0)
    yield m
    m.engine.close()


@pytest.fixture(scope="module")
def eng(model):
    return model.engine


@pytest.fixture(scope="module")
def frames():
    """3 frames of uniform noise in [-1.2, 1.2] for 7 rows: zero history, then the carry twice; beyond +-1 for the clamp"""
    rng = np.random.default_rng(7)
    return rng.uniform(-1.2, 1.2, (N_FRAMES, len(ROW_RATES), 1920)).astype(np.float32)


def _run(eng, row_rates, x, i16=False, reset=None):
    """x [frames, B, 1920] through a fresh Resampler whose row b runs at row_rates[b]; `reset` = (after_frame, row):
    `set_row` on that row once that many frames have run.  Returns (per-frame outputs [B, out_max], resampler plans of the
    rows).  The output tensor is pre-filled with a sentinel before every frame."""
    B = len(row_rates)
    rs = eng.new_resampler(B, [r for r in ROW_RATES if r != 24000])
    try:
        for b, r in enumerate(row_rates):
            rs.set_row(b, rs.index_of(r))
        outs = []
        for f in range(x.shape[0]):
            if reset is not None and reset[0] == f:
                rs.set_row(reset[1], rs.row_rate[reset[1]])
            out = torch.full((B, rs.out_max), SENTINEL_I if i16 else SENTINEL_F, dtype=torch.int16 if i16 else torch.float32,
                             device=eng.device)
            rs.frame(torch.from_numpy(x[f]).to(eng.device), out)
            torch.cuda.synchronize()
            outs.append(out.cpu().numpy())
        return outs, [rs.plans[rs.index_of(r)] for r in row_rates]
    finally:
        rs.close()


@pytest.fixture(scope="module")
def base(eng, frames):
    """the f32 and i16 runs every kernel test compares with, and the fp64 reference of each row (computed once)"""
    out_f, plans = _run(eng, ROW_RATES, frames)
    out_i, _ = _run(eng, ROW_RATES, frames, i16=True)
    ref = []
    for b, p in enumerate(plans):
        s = StreamRef(p.table, p.up, p.down)  # the kernel's own fp32 taps, in float64
        ref.append([s.frame(frames[f, b]) for f in range(N_FRAMES)])
    return dict(f=out_f, i=out_i, plans=plans, ref=ref)


def test_f32_within_the_dot_product_bound(base, frames):
    worst = {}
    for b, p in enumerate(base["plans"]):
        assert p.out_n == 1920 * p.up // p.down
        for f in range(N_FRAMES):
            y64, bound = base["ref"][b][f]
            got = base["f"][f][b]
            err = np.abs(got[:p.out_n].astype(np.float64) - y64)
            worst[p.rate] = max(worst.get(p.rate, 0.0), float((err / bound.clip(2.0 ** -24)).max()))
            assert (err <= bound).all(), (p.rate, f, float(err.max()), float(bound[err.argmax()]))
            # entries at n >= out_n of the pre-filled row are untouched
            assert (got[p.out_n:] == SENTINEL_F).all(), (p.rate, f)
    print("resampler f32 error / bound per rate:", {k: round(v, 3) for k, v in worst.items()})


def test_native_row_is_bit_equal_to_its_input(base, frames):
    assert base["plans"][0].native
    for f in range(N_FRAMES):
        assert np.array_equal(base["f"][f][0][:1920].view(np.uint32), frames[f, 0].view(np.uint32))
        assert np.array_equal(base["i"][f][0][:1920], to_i16_f32(frames[f, 0]))


def test_i16_is_the_conversion_of_the_f32_output(base):
    for b, p in enumerate(base["plans"]):
        for f in range(N_FRAMES):
            got = base["i"][f][b]
            assert np.array_equal(got[:p.out_n], to_i16_f32(base["f"][f][b][:p.out_n])), (p.rate, f)
            want = to_i16(base["ref"][b][f][0]).astype(np.int32)
            assert np.abs(got[:p.out_n].astype(np.int32) - want).max() <= 1, (p.rate, f)
            assert (got[p.out_n:] == SENTINEL_I).all(), (p.rate, f)
    # the input range exercises the clamp
    assert any((base["i"][f] == 32767).any() for f in range(N_FRAMES)) and any((base["i"][f] == -32767).any() for f in range(N_FRAMES))


def test_rows_are_independent_of_their_position(eng, base, frames):
    perm = [3, 5, 0, 6, 1, 4, 2]  # row j of the permuted run holds row perm[j]'s rate and input
    outs, plans = _run(eng, [ROW_RATES[k] for k in perm], np.ascontiguousarray(frames[:, perm]))
    for j, k in enumerate(perm):
        assert plans[j].rate == ROW_RATES[k]
        for f in range(N_FRAMES):
            assert np.array_equal(outs[f][j].view(np.uint32), base["f"][f][k].view(np.uint32)), (j, k, f)


def test_set_row_restarts_one_row_only(eng, base, frames):
    row = 5  # 44100 Hz
    outs, _ = _run(eng, ROW_RATES, frames, reset=(2, row))
    fresh, _ = _run(eng, ROW_RATES, frames[2:3])  # the third frame as the first frame of a fresh stream
    n = base["plans"][row].out_n
    assert np.array_equal(outs[2][row][:n].view(np.uint32), fresh[0][row][:n].view(np.uint32))
    assert not np.array_equal(outs[2][row][:n], base["f"][2][row][:n])  # the carried history did matter
    for f in range(N_FRAMES):
        for b in range(len(ROW_RATES)):
            if (f, b) != (2, row):
                assert np.array_equal(outs[f][b].view(np.uint32), base["f"][f][b].view(np.uint32)), (f, b)


def test_cabi_error_codes(eng, frames):
    from pocket_tts_amd._lib import PttsError

    rs = eng.new_resampler(2, [8000, 48000])
    try:
        lib, sp = eng.lib, eng._sp
        for row, idx in ((-1, 0), (2, 0), (0, -1), (0, 3), (0, 1 << 20)):
            assert lib.ptts_resampler_set_row(rs.handle, row, idx, sp) == -1, (row, idx)
            assert b"out of range" in lib.ptts_last_error()
        with pytest.raises(PttsError):
            rs.set_row(2, 0)
        assert rs.row_rate == [0, 0]
        with pytest.raises(ValueError):
            rs.index_of(44100)
        pcm = torch.from_numpy(frames[0, :2]).to(eng.device)
        out = torch.zeros(2, rs.out_max, device=eng.device)
        assert lib.ptts_resample_frame(rs.handle, None, C.c_void_p(out.data_ptr()), 0, sp) == -1
        assert lib.ptts_resample_frame(rs.handle, C.c_void_p(pcm.data_ptr()), None, 0, sp) == -1
        assert lib.ptts_resample_frame(None, C.c_void_p(pcm.data_ptr()), C.c_void_p(out.data_ptr()), 0, sp) == -1
        assert lib.ptts_resampler_set_row(None, 0, 0, sp) == -1
        # a rate the rules do not admit never reaches the device: 10560 Hz has 844.8 samples per frame (up 11, down 25)
        h = C.c_void_p()
        one = (C.c_int32 * 1)
        tab = (C.c_float * (11 * 46))()
        assert lib.ptts_resampler_create(eng.handle, 2, one(11), one(25), one(46), 1, tab, 11 * 46, C.byref(h)) == -1
        assert lib.ptts_resampler_create(eng.handle, 2, one(1), one(3), one(66), 1, tab, 66, C.byref(h)) == -1  # taps - 1 > 64
        assert lib.ptts_resampler_create(eng.handle, 2, one(1), one(3), one(61), 1, tab, 60, C.byref(h)) == -1  # table size
        ms = eng.new_mimi_state(3)
        assert lib.ptts_mimi_set_resampler(ms.handle, rs.handle, C.c_void_p(out.data_ptr()), 0) == -1  # batch 3 vs 2
        ms.close()
        # the refused calls launched nothing: both rows still run at the native rate with a zero history
        rs.frame(pcm, out)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy()[:, :1920], frames[0, :2])
    finally:
        rs.close()


# ---- through the batcher, the model and the server -------------------------------------------------------------------------
def _resample_ref(rs_plan, wav):
    """fp64 streaming resampling of a native-rate waveform (whole frames) with the plan's fp32 taps -> (y, bound)"""
    s = StreamRef(rs_plan.table, rs_plan.up, rs_plan.down)
    parts = [s.frame(wav[i:i + 1920]) for i in range(0, wav.shape[0], 1920)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def test_batcher_end_to_end(model):
    from pocket_tts_amd.batching import ContinuousBatcher
    from pocket_tts_amd.resample import plan

    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    # four requests fill the four slots at step 0; the fifth waits for a slot and runs at a rate that none of them has, so
    # its `set_row` changes the rate of a REUSED slot behind the frames of the slot's earlier request still queued on the
    # codec stream - the order the admission path relies on
    rates = [None, 8000, 44100, 48000, 16000]

    def run(sample_rates, req_rates):
        cb = ContinuousBatcher(model, slots=4, capacity=512, **({} if sample_rates is None else {"sample_rates": sample_rates}))
        try:
            reqs = [cb.submit(state, t, **({} if r is None else {"sample_rate": r})) for t, r in zip(TEXTS, req_rates)]
            cb.run_until_idle()
            return [(r.sample_rate, r.frames, r.result().numpy()) for r in reqs]
        finally:
            cb.close()

    plain = run(None, [None] * 5)
    got = run([8000, 16000, 44100, 48000], rates)
    with pytest.raises(ValueError):
        run([8000], [16000])
    assert len(plain) == len(got) == 5 and len({p[1] for p in plain}) > 1  # requests of different lengths
    for (rate_p, frames_p, wav_p), (rate, n_frames, wav), want in zip(plain, got, rates):
        assert rate_p == 24000 and rate == (want or 24000) and n_frames == frames_p and wav_p.shape[0] == frames_p * 1920
        p = plan(rate, 24000, 1920)
        assert wav.shape[0] == n_frames * p.out_n, (rate, wav.shape, n_frames)
        if want is None:
            assert np.array_equal(wav.view(np.uint32), wav_p.view(np.uint32))  # the native request: bit-identical
            continue
        y64, bound = _resample_ref(p, wav_p)
        err = np.abs(wav.astype(np.float64) - y64)
        assert (err <= bound).all(), (rate, float(err.max()))


def test_generate_audio_sample_rate(model):
    from pocket_tts_amd.resample import plan

    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    ref = model.generate_audio(state, TEXTS[0]).numpy()
    again = model.generate_audio(state, TEXTS[0], sample_rate=24000).numpy()
    assert np.array_equal(ref, again)
    wav = model.generate_audio(state, TEXTS[0], sample_rate=16000).numpy()
    y64, bound = _resample_ref(plan(16000), ref)
    assert wav.shape == y64.shape == (ref.shape[0] * 2 // 3,)
    assert (np.abs(wav.astype(np.float64) - y64) <= bound).all()
    with pytest.raises(ValueError, match="whole number"):
        model.generate_audio(state, TEXTS[0], sample_rate=10560)
    # a caller that cycles through rates does not pile up contexts (state, resampler, graphs): the oldest are released
    for rate in (8000, 48000, 32000):
        assert model.generate_audio(state, TEXTS[1], sample_rate=rate).shape[0] % plan(rate).out_n == 0
    assert sum(1 for k in model._ctx_cache if "rate" in k) <= model.RATE_CONTEXTS
    assert np.array_equal(model.generate_audio(state, TEXTS[0], sample_rate=16000).numpy(), wav)  # a rebuilt context


def test_server_sample_rate(model, tmp_path):
    import httpx

    from pocket_tts_amd.server import create_app

    shutil.copy(G / "e2e_voice.safetensors", tmp_path / "e2e_voice.safetensors")
    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    n_frames = model.generate_audio(state, TEXTS[0]).shape[0] // 1920
    app = create_app(model, slots=4, capacity=512, voices_dir=tmp_path, default_voice="e2e_voice", sample_rates=[8000, 16000])

    async def go():
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t", timeout=600) as cl:
                return await asyncio.gather(cl.post("/tts", data={"text": TEXTS[0], "temperature": "0", "sample_rate": "16000"}),
                                            cl.post("/tts", data={"text": TEXTS[0], "temperature": "0"}),
                                            cl.post("/tts", data={"text": TEXTS[0], "sample_rate": "44100"}))

    r16, r24, bad = asyncio.run(go())
    assert bad.status_code == 400 and "not configured" in bad.json()["detail"]
    for r, rate, out_n in ((r16, 16000, 1280), (r24, 24000, 1920)):
        assert r.status_code == 200, r.text[:200]
        with wave.open(io.BytesIO(r.content), "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, rate)
        assert len(r.content) - 44 == n_frames * out_n * 2 + 2 * int(rate * 0.2)  # 16000: frames * 1280 * 2 + 2 * 3200
        assert not np.frombuffer(r.content[-2 * int(rate * 0.2):], np.int16).any()
    assert np.frombuffer(r16.content[44:], np.int16)[:n_frames * 1280].any()
