"""Per-request output encoding on the GPU: the encoder alone against tests/g711_ref.py over every 16-bit sample, ragged rows
under guard bytes, a captured graph, the chain against the conversions the other stages already make, the launches of a
pipeline without the stage, the C ABI's refusals, and the batcher, the model and the server end to end.  Every comparison is
exact."""

import asyncio
import json
import re
import shutil
import struct
from pathlib import Path

import numpy as np
import pytest
import torch

import g711_ref

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"
FIX = json.loads((G / "g711.json").read_text())
NAMES = ["pcm_s16le", "pcm_f32le", "mulaw", "alaw"]
BPS = {"pcm_s16le": 2, "pcm_f32le": 4, "mulaw": 1, "alaw": 1}
GUARD_BYTE = 0xA5
GUARD = 4096  # a multiple of 16: the view between the bands keeps the buffer's alignment
TEXT = "Hello world. This is a test."
TEMP = 0.7
W, ROWS = 1920, 35


@pytest.fixture(scope="module")
def model():
    from pocket_tts_amd import TTSModel

    m = TTSModel.load_model(config=G / "e2e_tiny.yaml", temp=0.0)
    yield m
    m.engine.close()


@pytest.fixture(scope="module")
def eng(model):
    return model.engine


@pytest.fixture()
def warm(model):
    """the model at TEMP for one test"""
    model.temp = TEMP
    yield model
    model.temp = 0.0


def _want(name, x):
    """the bytes of the fp32 samples x in the encoding `name`, by the reference"""
    x = np.ascontiguousarray(x, np.float32)
    if name == "pcm_f32le":
        return x.tobytes()
    s = g711_ref.s16(x)
    if name == "pcm_s16le":
        return s.astype("<i2").tobytes()
    return (g711_ref.lin2ulaw(s) if name == "mulaw" else g711_ref.lin2alaw(s)).tobytes()


@pytest.fixture(scope="module")
def ramp():
    """[ROWS, W] fp32: every 16-bit sample but -32768 once, as the x that truncates back to it, then zeros; computed once"""
    s, x = g711_ref.ramp()
    assert np.array_equal(g711_ref.s16(x), s)
    full = np.zeros(ROWS * W, np.float32)
    full[:x.shape[0]] = x
    return full.reshape(ROWS, W)


def _guarded(eng, shape, pinned=False):
    """a contiguous uint8 tensor of `shape` in the middle of a larger buffer filled with the guard byte: (view, whole)"""
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8)
    big = big.pin_memory() if pinned else big.to(eng.device)
    return big[GUARD:GUARD + n].view(*shape), big


def _encode(eng, en, x, rows, pinned=False):
    """one frame of x [B, width] through `en` with row b on rows[b] = (n, name): the whole guarded buffer as numpy"""
    for b, (n, name) in enumerate(rows):
        en.set_row(b, n, name)
    out, big = _guarded(eng, (en.batch, en.pitch), pinned)
    xin = torch.from_numpy(np.ascontiguousarray(x)).to(eng.device)
    en.frame(xin, out)
    eng.sync()
    torch.cuda.synchronize()
    assert np.array_equal(xin.cpu().numpy().view(np.uint32), x.view(np.uint32)), "the input was written"
    return big.cpu().numpy().copy()


def _check_rows(whole, en, x, rows):
    """the first n * bps bytes of each row are the reference's, every other byte of the buffer is still the guard"""
    want = np.full(whole.shape, GUARD_BYTE, np.uint8)
    for b, (n, name) in enumerate(rows):
        line = np.frombuffer(_want(name, x[b, :n]), np.uint8)
        assert line.shape[0] == n * BPS[name]
        want[GUARD + b * en.pitch:GUARD + b * en.pitch + line.shape[0]] = line
    bad = np.nonzero(whole != want)[0]
    assert bad.size == 0, (bad[:8].tolist(), [(int(i - GUARD) // en.pitch, int(i - GUARD) % en.pitch) for i in bad[:8]])


# ---- the stage alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_every_sample_in_every_encoding(eng, ramp, name):
    en = eng.new_encoder(ROWS, W)
    try:
        assert en.pitch == 7680 and en.rows == [(W, "pcm_s16le")] * ROWS
        x = ramp
        if name == "pcm_f32le":  # the bits pass whatever they are
            x = ramp.copy()
            x[3, 5], x[3, 6], x[3, 7] = np.nan, np.inf, -np.inf
            x[4, 0:2] = np.array([0x7FC12345, 0xFFA00001], np.uint32).view(np.float32)  # NaNs with payloads
        rows = [(W, name)] * ROWS
        whole = _encode(eng, en, x, rows)
        _check_rows(whole, en, x, rows)
        got = whole[GUARD:GUARD + ROWS * en.pitch].reshape(ROWS, en.pitch)[:, :W * BPS[name]]
        if name == "pcm_s16le":
            assert np.array_equal(got.copy().view("<i2").reshape(-1)[:65535], g711_ref.ramp()[0])
        if name == "mulaw":
            assert got[0, 0] == 0x00 and got.reshape(-1)[65534] == 0x80 and got.reshape(-1)[32767] == 0xFF
        if name == "alaw":
            assert got[0, 0] == 0x2A and got.reshape(-1)[65534] == 0xAA and got.reshape(-1)[32767] == 0xD5
    finally:
        en.close()


def test_the_clamp_and_nan(eng):
    en = eng.new_encoder(2, 32)
    try:
        x = np.zeros((2, 32), np.float32)
        x[0, :8] = [1.5, -1.5, np.inf, -np.inf, np.nan, 1.0, -1.0, 3e38]
        x[1, :4] = [-0.0, 1e-30, -1e-30, 0.99999]
        for name in ("pcm_s16le", "mulaw", "alaw"):
            rows = [(32, name), (17, name)]
            whole = _encode(eng, en, x, rows)
            _check_rows(whole, en, x, rows)
        s = _encode(eng, en, x, [(32, "pcm_s16le")] * 2)[GUARD:GUARD + 16].copy().view("<i2")
        assert s.tolist() == [32767, -32767, 32767, -32767, -32767, 32767, -32767, 32767]
    finally:
        en.close()


@pytest.mark.parametrize("pinned", [True, False])
def test_ragged_rows_write_nothing_behind_their_bytes(eng, pinned):
    ns = [1, 2, 3, 5, 882, 1919, 1920]
    rng = np.random.default_rng(11)
    x = rng.uniform(-1.2, 1.2, (len(ns), W)).astype(np.float32)
    en = eng.new_encoder(len(ns), W)
    try:
        for shift in range(4):  # every n meets every encoding
            rows = [(n, NAMES[(i + shift) % 4]) for i, n in enumerate(ns)]
            _check_rows(_encode(eng, en, x, rows, pinned), en, x, rows)
    finally:
        en.close()


@pytest.mark.parametrize("pinned", [True, False])
def test_a_width_that_is_no_multiple_of_four(eng, pinned):
    rng = np.random.default_rng(12)
    x = rng.uniform(-1.2, 1.2, (5, 882)).astype(np.float32)
    en = eng.new_encoder(5, 882)
    try:
        assert en.pitch == 3536
        for shift in range(4):
            rows = [(882, NAMES[(i + shift) % 4]) for i in range(5)]
            _check_rows(_encode(eng, en, x, rows, pinned), en, x, rows)
        rows = [(881, "mulaw"), (1, "pcm_f32le"), (866, "pcm_s16le"), (880, "alaw"), (17, "pcm_s16le")]
        _check_rows(_encode(eng, en, x, rows, pinned), en, x, rows)
    finally:
        en.close()


def test_python_refusals(eng):
    en = eng.new_encoder(2, 64)
    try:
        x = torch.zeros(2, 64, device=eng.device)
        good = torch.zeros(2, en.pitch, dtype=torch.uint8, device=eng.device)
        for bad in (torch.zeros(2, 64, dtype=torch.uint8, device=eng.device), torch.zeros(2, en.pitch, device=eng.device),
                    torch.zeros(2, en.pitch, dtype=torch.uint8)):  # the wrong pitch, dtype, and pageable host memory
            with pytest.raises(ValueError, match="encoder output"):
                en.frame(x, bad)
        with pytest.raises(ValueError, match="encoder input"):
            en.frame(torch.zeros(2, 63, device=eng.device), good)
        with pytest.raises(ValueError, match="not configured"):
            en.set_row(0, 8, "opus")
        assert en.rows == [(64, "pcm_s16le")] * 2
    finally:
        en.close()


# ---- in a captured graph ------------------------------------------------------------------------------------------------------
def test_captured_graph_follows_set_row(eng):
    B = 3
    ms = eng.new_mimi_state(B)
    en = eng.new_encoder(B, eng.frame_samples)
    g = None
    try:
        lat = torch.randn(B, eng.ldim, device=eng.device, generator=torch.Generator(eng.device).manual_seed(3))
        pcm = torch.zeros(B, eng.frame_samples, device=eng.device)
        out, big = _guarded(eng, (B, en.pitch))
        rows = [(1920, "pcm_s16le"), (640, "mulaw"), (1919, "pcm_f32le")]
        for b, (n, name) in enumerate(rows):
            en.set_row(b, n, name)
        ms.set_encoder(en, out)
        g = eng.capture_mimi(ms, lat, pcm)
        ms.set_encoder(None)

        def replay(rows):
            big.fill_(GUARD_BYTE)
            eng.graph_launch(g)
            eng.sync()
            torch.cuda.synchronize()
            x = pcm.cpu().numpy()
            assert np.abs(x).max() > 0
            _check_rows(big.cpu().numpy(), en, x, rows)

        replay(rows)
        replay(rows)
        en.set_row(1, 5, "alaw")  # on the engine's stream, after the capture
        rows[1] = (5, "alaw")
        replay(rows)
        en.set_row(2, 1920, "mulaw")
        rows[2] = (1920, "mulaw")
        replay(rows)
        # eager decodes on a state with an encoder append the same launch
        ms.set_encoder(en, out)
        big.fill_(GUARD_BYTE)
        eng.mimi_decode(ms, lat, pcm)
        eng.sync()
        torch.cuda.synchronize()
        _check_rows(big.cpu().numpy(), en, pcm.cpu().numpy(), rows)
        ms.set_encoder(None)
    finally:
        if g is not None:
            eng.graph_destroy(g)
        en.close()
        ms.close()


# ---- against what the other stages already write ---------------------------------------------------------------------------
def test_the_chain_with_the_encoder_against_the_chain_without(eng):
    """resampler (8 kHz) -> leveler (+6 dB) -> encoder against the same chain without the encoder, whose leveler writes
    int16 (`pcm_i16`) or float32 itself: same latents, row by row"""
    from pocket_tts_amd.output_chain import ChainTable, OutputChain

    B = 4
    lats = [torch.randn(B, eng.ldim, device=eng.device, generator=torch.Generator(eng.device).manual_seed(20 + f))
            for f in range(3)]

    def run(encodings, pcm_i16):
        table = ChainTable(eng.sample_rate, eng.frame_samples, [8000], level=True, encodings=encodings)
        ms = eng.new_mimi_state(B)
        chain = OutputChain(eng, B, table, 1, pcm_i16)
        try:
            pcm = torch.zeros(B, eng.frame_samples, device=eng.device)
            for b in range(B):
                route = table.route(sample_rate=8000, gain_db=6, encoding=None if encodings is None else NAMES[b])
                assert route.n_out == 640
                chain.set_row(b, route)
            chain.attach(ms, 0)
            frames, pcms = [], []
            for lat in lats:
                eng.mimi_decode(ms, lat, pcm)
                eng.sync()
                torch.cuda.synchronize()
                frames.append(chain.out[0].numpy().copy())
                pcms.append(pcm.cpu().numpy().copy())
            chain.detach(ms)
            return frames, pcms, chain.out[0].dtype, tuple(chain.out[0].shape)
        finally:
            chain.close()
            ms.close()

    enc, pcm_e, dt, shape = run(NAMES[1:], False)
    assert dt == torch.uint8 and shape == (B, 7680)
    i16, pcm_i, dt, _ = run(None, True)
    assert dt == torch.int16
    f32, pcm_f, dt, _ = run(None, False)
    assert dt == torch.float32
    for f in range(3):
        # the three states decode the same PCM: what follows compares the output stages alone
        assert np.array_equal(pcm_e[f].view(np.uint32), pcm_i[f].view(np.uint32))
        assert np.array_equal(pcm_e[f].view(np.uint32), pcm_f[f].view(np.uint32))
        assert np.abs(i16[f][:, :640]).max() > 0
        assert enc[f][0, :1280].tobytes() == i16[f][0, :640].astype("<i2").tobytes()
        assert enc[f][1, :2560].tobytes() == f32[f][1, :640].astype("<f4").tobytes()
        assert enc[f][2, :640].tobytes() == g711_ref.lin2ulaw(i16[f][2, :640]).tobytes()
        assert enc[f][3, :640].tobytes() == g711_ref.lin2alaw(i16[f][3, :640]).tobytes()
    with pytest.raises(ValueError, match="pcm_i16 and encodings"):
        OutputChain(eng, B, ChainTable(eng.sample_rate, eng.frame_samples, encodings=[]), 1, True)


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


def test_without_encodings_the_launches_are_those_of_the_parent_commit(model, eng):
    """tests/golden/stretch_noop_launches.json holds what the commit before the first output stage records for one eager
    FlowLM step and one codec frame, on the batcher's states and on the `TTSModel` context: built without `encodings`, both
    still record the same launches at the same sites in the same order"""
    from pocket_tts_amd.batching import ContinuousBatcher

    want = json.loads((G / "stretch_noop_launches.json").read_text())
    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    cb = ContinuousBatcher(model, slots=2, capacity=512)
    try:
        cb.submit(state, "ok")
        cb.run_until_idle()
        assert cb.en is None and cb.pipe.en is None and cb.pipe.out is None and cb.pipe.pcm[0].is_pinned()
        got = _step_launches(eng, cb.st, cb.ms)
    finally:
        cb.close()
    assert len(got) == len(want["batcher"]) == 25
    assert [s for s, _ in got] == [s for s, _ in want["batcher"]]
    assert _untuned(got) == _untuned(map(tuple, want["batcher"]))
    model.generate_audio(state, "ok")
    ctxs = [c for k, c in model._ctx_cache.items() if "enc" not in k and "rate" not in k]
    assert ctxs and all(c["pipe"].en is None and c["pipe"].out is None for c in ctxs)
    for c in ctxs:
        got = _step_launches(eng, c["st"], c["ms"])
        assert len(got) == len(want["model"]) == 25
        assert [s for s, _ in got] == [s for s, _ in want["model"]]
        assert _untuned(got) == _untuned(map(tuple, want["model"]))


def test_an_encoder_set_and_cleared_leaves_the_launches_of_before(eng):
    fresh, used = eng.new_mimi_state(2), eng.new_mimi_state(2)
    en = eng.new_encoder(2, eng.frame_samples)
    try:
        want = _step_launches(eng, None, fresh)
        assert want and not any("encode" in s or "encode" in k for s, k in want)
        out = torch.zeros(2, en.pitch, dtype=torch.uint8, device=eng.device)
        used.set_encoder(en, out)
        assert _step_launches(eng, None, used) == want + [("encode", "encode")]
        used.set_encoder(None)
        assert _step_launches(eng, None, used) == want
    finally:
        en.close()
        fresh.close()
        used.close()


# ---- the C ABI's refusals --------------------------------------------------------------------------------------------------
def test_cabi_error_codes(eng):
    import ctypes as C

    lib, sp = eng.lib, eng._sp
    en = eng.new_encoder(2, 64)
    try:
        x = torch.zeros(2, 64, device=eng.device)
        out = torch.full((2, en.pitch), GUARD_BYTE, dtype=torch.uint8, device=eng.device)
        px, po = C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr())
        h = C.c_void_p()
        eng.sync()
        eng.profile_start()
        assert lib.ptts_encoder_create(None, 2, 64, C.byref(h)) == -1 and b"null" in lib.ptts_last_error()
        assert lib.ptts_encoder_create(eng.handle, 2, 64, None) == -1
        assert lib.ptts_encoder_create(eng.handle, 0, 64, C.byref(h)) == -1 and b"out of range" in lib.ptts_last_error()
        assert lib.ptts_encoder_create(eng.handle, 2, 0, C.byref(h)) == -1
        assert lib.ptts_encoder_set_row(None, 0, 1, 0, sp) == -1 and b"null" in lib.ptts_last_error()
        for row in (-1, 2):
            assert lib.ptts_encoder_set_row(en.handle, row, 1, 0, sp) == -1 and b"row out of range" in lib.ptts_last_error()
        for n in (0, -3, 65):
            assert lib.ptts_encoder_set_row(en.handle, 0, n, 0, sp) == -1 and b"[1, 64]" in lib.ptts_last_error(), n
        for code in (4, -1):
            assert lib.ptts_encoder_set_row(en.handle, 0, 1, code, sp) == -1 and b"[0, 3]" in lib.ptts_last_error(), code
        assert lib.ptts_encode_frame(None, px, po, sp) == -1
        assert lib.ptts_encode_frame(en.handle, None, po, sp) == -1
        assert lib.ptts_encode_frame(en.handle, px, None, sp) == -1 and b"null" in lib.ptts_last_error()
        assert lib.ptts_encode_frame(en.handle, px, C.c_void_p(out.data_ptr() + 4), sp) == -1 and b"16 bytes" in lib.ptts_last_error()
        ms = eng.new_mimi_state(3)
        assert lib.ptts_mimi_set_encoder(ms.handle, en.handle, None, po) == -1 and b"batch" in lib.ptts_last_error()  # 3 vs 2
        ms.close()
        ms = eng.new_mimi_state(2)
        assert lib.ptts_mimi_set_encoder(None, en.handle, None, po) == -1
        assert lib.ptts_mimi_set_encoder(ms.handle, en.handle, None, None) == -1 and b"null output" in lib.ptts_last_error()
        # width 64 is not the codec's frame
        assert lib.ptts_mimi_set_encoder(ms.handle, en.handle, None, po) == -1 and b"frame length" in lib.ptts_last_error()
        # an input buffer means "behind another stage": refused on a state that has none
        assert lib.ptts_mimi_set_encoder(ms.handle, en.handle, px, po) == -1 and b"input buffer" in lib.ptts_last_error()
        ms.close()
        assert not any("encode" in r["kernel"] or "encode" in r["site"] for r in eng.profile_stop())  # nothing was launched
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == GUARD_BYTE).all() and en.rows == [(64, "pcm_s16le")] * 2
        assert lib.ptts_abi_version() == 1
    finally:
        en.close()


# ---- through the batcher, the model and the server -------------------------------------------------------------------------
def _convert(name, f32):
    return np.frombuffer(_want(name, f32), {"pcm_s16le": "<i2", "pcm_f32le": "<f4"}.get(name, np.uint8))


def test_batcher_four_encodings_in_flight(model, eng):
    from pocket_tts_amd.batching import ContinuousBatcher

    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    with pytest.raises(ValueError, match="pcm_format and encodings"):
        ContinuousBatcher(model, slots=2, capacity=512, pcm_format="i16", encodings=["mulaw"])
    cb = ContinuousBatcher(model, slots=4, capacity=512, sample_rates=[8000], encodings=NAMES[1:])
    try:
        assert cb.en is not None and cb.pipe.out[0].dtype == torch.uint8 and cb.pipe.out[0].is_pinned()
        with pytest.raises(ValueError, match="not configured"):
            cb.submit(state, TEXT, encoding="opus")
        reqs = {n: cb.submit(state, TEXT, sample_rate=8000, seed=77, temperature=TEMP, encoding=n) for n in NAMES}
        cb.run_until_idle()
        got = {n: torch.cat(list(r)) for n, r in reqs.items()}
    finally:
        cb.close()
    f32 = got["pcm_f32le"].numpy()
    frames = reqs["pcm_f32le"].frames
    assert frames > 3 and f32.shape[0] == frames * 640 and f32.dtype == np.float32 and np.abs(f32).max() > 0.01
    assert [reqs[n].encoding for n in NAMES] == NAMES and all(reqs[n].sample_rate == 8000 for n in NAMES)
    for n, dt in zip(NAMES, (torch.int16, torch.float32, torch.uint8, torch.uint8)):
        assert got[n].dtype == dt and reqs[n].frames == frames and got[n].shape[0] == frames * 640, n
        assert np.array_equal(got[n].numpy(), _convert(n, f32)), n
    cb = ContinuousBatcher(model, slots=2, capacity=512)
    try:
        with pytest.raises(ValueError, match="build it with encodings"):
            cb.submit(state, TEXT, encoding="mulaw")
    finally:
        cb.close()


def test_generate_audio_stream_mulaw(warm, eng):
    model = warm
    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    plain = torch.cat(list(model.generate_audio_stream(state, TEXT, sample_rate=8000, seed=5))).numpy()
    chunks = list(model.generate_audio_stream(state, TEXT, sample_rate=8000, seed=5, encoding="mulaw"))
    assert all(c.dtype == torch.uint8 and 0 < c.shape[0] <= 640 for c in chunks)
    mu = torch.cat(chunks).numpy()
    assert plain.dtype == np.float32 and mu.shape == plain.shape and np.abs(plain).max() > 0.01
    assert np.array_equal(mu, _convert("mulaw", plain))
    # the cached context serves the other encodings
    n_ctx = sum(1 for k in model._ctx_cache if "enc" in k)
    for name in ("alaw", "pcm_s16le", "pcm_f32le"):
        other = model.generate_audio(state, TEXT, sample_rate=8000, seed=5, encoding=name).numpy()
        assert np.array_equal(other, _convert(name, plain)), name
    assert sum(1 for k in model._ctx_cache if "enc" in k) == n_ctx == 1
    with pytest.raises(ValueError, match="not configured"):
        model.generate_audio(state, TEXT, encoding="opus")


def test_server_alaw_and_raw(model, eng, tmp_path):
    import httpx

    from pocket_tts_amd.server import create_app

    shutil.copy(G / "e2e_voice.safetensors", tmp_path / "e2e_voice.safetensors")
    app = create_app(model, slots=2, capacity=512, voices_dir=tmp_path, default_voice="e2e_voice", sample_rates=[8000],
                     encodings=NAMES[1:])
    base = {"text": TEXT, "sample_rate": "8000", "seed": "9", "temperature": str(TEMP)}

    async def go():
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t", timeout=600) as cl:
                # one after the other: each request has the batcher to itself, like the ones it is compared with
                return [await cl.post("/tts", data={**base, **d}) for d in ({"encoding": "alaw"}, {},
                                                                             {"encoding": "alaw", "container": "raw"},
                                                                             {"encoding": "opus"})]

    alaw, pcm, raw, bad = asyncio.run(go())
    assert bad.status_code == 400 and "['pcm_s16le', 'pcm_f32le', 'mulaw', 'alaw']" in bad.json()["detail"]
    assert alaw.status_code == 200 and pcm.status_code == 200 and raw.status_code == 200
    h = alaw.content[:58]
    assert h[:4] == b"RIFF" and struct.unpack_from("<LHHL", h, 16) == (18, 6, 1, 8000) and h[38:42] == b"fact" and h[50:54] == b"data"
    assert pcm.content[:4] == b"RIFF" and struct.unpack_from("<HHL", pcm.content, 20) == (1, 1, 8000)
    s = np.frombuffer(pcm.content[44:], "<i2").astype(np.int64)
    codes = np.frombuffer(alaw.content[58:], np.uint8)
    assert codes.shape == s.shape and s.shape[0] > 1600 + 3 * 640 and np.abs(s).max() > 300
    assert (codes[-1600:] == 0xD5).all() and not s[-1600:].any()
    dec = np.asarray(FIX["alaw2lin"], np.int64)[codes]
    step = 16 << np.maximum((((codes ^ 0x55) >> 4) & 7).astype(np.int64) - 1, 0)  # the A-law step of each code, 16-bit scale
    assert (np.abs(dec - s) <= step).all()
    assert raw.headers["content-type"] == "application/octet-stream" and raw.headers["x-audio-encoding"] == "alaw"
    assert raw.headers["x-sample-rate"] == "8000" and raw.content == alaw.content[58:]
