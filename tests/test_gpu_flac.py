"""The FLAC packer on the GPU (csrc/ptts_flac.hip): every ring line byte for byte against the reference encoder of
`flac_ref.py`, decoded back with its independent decoder; the cut of a row's pre-roll on the device; frame numbers; captured
graphs that follow `set_row`; and a flac request through the batcher, the model and the server, whose decoded stream must be
the int16 samples the same request delivers as pcm_s16le."""

import asyncio
import shutil
from pathlib import Path

import numpy as np
import pytest
import torch

import flac_ref
import g711_ref
from test_flac_cpu import NS, signals

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"
GUARD_BYTE = 0xA5
TEXT = "Hello world. This is a test."
TEMP = 0.7


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
    model.temp = TEMP
    yield model
    model.temp = 0.0


def _ceil16(v):
    return (v + 15) // 16 * 16


def _run_lines(eng, pk, lines, pinned=True):
    """`lines`: uint8 [L, B, in_pitch], the encoder's bytes of L frames.  Each through `pk` into a ring slot filled with the
    guard byte: [L, B, pitch] as numpy"""
    out = torch.full((pk.batch, pk.pitch), GUARD_BYTE, dtype=torch.uint8)
    out = out.pin_memory() if pinned else out.to(eng.device)
    got = []
    for line in lines:
        x = torch.from_numpy(np.ascontiguousarray(line)).to(eng.device)
        out.fill_(GUARD_BYTE)
        torch.cuda.synchronize()
        pk.frame(x, out)
        eng.sync()
        torch.cuda.synchronize()
        got.append(out.cpu().numpy().copy())
    return np.stack(got)


def _check_line(line, want: bytes, pad=None):
    """a ring line: the prefix, `want`, up to the next 16 bytes zeros (or `pad`), then the guard"""
    n = len(want)
    assert int.from_bytes(line[:4].tobytes(), "little") == n and not line[4:16].any()
    assert line[16:16 + n].tobytes() == want
    end = 16 + _ceil16(n)
    if n:
        assert line[16 + n:end].tobytes() == (bytes(end - 16 - n) if pad is None else pad)
    assert (line[end:] == GUARD_BYTE).all()


def _as_bytes(rows, in_pitch):
    """int16 rows of any length -> uint8 [B, in_pitch], each at the start of its line, the rest 0x5A"""
    buf = np.full((len(rows), in_pitch), 0x5A, np.uint8)
    for b, x in enumerate(rows):
        raw = np.frombuffer(np.ascontiguousarray(x, "<i2").tobytes(), np.uint8)
        buf[b, :raw.shape[0]] = raw
    return buf


# ---- the stage alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pinned", [True, False])
def test_every_signal_at_every_block_size(eng, pinned):
    B, W = 7, 4608
    rates = (8000, 16000, 8000, 11025, 24000, 48000)
    sigs = [list(signals(n).values()) for n in NS]
    pk = eng.new_packer(B, W)
    try:
        assert pk.pitch == 16 + 4 * W and pk.in_pitch == 4 * W
        for b, n in enumerate(NS):
            pk.set_row(b, n, None, "flac", 0, 0, rates[b])
        pk.set_row(6, 1001, "mulaw")
        rng = np.random.default_rng(1)
        lines = []
        for f in range(7):  # line f: row b holds its signal (f + b) % 7; the pass-through row random bytes
            buf = _as_bytes([sigs[b][(f + b) % 7] for b in range(6)] + [np.zeros(0, np.int16)], pk.in_pitch)
            buf[6] = rng.integers(0, 256, pk.in_pitch, dtype=np.uint8)
            lines.append(buf)
        got = _run_lines(eng, pk, lines, pinned)
        kinds = set()
        for f in range(7):
            for b, n in enumerate(NS):
                x = sigs[b][(f + b) % 7]
                want = flac_ref.encode_frame(x, f, rates[b])
                assert len(want) <= 2 * n + 18
                _check_line(got[f, b], want)
                y, number, rate, block, used, kind = flac_ref.decode_frame(got[f, b, 16:16 + len(want)].tobytes())
                assert np.array_equal(y, x) and (number, rate, block, used) == (f, rates[b], n, len(want))
                kinds.add(kind)
            _check_line(got[f, 6], lines[f][6, :1001].tobytes(), pad=lines[f][6, 1001:1008].tobytes())
        assert kinds == {"constant", "verbatim", "fixed"}
    finally:
        pk.close()


def test_preroll_is_cut_on_the_device(eng):
    n, prerolls, L = 640, (0, 1, 639, 640, 1000), 6
    pk = eng.new_packer(len(prerolls), n)
    try:
        seq = [np.concatenate([signals(n, seed=10 * b + f)["ar2" if (f + b) % 3 else "sine"] for f in range(L)])
               for b in range(len(prerolls))]
        for b, p in enumerate(prerolls):
            pk.set_row(b, n, "pcm_s16le", "flac", p, 3, 8000)
        lines = [_as_bytes([s[f * n:(f + 1) * n] for s in seq], pk.in_pitch) for f in range(L)]
        got = _run_lines(eng, pk, lines)
        for b, p in enumerate(prerolls):
            lead = -(-p // n)
            for f in range(L):
                if f < lead:
                    _check_line(got[f, b], b"")
                    continue
                block = seq[b][p + (f - lead) * n:p + (f - lead + 1) * n]
                _check_line(got[f, b], flac_ref.encode_frame(block, 3 + f - lead, 8000))
            nbytes = [int.from_bytes(got[f, b, :4].tobytes(), "little") for f in range(L)]
            stream = b"".join(got[f, b, 16:16 + nbytes[f]].tobytes() for f in range(L))
            pcm = np.concatenate([fr[0] for fr in flac_ref.decode_frames(stream)])
            assert np.array_equal(pcm, seq[b][p:p + (L - lead) * n])
        # set_row puts the line counter back: the row leads again
        pk.set_row(4, n, None, "flac", 1000, 0, 8000)
        again = _run_lines(eng, pk, lines[:3])
        assert [int.from_bytes(again[f, 4, :4].tobytes(), "little") > 0 for f in range(3)] == [False, False, True]
        _check_line(again[2, 4], flac_ref.encode_frame(seq[4][1000:1640], 0, 8000))
    finally:
        pk.close()


def test_first_block_across_the_number_lengths(eng):
    n = 64
    pk = eng.new_packer(2, n)
    try:
        for b, first in enumerate((127, 2047)):
            pk.set_row(b, n, None, "flac", 0, first, 22050)
        x = [signals(n, seed=s)["ar2"] for s in range(4)]
        got = _run_lines(eng, pk, [_as_bytes(x[:2], pk.in_pitch), _as_bytes(x[2:], pk.in_pitch)])
        for f in range(2):
            for b, first in enumerate((127, 2047)):
                want = flac_ref.encode_frame(x[2 * f + b], first + f, 22050)
                _check_line(got[f, b], want)
        assert got[0, 0, 16 + 4] == 127 and got[1, 0, 16 + 4:16 + 6].tobytes() == b"\xc2\x80"
        assert got[0, 1, 16 + 4:16 + 6].tobytes() == b"\xdf\xbf" and got[1, 1, 16 + 4:16 + 7].tobytes() == b"\xe0\xa0\x80"
    finally:
        pk.close()


def test_python_refusals(eng):
    pk = eng.new_packer(2, 640)
    try:
        with pytest.raises(ValueError, match="16 to 4608"):
            pk.set_row(0, 15, None, "flac", 0, 0, 8000)
        with pytest.raises(ValueError, match="pcm_s16le"):
            pk.set_row(0, 640, "mulaw", "flac", 0, 0, 8000)
        with pytest.raises(ValueError, match="not configured"):
            pk.set_row(0, 640, None, "mp3", 0, 0, 8000)
        with pytest.raises(ValueError, match="uint8"):
            pk.frame(torch.zeros(2, pk.in_pitch, device=eng.device), torch.zeros(2, pk.pitch, dtype=torch.uint8, device=eng.device))
        with pytest.raises(ValueError, match="pinned"):
            pk.frame(torch.zeros(2, pk.in_pitch, dtype=torch.uint8, device=eng.device), torch.zeros(2, pk.pitch, dtype=torch.uint8))
        assert pk.rows == [(640, "pcm_s16le", None, 0, 0, None)] * 2
    finally:
        pk.close()


# ---- behind the codec ---------------------------------------------------------------------------------------------------
def test_captured_graph_follows_set_row(eng):
    B, W = 3, eng.frame_samples
    ms = eng.new_mimi_state(B)
    en, pk = eng.new_encoder(B, W), eng.new_packer(B, W)
    g = None
    try:
        lat = torch.randn(B, eng.ldim, device=eng.device, generator=torch.Generator(eng.device).manual_seed(3))
        pcm = torch.zeros(B, W, device=eng.device)
        mid = torch.zeros(B, en.pitch, dtype=torch.uint8, device=eng.device)
        out = torch.full((B, pk.pitch), GUARD_BYTE, dtype=torch.uint8).pin_memory()
        rows = [(1920, None, "flac", 24000), (640, "mulaw", None, None), (1919, None, "flac", 12345)]
        count = [0, 0, 0]

        def deal(b, row):
            rows[b], count[b] = row, 0
            n, enc, comp, rate = row
            en.set_row(b, n, enc)
            pk.set_row(b, n, enc, comp, 0, 40 * b, rate)

        for b, row in enumerate(rows):
            deal(b, row)
        ms.set_encoder(en, mid)
        ms.set_packer(pk, out, mid)
        g = eng.capture_mimi(ms, lat, pcm)
        ms.set_packer(None)
        ms.set_encoder(None)

        def check():
            x = pcm.cpu().numpy()
            assert np.abs(x).max() > 0
            s = g711_ref.s16(x)
            line = out.numpy()
            for b, (n, enc, comp, rate) in enumerate(rows):
                if comp is None:
                    want = g711_ref.lin2ulaw(s[b, :n]).tobytes()
                    assert int.from_bytes(line[b, :4].tobytes(), "little") == n and line[b, 16:16 + n].tobytes() == want
                    assert (line[b, 16 + _ceil16(n):] == GUARD_BYTE).all()
                else:
                    _check_line(line[b], flac_ref.encode_frame(s[b, :n].astype(np.int16), 40 * b + count[b], rate))
                count[b] += 1

        def replay():
            out.fill_(GUARD_BYTE)
            eng.graph_launch(g)
            eng.sync()
            torch.cuda.synchronize()
            check()

        replay()
        replay()
        deal(1, (640, None, "flac", 8000))  # on the engine's stream, after the capture
        replay()
        deal(2, (1920, "mulaw", None, None))
        deal(0, (17, None, "flac", 48000))
        replay()
        # eager decodes on a state with both links append the same launches
        ms.set_encoder(en, mid)
        ms.set_packer(pk, out, mid)
        out.fill_(GUARD_BYTE)
        eng.mimi_decode(ms, lat, pcm)
        eng.sync()
        torch.cuda.synchronize()
        check()
        ms.set_packer(None)
        ms.set_encoder(None)
    finally:
        if g is not None:
            eng.graph_destroy(g)
        pk.close()
        en.close()
        ms.close()


def test_cabi_refusals_come_before_any_launch(eng):
    import ctypes as C

    lib, sp = eng.lib, eng._sp
    W = eng.frame_samples
    pk, en = eng.new_packer(2, W), eng.new_encoder(2, W)
    small = eng.new_packer(2, 64)
    try:
        x = torch.zeros(2, pk.in_pitch, dtype=torch.uint8, device=eng.device)
        out = torch.full((2, pk.pitch), GUARD_BYTE, dtype=torch.uint8, device=eng.device)
        lat = torch.zeros(2, eng.ldim, device=eng.device)
        pcm = torch.zeros(2, W, device=eng.device)
        px, po = C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr())
        h = C.c_void_p()
        eng.sync()
        eng.profile_start()
        assert lib.ptts_flac_create(None, 2, 64, C.byref(h)) == -1 and b"null" in lib.ptts_last_error()
        assert lib.ptts_flac_create(eng.handle, 2, 64, None) == -1
        assert lib.ptts_flac_create(eng.handle, 0, 64, C.byref(h)) == -1 and b"out of range" in lib.ptts_last_error()
        assert lib.ptts_flac_create(eng.handle, 2, 0, C.byref(h)) == -1
        assert lib.ptts_flac_set_row(None, 0, 0, 1, 2, 0, 0, 0, sp) == -1 and b"null" in lib.ptts_last_error()
        for row in (-1, 2):
            assert lib.ptts_flac_set_row(pk.handle, row, 1, 640, 2, 8000, 0, 0, sp) == -1 and b"row out of range" in lib.ptts_last_error()
        for n in (0, 15, W + 1):
            assert lib.ptts_flac_set_row(pk.handle, 0, 1, n, 2, 8000, 0, 0, sp) == -1 and f"[16, {W}]".encode() in lib.ptts_last_error(), n
        assert lib.ptts_flac_set_row(small.handle, 0, 1, 65, 2, 8000, 0, 0, sp) == -1 and b"[16, 64]" in lib.ptts_last_error()
        for n in (0, W + 1):
            assert lib.ptts_flac_set_row(pk.handle, 0, 0, n, 2, 0, 0, 0, sp) == -1 and f"[1, {W}]".encode() in lib.ptts_last_error(), n
        assert lib.ptts_flac_set_row(pk.handle, 0, 0, 64, 3, 0, 0, 0, sp) == -1 and b"1, 2 or 4" in lib.ptts_last_error()
        assert lib.ptts_flac_set_row(pk.handle, 0, 2, 64, 2, 8000, 0, 0, sp) == -1 and b"mode" in lib.ptts_last_error()
        for rate in (0, 65536):
            assert lib.ptts_flac_set_row(pk.handle, 0, 1, 64, 2, rate, 0, 0, sp) == -1 and b"[1, 65535]" in lib.ptts_last_error()
        assert lib.ptts_flac_set_row(pk.handle, 0, 1, 64, 2, 8000, -1, 0, sp) == -1 and b"pre-roll" in lib.ptts_last_error()
        assert lib.ptts_flac_set_row(pk.handle, 0, 1, 64, 2, 8000, 0, -1, sp) == -1 and b"first block" in lib.ptts_last_error()
        assert lib.ptts_flac_frame(None, px, po, sp) == -1
        assert lib.ptts_flac_frame(pk.handle, None, po, sp) == -1
        assert lib.ptts_flac_frame(pk.handle, px, None, sp) == -1 and b"null" in lib.ptts_last_error()
        assert lib.ptts_flac_frame(pk.handle, px, C.c_void_p(out.data_ptr() + 4), sp) == -1 and b"16 bytes" in lib.ptts_last_error()
        ms = eng.new_mimi_state(2)
        assert lib.ptts_mimi_set_packer(None, pk.handle, px, po) == -1
        assert lib.ptts_mimi_set_packer(ms.handle, pk.handle, px, None) == -1 and b"null output" in lib.ptts_last_error()
        # a packer without an encoder on the state
        assert lib.ptts_mimi_set_packer(ms.handle, pk.handle, px, po) == -1 and b"needs an encoder" in lib.ptts_last_error()
        ms.set_encoder(en, x)
        assert lib.ptts_mimi_set_packer(ms.handle, pk.handle, None, po) == -1 and b"null input" in lib.ptts_last_error()
        assert lib.ptts_mimi_set_packer(ms.handle, small.handle, px, po) == -1 and b"width" in lib.ptts_last_error()
        # the encoder leaves, or writes another buffer: the frame is refused before the codec's first launch
        assert lib.ptts_mimi_set_packer(ms.handle, pk.handle, px, po) == 0
        ms.set_encoder(None)
        assert lib.ptts_mimi_decode(eng.handle, ms.handle, C.c_void_p(lat.data_ptr()), C.c_void_p(pcm.data_ptr()), sp) == -1
        assert b"no encoder" in lib.ptts_last_error()
        other = torch.zeros_like(x)
        ms.set_encoder(en, other)
        assert lib.ptts_mimi_decode(eng.handle, ms.handle, C.c_void_p(lat.data_ptr()), C.c_void_p(pcm.data_ptr()), sp) == -1
        assert b"not the buffer" in lib.ptts_last_error()
        assert lib.ptts_mimi_set_packer(ms.handle, None, None, None) == 0
        ms.set_encoder(None)
        ms.close()
        ms = eng.new_mimi_state(3)
        en3 = eng.new_encoder(3, W)
        x3 = torch.zeros(3, en3.pitch, dtype=torch.uint8, device=eng.device)
        ms.set_encoder(en3, x3)
        assert lib.ptts_mimi_set_packer(ms.handle, pk.handle, px, po) == -1 and b"batch" in lib.ptts_last_error()  # 2 vs 3
        ms.set_encoder(None)
        en3.close()
        ms.close()
        recs = eng.profile_stop()  # nothing was launched: no packer kernel, and no kernel of a codec frame
        assert not [r for r in recs if "flac" in r["kernel"] or r["site"]]
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == GUARD_BYTE).all() and pk.rows == [(W, "pcm_s16le", None, 0, 0, None)] * 2
    finally:
        small.close()
        en.close()
        pk.close()


# ---- through the batcher, the model and the server -------------------------------------------------------------------------
def _frames_of(chunks):
    """the uint8 chunks of a flac request, one frame each: (samples, numbers)"""
    assert all(c.dtype == torch.uint8 and c.ndim == 1 for c in chunks)
    frames = [flac_ref.decode_frames(c.numpy().tobytes()) for c in chunks]
    assert all(len(f) == 1 for f in frames)  # one uint8 chunk per frame
    return np.concatenate([f[0][0] for f in frames]), [f[0][1] for f in frames], frames


def test_batcher_flac_against_pcm_s16le(model, eng):
    from pocket_tts_amd.batching import ContinuousBatcher
    from pocket_tts_amd.tts_model import split_into_best_sentences

    m = model
    assert len(split_into_best_sentences(m.tokenizer.encode, m.tokenizer.sp, TEXT, 8, m.pad_with_spaces_for_short_inputs,
                                         m.remove_semicolons)) == 2
    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    with pytest.raises(ValueError, match="pcm_format and encodings"):
        ContinuousBatcher(model, slots=2, capacity=512, pcm_format="i16", compressions=["flac"])
    cb = ContinuousBatcher(model, slots=2, capacity=512, sample_rates=[8000], level=True, compressions=["flac"])
    try:
        assert cb.pk is not None and cb.en is not None and cb.pipe.out[0].shape[1] == 16 + 4 * 1920
        with pytest.raises(ValueError, match="not configured"):
            cb.submit(state, TEXT, compression="mp3")
        kw = dict(sample_rate=8000, seed=77, temperature=TEMP, gain_db=6, max_tokens=8)
        plain = cb.submit(state, TEXT, encoding="pcm_s16le", **kw)
        comp = cb.submit(state, TEXT, compression="flac", **kw)
        assert cb.chain.table.route(sample_rate=8000, gain_db=6).preroll % 640 != 0  # the cut is inside a line
        cb.run_until_idle()
        want = torch.cat(list(plain)).numpy()
        chunks = list(comp)
    finally:
        cb.close()
    assert comp.compression == "flac" and plain.compression is None and comp.sample_rate == 8000
    pcm, numbers, frames = _frames_of(chunks)
    assert want.dtype == np.int16 and plain.frames > 6 and want.shape[0] == plain.frames * 640 and np.abs(want).max() > 300
    assert numbers == list(range(plain.frames)) and comp.blocks == plain.frames  # consecutive across the two text chunks
    assert all(f[0][2] == 8000 and f[0][3] == 640 for f in frames)
    assert np.array_equal(pcm, want)
    ratio = sum(c.shape[0] for c in chunks) / (2.0 * want.shape[0])
    print(f"flac bytes / pcm_s16le bytes on the tiny model's audio: {ratio:.3f}")
    assert all(c.shape[0] <= 2 * 640 + 18 for c in chunks)
    cb = ContinuousBatcher(model, slots=2, capacity=512)
    try:
        with pytest.raises(ValueError, match="build it with\\s+compressions"):
            cb.submit(state, TEXT, compression="flac")
    finally:
        cb.close()


def test_generate_audio_stream_flac(warm, eng):
    from pocket_tts_amd.main import flac_stream_bytes

    model = warm
    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    kw = dict(sample_rate=8000, seed=5, gain_db=6, max_tokens=8)
    want = torch.cat(list(model.generate_audio_stream(state, TEXT, encoding="pcm_s16le", **kw))).numpy()
    chunks = list(model.generate_audio_stream(state, TEXT, compression="flac", **kw))
    pcm, numbers, _ = _frames_of(chunks)
    assert want.dtype == np.int16 and want.shape[0] % 640 == 0 and np.abs(want).max() > 300
    assert numbers == list(range(want.shape[0] // 640)) and np.array_equal(pcm, want)
    whole, rate, info = flac_ref.decode_stream(b"".join(flac_stream_bytes(chunks, 8000, 640)))
    assert rate == 8000 and np.array_equal(whole, np.concatenate([want, np.zeros(1600, np.int16)]))
    with pytest.raises(ValueError, match="pcm_s16le"):
        model.generate_audio(state, TEXT, encoding="mulaw", compression="flac")


def test_generate_audio_batch_flac(model, eng):
    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    texts = ["Hello world.", "This is a test."]
    plain = model.generate_audio_batch(state, texts)  # temp 0: the same latents in both calls
    packed = model.generate_audio_batch(state, texts, compression="flac")
    for f32, chunks in zip(plain, packed):
        pcm, numbers, frames = _frames_of(chunks)
        assert f32.shape[0] >= 3 * 1920 and numbers == list(range(f32.shape[0] // 1920))
        assert all(f[0][2] == 24000 and f[0][3] == 1920 for f in frames)
        assert np.array_equal(pcm, g711_ref.s16(f32.numpy()))
    with pytest.raises(TypeError, match="compression"):
        model.generate_audio_batch(state, texts, encoding="mulaw")
    with pytest.raises(ValueError, match="not configured"):
        model.generate_audio_batch(state, texts, compression="mp3")


def test_server_container_flac(model, eng, tmp_path):
    import httpx

    from pocket_tts_amd.server import create_app

    shutil.copy(G / "e2e_voice.safetensors", tmp_path / "e2e_voice.safetensors")
    app = create_app(model, slots=2, capacity=512, voices_dir=tmp_path, default_voice="e2e_voice", sample_rates=[8000],
                     level=True, encodings=["mulaw"], compressions=["flac"])
    base = {"text": TEXT, "sample_rate": "8000", "seed": "9", "temperature": str(TEMP), "gain_db": "6"}

    async def go():
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t", timeout=600) as cl:
                # one after the other: each request has the batcher to itself, like the one it is compared with
                return [await cl.post("/tts", data={**base, **d}) for d in ({"container": "flac"}, {},
                                                                             {"container": "flac", "encoding": "mulaw"})]

    fl, wav, bad = asyncio.run(go())
    assert bad.status_code == 400 and "pcm_s16le" in bad.json()["detail"]
    assert fl.status_code == 200 and fl.headers["content-type"] == "audio/flac" and wav.status_code == 200
    pcm, rate, info = flac_ref.decode_stream(fl.content)
    s = np.frombuffer(wav.content[44:], "<i2")
    assert rate == 8000 and info["block"] == 640 and info["total"] == 0
    assert s.shape[0] > 1600 + 3 * 640 and np.abs(s.astype(np.int64)).max() > 300 and not s[-1600:].any()
    assert np.array_equal(pcm, s)
    assert [f[5] for f in info["frames"][-3:]] == ["constant"] * 3 and info["frames"][-1][3] == 1600 - 2 * 640
