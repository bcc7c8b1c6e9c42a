"""The HTTP server (pocket_tts_amd/server.py) on the GPU, driven in-process (httpx.ASGITransport, no socket): concurrent
requests joining and leaving a 4-slot batch, per-request sampling settings, voice uploads, request validation, and the
`export-voice` command."""

import asyncio
import io
import math
import shutil
import subprocess
import sys
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"
REPO = Path(__file__).resolve().parents[1]
TOL = math.ceil(5e-4 * 32767) + 1  # the batcher-vs-single waveform tolerance in int16 steps
TEXTS = ["Hello world. This is a test.", "ok", "This is a longer sentence, with several clauses, to test it.",
         "How are you today?", "Short one.", "Another request arrives while the others are running."]


@pytest.fixture(scope="module")
def fx():
    import ast

    z = np.load(G / "e2e_tiny.npz", allow_pickle=False)
    d = {k: z[k] for k in z.files}
    d["meta"] = ast.literal_eval(str(d["meta"]))
    return d


@pytest.fixture(scope="module")
def model():
    from pocket_tts_amd import TTSModel

    m = TTSModel.load_model(config=G / "e2e_tiny.yaml", temp=0.0)
    yield m
    m.engine.close()


@pytest.fixture(scope="module")
def voices(tmp_path_factory):
    d = tmp_path_factory.mktemp("voices")
    shutil.copy(G / "e2e_voice.safetensors", d / "e2e_voice.safetensors")
    return d


def _wav_file(path, fx):
    pcm = (np.clip(fx["e2e_audio"][0], -1, 1) * 32767).astype(np.int16)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(24000); w.writeframes(pcm.tobytes())
    return path


def _multipart(fields, files, boundary="pocket-boundary-7"):
    out = b""
    for k, v in fields.items():
        out += f"--{boundary}\r\nContent-Disposition: form-data; name=\"{k}\"\r\n\r\n{v}\r\n".encode()
    for k, (fn, data) in files.items():
        out += (f"--{boundary}\r\nContent-Disposition: form-data; name=\"{k}\"; filename=\"{fn}\"\r\n"
                "Content-Type: audio/wav\r\n\r\n").encode() + data + b"\r\n"
    return f"multipart/form-data; boundary={boundary}", out + f"--{boundary}--\r\n".encode()


def _serve(model, voices, posts, slots=4, capacity=512, gets=("/health",)):
    """runs the app's lifespan, sends every GET, then every POST at once; returns (gets, posts) responses"""
    import httpx

    from pocket_tts_amd.server import create_app

    app = create_app(model, slots=slots, capacity=capacity, voices_dir=voices, default_voice="e2e_voice")

    async def go():
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t", timeout=600) as cl:
                g = [await cl.get(u) for u in gets]

                async def post(p):
                    if isinstance(p, tuple):
                        return await cl.post("/tts", content=p[1], headers={"content-type": p[0]})
                    return await cl.post("/tts", data=p)

                return g, await asyncio.gather(*[post(p) for p in posts])

    return asyncio.run(go())


def _samples(body: bytes) -> np.ndarray:
    assert body[:4] == b"RIFF" and body[8:16] == b"WAVEfmt " and body[36:40] == b"data"
    with wave.open(io.BytesIO(body), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 24000)
    return np.frombuffer(body[44:], dtype=np.int16)


def _check_against(body, ref):
    x = _samples(body)
    n = ref.shape[0]
    assert x.shape[0] == n + 4800, (x.shape[0], n)
    assert np.all(x[n:] == 0)
    want = (ref.clamp(-1, 1) * 32767).short().numpy().astype(np.int32)
    assert np.abs(x[:n].astype(np.int32) - want).max() <= TOL


def test_health_and_concurrent_requests_match_single_generation(model, voices):
    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    refs = [model.generate_audio(state, t) for t in TEXTS]
    assert len({r.shape[0] for r in refs}) > 1
    (health,), res = _serve(model, voices, [{"text": t, "temperature": "0"} for t in TEXTS])
    assert health.status_code == 200 and health.json() == {"status": "healthy"}
    for t, r, ref in zip(TEXTS, res, refs):
        assert r.status_code == 200 and r.headers["content-type"] == "audio/wav", (t, r.text[:200])
        _check_against(r.content, ref)


def test_mixed_sampling_settings_in_one_batch(model, voices):
    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    ref = model.generate_audio(state, TEXTS[0])
    posts = [{"text": TEXTS[0], "temperature": "0"},
             {"text": TEXTS[0], "temperature": "0.7"},
             {"text": TEXTS[0], "temperature": "0.7", "noise_clamp": "0.5", "eos_threshold": "-3.0"},
             {"text": TEXTS[3], "voice_url": "e2e_voice", "frames_after_eos": "1"}]
    _, res = _serve(model, voices, posts)
    assert [r.status_code for r in res] == [200] * 4
    _check_against(res[0].content, ref)
    for r in res[1:]:
        x = _samples(r.content)
        assert x.shape[0] > 4800 and (x.shape[0] - 4800) % 1920 == 0 and np.all(x[-4800:] == 0)
    # noise reached the sampled requests: their audio differs from the temperature-0 one
    a, b = _samples(res[0].content), _samples(res[1].content)
    m = min(a.shape[0], b.shape[0]) - 4800
    assert not np.array_equal(a[:m], b[:m])


def test_uploaded_voice(model, voices, fx, tmp_path):
    path = _wav_file(tmp_path / "prompt.wav", fx)
    ref = model.generate_audio(model.get_state_for_audio_prompt(path, truncate=True), TEXTS[0])
    ct, body = _multipart({"text": TEXTS[0], "temperature": "0"}, {"voice_wav": ("prompt.wav", path.read_bytes())})
    _, (r, r2) = _serve(model, voices, [(ct, body), {"text": TEXTS[4], "temperature": "0"}])
    assert r.status_code == 200 and r2.status_code == 200, r.text[:200]
    _check_against(r.content, ref)


def test_bad_requests_get_400(model, voices, fx, tmp_path):
    wav = _wav_file(tmp_path / "p.wav", fx).read_bytes()
    both = _multipart({"text": "hi", "voice_url": "e2e_voice"}, {"voice_wav": ("p.wav", wav)})
    garbage = _multipart({"text": "hi"}, {"voice_wav": ("p.wav", b"RIFF\x00\x01garbage")})
    posts = [{"text": "  "}, both,
             {"text": "hi", "voice_url": "https://example.com/v.safetensors"},
             {"text": "hi", "voice_url": "hf://kyutai/tts-voices/alba.safetensors"},
             {"text": "hi", "voice_url": "not_a_voice"},
             {"text": "hi", "temperature": "warm"}, {"text": "hi", "temperature": "-0.5"},
             {"text": "hi", "noise_clamp": "-2"}, {"text": "hi", "eos_threshold": "nan"},
             {"text": "hi", "frames_after_eos": "x"},
             {"text": TEXTS[2]},  # needs more KV positions than the 64 of a slot
             garbage]
    (health,), res = _serve(model, voices, posts, slots=2, capacity=64)
    assert health.status_code == 200
    assert [r.status_code for r in res] == [400] * len(posts), [r.text[:120] for r in res]
    assert "slot capacity" in res[10].json()["detail"]
    assert "runs offline" in res[2].json()["detail"]


def test_export_voice_command(model, fx, tmp_path):
    import safetensors.torch

    from pocket_tts_amd.tts_model import export_model_state

    wav = _wav_file(tmp_path / "prompt.wav", fx)
    out = tmp_path / "voice.safetensors"
    r = subprocess.run([sys.executable, "-m", "pocket_tts_amd", "export-voice", str(wav), str(out),
                        "--config", str(G / "e2e_tiny.yaml"), "-q"], cwd=REPO, timeout=600, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    export_model_state(model.get_state_for_audio_prompt(wav, truncate=True), tmp_path / "ref.safetensors")
    got, ref = safetensors.torch.load_file(str(out)), safetensors.torch.load_file(str(tmp_path / "ref.safetensors"))
    assert got.keys() == ref.keys()
    for k in ref:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
        assert torch.allclose(got[k].float(), ref[k].float(), atol=1e-5, rtol=0), k
    # `generate --voice` accepts it
    wav_out = model.generate_audio(model.get_state_for_audio_prompt(str(out)), "Short one.")
    assert wav_out.shape[0] > 0 and wav_out.shape[0] % 1920 == 0
