"""The HTTP server's host side without a GPU: form parsing, request validation against a stub model and batcher, the
WAV byte stream shared with the CLI, the `serve` / `export-voice` flags, and the numpy restatement of the device's
truncated-normal noise."""

import asyncio
import io
import sys
import wave

import numpy as np
import pytest
import torch

from noise_ref import counter_normal, counter_trunc_normal


# ---- WAV framing -------------------------------------------------------------------------------------------------
def _old_write_wav_stream(out, chunks, sample_rate, stream):
    """write_wav_stream before the framing was factored out (wave module; unseekable output keeps its header)"""
    w = wave.open(out, "wb")
    w.setnchannels(1)
    w.setsampwidth(2)
    w.setframerate(sample_rate)
    w.setnframes(1_000_000_000)
    for chunk in chunks:
        w.writeframesraw((chunk.clamp(-1, 1) * 32767).short().cpu().numpy().tobytes())
    w.writeframesraw(bytes(2 * int(sample_rate * 0.2)))
    if stream:
        w._patchheader = lambda: None
    w.close()


def _chunks():
    g = torch.Generator().manual_seed(0)
    return [torch.randn(1920, generator=g) * 0.7 for _ in range(5)] + [torch.full((1920,), 3.0), torch.zeros(7)]


def test_wav_stream_bytes_equal_the_cli_stream():
    from pocket_tts_amd.main import wav_stream_bytes

    ref = io.BytesIO()
    _old_write_wav_stream(ref, _chunks(), 24000, stream=True)
    got = b"".join(wav_stream_bytes(iter(_chunks()), 24000))
    assert got == ref.getvalue()
    # int16 chunks (the batcher's pcm_format="i16") are framed as they are
    i16 = [(c.clamp(-1, 1) * 32767).short() for c in _chunks()]
    assert b"".join(wav_stream_bytes(iter(i16), 24000)) == got


def test_write_wav_stream_file_is_byte_identical(tmp_path):
    from pocket_tts_amd.main import write_wav_stream

    ref = io.BytesIO()
    _old_write_wav_stream(ref, _chunks(), 24000, stream=False)
    n = write_wav_stream(str(tmp_path / "a.wav"), iter(_chunks()), 24000)
    assert (tmp_path / "a.wav").read_bytes() == ref.getvalue()
    assert n == 6 * 1920 + 7 + 4800


# ---- form parsing ------------------------------------------------------------------------------------------------
def _multipart(fields, files, boundary="XyZ-boundary-123"):
    out = b""
    for k, v in fields.items():
        out += f"--{boundary}\r\nContent-Disposition: form-data; name=\"{k}\"\r\n\r\n".encode() + v.encode() + b"\r\n"
    for k, (fn, data) in files.items():
        out += (f"--{boundary}\r\nContent-Disposition: form-data; name=\"{k}\"; filename=\"{fn}\"\r\n"
                "Content-Type: audio/wav\r\n\r\n").encode() + data + b"\r\n"
    out += f"--{boundary}--\r\n".encode()
    return f"multipart/form-data; boundary={boundary}", out


def test_parse_form_urlencoded():
    from pocket_tts_amd.server import parse_form

    f, files = parse_form("application/x-www-form-urlencoded", b"text=Hello+w%C3%B6rld%21&voice_url=alba&temperature=")
    assert f == {"text": "Hello wörld!", "voice_url": "alba", "temperature": ""} and files == {}
    f, _ = parse_form("application/x-www-form-urlencoded; charset=utf-8", b"")
    assert f == {}


def test_parse_form_multipart_with_binary_file():
    from pocket_tts_amd.server import parse_form

    blob = bytes(np.random.default_rng(0).integers(0, 256, 5000, dtype=np.uint8)) + b"\r\n--XyZ\r\n\r\n\r"
    ct, body = _multipart({"text": "héllo\r\nthere", "eos_threshold": "-3.5"}, {"voice_wav": ("v.wav", blob)})
    f, files = parse_form(ct, body)
    assert f == {"text": "héllo\r\nthere", "eos_threshold": "-3.5"}
    assert files == {"voice_wav": ("v.wav", blob)}


@pytest.mark.parametrize("ct,body", [
    ("text/plain", b"text=hi"),
    (None, b"text=hi"),
    ("application/x-www-form-urlencoded", b"\xff\xfe"),
    ("application/x-www-form-urlencoded", b"text"),
    ("multipart/form-data", b"--x\r\n\r\nhi\r\n--x--"),                                   # no boundary
    ("multipart/form-data; boundary=x", b"--x\r\nContent-Disposition: form-data; name=\"text\"\r\n\r\nhi"),  # not closed
    ("multipart/form-data; boundary=x", b"--x\r\nContent-Disposition: form-data\r\n\r\nhi\r\n--x--"),      # no name
    ("multipart/form-data; boundary=x", b"--x\r\nX-Other: 1\r\n\r\nhi\r\n--x--"),                        # no disposition
    ("multipart/form-data; boundary=x", b"--x\r\nContent-Disposition: form-data; name=\"t\"\r\nhi\r\n--x--"),
])
def test_parse_form_rejects_malformed_bodies(ct, body):
    from pocket_tts_amd.server import FormError, parse_form

    with pytest.raises(FormError):
        parse_form(ct, body)


@pytest.mark.parametrize("fields,ok", [
    ({"temperature": "0.5", "noise_clamp": "2", "eos_threshold": "-3", "frames_after_eos": "3"}, True),
    ({"temperature": ""}, True),
    ({"temperature": "abc"}, False),
    ({"temperature": "-0.1"}, False),
    ({"temperature": "nan"}, False),
    ({"temperature": "inf"}, False),
    ({"noise_clamp": "-1"}, False),
    ({"eos_threshold": "nan"}, False),
    ({"frames_after_eos": "1.5"}, False),
    ({"frames_after_eos": "-1"}, False),
])
def test_parse_settings(fields, ok):
    from pocket_tts_amd.server import FormError, parse_settings

    if ok:
        s = parse_settings(fields)
        assert set(s) == {"temperature", "noise_clamp", "eos_threshold", "frames_after_eos"}
    else:
        with pytest.raises(FormError):
            parse_settings(fields)


# ---- the app against a stub model and batcher ----------------------------------------------------------------------
class _StubRequest:
    def __init__(self, n):
        self.n = n

    def iter_batches(self):
        for i in range(self.n):
            yield [torch.full((4,), i, dtype=torch.int16)]


class _StubBatcher:
    def __init__(self):
        self.failed, self.submitted, self.started, self.closed = None, [], False, False

    def start(self):
        self.started = True

    def close(self):
        self.closed = True

    def exclusive(self, fn, *a, **k):
        return fn(*a, **k)

    def submit(self, state, text, fae=None, **settings):
        if text == "too long":
            raise ValueError("request needs 2000 KV positions; slot capacity is 1024")
        self.submitted.append((state, text, fae, settings))
        return _StubRequest(3)


class _StubModel:
    sample_rate = 24000
    noise_clamp = None

    def get_state_for_audio_prompt(self, path, truncate=False):
        path = str(path)
        if path.endswith(".safetensors"):
            return {"voice": path}
        with wave.open(path, "rb") as w:  # raises wave.Error / EOFError on garbage, like the real reader
            w.readframes(-1)
        return {"upload": truncate}


def _wav_bytes(n=100):
    b = io.BytesIO()
    with wave.open(b, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(24000); w.writeframes(bytes(2 * n))
    return b.getvalue()


def _run_app(tmp_path, requests, default_voice="v1", model=None):
    import httpx

    from pocket_tts_amd.server import create_app

    (tmp_path / "v1.safetensors").write_bytes(b"x")
    stub = _StubBatcher()
    app = create_app(model or _StubModel(), slots=4, capacity=64, voices_dir=tmp_path, default_voice=default_voice,
                     batcher_factory=lambda m, s, c: stub)

    async def go():
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t") as cl:
                out = []
                for kind, data in requests:
                    if kind == "get":
                        out.append(await cl.get(data))
                    elif kind == "form":
                        out.append(await cl.post("/tts", data=data))
                    else:
                        ct, body = data
                        out.append(await cl.post("/tts", content=body, headers={"content-type": ct}))
                return out

    res = asyncio.run(go())
    assert stub.started and stub.closed
    return res, stub


def test_app_health_and_stream(tmp_path):
    res, stub = _run_app(tmp_path, [("get", "/health"), ("form", {"text": "hi", "temperature": "0.3"}),
                                    ("get", "/")])
    assert res[0].status_code == 200 and res[0].json() == {"status": "healthy"}
    r = res[1]
    assert r.status_code == 200 and r.headers["content-type"] == "audio/wav"
    body = r.content
    assert body[:4] == b"RIFF" and len(body) == 44 + 3 * 8 + 2 * 4800
    assert np.array_equal(np.frombuffer(body[44:68], np.int16), np.repeat([0, 1, 2], 4))
    state, text, fae, settings = stub.submitted[0]
    assert state == {"voice": str(tmp_path / "v1.safetensors")} and text == "hi" and fae is None
    assert settings == {"temperature": 0.3, "noise_clamp": None, "eos_threshold": None}
    assert res[2].status_code == 200 and "<form" in res[2].text


def test_app_uses_the_model_noise_clamp_and_uploads(tmp_path):
    m = _StubModel()
    m.noise_clamp = 2.5
    ct, body = _multipart({"text": "hi"}, {"voice_wav": ("p.wav", _wav_bytes())})
    res, stub = _run_app(tmp_path, [("form", {"text": "hi"}), ("raw", (ct, body))], model=m)
    assert [r.status_code for r in res] == [200, 200]
    assert stub.submitted[0][3]["noise_clamp"] == 2.5
    assert stub.submitted[1][0] == {"upload": True}


def test_app_health_reports_a_failed_batcher(tmp_path):
    import httpx

    from pocket_tts_amd.server import create_app

    stub = _StubBatcher()
    stub.failed = RuntimeError("boom")
    app = create_app(_StubModel(), slots=1, capacity=8, batcher_factory=lambda m, s, c: stub)

    async def go():
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t") as cl:
                return await cl.get("/health")

    r = asyncio.run(go())
    assert r.status_code == 503 and "boom" in r.text


def test_app_rejects_bad_requests_with_400(tmp_path):
    ct_both, both = _multipart({"text": "hi", "voice_url": "v1"}, {"voice_wav": ("p.wav", _wav_bytes())})
    ct_bad, bad_upload = _multipart({"text": "hi"}, {"voice_wav": ("p.wav", b"RIFF not a wav")})
    cases = [
        ("form", {"text": "   "}),
        ("raw", (ct_both, both)),
        ("form", {"text": "hi", "voice_url": "https://example.com/v.safetensors"}),
        ("form", {"text": "hi", "voice_url": "hf://kyutai/voices/alba.safetensors"}),
        ("form", {"text": "hi", "voice_url": "nobody"}),
        ("form", {"text": "hi", "voice_url": "../v1"}),
        ("form", {"text": "hi", "temperature": "hot"}),
        ("form", {"text": "hi", "temperature": "-1"}),
        ("form", {"text": "hi", "noise_clamp": "x"}),
        ("form", {"text": "hi", "eos_threshold": "inf"}),
        ("form", {"text": "hi", "frames_after_eos": "many"}),
        ("form", {"text": "too long"}),
        ("raw", (ct_bad, bad_upload)),
        ("raw", ("text/plain", b"text=hi")),
    ]
    res, stub = _run_app(tmp_path, cases)
    assert [r.status_code for r in res] == [400] * len(cases), [r.text for r in res]
    assert "needs a download; this build runs offline" in res[2].json()["detail"]
    assert stub.submitted == []


def test_app_without_default_voice(tmp_path):
    res, _ = _run_app(tmp_path, [("form", {"text": "hi"}), ("form", {"text": "hi", "voice_url": "v1"})],
                      default_voice=None)
    assert [r.status_code for r in res] == [400, 200]


# ---- CLI ---------------------------------------------------------------------------------------------------------
def test_serve_and_export_voice_flags():
    from pocket_tts_amd.main import build_parser

    p = build_parser()
    a = p.parse_args(["serve"])
    assert (a.host, a.port, a.slots, a.capacity, a.temperature, a.eos_threshold, a.noise_clamp) == \
        ("localhost", 8000, 64, 1024, 0.7, -4.0, None)
    assert a.capacity >= 376 + 50 + 234 + 8
    a = p.parse_args(["serve", "--host", "0.0.0.0", "--port", "9000", "--config", "c.yaml", "--quantize", "--codec-bf16",
                      "--temperature", "0.5", "--lsd-decode-steps", "2", "--noise-clamp", "3", "--eos-threshold", "-2",
                      "--slots", "8", "--capacity", "600", "--voices-dir", "vd", "--default-voice", "alba"])
    assert (a.host, a.port, a.config, a.quantize, a.codec_bf16, a.temperature, a.lsd_decode_steps, a.noise_clamp,
            a.eos_threshold, a.slots, a.capacity, a.voices_dir, a.default_voice) == \
        ("0.0.0.0", 9000, "c.yaml", True, True, 0.5, 2, 3.0, -2.0, 8, 600, "vd", "alba")
    a = p.parse_args(["export-voice", "in.wav", "out.safetensors", "--language", "english", "-q"])
    assert (a.command, a.audio_path, a.export_path, a.language, a.quiet) == \
        ("export-voice", "in.wav", "out.safetensors", "english", True)
    a = p.parse_args(["export-voice", "in.wav", "out.safetensors", "--config", "c.yaml"])
    assert a.config == "c.yaml" and not a.quiet
    with pytest.raises(SystemExit):
        p.parse_args(["export-voice", "in.wav"])


def test_pocket_tts_shim_exports_the_commands():
    import pocket_tts.main as shim

    for name in ("cli_app", "serve_app", "export_voice_app", "wav_stream_bytes", "write_wav_stream"):
        assert callable(getattr(shim, name))


# ---- the numpy restatement of the device noise ---------------------------------------------------------------------
def test_counter_normal_is_standard_normal():
    from scipy import stats

    z = counter_normal(7, 3, np.arange(20000))
    assert stats.kstest(z, "norm").pvalue > 1e-3


@pytest.mark.parametrize("temp,clamp", [(0.7, 1.0), (0.7, 0.3), (1.0, 2.5), (0.25, 0.05)])
def test_truncated_draw_stays_in_range_and_is_truncnorm(temp, clamp):
    from scipy import stats

    z = counter_trunc_normal(11, 5, np.arange(20000), temp, clamp)
    assert np.all(np.abs(z) <= clamp)
    sd = temp ** 0.5
    assert stats.kstest(z, stats.truncnorm(-clamp / sd, clamp / sd, scale=sd).cdf).pvalue > 1e-3
