"""The output-sample-rate feature without a GPU: the filter design against scipy, the streaming fp64 reference against
scipy.signal.upfirdn, the admission rules, the server's `sample_rate` field against a stub batcher, the CLI flags, and the
kernel's index function swept on the CPU under a host sanitizer (a stand-alone C++ program run as a child process)."""

import asyncio
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from resample_ref import FRAME, NATIVE, RATES, StreamRef, poly_table

REPO = Path(__file__).resolve().parents[1]
OUT_N = {8000: 640, 11025: 882, 12000: 960, 16000: 1280, 22050: 1764, 32000: 2560, 44100: 3528, 48000: 3840}


# ---- the filter ----------------------------------------------------------------------------------------------------
def test_ratio_is_reduced():
    from pocket_tts_amd.resample import ratio

    assert ratio(8000, 24000) == (1, 3) and ratio(48000, 24000) == (2, 1) and ratio(24000, 24000) == (1, 1)
    assert ratio(44100, 24000) == (147, 80) and ratio(22050, 24000) == (147, 160) and ratio(11025, 24000) == (147, 320)


@pytest.mark.parametrize("rate", RATES)
def test_taps_equal_scipy_firwin(rate):
    from scipy.signal import firwin

    from pocket_tts_amd.resample import HIST, plan

    p = plan(rate, NATIVE, FRAME)
    m = max(p.up, p.down)
    L = 20 * m + 1
    want = firwin(L, 1.0 / m, window=("kaiser", 5.0)) * p.up
    assert p.h.dtype == np.float64 and p.h.shape == (L,)
    assert np.abs(p.h - want).max() <= 1e-12
    assert p.out_n == OUT_N[rate] and p.taps == -(-L // p.up) and p.taps - 1 <= HIST
    # the fp32 polyphase table: [ph][j] = h[ph + j * up], zero-padded
    assert p.table.dtype == np.float32 and p.table.shape == (p.up, p.taps)
    assert np.array_equal(p.table, poly_table(p.h, p.up, p.taps).astype(np.float32))
    flat = p.table.T.reshape(-1)
    assert np.array_equal(flat[:L], p.h.astype(np.float32)) and not flat[L:].any()


def test_native_rate_is_a_copy():
    from pocket_tts_amd.resample import plan, plans

    p = plan(NATIVE, NATIVE, FRAME)
    assert p.native and (p.up, p.down, p.taps, p.out_n) == (1, 1, 1, FRAME) and p.delay_input_samples == 0
    ps = plans([48000, 8000, 24000, 8000], NATIVE, FRAME)
    assert [q.rate for q in ps] == [24000, 48000, 8000]  # native first, every rate once
    assert plan(8000).delay_input_samples == 30.0  # 1.25 ms at 24 kHz
    x = np.random.default_rng(0).standard_normal(FRAME)
    y, bound = StreamRef(p.table, 1, 1).frame(x)
    assert np.array_equal(y, x) and not bound.any()


@pytest.mark.parametrize("rate", RATES)
def test_streaming_reference_equals_upfirdn(rate):
    from scipy.signal import upfirdn

    from pocket_tts_amd.resample import plan

    p = plan(rate, NATIVE, FRAME)
    n_frames = 3
    x = np.random.default_rng(rate).standard_normal(n_frames * FRAME)
    ref = StreamRef(poly_table(p.h, p.up, p.taps), p.up, p.down)
    got = np.concatenate([ref.frame(x[f * FRAME:(f + 1) * FRAME])[0] for f in range(n_frames)])
    want = upfirdn(p.h, x, p.up, p.down)[:n_frames * p.out_n]
    assert got.shape == want.shape == (n_frames * OUT_N[rate],)
    assert np.abs(got - want).max() <= 1e-12


def test_rate_validation_names_the_rule():
    from pocket_tts_amd.resample import plan

    for rate in (7999, 48001):
        with pytest.raises(ValueError, match=r"must be in \[8000, 48000\]"):
            plan(rate, NATIVE, FRAME)
    # fractional samples per frame: 10560 / 24000 = 11 / 25 and 1920 * 11 / 25 = 844.8; 8001 / 24000 = 2667 / 8000
    for rate in (10560, 8001):
        with pytest.raises(ValueError, match="not a whole number of output samples"):
            plan(rate, NATIVE, FRAME)
    # 10000 Hz is NOT such a rate, although it looks like one: 10000 / 24000 = 5 / 12 and 1920 * 5 / 12 = 800 exactly, and
    # its 49 taps per phase fit the history, so every rule admits it
    p = plan(10000, NATIVE, FRAME)
    assert (p.up, p.down, p.out_n, p.taps) == (5, 12, 800, 49)
    with pytest.raises(ValueError, match="samples of history"):
        plan(8000, 48000, 3840)  # up 1, down 6: 121 taps in one phase
    for bad in (16000.0, "16000", True, None):
        with pytest.raises(ValueError, match="must be an integer"):
            plan(bad, NATIVE, FRAME)


# ---- the index function under a host sanitizer --------------------------------------------------------------------------
def test_index_sweep_under_host_sanitizer(tmp_path):
    """every index the kernel's index function forms, for every documented rate and every output of a frame, on exact-size
    heap buffers under AddressSanitizer + UBSan; the result against the direct double-precision form"""
    from pocket_tts_amd.resample import plan

    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path / "resample_sweep"
    # the sanitizers' runtimes are linked statically: the program then needs no preloaded runtime and does not mind what
    # else the environment preloads, so the child runs in the environment as it is
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-I", str(REPO / "pocket_tts_amd" / "csrc"), "-o", str(exe),
                        str(REPO / "tests" / "cpp" / "resample_sweep.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    ps = [plan(rate, NATIVE, FRAME) for rate in RATES]
    blob = struct.pack("<ii", len(ps), FRAME)
    for p in ps:
        blob += struct.pack("<iii", p.up, p.down, p.taps) + p.table.astype("<f4").tobytes()
    (tmp_path / "tables.bin").write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # the leak checker needs ptrace, which build sandboxes often deny
    r = subprocess.run([str(exe), str(tmp_path / "tables.bin")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.strip() == f"ok {len(ps)} rates {sum(p.out_n for p in ps)} outputs"


# ---- the server's sample_rate field against a stub batcher ---------------------------------------------------------------
class _StubRequest:
    def __init__(self, n, samples):
        self.n, self.samples = n, samples

    def iter_batches(self):
        for i in range(self.n):
            yield [torch.full((self.samples,), i, dtype=torch.int16)]


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
        self.submitted.append(settings)
        rate = settings.get("sample_rate") or 24000
        return _StubRequest(3, 1920 * rate // 24000)


class _StubModel:
    sample_rate = 24000
    noise_clamp = None

    def get_state_for_audio_prompt(self, path, truncate=False):
        return {"voice": str(path)}


def _run_app(tmp_path, forms, sample_rates):
    import httpx

    from pocket_tts_amd.server import create_app

    (tmp_path / "v1.safetensors").write_bytes(b"x")
    stub = _StubBatcher()
    app = create_app(_StubModel(), slots=4, capacity=64, voices_dir=tmp_path, default_voice="v1",
                     batcher_factory=lambda m, s, c: stub, sample_rates=sample_rates)

    async def go():
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t") as cl:
                return [await cl.post("/tts", data=d) for d in forms], await cl.get("/")

    res, index = asyncio.run(go())
    assert stub.started and stub.closed
    return res, index, stub


def _header(body):
    assert body[:4] == b"RIFF" and body[8:16] == b"WAVEfmt " and body[36:40] == b"data"
    channels, rate, byte_rate, align, bits = struct.unpack("<HLLHH", body[22:36])
    assert (channels, bits, align, byte_rate) == (1, 16, 2, 2 * rate)
    return rate


def test_server_sample_rate_field(tmp_path):
    forms = [{"text": "hi", "sample_rate": "16000"}, {"text": "hi", "sample_rate": " 8000 "}, {"text": "hi"},
             {"text": "hi", "sample_rate": ""}, {"text": "hi", "sample_rate": "24000"}]
    res, index, stub = _run_app(tmp_path, forms, [8000, 16000, 48000])
    assert [r.status_code for r in res] == [200] * 5, [r.text[:200] for r in res]
    assert [s.get("sample_rate") for s in stub.submitted] == [16000, 8000, None, None, None]
    assert all("sample_rate" not in s for s in stub.submitted[2:])  # the native rate is a request like before
    for r, rate in zip(res, [16000, 8000, 24000, 24000, 24000]):
        body = r.content
        assert _header(body) == rate
        out_n = 1920 * rate // 24000
        assert len(body) == 44 + 3 * out_n * 2 + 2 * int(rate * 0.2)  # the frames, then 200 ms of silence at the rate
        x = np.frombuffer(body[44:], np.int16)
        assert np.array_equal(x[:3 * out_n], np.repeat([0, 1, 2], out_n)) and not x[3 * out_n:].any()
    assert 'name="sample_rate"' in index.text


def test_server_sample_rate_400(tmp_path):
    bad = [{"text": "hi", "sample_rate": "fast"}, {"text": "hi", "sample_rate": "16000.0"},
           {"text": "hi", "sample_rate": "44100"}, {"text": "hi", "sample_rate": "-8000"}]
    res, _, stub = _run_app(tmp_path, bad, [8000, 16000])
    assert [r.status_code for r in res] == [400] * 4 and not stub.submitted
    assert "must be an integer" in res[0].json()["detail"] and "not configured" in res[2].json()["detail"]
    # a server without sample_rates offers the codec's own rate only
    res, _, stub = _run_app(tmp_path, [{"text": "hi", "sample_rate": "16000"}, {"text": "hi", "sample_rate": "24000"}], None)
    assert [r.status_code for r in res] == [400, 200] and stub.submitted == [{"temperature": None, "noise_clamp": None,
                                                                               "eos_threshold": None}]


def test_server_refuses_an_inadmissible_configured_rate(tmp_path):
    from pocket_tts_amd.server import create_app

    with pytest.raises(ValueError, match="whole number"):
        create_app(_StubModel(), slots=1, capacity=8, batcher_factory=lambda m, s, c: _StubBatcher(), sample_rates=[10560])


def test_cli_flags():
    from pocket_tts_amd.main import build_parser

    ap = build_parser()
    assert ap.parse_args(["generate", "--sample-rate", "16000"]).sample_rate == 16000
    assert ap.parse_args(["generate"]).sample_rate is None
    assert ap.parse_args(["serve", "--sample-rates", "8000,16000,48000"]).sample_rates == [8000, 16000, 48000]
    assert ap.parse_args(["serve"]).sample_rates is None
    with pytest.raises(SystemExit):
        ap.parse_args(["serve", "--sample-rates", "8k"])


def test_cli_refuses_an_inadmissible_rate_before_it_opens_the_output(tmp_path, monkeypatch):
    """`generate_audio_stream` is a generator: it would raise only once the WAV file exists, header written at the bad rate"""
    from types import SimpleNamespace

    from pocket_tts_amd import main, tts_model

    class _Model(SimpleNamespace):
        def get_state_for_audio_prompt(self, voice):
            raise AssertionError("the rate is checked before any work for the request")

    monkeypatch.setattr(tts_model.TTSModel, "load_model",
                        staticmethod(lambda **kw: _Model(sample_rate=24000, engine=SimpleNamespace(frame_samples=1920))))
    out = tmp_path / "out.wav"
    assert main.cli_app(["generate", "--text", "hi", "--sample-rate", "10560", "--output-path", str(out), "-q"]) == 1
    assert not out.exists()
