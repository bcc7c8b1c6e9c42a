"""The speaking-rate feature without a GPU: the plan rule, the fp64 reference checked on its own, the server's `speed`
field against a stub batcher, the CLI flags, and the kernel's index functions swept on the CPU under a host sanitizer (a
stand-alone C++ program run as a child process)."""

import asyncio
import os
import shutil
import struct
import subprocess
from fractions import Fraction
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import stretch_ref
from resample_ref import FRAME, NATIVE, RATES

REPO = Path(__file__).resolve().parents[1]
OUT_N = {8000: 640, 11025: 882, 12000: 960, 16000: 1280, 22050: 1764, 24000: 1920, 32000: 2560, 44100: 3528, 48000: 3840}


# ---- the plan rule -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("speed,Ha,Hs,L,n_out", [(0.5, 240, 480, 1680, 3840), (0.8, 384, 480, 1920, 2400),
                                                 (1.25, 640, 512, 1920, 1536), (1.5, 480, 320, 1440, 1280),
                                                 (2.0, 960, 480, 1920, 960)])
def test_plan_check_values(speed, Ha, Hs, L, n_out):
    from pocket_tts_amd.stretch import HIST, plan

    p = plan(speed, 24000, 1920)
    assert (p.Ha, p.Hs, p.D, p.L, p.n_out) == (Ha, Hs, 144, L, n_out)
    assert p.K == 1920 // Ha and p.W == 2 * Hs and not p.identity
    assert p.L % p.Ha == 0 and p.L >= p.D + p.W + p.Hs and p.L - p.Ha < p.D + p.W + p.Hs  # L = Ha ceil((D + W + Hs) / Ha)
    assert p.L + p.D + p.Ha <= HIST
    assert p.preroll == L // Ha * Hs and p.drain_frames == -(-(L // Ha) // p.K)
    assert p.window.dtype == np.float32 and p.window.shape == (2 * Hs,)
    n = np.arange(2 * Hs)
    assert np.array_equal(p.window, (0.5 - 0.5 * np.cos(2 * np.pi * n / (2 * Hs))).astype(np.float32))


def test_plan_at_8_khz():
    from pocket_tts_amd.stretch import plan

    ok = []
    for s in (0.5, 0.75, 0.8, 1.2, 1.25, 1.5, 2.0):
        try:
            plan(s, 8000, 640)
            ok.append(s)
        except ValueError as e:
            assert "whole number of hops" in str(e)
    assert ok == [0.5, 0.8, 1.25, 2.0]
    p = plan(0.8, 8000, 640)
    assert (p.Ha, p.Hs, p.D, p.L, p.n_out) == (128, 160, 48, 640, 800)


def test_plan_refusals_name_the_rule():
    from pocket_tts_amd.stretch import plan

    for bad, msg in [("fast", "finite number"), (True, "finite number"), (float("nan"), "finite number"),
                     (0.77, "fraction p / q"), (1 / 21 + 1, "fraction p / q"), (0.45, r"must be in \[0.5, 2.0\]"),
                     (2.05, r"must be in \[0.5, 2.0\]"), (0.9, "no multiple of 9 divides 1920"),
                     (1.1, "no multiple of 11 divides 1920")]:
        with pytest.raises(ValueError, match=msg):
            plan(bad, 24000, 1920)
    with pytest.raises(ValueError, match="8 to 32 ms"):
        plan(0.5, 24000, 64)       # hops divide the frame, but none is long enough
    with pytest.raises(ValueError, match="more than the 8192"):
        plan(2.0, 96000, 7680)     # L + D + Ha = 7680 + 576 + 3840
    with pytest.raises(ValueError, match="staged window"):
        plan(2.0, 48000, 7680)     # L + D + Ha = 6048 fits, + n_in does not


def test_table_and_speed_list():
    from pocket_tts_amd.stretch import normalise_speeds, table

    speeds = normalise_speeds([1.5, 0.8, 1.5, 1.0])
    assert speeds == [1.0, 1.5, 0.8]
    plans, index = table([(24000, 1920), (8000, 640)], speeds)
    assert index == [[0, 1, 2], [3, None, 4]]  # 1.5 has no whole hops at 8 kHz
    assert plans[0].identity and plans[3].identity and plans[3].n_in == 640 and plans[4].Hs == 160
    assert plans[0].preroll == 0 and plans[0].drain_frames == 0 and plans[0].n_out == 1920
    with pytest.raises(ValueError, match="no multiple of 9"):
        table([(24000, 1920), (8000, 640)], normalise_speeds([0.9]))
    with pytest.raises(ValueError, match="must be in"):
        normalise_speeds([3.0])


# ---- the fp64 reference on its own -------------------------------------------------------------------------------------
def _noise(n, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n + 64)
    return np.convolve(x, np.hanning(33) / np.hanning(33).sum(), mode="valid")[:n] * 0.5


@pytest.mark.parametrize("speed,rate", [(0.5, 24000), (0.8, 24000), (1.25, 24000), (1.5, 24000), (2.0, 24000), (0.8, 8000)])
def test_streaming_reference_equals_the_whole_signal(speed, rate):
    from pocket_tts_amd.stretch import plan

    p = plan(speed, rate, OUT_N[rate])
    frames = 6
    x = _noise(frames * p.n_in, seed=int(speed * 100))
    y, deltas = stretch_ref.wsola(x, p, frames)
    assert y.shape == (frames * p.n_out,) and len(deltas) == frames * p.K
    assert deltas[0] == 0 and all(-p.D <= d <= p.D for d in deltas)
    # hop k reads nothing but zeros while k Ha - L + D + W <= 0: the output starts with that many silent hops
    assert not y[:((p.L - p.D - p.W) // p.Ha + 1) * p.Hs].any()
    st = stretch_ref.Stream(p)
    ys = np.concatenate([st.feed(x[f * p.n_in:(f + 1) * p.n_in]) for f in range(frames)])
    assert st.deltas == deltas
    assert np.max(np.abs(ys - y)) <= 1e-15 * np.max(np.abs(x)) * 4
    # with the drain frames the tail comes out: the last input sample shapes the output
    tail = np.concatenate([st.feed(np.zeros(p.n_in)) for _ in range(p.drain_frames)])
    full, _ = stretch_ref.wsola(x, p, frames + p.drain_frames)
    assert np.max(np.abs(np.concatenate([ys, tail]) - full)) <= 1e-15 * np.max(np.abs(x)) * 4
    assert len(full) >= p.preroll + frames * p.n_out


def test_tie_break():
    assert stretch_ref.choose(np.array([1.0, 3.0, 2.0, 3.0, 1.0]), 2) == -1   # equal |delta|: the negative one
    assert stretch_ref.choose(np.array([3.0, 1.0, 3.0, 1.0, 1.0]), 2) == 0    # the smallest |delta|
    assert stretch_ref.choose(np.zeros(7), 3) == 0
    assert stretch_ref.choose(np.array([0.0, 0.0, 0.0, 0.0, 5.0]), 2) == 2


@pytest.mark.parametrize("speed", [0.5, 0.8, 1.25, 2.0])
def test_a_constant_comes_back_constant(speed):
    from pocket_tts_amd.stretch import plan

    p = plan(speed, 24000, 1920)
    frames = 4
    y, _ = stretch_ref.wsola(np.full(frames * p.n_in, 0.75), p, frames)
    # w[n] + w[n + Hs] = 1 up to the table's fp32 rounding (2 * 2^-25 relative at most)
    assert np.max(np.abs(y[p.preroll + p.W:] - 0.75)) <= 0.75 * 2.0 ** -23


@pytest.mark.parametrize("speed", [0.5, 0.8, 1.25, 2.0])
def test_a_tone_keeps_its_pitch_and_level(speed):
    from pocket_tts_amd.stretch import plan

    p = plan(speed, 24000, 1920)
    frames = 50  # 4 s in
    t = np.arange(frames * p.n_in)
    x = 0.5 * np.sin(2 * np.pi * 210.0 * t / 24000)
    y, _ = stretch_ref.wsola(x, p, frames)
    y = y[p.preroll + p.W:]
    assert len(y) >= 24000  # a second at least
    nfft = 1 << 20
    spec = np.abs(np.fft.rfft(y * np.hanning(len(y)), nfft))
    k = int(np.argmax(spec))
    a, b, c = np.log(spec[k - 1:k + 2])
    peak = (k + 0.5 * (a - c) / (a - 2 * b + c)) * 24000 / nfft
    assert abs(peak - 210.0) <= 0.5, peak
    rms = float(np.sqrt(np.mean(y ** 2)))
    assert abs(rms - 0.5 / np.sqrt(2)) <= 1e-3, rms


# ---- the index functions under a host sanitizer --------------------------------------------------------------------------
def test_index_sweep_under_host_sanitizer(tmp_path):
    """every index the shared header forms, for every plan the rule admits at every documented rate (every fraction p / q
    with q <= 20 in [0.5, 2], and the rates' identity plans), on exact-size heap buffers under AddressSanitizer + UBSan"""
    from pocket_tts_amd.stretch import identity, plan

    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path / "stretch_sweep"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-I", str(REPO / "pocket_tts_amd" / "csrc"), "-o", str(exe),
                        str(REPO / "tests" / "cpp" / "stretch_sweep.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    speeds = sorted({Fraction(a, q) for q in range(1, 21) for a in range(1, 41) if Fraction(1, 2) <= Fraction(a, q) <= 2} - {Fraction(1)})
    ps = []
    for rate in sorted({NATIVE, *RATES}):
        ps.append(identity(rate, OUT_N[rate]))
        for s in speeds:
            try:
                ps.append(plan(float(s), rate, OUT_N[rate]))
            except ValueError:
                pass
    stretched = [p for p in ps if not p.identity]
    assert len(stretched) >= 40 and {p.rate for p in stretched} == {NATIVE, *RATES}
    blob = struct.pack("<i", len(ps))
    for p in ps:
        blob += struct.pack("<iiiii", *p.ints()) + p.window.astype("<f4").tobytes()
    (tmp_path / "plans.bin").write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # the leak checker needs ptrace, which build sandboxes often deny
    r = subprocess.run([str(exe), str(tmp_path / "plans.bin")], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.strip() == f"ok {len(ps)} plans {len(ps) - len(stretched)} identities {2 * sum(p.K for p in stretched)} hops"


def test_the_library_refuses_what_the_header_refuses(tmp_path):
    """ts_plan_ok, compiled on the host: the plans of the rule pass, and each broken rule fails"""
    cxx = shutil.which("g++") or shutil.which("c++")
    src = tmp_path / "ok.cpp"
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "ptts_stretch.h"\nint main(int c, char **v) {\n'
                   '  printf("%d\\n", (int)ts_plan_ok(atoi(v[1]), atoi(v[2]), atoi(v[3]), atoi(v[4]), atoi(v[5]), 8192));\n  return 0;\n}\n')
    exe = tmp_path / "ok"
    r = subprocess.run([cxx, "-std=c++17", "-I", str(REPO / "pocket_tts_amd" / "csrc"), "-o", str(exe), str(src)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]

    def ok(*v):
        return subprocess.run([str(exe), *map(str, v)], capture_output=True, text=True, timeout=60).stdout.strip() == "1"

    assert ok(1920, 640, 512, 144, 1920) and ok(1920, 1920, 1920, 0, 0) and ok(640, 128, 160, 48, 640)
    assert not ok(1920, 640, 512, 144, 1280)      # L < D + W + Hs: a read past the frame's end
    assert not ok(1920, 640, 512, 144, 2000)      # L is no multiple of Ha
    assert not ok(1920, 600, 512, 144, 1800)      # no whole hops per frame
    assert not ok(1920, 640, 256, 144, 1280)      # speed above 2
    assert not ok(1920, 640, 512, 600, 2560)      # 2 D + 1 candidates exceed the score line
    assert not ok(7680, 3840, 1920, 576, 7680)    # L + D + Ha > 8192
    assert not ok(7680, 1920, 960, 288, 3840)     # the staged window
    assert not ok(9000, 9000, 9000, 0, 0) and not ok(0, 1, 1, 0, 0)


# ---- the server's speed field against a stub batcher ------------------------------------------------------------------------
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
        from pocket_tts_amd.stretch import plan

        if settings.get("speed") is not None and fae is not None and fae < 1:  # the batcher's own refusal
            raise ValueError("a request with a speed needs frames_after_eos >= 1")
        self.submitted.append(settings)
        rate = settings.get("sample_rate") or 24000
        n = 1920 * rate // 24000
        if settings.get("speed") is not None:
            n = plan(settings["speed"], rate, n).n_out
        return _StubRequest(3, n)


class _StubModel:
    sample_rate = 24000
    noise_clamp = None
    engine = SimpleNamespace(frame_samples=1920)

    def get_state_for_audio_prompt(self, path, truncate=False):
        return {"voice": str(path)}


def _run_app(tmp_path, forms, sample_rates, speeds):
    import httpx

    from pocket_tts_amd.server import create_app

    (tmp_path / "v1.safetensors").write_bytes(b"x")
    stub = _StubBatcher()
    app = create_app(_StubModel(), slots=4, capacity=64, voices_dir=tmp_path, default_voice="v1",
                     batcher_factory=lambda m, s, c: stub, sample_rates=sample_rates, speeds=speeds)

    async def go():
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t") as cl:
                return [await cl.post("/tts", data=d) for d in forms], await cl.get("/")

    res, index = asyncio.run(go())
    assert stub.started and stub.closed
    return res, index, stub


def test_server_speed_field(tmp_path):
    forms = [{"text": "hi", "speed": "1.25"}, {"text": "hi", "speed": " 0.8 ", "sample_rate": "8000"}, {"text": "hi"},
             {"text": "hi", "speed": ""}, {"text": "hi", "speed": "1.0"}, {"text": "hi", "speed": "1.5"}]
    res, index, stub = _run_app(tmp_path, forms, [8000], [0.8, 1.25, 1.5])
    assert [r.status_code for r in res] == [200] * 6
    assert [s.get("speed") for s in stub.submitted] == [1.25, 0.8, None, None, None, 1.5]
    assert all("speed" not in s for s in stub.submitted[2:5])  # speed 1.0 is a request like before
    for r, (rate, n_out) in zip(res, [(24000, 1536), (8000, 800), (24000, 1920), (24000, 1920), (24000, 1920), (24000, 1280)]):
        body = r.content
        assert struct.unpack("<L", body[24:28])[0] == rate
        assert len(body) == 44 + 3 * n_out * 2 + 2 * int(rate * 0.2)  # the delivered samples, then 200 ms of silence
        x = np.frombuffer(body[44:], np.int16)
        assert np.array_equal(x[:3 * n_out], np.repeat([0, 1, 2], n_out)) and not x[3 * n_out:].any()
    assert 'name="speed"' in index.text


def test_server_speed_400(tmp_path):
    bad = [{"text": "hi", "speed": "fast"}, {"text": "hi", "speed": "nan"}, {"text": "hi", "speed": "2.0"},
           {"text": "hi", "speed": "1.5", "sample_rate": "8000"}, {"text": "hi", "speed": "1.25", "frames_after_eos": "0"}]
    res, _, stub = _run_app(tmp_path, bad, [8000], [0.8, 1.25, 1.5])
    assert [r.status_code for r in res] == [400] * 5 and not stub.submitted
    assert "frames_after_eos >= 1" in res[4].json()["detail"]  # what submit refuses reaches the client as a 400
    d = [r.json()["detail"] for r in res]
    assert "must be a number" in d[0] and "finite" in d[1] and "not configured" in d[2]
    assert "not admissible at 8000 Hz" in d[3] and "[1.0, 0.8, 1.25]" in d[3]  # the speeds that rate admits
    # a server without speeds speaks at 1.0 only
    res, _, stub = _run_app(tmp_path, [{"text": "hi", "speed": "1.25"}, {"text": "hi", "speed": "1.0"}], None, None)
    assert [r.status_code for r in res] == [400, 200] and stub.submitted == [{"temperature": None, "noise_clamp": None,
                                                                               "eos_threshold": None}]


def test_server_refuses_a_speed_no_rate_admits(tmp_path):
    from pocket_tts_amd.server import create_app

    for speeds, msg in [([0.9], "no multiple of 9"), ([3.0], "must be in"), ([0.77], "fraction")]:
        with pytest.raises(ValueError, match=msg):
            create_app(_StubModel(), slots=1, capacity=8, batcher_factory=lambda m, s, c: _StubBatcher(), speeds=speeds)
    # 1.5 has no whole hops at 8 kHz but does at the native rate: accepted
    create_app(_StubModel(), slots=1, capacity=8, batcher_factory=lambda m, s, c: _StubBatcher(), sample_rates=[8000], speeds=[1.5])


def test_cli_flags():
    from pocket_tts_amd.main import build_parser

    ap = build_parser()
    assert ap.parse_args(["generate", "--speed", "1.25"]).speed == 1.25
    assert ap.parse_args(["generate"]).speed is None
    assert ap.parse_args(["serve", "--speeds", "0.8,1.25,1.5"]).speeds == [0.8, 1.25, 1.5]
    assert ap.parse_args(["serve"]).speeds is None
    with pytest.raises(SystemExit):
        ap.parse_args(["serve", "--speeds", "fast"])


@pytest.mark.parametrize("extra", [["--speed", "0.9"], ["--speed", "1.5", "--sample-rate", "8000"], ["--speed", "3"]])
def test_cli_refuses_an_inadmissible_speed_before_it_opens_the_output(tmp_path, monkeypatch, extra):
    """`generate_audio_stream` is a generator: it would raise only once the WAV file exists"""
    from types import SimpleNamespace

    from pocket_tts_amd import main, tts_model

    class _Model(SimpleNamespace):
        def get_state_for_audio_prompt(self, voice):
            raise AssertionError("the speed is checked before any work for the request")

    monkeypatch.setattr(tts_model.TTSModel, "load_model",
                        staticmethod(lambda **kw: _Model(sample_rate=24000, engine=SimpleNamespace(frame_samples=1920))))
    out = tmp_path / "out.wav"
    assert main.cli_app(["generate", "--text", "hi", *extra, "--output-path", str(out), "-q"]) == 1
    assert not out.exists()
