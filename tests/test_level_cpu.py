"""The output-level feature without a GPU: the plan rule and the argument checks, the fp64 reference checked on its own
(streaming == whole signal, ceiling, transparency below the ceiling, release time), the server's `gain_db` / `peak_dbfs`
fields against a stub batcher, the CLI flags, and the kernel's index functions swept on the CPU under a host sanitizer (a
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

import level_ref
from resample_ref import NATIVE, RATES

REPO = Path(__file__).resolve().parents[1]
OUT_N = {8000: 640, 11025: 882, 12000: 960, 16000: 1280, 22050: 1764, 24000: 1920, 32000: 2560, 44100: 3528, 48000: 3840}
GPU_ROWS, gpu_signal = level_ref.GPU_ROWS, level_ref.gpu_signal


# ---- the plan rule and the argument checks -------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,n,LA", [(8000, 640, 40), (24000, 1920, 120), (48000, 3840, 240)])
def test_plan_values(rate, n, LA):
    from pocket_tts_amd.level import plan

    p = plan(rate, n)
    assert (p.n, p.LA, p.preroll, p.drain_frames) == (n, LA, LA, 1)
    assert p.a.dtype == np.float32 and p.a == np.float32(np.exp(-1.0 / (0.1 * rate)))
    assert p.k.dtype == np.float32 and p.k == np.float32(1.0 / LA)
    n_, LA_, a_bits, k_bits = p.ints()
    assert (n_, LA_) == (n, LA) and struct.unpack("<ff", struct.pack("<ii", a_bits, k_bits)) == (float(p.a), float(p.k))
    assert plan(11025, 882).LA == 56 and plan(44100, 3528).LA == 221  # ceil(0.005 rate)


def test_refusals_name_the_rule():
    from pocket_tts_amd.level import check, params, plan, table

    with pytest.raises(ValueError, match="exceeds the 512"):
        plan(192000, 8000)
    with pytest.raises(ValueError, match="shorter than the look-ahead of 120"):
        plan(24000, 119)
    with pytest.raises(ValueError, match="exceeds the kernel's 8192"):
        plan(24000, 8193)
    assert plan(24000, 120).n == 120 and plan(24000, 8192).n == 8192 and plan(102400, 512).LA == 512
    for bad in ("loud", True, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gain_db must be a finite number"):
            check(bad)
    for bad in (-40.5, 24.01):
        with pytest.raises(ValueError, match=r"gain_db .*must be in \[-40, 24\]"):
            check(bad)
    with pytest.raises(ValueError, match="peak_dbfs must be a finite number"):
        check(0, "x")
    for bad in (-20.5, 0.1):
        with pytest.raises(ValueError, match=r"peak_dbfs .*must be in \[-20, 0\]"):
            check(6, bad)
    with pytest.raises(ValueError, match="only meaningful together with gain_db"):
        check(None, -3)
    assert check(None) == (None, None) and check(6) == (6.0, -1.0) and check(0, 0) == (0.0, 0.0) and check(-40, -20) == (-40.0, -20.0)
    G, C = params(12, -1)
    assert G.dtype == np.float32 and G == np.float32(10 ** 0.6) and C == np.float32(10 ** -0.05)
    plans, index = table([(24000, 1920), (8000, 640), (24000, 1920), (24000, 960)])
    assert [(p.rate, p.n) for p in plans] == [(24000, 1920), (8000, 640), (24000, 960)] and index[(24000, 960)] == 2


# ---- the fp64 reference on its own -------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,n,gain", GPU_ROWS)
def test_streaming_reference_equals_the_whole_signal_and_the_ceiling_holds(rate, n, gain):
    from pocket_tts_amd.level import params, plan

    p = plan(rate, n)
    G, C = params(gain)
    x = gpu_signal(rate, n)
    y, u, r, g = level_ref.level(x, G, C, p.LA, p.a, p.k, full=True)
    st = level_ref.Stream(G, C, p.LA, p.a, p.k)
    ys = np.concatenate([st.feed(x[f * n:(f + 1) * n]) for f in range(4)])
    assert np.array_equal(ys, y)  # float64, exactly
    assert not y[:p.LA].any()  # the pre-roll
    assert np.max(np.abs(y)) <= float(C) * (1 + 2.0 ** -23)  # float64 never overshoots but for k LA, which is 1 only up to k's fp32 rounding
    # the contract in fp32 (what the kernel's arithmetic amounts to): the ceiling and the error bound of the GPU test
    y32 = level_ref.level_f32(x, G, C, p.LA, p.a, p.k)
    assert np.max(np.abs(y32)) <= float(C) * (1 + (p.LA + 8) * 2.0 ** -24)
    assert np.max(np.abs(y32 - y)) <= (p.LA + 64) * 2.0 ** -24 * np.max(np.abs(u))
    if gain > 0:
        assert 0.05 <= np.mean(r < 1) <= 0.5
    else:
        assert not (r < 1).any()


def test_a_signal_under_the_ceiling_comes_back_amplified_and_delayed():
    from pocket_tts_amd.level import params, plan

    p = plan(24000, 1920)
    G, C = params(6, -1)
    x = level_ref.signal(4 * 1920, seed=3)
    x = (x * (0.999 * float(C) / float(G) / np.max(np.abs(x)))).astype(np.float32)
    assert float(G) * np.max(np.abs(x)) <= float(C)
    want = np.concatenate([np.zeros(p.LA), float(G) * x.astype(np.float64)])[:len(x)]
    for y in (level_ref.level(x, G, C, p.LA, p.a, p.k), level_ref.level_f32(x, G, C, p.LA, p.a, p.k)):
        assert np.max(np.abs(y - want)) <= (p.LA + 8) * 2.0 ** -24 * np.max(np.abs(want))


def test_the_gain_recovers_after_a_burst():
    from pocket_tts_amd.level import params, plan

    rate = 24000
    p = plan(rate, 1920)
    G, C = params(12, -1)
    x = np.zeros(rate, np.float32)
    x[:2400] = 0.9 * np.sin(2 * np.pi * 440 * np.arange(2400) / rate)  # 0.1 s at +12 dB: about 12 dB of reduction
    _, _, _, g = level_ref.level(x, G, C, p.LA, p.a, p.k, full=True)
    end = 2400 + p.LA  # the last sample whose window sees the burst
    assert g[end] < 0.3
    assert g[end + int(0.1 * rate)] < 0.99   # not back within 1 % after 0.1 s
    assert g[end + int(0.5 * rate)] >= 0.99  # back after 0.5 s
    assert np.all(np.diff(g[end + p.LA:]) >= 0)  # and monotonically so


# ---- the index functions under a host sanitizer --------------------------------------------------------------------------
def _sweep_plans():
    from pocket_tts_amd.level import plan
    from pocket_tts_amd.stretch import plan as stretch_plan

    speeds = sorted({Fraction(a, q) for q in range(1, 21) for a in range(1, 41) if Fraction(1, 2) <= Fraction(a, q) <= 2} - {Fraction(1)})
    seen, ps = set(), []
    for rate in sorted({NATIVE, *RATES}):
        ns = [OUT_N[rate], plan(rate, OUT_N[rate]).LA, 8192]
        for s in speeds:
            try:
                ns.append(stretch_plan(float(s), rate, OUT_N[rate]).n_out)
            except ValueError:
                pass
        for n in ns:
            if (rate, n) not in seen:
                seen.add((rate, n))
                ps.append(plan(rate, n))
    return ps


def test_index_sweep_under_host_sanitizer(tmp_path):
    """every index the shared header forms, for every plan the rule admits (the documented rates x the samples per frame of
    every admissible speed, plus n = LA and n = 8192), on exact-size heap buffers under AddressSanitizer + UBSan"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path / "level_sweep"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-I", str(REPO / "pocket_tts_amd" / "csrc"), "-o", str(exe),
                        str(REPO / "tests" / "cpp" / "level_sweep.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    ps = _sweep_plans()
    assert len(ps) >= 60 and {p.rate for p in ps} == {NATIVE, *RATES}
    assert any(p.n == p.LA for p in ps) and any(p.n == 8192 for p in ps) and any(p.n % 2048 not in (0, p.n) for p in ps)
    blob = struct.pack("<i", len(ps))
    for p in ps:
        blob += struct.pack("<iiff", p.n, p.LA, float(p.a), float(p.k))
    (tmp_path / "plans.bin").write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # the leak checker needs ptrace, which build sandboxes often deny
    r = subprocess.run([str(exe), str(tmp_path / "plans.bin")], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.strip() == f"ok {len(ps)} plans {3 * sum(-(-p.n // 2048) for p in ps)} tiles"


def test_the_library_refuses_what_the_rule_refuses(tmp_path):
    """lv_plan_ok, compiled on the host: the plans of the rule pass, and each broken rule fails"""
    from pocket_tts_amd.level import plan

    cxx = shutil.which("g++") or shutil.which("c++")
    src = tmp_path / "ok.cpp"
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "ptts_level.h"\nint main(int c, char **v) {\n'
                   '  for (int i = 1; i + 1 < c; i += 2) printf("%d", (int)lv_plan_ok(atoi(v[i]), atoi(v[i + 1])));\n'
                   '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "ok"
    r = subprocess.run([cxx, "-std=c++17", "-I", str(REPO / "pocket_tts_amd" / "csrc"), "-o", str(exe), str(src)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = [(640, 40), (1920, 120), (3840, 240), (120, 120), (8192, 120), (512, 512),  # admitted
             (119, 120), (8193, 120), (1920, 0), (8000, 513), (0, 0), (-5, 1)]           # refused
    out = subprocess.run([str(exe), *[str(v) for c in cases for v in c]], capture_output=True, text=True, timeout=60).stdout.strip()
    assert out == "111111" + "000000"
    for (n, LA), ok in zip(cases, out):  # level.plan agrees: LA is the look-ahead of the rate 200 LA
        try:
            assert plan(200 * LA, n).LA == LA
            assert ok == "1", (n, LA)
        except ValueError:
            assert ok == "0", (n, LA)


# ---- the server's fields against a stub batcher ----------------------------------------------------------------------------
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
        if settings.get("gain_db") is not None and fae is not None and fae < 1:  # the batcher's own refusal
            raise ValueError("a request with a gain needs frames_after_eos >= 1")
        self.submitted.append(settings)
        return _StubRequest(3, 1920 * (settings.get("sample_rate") or 24000) // 24000)


class _StubModel:
    sample_rate = 24000
    noise_clamp = None
    engine = SimpleNamespace(frame_samples=1920)

    def get_state_for_audio_prompt(self, path, truncate=False):
        return {"voice": str(path)}


def _run_app(tmp_path, forms, **kw):
    import httpx

    from pocket_tts_amd.server import create_app

    (tmp_path / "v1.safetensors").write_bytes(b"x")
    stub = _StubBatcher()
    app = create_app(_StubModel(), slots=4, capacity=64, voices_dir=tmp_path, default_voice="v1",
                     batcher_factory=lambda m, s, c: stub, **kw)

    async def go():
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t") as cl:
                return [await cl.post("/tts", data=d) for d in forms], await cl.get("/")

    res, index = asyncio.run(go())
    assert stub.started and stub.closed
    return res, index, stub


def test_server_level_fields(tmp_path):
    forms = [{"text": "hi", "gain_db": "6"}, {"text": "hi", "gain_db": " -12.5 ", "peak_dbfs": "-3"}, {"text": "hi"},
             {"text": "hi", "gain_db": "", "peak_dbfs": ""}, {"text": "hi", "gain_db": "0", "sample_rate": "8000"}]
    res, index, stub = _run_app(tmp_path, forms, sample_rates=[8000], level=True)
    assert [r.status_code for r in res] == [200] * 5
    assert [(s.get("gain_db"), s.get("peak_dbfs")) for s in stub.submitted] == \
        [(6.0, -1.0), (-12.5, -3.0), (None, None), (None, None), (0.0, -1.0)]
    assert all("gain_db" not in s and "peak_dbfs" not in s for s in stub.submitted[2:4])  # a request like before
    for r, rate in zip(res, [24000, 24000, 24000, 24000, 8000]):
        n = 1920 * rate // 24000
        assert struct.unpack("<L", r.content[24:28])[0] == rate
        assert len(r.content) == 44 + 3 * n * 2 + 2 * int(rate * 0.2)  # header, chunks and silence are those of before
    assert 'name="gain_db"' in index.text and 'name="peak_dbfs"' in index.text


def test_server_level_400(tmp_path):
    bad = [{"text": "hi", "gain_db": "loud"}, {"text": "hi", "gain_db": "nan"}, {"text": "hi", "gain_db": "24.5"},
           {"text": "hi", "gain_db": "-41"}, {"text": "hi", "gain_db": "6", "peak_dbfs": "0.5"},
           {"text": "hi", "gain_db": "6", "peak_dbfs": "low"}, {"text": "hi", "peak_dbfs": "-3"},
           {"text": "hi", "gain_db": "6", "frames_after_eos": "0"}]
    res, _, stub = _run_app(tmp_path, bad, level=True)
    assert [r.status_code for r in res] == [400] * 8 and not stub.submitted
    d = [r.json()["detail"] for r in res]
    assert "must be a number" in d[0] and "finite" in d[1] and "[-40, 24]" in d[2] and "[-40, 24]" in d[3]
    assert "[-20, 0]" in d[4] and "must be a number" in d[5] and "together with gain_db" in d[6]
    assert "frames_after_eos >= 1" in d[7]  # what submit refuses reaches the client as a 400
    # a server without level refuses either field
    res, _, stub = _run_app(tmp_path, [{"text": "hi", "gain_db": "6"}, {"text": "hi", "peak_dbfs": "-3"}, {"text": "hi"}])
    assert [r.status_code for r in res] == [400, 400, 200]
    assert "without level" in res[0].json()["detail"] and "without level" in res[1].json()["detail"]
    assert stub.submitted == [{"temperature": None, "noise_clamp": None, "eos_threshold": None}]


def test_cli_flags():
    from pocket_tts_amd.main import build_parser

    ap = build_parser()
    a = ap.parse_args(["generate", "--gain-db", "6", "--peak-dbfs", "-3"])
    assert (a.gain_db, a.peak_dbfs) == (6.0, -3.0)
    a = ap.parse_args(["generate"])
    assert a.gain_db is None and a.peak_dbfs is None
    assert ap.parse_args(["serve", "--level"]).level is True and ap.parse_args(["serve"]).level is False
    with pytest.raises(SystemExit):
        ap.parse_args(["generate", "--gain-db", "loud"])


@pytest.mark.parametrize("extra", [["--gain-db", "30"], ["--peak-dbfs", "-3"], ["--gain-db", "nan"],
                                   ["--gain-db", "6", "--peak-dbfs", "1"]])
def test_cli_refuses_an_inadmissible_level_before_it_opens_the_output(tmp_path, monkeypatch, extra):
    """`generate_audio_stream` is a generator: it would raise only once the WAV file exists"""
    from pocket_tts_amd import main, tts_model

    class _Model(SimpleNamespace):
        def get_state_for_audio_prompt(self, voice):
            raise AssertionError("the level is checked before any work for the request")

    monkeypatch.setattr(tts_model.TTSModel, "load_model",
                        staticmethod(lambda **kw: _Model(sample_rate=24000, engine=SimpleNamespace(frame_samples=1920))))
    out = tmp_path / "out.wav"
    assert main.cli_app(["generate", "--text", "hi", *extra, "--output-path", str(out), "-q"]) == 1
    assert not out.exists()
