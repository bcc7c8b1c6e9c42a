"""The loudness feature without a GPU: the plan rule and the argument checks, the K-weighting against the standard's table,
the fp64 reference checked on its own (streaming == whole signal, the 997 Hz calibration anchor, and the property the feature
exists for: speech-like signals land within 1 LU of the target), `route()` with every mix of stages, the server's
`loudness_lufs` field against a stub batcher, the CLI flags, and the kernel's index functions and chunked recurrence swept on
the CPU under a host sanitizer (a stand-alone C++ program run as a child process)."""

import asyncio
import itertools
import os
import shutil
import struct
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import loudness_ref

REPO = Path(__file__).resolve().parents[1]
# ITU-R BS.1770-4, tables 1 and 2 (48 kHz): b0 b1 b2 a1 a2 of the shelf, then of the high-pass
BS1770_48K = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
              1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]


# ---- the plan rule and the argument checks -------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,n,S,chunk", [(8000, 640, 800, 1), (11025, 882, 1102, 1), (24000, 1920, 2400, 2),
                                            (48000, 7680, 4800, 8), (48000, 8192, 4800, 8), (44100, 1, 4410, 1)])
def test_plan_values(rate, n, S, chunk):
    from pocket_tts_amd import loudness

    p = loudness.plan(rate, n)
    assert (p.rate, p.n, p.S, p.D, p.preroll, p.chunk) == (rate, n, S, 4 * S, 4 * S, chunk)
    assert p.drain_frames == -(-4 * S // n) and p.ints() == (rate, n)
    assert p.coef.dtype == np.float64 and p.coef.shape == (10,) and p.powers.shape == (loudness.SCAN_STEPS, 2, 4, 4)
    d = p.doubles()
    assert d.dtype == np.float64 and d.shape == (loudness.DOUBLES_PER_PLAN,) and np.isfinite(d).all()
    (sb, sa), (hb, ha) = loudness_ref.coefficients(rate)  # the test's own restatement
    assert np.array_equal(p.coef, np.array([*sb, *sa[1:], *hb, *ha[1:]]))
    # the powers are those of the recurrence `step` runs: A^chunk applied to a state equals `chunk` steps on zero input
    s = [0.3, -0.2, 0.5, 0.1]
    want = p.powers[0, 0] @ np.array(s)
    assert np.abs(p.powers[:, 1]).max() <= 2.0 ** -53 * np.abs(p.powers[:, 0]).max() and p.powers[:, 1].any()  # hi + lo
    for _ in range(chunk):
        loudness.step([float(c) for c in p.coef], s, 0.0)
    assert np.allclose(want, s, rtol=1e-12, atol=1e-15)
    for t in range(1, loudness.SCAN_STEPS):
        assert np.allclose(p.powers[t, 0], p.powers[t - 1, 0] @ p.powers[t - 1, 0], rtol=1e-9, atol=1e-300)
    # the high-pass poles: radius sqrt(a2), 0.9705 at 8 kHz to 0.9950 at 48 kHz
    assert 0.970 < np.sqrt(p.coef[9]) < 0.9951


def test_the_48k_coefficients_are_the_table_of_the_standard():
    from pocket_tts_amd import loudness

    assert np.abs(loudness.kweighting(48000) - np.array(BS1770_48K)).max() <= 1e-9


def test_refusals_name_their_rule():
    from pocket_tts_amd import loudness

    for rate, n, text in ((7999, 640, r"\[8000, 48000\]"), (48001, 640, r"\[8000, 48000\]"), (24000, 0, r"\[1, 8192\]"),
                          (24000, 8193, r"\[1, 8192\]")):
        with pytest.raises(ValueError, match=text):
            loudness.plan(rate, n)
    assert loudness.check(None) is None and loudness.check(-16) == -16.0 and loudness.check(-40) == -40.0
    for v, text in ((-40.5, r"\[-40, -10\]"), (-9.9, r"\[-40, -10\]"), (float("nan"), "finite"), ("-16", "finite"),
                    (True, "finite")):
        with pytest.raises(ValueError, match=text):
            loudness.check(v)
    plans, index = loudness.table([(24000, 1920), (8000, 640), (24000, 1920)])
    assert len(plans) == 2 and index == {(24000, 1920): 0, (8000, 640): 1}
    with pytest.raises(ValueError, match="7000 Hz"):
        loudness.table([(24000, 1920), (7000, 560)])


# ---- the reference on its own ------------------------------------------------------------------------------------------------
def speech_like(rate, amp, seed):
    """4 s of low-passed noise under a syllable envelope (3 per second, with a slow swell)"""
    n = 4 * rate
    t = np.arange(n) / rate
    env = np.clip(np.sin(2 * np.pi * 3.0 * t + seed), 0, None) ** 2 * (0.6 + 0.4 * np.sin(2 * np.pi * 0.4 * t))
    x = np.convolve(np.random.default_rng(seed).standard_normal(n), np.ones(4) / 4, mode="same")
    return (amp * env * x).astype(np.float32)


def test_streaming_equals_the_whole_signal_exactly():
    x = speech_like(8000, 0.3, 2)[:12000]
    y, whole = loudness_ref.reference(x, 8000, -16.0)
    for n in (640, 1, 801):
        s = loudness_ref.Stream(8000, -16.0)
        parts = [s.frame(x[i:i + n]) for i in range(0, 3000 if n == 1 else len(x), n)]
        got = np.concatenate(parts)
        assert np.array_equal(got, y[:len(got)]), n
        m = len(s.c)
        assert s.c == whole.c[:m] and s.L == whole.L[:m] and s.Z == whole.Z[:m], n
    assert not y[:3200].any() and y[3200:].any() and len(whole.c) == 15


@pytest.mark.parametrize("rate", [8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000])
def test_a_full_scale_997_hz_sine_reads_minus_3_01_lufs(rate):
    """the calibration anchor of the standard; below 48 kHz the bilinear transform warps the shelf a little"""
    x = np.sin(2 * np.pi * 997.0 * np.arange(2 * rate) / rate)
    L = loudness_ref.integrated(x, rate)
    print(f"997 Hz at {rate} Hz: {L:.4f} LUFS")
    assert abs(L - -3.01) <= (0.01 if rate == 48000 else 0.05)


@pytest.fixture(scope="module")
def speech():
    """{rate: [(input level, signal)]}: four levels per rate, between -36 and -14 LUFS"""
    out = {}
    for rate in (8000, 24000, 48000):
        base = speech_like(rate, 1.0, 1).astype(np.float64)
        L1 = loudness_ref.integrated(base, rate)
        out[rate] = []
        for want in (-36.0, -30.0, -20.0, -14.6):
            x = (base * 10.0 ** ((want - L1) / 20.0)).astype(np.float32)
            out[rate].append((loudness_ref.integrated(x, rate), x))
    return out


@pytest.mark.parametrize("rate", [8000, 24000, 48000])
def test_speech_like_signals_land_within_1_lu_of_the_target(speech, rate):
    """the property the feature exists for: inputs that span more than 15 LU come out, after the delay, within 1.0 LU of
    the target (the prototype of the contract stays within 0.69 LU on such signals)"""
    levels = [L for L, _ in speech[rate]]
    assert max(levels) - min(levels) >= 15.0 and -36.5 <= min(levels) and max(levels) <= -14.0
    for T in (-16.0, -23.0):
        for L_in, x in speech[rate]:
            y, s = loudness_ref.reference(x, rate, T)
            L_out = loudness_ref.integrated(y[s.D:], rate)
            print(f"{rate} Hz, {L_in:.2f} LUFS -> target {T:g}: {L_out:.2f} LUFS, peak {np.abs(y).max():.2f}")
            assert abs(L_out - T) <= 1.0, (rate, L_in, T, L_out)


def test_the_measurement_freezes_after_1024_gating_blocks():
    s = loudness_ref.Stream(8000, -16.0)
    x = speech_like(8000, 0.2, 3)[:8000]
    s.S, s.D = 8, 32  # a short sub-block keeps the test quick; the rule is the same
    s.frame(np.tile(x, 2)[:8 * 1030])
    assert len(s.hist) == loudness_ref.MAX_BLOCKS == 1024 and len(s.c) == 1030
    assert s.c[1027] == s.c[1026] == s.c[1029] and s.L[1029] == s.L[1026]


# ---- route(): composition, pre-roll and drain frames with every mix of stages -------------------------------------------------
def test_route_with_every_mix_of_stages():
    from pocket_tts_amd import level, loudness, pitch, stretch
    from pocket_tts_amd.output_chain import ChainTable

    for rates, speeds, pitches, lvl in itertools.product((None, [8000]), (None, [1.25]), (None, ["17/16"]), (False, True)):
        t = ChainTable(24000, 1920, rates, speeds, lvl, pitches, True)
        assert t.loud_plans is not None and t.level_plans is not None and not t.empty  # the limiter comes with the stage
        assert set(t.loud_index) == set(t.level_index)
        for rate, speed, p in itertools.product((None, 8000) if rates else (None,), (None, 1.25) if speeds else (None,),
                                                (None, "17/16") if pitches else (None,)):
            try:
                plain = t.route(rate, speed, None, None, p)
            except ValueError:
                continue  # a speed or pitch the plan rule refuses on this line
            r = t.route(rate, speed, None, -3.0, p, -16.0)
            r_hz, n = rate or 24000, plain.n_out
            assert r.loud == (t.loud_index[(r_hz, n)], -16.0) and r.level == (t.level_index[(r_hz, n)], 0.0, -3.0)
            D, LA = loudness.plan(r_hz, n).D, level.plan(r_hz, n).LA
            assert r.n_out == n and r.preroll == plain.preroll + D + LA and r.drain_frames == -(-r.preroll // n)
            assert r.drain_stage == ("stretch" if r.stretched else "pitch" if r.pitched else "loud")
            assert (r.stretch_plan, r.pitch_plan, r.rate_index) == (plain.stretch_plan, plain.pitch_plan, plain.rate_index)
            assert t.route(rate, speed, None, None, p, -16.0).level[2] == -1.0  # the default ceiling
            assert plain.loud is None and plain.level is None and plain.drain_stage in ("stretch", "pitch", None)
            g = t.route(rate, speed, 6.0, None, p)  # a gain on its own still goes through the leveler alone
            assert g.loud is None and g.level[1] == 6.0 and g.preroll == plain.preroll + LA
            with pytest.raises(ValueError, match="exclude each other"):
                t.route(rate, speed, 6.0, None, p, -16.0)
            with pytest.raises(ValueError, match=r"\[-40, -10\]"):
                t.route(rate, speed, None, None, p, -9.0)
    assert stretch and pitch
    t = ChainTable(24000, 1920, [8000], None, True)
    with pytest.raises(ValueError, match="no loudness stage"):
        t.route(None, None, None, None, None, -16.0)
    assert t.loud_plans is None and ChainTable(24000, 1920).empty
    # existing constructions of a Route stay valid
    from pocket_tts_amd.output_chain import Route

    assert Route(0, 24000, None, False, None, 1920, 0, 0, None).loud is None
    with pytest.raises(ValueError, match=r"\[8000, 48000\]"):
        ChainTable(96000, 7680, None, None, False, None, True)


def test_single_loudness():
    from pocket_tts_amd.output_chain import ChainTable

    def one(rate=None, speed=None, gain_db=None, peak_dbfs=None, loudness_lufs=None):
        got = ChainTable.for_request(24000, 1920, rate, speed, gain_db, peak_dbfs, loudness_lufs=loudness_lufs)[1]
        return got["loudness_lufs"], got["peak_dbfs"]

    assert one() == (None, None)
    assert one(None, None, None, None, -16) == (-16.0, -1.0)
    assert one(8000, 1.25, None, -6, -23.0) == (-23.0, -6.0)
    with pytest.raises(ValueError, match="exclude each other"):
        one(None, None, 3.0, None, -16)
    with pytest.raises(ValueError, match=r"\[-20, 0\]"):
        one(None, None, None, 1.0, -16)


# ---- the index functions and the chunked recurrence under a host sanitizer --------------------------------------------------
def _sweep_plans():
    from pocket_tts_amd.loudness import plan

    ns = {1, 2, 640, 800, 801, 882, 1023, 1024, 1025, 1920, 3840, 4801, 7680, 8191, 8192}
    return [plan(rate, n) for rate in (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000) for n in sorted(ns)]


def test_index_sweep_under_host_sanitizer(tmp_path):
    """every index the shared header forms, for every admitted kind of plan (n = 1, n = 8192, 11,025 Hz with S = 1102, up to
    eleven sub-blocks per frame), on exact-size heap buffers under AddressSanitizer + UBSan, and the chunked recurrence against
    the serial one"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path / "loud_sweep"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-I", str(REPO / "pocket_tts_amd" / "csrc"), "-o", str(exe),
                        str(REPO / "tests" / "cpp" / "loud_sweep.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    ps = _sweep_plans()
    assert any(p.n == 1 for p in ps) and any(p.n == 8192 and p.rate == 8000 for p in ps) and any(p.S == 1102 for p in ps)
    blob = struct.pack("<i", len(ps))
    for p in ps:
        blob += struct.pack("<ii", *p.ints()) + p.doubles().tobytes()
    (tmp_path / "plans.bin").write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # the leak checker needs ptrace, which build sandboxes often deny
    r = subprocess.run([str(exe), str(tmp_path / "plans.bin")], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    frames = sum(-(-(p.D + 3 * p.S + p.n) // p.n) for p in ps)
    assert r.stdout.strip() == f"ok {len(ps)} plans {frames} frames"


def test_the_library_refuses_what_the_rule_refuses(tmp_path):
    """ld_plan_ok and the derived sizes, compiled on the host: the plans of the rule pass with the rule's S, D and chunk, and
    each broken rule fails"""
    from pocket_tts_amd.loudness import plan

    cxx = shutil.which("g++") or shutil.which("c++")
    src = tmp_path / "ok.cpp"
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "ptts_loud.h"\nint main(int c, char **v) {\n'
                   '  for (int i = 1; i + 1 < c; i += 2) { int r = atoi(v[i]), n = atoi(v[i + 1]);\n'
                   '    if (ld_plan_ok(r, n)) printf("1 %d %d %d\\n", ld_sub(r), ld_delay(r), ld_chunk(n)); else printf("0\\n"); }\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "ok"
    r = subprocess.run([cxx, "-std=c++17", "-I", str(REPO / "pocket_tts_amd" / "csrc"), "-o", str(exe), str(src)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = [(8000, 640), (48000, 8192), (11025, 882), (24000, 1), (44100, 3528),        # admitted
             (7999, 640), (48001, 1920), (24000, 0), (24000, 8193), (0, 0), (-8000, 640)]  # refused
    out = subprocess.run([str(exe), *[str(v) for c in cases for v in c]], capture_output=True, text=True, timeout=60).stdout
    for (rate, n), line in zip(cases, out.strip().splitlines(), strict=True):
        try:
            p = plan(rate, n)
            assert line == f"1 {p.S} {p.D} {p.chunk}", (rate, n, line)
        except ValueError:
            assert line == "0", (rate, n, line)


# ---- the server's fields against a stub batcher ----------------------------------------------------------------------------
class _StubRequest:
    def __init__(self, n, samples):
        self.n, self.samples = n, samples

    def iter_batches(self):
        for i in range(self.n):
            yield [torch.full((self.samples,), i, dtype=torch.int16)]


class _StubBatcher:
    def __init__(self):
        self.submitted, self.started, self.closed = [], False, False

    def start(self):
        self.started = True

    def close(self):
        self.closed = True

    def exclusive(self, fn, *a, **k):
        return fn(*a, **k)

    def submit(self, state, text, fae=None, **settings):
        if settings.get("loudness_lufs") is not None and fae is not None and fae < 1:  # the batcher's own refusal
            raise ValueError("a request with a loudness target needs frames_after_eos >= 1")
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


def test_server_loudness_fields(tmp_path):
    forms = [{"text": "hi", "loudness_lufs": "-16"}, {"text": "hi", "loudness_lufs": " -23.5 ", "peak_dbfs": "-3"},
             {"text": "hi"}, {"text": "hi", "loudness_lufs": "", "gain_db": ""},
             {"text": "hi", "loudness_lufs": "-16", "sample_rate": "8000"}, {"text": "hi", "gain_db": "6"}]
    res, index, stub = _run_app(tmp_path, forms, sample_rates=[8000], loudness=True, level=True)
    assert [r.status_code for r in res] == [200] * 6
    assert [(s.get("loudness_lufs"), s.get("gain_db"), s.get("peak_dbfs")) for s in stub.submitted] == \
        [(-16.0, None, -1.0), (-23.5, None, -3.0), (None, None, None), (None, None, None), (-16.0, None, -1.0),
         (None, 6.0, -1.0)]
    assert all("loudness_lufs" not in s and "peak_dbfs" not in s for s in stub.submitted[2:4])  # a request like before
    for r, rate in zip(res, [24000, 24000, 24000, 24000, 8000, 24000]):
        n = 1920 * rate // 24000
        assert struct.unpack("<L", r.content[24:28])[0] == rate
        assert len(r.content) == 44 + 3 * n * 2 + 2 * int(rate * 0.2)  # header, chunks and silence are those of before
    assert 'name="loudness_lufs"' in index.text


def test_server_loudness_400(tmp_path):
    bad = [{"text": "hi", "loudness_lufs": "loud"}, {"text": "hi", "loudness_lufs": "nan"}, {"text": "hi", "loudness_lufs": "-9"},
           {"text": "hi", "loudness_lufs": "-41"}, {"text": "hi", "loudness_lufs": "-16", "peak_dbfs": "0.5"},
           {"text": "hi", "loudness_lufs": "-16", "peak_dbfs": "low"}, {"text": "hi", "loudness_lufs": "-16", "gain_db": "6"},
           {"text": "hi", "loudness_lufs": "-16", "frames_after_eos": "0"}]
    res, _, stub = _run_app(tmp_path, bad, loudness=True, level=True)
    assert [r.status_code for r in res] == [400] * 8 and not stub.submitted
    d = [r.json()["detail"] for r in res]
    assert "must be a number" in d[0] and "finite" in d[1] and "[-40, -10]" in d[2] and "[-40, -10]" in d[3]
    assert "[-20, 0]" in d[4] and "must be a number" in d[5] and "exclude each other" in d[6]
    assert "frames_after_eos >= 1" in d[7]  # what submit refuses reaches the client as a 400
    # a server without loudness refuses the field
    res, _, stub = _run_app(tmp_path, [{"text": "hi", "loudness_lufs": "-16"}, {"text": "hi"}])
    assert [r.status_code for r in res] == [400, 200] and "without loudness" in res[0].json()["detail"]
    assert stub.submitted == [{"temperature": None, "noise_clamp": None, "eos_threshold": None}]
    # a line the rule refuses is refused when the server starts
    from pocket_tts_amd.server import create_app

    class _Big(_StubModel):
        sample_rate = 96000
        engine = SimpleNamespace(frame_samples=7680)

    with pytest.raises(ValueError, match=r"\[8000, 48000\]"):
        create_app(_Big(), slots=1, capacity=64, batcher_factory=lambda m, s, c: None, loudness=True)


def test_cli_flags():
    from pocket_tts_amd.main import build_parser

    ap = build_parser()
    a = ap.parse_args(["generate", "--loudness-lufs", "-16", "--peak-dbfs", "-3"])
    assert (a.loudness_lufs, a.peak_dbfs, a.gain_db) == (-16.0, -3.0, None)
    assert ap.parse_args(["generate"]).loudness_lufs is None
    assert ap.parse_args(["serve", "--loudness"]).loudness is True and ap.parse_args(["serve"]).loudness is False
    with pytest.raises(SystemExit):
        ap.parse_args(["generate", "--loudness-lufs", "loud"])


@pytest.mark.parametrize("extra", [["--loudness-lufs", "-5"], ["--loudness-lufs", "nan"], ["--loudness-lufs", "-16", "--gain-db", "3"],
                                   ["--loudness-lufs", "-16", "--peak-dbfs", "1"]])
def test_cli_refuses_an_inadmissible_target_before_it_opens_the_output(tmp_path, monkeypatch, extra):
    """`generate_audio_stream` is a generator: it would raise only once the WAV file exists"""
    from pocket_tts_amd import main, tts_model

    class _Model(SimpleNamespace):
        def get_state_for_audio_prompt(self, voice):
            raise AssertionError("the target is checked before any work for the request")

    monkeypatch.setattr(tts_model.TTSModel, "load_model",
                        staticmethod(lambda **kw: _Model(sample_rate=24000, engine=SimpleNamespace(frame_samples=1920))))
    out = tmp_path / "out.wav"
    assert main.cli_app(["generate", "--text", "hi", *extra, "--output-path", str(out), "-q"]) == 1
    assert not out.exists()


def test_cli_passes_the_target_on(tmp_path, monkeypatch):
    from pocket_tts_amd import main, tts_model

    seen = {}

    class _Model(SimpleNamespace):
        def get_state_for_audio_prompt(self, voice):
            return {}

        def generate_audio_stream(self, state, text, **kw):
            seen.update(kw)
            return iter([torch.zeros(1920)])

    monkeypatch.setattr(tts_model.TTSModel, "load_model",
                        staticmethod(lambda **kw: _Model(sample_rate=24000, engine=SimpleNamespace(frame_samples=1920))))
    out = tmp_path / "out.wav"
    assert main.cli_app(["generate", "--text", "hi", "--loudness-lufs", "-16", "--peak-dbfs", "-2", "--output-path", str(out), "-q"]) == 0
    assert (seen["loudness_lufs"], seen["peak_dbfs"], seen["gain_db"]) == (-16.0, -2.0, None) and out.exists()
