"""The leveler's true-peak mode without a GPU: the interpolator's table, the 4x meter `level.true_peak`, the float64 reference
(tests/truepeak_ref.py) and the property the mode is for, the rule and its refusals, `Route.preroll` / `drain_frames`,
`ChainTable.for_request`'s canonical form, the server's field against a stub batcher, the CLI flags, and the kernel's new
index functions swept on the CPU under a host sanitizer (a stand-alone C++ program run as a child process)."""

import asyncio
import os
import shutil
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import level_ref
import truepeak_ref as R

REPO = Path(__file__).resolve().parents[1]
LINES = [(8000, 640), (11025, 882), (24000, 1920), (48000, 3840)]


# ---- the table and the meter ------------------------------------------------------------------------------------------------
def test_the_taps_are_the_resamplers_4x_filter():
    from pocket_tts_amd import level, resample

    h = resample.prototype(4, 1)
    assert h.shape == (81,) and np.allclose(h, h[::-1], rtol=0, atol=1e-15)  # linear phase: a delay of 40 = 10 input samples
    assert abs(h[40] - 1) < 1e-3 and np.abs(np.delete(h[0::4], 10)).max() < 1e-15  # phase 0: a pure delay up to normalisation
    t = level.TP_TAPS
    assert t.shape == (3, 21) and t.dtype == np.float32 and not t.flags.writeable
    for p in (1, 2, 3):
        want = np.zeros(21)
        want[:len(h[p::4])] = h[p::4]
        assert np.array_equal(t[p - 1], want.astype(np.float32))
    assert (t[:, 20] == 0).all() and level.TP_DELAY == 10 and level.TP_NTAPS == 21
    assert level.TP_S == np.abs(t.astype(np.float64)).sum(axis=1).max() and 2.24 < level.TP_S < 2.25
    assert np.allclose(t.astype(np.float64).sum(axis=1), 1.0, atol=5e-4)  # unity gain at 0 Hz: levels read true


def test_true_peak_reads_the_waveform_between_the_samples():
    from pocket_tts_amd.level import dbtp, true_peak

    n = np.arange(4000)
    ramp = np.minimum(1.0, np.minimum(n, n[::-1]) / 400.0)  # no onset click
    x = 0.5 * np.sin(0.5 * np.pi * n + 0.25 * np.pi) * ramp
    assert np.abs(x).max() < 0.3536 and abs(true_peak(x) / 0.5 - 1) < 2e-3   # the textbook 3 dB
    assert abs(dbtp(true_peak(x)) - 20 * np.log10(0.5)) < 0.02
    slow = 0.5 * np.sin(2 * np.pi * 0.01 * n) * ramp
    assert abs(true_peak(slow) / 0.5 - 1) < 1e-3                              # nothing to find on a slow sine
    assert true_peak([]) == 0.0 and true_peak(np.zeros(5)) == 0.0 and dbtp(0.0) == -np.inf
    assert true_peak(np.array([0, 16384, 0], np.int16)) == pytest.approx(true_peak(np.array([0, 0.5, 0])))
    assert true_peak([0.1, np.nan, 0.2] + [0.0] * 30 + [0.3]) == pytest.approx(0.3, rel=0.05)  # NaN is skipped
    y = level_ref.signal(3000, seed=5)
    assert true_peak(y) == pytest.approx(R.meter(np.concatenate([y, np.zeros(20)]), __import__("pocket_tts_amd.level").level.TP_TAPS))


# ---- the reference and the property -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("line", LINES)
def test_reference_properties(line):
    from pocket_tts_amd.level import TP_TAPS, params, plan

    p = plan(*line, True)
    G, C = params(12.0, -1.0)
    x = level_ref.gpu_signal(*line)
    y, u, P, r, g, M = R.level_tp(x, G, C, p.LA, p.a, p.k, TP_TAPS, full=True)
    assert not y[:p.preroll].any() and y[p.preroll] == g[p.preroll] * u[0]
    assert np.abs(y).max() <= float(C) * (1 + 2.0 ** -23)                  # the sample-peak bound still holds
    assert np.all(P[10:] >= np.abs(u[:-10]))                               # because the detector never reads less
    assert M == R.meter(y, TP_TAPS) and M >= np.abs(y[:-10]).max()
    quiet = (x * 0.01).astype(np.float32)                                  # under the ceiling: a delay and a gain
    yq = R.level_tp(quiet, G, C, p.LA, p.a, p.k, TP_TAPS)
    want = np.concatenate([np.zeros(p.preroll), float(G) * quiet.astype(np.float64)])[:len(x)]
    assert np.abs(yq - want).max() <= 2.0 ** -22 * np.abs(want).max()


@pytest.mark.parametrize("name", R.PROPERTY_INPUTS)
@pytest.mark.parametrize("line", [(8000, 640), (24000, 1920), (48000, 3840)])
def test_the_reference_holds_the_true_peak_where_the_sample_peak_limiter_does_not(line, name):
    """+12 dB under -1 dB: the excess of the float64 reference over the ceiling by the 4x meter, which DESIGN.md quotes, is
    hundredths of a dB at the most on every input; the sample-peak limiter overshoots by 3 dB on the fs / 4 sine"""
    from pocket_tts_amd.level import TP_TAPS, params, plan, true_peak

    rate, n = line
    p = plan(rate, n, True)
    G, C = params(12.0, -1.0)
    x = np.concatenate([R.property_input(name, rate, 5 * n), np.zeros(n, np.float32)])
    tp = true_peak(R.level_tp(x, G, C, p.LA, p.a, p.k, TP_TAPS)) / float(C)
    sp = true_peak(R.level_sp(x, G, C, p.LA, p.a, p.k)) / float(C)
    print(f"{line} {name}: true-peak mode {20 * np.log10(tp):+.4f} dB, sample-peak mode {20 * np.log10(sp):+.3f} dB over the ceiling")
    assert 20 * np.log10(tp) <= 0.02
    if name == "sine":
        assert 20 * np.log10(sp) >= 2.9
    if name == "noise":
        assert 20 * np.log10(sp) >= 1.5


def test_a_nan_costs_one_sample_in_the_reference():
    from pocket_tts_amd.level import TP_TAPS, params, plan

    p = plan(24000, 1920, True)
    G, C = params(12.0, -1.0)
    x = level_ref.gpu_signal(24000, 1920)
    x[3000] = np.nan
    y, u, P, r, g, M = R.level_tp(x, G, C, p.LA, p.a, p.k, TP_TAPS, full=True)
    assert np.flatnonzero(np.isnan(y)).tolist() == [3000 + p.preroll]
    assert np.flatnonzero(np.isnan(P)).tolist() == [3010] and r[3010] == 1.0
    at = np.r_[3000:3010, 3011:3021]
    assert np.array_equal(P[at], np.abs(u[at - 10]))  # the sample peak where the window holds the NaN
    assert np.isfinite(M)


def test_the_error_bound_is_the_docstrings():
    from pocket_tts_amd.level import TP_S, tp_error_bound

    assert tp_error_bound(120, 0.5, 0.89) == (120 + 64) * 2.0 ** -24 + 22 * 2.0 ** -24 * TP_S           # max|u| <= C: no factor
    assert tp_error_bound(120, 3.56, 0.89) == pytest.approx((184 + 22 * TP_S * 4) * 2.0 ** -24)


# ---- the rule and its refusals ----------------------------------------------------------------------------------------------
def test_rule_and_refusals():
    from pocket_tts_amd.level import check, plan

    assert check(6, None, -2) == (6.0, -2.0) and check(0, None, 0) == (0.0, 0.0) and check(6, None, -20) == (6.0, -20.0)
    with pytest.raises(ValueError, match="exclude each other"):
        check(6, -1, -1)
    for bad in (0.1, -20.5):
        with pytest.raises(ValueError, match=r"peak_dbtp .*must be in \[-20, 0\]"):
            check(6, None, bad)
    for bad in ("x", True, float("nan")):
        with pytest.raises(ValueError, match="peak_dbtp must be a finite number"):
            check(6, None, bad)
    with pytest.raises(ValueError, match="peak_dbtp is only meaningful together with gain_db"):
        check(None, None, -1)
    with pytest.raises(ValueError, match=r"gain_db .*must be in \[-40, 24\]"):
        check(30, None, -1)
    for rate, n, LA in ((8000, 640, 40), (11025, 882, 56), (48000, 3840, 240)):
        p, q = plan(rate, n, True), plan(rate, n)
        assert (p.LA, p.preroll, p.drain_frames, p.true_peak) == (LA, LA + 10, 1, True)
        assert (q.preroll, q.true_peak) == (LA, False) and p.ints() == q.ints()
    assert plan(8000, 50, True).preroll == 50 and plan(8000, 49).n == 49
    with pytest.raises(ValueError, match="shorter than the look-ahead of 40 plus the true-peak detector's delay of 10"):
        plan(8000, 49, True)
    with pytest.raises(ValueError, match="shorter than the look-ahead of 40$"):
        plan(8000, 39, True)


def test_route_preroll_and_drain_frames():
    from pocket_tts_amd.output_chain import ChainSpec

    t = ChainSpec(sample_rates=[8000, 48000], loudness=True, true_peak=True).table(24000, 1920)
    assert t.true_peak and t.level_plans is not None and not t.empty
    for rate, n, LA in ((8000, 640, 40), (None, 1920, 120), (48000, 3840, 240)):
        a, b = t.route(sample_rate=rate, gain_db=6, peak_dbtp=-2), t.route(sample_rate=rate, gain_db=6, peak_dbfs=-2)
        assert (a.preroll, a.drain_frames, a.drain_stage, a.true_peak, a.n_out) == (LA + 10, 1, "level", True, n)
        assert (b.preroll, b.true_peak) == (LA, False) and a.level == b.level == (b.level[0], 6.0, -2.0)
        assert a.take(0, None) == (LA + 10, n) and a.take(n, 1) == (0, LA + 10)
    D = t.loud_plans[t.loud_index[(8000, 640)]].D
    r = t.route(sample_rate=8000, loudness_lufs=-16, peak_dbtp=-1)
    assert r.preroll == D + 50 and r.drain_frames == -(-(D + 50) // 640) and r.drain_stage == "loud" and r.true_peak
    assert r.level == (t.level_index[(8000, 640)], 0.0, -1.0)
    assert not t.route().true_peak and t.route().level is None and t.route().preroll == 0
    with pytest.raises(ValueError, match="exclude each other"):
        t.route(gain_db=6, peak_dbfs=-1, peak_dbtp=-1)
    with pytest.raises(ValueError, match="only meaningful together with gain_db"):
        t.route(peak_dbtp=-1)
    with pytest.raises(ValueError, match=r"\[-20, 0\]"):
        t.route(gain_db=6, peak_dbtp=-21)
    for spec in (ChainSpec(level=True), ChainSpec(loudness=True), ChainSpec()):
        with pytest.raises(ValueError, match="true_peak=True"):
            spec.table(24000, 1920).route(gain_db=None if spec == ChainSpec() else 6, peak_dbtp=-1)
    # the option brings the leveler, and a tag of its own
    only = ChainSpec(true_peak=True)
    assert only.tags() == ("tp",) and only.table(24000, 1920).route(gain_db=3, peak_dbtp=-1).preroll == 130
    assert ChainSpec(level=True, true_peak=True).tags() == ("level", "tp") and ChainSpec(level=True).tags() == ("level",)
    # a line the mode's rule refuses: 1920 samples at 0.5x of 8 kHz ... is fine; a frame shorter than LA + 10 is not
    short = ChainSpec(true_peak=True).table(8000, 45)
    assert short.route(gain_db=3).preroll == 40
    with pytest.raises(ValueError, match="plus the true-peak detector's delay"):
        short.route(gain_db=3, peak_dbtp=-1)


def test_for_request_canonical_form():
    from pocket_tts_amd.output_chain import ChainSpec, ChainTable, RequestError

    spec, req = ChainTable.for_request(24000, 1920, loudness_lufs=-16, peak_dbtp=-1)
    assert spec == ChainSpec(loudness=True, true_peak=True)
    assert req == dict(sample_rate=None, speed=None, gain_db=None, peak_dbfs=None, pitch=None, loudness_lufs=-16.0, encoding=None,
                       tone=None, peak_dbtp=-1.0)
    assert spec.table(24000, 1920).route(**req).true_peak
    spec, req = ChainTable.for_request(24000, 1920, sample_rate=8000, gain_db=6, peak_dbtp=-3, encoding="mulaw")
    assert spec.true_peak and spec.level and (req["gain_db"], req["peak_dbfs"], req["peak_dbtp"]) == (6.0, None, -3.0)
    assert spec.table(24000, 1920).route(**req).preroll == 50
    spec, req = ChainTable.for_request(24000, 1920, tone="warm", peak_dbtp=-2)  # the limiter behind the tone, at the ceiling
    assert (req["gain_db"], req["peak_dbtp"]) == (0.0, -2.0) and spec.true_peak
    spec, req = ChainTable.for_request(24000, 1920, dynamics="speech", peak_dbtp=-2)
    assert (req["gain_db"], req["peak_dbtp"], req["peak_dbfs"]) == (0.0, -2.0, None)
    # without the field the request is the dict it always was
    spec, req = ChainTable.for_request(24000, 1920, gain_db=6)
    assert "peak_dbtp" not in req and not spec.true_peak and req["peak_dbfs"] == -1.0
    for kw, field, msg in ((dict(gain_db=6, peak_dbfs=-1, peak_dbtp=-1), "peak_dbtp", "exclude each other"),
                           (dict(loudness_lufs=-16, peak_dbfs=-1, peak_dbtp=-1), "peak_dbtp", "exclude each other"),
                           (dict(peak_dbtp=-1), "peak_dbtp", "together with gain_db"),
                           (dict(gain_db=6, peak_dbtp=0.5), "peak_dbtp", r"\[-20, 0\]"),
                           (dict(gain_db=60, peak_dbtp=-1), "peak_dbtp", r"\[-40, 24\]")):
        with pytest.raises(RequestError, match=msg) as e:
            ChainTable.for_request(24000, 1920, **kw)
        assert e.value.field == field
    with pytest.raises(RequestError, match="plus the true-peak detector's delay") as e:
        ChainTable.for_request(8000, 45, gain_db=6, peak_dbtp=-1)
    assert e.value.field == "peak_dbtp"


# ---- the server's field against a stub batcher --------------------------------------------------------------------------------
class _StubRequest:
    def iter_batches(self):
        for i in range(3):
            yield [torch.full((1920,), i, dtype=torch.int16)]


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
        return _StubRequest()


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


def test_server_field(tmp_path):
    forms = [{"text": "hi", "loudness_lufs": "-16", "peak_dbtp": "-1"}, {"text": "hi", "gain_db": "6", "peak_dbtp": " -2.5 "},
             {"text": "hi", "tone": "warm", "peak_dbtp": "-3"}, {"text": "hi", "gain_db": "6", "peak_dbfs": "-3"},
             {"text": "hi", "gain_db": "6", "peak_dbtp": ""}, {"text": "hi"}]
    res, index, stub = _run_app(tmp_path, forms, loudness=True, tones=["warm"], true_peak=True)
    assert [r.status_code for r in res] == [200] * 6, [r.text[:200] for r in res]
    got = [{k: s[k] for k in ("gain_db", "loudness_lufs", "tone", "peak_dbfs", "peak_dbtp") if k in s} for s in stub.submitted]
    assert got == [dict(loudness_lufs=-16.0, peak_dbtp=-1.0), dict(gain_db=6.0, peak_dbtp=-2.5),
                   dict(tone=got[2]["tone"], peak_dbtp=-3.0), dict(gain_db=6.0, peak_dbfs=-3.0), dict(gain_db=6.0, peak_dbfs=-1.0),
                   {}]
    assert 'name="peak_dbtp"' in index.text


def test_server_400(tmp_path):
    bad = [{"text": "hi", "gain_db": "6", "peak_dbfs": "-1", "peak_dbtp": "-1"},
           {"text": "hi", "loudness_lufs": "-16", "peak_dbfs": "-1", "peak_dbtp": "-1"},
           {"text": "hi", "gain_db": "6", "peak_dbtp": "0.5"}, {"text": "hi", "gain_db": "6", "peak_dbtp": "low"},
           {"text": "hi", "peak_dbtp": "-1"}]
    res, _, stub = _run_app(tmp_path, bad, loudness=True, true_peak=True)
    assert [r.status_code for r in res] == [400] * 5 and not stub.submitted
    d = [r.json()["detail"] for r in res]
    assert "exclude each other" in d[0] and "exclude each other" in d[1] and "[-20, 0]" in d[2] and "must be a number" in d[3]
    assert "together with gain_db" in d[4]
    # a server started without true_peak refuses the field, whatever else it has
    for kw in (dict(level=True, loudness=True), {}):
        res, _, stub = _run_app(tmp_path, [{"text": "hi", "gain_db": "6", "peak_dbtp": "-1"}, {"text": "hi", "peak_dbtp": "-1"}], **kw)
        assert [r.status_code for r in res] == [400, 400] and not stub.submitted
        assert any("without true_peak" in r.json()["detail"] for r in res)


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
def test_cli_flags():
    from pocket_tts_amd.main import FLAGS, build_parser

    ap = build_parser()
    a = ap.parse_args(["generate", "--loudness-lufs", "-16", "--peak-dbtp", "-1"])
    assert (a.loudness_lufs, a.peak_dbtp, a.peak_dbfs) == (-16.0, -1.0, None)
    assert ap.parse_args(["generate"]).peak_dbtp is None
    assert ap.parse_args(["serve", "--true-peak"]).true_peak is True and ap.parse_args(["serve"]).true_peak is False
    with pytest.raises(SystemExit):
        ap.parse_args(["generate", "--peak-dbtp", "low"])
    assert FLAGS["peak_dbtp"] == "--peak-dbtp"


@pytest.mark.parametrize("extra", [["--gain-db", "6", "--peak-dbfs", "-1", "--peak-dbtp", "-1"], ["--peak-dbtp", "-1"],
                                   ["--loudness-lufs", "-16", "--peak-dbtp", "1"]])
def test_cli_refuses_before_it_opens_the_output(tmp_path, monkeypatch, caplog, extra):
    from pocket_tts_amd import main, tts_model

    class _Model(SimpleNamespace):
        def get_state_for_audio_prompt(self, voice):
            raise AssertionError("the ceiling is checked before any work for the request")

    monkeypatch.setattr(tts_model.TTSModel, "load_model",
                        staticmethod(lambda **kw: _Model(sample_rate=24000, engine=SimpleNamespace(frame_samples=1920))))
    out = tmp_path / "out.wav"
    assert main.cli_app(["generate", "--text", "hi", *extra, "--output-path", str(out)]) == 1
    assert not out.exists()


# ---- the index functions under a host sanitizer ----------------------------------------------------------------------------------
def test_index_sweep_under_host_sanitizer(tmp_path):
    """every pair (n, LA) the mode admits, every tile, on exact-size heap buffers under AddressSanitizer + UBSan"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path / "level_tp_sweep"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-I", str(REPO / "pocket_tts_amd" / "csrc"), "-o", str(exe),
                        str(REPO / "tests" / "cpp" / "level_tp_sweep.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # the leak checker needs ptrace, which build sandboxes often deny
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    pairs = sum(8192 - (LA + 10) + 1 for LA in range(1, 513))
    assert r.stdout.strip().startswith(f"ok {pairs} pairs ") and r.stdout.strip().endswith(" tiles")
