"""Per-request tone without a GPU: the grammar, the presets and the coefficients of `pocket_tts_amd/tone.py` against the
tests' own restatement (`tone_ref.py`) and, where it imports, scipy; the plan's powers; `route()` with the stages the tone
combines with; the server's `tone` field against a stub batcher; the CLI flags; and the kernel's index functions and chunked
recurrence swept on the CPU under a host sanitizer (a stand-alone C++ program run as a child process)."""

import asyncio
import math
import os
import re
import shutil
import struct
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tone_ref

REPO = Path(__file__).resolve().parents[1]
EIGHT = "hp:40;peak:200:6:4;peak:500:-6:2;peak:1000:3;peak:2000:-3:8;lowshelf:300:4;highshelf:3000:-4;lp:3500"
# the stage-level shapes of tests/test_gpu_tone.py
GPU_SHAPES = [(24000, 1920, "telephone"), (8000, 640, "telephone"), (11025, 882, "lowshelf:200:6"), (24000, 1025, EIGHT),
              (48000, 7680, "hp:40;peak:3000:6:4;highshelf:8000:-6")]


# ---- grammar, presets, canonical form ---------------------------------------------------------------------------------------
def test_canonical_form():
    from pocket_tts_amd import tone

    assert tone.normalise(None) is None and tone.normalise("") is None and tone.normalise(" Flat ") is None
    assert tone.normalise(" Telephone ") == "telephone"  # a preset stays a name
    r2 = repr(math.sqrt(0.5))
    assert tone.normalise("HP:120") == f"hp:120.0:{r2}"
    assert tone.normalise("hp:120;Peak:3000:4") == f"hp:120.0:{r2};peak:3000.0:4.0:1.0"
    assert tone.normalise("lowshelf:2e2:-3:0.5 ; lp:3400:2") == "lowshelf:200.0:-3.0:0.5;lp:3400.0:2.0"
    for spec in ["telephone", "hp:120;peak:3000:4", "highshelf:5000:4:0.9"]:
        assert tone.normalise(tone.normalise(spec)) == tone.normalise(spec)  # a fixed point
    assert tone.normalise_tones(["telephone", "flat", "Telephone", "hp:120", "hp:120.0"]) == ["telephone", f"hp:120.0:{r2}"]


def test_presets_expand_to_the_bands_of_the_issue():
    from pocket_tts_amd import tone

    assert list(tone.PRESETS) == ["telephone", "warm", "bright", "presence", "small_speaker", "deess"]
    r2 = math.sqrt(0.5)
    assert tone.bands("telephone") == [("hp", 300.0, None, 0.5411961), ("hp", 300.0, None, 1.3065630),
                                       ("lp", 3400.0, None, 0.5411961), ("lp", 3400.0, None, 1.3065630)]
    assert tone.bands("warm") == [("lowshelf", 200.0, 3.0, r2), ("highshelf", 6000.0, -3.0, r2)]
    assert tone.bands("bright") == [("highshelf", 5000.0, 4.0, r2)]
    assert tone.bands("presence") == [("hp", 80.0, None, r2), ("peak", 3000.0, 4.0, 1.0)]
    assert tone.bands("small_speaker") == [("hp", 180.0, None, r2), ("peak", 2500.0, 3.0, 0.8)]
    assert tone.bands("deess") == [("peak", 6500.0, -6.0, 2.0)]
    assert tone.bands(None) == [] and tone.bands("flat") == []
    for name in tone.PRESETS:  # the restatement holds the same numbers
        assert tone.bands(name) == tone_ref.parse(name)


@pytest.mark.parametrize("spec,words", [
    ("loud", "neither a preset"), ("notch:100:3", "neither a preset"), ("hp", "must read hp:f0[:q]"),
    ("hp:", "must read hp:f0[:q]"), ("hp:100:1:2", "must read hp:f0[:q]"), ("peak:1000:3:1:1", "must read peak:f0:gain_db[:q]"),
    ("peak:1000", "needs a gain"), ("lowshelf:200", "needs a gain"), ("highshelf:200:", "needs a gain"),
    ("hp:abc", "f0 of band 'hp:abc' must be a number"), ("hp:19.9", "f0 of band 'hp:19.9' must be in [20, 21600]"),
    ("hp:21601", "must be in [20, 21600]"), ("hp:nan", "must be in [20, 21600]"),
    ("peak:1000:24.5", "gain_db of band 'peak:1000:24.5' must be in [-24, 24]"), ("peak:1000:-25", "must be in [-24, 24]"),
    ("peak:1000:x", "gain_db of band 'peak:1000:x' must be a number"),
    ("hp:100:0.09", "q of band 'hp:100:0.09' must be in [0.1, 16]"), ("peak:1000:3:16.5", "must be in [0.1, 16]"),
    ("hp:100;;lp:3000", "neither a preset"), (";".join(["hp:100"] * 9), "9 sections, at most 8"),
    ("telephone;hp:100", "neither a preset"),
])
def test_refusals_name_their_rule(spec, words):
    from pocket_tts_amd import tone

    with pytest.raises(ValueError) as e:
        tone.normalise(spec)
    assert words in str(e.value) and "tone" in str(e.value)


def test_limits_are_inclusive_and_non_strings_are_refused():
    from pocket_tts_amd import tone

    assert tone.normalise("peak:20:24:16") and tone.normalise("peak:21600:-24:0.1")
    assert len(tone.bands(";".join(["hp:100"] * 8))) == 8
    for bad in (3, 1.5, True, ["telephone"]):
        with pytest.raises(ValueError, match="preset's name or a band list"):
            tone.normalise(bad)
    with pytest.raises(ValueError, match="list of tones"):
        tone.normalise_tones("telephone")


def test_admissibility_depends_on_the_rate():
    from pocket_tts_amd import tone

    with pytest.raises(ValueError) as e:
        tone.plan(8000, 640, "bright")
    msg = str(e.value)
    assert "'bright' is not admissible at 8000 Hz" in msg and "highshelf at 5000 Hz" in msg and "0.45" in msg
    assert "['telephone', 'presence', 'small_speaker']" in msg  # what that rate admits
    assert tone.presets_at(8000) == ["telephone", "presence", "small_speaker"]
    assert tone.presets_at(16000) == list(tone.PRESETS) and tone.plan(16000, 1280, "bright").K == 1
    with pytest.raises(ValueError, match=r"f0 must be in \[20, 3600\] there"):
        tone.plan(8000, 640, "hp:3601")
    assert tone.plan(8000, 640, "hp:3600").K == 1  # 0.45 x rate itself is admitted
    for rate, n, words in [(7999, 640, "rate must be in [8000, 48000]"), (48001, 640, "rate must be in"),
                           (24000, 0, "not in [1, 8192]"), (24000, 8193, "not in [1, 8192]")]:
        with pytest.raises(ValueError) as e:
            tone.plan(rate, n, "hp:100")
        assert words in str(e.value)
    with pytest.raises(ValueError, match="bypass has no plan"):
        tone.plan(24000, 1920, "flat")


# ---- coefficients -------------------------------------------------------------------------------------------------------------
ALL_SPECS = ["telephone", "warm", "bright", "presence", "small_speaker", "deess", "hp:40", "lp:20:16", "peak:20:24:16",
             "peak:9000:-24:0.1", "lowshelf:200:6", "highshelf:8000:-6:2", EIGHT]


@pytest.mark.parametrize("rate", [8000, 11025, 16000, 24000, 44100, 48000])
def test_coefficients_equal_the_restatement(rate):
    from pocket_tts_amd import tone

    seen = 0
    for spec in ALL_SPECS:
        if any(f0 > 0.45 * rate for _, f0, _, _ in tone_ref.parse(spec)):
            continue
        got, want = tone.coefficients(spec, rate), tone_ref.coefficients(spec, rate)
        assert got.dtype == np.float64 and got.shape == want.shape == (len(tone_ref.parse(spec)), 5)
        assert np.all(np.abs(got - want) <= 1e-15 * np.abs(want)), spec
        seen += 1
    assert seen >= 6


def _gain_db(c, f, rate):
    z = np.exp(-2j * np.pi * f / rate)
    return 20.0 * np.log10(abs((c[0] + c[1] * z + c[2] * z * z) / (1.0 + c[3] * z + c[4] * z * z)))


def test_the_responses_are_those_the_kinds_promise():
    """what the issue checked with freqz at 24 kHz: the shelves give gain_db at DC and at Nyquist and half of it at f0, the
    peak gain_db at f0, hp and lp -3.01 dB at f0 with q = 1 / sqrt(2); all poles inside the unit circle"""
    from pocket_tts_amd import tone

    rate = 24000
    lo, hi = tone.section("lowshelf", 200.0, 6.0, math.sqrt(0.5), rate), tone.section("highshelf", 5000.0, -4.0, math.sqrt(0.5), rate)
    assert abs(_gain_db(lo, 0.0, rate) - 6.0) < 1e-9 and abs(_gain_db(lo, 12000.0, rate)) < 1e-9
    assert abs(_gain_db(lo, 200.0, rate) - 3.0) < 1e-9
    assert abs(_gain_db(hi, 12000.0, rate) + 4.0) < 1e-9 and abs(_gain_db(hi, 0.0, rate)) < 1e-9
    assert abs(_gain_db(hi, 5000.0, rate) + 2.0) < 1e-9
    assert abs(_gain_db(tone.section("peak", 3000.0, 4.0, 1.0, rate), 3000.0, rate) - 4.0) < 1e-9
    for kind in ("hp", "lp"):
        assert abs(_gain_db(tone.section(kind, 1000.0, None, math.sqrt(0.5), rate), 1000.0, rate) + 3.0103) < 1e-4
    for spec in ALL_SPECS:
        for c in tone.coefficients(spec, 48000):
            assert np.abs(np.roots([1.0, c[3], c[4]])).max() < 1.0, spec


def test_the_serial_definition_against_scipy():
    signal = pytest.importorskip("scipy.signal")
    from pocket_tts_amd import tone

    x = np.random.default_rng(5).standard_normal(24000) * 0.25
    for spec in ["telephone", "presence", EIGHT]:
        c = tone.coefficients(spec, 24000)
        sos = np.array([[b0, b1, b2, 1.0, a1, a2] for b0, b1, b2, a1, a2 in c])
        want = signal.sosfilt(sos, x)  # transposed direct form II as well
        got, _ = tone.run(c, x)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), spec
        ref = tone_ref.reference(spec, 24000, x)  # direct form I
        assert np.abs(ref - want).max() <= 1e-11 * np.abs(want).max(), spec


def test_the_two_forms_agree_and_streaming_equals_the_whole_signal():
    """transposed direct form II (`tone.run`, the stage's definition) against direct form I (`tone_ref`), and `tone_ref.Stream`
    frame by frame against one call"""
    from pocket_tts_amd import tone

    x = np.random.default_rng(6).standard_normal((2, 3 * 640)) * 0.25
    c = tone.coefficients("telephone", 8000)
    whole = tone_ref.reference("telephone", 8000, x)
    st = tone_ref.Stream(tone_ref.coefficients("telephone", 8000), 2)
    assert np.array_equal(np.concatenate([st.frame(x[:, i * 640:(i + 1) * 640]) for i in range(3)], axis=1), whole)
    got, state = tone.run(c, x[0])
    assert np.abs(got - whole[0]).max() <= 1e-12 * np.abs(whole[0]).max()
    a, s = tone.run(c, x[0, :1000])  # the carried state continues the stream
    b, s = tone.run(c, x[0, 1000:], s)
    assert np.array_equal(np.concatenate([a, b]), got) and np.array_equal(s, state)


# ---- the plan -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,n,spec", GPU_SHAPES + [(44100, 1, "hp:100"), (48000, 8192, "telephone")])
def test_plan_values(rate, n, spec):
    from pocket_tts_amd import tone

    p = tone.plan(rate, n, spec)
    K = len(tone_ref.parse(spec))
    assert (p.rate, p.n, p.K, p.chunk, p.tone) == (rate, n, K, -(-n // 1024), tone.normalise(spec)) and p.ints() == (rate, n, K)
    assert p.coef.shape == (K, 5) and p.powers.shape == (K, tone.SCAN_STEPS, 2, 2) and p.powers.dtype == np.float64
    d = p.doubles()
    assert d.dtype == np.float64 and d.shape == (tone.DOUBLES_PER_PLAN,) == (360,) and np.isfinite(d).all()
    assert np.array_equal(d[:5 * K], p.coef.reshape(-1)) and not d[5 * K:40].any()
    assert np.array_equal(d[40:40 + 40 * K], p.powers.reshape(-1)) and not d[40 + 40 * K:].any()
    for k in range(K):  # A^chunk applied to a state equals `chunk` steps of the section on zero input
        s = [0.3, -0.2]
        want = p.powers[k, 0] @ np.array(s)
        for _ in range(p.chunk):
            tone.step([float(v) for v in p.coef[k]], s, 0.0)
        assert np.allclose(want, s, rtol=1e-12, atol=1e-300)
        for t in range(1, tone.SCAN_STEPS):  # each the square of the one before, up to what squaring in float64 loses
            sq = p.powers[k, t - 1] @ p.powers[k, t - 1]
            assert np.allclose(p.powers[k, t], sq, rtol=1e-9, atol=1e-9 * np.abs(sq).max() + 1e-300)


def test_table_has_the_shape_of_the_pitch_table():
    from pocket_tts_amd import tone

    tones = tone.normalise_tones(["telephone", "bright"])
    plans, index = tone.table([(24000, 1920), (8000, 640), (24000, 1920), (16000, 1280)], tones)
    assert index == {(24000, 1920): [0, 1], (8000, 640): [2, None], (16000, 1280): [3, 4]}
    assert [(p.rate, p.n, p.tone) for p in plans] == [(24000, 1920, "telephone"), (24000, 1920, "bright"), (8000, 640, "telephone"),
                                                      (16000, 1280, "telephone"), (16000, 1280, "bright")]
    with pytest.raises(ValueError, match="'bright' is not admissible at 8000 Hz"):
        tone.table([(8000, 640)], tones)  # admissible on none of the lines


# ---- ChainTable / Route -----------------------------------------------------------------------------------------------------
def test_route_a_tone_alone_brings_the_limiter():
    from pocket_tts_amd import level
    from pocket_tts_amd.output_chain import ChainTable

    t = ChainTable(24000, 1920, tones=["telephone", "bright"])
    assert t.tones == ["telephone", "bright"] and not t.empty and t.level_plans is not None and t.loud_plans is None
    LA = level.plan(24000, 1920).LA
    r = t.route(tone="telephone")
    assert (r.tone_plan, r.toned, r.level, r.preroll, r.drain_stage) == (0, True, (0, 0.0, -1.0), LA, "level")
    assert r.drain_frames == -(-LA // 1920) and r.n_out == 1920
    r = t.route(tone=" Bright ", peak_dbfs=-3)
    assert (r.tone_plan, r.level) == (1, (0, 0.0, -3.0))
    r = t.route(tone="telephone", gain_db=6)  # tone + gain compose: the request's own gain
    assert (r.tone_plan, r.level, r.preroll, r.drain_stage) == (0, (0, 6.0, -1.0), LA, "level")
    for flat in (None, "", "flat"):
        r = t.route(tone=flat)
        assert (r.tone_plan, r.toned, r.level, r.preroll, r.drain_stage) == (None, False, None, 0, None)


def test_route_tone_and_loudness_compose():
    from pocket_tts_amd import level, loudness
    from pocket_tts_amd.output_chain import ChainTable

    t = ChainTable(24000, 1920, loudness=True, tones=["warm"])
    r = t.route(tone="warm", loudness_lufs=-16)
    D, LA = loudness.plan(24000, 1920).D, level.plan(24000, 1920).LA
    assert (r.tone_plan, r.loud, r.level, r.preroll, r.drain_stage) == (0, (0, -16.0), (0, 0.0, -1.0), D + LA, "loud")
    with pytest.raises(ValueError, match="exclude each other"):
        t.route(tone="warm", loudness_lufs=-16, gain_db=3)


def test_route_an_untoned_request_is_routed_as_on_a_levelled_table():
    from pocket_tts_amd.output_chain import ChainTable, Route

    kw = dict(sample_rates=[8000, 16000], speeds=[1.25], pitches=["5/4"])
    toned = ChainTable(24000, 1920, tones=["telephone", "bright"], **kw)
    plain = ChainTable(24000, 1920, level=True, **kw)
    for req in [{}, {"sample_rate": 8000}, {"speed": 1.25, "gain_db": 3.0}, {"sample_rate": 16000, "pitch": "5/4", "gain_db": -2.0,
                                                                            "peak_dbfs": -6.0}]:
        assert toned.route(**req) == plain.route(**req)
    # Route's new fields sit at the end with defaults: positional construction as before
    r = Route(0, 24000, None, False, None, 1920, 0, 0, None)
    assert (r.tone_plan, r.toned) == (None, False)
    # over the lines the pitcher leaves: the stretched lines as well
    assert set(toned.tone_index) == {(24000, 1920), (8000, 640), (16000, 1280), (24000, 1536), (8000, 512), (16000, 1024)}


def test_route_refusals():
    from pocket_tts_amd.output_chain import ChainTable

    t = ChainTable(24000, 1920, sample_rates=[8000], tones=["telephone", "bright"])
    with pytest.raises(ValueError) as e:
        t.route(tone="warm")
    assert "'warm' is not configured" in str(e.value) and "['telephone', 'bright']" in str(e.value)
    with pytest.raises(ValueError) as e:
        t.route(sample_rate=8000, tone="bright")
    assert "not admissible at 8000 Hz (admissible there: ['telephone'])" in str(e.value)
    with pytest.raises(ValueError, match="neither a preset"):
        t.route(tone="nope:1")
    with pytest.raises(ValueError, match="no tone stage"):
        ChainTable(24000, 1920, level=True).route(tone="telephone")
    assert ChainTable(24000, 1920).route(tone="flat").toned is False  # the bypass is no tone
    with pytest.raises(ValueError, match="no tone but the bypass"):
        ChainTable(24000, 1920, tones=["flat"])
    with pytest.raises(ValueError, match="not admissible at 8000 Hz"):
        ChainTable(8000, 640, tones=["bright"])


def test_single_tone():
    from pocket_tts_amd.output_chain import ChainTable

    one = lambda rate, speed, tone: ChainTable.for_request(24000, 1920, rate, speed, tone=tone)[1]["tone"]  # noqa: E731
    assert one(None, None, None) is None
    assert one(None, None, "FLAT") is None
    assert one(8000, None, "Telephone") == "telephone"
    assert one(None, 1.25, "hp:120") == f"hp:120.0:{math.sqrt(0.5)!r}"
    with pytest.raises(ValueError, match="not admissible at 8000 Hz"):
        one(8000, None, "bright")


# ---- the server's field -------------------------------------------------------------------------------------------------------
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


def test_server_tone_field(tmp_path):
    forms = [{"text": "hi", "tone": "telephone"}, {"text": "hi", "tone": " Telephone ", "sample_rate": "8000", "peak_dbfs": "-3"},
             {"text": "hi"}, {"text": "hi", "tone": ""}, {"text": "hi", "tone": "flat"},
             {"text": "hi", "tone": "HP:120;peak:3000:4", "gain_db": "3"}, {"text": "hi", "tone": "bright", "loudness_lufs": "-16"}]
    res, index, stub = _run_app(tmp_path, forms, sample_rates=[8000], level=True, loudness=True,
                                tones=["telephone", "bright", "hp:120;peak:3000:4"])
    assert [r.status_code for r in res] == [200] * 7, [r.text for r in res]
    band = f"hp:120.0:{math.sqrt(0.5)!r};peak:3000.0:4.0:1.0"
    got = [(s.get("tone"), s.get("gain_db"), s.get("peak_dbfs"), s.get("loudness_lufs"), s.get("sample_rate")) for s in stub.submitted]
    assert got == [("telephone", None, None, None, None), ("telephone", None, -3.0, None, 8000), (None, None, None, None, None),
                   (None, None, None, None, None), (None, None, None, None, None), (band, 3.0, -1.0, None, None),
                   ("bright", None, -1.0, -16.0, None)]
    assert 'name="tone"' in index.text


def test_server_tone_400(tmp_path):
    bad = [{"text": "hi", "tone": "warm"}, {"text": "hi", "tone": "bright", "sample_rate": "8000"}, {"text": "hi", "tone": "peak:1000"},
           {"text": "hi", "tone": "telephone", "peak_dbfs": "3"}, {"text": "hi", "tone": "telephone", "peak_dbfs": "low"}]
    res, _, stub = _run_app(tmp_path, bad, sample_rates=[8000], tones=["telephone", "bright"])
    assert [r.status_code for r in res] == [400] * 5 and not stub.submitted
    d = [r.json()["detail"] for r in res]
    assert "'warm' is not configured" in d[0] and "['telephone', 'bright']" in d[0]           # the configured list
    assert "not admissible at 8000 Hz (admissible there: ['telephone'])" in d[1]              # the admissible list
    assert "needs a gain" in d[2] and "[-20, 0]" in d[3] and "must be a number" in d[4]
    # a server without tones refuses the field, and takes the bypass
    res, _, stub = _run_app(tmp_path, [{"text": "hi", "tone": "telephone"}, {"text": "hi", "tone": "flat"}, {"text": "hi"}])
    assert [r.status_code for r in res] == [400, 200, 200] and "without tones" in res[0].json()["detail"]
    assert all("tone" not in s for s in stub.submitted)
    # a tone no line admits is refused when the server starts
    from pocket_tts_amd.server import create_app

    with pytest.raises(ValueError, match="not admissible"):
        create_app(SimpleNamespace(sample_rate=8000, noise_clamp=None, engine=SimpleNamespace(frame_samples=640)), slots=1,
                   capacity=64, batcher_factory=lambda m, s, c: None, tones=["bright"])


# ---- the command line ---------------------------------------------------------------------------------------------------------
def test_cli_tone_flags(tmp_path, monkeypatch):
    from pocket_tts_amd import main, tts_model

    a = main.build_parser().parse_args(["serve", "--tones", "telephone,warm,hp:120;peak:3000:4"])
    assert a.tones == ["telephone", "warm", "hp:120;peak:3000:4"]
    with pytest.raises(SystemExit):
        main.build_parser().parse_args(["serve", "--tones", "telephone,nope"])
    seen = {}

    class _Model(SimpleNamespace):
        def get_state_for_audio_prompt(self, v):
            return {}

        def generate_audio_stream(self, state, text, **kw):
            seen.update(kw)
            return iter([torch.zeros(1920)])

    monkeypatch.setattr(tts_model.TTSModel, "load_model",
                        staticmethod(lambda **kw: _Model(sample_rate=24000, engine=SimpleNamespace(frame_samples=1920))))
    out = tmp_path / "out.wav"
    assert main.cli_app(["generate", "--text", "hi", "--tone", "Telephone", "--peak-dbfs", "-2", "--output-path", str(out), "-q"]) == 0
    assert (seen["tone"], seen["peak_dbfs"], seen["gain_db"]) == ("telephone", -2.0, None) and out.exists()
    out2 = tmp_path / "out2.wav"  # refused before the output is opened
    assert main.cli_app(["generate", "--text", "hi", "--tone", "bright", "--sample-rate", "8000", "--output-path", str(out2), "-q"]) == 1
    assert main.cli_app(["generate", "--text", "hi", "--tone", "peak:100", "--output-path", str(out2), "-q"]) == 1
    assert not out2.exists()


# ---- the header and the chunked recurrence under a host sanitizer -----------------------------------------------------------
def test_the_header_holds_the_rule_modules_constants():
    from pocket_tts_amd import tone

    text = (REPO / "pocket_tts_amd" / "csrc" / "ptts_tone.h").read_text()
    val = lambda name: int(re.search(rf"#define {name} (\d+)", text).group(1))  # noqa: E731
    assert (val("PTTS_TN_MIN_RATE"), val("PTTS_TN_MAX_RATE"), val("PTTS_TN_MAX_N")) == (tone.RATE_MIN, tone.RATE_MAX, tone.MAX_N)
    assert (val("PTTS_TN_THREADS"), val("PTTS_TN_SCAN"), val("PTTS_TN_MAX_SECTIONS")) == (tone.THREADS, tone.SCAN_STEPS, tone.MAX_SECTIONS)
    assert 1 << tone.SCAN_STEPS == tone.THREADS and tone.MAX_N == 8 * tone.THREADS


def _sweep(tmp_path, plans):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path / "tone_sweep"
    if not exe.exists():
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan", "-I", str(REPO / "pocket_tts_amd" / "csrc"), "-o", str(exe),
                            str(REPO / "tests" / "cpp" / "tone_sweep.cpp")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
    blob = struct.pack("<i", len(plans))
    for p in plans:
        blob += struct.pack("<iii", *p.ints()) + p.doubles().tobytes()
    (tmp_path / "plans.bin").write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # the leak checker needs ptrace, which build sandboxes often deny
    r = subprocess.run([str(exe), str(tmp_path / "plans.bin")], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    m = re.fullmatch(rf"ok {len(plans)} plans {12 * len(plans)} frames e64 (\S+)", r.stdout.strip())
    assert m, r.stdout
    return float(m.group(1))


def test_chunked_recurrence_under_host_sanitizer(tmp_path):
    """every index the shared header forms, on exact-size heap buffers under AddressSanitizer + UBSan, and the chunked
    recurrence against the serial one: every preset, the corners of the grammar and an eight-section tone, at n = 1, one
    sample per thread, a partial last chunk, every chunk size and n = 8192.  The program itself fails above 2^-25"""
    from pocket_tts_amd import tone

    specs = [*tone.PRESETS, "hp:20:16", "lp:20:16", "peak:20:24:16", "lowshelf:20:24", "highshelf:3600:-24", EIGHT,
             ";".join(["peak:20:24:16"] * 8)]
    ns = [1, 2, 640, 882, 1023, 1024, 1025, 1920, 2049, 3840, 4097, 5121, 6145, 7680, 8191, 8192]
    plans = []
    for spec in specs:
        for rate in (8000, 11025, 24000, 48000):
            for n in ns:
                try:
                    plans.append(tone.plan(rate, n, spec))
                except ValueError:
                    assert spec in ("warm", "bright", "deess") and rate < 16000
    assert {p.chunk for p in plans} == set(range(1, 9)) and any(p.K == 8 for p in plans)
    e64 = _sweep(tmp_path, plans)
    print(f"e64 over {len(plans)} plans: {e64:.3e}")
    assert 0.0 < e64 <= 2.0 ** -25


def test_e64_of_the_gpu_tests_shapes(tmp_path):
    """the figure tests/test_gpu_tone.py builds its bound from: the largest |chunked - serial| / running peak over the shapes
    it runs, measured here on the CPU.  That file holds it rounded up; it must neither fall below the measurement nor grow
    past four times it"""
    from pocket_tts_amd import tone

    e64 = _sweep(tmp_path, [tone.plan(rate, n, spec) for rate, n, spec in GPU_SHAPES])
    print(f"e64 of the GPU test's shapes: {e64:.3e}")
    src = (REPO / "tests" / "test_gpu_tone.py").read_text()
    held = float(re.search(r"^E64 = (\S+)", src, re.M).group(1))
    assert e64 <= held <= 4.0 * e64
