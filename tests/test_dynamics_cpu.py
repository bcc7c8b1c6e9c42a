"""Per-request dynamics without a GPU: the grammar and the presets of `pocket_tts_amd/dynamics.py`, the static curve, the
properties of the streaming definition on the tests' own restatement (`dynamics_ref.py`), E of the chunk / scan / re-run
scheme over the shapes of tests/test_gpu_dynamics.py; the plan; `route()` and `for_request` with the stages the compressor
combines with; the server's `dynamics` field against a stub batcher; the CLI flags; and the kernel's index functions and
chunked recurrences swept on the CPU under a host sanitizer (a stand-alone C++ program run as a child process)."""

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

import dynamics_ref

REPO = Path(__file__).resolve().parents[1]
K = math.log(10.0) / 20.0
SPEECH = "threshold=-20.0;ratio=3.0;knee=6.0;attack=5.0;release=100.0;makeup=4.0"
# T / R / W / attack / release / M of the issue's prototype run, next to the settings of the GPU test's rows
FIVE = ["threshold=-20;ratio=3;knee=6;attack=5;release=100;makeup=4", dynamics_ref.CORNER,
        "threshold=0;ratio=1;knee=24;attack=100;release=2000;makeup=0", "threshold=-18;ratio=6;knee=4;attack=2;release=60;makeup=6",
        "threshold=-30;ratio=20;knee=24;attack=0.1;release=2000;makeup=12"]


# ---- grammar, presets, canonical form ---------------------------------------------------------------------------------------
def test_canonical_form():
    from pocket_tts_amd import dynamics

    for off in (None, "", "  ", "off", " OFF "):
        assert dynamics.normalise(off) is None
    assert dynamics.normalise(" Speech ") == "speech"  # a preset stays a name
    assert dynamics.normalise("threshold=-24;ratio=4") == "threshold=-24.0;ratio=4.0;knee=6.0;attack=5.0;release=100.0;makeup=4.0"
    assert dynamics.normalise(" Makeup = 2e0 ; RATIO=4 ") == "threshold=-20.0;ratio=4.0;knee=6.0;attack=5.0;release=100.0;makeup=2.0"
    assert dynamics.normalise("knee=0") == "threshold=-20.0;ratio=3.0;knee=0.0;attack=5.0;release=100.0;makeup=4.0"
    for spec in ["speech", "threshold=-24;ratio=4", dynamics_ref.CORNER, "attack=0.1"]:
        assert dynamics.normalise(dynamics.normalise(spec)) == dynamics.normalise(spec)  # a fixed point
    # the pair list of a preset's values is not the preset's name: tables key on the string
    assert dynamics.normalise(dynamics.PRESETS["speech"]) == SPEECH != "speech"
    assert dynamics.normalise_dynamics(["speech", "off", "Speech", "ratio=4", "ratio=4.0", None]) == [
        "speech", "threshold=-20.0;ratio=4.0;knee=6.0;attack=5.0;release=100.0;makeup=4.0"]


def test_presets_expand_to_the_values_of_the_issue():
    from pocket_tts_amd import dynamics

    assert list(dynamics.PRESETS) == ["speech", "gentle", "broadcast", "telephone"]
    want = {"speech": (-20, 3, 6, 5, 100, 4), "gentle": (-16, 2, 10, 10, 200, 2), "broadcast": (-24, 4, 8, 3, 150, 8),
            "telephone": (-18, 6, 4, 2, 60, 6)}
    for name, vals in want.items():
        assert tuple(dynamics.values(name)[k] for k in dynamics.KEYS) == tuple(map(float, vals)), name
        assert dynamics_ref.parse(name) == tuple(map(float, vals))  # the restatement holds the same numbers
    assert dynamics.values("ratio=4") == dict(dynamics.values("speech"), ratio=4.0)  # what is left out is that of speech
    with pytest.raises(ValueError, match="bypass"):
        dynamics.values("off")


@pytest.mark.parametrize("key,lo,hi", [("threshold", -60.0, 0.0), ("ratio", 1.0, 20.0), ("knee", 0.0, 24.0),
                                       ("attack", 0.1, 100.0), ("release", 10.0, 2000.0), ("makeup", 0.0, 24.0)])
def test_every_range_edge_is_accepted_and_the_value_just_outside_refused(key, lo, hi):
    from pocket_tts_amd import dynamics

    assert dynamics.RANGES[key] == (lo, hi)
    for edge in (lo, hi):
        assert dynamics.values(f"{key}={edge!r}")[key] == edge
    for outside in (math.nextafter(lo, -math.inf), math.nextafter(hi, math.inf), float("nan"), float("inf")):
        with pytest.raises(ValueError) as e:
            dynamics.normalise(f"{key}={outside!r}")
        assert f"{key} must be in [{lo:g}, {hi:g}]" in str(e.value) and "dynamics" in str(e.value)
    with pytest.raises(ValueError, match=f"{key} must be a number"):
        dynamics.normalise(f"{key}=loud")


@pytest.mark.parametrize("spec,words", [
    ("loud", "neither a preset"), ("gain=3", "neither a preset"), ("ratio", "neither a preset"), ("speech;ratio=4", "neither a preset"),
    ("ratio=4;;knee=2", "neither a preset"), ("ratio=4;ratio=4", "the key ratio is given twice"),
    ("ratio=4;Ratio=5", "the key ratio is given twice"), ("ratio=", "ratio must be a number"),
])
def test_refusals_name_their_rule(spec, words):
    from pocket_tts_amd import dynamics

    with pytest.raises(ValueError) as e:
        dynamics.normalise(spec)
    assert words in str(e.value) and "dynamics" in str(e.value)


def test_non_strings_and_empty_lists_are_refused():
    from pocket_tts_amd import dynamics

    for bad in (3, 1.5, True, ["speech"]):
        with pytest.raises(ValueError, match="preset's name or a list of key=value pairs"):
            dynamics.normalise(bad)
    with pytest.raises(ValueError, match="list of settings"):
        dynamics.normalise_dynamics("speech")
    for empty in ([], ["off"], [None, ""]):
        with pytest.raises(ValueError, match="holds no setting"):
            dynamics.normalise_dynamics(empty)


# ---- the static curve -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,R,W", [(-20.0, 3.0, 6.0), (-60.0, 20.0, 24.0), (0.0, 1.5, 0.5), (-24.0, 4.0, 8.0)])
def test_the_static_curve(T, R, W):
    from pocket_tts_amd import dynamics

    k, h = 1.0 - 1.0 / R, 1e-6
    c = lambda L: dynamics.curve(L, T, k, W)  # noqa: E731
    lo, hi = T - W / 2.0, T + W / 2.0
    for L in (-120.0, lo - 10.0, lo - h, lo):
        assert c(L) == 0.0  # zero below T - W / 2
    for L in (hi, hi + h, hi + 1.0, 0.0 if hi < 0 else hi + 5.0, 120.0):
        assert c(L) == k * (L - T)  # slope k above T + W / 2
    assert abs((c(hi + 3.0) - c(hi + 1.0)) / 2.0 - k) < 1e-12
    # continuous, with a continuous first derivative, at both knee edges: finite differences at 1e-6 dB
    for edge, slope in ((lo, 0.0), (hi, k)):
        assert abs(c(edge + h) - c(edge - h)) <= 2.0 * h * k + 1e-12
        inner = (c(edge + h) - c(edge)) / h if edge == lo else (c(edge) - c(edge - h)) / h
        assert abs(inner - slope) <= k * h / W + 1e-9  # the parabola's slope moves by k / W per dB
    assert abs(c(T) - k * W / 8.0) < 1e-12 and c(T) == dynamics_ref.curve(T, T, k, W)
    xs = np.linspace(lo - 1.0, hi + 1.0, 2001)
    ys = np.array([c(float(v)) for v in xs])
    assert (ys >= 0.0).all() and (np.diff(ys) >= -1e-15).all()  # a reduction, growing with the level


def test_knee_zero_is_the_hard_knee():
    from pocket_tts_amd import dynamics

    T, k = -20.0, 0.75
    for L in (-120.0, -20.0 - 1e-9, -20.0):
        assert dynamics.curve(L, T, k, 0.0) == 0.0
    for L in (-20.0 + 1e-9, -10.0, 0.0, 120.0):
        assert dynamics.curve(L, T, k, 0.0) == k * (L - T)
    assert dynamics.curve(-10.0, T, 0.0, 6.0) == 0.0  # ratio 1: no reduction anywhere
    assert dynamics.level(0.0) == dynamics.level(float("nan")) == pytest.approx(-120.0, abs=1e-12)
    assert dynamics.level(float("inf")) == dynamics.level(-3e9) == pytest.approx(120.0, abs=1e-12)
    assert dynamics.level(-0.5) == pytest.approx(20.0 * math.log10(0.5), abs=1e-12)


# ---- the reference model on a constant-level input of alternating sign ---------------------------------------------------------
def _alternating(amp, count):
    return (amp * (1.0 - 2.0 * (np.arange(count) % 2))).astype(np.float32)


@pytest.mark.parametrize("setting,rate", [("speech", 24000), ("telephone", 8000), (dynamics_ref.CORNER, 24000),
                                          ("broadcast", 48000), ("attack=100;release=2000", 8000)])
def test_attack_reaches_the_curve(setting, rate):
    """after ceil(12 attack) samples s is within c e^-12 + 1e-9 dB of c, and 0 <= s <= c on the way"""
    T, R, W, attack, _, M = dynamics_ref.parse(setting)
    tau = attack * rate / 1000.0
    count = math.ceil(12.0 * tau)
    amp = float(np.float32(0.5))
    c = dynamics_ref.curve(math.log(amp) / K, T, 1.0 - 1.0 / R, W)
    assert c > 0.0
    y, s = dynamics_ref.Serial(setting, rate).frame(_alternating(amp, count + 5))
    assert (s >= 0.0).all() and (s <= c + 1e-12).all() and (np.diff(s) > 0.0).all()
    assert abs(s[count - 1] - c) <= c * math.exp(-12.0) + 1e-9
    assert (np.abs(y) <= math.exp(M * K) * amp * (1.0 + 1e-15)).all()  # the gain never exceeds the make-up


def test_ratio_one_is_the_makeup_gain_exactly():
    x = dynamics_ref.signal(640, 5)
    for M in (0.0, 3.5, 24.0):
        setting = f"ratio=1;makeup={M!r}"
        y, s = dynamics_ref.reference(setting, 8000, x, 640)
        assert not s.any()
        assert np.array_equal(y.astype(np.float32), (math.exp(M * K) * x.astype(np.float64)).astype(np.float32))


def test_an_inf_sample_leaves_s_finite_and_the_row_recovers():
    amp, n = float(np.float32(0.1)), 24000
    x = _alternating(amp, n)
    x[100] = np.inf
    ser = dynamics_ref.Serial("speech", 24000)
    y, s = ser.frame(x)
    T, R, W, *_ = dynamics_ref.parse("speech")
    c = dynamics_ref.curve(math.log(amp) / K, T, 1.0 - 1.0 / R, W)
    assert np.isfinite(s).all() and s.max() <= (1.0 - 1.0 / R) * (120.0 - T)  # the clamp at 1e6: 120 dBFS, no more
    assert np.isinf(y[100]) and np.isfinite(np.delete(y, 100)).all()
    assert s[101] > c + 1.0 and abs(s[-1] - c) < 1e-6  # it ducked, and a second later it is back on the curve
    assert math.isfinite(ser.p) and math.isfinite(ser.s)


def test_a_nan_sample_comes_out_as_nan_and_leaves_p_and_s_untouched():
    amp = float(np.float32(0.25))
    x = _alternating(amp, 4000)
    clean = dynamics_ref.Serial("telephone", 8000)
    y0, s0 = clean.frame(x)
    x[1000] = np.nan
    odd = dynamics_ref.Serial("telephone", 8000)
    y, s = odd.frame(x)
    assert np.isnan(y[1000]) and np.isfinite(np.delete(y, 1000)).all() and np.isfinite(s).all()
    # a NaN counts as the floor: p decays by one release step under it and is back at once, s dips by less than that
    assert 0.0 < s0[1000] - s[1000] < s0[1000] * (1.0 - odd.aR) + 1e-12
    assert np.array_equal(s[:1000], s0[:1000]) and abs(s[-1] - s0[-1]) < 1e-9 and (odd.p, odd.s) == pytest.approx((clean.p, clean.s), abs=1e-9)


def test_the_rule_module_runs_the_restatement():
    """`dynamics.run` (the stage's definition, carried state and all) against `dynamics_ref.Serial`: the same operations in
    the same order, so they agree exactly, NaN and Inf included"""
    from pocket_tts_amd import dynamics

    for b, r in enumerate(dynamics_ref.ROWS):
        if r is None or r[1] > 2000:
            continue
        rate, n, setting = r
        x = dynamics_ref.signal(n, 300 + b, odd=True)
        pl, st, ser = dynamics.plan(rate, n, setting), None, dynamics_ref.Serial(setting, rate)
        for f in range(dynamics_ref.F):
            got, st = dynamics.run(pl, x[f * n:(f + 1) * n], st)
            want, _ = ser.frame(x[f * n:(f + 1) * n])
            assert np.array_equal(got, want, equal_nan=True), (b, f)
        assert st == (ser.p, ser.s)


# ---- E ----------------------------------------------------------------------------------------------------------------------------
def _e_of(rate, n, setting, seed, odd=False):
    """(the largest |s_chunked - s_serial| in dB, differing fp32 output samples, samples) over the GPU test's signal"""
    x = dynamics_ref.signal(n, seed, odd)
    ser, ch = dynamics_ref.Serial(setting, rate), dynamics_ref.Chunked(setting, rate)
    worst = differ = 0
    for f in range(dynamics_ref.F):
        y1, s1 = ser.frame(x[f * n:(f + 1) * n])
        y2, s2 = ch.frame(x[f * n:(f + 1) * n])
        worst = max(worst, float(np.abs(s1 - s2).max()))
        with np.errstate(over="ignore", invalid="ignore"):
            differ += int((y1.astype(np.float32).view(np.uint32) != y2.astype(np.float32).view(np.uint32)).sum())
    assert abs(ser.s - ch.s) <= worst and ch.p == pytest.approx(ser.p, rel=1e-12, abs=1e-12)  # the carried state as well
    return worst, differ, x.shape[0]


def test_e_of_the_gpu_tests_shapes():
    """the figure tests/test_gpu_dynamics.py builds its bound from: the largest |s_chunked - s_serial| in dB over the rows it
    runs, on their own signals, measured here on the CPU.  That file holds it rounded up; it must neither fall below the
    measurement nor grow past four times it"""
    e = 0.0
    for b, r in enumerate(dynamics_ref.ROWS):
        if r is not None:
            worst, differ, count = _e_of(*r, 200 + b, b == dynamics_ref.ODD)
            print(f"dynamics row {b} {r}: E = {worst:.3e} dB, {differ} of {count} fp32 samples differ")
            e = max(e, worst)
    print(f"E of the GPU test's rows: {e:.3e} dB")
    src = (REPO / "tests" / "test_gpu_dynamics.py").read_text()
    held = float(re.search(r"^E_DB = (\S+)", src, re.M).group(1))
    assert 0.0 < e <= held <= 4.0 * e


def test_e_at_the_corners_of_the_grammar():
    """the five settings of the corners on a long, a short and a one-sample line: the scheme stays below 1e-10 dB, which is
    1.2e-11 of the gain, four orders below the rounding to fp32"""
    e = 0.0
    for j, setting in enumerate(FIVE):
        for rate, n in ((24000, 1025), (8000, 1), (48000, 3840)):
            e = max(e, _e_of(rate, n, setting, 400 + j)[0])
    print(f"E at the corners: {e:.3e} dB")
    assert e <= 1e-10


# ---- the plan ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,n,setting", [r for r in dynamics_ref.ROWS if r is not None] + [(44100, 1, "gentle"), (48000, 8192, "speech")])
def test_plan_values(rate, n, setting):
    from pocket_tts_amd import dynamics

    p = dynamics.plan(rate, n, setting)
    T, R, W, attack, release, M = dynamics_ref.parse(setting)
    assert (p.rate, p.n, p.chunk, p.setting) == (rate, n, -(-n // 1024), dynamics.normalise(setting)) and p.ints() == (rate, n)
    assert (p.T, p.k, p.W, p.M) == (T, 1.0 - 1.0 / R, W, M)
    assert p.aA == math.exp(-1.0 / (attack * rate / 1000.0)) and p.aR == math.exp(-1.0 / (release * rate / 1000.0))
    d = p.doubles()
    assert d.dtype == np.float64 and d.shape == (dynamics.DOUBLES_PER_PLAN,) == (26,) and np.isfinite(d).all()
    assert list(d[:6]) == [p.T, p.k, p.W, p.M, p.aA, p.aR]
    assert np.array_equal(d[6:16], p.pow_a) and np.array_equal(d[16:], p.pow_r)
    for a, pw in ((p.aA, p.pow_a), (p.aR, p.pow_r)):  # the powers, computed directly: a^(chunk 2^j) up to rounding
        assert ((pw >= 0.0) & (pw < 1.0)).all()
        for j in range(dynamics.SCAN_STEPS):
            assert pw[j] == pytest.approx(a ** (p.chunk << j), rel=1e-9, abs=1e-300)


def test_plan_refusals_and_the_table():
    from pocket_tts_amd import dynamics

    for rate, n, words in ((7999, 640, "rate must be in"), (48001, 1920, "rate must be in"), (24000, 0, "not in [1, 8192]"),
                           (24000, 8193, "not in [1, 8192]")):
        with pytest.raises(ValueError, match=re.escape(words)):
            dynamics.plan(rate, n, "speech")
    with pytest.raises(ValueError, match="bypass has no plan"):
        dynamics.plan(24000, 1920, "off")
    settings = dynamics.normalise_dynamics(["speech", "ratio=4"])
    plans, index = dynamics.table([(24000, 1920), (8000, 640), (24000, 1920)], settings)
    assert index == {(24000, 1920): [0, 1], (8000, 640): [2, 3]}
    assert [(p.rate, p.n, p.setting) for p in plans] == [(24000, 1920, "speech"), (24000, 1920, settings[1]), (8000, 640, "speech"),
                                                         (8000, 640, settings[1])]
    with pytest.raises(ValueError, match="rate must be in"):
        dynamics.table([(4000, 320)], settings)  # admissible on none of the lines


# ---- ChainTable / Route / for_request / ChainSpec --------------------------------------------------------------------------------
def test_route_a_setting_alone_brings_the_limiter():
    from pocket_tts_amd import level
    from pocket_tts_amd.output_chain import ChainTable

    t = ChainTable(24000, 1920, dynamics=["speech", "threshold=-24;ratio=4"])
    canon = "threshold=-24.0;ratio=4.0;knee=6.0;attack=5.0;release=100.0;makeup=4.0"
    assert t.dynamics == ["speech", canon] and not t.empty and t.level_plans is not None
    assert t.loud_plans is None and t.tone_plans is None and len(t.dyn_plans) == 2 and t.dyn_index == {(24000, 1920): [0, 1]}
    assert t.dynamics_of(24000, 1920) == ["speech", canon]
    LA = level.plan(24000, 1920).LA
    r = t.route(dynamics="speech")
    assert (r.dyn_plan, r.dynamic, r.level, r.preroll, r.drain_stage) == (0, True, (0, 0.0, -1.0), LA, "level")  # level = (plan, 0.0, peak)
    assert r.drain_frames == -(-LA // 1920) and r.n_out == 1920 and (r.tone_plan, r.toned) == (None, False)
    r = t.route(dynamics=" Ratio=4 ; threshold=-24", peak_dbfs=-3)  # peak_dbfs is allowed behind a setting
    assert (r.dyn_plan, r.level) == (1, (0, 0.0, -3.0))
    r = t.route(dynamics="speech", gain_db=6)  # the request's own gain
    assert (r.dyn_plan, r.level, r.preroll, r.drain_stage) == (0, (0, 6.0, -1.0), LA, "level")
    for off in (None, "", "off"):
        r = t.route(dynamics=off)
        assert (r.dyn_plan, r.dynamic, r.level, r.preroll, r.drain_stage) == (None, False, None, 0, None)
    with pytest.raises(ValueError, match="only meaningful together"):
        t.route(peak_dbfs=-3)


def test_route_dynamics_combines_with_tone_gain_and_loudness():
    from pocket_tts_amd import level, loudness
    from pocket_tts_amd.output_chain import ChainTable

    t = ChainTable(24000, 1920, sample_rates=[8000], loudness=True, tones=["warm", "telephone"], dynamics=["speech", "telephone"])
    D, LA = loudness.plan(24000, 1920).D, level.plan(24000, 1920).LA
    r = t.route(tone="warm", dynamics="telephone", loudness_lufs=-16)
    assert (r.tone_plan, r.dyn_plan, r.loud, r.level, r.preroll, r.drain_stage) == (0, 1, (0, -16.0), (0, 0.0, -1.0), D + LA, "loud")
    r = t.route(tone="warm", dynamics="speech", gain_db=-3.0, peak_dbfs=-2.0)
    assert (r.tone_plan, r.dyn_plan, r.loud, r.level, r.preroll) == (0, 0, None, (0, -3.0, -2.0), LA)
    r = t.route(sample_rate=8000, tone="telephone", dynamics="speech")  # the plans of the request's own line
    assert t.dyn_plans[r.dyn_plan].rate == 8000 and t.dyn_plans[r.dyn_plan].n == 640 and r.tone_plan is not None
    assert r.level == (t.level_index[(8000, 640)], 0.0, -1.0)
    with pytest.raises(ValueError, match="exclude each other"):
        t.route(dynamics="speech", loudness_lufs=-16, gain_db=3)


def test_route_a_request_without_a_setting_is_routed_as_on_a_levelled_table():
    from pocket_tts_amd.output_chain import ChainSpec, ChainTable, Route

    kw = dict(sample_rates=[8000, 16000], speeds=[1.25], pitches=["5/4"])
    dyn = ChainTable(24000, 1920, dynamics=["speech"], **kw)
    plain = ChainTable(24000, 1920, level=True, **kw)
    for req in [{}, {"sample_rate": 8000}, {"speed": 1.25, "gain_db": 3.0}, {"sample_rate": 16000, "pitch": "5/4", "gain_db": -2.0,
                                                                            "peak_dbfs": -6.0}]:
        assert dyn.route(**req) == plain.route(**req)
    # Route's new fields sit at the end with defaults: positional construction as before
    r = Route(0, 24000, None, False, None, 1920, 0, 0, None)
    assert r.dyn_plan is None and r.dynamic is False
    # over the lines the pitcher leaves: the stretched lines as well
    assert set(dyn.dyn_index) == {(24000, 1920), (8000, 640), (16000, 1280), (24000, 1536), (8000, 512), (16000, 1024)}
    # the spec: the new option is the last field, its tag sits before the packer's
    assert list(ChainSpec.TAGS)[-1] == "compressions" and list(ChainSpec.TAGS)[-2] == "dynamics"
    assert ChainSpec(None, None, False, None, False, None, None, None, ["speech"]).dynamics == ("speech",)
    assert ChainSpec().tags() == () and ChainSpec(dynamics=["speech", "gentle"]).tags() == ("dyn", "speech", "gentle")
    assert ChainSpec(tones=["warm"], dynamics=["speech"], compressions=["flac"]).tags() == ("tone", "warm", "dyn", "speech", "comp")
    assert ChainSpec(dynamics=["speech"]).table(24000, 1920).dynamics == ["speech"]


def test_route_refusals():
    from pocket_tts_amd.output_chain import ChainTable

    t = ChainTable(24000, 1920, dynamics=["speech", "gentle"])
    with pytest.raises(ValueError) as e:
        t.route(dynamics="broadcast")
    assert "'broadcast' is not configured" in str(e.value) and "['speech', 'gentle']" in str(e.value)
    with pytest.raises(ValueError, match="ratio must be in"):
        t.route(dynamics="ratio=21")
    with pytest.raises(ValueError, match="no dynamics stage"):
        ChainTable(24000, 1920, level=True).route(dynamics="speech")
    assert ChainTable(24000, 1920).route(dynamics="off").dynamic is False  # the bypass is no setting
    with pytest.raises(ValueError, match="holds no setting"):
        ChainTable(24000, 1920, dynamics=["off"])
    with pytest.raises(ValueError, match="holds no setting"):
        ChainTable(24000, 1920, dynamics=[])
    with pytest.raises(ValueError, match="list of settings"):
        ChainTable(24000, 1920, dynamics="speech")


def test_for_request():
    from pocket_tts_amd.output_chain import ChainSpec, ChainTable, RequestError

    base = dict(sample_rate=None, speed=None, gain_db=None, peak_dbfs=None, pitch=None, loudness_lufs=None, encoding=None, tone=None)
    for off in (None, "", "off"):  # a request without the field yields the request dict it always did
        spec, req = ChainTable.for_request(24000, 1920, dynamics=off)
        assert req == base and spec == ChainSpec() and "dynamics" not in req
    spec, req = ChainTable.for_request(24000, 1920, dynamics=" Speech ")
    assert req == dict(base, gain_db=0.0, peak_dbfs=-1.0, dynamics="speech")
    assert spec == ChainSpec(level=True, dynamics=("speech",)) and spec.tags() == ("level", "dyn", "speech")
    assert spec.table(24000, 1920).route(**req).level == (0, 0.0, -1.0)
    spec, req = ChainTable.for_request(24000, 1920, 8000, None, 3.0, -2.0, None, None, "mulaw", "telephone", None, "ratio=4")
    canon = "threshold=-20.0;ratio=4.0;knee=6.0;attack=5.0;release=100.0;makeup=4.0"
    assert (req["dynamics"], req["tone"], req["gain_db"], req["peak_dbfs"]) == (canon, "telephone", 3.0, -2.0)
    assert spec.dynamics == (canon,) and spec.tones == ("telephone",) and spec.level
    r = spec.table(24000, 1920).route(**req)
    assert (r.rate, r.n_out, r.dynamic, r.toned, r.level[1:]) == (8000, 640, True, True, (3.0, -2.0))
    spec, req = ChainTable.for_request(24000, 1920, dynamics="gentle", loudness_lufs=-23)
    assert (req["gain_db"], req["loudness_lufs"], req["peak_dbfs"]) == (None, -23.0, -1.0) and spec.loudness and not spec.level
    assert spec.table(24000, 1920).route(**req).level == (0, 0.0, -1.0)
    for bad in ("loud", "ratio=0.5", "ratio=2;ratio=3"):
        with pytest.raises(RequestError) as e:
            ChainTable.for_request(24000, 1920, dynamics=bad)
        assert e.value.field == "dynamics"
    with pytest.raises(RequestError) as e:  # the walk is in chain order: the tone is refused first
        ChainTable.for_request(24000, 1920, tone="nope", dynamics="loud")
    assert e.value.field == "tone"


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


def test_server_dynamics_field(tmp_path):
    forms = [{"text": "hi", "dynamics": "speech"}, {"text": "hi", "dynamics": " Speech ", "sample_rate": "8000", "peak_dbfs": "-3"},
             {"text": "hi"}, {"text": "hi", "dynamics": ""}, {"text": "hi", "dynamics": "off"},
             {"text": "hi", "dynamics": "Ratio=4;threshold=-24", "gain_db": "3"},
             {"text": "hi", "dynamics": "speech", "loudness_lufs": "-16"}, {"text": "hi", "dynamics": "speech", "tone": "warm"}]
    res, index, stub = _run_app(tmp_path, forms, sample_rates=[8000], level=True, loudness=True, tones=["warm"],
                                dynamics=["speech", "threshold=-24;ratio=4"])
    assert [r.status_code for r in res] == [200] * 8, [r.text for r in res]
    canon = "threshold=-24.0;ratio=4.0;knee=6.0;attack=5.0;release=100.0;makeup=4.0"
    got = [(s.get("dynamics"), s.get("gain_db"), s.get("peak_dbfs"), s.get("loudness_lufs"), s.get("sample_rate"), s.get("tone"))
           for s in stub.submitted]
    assert got == [("speech", None, None, None, None, None), ("speech", None, -3.0, None, 8000, None), (None,) * 6, (None,) * 6,
                   (None,) * 6, (canon, 3.0, -1.0, None, None, None), ("speech", None, -1.0, -16.0, None, None),
                   ("speech", None, None, None, None, "warm")]
    assert all("dynamics" not in s for s in stub.submitted[2:5])
    assert 'name="dynamics"' in index.text


def test_server_dynamics_400(tmp_path):
    bad = [{"text": "hi", "dynamics": "broadcast"}, {"text": "hi", "dynamics": "ratio=21"}, {"text": "hi", "dynamics": "loud"},
           {"text": "hi", "dynamics": "speech", "peak_dbfs": "3"}, {"text": "hi", "dynamics": "speech", "peak_dbfs": "low"}]
    res, _, stub = _run_app(tmp_path, bad, sample_rates=[8000], dynamics=["speech", "gentle"])
    assert [r.status_code for r in res] == [400] * 5 and not stub.submitted
    d = [r.json()["detail"] for r in res]
    assert "'broadcast' is not configured" in d[0] and "['speech', 'gentle']" in d[0]  # the admissible list
    assert "ratio must be in [1, 20]" in d[1] and "neither a preset" in d[2] and "[-20, 0]" in d[3] and "must be a number" in d[4]
    # a server without the option refuses the field, and takes the bypass
    res, _, stub = _run_app(tmp_path, [{"text": "hi", "dynamics": "speech"}, {"text": "hi", "dynamics": "off"}, {"text": "hi"}])
    assert [r.status_code for r in res] == [400, 200, 200] and "without dynamics" in res[0].json()["detail"]
    assert all("dynamics" not in s for s in stub.submitted)
    # what the grammar refuses in the list is refused when the server starts
    from pocket_tts_amd.server import create_app

    with pytest.raises(ValueError, match="knee must be in"):
        create_app(_StubModel(), slots=1, capacity=64, batcher_factory=lambda m, s, c: None, dynamics=["speech", "knee=25"])


# ---- the command line ---------------------------------------------------------------------------------------------------------
def test_cli_dynamics_flags(tmp_path, monkeypatch):
    from pocket_tts_amd import main, tts_model

    a = main.build_parser().parse_args(["serve", "--dynamics", "speech,threshold=-24;ratio=4"])
    assert a.dynamics == ["speech", "threshold=-24;ratio=4"]
    assert main.build_parser().parse_args(["serve"]).dynamics is None
    for bad in ("speech,nope", "off", "ratio=4;ratio=5"):
        with pytest.raises(SystemExit):
            main.build_parser().parse_args(["serve", "--dynamics", bad])
    assert main.FLAGS["dynamics"] == "--dynamics"
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
    assert main.cli_app(["generate", "--text", "hi", "--dynamics", "Speech", "--peak-dbfs", "-2", "--output-path", str(out), "-q"]) == 0
    assert (seen["dynamics"], seen["peak_dbfs"], seen["gain_db"]) == ("speech", -2.0, None) and out.exists()
    seen.clear()
    assert main.cli_app(["generate", "--text", "hi", "--output-path", str(out), "-q"]) == 0
    assert "dynamics" not in seen  # a request without the flag is the request it always was
    out2 = tmp_path / "out2.wav"  # refused before the output is opened
    assert main.cli_app(["generate", "--text", "hi", "--dynamics", "ratio=0", "--output-path", str(out2), "-q"]) == 1
    assert main.cli_app(["generate", "--text", "hi", "--dynamics", "loud", "--output-path", str(out2), "-q"]) == 1
    assert not out2.exists()


# ---- the header and the chunked recurrences under a host sanitizer ------------------------------------------------------------
def test_the_header_holds_the_rule_modules_constants():
    from pocket_tts_amd import dynamics

    text = (REPO / "pocket_tts_amd" / "csrc" / "ptts_dyn.h").read_text()
    val = lambda name: int(re.search(rf"#define {name} (\d+)", text).group(1))  # noqa: E731
    assert (val("PTTS_DY_MIN_RATE"), val("PTTS_DY_MAX_RATE"), val("PTTS_DY_MAX_N")) == (dynamics.RATE_MIN, dynamics.RATE_MAX, dynamics.MAX_N)
    assert (val("PTTS_DY_THREADS"), val("PTTS_DY_SCAN"), val("PTTS_DY_PLAN_INTS")) == (dynamics.THREADS, dynamics.SCAN_STEPS, 2)
    assert 1 << dynamics.SCAN_STEPS == dynamics.THREADS and dynamics.MAX_N == 8 * dynamics.THREADS
    assert float(re.search(r"#define PTTS_DY_K (\S+)", text).group(1)) == dynamics.K == dynamics_ref.K
    assert (float(re.search(r"#define PTTS_DY_A_MIN (\S+)", text).group(1)),
            float(re.search(r"#define PTTS_DY_A_MAX (\S+)", text).group(1))) == (dynamics.A_MIN, dynamics.A_MAX)
    # the C ABI's names in the three places that must agree
    from pocket_tts_amd import _lib

    names = ["ptts_dynamics_create", "ptts_dynamics_destroy", "ptts_dynamics_set_row", "ptts_dynamics_frame", "ptts_mimi_set_dynamics"]
    public = (REPO / "include" / "ptts.h").read_text()
    unit = (REPO / "pocket_tts_amd" / "csrc" / "ptts_dyn.hip").read_text() + (REPO / "pocket_tts_amd" / "csrc" / "ptts_codec.hip").read_text()
    for name in names:
        assert name in _lib.PROTOTYPES and f"{name}(" in public and f'extern "C" ' in unit and f" {name}(" in unit, name


def _sweep(tmp_path, plans):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path / "dyn_sweep"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-I", str(REPO / "pocket_tts_amd" / "csrc"), "-o", str(exe),
                        str(REPO / "tests" / "cpp" / "dyn_sweep.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    blob = struct.pack("<i", len(plans))
    for p in plans:
        blob += struct.pack("<ii", *p.ints()) + p.doubles().tobytes()
    (tmp_path / "plans.bin").write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # the leak checker needs ptrace, which build sandboxes often deny
    r = subprocess.run([str(exe), str(tmp_path / "plans.bin")], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    m = re.fullmatch(rf"ok {len(plans)} plans {12 * len(plans)} frames e_db (\S+)", r.stdout.strip())
    assert m, r.stdout
    return float(m.group(1))


def test_chunked_recurrences_under_host_sanitizer(tmp_path):
    """every index the shared header forms, on exact-size heap buffers under AddressSanitizer + UBSan, and the two chunked
    recurrences against the header's serial sample step: every preset and the corners of the grammar, at n = 1, less than a
    wave, one sample per thread, a partial last chunk, every chunk size and n = 8192.  The program itself fails above 1e-9 dB"""
    from pocket_tts_amd import dynamics

    ns = [1, 2, 63, 640, 1023, 1024, 1025, 1920, 2049, 3840, 4097, 5121, 6145, 7680, 8191, 8192]
    plans = [dynamics.plan(rate, n, s) for s in [*dynamics.PRESETS, *FIVE] for rate in (8000, 24000, 48000) for n in ns]
    assert {p.chunk for p in plans} == set(range(1, 9))
    e = _sweep(tmp_path, plans)
    print(f"e_db over {len(plans)} plans: {e:.3e}")
    assert 0.0 < e <= 1e-9
