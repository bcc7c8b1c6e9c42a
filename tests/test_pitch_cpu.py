"""Per-request pitch without a GPU: the plan rule (pocket_tts_amd/pitch.py), the composed fp64 reference on its own
(tests/pitch_ref.py), the routes through the output chain, the index functions of csrc/ptts_pitch.h under a host sanitizer,
the library's admission check compiled on the host, and the server's and the CLI's pitch settings against stubs."""

import asyncio
import math
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

import pitch_ref
import stretch_ref
from resample_ref import NATIVE, RATES

REPO = Path(__file__).resolve().parents[1]
OUT_N = {8000: 640, 11025: 882, 12000: 960, 16000: 1280, 22050: 1764, 24000: 1920, 32000: 2560, 44100: 3528, 48000: 3840}


# ---- the plan rule -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,rate,n,Ha,Hs,D,L,n_mid,T", [("2/1", 24000, 1920, 240, 480, 144, 1680, 3840, 41),
                                                        ("1/2", 24000, 1920, 960, 480, 144, 1920, 960, 21),
                                                        ("17/16", 24000, 1920, 480, 510, 144, 1920, 2040, 22),
                                                        ("4/5", 8000, 640, 160, 128, 48, 480, 512, 21)])
def test_plan_check_values(r, rate, n, Ha, Hs, D, L, n_mid, T):
    from pocket_tts_amd import resample, stretch
    from pocket_tts_amd.pitch import HIST, plan

    p = plan(r, rate, n)
    f = Fraction(r)
    assert (p.P, p.Q, p.frac, p.pitch) == (f.numerator, f.denominator, f, float(f)) and not p.identity
    assert (p.sp.Ha, p.sp.Hs, p.sp.D, p.sp.L, p.n_mid, p.T) == (Ha, Hs, D, L, n_mid, T)
    assert p.sp.ints() == stretch.plan(float(1 / f), rate, n).ints()  # the WSOLA part is the stretch rule's plan, unchanged
    assert p.preroll == L and p.drain_frames == 1 and p.n_out == n and p.ints() == (n, Ha, Hs, D, L, p.P, p.Q, T)
    assert p.sp.Ha * p.P == p.sp.Hs * p.Q and p.n_mid * p.Q == n * p.P and p.n_mid * p.Q % p.P == 0 and T - 1 <= HIST
    assert p.sp.L // p.sp.Ha * p.sp.Hs * p.Q == L * p.P  # the WSOLA pre-roll, resampled, is L exactly
    h = resample.prototype(p.Q, p.P)
    assert np.array_equal(p.h, h) and p.table.dtype == np.float32 and p.table.shape == (p.Q, T)
    for ph in range(p.Q):
        taps = h[ph::p.Q]
        assert np.array_equal(p.table[ph, :len(taps)], taps.astype(np.float32)) and not p.table[ph, len(taps):].any()


def test_identity_and_lists():
    from pocket_tts_amd.pitch import fraction, identity, normalise_pitches, plan, table

    for one in (1, 1.0, "1/1", Fraction(3, 3)):
        p = plan(one, 24000, 1920)
        assert p.identity and p.preroll == 0 and p.drain_frames == 0 and p.n_out == p.n_mid == 1920 and p.T == 1
    assert identity(8000, 640).ints() == (640, 640, 640, 0, 0, 1, 1, 1)
    assert fraction("17/16") == fraction(1.0625) == fraction(" 17/16 ") == Fraction(17, 16)
    assert normalise_pitches(["5/4", 0.8, 1.25, 1]) == [1.0, 1.25, 0.8]
    plans, index = table([(24000, 1920), (8000, 640), (24000, 1920)], normalise_pitches(["2/3", "4/5"]))
    assert index == {(24000, 1920): [0, 1, 2], (8000, 640): [3, None, 4]}  # 2/3 has no whole hops at 8 kHz
    assert plans[0].identity and plans[3].identity and plans[3].n == 640 and plans[4].sp.Hs == 128
    with pytest.raises(ValueError, match="no multiple of 9"):
        table([(24000, 1920), (8000, 640)], normalise_pitches(["8/9"]))


def test_refusals_name_the_rule():
    from pocket_tts_amd.pitch import fraction, normalise_pitches, plan

    for bad, msg in [("8/9", "pitch 8/9: .*no multiple of 9 divides 1920"), (0.77, "fraction P / Q"), ("0.77", "fraction P / Q"),
                     (2.5, r"must be in \[0.5, 2.0\]"), ("2/5", r"must be in \[0.5, 2.0\]"), ("high", "number or a fraction"),
                     ("1/0", "number or a fraction"), (True, "finite number"), (float("nan"), "finite number"),
                     (1.95, "fraction P / Q"), ("39/20", "fraction P / Q")]:  # 39 / 20: Q <= 20 but P is not
        with pytest.raises(ValueError, match=msg):
            plan(bad, 24000, 1920)
    with pytest.raises(ValueError, match="fraction P / Q"):
        fraction(1 / 21 + 1)
    with pytest.raises(ValueError, match="must be in"):
        normalise_pitches([3])


def test_nearest_and_the_admitted_ratios():
    from pocket_tts_amd.pitch import admissible, nearest, plan

    f, c = nearest(1, 24000, 1920)
    assert f == Fraction(17, 16) and 0 < c <= 6
    for st, want in ((12, 2), (-12, Fraction(1, 2)), (0, 1), (7, Fraction(3, 2)), (-5, Fraction(3, 4)), (2, Fraction(9, 8)),
                     (-1, Fraction(19, 20))):
        f, c = nearest(st, 24000, 1920)
        assert f == want and abs(c - (1200 * math.log2(want) - 100 * st)) < 1e-9
    assert nearest(12)[1] == nearest(-12)[1] == 0.0
    assert all(abs(nearest(st, 24000, 1920)[1]) <= 18 for st in range(-12, 13))
    counts = {rate: len(admissible(rate, OUT_N[rate])) for rate in OUT_N}  # 1 / 1 included
    assert counts == {24000: 53, 12000: 53, 48000: 53, 8000: 35, 16000: 35, 32000: 35, 11025: 37, 22050: 46, 44100: 52}
    window = mid = 0
    for rate, n in OUT_N.items():
        for f in admissible(rate, n):
            p = plan(f, rate, n)
            if not p.identity:
                window, mid = max(window, p.sp.L + p.sp.D + p.sp.Ha + n), max(mid, p.n_mid)
    assert (window, mid) == (9888, 7680)  # what the kernel stages in LDS at most, and its longest mid line
    with pytest.raises(ValueError, match="must be in"):
        nearest(13)


# ---- the fp64 reference on its own -------------------------------------------------------------------------------------
def _noise(n, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n + 64)
    return np.convolve(x, np.hanning(33) / np.hanning(33).sum(), mode="valid")[:n] * 0.5


@pytest.mark.parametrize("r,rate", [("1/2", 24000), ("4/5", 24000), ("17/16", 24000), ("3/2", 24000), ("2/1", 24000), ("4/5", 8000)])
def test_streaming_reference_equals_the_whole_signal(r, rate):
    """frame by frame (`pitch_ref.Stream`) == WSOLA of the whole signal, zero-stuffed by Q, convolved with the prototype and
    decimated by P, with the fp64 table on both sides"""
    from pocket_tts_amd.pitch import plan

    p = plan(r, rate, OUT_N[rate])
    frames = 4 + p.drain_frames
    x = _noise(4 * p.n, seed=p.P * 100 + p.Q)
    st = pitch_ref.Stream(p)
    ys = np.concatenate([st.feed(x[f * p.n:(f + 1) * p.n] if f < 4 else np.zeros(p.n)) for f in range(frames)])
    mid, deltas = stretch_ref.wsola(x, p.sp, frames)
    assert st.deltas == deltas and ys.shape == (frames * p.n,)
    up = np.zeros(len(mid) * p.Q)
    up[::p.Q] = mid
    whole = np.convolve(up, p.h)[::p.P][:frames * p.n]
    assert np.max(np.abs(ys - whole)) <= 1e-12
    y2 = pitch_ref.pitch(x, p, frames)[0]
    assert np.max(np.abs(ys - y2)) <= 1e-12
    silent = ((p.sp.L - p.sp.D - p.sp.W) // p.sp.Ha + 1) * p.sp.Hs  # mid samples before the first hop that reads the stream
    assert ys[p.preroll:p.preroll + 4 * p.n].any() and not ys[:silent * p.Q // p.P].any()


@pytest.mark.parametrize("r", ["1/2", "4/5", "17/16", "3/2", "2/1"])
def test_a_tone_moves_by_r_and_keeps_its_level(r):
    from pocket_tts_amd.pitch import plan

    p = plan(r, 24000, 1920)
    frames = 50  # 4 s
    t = np.arange(frames * p.n)
    x = 0.5 * np.sin(2 * np.pi * 210.0 * t / 24000)
    y = pitch_ref.pitch(x, p, frames)[0]
    y = y[p.preroll + 2 * p.sp.W:]
    assert len(y) >= 24000  # a second at least
    nfft = 1 << 20
    spec = np.abs(np.fft.rfft(y * np.hanning(len(y)), nfft))
    k = int(np.argmax(spec))
    a, b, c = np.log(spec[k - 1:k + 2])
    peak = (k + 0.5 * (a - c) / (a - 2 * b + c)) * 24000 / nfft
    assert abs(peak - 210.0 * float(p.frac)) <= 0.5, peak
    rms = float(np.sqrt(np.mean(y ** 2)))
    assert abs(rms - 0.5 / np.sqrt(2)) <= 1e-3, rms


# ---- the routes through the output chain ----------------------------------------------------------------------------------
def test_chain_table_and_routes():
    from pocket_tts_amd import level, pitch, stretch
    from pocket_tts_amd.output_chain import ChainTable, Route

    FS = 1920
    bare = ChainTable(NATIVE, FS)
    assert bare.empty and bare.pitches is None and bare.pitch_plans is None and bare.pitch_index is None
    assert bare.route() == Route(0, NATIVE, None, False, None, FS, 0, 0, None)
    assert bare.route(pitch=1.0) == bare.route() and bare.route().pitch_plan is None and not bare.route().pitched
    with pytest.raises(ValueError, match="pitch 1.0 only.*pitches"):
        bare.route(pitch="5/4")
    with pytest.raises(ValueError, match="pitch 1.0 only.*pitches"):
        ChainTable(NATIVE, FS, speeds=[1.25], level=True).route(pitch=1.25)

    t = ChainTable(NATIVE, FS, [16000], [1.25], level=True, pitches=["5/4"])
    assert not t.empty and t.pitches == [1.0, 1.25]
    sp = stretch.plan(1.25, 16000, 1280)
    assert sp.n_out == 1024
    assert set(t.pitch_index) == {(24000, 1920), (24000, 1536), (16000, 1280), (16000, 1024)}
    assert set(t.level_index) == set(t.pitch_index)  # the pitcher keeps n: the leveler's lines are those of before
    r = t.route(16000, 1.25, 6, None, "5/4")
    pp = t.pitch_plans[r.pitch_plan]
    assert (pp.rate, pp.n, pp.pitch) == (16000, 1024, 1.25) and r.pitched and r.stretched
    assert r.n_out == 1024 and r.level[0] == t.level_index[(16000, 1024)]
    assert r.preroll == sp.preroll + pp.L + level.plan(16000, 1024).LA and pp.L == pitch.plan("5/4", 16000, 1024).sp.L
    assert r.drain_frames == -(-r.preroll // 1024) and r.drain_stage == "stretch"
    r2 = t.route(16000, None, 6, None, 1.25)
    pp2 = t.pitch_plans[r2.pitch_plan]
    assert (pp2.rate, pp2.n) == (16000, 1280) and r2.pitched and not r2.stretched and r2.drain_stage == "pitch"
    assert r2.preroll == pp2.L + level.plan(16000, 1280).LA and r2.n_out == 1280
    r3 = t.route(16000, None, 6)
    assert not r3.pitched and t.pitch_plans[r3.pitch_plan].identity and r3.drain_stage == "level"
    r4 = t.route()
    assert r4.preroll == 0 and r4.drain_stage is None and not r4.pitched and t.pitch_plans[r4.pitch_plan].n == FS
    with pytest.raises(ValueError, match="not configured"):
        t.route(pitch="3/2")
    with pytest.raises(ValueError, match=r"not admissible on frames of 1280 samples at 16000 Hz \(admissible there: \[1.0, 1.25\]\)"):
        ChainTable(NATIVE, FS, [16000], pitches=["5/4", "4/3"]).route(16000, pitch="4/3")
    with pytest.raises(ValueError, match="no multiple of 9"):
        ChainTable(NATIVE, FS, pitches=["8/9"])
    # take() over a simulated run: exactly [preroll, preroll + F n)
    for route in (r, r2):
        F, pos, got = 7, 0, []
        for f in range(F + route.drain_frames):
            lo, hi = route.take(pos, None if f < F - 1 else F)
            got += list(range(pos + lo, pos + hi))
            pos += route.n_out
        assert got == list(range(route.preroll, route.preroll + F * route.n_out))

    one = lambda *a, **kw: ChainTable.for_request(NATIVE, FS, *a, **kw)[1]  # noqa: E731
    got = one(16000, 1.25, 6, None)
    assert (got["sample_rate"], got["speed"], got["gain_db"], got["peak_dbfs"]) == (16000, 1.25, 6.0, -1.0)  # as before
    assert one(16000, 1.25, pitch="5/4")["pitch"] == 1.25
    assert one(pitch=1.0)["pitch"] is None and one(pitch=None)["pitch"] is None
    with pytest.raises(ValueError, match="no multiple of 9"):
        one(pitch="8/9")
    with pytest.raises(ValueError, match="no multiple of 3"):  # 2/3 behind 8 kHz: frames of 640 samples
        one(8000, pitch="2/3")


# ---- the index functions under a host sanitizer --------------------------------------------------------------------------
def _admitted():
    from pocket_tts_amd.pitch import admissible, identity, plan

    ps = []
    for rate in sorted({NATIVE, *RATES}):
        ps.append(identity(rate, OUT_N[rate]))
        ps += [plan(f, rate, OUT_N[rate]) for f in admissible(rate, OUT_N[rate]) if f != 1]
    return ps


def test_index_sweep_under_host_sanitizer(tmp_path):
    """every index the shared headers form, for every plan the rule admits at every documented rate (every reduced P / Q with
    P, Q <= 20 in [0.5, 2], and the rates' identity plans), on exact-size heap buffers under AddressSanitizer + UBSan"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path / "pitch_sweep"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-I", str(REPO / "pocket_tts_amd" / "csrc"), "-o", str(exe),
                        str(REPO / "tests" / "cpp" / "pitch_sweep.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    ps = _admitted()
    shifted = [p for p in ps if not p.identity]
    assert len(shifted) == 3 * 52 + 3 * 34 + 36 + 45 + 51 and {p.rate for p in shifted} == {NATIVE, *RATES}
    blob = struct.pack("<i", len(ps))
    for p in ps:
        blob += struct.pack("<8i", *p.ints()) + p.sp.window.astype("<f4").tobytes() + p.table.astype("<f4").tobytes()
    (tmp_path / "plans.bin").write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # the leak checker needs ptrace, which build sandboxes often deny
    r = subprocess.run([str(exe), str(tmp_path / "plans.bin")], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.strip() == (f"ok {len(ps)} plans {len(ps) - len(shifted)} identities {2 * sum(p.K for p in shifted)} hops "
                                f"{2 * sum(p.n for p in shifted)} outputs")


def test_the_library_refuses_what_the_header_refuses(tmp_path):
    """pt_plan_ok, compiled on the host: the plans of the rule pass, and each broken rule fails"""
    cxx = shutil.which("g++") or shutil.which("c++")
    src = tmp_path / "ok.cpp"
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "ptts_pitch.h"\nint main(int c, char **v) {\n'
                   '  int a[10];\n  for (int i = 0; i < 10; ++i) a[i] = atoi(v[i + 1]);\n'
                   '  printf("%d\\n", (int)pt_plan_ok(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9]));\n  return 0;\n}\n')
    exe = tmp_path / "ok"
    r = subprocess.run([cxx, "-std=c++17", "-I", str(REPO / "pocket_tts_amd" / "csrc"), "-o", str(exe), str(src)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]

    def ok(*v, max_in=8192, max_mid=16384):
        return subprocess.run([str(exe), *map(str, (*v, max_in, max_mid))], capture_output=True, text=True,
                              timeout=60).stdout.strip() == "1"

    from pocket_tts_amd.pitch import identity, plan

    for p in (plan("2/1"), plan("1/2"), plan("17/16"), plan("4/5", 8000, 640), plan("19/20"), identity(24000, 1920),
              plan("3/2", 48000, 3840)):
        assert ok(*p.ints()), p.ints()
    assert ok(1920, 480, 510, 144, 1920, 17, 16, 22)
    assert not ok(1920, 480, 510, 144, 1440, 17, 16, 22)     # ts_plan_ok: L < D + W + Hs, a read past the frame's end
    assert not ok(1920, 500, 510, 144, 2000, 17, 16, 22)     # ts_plan_ok: no whole hops per frame
    assert not ok(1920, 480, 510, 144, 1920, 17, 15, 22)     # Ha / Q != Hs / P
    assert not ok(1920, 480, 512, 144, 1920, 16, 15, 23)     # Ha / Q == Hs / P == 32, but 512 / 480 is 16 / 15 ... and
    assert ok(1920, 480, 512, 144, 1920, 16, 15, 22)         # ... its tap count is 22, not 23
    assert not ok(1920, 480, 510, 144, 1920, 34, 32, 22)     # not reduced, and P, Q above 20
    assert not ok(1920, 960, 480, 144, 1920, 2, 4, 21)       # not reduced
    assert not ok(1920, 480, 510, 144, 1920, 17, 16, 21) and not ok(1920, 480, 510, 144, 1920, 17, 16, 23)  # the tap count
    assert not ok(1920, 480, 510, 144, 1920, 17, 16, 22, max_mid=2039) and ok(1920, 480, 510, 144, 1920, 17, 16, 22, max_mid=2040)
    assert not ok(1920, 1920, 1920, 0, 0, 1, 1, 2) and not ok(1920, 1920, 1920, 0, 0, 2, 1, 1)  # an identity is P = Q = T = 1
    assert not ok(1920, 480, 510, 144, 1920, 1, 1, 1)        # P == Q on a plan that stretches
    assert not ok(1920, 480, 510, 144, 1920, 0, 16, 22) and not ok(1920, 480, 510, 144, 1920, 17, 21, 22)
    assert not ok(9000, 9000, 9000, 0, 0, 1, 1, 1)


# ---- the server's pitch field and the CLI's flags against stubs ---------------------------------------------------------------
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
        if settings.get("pitch") is not None and fae is not None and fae < 1:  # the batcher's own refusal
            raise ValueError("a request with a pitch needs frames_after_eos >= 1")
        self.submitted.append(settings)
        rate = settings.get("sample_rate") or 24000
        return _StubRequest(3, 1920 * rate // 24000)


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


def test_server_pitch_field(tmp_path):
    forms = [{"text": "hi", "pitch": "17/16"}, {"text": "hi", "pitch": " 0.8 ", "sample_rate": "8000"}, {"text": "hi"},
             {"text": "hi", "pitch": ""}, {"text": "hi", "pitch": "1.0"}, {"text": "hi", "pitch": "1.25"}]
    res, index, stub = _run_app(tmp_path, forms, sample_rates=[8000], pitches=["17/16", "5/4", "4/5"])
    assert [r.status_code for r in res] == [200] * 6, [r.text[:200] for r in res]
    assert [s.get("pitch") for s in stub.submitted] == [1.0625, 0.8, None, None, None, 1.25]
    assert all("pitch" not in s for s in stub.submitted[2:5])  # pitch 1.0 is a request like before
    for r, rate in zip(res, (24000, 8000, 24000, 24000, 24000, 24000)):
        n = 1920 * rate // 24000
        assert struct.unpack("<L", r.content[24:28])[0] == rate
        assert len(r.content) == 44 + 3 * n * 2 + 2 * int(rate * 0.2)  # the pitch keeps a request's length
    assert 'name="pitch"' in index.text


def test_server_pitch_400(tmp_path):
    bad = [{"text": "hi", "pitch": "high"}, {"text": "hi", "pitch": "nan"}, {"text": "hi", "pitch": "3/2"},
           {"text": "hi", "pitch": "4/3", "sample_rate": "8000"}, {"text": "hi", "pitch": "4/3", "frames_after_eos": "0"},
           {"text": "hi", "pitch": "3"}]
    res, _, stub = _run_app(tmp_path, bad, sample_rates=[8000], pitches=["17/16", "4/3", "4/5"])
    assert [r.status_code for r in res] == [400] * 6 and not stub.submitted
    d = [r.json()["detail"] for r in res]
    assert "number or a fraction" in d[0] and "finite" in d[1]
    assert "not configured" in d[2] and f"[1.0, 1.0625, {4 / 3}, 0.8]" in d[2]          # the admissible list
    assert "not admissible on frames of 640 samples at 8000 Hz" in d[3] and "[1.0, 1.0625, 0.8]" in d[3]
    assert "frames_after_eos >= 1" in d[4] and "not configured" in d[5]
    # a server started without pitches speaks at pitch 1.0 only
    res, _, stub = _run_app(tmp_path, [{"text": "hi", "pitch": "5/4"}, {"text": "hi", "pitch": "1"}])
    assert [r.status_code for r in res] == [400, 200] and "pitch 1.0 only" in res[0].json()["detail"]
    assert stub.submitted == [{"temperature": None, "noise_clamp": None, "eos_threshold": None}]
    from pocket_tts_amd.server import create_app

    for pitches, msg in [(["8/9"], "no multiple of 9"), ([3.0], "must be in"), ([0.77], "fraction")]:
        with pytest.raises(ValueError, match=msg):
            create_app(_StubModel(), slots=1, capacity=8, batcher_factory=lambda m, s, c: _StubBatcher(), pitches=pitches)


def test_cli_flags():
    from pocket_tts_amd.main import build_parser

    ap = build_parser()
    assert ap.parse_args(["generate", "--pitch", "17/16"]).pitch == "17/16"
    assert ap.parse_args(["generate", "--pitch-semitones", "-2"]).pitch_semitones == -2.0
    g = ap.parse_args(["generate"])
    assert g.pitch is None and g.pitch_semitones is None
    assert ap.parse_args(["serve", "--pitches", "17/16,5/4,0.8"]).pitches == [1.0625, 1.25, 0.8]
    assert ap.parse_args(["serve"]).pitches is None
    with pytest.raises(SystemExit):
        ap.parse_args(["serve", "--pitches", "high"])


@pytest.mark.parametrize("extra", [["--pitch", "8/9"], ["--pitch", "2/3", "--sample-rate", "8000"], ["--pitch", "3"],
                                   ["--pitch-semitones", "13"], ["--pitch", "5/4", "--pitch-semitones", "2"]])
def test_cli_refuses_an_inadmissible_pitch_before_it_opens_the_output(tmp_path, monkeypatch, extra):
    """`generate_audio_stream` is a generator: it would raise only once the WAV file exists"""
    from pocket_tts_amd import main, tts_model

    class _Model(SimpleNamespace):
        def get_state_for_audio_prompt(self, voice):
            raise AssertionError("the pitch is checked before any work for the request")

    monkeypatch.setattr(tts_model.TTSModel, "load_model",
                        staticmethod(lambda **kw: _Model(sample_rate=24000, engine=SimpleNamespace(frame_samples=1920))))
    out = tmp_path / "out.wav"
    assert main.cli_app(["generate", "--text", "hi", *extra, "--output-path", str(out), "-q"]) == 1
    assert not out.exists()


def test_cli_resolves_semitones_to_the_nearest_ratio(tmp_path, monkeypatch, caplog):
    from pocket_tts_amd import main, tts_model

    seen = {}

    class _Model(SimpleNamespace):
        def get_state_for_audio_prompt(self, voice):
            return {}

        def generate_audio_stream(self, state, text, **kw):
            seen.update(kw)
            yield torch.zeros(1920)

    monkeypatch.setattr(tts_model.TTSModel, "load_model",
                        staticmethod(lambda **kw: _Model(sample_rate=24000, engine=SimpleNamespace(frame_samples=1920))))
    out = tmp_path / "out.wav"
    with caplog.at_level("INFO"):
        assert main.cli_app(["generate", "--text", "hi", "--pitch-semitones", "1", "--output-path", str(out)]) == 0
    assert seen.get("pitch") == 1.0625 and out.exists()
    assert "17/16" in caplog.text and "cents" in caplog.text
