"""Per-request output level on the GPU: the leveler kernel against the fp64 reference (tests/level_ref.py) - error bound,
ceiling, exactness and isolation, streaming state, captured graphs, the whole output chain - and the path through the
continuous batcher, `TTSModel.generate_audio_stream` and the HTTP server (tiny model).

Largest |y - y64| observed on an MI355X, against the bound (LA + 64) 2^-24 max|u|: see the "output level" section of
DESIGN.md."""

import asyncio
import io
import json
import re
import shutil
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

import level_ref
from level_ref import GPU_FRAMES as F

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"
SENTINEL_F, SENTINEL_I = -77.0, -12345
GUARD = 4096
TEXT = "Hello world. This is a test."


def _plans(case):
    from pocket_tts_amd.level import plan

    return [plan(24000, 1920), plan(8000, 640), plan(24000, 960)] if case == "four" else [plan(48000, 3840)]


def _rows(case):
    """(plan index or None for bypass, gain_db) of each row"""
    return [(None, None), (0, 12.0), (1, 12.0), (2, -6.0)] if case == "four" else [(0, 12.0)]


@pytest.fixture(scope="module")
def model():
    from pocket_tts_amd import TTSModel

    m = TTSModel.load_model(config=G / "e2e_tiny.yaml", temp=0.0)
    yield m
    m.engine.close()


@pytest.fixture(scope="module")
def eng(model):
    return model.engine


@pytest.fixture(scope="module")
def ref():
    """per case: the rows' input streams and, for each limiting row, the whole-signal float64 reference fed the fp32 G, C, a, k.
    The conditions on the reference alone are asserted here, before anything runs on the GPU."""
    from pocket_tts_amd.level import params

    out = {}
    for case in ("four", "two_tiles"):
        plans, rows = _plans(case), _rows(case)
        streams, refs = [], []
        for idx, gain in rows:
            if idx is None:
                streams.append(level_ref.signal(F * 1920, seed=99))
                refs.append(None)
                continue
            p = plans[idx]
            x = level_ref.gpu_signal(p.rate, p.n)
            Gf, Cf = params(gain)
            y, u, r, g = level_ref.level(x, Gf, Cf, p.LA, p.a, p.k, full=True)
            if gain > 0:
                assert 0.05 <= np.mean(r < 1) <= 0.5, (case, idx, np.mean(r < 1))
                assert any(g[f * p.n - 1] < 1 and g[f * p.n] < 1 for f in range(1, F)), (case, idx)
            else:
                assert not (r < 1).any()  # this row never limits
            streams.append(x)
            refs.append(dict(y=y, u=u, C=float(Cf), p=p))
        out[case] = (streams, refs)
    return out


def _lines(case, streams, order=None):
    """[frames, B, width] input lines: row b's frame at the front of its line, NaN behind it (nothing may read it)"""
    plans, rows = _plans(case), _rows(case)
    width = max(p.n for p in plans)
    order = list(range(len(rows))) if order is None else order
    x = np.full((F, len(order), width), np.nan, np.float32)
    for j, b in enumerate(order):
        n = width if rows[b][0] is None else plans[rows[b][0]].n
        x[:, j, :n] = streams[b].reshape(F, -1)[:, :n]
    return x


def _guarded(eng, shape, fill, dtype):
    """a contiguous device tensor of `shape` in the middle of a larger buffer filled with `fill`: (view, whole buffer)"""
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=eng.device)
    return big[GUARD:GUARD + n].view(*shape), big


def _run(eng, case, x, order=None, i16=False, extra=0, events=None):
    """x [frames, B, width] through a fresh Leveler whose row j runs row `order[j]` of the case, then `extra` frames of NaN
    lines; `events` = {frame: [("set_row", j) | ("drain", j)]} applied before that frame.  The output and the guard bands
    around it are pre-filled with sentinels before every frame.  Returns outs [frames][B, width]."""
    plans, rows = _plans(case), _rows(case)
    order = list(range(len(rows))) if order is None else order
    B = len(order)
    lv = eng.new_leveler(B, plans)
    fill = SENTINEL_I if i16 else SENTINEL_F
    try:
        for j, b in enumerate(order):
            lv.set_row(j, rows[b][0], rows[b][1])
        outs = []
        for f in range(x.shape[0] + extra):
            for kind, j in (events or {}).get(f, ()):
                if kind == "set_row":
                    lv.set_row(j, *lv.rows[j])
                else:
                    lv.set_row_drain(j, True)
            out, out_big = _guarded(eng, (B, lv.width), fill, torch.int16 if i16 else torch.float32)
            line = x[f] if f < x.shape[0] else np.full_like(x[0], np.nan)
            xin, _ = _guarded(eng, (B, lv.width), float("nan"), torch.float32)
            xin.copy_(torch.from_numpy(line))
            lv.frame(xin, out)
            torch.cuda.synchronize()
            g = out_big.cpu().numpy()
            assert (g[:GUARD] == fill).all() and (g[-GUARD:] == fill).all(), "a write outside the buffer"
            assert np.array_equal(xin.cpu().numpy().view(np.uint32), line.view(np.uint32)), "the input was written"
            outs.append(out.cpu().numpy())
        return outs
    finally:
        lv.close()


def _stream_of(outs, j, n):
    return np.concatenate([o[j, :n] for o in outs])


@pytest.fixture(scope="module")
def base(eng, ref):
    """the f32 outputs of both cases, computed once"""
    return {case: _run(eng, case, _lines(case, ref[case][0])) for case in ("four", "two_tiles")}


@pytest.mark.parametrize("case", ["four", "two_tiles"])
def test_against_the_reference(eng, ref, base, case):
    streams, refs = ref[case]
    outs = base[case]
    rows, plans = _rows(case), _plans(case)
    width = outs[0].shape[1]
    for j, (idx, gain) in enumerate(rows):
        if idx is None:  # the bypass row is bitwise its input (its whole line: a row without a plan has no n)
            got = _stream_of(outs, j, width)
            assert np.array_equal(got.view(np.uint32), streams[j].view(np.uint32))
            continue
        R = refs[j]
        p = R["p"]
        y = _stream_of(outs, j, p.n)
        assert np.isfinite(y).all()
        err = float(np.max(np.abs(y.astype(np.float64) - R["y"])))
        bound = (p.LA + 64) * 2.0 ** -24 * float(np.max(np.abs(R["u"])))
        peak = float(np.max(np.abs(y)))
        print(f"level {case} row {j} ({p.rate} Hz, n {p.n}, {gain:+g} dB): max|y - y64| = {err:.3e} (bound {bound:.3e}), "
              f"max|y| / C = {peak / R['C']:.8f}")
        assert err <= bound, (case, j, err, bound)
        assert peak <= R["C"] * (1 + (p.LA + 8) * 2.0 ** -24), (case, j, peak)
        for o in outs:  # nothing beyond n of the row's output line is written
            assert (o[j, p.n:] == SENTINEL_F).all()


@pytest.mark.parametrize("case", ["four", "two_tiles"])
def test_int16_is_the_conversion_of_the_f32_output(eng, ref, base, case):
    outs16 = _run(eng, case, _lines(case, ref[case][0]), i16=True)
    rows, plans = _rows(case), _plans(case)
    for j, (idx, _) in enumerate(rows):
        n = outs16[0].shape[1] if idx is None else plans[idx].n
        for o16, o in zip(outs16, base[case]):
            assert np.array_equal(o16[j, :n], level_ref.pcm16(o[j, :n]))
            assert (o16[j, n:] == SENTINEL_I).all()


def test_a_nan_inside_a_frame_makes_one_output_sample_nan(eng, ref, base):
    streams, _ = ref["four"]
    plans = _plans("four")
    x = _lines("four", streams)
    x0 = x.copy()
    x[1, 1, 100] = np.nan     # row 1 (24 kHz): frame 1, sample 100
    x0[1, 1, 100] = 0.0       # r = 1 either way: every other sample must not notice
    x[2, 2, 639] = np.nan     # row 2 (8 kHz): the last sample of frame 2, its output falls into frame 3
    x0[2, 2, 639] = 0.0
    a, b = _run(eng, "four", x), _run(eng, "four", x0)
    for j, at in ((1, 1920 + 100 + plans[0].LA), (2, 2 * 640 + 639 + plans[1].LA)):
        n = plans[j - 1].n
        ya, yb = _stream_of(a, j, n), _stream_of(b, j, n)
        assert np.flatnonzero(np.isnan(ya)).tolist() == [at] and np.isfinite(yb).all()
        keep = np.arange(len(ya)) != at
        assert np.array_equal(ya[keep].view(np.uint32), yb[keep].view(np.uint32))
    for j in (0, 3):  # the other rows do not notice at all
        assert np.array_equal(_stream_of(a, j, 960).view(np.uint32), _stream_of(base["four"], j, 960).view(np.uint32))


def test_a_row_is_bitwise_the_same_in_any_slot_and_any_batch(eng, ref, base):
    streams, _ = ref["four"]
    plans, rows = _plans("four"), _rows("four")
    order = [3, 2, 1, 0]
    perm = _run(eng, "four", _lines("four", streams, order), order=order)
    for j, b in enumerate(order):
        n = 1920 if rows[b][0] is None else plans[rows[b][0]].n
        assert np.array_equal(_stream_of(perm, j, n).view(np.uint32), _stream_of(base["four"], b, n).view(np.uint32)), b
    for b in (1, 2, 3):
        n = plans[rows[b][0]].n
        one = _run(eng, "four", _lines("four", streams, [b]), order=[b])
        assert np.array_equal(_stream_of(one, 0, n).view(np.uint32), _stream_of(base["four"], b, n).view(np.uint32)), b


def test_set_row_restarts_a_row_from_zero_state(eng, ref, base):
    streams, _ = ref["four"]
    x = _lines("four", streams)
    a = _run(eng, "four", x, events={2: [("set_row", 1)]})
    fresh = _run(eng, "four", x[2:])
    assert np.array_equal(_stream_of(a[2:], 1, 1920).view(np.uint32), _stream_of(fresh, 1, 1920).view(np.uint32))
    assert not np.array_equal(_stream_of(a[2:], 1, 1920), _stream_of(base["four"][2:], 1, 1920))  # the state mattered
    for j in (0, 2, 3):  # the other rows carry on
        assert np.array_equal(_stream_of(a, j, 640).view(np.uint32), _stream_of(base["four"], j, 640).view(np.uint32))


@pytest.mark.parametrize("case,j", [("four", 1), ("four", 2), ("two_tiles", 0)])
def test_drain_emits_the_tail_then_exact_zeros(eng, ref, base, case, j):
    """after the flag the input line holds NaN: it is not read"""
    streams, refs = ref[case]
    p = refs[j]["p"]
    x = _lines(case, streams)
    x[3, j, :] = np.nan
    outs = _run(eng, case, x, extra=1, events={3: [("drain", j)]})
    for f in range(3):
        assert np.array_equal(outs[f][j, :p.n].view(np.uint32), base[case][f][j, :p.n].view(np.uint32))
    tail, after = outs[3][j, :p.n], outs[4][j, :p.n]
    assert tail[:p.LA].any() and not tail[p.LA:].any() and not after.any()
    from pocket_tts_amd.level import params

    Gf, Cf = params(_rows(case)[j][1])
    y = level_ref.level(np.concatenate([streams[j][:3 * p.n], np.zeros(p.n, np.float32)]), Gf, Cf, p.LA, p.a, p.k)
    assert np.max(np.abs(tail - y[3 * p.n:])) <= (p.LA + 64) * 2.0 ** -24 * float(np.max(np.abs(refs[j]["u"])))


def test_captured_graph_follows_set_row_and_drain(eng):
    """a codec graph captured with a leveler: a later set_row (a new gain) and set_row_drain change what its replays compute,
    exactly as they change a leveler of its own fed the same PCM frame by frame"""
    B = 4
    plans = _plans("four")
    ms = eng.new_mimi_state(B)
    lv, twin = eng.new_leveler(B, plans), eng.new_leveler(B, plans)
    g = None
    try:
        lat = torch.randn(B, eng.ldim, device=eng.device, generator=torch.Generator(eng.device).manual_seed(3))
        pcm = torch.zeros(B, eng.frame_samples, device=eng.device)
        out = torch.full((B, lv.width), SENTINEL_F, device=eng.device)
        want = torch.full((B, lv.width), SENTINEL_F, device=eng.device)
        for s in (lv, twin):
            s.set_row(1, 0, 24.0, -20.0)
            s.set_row(2, 1, 12.0)
            s.set_row(3, 2, -6.0)
        ms.set_leveler(lv, out)
        g = eng.capture_mimi(ms, lat, pcm)
        ms.set_leveler(None)

        def step(tag):
            eng.graph_launch(g)
            eng.sync()
            twin.frame(pcm, want)
            torch.cuda.synchronize()
            assert pcm.abs().max().item() > 0
            assert np.array_equal(out.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32)), tag
            return out.cpu().numpy().copy(), pcm.cpu().numpy().copy()

        for f in range(3):
            a, x = step(("plain", f))
        assert np.array_equal(a[0], x[0]) and np.abs(a[1]).max() <= 0.1 * (1 + 128 * 2.0 ** -24)  # bypass; the -20 dBFS ceiling
        assert (a[2][640:] == SENTINEL_F).all() and (a[3][960:] == SENTINEL_F).all()
        for s in (lv, twin):
            s.set_row(1, 0, -6.0)   # a new gain
            s.set_row(0, 0, 6.0)    # the bypass row starts limiting
        b_, _ = step("set_row")
        assert not np.array_equal(b_[1], a[1]) and not b_[0][:plans[0].LA].any()
        for s in (lv, twin):
            s.set_row_drain(0, True)
            s.set_row_drain(2, True)
        c, _ = step("drain")
        assert not c[0][plans[0].LA:].any() and not c[2][plans[1].LA:640].any()
        # eager decodes on a state with a leveler append the same launch
        ms.set_leveler(lv, out)
        eng.mimi_decode(ms, lat, pcm)
        eng.sync()
        twin.frame(pcm, want)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
        ms.set_leveler(None)
    finally:
        if g is not None:
            eng.graph_destroy(g)
        lv.close()
        twin.close()
        ms.close()


def test_the_chain_in_one_graph_equals_its_stages_one_by_one(eng):
    """codec -> resampler (8 kHz) -> stretcher (1.25) -> leveler in one captured graph, against a resampler, a stretcher and
    a leveler of their own run one by one on the recorded intermediate buffers: bitwise"""
    from pocket_tts_amd import level, stretch

    B = 2
    ms = eng.new_mimi_state(B)
    rates = [(24000, 1920), (8000, 640)]
    ts_plans, index = stretch.table(rates, [1.0, 1.25])
    lv_plans, lv_index = level.table([(rates[r][0], ts_plans[i].n_out) for r, row in enumerate(index) for i in row if i is not None])
    made = [(eng.new_resampler(B, [8000]), eng.new_stretcher(B, ts_plans), eng.new_leveler(B, lv_plans)) for _ in range(2)]
    (rs, ts, lv), (rs2, ts2, lv2) = made
    g = None
    try:
        r8 = rs.index_of(8000)
        p8 = index[1][1]
        n8 = ts_plans[p8].n_out
        assert ts_plans[p8].n_in == 640 and n8 == 512
        for a, b, c in made:
            a.set_row(0, r8)
            b.set_row(0, p8)
            c.set_row(0, lv_index[(8000, n8)], 18.0, -6.0)
            c.set_row(1, lv_index[(24000, 1920)], 18.0)  # row 1: native rate, speed 1.0, levelled
        lat = torch.randn(B, eng.ldim, device=eng.device, generator=torch.Generator(eng.device).manual_seed(4))
        pcm = torch.zeros(B, eng.frame_samples, device=eng.device)
        mid1 = torch.zeros(B, rs.out_max, device=eng.device)
        mid2 = torch.zeros(B, ts.out_max, device=eng.device)
        out = torch.full((B, lv.width), SENTINEL_F, device=eng.device)
        w1, w2, w3 = torch.zeros_like(mid1), torch.zeros_like(mid2), torch.full_like(out, SENTINEL_F)
        ms.set_resampler(rs, mid1)
        ms.set_stretcher(ts, mid2, mid1)
        ms.set_leveler(lv, out, mid2)
        g = eng.capture_mimi(ms, lat, pcm)
        ms.set_leveler(None)
        ms.set_stretcher(None)
        ms.set_resampler(None)
        for f in range(4):
            eng.graph_launch(g)
            eng.sync()
            rs2.frame(pcm, w1)
            torch.cuda.synchronize()
            assert np.array_equal(w1.cpu().numpy()[0, :640].view(np.uint32), mid1.cpu().numpy()[0, :640].view(np.uint32)), f
            ts2.frame(mid1, w2)
            torch.cuda.synchronize()
            assert np.array_equal(w2.cpu().numpy()[0, :n8].view(np.uint32), mid2.cpu().numpy()[0, :n8].view(np.uint32)), f
            lv2.frame(mid2, w3)
            torch.cuda.synchronize()
            assert np.array_equal(w3.cpu().numpy().view(np.uint32), out.cpu().numpy().view(np.uint32)), f
            o = out.cpu().numpy()
            assert (o[0, n8:] == SENTINEL_F).all() and np.isfinite(o[0, :n8]).all() and np.isfinite(o[1]).all()
        assert o[0, :n8].any() and o[1].any()
    finally:
        if g is not None:
            eng.graph_destroy(g)
        for a, b, c in made:
            c.close()
            b.close()
            a.close()
        ms.close()


def test_cabi_error_codes(eng):
    import ctypes as C

    lv = eng.new_leveler(2, _plans("four"))
    try:
        lib, sp = eng.lib, eng._sp
        for row, idx in ((-1, 0), (2, 0), (0, -2), (0, 3), (0, 1 << 20)):
            assert lib.ptts_leveler_set_row(lv.handle, row, idx, 1.0, 0.5, sp) == -1, (row, idx)
            assert b"out of range" in lib.ptts_last_error()
        for gain, ceil in ((0.0, 0.5), (17.0, 0.5), (float("nan"), 0.5), (1.0, 0.0), (1.0, 1.5), (1.0, float("nan"))):
            assert lib.ptts_leveler_set_row(lv.handle, 0, 0, gain, ceil, sp) == -1, (gain, ceil)
        assert lib.ptts_leveler_set_row_drain(lv.handle, 2, 1, sp) == -1 and lib.ptts_leveler_set_row_drain(None, 0, 1, sp) == -1
        with pytest.raises(ValueError, match="gain_db"):
            lv.set_row(0, 0, 30.0)
        assert lv.rows == [(-1, None, None)] * 2
        x = torch.zeros(2, lv.width, device=eng.device)
        out = torch.zeros(2, lv.width, device=eng.device)
        assert lib.ptts_level_frame(lv.handle, None, C.c_void_p(out.data_ptr()), 0, sp) == -1
        assert lib.ptts_level_frame(lv.handle, C.c_void_p(x.data_ptr()), None, 0, sp) == -1
        assert lib.ptts_level_frame(None, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), 0, sp) == -1
        h = C.c_void_p()
        from pocket_tts_amd.level import LevelPlan

        for n, LA in ((119, 120), (8193, 120), (1920, 0), (1920, 513)):  # a plan that breaks a rule never reaches the device
            arr = (C.c_int32 * 4)(*LevelPlan(24000, n, LA, np.float32(0.999), np.float32(1.0 / max(LA, 1))).ints())
            assert lib.ptts_leveler_create(eng.handle, 2, arr, 1, C.byref(h)) == -1 and b"not admissible" in lib.ptts_last_error()
        ms = eng.new_mimi_state(3)
        assert lib.ptts_mimi_set_leveler(ms.handle, lv.handle, None, C.c_void_p(out.data_ptr()), 0) == -1  # batch 3 vs 2
        ms.close()
        ms = eng.new_mimi_state(2)
        # an input buffer means "behind the resampler or the stretcher": refused on a state that has neither
        assert lib.ptts_mimi_set_leveler(ms.handle, lv.handle, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), 0) == -1
        ms.close()
    finally:
        lv.close()


# ---- through the batcher, the model and the server -------------------------------------------------------------------------
def _twin(eng, wav, gain_db, peak_dbfs=None, rate=24000, n=1920, i16=False):
    """what a leveler of its own makes of `wav` (whole frames of n samples) fed frame by frame plus one zero frame: the
    pre-roll dropped, frames * n samples"""
    from pocket_tts_amd.level import plan

    frames = wav.shape[0] // n
    assert frames * n == wav.shape[0]
    p = plan(rate, n)
    lv = eng.new_leveler(1, [p])
    try:
        lv.set_row(0, 0, gain_db, peak_dbfs)
        parts = []
        for f in range(frames + 1):
            x = torch.zeros(1, n, device=eng.device)
            if f < frames:
                x[0] = torch.from_numpy(wav[f * n:(f + 1) * n])
            out = torch.zeros(1, n, dtype=torch.int16 if i16 else torch.float32, device=eng.device)
            lv.frame(x, out)
            torch.cuda.synchronize()
            parts.append(out.cpu().numpy()[0])
        return np.concatenate(parts)[p.LA:p.LA + frames * n]
    finally:
        lv.close()


@pytest.fixture(scope="module")
def alone(model):
    """(frames, waveform) of TEXT as the only request of a fresh batcher without a level stage (2 slots).  The bitwise
    comparisons below are between requests that ran this way - alone, in slot 0, prefilled on their own: the codec's samples
    are reproducible bit for bit under the same placement and traffic only, which a check of the leveler must not depend on."""
    from pocket_tts_amd.batching import ContinuousBatcher

    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    cb = ContinuousBatcher(model, slots=2, capacity=512)
    try:
        r = cb.submit(state, TEXT)
        cb.run_until_idle()
        return r.frames, r.result().numpy()
    finally:
        cb.close()


def test_batcher_end_to_end(model, eng, alone):
    from pocket_tts_amd.batching import ContinuousBatcher

    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    frames, wav_p = alone
    assert wav_p.shape[0] == frames * 1920
    cb = ContinuousBatcher(model, slots=2, capacity=512, level=True)
    try:
        with pytest.raises(ValueError, match=r"\[-40, 24\]"):
            cb.submit(state, TEXT, gain_db=30)
        with pytest.raises(ValueError, match="together with gain_db"):
            cb.submit(state, TEXT, peak_dbfs=-3)
        with pytest.raises(ValueError, match="frames_after_eos >= 1"):
            cb.submit(state, TEXT, frames_after_eos=0, gain_db=12)
        r = cb.submit(state, TEXT, gain_db=12)
        cb.run_until_idle()
        wav = r.result().numpy()
        assert r.frames == frames and wav.shape[0] == frames * 1920
        assert np.array_equal(wav.view(np.uint32), _twin(eng, wav_p, 12).view(np.uint32))
        assert np.abs(wav).max() <= 10 ** -0.05 * (1 + 128 * 2.0 ** -24)
        # then, in the slot the levelled request has drained and left: a request without a gain is bit-identical
        r = cb.submit(state, TEXT)
        cb.run_until_idle()
        assert np.array_equal(r.result().numpy().view(np.uint32), wav_p.view(np.uint32))
        # two at once, one levelled: frame counts and sample counts are those of before
        reqs = [cb.submit(state, TEXT, gain_db=-6, peak_dbfs=-3), cb.submit(state, "ok")]
        cb.run_until_idle()
        for q in reqs:
            w = q.result().numpy()
            assert w.shape[0] == q.frames * 1920 and np.isfinite(w).all() and w.any()
    finally:
        cb.close()
    cb = ContinuousBatcher(model, slots=2, capacity=512)
    try:
        with pytest.raises(ValueError, match="no level stage"):
            cb.submit(state, TEXT, gain_db=12)
    finally:
        cb.close()


def test_batcher_with_rate_speed_and_gain(model, eng):
    """behind the resampler and the stretcher: a request at 8 kHz, 1.25 and +12 dB delivers the sample count of the same
    request without a gain, stays under the ceiling, and every sample is its gain-less sample times G times a g in [0, 1]
    (the limiter's state at the row's start and end sees the stretcher's own pre-roll and tail, so the twin of the other
    tests does not apply bit for bit)"""
    from pocket_tts_amd.batching import ContinuousBatcher
    from pocket_tts_amd.level import plan

    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    got = []
    for kw in ({"sample_rate": 8000, "speed": 1.25}, {"sample_rate": 8000, "speed": 1.25, "gain_db": 12}):
        cb = ContinuousBatcher(model, slots=2, capacity=512, sample_rates=[8000], speeds=[1.25], level=True)
        try:
            r = cb.submit(state, TEXT, **kw)
            cb.run_until_idle()
            got.append((r.frames, r.result().numpy()))
        finally:
            cb.close()
    (f0, w0), (f1, w1) = got
    LA = plan(8000, 512).LA
    assert f0 == f1 and w0.shape[0] == w1.shape[0] == f0 * 512
    assert np.isfinite(w1).all() and np.abs(w1).max() <= 10 ** -0.05 * (1 + (LA + 8) * 2.0 ** -24)
    from pocket_tts_amd.level import linear

    u = np.float32(linear(12)) * w0
    assert np.all(np.abs(w1) <= np.abs(u) * (1 + (LA + 8) * 2.0 ** -24)) and np.all(w1 * u >= 0)
    assert w1.any()


def test_generate_audio_stream_gain(model, eng):
    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    ref_chunks = [c.numpy() for c in model.generate_audio_stream(state, TEXT)]
    wav_p = np.concatenate(ref_chunks)
    chunks = [c.numpy() for c in model.generate_audio_stream(state, TEXT, gain_db=12)]
    wav = np.concatenate(chunks)
    assert wav.shape[0] == wav_p.shape[0] and all(0 < c.shape[0] <= 1920 for c in chunks)
    assert np.array_equal(wav.view(np.uint32), _twin(eng, wav_p, 12).view(np.uint32))
    # the cached context, restarted, with another gain and ceiling
    wav2 = model.generate_audio(state, TEXT, gain_db=0, peak_dbfs=-20).numpy()
    assert np.array_equal(wav2.view(np.uint32), _twin(eng, wav_p, 0, -20).view(np.uint32))
    assert np.abs(wav2).max() <= 0.1 * (1 + 128 * 2.0 ** -24)
    with pytest.raises(ValueError, match=r"\[-40, 24\]"):
        model.generate_audio(state, TEXT, gain_db=-50)
    assert sum(1 for k in model._ctx_cache if "speed" in k or "rate" in k or "level" in k) <= model.RATE_CONTEXTS


def test_server_gain(model, eng, alone, tmp_path):
    import httpx

    from pocket_tts_amd.server import create_app

    shutil.copy(G / "e2e_voice.safetensors", tmp_path / "e2e_voice.safetensors")
    frames, wav_p = alone
    app = create_app(model, slots=2, capacity=512, voices_dir=tmp_path, default_voice="e2e_voice", level=True)

    async def go():
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t", timeout=600) as cl:
                # one after the other: each request has the batcher to itself, like the one it is compared with
                return [await cl.post("/tts", data=d) for d in ({"text": TEXT, "gain_db": "12"}, {"text": TEXT},
                                                                 {"text": TEXT, "gain_db": "40"},
                                                                 {"text": TEXT, "gain_db": "12", "frames_after_eos": "0"})]

    loud, normal, bad, bad_fae = asyncio.run(go())
    assert bad.status_code == 400 and "[-40, 24]" in bad.json()["detail"]
    assert bad_fae.status_code == 400 and "frames_after_eos >= 1" in bad_fae.json()["detail"]
    for r in (loud, normal):
        assert r.status_code == 200, r.text[:200]
        with wave.open(io.BytesIO(r.content), "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 24000)
        assert len(r.content) - 44 == frames * 1920 * 2 + 2 * 4800
        assert not np.frombuffer(r.content[-2 * 4800:], np.int16).any()
    assert np.array_equal(np.frombuffer(normal.content[44:], np.int16)[:frames * 1920], level_ref.pcm16(wav_p))
    assert np.array_equal(np.frombuffer(loud.content[44:], np.int16)[:frames * 1920], _twin(eng, wav_p, 12, i16=True))


# ---- feature off ------------------------------------------------------------------------------------------------------------
def _step_launches(eng, st, ms):
    """(site, kernel) of every launch of one eager FlowLM step followed by one eager codec frame, in launch order"""
    lat = torch.zeros(ms.batch, eng.ldim, device=eng.device)
    pcm = torch.zeros(ms.batch, eng.frame_samples, device=eng.device)
    eng.sync()
    eng.profile_start()
    if st is not None:
        eng.lm_decode_step(st, None, None, 1, float("inf"))
    eng.mimi_decode(ms, lat, pcm)
    return [(r["site"], r["kernel"]) for r in eng.profile_stop()]


def _untuned(rows):
    """the launch list with what the tuner chooses per process taken out of the names: the template arguments and the
    '@threads' of the GEMM and attention kernels (their family and prologue suffix stay); every other name stays whole"""
    return [(s, re.sub(r"<[^>]*>", "", k).split("@")[0] if k.startswith(("gemm", "attn")) else k) for s, k in rows]


def test_without_level_the_launches_are_those_of_the_parent_commit(model, eng):
    """tests/golden/stretch_noop_launches.json holds what the commit before the stretch feature records for one eager FlowLM
    step and one codec frame, on the batcher's states and on the `TTSModel` context: built without `level`, both still record
    the same launches at the same sites in the same order, with the same kernel names wherever the tuner has no say"""
    from pocket_tts_amd.batching import ContinuousBatcher

    want = json.loads((G / "stretch_noop_launches.json").read_text())
    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    cb = ContinuousBatcher(model, slots=2, capacity=512)
    try:
        cb.submit(state, "ok")
        cb.run_until_idle()
        assert cb.lv is None and not cb.lagging and cb.pipe.out is None and cb.pipe.pcm[0].is_pinned()  # the buffers of before
        got = _step_launches(eng, cb.st, cb.ms)
    finally:
        cb.close()
    assert len(got) == len(want["batcher"]) == 25
    assert [s for s, _ in got] == [s for s, _ in want["batcher"]]
    assert _untuned(got) == _untuned(map(tuple, want["batcher"]))
    model.generate_audio(state, "ok")
    ctxs = [c for k, c in model._ctx_cache.items() if "speed" not in k and "rate" not in k and "level" not in k]
    assert ctxs and all(c["pipe"].lv is None and c["pipe"].out is None for c in ctxs)
    for c in ctxs:
        got = _step_launches(eng, c["st"], c["ms"])
        assert len(got) == len(want["model"]) == 25
        assert [s for s, _ in got] == [s for s, _ in want["model"]]
        assert _untuned(got) == _untuned(map(tuple, want["model"]))


def test_a_leveler_set_and_cleared_leaves_the_launches_of_before(eng):
    fresh, used = eng.new_mimi_state(2), eng.new_mimi_state(2)
    lv = eng.new_leveler(2, _plans("four"))
    try:
        want = _step_launches(eng, None, fresh)
        assert want and not any("level" in s or "level" in k for s, k in want)
        out = torch.zeros(2, lv.width, device=eng.device)
        used.set_leveler(lv, out)
        assert _step_launches(eng, None, used) == want + [("level", "level")]
        used.set_leveler(None)
        assert _step_launches(eng, None, used) == want
    finally:
        lv.close()
        fresh.close()
        used.close()
