"""The leveler's true-peak mode on the GPU: the kernel against the float64 reference (tests/truepeak_ref.py) - error bound,
meter, int16 - the property the mode is for (the 4x meter reads the ceiling where the sample-peak limiter overshoots it by
3 dB), that rows without the mode compute bit for bit what they computed before, streaming state, captured graphs, the chain,
NaN, the C ABI's refusals, and the path through the batcher, the model, the command and the server (tiny model).

Observed on an MI355X: see the "true peak" section of DESIGN.md."""

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
import truepeak_ref as R

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"
SENTINEL_F, SENTINEL_I = -77.0, -12345
GUARD = 4096
TEXT = "Hello world. This is a test."
F = 6                                                             # frames
LINES = [(8000, 640), (11025, 882), (24000, 1920), (48000, 3840)]  # 11025: an odd LA; 48000: two tiles
GAINS = [-6.0, 0.0, 12.0]
# the rows of every batch: a true-peak row, a sample-peak row, a bypass row, a true-peak row set to drain after frame 3
KINDS = ("tp", "sp", "bypass", "tp_drain")
DRAIN_AT = 4  # the first frame the draining row reads as zeros


@pytest.fixture(scope="module")
def model():
    from pocket_tts_amd import TTSModel

    m = TTSModel.load_model(config=G / "e2e_tiny.yaml", temp=0.0)
    yield m
    m.engine.close()


@pytest.fixture(scope="module")
def eng(model):
    return model.engine


def _plan(line):
    from pocket_tts_amd.level import plan

    return plan(*line, True)


def _streams(line):
    """the rows' input streams: the limiter test's signal (full-scale single samples at frame and tile boundaries) for the
    limiting rows, another for the bypass row"""
    rate, n = line
    x = level_ref.gpu_signal(rate, n, frames=F)
    return {"tp": x, "sp": x, "bypass": level_ref.signal(F * n, seed=99), "tp_drain": x}


def _lines(line, kinds, streams=None):
    """[F, B, n] input lines"""
    streams = streams or _streams(line)
    return np.stack([streams[k].reshape(F, -1) for k in kinds], axis=1).astype(np.float32)


def _guarded(eng, shape, fill, dtype):
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=eng.device)
    return big[GUARD:GUARD + n].view(*shape), big


def _set(lv, j, kind, gain):
    if kind == "bypass":
        lv.set_row(j)
    else:
        lv.set_row(j, 0, gain, -1.0, kind != "sp")


def _run(eng, line, gain, x, kinds=KINDS, enabled=True, i16=False, extra=0, events=None):
    """x [frames, B, n] through a fresh leveler of the line's plan (with the mode unless `enabled` is False) whose row j is
    of kind `kinds[j]` at `gain` dB under -1 dB, then `extra` frames of NaN lines; a "tp_drain" row is set to drain before
    frame DRAIN_AT, `events` = {frame: [("set_row", j)]} are applied before that frame.  Output and guard bands are
    pre-filled with sentinels.  Returns (outs [frames][B, n], meters [B] read after the last frame)."""
    B = len(kinds)
    lv = eng.new_leveler(B, [_plan(line)], enabled) if enabled else eng.new_leveler(B, [_plan(line)])
    fill = SENTINEL_I if i16 else SENTINEL_F
    try:
        for j, kind in enumerate(kinds):
            _set(lv, j, kind, gain)
        outs = []
        for f in range(x.shape[0] + extra):
            for what, j in (events or {}).get(f, ()):
                assert what == "set_row"
                _set(lv, j, kinds[j], gain)
            if f == DRAIN_AT:
                for j, kind in enumerate(kinds):
                    if kind == "tp_drain":
                        lv.set_row_drain(j, True)
            out, out_big = _guarded(eng, (B, lv.width), fill, torch.int16 if i16 else torch.float32)
            src = x[f] if f < x.shape[0] else np.full_like(x[0], np.nan)
            xin, _ = _guarded(eng, (B, lv.width), float("nan"), torch.float32)
            xin.copy_(torch.from_numpy(src))
            lv.frame(xin, out)
            torch.cuda.synchronize()
            g = out_big.cpu().numpy()
            assert (g[:GUARD] == fill).all() and (g[-GUARD:] == fill).all(), "a write outside the buffer"
            assert np.array_equal(xin.cpu().numpy().view(np.uint32), src.view(np.uint32)), "the input was written"
            outs.append(out.cpu().numpy())
        meters = [lv.row_true_peak(j) for j in range(B)] if enabled else [None] * B
        return outs, meters
    finally:
        lv.close()


def _stream_of(outs, j):
    return np.concatenate([o[j] for o in outs])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


@pytest.fixture(scope="module")
def ref():
    """per (line, gain): the float64 references of the rows, computed once and left alone"""
    from pocket_tts_amd.level import TP_TAPS, params

    out = {}
    for line in LINES:
        p = _plan(line)
        s = _streams(line)
        for gain in GAINS:
            Gf, Cf = params(gain, -1.0)
            y, u, P, r, g, M = R.level_tp(s["tp"], Gf, Cf, p.LA, p.a, p.k, TP_TAPS, full=True)
            xd = s["tp_drain"].copy()
            xd[DRAIN_AT * p.n:] = 0.0
            yd, _, _, _, _, Md = R.level_tp(xd, Gf, Cf, p.LA, p.a, p.k, TP_TAPS, full=True)
            ysp = level_ref.level(s["sp"], Gf, Cf, p.LA, p.a, p.k)
            if gain > 0:
                assert 0.05 <= np.mean(r < 1) <= 0.6, (line, gain, np.mean(r < 1))  # the row limits, and not all the time
            elif gain == 0:
                assert (r < 1).any() and (g[DRAIN_AT * p.n - 1] < 1 or g[2 * p.n] < 1)  # at the full-scale samples only
            out[(line, gain)] = dict(tp=(y, M), tp_drain=(yd, Md), sp=ysp, umax=float(np.abs(u).max()), C=float(Cf), p=p)
    return out


@pytest.fixture(scope="module")
def base(eng):
    """the f32 outputs and the meters of every (line, gain), computed once"""
    return {(line, gain): _run(eng, line, gain, _lines(line, KINDS)) for line in LINES for gain in GAINS}


# ---- 2. the kernel against the float64 reference ----------------------------------------------------------------------------
@pytest.mark.parametrize("gain", GAINS)
@pytest.mark.parametrize("line", LINES)
def test_against_the_reference(ref, base, line, gain):
    from pocket_tts_amd.level import tp_error_bound

    Rf = ref[(line, gain)]
    p, umax, C = Rf["p"], Rf["umax"], Rf["C"]
    outs, meters = base[(line, gain)]
    bound = tp_error_bound(p.LA, umax, C) * umax
    for j, kind in enumerate(KINDS):
        y = _stream_of(outs, j)
        if kind == "bypass":
            assert np.array_equal(_bits(y), _bits(_streams(line)["bypass"])) and meters[j] is None
            continue
        assert np.isfinite(y).all()
        if kind == "sp":  # the sample-peak row beside them, under the bound of its own test
            err = float(np.abs(y - Rf["sp"]).max())
            assert err <= (p.LA + 64) * 2.0 ** -24 * umax and meters[j] is None
            continue
        y64, M64 = Rf[kind]
        err = float(np.abs(y.astype(np.float64) - y64).max())
        merr = abs(meters[j] - M64)
        print(f"true peak {line} {gain:+g} dB row {kind}: max|y - y64| = {err:.3e}, {err / bound:.4f} of the bound {bound:.3e}; "
              f"|M - M64| = {merr:.3e}, {merr / bound:.4f} of it; M / C = {meters[j] / C:.6f}, max|y| / C = "
              f"{np.abs(y).max() / C:.8f}")
        assert err <= bound, (line, gain, kind, err, bound)
        assert merr <= bound, (line, gain, kind, meters[j], M64)
        assert np.abs(y).max() <= C * (1 + (p.LA + 8) * 2.0 ** -24)  # the sample-peak bound still holds
        assert not y[:p.preroll].any()                               # the pre-roll: LA + 10 exact zeros
        if kind == "tp_drain":  # the tail, then exact zeros
            tail = y[DRAIN_AT * p.n:]
            assert tail[:p.preroll].any() and not tail[p.preroll:].any()


@pytest.mark.parametrize("line", LINES)
def test_int16_is_the_conversion_of_the_f32_output(eng, base, line):
    outs16, meters = _run(eng, line, 12.0, _lines(line, KINDS), i16=True)
    for o16, o in zip(outs16, base[(line, 12.0)][0]):
        assert np.array_equal(o16, level_ref.pcm16(o))
    assert meters == base[(line, 12.0)][1]  # the meter reads the f32 samples either way


# ---- 1. nothing existing moves ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("line", [(11025, 882), (48000, 3840)])
def test_a_sample_peak_row_is_bitwise_the_same_with_and_without_the_mode(eng, base, line):
    """the leveler has the mode or not; the other rows use it or not; any slot, any batch"""
    s = _streams(line)
    want = _stream_of(base[(line, 12.0)][0], 1)  # beside two true-peak rows on a leveler with the mode, slot 1 of 4
    one = np.stack([s["sp"].reshape(F, -1)], axis=1)
    for enabled, kinds, x, j in ((False, ("sp",), one, 0),                                  # no mode, alone
                                 (True, ("sp",), one, 0),                                   # the mode, nobody uses it
                                 (False, ("bypass", "sp", "sp"), _lines(line, ("bypass", "sp", "sp")), 2),
                                 (True, ("tp", "tp_drain", "bypass", "sp"), _lines(line, ("tp", "tp_drain", "bypass", "sp")), 3)):
        outs, _ = _run(eng, line, 12.0, x, kinds, enabled)
        assert np.array_equal(_bits(_stream_of(outs, j)), _bits(want)), (enabled, kinds)
    # and a true-peak row does not depend on its slot or its neighbours either
    outs, meters = _run(eng, line, 12.0, one, ("tp",))
    assert np.array_equal(_bits(_stream_of(outs, 0)), _bits(_stream_of(base[(line, 12.0)][0], 0)))
    assert meters[0] == base[(line, 12.0)][1][0]


def _step_launches(eng, st, ms):
    lat = torch.zeros(ms.batch, eng.ldim, device=eng.device)
    pcm = torch.zeros(ms.batch, eng.frame_samples, device=eng.device)
    eng.sync()
    eng.profile_start()
    if st is not None:
        eng.lm_decode_step(st, None, None, 1, float("inf"))
    eng.mimi_decode(ms, lat, pcm)
    return [(r["site"], r["kernel"]) for r in eng.profile_stop()]


def _untuned(rows):
    """the launch list without what the tuner chooses per process: the template arguments and '@threads' of the GEMM and
    attention kernels"""
    return [(s, re.sub(r"<[^>]*>", "", k).split("@")[0] if k.startswith(("gemm", "attn")) else k) for s, k in rows]


def test_without_true_peak_the_launches_and_buffers_are_those_of_the_parent_commit(model, eng):
    """tests/golden/truepeak_noop_launches.json holds what the commit before this feature records for one eager FlowLM step
    and one codec frame on a batcher built with `level=True`: built without `true_peak` it still records that, and its
    leveler has none of the mode's buffers"""
    from pocket_tts_amd.batching import ContinuousBatcher

    want = json.loads((G / "truepeak_noop_launches.json").read_text())
    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    cb = ContinuousBatcher(model, slots=2, capacity=512, level=True)
    try:
        cb.submit(state, "ok", gain_db=6)
        cb.run_until_idle()
        assert cb.lv is not None and not cb.lv.true_peak and not cb.chain.table.true_peak
        with pytest.raises(ValueError, match="no true-peak mode"):
            cb.lv.row_true_peak(0)
        with pytest.raises(ValueError, match="true_peak=True"):
            cb.submit(state, "ok", gain_db=6, peak_dbtp=-1)
        assert cb.pipe.out[0].shape == (2, 1920) and cb.pipe.out[0].is_pinned()
        cb.chain.attach(cb.ms, 0)  # as the batcher's captures see the state: the chain's launches behind the codec's
        try:
            got = _step_launches(eng, cb.st, cb.ms)
        finally:
            cb.chain.detach(cb.ms)
    finally:
        cb.close()
    assert [s for s, _ in got] == [s for s, _ in want["batcher_level"]]
    assert _untuned(got) == _untuned(map(tuple, want["batcher_level"]))
    assert got[-1] == ("level", "level")


# ---- 3. the property users buy ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.PROPERTY_INPUTS)
@pytest.mark.parametrize("line", [(8000, 640), (24000, 1920)])
def test_the_4x_meter_reads_the_ceiling(eng, line, name):
    """+12 dB under -1: what `level.true_peak` reads on the output of a sample-peak row (3 dB over the ceiling on the fs / 4
    sine at 45 degrees) and of a true-peak row (the ceiling, plus what the float64 reference itself exceeds it by on this
    input, plus 0.01 dB for fp32)"""
    from pocket_tts_amd.level import TP_TAPS, params, true_peak

    rate, n = line
    p = _plan(line)
    x = np.concatenate([R.property_input(name, rate, (F - 1) * n), np.zeros(n, np.float32)])  # the last frame flushes the tail
    Gf, Cf = params(12.0, -1.0)
    C = float(Cf)
    excess = max(true_peak(R.level_tp(x, Gf, Cf, p.LA, p.a, p.k, TP_TAPS)) / C, 1.0)
    lines = np.stack([x.reshape(F, -1)] * 2, axis=1)
    outs, meters = _run(eng, line, 12.0, lines, ("tp", "sp"))
    tp, sp = true_peak(_stream_of(outs, 0)), true_peak(_stream_of(outs, 1))
    print(f"true peak {line} {name}: the sample-peak row reads {20 * np.log10(sp / C):+.3f} dB over the ceiling, the true-peak "
          f"row {20 * np.log10(tp / C):+.4f} dB (the float64 reference {20 * np.log10(excess):+.4f} dB), its meter "
          f"{20 * np.log10(meters[0] / C):+.4f} dB")
    if name == "sine":
        assert sp >= C * 10 ** (2.9 / 20)
    assert tp <= C * excess * 10 ** (0.01 / 20)
    # the device meter is that reading, up to its own 21 fp32 products
    from pocket_tts_amd.level import TP_S

    assert abs(meters[0] - tp) <= 23 * 2.0 ** -24 * TP_S * float(np.abs(_stream_of(outs, 0)).max())


# ---- 4. stage behaviour -----------------------------------------------------------------------------------------------------
def test_set_row_restarts_the_state_and_the_meter(eng, base):
    line = (24000, 1920)
    x = _lines(line, KINDS)
    a, ma = _run(eng, line, 12.0, x[:4], events={2: [("set_row", 0)]})
    fresh, mf = _run(eng, line, 12.0, x[2:4])
    assert np.array_equal(_bits(_stream_of(a[2:], 0)), _bits(_stream_of(fresh, 0))) and ma[0] == mf[0]
    assert not np.array_equal(_stream_of(a[2:], 0), _stream_of(base[(line, 12.0)][0][2:4], 0))  # the state mattered
    for j in (1, 2, 3):  # the other rows carry on
        assert np.array_equal(_bits(_stream_of(a, j)), _bits(_stream_of(base[(line, 12.0)][0][:4], j)))
    whole, mw = _run(eng, line, 12.0, x[:4])
    assert mw[3] == ma[3]


@pytest.mark.parametrize("line", [(11025, 882), (48000, 3840)])
def test_drain_does_not_read_its_input_and_pushes_the_tail_through_the_meter(eng, ref, base, line):
    """after the flag the input lines hold NaN; the meter is that of the reference, whose stream ends in zeros, and `level.
    true_peak` of what the row wrote"""
    from pocket_tts_amd.level import TP_S, tp_error_bound, true_peak

    x = _lines(line, KINDS)
    x[DRAIN_AT:, 3, :] = np.nan
    outs, meters = _run(eng, line, 12.0, x, extra=1)
    y = _stream_of(outs, 3)
    assert np.array_equal(_bits(y[:F * line[1]]), _bits(_stream_of(base[(line, 12.0)][0], 3))) and not outs[F][3].any()
    Rf = ref[(line, 12.0)]
    assert abs(meters[3] - Rf["tp_drain"][1]) <= tp_error_bound(Rf["p"].LA, Rf["umax"], Rf["C"]) * Rf["umax"]
    assert abs(meters[3] - true_peak(y)) <= 23 * 2.0 ** -24 * TP_S * float(np.abs(y).max())


def test_a_nan_costs_one_output_sample(eng, base):
    """level.py, "True-peak mode": y[s + 10 + LA] is NaN and no other sample; the detector falls back to the sample peak
    where its window holds the NaN, so the ceiling still holds; the meter skips it"""
    line = (24000, 1920)
    p = _plan(line)
    x = _lines(line, KINDS)
    x[1, 0, 100] = np.nan     # row 0: frame 1, sample 100
    x[2, 3, 1919] = np.nan    # row 3: the last sample of frame 2, its output falls into frame 3
    outs, meters = _run(eng, line, 12.0, x)
    C = 10 ** (-1 / 20)
    for j, at in ((0, 1920 + 100 + p.preroll), (3, 2 * 1920 + 1919 + p.preroll)):
        y = _stream_of(outs, j)
        assert np.flatnonzero(np.isnan(y)).tolist() == [at]
        assert np.nanmax(np.abs(y)) <= C * (1 + (p.LA + 8) * 2.0 ** -24)
        assert np.isfinite(meters[j]) and meters[j] > 0
        far = np.arange(len(y)) < at - 2 * p.LA - 64  # before the NaN's window reaches them, nothing differs
        assert np.array_equal(_bits(y[far]), _bits(_stream_of(base[(line, 12.0)][0], j)[far]))
    for j in (1, 2):  # the other rows do not notice
        assert np.array_equal(_bits(_stream_of(outs, j)), _bits(_stream_of(base[(line, 12.0)][0], j)))


def test_captured_graph_follows_set_row_mode_and_drain(eng):
    """a codec graph captured with a leveler that has the mode: a later set_row (another mode, another gain) and
    set_row_drain change what its replays compute, exactly as they change a leveler of its own fed the same PCM"""
    from pocket_tts_amd.level import plan

    B = 4
    plans = [plan(24000, 1920), plan(8000, 640), plan(24000, 960)]
    ms = eng.new_mimi_state(B)
    lv, twin = eng.new_leveler(B, plans, True), eng.new_leveler(B, plans, True)
    g = None
    try:
        lat = torch.randn(B, eng.ldim, device=eng.device, generator=torch.Generator(eng.device).manual_seed(3))
        pcm = torch.zeros(B, eng.frame_samples, device=eng.device)
        out = torch.full((B, lv.width), SENTINEL_F, device=eng.device)
        want = torch.full((B, lv.width), SENTINEL_F, device=eng.device)
        for s in (lv, twin):
            s.set_row(1, 0, 24.0, -20.0, True)
            s.set_row(2, 1, 12.0)
            s.set_row(3, 2, 18.0, -6.0, True)
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
            assert [lv.row_true_peak(j) for j in range(B)] == [twin.row_true_peak(j) for j in range(B)], tag
            return out.cpu().numpy().copy(), pcm.cpu().numpy().copy()

        for f in range(3):
            a, x = step(("plain", f))
        assert np.array_equal(a[0], x[0]) and lv.row_true_peak(1) > 0 and lv.row_true_peak(2) is None
        assert (a[2][640:] == SENTINEL_F).all() and (a[3][960:] == SENTINEL_F).all()
        for s in (lv, twin):
            s.set_row(1, 0, 24.0, -20.0)        # the same gain and ceiling as a sample peak
            s.set_row(0, 0, 6.0, -1.0, True)    # the bypass row starts limiting, in the mode
        b_, _ = step("set_row")
        assert not np.array_equal(b_[1], a[1]) and not b_[0][:plans[0].LA + 10].any() and lv.row_true_peak(1) is None
        for s in (lv, twin):
            s.set_row_drain(0, True)
            s.set_row_drain(3, True)
        c, _ = step("drain")
        assert c[0][:plans[0].LA + 10].any() and not c[0][plans[0].LA + 10:].any()
        assert not c[3][plans[2].LA + 10:960].any()
    finally:
        if g is not None:
            eng.graph_destroy(g)
        lv.close()
        twin.close()
        ms.close()


def test_the_chain_in_one_graph_equals_its_stages_one_by_one(eng):
    """codec -> resampler (8 kHz) -> leveler in true-peak mode in one captured graph, against a resampler and a leveler of
    their own run one by one on the recorded intermediate buffer: bitwise, meters included"""
    from pocket_tts_amd import level

    B = 2
    ms = eng.new_mimi_state(B)
    lv_plans, lv_index = level.table([(24000, 1920), (8000, 640)])
    made = [(eng.new_resampler(B, [8000]), eng.new_leveler(B, lv_plans, True)) for _ in range(2)]
    (rs, lv), (rs2, lv2) = made
    g = None
    try:
        for a, c in made:
            a.set_row(0, a.index_of(8000))
            c.set_row(0, lv_index[(8000, 640)], 18.0, -6.0, True)
            c.set_row(1, lv_index[(24000, 1920)], 18.0, -1.0, True)
        lat = torch.randn(B, eng.ldim, device=eng.device, generator=torch.Generator(eng.device).manual_seed(4))
        pcm = torch.zeros(B, eng.frame_samples, device=eng.device)
        mid = torch.zeros(B, rs.out_max, device=eng.device)
        out = torch.full((B, lv.width), SENTINEL_F, device=eng.device)
        w1, w2 = torch.zeros_like(mid), torch.full_like(out, SENTINEL_F)
        ms.set_resampler(rs, mid)
        ms.set_leveler(lv, out, mid)
        g = eng.capture_mimi(ms, lat, pcm)
        ms.set_leveler(None)
        ms.set_resampler(None)
        for f in range(4):
            eng.graph_launch(g)
            eng.sync()
            rs2.frame(pcm, w1)
            torch.cuda.synchronize()
            assert np.array_equal(w1.cpu().numpy()[0, :640].view(np.uint32), mid.cpu().numpy()[0, :640].view(np.uint32)), f
            lv2.frame(mid, w2)
            torch.cuda.synchronize()
            assert np.array_equal(w2.cpu().numpy().view(np.uint32), out.cpu().numpy().view(np.uint32)), f
        o = out.cpu().numpy()
        assert (o[0, 640:] == SENTINEL_F).all() and o[0, :640].any() and o[1].any() and np.isfinite(o[1]).all()
        assert [lv.row_true_peak(j) for j in range(B)] == [lv2.row_true_peak(j) for j in range(B)]
        assert lv.row_true_peak(0) > 0 and lv.row_true_peak(1) > 0
    finally:
        if g is not None:
            eng.graph_destroy(g)
        for a, c in made:
            c.close()
            a.close()
        ms.close()


def test_cabi_error_codes(eng):
    import ctypes as C

    from pocket_tts_amd.level import TP_TAPS, LevelPlan, plan

    tight = LevelPlan(8000, 45, 40, np.float32(0.99), np.float32(1 / 40))  # admissible, but LA + 10 > n
    lv, plain = eng.new_leveler(2, [plan(24000, 1920), tight], True), eng.new_leveler(2, [plan(24000, 1920)])
    try:
        lib, sp = eng.lib, eng._sp
        taps = np.ascontiguousarray(TP_TAPS).ctypes.data_as(C.POINTER(C.c_float))
        v = C.c_float()
        assert lib.ptts_leveler_enable_true_peak(lv.handle, taps) == -1 and b"already" in lib.ptts_last_error()
        assert lib.ptts_leveler_enable_true_peak(None, taps) == -1 and lib.ptts_leveler_enable_true_peak(plain.handle, None) == -1
        bad = np.ascontiguousarray(TP_TAPS).copy()
        bad[1, 3] = np.nan
        assert lib.ptts_leveler_enable_true_peak(plain.handle, bad.ctypes.data_as(C.POINTER(C.c_float))) == -1
        for row, idx in ((-1, 0), (2, 0), (0, -1), (0, -2), (0, 2), (0, 1 << 20)):  # -1: bypass has no mode
            assert lib.ptts_leveler_set_row_tp(lv.handle, row, idx, 1.0, 0.5, sp) == -1, (row, idx)
            assert b"out of range" in lib.ptts_last_error()
        for gain, ceil in ((0.0, 0.5), (17.0, 0.5), (float("nan"), 0.5), (1.0, 0.0), (1.0, 1.5), (1.0, float("nan"))):
            assert lib.ptts_leveler_set_row_tp(lv.handle, 0, 0, gain, ceil, sp) == -1, (gain, ceil)
        assert lib.ptts_leveler_set_row_tp(lv.handle, 0, 1, 1.0, 0.5, sp) == -1 and b"LA + 10 exceeds n" in lib.ptts_last_error()
        assert lib.ptts_leveler_set_row(lv.handle, 0, 1, 1.0, 0.5, sp) == 0  # the same plan serves a sample-peak row
        assert lib.ptts_leveler_set_row_tp(plain.handle, 0, 0, 1.0, 0.5, sp) == -1 and b"no true-peak mode" in lib.ptts_last_error()
        assert lib.ptts_leveler_set_row_tp(None, 0, 0, 1.0, 0.5, sp) == -1 and b"null leveler" in lib.ptts_last_error()
        assert lib.ptts_leveler_row_true_peak(plain.handle, 0, C.byref(v), sp) == -1 and b"no true-peak mode" in lib.ptts_last_error()
        assert lib.ptts_leveler_row_true_peak(None, 0, C.byref(v), sp) == -1
        assert lib.ptts_leveler_row_true_peak(lv.handle, 2, C.byref(v), sp) == -1 and b"row out of range" in lib.ptts_last_error()
        assert lib.ptts_leveler_row_true_peak(lv.handle, 0, None, sp) == -1
        assert lib.ptts_leveler_row_true_peak(lv.handle, 0, C.byref(v), sp) == 0 and v.value == 0.0
        with pytest.raises(ValueError, match="no true-peak mode"):
            plain.set_row(0, 0, 6.0, -1.0, True)
        with pytest.raises(ValueError, match="plus the true-peak detector's delay"):
            lv.set_row(0, 1, 6.0, -1.0, True)
        with pytest.raises(ValueError, match="together with gain_db"):
            lv.set_row(0, None, None, None, True)
        assert lv.row_mode == [False, False]
    finally:
        lv.close()
        plain.close()


# ---- 5. through the batcher, the model, the command and the server -----------------------------------------------------------
# the largest excess of the float64 reference over the ceiling among the inputs of the property test (white noise at 8 kHz,
# DESIGN.md "true peak"), plus the 0.01 dB of that test for fp32
EXCESS_DB = 0.0066 + 0.01
FIELDS = dict(loudness_lufs=-16, peak_dbtp=-1)
ULAW_HALF_STEP = 128 / 8159  # half the widest interval of G.711 mu-law, of full scale


def _ceiling_ok(peak_linear):
    return 20 * np.log10(peak_linear) <= -1 + EXCESS_DB


@pytest.mark.parametrize("rate,encoding", [(8000, "mulaw"), (24000, None)])
def test_batcher_end_to_end(model, rate, encoding):
    import g711_ref
    from pocket_tts_amd.batching import ContinuousBatcher
    from pocket_tts_amd.level import TP_S, true_peak

    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    kw = dict(sample_rates=[8000], encodings=["mulaw"]) if encoding else {}
    req = dict(sample_rate=rate, encoding=encoding) if encoding else {}
    got = []
    for fields in (FIELDS, dict(loudness_lufs=-16, peak_dbfs=-1)):
        cb = ContinuousBatcher(model, slots=2, capacity=512, loudness=True, true_peak=True, **kw)
        try:
            assert cb.lv.true_peak
            if fields is FIELDS:
                with pytest.raises(ValueError, match="exclude each other"):
                    cb.submit(state, TEXT, loudness_lufs=-16, peak_dbfs=-1, peak_dbtp=-1)
                with pytest.raises(ValueError, match="frames_after_eos >= 1"):
                    cb.submit(state, TEXT, frames_after_eos=0, gain_db=6, peak_dbtp=-1)
            r = cb.submit(state, TEXT, **req, **fields)
            cb.run_until_idle()
            got.append((r, r.result().numpy()))
        finally:
            cb.close()
    (r, wav), (r0, wav0) = got
    assert r.frames == r0.frames and wav.shape == wav0.shape and wav.dtype == wav0.dtype  # the counts of the same request without
    assert r0.true_peak is None and r0.true_peak_dbtp is None
    assert r.true_peak > 0 and _ceiling_ok(r.true_peak), r.true_peak_dbtp
    assert r.true_peak_dbtp == pytest.approx(20 * np.log10(r.true_peak))
    if encoding:  # the delivered samples are the row's, up to the codec's quantisation
        y = g711_ref.ulaw2lin(wav).astype(np.float64) / 32768.0
        assert abs(true_peak(y) - r.true_peak) <= TP_S * ULAW_HALF_STEP
    else:
        assert wav.dtype == np.float32 and abs(true_peak(wav) - r.true_peak) <= 23 * 2.0 ** -24 * TP_S * float(np.abs(wav).max())
    if not encoding:  # and with a gain that makes the limiter work, under another ceiling
        cb = ContinuousBatcher(model, slots=2, capacity=512, true_peak=True)
        try:
            q = cb.submit(state, TEXT, gain_db=24, peak_dbtp=-6)
            cb.run_until_idle()
            loud = q.result().numpy()
        finally:
            cb.close()
        assert loud.shape == wav.shape and np.abs(loud).max() >= 0.9 * 10 ** (-6 / 20)
        assert 20 * np.log10(q.true_peak) <= -6 + EXCESS_DB, q.true_peak_dbtp
        assert abs(true_peak(loud) - q.true_peak) <= 23 * 2.0 ** -24 * TP_S * float(np.abs(loud).max())
        print(f"true peak, batcher at +24 dB under -6 dBTP: {q.true_peak_dbtp:+.4f} dBTP")
    print(f"true peak, batcher at {rate} Hz {encoding or 'f32'}: {r.true_peak_dbtp:+.4f} dBTP; the same request under a sample "
          f"peak reads {20 * np.log10(true_peak(wav0 if not encoding else g711_ref.ulaw2lin(wav0) / 32768.0)):+.3f}")


def test_generate_audio_stream(model):
    from pocket_tts_amd.level import TP_S, true_peak

    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    try:
        plain = model.generate_audio(state, TEXT, loudness_lufs=-16, peak_dbfs=-1).numpy()
        assert model.last_true_peak is None
        chunks = [c.numpy() for c in model.generate_audio_stream(state, TEXT, **FIELDS)]
        wav = np.concatenate(chunks)
        assert wav.shape == plain.shape and all(0 < c.shape[0] <= 1920 for c in chunks)
        assert _ceiling_ok(model.last_true_peak)
        assert abs(true_peak(wav) - model.last_true_peak) <= 23 * 2.0 ** -24 * TP_S * float(np.abs(wav).max())
        # 8 kHz mu-law, and the cached context again with a gain in place of the target
        import g711_ref

        u0 = model.generate_audio(state, TEXT, sample_rate=8000, encoding="mulaw", loudness_lufs=-16).numpy()
        assert model.last_true_peak is None
        u = model.generate_audio(state, TEXT, sample_rate=8000, encoding="mulaw", **FIELDS).numpy()
        assert u.shape == u0.shape and u.dtype == np.uint8 and _ceiling_ok(model.last_true_peak)
        assert abs(true_peak(g711_ref.ulaw2lin(u) / 32768.0) - model.last_true_peak) <= TP_S * ULAW_HALF_STEP
        with pytest.raises(ValueError, match="exclude each other"):
            model.generate_audio(state, TEXT, gain_db=6, peak_dbfs=-1, peak_dbtp=-1)
        with pytest.raises(ValueError, match="together with gain_db"):
            model.generate_audio(state, TEXT, peak_dbtp=-1)
        assert any("tp" in k[4:] for k in model._ctx_cache)
    finally:
        model._drop_rate_contexts(0)


def test_generate_logs_the_measured_true_peak(model, tmp_path, monkeypatch, caplog):
    import logging

    import g711_ref
    from pocket_tts_amd import main, tts_model
    from pocket_tts_amd.level import TP_S, true_peak

    monkeypatch.setattr(tts_model.TTSModel, "load_model", staticmethod(lambda **kw: model))
    caplog.set_level(logging.INFO)
    try:
        for extra, width in ((["--sample-rate", "8000", "--encoding", "mulaw"], 1), ([], 2)):
            out = tmp_path / f"o{width}.wav"
            caplog.clear()
            assert main.cli_app(["generate", "--voice", str(G / "e2e_voice.safetensors"), "--text", TEXT, "--loudness-lufs", "-16",
                                 "--peak-dbtp", "-1", *extra, "--output-path", str(out)]) == 0
            said = [m for m in caplog.messages if m.startswith("true peak ")]
            assert len(said) == 1 and re.fullmatch(r"true peak -?\d+\.\d\d dBTP", said[0]), caplog.messages
            db = float(said[0].split()[2])
            assert db <= -1 + EXCESS_DB + 0.005  # two decimals
            data = out.read_bytes()
            pcm = data[data.index(b"data") + 8:]
            y = g711_ref.ulaw2lin(np.frombuffer(pcm, np.uint8)) / 32768.0 if width == 1 else np.frombuffer(pcm, np.int16) / 32768.0
            tol = TP_S * (ULAW_HALF_STEP if width == 1 else 2.0 ** -16)
            assert abs(true_peak(y) - 10 ** (db / 20)) <= tol + 10 ** (db / 20) * (10 ** (0.005 / 20) - 1)
        assert main.cli_app(["generate", "--voice", str(G / "e2e_voice.safetensors"), "--text", TEXT, "--gain-db", "3", "--peak-dbfs",
                             "-1", "--peak-dbtp", "-1", "--output-path", str(tmp_path / "no.wav"), "-q"]) == 1
        assert not (tmp_path / "no.wav").exists()
    finally:
        model._drop_rate_contexts(0)


def test_server(model, tmp_path):
    import g711_ref
    import httpx

    from pocket_tts_amd.level import TP_S, true_peak
    from pocket_tts_amd.server import create_app

    shutil.copy(G / "e2e_voice.safetensors", tmp_path / "e2e_voice.safetensors")
    app = create_app(model, slots=2, capacity=512, voices_dir=tmp_path, default_voice="e2e_voice", sample_rates=[8000],
                     encodings=["mulaw"], loudness=True, true_peak=True)
    plain = create_app(model, slots=2, capacity=512, voices_dir=tmp_path, default_voice="e2e_voice", loudness=True)
    tp = {"loudness_lufs": "-16", "peak_dbtp": "-1"}

    async def go(app, forms):
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t", timeout=600) as cl:
                return [await cl.post("/tts", data=d) for d in forms]

    res = asyncio.run(go(app, [{"text": TEXT, **tp}, {"text": TEXT, "loudness_lufs": "-16"},
                               {"text": TEXT, "sample_rate": "8000", "encoding": "mulaw", **tp},
                               {"text": TEXT, "sample_rate": "8000", "encoding": "mulaw", "loudness_lufs": "-16"},
                               {"text": TEXT, "peak_dbfs": "-1", **tp}]))
    assert [r.status_code for r in res] == [200, 200, 200, 200, 400], [r.text[:200] for r in res]
    assert "exclude each other" in res[4].json()["detail"]
    assert len(res[0].content) == len(res[1].content) and len(res[2].content) == len(res[3].content)
    C = 10 ** (-1 / 20)
    with wave.open(io.BytesIO(res[0].content), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 24000)
    y = np.frombuffer(res[0].content[44:], np.int16) / 32768.0
    assert y.any() and true_peak(y) <= C * 10 ** (EXCESS_DB / 20) + TP_S * 2.0 ** -16
    data = res[2].content
    u = g711_ref.ulaw2lin(np.frombuffer(data[data.index(b"data") + 8:], np.uint8)) / 32768.0
    assert u.any() and true_peak(u) <= C * 10 ** (EXCESS_DB / 20) + TP_S * ULAW_HALF_STEP
    res = asyncio.run(go(plain, [{"text": TEXT, **tp}]))
    assert res[0].status_code == 400 and "without true_peak" in res[0].json()["detail"]
