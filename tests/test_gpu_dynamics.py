"""Per-request dynamics on the GPU: the compressor kernel against the serial float64 reference (tests/dynamics_ref.py) under
the bound of one fp32 rounding plus the float64 scheme's own error, exactness and isolation, streaming state, captured graphs,
the whole output chain - and the path through the continuous batcher, `TTSModel.generate_audio_stream`, the `generate` command
and the HTTP server (tiny model).

E_DB is the largest |s_chunked - s_serial| in dB of the float64 chunk / scan / re-run scheme over the rows below on their own
signals, measured on the CPU (tests/test_dynamics_cpu.py::test_e_of_the_gpu_tests_shapes prints it and holds it against this
file): 4.9e-13 for the rows of up to 1920 samples and 6.9e-13 for (48000, 7680)."""

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

import dynamics_ref
import level_ref
import tone_ref
from dynamics_ref import ODD, ROWS, WIDTH, F

E_DB = 1.0e-12
E_REL = E_DB * np.log(10.0) / 20.0  # E': the relative gain error of the float64 scheme

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"
SENTINEL_F = -77.0
GUARD = 4096
TEXT = "Hello world. This is a test."
SEEDED = dict(seed=77, temperature=0.7)


def _plans():
    from pocket_tts_amd.dynamics import plan

    return [plan(*r) for r in ROWS if r is not None]


def _plan_index(b):
    return None if ROWS[b] is None else sum(1 for r in ROWS[:b] if r is not None)


@pytest.fixture(scope="module")
def ref():
    """the rows' input streams and, for each compressed row, the float64 reference; computed once and left unchanged"""
    streams, refs = [], []
    for b, r in enumerate(ROWS):
        if r is None:
            streams.append(np.random.default_rng(100 + b).standard_normal(F * WIDTH).astype(np.float32))
            refs.append(None)
            continue
        rate, n, setting = r
        x = dynamics_ref.signal(n, 200 + b, b == ODD)
        y64, s = dynamics_ref.reference(setting, rate, x, n)
        fin = np.isfinite(x)
        assert np.array_equal(np.isnan(y64), np.isnan(x)) and np.array_equal(np.isinf(y64), np.isinf(x))
        assert (fin.all() if b != ODD else (~fin).sum() == 2) and np.abs(y64[fin][:3 * n]).max() > 0.01
        T = dynamics_ref.parse(setting)[0]
        loud = 20.0 * np.log10(np.maximum(np.abs(x[fin]), 1e-6)) > T
        assert 0.02 < loud.mean() < 0.9  # the signal crosses the threshold in both directions
        # the release rings out on the silence: no output, and a detector that is not at rest when the noise returns
        assert not y64[3 * n:5 * n].any() and s[5 * n - 1] > 0.0
        streams.append(x)
        refs.append(y64)
    for y in refs:
        if y is not None:
            y.setflags(write=False)
    return streams, refs


def _lines(streams, order=None, frames=F):
    """[frames, B, WIDTH] input lines: row b's frame at the front of its line, NaN behind it (nothing may read it)"""
    order = list(range(len(ROWS))) if order is None else order
    x = np.full((frames, len(order), WIDTH), np.nan, np.float32)
    for j, b in enumerate(order):
        n = WIDTH if ROWS[b] is None else ROWS[b][1]
        x[:, j, :n] = streams[b][:frames * n].reshape(frames, n)
    return x


def _guarded(eng, shape, fill, dtype=torch.float32):
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=eng.device)
    return big[GUARD:GUARD + n].view(*shape), big


def _run(eng, x, order=None, events=None):
    """x [frames, B, WIDTH] through a fresh Dynamics whose row j runs row `order[j]`; `events` = {frame: [j]}: set_row of row
    j again before that frame.  The output and the guard bands around it are pre-filled with sentinels before every frame.
    Returns outs [frames][B, WIDTH]"""
    order = list(range(len(ROWS))) if order is None else order
    B = len(order)
    dy = eng.new_dynamics(B, _plans(), WIDTH)
    try:
        assert dy.width == WIDTH and dy.row_plan == [-1] * B
        for j, b in enumerate(order):
            dy.set_row(j, _plan_index(b))
        outs = []
        for f in range(x.shape[0]):
            for j in (events or {}).get(f, ()):
                dy.set_row(j, dy.row_plan[j])
            out, out_big = _guarded(eng, (B, WIDTH), SENTINEL_F)
            xin, _ = _guarded(eng, (B, WIDTH), float("nan"))
            xin.copy_(torch.from_numpy(x[f]))
            dy.frame(xin, out)
            torch.cuda.synchronize()
            g = out_big.cpu().numpy()
            assert (g[:GUARD] == SENTINEL_F).all() and (g[-GUARD:] == SENTINEL_F).all(), "a write outside the buffer"
            assert np.array_equal(xin.cpu().numpy().view(np.uint32), x[f].view(np.uint32)), "the input was written"
            outs.append(out.cpu().numpy())
        return outs
    finally:
        dy.close()


def _stream_of(outs, j, n):
    return np.concatenate([o[j, :n] for o in outs])


def _bound(y64):
    """one fp32 rounding of the sample, plus ten times the float64 scheme's own relative error (ten: the device's log and exp
    are each a couple of float64 ulps from the host's, three orders below E)"""
    return 2.0 ** -24 * np.abs(y64) + 10.0 * E_REL * np.abs(y64)


def _check(y, y64, what):
    """NaN and Inf where the reference has them, and every other sample within `_bound`; returns the largest share of it"""
    fin = np.isfinite(y64)
    assert np.array_equal(np.isnan(y), np.isnan(y64)), (what, "NaN positions")
    assert np.array_equal(y[~fin], y64[~fin].astype(np.float32), equal_nan=True), (what, "Inf positions")
    err, bound = np.abs(y[fin].astype(np.float64) - y64[fin]), _bound(y64[fin])
    k = int(np.argmax(err / np.maximum(bound, 1e-300)))
    share = err[k] / max(bound[k], 1e-300)
    print(f"{what}: largest |y - y64| = {err.max():.3g}; largest share of the bound {share:.3f} at sample {k}")
    assert (err <= bound).all(), (what, k, err[k], bound[k])
    return share


@pytest.fixture(scope="module")
def model():
    """a model of this file's own: the contexts it leaves in the model's cache reach no other file's tests"""
    from pocket_tts_amd import TTSModel

    m = TTSModel.load_model(config=G / "e2e_tiny.yaml", temp=0.0)
    yield m
    m.engine.close()


@pytest.fixture(scope="module")
def eng(model):
    return model.engine


@pytest.fixture(scope="module")
def base(eng, ref):
    return _run(eng, _lines(ref[0]))


def test_against_the_reference(ref, base):
    streams, refs = ref
    worst = 0.0
    for b, r in enumerate(ROWS):
        if r is None:
            got = np.stack([o[b] for o in base])
            assert np.array_equal(got.view(np.uint32), streams[b].reshape(F, WIDTH).view(np.uint32))  # bypass: the whole line
            continue
        rate, n, setting = r
        for o in base:
            assert (o[b, n:] == SENTINEL_F).all(), (b, "written past the row's n")
        y, y64 = _stream_of(base, b, n), refs[b]
        assert y.shape == y64.shape
        worst = max(worst, _check(y, y64, f"dynamics row {b} {r}"))
    print(f"dynamics: worst share of the bound {worst:.3f}")


def test_a_row_is_bitwise_the_same_in_any_slot_and_any_batch(eng, ref, base):
    streams, _ = ref
    order = [5, 4, 4, 0, 3, 2, 1, 1, 5]
    outs = _run(eng, _lines(streams, order), order)
    for j, b in enumerate(order):
        n = WIDTH if ROWS[b] is None else ROWS[b][1]
        assert np.array_equal(_stream_of(outs, j, n).view(np.uint32), _stream_of(base, b, n).view(np.uint32)), (j, b)
    for b in (1, 3, 5):  # alone in a batch of one
        outs = _run(eng, _lines(streams, [b]), [b])
        n = ROWS[b][1]
        assert np.array_equal(_stream_of(outs, 0, n).view(np.uint32), _stream_of(base, b, n).view(np.uint32)), b


def test_set_row_restarts_a_row_from_zero_state(eng, ref, base):
    """rows that have run three frames and are set again: from there on they are fresh rows fed frames 3 ..; the others go on"""
    streams, _ = ref
    x = _lines(streams)
    x2 = np.concatenate([x[:3], x[:F - 3]])  # every row sees its first frames again from frame 3 on
    outs = _run(eng, x2, events={3: [1, 3, 5]})
    for b in (1, 3, 5):
        n = ROWS[b][1]
        assert np.array_equal(_stream_of(outs[3:], b, n).view(np.uint32), _stream_of(base[:F - 3], b, n).view(np.uint32)), b
    for b in (2, 4):  # a row that was not set again carries its state over: its frames 3 .. differ from a fresh row's
        n = ROWS[b][1]
        assert not np.array_equal(_stream_of(outs[3:], b, n), _stream_of(base[:F - 3], b, n), equal_nan=True)


def _frame_plans():
    from pocket_tts_amd.dynamics import plan

    return [plan(24000, 1920, "speech"), plan(24000, 1920, "broadcast"), plan(24000, 1920, dynamics_ref.CORNER)]


def test_captured_graph_follows_set_row(eng):
    """a codec graph captured with a compressor and a leveler: a later set_row to another plan and to bypass changes what its
    replays compute, without recapture, exactly as it changes stages of their own fed the same PCM frame by frame"""
    from pocket_tts_amd import level

    B = 3
    assert eng.frame_samples == 1920
    plans, lplans = _frame_plans(), [level.plan(24000, 1920)]
    ms = eng.new_mimi_state(B)
    dy, twin = eng.new_dynamics(B, plans), eng.new_dynamics(B, plans)
    lv, lv2 = eng.new_leveler(B, lplans), eng.new_leveler(B, lplans)
    g = None
    try:
        lat = torch.randn(B, eng.ldim, device=eng.device, generator=torch.Generator(eng.device).manual_seed(3))
        pcm = torch.zeros(B, 1920, device=eng.device)
        mid, mid2 = torch.full((B, 1920), SENTINEL_F, device=eng.device), torch.full((B, 1920), SENTINEL_F, device=eng.device)
        out, want = torch.full((B, 1920), SENTINEL_F, device=eng.device), torch.full((B, 1920), SENTINEL_F, device=eng.device)
        for s, v in ((dy, lv), (twin, lv2)):
            s.set_row(1, 0)
            s.set_row(2, 2)
            for b in range(B):
                v.set_row(b, 0, 0.0)
        ms.set_dynamics(dy, mid)
        ms.set_leveler(lv, out, mid)
        g = eng.capture_mimi(ms, lat, pcm)
        ms.set_leveler(None)
        ms.set_dynamics(None)
        u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731

        def step(tag):
            eng.graph_launch(g)
            eng.sync()
            twin.frame(pcm, mid2)
            lv2.frame(mid2, want)
            torch.cuda.synchronize()
            assert pcm.abs().max().item() > 0
            assert np.array_equal(u32(mid), u32(mid2)), tag
            assert np.array_equal(u32(out), u32(want)), tag
            return mid.cpu().numpy().copy(), pcm.cpu().numpy().copy()

        for f in range(3):
            a, x = step(("plain", f))
        assert np.array_equal(a[0], x[0]) and not np.array_equal(a[1], x[1]) and not np.array_equal(a[2], x[2])
        for s in (dy, twin):
            s.set_row(1, 1)   # another plan
            s.set_row(2, -1)  # to bypass
            s.set_row(0, 0)   # from bypass to a plan
        for f in range(3):
            b_, x = step(("set_row", f))
        assert np.array_equal(b_[2], x[2]) and not np.array_equal(b_[0], x[0]) and not np.array_equal(b_[1], x[1])
        # an eager decode on a state with the two stages appends the same launches
        ms.set_dynamics(dy, mid)
        ms.set_leveler(lv, out, mid)
        eng.mimi_decode(ms, lat, pcm)
        eng.sync()
        twin.frame(pcm, mid2)
        lv2.frame(mid2, want)
        torch.cuda.synchronize()
        assert np.array_equal(u32(out), u32(want))
        ms.set_leveler(None)
        ms.set_dynamics(None)
    finally:
        if g is not None:
            eng.graph_destroy(g)
        for s in (lv, lv2, dy, twin):
            s.close()
        ms.close()


def test_the_chain_in_one_graph_equals_its_stages_one_by_one(eng):
    """codec -> resampler -> toner -> compressor -> normaliser -> leveler -> encoder in one captured graph (an `OutputChain`
    of a table with these options), against stages of their own run one by one through f32 device buffers on the same PCM:
    bit for bit after every frame.  Row 0 at 8 kHz on every stage, row 1 at the native rate with a setting and a gain"""
    from pocket_tts_amd.output_chain import ChainTable, OutputChain

    B, fs, dev = 2, eng.frame_samples, eng.device
    table = ChainTable(eng.sample_rate, fs, sample_rates=[8000], loudness=True, encodings=["mulaw", "pcm_f32le"],
                       tones=["telephone"], dynamics=["speech", "broadcast"])
    routes = [table.route(sample_rate=8000, tone="telephone", dynamics="speech", loudness_lufs=-16.0, peak_dbfs=-3.0,
                          encoding="mulaw"),
              table.route(dynamics="broadcast", gain_db=3.0, encoding="pcm_f32le")]
    assert [r.dyn_plan is not None for r in routes] == [True, True] and routes[0].n_out == 640 and routes[1].n_out == fs
    ms = eng.new_mimi_state(B)
    chain = OutputChain(eng, B, table, 1)
    twins = [eng.new_resampler(B, table.sample_rates), eng.new_toner(B, table.tone_plans, table.width),
             eng.new_dynamics(B, table.dyn_plans, table.width), eng.new_normalizer(B, table.loud_plans),
             eng.new_leveler(B, table.level_plans), eng.new_encoder(B, table.width)]
    g = None
    try:
        assert [type(s) for s in chain.stages()] == [type(s) for s in twins]
        assert chain.dy is not None and chain.per_kind()[4] is chain.dy and len(chain.per_kind()) == 8
        bufs = [torch.full((B, table.width), SENTINEL_F, device=dev) for _ in twins[:-1]]
        bufs.append(torch.zeros(B, twins[-1].pitch, dtype=torch.uint8, device=dev))
        lat = torch.randn(B, eng.ldim, device=dev, generator=torch.Generator(dev).manual_seed(4))
        pcm = torch.zeros(B, fs, device=dev)
        chain.attach(ms, 0)
        g = eng.capture_mimi(ms, lat, pcm)
        chain.detach(ms)
        for b, r in enumerate(routes):
            chain.set_row(b, r)
            for s, args in zip(twins, ((r.rate_index,), (r.tone_plan,), (r.dyn_plan,), r.loud or (None, None),
                                       r.level or (None, None, None), (r.n_out, r.encoding))):
                s.set_row(b, *args)
        for f in range(7):  # D = 400 ms of the normaliser are over after five frames
            eng.graph_launch(g)
            eng.sync()
            x = pcm
            for s, y in zip(twins, bufs):
                s.frame(x, y)
                x = y
            torch.cuda.synchronize()
            for (got, want), s in zip(zip(chain._between, bufs[:-1]), twins):  # every buffer between two stages
                for b, r in enumerate(routes):
                    assert np.array_equal(got.cpu().numpy()[b, :r.n_out].view(np.uint32),
                                          want.cpu().numpy()[b, :r.n_out].view(np.uint32)), (f, b, type(s).__name__)
            line, want = chain.out[0].numpy(), bufs[-1].cpu().numpy()
            for b, r in enumerate(routes):
                nb = r.n_out * r.bytes_per_sample
                assert np.array_equal(line[b, :nb], want[b, :nb]), (f, b)
        last = bufs[-2].cpu().numpy()
        assert last[0, :640].any() and last[1].any() and np.isfinite(last[0, :640]).all() and np.isfinite(last[1]).all()
        dyn_in, dyn_out = bufs[1].cpu().numpy(), bufs[2].cpu().numpy()
        assert not np.array_equal(dyn_in[0, :640], dyn_out[0, :640]) and not np.array_equal(dyn_in[1], dyn_out[1])
    finally:
        if g is not None:
            eng.graph_destroy(g)
        for s in reversed(twins):
            s.close()
        chain.close()
        ms.close()


def test_cabi_error_codes(eng):
    import ctypes as C

    from pocket_tts_amd import dynamics, level

    plans = _frame_plans()
    dy = eng.new_dynamics(2, plans)
    try:
        lib, sp = eng.lib, eng._sp
        for row, idx in ((-1, 0), (2, 0), (0, -2), (0, 3), (0, 1 << 20)):  # bad row, bad plan index
            assert lib.ptts_dynamics_set_row(dy.handle, row, idx, sp) == -1, (row, idx)
            assert b"out of range" in lib.ptts_last_error()
        assert lib.ptts_dynamics_set_row(None, 0, 0, sp) == -1
        with pytest.raises(ValueError, match="plan index"):
            dy.set_row(0, 3)
        assert dy.row_plan == [-1, -1]
        x = torch.zeros(2, dy.width, device=eng.device)
        out = torch.zeros(2, dy.width, device=eng.device)
        px, po = C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr())
        assert lib.ptts_dynamics_frame(dy.handle, None, po, sp) == -1 and lib.ptts_dynamics_frame(dy.handle, px, None, sp) == -1
        assert lib.ptts_dynamics_frame(None, px, po, sp) == -1
        assert lib.ptts_dynamics_frame(dy.handle, px, px, sp) == -1 and b"in place" in lib.ptts_last_error()  # in == out
        for bad in (torch.zeros(2, dy.width - 1, device=eng.device), torch.zeros(3, dy.width, device=eng.device),
                    torch.zeros(2, dy.width, dtype=torch.float64, device=eng.device), torch.zeros(2, dy.width)):
            with pytest.raises(ValueError, match="compressor input"):  # width mismatch and friends, before the library is called
                dy.frame(bad, out)
            with pytest.raises(ValueError, match="compressor input"):
                dy.frame(x, bad)
        h = C.c_void_p()
        d = np.ascontiguousarray(plans[0].doubles())
        pd = d.ctypes.data_as(C.POINTER(C.c_double))
        ok = (C.c_int32 * 2)(24000, 1920)
        for args in ((None, 2, 0, ok, 1, pd, d.size, C.byref(h)), (eng.handle, 2, 0, None, 1, pd, d.size, C.byref(h)),
                     (eng.handle, 2, 0, ok, 1, None, d.size, C.byref(h)), (eng.handle, 2, 0, ok, 1, pd, d.size, None)):
            assert lib.ptts_dynamics_create(*args) == -1 and b"null argument" in lib.ptts_last_error()
        for batch, n_plans in ((0, 1), (-1, 1), (2, 0), (2, 1025)):
            assert lib.ptts_dynamics_create(eng.handle, batch, 0, ok, n_plans, pd, d.size * max(n_plans, 0), C.byref(h)) == -1
            assert b"out of range" in lib.ptts_last_error()
        for rate, n in ((7999, 640), (48001, 1920), (24000, 0), (24000, 8193), (24000, -1)):
            arr = (C.c_int32 * 2)(rate, n)  # a plan that breaks a rule never reaches the device
            assert lib.ptts_dynamics_create(eng.handle, 2, 0, arr, 1, pd, d.size, C.byref(h)) == -1
            assert b"not admissible" in lib.ptts_last_error()
        assert lib.ptts_dynamics_create(eng.handle, 2, 0, ok, 1, pd, d.size - 1, C.byref(h)) == -1
        assert b"doubles per plan" in lib.ptts_last_error()
        assert lib.ptts_dynamics_create(eng.handle, 2, 1919, ok, 1, pd, d.size, C.byref(h)) == -1  # a line narrower than a plan
        assert b"longer than the line" in lib.ptts_last_error()
        assert lib.ptts_dynamics_create(eng.handle, 2, 8193, ok, 1, pd, d.size, C.byref(h)) == -1
        for i, v in ((0, np.inf), (4, np.nan), (25, -np.inf)):
            bad = d.copy()
            bad[i] = v
            assert lib.ptts_dynamics_create(eng.handle, 2, 0, ok, 1, bad.ctypes.data_as(C.POINTER(C.c_double)), d.size, C.byref(h)) == -1
            assert b"not finite" in lib.ptts_last_error()
        for i, v in ((0, 1.0), (0, -61.0), (1, -0.5), (1, 1.0), (2, 25.0), (3, -1.0), (4, 1.0), (5, 0.0), (7, 1.5), (20, -0.1)):
            bad = d.copy()  # T, k, W, M, aA, aR and the powers outside the grammar's ranges: an expander, a decay that grows
            bad[i] = v
            assert lib.ptts_dynamics_create(eng.handle, 2, 0, ok, 1, bad.ctypes.data_as(C.POINTER(C.c_double)), d.size, C.byref(h)) == -1
            assert b"outside the range" in lib.ptts_last_error(), (i, v)
        assert dynamics.DOUBLES_PER_PLAN == d.size
        ms = eng.new_mimi_state(3)
        assert lib.ptts_mimi_set_dynamics(ms.handle, dy.handle, None, po) == -1 and b"batch" in lib.ptts_last_error()  # 3 vs 2
        ms.close()
        ms = eng.new_mimi_state(2)
        assert lib.ptts_mimi_set_dynamics(None, dy.handle, None, po) == -1
        assert lib.ptts_mimi_set_dynamics(ms.handle, dy.handle, None, None) == -1 and b"null output" in lib.ptts_last_error()
        assert lib.ptts_mimi_set_dynamics(ms.handle, dy.handle, po, po) == -1 and b"in place" in lib.ptts_last_error()
        # an input buffer means "behind an earlier stage": refused on a state that has none
        assert lib.ptts_mimi_set_dynamics(ms.handle, dy.handle, px, po) == -1 and b"input buffer" in lib.ptts_last_error()
        wide = eng.new_dynamics(2, plans, 2048)  # width mismatch: the compressor's line is not the state's frame
        wo = torch.zeros(2, 2048, device=eng.device)
        assert lib.ptts_mimi_set_dynamics(ms.handle, wide.handle, None, C.c_void_p(wo.data_ptr())) == -1
        assert b"frame length" in lib.ptts_last_error()
        wide.close()
        # a frame with a compressor but no leveler fails, and nothing of the compressor is enqueued before the check
        lat = torch.zeros(2, eng.ldim, device=eng.device)
        pcm = torch.zeros(2, eng.frame_samples, device=eng.device)
        assert lib.ptts_mimi_set_dynamics(ms.handle, dy.handle, None, po) == 0
        assert lib.ptts_mimi_decode(eng.handle, ms.handle, C.c_void_p(lat.data_ptr()), C.c_void_p(pcm.data_ptr()), sp) == -1
        assert b"compressor must be followed by a leveler" in lib.ptts_last_error()
        # the leveler accepts an input buffer on a state whose only earlier stage is the compressor
        lv = eng.new_leveler(2, [level.plan(24000, 1920)])
        out2 = torch.zeros(2, lv.width, device=eng.device)
        assert lib.ptts_mimi_set_leveler(ms.handle, lv.handle, po, C.c_void_p(out2.data_ptr()), 0) == 0
        assert lib.ptts_mimi_set_leveler(ms.handle, None, None, None, 0) == 0
        assert lib.ptts_mimi_set_dynamics(ms.handle, None, None, None) == 0
        eng.sync()
        lv.close()
        ms.close()
    finally:
        dy.close()


# ---- through the batcher, the model, the command and the server -------------------------------------------------------------
def _compressed_and_limited(wav_p, setting, rate=24000, n=1920, peak_dbfs=None):
    """the waveform without the setting through `dynamics_ref` and then `level_ref` at gain 0 dB, all in float64: (what the
    request delivers, the bound on |delivered - that|).  The compressor's share of the bound is `_bound` of its own output.
    Where no sample of the compressor's reference exceeds the ceiling, `level_ref` never reduces (r = 1 throughout, asserted)
    and the leveler is a delay of LA samples at a gain of exactly 1, so what is delivered is the compressor's output and that
    is all of the bound; the reference's own gain leaves 1 by some 5e-8 there, because it smooths in float64 with the plan's
    fp32 constants, so it is not what the samples are held against.  Where the attack lets a peak through and the limiter
    works, the samples are held against `level_ref`, and the leveler's own fp32 arithmetic comes on top, under the bound
    tests/test_gpu_level.py holds it to against the same reference, (LA + 64) 2^-24 of the largest sample it is fed"""
    from pocket_tts_amd import level

    y64, _ = dynamics_ref.reference(setting, rate, wav_p, n)
    lp = level.plan(rate, n)
    Gl, Cl = level.params(0.0, peak_dbfs)
    y, u, r, g = level_ref.level(np.concatenate([y64, np.zeros(lp.LA)]), Gl, Cl, lp.LA, lp.a, lp.k, full=True)
    y = y[lp.LA:lp.LA + wav_p.shape[0]]
    idle = bool((r == 1.0).all())
    assert idle == (np.abs(y64).max() <= float(Cl)) and np.array_equal(u[:y64.shape[0]], y64)
    print(f"{setting} at {rate} Hz: the reference's largest sample is {np.abs(y64).max():.4f} under a ceiling of {float(Cl):.4f}: "
          f"the limiter {'is idle' if idle else 'works'}; the reference's gain leaves 1 by {np.abs(g - 1.0).max():.3g}")
    if idle:
        return y64, _bound(y64)
    return y, _bound(y64) + (lp.LA + 64) * 2.0 ** -24 * np.abs(y64).max()


def _within(wav, want, bound, what):
    err = np.abs(wav.astype(np.float64) - want)
    k = int(np.argmax(err / np.maximum(bound, 1e-300)))
    print(f"{what}: largest |y - y64| = {err.max():.3g}; largest share of the bound {err[k] / max(bound[k], 1e-300):.3f}")
    assert (err <= bound).all(), (what, k, err[k], bound[k])


@pytest.fixture(scope="module")
def alone(model):
    """(frames, waveform) of the seeded TEXT as the only request of a fresh batcher with the leveler alone (2 slots), without
    a gain: the leveler's bypass, the model's own samples"""
    from pocket_tts_amd.batching import ContinuousBatcher

    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    cb = ContinuousBatcher(model, slots=2, capacity=512, level=True)
    try:
        assert cb.dy is None
        r = cb.submit(state, TEXT, **SEEDED)
        cb.run_until_idle()
        return r.frames, r.result().numpy()
    finally:
        cb.close()


def test_batcher_end_to_end(model, eng, alone):
    from pocket_tts_amd.batching import ContinuousBatcher

    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    frames, wav_p = alone
    assert wav_p.shape[0] == frames * 1920 and wav_p.any()
    cb = ContinuousBatcher(model, slots=2, capacity=512, dynamics=["speech", "threshold=-24;ratio=4;makeup=0"])
    try:
        assert cb.dy is not None and cb.lv is not None and cb.ln is None and cb.tn is None and cb.lagging
        with pytest.raises(ValueError, match="is not configured"):
            cb.submit(state, TEXT, dynamics="gentle")
        with pytest.raises(ValueError, match="ratio must be in"):
            cb.submit(state, TEXT, dynamics="ratio=0")
        with pytest.raises(ValueError, match="frames_after_eos >= 1"):
            cb.submit(state, TEXT, frames_after_eos=0, dynamics="speech")
        r = cb.submit(state, TEXT, dynamics="speech", **SEEDED)
        cb.run_until_idle()
        wav = r.result().numpy()
        assert r.frames == frames and wav.shape[0] == frames * 1920  # the sample counts of the plain request
        want, bound = _compressed_and_limited(wav_p, "speech")
        _within(wav, want, bound, "batcher, speech at 24 kHz")
        assert not np.array_equal(wav, wav_p)
        # then, in the slot the compressed request has left: a request without the field is bitwise the one of a batcher
        # built without the option
        r = cb.submit(state, TEXT, **SEEDED)
        cb.run_until_idle()
        assert np.array_equal(r.result().numpy().view(np.uint32), wav_p.view(np.uint32))
        # and a pair list, under its canonical form, with a ceiling of its own
        r = cb.submit(state, TEXT, dynamics=" Ratio=4 ; threshold=-24; makeup=0", peak_dbfs=0.0, **SEEDED)
        cb.run_until_idle()
        want, bound = _compressed_and_limited(wav_p, "threshold=-24;ratio=4;makeup=0", peak_dbfs=0.0)
        _within(r.result().numpy(), want, bound, "batcher, threshold=-24;ratio=4;makeup=0")
    finally:
        cb.close()
    cb = ContinuousBatcher(model, slots=2, capacity=512, level=True)
    try:
        with pytest.raises(ValueError, match="no dynamics stage"):
            cb.submit(state, TEXT, dynamics="speech")
    finally:
        cb.close()


def test_generate_audio_stream_the_command_and_the_server_field(model, eng, tmp_path, monkeypatch):
    import httpx

    from pocket_tts_amd import main, tts_model
    from pocket_tts_amd.server import create_app

    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    try:
        # 8 kHz, float32: the stream without the setting is the reference's input
        wav8 = np.concatenate([c.numpy() for c in model.generate_audio_stream(state, TEXT, sample_rate=8000)])
        chunks = [c.numpy() for c in model.generate_audio_stream(state, TEXT, dynamics="telephone", sample_rate=8000,
                                                                 encoding="pcm_f32le")]
        assert all(c.dtype == np.float32 and 0 < c.shape[0] <= 640 for c in chunks)
        f32 = np.concatenate(chunks)
        assert f32.shape == wav8.shape
        want, bound = _compressed_and_limited(wav8, "telephone", 8000, 640)
        _within(f32, want, bound, "model, telephone at 8 kHz")
        whole = model.generate_audio(state, TEXT, dynamics="telephone", sample_rate=8000, encoding="pcm_f32le").numpy()
        assert np.array_equal(whole.view(np.uint32), f32.view(np.uint32))
        with pytest.raises(ValueError, match="neither a preset"):
            model.generate_audio(state, TEXT, dynamics="loud")
        with pytest.raises(ValueError, match="makeup must be in"):
            model.generate_audio(state, TEXT, dynamics="makeup=25")
        assert any("dyn" in k[4:] and "level" in k[4:] for k in model._ctx_cache)
        # `generate --dynamics` writes the same samples as 16-bit PCM
        monkeypatch.setattr(tts_model.TTSModel, "load_model", staticmethod(lambda **kw: model))
        out = tmp_path / "o.wav"
        assert main.cli_app(["generate", "--voice", str(G / "e2e_voice.safetensors"), "--text", TEXT, "--dynamics", "Telephone",
                             "--sample-rate", "8000", "--output-path", str(out), "-q"]) == 0
        with wave.open(str(out), "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 8000)
            cli = np.frombuffer(w.readframes(w.getnframes()), np.int16)[:f32.shape[0]]
        assert np.abs(cli.astype(np.int64) - level_ref.pcm16(f32).astype(np.int64)).max() <= 1
        assert main.cli_app(["generate", "--voice", str(G / "e2e_voice.safetensors"), "--text", TEXT, "--dynamics", "knee=-1",
                             "--output-path", str(tmp_path / "no.wav"), "-q"]) == 1 and not (tmp_path / "no.wav").exists()
    finally:
        model._drop_rate_contexts(0)
    assert not any("dyn" in k[4:] for k in model._ctx_cache)

    shutil.copy(G / "e2e_voice.safetensors", tmp_path / "e2e_voice.safetensors")
    app = create_app(model, slots=2, capacity=512, voices_dir=tmp_path, default_voice="e2e_voice", sample_rates=[8000],
                     dynamics=["telephone", "speech"])
    plain = create_app(model, slots=2, capacity=512, voices_dir=tmp_path, default_voice="e2e_voice")

    async def go(app, forms):
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t", timeout=600) as cl:
                return [await cl.post("/tts", data=d) for d in forms]

    ok, other = asyncio.run(go(app, [{"text": TEXT, "dynamics": "telephone", "sample_rate": "8000"},
                                     {"text": TEXT, "dynamics": "gentle"}]))
    (without,) = asyncio.run(go(plain, [{"text": TEXT, "dynamics": "telephone"}]))
    assert other.status_code == 400 and "['telephone', 'speech']" in other.json()["detail"]
    assert without.status_code == 400 and "without dynamics" in without.json()["detail"]
    assert ok.status_code == 200, ok.text[:200]
    with wave.open(io.BytesIO(ok.content), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 8000)
    pcm = np.frombuffer(ok.content[44:], np.int16)[:f32.shape[0]]
    assert np.abs(pcm.astype(np.int64) - level_ref.pcm16(f32).astype(np.int64)).max() <= 1  # the same stream, as 16-bit samples


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


def test_without_dynamics_the_launches_are_those_of_the_parent_commit(model, eng):
    """tests/golden/stretch_noop_launches.json holds what the commit before the output chain records for one eager FlowLM
    step and one codec frame, on the batcher's states and on the `TTSModel` context: built without `dynamics`, both still
    record the same launches at the same sites in the same order"""
    from pocket_tts_amd.batching import ContinuousBatcher

    want = json.loads((G / "stretch_noop_launches.json").read_text())
    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    cb = ContinuousBatcher(model, slots=2, capacity=512)
    try:
        cb.submit(state, "ok")
        cb.run_until_idle()
        assert cb.dy is None and cb.tn is None and cb.lv is None and not cb.lagging and cb.pipe.out is None
        assert cb.pipe.pcm[0].is_pinned() and cb.pipe.dy is None
        got = _step_launches(eng, cb.st, cb.ms)
    finally:
        cb.close()
    assert len(got) == len(want["batcher"]) == 25
    assert [s for s, _ in got] == [s for s, _ in want["batcher"]]
    assert _untuned(got) == _untuned(map(tuple, want["batcher"]))
    model._drop_rate_contexts(0)
    model.generate_audio(state, "ok")
    ctxs = [c for k, c in model._ctx_cache.items() if len(k) == 4]
    assert ctxs and all(c["pipe"].dy is None and c["pipe"].lv is None and c["pipe"].out is None for c in ctxs)
    for c in ctxs:
        got = _step_launches(eng, c["st"], c["ms"])
        assert len(got) == len(want["model"]) == 25
        assert [s for s, _ in got] == [s for s, _ in want["model"]]
        assert _untuned(got) == _untuned(map(tuple, want["model"]))


def test_a_compressor_set_and_cleared_leaves_the_launches_of_before(eng):
    from pocket_tts_amd import level, loudness, tone

    fresh, used = eng.new_mimi_state(2), eng.new_mimi_state(2)
    tn = eng.new_toner(2, [tone.plan(24000, 1920, "warm")])
    dy = eng.new_dynamics(2, _frame_plans())
    ln = eng.new_normalizer(2, [loudness.plan(24000, 1920)])
    lv = eng.new_leveler(2, [level.plan(24000, 1920)])
    try:
        want = _step_launches(eng, None, fresh)
        assert want and not any("dynamics" in s or "dynamics" in k for s, k in want)
        m1, m2, m3, out = (torch.zeros(2, 1920, device=eng.device) for _ in range(4))
        used.set_dynamics(dy, m2)
        used.set_leveler(lv, out, m2)
        assert _step_launches(eng, None, used) == want + [("dynamics", "dynamics"), ("level", "level")]
        used.set_leveler(None)
        used.set_dynamics(None)
        assert _step_launches(eng, None, used) == want
        # between the toner's launch and the normaliser's
        used.set_tone(tn, m1)
        used.set_loudnorm(ln, m3, m1)
        used.set_leveler(lv, out, m3)
        without = _step_launches(eng, None, used)
        used.set_leveler(None)
        used.set_loudnorm(None)
        used.set_dynamics(dy, m2, m1)
        used.set_loudnorm(ln, m3, m2)
        used.set_leveler(lv, out, m3)
        with_dyn = _step_launches(eng, None, used)
        i = [s for s, _ in without].index("loudnorm")
        assert without[i - 1][0] == "tone" and with_dyn == without[:i] + [("dynamics", "dynamics")] + without[i:]
        for off in (used.set_leveler, used.set_loudnorm, used.set_dynamics, used.set_tone):
            off(None)
        assert _step_launches(eng, None, used) == want
    finally:
        for s in (lv, ln, dy, tn):
            s.close()
        fresh.close()
        used.close()
