"""Per-request speaking rate on the GPU: the WSOLA kernel against the fp64 reference (tests/stretch_ref.py) - the choice
of every hop, the overlap-add, exactness and isolation, streaming - and the path through the continuous batcher,
`TTSModel.generate_audio_stream` and the HTTP server (tiny model)."""

import asyncio
import ctypes as C
import io
import shutil
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

import stretch_ref

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"
N_FRAMES = 6
SENTINEL_F, SENTINEL_I, SENTINEL_D = -77.0, -12345, -99999
GUARD = 4096
TEXTS = ["Hello world. This is a test.", "ok", "How are you today?"]
# the impulse period of each row's input makes the best continuation fall on +D or -D at some hops (asserted below)
PERIODS = [300, 312, 384, 112]
SEEDS = [10, 11, 38, 13]  # with these no hop of the fp64 reference is a near-tie (asserted below)


def _plans():
    from pocket_tts_amd.stretch import identity, plan

    # a different n_in per row is on purpose: row 3 reads the first 640 samples of its line only
    return [identity(24000, 1920), plan(2.0, 24000, 1920), plan(0.5, 24000, 1920), plan(0.8, 8000, 640)]


def _signal(n, period, seed):
    """band-limited noise plus an impulse train (9-sample Hann pulses every `period` samples), float32, |x| < 1"""
    rng = np.random.default_rng(seed)
    h = np.hanning(33)
    x = np.convolve(rng.standard_normal(n + 32), h / h.sum(), mode="valid")[:n] * 0.3
    for s in range(period // 2, n - 9, period):
        x[s:s + 9] += 0.8 * np.hanning(9)
    return x.astype(np.float32)


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
def plans():
    return _plans()


@pytest.fixture(scope="module")
def streams(plans):
    """each row's input stream: N_FRAMES * n_in samples"""
    return [_signal(N_FRAMES * p.n_in, PERIODS[b], SEEDS[b]) for b, p in enumerate(plans)]


def _lines(plans, streams, order=None):
    """[frames, B, 1920] input lines: row b's frame at the front of its line, NaN behind it (nothing may read it)"""
    order = list(range(len(plans))) if order is None else order
    x = np.full((N_FRAMES, len(order), 1920), np.nan, np.float32)
    for j, b in enumerate(order):
        n = plans[b].n_in
        x[:, j, :n] = streams[b].reshape(N_FRAMES, n)
    return x


def _guarded(eng, shape, fill, dtype):
    """a contiguous device tensor of `shape` in the middle of a larger buffer filled with `fill`: (view, whole buffer)"""
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=eng.device)
    return big[GUARD:GUARD + n].view(*shape), big


def _run(eng, row_plans, x, i16=False, extra=0, events=None):
    """x [frames, B, 1920] through a fresh Stretcher whose row j runs `row_plans[j]`, then `extra` frames of NaN lines;
    `events` = {frame: [("set_row", row) | ("drain", row)]} applied before that frame.  The output, the delta tap and the
    guard bands around both are pre-filled with sentinels before every frame.  Returns (outs [frames][B, out_max],
    deltas [frames][B, k_max])."""
    B = len(row_plans)
    ts = eng.new_stretcher(B, _plans())
    table = [p.ints() for p in ts.plans]
    try:
        for j, p in enumerate(row_plans):
            ts.set_row(j, table.index(p.ints()))
        outs, deltas = [], []
        for f in range(x.shape[0] + extra):
            for kind, row in (events or {}).get(f, ()):
                if kind == "set_row":
                    ts.set_row(row, ts.row_plan[row])
                else:
                    ts.set_row_drain(row, True)
            out, out_big = _guarded(eng, (B, ts.out_max), SENTINEL_I if i16 else SENTINEL_F, torch.int16 if i16 else torch.float32)
            dl, dl_big = _guarded(eng, (B, ts.k_max), SENTINEL_D, torch.int32)
            line = x[f] if f < x.shape[0] else np.full_like(x[0], np.nan)
            xin, x_big = _guarded(eng, (B, 1920), float("nan"), torch.float32)
            xin.copy_(torch.from_numpy(line))
            ts.frame(xin, out, dl)
            torch.cuda.synchronize()
            for big, fill in ((out_big, SENTINEL_I if i16 else SENTINEL_F), (dl_big, SENTINEL_D)):
                g = big.cpu().numpy()
                assert (g[:GUARD] == fill).all() and (g[-GUARD:] == fill).all(), "a write outside the buffer"
            assert np.array_equal(xin.cpu().numpy().view(np.uint32), line.view(np.uint32)), "the input was written"
            outs.append(out.cpu().numpy())
            deltas.append(dl.cpu().numpy())
        return outs, deltas
    finally:
        ts.close()


@pytest.fixture(scope="module")
def base(eng, plans, streams):
    """the f32 and i16 runs every kernel test compares with: six single-frame calls, four rows in one launch"""
    x = _lines(plans, streams)
    out_f, dl = _run(eng, plans, x)
    out_i, dl_i = _run(eng, plans, x, i16=True)
    y, d = [], []
    for b, p in enumerate(plans):
        y.append(np.concatenate([out_f[f][b][:p.n_out] for f in range(N_FRAMES)]))
        d.append([] if p.identity else [int(v) for f in range(N_FRAMES) for v in dl[f][b][:p.K]])
    return dict(f=out_f, i=out_i, dl=dl, dl_i=dl_i, y=y, d=d, x=x)


def test_the_inputs_do_what_they_are_for(plans, streams):
    """by the fp64 reference alone: some hops pick +D and some -D, and wherever two candidates do not tie exactly the best
    leads the second best by at least twice the bound of test_choice_of_every_hop, so that an fp32 implementation within
    its error bound makes the reference's choices"""
    seen = set()
    for b, p in enumerate(plans):
        if p.identity:
            continue
        x = streams[b].astype(np.float64)
        _, d = stretch_ref.wsola(x, p, N_FRAMES)
        seen |= {v / p.D for v in d if abs(v) == p.D}
        for k in range(1, len(d)):
            s, a = stretch_ref.scores(x, p, k, (k - 1) * p.Ha - p.L + d[k - 1])
            top = np.sort(s)[-2:]
            assert top[1] == top[0] == 0 or top[1] - top[0] >= 2 * (2 * p.Hs * 2.0 ** -23 * a.max()), (b, k)
    assert seen == {-1.0, 1.0}


def test_choice_of_every_hop(base, plans, streams):
    """teacher-forced on the kernel's own previous delta, the kernel's delta scores within twice the fp32 dot-product error
    bound n 2^-24 sum|a b| of the fp64 maximum (once for each of the two scores compared): no hop is left out"""
    agree = total = 0
    for b, p in enumerate(plans):
        if p.identity:
            continue
        x, d = streams[b].astype(np.float64), base["d"][b]
        assert len(d) == N_FRAMES * p.K and d[0] == 0
        assert all(-p.D <= v <= p.D for v in d), (b, d)
        for k in range(1, len(d)):
            s, a = stretch_ref.scores(x, p, k, (k - 1) * p.Ha - p.L + d[k - 1])
            bound = 2 * p.Hs * 2.0 ** -23 * a.max()
            assert s[d[k] + p.D] >= s.max() - bound, (b, k, d[k], float(s[d[k] + p.D]), float(s.max()), bound)
            agree += d[k] == stretch_ref.choose(s, p.D)
            total += 1
        assert {abs(v) for v in d} & {p.D}, (b, d)  # the row did pick an end of its range
    print(f"fp32 and fp64 choices agree on {agree} of {total} hops")
    # rows that are not asked for deltas keep the tap's sentinel, as do the entries past a row's K
    assert (base["dl"][0][0] == SENTINEL_D).all()
    for b, p in enumerate(plans):
        if not p.identity:
            assert all((base["dl"][f][b][p.K:] == SENTINEL_D).all() for f in range(N_FRAMES))


def test_overlap_add_and_streaming(base, plans, streams):
    """six single-frame calls against the whole-signal reference, pre-roll included: with the kernel's deltas
    |y - y_ref| <= 4 * 2^-24 * max|x| (two products and one add per sample, w from the same fp32 table); where the fp64
    reference on its own makes the same choices (it does for these inputs) that is its own output"""
    for b, p in enumerate(plans):
        if p.identity:
            continue
        x = streams[b].astype(np.float64)
        want = stretch_ref.overlap_add(x, p, base["d"][b])
        y = base["y"][b]
        assert y.shape == want.shape == (N_FRAMES * p.n_out,)
        tol = 4 * 2.0 ** -24 * np.abs(x).max()
        err = np.abs(y.astype(np.float64) - want).max()
        print(f"row {b}: max |y - y_ref| = {err:.3g}, bound {tol:.3g}")
        assert err <= tol, (b, err, tol)
        own, d_own = stretch_ref.wsola(x, p, N_FRAMES)
        assert d_own == base["d"][b]
        assert np.abs(y.astype(np.float64) - own).max() <= tol
        assert y[p.preroll:].any() and not y[:((p.L - p.D - p.W) // p.Ha + 1) * p.Hs].any()


def test_i16_is_the_conversion_of_the_f32_output(base, plans):
    for b, p in enumerate(plans):
        for f in range(N_FRAMES):
            assert np.array_equal(base["i"][f][b][:p.n_out], stretch_ref.pcm16(base["f"][f][b][:p.n_out])), (b, f)
            assert (base["i"][f][b][p.n_out:] == SENTINEL_I).all(), (b, f)
            assert np.array_equal(base["dl_i"][f], base["dl"][f])


def test_identity_row_and_untouched_memory(base, plans):
    assert plans[0].identity
    for f in range(N_FRAMES):
        assert np.array_equal(base["f"][f][0][:1920].view(np.uint32), base["x"][f, 0].view(np.uint32))
        for b, p in enumerate(plans):
            # nothing beyond n_out of a row's line is written, and no NaN from behind a row's n_in was read
            assert (base["f"][f][b][p.n_out:] == SENTINEL_F).all(), (f, b)
            assert np.isfinite(base["f"][f][b][:p.n_out]).all(), (f, b)


def test_rows_do_not_depend_on_the_other_rows(eng, base, plans, streams):
    order = [2, 0, 3, 1]  # row j of the permuted run holds row order[j]'s plan and input
    outs, dl = _run(eng, [plans[b] for b in order], _lines(plans, streams, order))
    for j, b in enumerate(order):
        for f in range(N_FRAMES):
            n = plans[b].n_out
            assert np.array_equal(outs[f][j][:n].view(np.uint32), base["f"][f][b][:n].view(np.uint32)), (j, b, f)
    # and not on their plans: every other row on the identity plan
    for b in (1, 3):
        solo = [plans[0]] * 4
        solo[b] = plans[b]
        x = _lines(plans, streams)
        outs, _ = _run(eng, solo, x)
        for f in range(N_FRAMES):
            n = plans[b].n_out
            assert np.array_equal(outs[f][b][:n].view(np.uint32), base["f"][f][b][:n].view(np.uint32)), (b, f)


def test_set_row_restarts_one_row_only(eng, base, plans, streams):
    row, at = 2, 3
    x = _lines(plans, streams)
    outs, _ = _run(eng, plans, x, events={at: [("set_row", row)]})
    fresh, _ = _run(eng, plans, x[at:])  # frames 3.. as the start of a fresh stream
    n = plans[row].n_out
    for f in range(at, N_FRAMES):
        assert np.array_equal(outs[f][row][:n].view(np.uint32), fresh[f - at][row][:n].view(np.uint32)), f
    assert not np.array_equal(outs[at][row][:n], base["f"][at][row][:n])  # the carried state did matter
    for f in range(N_FRAMES):
        for b, p in enumerate(plans):
            if b != row or f < at:
                assert np.array_equal(outs[f][b][:p.n_out].view(np.uint32), base["f"][f][b][:p.n_out].view(np.uint32)), (f, b)


def test_drain_is_the_stream_followed_by_zeros(eng, base, plans, streams):
    """after set_row_drain a row's incoming frames (NaN here) count as zeros: the output is the reference of x || 0"""
    extra = max(p.drain_frames for p in plans)
    outs, dl = _run(eng, plans, _lines(plans, streams), extra=extra,
                    events={N_FRAMES: [("drain", b) for b in range(len(plans))]})
    for b, p in enumerate(plans):
        if p.identity:
            assert not outs[N_FRAMES][b][:p.n_out].any()  # a copy of zeros
            continue
        y = np.concatenate([outs[f][b][:p.n_out] for f in range(N_FRAMES + extra)])
        d = [int(v) for f in range(N_FRAMES + extra) for v in dl[f][b][:p.K]]
        x = streams[b].astype(np.float64)
        assert np.array_equal(y[:N_FRAMES * p.n_out], base["y"][b]) and d[:N_FRAMES * p.K] == base["d"][b]
        own, d_own = stretch_ref.wsola(x, p, N_FRAMES + extra)
        assert d == d_own, b
        assert np.abs(y - own).max() <= 4 * 2.0 ** -24 * np.abs(x).max()
        # the tail is there: pre-roll + frames * n_out samples are covered, and the last input samples shape the output
        assert p.preroll + N_FRAMES * p.n_out <= len(y) and y[N_FRAMES * p.n_out:p.preroll + N_FRAMES * p.n_out].any()


def test_tie_break_among_equal_scores(eng, plans):
    """Inputs that repeat bit for bit with period 2 d: the segments at +d and -d hold the same samples in the same places, so
    their fp32 scores are equal whatever the order of summation, and they are the maxima when the best continuation lies
    half a period off.  The kernel must take the negative one (equal |delta|); wherever the fp64 scores, teacher-forced on
    the kernel's previous delta, have several exact maxima, it must take the one the rule names."""
    periods = [None, 192, 160, 64]  # Hs - Ha = -480, +240, +32 is half a period off, modulo the period
    rng = np.random.default_rng(5)
    streams = [rng.uniform(-0.9, 0.9, N_FRAMES * p.n_in).astype(np.float32) if t is None else
               np.tile(rng.uniform(-0.9, 0.9, t).astype(np.float32), N_FRAMES * p.n_in // t + 1)[:N_FRAMES * p.n_in]
               for p, t in zip(plans, periods)]
    _, dl = _run(eng, plans, _lines(plans, streams))
    for b, p in enumerate(plans):
        if p.identity:
            continue
        x, half = streams[b].astype(np.float64), periods[b] // 2
        d = [int(v) for f in range(N_FRAMES) for v in dl[f][b][:p.K]]
        tied = 0
        for k in range(1, len(d)):
            s, a = stretch_ref.scores(x, p, k, (k - 1) * p.Ha - p.L + d[k - 1])
            assert s[d[k] + p.D] >= s.max() - 2 * p.Hs * 2.0 ** -23 * a.max(), (b, k)
            best = np.flatnonzero(s == s.max()) - p.D
            if len(best) > 1 and s.max() > 0:
                assert list(best) == [-half, half], (b, k, best)
                assert d[k] == stretch_ref.choose(s, p.D) == -half, (b, k, d[k])
                tied += 1
        assert tied >= 3, (b, d)


def test_captured_graph_follows_set_row_and_drain(eng, plans):
    """a codec graph captured with a stretcher: a later set_row and set_row_drain change what its replays compute, exactly
    as they change a stretcher of its own fed the same PCM frame by frame"""
    B = 4
    ms = eng.new_mimi_state(B)
    ts, twin = eng.new_stretcher(B, plans), eng.new_stretcher(B, plans)
    g = None
    try:
        lat = torch.randn(B, eng.ldim, device=eng.device, generator=torch.Generator(eng.device).manual_seed(3))
        pcm = torch.zeros(B, eng.frame_samples, device=eng.device)
        out = torch.full((B, ts.out_max), SENTINEL_F, device=eng.device)
        want = torch.full((B, ts.out_max), SENTINEL_F, device=eng.device)
        for b in range(B):
            ts.set_row(b, b)
            twin.set_row(b, b)
        ms.set_stretcher(ts, out)
        g = eng.capture_mimi(ms, lat, pcm)
        ms.set_stretcher(None)

        def step(tag):
            eng.graph_launch(g)
            eng.sync()
            twin.frame(pcm, want)
            torch.cuda.synchronize()
            assert pcm.abs().max().item() > 0
            assert np.array_equal(out.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32)), tag
            return out.cpu().numpy().copy()

        for f in range(3):
            a = step(("plain", f))
        for s in (ts, twin):
            s.set_row(1, 2)   # the 2.0 row moves to the 0.5 plan: 3840 samples from now on
            s.set_row(2, 0)   # and the 0.5 row to the identity
        b_ = step("set_row")
        assert (a[1][960:] == SENTINEL_F).all() and (b_[2][:1920] == pcm.cpu().numpy()[2]).all()
        for s in (ts, twin):
            s.set_row_drain(2, True)
            s.set_row_drain(3, True)
        c = step("drain")
        assert not c[2][:1920].any()
        # eager decodes on a state with a stretcher append the same launch
        ms.set_stretcher(ts, out)
        eng.mimi_decode(ms, lat, pcm)
        eng.sync()
        twin.frame(pcm, want)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
        ms.set_stretcher(None)
    finally:
        if g is not None:
            eng.graph_destroy(g)
        ts.close()
        twin.close()
        ms.close()


def test_cabi_error_codes(eng, plans):
    from pocket_tts_amd._lib import PttsError

    ts = eng.new_stretcher(2, plans)
    try:
        lib, sp = eng.lib, eng._sp
        for row, idx in ((-1, 0), (2, 0), (0, -1), (0, 4), (0, 1 << 20)):
            assert lib.ptts_stretcher_set_row(ts.handle, row, idx, sp) == -1, (row, idx)
            assert b"out of range" in lib.ptts_last_error()
        assert lib.ptts_stretcher_set_row_drain(ts.handle, 2, 1, sp) == -1 and lib.ptts_stretcher_set_row_drain(None, 0, 1, sp) == -1
        with pytest.raises(PttsError):
            ts.set_row(2, 0)
        assert ts.row_plan == [0, 0]
        x = torch.zeros(2, 1920, device=eng.device)
        out = torch.zeros(2, ts.out_max, device=eng.device)
        assert lib.ptts_stretch_frame(ts.handle, None, C.c_void_p(out.data_ptr()), 0, None, sp) == -1
        assert lib.ptts_stretch_frame(ts.handle, C.c_void_p(x.data_ptr()), None, 0, None, sp) == -1
        assert lib.ptts_stretch_frame(None, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), 0, None, sp) == -1
        # a plan that breaks a rule never reaches the device
        h = C.c_void_p()
        win = (C.c_float * 4096)()

        def create(*ints, floats=None):
            arr = (C.c_int32 * 5)(*ints)
            return lib.ptts_stretcher_create(eng.handle, 2, arr, 1, win, 2 * ints[2] if floats is None else floats, C.byref(h))

        assert create(1920, 640, 512, 144, 1280) == -1 and b"not admissible" in lib.ptts_last_error()  # L < D + W + Hs
        assert create(1920, 600, 512, 144, 1800) == -1      # no whole hops per frame
        assert create(1920, 640, 256, 144, 1280) == -1      # speed above 2
        assert create(1920, 640, 512, 144, 1920, floats=1000) == -1 and b"windows" in lib.ptts_last_error()
        ms = eng.new_mimi_state(3)
        assert lib.ptts_mimi_set_stretcher(ms.handle, ts.handle, None, C.c_void_p(out.data_ptr()), 0) == -1  # batch 3 vs 2
        ms.close()
        ms = eng.new_mimi_state(2)
        # an input buffer means "behind the resampler": refused on a state that has none
        assert lib.ptts_mimi_set_stretcher(ms.handle, ts.handle, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), 0) == -1
        ms.close()
    finally:
        ts.close()


# ---- through the batcher, the model and the server -------------------------------------------------------------------------
def _twin(eng, p, wav, n_in=1920, i16=False):
    """what a stretcher of its own makes of `wav` (whole frames of n_in samples) fed frame by frame on plan `p`, then drained:
    the pre-roll dropped, frames * n_out samples"""
    frames = wav.shape[0] // n_in
    assert frames * n_in == wav.shape[0]
    ts = eng.new_stretcher(1, [p])
    try:
        parts = []
        for f in range(frames + p.drain_frames):
            if f == frames:
                ts.set_row_drain(0, True)
            x = torch.zeros(1, n_in, device=eng.device)
            if f < frames:
                x[0] = torch.from_numpy(wav[f * n_in:(f + 1) * n_in])
            out = torch.zeros(1, p.n_out, dtype=torch.int16 if i16 else torch.float32, device=eng.device)
            ts.frame(x, out)
            torch.cuda.synchronize()
            parts.append(out.cpu().numpy()[0])
        return np.concatenate(parts)[p.preroll:p.preroll + frames * p.n_out]
    finally:
        ts.close()


@pytest.fixture(scope="module")
def alone(model):
    """alone(text, **kw) -> (frames, waveform) of one request that has a fresh batcher (2 slots, built with **kw) to itself.
    The bitwise comparisons below are all between requests that ran this way - alone, in slot 0, prefilled on their own:
    the codec's samples are reproducible bit for bit under the same placement and traffic, and only within a tolerance
    otherwise (tests/test_gpu_seed.py), which a bitwise check of the stretch must not depend on."""
    from pocket_tts_amd.batching import ContinuousBatcher

    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    cache = {}

    def run(text, **kw):
        key = (text, tuple(sorted((k, tuple(v)) for k, v in kw.items())))
        if key not in cache:
            cb = ContinuousBatcher(model, slots=2, capacity=512, **kw)
            try:
                r = cb.submit(state, text)
                cb.run_until_idle()
                cache[key] = (r.frames, r.result().numpy())
            finally:
                cb.close()
        return cache[key]

    return run


def test_batcher_end_to_end(model, eng, alone):
    from pocket_tts_amd.batching import ContinuousBatcher
    from pocket_tts_amd.stretch import plan

    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    p = plan(1.25)
    assert p.n_out == 1536
    assert len({alone(t)[0] for t in TEXTS}) > 1  # requests of different lengths
    placed = []
    cb = ContinuousBatcher(model, slots=2, capacity=512, speeds=[1.25])
    admit = cb._admit_group
    cb._admit_group = lambda jobs, rows: (placed.extend(int(b) for b in rows), admit(jobs, rows))[1]
    try:
        with pytest.raises(ValueError, match="not configured"):
            cb.submit(state, TEXTS[1], speed=1.5)
        with pytest.raises(ValueError, match="fraction"):
            cb.submit(state, TEXTS[1], speed=0.77)
        with pytest.raises(ValueError, match="frames_after_eos >= 1"):  # the batcher could not set the drain in time
            cb.submit(state, TEXTS[1], frames_after_eos=0, speed=1.25)
        # one after the other: each has the batcher to itself, and each but the first starts in the slot that a stretched
        # request has just drained and left
        for text, speed in ((TEXTS[0], 1.25), (TEXTS[2], 1.25), (TEXTS[1], None), (TEXTS[0], 1.25)):
            r = cb.submit(state, text, **({} if speed is None else {"speed": speed}))
            cb.run_until_idle()
            frames, wav = r.frames, r.result().numpy()
            frames_p, wav_p = alone(text)
            assert frames == frames_p and wav_p.shape[0] == frames_p * 1920
            if speed is None:  # a request without a speed on a batcher with speeds: bit-identical
                assert np.array_equal(wav.view(np.uint32), wav_p.view(np.uint32))
                continue
            assert wav.shape[0] == frames * 1536, (text, wav.shape, frames)
            assert np.array_equal(wav.view(np.uint32), _twin(eng, p, wav_p).view(np.uint32)), text
        assert placed == [0, 0, 0, 0]
        # three requests on two slots at once: the third waits for a slot while its predecessor drains
        reqs = [cb.submit(state, TEXTS[0], speed=1.25), cb.submit(state, TEXTS[1]), cb.submit(state, TEXTS[2], speed=1.25)]
        cb.run_until_idle()
        for r, text, n_out in zip(reqs, TEXTS, (1536, 1920, 1536)):
            wav = r.result().numpy()
            assert r.frames == alone(text)[0] and wav.shape[0] == r.frames * n_out and np.isfinite(wav).all() and wav.any()
    finally:
        cb.close()
    cb = ContinuousBatcher(model, slots=2, capacity=512)
    try:
        with pytest.raises(ValueError, match="1.0 only"):
            cb.submit(state, TEXTS[1], speed=1.25)
    finally:
        cb.close()


def test_batcher_with_rates_and_speeds(model, eng):
    """behind the resampler: a request at 8 kHz and 0.8 is the stretch of the same request at 8 kHz and 1.0"""
    from pocket_tts_amd.batching import ContinuousBatcher
    from pocket_tts_amd.stretch import plan

    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    with pytest.raises(ValueError, match="no multiple of 9"):
        ContinuousBatcher(model, slots=2, capacity=512, sample_rates=[8000], speeds=[0.9])
    cb = ContinuousBatcher(model, slots=2, capacity=512, sample_rates=[8000], speeds=[0.8, 1.5])
    try:
        with pytest.raises(ValueError, match=r"not admissible at 8000 Hz \(admissible there: \[1.0, 0.8\]\)"):
            cb.submit(state, TEXTS[0], sample_rate=8000, speed=1.5)
        got = []
        for kw in ({"sample_rate": 8000}, {"sample_rate": 8000, "speed": 0.8}, {"speed": 1.5}):  # one after the other
            r = cb.submit(state, TEXTS[0], **kw)
            cb.run_until_idle()
            got.append((r.frames, r.result().numpy()))
        (f0, w0), (f1, w1), (f2, w2) = got
    finally:
        cb.close()
    assert f0 == f1 == f2 and w0.shape[0] == f0 * 640 and w1.shape[0] == f0 * 800 and w2.shape[0] == f0 * 1280
    assert np.array_equal(w1.view(np.uint32), _twin(eng, plan(0.8, 8000, 640), w0, n_in=640).view(np.uint32))


def test_generate_audio_stream_speed(model, eng):
    from pocket_tts_amd.stretch import plan

    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    ref = model.generate_audio(state, TEXTS[0]).numpy()
    assert np.array_equal(model.generate_audio(state, TEXTS[0], speed=1.0).numpy(), ref)
    p = plan(1.25)
    chunks = [c.numpy() for c in model.generate_audio_stream(state, TEXTS[0], speed=1.25)]
    wav = np.concatenate(chunks)
    assert all(0 < c.shape[0] <= p.n_out for c in chunks)
    assert wav.shape[0] == ref.shape[0] // 1920 * 1536
    assert np.array_equal(wav.view(np.uint32), _twin(eng, p, ref).view(np.uint32))
    assert np.array_equal(model.generate_audio(state, TEXTS[0], speed=1.25).numpy(), wav)  # the cached context, restarted
    with pytest.raises(ValueError, match="no multiple of 9"):
        model.generate_audio(state, TEXTS[0], speed=0.9)
    with pytest.raises(ValueError, match="no multiple of 3"):
        model.generate_audio(state, TEXTS[0], speed=1.5, sample_rate=8000)
    assert sum(1 for k in model._ctx_cache if "speed" in k or "rate" in k) <= model.RATE_CONTEXTS


def test_server_speed(model, eng, alone, tmp_path):
    import httpx

    from pocket_tts_amd.server import create_app
    from pocket_tts_amd.stretch import plan

    shutil.copy(G / "e2e_voice.safetensors", tmp_path / "e2e_voice.safetensors")
    frames, wav_p = alone(TEXTS[0])
    app = create_app(model, slots=2, capacity=512, voices_dir=tmp_path, default_voice="e2e_voice", sample_rates=[8000],
                     speeds=[1.25, 1.5])

    async def go():
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t", timeout=600) as cl:
                # one after the other: each request has the batcher to itself, like the one it is compared with
                return [await cl.post("/tts", data=d) for d in ({"text": TEXTS[0], "speed": "1.25"}, {"text": TEXTS[0]},
                                                                 {"text": TEXTS[0], "speed": "0.8"},
                                                                 {"text": TEXTS[0], "speed": "1.5", "sample_rate": "8000"},
                                                                 {"text": TEXTS[0], "speed": "1.25", "frames_after_eos": "0"})]

    fast, normal, bad, bad_rate, bad_fae = asyncio.run(go())
    assert bad_fae.status_code == 400 and "frames_after_eos >= 1" in bad_fae.json()["detail"]
    assert bad.status_code == 400 and "not configured" in bad.json()["detail"]
    assert bad_rate.status_code == 400 and "not admissible at 8000 Hz" in bad_rate.json()["detail"]
    for r, n_out in ((fast, 1536), (normal, 1920)):
        assert r.status_code == 200, r.text[:200]
        with wave.open(io.BytesIO(r.content), "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 24000)
        assert len(r.content) - 44 == frames * n_out * 2 + 2 * 4800
        assert not np.frombuffer(r.content[-2 * 4800:], np.int16).any()
    assert np.array_equal(np.frombuffer(normal.content[44:], np.int16)[:frames * 1920], stretch_ref.pcm16(wav_p))
    assert np.array_equal(np.frombuffer(fast.content[44:], np.int16)[:frames * 1536], _twin(eng, plan(1.25), wav_p, i16=True))


# ---- no-op ------------------------------------------------------------------------------------------------------------------
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


def _codec_launches(eng, ms):
    return _step_launches(eng, None, ms)


def _untuned(rows):
    """the launch list with what the tuner chooses per process taken out of the names: the template arguments and the
    '@threads' of the GEMM and attention kernels (their family and prologue suffix stay); every other name stays whole"""
    import re

    return [(s, re.sub(r"<[^>]*>", "", k).split("@")[0] if k.startswith(("gemm", "attn")) else k) for s, k in rows]


def test_without_speeds_the_launches_are_those_of_the_parent_commit(model, eng):
    """tests/golden/stretch_noop_launches.json holds what the commit before this feature records for one eager FlowLM step
    and one codec frame, on the batcher's states and on the `TTSModel` context: built without `speeds`, both record the same
    launches at the same sites in the same order, with the same kernel names wherever the tuner has no say"""
    import json

    from pocket_tts_amd.batching import ContinuousBatcher

    want = json.loads((G / "stretch_noop_launches.json").read_text())
    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    cb = ContinuousBatcher(model, slots=2, capacity=512)
    try:
        cb.submit(state, "ok")
        cb.run_until_idle()
        got = _step_launches(eng, cb.st, cb.ms)
    finally:
        cb.close()
    assert len(got) == len(want["batcher"]) == 25
    assert [s for s, _ in got] == [s for s, _ in want["batcher"]]
    assert _untuned(got) == _untuned(map(tuple, want["batcher"]))
    model.generate_audio(state, "ok")
    ctxs = [c for k, c in model._ctx_cache.items() if "speed" not in k and "rate" not in k]
    assert ctxs
    for c in ctxs:
        got = _step_launches(eng, c["st"], c["ms"])
        assert len(got) == len(want["model"]) == 25
        assert [s for s, _ in got] == [s for s, _ in want["model"]]
        assert _untuned(got) == _untuned(map(tuple, want["model"]))


def test_without_speeds_the_launches_are_those_of_before(model, eng, plans):
    """A codec frame of a state without output stages is `mimi_enqueue` alone, which the feature does not touch.  The
    batcher and the `TTSModel` context built without `speeds` record, launch for launch, what a state that never saw an
    output stage records; one that had a stretcher and lost it records the same; with a stretcher there is exactly one
    more launch, the last one."""
    from pocket_tts_amd.batching import ContinuousBatcher

    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    for B, make in ((2, lambda: ContinuousBatcher(model, slots=2, capacity=512)),
                    (2, lambda: ContinuousBatcher(model, slots=2, capacity=512, speeds=[1.25]))):
        cb = make()
        try:
            cb.submit(state, TEXTS[1])
            cb.run_until_idle()
            fresh = eng.new_mimi_state(B)
            want = _codec_launches(eng, fresh)
            assert want and not any("stretch" in s or "stretch" in k or "resample" in k for s, k in want)
            assert _codec_launches(eng, cb.ms) == want
            if cb.ts is not None:
                out = torch.zeros(B, cb.ts.out_max, device=eng.device)
                fresh.set_stretcher(cb.ts, out)
                assert _codec_launches(eng, fresh) == want + [("stretch", "stretch")]
                fresh.set_stretcher(None)
                assert _codec_launches(eng, fresh) == want
            else:
                assert cb.pipe.out is None and cb.pipe.pcm[0].is_pinned()  # the buffers of before
            fresh.close()
        finally:
            cb.close()
    model.generate_audio(state, TEXTS[1])
    ctxs = [c for k, c in model._ctx_cache.items() if "speed" not in k and "rate" not in k]
    assert ctxs and all(c["pipe"].ts is None and c["pipe"].out is None for c in ctxs)
    fresh = eng.new_mimi_state(1)
    assert _codec_launches(eng, ctxs[0]["ms"]) == _codec_launches(eng, fresh)
    fresh.close()
