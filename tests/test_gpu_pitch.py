"""Per-request pitch on the GPU: the pitch kernel against the composed fp64 reference (tests/pitch_ref.py) - the choice of
every hop, the mid line, the FIR, exactness and isolation, streaming - and the path through the continuous batcher,
`TTSModel.generate_audio` and the HTTP server (tiny model)."""

import asyncio
import ctypes as C
import io
import json
import shutil
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

import pitch_ref
import stretch_ref

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"
N_FRAMES = 6
SENTINEL_F, SENTINEL_I, SENTINEL_D, SENTINEL_M = -77.0, -12345, -99999, -55.0
GUARD = 4096
TEXTS = ["Hello world. This is a test.", "ok", "How are you today?"]
PERIODS = [300, 300, 312, 384, 112]
SEEDS = [10, 3, 1, 2, 0]  # with these no hop of the fp64 reference is a near-tie (asserted below)


def _plans():
    from pocket_tts_amd.pitch import identity, plan

    # a different n per row is on purpose: row 4 reads the first 640 samples of its line only
    return [identity(24000, 1920), plan("2/1", 24000, 1920), plan("1/2", 24000, 1920), plan("17/16", 24000, 1920),
            plan("4/5", 8000, 640)]


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
    """each row's input stream: N_FRAMES * n samples"""
    return [pitch_ref._signal(N_FRAMES * p.n, PERIODS[b], SEEDS[b]) for b, p in enumerate(plans)]


@pytest.fixture(scope="module")
def ref(plans, streams):
    """the all-fp64 reference of every row over the six frames and the drain frame (x || 0), computed once: y, mid, deltas"""
    out = []
    for p, x in zip(plans, streams):
        if p.identity:
            out.append(None)
            continue
        y, _, _, mid, deltas = pitch_ref.pitch(x.astype(np.float64), p, N_FRAMES + p.drain_frames, p.table)
        out.append(dict(y=y, mid=mid, d=deltas))
    return out


def _lines(plans, streams, order=None):
    """[frames, B, 1920] input lines: row b's frame at the front of its line, NaN behind it (nothing may read it)"""
    order = list(range(len(plans))) if order is None else order
    x = np.full((N_FRAMES, len(order), 1920), np.nan, np.float32)
    for j, b in enumerate(order):
        n = plans[b].n
        x[:, j, :n] = streams[b].reshape(N_FRAMES, n)
    return x


def _guarded(eng, shape, fill, dtype):
    """a contiguous device tensor of `shape` in the middle of a larger buffer filled with `fill`: (view, whole buffer)"""
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=eng.device)
    return big[GUARD:GUARD + n].view(*shape), big


def _run(eng, row_plans, x, i16=False, extra=0, events=None):
    """x [frames, B, 1920] through a fresh Pitcher whose row j runs `row_plans[j]`, then `extra` frames of NaN lines;
    `events` = {frame: [("set_row", row) | ("drain", row)]} applied before that frame.  The output, both taps and the guard
    bands around them are pre-filled with sentinels before every frame.  Returns (outs [frames][B, width], deltas
    [frames][B, k_max], mids [frames][B, mid_max])."""
    B = len(row_plans)
    ps = eng.new_pitcher(B, _plans())
    table = [p.ints() for p in ps.plans]
    try:
        for j, p in enumerate(row_plans):
            ps.set_row(j, table.index(p.ints()))
        outs, deltas, mids = [], [], []
        for f in range(x.shape[0] + extra):
            for kind, row in (events or {}).get(f, ()):
                if kind == "set_row":
                    ps.set_row(row, ps.row_plan[row])
                else:
                    ps.set_row_drain(row, True)
            out, out_big = _guarded(eng, (B, ps.width), SENTINEL_I if i16 else SENTINEL_F, torch.int16 if i16 else torch.float32)
            dl, dl_big = _guarded(eng, (B, ps.k_max), SENTINEL_D, torch.int32)
            md, md_big = _guarded(eng, (B, ps.mid_max), SENTINEL_M, torch.float32)
            line = x[f] if f < x.shape[0] else np.full_like(x[0], np.nan)
            xin, x_big = _guarded(eng, (B, 1920), float("nan"), torch.float32)
            xin.copy_(torch.from_numpy(line))
            ps.frame(xin, out, dl, md)
            torch.cuda.synchronize()
            for big, fill in ((out_big, SENTINEL_I if i16 else SENTINEL_F), (dl_big, SENTINEL_D), (md_big, SENTINEL_M)):
                g = big.cpu().numpy()
                assert (g[:GUARD] == fill).all() and (g[-GUARD:] == fill).all(), "a write outside the buffer"
            assert np.array_equal(xin.cpu().numpy().view(np.uint32), line.view(np.uint32)), "the input was written"
            outs.append(out.cpu().numpy())
            deltas.append(dl.cpu().numpy())
            mids.append(md.cpu().numpy())
        return outs, deltas, mids
    finally:
        ps.close()


def _cat(rows, b, n, frames):
    return np.concatenate([rows[f][b][:n] for f in range(frames)])


@pytest.fixture(scope="module")
def base(eng, plans, streams):
    """the f32 and i16 runs every kernel test compares with: six single-frame calls, five rows in one launch"""
    x = _lines(plans, streams)
    out_f, dl, md = _run(eng, plans, x)
    out_i, dl_i, md_i = _run(eng, plans, x, i16=True)
    y = [_cat(out_f, b, p.n, N_FRAMES) for b, p in enumerate(plans)]
    m = [None if p.identity else _cat(md, b, p.n_mid, N_FRAMES) for b, p in enumerate(plans)]
    d = [[] if p.identity else [int(v) for f in range(N_FRAMES) for v in dl[f][b][:p.K]] for b, p in enumerate(plans)]
    return dict(f=out_f, i=out_i, dl=dl, dl_i=dl_i, md=md, md_i=md_i, y=y, m=m, d=d, x=x)


def _fir_bound(p, mid32):
    """(y, bound, gain): the fp64 FIR over the kernel's own mid samples with its own fp32 table, and `StreamRef`'s bound"""
    return pitch_ref.fir(np.asarray(mid32, np.float64), p, p.table)


def test_the_inputs_do_what_they_are_for(plans, streams, ref):
    """by the fp64 reference alone, over the six frames and the drain frame: wherever two candidates do not tie exactly the
    best leads the second best by at least twice the bound of test_deltas, so that an fp32 implementation within its error
    bound makes the reference's choices; and some hops pick an end of the range"""
    ends = set()
    for b, p in enumerate(plans):
        if p.identity:
            continue
        sp, x, d = p.sp, streams[b].astype(np.float64), ref[b]["d"]
        assert len(d) == (N_FRAMES + p.drain_frames) * p.K
        ends |= {v // sp.D for v in d if abs(v) == sp.D}
        worst = np.inf
        for k in range(1, len(d)):
            s, a = stretch_ref.scores(x, sp, k, (k - 1) * sp.Ha - sp.L + d[k - 1])
            top = np.sort(s)[-2:]
            need = 2 * (2 * sp.Hs * 2.0 ** -23 * a.max())
            assert top[1] == top[0] == 0 or top[1] - top[0] >= need, (b, k)
            if top[1] != top[0]:
                worst = min(worst, (top[1] - top[0]) / need)
        print(f"row {b}: the smallest lead is {worst:.3g} times the required one")
    assert ends == {-1, 1}


def test_deltas(base, plans, streams, ref):
    """the kernel's deltas are the reference's at every hop (the margin above makes that a consequence of the fp32 dot
    product's error bound); teacher-forced on the kernel's own previous delta, each chosen score is within 2 Hs 2^-23 max a
    of the fp64 maximum"""
    for b, p in enumerate(plans):
        if p.identity:
            continue
        sp, x, d = p.sp, streams[b].astype(np.float64), base["d"][b]
        assert len(d) == N_FRAMES * p.K and d[0] == 0 and all(-sp.D <= v <= sp.D for v in d), (b, d)
        assert d == ref[b]["d"][:len(d)], b
        for k in range(1, len(d)):
            s, a = stretch_ref.scores(x, sp, k, (k - 1) * sp.Ha - sp.L + d[k - 1])
            bound = 2 * sp.Hs * 2.0 ** -23 * a.max()
            assert s[d[k] + sp.D] >= s.max() - bound, (b, k, d[k], float(s[d[k] + sp.D]), float(s.max()), bound)


def test_mid_line(base, plans, streams):
    """|mid - overlap_add(x, the kernel's deltas)| <= 4 * 2^-24 * max|x| (two products and one add per sample, w from the same
    fp32 table)"""
    for b, p in enumerate(plans):
        if p.identity:
            continue
        x = streams[b].astype(np.float64)
        want = stretch_ref.overlap_add(x, p.sp, base["d"][b])
        m = base["m"][b]
        assert m.shape == want.shape == (N_FRAMES * p.n_mid,)
        tol = 4 * 2.0 ** -24 * np.abs(x).max()
        err = np.abs(m.astype(np.float64) - want).max()
        print(f"row {b}: max |mid - mid_ref| = {err:.3g}, bound {tol:.3g}")
        assert err <= tol, (b, err, tol)


def test_fir_and_end_to_end(base, plans, streams, ref):
    """the f32 output against the fp64 FIR over the kernel's own mid samples with its own fp32 table, within `StreamRef`'s
    bound (T + 2) 2^-24 sum|h m| + 2^-24; and against the all-fp64 reference within that plus what the mid line's own error
    can contribute, (sum_j |table[ph][j]|) * 4 * 2^-24 * max|x|"""
    for b, p in enumerate(plans):
        if p.identity:
            continue
        y = base["y"][b].astype(np.float64)
        want, bound, gain = _fir_bound(p, base["m"][b])
        assert y.shape == want.shape == (N_FRAMES * p.n,)
        err = np.abs(y - want)
        print(f"row {b}: FIR max err {err.max():.3g}, largest err / bound {np.max(err / bound):.3g}")
        assert (err <= bound).all(), (b, float(np.max(err / bound)))
        full = ref[b]["y"][:N_FRAMES * p.n]
        tol = bound + gain * 4 * 2.0 ** -24 * np.abs(streams[b]).max()
        err = np.abs(y - full)
        print(f"row {b}: end to end max err {err.max():.3g}, largest err / bound {np.max(err / tol):.3g}")
        assert (err <= tol).all(), (b, float(np.max(err / tol)))
        assert y[p.preroll:].any()


def test_i16_is_the_conversion_of_the_f32_output(base, plans):
    for b, p in enumerate(plans):
        for f in range(N_FRAMES):
            assert np.array_equal(base["i"][f][b][:p.n], stretch_ref.pcm16(base["f"][f][b][:p.n])), (b, f)
            assert (base["i"][f][b][p.n:] == SENTINEL_I).all(), (b, f)
    for f in range(N_FRAMES):
        assert np.array_equal(base["dl_i"][f], base["dl"][f])
        assert np.array_equal(base["md_i"][f].view(np.uint32), base["md"][f].view(np.uint32))


def test_identity_row_and_untouched_memory(base, plans):
    assert plans[0].identity
    for f in range(N_FRAMES):
        assert np.array_equal(base["f"][f][0][:1920].view(np.uint32), base["x"][f, 0].view(np.uint32))
        # rows on the identity plan leave both taps alone
        assert (base["dl"][f][0] == SENTINEL_D).all() and (base["md"][f][0] == SENTINEL_M).all()
        for b, p in enumerate(plans):
            # nothing beyond n, n_mid or K of a row's line is written, and no NaN from behind a row's n was read
            assert (base["f"][f][b][p.n:] == SENTINEL_F).all(), (f, b)
            assert np.isfinite(base["f"][f][b][:p.n]).all(), (f, b)
            if not p.identity:
                assert (base["md"][f][b][p.n_mid:] == SENTINEL_M).all() and np.isfinite(base["md"][f][b][:p.n_mid]).all(), (f, b)
                assert (base["dl"][f][b][p.K:] == SENTINEL_D).all(), (f, b)


def test_rows_do_not_depend_on_the_other_rows(eng, base, plans, streams):
    order = [2, 4, 0, 3, 1]  # row j of the permuted run holds row order[j]'s plan and input
    outs, _, _ = _run(eng, [plans[b] for b in order], _lines(plans, streams, order))
    for j, b in enumerate(order):
        for f in range(N_FRAMES):
            n = plans[b].n
            assert np.array_equal(outs[f][j][:n].view(np.uint32), base["f"][f][b][:n].view(np.uint32)), (j, b, f)
    # and not on their plans: every other row on the identity plan
    for b in (1, 3, 4):
        solo = [plans[0]] * len(plans)
        solo[b] = plans[b]
        outs, _, _ = _run(eng, solo, _lines(plans, streams))
        for f in range(N_FRAMES):
            n = plans[b].n
            assert np.array_equal(outs[f][b][:n].view(np.uint32), base["f"][f][b][:n].view(np.uint32)), (b, f)


def test_set_row_restarts_one_row_only(eng, base, plans, streams):
    row, at = 3, 3
    x = _lines(plans, streams)
    outs, _, _ = _run(eng, plans, x, events={at: [("set_row", row)]})
    fresh, _, _ = _run(eng, plans, x[at:])  # frames 3.. as the start of a fresh stream
    n = plans[row].n
    for f in range(at, N_FRAMES):
        assert np.array_equal(outs[f][row][:n].view(np.uint32), fresh[f - at][row][:n].view(np.uint32)), f
    assert not np.array_equal(outs[at][row][:n], base["f"][at][row][:n])  # the carried state did matter
    for f in range(N_FRAMES):
        for b, p in enumerate(plans):
            if b != row or f < at:
                assert np.array_equal(outs[f][b][:p.n].view(np.uint32), base["f"][f][b][:p.n].view(np.uint32)), (f, b)


def test_drain_is_the_stream_followed_by_zeros(eng, base, plans, streams, ref):
    """after set_row_drain a row's incoming frames (NaN here) count as zeros: the output is the reference of x || 0"""
    extra = max(p.drain_frames for p in plans)
    assert extra == 1
    outs, dl, md = _run(eng, plans, _lines(plans, streams), extra=extra,
                        events={N_FRAMES: [("drain", b) for b in range(len(plans))]})
    for b, p in enumerate(plans):
        if p.identity:
            assert not outs[N_FRAMES][b][:p.n].any()  # a copy of zeros
            continue
        F = N_FRAMES + extra
        y, m = _cat(outs, b, p.n, F), _cat(md, b, p.n_mid, F)
        d = [int(v) for f in range(F) for v in dl[f][b][:p.K]]
        assert np.array_equal(y[:N_FRAMES * p.n], base["y"][b]) and d[:N_FRAMES * p.K] == base["d"][b]
        assert d == ref[b]["d"], b
        want, bound, gain = _fir_bound(p, m)
        tol = bound + gain * 4 * 2.0 ** -24 * np.abs(streams[b]).max()
        assert (np.abs(y - ref[b]["y"]) <= tol).all() and (np.abs(y - want) <= bound).all(), b
        # the tail is there: pre-roll + frames * n samples are covered, and the last input samples shape the output
        assert p.preroll + N_FRAMES * p.n <= len(y) and y[N_FRAMES * p.n:p.preroll + N_FRAMES * p.n].any()


def test_captured_graph_follows_set_row_and_drain(eng, plans):
    """a codec graph captured with a pitcher: a later set_row and set_row_drain change what its replays compute, exactly as
    they change a pitcher of its own fed the same PCM frame by frame"""
    B = 4
    table = plans[:4]  # the 24 kHz plans: identity, 2/1, 1/2, 17/16
    ms = eng.new_mimi_state(B)
    ps, twin = eng.new_pitcher(B, table), eng.new_pitcher(B, table)
    g = None
    try:
        lat = torch.randn(B, eng.ldim, device=eng.device, generator=torch.Generator(eng.device).manual_seed(3))
        pcm = torch.zeros(B, eng.frame_samples, device=eng.device)
        out = torch.full((B, ps.width), SENTINEL_F, device=eng.device)
        want = torch.full((B, ps.width), SENTINEL_F, device=eng.device)
        for b in range(B):
            ps.set_row(b, b)
            twin.set_row(b, b)
        ms.set_pitcher(ps, out)
        g = eng.capture_mimi(ms, lat, pcm)
        ms.set_pitcher(None)

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
        assert a[1].any() and a[3].any()  # past the pre-roll of 1680 / 1920 samples: the pitched rows sound
        for s in (ps, twin):
            s.set_row(1, 2)   # the 2/1 row moves to the 1/2 plan
            s.set_row(2, 0)   # and the 1/2 row to the identity
        b_ = step("set_row")
        assert not b_[1][:960].any() and (b_[2] == pcm.cpu().numpy()[2]).all()  # a fresh stream's pre-roll; a copy
        for s in (ps, twin):
            s.set_row_drain(2, True)
            s.set_row_drain(3, True)
        c = step("drain")
        assert not c[2].any() and c[3].any()
        # eager decodes on a state with a pitcher append the same launch
        ms.set_pitcher(ps, out)
        eng.mimi_decode(ms, lat, pcm)
        eng.sync()
        twin.frame(pcm, want)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
        ms.set_pitcher(None)
    finally:
        if g is not None:
            eng.graph_destroy(g)
        ps.close()
        twin.close()
        ms.close()


def test_cabi_error_codes(eng, plans):
    from pocket_tts_amd._lib import PttsError

    ps = eng.new_pitcher(2, plans)
    try:
        lib, sp = eng.lib, eng._sp
        for row, idx in ((-1, 0), (2, 0), (0, -1), (0, 5), (0, 1 << 20)):
            assert lib.ptts_pitcher_set_row(ps.handle, row, idx, sp) == -1, (row, idx)
            assert b"out of range" in lib.ptts_last_error()
        assert lib.ptts_pitcher_set_row_drain(ps.handle, 2, 1, sp) == -1 and lib.ptts_pitcher_set_row_drain(None, 0, 1, sp) == -1
        with pytest.raises(PttsError):
            ps.set_row(2, 0)
        assert ps.row_plan == [0, 0]
        x = torch.zeros(2, 1920, device=eng.device)
        out = torch.zeros(2, ps.width, device=eng.device)
        assert lib.ptts_pitch_frame(ps.handle, None, C.c_void_p(out.data_ptr()), 0, None, None, sp) == -1
        assert lib.ptts_pitch_frame(ps.handle, C.c_void_p(x.data_ptr()), None, 0, None, None, sp) == -1
        assert lib.ptts_pitch_frame(None, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), 0, None, None, sp) == -1
        # a plan that breaks a rule never reaches the device
        h = C.c_void_p()
        win, tab = (C.c_float * 4096)(), (C.c_float * 4096)()

        def create(*ints, floats=None, tfloats=None):
            arr = (C.c_int32 * 8)(*ints)
            return lib.ptts_pitcher_create(eng.handle, 2, arr, 1, win, 2 * ints[2] if floats is None else floats, tab,
                                           ints[6] * ints[7] if tfloats is None else tfloats, C.byref(h))

        assert create(1920, 480, 510, 144, 1440, 17, 16, 22) == -1 and b"not admissible" in lib.ptts_last_error()  # L too short
        assert create(1920, 480, 510, 144, 1920, 17, 15, 22) == -1      # Ha / Q != Hs / P
        assert create(1920, 480, 510, 144, 1920, 17, 16, 21) == -1      # the tap count
        assert create(1920, 480, 510, 144, 1920, 17, 16, 22, floats=1000) == -1 and b"windows" in lib.ptts_last_error()
        assert create(1920, 480, 510, 144, 1920, 17, 16, 22, tfloats=100) == -1 and b"tables" in lib.ptts_last_error()
        ms = eng.new_mimi_state(3)
        assert lib.ptts_mimi_set_pitcher(ms.handle, ps.handle, None, C.c_void_p(out.data_ptr()), 0) == -1  # batch 3 vs 2
        ms.close()
        ms = eng.new_mimi_state(2)
        # an input buffer means "behind another stage": refused on a state that has none
        assert lib.ptts_mimi_set_pitcher(ms.handle, ps.handle, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), 0) == -1
        # and the leveler accepts an input buffer behind a pitcher
        from pocket_tts_amd import level

        lv = eng.new_leveler(2, [level.plan(24000, 1920)])
        assert lib.ptts_mimi_set_leveler(ms.handle, lv.handle, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), 0) == -1
        ms.set_pitcher(ps, x)
        ms.set_leveler(lv, out, x)
        ms.set_leveler(None)
        ms.set_pitcher(None)
        lv.close()
        ms.close()
    finally:
        ps.close()


# ---- through the batcher, the model and the server -------------------------------------------------------------------------
def _twin(eng, p, wav, i16=False):
    """what a pitcher of its own makes of `wav` (whole frames of p.n samples) fed frame by frame on plan `p`, then drained:
    the pre-roll dropped, frames * n samples"""
    frames = wav.shape[0] // p.n
    assert frames * p.n == wav.shape[0]
    ps = eng.new_pitcher(1, [p])
    try:
        parts = []
        for f in range(frames + p.drain_frames):
            if f == frames:
                ps.set_row_drain(0, True)
            x = torch.zeros(1, p.n, device=eng.device)
            if f < frames:
                x[0] = torch.from_numpy(wav[f * p.n:(f + 1) * p.n])
            out = torch.zeros(1, p.n, dtype=torch.int16 if i16 else torch.float32, device=eng.device)
            ps.frame(x, out)
            torch.cuda.synchronize()
            parts.append(out.cpu().numpy()[0])
        return np.concatenate(parts)[p.preroll:p.preroll + frames * p.n]
    finally:
        ps.close()


def _raw(eng, stage, n_in, n_out, src, frames, drain_at):
    """the raw lines, pre-roll and tail included, that `stage` (a stretcher or a pitcher of one row on its plan) makes of the
    stream `src` fed frame by frame and set to drain before frame `drain_at`: frames * n_out samples"""
    parts = []
    for f in range(frames):
        if f == drain_at:
            stage.set_row_drain(0, True)
        x = torch.zeros(1, n_in, device=eng.device)
        if (f + 1) * n_in <= len(src):
            x[0] = torch.from_numpy(src[f * n_in:(f + 1) * n_in])
        out = torch.zeros(1, n_out, device=eng.device)
        stage.frame(x, out)
        torch.cuda.synchronize()
        parts.append(out.cpu().numpy()[0])
    return np.concatenate(parts)


def _against_the_reference(got, src, p, tag, skip=0):
    """`got`: the samples a pitched request delivered; `src`: the stream its pitcher was fed from the row's start (zeros
    behind its end), of which `got` answers the part that starts at `skip`.  The fp64 reference of src || 0 makes the kernel's
    choices as long as no hop is a near-tie (the margin of test_the_inputs_do_what_they_are_for); the samples that the hops
    before the first near-tie decide are compared within the end-to-end bound of test_fir_and_end_to_end.  Returns the share
    of the hops that were compared."""
    lo = skip + p.preroll
    frames = -(-(lo + len(got)) // p.n)
    x, sp = np.zeros(frames * p.n), p.sp
    x[:min(len(src), len(x))] = src[:len(x)]
    y, bound, gain, _, d = pitch_ref.pitch(x, p, frames, p.table)
    safe = len(d)
    for k in range(1, len(d)):
        s, a = stretch_ref.scores(x, sp, k, (k - 1) * sp.Ha - sp.L + d[k - 1])
        top = np.sort(s)[-2:]
        if not (top[1] == top[0] == 0 or top[1] - top[0] >= 2 * (2 * sp.Hs * 2.0 ** -23 * a.max())):
            safe = k
            break
    # the mid samples before safe * Hs are final after hop safe - 1; output N reads mid samples up to N P / Q
    n_ok = min(len(y), safe * sp.Hs * p.Q // p.P)
    tol = bound + gain * 4 * 2.0 ** -24 * np.abs(x).max()
    hi = min(lo + len(got), n_ok)
    err = np.abs(got[:max(hi - lo, 0)].astype(np.float64) - y[lo:hi])
    print(f"{tag}: {safe} of {len(d)} hops compared, {max(hi - lo, 0)} of {len(got)} samples, "
          f"largest err / bound {np.max(err / tol[lo:hi]) if len(err) else 0:.3g}")
    assert (err <= tol[lo:hi]).all(), tag
    return safe / len(d)


def _three(model, **kw):
    """the three requests (pitch None, 17/16, 4/5) on a fresh batcher of 4 slots built with **kw, submitted together:
    [(frames, samples)]"""
    from pocket_tts_amd.batching import ContinuousBatcher

    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    cb = ContinuousBatcher(model, slots=4, capacity=512, **kw)
    try:
        pitches = (None, "17/16", "4/5") if kw else (None, None, None)
        reqs = [cb.submit(state, t, **({} if p is None else {"pitch": p})) for t, p in zip(TEXTS, pitches)]
        cb.run_until_idle()
        return [(r.frames, r.result().numpy()) for r in reqs], cb.chain.ps is None and cb.pipe.out is None
    finally:
        cb.close()


def test_batcher_end_to_end(model, eng):
    """the same three requests, submitted together, on a batcher without pitches and on one with them: the same placement and
    traffic, so the codec's samples are the same bits and the pitched requests are the pitch of the unpitched run's samples"""
    from pocket_tts_amd.batching import ContinuousBatcher
    from pocket_tts_amd.pitch import plan

    plain, bare = _three(model)
    pitched, _ = _three(model, pitches=["17/16", "4/5"])
    assert bare and len({f for f, _ in plain}) > 1  # requests of different lengths
    for (f0, w0), (f1, w1), r in zip(plain, pitched, (None, "17/16", "4/5")):
        assert f0 == f1 and w0.shape == w1.shape == (f0 * 1920,)
        if r is None:
            assert np.array_equal(w0.view(np.uint32), w1.view(np.uint32))
            continue
        assert np.isfinite(w1).all() and w1.any() and not np.array_equal(w0, w1)
        assert _against_the_reference(w1, w0, plan(r), f"batcher {r}") >= 0.9
    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    cb = ContinuousBatcher(model, slots=2, capacity=512, pitches=["17/16"])
    try:
        with pytest.raises(ValueError, match="not configured"):
            cb.submit(state, TEXTS[1], pitch="5/4")
        with pytest.raises(ValueError, match="fraction"):
            cb.submit(state, TEXTS[1], pitch=0.77)
        with pytest.raises(ValueError, match="frames_after_eos >= 1"):
            cb.submit(state, TEXTS[1], frames_after_eos=0, pitch="17/16")
        # alone in slot 0: bitwise a pitcher of its own over the unpitched request's samples, which ran the same way
        got = []
        for kw in ({}, {"pitch": "17/16"}):
            r = cb.submit(state, TEXTS[0], **kw)
            cb.run_until_idle()
            got.append((r.frames, r.result().numpy()))
        (f0, w0), (f1, w1) = got
        assert f0 == f1 and np.array_equal(w1.view(np.uint32), _twin(eng, plan("17/16"), w0).view(np.uint32))
    finally:
        cb.close()
    cb = ContinuousBatcher(model, slots=2, capacity=512)
    try:
        with pytest.raises(ValueError, match="pitch 1.0 only"):
            cb.submit(state, TEXTS[1], pitch="17/16")
    finally:
        cb.close()


def test_full_chain(model, eng):
    """rates [16000], speeds [1.25], pitches [5/4], level: the request (16000, 1.25, 5/4, +6 dB) delivers exactly F * 1024
    samples under the ceiling, and equals the composition of the fp64 references stage by stage.  The same text runs four
    times alone in slot 0 (the stages before a new one are then the same bits): at 16 kHz, then with the speed, the pitch and
    the gain added one by one.  A stretcher and a pitcher of their own, fed what the run before delivered, give the raw lines
    (pre-roll and tail included) that the next stage read; their slices are the runs' samples bit for bit.  The pitcher's
    fp64 reference over its raw input holds within the end-to-end bound of the kernel test wherever its hops had no near-tie
    before, the leveler's over its raw input within its bound (LA + 64) 2^-24 max|u| (tests/test_gpu_level.py).
    Text: TEXTS[0]."""
    import level_ref

    from pocket_tts_amd import level, stretch
    from pocket_tts_amd.batching import ContinuousBatcher
    from pocket_tts_amd.pitch import plan

    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    cb = ContinuousBatcher(model, slots=2, capacity=512, sample_rates=[16000], speeds=[1.25], pitches=["5/4"], level=True)
    try:
        got = []
        for kw in ({}, {"speed": 1.25}, {"speed": 1.25, "pitch": "5/4"}, {"speed": 1.25, "pitch": "5/4", "gain_db": 6.0}):
            r = cb.submit(state, TEXTS[0], sample_rate=16000, **kw)
            cb.run_until_idle()
            got.append((r.frames, r.result().numpy()))
        route = cb.chain.table.route(16000, 1.25, 6.0, None, "5/4")
    finally:
        cb.close()
    (F, wa), (f0, w0), (f1, w1), (f2, w2) = got
    assert F == f0 == f1 == f2 and wa.shape == (F * 1280,) and w0.shape == w1.shape == w2.shape == (F * 1024,)
    sp, pp, lp = stretch.plan(1.25, 16000, 1280), plan("5/4", 16000, 1024), level.plan(16000, 1024)
    assert route.preroll == sp.preroll + pp.L + lp.LA and route.n_out == 1024 and route.drain_stage == "stretch"
    frames = F + route.drain_frames
    ts, ps = eng.new_stretcher(1, [sp]), eng.new_pitcher(1, [pp])
    try:
        s_raw = _raw(eng, ts, 1280, 1024, wa, frames, F)      # what the pitcher read
        p_raw = _raw(eng, ps, 1024, 1024, s_raw, frames, -1)  # what the leveler read
    finally:
        ts.close()
        ps.close()
    assert np.array_equal(s_raw[sp.preroll:sp.preroll + F * 1024].view(np.uint32), w0.view(np.uint32))
    lo = sp.preroll + pp.L
    assert np.array_equal(p_raw[lo:lo + F * 1024].view(np.uint32), w1.view(np.uint32))
    assert _against_the_reference(w1, s_raw, pp, "full chain, pitch 5/4 at (16000, 1024)", skip=sp.preroll) >= 0.9
    Gl, Cl = level.params(6.0)
    y, u, _, _ = level_ref.level(p_raw.astype(np.float64), Gl, Cl, lp.LA, lp.a, lp.k, full=True)
    assert lo + lp.LA + F * 1024 <= len(y)
    err = float(np.max(np.abs(w2.astype(np.float64) - y[lo + lp.LA:lo + lp.LA + F * 1024])))
    bound = (lp.LA + 64) * 2.0 ** -24 * float(np.max(np.abs(u)))
    print(f"full chain, level: max|y - y64| = {err:.3e} (bound {bound:.3e}), max|y| / C = {np.abs(w2).max() / float(Cl):.6f}")
    assert err <= bound
    assert np.abs(w2).max() <= float(Cl) * (1 + (lp.LA + 8) * 2.0 ** -24)


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
    """the launch list with what the tuner chooses per process taken out of the names"""
    import re

    return [(s, re.sub(r"<[^>]*>", "", k).split("@")[0] if k.startswith(("gemm", "attn")) else k) for s, k in rows]


def test_without_pitches_the_launches_are_those_of_the_parent_commit(model, eng, plans):
    """tests/golden/stretch_noop_launches.json holds what a build without output stages records for one eager FlowLM step and
    one codec frame: a batcher built without `pitches` records the same, and has no pitcher and no output ring; with a
    pitcher a codec frame has exactly one more launch, the last one, and without it again the launches of before"""
    from pocket_tts_amd.batching import ContinuousBatcher

    want = json.loads((G / "stretch_noop_launches.json").read_text())
    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    cb = ContinuousBatcher(model, slots=2, capacity=512)
    try:
        cb.submit(state, "ok")
        cb.run_until_idle()
        assert cb.chain.ps is None and cb.ps is None and cb.pipe.out is None and cb.pipe.pcm[0].is_pinned()
        got = _step_launches(eng, cb.st, cb.ms)
    finally:
        cb.close()
    assert len(got) == len(want["batcher"]) == 25
    assert [s for s, _ in got] == [s for s, _ in want["batcher"]]
    assert _untuned(got) == _untuned(map(tuple, want["batcher"]))
    fresh = eng.new_mimi_state(2)
    ps = eng.new_pitcher(2, plans)
    try:
        before = _step_launches(eng, None, fresh)
        out = torch.zeros(2, ps.width, device=eng.device)
        fresh.set_pitcher(ps, out)
        assert _step_launches(eng, None, fresh) == before + [("pitch", "pitch")]
        fresh.set_pitcher(None)
        assert _step_launches(eng, None, fresh) == before
    finally:
        ps.close()
        fresh.close()


def test_generate_audio_pitch(model, eng):
    from pocket_tts_amd.pitch import plan

    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    ref = model.generate_audio(state, TEXTS[0]).numpy()
    assert np.array_equal(model.generate_audio(state, TEXTS[0], pitch=1.0).numpy(), ref)
    p = plan("17/16")
    chunks = [c.numpy() for c in model.generate_audio_stream(state, TEXTS[0], pitch="17/16")]
    wav = np.concatenate(chunks)
    assert all(0 < c.shape[0] <= p.n for c in chunks) and wav.shape == ref.shape
    assert np.array_equal(wav.view(np.uint32), _twin(eng, p, ref).view(np.uint32))
    assert np.array_equal(model.generate_audio(state, TEXTS[0], pitch=1.0625).numpy(), wav)  # the cached context, restarted
    assert _against_the_reference(wav, ref, p, "generate_audio 17/16") >= 0.9
    with pytest.raises(ValueError, match="no multiple of 9"):
        model.generate_audio(state, TEXTS[0], pitch="8/9")
    with pytest.raises(ValueError, match="no multiple of 3"):
        model.generate_audio(state, TEXTS[0], pitch="2/3", sample_rate=8000)


def test_server_pitch(model, eng, tmp_path):
    import httpx

    from pocket_tts_amd.batching import ContinuousBatcher
    from pocket_tts_amd.pitch import plan
    from pocket_tts_amd.server import create_app

    shutil.copy(G / "e2e_voice.safetensors", tmp_path / "e2e_voice.safetensors")
    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    cb = ContinuousBatcher(model, slots=2, capacity=512)
    try:
        r = cb.submit(state, TEXTS[0])
        cb.run_until_idle()
        frames, wav_p = r.frames, r.result().numpy()
    finally:
        cb.close()
    app = create_app(model, slots=2, capacity=512, voices_dir=tmp_path, default_voice="e2e_voice", pitches=["17/16", "4/5"])

    async def go():
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t", timeout=600) as cl:
                # one after the other: each request has the batcher to itself, like the one it is compared with
                return [await cl.post("/tts", data=d) for d in ({"text": TEXTS[0], "pitch": "17/16"}, {"text": TEXTS[0]},
                                                                 {"text": TEXTS[0], "pitch": "5/4"},
                                                                 {"text": TEXTS[0], "pitch": "17/16", "frames_after_eos": "0"})]

    high, normal, bad, bad_fae = asyncio.run(go())
    assert bad.status_code == 400 and "not configured" in bad.json()["detail"] and "1.0625" in bad.json()["detail"]
    assert bad_fae.status_code == 400 and "frames_after_eos >= 1" in bad_fae.json()["detail"]
    for r in (high, normal):
        assert r.status_code == 200, r.text[:200]
        with wave.open(io.BytesIO(r.content), "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 24000)
        assert len(r.content) - 44 == frames * 1920 * 2 + 2 * 4800  # the WAV of the unpitched length
    assert np.array_equal(np.frombuffer(normal.content[44:], np.int16)[:frames * 1920], stretch_ref.pcm16(wav_p))
    assert np.array_equal(np.frombuffer(high.content[44:], np.int16)[:frames * 1920],
                          _twin(eng, plan("17/16"), wav_p, i16=True))
