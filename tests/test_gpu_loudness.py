"""Per-request loudness target on the GPU: the normaliser kernel against the fp64 reference (tests/loudness_ref.py) - the
measurement through the test tap, the error bound of the output, exactness and isolation, streaming state, captured graphs,
the whole output chain - and the path through the continuous batcher, `TTSModel.generate_audio_stream` and the HTTP server
(tiny model).

Largest |y - y64| observed on an MI355X, against the bound 16 * 2^-24 * max(k_j, k_{j+1}) * |x[i - D]|: see the "loudness
target" section of DESIGN.md."""

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

import loudness_ref

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"
SENTINEL_F = -77.0
GUARD = 4096
TEXT = "Hello world. This is a test."
F = 16  # frames of signal in both launches
SEED = 100  # chosen on the reference alone, so that no gating block lies within 0.01 LU of a gate
# (rate, n, target, amplitude of the loud part); None: bypass.  Row 3 is quiet enough to sit on the +20 dB clamp.
CASES = {"five": [None, (24000, 1920, -16.0, 0.25), (8000, 640, -23.0, 0.25), (24000, 960, -16.0, 0.01),
                  (11025, 882, -16.0, 0.25)],
         "two_per_frame": [(48000, 7680, -16.0, 0.25)]}
CLAMPED = {"five": 3}
EXTRA = {"five": 11, "two_per_frame": 4}  # drain frames: ceil(D / n) + 1 of the row that needs most


def _plans(case):
    from pocket_tts_amd.loudness import plan

    return [plan(r[0], r[1]) for r in CASES[case] if r is not None]


def _plan_index(case, b):
    return None if CASES[case][b] is None else sum(1 for r in CASES[case][:b] if r is not None)


def _signal(rate, n, amp, seed):
    """F frames: loud for 2 sub-blocks, 15 dB softer for 4, digital silence for 4, loud to the end"""
    S = rate // 10
    x = np.random.default_rng(seed).standard_normal(F * n)
    x = np.convolve(x, np.ones(3) / 3.0, mode="same") * amp
    g = np.ones(F * n)
    g[2 * S:6 * S] = 10.0 ** (-15.0 / 20.0)
    g[6 * S:10 * S] = 0.0
    return (x * g).astype(np.float32)


@pytest.fixture(scope="module")
def ref():
    """per case: the rows' input streams and, for each normalising row, the float64 reference fed frame by frame, F frames
    of signal and EXTRA[case] frames of zeros (the drain).  The conditions on the reference alone are asserted here, before
    anything runs on the GPU."""
    out = {}
    for case, rows in CASES.items():
        streams, refs = [], []
        for b, r in enumerate(rows):
            if r is None:
                streams.append(np.random.default_rng(100 + b).standard_normal(F * 1920).astype(np.float32))
                refs.append(None)
                continue
            rate, n, T, amp = r
            x = _signal(rate, n, amp, SEED + 10 * len(case) + b)
            s = loudness_ref.Stream(rate, T)
            y = [s.frame(x[f * n:(f + 1) * n]) for f in range(F)]
            marks = (len(s.c), dict(s.l), list(s.hist))  # the measurement at the end of the signal
            y += [s.frame(np.zeros(n, np.float32)) for _ in range(EXTRA[case])]
            streams.append(x)
            refs.append((s, np.concatenate(y), marks))
        out[case] = (streams, refs)
        abs_fail = rel_only = straddle = 0
        for b, r in enumerate(rows):
            if r is None:
                continue
            rate, n, T, amp = r
            s, _, (m_end, l, hist) = refs[b]
            S, D = s.S, s.D
            ls = [l[m] for m in sorted(l)]
            # the gates, drain frames included: no gating block within 0.01 LU of the absolute gate, or of the relative gate
            # of any L_m
            la = [s.l[m] for m in sorted(s.l)]
            assert all(abs(v + 70.0) > 0.01 for v in la if np.isfinite(v)), (case, b)
            for m in range(3, len(s.c)):
                A = [Z for Z in s.hist[:m - 2] if loudness_ref.lufs(Z) > -70.0]
                if A:
                    gamma = loudness_ref.lufs(sum(A) / len(A)) - 10.0
                    assert all(abs(v - gamma) > 0.01 for v in la[:m - 2] if np.isfinite(v)), (case, b, m)
            A = [Z for Z in hist if loudness_ref.lufs(Z) > -70.0]
            gamma = loudness_ref.lufs(sum(A) / len(A)) - 10.0
            abs_fail += sum(1 for v in ls if v <= -70.0)
            rel_only += sum(1 for v in ls if -70.0 < v <= gamma)
            c = np.array([float(v) for v in s.c[:m_end]])
            if b == CLAMPED.get(case):
                assert (c[3:] == 10.0).all() and m_end > 3, (case, b, c)  # on the +20 dB clamp from its first gain on
            else:
                assert (c < 10.0).all() and (c > 0.1).all(), (case, b, c)
                for j in range(m_end - 4):  # the ramp of delayed sub-block j: outputs [D + j S, D + (j + 1) S)
                    lo, hi = D + j * S, D + (j + 1) * S
                    if hi <= F * n and (lo // n) != ((hi - 1) // n) and lo % n != 0:
                        if abs(20.0 * np.log10(s.knot(j + 1) / s.knot(j))) >= 1.0:
                            straddle += 1
        assert abs_fail >= 1 and rel_only >= 1 and straddle >= 1, (case, abs_fail, rel_only, straddle)
    return out


def _lines(case, streams, order=None, frames=F):
    """[frames, B, width] input lines: row b's frame at the front of its line, NaN behind it (nothing may read it)"""
    rows = CASES[case]
    width = max(p.n for p in _plans(case))
    order = list(range(len(rows))) if order is None else order
    x = np.full((frames, len(order), width), np.nan, np.float32)
    for j, b in enumerate(order):
        n = width if rows[b] is None else rows[b][1]
        x[:, j, :n] = streams[b][:frames * n].reshape(frames, n) if rows[b] is not None else \
            streams[b].reshape(F, -1)[:frames, :n]
    return x


def _guarded(eng, shape, fill, dtype):
    """a contiguous device tensor of `shape` in the middle of a larger buffer filled with `fill`: (view, whole buffer)"""
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=eng.device)
    return big[GUARD:GUARD + n].view(*shape), big


def _run(eng, case, x, order=None, extra=0, events=None):
    """x [frames, B, width] through a fresh Normalizer whose row j runs row `order[j]` of the case, then every row set to
    drain and `extra` frames of NaN lines; `events` = {frame: [("set_row", j)]} applied before that frame.  The output and
    the guard bands around it are pre-filled with sentinels before every frame.  Returns (outs [frames][B, width], taps
    [frames][B, 4])."""
    plans, rows = _plans(case), CASES[case]
    order = list(range(len(rows))) if order is None else order
    B = len(order)
    ln = eng.new_normalizer(B, plans)
    try:
        for j, b in enumerate(order):
            ln.set_row(j, _plan_index(case, b), None if rows[b] is None else rows[b][2])
        outs, taps = [], []
        for f in range(x.shape[0] + extra):
            for kind, j in (events or {}).get(f, ()):
                assert kind == "set_row"
                ln.set_row(j, *ln.rows[j])
            if f == x.shape[0]:
                for j in range(B):
                    ln.set_row_drain(j, True)
            out, out_big = _guarded(eng, (B, ln.width), SENTINEL_F, torch.float32)
            tap, tap_big = _guarded(eng, (B, 4), -5.0, torch.float64)
            line = x[f] if f < x.shape[0] else np.full_like(x[0], np.nan)
            xin, _ = _guarded(eng, (B, ln.width), float("nan"), torch.float32)
            xin.copy_(torch.from_numpy(line))
            ln.frame(xin, out, tap)
            torch.cuda.synchronize()
            for big, fill in ((out_big, SENTINEL_F), (tap_big, -5.0)):
                g = big.cpu().numpy()
                assert (g[:GUARD] == fill).all() and (g[-GUARD:] == fill).all(), "a write outside the buffer"
            assert np.array_equal(xin.cpu().numpy().view(np.uint32), line.view(np.uint32)), "the input was written"
            outs.append(out.cpu().numpy())
            taps.append(tap.cpu().numpy())
        return outs, taps
    finally:
        ln.close()


def _stream_of(outs, j, n):
    return np.concatenate([o[j, :n] for o in outs])


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
def base(eng, ref):
    """the outputs and taps of both cases with their drain frames, computed once"""
    return {case: _run(eng, case, _lines(case, ref[case][0]), extra=EXTRA[case]) for case in CASES}


@pytest.mark.parametrize("case", list(CASES))
def test_against_the_reference(eng, ref, base, case):
    """the measurement (tap) after every frame, the output under the fp32 bound, the exact zeros of the pre-roll and after
    the drained tail, the bypass row, and nothing written past a row's n"""
    streams, refs = ref[case]
    outs, taps = base[case]
    worst = 0.0
    for b, r in enumerate(CASES[case]):
        if r is None:
            got = np.stack([o[b] for o in outs[:F]])
            assert np.array_equal(got.view(np.uint32), streams[b].reshape(F, -1).view(np.uint32))  # bypass: the whole line
            assert all((t[b] == -5.0).all() for t in taps)  # and no tap
            continue
        rate, n, T, amp = r
        s, y64, _ = refs[b]
        S, D = s.S, s.D
        for f, t in enumerate(taps):
            cnt = ((f + 1) * n) // S
            assert t[b, 0] == cnt, (b, f, t[b, 0], cnt)
            if cnt == 0:
                continue
            L, Z, c = s.L[cnt - 1], s.Z[cnt - 1], float(s.c[cnt - 1])
            if L is None:
                assert np.isnan(t[b, 1]), (b, f)
            else:
                assert abs(t[b, 1] - L) <= 1e-9, (b, f, t[b, 1], L)
            assert abs(t[b, 2] - c) <= 2.0 ** -23 * c, (b, f, t[b, 2], c)  # one fp32 ulp: pow of the device against the host's
            # Z is compared over the frames of signal, L and c over all.  In the drain frames the filters ring out for up to a
            # second, to 1e-90 of the signal's energy, where two float64 recurrences of different form no longer agree to
            # 1e-10 (the serial transposed form against the reference's direct form: 1.6e-11 already after 0.5 s); such
            # blocks lie below the absolute gate and do not enter L
            if Z is not None and f < F:
                assert abs(t[b, 3] - Z) <= 1e-10 * Z, (b, f, t[b, 3], Z)
        y = _stream_of(outs, b, n)
        assert y.shape == y64.shape and np.isfinite(y).all()
        assert not y[:D].any() and y[D:D + S].any()
        bound = s.bound(0, y.shape[0])
        err = np.abs(y.astype(np.float64) - y64)
        k = int(np.argmax(err - bound))
        assert (err <= bound).all(), (b, k, err[k], bound[k])
        k = int(np.argmax(np.where(bound > 0, err / np.maximum(bound, 1e-300), 0.0)))
        print(f"loudness {case} row {b}: largest |y - y64| = {err.max():.3g}; largest share of the bound {err[k] / bound[k]:.3f} "
              f"({err[k]:.3g} of {bound[k]:.3g})")
        worst = max(worst, float(err[k] / bound[k]))
        assert not y[F * n + D:].any() and y[F * n:F * n + D].any()  # the drained tail, then exact zeros
        for o in outs:
            assert (o[b, n:] == SENTINEL_F).all(), "a write past the row's n"
    print(f"loudness {case}: largest |y - y64| / bound = {worst:.3f}")


def test_a_row_is_bitwise_the_same_in_any_slot_and_any_batch(eng, ref, base):
    streams, _ = ref["five"]
    order = [4, 2, 0, 1, 3]
    outs, taps = _run(eng, "five", _lines("five", streams, order), order)
    for j, b in enumerate(order):
        for f in range(F):
            assert np.array_equal(outs[f][j].view(np.uint32), base["five"][0][f][b].view(np.uint32)), (b, f)
            assert np.array_equal(taps[f][j].view(np.uint64), base["five"][1][f][b].view(np.uint64)), (b, f)
    outs, _ = _run(eng, "five", _lines("five", streams, [1]), [1])
    for f in range(F):
        assert np.array_equal(outs[f][0].view(np.uint32), base["five"][0][f][1].view(np.uint32)), f


def test_set_row_restarts_a_row_from_zero_state(eng, ref, base):
    streams, _ = ref["five"]
    x = _lines("five", streams, frames=9)
    outs, taps = _run(eng, "five", np.concatenate([x[:7], x]), events={7: [("set_row", 1), ("set_row", 4)]})
    for b in (1, 4):
        for f in range(9):
            assert np.array_equal(outs[7 + f][b].view(np.uint32), base["five"][0][f][b].view(np.uint32)), (b, f)
            assert np.array_equal(taps[7 + f][b].view(np.uint64), base["five"][1][f][b].view(np.uint64)), (b, f)
    for f in range(7):  # the rows beside them are not touched
        for b in (0, 2, 3):
            assert np.array_equal(outs[f][b].view(np.uint32), base["five"][0][f][b].view(np.uint32)), (b, f)


def _twin_chain(eng, wav, target, peak_dbfs=None, rate=24000, n=1920, i16=False):
    """what a normaliser and a leveler of their own make of `wav` (whole frames of n samples) fed frame by frame, then the
    normaliser's row set to drain and the route's drain frames: the pre-roll dropped, frames * n samples"""
    from pocket_tts_amd import level, loudness

    frames = wav.shape[0] // n
    assert frames * n == wav.shape[0]
    pl, pv = loudness.plan(rate, n), level.plan(rate, n)
    preroll = pl.D + pv.LA
    ln, lv = eng.new_normalizer(1, [pl]), eng.new_leveler(1, [pv])
    try:
        ln.set_row(0, 0, target)
        lv.set_row(0, 0, 0.0, peak_dbfs)
        parts = []
        for f in range(frames + -(-preroll // n)):
            x = torch.full((1, n), float("nan"), device=eng.device)
            if f < frames:
                x[0] = torch.from_numpy(wav[f * n:(f + 1) * n])
            elif f == frames:
                ln.set_row_drain(0, True)
            mid = torch.zeros(1, n, device=eng.device)
            out = torch.zeros(1, n, dtype=torch.int16 if i16 else torch.float32, device=eng.device)
            ln.frame(x, mid)
            lv.frame(mid, out)
            torch.cuda.synchronize()
            parts.append(out.cpu().numpy()[0])
        return np.concatenate(parts)[preroll:preroll + frames * n]
    finally:
        lv.close()
        ln.close()


def test_captured_graph_follows_set_row_and_drain(eng):
    """a codec graph captured with a normaliser and a leveler: a later set_row (a new target) and set_row_drain change what
    its replays compute, exactly as they change stages of their own fed the same PCM frame by frame"""
    from pocket_tts_amd import level

    B = 5
    plans = _plans("five")
    lplans = [level.plan(p.rate, p.n) for p in plans]
    ms = eng.new_mimi_state(B)
    ln, twin = eng.new_normalizer(B, plans), eng.new_normalizer(B, plans)
    lv, lv2 = eng.new_leveler(B, lplans), eng.new_leveler(B, lplans)
    g = None
    try:
        lat = torch.randn(B, eng.ldim, device=eng.device, generator=torch.Generator(eng.device).manual_seed(3))
        pcm = torch.zeros(B, eng.frame_samples, device=eng.device)
        mid, mid2 = torch.full((B, ln.width), SENTINEL_F, device=eng.device), torch.full((B, ln.width), SENTINEL_F, device=eng.device)
        out, want = torch.full((B, lv.width), SENTINEL_F, device=eng.device), torch.full((B, lv.width), SENTINEL_F, device=eng.device)
        for s, v in ((ln, lv), (twin, lv2)):
            for b in (1, 2, 3):
                s.set_row(b, b - 1, -16.0)
                v.set_row(b, b - 1, 0.0)
        ms.set_loudnorm(ln, mid)
        ms.set_leveler(lv, out, mid)
        g = eng.capture_mimi(ms, lat, pcm)
        ms.set_leveler(None)
        ms.set_loudnorm(None)

        def step(tag):
            eng.graph_launch(g)
            eng.sync()
            twin.frame(pcm, mid2)
            lv2.frame(mid2, want)
            torch.cuda.synchronize()
            assert pcm.abs().max().item() > 0
            assert np.array_equal(mid.cpu().numpy().view(np.uint32), mid2.cpu().numpy().view(np.uint32)), tag
            assert np.array_equal(out.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32)), tag
            return mid.cpu().numpy().copy(), pcm.cpu().numpy().copy()

        for f in range(6):
            a, x = step(("plain", f))
        assert np.array_equal(a[0], x[0]) and np.array_equal(a[4], x[4])  # bypass rows
        assert a[2][:640].any() and (a[2][640:] == SENTINEL_F).all() and (a[3][960:] == SENTINEL_F).all()  # 8 kHz: D = 5 frames
        for s, v in ((ln, lv), (twin, lv2)):
            s.set_row(2, 1, -30.0)  # a new target: the row restarts
            s.set_row(0, 0, -16.0)  # a bypass row starts normalising
            v.set_row(0, 0, 0.0)
        b_, _ = step("set_row")
        assert not b_[2][:640].any() and not b_[0].any()  # both are in their pre-roll again
        for f in range(5):
            c, _ = step(("again", f))
        assert c[0].any() and c[2][:640].any()
        for s in (ln, twin):
            s.set_row_drain(0, True)
            s.set_row_drain(2, True)
        for f in range(6):
            d, _ = step(("drain", f))
        assert not d[0].any() and not d[2][:640].any() and d[1].any()
        # eager decodes on a state with the two stages append the same launches
        ms.set_loudnorm(ln, mid)
        ms.set_leveler(lv, out, mid)
        eng.mimi_decode(ms, lat, pcm)
        eng.sync()
        twin.frame(pcm, mid2)
        lv2.frame(mid2, want)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
        ms.set_leveler(None)
        ms.set_loudnorm(None)
    finally:
        if g is not None:
            eng.graph_destroy(g)
        for s in (lv, lv2, ln, twin):
            s.close()
        ms.close()


def test_the_chain_in_one_graph_equals_its_stages_one_by_one(eng):
    """codec -> resampler (8 kHz) -> stretcher (1.25) -> normaliser -> leveler in one captured graph, against stages of
    their own run one by one on the recorded intermediate buffers: bitwise"""
    from pocket_tts_amd import level, loudness, stretch

    B = 2
    ms = eng.new_mimi_state(B)
    rates = [(24000, 1920), (8000, 640)]
    ts_plans, index = stretch.table(rates, [1.0, 1.25])
    lines = [(rates[r][0], ts_plans[i].n_out) for r, row in enumerate(index) for i in row if i is not None]
    ln_plans, ln_index = loudness.table(lines)
    lv_plans, lv_index = level.table(lines)
    made = [(eng.new_resampler(B, [8000]), eng.new_stretcher(B, ts_plans), eng.new_normalizer(B, ln_plans),
             eng.new_leveler(B, lv_plans)) for _ in range(2)]
    (rs, ts, ln, lv), (rs2, ts2, ln2, lv2) = made
    g = None
    try:
        r8, p8 = rs.index_of(8000), index[1][1]
        n8 = ts_plans[p8].n_out
        assert ts_plans[p8].n_in == 640 and n8 == 512
        for a, b, c, d in made:
            a.set_row(0, r8)
            b.set_row(0, p8)
            c.set_row(0, ln_index[(8000, n8)], -16.0)
            d.set_row(0, lv_index[(8000, n8)], 0.0, -6.0)
            c.set_row(1, ln_index[(24000, 1920)], -23.0)  # row 1: native rate, speed 1.0, normalised
            d.set_row(1, lv_index[(24000, 1920)], 0.0)
        lat = torch.randn(B, eng.ldim, device=eng.device, generator=torch.Generator(eng.device).manual_seed(4))
        pcm = torch.zeros(B, eng.frame_samples, device=eng.device)
        mid1 = torch.zeros(B, rs.out_max, device=eng.device)
        mid2 = torch.zeros(B, ts.out_max, device=eng.device)
        mid3 = torch.full((B, ln.width), SENTINEL_F, device=eng.device)
        out = torch.full((B, lv.width), SENTINEL_F, device=eng.device)
        w1, w2, w3, w4 = torch.zeros_like(mid1), torch.zeros_like(mid2), torch.full_like(mid3, SENTINEL_F), torch.full_like(out, SENTINEL_F)
        ms.set_resampler(rs, mid1)
        ms.set_stretcher(ts, mid2, mid1)
        ms.set_loudnorm(ln, mid3, mid2)
        ms.set_leveler(lv, out, mid3)
        g = eng.capture_mimi(ms, lat, pcm)
        ms.set_leveler(None)
        ms.set_loudnorm(None)
        ms.set_stretcher(None)
        ms.set_resampler(None)
        u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
        for f in range(9):  # 8 kHz, 512 per frame: D = 3200 is over after 7 frames
            eng.graph_launch(g)
            eng.sync()
            rs2.frame(pcm, w1)
            torch.cuda.synchronize()
            assert np.array_equal(u32(w1)[0, :640], u32(mid1)[0, :640]), f
            ts2.frame(mid1, w2)
            torch.cuda.synchronize()
            assert np.array_equal(u32(w2)[0, :n8], u32(mid2)[0, :n8]), f
            ln2.frame(mid2, w3)
            torch.cuda.synchronize()
            assert np.array_equal(u32(w3), u32(mid3)), f
            lv2.frame(mid3, w4)
            torch.cuda.synchronize()
            assert np.array_equal(u32(w4), u32(out)), f
            o = out.cpu().numpy()
            assert (o[0, n8:] == SENTINEL_F).all() and np.isfinite(o[0, :n8]).all() and np.isfinite(o[1]).all()
        assert o[0, :n8].any() and o[1].any()
    finally:
        if g is not None:
            eng.graph_destroy(g)
        for stages in made:
            for s in reversed(stages):
                s.close()
        ms.close()


def test_cabi_error_codes(eng):
    import ctypes as C

    from pocket_tts_amd import loudness

    plans = _plans("five")
    ln = eng.new_normalizer(2, plans)
    try:
        lib, sp = eng.lib, eng._sp
        for row, idx in ((-1, 0), (2, 0), (0, -2), (0, 4), (0, 1 << 20)):
            assert lib.ptts_loudnorm_set_row(ln.handle, row, idx, -16.0, sp) == -1, (row, idx)
            assert b"out of range" in lib.ptts_last_error()
        for t in (-40.5, -9.0, float("nan"), float("inf")):
            assert lib.ptts_loudnorm_set_row(ln.handle, 0, 0, t, sp) == -1 and b"[-40, -10]" in lib.ptts_last_error(), t
        assert lib.ptts_loudnorm_set_row_drain(ln.handle, 2, 1, sp) == -1 and lib.ptts_loudnorm_set_row_drain(None, 0, 1, sp) == -1
        with pytest.raises(ValueError, match="loudness_lufs"):
            ln.set_row(0, 0, -5.0)
        assert ln.rows == [(-1, None)] * 2
        x = torch.zeros(2, ln.width, device=eng.device)
        out = torch.zeros(2, ln.width, device=eng.device)
        px, po = C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr())
        assert lib.ptts_loudnorm_frame(ln.handle, None, po, None, sp) == -1
        assert lib.ptts_loudnorm_frame(ln.handle, px, None, None, sp) == -1
        assert lib.ptts_loudnorm_frame(None, px, po, None, sp) == -1
        assert lib.ptts_loudnorm_frame(ln.handle, px, px, None, sp) == -1 and b"in place" in lib.ptts_last_error()
        h = C.c_void_p()
        d = np.ascontiguousarray(plans[0].doubles())
        pd = d.ctypes.data_as(C.POINTER(C.c_double))
        for rate, n in ((7999, 640), (48001, 1920), (24000, 0), (24000, 8193)):  # a plan that breaks a rule never reaches the device
            arr = (C.c_int32 * 2)(rate, n)
            assert lib.ptts_loudnorm_create(eng.handle, 2, arr, 1, pd, d.size, C.byref(h)) == -1
            assert b"not admissible" in lib.ptts_last_error()
        arr = (C.c_int32 * 2)(24000, 1920)
        assert lib.ptts_loudnorm_create(eng.handle, 2, arr, 1, pd, d.size - 1, C.byref(h)) == -1
        bad = d.copy()
        bad[20] = np.nan
        assert lib.ptts_loudnorm_create(eng.handle, 2, arr, 1, bad.ctypes.data_as(C.POINTER(C.c_double)), d.size, C.byref(h)) == -1
        assert b"not finite" in lib.ptts_last_error()
        assert loudness.DOUBLES_PER_PLAN == d.size
        ms = eng.new_mimi_state(3)
        assert lib.ptts_mimi_set_loudnorm(ms.handle, ln.handle, None, po) == -1  # batch 3 vs 2
        ms.close()
        ms = eng.new_mimi_state(2)
        # an input buffer means "behind an earlier stage": refused on a state that has none
        assert lib.ptts_mimi_set_loudnorm(ms.handle, ln.handle, px, po) == -1
        # a frame with a normaliser but no leveler fails, and nothing of the normaliser is enqueued before the check
        lat = torch.zeros(2, eng.ldim, device=eng.device)
        pcm = torch.zeros(2, eng.frame_samples, device=eng.device)
        assert lib.ptts_mimi_set_loudnorm(ms.handle, ln.handle, None, po) == 0
        assert lib.ptts_mimi_decode(eng.handle, ms.handle, C.c_void_p(lat.data_ptr()), C.c_void_p(pcm.data_ptr()), sp) == -1
        assert b"followed by a leveler" in lib.ptts_last_error()
        assert lib.ptts_mimi_set_loudnorm(ms.handle, None, None, None) == 0
        # the leveler accepts an input buffer on a state whose only earlier stage is the normaliser
        from pocket_tts_amd import level

        lv = eng.new_leveler(2, [level.plan(p.rate, p.n) for p in plans])
        out2 = torch.zeros(2, lv.width, device=eng.device)
        assert lib.ptts_mimi_set_loudnorm(ms.handle, ln.handle, None, po) == 0
        assert lib.ptts_mimi_set_leveler(ms.handle, lv.handle, po, C.c_void_p(out2.data_ptr()), 0) == 0
        assert lib.ptts_mimi_set_leveler(ms.handle, None, None, None, 0) == 0
        assert lib.ptts_mimi_set_loudnorm(ms.handle, None, None, None) == 0
        eng.sync()
        lv.close()
        ms.close()
    finally:
        ln.close()


# ---- through the batcher, the model and the server -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def alone(model):
    """(frames, waveform) of TEXT as the only request of a fresh batcher without an output chain (2 slots).  The bitwise
    comparisons below are between requests that ran this way - alone, in slot 0, prefilled on their own."""
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
    cb = ContinuousBatcher(model, slots=2, capacity=512, loudness=True)
    try:
        with pytest.raises(ValueError, match=r"\[-40, -10\]"):
            cb.submit(state, TEXT, loudness_lufs=-5)
        with pytest.raises(ValueError, match="exclude each other"):
            cb.submit(state, TEXT, loudness_lufs=-16, gain_db=3)
        with pytest.raises(ValueError, match="frames_after_eos >= 1"):
            cb.submit(state, TEXT, frames_after_eos=0, loudness_lufs=-16)
        r = cb.submit(state, TEXT, loudness_lufs=-16)
        cb.run_until_idle()
        wav = r.result().numpy()
        assert r.frames == frames and wav.shape[0] == frames * 1920
        assert np.array_equal(wav.view(np.uint32), _twin_chain(eng, wav_p, -16).view(np.uint32))
        assert np.abs(wav).max() <= 10 ** -0.05 * (1 + 128 * 2.0 ** -24) and wav.any()
        # then, in the slot the normalised request has drained and left: a request without a target is bit-identical
        r = cb.submit(state, TEXT)
        cb.run_until_idle()
        assert np.array_equal(r.result().numpy().view(np.uint32), wav_p.view(np.uint32))
    finally:
        cb.close()
    cb = ContinuousBatcher(model, slots=2, capacity=512)
    try:
        with pytest.raises(ValueError, match="no loudness stage"):
            cb.submit(state, TEXT, loudness_lufs=-16)
    finally:
        cb.close()


def test_generate_audio_stream_loudness(model, eng):
    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    wav_p = np.concatenate([c.numpy() for c in model.generate_audio_stream(state, TEXT)])
    chunks = [c.numpy() for c in model.generate_audio_stream(state, TEXT, loudness_lufs=-16)]
    wav = np.concatenate(chunks)
    assert wav.shape[0] == wav_p.shape[0] and all(0 < c.shape[0] <= 1920 for c in chunks)
    assert np.array_equal(wav.view(np.uint32), _twin_chain(eng, wav_p, -16).view(np.uint32))
    # the cached context, restarted, with another target and ceiling
    wav2 = model.generate_audio(state, TEXT, loudness_lufs=-23, peak_dbfs=-20).numpy()
    assert np.array_equal(wav2.view(np.uint32), _twin_chain(eng, wav_p, -23, -20).view(np.uint32))
    assert np.abs(wav2).max() <= 0.1 * (1 + 128 * 2.0 ** -24)
    with pytest.raises(ValueError, match="exclude each other"):
        model.generate_audio(state, TEXT, loudness_lufs=-16, gain_db=3)
    with pytest.raises(ValueError, match=r"\[-40, -10\]"):
        model.generate_audio(state, TEXT, loudness_lufs=0)


def test_server_loudness(model, eng, alone, tmp_path):
    import httpx

    from pocket_tts_amd.server import create_app

    shutil.copy(G / "e2e_voice.safetensors", tmp_path / "e2e_voice.safetensors")
    frames, wav_p = alone
    app = create_app(model, slots=2, capacity=512, voices_dir=tmp_path, default_voice="e2e_voice", loudness=True)

    async def go():
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t", timeout=600) as cl:
                # one after the other: each request has the batcher to itself, like the one it is compared with
                return [await cl.post("/tts", data=d) for d in ({"text": TEXT, "loudness_lufs": "-16"},
                                                                 {"text": TEXT, "loudness_lufs": "-16", "gain_db": "3"},
                                                                 {"text": TEXT, "loudness_lufs": "-3"},
                                                                 {"text": TEXT, "loudness_lufs": "-16", "frames_after_eos": "0"})]

    ok, both, bad, bad_fae = asyncio.run(go())
    assert both.status_code == 400 and "exclude each other" in both.json()["detail"]
    assert bad.status_code == 400 and "[-40, -10]" in bad.json()["detail"]
    assert bad_fae.status_code == 400 and "frames_after_eos >= 1" in bad_fae.json()["detail"]
    assert ok.status_code == 200, ok.text[:200]
    with wave.open(io.BytesIO(ok.content), "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 24000)
    assert len(ok.content) - 44 == frames * 1920 * 2 + 2 * 4800
    assert np.array_equal(np.frombuffer(ok.content[44:], np.int16)[:frames * 1920], _twin_chain(eng, wav_p, -16, i16=True))


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


def test_without_loudness_the_launches_are_those_of_the_parent_commit(model, eng):
    """tests/golden/stretch_noop_launches.json holds what the commit before the output chain records for one eager FlowLM
    step and one codec frame, on the batcher's states and on the `TTSModel` context: built without `loudness`, both still
    record the same launches at the same sites in the same order, with the same kernel names wherever the tuner has no say"""
    from pocket_tts_amd.batching import ContinuousBatcher

    want = json.loads((G / "stretch_noop_launches.json").read_text())
    state = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    cb = ContinuousBatcher(model, slots=2, capacity=512)
    try:
        cb.submit(state, "ok")
        cb.run_until_idle()
        assert cb.ln is None and cb.lv is None and not cb.lagging and cb.pipe.out is None and cb.pipe.pcm[0].is_pinned()
        got = _step_launches(eng, cb.st, cb.ms)
    finally:
        cb.close()
    assert len(got) == len(want["batcher"]) == 25
    assert [s for s, _ in got] == [s for s, _ in want["batcher"]]
    assert _untuned(got) == _untuned(map(tuple, want["batcher"]))
    model.generate_audio(state, "ok")
    ctxs = [c for k, c in model._ctx_cache.items() if not {"speed", "rate", "level", "pitch", "loud"} & set(k[4:])]
    assert ctxs and all(c["pipe"].ln is None and c["pipe"].lv is None and c["pipe"].out is None for c in ctxs)
    for c in ctxs:
        got = _step_launches(eng, c["st"], c["ms"])
        assert len(got) == len(want["model"]) == 25
        assert [s for s, _ in got] == [s for s, _ in want["model"]]
        assert _untuned(got) == _untuned(map(tuple, want["model"]))


def test_a_normaliser_set_and_cleared_leaves_the_launches_of_before(eng):
    from pocket_tts_amd import level

    fresh, used = eng.new_mimi_state(2), eng.new_mimi_state(2)
    plans = _plans("five")
    ln = eng.new_normalizer(2, plans)
    lv = eng.new_leveler(2, [level.plan(p.rate, p.n) for p in plans])
    try:
        want = _step_launches(eng, None, fresh)
        assert want and not any("loud" in s or "loud" in k for s, k in want)
        mid = torch.zeros(2, ln.width, device=eng.device)
        out = torch.zeros(2, lv.width, device=eng.device)
        used.set_loudnorm(ln, mid)
        used.set_leveler(lv, out, mid)
        assert _step_launches(eng, None, used) == want + [("loudnorm", "loudnorm"), ("level", "level")]
        used.set_leveler(None)
        used.set_loudnorm(None)
        assert _step_launches(eng, None, used) == want
    finally:
        lv.close()
        ln.close()
        fresh.close()
        used.close()
