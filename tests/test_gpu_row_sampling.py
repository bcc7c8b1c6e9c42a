"""Per-row sampling overrides of a FlowLM state (ptts_lm_state_set_row_sampling): the device generator's draws per row
(read back with debug_read(state, "noise")) against the numpy restatement in tests/noise_ref.py, and the per-row EOS
threshold of the head epilogue, eager and inside a captured step."""

import math
from pathlib import Path

import numpy as np
import pytest
import torch

from noise_ref import row_noise

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"


@pytest.fixture(scope="module")
def eng():
    from pocket_tts_amd import TTSModel

    m = TTSModel.load_model(config=G / "e2e_tiny.yaml", temp=0.0)
    yield m.engine
    m.engine.close()


def _state(eng, B, temp, seed, cap=32):
    st = eng.new_lm_state(B, cap)
    g = torch.Generator().manual_seed(1)
    eng.lm_prefill(st, torch.randn(B, 4, eng.D, generator=g) * 0.5)
    st.set_noise(temp, seed)
    return st


def _step(eng, st, thr=-4.0):
    _, logit, eos = eng.lm_decode_step(st, None, None, 1, thr)
    torch.cuda.synchronize()
    return eng.debug_read(st, "noise").cpu().numpy(), logit.cpu().numpy(), eos.cpu().numpy()


def _close(z, ref, temp):
    return np.abs(z.astype(np.float64) - ref).max() <= 1e-5 * math.sqrt(temp)


def test_rows_without_override_match_numpy_and_are_unchanged_by_set_clear(eng):
    B, T, seed = 5, 0.7, 3
    a, b = _state(eng, B, T, seed), _state(eng, B, T, seed)
    for r in (1, 3):
        b.set_row_sampling(r, 0.2, 0.5, -1.0)
        b.clear_row_sampling(r)
    for k in range(3):
        za, _, _ = _step(eng, a)
        zb, _, _ = _step(eng, b)
        assert np.array_equal(za.view(np.uint32), zb.view(np.uint32)), k
        for r in range(B):
            assert _close(za[r], row_noise(seed, k, r, eng.ldim, T), T), (k, r)
    a.close(); b.close()


def test_overridden_temperature_is_bitwise_set_noise(eng):
    B, seed = 4, 9
    a, b = _state(eng, B, 0.7, seed), _state(eng, B, 0.3, seed)
    a.set_row_sampling(2, 0.3, None, -4.0)
    for k in range(3):
        za, _, _ = _step(eng, a)
        zb, _, _ = _step(eng, b)
        assert np.array_equal(za[2].view(np.uint32), zb[2].view(np.uint32)), k
        assert not np.array_equal(za[1], zb[1])
        assert _close(za[1], row_noise(seed, k, 1, eng.ldim, 0.7), 0.7)
    a.close(); b.close()


def test_clamped_rows_are_truncated_normal(eng):
    from scipy import stats

    B, seed, steps = 4, 5, 200
    rows = {1: (0.7, 0.5), 3: (1.0, 1.5)}
    st = _state(eng, B, 0.7, seed, cap=4 + steps + 16)
    for r, (t, c) in rows.items():
        st.set_row_sampling(r, t, c, -4.0)
    pool = {r: [] for r in rows}
    for k in range(steps):
        z, _, _ = _step(eng, st)
        for r, (t, c) in rows.items():
            assert np.all(np.abs(z[r]) <= c), (k, r)
            assert _close(z[r], row_noise(seed, k, r, eng.ldim, t, c), t), (k, r)
            pool[r].append(z[r].astype(np.float64))
        assert _close(z[0], row_noise(seed, k, 0, eng.ldim, 0.7), 0.7)
    for r, (t, c) in rows.items():
        sd = math.sqrt(t)
        p = stats.kstest(np.concatenate(pool[r]), stats.truncnorm(-c / sd, c / sd, scale=sd).cdf).pvalue
        assert p > 1e-3, (r, p)
    st.close()


@pytest.mark.parametrize("clamp", [None, 1.0])
def test_temperature_zero_row_is_zero(eng, clamp):
    st = _state(eng, 4, 0.7, 2)
    st.set_row_sampling(2, 0.0, clamp, -4.0)
    for _ in range(2):
        z, _, _ = _step(eng, st)
        assert np.all(z[2] == 0) and np.all(np.abs(z[[0, 1, 3]]).max(axis=1) > 0)
    st.close()
    # a state whose own temperature is 0 still draws for a row overridden to temp > 0
    st = _state(eng, 3, 0.0, 4)
    st.set_row_sampling(1, 0.5, clamp, -4.0)
    z, _, _ = _step(eng, st)
    assert np.all(z[[0, 2]] == 0) and np.abs(z[1]).max() > 0
    assert _close(z[1], row_noise(4, 0, 1, eng.ldim, 0.5, clamp), 0.5)
    st.close()


def _check_eos(logit, eos, thr):
    assert np.array_equal(eos != 0, logit > thr), (logit, eos, thr)


def test_eos_threshold_per_row_eager_and_captured(eng):
    B = 6
    st = _state(eng, B, 0.0, 0, cap=64)
    step_thr = -1e9
    thr = np.full(B, step_thr)
    _, logit, _ = _step(eng, st, step_thr)
    for r, v in ((0, 1e9), (2, float(logit[2])), (4, float(logit[4]) - 1e-3)):
        st.set_row_sampling(r, 0.0, None, v)
        thr[r] = v
    for _ in range(3):
        _, logit, eos = _step(eng, st, step_thr)
        _check_eos(logit, eos, thr.astype(np.float32))
        assert eos[0] == 0 and eos[1] == 1
    # a captured step reads the overrides written after its capture
    dev = eng.device
    out_lat = torch.empty((B, eng.ldim), device=dev)
    out_logit = torch.empty((B,), device=dev)
    out_eos = torch.empty((B,), dtype=torch.uint8, device=dev)
    g = eng.capture_lm_step(st, None, 1, step_thr, out_lat, out_logit, out_eos)
    try:
        for it in range(3):
            thr = np.full(B, step_thr)
            for r in range(B):
                if (r + it) % 2:
                    v = 1e9 if r % 3 == 0 else -0.05 * r
                    st.set_row_sampling(r, 0.0, None, v)
                    thr[r] = v
                else:
                    st.clear_row_sampling(r)
            eng.graph_launch(g)
            torch.cuda.synchronize()
            _check_eos(out_logit.cpu().numpy(), out_eos.cpu().numpy(), thr.astype(np.float32))
            assert out_eos.cpu().numpy()[[r for r in range(B) if (r + it) % 2 and r % 3 == 0]].sum() == 0
    finally:
        eng.graph_destroy(g)
    st.close()


def test_reset_clears_overrides(eng):
    seed, T = 6, 0.7
    st = _state(eng, 3, T, seed)
    st.set_row_sampling(1, 0.0, None, 1e9)
    z, _, eos = _step(eng, st, -1e9)
    assert np.all(z[1] == 0) and eos[1] == 0 and eos[0] == 1
    st.reset()
    z, _, eos = _step(eng, st, -1e9)  # the step counter keeps running: second step of this state
    assert eos[1] == 1
    assert _close(z[1], row_noise(seed, 1, 1, eng.ldim, T), T)
    st.close()


def test_cabi_rejects_bad_rows_and_temperatures(eng):
    from pocket_tts_amd._lib import PttsError

    st = _state(eng, 2, 0.7, 0)
    for args in ((2, 0.5), (-1, 0.5), (0, -0.1), (0, float("nan")), (0, float("inf"))):
        with pytest.raises(PttsError):
            st.set_row_sampling(args[0], args[1], None, -4.0)
    for row in (2, -1):
        with pytest.raises(PttsError):
            st.clear_row_sampling(row)
    lib = eng.lib
    assert lib.ptts_lm_state_set_row_sampling(st.handle, 5, 0.5, 0.0, -4.0, None) < 0
    assert lib.ptts_lm_state_set_row_sampling(st.handle, 0, -1.0, 0.0, -4.0, None) < 0
    assert lib.ptts_lm_state_set_row_sampling(st.handle, 0, float("nan"), 0.0, -4.0, None) < 0
    assert lib.ptts_lm_state_set_row_sampling(st.handle, 1, 0.5, 1.0, -4.0, None) == 0
    st.close()
