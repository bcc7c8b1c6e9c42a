"""Per-request seeds on the GPU.  Engine level: a seeded row of a FlowLM state (ptts_lm_state_set_row_seed) draws
`noise_ref.row_noise(seed, j, 0, ...)` at its j-th step, bit for bit the same in any row of any state, and rows without a
seed draw what they drew before.  Public API at temp 0.7: the same (text, seed) through `generate_audio`,
`generate_audio_batch`, `ContinuousBatcher.submit` and `POST /tts` gives the same frames and, within the project's
batch-vs-single bound, the same waveform; the numpy oracle fed with the restated noise takes the same EOS decisions."""

import asyncio
import math
import shutil
from pathlib import Path

import numpy as np
import pytest
import torch

from noise_ref import row_noise
from seed_ref import CASES, EOS_MARGIN, EOS_THRESHOLD, TEMP, oracle_seeded

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"
WAV_TOL = 5e-4   # batch-vs-single and temp-0.7 fixture bound of test_gpu_e2e.py
LAT_ATOL = 2e-4  # ATOL of test_gpu_parity.py
FILLERS = ["Yes.", "This is a longer sentence, with several clauses, to test it.", "one two three four five six",
           "Hello world."]


@pytest.fixture(scope="module")
def model():
    from pocket_tts_amd import TTSModel

    m = TTSModel.load_model(config=G / "e2e_tiny.yaml", temp=0.0)
    yield m
    m.engine.close()


@pytest.fixture(scope="module")
def eng(model):
    return model.engine


@pytest.fixture()
def warm(model):
    """the model at TEMP for one test"""
    model.temp = TEMP
    yield model
    model.temp = 0.0


def _state(eng, B, temp, seed, cap=48):
    st = eng.new_lm_state(B, cap)
    g = torch.Generator().manual_seed(1)
    eng.lm_prefill(st, torch.randn(B, 4, eng.D, generator=g) * 0.5)
    st.set_noise(temp, seed)
    return st


def _step(eng, st, thr=-4.0):
    eng.lm_decode_step(st, None, None, 1, thr)
    torch.cuda.synchronize()
    return eng.debug_read(st, "noise").cpu().numpy()


def _bits(z):
    return np.ascontiguousarray(z).view(np.uint32)


def _close(z, ref, temp):
    return np.abs(z.astype(np.float64) - ref).max() <= 1e-5 * math.sqrt(temp)


# ---- engine level ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_temp,clamp", [(None, None), (0.3, None), (0.3, 0.4), (0.7, 1.0)])
def test_seeded_row_matches_numpy(eng, row_temp, clamp):
    B, T, state_seed, S = 5, 0.7, 3, 11
    st = _state(eng, B, T, state_seed)
    if row_temp is not None:
        st.set_row_sampling(2, row_temp, clamp, -4.0)
    st.set_row_seed(2, S)
    t = T if row_temp is None else row_temp
    for j in range(4):
        z = _step(eng, st)
        assert _close(z[2], row_noise(S, j, 0, eng.ldim, t, clamp), t), j
        if clamp:
            assert np.all(np.abs(z[2]) <= clamp)
        for r in (0, 1, 3, 4):  # the others: the state's seed, the state's counter, their row index
            assert _close(z[r], row_noise(state_seed, j, r, eng.ldim, T), T), (j, r)
    assert not st.error()
    st.close()


def test_placement_independence_is_bitwise(eng):
    S, n = 2 ** 62 + 5, 12
    one = _state(eng, 1, 0.7, 100)
    one.set_row_seed(0, S)
    want = [_bits(_step(eng, one)[0]).copy() for _ in range(n)]
    one.close()
    assert len({w.tobytes() for w in want}) == n
    six = _state(eng, 6, 0.7, 200)
    six.set_row_seed(4, S)
    six.set_row_seed(1, S)
    for j in range(5):
        z = _step(eng, six)
        assert np.array_equal(_bits(z[4]), want[j]) and np.array_equal(_bits(z[1]), want[j]), j
    six.set_row_seed(2, S)  # joins 5 steps later: its step j is the others' step j
    for j in range(5):
        z = _step(eng, six)
        assert np.array_equal(_bits(z[2]), want[j]), j
        assert np.array_equal(_bits(z[4]), want[5 + j]) and np.array_equal(_bits(z[1]), want[5 + j]), j
    six.set_row_seed(4, S)  # re-seeding restarts the stream
    z = _step(eng, six)
    assert np.array_equal(_bits(z[4]), want[0]) and np.array_equal(_bits(z[2]), want[5]) and np.array_equal(_bits(z[1]), want[10])
    # another temperature scales the same stream
    six.set_row_sampling(4, 0.3, None, -4.0)
    z = _step(eng, six)
    assert _close(z[4], row_noise(S, 1, 0, eng.ldim, 0.3), 0.3)
    assert not six.error()
    six.close()


def test_unseeded_rows_and_cleared_rows_draw_what_they_drew(eng):
    B, T, seed = 5, 0.7, 9
    a, b = _state(eng, B, T, seed), _state(eng, B, T, seed)
    b.set_row_seed(1, 77)
    b.set_row_seed(3, 78)
    b.set_row_seed(2, 79)
    b.clear_row_seed(2)  # set-then-clear: as if never seeded
    for j in range(3):
        za, zb = _step(eng, a), _step(eng, b)
        assert np.array_equal(_bits(za[[0, 2, 4]]), _bits(zb[[0, 2, 4]])), j
        assert not np.array_equal(za[1], zb[1]) and not np.array_equal(za[3], zb[3])
    b.clear_row_seed(1)  # a cleared row is back on the state's stream at the state's counter
    za, zb = _step(eng, a), _step(eng, b)
    assert np.array_equal(_bits(za[[0, 1, 2, 4]]), _bits(zb[[0, 1, 2, 4]]))
    a.reset(); b.reset()  # reset clears every seed; the state's counter keeps running
    za, zb = _step(eng, a), _step(eng, b)
    assert np.array_equal(_bits(za), _bits(zb))
    assert _close(zb[3], row_noise(seed, 4, 3, eng.ldim, T), T)
    a.close(); b.close()


def test_temperature_zero_seeded_rows_are_zero(eng):
    st = _state(eng, 3, 0.7, 2)
    st.set_row_seed(1, 5)
    st.set_row_sampling(1, 0.0, None, -4.0)
    z = _step(eng, st)
    assert np.all(z[1] == 0) and np.abs(z[0]).max() > 0
    st.close()
    st = _state(eng, 3, 0.0, 2)  # a state at temperature 0: a seed alone draws nothing, an override to temp > 0 does
    st.set_row_seed(1, 5)
    st.set_row_seed(2, 5)
    st.set_row_sampling(2, 0.5, None, -4.0)
    z = _step(eng, st)
    assert np.all(z[[0, 1]] == 0) and _close(z[2], row_noise(5, 0, 0, eng.ldim, 0.5), 0.5)
    st.close()


def test_captured_step_reads_seeds_written_after_capture(eng):
    B, T, state_seed = 4, 0.7, 21
    st = _state(eng, B, T, state_seed, cap=64)
    dev = eng.device
    outs = (torch.empty((B, eng.ldim), device=dev), torch.empty((B,), device=dev),
            torch.empty((B,), dtype=torch.uint8, device=dev))
    g = eng.capture_lm_step(st, None, 1, -4.0, *outs)
    try:
        def launch():
            eng.graph_launch(g)
            torch.cuda.synchronize()
            return eng.debug_read(st, "noise").cpu().numpy()

        z = launch()
        for r in range(B):
            assert _close(z[r], row_noise(state_seed, 0, r, eng.ldim, T), T)
        st.set_row_seed(1, 31)
        st.set_row_seed(3, 32)
        for j in range(3):
            z = launch()
            assert _close(z[1], row_noise(31, j, 0, eng.ldim, T), T) and _close(z[3], row_noise(32, j, 0, eng.ldim, T), T), j
            assert _close(z[0], row_noise(state_seed, 1 + j, 0, eng.ldim, T), T), j  # the state's counter ran on
        st.clear_row_seed(1)
        st.set_row_seed(3, 31)
        z = launch()
        assert _close(z[1], row_noise(state_seed, 4, 1, eng.ldim, T), T) and _close(z[3], row_noise(31, 0, 0, eng.ldim, T), T)
        assert not st.error()  # the cooperative kernels' hand-off epoch (the state's counter) was not disturbed
    finally:
        eng.graph_destroy(g)
    st.close()


def test_parked_rows_do_not_consume_their_stream(eng):
    """the row-local counter advances for active rows only, as the row's position does"""
    st = _state(eng, 3, 0.7, 1)
    st.set_row_seed(1, 41)
    st.set_row_active(1, False)
    _step(eng, st)
    _step(eng, st)
    st.set_row_active(1, True)
    z = _step(eng, st)
    assert _close(z[1], row_noise(41, 0, 0, eng.ldim, 0.7), 0.7)
    z = _step(eng, st)
    assert _close(z[1], row_noise(41, 1, 0, eng.ldim, 0.7), 0.7)
    st.close()


def test_copy_row_from_leaves_the_seed_alone(eng):
    src = _state(eng, 1, 0.7, 1)
    dst = _state(eng, 3, 0.7, 2)
    dst.set_row_seed(1, 51)
    _step(eng, dst)
    dst.copy_row_from(1, src, 0)
    z = _step(eng, dst)
    assert _close(z[1], row_noise(51, 1, 0, eng.ldim, 0.7), 0.7)
    src.close(); dst.close()


def test_cabi_rejects_bad_rows_and_seeds(eng):
    from pocket_tts_amd._lib import PttsError

    st = _state(eng, 2, 0.7, 0)
    for row in (2, -1):
        with pytest.raises(PttsError):
            st.set_row_seed(row, 1)
        with pytest.raises(PttsError):
            st.clear_row_seed(row)
    for bad in (-1, 1.5, True, 2 ** 64):
        with pytest.raises(ValueError):
            st.set_row_seed(0, bad)
    lib = eng.lib
    assert lib.ptts_lm_state_set_row_seed(st.handle, 5, 1, None) < 0
    assert lib.ptts_lm_state_clear_row_seed(st.handle, -1, None) < 0
    assert lib.ptts_lm_state_set_row_seed(st.handle, 1, 2 ** 64 - 1, None) == 0
    assert lib.ptts_lm_state_clear_row_seed(st.handle, 1, None) == 0
    assert lib.ptts_abi_version() == 1
    st.close()


# ---- public API -----------------------------------------------------------------------------------------------------
def _voice(model):
    return model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")


def _maxdiff(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def test_generate_audio_repeats_with_a_seed_and_keeps_the_unseeded_path(warm):
    model, state = warm, _voice(warm)
    text = CASES[0][0]
    a = model.generate_audio(state, text, seed=7)
    torch.manual_seed(123)  # a seeded call reads nothing from torch's generator
    b = model.generate_audio(state, text, seed=7)
    assert a.shape == b.shape and torch.equal(a, b)
    c = model.generate_audio(state, text, seed=8)
    assert c.shape != a.shape or not torch.equal(a, c)
    chunks = list(model.generate_audio_stream(state, text, seed=7))
    assert all(ch.shape == (1920,) for ch in chunks) and torch.equal(torch.cat(chunks), a)
    # today's behaviour kept: the unseeded call draws from torch's global generator
    torch.manual_seed(5)
    u1 = model.generate_audio(state, text)
    mid = model.generate_audio(state, text, seed=7)  # leaves the generator where it was
    u2 = model.generate_audio(state, text)
    torch.manual_seed(5)
    v1 = model.generate_audio(state, text)
    v2 = model.generate_audio(state, text)
    assert torch.equal(u1, v1) and torch.equal(u2, v2) and torch.equal(mid, a)
    assert u1.shape != a.shape or not torch.equal(u1, a)
    for bad in (-1, 1.5, True, 2 ** 63):
        with pytest.raises(ValueError):
            model.generate_audio(state, text, seed=bad)
    with pytest.raises(ValueError):
        model.generate_audio_batch(state, [text], seeds=[1, 2])


def test_same_request_through_every_entry_point(warm):
    """`generate_audio(seed=)` is the reference; the batch call and the batcher (two submissions under different traffic,
    landing in different slots) must give the same frame count and a waveform within WAV_TOL, also against each other"""
    from pocket_tts_amd.batching import ContinuousBatcher

    model, state = warm, _voice(warm)
    refs = [model.generate_audio(state, t, max_tokens=mt, seed=s) for t, s, mt in CASES]
    assert len({r.shape[0] for r in refs}) > 1
    worst = {}

    def check(name, got, want, case):
        assert got.shape == want.shape, (name, case, got.shape, want.shape)
        d = _maxdiff(got.numpy(), want.numpy())
        worst[name] = max(worst.get(name, 0.0), d)
        return d

    # one batch call: the single-chunk cases between other texts, seeded differently or not at all
    single = [i for i, c in enumerate(CASES) if c[2] == 50]
    texts, seeds, where = [], [], {}
    for k, i in enumerate(single):
        texts += [FILLERS[k % len(FILLERS)], CASES[i][0]]
        seeds += [None if k % 2 else 1000 + k, CASES[i][1]]
        where[i] = len(texts) - 1
    outs = model.generate_audio_batch(state, texts, seeds=seeds)
    diffs = [check("batch", outs[where[i]], refs[i], CASES[i]) for i in single]

    # the batcher, twice, with different traffic around the requests
    placed = {}
    cb = ContinuousBatcher(model, slots=3, capacity=512, noise_seed=5)
    admit = cb._admit_group

    def record(jobs, rows):
        for j, b in zip(jobs, rows):
            placed.setdefault(j.req.id, []).append(b)
        return admit(jobs, rows)

    cb._admit_group = record
    try:
        first = [cb.submit(state, t, max_tokens=mt, seed=s) for t, s, mt in CASES[:3]]
        for _ in range(4):
            cb.step()
        other = [cb.submit(state, FILLERS[0]), cb.submit(state, FILLERS[1], seed=4242, temperature=0.3)]
        first += [cb.submit(state, t, max_tokens=mt, seed=s) for t, s, mt in CASES[3:]]
        cb.run_until_idle()
        outs_a = [r.result() for r in first]
        [r.result() for r in other]
        other = [cb.submit(state, FILLERS[2], temperature=1.0, noise_clamp=0.5), cb.submit(state, FILLERS[3], seed=CASES[0][1])]
        for _ in range(3):
            cb.step()
        second = [cb.submit(state, t, max_tokens=mt, seed=s) for t, s, mt in reversed(CASES)][::-1]
        cb.step()
        other.append(cb.submit(state, FILLERS[1]))
        cb.run_until_idle()
        outs_b = [r.result() for r in second]
        [r.result() for r in other]
    finally:
        cb.close()
    for i, case in enumerate(CASES):
        diffs.append(check("batcher", outs_a[i], refs[i], case))
        diffs.append(check("batcher", outs_b[i], refs[i], case))
        diffs.append(check("batcher-vs-batcher", outs_a[i], outs_b[i], case))
    moved = [i for i in range(len(CASES)) if placed[first[i].id] != placed[second[i].id]]
    print(f"seed consistency: largest waveform differences {worst}; slots of the first / second submission "
          f"{[(placed[a.id], placed[b.id]) for a, b in zip(first, second)]}")
    assert moved, "no request changed its slot between the two submissions"
    assert max(diffs) < WAV_TOL, worst


def test_seeded_generation_matches_the_oracle(warm):
    """the numpy oracle's loop with noise[j] = row_noise(chunk seed, j, 0, ...) on the same prefilled state: same EOS step
    and frame count as the seeded device run, first 8 latents within LAT_ATOL; the EOS margin holds for every case"""
    from pocket_tts_amd.engine import chunk_seed

    model, eng, state = warm, warm.engine, _voice(warm)
    voice = model._voice_acquire(state)
    try:
        for text, seed, mt in CASES:
            chunks = oracle_seeded(text, seed, mt)
            frames = 0
            for i, c in enumerate(chunks):
                margin = float(np.abs(c["logits"] - EOS_THRESHOLD).min())
                assert margin >= EOS_MARGIN, (text, seed, i, margin)
                st = eng.new_lm_state(1, c["t_voice"] + c["tokens"].shape[1] + c["gen"])
                st.copy_from(voice.st)
                eng.lm_prefill(st, eng.embed_text(torch.from_numpy(c["tokens"])))
                st.set_noise(TEMP, 0)
                st.set_row_seed(0, chunk_seed(seed, i))
                lat, eos_step = [], None
                for step in range(c["gen"]):
                    x, logit, is_eos = eng.lm_decode_step(st, None, None, 1, EOS_THRESHOLD)
                    torch.cuda.synchronize()
                    if bool(is_eos[0]) and eos_step is None:
                        eos_step = step
                    if eos_step is not None and step >= eos_step + c["fae"]:
                        break
                    lat.append(x.cpu().numpy().copy())
                assert not st.error()
                st.close()
                assert eos_step == c["eos_step"] and len(lat) == c["frames"], (text, i, eos_step, c["eos_step"])
                err = [_maxdiff(a, b) for a, b in zip(lat, c["lat"])]
                print(f"oracle drift {text[:24]!r} seed {seed} chunk {i}: first 8 {max(err[:8]):.2e}, all {len(err)} "
                      f"steps {max(err):.2e}, EOS margin {margin:.3g}")
                assert max(err[:8]) < LAT_ATOL, (text, i, err[:8])
                frames += c["frames"]
            wav = model.generate_audio(state, text, max_tokens=mt, seed=seed)
            assert wav.shape[0] == frames * eng.frame_samples, (text, wav.shape[0], frames)
    finally:
        model._voice_release(voice)


def test_tts_endpoint_repeats_a_seeded_request(model, tmp_path):
    import httpx

    from pocket_tts_amd.server import create_app
    from test_gpu_server import _samples

    shutil.copy(G / "e2e_voice.safetensors", tmp_path / "e2e_voice.safetensors")
    app = create_app(model, slots=4, capacity=512, voices_dir=tmp_path, default_voice="e2e_voice")
    text, seed = CASES[0][0], CASES[0][1]
    mine = {"text": text, "temperature": str(TEMP), "seed": str(seed)}

    async def go():
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t", timeout=600) as cl:
                one = await asyncio.gather(cl.post("/tts", data=mine), cl.post("/tts", data={"text": FILLERS[1], "temperature": "0.7"}))
                two = await asyncio.gather(cl.post("/tts", data={"text": FILLERS[0], "temperature": "0.5", "seed": "3"}),
                                           cl.post("/tts", data={"text": FILLERS[2]}), cl.post("/tts", data=mine))
                bad = await cl.post("/tts", data={"text": text, "seed": "-4"})
                return one[0], two[2], bad

    a, b, bad = asyncio.run(go())
    assert a.status_code == 200 and b.status_code == 200 and bad.status_code == 400
    assert len(a.content) == len(b.content)
    xa, xb = _samples(a.content).astype(np.int32), _samples(b.content).astype(np.int32)
    assert xa.shape[0] > 4800
    d = int(np.abs(xa - xb).max())
    print(f"/tts seeded twice: {xa.shape[0]} samples, largest difference {d} LSB")
    assert d <= 16  # the int16 form of WAV_TOL that test_gpu_e2e.py uses
