"""The text chunks of one request in parallel rows (`ContinuousBatcher(parallel_chunks=)`), on the GPU: a request whose chunks
run side by side delivers what it delivers when they run one after the other - the same frames chunk by chunk, the waveform
within the project's batch-vs-single bound - in fewer scheduler steps, never holds more slots than its window, keeps the order
behind a lagging output chain and in FLAC frame numbers, speaks a script of several voices, and can be cancelled."""

import math
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

import flac_ref
from seed_ref import LONG_TEXT, TEMP

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"
WAV_TOL = 5e-4  # the project's batch-vs-single bound (tests/test_gpu_seed.py:21, from test_gpu_e2e.py)
# tests/test_gpu_stretch.py compares a batcher's stretched rows with a single run bit for bit where both ran under the same
# placement, and names the bound of tests/test_gpu_seed.py for runs under another placement (its `alone` fixture): that
# bound, under its own name here.  Rows of window 3 and rows of window 1 are placed differently.
STRETCH_TOL = WAV_TOL
MT = 12  # max_tokens: LONG_TEXT makes 5 chunks of 6 to 13 tokens, SIX makes 6 chunks of 4 to 13
SIX = "Yes. This is a longer sentence, with several clauses, to test it. Hello world. How are you today? Short one."
# seeds picked with tests/seed_ref.py's oracle: the chunks of LONG_TEXT then have the frame counts 8, 6, 7, 4, 6 (seed 12)
# and 8, 6, 6, 4, 6 (seed 7), with every EOS logit more than 0.1 from the threshold
SEED = 12


@pytest.fixture(scope="module")
def model():
    from pocket_tts_amd import TTSModel

    m = TTSModel.load_model(config=G / "e2e_tiny.yaml", temp=0.0)
    yield m
    m._drop_batch_contexts()
    m._drop_rate_contexts()
    m.engine.close()


@pytest.fixture(scope="module")
def state(model):
    return model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")


@pytest.fixture()
def warm(model):
    """the model at TEMP for one test"""
    model.temp = TEMP
    yield model
    model.temp = 0.0


def _chunks(model, text, max_tokens=MT):
    from pocket_tts_amd.text import split_into_best_sentences

    return split_into_best_sentences(model.tokenizer.encode, model.tokenizer.sp, text, max_tokens,
                                     model.pad_with_spaces_for_short_inputs, model.remove_semicolons)


def _maxdiff(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


class Spy:
    """records, around a batcher's own methods, the rounds of admission [(request id, chunk index, row)] with the step at
    which each happened, and the frame count of every chunk as it leaves"""

    def __init__(self, cb):
        self.cb, self.rounds, self.frames, self.row = cb, [], {}, {}
        admit, finish = cb._admit_group, cb._finish

        def admit_group(jobs, rows):
            self.rounds.append((cb.g, [(j.req.id, j.index, int(b)) for j, b in zip(jobs, rows)]))
            for j, b in zip(jobs, rows):
                self.row[id(j)] = int(b)
            return admit(jobs, rows)

        def finish_job(job):
            self.frames[(job.req.id, job.index)] = int(cb.a_emit[self.row[id(job)]])  # the row's count until it is dealt again
            return finish(job)

        cb._admit_group, cb._finish = admit_group, finish_job

    def chunk_frames(self, req):
        got = {k[1]: v for k, v in self.frames.items() if k[0] == req.id}
        return [got[i] for i in range(len(got))]

    def together(self, req):
        """the largest number of chunks of `req` admitted in one round"""
        return max(sum(1 for rid, _, _ in jobs if rid == req.id) for _, jobs in self.rounds)

    def admitted_at(self, req, index=None):
        """position, in the order of admission, of the request's chunk `index` (None: its first)"""
        flat = [(rid, i) for _, jobs in self.rounds for rid, i, _ in jobs]
        return min(n for n, (rid, i) in enumerate(flat) if rid == req.id and (index is None or i == index))


def _windows(model, state, text, windows, slots=4, build=None, **submit):
    """the same request once per window on one batcher, each time with the batcher to itself:
    [(waveform, frames per chunk, scheduler steps, chunks admitted together, Request)]"""
    from pocket_tts_amd.batching import ContinuousBatcher

    cb = ContinuousBatcher(model, slots=slots, capacity=512, noise_seed=5, parallel_chunks=max(windows), **(build or {}))
    spy, out = Spy(cb), []
    try:
        for w in windows:
            g0, spy.rounds = cb.g, []
            req = cb.submit(state, text, max_tokens=MT, parallel_chunks=w, **submit)
            cb.run_until_idle()
            parts = list(req)
            out.append((parts, spy.chunk_frames(req), cb.g - g0, spy.together(req), req))
        assert cb.failed is None
    finally:
        cb.close()
    return out


def _same_request(model, state, text, n_chunks, **submit):
    (p4, f4, g4, t4, r4), (p1, f1, g1, t1, r1) = _windows(model, state, text, (4, 1), **submit)
    w4, w1 = torch.cat(p4), torch.cat(p1)
    ref = model.generate_audio(state, text, max_tokens=MT, seed=submit.get("seed"))
    assert len(f1) == n_chunks and len(set(f1)) > 1, f1  # chunks of different lengths
    assert f4 == f1 and r4.frames == r1.frames == sum(f1)
    assert w4.shape == w1.shape == ref.shape == (sum(f1) * 1920,)
    d = {"window 4 vs single": _maxdiff(w4, ref), "window 1 vs single": _maxdiff(w1, ref), "window 4 vs window 1": _maxdiff(w4, w1)}
    print(f"frames per chunk {f1}; steps: window 4 {g4}, window 1 {g1}; admitted together {t4} / {t1}; differences {d}")
    assert t4 >= 2 and t1 == 1
    assert g4 < g1
    assert max(d.values()) < WAV_TOL, d


def test_seeded_request_window_4_against_window_1(warm, state):
    chunks = _chunks(warm, LONG_TEXT)
    assert 4 <= len(chunks) <= 6 and len({len(warm.tokenizer.encode(c)) for c in chunks}) > 1
    _same_request(warm, state, LONG_TEXT, len(chunks), seed=SEED)


def test_unseeded_request_at_temp_0(model, state):
    _same_request(model, state, LONG_TEXT, len(_chunks(model, LONG_TEXT)))


def test_order_under_pressure(model, state):
    """3 slots, window 2: the long request never owns more than 2 of them, the two short ones that arrive later get the
    rest in their order and are admitted before the long one's last chunk"""
    from pocket_tts_amd.batching import ContinuousBatcher

    n = len(_chunks(model, SIX))
    assert n == 6
    cb = ContinuousBatcher(model, slots=3, capacity=512, parallel_chunks=2)
    spy, owned = Spy(cb), []

    def step():
        more = cb.step()
        held = sum(1 for j in cb.slot if j is not None and j.req is long)
        owned.append(held + sum(1 for j in cb.waiting if j.req is long))
        return more

    try:
        long = cb.submit(state, SIX, max_tokens=MT)
        for _ in range(4):
            step()
        short = [cb.submit(state, "ok"), cb.submit(state, "Yes.")]
        while step():
            pass
        cb.run_until_idle()
        wav = long.result()
        shorts = [r.result() for r in short]
        frames = spy.chunk_frames(long)
        again = cb.submit(state, SIX, max_tokens=MT, parallel_chunks=1)
        cb.run_until_idle()
        serial = again.result()
        assert cb.failed is None
    finally:
        cb.close()
    assert all(r.error is None and w.shape[0] == r.frames * 1920 > 0 for r, w in zip(short, shorts))
    assert len(frames) == n and frames == spy.chunk_frames(again) and wav.shape == serial.shape == (sum(frames) * 1920,)
    d = _maxdiff(wav, serial)
    print(f"under pressure: frames {frames}, slots and waiting jobs owned per step {owned}, difference to window 1 {d}")
    assert d < WAV_TOL
    assert max(owned) == 2
    last = spy.admitted_at(long, n - 1)
    assert spy.admitted_at(short[0]) < spy.admitted_at(short[1]) < last


def test_a_lagging_chain(model, state):
    """speed 1.25 and a gain: the rows lag, so the drain frames of one chunk overlap the first frames of the next"""
    from pocket_tts_amd.output_chain import ChainSpec

    (p3, f3, g3, t3, r3), (p1, f1, g1, t1, r1) = _windows(
        model, state, LONG_TEXT, (3, 1), slots=3, build=dict(spec=ChainSpec(speeds=[1.25], level=True)),
        speed=1.25, gain_db=6, frames_after_eos=2)
    w3, w1 = torch.cat(p3), torch.cat(p1)
    assert t3 >= 2 and t1 == 1 and len(f1) == 5
    assert f3 == f1 and r3.frames == r1.frames == sum(f1)
    assert w3.shape == w1.shape == (sum(f1) * 1536,)
    d = _maxdiff(w3, w1)
    print(f"lagging chain: frames per chunk {f1}, steps {g3} / {g1}, difference {d}")
    assert d < STRETCH_TOL


def test_flac_frames_are_numbered_in_text_order(model, state):
    (p3, f3, g3, t3, r3), (p1, f1, g1, t1, r1) = _windows(model, state, LONG_TEXT, (3, 1), slots=3,
                                                          build=dict(compressions=["flac"]), compression="flac")
    assert t3 >= 2 and t1 == 1 and f3 == f1
    assert len(p3) == len(p1) == sum(f1) == r3.blocks == r1.blocks
    assert all(p.dtype == torch.uint8 for p in p3)
    dec3 = flac_ref.decode_frames(b"".join(p.numpy().tobytes() for p in p3), 24000)  # checks both CRCs of every frame
    dec1 = flac_ref.decode_frames(b"".join(p.numpy().tobytes() for p in p1), 24000)
    assert [f[1] for f in dec3] == [f[1] for f in dec1] == list(range(sum(f1)))
    x3 = np.concatenate([f[0] for f in dec3]).astype(np.int32)
    x1 = np.concatenate([f[0] for f in dec1]).astype(np.int32)
    assert x3.shape == x1.shape == (sum(f1) * 1920,) and x1.any()
    d = int(np.abs(x3 - x1).max())
    print(f"flac: {len(p3)} frames, largest difference {d} LSB")
    assert d <= math.ceil(WAV_TOL * 32767) + 1


def test_script_of_two_voices(warm, state):
    """Segments A, B, A: each piece is what the single path makes of that chunk with its voice and
    `chunk_seed(seed, index in the whole script)`.  The single path takes the derived seed as it is:
    `_generate_audio_stream_short_text(voice, chunk, frames_after_eos, True, row_seed, spec, request)`."""
    from pocket_tts_amd.batching import ContinuousBatcher
    from pocket_tts_amd.engine import chunk_seed
    from pocket_tts_amd.output_chain import ChainTable
    from pocket_tts_amd.text import prepare_text_prompt

    model = warm
    other = model.get_state_for_conditioning(
        torch.randn(1, 45, model.engine.D, generator=torch.Generator().manual_seed(5)) * 0.1)
    segments = [(state, "Hello world. This is a test."), (other, "How are you today? Short one."),
                (state, "with several clauses.")]
    pieces = [(v, c) for v, t in segments for c in _chunks(model, t)]
    assert len(pieces) == 5
    spec, request = ChainTable.for_request(int(model.sample_rate), model.engine.frame_samples)
    refs = []
    for i, (voice, chunk) in enumerate(pieces):
        fae = model.model_recommended_frames_after_eos
        if fae is None:
            fae = prepare_text_prompt(chunk, model.pad_with_spaces_for_short_inputs, model.remove_semicolons)[1] + 2
        refs.append(torch.cat(list(model._generate_audio_stream_short_text(voice, chunk, fae, True, chunk_seed(SEED, i),
                                                                            spec, request))))
    cb = ContinuousBatcher(model, slots=4, capacity=512, noise_seed=5, parallel_chunks=4)
    spy = Spy(cb)
    try:
        req = cb.submit_script(segments, max_tokens=MT, seed=SEED)
        cb.run_until_idle()
        wav = req.result()
        with pytest.raises(ValueError, match="empty"):
            cb.submit_script([(state, "Hello."), (other, " ")])
        assert cb.failed is None
    finally:
        cb.close()
    frames = spy.chunk_frames(req)
    assert frames == [r.shape[0] // 1920 for r in refs] and wav.shape[0] == sum(frames) * 1920
    assert spy.together(req) >= 2
    diffs = [_maxdiff(got, ref) for got, ref in zip(wav.split([f * 1920 for f in frames]), refs)]
    print(f"script: frames per piece {frames}, differences {diffs}")
    assert max(diffs) < WAV_TOL


def test_cancel(warm, state):
    from pocket_tts_amd.batching import ContinuousBatcher

    model = warm
    cb = ContinuousBatcher(model, slots=3, capacity=512, noise_seed=5, parallel_chunks=2)
    try:
        req = cb.submit(state, SIX, max_tokens=MT, seed=SEED)
        for _ in range(5):
            cb.step()
        assert any(j is not None for j in cb.slot) and cb._chain  # chunks in rows, chunks not yet released
        req.cancel()
        req.cancel()
        cb.run_until_idle()
        assert all(j is None for j in cb.slot) and not cb.waiting and not cb._chain and not cb._outstanding
        got = list(req)  # ends without raising, behind what had been forwarded
        assert req.error is None and len(got) == req.frames <= 5  # no more than the five steps had produced
        req.cancel()  # after the end: nothing
        assert req._q.empty()
        text = "Hello world. This is a test."
        after = cb.submit(state, text, seed=7)
        cb.run_until_idle()
        wav = after.result()
        assert cb.failed is None
    finally:
        cb.close()
    ref = model.generate_audio(state, text, seed=7)
    assert wav.shape == ref.shape
    d = _maxdiff(wav, ref)
    print(f"cancel: {len(got)} frames forwarded before it; the request behind it differs from its reference by {d}")
    assert d < WAV_TOL


def test_a_chunk_that_fails_at_admission_takes_its_siblings_along(model, state):
    """a script whose second segment has a voice state the import refuses (wrong head count): the chunks of the first
    segment, admitted beside it, leave their slots, the chunks behind it never run, the consumer gets the error, and the
    batcher serves the next request"""
    from pocket_tts_amd.batching import ContinuousBatcher

    bad = {k: dict(v) for k, v in state.items()}
    first = next(iter(bad))
    bad[first]["cache"] = bad[first]["cache"][:, :, :, :1]
    text = "Hello world. This is a test."
    cb = ContinuousBatcher(model, slots=4, capacity=512, parallel_chunks=4)
    try:
        req = cb.submit_script([(state, text), (bad, "How are you today?"), (state, SIX)], max_tokens=MT)
        assert len(cb.waiting) == 4 and len(cb._chain[req.id]) == 5  # 2 + 1 + 6 chunks, four of them released
        # the first round admits chunks 0 to 3 as one group, which fails; one by one, 0 and 1 reach their rows, 2 is refused
        assert cb.step() is False
        assert req.error is not None
        assert all(j is None for j in cb.slot) and not cb.waiting and not cb._chain and not cb._outstanding
        with pytest.raises((ValueError, KeyError, IndexError, TypeError)):
            list(req)
        after = cb.submit(state, text)
        cb.run_until_idle()
        wav = after.result()
        assert cb.failed is None
    finally:
        cb.close()
    ref = model.generate_audio(state, text)
    assert wav.shape == ref.shape and _maxdiff(wav, ref) < WAV_TOL


def test_generate_audio_parallel_chunks(warm, state, tmp_path, monkeypatch):
    from pocket_tts_amd import main, tts_model

    model = warm
    ref = model.generate_audio(state, LONG_TEXT, max_tokens=MT, seed=7)
    assert not model._batchers
    wav = model.generate_audio(state, LONG_TEXT, max_tokens=MT, seed=7, parallel_chunks=4)
    assert len(model._batchers) == 1
    cb = next(iter(model._batchers.values()))
    assert cb.B == 4 and cb.parallel_chunks == 4
    items = list(model.generate_audio_stream(state, LONG_TEXT, max_tokens=MT, seed=7, parallel_chunks=4))
    assert list(model._batchers.values()) == [cb] and cb.failed is None  # the second call reused the batcher
    assert all(i.shape == (1920,) and i.dtype == torch.float32 for i in items)
    again = torch.cat(items)
    d = {"parallel vs serial": _maxdiff(wav, ref) if wav.shape == ref.shape else None,
         "stream vs tensor": _maxdiff(again, wav) if again.shape == wav.shape else None}
    print(f"generate_audio(parallel_chunks=4): {wav.shape[0] // 1920} frames, differences {d}")
    assert wav.shape == ref.shape == again.shape
    assert d["parallel vs serial"] < WAV_TOL and d["stream vs tensor"] < WAV_TOL
    # one chunk, or a window of 1: the path of before, no batcher
    one = model.generate_audio(state, "Hello world.", seed=7, parallel_chunks=4)
    assert torch.equal(one, model.generate_audio(state, "Hello world.", seed=7)) and len(model._batchers) == 1
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="parallel_chunks"):
            model.generate_audio(state, LONG_TEXT, max_tokens=MT, parallel_chunks=bad)
    # a consumer that stops early leaves no row behind
    stream = model.generate_audio_stream(state, LONG_TEXT, max_tokens=MT, seed=7, parallel_chunks=4)
    next(stream)
    stream.close()
    assert all(j is None for j in cb.slot) and not cb.waiting and not cb._chain and cb.failed is None
    # the command line
    monkeypatch.setattr(tts_model.TTSModel, "load_model", staticmethod(lambda **kw: model))
    sizes = []
    for extra in ([], ["--parallel-chunks", "4"]):
        out = tmp_path / f"out{len(extra)}.wav"
        assert main.cli_app(["generate", "--text", LONG_TEXT, "--voice", str(G / "e2e_voice.safetensors"), "--max-tokens",
                             str(MT), "--seed", "7", *extra, "--output-path", str(out), "-q"]) == 0
        with wave.open(str(out), "rb") as w:
            sizes.append(w.getnframes())
    assert sizes[0] == sizes[1] == ref.shape[0] + 4800
    model._drop_batch_contexts()
    assert not model._batchers and cb._closed
