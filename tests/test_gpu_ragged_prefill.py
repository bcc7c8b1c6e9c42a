"""Ragged prefill (`ptts_lm_prefill_ragged`, include/ptts.h): rows of different lengths in one pass through the FlowLM layers.
Engine level, through the C ABI on the tiny config of tests/golden/e2e_tiny.yaml (synthetic weights): every row ends as the
existing `ptts_lm_prefill` leaves it when run on that row alone, the padding is inert bit for bit, nothing outside a row's
own new positions is written, and a row may end exactly at the capacity.  Public API: the batcher admits requests of any
voice and token count in ONE `_admit_group` call, and `generate_audio_batch` prefills its rows in one pass; both reproduce
`generate_audio`.  `-m gpu`."""

import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from test_gpu_parity import ATOL, dev  # ATOL: the fp32 FlowLM parity bound (the GEMM tile may differ with M)

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"
WAV_TOL = 5e-4  # batch-vs-single bound of test_gpu_e2e.py / test_gpu_seed.py

LENS = [1, 16, 17, 33, 0]   # ends inside a query block / whole padding blocks behind it / crosses a block / no padding / untouched
OFFS = [0, 5, 16, 37, 9]
T_MAX = 33                  # M = 5 * 33 = 165 rows: not a multiple of 16
CAP = 80                    # 37 + 33 + one decode step, a multiple of 16


@pytest.fixture(scope="module")
def model():
    from pocket_tts_amd import TTSModel

    m = TTSModel.load_model(config=G / "e2e_tiny.yaml", temp=0.0)
    yield m
    m.engine.close()


@pytest.fixture(scope="module")
def eng(model):
    return model.engine


def _maxerr(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)))) if np.size(a) else 0.0


def _sentinel(eng, B, cap):
    """finite, position-dependent values no kernel produces by accident"""
    i = np.arange(2 * B * cap * eng.H * 64, dtype=np.float32).reshape(2, B, cap, eng.H, 64)
    return 7.0 + (i % 251) / 256.0


class _Case:
    """history per row (random keys / values, imported), embeddings, and the per-row reference: a batch-1 state with the same
    history, prefilled by the existing ptts_lm_prefill with T = len[b]"""

    def __init__(self, eng, lens, offs, t_max, cap, seed=0):
        rng = np.random.default_rng(seed)
        self.eng, self.lens, self.offs, self.t_max, self.cap, self.B = eng, lens, offs, t_max, cap, len(lens)
        self.hist = [[(rng.standard_normal((2, 1, o, eng.H, 64)) * 0.5).astype(np.float32) for _ in range(eng.L)] for o in offs]
        self.emb = (rng.standard_normal((self.B, t_max, eng.D)) * 0.5).astype(np.float32)
        self.noise = (rng.standard_normal((self.B, t_max, eng.D)) * 1e3).astype(np.float32)
        self._ref = None

    def one(self, b, cap=None):
        """batch-1 state holding row b's history"""
        st = self.eng.new_lm_state(1, cap or self.cap)
        if self.offs[b]:
            for l in range(self.eng.L):
                st.import_layer(l, dev(self.hist[b][l]), self.offs[b])
        return st

    def padded(self, scale_noise):
        """the embeddings with zeros or 1e3-scale noise behind each row's real positions"""
        e = self.emb.copy()
        for b, n in enumerate(self.lens):
            e[b, n:] = self.noise[b, n:] if scale_noise else 0.0
        return e

    def state(self, sentinel=True):
        """the batch state: sentinel up to the capacity in every layer, then each row's history on top (full copies: the
        borrowed layout has its own test)"""
        eng = self.eng
        st = eng.new_lm_state(self.B, self.cap)
        assert self.cap % 16 == 0
        if sentinel:
            s = dev(_sentinel(eng, self.B, self.cap))
            for l in range(eng.L):
                st.import_layer(l, s, self.cap)
        eng.set_option("share_prefix", 0)
        try:
            for b in range(self.B):
                one = self.one(b)
                st.copy_row_from(b, one, 0)
                eng.sync()
                one.close()
        finally:
            eng.set_option("share_prefix", 1)
        assert list(st.offsets()) == list(self.offs)
        return st

    def ref(self):
        """per row: (K / V of every layer over [0, off + len), offset, latent and EOS logit of one decode step or None)"""
        if self._ref is None:
            eng, out = self.eng, []
            for b in range(self.B):
                st = self.one(b, self.cap + 16)
                if self.lens[b]:
                    eng.lm_prefill(st, dev(self.emb[b:b + 1, :self.lens[b]]))
                end = self.offs[b] + self.lens[b]
                kv = [st.export_layer(l, end).cpu().numpy()[:, 0] for l in range(eng.L)]
                off = int(st.offsets()[0])
                lat = lg = None
                if end < self.cap:
                    lat, lg, _ = eng.lm_decode_step(st, None, None, 1, -4.0)
                    eng.sync()
                    lat, lg = lat.cpu().numpy()[0].copy(), float(lg.cpu().numpy()[0])
                st.close()
                out.append((kv, off, lat, lg))
            self._ref = out
        return self._ref


def _run(case, scale_noise, lens=None, step=True):
    """one ragged call on a fresh sentinel state -> (planes [L] of [2, B, cap, H, 64], offsets, latents, logits)"""
    eng = case.eng
    st = case.state()
    eng.lm_prefill(st, dev(case.padded(scale_noise)), lens or case.lens)
    eng.sync()
    assert not st.error()
    planes = [st.export_layer(l, case.cap).cpu().numpy() for l in range(eng.L)]
    off = list(st.offsets())
    lat = lg = None
    if step:
        lat, lg, _ = eng.lm_decode_step(st, None, None, 1, -4.0)
        eng.sync()
        lat, lg = lat.cpu().numpy().copy(), lg.cpu().numpy().copy()
    st.close()
    return planes, off, lat, lg


@pytest.fixture(scope="module")
def base(eng):
    case = _Case(eng, LENS, OFFS, T_MAX, CAP)
    case.ref()
    return case, _run(case, False)


def _compare_rows(case, got, what):
    """every row of a ragged result against its batch-1 reference, the worst differences printed"""
    planes, off, lat, lg = got
    worst = dict(kv=0.0, lat=0.0, logit=0.0)
    for b, (kv, roff, rlat, rlg) in enumerate(case.ref()):
        assert off[b] == roff == case.offs[b] + case.lens[b], (b, off[b], roff)
        for l in range(case.eng.L):
            worst["kv"] = max(worst["kv"], _maxerr(planes[l][:, b, :roff], kv[l]))
        if lat is not None and rlat is not None:
            worst["lat"] = max(worst["lat"], _maxerr(lat[b], rlat))
            worst["logit"] = max(worst["logit"], abs(float(lg[b]) - rlg))
    print(f"{what}: worst |ragged - per-row prefill| K/V {worst['kv']:.2e}, next latent {worst['lat']:.2e}, "
          f"EOS logit {worst['logit']:.2e}")
    assert max(worst.values()) < ATOL, worst


def test_ragged_equals_per_row_prefill(base):
    case, got = base
    _compare_rows(case, got, "B 5, t_max 33, lengths [1, 16, 17, 33, 0]")


def test_padding_is_inert_bitwise(base):
    case, (planes, off, lat, lg) = base
    planes2, off2, lat2, lg2 = _run(case, True)
    assert off == off2
    for a, b in zip(planes, planes2):
        assert np.array_equal(a, b)
    assert np.array_equal(lat, lat2) and np.array_equal(lg, lg2)


def _check_outside(case, planes, lens, rows=None):
    """history bitwise in place, sentinel bitwise at and beyond offset + len"""
    sent = _sentinel(case.eng, case.B, case.cap)
    for b in rows if rows is not None else range(case.B):
        o, end = case.offs[b], case.offs[b] + lens[b]
        for l in range(case.eng.L):
            assert np.array_equal(planes[l][:, b, end:], sent[:, b, end:]), (b, l)
            assert np.array_equal(planes[l][:, b, :o], case.hist[b][l][:, 0]), (b, l)
            if lens[b]:
                assert not np.array_equal(planes[l][:, b, o:end], sent[:, b, o:end]), (b, l)


def test_nothing_is_written_outside(base):
    case, (planes, off, _, _) = base
    _check_outside(case, planes, case.lens)
    assert off[4] == OFFS[4]  # the zero-length row: history and sentinel whole (checked above), position unchanged


def test_exact_capacity(eng):
    cap, t_max = 48, 33
    # row 0 fills the cache with t_max itself; row 1 ends exactly at cap while its padding would lie 25 positions past it;
    # row 2 is the neighbour behind it in memory
    case = _Case(eng, [33, 8, 5], [15, 40, 20], t_max, cap, seed=1)
    assert case.offs[1] + case.lens[1] == cap and case.offs[1] + t_max > cap
    got = _run(case, True, step=False)
    _compare_rows(case, got, "exact capacity")
    _check_outside(case, got[0], case.lens)
    # one position too many: refused, nothing changes
    st = case.state()
    before = [st.export_layer(l, cap).cpu().numpy() for l in range(eng.L)]
    with pytest.raises(ValueError):
        eng.lm_prefill(st, dev(case.padded(False)), [33, 9, 5])
    eng.sync()
    assert list(st.offsets()) == case.offs and not st.error()
    for l in range(eng.L):
        assert np.array_equal(st.export_layer(l, cap).cpu().numpy(), before[l])
    st.close()


def test_borrowed_prefix(eng):
    """rows 0 and 1 clone one voice of 37 positions (they borrow its first 32), row 2 another voice of 20 (borrows 16)"""
    rng = np.random.default_rng(3)
    v_emb = [(rng.standard_normal((1, n, eng.D)) * 0.5).astype(np.float32) for n in (37, 20)]
    lens, t_max, src = [7, 18, 3], 18, [0, 0, 1]
    emb = (rng.standard_normal((3, t_max, eng.D)) * 0.5).astype(np.float32)
    res = {}
    for share in (1, 0):
        eng.set_option("share_prefix", share)
        try:
            voices = [eng.new_lm_state(1, n + 4) for n in (37, 20)]
            for v, e in zip(voices, v_emb):
                eng.lm_prefill(v, dev(e))
            st = eng.new_lm_state(3, 37 + t_max + 2)
            for b in range(3):
                st.copy_row_from(b, voices[src[b]], 0)
            eng.lm_prefill(st, dev(emb), lens)
            off = list(st.offsets())
            assert off == [37 + 7, 37 + 18, 20 + 3]
            kv = [st.export_layer(l, max(off)).cpu().numpy() for l in range(eng.L)]
            lat, lg, _ = eng.lm_decode_step(st, None, None, 1, -4.0)
            eng.sync()
            assert not st.error()
            res[share] = (kv, lat.cpu().numpy().copy(), lg.cpu().numpy().copy())
            if share:  # the per-row reference: a clone of the row's voice, prefilled alone by ptts_lm_prefill
                worst = 0.0
                for b in range(3):
                    one = eng.new_lm_state(1, 37 + t_max + 2)
                    one.copy_from(voices[src[b]])
                    eng.lm_prefill(one, dev(emb[b:b + 1, :lens[b]]))
                    for l in range(eng.L):
                        worst = max(worst, _maxerr(kv[l][:, b, :off[b]], one.export_layer(l, off[b]).cpu().numpy()[:, 0]))
                    rl, rg, _ = eng.lm_decode_step(one, None, None, 1, -4.0)
                    eng.sync()
                    worst = max(worst, _maxerr(res[1][1][b], rl.cpu().numpy()[0]))
                    worst = max(worst, abs(float(res[1][2][b]) - float(rg.cpu().numpy()[0])))
                    one.close()
                print(f"borrowed prefix: worst |ragged - per-row prefill| {worst:.2e}")
                assert worst < ATOL
            st.close()
            for v in voices:
                v.close()
        finally:
            eng.set_option("share_prefix", 1)
    for a, b in zip(res[1][0], res[0][0]):
        assert np.array_equal(a, b)
    assert np.array_equal(res[1][1], res[0][1]) and np.array_equal(res[1][2], res[0][2])


def test_oracle(model, base):
    """row 2 (16 positions of history, 17 new ones) in the numpy oracle"""
    from oracle import np_oracle as O
    from pocket_tts_amd.tts_model import _load_weights

    case, (planes, _, _, _) = base
    b, eng = 2, case.eng
    lm = O.FlowLM(model.config, _load_weights(model.config))
    ost = lm.init_state(1, CAP)
    for l in range(eng.L):
        ost[l]["cache"][:, :, :OFFS[b]] = case.hist[b][l]
        ost[l]["offset"] = OFFS[b]
    lm.prefill(ost, case.emb[b:b + 1, :LENS[b]])
    end = OFFS[b] + LENS[b]
    worst = max(_maxerr(planes[l][:, b, :end], ost[l]["cache"][:, 0, :end]) for l in range(eng.L))
    print(f"oracle: worst K/V difference {worst:.2e}")
    assert worst < ATOL


def test_argument_checks(eng, base):
    case = base[0]
    st = case.state()
    before = [st.export_layer(l, CAP).cpu().numpy() for l in range(eng.L)]
    emb = dev(case.padded(False))

    def call(lens, t_max):
        return eng.lib.ptts_lm_prefill_ragged(eng.handle, st.handle, emb.data_ptr(), (C.c_int32 * 5)(*lens), t_max, eng._sp)

    assert call([1, -1, 2, 3, 0], T_MAX) == -1
    assert call([1, T_MAX + 1, 2, 3, 0], T_MAX) == -1
    assert call([0, 0, 0, 0, 0], 0) == -1
    assert call([0, 0, 0, 0, 0], T_MAX) == 0
    eng.sync()
    assert list(st.offsets()) == OFFS and not st.error()
    for l in range(eng.L):
        assert np.array_equal(st.export_layer(l, CAP).cpu().numpy(), before[l])
    st.close()
    # equal lengths: what ptts_lm_prefill gives
    a, b = case.state(), case.state()
    e7 = dev(case.emb[:, :7].copy())
    eng.lm_prefill(a, e7)
    eng.lm_prefill(b, e7, [7] * 5)
    assert list(a.offsets()) == list(b.offsets()) == [o + 7 for o in OFFS]
    worst = max(_maxerr(a.export_layer(l, CAP).cpu().numpy(), b.export_layer(l, CAP).cpu().numpy()) for l in range(eng.L))
    print(f"equal lengths: worst |ragged - ptts_lm_prefill| {worst:.2e}")
    assert worst < ATOL
    a.close()
    b.close()


# ---- public API -----------------------------------------------------------------------------------------------------
TEXTS = ["Hello world. This is a test.", "ok", "This is a longer sentence, with several clauses, to test it.", "How are you today?"]
SEEDS = [11, 12, 13, 14]


def _voices(model):
    va = model.get_state_for_audio_prompt(G / "e2e_voice.safetensors")
    vb = model.get_state_for_conditioning(torch.randn(1, 45, model.engine.D, generator=torch.Generator().manual_seed(5)) * 0.1)
    return va, vb


def test_batcher_admits_mixed_requests_in_one_group(model):
    from pocket_tts_amd.batching import ContinuousBatcher

    va, vb = _voices(model)
    voices = [va, vb, va, vb]
    model.temp = 0.7
    try:
        refs = [model.generate_audio(v, t, seed=s) for v, t, s in zip(voices, TEXTS, SEEDS)]
        calls, counts = [], []
        cb = ContinuousBatcher(model, slots=4, capacity=512, noise_seed=5)
        admit = cb._admit_group

        def record(jobs, rows):
            calls.append([j.req.id for j in jobs])
            counts.append([j.tokens.shape[1] for j in jobs])
            return admit(jobs, rows)

        cb._admit_group = record
        try:
            reqs = [cb.submit(v, t, seed=s) for v, t, s in zip(voices, TEXTS, SEEDS)]
            cb.run_until_idle()
            outs = [r.result() for r in reqs]
        finally:
            cb.close()
    finally:
        model.temp = 0.0
    assert len(calls) == 1 and sorted(calls[0]) == sorted(r.id for r in reqs), calls
    assert len(set(counts[0])) == 4, counts
    worst = 0.0
    for t, a, b in zip(TEXTS, refs, outs):
        assert a.shape == b.shape and a.shape[0] % model.engine.frame_samples == 0, (t, a.shape, b.shape)
        worst = max(worst, _maxerr(a.numpy(), b.numpy()))
    print(f"batcher, one ragged admission: frames {[a.shape[0] // model.engine.frame_samples for a in refs]}, "
          f"worst waveform difference {worst:.2e}")
    assert worst < WAV_TOL


def test_generate_audio_batch_of_mixed_lengths(model):
    va, _ = _voices(model)
    texts, seeds = TEXTS[:3], SEEDS[:3]
    model.temp = 0.7
    try:
        refs = [model.generate_audio(va, t, seed=s) for t, s in zip(texts, seeds)]
        outs = model.generate_audio_batch(va, texts, seeds=seeds)
    finally:
        model.temp = 0.0
    worst = 0.0
    for t, a, b in zip(texts, refs, outs):
        assert a.shape == b.shape, (t, a.shape, b.shape)
        worst = max(worst, _maxerr(a.numpy(), b.numpy()))
    print(f"generate_audio_batch, one ragged prefill: worst waveform difference {worst:.2e}")
    assert worst < WAV_TOL
