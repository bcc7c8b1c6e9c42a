"""The codec frame in its two parts (ptts_mimi_decode_tr / ptts_mimi_decode_seanet): the transformer of a frame PAIR in one
launch sequence (32 rows per sequence, the T-general path) must give what two single frames give, through the 4-slot
hand-over ring, across ring wraps of the K / V cache, resets and any mix of pairs and singles on one state.

Tolerance: the project's own, test_gpu_parity.ATOL (max-abs 2e-4 on O(1) values): a pair runs the same fp32 arithmetic as two
singles with other GEMM tiles and another split of the attention keys, i.e. another summation order, which is what ATOL
allows between any two evaluations here (GPU against the oracle, tuned against untuned tiles).  `-m gpu`."""

import numpy as np
import pytest
import torch

from conftest import synth_weights
from test_gpu_parity import ATOL, _maxerr, dev, get_engine

pytestmark = pytest.mark.gpu

NF = 40  # en100m: the 288-slot K / V ring wraps at frame 18 and the 250-key window is active from frame 16 on
_REF = {}


def latents(B, ldim, seed, nf=NF):
    return np.random.default_rng(seed).standard_normal((nf, B, ldim)).astype(np.float32)


def singles(eng, B, lat, taps=True):
    """every frame through ptts_mimi_decode on a fresh state: PCM and the transformer's output per frame"""
    ms = eng.new_mimi_state(B)
    pcm, tr = [], []
    for f in range(len(lat)):
        out = eng.mimi_decode(ms, dev(lat[f]))
        torch.cuda.synchronize()
        pcm.append(out.cpu().numpy())
        if taps:
            tr.append(eng.debug_read(ms, "dec_tr").cpu().numpy())
    ms.close()
    return np.stack(pcm), (np.stack(tr) if taps else None)


def slot(eng, ms, frame):
    """the transformer's output of `frame` (counted from the state's last reset), from its slot of the hand-over ring"""
    return eng.debug_read(ms, f"dec_tr_slot{frame & 3}").cpu().numpy()


def run_plan(eng, ms, lat, plan, taps=True, f0=0):
    """plan: a string over 'P' (pair), 'S' (single in two parts), 'W' (single, whole frame); frames in order from lat,
    the first of which is the state's frame f0"""
    pcm, tr, f = [], [], 0
    for op in plan:
        if op == "P":
            eng.mimi_decode_tr(ms, dev(lat[f]), dev(lat[f + 1]))
            if taps:
                tr += [slot(eng, ms, f0 + f), slot(eng, ms, f0 + f + 1)]
            for _ in range(2):
                pcm.append(eng.mimi_decode_seanet(ms).cpu().numpy())
            f += 2
        elif op == "S":
            eng.mimi_decode_tr(ms, dev(lat[f]))
            if taps:
                tr.append(slot(eng, ms, f0 + f))
            pcm.append(eng.mimi_decode_seanet(ms).cpu().numpy())
            f += 1
        else:
            pcm.append(eng.mimi_decode(ms, dev(lat[f])).cpu().numpy())
            if taps:
                tr.append(eng.debug_read(ms, "dec_tr").cpu().numpy())
            f += 1
        torch.cuda.synchronize()
    return np.stack(pcm), (np.stack(tr) if taps else None)


def en100m_reference():
    """the numpy oracle's PCM of the en100m run, and the GPU's single-frame run of the same latents: computed once"""
    if "en100m" not in _REF:
        from oracle import np_oracle as O

        cfg, W = synth_weights("en100m")
        eng = get_engine("en100m")
        B = 2
        lat = latents(B, eng.ldim, 901)
        dec = O.MimiDecoder(cfg, W)
        ost = dec.init_state(B, NF)
        ref = np.stack([dec.decode(ost, lat[f]) for f in range(NF)])
        pcm, tr = singles(eng, B, lat)
        _REF["en100m"] = dict(lat=lat, oracle=ref, pcm=pcm, tr=tr)
    return _REF["en100m"]


@pytest.mark.parametrize("cfg_name,B", [("tiny", 3), ("en100m", 2)])
def test_pairs_match_singles(cfg_name, B):
    """40 frames from reset as 20 pairs and as 40 singles: PCM and the transformer output of every frame within ATOL; the
    en100m run also against the oracle's decoder"""
    eng = get_engine(cfg_name)
    if cfg_name == "en100m":
        r = en100m_reference()
        lat, pcm1, tr1 = r["lat"], r["pcm"], r["tr"]
    else:
        lat = latents(B, eng.ldim, 900)
        pcm1, tr1 = singles(eng, B, lat)
    ms = eng.new_mimi_state(B)
    pcm2, tr2 = run_plan(eng, ms, lat, "P" * (NF // 2))
    ms.close()
    e_tr = np.abs(tr2 - tr1).reshape(NF, -1).max(1)
    e_pcm = np.abs(pcm2 - pcm1).reshape(NF, -1).max(1)
    print(f"{cfg_name} B={B}: pairs vs singles, transformer output worst {e_tr.max():.2e}, PCM worst {e_pcm.max():.2e}; "
          f"bitwise equal: transformer {np.array_equal(tr1, tr2)}, PCM {np.array_equal(pcm1, pcm2)}")
    assert e_tr.max() < ATOL, e_tr
    assert e_pcm.max() < ATOL, e_pcm
    assert np.abs(pcm2).max() > 0
    if cfg_name == "en100m":
        e_or = np.abs(pcm2 - r["oracle"]).reshape(NF, -1).max(1)
        print(f"en100m pairs vs oracle: worst PCM error {e_or.max():.2e}")
        assert e_or.max() < ATOL, e_or


def test_mixed_pairs_and_singles_on_one_state():
    """pair, pair, single (a 5-frame utterance), reset, pair, single, single, pair: slot and counter bookkeeping, the zq
    carry across a pair boundary, a single after a pair, whole frames between parts"""
    eng = get_engine("tiny")
    B = 3
    lat = latents(B, eng.ldim, 902, 11)
    ref1, tr1 = singles(eng, B, lat[:5])
    ref2, tr2 = singles(eng, B, lat[5:])
    ms = eng.new_mimi_state(B)
    pcm, tr = run_plan(eng, ms, lat[:5], "PPS")
    assert _maxerr(pcm, ref1) < ATOL and _maxerr(tr, tr1) < ATOL
    ms.reset()
    pcm, tr = run_plan(eng, ms, lat[5:], "PSWP")
    e = np.abs(pcm - ref2).reshape(6, -1).max(1)
    assert e.max() < ATOL and _maxerr(tr, tr2) < ATOL, e
    ms.close()


def test_hand_over_refusals():
    """the ring holds a pair beside the frame before it: a second pair before SEANet has read the first is refused, and
    so is a SEANet decode without a frame; nothing is enqueued by a refused call"""
    eng = get_engine("tiny")
    B = 3
    lat = latents(B, eng.ldim, 903, 4)
    ref, _ = singles(eng, B, lat, taps=False)
    ms = eng.new_mimi_state(B)
    with pytest.raises(Exception):
        eng.mimi_decode_seanet(ms)
    eng.mimi_decode_tr(ms, dev(lat[0]), dev(lat[1]))
    with pytest.raises(Exception):
        eng.mimi_decode_tr(ms, dev(lat[2]), dev(lat[3]))
    got = [eng.mimi_decode_seanet(ms).cpu().numpy()]
    eng.mimi_decode_tr(ms, dev(lat[2]), dev(lat[3]))  # one frame waiting: a pair fits
    got += [eng.mimi_decode_seanet(ms).cpu().numpy() for _ in range(3)]
    torch.cuda.synchronize()
    assert _maxerr(np.stack(got), ref) < ATOL
    ms.close()


def test_reset_row_between_launches():
    """reset_row of one row between two launches: that row continues as a fresh state's, the others are unchanged; all
    four hand-over slots of the row are zeroed"""
    eng = get_engine("tiny")
    B, row = 3, 1
    lat = latents(B, eng.ldim, 904, 8)
    ref, _ = singles(eng, B, lat, taps=False)
    fresh, _ = singles(eng, B, lat[4:], taps=False)  # what a row that starts at frame 4 gives
    ms = eng.new_mimi_state(B)
    pcm_a, _ = run_plan(eng, ms, lat[:4], "PP", taps=False)
    ms.reset_row(row)
    for k in range(4):
        t = eng.debug_read(ms, f"dec_tr_slot{k}").cpu().numpy().reshape(B, 16, -1)
        assert not t[row].any() and t[(row + 1) % B].any(), k
    pcm_b, _ = run_plan(eng, ms, lat[4:], "PSW", taps=False, f0=4)
    torch.cuda.synchronize()
    others = [b for b in range(B) if b != row]
    assert _maxerr(pcm_a, ref[:4]) < ATOL
    assert _maxerr(pcm_b[:, others], ref[4:, others]) < ATOL
    assert _maxerr(pcm_b[:, row], fresh[:, row]) < ATOL
    ms.close()


def test_single_frames_on_the_288_slot_ring_vs_oracle():
    """en100m, 40 single frames at batch 2 through ptts_mimi_decode: the K / V ring (context + two frames = 288 slots)
    wraps and the 250-key window is active; against the numpy oracle at the bound of tests/test_gpu_split.py"""
    r = en100m_reference()
    e = np.abs(r["pcm"] - r["oracle"]).reshape(NF, -1).max(1)
    print(f"en100m B=2: single frames vs oracle, worst PCM error {e.max():.2e} over {NF} frames (tolerance {ATOL:.0e})")
    assert e.max() < ATOL, e
