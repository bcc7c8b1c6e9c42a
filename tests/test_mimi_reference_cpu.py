"""Pins tests/mimi_ref.py and proves that the GPU matrix's bound (tests/test_gpu_mimi_matrix.py: 8 E32 per stage)
discriminates.  No GPU.

1. The stage functions chained in float32 are `oracle.np_oracle.MimiDecoder` (itself tied to the reference project's goldens
   by test_oracle_golden.py), tap by tap over 6 frames, within the 1e-5 that ties float32 to the oracle in
   test_flow_reference_cpu.py.
2. The float64 chain meets the committed taps of tests/golden/golden_tiny_b2.npz within that file's 2e-4.
3. Every seeded defect of `mimi_ref.MUTANTS` moves the fp64 result of its designated stages by at least 32 E32, 4 times the
   GPU tolerance, on the smallest case the GPU matrix runs for the stage: B = 1 (B = 3 for the defect that needs a sequence
   boundary), at the first frame the defect can show (frame 1 for a wrong parity or a dropped carry, frame 3 for the window,
   frame 4, where positions pass the ring's 64 slots, for the ring position).  The 32 is a condition that keeps the GPU bound
   meaningful, not a measurement."""

import numpy as np
import pytest

import mimi_ref as R
from conftest import synth_weights
from oracle import np_oracle as O

GPU_FACTOR = 8  # test_gpu_mimi_matrix.FACTOR
MUTANT_FACTOR = 4 * GPU_FACTOR
ELU_TAPS = ("seanet0", "seanet3", "seanet6", "seanet9")
RATIOS = {}


def oracle_taps(cfg, W, latents):
    """per frame the oracle's taps in the engine's convention: [B, T, C], ELU applied where the producer applies it"""
    dec = O.MimiDecoder(cfg, W)
    st = dec.init_state(latents.shape[1], len(latents))
    out = []
    for lat in latents:
        taps = {}
        pcm = dec.decode(st, lat, taps)
        t = {k: (O.elu(v) if k in ELU_TAPS else v).transpose(0, 2, 1) for k, v in taps.items() if k in R.OUTPUT_TAP.values()}
        t["pcm"] = pcm
        out.append(t)
    return out


@pytest.mark.parametrize("name", ["tiny", "nf64"])
def test_float32_chain_is_the_oracle(name):
    cfg, W = R.codec_weights(name)
    latents = R.seeded_latents(cfg, 6, 2, 5)
    want = oracle_taps(cfg, W, latents)
    for fused_tail in (False, True):
        chain = R.Chain(cfg, W, 2, np.float32, fused_tail=fused_tail)
        for f, lat in enumerate(latents):
            got = chain.decode(lat)
            names = [k for k in got if k != "latent" and not k.startswith("tr_")]  # the oracle taps no layer's inside
            assert set(names) == set(want[f]) - ({"seanet9"} if fused_tail else set())
            for k in names:
                assert got[k].dtype == np.float32 and got[k].shape == want[f][k].shape, (k, got[k].shape)
                assert np.abs(got[k] - want[f][k]).max() <= 1e-5, (name, f, k)


def test_float64_chain_meets_the_golden_taps(golden):
    g = golden("tiny_b2")
    m = g["meta"]
    cfg, W = synth_weights(m["config"], m["seed"])
    chain = R.Chain(cfg, W, m["B"])
    for f, lat in enumerate(g["mimi_latents"]):
        got = chain.decode(lat)
        assert np.abs(got["pcm"] - g["pcm"][f]).max() < 2e-4, f
        if f >= 3:
            continue
        for k in [k for k in g if k.startswith("tap_") and k != "tap_seanet11"]:
            ref = g[k][f].astype(np.float64)  # [B, C, T], raw
            if k[4:] in ELU_TAPS:
                ref = np.where(ref > 0, ref, np.expm1(np.minimum(ref, 0)))
            assert np.abs(got[k[4:]] - ref.transpose(0, 2, 1)).max() < 2e-4, (f, k)


def test_reset_row_restarts_one_sequence():
    """after `reset_row` the row reproduces its own first frames on the same latents; the other rows are not touched"""
    cfg, W = R.codec_weights("tiny")
    latents = R.seeded_latents(cfg, 5, 3, 9)
    latents[3:, 2] = latents[:2, 2]
    plain, reset = R.Chain(cfg, W, 3), R.Chain(cfg, W, 3)
    a = [plain.decode(lat)["pcm"] for lat in latents]
    b = []
    for f, lat in enumerate(latents):
        if f == 3:
            reset.reset_row(2)
        b.append(reset.decode(lat)["pcm"])
    for f in range(5):
        assert np.array_equal(a[f][:2], b[f][:2])
    assert np.abs(b[3][2] - a[0][2]).max() <= 1e-12 and np.abs(b[4][2] - a[1][2]).max() <= 1e-12
    assert np.abs(a[3][2] - a[0][2]).max() > 1e-3


# mutant -> [(configuration, stage, B, frame)]
CONV = [("tiny", "S0"), ("nf64", "C1"), ("tiny", "R2"), ("nf64", "R3"), ("tiny", "L"), ("nf64", "L")]
DESIGNATED = {
    "parity": [(c, s, 1, 1) for c, s in CONV + [("tiny", "C3"), ("nf64", "R1")]],
    "seqcut": [(c, s, 3, 0) for c, s in CONV] + [("nf64", "C2", 3, 2)],
    "skip_elu": [("tiny", "R1", 1, 0), ("tiny", "R3", 1, 0), ("nf64", "R2", 1, 0), ("nf64", "R3", 1, 0), ("nf64", "R3L", 1, 1)],
    "elu_twice": [("tiny", "C1", 1, 0), ("nf64", "C2", 1, 0), ("nf64", "C3", 1, 0)],
    "up_swap": [("tiny", "P", 1, 1), ("nf64", "P", 1, 1)],
    "no_mean": [("tiny", "P", 1, 0), ("nf64", "P", 1, 0)],
    "rope_ring": [("tiny1", "A", 1, 4), ("nf64", "A", 1, 4), ("tiny", "T", 1, 4)],
    "window": [("tiny1", "A", 1, 3), ("nf64", "A", 1, 3), ("tiny", "T", 1, 3)],
    "no_carry": [("tiny", "L", 1, 1), ("nf64", "L", 1, 1), ("nf64", "R3L", 1, 1)],
    "taps_rev": [("tiny", "L", 1, 0), ("nf64", "L", 1, 0), ("nf64", "R3L", 1, 0)],
    "no_ls": [("tiny1", "B", 1, 0), ("nf64", "B", 1, 0), ("tiny", "D", 1, 0), ("nf64", "D", 1, 0)],
    "tanh_gelu": [("tiny", "C", 1, 0), ("nf64", "C", 1, 0)],
    "no_bias2": [("tiny", "R1", 1, 0), ("tiny", "R3", 1, 0), ("nf64", "R2", 1, 0), ("nf64", "R3L", 1, 0)],
}
_FRAMES = {}


def frames_of(name, B):
    """the taps of 6 frames of the float32 chain on seeded latents: the stage inputs of the experiments"""
    if (name, B) not in _FRAMES:
        cfg, W = R.codec_weights(name)
        chain = R.Chain(cfg, W, B, np.float32)
        _FRAMES[(name, B)] = [chain.decode(lat) for lat in R.seeded_latents(cfg, 6, B, 100 + B)]
    return _FRAMES[(name, B)]


def test_every_mutant_is_designated():
    assert sorted(DESIGNATED) == sorted(R.MUTANTS)
    assert {s for d in DESIGNATED.values() for _, s, _, _ in d} == set(R.STAGES)


@pytest.mark.parametrize("mutant,name,stage,B,f", [(m, *d) for m, ds in sorted(DESIGNATED.items()) for d in ds])
def test_mutant_moves_the_result(mutant, name, stage, B, f):
    cfg, W = R.codec_weights(name)
    inputs = R.stage_inputs(stage, cfg, W, frames_of(name, B), f)
    y64, e32 = R.stage_e32(stage, inputs)
    moved = float(np.abs(R.STAGES[stage](**inputs, mutate=mutant) - y64).max())
    RATIOS[(mutant, name, stage)] = (B, f, e32, moved)
    print(f"mutant {mutant} {name} {stage} B={B} frame {f}: E32 {e32:.2e}, moved {moved:.2e} = {moved / e32:.3g} x E32")
    assert e32 > 0
    assert moved >= MUTANT_FACTOR * e32, (moved, e32, moved / e32)


def test_e32_is_a_float32_rounding_error():
    """every stage's E32 is positive and within the 1e-5 that ties float32 to the oracle, at every frame"""
    for name in R.CONFIG_NAMES:
        cfg, W = R.codec_weights(name)
        frames = frames_of(name, 1)
        one = cfg.mimi.transformer.num_layers == 1
        for stage in R.STAGES:
            if (stage in ("A", "B") and not one) or (stage == "T" and one):
                continue  # A and B are defined on one layer, T is judged on two
            for f in (0, 5):
                _, e32 = R.stage_e32(stage, R.stage_inputs(stage, cfg, W, frames, f))
                assert 0 < e32 <= 1e-5, (name, stage, f, e32)


def test_zz_mutation_table():
    print(f"\nseeded defects against the fp64 stage references (required: >= {MUTANT_FACTOR} x E32)")
    for (m, name, stage), (B, f, e, moved) in sorted(RATIOS.items()):
        print(f"  {m:9s} {name:5s} {stage:3s} B={B} f={f}  E32 {e:.2e}  moved {moved:.2e}  = {moved / e:9.3g} x E32   {R.MUTANTS[m]}")
