"""Pins tests/voice_ref.py and proves that the GPU matrix's bound (tests/test_gpu_voice_matrix.py: 8 E32 per stage)
discriminates.  No GPU.

1. The fp64 chain of the stage functions agrees with `oracle.np_oracle.VoiceEncoder` (float32, itself tied to the reference
   project's goldens by test_oracle_golden.py) tap by tap, within ORACLE_FACTOR = 8 times the chain's own float32 error at
   that tap: the oracle is one more float32 evaluation in one more summation order (einsum), the allowance the GPU kernels
   get for theirs.
2. The fp64 chain meets the reference-generated goldens `encode_tiny` (every committed tap) and `encode_en100m` within the
   2e-4 of test_oracle_golden.py.
3. Every seeded defect of `voice_ref.MUTANTS` moves the fp64 result of its designated stages by at least 32 E32, 4 times the
   GPU tolerance, on the very audio the GPU matrix uses (`voice_ref.case_audio`), at the lengths where the defect can show:
   a tail exists only where the audio ends inside a frame; the window needs more positions than the context of 40 (3 frames
   and more); 6, 5, 4 differs from 4, 5, 6 in rounds 1 and 3 only.  A RoPE that starts at position 1 leaves every attention
   score as it is (scores depend on q - k only: the fp64 attention output moves by the rounding of the float32 angle alone,
   measured <= 1.94 E32, within the GPU bound), so it
   is designated to stage Q, the queries and keys the attention kernel reads.  The 32 is a condition that keeps the GPU
   bound meaningful, not a measurement.
4. Every stage's E32 is positive on every input that stage is judged on."""

import numpy as np
import pytest

import voice_ref as V
from conftest import synth_weights
from oracle import np_oracle as O

GPU_FACTOR = 8  # test_gpu_voice_matrix.FACTOR
MUTANT_FACTOR = 4 * GPU_FACTOR
ORACLE_FACTOR = 8
ATOL = 2e-4  # test_oracle_golden.ATOL
RATIOS = {}
ORACLE_TAPS = {"enc0": "conv0_raw", "enc1": "se1", "enc3": "down1_raw", "enc4": "se2", "enc6": "down2_raw", "enc7": "se3",
               "enc9": "down3_raw", "enc11": "final", "enc_tr": "enc_tr"}  # se<i>: the oracle's raw sum, ELU'd
F1, F3, F6, F17 = V.LENGTHS[1], V.LENGTHS[3], V.LENGTHS[4], V.LENGTHS[6]
_TAPS = {}


def weights(name):
    return synth_weights(name) if name == "en100m" else V.codec_weights(name)


def taps_of(name, n):
    """the float32 chain's taps on the matrix's audio of this case: the stage inputs of the experiments"""
    if (name, n) not in _TAPS:
        cfg, W = weights(name)
        _TAPS[(name, n)] = V.encode(cfg, W, V.case_audio(name, n), np.float32)
    return _TAPS[(name, n)]


@pytest.mark.parametrize("name,n", [("tiny", F3), ("nf64", V.LENGTHS[2]), ("tiny1", V.LENGTHS[0])])
def test_float64_chain_agrees_with_the_oracle(name, n):
    cfg, W = V.codec_weights(name)
    audio = V.case_audio(name, n)
    want = {}
    enc = O.VoiceEncoder(cfg, W)
    lat = enc.encode_to_latent(audio[None, None], want)
    assert set(want) == set(ORACLE_TAPS)
    want = {ORACLE_TAPS[k]: (O.elu(v) if ORACLE_TAPS[k].startswith("se") else v)[0].T for k, v in want.items()}
    want["latent"] = lat[0].T
    want["cond"] = enc.conditioning(audio[None, None])[0]
    t64, e32 = V.chain_taps_e32(cfg, W, audio)
    assert np.array_equal(t64["audio"][:n], audio) and not t64["audio"][n:].any() and len(t64["audio"]) % V.FRAME == 0
    for k, v in want.items():
        assert v.shape == t64[k].shape and e32[k] > 0, (k, v.shape, t64[k].shape)
        err = float(np.abs(v - t64[k]).max())
        print(f"{name} {n} {k:10s} |oracle - y64| {err:.2e}  chain E32 {e32[k]:.2e}  ratio {err / e32[k]:.2f}")
        assert err <= ORACLE_FACTOR * e32[k], (k, err, e32[k])


@pytest.mark.parametrize("case", ["encode_tiny", "encode_en100m"])
def test_float64_chain_meets_the_goldens(golden, case):
    g = golden(case)
    m = g["meta"]
    cfg, W = synth_weights(m["config"], m["seed"])
    t = V.encode(cfg, W, g["audio"][0, 0])
    assert np.abs(t["latent"] - g["latent"][0].T).max() < ATOL
    assert np.abs(t["cond"] - g["conditioning"][0]).max() < ATOL
    for k, name in ORACLE_TAPS.items():
        if "tap_" + k in g:
            ref = g["tap_" + k][0].T.astype(np.float64)
            if name.startswith("se"):
                ref = np.where(ref > 0, ref, np.expm1(np.minimum(ref, 0)))
            assert np.abs(t[name] - ref).max() < ATOL, k
    assert case != "encode_tiny" or all("tap_" + k in g for k in ORACLE_TAPS)


# mutant -> [(configuration, stage, samples)]
ENDS_IN_FRAME = [n for n in V.LENGTHS if n % V.FRAME]
ABOVE_CONTEXT = [n for n in V.LENGTHS if -(-n // V.FRAME) * 16 > 40]
DESIGNATED = {
    "tail_repeat": [(c, s, n) for n in ENDS_IN_FRAME for c, s in (("tiny", "E0"), ("nf64", "E0e"))] + [("en100m", "E0", F17)],
    "ctx_2r1": [("tiny", "Dn1", F1), ("nf64", "Dn2", F1), ("tiny1", "Dn3", F1), ("nf64", "Dn1e", F3), ("en100m", "Dn3", F17)],
    "phase": [("tiny", "Dn1", F1), ("nf64", "Dn2", F1), ("tiny1", "Dn3", F1), ("tiny", "Dn3e", F3), ("en100m", "Dn2", F17)],
    "ratios_rev": [("tiny", "Dn1", F1), ("nf64", "Dn3", F1), ("nf64", "Dn1e", F3), ("en100m", "Dn1", F17)],
    "skip_elu": [("tiny", "Rb1", F1), ("nf64", "Rb2", F1), ("tiny1", "Rb3", F1), ("en100m", "Rb1", F17)],
    "elu_twice": [("tiny", "Ra1", F1), ("nf64", "Ra2", F1), ("tiny1", "Ra3", F1), ("tiny", "Dn2e", F1), ("nf64", "F", F1),
                  ("en100m", "Ra3", F17)],
    "ds_zero": [(c, "DS", n) for c in V.CONFIG_NAMES for n in (V.LENGTHS[0], F17)] + [("en100m", "DS", F17)],
    "ds_swap": [(c, "DS", n) for c in V.CONFIG_NAMES for n in (V.LENGTHS[0], F17)] + [("en100m", "DS", F17)],
    "window": [(c, s, n) for n in ABOVE_CONTEXT for c, s in (("tiny", "T"), ("tiny1", "A"), ("nf64", "A"))] + [("en100m", "T", F17)],
    "rope_pos1": [(c, "Q", n) for c in ("tiny1", "nf64") for n in (V.LENGTHS[0], F6, F17)],
    "no_ls": [("tiny1", "B", F1), ("nf64", "B", F6), ("tiny", "D", F1), ("nf64", "D", F1), ("en100m", "D", F17)],
    "tanh_gelu": [("tiny", "C", F1), ("nf64", "C", F1), ("tiny1", "C", F6), ("en100m", "C", F17)],
    "proj_prev": [(c, "SP", n) for c in V.CONFIG_NAMES for n in (V.LENGTHS[0], F17)] + [("en100m", "SP", F17)],
}


def test_every_mutant_is_designated():
    assert sorted(DESIGNATED) == sorted(V.MUTANTS)
    assert {s for d in DESIGNATED.values() for _, s, _ in d} == set(V.STAGES)
    assert ABOVE_CONTEXT == list(V.LENGTHS[3:]) and len(ENDS_IN_FRAME) == 4


@pytest.mark.parametrize("mutant,name,stage,n", [(m, *d) for m, ds in sorted(DESIGNATED.items()) for d in ds])
def test_mutant_moves_the_result(mutant, name, stage, n):
    cfg, W = weights(name)
    inputs = V.stage_inputs(stage, cfg, W, taps_of(name, n), V.case_audio(name, n))
    y64, e32 = V.stage_e32(stage, inputs)
    moved = float(np.abs(V.STAGES[stage](**inputs, mutate=mutant) - y64).max())
    RATIOS[(mutant, name, stage, n)] = (e32, moved)
    print(f"mutant {mutant} {name} {stage} n={n}: E32 {e32:.2e}, moved {moved:.2e} = {moved / e32:.3g} x E32")
    assert e32 > 0
    assert moved >= MUTANT_FACTOR * e32, (moved, e32, moved / e32)


@pytest.mark.parametrize("name", ["tiny1", "nf64"])
def test_a_rope_start_offset_cannot_show_in_the_attention_output(name):
    """why `rope_pos1` is judged on stage Q: in fp64 the attention output moves by the rounding of the float32 angle only"""
    cfg, W = V.codec_weights(name)
    for n in (F1, F17):
        inputs = V.stage_inputs("A", cfg, W, taps_of(name, n), None)
        y64, e32 = V.stage_e32("A", inputs)
        moved = float(np.abs(V._transformer(cfg, W, inputs["x"], np.float64, "np", False, "rope_pos1")["attn"] - y64).max())
        print(f"{name} n={n}: stage A moves by {moved / e32:.3g} x E32")
        assert moved < GPU_FACTOR * e32


@pytest.mark.parametrize("name", V.CONFIG_NAMES + ("en100m",))
def test_e32_is_a_float32_rounding_error(name):
    """every stage's E32 is positive and within the 1e-5 that ties float32 to the oracle, at every length it is judged on"""
    cfg, W = weights(name)
    for n in V.LENGTHS if name != "en100m" else (F17,):
        taps, audio = taps_of(name, n), V.case_audio(name, n)
        for stage in V.stages_of(cfg):
            _, e32 = V.stage_e32(stage, V.stage_inputs(stage, cfg, W, taps, audio))
            assert 0 < e32 <= 1e-5, (name, n, stage, e32)
        (_, e_lat), (_, e_cond) = V.chain_e32(cfg, W, audio)
        assert e_lat > 0 and e_cond > 0, (name, n, e_lat, e_cond)


def test_zz_mutation_table():
    print(f"\nseeded defects against the fp64 stage references (required: >= {MUTANT_FACTOR} x E32)")
    for (m, name, stage, n), (e, moved) in sorted(RATIOS.items()):
        print(f"  {m:11s} {name:6s} {stage:4s} n={n:5d}  E32 {e:.2e}  moved {moved:.2e}  = {moved / e:9.3g} x E32   {V.MUTANTS[m]}")
