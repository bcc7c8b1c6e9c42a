"""The refusals the nine output stages share, word for word: a null handle, a row or a plan index out of range, a drain
flag for a bad row, a frame without its stage or its buffers, and the output chain's two complaints about a stage of the
wrong batch or the wrong width.  Every one is refused on the host before any launch (tiny model, batch 2, one plan per
stage)."""

from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu
G = Path(__file__).parent / "golden"
B = 2

# per stage: the C ABI's prefix, the words of a null handle, what an index is called, the lowest index it takes, whether it
# has a drain flag, and what follows (row, index) in its set_row
STAGES = {
    "resampler": ("resampler", "null resampler", "rate", 0, False, ()),
    "stretcher": ("stretcher", "null stretcher", "plan", 0, True, ()),
    "pitcher": ("pitcher", "null pitcher", "plan", 0, True, ()),
    "toner": ("tone", "null toner", "plan", -1, False, ()),
    "dynamics": ("dynamics", "null compressor", "plan", -1, False, ()),
    "normalizer": ("loudnorm", "null normaliser", "plan", -1, True, (-16.0,)),
    "leveler": ("leveler", "null leveler", "plan", -1, True, (1.0, 1.0)),
    "encoder": ("encoder", "null encoder", None, None, False, ()),
    "packer": ("flac", "null packer", None, None, False, ()),
}

# per stage: its frame entry point, what it takes between (handle, in, out) and the stream, and the message of a null call
FRAMES = {
    "resampler": ("ptts_resample_frame", (0,), "resample_frame: null argument"),
    "stretcher": ("ptts_stretch_frame", (0, None), "stretch_frame: null argument"),
    "pitcher": ("ptts_pitch_frame", (0, None, None), "pitch_frame: null argument"),
    "toner": ("ptts_tone_frame", (), "tone_frame: null argument"),
    "dynamics": ("ptts_dynamics_frame", (), "dynamics_frame: null argument"),
    "normalizer": ("ptts_loudnorm_frame", (None,), "loudnorm_frame: null argument"),
    "leveler": ("ptts_level_frame", (0,), "level_frame: null argument"),
    "encoder": ("ptts_encode_frame", (), "encode_frame: null argument"),
    "packer": ("ptts_flac_frame", (), "flac_frame: null argument"),
}

WANT = {
    "resampler": ["resampler_set_row: null resampler", "resampler_set_row: row out of range", "resampler_set_row: row out of range",
                  "resampler_set_row: rate index out of range", "resampler_set_row: rate index out of range"],
    "stretcher": ["stretcher_set_row: null stretcher", "stretcher_set_row: row out of range", "stretcher_set_row: row out of range",
                  "stretcher_set_row: plan index out of range", "stretcher_set_row: plan index out of range",
                  "stretcher_set_row_drain: null stretcher", "stretcher_set_row_drain: row out of range",
                  "stretcher_set_row_drain: row out of range"],
    "pitcher": ["pitcher_set_row: null pitcher", "pitcher_set_row: row out of range", "pitcher_set_row: row out of range",
                "pitcher_set_row: plan index out of range", "pitcher_set_row: plan index out of range",
                "pitcher_set_row_drain: null pitcher", "pitcher_set_row_drain: row out of range",
                "pitcher_set_row_drain: row out of range"],
    "toner": ["tone_set_row: null toner", "tone_set_row: row out of range", "tone_set_row: row out of range",
              "tone_set_row: plan index out of range", "tone_set_row: plan index out of range"],
    "dynamics": ["dynamics_set_row: null compressor", "dynamics_set_row: row out of range", "dynamics_set_row: row out of range",
                 "dynamics_set_row: plan index out of range", "dynamics_set_row: plan index out of range"],
    "normalizer": ["loudnorm_set_row: null normaliser", "loudnorm_set_row: row out of range", "loudnorm_set_row: row out of range",
                   "loudnorm_set_row: plan index out of range", "loudnorm_set_row: plan index out of range",
                   "loudnorm_set_row_drain: null normaliser", "loudnorm_set_row_drain: row out of range",
                   "loudnorm_set_row_drain: row out of range"],
    "leveler": ["leveler_set_row: null leveler", "leveler_set_row: row out of range", "leveler_set_row: row out of range",
                "leveler_set_row: plan index out of range", "leveler_set_row: plan index out of range",
                "leveler_set_row_drain: null leveler", "leveler_set_row_drain: row out of range",
                "leveler_set_row_drain: row out of range"],
    "encoder": ["encoder_set_row: null encoder", "encoder_set_row: row out of range", "encoder_set_row: row out of range"],
    "packer": ["flac_set_row: null packer", "flac_set_row: row out of range", "flac_set_row: row out of range"],
}


@pytest.fixture(scope="module")
def eng():
    from pocket_tts_amd import TTSModel

    m = TTSModel.load_model(config=G / "e2e_tiny.yaml", temp=0.0)
    yield m.engine
    m.engine.close()


def _new(eng, name, batch=B):
    """the stage at `batch` with one small admissible plan"""
    from pocket_tts_amd import dynamics, level, loudness, pitch, stretch, tone

    rate, fs = eng.sample_rate, eng.frame_samples
    return {
        "resampler": lambda: eng.new_resampler(batch, []),
        "stretcher": lambda: eng.new_stretcher(batch, [stretch.plan(0.8, rate, fs)]),
        "pitcher": lambda: eng.new_pitcher(batch, [pitch.plan("5/4", rate, fs)]),
        "toner": lambda: eng.new_toner(batch, [tone.plan(24000, 1, "warm")]),
        "dynamics": lambda: eng.new_dynamics(batch, [dynamics.plan(24000, 1, "speech")]),
        "normalizer": lambda: eng.new_normalizer(batch, [loudness.plan(8000, 1)]),
        "leveler": lambda: eng.new_leveler(batch, [level.plan(8000, 40)]),
        "encoder": lambda: eng.new_encoder(batch, 1),
        "packer": lambda: eng.new_packer(batch, 1),
    }[name]()


def _refused(eng, fn, *args):
    """the call's error text; it must be refused as a bad argument"""
    assert fn(*args) == -1
    return eng.lib.ptts_last_error().decode()


@pytest.mark.parametrize("name", list(STAGES))
def test_the_shared_refusals_word_for_word(eng, name):
    prefix, _, what, lowest, drains, extra = STAGES[name]
    lib, sp = eng.lib, eng._sp
    set_row = getattr(lib, f"ptts_{prefix}_set_row")
    st = _new(eng, name)
    try:
        n_plans = len(st.plans) if what else None
        assert n_plans in (1, None)
        # what a valid call passes behind the row: the encoder's (n, code), the packer's pass-through of one sample
        ok = {"encoder": (1, 0), "packer": (0, 1, 2, 0, 0, 0)}.get(name, (0, *extra))
        got = [_refused(eng, set_row, None, 0, *ok, sp)]
        got += [_refused(eng, set_row, st.handle, row, *ok, sp) for row in (-1, B)]
        if what:
            got += [_refused(eng, set_row, st.handle, 0, idx, *extra, sp) for idx in (n_plans, lowest - 1)]
        if drains:
            drain = getattr(lib, f"ptts_{prefix}_set_row_drain")
            got += [_refused(eng, drain, None, 0, 1, sp)]
            got += [_refused(eng, drain, st.handle, row, 1, sp) for row in (-1, B)]
        assert got == WANT[name]
        # the frame entry: no stage, then a stage without its input, then without its output; nothing is enqueued
        fn, extra_f, message = FRAMES[name]
        frame, keep = getattr(lib, fn), torch.zeros(64, device=eng.device)
        buf = keep.data_ptr()
        for args in ((None, buf, buf), (st.handle, None, buf), (st.handle, buf, None)):
            assert _refused(eng, frame, *args, *extra_f, sp) == message
    finally:
        st.close()


def test_the_chain_refuses_a_stage_of_the_wrong_batch_or_width(eng):
    assert eng.frame_samples != 40
    ms, wide, narrow = eng.new_mimi_state(B), _new(eng, "leveler", B + 1), _new(eng, "leveler")
    out = torch.zeros(B + 1, eng.frame_samples, device=eng.device)
    try:
        set_leveler = eng.lib.ptts_mimi_set_leveler
        assert _refused(eng, set_leveler, ms.handle, wide.handle, None, out.data_ptr(), 0) == \
            "set_leveler: the leveler's batch is not the state's"
        assert _refused(eng, set_leveler, ms.handle, narrow.handle, None, out.data_ptr(), 0) == \
            "set_leveler: the leveler's frame length is not the state's"
    finally:
        narrow.close()
        wide.close()
        ms.close()
