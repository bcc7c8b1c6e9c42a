"""CPU-side checks of the ragged prefill: the padding helper and the C-ABI prototype of ptts_lm_prefill_ragged."""

import ctypes as C
import re
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parents[1]


def test_pad_token_rows_shapes_lengths_and_pad_id():
    from pocket_tts_amd.engine import pad_token_rows

    rows = [torch.tensor([[5, 6, 7]]), torch.tensor([9]), [3, 4], torch.zeros((1, 0), dtype=torch.long)]
    ids, lengths = pad_token_rows(rows)
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (4, 3) and lengths == [3, 1, 2, 0]
    assert ids.tolist() == [[5, 6, 7], [9, 0, 0], [3, 4, 0], [0, 0, 0]]
    ids, lengths = pad_token_rows(rows[:2], pad_id=2)
    assert ids.tolist() == [[5, 6, 7], [9, 2, 2]] and lengths == [3, 1]
    # equal lengths: nothing is padded; rows without a token still give one (padding) column, t_max >= 1
    ids, lengths = pad_token_rows([torch.tensor([1, 2]), torch.tensor([3, 4])])
    assert ids.tolist() == [[1, 2], [3, 4]] and lengths == [2, 2]
    ids, lengths = pad_token_rows([[], []])
    assert tuple(ids.shape) == (2, 1) and lengths == [0, 0]
    with pytest.raises(ValueError):
        pad_token_rows([])


def test_prototype_matches_the_header_line():
    from pocket_tts_amd._lib import PROTOTYPES

    header = (REPO / "include" / "ptts.h").read_text()
    m = re.search(r"^int ptts_lm_prefill_ragged\(([^;]*)\);", header, re.M)
    assert m, "ptts_lm_prefill_ragged is not declared in include/ptts.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["ptts_engine *e", "ptts_lm_state *s", "const float *d_emb", "const int32_t *h_len", "int32_t t_max",
                      "void *stream"]
    res, args = PROTOTYPES["ptts_lm_prefill_ragged"]
    assert res is C.c_int
    assert args == [C.c_void_p if "*" in p else C.c_int32 for p in params]
