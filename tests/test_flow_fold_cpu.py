"""Host side of the flow fold (csrc/ptts_flow.h, flow_cluster_mod_kernel), without a GPU: the exchange-slot offsets and the
table of modulation tiles, through the two C-ABI calls that wrap the very functions the kernel and the allocation use
(`flow_slot`, `flow_mod_tiles`)."""

import ctypes as C

import numpy as np
import pytest

NF = 3  # FLOW_MOD_FRAGS: layer output, shift, scale


@pytest.fixture(scope="module")
def lib():
    from pocket_tts_amd import _lib

    _lib.build()
    return _lib.load()


def enumerate_slots(lib, fdf, rt, nph, nf, ng):
    return np.array([lib.ptts_flow_slot_offset(fdf, rt, nph, nf, g, p, t, j, f)
                     for g in range(ng) for p in range(nph) for t in range(rt) for j in range(fdf) for f in range(nf)],
                    dtype=np.int64)


@pytest.mark.parametrize("fdf", [4, 12, 16, 32])
def test_slots_are_dense_and_disjoint(lib, fdf):
    """Every (row group, phase, row tile, producer, fragment) owns its own 256 floats; in the nested order of that tuple
    the slots are back to back, so the buffer size the allocation asks for, offset(ng, 0, 0, 0, 0), is exactly their sum."""
    depth, rt = 2, 1
    for steps in range(1, 5):
        nph = steps * (2 * depth + 2)
        for ng in range(1, 8):
            off = enumerate_slots(lib, fdf, rt, nph, NF, ng)
            assert np.array_equal(off, 256 * np.arange(ng * nph * rt * fdf * NF)), (fdf, steps, ng)
            assert lib.ptts_flow_slot_offset(fdf, rt, nph, NF, ng, 0, 0, 0, 0) == 256 * off.size
    # the unfolded kernel's layout [NG][phases][RT][FDF][256] is the same function with one fragment per slot
    off = enumerate_slots(lib, fdf, 2, 6, 1, 3)
    assert np.array_equal(off, 256 * np.arange(3 * 6 * 2 * fdf))


def test_slots_at_the_flagship_shape(lib):
    """flow_dim 512, depth 6, one LSD step, 4 row groups: no overlap, and a group's slots fit the 2 GiB a buffer resource
    addresses with 32-bit offsets even at 64 LSD steps"""
    off = enumerate_slots(lib, 32, 1, 14, NF, 4)
    assert len(set(off.tolist())) == off.size and off.min() == 0 and off.max() == 256 * (off.size - 1)
    assert 4 * lib.ptts_flow_slot_offset(32, 1, 64 * 14, NF, 1, 0, 0, 0, 0) < 0x7FFFFFF0


def chunks(fdf, depth):
    """name -> first 16-column tile, from the reference's own chunking of the AdaLN outputs (tests/flow_ref.py:139,144:
    np.split(.., 3) -> shift, scale, gate per block, np.split(.., 2) -> shift, scale of the final layer), concatenated in
    the order the engine packs them: blocks 0 .. depth - 1, then the final layer"""
    FD = 16 * fdf
    col = np.arange((3 * depth + 2) * FD)
    out = {}
    for r in range(depth):
        shift, scale, gate = np.split(col[r * 3 * FD:(r + 1) * 3 * FD], 3, axis=-1)
        out[("shift", r)], out[("scale", r)], out[("gate", r)] = shift, scale, gate
    shift, scale = np.split(col[depth * 3 * FD:], 2, axis=-1)
    out[("shift", depth)], out[("scale", depth)] = shift, scale
    return out


@pytest.mark.parametrize("fdf,depth", [(4, 2), (12, 2), (16, 2), (32, 6), (8, 1)])
def test_tile_table_matches_the_reference_chunking(lib, fdf, depth):
    ref = chunks(fdf, depth)
    pps = 2 * depth + 2
    for j in range(fdf):
        seen = []
        for ph in range(pps):
            n = C.c_int32(-1)
            t0 = lib.ptts_flow_mod_tiles(fdf, depth, ph, j, C.byref(n))
            if ph == 0:
                want = [("shift", 0), ("scale", 0)]
            elif ph == pps - 1:
                want = []
            elif (ph - 1) % 2 == 0:  # a block's first linear: its own gate, used by the next phase's epilogue
                want = [("gate", (ph - 1) // 2)]
            else:                    # a block's second linear: the next LayerNorm's shift and scale
                want = [("shift", (ph - 1) // 2 + 1), ("scale", (ph - 1) // 2 + 1)]
            assert n.value == len(want), (ph, j)
            for s, key in enumerate(want):
                tile = t0 + s * fdf
                assert np.array_equal(ref[key][16 * j:16 * j + 16], np.arange(16 * tile, 16 * tile + 16)), (ph, j, key)
            seen += want
        # every vector's tile j exactly once per LSD step: 2 + depth * (1 + 2) tiles
        assert sorted(seen) == sorted(ref) and len(seen) == 2 + 3 * depth
