"""Pins tests/lm_ref.py and proves that the GPU matrix's bound (tests/test_gpu_lm_matrix.py: 8 E32) discriminates.
No GPU.

a. `LMRef` in float32 agrees with `oracle.np_oracle.FlowLM` (itself tied to the reference project's goldens by
   test_oracle_golden.py) on `tiny` and `en100m`: the cache after `prefill`, the layer stack's output of `backbone`, and
   the taps of `decode_step` up to the transformer output.  Both are float32 evaluations of the same formulas; LMRef's
   is within E32 of fp64 by E32's definition, the oracle's differs from it only in the order of BLAS sums (batched
   against per row), so |ref32 - oracle| <= ORACLE_FACTOR x E32 with ORACLE_FACTOR = 4 (one E32 for LMRef, three for the
   oracle's order).  Measured worst: 1.52 x E32 on tiny, 1.50 x E32 on en100m (the prefill's layer-0 K and V agree bit for bit).
b. Self-consistency of the state model in fp64, to 1e-12 relative: chunked = whole prefill, a ragged row = that row
   alone, a decode step = a one-token prefill of the same input, a parked row stays at position 0 and only ever rewrites
   slot 0 of its own cache (the library's contract, include/ptts.h).
c. Every seeded defect of `lm_ref.MUTANTS` moves at least one judged output of at least one case of the GPU matrix by
   >= 32 x E32 of that output: 4 times the GPU tolerance.  The 32 is a condition on the choice of cases, not a
   measurement.  A defect is run as a chain of its own over the same case; it is judged at the first call whose outputs
   it moves, i.e. the call that found the same float32 operands as the true chain."""

import numpy as np
import pytest

from lm_ref import CASES, MUTANTS, LMRef, RefDriver, evaluate, lm_e32, lm_weights
from oracle import np_oracle as O

GPU_FACTOR = 8            # test_gpu_lm_matrix.FACTOR
MUTANT_FACTOR = 4 * GPU_FACTOR
ORACLE_FACTOR = 4
RATIOS = {}               # (mutant, family) -> best ratio over the family's cases


# ------------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize("name", ["tiny", "en100m"])
def test_float32_reference_is_the_oracle(name):
    cfg, W = lm_weights(name)
    rng = np.random.default_rng(5)
    B, T, cap = 2, 11, 16
    lm = O.FlowLM(cfg, W)
    emb = (rng.standard_normal((B, T, lm.D)) * 0.5).astype(np.float32)
    lat = (rng.standard_normal((B, lm.ldim)) * 0.8).astype(np.float32)
    lat[0, :] = np.nan
    lat[1, 1::3] = np.nan
    last = f"flow_lm.transformer.layers.{lm.L - 1}:out"
    worst = 0.0

    def check(got, want, e32, what):
        nonlocal worst
        assert got.dtype == np.float32
        err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        worst = max(worst, err / e32)
        print(f"  {name} {what:12s} |ref32 - oracle| {err:.3e} = {err / e32:.2f} x E32 ({e32:.3e})")
        assert err <= ORACLE_FACTOR * e32, (what, err, e32)

    # prefill: the cache; backbone: the stack's output x (the tap of the last layer)
    ost = lm.init_state(B, cap)
    taps = {}
    lm.backbone(ost, emb, np.zeros((B, 0, lm.ldim), np.float32), taps)
    empty = LMRef(cfg, W, B, cap, np.float32).snapshot()
    op = ("prefill", emb, None)
    res, ref32 = evaluate(cfg, W, empty, op, np.float32)
    _, e32, ref64 = lm_e32(cfg, W, empty, op)
    assert list(ref32.off) == [T] * B == [s["offset"] for s in ost][:B]
    check(np.stack(res.x), taps[last], e32["x"], "prefill x")
    for l in range(lm.L):
        for j, kv in enumerate("KV"):
            check(ref32.kv[l][j][:, :T], ost[l]["cache"][j][:, :T], e32[f"{kv}{l}"], f"prefill {kv}{l}")
    # decode_step: BOS substitution, input_linear, the layers on top of the oracle's own cache
    snap = dict(kv=[np.nan_to_num(s["cache"]) for s in ost], off=np.full(B, T))
    taps = {}
    lm.decode_step(ost, lat, None, 1, -4.0, taps)
    op = ("decode", lat)
    res, ref32 = evaluate(cfg, W, snap, op, np.float32)
    _, e32, _ = lm_e32(cfg, W, snap, op)
    assert list(ref32.off) == [T + 1] * B
    check(np.stack(res.x), taps[last], e32["x"], "decode x")
    for l in range(lm.L):
        for j, kv in enumerate("KV"):
            check(ref32.kv[l][j][:, T:T + 1], ost[l]["cache"][j][:, T:T + 1], e32[f"{kv}{l}"], f"decode {kv}{l}")
    print(f"  {name}: worst |ref32 - oracle| = {worst:.2f} x E32 (bound {ORACLE_FACTOR})")


# ------------------------------------------------------------------------------------------------ b
def close(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= 1e-12 * max(1.0, float(np.abs(b).max())), float(np.abs(a - b).max())


def test_chunked_prefill_is_whole_prefill():
    cfg, W = lm_weights("tiny")
    rng = np.random.default_rng(1)
    emb = (rng.standard_normal((2, 42, 128)) * 0.3).astype(np.float32)
    whole, parts = LMRef(cfg, W, 2, 48), LMRef(cfg, W, 2, 48)
    rw = whole.prefill(emb)
    r1, r2 = parts.prefill(emb[:, :37]), parts.prefill(emb[:, 37:])
    assert list(parts.off) == list(whole.off) == [42, 42] and list(r2.start) == [37, 37]
    for b in range(2):
        close(np.concatenate([r1.x[b], r2.x[b]]), rw.x[b])
    for l in range(whole.L):
        close(parts.kv[l], whole.kv[l])


def test_ragged_row_is_that_row_alone():
    cfg, W = lm_weights("tiny")
    rng = np.random.default_rng(2)
    lengths = [0, 1, 16, 17, 20]
    emb = (rng.standard_normal((5, 20, 128)) * 0.3).astype(np.float32)
    for b, n in enumerate(lengths):
        emb[b, n:] = 1e6
    rag = LMRef(cfg, W, 5, 32)
    for l in range(rag.L):
        rag.kv[l][...] = 7.0
    res = rag.prefill(emb, lengths)
    assert list(rag.off) == lengths
    for b, n in enumerate(lengths):
        for l in range(rag.L):
            assert (rag.kv[l][:, b, n:] == 7.0).all()  # nothing at or beyond the row's length is written
        if n == 0:
            assert res.x[b].shape == (0, 128)
            continue
        alone = LMRef(cfg, W, 1, 32)
        ra = alone.prefill(emb[b:b + 1, :n])
        close(res.x[b], ra.x[0])
        for l in range(rag.L):
            close(rag.kv[l][:, b, :n], alone.kv[l][:, 0, :n])
            close(res.kv[l][b], ra.kv[l][0])


def test_decode_step_is_a_one_token_prefill():
    cfg, W = lm_weights("tiny")
    rng = np.random.default_rng(3)
    emb = (rng.standard_normal((3, 9, 128)) * 0.3).astype(np.float32)
    lat = (rng.standard_normal((3, 32)) * 0.8).astype(np.float32)
    lat[0, :] = np.nan
    lat[1, 1::3] = np.nan
    a, b = LMRef(cfg, W, 3, 16), LMRef(cfg, W, 3, 16)
    a.prefill(emb)
    b.prefill(emb)
    ra = a.decode(lat)
    bos = W["flow_lm.bos_emb"].astype(np.float64)
    seq = np.where(np.isnan(lat), bos[None, :], lat.astype(np.float64))
    assert np.array_equal(seq[0], bos) and (seq[1, 1::3] == bos[1::3]).all() and (seq[1, 0::3] == lat[1, 0::3]).all()
    rb = b.prefill((seq @ W["flow_lm.input_linear.weight"].astype(np.float64).T)[:, None, :])
    assert list(a.off) == list(b.off) == [10] * 3
    for r in range(3):
        close(ra.x[r], rb.x[r])
    for l in range(a.L):
        close(a.kv[l], b.kv[l])


def test_parked_row_stays_at_position_zero():
    cfg, W = lm_weights("tiny")
    rng = np.random.default_rng(4)
    st = LMRef(cfg, W, 3, 16)
    st.prefill((rng.standard_normal((3, 9, 128)) * 0.3).astype(np.float32))
    st.set_row_active(1, False)
    assert list(st.off) == [9, 0, 9]
    before = [k.copy() for k in st.kv]
    for step in range(3):
        lat = (rng.standard_normal((3, 32)) * 0.8).astype(np.float32)
        res = st.decode(lat)
        assert list(st.off) == [10 + step, 0, 10 + step] and list(res.start) == [9 + step, 0, 9 + step]
        alone = LMRef(cfg, W, 1, 16)  # the parked row computes what a fresh sequence computes at its first position
        ra = alone.decode(lat[1:2])
        close(res.x[1], ra.x[0])
        for l in range(st.L):
            assert np.array_equal(st.kv[l][:, 1, 1:], before[l][:, 1, 1:])  # only slot 0 of its cache is ever written
            close(st.kv[l][:, 1, 0], alone.kv[l][:, 0, 0])
    # un-parking by a copy gives the row a sequence again
    src = LMRef(cfg, W, 1, 16)
    src.prefill((rng.standard_normal((1, 5, 128)) * 0.3).astype(np.float32))
    st.copy_row(1, src)
    assert st.active.all() and list(st.off) == [12, 5, 12]
    st.decode((rng.standard_normal((3, 32)) * 0.8).astype(np.float32))
    assert list(st.off) == [13, 6, 13]


def test_import_reset_and_copy_bookkeeping():
    cfg, W = lm_weights("tiny")
    rng = np.random.default_rng(6)
    cache = rng.standard_normal((2, 1, 12, 2, 64)).astype(np.float32)
    st = LMRef(cfg, W, 3, 16)
    for l in range(st.L):
        st.import_cache(l, cache, 10)
    assert list(st.off) == [10] * 3 and all(np.array_equal(st.kv[0][:, b, :10], cache[:, 0, :10]) for b in range(3))
    assert (st.kv[0][:, :, 10:] == 0).all()
    st.reset()
    assert list(st.off) == [0] * 3 and np.array_equal(st.kv[1][:, 2, :10], cache[:, 0, :10])
    src = LMRef(cfg, W, 1, 16)
    src.prefill((rng.standard_normal((1, 7, 128)) * 0.3).astype(np.float32))
    st.copy_from(src)
    assert list(st.off) == [7] * 3 and np.array_equal(st.kv[1][:, 2, :7], src.kv[1][:, 0, :7])
    assert np.array_equal(st.kv[1][:, 2, 7:10], cache[:, 0, 7:10].astype(np.float64))  # beyond the copy: untouched


# ------------------------------------------------------------------------------------------------ c
# The mutation test runs the tiny cases of every family (en100m repeats them at K = 1024; its fp64 chains take seconds).
FAMILIES = [f for f in CASES if f != "cluster"]  # "cluster": the same cases on another kernel, the same reference
_TRUE = {}


def true_chain(family, cid):
    """the case on the unmutated reference: [(op, Written, E32 per output, offsets after)] of its judged calls"""
    if (family, cid) not in _TRUE:
        _, name, fn, args = next(c for c in CASES[family] if c[0] == cid)
        d = RefDriver(name)
        fn(d, *args)
        out = []
        for op, snap, res, off in d.calls:
            res64, e32, _ = lm_e32(d.cfg, d.W, snap, op)
            y, y64 = res.outputs(), res64.outputs()
            assert all(np.array_equal(y[k], y64[k]) for k in y)  # the chain's call IS the call judged on its operands
            out.append((op, y, e32, off))
        _TRUE[(family, cid)] = out
    return _TRUE[(family, cid)]


def mutant_ratio(mutant, family, cid):
    """worst moved / E32 over the outputs of the first judged call whose outputs the defect moves (0: none)"""
    _, name, fn, args = next(c for c in CASES[family] if c[0] == cid)
    d = RefDriver(name, mutate=mutant)
    fn(d, *args)
    truth = true_chain(family, cid)
    assert len(d.calls) == len(truth)
    for (_, _, res, _), (_, y, e32, _) in zip(d.calls, truth):
        ym = res.outputs()
        moved = {k: float(np.abs(ym[k] - y[k]).max()) for k in y}
        if max(moved.values()) > 0:
            return max(moved[k] / e32[k] for k in y)
    return 0.0


def tiny_cases(family):
    return [c[0] for c in CASES[family] if c[1] == "tiny"]


@pytest.mark.parametrize("family", FAMILIES)
def test_mutants_on_family(family):
    for mutant in MUTANTS:
        RATIOS[(mutant, family)] = max(mutant_ratio(mutant, family, cid) for cid in tiny_cases(family))
        print(f"  {mutant:11s} {family:9s} {RATIOS[(mutant, family)]:12.4g} x E32")


def test_zz_every_mutant_moves_a_judged_output():
    """the mutant x case-family table; every defect reaches 32 x E32 in at least one family"""
    assert sorted({m for m, _ in RATIOS}) == sorted(MUTANTS) and sorted({f for _, f in RATIOS}) == sorted(FAMILIES)
    print(f"\nseeded defects against the fp64 reference: worst moved / E32 of the first call moved (required: >= {MUTANT_FACTOR} in a family)")
    print(f"  {'mutant':11s}" + "".join(f" {f:>10s}" for f in FAMILIES))
    for m in MUTANTS:
        print(f"  {m:11s}" + "".join(f" {RATIOS[(m, f)]:10.3g}" for f in FAMILIES) + f"   {MUTANTS[m]}")
    for m in MUTANTS:
        best = max(RATIOS[(m, f)] for f in FAMILIES)
        assert best >= MUTANT_FACTOR, (m, best)
