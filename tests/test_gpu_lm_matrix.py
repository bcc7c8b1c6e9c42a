"""The FlowLM transformer backbone (embeddings or latents -> residual stream x and the KV cache) against the fp64
reference of tests/lm_ref.py, through the public engine calls only: prefill, chunked and ragged prefill, decode steps
(per-layer launches and the single-launch `lm_cluster` stack), rows at mixed positions with a parked row, positions
around 1000, and borrowed voice prefixes with and without the cascade kernel.  `-m gpu`.

Every judged call is judged on its own operands: the caches of all layers, the offsets and the active flags are read
back before the call (`export_layer`, `offsets`), the reference evaluates the same call from them in fp64, and for the
residual stream of the real rows (`debug_read` "prefill_x" / "x") and the K and V rows the call wrote at EVERY layer

    max|gpu - y64| <= FACTOR * E32(call, output)            FACTOR = 8

with E32 the loss of a plain float32 evaluation of the same call on the same operands (lm_ref.lm_e32: the larger of a
two-pass and a one-pass LayerNorm variance, RoPE frequencies and angles rounded to float32 as the reference project
does); it is computed from the reference, never from the kernels.  8 is the project's figure for kernels that differ from
numpy only in summation order (test_gpu_flow_matrix.py, test_gpu_mimi_matrix.py).  Every seeded defect of
lm_ref.MUTANTS moves a judged output of one of these cases by >= 32 E32 (tests/test_lm_reference_cpu.py), 4 x this bound.

Besides the bound, every call asserts: all outputs finite; offsets exact; every cache position the call did not write
bit-identical to what it was (all rows, layers, K and V, up to the capacity); `st.error()` false; and, from the
profiler's (site, kernel) records, the kernels that ran: `prep_in` at lm.prep (decode) or `rope_table` at lm.rope
(prefill), `+ln` and no weight-format suffix on lm.qkv and lm.ff1, the expected attention family at lm.attn, or one
`lm_cluster@` launch and no per-layer site at all.  A silent fall-back fails the case.  import / copy / park are checked
bit for bit against what they were given.

A parked row follows the library's contract (include/ptts.h): parking pins it to position 0, where it keeps flowing
through the kernels.  Its offset stays 0 and every slot of its cache but slot 0 is bit-identical from step to step; slot
0 and its x are what a sequence computes at its first position and are judged like every other row.

Measured worst max|gpu - y64| / E32 per (config, path, kernel at lm.attn) on an MI355X (bound 8):
  config  family    call     lm.attn            x      K      V
  en100m  cluster   decode   lm_cluster      0.85   1.03   0.83
  en100m  decode    decode   attn_decode     0.79   1.13   0.90
  en100m  prefill   prefill  attn            1.30   1.13   1.31
  tiny    bigpos    decode   attn_decode     1.01   1.01   1.73
  tiny    bigpos    prefill  attn            0.85   1.01   0.98
  tiny    borrowed  decode   attn_cascade    0.50   1.09   0.54
  tiny    borrowed  decode   attn_decode     0.91   1.09   1.41
  tiny    borrowed  prefill  attn            0.71   1.03   0.60
  tiny    chunked   prefill  attn            0.66   1.07   0.64
  tiny    cluster   decode   lm_cluster      1.43   1.21   2.17
  tiny    decode    decode   attn_decode     0.87   1.21   1.61
  tiny    mixed     decode   attn_decode     0.83   1.15   0.97
  tiny    prefill   prefill  attn            1.22   1.92   1.67
  tiny    prefill   prefill  attn_decode     1.36   1.30   1.07
  tiny    ragged    prefill  attn            0.61   0.89   0.47

(K, V: the worst layer.  "attn_decode" under prefill is the one-position prefill.)  The slowest case takes 0.7 s."""

import numpy as np
import pytest
import torch

from lm_ref import CASES, lm_e32, lm_weights

pytestmark = pytest.mark.gpu

FACTOR = 8
THR = -4.0
DEFAULTS = dict(share_prefix=1, prefix_cascade=1, lm_cluster=0)  # include/ptts.h, ptts_set_option
STATS = {}  # (config, family, call kind, kernel at lm.attn, output kind) -> worst err / E32
# every path of the matrix, as (family, call kind, kernel at lm.attn); the last test wants each seen on both configs it names
PATHS = {
    ("prefill", "prefill", "attn"): ("tiny", "en100m"), ("prefill", "prefill", "attn_decode"): ("tiny",),
    ("chunked", "prefill", "attn"): ("tiny",), ("ragged", "prefill", "attn"): ("tiny",),
    ("decode", "decode", "attn_decode"): ("tiny", "en100m"), ("mixed", "decode", "attn_decode"): ("tiny",),
    ("bigpos", "decode", "attn_decode"): ("tiny",), ("bigpos", "prefill", "attn"): ("tiny",),
    ("borrowed", "prefill", "attn"): ("tiny",), ("borrowed", "decode", "attn_decode"): ("tiny",),
    ("borrowed", "decode", "attn_cascade"): ("tiny",), ("cluster", "decode", "lm_cluster"): ("tiny", "en100m"),
}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


@pytest.fixture(scope="module")
def engines():
    """one engine per config for the whole module"""
    from pocket_tts_amd.engine import Engine

    cache = {}

    def get(name):
        if name not in cache:
            cfg, W = lm_weights(name)
            cache[name] = Engine(cfg, W, "cuda:0")
        return cache[name]

    yield get
    for eng in cache.values():
        eng.close()


def pre_of(kernel):
    """prologue / weight-format suffixes of a GEMM label "<cfg>+a+b@threads" """
    return kernel.split("@")[0].split("+")[1:]


def check_kernels(prof, kind, attn, L, suffix=(None, None)):
    """the kernels of the backbone that ran are those of the expected path.  `suffix`: the weight-format suffix of the
    attention Linears (lm.qkv, lm.out) and of the FFN Linears (lm.ff1, lm.ff2); None: fp32 weights"""
    at = lambda site: [(k, n) for s, k, n in prof if s == site]  # noqa: E731
    count = lambda site: sum(n for _, n in at(site))  # noqa: E731
    fmt = {"lm.qkv": suffix[0], "lm.out": suffix[0], "lm.ff1": suffix[1], "lm.ff2": suffix[1]}
    for s, k, _ in prof:
        if s.startswith("lm."):
            assert {"q8", "b16", "split"} & set(pre_of(k)) == {fmt.get(s)} - {None}, (s, k)
    if kind == "decode":
        assert at("lm.prep") == [("prep_in", 1)] and not at("lm.rope") and not at("lm.in_linear"), prof
    else:
        assert at("lm.rope") == [("rope_table", 1)] and not at("lm.prep"), prof
    if attn == "lm_cluster":
        assert len(at("lm.cluster")) == 1 and at("lm.cluster")[0][0].startswith("lm_cluster@") and count("lm.cluster") == 1, prof
        for site in ("lm.qkv", "lm.attn", "lm.out", "lm.ff1", "lm.ff2"):
            assert not at(site), prof
        return
    assert not at("lm.cluster"), prof
    sites = {"lm.prep" if kind == "decode" else "lm.rope", "lm.qkv", "lm.attn", "lm.out", "lm.ff1", "lm.ff2"}
    assert {s for s, _, _ in prof if s.startswith("lm.")} == sites, prof
    for site, pre in (("lm.qkv", ["ln"]), ("lm.out", []), ("lm.ff1", ["ln"]), ("lm.ff2", [])):
        want = pre + ([fmt[site]] if fmt[site] else [])
        assert count(site) == L and all(pre_of(k) == want for k, _ in at(site)), (site, prof)
    fam = [(k.split("@")[0], n) for k, n in at("lm.attn") if not k.startswith("attn_combine")]
    assert {f for f, _ in fam} == {attn} and sum(n for _, n in fam) == L, (attn, prof)


class State:
    def __init__(self, st, B, cap):
        self.st, self.B, self.cap = st, B, cap
        self.off = np.zeros(B, np.int64)      # host mirror of what the offsets must be
        self.active = np.ones(B, bool)


class GpuDriver:
    """lm_ref's driver interface on the engine: runs each call, judges it against the reference on its own operands"""

    def __init__(self, eng, name, family):
        self.eng, self.name, self.family = eng, name, family
        self.cfg, self.W = lm_weights(name)
        self.D, self.H, self.L, self.ldim = eng.D, eng.H, eng.L, eng.ldim
        self.open, self.worst, self.changed = [], {}, False

    # ---- states and bookkeeping
    def new(self, B, cap):
        assert cap % 16 == 0
        s = State(self.eng.new_lm_state(B, cap), B, cap)
        self.open.append(s)
        return s

    def close(self, s):
        s.st.close()
        self.open.remove(s)

    def options(self, **kw):
        self.changed = True
        for k, v in kw.items():
            self.eng.set_option(k, v)

    def finish(self):
        for s in list(self.open):
            self.close(s)
        if self.changed:
            for k, v in DEFAULTS.items():
                self.eng.set_option(k, v)

    def export(self, s):
        return [s.st.export_layer(l, s.cap).cpu().numpy() for l in range(self.L)]

    def offsets_are(self, s):
        assert list(s.st.offsets()) == list(s.off), (list(s.st.offsets()), list(s.off))

    def import_cache(self, s, caches, t):
        for l, c in enumerate(caches):
            s.st.import_layer(l, torch.from_numpy(c), t)
        s.off[:] = t
        self.offsets_are(s)
        for got, c in zip(self.export(s), caches):
            want = np.ascontiguousarray(np.broadcast_to(c[:, :, :t], got[:, :, :t].shape))
            assert np.array_equal(np.ascontiguousarray(got[:, :, :t]).view(np.uint32), want.view(np.uint32))

    def reset(self, s):
        s.st.reset()
        s.off[:] = 0
        s.active[:] = True
        self.offsets_are(s)

    def _copied(self, s, rows, src, before):
        """the rows hold the source's sequence bit for bit, at its length; every other row is what it was"""
        want, got = self.export(src), self.export(s)
        for l in range(self.L):
            for b in range(s.B):
                if b in rows:
                    T = int(src.off[rows[b]])
                    assert np.array_equal(got[l][:, b, :T].view(np.uint32), want[l][:, rows[b], :T].view(np.uint32)), (l, b)
                else:
                    assert np.array_equal(got[l][:, b].view(np.uint32), before[l][:, b].view(np.uint32)), (l, b)

    def copy_from(self, s, src):
        before = self.export(s)
        s.st.copy_from(src.st)
        rows = {b: 0 if src.B == 1 else b for b in range(s.B)}
        for b, sb in rows.items():
            s.off[b] = src.off[sb]
        self.offsets_are(s)
        self._copied(s, rows, src, before)

    def copy_row(self, s, row, src, src_row=0):
        before = self.export(s)
        s.st.copy_row_from(row, src.st, src_row)
        s.off[row], s.active[row] = src.off[src_row], True
        self.offsets_are(s)
        self._copied(s, {row: src_row}, src, before)

    def park(self, s, row):
        before = self.export(s)
        s.st.set_row_active(row, False)
        s.off[row], s.active[row] = 0, False
        self.offsets_are(s)
        # the other rows are what they were; the parked row's sequence is given up (a prefix it borrowed is released), what
        # its cache holds from here on is the baseline the steps are compared with
        rows = [b for b in range(s.B) if b != row]
        for a, b in zip(self.export(s), before):
            assert np.array_equal(a[:, rows].view(np.uint32), b[:, rows].view(np.uint32))

    # ---- the calls that are judged
    def prefill(self, s, emb, lengths=None, judge=True, attn="attn"):
        self._call(s, ("prefill", emb, lengths), judge, attn)

    def decode(self, s, latent_in, attn="attn_decode"):
        self._call(s, ("decode", latent_in), True, attn)

    def _call(self, s, op, judge, attn):
        eng, kind, B = self.eng, op[0], s.B
        self.offsets_are(s)
        before = self.export(s)
        snap = dict(kv=before, off=s.off.copy(), active=s.active.copy())
        eng.profile_start()
        try:
            if kind == "prefill":
                T = op[1].shape[1]
                n = np.full(B, T) if op[2] is None else np.asarray(op[2])
                eng.lm_prefill(s.st, dev(op[1]), None if op[2] is None else [int(v) for v in op[2]])
                grow = n
            else:
                n, grow = np.ones(B, np.int64), s.active.astype(np.int64)
                eng.lm_decode_step(s.st, dev(op[1]), dev(np.zeros((B, self.ldim), np.float32)), 1, THR)
        finally:
            prof = [(r["site"], r["kernel"], r["count"]) for r in eng.profile_stop()]
        torch.cuda.synchronize()
        assert not s.st.error()
        if kind == "prefill":
            x = eng.debug_read(s.st, "prefill_x").cpu().numpy()[:B * T].reshape(B, T, self.D)
        else:
            x = eng.debug_read(s.st, "x").cpu().numpy()[:B].reshape(B, 1, self.D)
        after = self.export(s)
        start = s.off.copy()
        s.off += grow
        self.offsets_are(s)
        if n.any():
            self.check_kernels(prof, kind, attn)
        else:
            assert not [r for r in prof if r[0].startswith("lm.")], prof
        # every position the call did not write is bit-identical
        wrote = np.zeros((B, s.cap), bool)
        for b in range(B):
            wrote[b, start[b]:start[b] + n[b]] = True
        for l in range(self.L):
            same = after[l].view(np.uint32) == before[l].view(np.uint32)
            assert same[:, ~wrote].all(), (l, np.argwhere(~same & ~wrote[None, :, :, None, None])[:4])
        if not judge:
            return
        got = {"x": np.concatenate([x[b, :n[b]].reshape(-1) for b in range(B)])}
        for l in range(self.L):
            for j, name in enumerate("KV"):
                got[f"{name}{l}"] = np.concatenate([after[l][j, b, start[b]:start[b] + n[b]].reshape(-1) for b in range(B)])
        self.judge(s, snap, op, attn, got, start, n)

    def check_kernels(self, prof, kind, attn):
        check_kernels(prof, kind, attn, self.L)

    def judge(self, s, snap, op, attn, got, start, n):
        """the call's outputs `got` (as Written.outputs() names them) against the reference on the operands `snap`"""
        kind, B = op[0], s.B
        res64, e32, ref64 = lm_e32(self.cfg, self.W, snap, op)
        assert list(ref64.off) == list(s.off) and list(res64.start) == list(start) and list(res64.n) == list(n)
        y64 = res64.outputs()
        ratios = {}
        for name, ref in y64.items():
            g = got[name]
            assert g.shape == ref.shape and np.isfinite(g).all(), name
            assert e32[name] > 0
            ratios[name] = float(np.abs(g.astype(np.float64) - ref).max()) / e32[name]
        line = " ".join(f"{k} {v:.2f}" for k, v in ratios.items())
        print(f"  {self.name} {self.family} {kind} B={B} n={int(n.max())} at {int(start.max())} [{attn}]: {line}")
        for name, r in ratios.items():
            key = (self.name, self.family, kind, attn, name[0])
            STATS[key] = max(STATS.get(key, 0.0), r)
            self.worst[name] = max(self.worst.get(name, 0.0), r)


def run_case(engines, family, cid):
    _, name, fn, args = next(c for c in CASES[family] if c[0] == cid)
    d = GpuDriver(engines(name), name, family)
    try:
        fn(d, *args)
    finally:
        d.finish()
    assert d.worst and all(v <= FACTOR for v in d.worst.values()), {k: round(v, 2) for k, v in d.worst.items() if v > FACTOR}


def ids(family):
    return [c[0] for c in CASES[family]]


@pytest.mark.parametrize("cid", ids("prefill"))
def test_prefill_from_empty(engines, cid):
    run_case(engines, "prefill", cid)


@pytest.mark.parametrize("cid", ids("chunked"))
def test_chunked_prefill(engines, cid):
    run_case(engines, "chunked", cid)


def test_ragged_prefill(engines):
    """lengths [0, 1, 16, 17, 20] of 20 with padding around 1e6 over a cache holding a pattern, a second ragged chunk on top"""
    run_case(engines, "ragged", "tiny")


@pytest.mark.parametrize("cid", ids("decode"))
def test_decode(engines, cid):
    run_case(engines, "decode", cid)


def test_mixed_positions_and_a_parked_row(engines):
    run_case(engines, "mixed", "tiny")


def test_large_positions(engines):
    run_case(engines, "bigpos", "tiny")


@pytest.mark.parametrize("cid", ids("borrowed"))
def test_borrowed_prefix(engines, cid):
    run_case(engines, "borrowed", cid)


@pytest.mark.parametrize("cid", ids("cluster"))
def test_single_launch_stack(engines, cid):
    run_case(engines, "cluster", cid)


def test_zz_error_table_and_coverage():
    """worst err / E32 per (config, path, kernel) of this session, and every path of the matrix seen"""
    print(f"\nFlowLM backbone: worst max|gpu - y64| / E32 (bound {FACTOR})")
    print(f"  {'config':7s} {'family':9s} {'call':8s} {'lm.attn':13s} {'x':>6s} {'K':>6s} {'V':>6s}")
    for key in sorted({k[:4] for k in STATS}):
        print(f"  {key[0]:7s} {key[1]:9s} {key[2]:8s} {key[3]:13s}" + "".join(f" {STATS[key + (o,)]:6.2f}" for o in "xKV"))
    seen = {k[:4] for k in STATS}
    missing = [(name,) + path for path, names in PATHS.items() for name in names if (name,) + path not in seen]
    assert not missing, missing
    assert all(v <= FACTOR for v in STATS.values())
