"""The voice-prompt encoder against the fp64 stage references of tests/voice_ref.py, stage by stage, at the length edges,
through the public `Engine.encode_voice`.  `-m gpu`.

Per case: seeded noise of amplitude 0.2 (another seed per case) is encoded with the engine option `debug_taps` 1, every
intermediate is read back (`Engine.debug_read_encoder`) and every stage is judged ON THE INPUT THE KERNELS CONSUMED:

    max|gpu - y64| <= FACTOR * E32(stage)            FACTOR = 8

E32 is the loss of a plain float32 evaluation of the same formulas on the same inputs (voice_ref.stage_e32); it comes from
the reference, never from the kernels.  8, as for the Mimi decoder and the flow head: the kernels split K over waves and sum
in 4-wide MFMA chains, another order than numpy's.  The latent and the conditioning are also judged against the fp64 CHAIN
of all stages and that chain's own float32 error.  Every seeded defect of voice_ref.MUTANTS moves its stage by >= 32 E32
(tests/test_voice_reference_cpu.py), 4 x this bound.

The kernels that ran are asserted from the profiler's (site, kernel) records against the launches the geometry implies
(the dispatcher's static choice, or the pinned tile configuration where the shape admits it; the attention kernel's grid
with its number of key splits), so a silent fall-back to another kernel fails the case instead of passing it there.  The
worst ratio per (configuration, stage, kernel) is printed by the last test."""

import numpy as np
import pytest
import torch

import voice_ref as V
from conftest import synth_weights
from gemm_ref import CFG_NAME, CFG_SHAPE
from pocket_tts_amd._lib import PttsError
from pocket_tts_amd.weights import mimi_encode_spec

pytestmark = pytest.mark.gpu

FACTOR = 8
NCFG = len(CFG_NAME)
FRAME = V.FRAME
SWEEP_N = 2 * FRAME - 500  # 2 frames, ends inside the second
STATS = {}  # (config, stage, kernel labels) -> worst err / E32
SPLITS = {}  # (config, samples) -> key splits of the attention launches
COVER = {}  # config -> {site#round: tile configurations that ran there}
REFUSED = {}  # config -> {site#round: tile configurations the shape does not admit}
SWEEP_CASES = {}  # config -> tile configurations the sweep pinned
EPI_STORE, EPI_RES, EPI_QKV = 0, 1, 3  # csrc/ptts_kernels.h
PRE_NONE, PRE_LNFOLD = 0, 3
ACT_NONE, ACT_GELU, ACT_ELU = 0, 1, 3


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def cdiv(a, b):
    return -(-a // b)


def weights(name):
    return synth_weights(name) if name == "en100m" else V.codec_weights(name)


@pytest.fixture(scope="module")
def engines():
    """one engine per configuration for the whole module"""
    from pocket_tts_amd.engine import Engine

    cache = {}

    def get(name):
        if name not in cache:
            cfg, W = weights(name)
            cache[name] = (Engine(cfg, W, "cuda:0"), cfg, W)
        return cache[name]

    yield get
    for eng, _, _ in cache.values():
        eng.close()


# ---- what must have run ----------------------------------------------------------------------------------------------
def gemm_sites(cfg, n):
    """the encoder's GEMM launches of n samples in launch order: (site#round, (NT, KF, CF, ntaps, MT, epilogue, prologue,
    activation, xstride, halo_mode, raw copy, residual operand)), the first 12 integers of the dispatcher's tune_key"""
    sn, tr = cfg.mimi.seanet, cfg.mimi.transformer
    C, FF, nf = tr.d_model, tr.dim_feedforward, sn.n_filters
    frames = cdiv(n, FRAME)
    rows = frames * FRAME
    s = [("enc.conv0", (nf // 16, sn.kernel_size, 1, sn.kernel_size, rows // 16, EPI_STORE, PRE_NONE, ACT_ELU, 1, 1, 1, 0))]
    dim = nf
    for i, r in enumerate(reversed(sn.ratios), 1):
        hid, k3 = dim // sn.compress, sn.residual_kernel_size
        s.append((f"enc.res_a#{i}", (hid // 16, k3 * dim // 16, dim // 16, k3, rows // 16, EPI_STORE, PRE_NONE, ACT_ELU, 1, 1, 0, 0)))
        s.append((f"enc.res_b#{i}", (dim // 16, hid // 16, hid // 16, 1, rows // 16, EPI_RES, PRE_NONE, ACT_ELU, 1, 1, 0, 1)))
        rows //= r
        s.append((f"enc.down#{i}", (2 * dim // 16, 2 * r * dim // 16, dim // 16, 2 * r, rows // 16, EPI_STORE, PRE_NONE, ACT_ELU, r, 1, 1, 0)))
        dim *= 2
    k3, MT2 = sn.last_kernel_size, rows // 16
    assert rows == 16 * frames
    s.append(("enc.final", (C // 16, k3 * dim // 16, dim // 16, k3, MT2, EPI_STORE, PRE_NONE, ACT_NONE, 1, 1, 0, 0)))
    for l in range(tr.num_layers):
        s.append((f"enc.qkv#{l}", (3 * C // 16, C // 16, C // 16, 1, MT2, EPI_QKV, PRE_LNFOLD, ACT_NONE, 1, 0, 0, 0)))
        s.append((f"enc.out#{l}", (C // 16, C // 16, C // 16, 1, MT2, EPI_RES, PRE_NONE, ACT_NONE, 1, 0, 0, 1)))
        s.append((f"enc.ff1#{l}", (FF // 16, C // 16, C // 16, 1, MT2, EPI_STORE, PRE_LNFOLD, ACT_GELU, 1, 0, 0, 0)))
        s.append((f"enc.ff2#{l}", (C // 16, FF // 16, FF // 16, 1, MT2, EPI_RES, PRE_NONE, ACT_NONE, 1, 0, 0, 1)))
    st, ldim, D = cfg.upsample_stride, cfg.mimi.quantizer.dimension, cfg.flow_lm.transformer.d_model
    s.append(("enc.downsample", (ldim // 16, 2 * st * C // 16, C // 16, 2 * st, cdiv(frames, 16), EPI_STORE, PRE_NONE, ACT_NONE, st, 2, 0, 0)))
    s.append(("enc.speaker_proj", (D // 16, ldim // 16, ldim // 16, 1, cdiv(frames, 16), EPI_STORE, PRE_NONE, ACT_NONE, 1, 0, 0, 0)))
    return s


def pick_cfg(NT, KF, MT, epi):
    """the dispatcher's static choice (pick_cfg, csrc/ptts_dispatch.hip)"""
    tiled = cdiv(NT, 4) * cdiv(MT, 8)
    wide = 3 if NT >= 4 else 4 if NT >= 2 else 5
    if MT >= 256 and NT >= 4 and KF % 2 == 0 and epi != EPI_QKV:
        return 8 if NT >= 8 else 9
    if MT > 4 and tiled >= 192:
        return wide
    if MT >= 8 and NT >= 2 and KF >= 32 and cdiv(NT, 2) * cdiv(MT, 4) >= 128:
        return 7
    if MT > 64:
        return 6 if tiled < 192 else wide
    tm = 4 if MT >= 4 else 2 if MT >= 2 else 1
    while tm > 1 and NT * cdiv(MT, tm) < 256:
        tm >>= 1
    return {4: 2, 2: 1, 1: 0}[tm]


def admitted(c, NT, KF, MT):
    """cfg_valid (csrc/ptts_dispatch.hip) for fp32 weights and the encoder's prologues (none, folded LayerNorm)"""
    s = CFG_SHAPE[c]
    if s[2] == 0:  # LDS-staged: two k-fragments per stage
        return KF % 2 == 0 and MT >= s[1] and 2 * NT >= s[0]
    tn, tm = s[0] * s[3], s[1] * s[4]
    if (tm > 1 and tm > 2 * MT) or (tn > 1 and tn > 2 * NT):
        return False  # mostly padding
    return not (s[2] > 1 and KF < 2)  # something to split


def label_of(c, pre, NT, MT):
    s = CFG_SHAPE[c]
    if s[2] == 0:
        threads = cdiv(NT, s[0]) * cdiv(MT, s[1]) * 256
    else:
        threads = cdiv(NT, s[0] * s[3]) * cdiv(MT, s[1] * s[4]) * 64 * s[2] * s[3] * s[4]
    return f"{CFG_NAME[c]}{'+ln' if pre == PRE_LNFOLD else ''}@{threads}"


def attn_launch(cfg, n):
    """(key splits, label) of the encoder's attention launch: attn_nw, attn_splits and launch_attn_kernel of
    csrc/ptts_dispatch.hip for H heads x QB query blocks and a window of `context` keys"""
    tr = cfg.mimi.transformer
    QB = cdiv(n, FRAME)
    base = tr.num_heads * QB
    nw = 4 if base <= 128 else 2 if base <= 256 else 1
    tiles = cdiv(min(QB, cdiv(tr.context, 16) + 2), nw)
    splits = max(1, min(max(1, cdiv(1024, base * nw)), tiles))
    return splits, f"attn@{base * splits * 64 * nw}"


def expected_launches(name, cfg, n, pinned=None):
    """site#round -> the kernel labels of its launches; records which pinned configurations ran or were not admitted"""
    want = {}
    for site, (NT, KF, CF, ntaps, MT, epi, pre, *_rest) in gemm_sites(cfg, n):
        c = pick_cfg(NT, KF, MT, epi)
        if pinned is not None:
            ok = admitted(pinned, NT, KF, MT)
            (COVER if ok else REFUSED).setdefault(name, {}).setdefault(site, set()).add(pinned)
            c = pinned if ok else c
        want[site] = [label_of(c, pre, NT, MT)]
    splits, label = attn_launch(cfg, n)
    for l in range(cfg.mimi.transformer.num_layers):
        want[f"enc.attn#{l}"] = [label] + (["attn_combine"] if splits > 1 else [])
    return want


def check_kernels(prof, want):
    """the profiler's records are exactly the launches `want`, site by site"""
    by_site = {}
    for site, labels in want.items():
        by_site.setdefault(site.split("#")[0], []).extend(labels)
    got = {}
    for s, k in prof:
        got.setdefault(s, []).append(k)
    assert sorted(got) == sorted(by_site), (sorted(got), sorted(by_site))
    for site, labels in by_site.items():
        assert sorted(got[site]) == sorted(labels), (site, got[site], labels)


def stage_sites(cfg, stage):
    last = cfg.mimi.transformer.num_layers - 1
    tr = {"Q": ("qkv",), "A": ("qkv", "attn"), "T": ("qkv", "attn"), "B": ("out",), "C": ("ff1",), "D": ("ff2",)}
    if stage in tr:
        return [f"enc.{s}#{last}" for s in tr[stage]]
    if stage[:2] in ("Ra", "Rb", "Dn"):
        return [{"Ra": "enc.res_a", "Rb": "enc.res_b", "Dn": "enc.down"}[stage[:2]] + "#" + stage[2]]
    return [{"E0": "enc.conv0", "E0e": "enc.conv0", "F": "enc.final", "DS": "enc.downsample", "SP": "enc.speaker_proj"}[stage]]


def label_of_stage(cfg, want, stage):
    """the kernels of the stage's launches, without grid sizes"""
    return " ".join(want[s][0].split("@")[0] for s in stage_sites(cfg, stage))


# ---- running and judging --------------------------------------------------------------------------------------------------
def gpu(fn):
    """a HIP error ends the session: the device may be in any state, nothing more is started on it"""
    try:
        return fn()
    except (PttsError, RuntimeError) as e:
        pytest.exit(f"GPU error in the voice matrix, session ended: {e}", returncode=3)


def encode(eng, audio, taps):
    """-> latent and conditioning as returned, the profiler's (site, kernel) records and, with `taps`, every intermediate.
    `audio`: numpy samples, or a device tensor that is passed as it is"""
    def run():
        eng.set_option("debug_taps", int(taps))
        eng.profile_start()
        lat, cond = eng.encode_voice(dev(audio) if isinstance(audio, np.ndarray) else audio)
        prof = eng.profile_stop()
        torch.cuda.synchronize()
        out = dict(latent_out=lat.cpu().numpy(), cond_out=cond.cpu().numpy(),
                   prof=[(r["site"], r["kernel"]) for r in prof for _ in range(r["count"])])
        if taps:
            for name in V.TAPS:
                out[name] = eng.debug_read_encoder(name).cpu().numpy()
        eng.set_option("debug_taps", 0)
        return out

    return gpu(run)


def judge(name, cfg, W, enc, audio, want):
    """asserts shapes, finiteness and the bound for every stage, each against its OWN E32, then the whole chain; records
    STATS"""
    n, frames = len(audio), cdiv(len(audio), FRAME)
    tap = enc["audio"]
    assert tap.shape == (frames * FRAME, 16)
    assert np.array_equal(tap[:n, 0], audio) and not tap[n:, 0].any() and not tap[:, 1:].any()
    assert np.array_equal(enc["latent"], enc["latent_out"]) and np.array_equal(enc["cond"], enc["cond_out"])
    assert enc["latent_out"].shape == (frames, cfg.mimi.quantizer.dimension)
    assert enc["cond_out"].shape == (frames, cfg.flow_lm.transformer.d_model)
    worst = {}

    def ratio(stage, got, y64, e32):
        assert got.shape == y64.shape and np.isfinite(got).all(), (stage, got.shape, y64.shape)
        err = float(np.abs(got.astype(np.float64) - y64).max())
        label = label_of_stage(cfg, want, stage[6:] if stage.startswith("chain ") else stage)
        worst[(name, stage, label)] = err / e32
        print(f"  n={n:5d} {stage:9s} err {err:.3e}  E32 {e32:.3e}  ratio {err / e32:.2f}  {label}")

    for stage in V.stages_of(cfg):
        ratio(stage, enc[V.OUTPUT_TAP[stage]], *V.stage_e32(stage, V.stage_inputs(stage, cfg, W, enc, audio)))
    (lat64, e_lat), (cond64, e_cond) = V.chain_e32(cfg, W, audio)
    ratio("chain DS", enc["latent_out"], lat64, e_lat)
    ratio("chain SP", enc["cond_out"], cond64, e_cond)
    for key, v in worst.items():
        STATS[key] = max(STATS.get(key, 0.0), v)
    bad = {k: round(v, 2) for k, v in worst.items() if v > FACTOR}
    assert not bad, bad


def run_case(engines, name, n, pinned=None, case=()):
    eng, cfg, W = engines(name)
    audio = V.case_audio((name,) + case if case else name, n)
    enc = encode(eng, audio, taps=True)
    want = expected_launches(name, cfg, n, pinned)
    check_kernels(enc["prof"], want)
    judge(name, cfg, W, enc, audio, want)
    return enc


# the frame boundary; above the context of 40; whole key tiles outside the window; one and two row tiles of the downsample
@pytest.mark.parametrize("n", V.LENGTHS)
@pytest.mark.parametrize("name", V.CONFIG_NAMES)
def test_lengths(engines, name, n):
    run_case(engines, name, n)
    SPLITS[(name, n)] = attn_launch(engines(name)[1], n)[0]


def test_real_size(engines):
    """the 100M model's encoder at 17 frames: 272 positions, above the real context of 250, with the real channel widths"""
    n = V.LENGTHS[-1]
    run_case(engines, "en100m", n)
    SPLITS[("en100m", n)] = attn_launch(engines("en100m")[1], n)[0]


# ---- properties, bitwise ----------------------------------------------------------------------------------------------
def outputs(eng, audio, taps=False):
    e = encode(eng, audio, taps)
    return e["latent_out"], e["cond_out"], e["prof"]


@pytest.mark.parametrize("n", [1, FRAME - 1, 2 * FRAME + 700])
def test_zero_tail_equals_zero_extension(engines, n):
    """encode(a[:n]) is encode of a[:n] zero-extended to the next whole frame"""
    eng, cfg, _ = engines("tiny")
    a = V.case_audio("zero tail", n)
    lat, cond, _ = outputs(eng, a)
    lat2, cond2, _ = outputs(eng, np.concatenate([a, np.zeros((-n) % FRAME, np.float32)]))
    assert np.isfinite(lat).all() and np.array_equal(lat, lat2) and np.array_equal(cond, cond2)


@pytest.mark.parametrize("n", [1, FRAME - 1, 2 * FRAME + 700])
def test_nothing_behind_n_samples_is_read(engines, n):
    """the same audio as a view into a larger buffer whose other elements are 1e30"""
    eng, cfg, _ = engines("tiny")
    a = V.case_audio("view", n)
    lat, cond, _ = outputs(eng, a)
    big = dev(np.concatenate([a, np.full(2 * FRAME, 1e30, np.float32)]))
    view = big[:n]
    assert view.data_ptr() == big.data_ptr() and view.is_contiguous()
    lat2, cond2, _ = outputs(eng, view)
    assert np.isfinite(lat2).all() and np.array_equal(lat, lat2) and np.array_equal(cond, cond2)


@pytest.mark.parametrize("name", ["tiny", "nf64"])
def test_repeatable_and_taps_change_nothing(engines, name):
    """two calls are equal; `debug_taps` 0 and 1 give equal results and the same launches, those the geometry implies; without
    the option nothing is kept"""
    eng, cfg, _ = engines(name)
    n = 6 * FRAME
    a = V.case_audio((name, "repeat"), n)
    lat, cond, prof = outputs(eng, a)
    lat2, cond2, prof2 = outputs(eng, a)
    lat3, cond3, prof3 = outputs(eng, a, taps=True)
    assert np.array_equal(lat, lat2) and np.array_equal(cond, cond2) and np.array_equal(lat, lat3) and np.array_equal(cond, cond3)
    assert prof == prof2 == prof3
    check_kernels(prof, expected_launches(name, cfg, n))
    print(f"\n{name}: launches of one encode_voice of {n} samples with debug_taps 0")
    for s, k in prof:
        print(f"  {s:18s} {k}")
    outputs(eng, a)
    with pytest.raises(PttsError, match="debug_taps"):
        eng.debug_read_encoder("final")


# ---- every tile configuration at every encoder GEMM site ---------------------------------------------------------------
@pytest.mark.parametrize("c", range(NCFG))
@pytest.mark.parametrize("name", ["tiny", "nf64"])
def test_every_tile_configuration(engines, name, c):
    """the tuner's table is the one public route to a tile configuration (choose_cfg): a line per encoder GEMM shape, built
    from the geometry, pins configuration c.  The profiler must show c EXACTLY at the sites whose shape admits it
    (elsewhere choose_cfg falls back to the static choice), and every stage meets the bound"""
    eng, cfg, _ = engines(name)
    SWEEP_CASES.setdefault(name, set()).add(c)
    keys = dict.fromkeys(" ".join(map(str, key)) + " 0" for _, key in gemm_sites(cfg, SWEEP_N))  # wfmt 0: fp32 weights
    try:
        assert eng.tune_import("".join(f"{k} {c}\n" for k in keys)) == len(keys)
        run_case(engines, name, SWEEP_N, pinned=c, case=("cfg", c))
    finally:
        eng.tune_clear()


# ---- argument checks --------------------------------------------------------------------------------------------------
def test_argument_checks(engines):
    from pocket_tts_amd.engine import Engine

    eng, cfg, W = engines("tiny")
    with pytest.raises(PttsError, match="empty audio"):
        eng.encode_voice(torch.zeros(0, device="cuda:0"))
    optional = set(mimi_encode_spec(cfg))
    bare = gpu(lambda: Engine(cfg, {k: v for k, v in W.items() if k not in optional}, "cuda:0"))
    try:
        assert not bare.has_voice_encoder
        with pytest.raises(PttsError, match="error -3"):
            bare.encode_voice(dev(V.case_audio("bare", FRAME)))
    finally:
        bare.close()


def test_zz_error_table():
    """worst err / E32 per (configuration, stage, kernel) of this session; attention ran with one key split and with more;
    every GEMM site of a complete sweep ran under at least two tile configurations"""
    print(f"\nvoice encoder: worst max|gpu - y64| / E32 (bound {FACTOR})")
    for (name, stage, label), v in sorted(STATS.items()):
        print(f"  {name:6s} {stage:9s} {v:6.2f}  {label}")
    assert all(v <= FACTOR for v in STATS.values())
    print("  key splits of the attention launches:", {f"{k[0]}:{k[1]}": v for k, v in sorted(SPLITS.items())})
    if len([k for k in SPLITS if k[0] != "en100m"]) == len(V.CONFIG_NAMES) * len(V.LENGTHS):
        assert 1 in SPLITS.values() and max(SPLITS.values()) > 1, SPLITS
    for name, forced in SWEEP_CASES.items():
        for site in sorted(COVER.get(name, {})):
            print(f"  {name} {site:18s} ran {sorted(COVER[name][site])}  not admitted {sorted(REFUSED.get(name, {}).get(site, ()))}")
        if len(forced) == NCFG:  # a complete sweep
            sites = [s for s, _ in gemm_sites(weights(name)[0], SWEEP_N)]
            few = {s: sorted(COVER[name].get(s, ())) for s in sites if len(COVER[name].get(s, ())) < 2}
            assert not few, (name, few)
