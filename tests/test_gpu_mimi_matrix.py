"""The fp32 Mimi decoder against the fp64 stage references of tests/mimi_ref.py, stage by stage, on every kernel path, through
the public `Engine.mimi_decode`.  `-m gpu`.

Per case: a fresh state decodes 6 frames of seeded latents (different per frame and sequence) with the engine option
`debug_taps` 1.  "tiny" has context 40 and a ring of 64 slots, so 6 frames cover the zero-carry first frame, the window
dropping keys (from position 40, in frame 2) and the ring wrapping (frame 4).  After each frame every tap is read back
(`Engine.debug_read`) and every stage is judged ON THE INPUT THE KERNELS CONSUMED (this frame's input tap, the previous
frame's tail):

    max|gpu - y64| <= FACTOR * E32(stage, frame)            FACTOR = 8

E32 is the loss of a plain float32 evaluation of the same formulas on the same inputs (mimi_ref.stage_e32); it comes from
the reference, never from the kernels.  8, as for the flow head: the kernels split K over waves and sum in 4-wide MFMA
chains, another order than numpy's.  Every seeded defect of mimi_ref.MUTANTS moves its stage by >= 32 E32
(tests/test_mimi_reference_cpu.py), 4 x this bound.

The kernels that ran are asserted from the profiler's (site, kernel) records, so a silent fall-back to another kernel or
tile configuration fails the case instead of passing it there.  The worst ratio per (configuration, stage, kernel) is
printed by the last test."""

import zlib

import numpy as np
import pytest
import torch

import mimi_ref as R
from gemm_ref import CFG_NAME, CFG_SHAPE
from pocket_tts_amd._lib import PttsError

pytestmark = pytest.mark.gpu

FACTOR = 8
FRAMES = 6
NCFG = len(CFG_NAME)
TAPS = ("upsample", "tr_attn", "tr_resid", "tr_ff", "dec_tr", "seanet0", "seanet2", "seanet3", "seanet5", "seanet6",
        "seanet8", "seanet9")
DEFAULTS = dict(fuse_res=1, single_store=1, fuse_pcm=1, debug_taps=0)  # opt_* in csrc/ptts_host.h
STATS = {}  # (config, stage, kernel label) -> worst err / E32
SWEPT = {}  # config -> tile configurations that ran at some site of the sweep
SWEEP_CASES = {}  # config -> tile configurations the sweep forced


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def cdiv(a, b):
    return -(-a // b)


def seed_of(*case):
    return zlib.crc32(repr(case).encode())


@pytest.fixture(scope="module")
def engines():
    """one engine per configuration for the whole module"""
    from pocket_tts_amd.engine import Engine

    cache = {}

    def get(name):
        if name not in cache:
            cfg, W = R.codec_weights(name)
            cache[name] = (Engine(cfg, W, "cuda:0"), cfg, W)
        return cache[name]

    yield get
    for eng, _, _ in cache.values():
        eng.close()


# ---- what must have run ----------------------------------------------------------------------------------------------
def seanet_dims(cfg):
    """per stage i = 1..3: (cin, cout, hid, ratio, rows in, rows out) per sequence"""
    sn = cfg.mimi.seanet
    out, mult, rows = [], 8, 16
    for r in sn.ratios:
        cin = mult * sn.n_filters
        out.append((cin, cin // 2, cin // 2 // sn.compress, r, rows, rows * r))
        rows *= r
        mult //= 2
    return out


def fusable(cfg, i, B):
    """resblock_fusable (csrc/ptts_dispatch.hip): (hidden, out) column tiles (2, 4) or (4, 8), at least 4 row tiles"""
    _, cout, hid, _, _, rows = seanet_dims(cfg)[i - 1]
    return (hid // 16, cout // 16) in ((2, 4), (4, 8)) and B * rows // 16 >= 4


def pre_of(kernel):
    """prologue / weight-format suffixes of a label "<kernel>+a+b@threads" """
    return kernel.split("@")[0].split("+")[1:]


def at(prof, site):
    return [k for s, k in prof if s == site]


def check_kernels(prof, cfg, B, opts):
    """each seanet.* / mimi.* site ran the kernel the options imply (fp32 weights everywhere)"""
    for s, k in prof:
        assert not {"q8", "b16", "split"} & set(pre_of(k)), (s, k)
    L = cfg.mimi.transformer.num_layers
    assert at(prof, "mimi.prologue") == ["mimi_prologue"], prof
    for site, pre in (("mimi.qkv", ["ln"]), ("mimi.out", []), ("mimi.ff1", ["ln"]), ("mimi.ff2", [])):
        got = at(prof, site)
        assert len(got) == L and all(k.startswith("gemm") and pre_of(k) == pre for k in got), (site, got)
    assert len(at(prof, "mimi.attn")) >= L, prof
    assert len(at(prof, "seanet.conv0")) == 1 and pre_of(at(prof, "seanet.conv0")[0]) == [], prof
    single = ["elu"] if opts["single_store"] else []
    fused_pcm = False
    for i in (1, 2, 3):
        _, cout, hid, _, _, rows = seanet_dims(cfg)[i - 1]
        ct, ra, rb = (at(prof, f"seanet.{s}{i}{x}") for s, x in (("convtr", ""), ("res", "a"), ("res", "b")))
        assert len(ct) == 1 and ct[0].startswith("gemm") and pre_of(ct[0]) == [], (i, ct)
        if opts["fuse_res"] and fusable(cfg, i, B):
            want = f"resblock<{hid // 16},{cout // 16}>" + "".join("+" + p for p in single) + f"@{cdiv(B * rows // 16, 4) * 256}"
            assert ra == [want] and rb == [], (i, want, ra, rb)
            fused_pcm = fused_pcm or (i == 3 and bool(opts["fuse_pcm"]) and hid == 32 and rows % 64 == 0)
        else:
            assert len(ra) == 1 and ra[0].startswith("gemm") and pre_of(ra[0]) == single, (i, ra)
            assert len(rb) == 1 and rb[0].startswith("gemm") and pre_of(rb[0]) == [], (i, rb)
    last = at(prof, "seanet.conv_last")
    assert len(last) == 1, prof
    if fused_pcm:
        assert last[0] == "pcm_fix", last
    elif cfg.mimi.seanet.n_filters == 64:
        assert last[0] == "pcm_conv", last
    else:
        assert last[0].startswith("gemm") and pre_of(last[0]) == [], last
    return fused_pcm


STAGE_SITES = {"P": ("mimi.prologue",), "A": ("mimi.qkv", "mimi.attn"), "T": ("mimi.qkv", "mimi.attn"), "B": ("mimi.out",),
               "C": ("mimi.ff1",), "D": ("mimi.ff2",), "S0": ("seanet.conv0",), "L": ("seanet.conv_last",),
               "R3L": ("seanet.res3a", "seanet.conv_last"),
               **{f"C{i}": (f"seanet.convtr{i}",) for i in (1, 2, 3)},
               **{f"R{i}": (f"seanet.res{i}a", f"seanet.res{i}b") for i in (1, 2, 3)}}


def label_of_stage(prof, stage):
    """the kernels of the stage's sites, without grid sizes (the last layer's for the transformer's sites)"""
    names = []
    for site in STAGE_SITES[stage]:
        got = at(prof, site)
        if got:
            names.append(got[-1].split("@")[0])
    return " ".join(names)


# ---- running and judging --------------------------------------------------------------------------------------------------
def decode_frames(eng, cfg, B, latents, opts, resets=(), i16=False):
    """-> one dict per frame: latent, PCM, every readable tap as [B, T, C], the profiler's (site, kernel) records and,
    with i16, the int16 PCM.  A HIP error ends the session: the device may be in any state, nothing more is started"""
    taps = [t for t in TAPS if opts["debug_taps"] or t in ("upsample", "seanet8")]
    for k, v in opts.items():
        eng.set_option(k, v)
    ms = eng.new_mimi_state(B)
    try:
        frames = _decode(eng, ms, B, latents, taps, resets, i16)
    except (PttsError, RuntimeError) as e:
        pytest.exit(f"GPU error in the Mimi matrix, session ended: {e}", returncode=3)
    ms.close()
    for k, v in DEFAULTS.items():
        eng.set_option(k, v)
    return frames


def _decode(eng, ms, B, latents, taps, resets, i16):
    frames = []
    buf = torch.zeros((B, eng.frame_samples), dtype=torch.int16, device="cuda:0") if i16 else None
    if i16:
        ms.set_pcm_i16(buf)
    for f, lat in enumerate(latents):
        for fr, row in resets:
            if fr == f:
                ms.reset_row(row)
        eng.profile_start()
        pcm = eng.mimi_decode(ms, dev(lat))
        prof = eng.profile_stop()
        torch.cuda.synchronize()
        t = dict(latent=lat, pcm=pcm.cpu().numpy(), prof=[(r["site"], r["kernel"]) for r in prof for _ in range(r["count"])])
        for name in taps:
            x = eng.debug_read(ms, name).cpu().numpy()
            t[name] = x.reshape(B, x.shape[0] // B, x.shape[1])
        if i16:
            t["pcm_i16"] = buf.cpu().numpy().copy()
        frames.append(t)
    return frames


def stages_of(name, cfg):
    one = cfg.mimi.transformer.num_layers == 1
    return ["P"] + (["A", "B"] if one else ["T"]) + ["C", "D", "S0", "C1", "R1", "C2", "R2", "C3", "R3", "L"] + \
        (["R3L"] if name == "nf64" else [])


def starts_of(B, f, resets):
    start = np.zeros(B, np.int64)
    for fr, row in resets:
        if fr <= f:
            start[row] = fr
    return start


def judge(name, cfg, W, frames, stages, resets=()):
    """asserts finiteness and the bound for every stage of every frame, each against its OWN E32; records STATS"""
    B = frames[0]["latent"].shape[0]
    worst = {}
    for f, fr in enumerate(frames):
        for stage in stages:
            got = fr[R.OUTPUT_TAP[stage]]
            y64, e32 = R.stage_e32(stage, R.stage_inputs(stage, cfg, W, frames, f, starts_of(B, f, resets)))
            assert got.shape == y64.shape and np.isfinite(got).all(), (stage, f, got.shape, y64.shape)
            err = float(np.abs(got.astype(np.float64) - y64).max())
            key = (name, stage, label_of_stage(fr["prof"], stage))
            worst[key] = max(worst.get(key, 0.0), err / e32)
            print(f"  frame {f} {stage:3s} err {err:.3e}  E32 {e32:.3e}  ratio {err / e32:.2f}  {key[2]}")
    for key, v in worst.items():
        STATS[key] = max(STATS.get(key, 0.0), v)
    bad = {k: round(v, 2) for k, v in worst.items() if v > FACTOR}
    assert not bad, bad
    return worst


def run_case(engines, name, B, opts=None, resets=(), i16=False, scale=1.0, case=()):
    eng, cfg, W = engines(name)
    opts = {**DEFAULTS, "debug_taps": 1, **(opts or {})}
    latents = R.seeded_latents(cfg, FRAMES, B, seed_of(name, B, sorted(opts.items()), resets, case), scale)
    frames = decode_frames(eng, cfg, B, latents, opts, resets, i16)
    for fr in frames:
        check_kernels(fr["prof"], cfg, B, opts)
    judge(name, cfg, W, frames, stages_of(name, cfg), resets)
    return frames


# one row tile; partial tiles; MT 5 with 30 row tiles in stage 1; sequence boundaries inside and across 64-row tiles
@pytest.mark.parametrize("B", [1, 3, 5, 17])
@pytest.mark.parametrize("name", R.CONFIG_NAMES)
def test_batches(engines, name, B):
    run_case(engines, name, B)


OPTIONS = {"fuse_res0": dict(fuse_res=0), "single_store0": dict(single_store=0), "fuse_pcm0": dict(fuse_pcm=0),
           "all_off": dict(fuse_res=0, single_store=0, fuse_pcm=0)}


@pytest.mark.parametrize("opt", sorted(OPTIONS))
@pytest.mark.parametrize("name", R.CONFIG_NAMES)
def test_options(engines, name, opt):
    run_case(engines, name, 3, OPTIONS[opt])


@pytest.mark.parametrize("name", R.CONFIG_NAMES)
def test_production_launch_without_taps(engines, name):
    """`debug_taps` 0, what production runs: the last block's output never leaves the CU on "nf64".  Only the latents go in
    and the PCM comes out, so the PCM is judged against the fp64 CHAIN of all stages and that chain's own float32 error;
    on "nf64" the chain ends in stage R3L, which is also judged alone on the stage-3 input the kernels consumed."""
    eng, cfg, W = engines(name)
    B = 3
    latents = R.seeded_latents(cfg, FRAMES, B, seed_of(name, "no taps"))
    frames = decode_frames(eng, cfg, B, latents, DEFAULTS)
    for fr in frames:
        assert check_kernels(fr["prof"], cfg, B, DEFAULTS) == (name == "nf64")
    if name == "nf64":
        judge(name, cfg, W, frames, ["R3L"])
    worst = 0.0
    for f, (pcm64, e32) in enumerate(R.chain_e32(cfg, W, latents, fused_tail=name == "nf64")):
        got = frames[f]["pcm"]
        assert got.shape == pcm64.shape and np.isfinite(got).all()
        err = float(np.abs(got.astype(np.float64) - pcm64).max())
        worst = max(worst, err / e32)
        print(f"  frame {f} chain err {err:.3e}  E32 {e32:.3e}  ratio {err / e32:.2f}")
    key = (name, "chain", label_of_stage(frames[0]["prof"], "L"))
    STATS[key] = max(STATS.get(key, 0.0), worst)
    assert worst <= FACTOR, worst


def test_reset_row(engines):
    """`reset_row` on the last row before frame 3: the reference restarts that row with zero tails at position 0 and leaves
    the other rows alone"""
    run_case(engines, "nf64", 3, resets=((3, 2),))


@pytest.mark.parametrize("name,opt,kernel", [("nf64", {}, "pcm_fix"), ("nf64", dict(fuse_pcm=0), "pcm_conv"), ("tiny", {}, "gemm")],
                         ids=["pcm_fix", "pcm_conv", "epi_pcm"])
def test_int16_pcm(engines, name, opt, kernel):
    """the int16 copy of each last-conv path is trunc(clamp(pcm, -1, 1) * 32767) of the GPU's own fp32 PCM, exactly; that
    PCM is judged like every other case's.  Latents x 2, so that samples pass +1 and -1"""
    frames = run_case(engines, name, 3, opt, i16=True, scale=2.0, case=("i16",))
    pcm = np.stack([fr["pcm"] for fr in frames])
    assert pcm.max() > 1.0 and pcm.min() < -1.0, (pcm.min(), pcm.max())
    for fr in frames:
        last = at(fr["prof"], "seanet.conv_last")
        assert len(last) == 1 and last[0].startswith(kernel), last
        want = (np.clip(fr["pcm"], np.float32(-1), np.float32(1)) * np.float32(32767)).astype(np.int16)
        assert np.array_equal(fr["pcm_i16"], want)


# ---- every tile configuration at every codec GEMM site ----------------------------------------------------------------
def gemm_sites(cfg, B):
    """site -> (NT, KF, MT, prologue) of the codec's GEMM launches under the default options"""
    tr, sn = cfg.mimi.transformer, cfg.mimi.seanet
    C, FF = tr.d_model, tr.dim_feedforward
    s = {"mimi.qkv": (3 * C // 16, C // 16, B, "ln"), "mimi.out": (C // 16, C // 16, B, ""),
         "mimi.ff1": (FF // 16, C // 16, B, "ln"), "mimi.ff2": (C // 16, FF // 16, B, ""),
         "seanet.conv0": (8 * sn.n_filters // 16, sn.kernel_size * sn.dimension // 16, B, "")}
    for i, (cin, cout, hid, r, rin, rout) in enumerate(seanet_dims(cfg), 1):
        s[f"seanet.convtr{i}"] = (r * cout // 16, 2 * cin // 16, B * rin // 16, "")
        if not fusable(cfg, i, B):
            s[f"seanet.res{i}a"] = (cdiv(hid, 16), 3 * cout // 16, B * rout // 16, "elu")
            s[f"seanet.res{i}b"] = (cout // 16, cdiv(hid, 16), B * rout // 16, "")
    if sn.n_filters != 64:  # CF == 4 takes the vector-ALU kernel
        s["seanet.conv_last"] = (1, sn.last_kernel_size * sn.n_filters // 16, B * seanet_dims(cfg)[-1][5] // 16, "")
    return s


def admitted(c, NT, KF, MT, pre):
    """cfg_valid (csrc/ptts_dispatch.hip) for fp32 weights"""
    s = CFG_SHAPE[c]
    if s[2] == 0:  # LDS-staged: two k-fragments per stage; plain, LN-folded or ELU operand
        return KF % 2 == 0 and pre in ("", "ln", "elu") and MT >= s[1] and 2 * NT >= s[0]
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
    return f"{CFG_NAME[c]}{'+' + pre if pre else ''}@{threads}"


_TABLES = {}


def tuned_table(eng, name, B):
    """the tuner's table of this engine at batch B, measured once: its lines without the configuration column"""
    if (name, B) not in _TABLES:
        eng.tune(B, force=True)
        lines = [ln.split() for ln in eng._tune_table()]
        assert lines and all(len(f) == 14 for f in lines), "the tuner measured nothing (PTTS_NO_TUNE set?)"
        _TABLES[(name, B)] = [" ".join(f[:13]) for f in lines]
        eng.tune_clear()
    return _TABLES[(name, B)]


@pytest.mark.parametrize("c", range(NCFG))
@pytest.mark.parametrize("name", ["tiny", "nf64"])
def test_every_tile_configuration(engines, name, c):
    """the tuner's table is the one public route by which production reaches a tile configuration (choose_cfg): every line
    of the table tuned for B = 5 is rewritten to configuration c.  The profiler must show c EXACTLY at the sites where
    cfg_valid's fp32 rule admits it (elsewhere choose_cfg falls back to the heuristic), and every stage meets the bound"""
    eng, cfg, W = engines(name)
    B = 5
    keys = tuned_table(eng, name, B)
    sites = gemm_sites(cfg, B)
    SWEEP_CASES.setdefault(name, set()).add(c)
    try:
        assert eng.tune_import("".join(f"{k} {c}\n" for k in keys)) == len(keys)
        frames = run_case(engines, name, B, case=("cfg", c))
    finally:
        eng.tune_clear()
    for fr in frames:
        gemms = {s for s, k in fr["prof"] if k.startswith("gemm")}
        assert gemms == set(sites), (sorted(gemms), sorted(sites))
        for site, (NT, KF, MT, pre) in sites.items():
            for k in at(fr["prof"], site):
                if admitted(c, NT, KF, MT, pre):
                    assert k == label_of(c, pre, NT, MT), (site, c, k)
                    SWEPT.setdefault(name, set()).add(c)
                else:
                    assert k.split("+")[0].split("@")[0] != CFG_NAME[c], (site, c, k)


def test_zz_error_table():
    """worst err / E32 per (configuration, stage, kernel) of this session; every tile configuration ran at some site of a
    complete sweep"""
    print(f"\nMimi decoder: worst max|gpu - y64| / E32 (bound {FACTOR})")
    for (name, stage, label), v in sorted(STATS.items()):
        print(f"  {name:5s} {stage:5s} {v:6.2f}  {label}")
    assert all(v <= FACTOR for v in STATS.values())
    for name, ran in SWEPT.items():
        print(f"  {name}: tile configurations that ran: {sorted(ran)}")
    for name, forced in SWEEP_CASES.items():
        if len(forced) == NCFG:  # a complete sweep
            assert SWEPT.get(name) == set(range(NCFG)), (name, SWEPT.get(name))
