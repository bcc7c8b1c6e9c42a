"""The decoder the `codec_bf16` and `codec_fp8` engines run (mimi_enqueue_h, csrc/ptts_codec.hip) against the fp64 format
stages of tests/mimi_ref.py, LAUNCH BY LAUNCH, through the public `Engine.mimi_decode` (one case through `mimi_decode_tr` +
`mimi_decode_seanet`, so parts 1 and 2 and the hand-over through tr_out's parity halves run).  `-m gpu`.

Per case: a fresh state decodes 6 frames of seeded latents with the engine option `debug_taps` 1: the zero-carry first
frame, the window dropping keys (context 40, from frame 2) and the ring of 80 slots wrapping (frame 5).  After each frame
every input and output of every launch is read back (`Engine.debug_read`: bf16 values, e4m3 codes, the fp32 queries and
every slot of the K / V rings) and each launch is judged ON THE INPUT IT CONSUMED.  For every element of every output of
every frame,

    |gpu - y64| <= FACTOR * E32(stage, output, frame) [+ f8_mfma_bound + 2 u |y64| for an e4m3 GEMM], then the output's rounding

FACTOR = 8 as in tests/test_gpu_mimi_matrix.py and for the reason given there (the kernels split K over MFMA steps and sum
in another order than numpy); E32 is the loss of a float32 evaluation of the same formulas on the same inputs
(mimi_ref.fstage_e32), from the reference alone.  The e4m3 MFMA does not sum its 32 products as fp32 does:
codec_ref.f8_mfma_bound adds what the model tests/test_gpu_codec_matrix.py pins drops, and 2 u |y64| (u = 2^-24) are the
two roundings of the fp8 epilogue that file states (wscale * xs, then the product; E32's float32 evaluation makes them too,
but at its own operands).  Output rounding exactly as that file does it: a bf16 output lies within half a bf16 ulp of the
bounded interval, an e4m3 output is one of the two e4m3 neighbours of the interval's ends times yinv and exactly +-448
where the interval saturates, fp32 outputs (queries, K / V rows, PCM) carry no output rounding, the int16 PCM lies within
one step.  None of these figures is
fitted to what the kernels produce.

Besides the bound: outputs are finite; the ring slots a frame must not write are bit-identical before and after; rows of
other sequences are bitwise those of a twin state that was not reset; the profiler's records show the expected kernel at
every site (`gemm_f8` on exactly the nine SEANet convolutions of an fp8 engine, nowhere on a bf16 one); the scales of the
fp8 codec are 2 amax / 448 of the taps of a bf16 engine decoding the calibration latents, index by index.

Measured on an MI355X: worst distance from the bounded interval in units of the bound, per (configuration, format,
stage.output, kernel); nf64* = the worst of `nf64` and `nf64x2` over all their cases, layers and SEANet stages merged.
fp32 and bf16 outputs sit at <= 0.22 of the bound; an e4m3 output is measured against the bound PLUS the width of its
rounding interval, so a correctly rounded code shows up to 0.5.  `f8_scales` was bit-equal to 2 amax / 448 at all nine
indices and every weight image to the reference's.  No kernel, scale index, stride or calibration defect was found.
Slowest cases: 26 s (B = 17, fp8, six frames), then 6 s (B = 3, fp8): the time is the reference's (the fp8 bound visits
every product of every fp8 GEMM, 17 sequences of 1920 rows in the last stage), not the GPU's.

  nf64*  bf16 A.attn      0.028  attn
  en100m bf16 A.attn      0.017  attn_combine
  en100m bf16 B.resid     0.001  gemm_h<1,1,2,2>
  nf64*  bf16 B.resid     0.035  gemm_h<1,1,2,2>
  en100m bf16 C.ff        0.006  gemm_h<1,1,2,2>+ln
  nf64*  bf16 C.ff        0.013  gemm_h<1,1,2,2>+ln
  en100m bf16 Cv.elu      0.032  gemm_h<1,1,2,2>
  nf64*  bf16 Cv.elu      0.045  gemm_h<1,1,2,2>
  nf64*  bf16 Cv.elu      0.032  gemm_h<1,2,2,2>
  nf64*  bf16 Cv.elu      0.021  gemm_h<2,2,2,2>
  en100m bf16 Cv.raw      0.017  gemm_h<1,1,2,2>
  nf64*  bf16 Cv.raw      0.057  gemm_h<1,1,2,2>
  nf64*  bf16 Cv.raw      0.028  gemm_h<1,2,2,2>
  nf64*  bf16 Cv.raw      0.017  gemm_h<2,2,2,2>
  en100m bf16 D.out       0.031  gemm_h<1,1,2,2>
  nf64*  bf16 D.out       0.032  gemm_h<1,1,2,2>
  en100m bf16 L.pcm       0.175  pcm_conv_h
  nf64*  bf16 L.pcm       0.167  pcm_conv_h
  en100m bf16 P.upsample  0.004  mimi_prologue
  nf64*  bf16 P.upsample  0.022  mimi_prologue
  en100m bf16 Q.k         0.068  gemm_h<1,1,2,2>+ln
  nf64*  bf16 Q.k         0.070  gemm_h<1,1,2,2>+ln
  en100m bf16 Q.q         0.080  gemm_h<1,1,2,2>+ln
  nf64*  bf16 Q.q         0.078  gemm_h<1,1,2,2>+ln
  en100m bf16 Q.v         0.061  gemm_h<1,1,2,2>+ln
  nf64*  bf16 Q.v         0.082  gemm_h<1,1,2,2>+ln
  en100m bf16 Ra.h        0.019  gemm_h<1,1,2,2>
  nf64*  bf16 Ra.h        0.041  gemm_h<1,1,2,2>
  en100m bf16 Rb.out      0.040  gemm_h<1,1,2,2>
  nf64*  bf16 Rb.out      0.052  gemm_h<1,1,2,2>
  nf64*  bf16 Rb.out      0.039  gemm_h<1,2,2,2>
  en100m bf16 S.a0        0.008  gemm_h<1,1,2,2>
  nf64*  bf16 S.a0        0.040  gemm_h<1,1,2,2>
  nf64*  fp8  A.attn      0.029  attn
  en100m fp8  A.attn      0.011  attn_combine
  en100m fp8  B.resid     0.040  gemm_h<1,1,2,2>
  nf64*  fp8  B.resid     0.014  gemm_h<1,1,2,2>
  en100m fp8  C.ff        0.008  gemm_h<1,1,2,2>+ln
  nf64*  fp8  C.ff        0.013  gemm_h<1,1,2,2>+ln
  en100m fp8  Cv.elu      0.496  gemm_f8
  nf64*  fp8  Cv.elu      0.496  gemm_f8
  en100m fp8  Cv.raw      0.024  gemm_f8
  nf64*  fp8  Cv.raw      0.023  gemm_f8
  en100m fp8  D.out       0.014  gemm_h<1,1,2,2>
  nf64*  fp8  D.out       0.042  gemm_h<1,1,2,2>
  en100m fp8  L.pcm       0.214  pcm_conv_h
  nf64*  fp8  L.pcm       0.203  pcm_conv_h
  en100m fp8  P.upsample  0.001  mimi_prologue
  nf64*  fp8  P.upsample  0.029  mimi_prologue
  en100m fp8  Q.k         0.062  gemm_h<1,1,2,2>+ln
  nf64*  fp8  Q.k         0.076  gemm_h<1,1,2,2>+ln
  en100m fp8  Q.q         0.059  gemm_h<1,1,2,2>+ln
  nf64*  fp8  Q.q         0.074  gemm_h<1,1,2,2>+ln
  en100m fp8  Q.v         0.077  gemm_h<1,1,2,2>+ln
  nf64*  fp8  Q.v         0.071  gemm_h<1,1,2,2>+ln
  en100m fp8  Ra.h        0.495  gemm_f8
  nf64*  fp8  Ra.h        0.497  gemm_f8
  en100m fp8  Rb.out      0.498  gemm_f8
  nf64*  fp8  Rb.out      0.499  gemm_f8
  en100m fp8  S.a0        0.500  gemm_h<1,1,2,2>
  nf64*  fp8  S.a0        0.500  gemm_h<1,1,2,2>

Seeded defects, each seeded once in ptts_codec.hip in a local build that is not committed, each caught on the MI355X:
  * `sc_in` of the transposed convs of stages 2 and 3 read from the next index: test_batches[nf64-fp8-3] fails at Cv2.raw
    (55 x the bound), Cv3.raw (153 x) and both ELU'd e4m3 outputs (codes outside the interval's neighbours);
  * `a.R` pointed at `cbuf` (the ELU'd copy) instead of `craw`: test_batches[nf64-bf16-3] fails at Rb1 / Rb2 / Rb3.out
    (1.1e5 .. 3.5e5 x), test_batches[nf64-fp8-3] at the same three launches (codes outside the neighbours);
  * `par` dropped from the input stride of stage 2's k3 conv (the halo from the current frame's slot):
    test_batches[nf64-fp8-3] fails at Ra2.h in every frame (codes outside the neighbours);
  * `amax` scanning only parity slot 0: test_fp8_scales_are_the_calibration_amax fails at indices 0, 1, 3, 6, 7 (the rings;
    scales 1.3 .. 5.7 % low), the hidden activations' indices 2, 5, 8 (no ring) stay bit-equal.

The weight images the launches multiply by are read back (`w_<site>`, `ws_<site>`) and compared bit for bit with
`gemm_ref.bf16_round`, `codec_ref.quant_weight_f8` and the reference's own images (`mimi_ref.site_weights`); the int16 PCM
lies within one step of the reference's on every sample of every case."""

import time
import zlib

import numpy as np
import pytest
import torch

import codec_ref as CR
import mimi_ref as R
from pocket_tts_amd._lib import PttsError
from test_gpu_codec_matrix import NAMES, prod_tile

pytestmark = pytest.mark.gpu

FACTOR = 8
FRAMES = 6
STATS = {}  # (config, format, stage.output, kernel) -> worst ratio to the bound
TIMES = {}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def seed_of(*case):
    return zlib.crc32(repr(case).encode())


def weights_of(name):
    if name == "en100m":
        from conftest import synth_weights

        return synth_weights("en100m")
    return R.codec_weights(name)


@pytest.fixture(scope="module")
def engines():
    """one engine per (configuration, format) for the whole module"""
    from pocket_tts_amd.engine import Engine

    cache = {}

    def get(name, fmt):
        if (name, fmt) not in cache:
            cfg, W = weights_of(name)
            cache[(name, fmt)] = (Engine(cfg, W, "cuda:0", quantize_groups={"codec_" + fmt}), cfg, W)
        return cache[(name, fmt)]

    yield get
    for eng, _, _ in cache.values():
        eng.close()


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.time()
    yield
    TIMES[request.node.name] = time.time() - t0


# ---- reading a frame back ----------------------------------------------------------------------------------------------
def tap_names(cfg):
    L = cfg.mimi.transformer.num_layers
    names = ["upsample", "dec_tr", "seanet0"]
    for l in range(L):
        names += [f"tr_q{l}", f"tr_k{l}", f"tr_v{l}", f"tr_attn{l}", f"tr_resid{l}", f"tr_ff{l}"] + ([f"tr_in{l}"] if l else [])
    for i in (1, 2, 3):
        names += [f"seanet{3 * i - 1}", f"seanet_c{i}", f"seanet_h{i}", f"seanet{3 * i}"]
    return names


def read_taps(eng, ms, B, names):
    t = {}
    for name in names:
        x = eng.debug_read(ms, name).cpu().numpy()
        t[name] = x.reshape(B, x.shape[0] // B, x.shape[1])
    return t


def decode_frames(eng, cfg, B, latents, resets=(), split=False):
    """-> (one dict per frame: latent, PCM, every tap as [B, T, C], the profiler's (site, kernel) records; the K / V rings
    before the first frame; the fp8 engine's activation scales or None).  A HIP error ends the session: the device may be in
    any state, nothing more is started"""
    names = tap_names(cfg)
    eng.set_option("debug_taps", 1)
    ms = eng.new_mimi_state(B)
    frames, scales = [], None
    i16 = torch.zeros((B, eng.frame_samples), dtype=torch.int16, device="cuda:0")
    try:
        ms.set_pcm_i16(i16)
        if "codec_fp8" in eng.quantize_groups:
            scales = eng.debug_read(ms, "f8_scales").cpu().numpy()[0]
        rings0 = read_taps(eng, ms, B, [n for n in names if n[:4] in ("tr_k", "tr_v")])
        for f, lat in enumerate(latents):
            for fr, row in resets:
                if fr == f:
                    ms.reset_row(row)
            eng.profile_start()
            if split:
                eng.mimi_decode_tr(ms, dev(lat))
                pcm = eng.mimi_decode_seanet(ms)
            else:
                pcm = eng.mimi_decode(ms, dev(lat))
            prof = eng.profile_stop()
            torch.cuda.synchronize()
            t = dict(latent=lat, pcm=pcm.cpu().numpy(), prof=[(r["site"], r["kernel"]) for r in prof for _ in range(r["count"])])
            t.update(read_taps(eng, ms, B, names))
            t["pcm_i16"] = i16.cpu().numpy().copy()
            t["tr_in0"] = t["upsample"]
            frames.append(t)
    except (PttsError, RuntimeError) as e:
        pytest.exit(f"GPU error in the codec format matrix, session ended: {e}", returncode=3)
    finally:
        eng.set_option("debug_taps", 0)
    ms.close()
    return frames, rings0, scales


# ---- what must have run ----------------------------------------------------------------------------------------------
def at(prof, site):
    return [k for s, k in prof if s == site]


def gemm_sites(cfg, B):
    """site -> (NT, MT, +ln) of the codec's GEMM launches"""
    tr, sn = cfg.mimi.transformer, cfg.mimi.seanet
    C, FF = tr.d_model, tr.dim_feedforward
    s = {"mimi.qkv": (3 * C // 16, B, True), "mimi.out": (C // 16, B, False), "mimi.ff1": (FF // 16, B, True),
         "mimi.ff2": (C // 16, B, False), "seanet.conv0": (8 * sn.n_filters // 16, B, False)}
    mult, rows = 8, 16
    for i, r in enumerate(sn.ratios, 1):
        cout = mult * sn.n_filters // 2
        hid = cout // sn.compress
        s[f"seanet.convtr{i}"] = (r * cout // 16, B * rows // 16, False)
        rows *= r
        s[f"seanet.res{i}a"] = (hid // 16, B * rows // 16, False)
        s[f"seanet.res{i}b"] = (cout // 16, B * rows // 16, False)
        mult //= 2
    return s


F8_SITES = {f"seanet.{s}" for i in (1, 2, 3) for s in (f"convtr{i}", f"res{i}a", f"res{i}b")}


def check_kernels(prof, cfg, B, fmt):
    """the kernel family, the production tile of choose_h_tile / choose_f8_tile and the +ln prologue at every site"""
    L = cfg.mimi.transformer.num_layers
    assert at(prof, "mimi.prologue") == ["mimi_prologue"], prof
    attn = at(prof, "mimi.attn")
    comb = [k for k in attn if k.startswith("attn_combine")]
    assert all(k.startswith("attn") for k in attn) and len(attn) - len(comb) == L and len(comb) in (0, L), attn
    assert at(prof, "seanet.conv_last") == ["pcm_conv_h"], prof
    f8_ran = {s for s, k in prof if k.startswith("gemm_f8")}
    assert f8_ran == (F8_SITES if fmt == "fp8" else set()), sorted(f8_ran)
    for site, (NT, MT, ln) in gemm_sites(cfg, B).items():
        got = at(prof, site)
        assert len(got) == (L if site.startswith("mimi.") else 1), (site, got)
        for k in got:
            if fmt == "fp8" and site in F8_SITES:
                assert k.startswith("gemm_f8@"), (site, k)
            else:
                assert k.split("@")[0] == NAMES[prod_tile(NT, MT)] + ("+ln" if ln else ""), (site, k, NT, MT)


# ---- judging -----------------------------------------------------------------------------------------------------------
def starts_of(B, f, resets):
    start = np.zeros(B, np.int64)
    for fr, row in resets:
        if fr <= f:
            start[row] = fr
    return start


def label_at(prof, *sites):
    return " ".join(at(prof, s)[-1].split("@")[0] for s in sites if at(prof, s))


def judge(name, fmt, cfg, W, frames, rings0, scales, resets=()):
    """every launch of every frame against its own bound; records STATS; -> {key: worst ratio}"""
    B = frames[0]["latent"].shape[0]
    L, ring = cfg.mimi.transformer.num_layers, frames[0]["tr_k0"].shape[1]
    worst = {}
    com = dict(cfg=cfg, W=W, fmt=fmt)

    def note(stage, out, label, ratio, f):
        key = (name, fmt, f"{stage}.{out}", label)
        worst[key] = max(worst.get(key, 0.0), ratio)
        if ratio > 1:
            print(f"  frame {f} {stage}.{out} ratio {ratio:.3g}  {label}")

    def run(stage, fn, kw, outs, f, label, extra=None):
        """outs: {output name: (tap array, kind, scale index)}"""
        y64, e32 = R.fstage_e32(fn, {**com, **kw})
        # an fp8 site's extra term, from the value before the activation (|ELU'| <= 1): once for both of its outputs
        ex = extra(y64[next(iter(outs))]) if extra is not None else 0.0
        for out, (got, kind, k) in outs.items():
            tol = FACTOR * e32[out] + ex
            assert np.all(tol > 0), (stage, out)
            note(stage, out, label, R.ratio_of(got, y64[out], tol, kind, None if k is None else R.yinv_of(scales, k)), f)

    for f, cur in enumerate(frames):
        start = starts_of(B, f, resets)
        live = start < f
        pos0 = 16 * (f - start)
        pos = pos0[:, None] + np.arange(16)[None, :]
        prof = cur["prof"]
        keep = live[:, None, None].astype(np.float64)

        def tail(tap, n):
            return np.zeros_like(cur[tap][:, :n]) if f == 0 else frames[f - 1][tap][:, -n:] * keep

        run("P", R.fstage_P, dict(lat=cur["latent"], lat_prev=frames[f - 1]["latent"] if f else cur["latent"], live=live),
            {"upsample": (cur["upsample"], "bf16", None)}, f, label_at(prof, "mimi.prologue"))
        slots = pos % ring
        for l in range(L):
            last = l == L - 1
            x = cur[f"tr_in{l}"]
            K, V = cur[f"tr_k{l}"], cur[f"tr_v{l}"]
            Kb, Vb = (frames[f - 1] if f else rings0)[f"tr_k{l}"], (frames[f - 1] if f else rings0)[f"tr_v{l}"]
            written = np.zeros((B, ring), bool)
            for b in range(B):
                written[b, slots[b]] = True
            assert np.array_equal(K[~written].view(np.uint32), Kb[~written].view(np.uint32)), f"layer {l}: a K slot the frame must not write changed"
            assert np.array_equal(V[~written].view(np.uint32), Vb[~written].view(np.uint32)), f"layer {l}: a V slot the frame must not write changed"
            rows = lambda a: np.stack([a[b, slots[b]] for b in range(B)])  # noqa: E731
            lab = label_at(prof, "mimi.qkv")
            run(f"Q{'' if last else l}", R.fstage_Q, dict(l=l, x=x, pos=pos),
                {"q": (cur[f"tr_q{l}"], "f32", None), "k": (rows(K), "f32", None), "v": (rows(V), "f32", None)}, f, lab)
            run(f"A{'' if last else l}", R.fstage_A, dict(q=cur[f"tr_q{l}"], K=K, V=V, pos0=pos0),
                {"attn": (cur[f"tr_attn{l}"], "bf16", None)}, f, label_at(prof, "mimi.attn"))
            run(f"B{'' if last else l}", R.fstage_B, dict(l=l, attn=cur[f"tr_attn{l}"], x=x),
                {"resid": (cur[f"tr_resid{l}"], "bf16", None)}, f, label_at(prof, "mimi.out"))
            run(f"C{'' if last else l}", R.fstage_C, dict(l=l, resid=cur[f"tr_resid{l}"]),
                {"ff": (cur[f"tr_ff{l}"], "bf16", None)}, f, label_at(prof, "mimi.ff1"))
            run(f"D{'' if last else l}", R.fstage_D, dict(l=l, ff=cur[f"tr_ff{l}"], resid=cur[f"tr_resid{l}"]),
                {"out": (cur["dec_tr" if last else f"tr_in{l + 1}"], "bf16", None)}, f, label_at(prof, "mimi.ff2"))
        kind0, k0 = R.out_kind(fmt, ("conv0",))
        run("S0", R.fstage_S0, dict(x=cur["dec_tr"], tail=tail("dec_tr", 6), scales=scales),
            {"a0": (cur["seanet0"], kind0, k0)}, f, label_at(prof, "seanet.conv0"))
        src = "seanet0"
        for i in (1, 2, 3):
            raw, c, h, o = f"seanet{3 * i - 1}", f"seanet_c{i}", f"seanet_h{i}", f"seanet{3 * i}"
            f8 = fmt == "fp8"
            xx = np.concatenate([tail(src, 1), cur[src]], axis=1)
            cols = np.concatenate([xx[:, 1:], xx[:, :-1]], axis=-1)
            kc, sc = R.out_kind(fmt, ("convtr", i))
            run(f"Cv{i}", R.fstage_Cv, dict(i=i, x=cur[src], tail=tail(src, 1), scales=scales),
                {"raw": (cur[raw], "bf16", None), "elu": (cur[c], kc, sc)}, f, label_at(prof, f"seanet.convtr{i}"),
                (lambda y, cols=cols, i=i: R.f8_extra(cfg, W, ("convtr", i), cols, scales, y.reshape(cols.shape[0], cols.shape[1], -1)).reshape(y.shape)) if f8 else None)
            cols = R._im2col(np.concatenate([tail(c, 2), cur[c]], axis=1), 3)
            kh, sh = R.out_kind(fmt, ("res_a", i))
            run(f"Ra{i}", R.fstage_Ra, dict(i=i, x=cur[c], tail=tail(c, 2), scales=scales), {"h": (cur[h], kh, sh)}, f,
                label_at(prof, f"seanet.res{i}a"), (lambda y, cols=cols, i=i: R.f8_extra(cfg, W, ("res_a", i), cols, scales, y)) if f8 else None)
            ko, so = R.out_kind(fmt, ("res_b", i))
            run(f"Rb{i}", R.fstage_Rb, dict(i=i, h=cur[h], skip=cur[raw], scales=scales), {"out": (cur[o], ko, so)}, f,
                label_at(prof, f"seanet.res{i}b"), (lambda y, hh=cur[h], i=i: R.f8_extra(cfg, W, ("res_b", i), hh, scales, y)) if f8 else None)
            src = o
        run("L", R.fstage_L, dict(x=cur["seanet9"], tail=tail("seanet9", 2)), {"pcm": (cur["pcm"], "f32", None)}, f,
            label_at(prof, "seanet.conv_last"))
        # the int16 copy: within one step of the reference's trunc(clamp(y64, -1, 1) * 32767) on every sample
        want = np.trunc(np.clip(R.fstage_L(cfg, W, fmt, cur["seanet9"], tail("seanet9", 2))["pcm"], -1.0, 1.0) * 32767.0)
        step = np.abs(cur["pcm_i16"].astype(np.float64) - want)
        assert step.shape == want.shape and step.max() <= 1, (f, step.max())
    for key, v in worst.items():
        STATS[key] = max(STATS.get(key, 0.0), v)
    bad = {k: round(v, 2) for k, v in worst.items() if not v <= 1}
    assert not bad, bad
    return worst


def representable(cfg, fmt, frames):
    """every tap comes back as values of the format its buffer has: bf16 values, e4m3 codes"""
    e4 = {"seanet0", "seanet_c1", "seanet_h1", "seanet3", "seanet_c2", "seanet_h2", "seanet6", "seanet_c3", "seanet_h3"} if fmt == "fp8" else set()
    for fr in frames:
        for name in tap_names(cfg):
            if name[:4] in ("tr_q", "tr_k", "tr_v"):
                continue
            assert (R.is_e4m3 if name in e4 else R.is_bf16)(fr[name]), (name, fmt)


def run_case(engines, name, fmt, B, resets=(), scale=1.0, split=False, frames_n=FRAMES, case=()):
    eng, cfg, W = engines(name, fmt)
    latents = R.seeded_latents(cfg, frames_n, B, seed_of(name, fmt, B, resets, case), scale)
    frames, rings0, scales = decode_frames(eng, cfg, B, latents, resets, split)
    for fr in frames:
        check_kernels(fr["prof"], cfg, B, fmt)
    representable(cfg, fmt, frames)
    judge(name, fmt, cfg, W, frames, rings0, scales, resets)
    return frames, scales


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("fmt", R.FMTS)
@pytest.mark.parametrize("name", ["nf64", "nf64x2"])
def test_batches(engines, name, fmt, B):
    run_case(engines, name, fmt, B)


@pytest.mark.parametrize("fmt", R.FMTS)
def test_batch_17(engines, fmt):
    """17 sequences: not a multiple of the 16 that share a tile of zq"""
    run_case(engines, "nf64", fmt, 17)


@pytest.mark.parametrize("fmt", R.FMTS)
def test_two_parts(engines, fmt):
    """`mimi_decode_tr` then `mimi_decode_seanet`: parts 1 and 2 meet in tr_out's two parity halves"""
    run_case(engines, "nf64x2", fmt, 3, split=True, case=("parts",))


@pytest.mark.parametrize("fmt", R.FMTS)
def test_reset_row(engines, fmt):
    """`reset_row` on the last row before frame 3: the reference restarts that row with zero tails at position 0; the other
    rows are bitwise those of a twin state that was never reset"""
    B, resets = 3, ((3, 2),)
    frames, _ = run_case(engines, "nf64", fmt, B, resets=resets, case=("reset",))
    eng, cfg, W = engines("nf64", fmt)
    latents = R.seeded_latents(cfg, FRAMES, B, seed_of("nf64", fmt, B, resets, ("reset",)))
    twin = decode_frames(eng, cfg, B, latents)[0]
    for f in range(FRAMES):
        for name in tap_names(cfg) + ["pcm"]:
            a, b = frames[f][name], twin[f][name]
            assert np.array_equal(a[:2].view(np.uint32), b[:2].view(np.uint32)), (f, name)
        assert (f < 3) == np.array_equal(frames[f]["pcm"][2], twin[f]["pcm"][2]), f


def test_fp8_saturating_latents(engines):
    """latents scaled up until the REFERENCE chain, with the reference's own calibration, saturates e4m3 in a SEANet tap
    (asserted on the CPU); the device's codes must then be exactly +-448 wherever the bounded interval saturates"""
    eng, cfg, W = engines("nf64", "fp8")
    B, scale = 3, 6.0
    calib = R.seeded_latents(cfg, 6, 8, 5)
    ref_scales = R.calibrate(cfg, W, calib)
    latents = R.seeded_latents(cfg, FRAMES, B, seed_of("nf64", "fp8", B, (), ("sat",)), scale)
    ch = R.FChain(cfg, W, B, "fp8", ref_scales)
    sat = 0
    for lat in latents:
        t = ch.decode(lat)
        sat += sum(int((np.abs(t[n]) == 448.0).sum()) for n in R.SCALE_TAP.values())
    assert sat > 0, "the reference chain does not saturate: scale the latents further"
    frames, _ = run_case(engines, "nf64", "fp8", B, scale=scale, case=("sat",))
    print("  saturated codes on the device:", sum(int((np.abs(fr[n]) == 448.0).sum()) for fr in frames for n in R.SCALE_TAP.values()))


@pytest.mark.parametrize("fmt", R.FMTS)
def test_latents_near_zero(engines, fmt):
    """e4m3 subnormals and exact zeros; the de-normalised latent is emb_mean + 1e-4 std z"""
    frames, _ = run_case(engines, "nf64", fmt, 3, scale=1e-4, case=("zero",))
    if fmt == "fp8":
        codes = np.concatenate([np.abs(fr[n]).ravel() for fr in frames for n in R.SCALE_TAP.values()])
        assert (codes == 0).any() and ((codes > 0) & (codes < 2.0 ** -6)).any(), "no exact zero or no e4m3 subnormal"


@pytest.mark.parametrize("fmt", R.FMTS)
def test_production_tiles_en100m(engines, fmt):
    """the 100M model's codec at B = 2, 3 frames: the production tile choice of choose_h_tile / choose_f8_tile"""
    run_case(engines, "en100m", fmt, 2, frames_n=3)


# ---- read-back ---------------------------------------------------------------------------------------------------------
def test_debug_read_refuses_what_the_format_lacks(engines):
    eng, cfg, W = engines("nf64x2", "bf16")
    ms = eng.new_mimi_state(2)
    lat = dev(R.seeded_latents(cfg, 1, 2, 3)[0])
    eng.set_option("debug_taps", 0)
    eng.mimi_decode(ms, lat)
    with pytest.raises(PttsError, match="no fp8 codec"):
        eng.debug_read(ms, "f8_scales")
    with pytest.raises(PttsError, match="has 2 slots"):
        eng.debug_read(ms, "dec_tr_slot2")
    for name in ("tr_in1", "tr_resid0", "tr_q0"):
        with pytest.raises(PttsError, match="debug_taps"):
            eng.debug_read(ms, name)
    for name in ("tr_in2", "tr_k2", "seanet_c4", "seanet_h0", "calib_latent6", "tr_qkv", "seanet4"):
        with pytest.raises(PttsError, match="unknown buffer"):
            eng.debug_read(ms, name)
    with pytest.raises(PttsError, match="batch 8"):
        eng.debug_read(ms, "calib_latent0")
    with pytest.raises(PttsError, match="frame pairs|hand-over ring"):  # the reduced-precision codecs take single frames only
        eng.mimi_decode_tr(ms, lat, lat)
    ms.close()


def test_debug_read_refusals_of_the_other_formats(engines):
    """an fp8 engine's hand-over ring has two slots; the fp32 codec keeps a fused block's hidden activation on chip and has
    no reduced-precision weight image; copies of an earlier frame are refused as stale"""
    from pocket_tts_amd.engine import Engine

    eng, cfg, W = engines("nf64x2", "fp8")
    ms = eng.new_mimi_state(2)
    lat = dev(R.seeded_latents(cfg, 1, 2, 3)[0])
    eng.set_option("debug_taps", 1)
    eng.mimi_decode(ms, lat)
    assert R.is_bf16(eng.debug_read(ms, "tr_in1").cpu().numpy())
    for name in ("dec_tr_slot2", "dec_tr_slot3"):
        with pytest.raises(PttsError, match="has 2 slots"):
            eng.debug_read(ms, name)
    with pytest.raises(PttsError, match="no e4m3 weight image"):
        eng.debug_read(ms, "ws_conv0")
    eng.set_option("debug_taps", 0)
    eng.mimi_decode(ms, lat)
    eng.set_option("debug_taps", 1)
    with pytest.raises(PttsError, match="stale"):
        eng.debug_read(ms, "tr_in1")
    eng.mimi_decode(ms, lat)
    assert R.is_bf16(eng.debug_read(ms, "tr_resid0").cpu().numpy())
    eng.set_option("debug_taps", 0)
    ms.close()
    cfg, W = R.codec_weights("nf64")
    e32 = Engine(cfg, W, "cuda:0")
    try:
        ms = e32.new_mimi_state(3)
        e32.mimi_decode(ms, dev(R.seeded_latents(cfg, 1, 3, 3)[0]))
        with pytest.raises(PttsError, match="stays on chip in the fused"):
            e32.debug_read(ms, "seanet_h2")
        with pytest.raises(PttsError, match="no reduced-precision weight image"):
            e32.debug_read(ms, "w_conv0")
        ms.close()
    finally:
        e32.close()


# ---- weight images -----------------------------------------------------------------------------------------------------
def weight_sites(cfg):
    L = cfg.mimi.transformer.num_layers
    return [(k, l) for l in range(L) for k in ("qkv", "out", "ff1", "ff2")] + [("conv0",)] + \
        [(k, i) for i in (1, 2, 3) for k in ("convtr", "res_a", "res_b")]


@pytest.mark.parametrize("fmt", R.FMTS)
@pytest.mark.parametrize("name", ["nf64x2", "en100m"])
def test_weight_images_bit_for_bit(engines, name, fmt):
    """the image every launch multiplies by, as the engine packed it: bf16 against gemm_ref.bf16_round of the fp32 matrix
    (a +ln site: of the fp32 product w * ln_w), e4m3 codes and wscale against codec_ref.quant_weight_f8, and both against
    the images the reference's stages use"""
    from gemm_ref import bf16_round

    eng, cfg, W = engines(name, fmt)
    ms = eng.new_mimi_state(1)
    try:
        for site in weight_sites(cfg):
            tag = site[0] + (str(site[1]) if len(site) > 1 else "")
            got = eng.debug_read(ms, "w_" + tag).cpu().numpy().astype(np.float64)
            f32 = R.site_weights(cfg, W, site, "f32")[0]
            f8 = fmt == "fp8" and site in R.SC_IN
            mine, _, ws = R.site_weights(cfg, W, site, "fp8" if f8 else "bf16")
            if site[0] == "convtr":  # the packer's tap 0 is the previous input row, the reference's first half the current one
                C = got.shape[1] // 2
                got = np.concatenate([got[:, C:], got[:, :C]], axis=1)
            assert got.shape == mine.shape, (site, got.shape, mine.shape)
            assert np.array_equal(got, mine), site
            if f8:
                gws = eng.debug_read(ms, "ws_" + tag).cpu().numpy()[0]
                deq, scale = CR.quant_weight_f8(torch.from_numpy(f32))
                assert np.array_equal(gws.astype(np.float64), scale.numpy()) and np.array_equal(gws, ws), site
                assert np.array_equal((got * gws.astype(np.float64)[:, None]).astype(np.float32).astype(np.float64), deq.numpy()), site
            else:
                assert np.array_equal(got, bf16_round(torch.from_numpy(f32)).numpy()), site
    finally:
        ms.close()


# ---- calibration ---------------------------------------------------------------------------------------------------------
def scales_match(f8s, amax, rel=2.0 ** -8):
    """indices at which f8_scales is not 2 amax / 448 of the expected tap, within one bf16 ulp of amax (the most another
    tile, hence summation order, can move the largest bf16 element); unused indices must be 1"""
    bad = []
    for k in range(16):
        if k in amax:
            if not abs(float(f8s[k]) * 448.0 / 2.0 - amax[k]) <= rel * amax[k]:
                bad.append(k)
        elif f8s[k] != 1.0:
            bad.append(k)
    return bad


def test_fp8_scales_are_the_calibration_amax(engines):
    """calibrate_fp8_codec, amax_bf16_kernel and the rule 2 amax / 448: the calibration latents through a bf16 engine on
    the same weights, amax of the tap each index stands for over the 6 frames"""
    e8, cfg, W = engines("nf64", "fp8")
    e16 = engines("nf64", "bf16")[0]
    B = 8
    m8 = e8.new_mimi_state(B)
    f8s = e8.debug_read(m8, "f8_scales").cpu().numpy()[0]
    lats = np.stack([e8.debug_read(m8, f"calib_latent{f}").cpu().numpy() for f in range(6)])
    m8.close()
    assert lats.shape == (6, B, cfg.mimi.quantizer.dimension) and np.isfinite(lats).all()
    assert abs(lats.mean()) < 0.1 and 0.9 < lats.std() < 1.1 and len(np.unique(lats)) > lats.size // 2
    frames = decode_frames(e16, cfg, B, lats)[0]
    amax = {k: max(float(np.abs(fr[n]).max()) for fr in frames) for k, n in R.SCALE_TAP.items()}
    want = R.scales_from_amax(amax)
    print("\n  k  f8_scales    2 amax / 448  (tap)")
    for k, n in R.SCALE_TAP.items():
        print(f"  {k}  {f8s[k]:.6e}  {want[k]:.6e}  {n}{'' if f8s[k] == want[k] else '   NOT bit-equal'}")
    print("  bit equality held" if np.array_equal(f8s, want) else "  bit equality did NOT hold")
    assert scales_match(f8s, amax) == []
    # the index map: another tap's amax at one index breaks exactly that index
    for k in R.SCALE_TAP:
        assert scales_match(f8s, {**amax, k: amax[k] * (1 + 2.0 ** -5)}) == [k]
    # and the reference's calibration of the same latents agrees to the flips of a 14-launch bf16 chain
    ref = R.calibrate(cfg, W, lats)
    print("  reference calibration / device:", np.round(ref[:9] / f8s[:9], 3))


def test_zz_error_table():
    """worst ratio to the bound per (configuration, format, stage.output, kernel) of this session, and the slowest tests"""
    print(f"\ncodec formats: worst distance from the bounded interval / bound (FACTOR {FACTOR})")
    for (name, fmt, stage, label), v in sorted(STATS.items()):
        print(f"  {name:7s} {fmt:4s} {stage:10s} {v:7.3f}  {label}")
    for n, t in sorted(TIMES.items(), key=lambda kv: -kv[1])[:5]:
        print(f"  {t:6.1f} s  {n}")
    assert STATS and all(v <= 1 for v in STATS.values())
