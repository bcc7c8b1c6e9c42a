"""CPU checks of the host logic: config schema, weight inventory, WAV writer."""

import sys
import wave

import numpy as np
import pytest
import torch

from pocket_tts_amd.config import CONFIGS_DIR, config_from_dict, config_to_dict, load_config, named_config
from pocket_tts_amd.weights import count_params, flow_lm_spec, generate_tensor, mimi_decode_spec, state_dict_spec


def test_all_language_configs_load():
    files = sorted(CONFIGS_DIR.glob("*.yaml"))
    assert len(files) == 12
    for f in files:
        c = load_config(f)
        assert c.flow_lm.transformer.num_layers in (6, 24)
        assert c.frame_samples == 1920 and c.upsample_stride == 16
    assert load_config(CONFIGS_DIR / "french_24l.yaml").model_recommended_frames_after_eos == 8


def test_config_is_strict_and_missing_file_raises():
    d = config_to_dict(named_config("tiny"))
    d["flow_lm"]["bogus"] = 1
    with pytest.raises(ValueError):
        config_from_dict(d)
    with pytest.raises(FileNotFoundError):
        load_config(CONFIGS_DIR / "klingon.yaml")


def test_param_counts_match_survey():
    """FlowLM 89.41 M total; decode-side Mimi 10.31 M"""
    cfg = named_config("en100m")
    lm = flow_lm_spec(cfg)
    n_lm = count_params(lm) - 2 * 128 - 1024 * 32  # buffers `freqs` and speaker_proj_weight are not in the count
    assert abs(n_lm / 1e6 - 89.41) < 0.02, n_lm
    assert abs(count_params(mimi_decode_spec(cfg)) / 1e6 - 10.31) < 0.01
    assert len(state_dict_spec(named_config("24l"))) > len(state_dict_spec(cfg))


def test_generator_is_deterministic_and_name_keyed():
    a = generate_tensor("flow_lm.input_linear.weight", (1024, 32), 0)
    b = generate_tensor("flow_lm.input_linear.weight", (1024, 32), 0)
    c = generate_tensor("flow_lm.input_linear.weight", (1024, 32), 1)
    d = generate_tensor("flow_lm.other.weight", (1024, 32), 0)
    assert np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(a, d)
    assert a.dtype == np.float32 and abs(float(a.std()) - (3.0 / 32) ** 0.5 / 3 ** 0.5) < 0.01


def test_wav_writer(tmp_path):
    from pocket_tts_amd.main import write_wav_stream

    chunks = [torch.full((1920,), 0.5), torch.full((1920,), -2.0)]
    n = write_wav_stream(str(tmp_path / "a.wav"), iter(chunks), 24000)
    assert n == 2 * 1920 + 4800
    with wave.open(str(tmp_path / "a.wav"), "rb") as w:
        assert (w.getnchannels(), w.getframerate(), w.getsampwidth(), w.getnframes()) == (1, 24000, 2, n)
        x = np.frombuffer(w.readframes(n), dtype=np.int16)
    assert x[0] == 16383 and x[1920] == -32767 and np.all(x[-4800:] == 0)


def test_eos_bookkeeping_matches_reference_loop():
    """pocket_tts_amd.batching.eos_bookkeeping (per-row EOS / frame-count decision of the batched paths) against a
    literal restatement of the reference's loop (tts_model.py:756-775) on random EOS flag sequences: the number of
    latents the reference puts in its queue must equal n_emit, for every max_gen_len / frames_after_eos."""
    import random

    from pocket_tts_amd.batching import eos_bookkeeping as f  # importable without a GPU (the engine loads lazily)

    def reference(flags, max_gen_len, fae):
        put, eos_step = 0, None
        for step in range(max_gen_len):
            if flags[step] and eos_step is None:
                eos_step = step
            if eos_step is not None and step >= eos_step + fae:
                break
            put += 1
        return put

    rnd = random.Random(0)
    for _ in range(2000):
        n, fae = rnd.randint(1, 40), rnd.randint(0, 6)
        flags = [rnd.random() < 0.08 for _ in range(n + 8)]
        eos, n_emit, step = None, None, 0
        while n_emit is None:
            eos, n_emit = f(step, n, fae, eos, flags[step] if step < len(flags) else False)
            step += 1
        assert n_emit == reference(flags, n, fae), (flags, n, fae)


def test_eos_bookkeeping_rows_matches_scalar_version():
    """the vectorised per-row bookkeeping of the batched paths (rows at different local steps, decisions read with a
    lag) == the scalar `eos_bookkeeping`, row by row: same n_emit, same eos_step, decided at the same step"""
    from pocket_tts_amd.batching import eos_bookkeeping, eos_bookkeeping_rows

    rng = np.random.default_rng(3)
    for _ in range(50):
        B = int(rng.integers(1, 40))
        gen, fae = rng.integers(1, 40, B), rng.integers(0, 6, B)
        start = rng.integers(0, 7, B)                     # rows join at different global steps
        flags = rng.random((60, B)) < 0.08
        eos, emit = np.full(B, -1, np.int64), np.full(B, -1, np.int64)
        want = [(None, None)] * B
        for g in range(60):
            rows = start <= g
            eos_bookkeeping_rows(g - start, gen, fae, eos, emit, flags[g], rows)
            for b in range(B):
                if rows[b] and want[b][1] is None:
                    want[b] = eos_bookkeeping(g - start[b], int(gen[b]), int(fae[b]), want[b][0], bool(flags[g, b]))
                assert (emit[b] if emit[b] >= 0 else None) == want[b][1], (g, b)
                if want[b][1] is None:
                    assert (eos[b] if eos[b] >= 0 else None) == want[b][0], (g, b)
        assert (emit >= 0).all()


def test_pmc_tool_labels_match_the_profiler_labels():
    """tools/pmc_traffic.py turns rocprofv3's demangled kernel names into the labels bench.py's profiler uses
    (configuration + operand variant, '@<work-items>' appended by the caller), so that `roofline.traffic` finds them."""
    import importlib.util
    from pathlib import Path

    spec = importlib.util.spec_from_file_location("pmc_traffic", Path(__file__).parent.parent / "tools" / "pmc_traffic.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    n = mod.norm
    assert n("void gemm_kernel<1, 1, 8, 1, 1, 3, false>(GemmArgs)") == "gemm<1,1,8,1,1>+ln"
    assert n("void gemm_kernel<2, 2, 4, 1, 1, 0, false>(GemmArgs)") == "gemm<2,2,4,1,1>"
    assert n("void gemm_kernel<1, 1, 4, 1, 1, 4, false>(GemmArgs)") == "gemm<1,1,4,1,1>+lnmod"
    assert n("void gemm_kernel<2, 2, 4, 1, 1, 2, false>(GemmArgs)") == "gemm<2,2,4,1,1>+addsilu"
    assert n("void gemm_kernel<1, 2, 4, 1, 1, 3, true>(GemmArgs)") == "gemm<1,2,4,1,1>+ln+q8"
    assert n("void gemm_kernel<1, 2, 4, 1, 1, 3, 1>(GemmArgs)") == "gemm<1,2,4,1,1>+ln+q8"  # round 3: the flag became an int
    assert n("void gemm_kernel<2, 2, 4, 1, 1, 0, 0>(GemmArgs)") == "gemm<2,2,4,1,1>"
    assert n("void gemm_kernel<1, 1, 4, 1, 1, 0, 2>(GemmArgs)") == "gemm<1,1,4,1,1>+b16"
    assert n("void gemm_lds_kernel<4, 4, 2, 3, 2>(GemmArgs)") == "gemm_lds<4,4,2>+ln"
    assert n("void gemm_lds_kernel<4, 2, 2, 0, 2>(GemmArgs)") == "gemm_lds<4,2,2>"
    assert n("void gemm_lds_kernel<4, 4, 2, 1, 3, 0>(GemmArgs)") == "gemm_lds<4,4,2>+elu"       # operand ELU on read (single store)
    assert n("void gemm_lds_kernel<4, 2, 2, 1, 2, 4>(GemmArgs)") == "resblock<2,4>+elu"        # fused residual block, same
    assert n("void gemm_lds_kernel<4, 4, 2, 0, 2, 8>(GemmArgs)") == "resblock<4,8>"
    assert n("void attn_cascade_kernel<4, 2, 3, 1>(AttnArgs)") == "attn_cascade"
    assert n("pcm_fix_kernel(float const*, float const*, long, int const*, float const*, float*, short*, int, int)") == "pcm_fix"
    assert n("void attn_decode_kernel<1, true>(AttnArgs)") == "attn_decode"
    assert n("attn_kernel(AttnArgs)") == "attn"
    assert n("attn_combine_kernel(AttnArgs)") == "attn_combine"
    assert n("step_tail_kernel(int*, int, int, int*, int const*)") == "step_tail"


def test_bench_presets_and_rank_spawning():
    """bench.py: `--preset config4` is BASELINE.json configs[3] (24-layer model, 32 utterances per GPU); `--gpus N`
    without a launcher spawns N ranks itself and exits non-zero when a rank fails (here: no GPU in this container)."""
    import subprocess
    import sys

    import bench

    a = bench.parse(["--preset", "config4", "--gpus", "8"])
    assert (a.config, a.batch, a.gpus, a.quantize) == ("24l", 32, 8, False)
    a = bench.parse([])
    assert (a.config, a.batch, a.gpus, a.steps) == ("en100m", 64, 1, 125)
    assert not a.full and a.no_profile and a.no_latency and a.no_api and a.no_cpu_baseline  # plain run: headline only
    f = bench.parse(["--full", "--dump-outputs", "d"])
    assert f.dump_outputs == "d" and not (f.no_profile or f.no_latency or f.no_api or f.no_cpu_baseline)
    assert bench.parse(["--preset", "int8"]).quantize and bench.parse(["--batch", "4", "--preset", "b1"]).batch == 4
    import torch

    if not torch.cuda.is_available():
        r = subprocess.run([sys.executable, bench.__file__, "--gpus", "2", "--steps", "1", "--warmup", "0"],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode != 0
        assert "rank 0 exited" in r.stderr and "rank 1 exited" in r.stderr
    # the rank plumbing end to end on CPU (world_size 2, gloo): spawned ranks rendezvous on 127.0.0.1, the value is the
    # sum of the ranks' audio over the MAX of their wall times, rank 0 alone prints the line
    import json
    import os

    env = dict(os.environ, PTTS_BENCH_DRYRUN="1")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, bench.__file__, "--gpus", "2", "--steps", "10", "--warmup", "0", "--batch", "5"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    audio = 5 * 10 * 0.08
    assert d["n_gpus"] == 2 and abs(d["value"] - 2 * audio / 0.2) < 1e-6
    assert [round(v, 6) for v in d["per_rank_xrt"]] == [round(audio / 0.1, 6), round(audio / 0.2, 6)]


def test_bench_dump_outputs_last_slot_and_row_sample(tmp_path, monkeypatch):
    """bench.py --dump-outputs: the ring slot of the LAST step ((t - 1) % nb) as float32, `_rank<r>` names on ranks > 0,
    and beyond the size cap one seeded sample of rows, the same rows in every array.  Each slot holds its row number plus
    a slot-specific offset, so slot and rows can be read back from the files."""
    import types

    import bench

    B, nb, t = 6, 4, 7
    rows = torch.arange(B, dtype=torch.float32)
    pcm = [rows[:, None] + 1000.0 * i + torch.zeros(B, 5) for i in range(nb)]
    lat = [rows[:, None] + 100.0 * i + torch.zeros(B, 3) for i in range(nb)]
    logit = [rows + 10.0 * i for i in range(nb)]
    job = types.SimpleNamespace(pipe=types.SimpleNamespace(t=t, nb=nb, lat=lat, logit=logit, pcm_of=lambda f: pcm[f % nb]))
    q = (t - 1) % nb

    bench.dump_outputs(job, str(tmp_path / "all"), 0, 1)
    for name, ref in (("pcm", pcm[q]), ("latent", lat[q]), ("eos_logit", logit[q])):
        a = np.load(tmp_path / "all" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, ref.numpy())

    per_row = (5 + 3 + 1) * 4
    monkeypatch.setattr(bench, "DUMP_BYTES", 2 * 4 * per_row)  # two ranks: 4 of the 6 rows each
    bench.dump_outputs(job, str(tmp_path / "cap"), 1, 2)
    assert sorted(p.name for p in (tmp_path / "cap").iterdir()) == ["eos_logit_rank1.npy", "latent_rank1.npy", "pcm_rank1.npy"]
    p, la, lo = (np.load(tmp_path / "cap" / f"{n}_rank1.npy") for n in ("pcm", "latent", "eos_logit"))
    kept = lo - 10.0 * q
    assert len(kept) == 4 and np.array_equal(kept, np.unique(kept))
    assert np.array_equal(p[:, 0] - 1000.0 * q, kept) and np.array_equal(la[:, 0] - 100.0 * q, kept)


def test_drop_in_package_name():
    """`import pocket_tts` is the drop-in: the reference exports exactly TTSModel and export_model_state
    (pocket_tts/__init__.py:6-19; its tests/test_python_api.py:8-26 checks `__all__`), and `pocket_tts.main:cli_app`
    is the console-script entry point (pyproject.toml:71-72)."""
    import importlib

    sys.modules.pop("pocket_tts", None)
    m = importlib.import_module("pocket_tts")
    assert "pocket_tts_amd" not in m.__file__ and m.__file__.endswith("pocket_tts/__init__.py")
    assert sorted(m.__all__) == ["TTSModel", "export_model_state"]
    import pocket_tts_amd

    assert m.TTSModel is pocket_tts_amd.TTSModel and m.export_model_state is pocket_tts_amd.export_model_state
    main = importlib.import_module("pocket_tts.main")
    assert callable(main.cli_app)
    with pytest.raises(SystemExit):
        main.cli_app(["generate", "--help"])
