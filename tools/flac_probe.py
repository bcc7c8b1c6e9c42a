"""What the FLAC packer costs per step: the batch-64 step pipeline of the 100M model (synthetic weights, temp 0.7, device
noise, EOS off) four ways, alternating in one process: without the stage, the codec's last kernel writing int16 itself ("off":
the "off" leg of tools/encode_probe.py, which also runs on a commit without the packer), with encoder and packer and every row
passing its pcm_s16le bytes through ("pass"), and with every row on flac at 24 kHz ("flac24k") and, behind the resampler, at 8
kHz ("flac8k").  Prints one JSON line per leg and repetition and writes them, with the per-leg medians, to --out.  A flac leg
also records the mean frame size of its last line against the 2 n bytes of pcm_s16le; synthetic weights make noise-like audio,
so that ratio says little about speech (`--ratio` measures a speech-like synthetic signal through the stage alone).

    python tools/flac_probe.py --out profiles/flac_probe.json
"""

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

LEGS = {"off": dict(pcm_i16=True), "pass": dict(compressions=["flac"]), "flac24k": dict(compressions=["flac"]),
        "flac8k": dict(sample_rates=[8000], compressions=["flac"])}
REQUESTS = {"pass": dict(), "flac24k": dict(compression="flac"), "flac8k": dict(sample_rate=8000, compression="flac")}


def speech_like(n_total, rate, seed=0):
    """int16: an AR(2) resonance under a slow syllable envelope, -20 dBFS RMS, with pauses: closer to recorded speech than
    the synthetic weights' output"""
    import numpy as np

    rng = np.random.default_rng(seed)
    e = rng.standard_normal(n_total)
    r, w = 0.97, 2 * np.pi * 500.0 / rate
    from scipy.signal import lfilter

    y = lfilter([1.0], [1.0, -2 * r * np.cos(w), r * r], e)
    t = np.arange(n_total) / rate
    env = np.clip(np.sin(2 * np.pi * 3.0 * t), 0.0, None) ** 2 * (np.sin(2 * np.pi * 0.4 * t) > -0.3)
    y = y * env
    y *= 0.1 * 32768 / max(np.sqrt(np.mean(y ** 2)), 1e-9)
    return np.clip(np.round(y), -32768, 32767).astype(np.int16)


def ratio_leg(eng, rate, n, lines=125):
    """the stage alone on `lines` lines of the speech-like signal: flac bytes / pcm_s16le bytes"""
    import numpy as np
    import torch

    pk = eng.new_packer(1, n)
    pk.set_row(0, n, None, "flac", 0, 0, rate)
    x = speech_like(lines * n, rate)
    out = torch.zeros(1, pk.pitch, dtype=torch.uint8).pin_memory()
    total = 0
    for f in range(lines):
        buf = np.zeros((1, pk.in_pitch), np.uint8)
        buf[0, :2 * n] = np.frombuffer(x[f * n:(f + 1) * n].tobytes(), np.uint8)
        pk.frame(torch.from_numpy(buf).to(eng.device), out)
        eng.sync()
        total += int.from_bytes(out[0, :4].numpy().tobytes(), "little")
    pk.close()
    return dict(leg=f"ratio{rate}", rate=rate, n=n, lines=lines, flac_bytes=total, pcm_bytes=2 * n * lines,
                ratio=round(total / (2.0 * n * lines), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="en100m")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=375)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="off,pass,flac24k,flac8k")
    ap.add_argument("--ratio", action="store_true", help="also the compression ratio of a speech-like signal, stage alone")
    ap.add_argument("--tag", default=None, help="written into every line, e.g. the commit that was measured")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from pocket_tts_amd.config import named_config
    from pocket_tts_amd.engine import Engine, StepPipeline
    from pocket_tts_amd.weights import generate_state_dict

    cfg = named_config(a.config)
    eng = Engine(cfg, generate_state_dict(cfg, 0), "cuda:0")
    B = a.batch
    cap = 64 + a.warmup + a.steps + 8
    emb = (torch.randn(B, 48, eng.D, generator=torch.Generator().manual_seed(1)) * 0.1).to(eng.device)
    legs = {}
    for name in a.legs.split(","):
        st, ms = eng.new_lm_state(B, cap), eng.new_mimi_state(B)
        st.set_noise(0.7, 1234)
        pipe = StepPipeline(eng, st, ms, None, 1, float("inf"), mode="events", **LEGS[name])
        route = None
        if name != "off":
            route = pipe.chain.table.route(**REQUESTS[name])
            for b in range(B):
                pipe.chain.set_row(b, route, pipe.s2)
        legs[name] = (st, ms, pipe, route)
    rows = []
    for rep in range(a.reps):
        for name, (st, ms, pipe, route) in legs.items():
            st.reset()
            eng.lm_prefill(st, emb)
            pipe.restart()  # the rows keep their routes
            for _ in range(a.warmup):
                pipe.step()
            pipe.sync()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                pipe.step()
            pipe.sync()
            ms_step = (time.perf_counter() - t0) * 1e3 / a.steps
            row = dict(leg=name, rep=rep, batch=B, steps=a.steps, ms_per_step=round(ms_step, 4),
                       audio_s_per_s=round(B * eng.frame_samples / cfg.mimi.sample_rate / (ms_step * 1e-3), 1),
                       pcm_bytes_per_row=2 * (eng.frame_samples if route is None else route.n_out))
            if route is not None:  # what the last line's prefixes say
                y = pipe.out_of(pipe.decoded - 1).numpy()
                sizes = y[:, :4].copy().view("<u4")[:, 0]
                row["mean_bytes_of_last_line"] = round(float(sizes.mean()), 1)
                row["max_bytes_of_last_line"] = int(sizes.max())
            if a.tag:
                row["tag"] = a.tag
            rows.append(row)
            print(json.dumps(row), flush=True)
    for st, ms, pipe, route in legs.values():
        pipe.close()
    ratios = []
    if a.ratio:
        for rate, n in ((24000, 1920), (8000, 640)):
            ratios.append(ratio_leg(eng, rate, n))
            print(json.dumps(ratios[-1]), flush=True)
    eng.close()
    summary = {name: statistics.median(r["ms_per_step"] for r in rows if r["leg"] == name) for name in legs}
    print(json.dumps(dict(median_ms_per_step=summary)), flush=True)
    if a.out:
        Path(a.out).write_text(json.dumps(dict(config=a.config, batch=B, steps=a.steps, warmup=a.warmup,
                                               median_ms_per_step=summary, runs=rows, speech_like=ratios), indent=1) + "\n")


if __name__ == "__main__":
    main()
