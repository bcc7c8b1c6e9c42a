"""What the dynamics feature costs per step: the batch-64 step pipeline of the 100M model (synthetic weights, temp 0.7, device
noise, EOS off) three ways, alternating in one process: without the stage ("off": what the commit before the feature runs),
with a compressor (and the leveler it brings) and every row on bypass ("bypass"), and with every row on `speech` at 24 kHz
("speech").  One more leg says what to compare them with: the leveler alone on bypass ("level_bypass": "bypass" minus this is
the compressor's own bypass).  Prints one JSON line per leg and repetition and writes them, with the per-leg medians, to
--out.  Then the compressor's kernel alone, timed by the library's profiler at batch 64, at (24000, 1920), (8000, 640) and
(48000, 7680) ("kernel_us").

    python tools/dynamics_probe.py --out profiles/dynamics_probe.json
"""

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def kernel_times(eng, B, frames=200):
    """{shape: microseconds per launch of the compressor's kernel, every row on `speech` (None: on bypass)}"""
    import torch

    from pocket_tts_amd import dynamics

    out = {}
    for rate, n, setting in ((24000, 1920, None), (24000, 1920, "speech"), (8000, 640, "speech"), (48000, 7680, "speech")):
        plan = dynamics.plan(rate, n, setting or "speech")
        dy = eng.new_dynamics(B, [plan])
        for b in range(B):
            dy.set_row(b, None if setting is None else 0)
        x = torch.randn(B, n, device=eng.device, generator=torch.Generator(eng.device).manual_seed(1)) * 0.1
        y = torch.zeros(B, n, device=eng.device)
        for _ in range(20):
            dy.frame(x, y)
        eng.sync()
        eng.profile_start()
        for _ in range(frames):
            dy.frame(x, y)
        rows = [r for r in eng.profile_stop() if r["kernel"] == "dynamics"]
        us = 1e3 * sum(r["total_ms"] for r in rows) / sum(r["count"] for r in rows)
        out[f"{rate}/{n}/{setting or 'bypass'}"] = dict(us_per_launch=round(us, 2), chunk=plan.chunk,
                                                       scan_steps=(-(-plan.n // plan.chunk) - 1).bit_length())
        dy.close()
    return out


LEGS = {  # name: (StepPipeline keywords, the route of every row)
    "off": ({}, None),
    "level_bypass": ({"level": True}, None),
    "bypass": ({"dynamics": ["speech"]}, None),
    "speech": ({"dynamics": ["speech"]}, {"dynamics": "speech"}),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="en100m")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=375)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default=",".join(LEGS))
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
        kw, route = LEGS[name]
        st, ms = eng.new_lm_state(B, cap), eng.new_mimi_state(B)
        st.set_noise(0.7, 1234)
        pipe = StepPipeline(eng, st, ms, None, 1, float("inf"), mode="events", pcm_i16=True, **kw)
        if route is not None:
            for b in range(B):
                pipe.chain.set_row(b, pipe.chain.table.route(**route), pipe.s2)
        legs[name] = (st, ms, pipe)
    rows = []
    for rep in range(a.reps):
        for name, (st, ms, pipe) in legs.items():
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
                       audio_s_per_s=round(B * eng.frame_samples / cfg.mimi.sample_rate / (ms_step * 1e-3), 1))
            if LEGS[name][1] is not None:  # the stages did work: the last frame is not silent
                n = pipe.chain.table.route(**LEGS[name][1]).n_out
                y = pipe.out_of(pipe.decoded - 1)[:, :n].numpy().astype("float32") / 32767.0
                row["rms_of_last_frame"] = round(float((y ** 2).mean() ** 0.5), 4)
            if a.tag:
                row["tag"] = a.tag
            rows.append(row)
            print(json.dumps(row), flush=True)
    for st, ms, pipe in legs.values():
        pipe.close()
    kernel_us = kernel_times(eng, B)
    print(json.dumps(dict(kernel_us=kernel_us)), flush=True)
    eng.close()
    summary = {name: statistics.median(r["ms_per_step"] for r in rows if r["leg"] == name) for name in legs}
    print(json.dumps(dict(median_ms_per_step=summary)), flush=True)
    if a.out:
        Path(a.out).write_text(json.dumps(dict(config=a.config, batch=B, steps=a.steps, warmup=a.warmup,
                                               median_ms_per_step=summary, kernel_us=kernel_us, runs=rows), indent=1) + "\n")


if __name__ == "__main__":
    main()
