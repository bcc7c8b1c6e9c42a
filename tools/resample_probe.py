"""What the output-sample-rate feature costs per step: the batch-64 step pipeline of the 100M model (synthetic weights, temp
0.7, device noise, EOS off), with and without `sample_rates`, alternating in one process.  Prints one JSON line per leg and
writes them to --out.

    python tools/resample_probe.py --out profiles/resample_cost.jsonl
    python tools/resample_probe.py --legs off --tag parent     # in a checkout of the parent commit, which has only this leg
    rocprofv3 --kernel-trace --stats ... -- python tools/resample_probe.py --legs on --reps 1    # per-kernel times
"""

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="en100m")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=375)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rates", default="8000,16000,44100,48000")
    ap.add_argument("--legs", default="off,on", help="off: no sample_rates, on: with them")
    ap.add_argument("--tag", default=None, help="written into every line, e.g. the commit that was measured")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from pocket_tts_amd.config import named_config
    from pocket_tts_amd.engine import Engine, StepPipeline
    from pocket_tts_amd.weights import generate_state_dict

    cfg = named_config(a.config)
    eng = Engine(cfg, generate_state_dict(cfg, 0), "cuda:0")
    B, rates = a.batch, [int(r) for r in a.rates.split(",")]
    cap = 64 + a.warmup + a.steps + 8
    emb = (torch.randn(B, 48, eng.D, generator=torch.Generator().manual_seed(1)) * 0.1).to(eng.device)
    legs = {}
    for name, sr in [(n, {"off": None, "on": rates}[n]) for n in a.legs.split(",")]:
        st, ms = eng.new_lm_state(B, cap), eng.new_mimi_state(B)
        st.set_noise(0.7, 1234)
        kw = {} if sr is None else {"sample_rates": sr}
        pipe = StepPipeline(eng, st, ms, None, 1, float("inf"), mode="events", pcm_i16=True, **kw)
        if sr is not None:  # rows spread over the native rate and every configured one
            for b in range(B):
                pipe.rs.set_row(b, b % len(pipe.rs.rates), pipe.s2)
        legs[name] = (st, ms, pipe)
    rows = []
    for rep in range(a.reps):
        for name, (st, ms, pipe) in legs.items():
            st.reset()
            eng.lm_prefill(st, emb)
            pipe.restart()
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
                       sample_rates=None if name == "off" else pipe.rs.rates)
            if a.tag:
                row["tag"] = a.tag
            rows.append(row)
            print(json.dumps(row), flush=True)
    for st, ms, pipe in legs.values():
        pipe.close()
    eng.close()
    if a.out:
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
