"""What the leveler's true-peak mode costs per step: the batch-64 step pipeline of the 100M model (synthetic weights, temp
0.7, device noise, EOS off) three ways, alternating in one process, every row at --gain-db under -1 dB: the leveler without
the mode ("off": the `limit` leg of tools/level_probe.py), with the mode and no row using it ("unused"), and with every row
at peak_dbtp -1 ("true_peak").  Prints one JSON line per leg and repetition and writes them, with the per-leg medians, to
--out.

    python tools/truepeak_probe.py --out profiles/truepeak_probe.json
"""

import argparse
import json
import statistics
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
    ap.add_argument("--gain-db", type=float, default=12.0)
    ap.add_argument("--legs", default="off,unused,true_peak")
    ap.add_argument("--tag", default=None, help="written into every line, e.g. the commit that was measured")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from pocket_tts_amd.config import named_config
    from pocket_tts_amd.engine import Engine, StepPipeline
    from pocket_tts_amd.level import dbtp
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
        kw = {"level": True} if name == "off" else {"level": True, "true_peak": True}
        pipe = StepPipeline(eng, st, ms, None, 1, float("inf"), mode="events", pcm_i16=True, **kw)
        ceiling = {"peak_dbtp": -1.0} if name == "true_peak" else {"peak_dbfs": -1.0}
        for b in range(B):
            pipe.chain.set_row(b, pipe.chain.table.route(gain_db=a.gain_db, **ceiling), pipe.s2)
        legs[name] = (st, ms, pipe)
    rows = []
    for rep in range(a.reps):
        for name, (st, ms, pipe) in legs.items():
            st.reset()
            eng.lm_prefill(st, emb)
            pipe.restart()  # the rows keep their plans, gains and modes
            for _ in range(a.warmup):
                pipe.step()
            pipe.sync()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                pipe.step()
            pipe.sync()
            ms_step = (time.perf_counter() - t0) * 1e3 / a.steps
            y = pipe.out_of(pipe.decoded - 1).numpy().astype("float32") / 32767.0
            row = dict(leg=name, rep=rep, batch=B, steps=a.steps, ms_per_step=round(ms_step, 4),
                       audio_s_per_s=round(B * eng.frame_samples / cfg.mimi.sample_rate / (ms_step * 1e-3), 1),
                       gain_db=a.gain_db, peak_of_last_frame=round(float(abs(y).max()), 4))
            if name == "true_peak":  # the meters after warmup + steps frames: what the rows wrote, by the 4x meter
                row["max_row_dbtp"] = round(max(dbtp(pipe.chain.lv.row_true_peak(b, pipe.s2)) for b in range(B)), 4)
            if a.tag:
                row["tag"] = a.tag
            rows.append(row)
            print(json.dumps(row), flush=True)
    for st, ms, pipe in legs.values():
        pipe.close()
    eng.close()
    summary = {name: statistics.median(r["ms_per_step"] for r in rows if r["leg"] == name) for name in legs}
    print(json.dumps(dict(median_ms_per_step=summary)), flush=True)
    if a.out:
        Path(a.out).write_text(json.dumps(dict(config=a.config, batch=B, steps=a.steps, warmup=a.warmup, gain_db=a.gain_db,
                                               median_ms_per_step=summary, runs=rows), indent=1) + "\n")


if __name__ == "__main__":
    main()
