"""What the output-encoding feature costs per step: the batch-64 step pipeline of the 100M model (synthetic weights, temp 0.7,
device noise, EOS off) three ways, alternating in one process: without the stage, the codec's last kernel writing int16
itself ("off": the "off" leg of tools/level_probe.py), with the encoder and every row on pcm_s16le ("s16"), and with the
resampler and the encoder and every row on mulaw at 8 kHz ("mulaw8k").  Prints one JSON line per leg and repetition and
writes them, with the per-leg medians, to --out.

    python tools/encode_probe.py --out profiles/encode_probe.json
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
    ap.add_argument("--legs", default="off,s16,mulaw8k")
    ap.add_argument("--tag", default=None, help="written into every line, e.g. the commit that was measured")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from pocket_tts_amd.config import named_config
    from pocket_tts_amd.encoding import NAMES
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
        kw = {"off": dict(pcm_i16=True), "s16": dict(encodings=list(NAMES)),
              "mulaw8k": dict(sample_rates=[8000], encodings=list(NAMES))}[name]
        pipe = StepPipeline(eng, st, ms, None, 1, float("inf"), mode="events", **kw)
        route = None
        if name != "off":
            request = dict(sample_rate=8000, encoding="mulaw") if name == "mulaw8k" else dict(encoding="pcm_s16le")
            route = pipe.chain.table.route(**request)
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
                       bytes_per_row=2 * eng.frame_samples if route is None else route.n_out * route.bytes_per_sample)
            if route is not None:  # the encoder did work: bytes of the last frame that are not the encoding's silence
                y = pipe.out_of(pipe.decoded - 1).numpy()[:, :row["bytes_per_row"]]
                row["busy_bytes_of_last_frame"] = int((y != (0xFF if name == "mulaw8k" else 0)).sum())
            if a.tag:
                row["tag"] = a.tag
            rows.append(row)
            print(json.dumps(row), flush=True)
    for st, ms, pipe, route in legs.values():
        pipe.close()
    eng.close()
    summary = {name: statistics.median(r["ms_per_step"] for r in rows if r["leg"] == name) for name in legs}
    print(json.dumps(dict(median_ms_per_step=summary)), flush=True)
    if a.out:
        Path(a.out).write_text(json.dumps(dict(config=a.config, batch=B, steps=a.steps, warmup=a.warmup,
                                               median_ms_per_step=summary, runs=rows), indent=1) + "\n")


if __name__ == "__main__":
    main()
