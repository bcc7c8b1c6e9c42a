"""Batch-1 streaming at temp 0.7 with and without a seed: ms per frame of `TTSModel.generate_audio_stream` on the 100M
English model (synthetic weights, the fixture tokenizer).  Without a seed every step draws 32 floats from torch's CPU
generator and copies them to the device; with a seed the step draws on the device.  EOS is disabled, so every run decodes
the same number of frames; the two settings alternate and the median per setting is printed as one JSON line and
written to `--out` (run on the GPU box):
    python tools/seed_probe.py [--rounds R] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("PTTS_TUNE_CACHE", os.path.join(ROOT, "profiles", "tune_cache_mi355x.txt"))
import torch

from pocket_tts_amd import TTSModel

TEXT = "This is a longer sentence, with several clauses, to test it."


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seed_probe.json"))
    a = ap.parse_args()
    m = TTSModel.load_model(config=os.path.join(ROOT, "tests", "golden", "e2e2_en100m.yaml"), temp=0.7, eos_threshold=1e9)
    state = m.get_state_for_conditioning(torch.randn(1, 50, m.engine.D, generator=torch.Generator().manual_seed(0)) * 0.1)
    times = {"unseeded_host_draw": [], "seeded_device_draw": []}
    frames = 0

    def run(seed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = sum(1 for _ in m.generate_audio_stream(state, TEXT, seed=seed))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n, n

    run(None), run(1)  # contexts, graphs, tile choices
    for r in range(a.rounds):
        for name, seed in (("unseeded_host_draw", None), ("seeded_device_draw", 100 + r)):
            ms, frames = run(seed)
            times[name].append(ms)
    out = {"config": "e2e2_en100m", "batch": 1, "temp": 0.7, "frames_per_run": frames, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0),
           "ms_per_frame": {k: {"median": round(statistics.median(v), 4), "runs": [round(x, 4) for x in v]}
                            for k, v in times.items()}}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    m.engine.close()


if __name__ == "__main__":
    main()
