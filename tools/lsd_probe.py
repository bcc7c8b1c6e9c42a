"""Cost of per-row LSD schedules: ms per FlowLM step graph (StepPipeline's captured step, replayed alone on its stream) at
batch 64, en100m, for five settings: a state without the capacity at n = 1; a state with capacity K = 4 and every row at
1; every row at 2; one row at 4 and the rest at 1; every row at 4.  Settings are interleaved over several rounds and the
median per setting is written to profiles/row_lsd_probe.json.  Every measurement starts from the same context (state reset +
prefill), so the settings see the same attention lengths (run on the GPU box):
    python tools/lsd_probe.py [--rounds R] [--steps N] [--out PATH]
Under `rocprofv3 --kernel-trace` the flow-cluster dispatches come in setting order (the JSON lists it), 4 warm-up steps +
`--steps` per setting and round."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("PTTS_TUNE_CACHE", os.path.join(ROOT, "profiles", "tune_cache_mi355x.txt"))
import torch

from pocket_tts_amd.config import named_config
from pocket_tts_amd.engine import Engine, StepPipeline
from pocket_tts_amd.weights import generate_state_dict

B, K, PREFIX = 64, 4, 50
SETTINGS = [("unreserved_n1", None), ("reserved_all1", [1] * B), ("reserved_all2", [2] * B),
            ("reserved_one4_rest1", [4] + [1] * (B - 1)), ("reserved_all4", [4] * B)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "row_lsd_probe.json"))
    a = ap.parse_args()
    cfg = named_config("en100m")
    eng = Engine(cfg, generate_state_dict(cfg, 0), "cuda:0")
    cap = PREFIX + a.steps + 16
    emb = torch.randn(B, PREFIX, eng.D, generator=torch.Generator().manual_seed(0)) * 0.3

    def make(reserve):
        st = eng.new_lm_state(B, cap)
        if reserve:
            st.reserve_row_lsd(K)  # before the pipeline captures its graphs
        st.set_noise(0.7, 0)
        ms = eng.new_mimi_state(B)
        return st, ms, StepPipeline(eng, st, ms, None, 1, -4.0, mode="events")

    plain, reserved = make(False), make(True)
    times = {name: [] for name, _ in SETTINGS}
    for r in range(a.rounds):
        for name, counts in SETTINGS:
            st, _, pipe = plain if counts is None else reserved
            st.reset()  # same context for every measurement; also clears the overrides
            eng.lm_prefill(st, emb.to(eng.device))
            eng.sync()
            if counts is not None:
                for row, n in enumerate(counts):
                    st.set_row_lsd(row, n)
            for i in range(4):  # warm-up
                eng.graph_launch(pipe.g_first[i % pipe.nb], pipe.s1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.steps):
                eng.graph_launch(pipe.g_first[i % pipe.nb], pipe.s1)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / a.steps * 1e3)
            assert not st.error()
    res = {name: {"ms_per_step_median": statistics.median(v), "ms_per_step": [round(x, 4) for x in v]}
           for name, v in times.items()}
    base = res["unreserved_n1"]["ms_per_step_median"]
    for v in res.values():
        v["vs_unreserved"] = round(v["ms_per_step_median"] / base, 4)
    out = {"batch": B, "config": "en100m", "capacity": K, "rounds": a.rounds, "steps_per_round": a.steps,
           "warmup_steps_per_round": 4, "order": [n for n, _ in SETTINGS], "device": torch.cuda.get_device_name(0),
           "settings": res}
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
