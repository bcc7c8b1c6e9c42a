"""Worker for tests/test_gpu_flow_matrix.py: started as a fresh process with PTTS_FLOW_RT=2 (read once per process), runs
two cluster cases of the flow-head matrix and writes {config: {cluster_kernel, ratio: {output: err / E32}}} as JSON."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from flow_ref import flow_weights  # noqa: E402
from test_gpu_flow_matrix import check_path, compare, run_head, seed_of  # noqa: E402


def main():
    from pocket_tts_amd.engine import Engine

    assert os.environ.get("PTTS_FLOW_RT") == "2"
    res = {}
    for name, B in (("F256", 33), ("F64", 17)):
        cfg, W = flow_weights(name)
        eng = Engine(cfg, W, "cuda:0")
        try:
            steps = run_head(eng, B, 2, seed_of(name, B, "rt2"))
        finally:
            eng.close()
        for s in steps:
            check_path(s["prof"], True, 2, False)
        ratio = compare(steps, cfg, W, 2, None, (name, "cluster RT=2", "plain"))
        res[name] = dict(cluster_kernel=[k for s, k in steps[0]["prof"] if s == "flow.cluster"][0], ratio=ratio)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main()
