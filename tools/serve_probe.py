"""Server throughput probe: the HTTP app of pocket_tts_amd/server.py driven in-process (plain ASGI calls, no socket) with
N concurrent requests of the text bench.py's API leg uses, against `ContinuousBatcher` run directly on the same workload
(bench.py --full reports that figure as `continuous_batcher_xrt`), in one process on one engine.

    python tools/serve_probe.py [--config en100m] [--requests 64] [--reps 3] [--out profiles/serve_probe.json]

Reports aggregate audio seconds per second for both, their ratio, and the p50 / p99 time from sending a request to
its first audio byte (the chunk after the WAV header).  Fixed-length requests (EOS threshold +inf), as in bench.py.

    python tools/serve_probe.py --traffic mixed [--voices 4] [...]

Mixed traffic, the batcher only: the requests' texts have pairwise different token counts (8 .. 7 + requests) and are dealt
over `--voices` voices of different lengths, all submitted before the first step.  Reports the admission time (submission
to the end of the scheduler's first iteration: every request prefilled and in its slot, one step enqueued) and the
aggregate audio seconds per second.
"""

from __future__ import annotations

import argparse
import asyncio
import json
import os
import sys
import tempfile
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))


async def _post(app, body: bytes, ctype: str):
    """one POST /tts through the app's ASGI callable: (time to first audio byte, total time, body bytes)"""
    t0 = time.perf_counter()
    first, n, status = None, 0, None
    pending = [{"type": "http.request", "body": body, "more_body": False}]
    never = asyncio.Event()

    async def receive():
        if pending:
            return pending.pop()
        await never.wait()  # the client stays connected

    async def send(msg):
        nonlocal first, n, status
        if msg["type"] == "http.response.start":
            status = msg["status"]
        elif msg["type"] == "http.response.body" and msg.get("body"):
            n += len(msg["body"])
            if first is None and n > 44:
                first = time.perf_counter() - t0

    scope = {"type": "http", "asgi": {"version": "3.0"}, "http_version": "1.1", "method": "POST", "scheme": "http",
             "path": "/tts", "raw_path": b"/tts", "query_string": b"", "root_path": "",
             "headers": [(b"content-type", ctype.encode()), (b"content-length", str(len(body)).encode())],
             "client": ("127.0.0.1", 1), "server": ("probe", 80)}
    await app(scope, receive, send)
    assert status == 200, status
    return first, time.perf_counter() - t0, n


def _mixed(args, eng, cfg, model, g):
    """64 requests of pairwise different token counts over a few voices through the batcher"""
    import numpy as np
    import torch

    from bench import FRAME_S
    from pocket_tts_amd.batching import ContinuousBatcher
    from pocket_tts_amd.tts_model import _export_lm_state

    B = args.requests
    voices = []
    for v in range(args.voices):
        n = args.voice_len - 7 * v  # voices of different lengths
        vst = eng.new_lm_state(1, n)
        eng.lm_prefill(vst, (torch.randn(1, n, eng.D, generator=g) * 0.1).to(eng.device))
        voices.append(_export_lm_state(eng, vst, n))
        vst.close()
    words = "the quick brown fox jumps over the lazy dog and runs far away from here "
    texts = [(words * 4)[:8 + i].replace(" ", "a") for i in range(B)]  # one token per character: 8 .. 7 + B tokens, no split
    cb = ContinuousBatcher(model, slots=B, capacity=640)  # voice + 73 tokens + 330 frames
    admit, wall, samples = [], [], set()
    try:
        seen = []
        inner = cb._admit_group

        def record(jobs, rows):
            seen.extend(j.tokens.shape[1] for j in jobs)
            return inner(jobs, rows)

        cb._admit_group = record
        for i in range(args.reps + 1):
            eng.sync()
            t0 = time.perf_counter()
            reqs = [cb.submit(voices[k % len(voices)], t, max_tokens=10 ** 6) for k, t in enumerate(texts)]
            cb.step()
            t1 = time.perf_counter()
            cb.run_until_idle()
            n = sum(chunk.shape[0] for r in reqs for chunk in r)
            dt = time.perf_counter() - t0
            samples.add(n)
            if i:
                admit.append(t1 - t0)
                wall.append(dt)
        assert len(seen) == B * (args.reps + 1) and len(set(seen[:B])) == B, "the token counts are not pairwise different"
        assert len(samples) == 1 and min(samples) > 0, samples
    finally:
        cb.close()
    frames = samples.pop() // eng.frame_samples
    audio = frames * FRAME_S
    return dict(config=args.config, traffic="mixed", requests=B, voices=len(voices), tokens=[min(seen), max(seen)],
                frames=frames, reps=args.reps, admission_ms=[round(a * 1e3, 2) for a in admit],
                admission_ms_median=float(np.median(admit)) * 1e3, wall_ms=[round(w * 1e3, 1) for w in wall],
                continuous_batcher_xrt=audio / float(np.median(wall)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="en100m", choices=["en100m", "24l", "tiny"])
    ap.add_argument("--requests", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--voice-len", type=int, default=126)
    ap.add_argument("--temp", type=float, default=0.7)
    ap.add_argument("--traffic", default="uniform", choices=["uniform", "mixed"])
    ap.add_argument("--voices", type=int, default=4, help="mixed traffic: number of voices")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    os.environ.setdefault("PTTS_TUNE_CACHE", str(REPO / "profiles" / "tune_cache_mi355x.txt"))
    os.environ.setdefault("PTTS_TUNE_CACHE_OUT", "")
    import logging
    import urllib.parse

    import numpy as np
    import torch

    from bench import FRAME_S, _CharTokenizer
    from pocket_tts_amd.batching import ContinuousBatcher
    from pocket_tts_amd.config import named_config
    from pocket_tts_amd.engine import Engine
    from pocket_tts_amd.server import create_app
    from pocket_tts_amd.text import estimate_max_gen_len
    from pocket_tts_amd.tts_model import TTSModel, _export_lm_state, export_model_state
    from pocket_tts_amd.weights import generate_state_dict

    logging.getLogger("pocket_tts_amd").setLevel(logging.ERROR)  # "max length without EOS" per request is expected
    dev = torch.device("cuda:0")
    cfg = named_config(args.config)
    eng = Engine(cfg, generate_state_dict(cfg, 0), dev)
    B = args.requests
    model = TTSModel(eng, cfg, _CharTokenizer(cfg.flow_lm.lookup_table.n_bins), args.temp, 1, None, float("inf"))
    vst = eng.new_lm_state(1, args.voice_len)
    g = torch.Generator().manual_seed(0)
    eng.lm_prefill(vst, (torch.randn(1, args.voice_len, eng.D, generator=g) * 0.1).to(dev))
    voice_state = _export_lm_state(eng, vst, args.voice_len)
    vst.close()
    if args.traffic == "mixed":
        out = _mixed(args, eng, cfg, model, g)
        eng.close()
        line = json.dumps(out)
        print(line)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(line + "\n")
        return
    texts = [f"The quick brown fox jumps {i:04d}." for i in range(B)]  # 32 tokens each, as bench.py's API leg
    frames = estimate_max_gen_len(32, cfg.mimi.frame_rate)
    audio = B * frames * FRAME_S
    out = dict(config=args.config, requests=B, frames_per_request=frames, reps=args.reps)

    # the batcher on its own (bench.py api_batch: continuous_batcher_xrt)
    cb = ContinuousBatcher(model, slots=B, capacity=512)
    try:
        ts = []
        for i in range(args.reps + 1):
            eng.sync()
            t0 = time.perf_counter()
            reqs = [cb.submit(voice_state, t) for t in texts]
            cb.run_until_idle()
            n = sum(chunk.shape[0] for r in reqs for chunk in r)
            dt = time.perf_counter() - t0
            assert n == B * frames * eng.frame_samples
            if i:
                ts.append(dt)
    finally:
        cb.close()
    out["continuous_batcher_xrt"] = audio / float(np.median(ts))

    # the server: same requests as form posts, all at once
    with tempfile.TemporaryDirectory() as vd:
        export_model_state(voice_state, Path(vd) / "probe.safetensors")
        app = create_app(model, slots=B, capacity=512, voices_dir=vd, default_voice="probe")
        bodies = [urllib.parse.urlencode({"text": t}).encode() for t in texts]

        async def run():
            async with app.router.lifespan_context(app):
                res = []
                for i in range(args.reps + 1):
                    t0 = time.perf_counter()
                    r = await asyncio.gather(*[_post(app, b, "application/x-www-form-urlencoded") for b in bodies])
                    dt = time.perf_counter() - t0
                    assert all(x[2] == 44 + 2 * (frames * eng.frame_samples + 4800) for x in r)
                    if i:
                        res.append((dt, [x[0] for x in r]))
                return res

        res = asyncio.run(run())
    walls = [dt for dt, _ in res]
    ttfb = np.array([t for _, f in res for t in f]) * 1e3
    out["server_xrt"] = audio / float(np.median(walls))
    out["server_over_batcher"] = out["server_xrt"] / out["continuous_batcher_xrt"]
    out["server_first_audio_ms_p50"] = float(np.percentile(ttfb, 50))
    out["server_first_audio_ms_p99"] = float(np.percentile(ttfb, 99))
    out["server_wall_ms"] = [round(w * 1e3, 1) for w in walls]
    eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
