"""Long-form probe: one text of about 64 sentences through `ContinuousBatcher(slots=64)` with the request's chunks one after
the other (window 1, the behaviour before `parallel_chunks`) and 4, 16 and 64 at a time, on bench.py's synthetic en100m model
with one voice, in one process on one engine.

    python tools/longform_probe.py [--config en100m] [--sentences 64] [--windows 1,4,16,64] [--out profiles/longform_probe.json]

For each window: wall time, scheduler steps (`cb.g`) and audio seconds per second.  Fixed-length chunks (EOS threshold +inf),
as in bench.py, so a chunk of n tokens runs `estimate_max_gen_len(n)` frames and the sentences, 26 to 48 characters long,
make chunks of different lengths.  Then the same once more with `--short` (32) short requests submitted behind the long one:
what the window costs the others, as the time until the last of them has finished.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))


def _run(cb, voice, text, window, shorts, frame_s, frame_samples):
    """one long request at `window` with `shorts` short texts behind it, the scheduler driven from here"""
    import queue

    g0 = cb.g
    t0 = time.perf_counter()
    long = cb.submit(voice, text, parallel_chunks=window)
    others = [cb.submit(voice, t) for t in shorts]
    samples = {r.id: 0 for r in [long, *others]}
    left, t_others = {r.id: r for r in [long, *others]}, None

    def pull():  # the consumers: what has arrived is counted and let go (an item keeps its whole frame of 64 rows alive)
        nonlocal t_others
        for r in list(left.values()):
            try:
                while True:
                    item = r._q.get_nowait()
                    if item is None:
                        del left[r.id]
                        if t_others is None and others and not any(o.id in left for o in others):
                            t_others = time.perf_counter() - t0
                        break
                    samples[r.id] += item.shape[0]
            except queue.Empty:
                pass

    while cb.step():
        pull()
    cb.run_until_idle()
    pull()
    wall = time.perf_counter() - t0
    assert not left
    n_long = samples[long.id]
    n_others = sum(samples[r.id] for r in others)
    out = dict(window=window, wall_ms=round(wall * 1e3, 1), steps=cb.g - g0, frames=n_long // frame_samples,
               audio_s_per_s=round((n_long + n_others) / frame_samples * frame_s / wall, 1))
    if shorts:
        out.update(short_requests=len(shorts), short_frames=n_others // frame_samples,
                   short_all_done_ms=round((wall if t_others is None else t_others) * 1e3, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="en100m", choices=["en100m", "24l", "tiny"])
    ap.add_argument("--sentences", type=int, default=64)
    ap.add_argument("--windows", default="1,4,16,64")
    ap.add_argument("--short", type=int, default=32, help="short requests submitted alongside in the second pass")
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--voice-len", type=int, default=126)
    ap.add_argument("--temp", type=float, default=0.7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    os.environ.setdefault("PTTS_TUNE_CACHE", str(REPO / "profiles" / "tune_cache_mi355x.txt"))
    os.environ.setdefault("PTTS_TUNE_CACHE_OUT", "")
    import logging

    import torch

    from bench import FRAME_S, _CharTokenizer
    from pocket_tts_amd.batching import ContinuousBatcher
    from pocket_tts_amd.config import named_config
    from pocket_tts_amd.engine import Engine
    from pocket_tts_amd.text import estimate_max_gen_len, split_into_best_sentences
    from pocket_tts_amd.tts_model import TTSModel, _export_lm_state
    from pocket_tts_amd.weights import generate_state_dict

    logging.getLogger("pocket_tts_amd").setLevel(logging.ERROR)  # "max length without EOS" per chunk is expected
    dev = torch.device("cuda:0")
    cfg = named_config(args.config)
    eng = Engine(cfg, generate_state_dict(cfg, 0), dev)
    model = TTSModel(eng, cfg, _CharTokenizer(cfg.flow_lm.lookup_table.n_bins), args.temp, 1, None, float("inf"))
    vst = eng.new_lm_state(1, args.voice_len)
    g = torch.Generator().manual_seed(0)
    eng.lm_prefill(vst, (torch.randn(1, args.voice_len, eng.D, generator=g) * 0.1).to(dev))
    voice = _export_lm_state(eng, vst, args.voice_len)
    vst.close()

    # sentences of 26 .. 48 characters (one token each): no two of them fit one chunk of 50 tokens
    words = "the quick brown fox jumps over the lazy dog and runs far away from here "
    text = " ".join((words * 2)[:26 + (7 * i) % 22].rstrip() + "." for i in range(args.sentences))
    chunks = split_into_best_sentences(model.tokenizer.encode, model.tokenizer.sp, text, 50,
                                       model.pad_with_spaces_for_short_inputs, model.remove_semicolons)
    gens = [estimate_max_gen_len(len(model.tokenizer.encode(c)), cfg.mimi.frame_rate) for c in chunks]
    shorts = [f"Short {i:02d}." for i in range(args.short)]
    windows = [int(w) for w in args.windows.split(",")]
    out = dict(config=args.config, slots=args.slots, chunks=len(chunks), frames_per_chunk=[min(gens), max(gens)],
               frames=sum(gens), runs=[], runs_with_short_requests=[])
    cb = ContinuousBatcher(model, slots=args.slots, capacity=640, parallel_chunks=max(windows))
    try:
        _run(cb, voice, text, max(windows), shorts, FRAME_S, eng.frame_samples)  # warm-up: not reported
        for key, others in (("runs", []), ("runs_with_short_requests", shorts)):
            for w in windows:
                eng.sync()
                r = _run(cb, voice, text, w, others, FRAME_S, eng.frame_samples)
                assert r["frames"] == sum(gens), (r, sum(gens))
                out[key].append(r)
                print(json.dumps(r), flush=True)
    finally:
        cb.close()
    eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
