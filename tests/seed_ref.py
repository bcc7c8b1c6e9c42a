"""Oracle side of the per-request seed tests: the reference's generation loop (`oracle.np_oracle`) fed with the noise a
seeded request draws on the device, restated by `noise_ref.row_noise`: step j of text chunk i of a request seeded S uses
`row_noise(chunk_seed(S, i), j, 0, ldim, temp, clamp)`.

CASES are the (text, seed, max_tokens) the GPU tests run at TEMP.  They were picked with `margins()` below (CPU only) so
that every EOS logit of every case keeps at least EOS_MARGIN from the threshold: frame counts are then exact decisions,
not roundings.  The GPU tests assert that margin for every case."""

from pathlib import Path

import numpy as np

from noise_ref import row_noise

G = Path(__file__).parent / "golden"
TEMP = 0.7
EOS_THRESHOLD = -4.0
EOS_MARGIN = 1e-3  # the distance from the threshold at which the project takes EOS decisions as exact
LONG_TEXT = "Hello world. This is a test. How are you today? This is a longer sentence, with several clauses."
CASES = [
    ("Hello world. This is a test.", 7, 50),
    ("ok", 12345, 50),
    ("How are you today?", 2 ** 62 + 3, 50),
    ("Short one.", 0, 50),
    ("Another request arrives while the others are running.", 99, 50),
    (LONG_TEXT, 2024, 12),
]


def _tiny():
    import safetensors.numpy
    import sentencepiece

    from pocket_tts_amd.config import load_config
    from pocket_tts_amd.weights import generate_state_dict

    cfg = load_config(G / "e2e_tiny.yaml")
    return (cfg, generate_state_dict(cfg, 0), safetensors.numpy.load_file(str(G / "e2e_voice.safetensors")),
            sentencepiece.SentencePieceProcessor(str(G / "e2e_sp.model")))


def chunk_plan(cfg, sp, text, max_tokens):
    """[(chunk text, token ids [1, T], max_gen_len, frames_after_eos)] as `TTSModel.generate_audio_stream` runs them"""
    from pocket_tts_amd.text import estimate_max_gen_len, prepare_text_prompt, split_into_best_sentences

    enc = lambda s: sp.encode(s, out_type=int)  # noqa: E731
    plan = []
    for chunk in split_into_best_sentences(enc, sp, text, max_tokens, cfg.pad_with_spaces_for_short_inputs,
                                           cfg.remove_semicolons):
        _, guess = prepare_text_prompt(chunk, cfg.pad_with_spaces_for_short_inputs, cfg.remove_semicolons)
        fae = cfg.model_recommended_frames_after_eos if cfg.model_recommended_frames_after_eos is not None else guess + 2
        toks = np.array(enc(chunk))[None]
        plan.append((chunk, toks, estimate_max_gen_len(toks.shape[1], cfg.mimi.frame_rate), fae))
    return plan


def seeded_noise(seed, chunk, steps, ldim, temp=TEMP, clamp=None):
    """the LSD start points of `steps` steps of one chunk, f32 [steps][1, ldim]"""
    from pocket_tts_amd.engine import chunk_seed

    cs = chunk_seed(seed, chunk)
    return [row_noise(cs, j, 0, ldim, temp, clamp).astype(np.float32)[None] for j in range(steps)]


def oracle_seeded(text, seed, max_tokens=50, temp=TEMP, clamp=None, tiny=None):
    """The oracle's generation of a seeded request: one dict per text chunk with the prefilled token ids, the latents
    [n, 1, ldim], every step's EOS logit, the EOS step and the frame count."""
    from oracle import np_oracle as O

    cfg, W, voice, sp = tiny or _tiny()
    lm = O.FlowLM(cfg, W)
    out = []
    for i, (chunk, toks, gen, fae) in enumerate(chunk_plan(cfg, sp, text, max_tokens)):
        T = voice["transformer.layers.0.self_attn/cache"].shape[2]
        st = lm.init_state(1, T + toks.shape[1] + gen)
        for li, s in enumerate(st):
            s["cache"][:, :, :T] = voice[f"transformer.layers.{li}.self_attn/cache"]
            s["offset"] = T
        lm.prefill(st, lm.embed_text(toks))
        lat, logits, eos_step = O.autoregressive_generation(lm, st, gen, fae, seeded_noise(seed, i, gen, lm.ldim, temp, clamp),
                                                            1, EOS_THRESHOLD)
        out.append(dict(chunk=chunk, tokens=toks, gen=gen, fae=fae, lat=lat, logits=logits.reshape(-1), eos_step=eos_step,
                        frames=lat.shape[0], t_voice=T))
    return out


def margins(cases=CASES):
    """min |logit - threshold| over every step of every case (authoring aid; the GPU tests assert it per case)"""
    tiny = _tiny()
    res = []
    for text, seed, mt in cases:
        chunks = oracle_seeded(text, seed, mt, tiny=tiny)
        res.append((text, seed, min(float(np.abs(c["logits"] - EOS_THRESHOLD).min()) for c in chunks),
                    [c["frames"] for c in chunks], [c["eos_step"] for c in chunks]))
    return res


if __name__ == "__main__":
    for row in margins():
        print(row)
