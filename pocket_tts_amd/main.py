"""The reference's commands (pocket_tts/main.py) over the MI355X engine.

    python -m pocket_tts_amd generate --config cfg.yaml --voice voice.safetensors --text "..." \
        --output-path out.wav
    python -m pocket_tts_amd serve --config cfg.yaml --voices-dir voices/ --default-voice alba
    python -m pocket_tts_amd export-voice prompt.wav voice.safetensors --config cfg.yaml

`generate` writes 24 kHz mono 16-bit WAV followed by 200 ms of silence (reference data/audio.py:69-72,99-107);
`--sample-rate 8000|16000|44100|48000|...` resamples it on the GPU (resample.py).
`serve` runs the HTTP server of `server.py` (`GET /health`, `POST /tts` streaming the same WAV bytes) on a continuous
batcher, with per-request temperature, noise clamp, EOS threshold and seed, and with `--sample-rates 8000,16000,48000` a
per-request `sample_rate`, and with `--speeds 0.8,1.25,1.5` a per-request `speed` (pitch-preserving time-stretch on the GPU,
stretch.py; `generate --speed 1.25` is the same for one text), and with `--level` a per-request `gain_db` / `peak_dbfs`
(gain plus a look-ahead peak limiter on the GPU, level.py; `generate --gain-db 6 [--peak-dbfs -1]`), and with
`--pitches 17/16,5/4,4/5` a per-request `pitch` (a frequency ratio; pitch shift on the GPU, pitch.py; `generate --pitch 17/16`
or `generate --pitch-semitones 1` is the same for one text), and with `--loudness` a per-request `loudness_lufs` (a streaming
BS.1770 normaliser on the GPU, loudness.py; `generate --loudness-lufs -16 [--peak-dbfs -1]`), and with
`--encodings mulaw,alaw,pcm_f32le` a per-request `encoding` (G.711 or float samples, encoded on the GPU, encoding.py;
`generate --sample-rate 8000 --encoding mulaw` is the same for one text) and `container=raw` for the bytes without a WAV
header, and with `--tones telephone,warm,"hp:120;peak:3000:4"` a per-request `tone` (a parametric equaliser on the GPU,
tone.py; `generate --tone telephone` is the same for one text), and with `--dynamics speech,"threshold=-24;ratio=4"` a
per-request `dynamics` (a speech compressor on the GPU, dynamics.py; `generate --dynamics speech`), and with
`--true-peak` a per-request `peak_dbtp` in place of `peak_dbfs` (the ceiling as a BS.1770-4 true peak: a 4x oversampled
limiter and meter on the GPU, level.py; `generate --loudness-lufs -16 --peak-dbtp -1` logs the measured true peak), and with
`--parallel-chunks W` up to W sentences of a request at a time as rows of the batch, delivered in text order (batching.py;
`generate --parallel-chunks W` is the same for one text).  `export-voice` encodes an audio prompt (first 30 s)
into a voice-state file that `generate --voice` and the server's voices directory accept.
"""

from __future__ import annotations

import argparse
import logging
import struct
import sys

logger = logging.getLogger("pocket_tts_amd")

DEFAULT_TEXT = ("Hello world. I am Kyutai's Pocket TTS. I'm fast enough to run on small CPUs. "
                "I hope you'll like me.")


# the flags behind each request field of `ChainTable.for_request`, as `generate` names them when a rule refuses one
FLAGS = dict(sample_rate="--sample-rate", speed="--speed", pitch="--pitch / --pitch-semitones", tone="--tone",
             loudness_lufs="--loudness-lufs / --peak-dbfs", gain_db="--gain-db / --peak-dbfs", encoding="--encoding",
             compression="--compression", dynamics="--dynamics", peak_dbtp="--peak-dbtp")

_STREAM_FRAMES = 1_000_000_000  # streaming: the length is not known up front, the header announces this many samples


def _wav_header(n_samples: int, sample_rate: int, encoding: str = "pcm_s16le") -> bytes:
    """RIFF header of a mono file in `encoding` (encoding.py).  `pcm_s16le`: the 44 bytes `wave` writes.  The others are
    no PCM in the sense of the format and get what it asks of those: an 18-byte `fmt ` chunk (cbSize 0) with the encoding's
    format tag, a `fact` chunk with the number of samples, then `data`: 58 bytes."""
    from .encoding import BYTES_PER_SAMPLE, WAV_FORMAT_TAG

    bps = BYTES_PER_SAMPLE[encoding]
    data = bps * n_samples
    if encoding == "pcm_s16le":
        return struct.pack("<4sL4s4sLHHLLHH4sL", b"RIFF", 36 + data, b"WAVE", b"fmt ", 16, 1, 1, sample_rate, 2 * sample_rate,
                           2, 16, b"data", data)
    return struct.pack("<4sL4s4sLHHLLHHH4sLL4sL", b"RIFF", 50 + data, b"WAVE", b"fmt ", 18, WAV_FORMAT_TAG[encoding], 1,
                       sample_rate, bps * sample_rate, bps, 8 * bps, 0, b"fact", 4, n_samples, b"data", data)


def _wav_offsets(encoding: str):
    """(header length, offsets of the RIFF length, the `fact` sample count (None without one) and the `data` length)"""
    return (44, 4, None, 40) if encoding == "pcm_s16le" else (58, 4, 46, 54)


def wav_stream_bytes(chunks, sample_rate: int, encoding: str | None = None, header: bool = True):
    """The bytes of a streamed WAV: the provisional header, each chunk's frames as soon as it arrives, then 200 ms of
    silence.  `encoding` None or "pcm_s16le": 16-bit frames; fp32 chunks are clamped and converted like data/audio.py:79,
    int16 chunks (the batcher's `pcm_format="i16"`, or its "pcm_s16le") are already converted.  Another `encoding`
    (encoding.py): the chunks are what the encoder wrote, float32 for "pcm_f32le", uint8 for "mulaw" and "alaw", and their
    bytes are written as they come; the silence is the encoding's own (FF in mu-law, D5 in A-law: a zero byte there is a
    full-scale sample).  `header` False: the same without the header (the server's `container=raw`)."""
    import torch

    from . import encoding as rule

    enc = rule.check(encoding)
    if header:
        yield _wav_header(_STREAM_FRAMES, sample_rate, enc)
    for chunk in chunks:
        if enc == rule.PCM_S16LE:
            if chunk.dtype != torch.int16:
                chunk = (chunk.clamp(-1, 1) * 32767).short()
        elif chunk.dtype != rule.torch_dtype(enc):
            raise ValueError(f"encoding {enc!r}: expected {rule.torch_dtype(enc)} chunks, got {chunk.dtype}")
        yield chunk.cpu().numpy().tobytes()
    yield rule.silence(enc, int(sample_rate * 0.2))


def write_wav_stream(path, chunks, sample_rate: int, encoding: str | None = None) -> int:
    """fp32 chunks -> clamp, int16, raw frames (or, with `encoding`, the encoder's chunks as `wav_stream_bytes` takes them);
    200 ms of trailing silence.  Returns samples written.  A file gets the real lengths patched into its header at the end;
    stdout keeps the provisional one."""
    from . import encoding as rule

    enc = rule.check(encoding)
    head, at_riff, at_fact, at_data = _wav_offsets(enc)
    bps = rule.BYTES_PER_SAMPLE[enc]
    out = sys.stdout.buffer if path == "-" else open(path, "wb")
    n = 0
    with out:
        for b in wav_stream_bytes(chunks, sample_rate, encoding):
            out.write(b)
            n += len(b)
        n = (n - head) // bps
        if path != "-":
            out.seek(at_riff)
            out.write(struct.pack("<L", head - 8 + bps * n))
            if at_fact is not None:
                out.seek(at_fact)
                out.write(struct.pack("<L", n))
            out.seek(at_data)
            out.write(struct.pack("<L", bps * n))
    return n


def flac_stream_bytes(chunks, sample_rate: int, n: int):
    """The bytes of a streamed FLAC file: the stream header for blocks of `n` samples (total unknown), each chunk - one whole
    frame, a uint8 tensor or array as a flac request delivers it - as soon as it arrives, then the 200 ms of silence every
    container gets, as CONSTANT frames numbered on from the last one (`flac.py`).  An item of `chunks` may also be a list of
    chunks (`Request.iter_batches`): its frames leave as one item."""
    from . import flac

    yield flac.stream_header(sample_rate, n)
    count = 0
    for item in chunks:
        parts = []
        for chunk in item if isinstance(item, (list, tuple)) else (item,):
            data = chunk.cpu().numpy() if hasattr(chunk, "cpu") else chunk
            if str(data.dtype) != "uint8":
                raise ValueError(f"compression 'flac': expected uint8 chunks, one frame each, got {data.dtype}")
            parts.append(data.tobytes())
        yield b"".join(parts)
        count += len(parts)
    yield flac.silence(count, sample_rate, n)


def write_flac_stream(path, chunks, sample_rate: int, n: int) -> int:
    """`flac_stream_bytes` to a file or stdout ("-").  Returns samples written.  A file gets the total sample count patched
    into its STREAMINFO at the end; stdout keeps 0, "unknown"."""
    from . import flac

    out = sys.stdout.buffer if path == "-" else open(path, "wb")
    items = 0
    with out:
        for b in flac_stream_bytes(chunks, sample_rate, n):
            out.write(b)
            items += 1
        total = (items - 2) * int(n) + int(sample_rate) // 5  # all but the header and the tail are one frame each
        if path != "-":
            out.seek(0)
            out.write(flac.patch_total(flac.stream_header(sample_rate, n), total))
    return total


def parse_compression_list(text: str) -> list:
    """"flac" -> ["flac"] (the `serve --compressions` value)"""
    from .flac import normalise_compressions

    names = [t.strip() for t in text.split(",") if t.strip()]
    if not names:
        raise argparse.ArgumentTypeError("expected at least one compression")
    try:
        return normalise_compressions(names)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def parse_encoding_list(text: str) -> list:
    """"mulaw,alaw,pcm_f32le" -> ["mulaw", "alaw", "pcm_f32le"] (the `serve --encodings` value)"""
    from .encoding import normalise_encodings

    names = [t.strip() for t in text.split(",") if t.strip()]
    if not names:
        raise argparse.ArgumentTypeError("expected at least one encoding")
    try:
        normalise_encodings(names)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None
    return names


def parse_tone_list(text: str) -> list:
    """"telephone,warm,hp:120;peak:3000:4" -> ["telephone", "warm", "hp:120;peak:3000:4"] (the `serve --tones` value): tones
    are joined by commas, the bands of one tone by semicolons"""
    from .tone import normalise_tones

    names = [t.strip() for t in text.split(",") if t.strip()]
    try:
        if not normalise_tones(names):
            raise ValueError("expected at least one tone")
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None
    return names


def parse_dynamics_list(text: str) -> list:
    """"speech,threshold=-24;ratio=4" -> ["speech", "threshold=-24;ratio=4"] (the `serve --dynamics` value): settings are
    joined by commas, the pairs of one setting by semicolons"""
    from .dynamics import normalise_dynamics

    names = [t.strip() for t in text.split(",") if t.strip()]
    try:
        normalise_dynamics(names)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None
    return names


def parse_rate_list(text: str) -> list:
    """"8000,16000,48000" -> [8000, 16000, 48000] (the `serve --sample-rates` value)"""
    try:
        rates = [int(t) for t in text.split(",") if t.strip()]
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected integers separated by commas, got {text!r}") from None
    if not rates:
        raise argparse.ArgumentTypeError("expected at least one rate")
    return rates


def parse_speed_list(text: str) -> list:
    """"0.8,1.25,1.5" -> [0.8, 1.25, 1.5] (the `serve --speeds` value)"""
    try:
        speeds = [float(t) for t in text.split(",") if t.strip()]
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected numbers separated by commas, got {text!r}") from None
    if not speeds:
        raise argparse.ArgumentTypeError("expected at least one speed")
    return speeds


def parse_pitch_list(text: str) -> list:
    """"17/16,5/4,0.8" -> [1.0625, 1.25, 0.8] (the `serve --pitches` value): ratios as numbers or "P/Q"""
    from .pitch import fraction

    try:
        pitches = [float(fraction(t)) for t in text.split(",") if t.strip()]
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None
    if not pitches:
        raise argparse.ArgumentTypeError("expected at least one pitch")
    return pitches


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="pocket-tts")
    sub = ap.add_subparsers(dest="command", required=True)
    g = sub.add_parser("generate", help="Generate speech")
    g.add_argument("--text", default=None, help="Text to generate ('-' reads stdin)")
    g.add_argument("--voice", default=None, help="Voice state (.safetensors exported by export_model_state)")
    g.add_argument("-q", "--quiet", action="store_true", help="Disable logging output")
    g.add_argument("--language", default=None)
    g.add_argument("--config", default=None, help="Path to a local model config .yaml")
    g.add_argument("--lsd-decode-steps", type=int, default=1)
    g.add_argument("--temperature", type=float, default=0.7)
    g.add_argument("--noise-clamp", type=float, default=None)
    g.add_argument("--eos-threshold", type=float, default=-4.0)
    g.add_argument("--frames-after-eos", type=int, default=None)
    g.add_argument("--seed", type=int, default=None,
                   help="Seed of the noise in [0, 2**63): the same seed, text and settings give the same audio again")
    g.add_argument("--sample-rate", type=int, default=None,
                   help="Output sample rate (e.g. 8000, 16000, 22050, 44100, 48000; default: the codec's 24000), resampled on the GPU")
    g.add_argument("--speed", type=float, default=None,
                   help="Speaking rate in [0.5, 2] (e.g. 0.8, 1.25, 1.5; default 1.0): time-stretched on the GPU at constant pitch")
    g.add_argument("--pitch", default=None, metavar="P/Q",
                   help="Pitch as a frequency ratio in [0.5, 2], a fraction P/Q with P, Q <= 20 or a number (e.g. 17/16, 5/4, "
                        "0.8; default 1): shifted on the GPU, the formants move with it")
    g.add_argument("--pitch-semitones", type=float, default=None, metavar="ST",
                   help="Pitch in semitones, in [-12, 12]: the admissible ratio nearest to 2^(ST/12) is used")
    g.add_argument("--gain-db", type=float, default=None,
                   help="Output gain in dB, in [-40, 24], with a peak limiter that guarantees the ceiling (default: none)")
    g.add_argument("--loudness-lufs", type=float, default=None, metavar="LUFS",
                   help="Loudness target in LUFS, in [-40, -10] (e.g. -16, -23): normalised on the GPU by ITU-R BS.1770-4, sentence "
                        "by sentence, with the peak limiter behind it; excludes --gain-db (default: none)")
    g.add_argument("--tone", default=None, metavar="TONE",
                   help="Tone: a preset (telephone, warm, bright, presence, small_speaker, deess) or a band list "
                        "kind:f0[:gain_db[:q]];... with kinds hp, lp, peak, lowshelf, highshelf, e.g. \"hp:120;peak:3000:4\": "
                        "equalised on the GPU, with the peak limiter behind it (default: none)")
    g.add_argument("--peak-dbfs", type=float, default=None,
                   help="Ceiling of the peak limiter in dBFS, in [-20, 0] (default -1); only together with --gain-db, "
                        "--loudness-lufs, --tone or --dynamics")
    g.add_argument("--peak-dbtp", type=float, default=None,
                   help="Ceiling of the limiter as a true peak in dBTP (ITU-R BS.1770-4: the peak of the 4x oversampled "
                        "waveform), in [-20, 0], e.g. -1; in place of --peak-dbfs, which it excludes.  The measured true peak "
                        "is logged when done")
    g.add_argument("--dynamics", default=None, metavar="SETTING",
                   help="Dynamics: a compressor preset (speech, gentle, broadcast, telephone) or key=value pairs joined by ';' "
                        "with the keys threshold, ratio, knee, attack, release, makeup, e.g. \"threshold=-24;ratio=4\": "
                        "compressed on the GPU behind the tone and in front of the loudness measurement, with the peak "
                        "limiter behind (default: none)")
    g.add_argument("--encoding", default=None, choices=["pcm_s16le", "pcm_f32le", "mulaw", "alaw"],
                   help="Sample encoding of the WAV, encoded on the GPU: 16-bit PCM, 32-bit float, or ITU-T G.711 mu-law / A-law "
                        "(telephony; use it with --sample-rate 8000).  Default: 16-bit PCM, converted on the host")
    g.add_argument("--compression", default=None, choices=["flac"],
                   help="Write a .flac file: lossless frames encoded on the GPU, which decode to the very samples of the 16-bit "
                        "WAV; only with --encoding pcm_s16le or none (default: none, a WAV)")
    g.add_argument("--output-path", default=None, help="Default: ./tts_output.wav, or ./tts_output.flac with --compression flac")
    g.add_argument("--device", default="cuda:0")
    g.add_argument("--max-tokens", type=int, default=50)
    g.add_argument("--parallel-chunks", type=int, default=1, metavar="W",
                   help="Run up to W sentences of a long text at a time, as rows of one batch; the audio comes out in text "
                        "order (default 1: one after the other)")
    g.add_argument("--quantize", action="store_true")
    g.add_argument("--codec-bf16", action="store_true",
                   help="bf16 weights + activations in the Mimi codec (fp32 accumulate; not in the reference, ~44 dB SNR)")

    s = sub.add_parser("serve", help="Start the HTTP server (POST /tts streams a WAV)")
    s.add_argument("--host", default="localhost", help="Host to bind to")
    s.add_argument("--port", type=int, default=8000, help="Port to bind to")
    s.add_argument("--language", default=None)
    s.add_argument("--config", default=None, help="Path to a local model config .yaml")
    s.add_argument("--quantize", action="store_true")
    s.add_argument("--codec-bf16", action="store_true")
    s.add_argument("--device", default="cuda:0")
    s.add_argument("--temperature", type=float, default=0.7, help="Default temperature of a request")
    s.add_argument("--lsd-decode-steps", type=int, default=1, help="Default lsd_decode_steps of a request")
    s.add_argument("--max-lsd-decode-steps", type=int, default=None,
                   help="Largest lsd_decode_steps a request may ask for (default: --lsd-decode-steps).  A step takes as "
                        "long as its slowest rows: one request at a high count slows every request in the batch")
    s.add_argument("--sample-rates", type=parse_rate_list, default=None, metavar="R1,R2,...",
                   help="Output sample rates a request may choose with the form field sample_rate, e.g. 8000,16000,48000 "
                        "(the codec's own rate is always available)")
    s.add_argument("--speeds", type=parse_speed_list, default=None, metavar="S1,S2,...",
                   help="Speaking rates a request may choose with the form field speed, e.g. 0.8,1.25,1.5 (1.0 is always "
                        "available); each must give whole hops per frame at one of the server's rates")
    s.add_argument("--pitches", type=parse_pitch_list, default=None, metavar="P1/Q1,P2/Q2,...",
                   help="Pitch ratios a request may choose with the form field pitch, e.g. 17/16,5/4,4/5 (1 is always "
                        "available); each must give whole hops per frame on one of the server's lines")
    s.add_argument("--loudness", action="store_true",
                   help="Requests may set a loudness target with the form field loudness_lufs (BS.1770 normaliser plus the "
                        "peak limiter on the GPU)")
    s.add_argument("--encodings", type=parse_encoding_list, default=None, metavar="E1,E2,...",
                   help="Sample encodings a request may choose with the form field encoding, among mulaw, alaw and pcm_f32le "
                        "(pcm_s16le is always available); encoded on the GPU")
    s.add_argument("--compressions", type=parse_compression_list, default=None, metavar="C1,...",
                   help="Compressions a request may choose with the form field container, i.e. flac: lossless frames encoded on "
                        "the GPU, streamed as audio/flac")
    s.add_argument("--tones", type=parse_tone_list, default=None, metavar="T1,T2,...",
                   help="Tones a request may choose with the form field tone: presets or band lists, e.g. "
                        "telephone,warm,hp:120;peak:3000:4 (bands are joined by ';', tones by ','); equalised on the GPU, with "
                        "the peak limiter behind")
    s.add_argument("--dynamics", type=parse_dynamics_list, default=None, metavar="S1,S2,...",
                   help="Compressor settings a request may choose with the form field dynamics: presets or key=value lists, "
                        "e.g. speech,threshold=-24;ratio=4 (pairs are joined by ';', settings by ','); compressed on the GPU, "
                        "with the peak limiter behind")
    s.add_argument("--level", action="store_true",
                   help="Requests may set their output level with the form fields gain_db and peak_dbfs (gain plus a peak "
                        "limiter on the GPU)")
    s.add_argument("--true-peak", action="store_true",
                   help="Requests may state their ceiling as a true peak with the form field peak_dbtp in place of peak_dbfs "
                        "(a 4x oversampled limiter and meter on the GPU; brings the limiter with it, like --level)")
    s.add_argument("--noise-clamp", type=float, default=None, help="Default noise clamp of a request")
    s.add_argument("--eos-threshold", type=float, default=-4.0, help="Default EOS threshold of a request")
    s.add_argument("--slots", type=int, default=64, help="Utterances decoded together")
    s.add_argument("--parallel-chunks", type=int, default=1, metavar="W",
                   help="Every request runs up to W sentences of its text at a time in slots of their own; a request never "
                        "holds more than W slots (default 1: one after the other)")
    s.add_argument("--capacity", type=int, default=1024,
                   help="KV positions per slot: voice + text chunk + generated frames (a 30 s voice prompt is 376)")
    s.add_argument("--voices-dir", default=None, help="Directory of <name>.safetensors voice states for voice_url=<name>")
    s.add_argument("--default-voice", default=None, help="Voice name used when a request names none")
    s.add_argument("-q", "--quiet", action="store_true", help="Disable logging output")

    x = sub.add_parser("export-voice", help="Encode an audio prompt into a voice-state .safetensors file")
    x.add_argument("audio_path", help="Audio prompt (WAV; the first 30 s are used)")
    x.add_argument("export_path", help="Output .safetensors file")
    x.add_argument("-q", "--quiet", action="store_true", help="Disable logging output")
    x.add_argument("--language", default=None)
    x.add_argument("--config", default=None, help="Path to a local model config .yaml")
    x.add_argument("--device", default="cuda:0")
    return ap


def serve_app(args) -> int:
    import dataclasses

    import uvicorn

    from .output_chain import ChainSpec
    from .server import create_app
    from .tts_model import TTSModel

    model = TTSModel.load_model(language=args.language, config=args.config, temp=args.temperature,
                                lsd_decode_steps=args.lsd_decode_steps, noise_clamp=args.noise_clamp,
                                eos_threshold=args.eos_threshold, quantize=args.quantize, codec_bf16=args.codec_bf16,
                                device=args.device)
    # the model's noise clamp reaches every request as a per-request setting (server.py); the flags of the output chain
    # carry the names of its options
    app = create_app(model, slots=args.slots, capacity=args.capacity, voices_dir=args.voices_dir,
                     default_voice=args.default_voice, max_lsd_decode_steps=args.max_lsd_decode_steps,
                     parallel_chunks=args.parallel_chunks, **{f.name: getattr(args, f.name) for f in dataclasses.fields(ChainSpec)})
    uvicorn.run(app, host=args.host, port=args.port, log_level="error" if args.quiet else "info")
    return 0


def export_voice_app(args) -> int:
    from .tts_model import TTSModel, export_model_state

    model = TTSModel.load_model(language=args.language, config=args.config, device=args.device)
    state = model.get_state_for_audio_prompt(args.audio_path, truncate=True)
    export_model_state(state, args.export_path)
    logger.info("Voice state written in %s", args.export_path)
    return 0


def cli_app(argv=None) -> int:
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.ERROR if args.quiet else logging.INFO)
    if args.command == "serve":
        return serve_app(args)
    if args.command == "export-voice":
        return export_voice_app(args)
    text = DEFAULT_TEXT if args.text is None else args.text
    if text == "-":
        text = sys.stdin.read()
    if not text.strip():
        logger.error("No input received from stdin.")
        return 1
    if args.parallel_chunks < 1:
        logger.error("--parallel-chunks: must be at least 1, got %d", args.parallel_chunks)
        return 1
    from .tts_model import TTSModel

    model = TTSModel.load_model(language=args.language, config=args.config, temp=args.temperature,
                                lsd_decode_steps=args.lsd_decode_steps, noise_clamp=args.noise_clamp,
                                eos_threshold=args.eos_threshold, quantize=args.quantize, codec_bf16=args.codec_bf16,
                                device=args.device)
    # generate_audio_stream is a generator and would refuse its arguments only once write_wav_stream has opened the file:
    # walk the request's chain here, so the message names the flag at fault (the first in chain order)
    from .output_chain import ChainTable

    native, fs = int(model.sample_rate), model.engine.frame_samples
    try:
        if args.pitch is not None and args.pitch_semitones is not None:
            raise ValueError("give one of --pitch and --pitch-semitones")
        pitch = args.pitch
        if args.pitch_semitones is not None:  # semitones become the nearest ratio the rule admits behind the rate and the speed
            from .pitch import nearest

            pitch, cents = nearest(args.pitch_semitones, *ChainTable.line_of(native, fs, args.sample_rate, args.speed)[2])
            logger.info("--pitch-semitones %g: pitch %s, %+.1f cents from the request", args.pitch_semitones, pitch, cents)
        _, request = ChainTable.for_request(native, fs, args.sample_rate, args.speed, args.gain_db, args.peak_dbfs, pitch,
                                            args.loudness_lufs, args.encoding, args.tone, args.compression, args.dynamics,
                                            args.peak_dbtp)
    except ValueError as e:  # a `RequestError` names its field; the others are those of the two pitch flags above
        logger.error("%s: %s", FLAGS[getattr(e, "field", "pitch")], e)
        return 1
    voice = args.voice if args.voice is not None else "alba"
    state = model.get_state_for_audio_prompt(voice)
    request["gain_db"] = args.gain_db  # as it came: the limiter's 0 dB behind a tone alone is for the model to fill in
    chunks = model.generate_audio_stream(state, text, frames_after_eos=args.frames_after_eos, max_tokens=args.max_tokens,
                                         seed=args.seed, parallel_chunks=args.parallel_chunks, **request)
    rate = args.sample_rate or model.sample_rate
    if args.output_path is None:
        args.output_path = "./tts_output.flac" if args.compression else "./tts_output.wav"
    if args.compression:
        n = ChainTable.line_of(native, fs, args.sample_rate, args.speed)[2][1]  # the samples of a frame behind rate and speed
        write_flac_stream(args.output_path, chunks, rate, n)
    else:
        write_wav_stream(args.output_path, chunks, rate, args.encoding)
    if args.output_path != "-":
        logger.info("Results written in %s", args.output_path)
    if args.peak_dbtp is not None and model.last_true_peak is not None:
        from .level import dbtp

        # what `level.true_peak` reads on the samples before their encoding: the device meter's maximum over the sentences
        logger.info("true peak %.2f dBTP", dbtp(model.last_true_peak))
    return 0


if __name__ == "__main__":
    sys.exit(cli_app())
