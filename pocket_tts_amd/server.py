"""HTTP server on the continuous batcher: the reference's `pocket-tts serve` (`/health`, `POST /tts` streaming a WAV,
pocket_tts/main.py:121-214) with every request decoded in one shared batch.

`POST /tts` takes the reference's form fields - `text`, `voice_url` (here: the name of a voice state in the voices
directory) or the file `voice_wav` - plus this server's optional per-request settings `temperature`, `noise_clamp`,
`eos_threshold`, `frames_after_eos`, `lsd_decode_steps`, `seed` (the same seed, text and settings give the same noise
again), `sample_rate` (one of the rates the server was started with, or the codec's own) and `speed` (one of the speaking
rates the server was started with that the plan rule of `stretch.py` admits at the request's rate, or 1.0), `pitch` (one
of the frequency ratios the server was started with that the plan rule of `pitch.py` admits behind the request's rate and
speed, a number or "P/Q", or 1), and on a
server started with `level` the output level `gain_db` with its ceiling `peak_dbfs` (`level.py`), and on a server started
with `loudness` the loudness target `loudness_lufs` (`loudness.py`; with `peak_dbfs` as its ceiling, without `gain_db`).
On a server started with `true_peak` the field `peak_dbtp` states that ceiling as a true peak in place of `peak_dbfs`
(`level.py`, "True-peak mode"; both together, or the field on a server started without, get a 400).  The body is the WAV the `generate` command writes (`main.wav_stream_bytes`):
the streaming header, the 16-bit frames as each is decoded, 200 ms of silence.  On a server started with `encodings` the
field `encoding` chooses the sample encoding among them and `pcm_s16le` (`encoding.py`: ITU-T G.711 `mulaw` / `alaw`, or
`pcm_f32le`), encoded on the GPU; header and silence follow it.  On a server started with `compressions` `container=flac`
answers `audio/flac`, lossless frames encoded on the GPU (`flac.py`).  `container=raw` (default `wav`) leaves the header out: the
encoded samples and the trailing silence as `application/octet-stream`, with the response headers `X-Audio-Encoding` and
`X-Sample-Rate` - what a media-stream gateway forwards.  On a server started with `tones` the field `tone` chooses one of
them (`tone.py`: a preset such as `telephone`, or a band list), equalised on the GPU with the peak limiter behind it
(`peak_dbfs` is then its ceiling); a tone the request's rate does not admit gets a 400 with those it admits.  On a server
started with `dynamics` the field `dynamics` chooses one of its compressor settings (`dynamics.py`: a preset such as
`speech`, or key=value pairs), compressed on the GPU behind the tone with the peak limiter behind it; a setting that is not
configured gets a 400 with the list of those that are.  Instead of `text` and a voice a request may send `script`, a JSON
list of {"voice": <name>, "text": <text>} objects (at most 256): one request, one stream, each entry spoken in its voice of
the voices directory, in order; a malformed value, an empty list, an entry without text or with an unknown voice gets a 400
that names the entry.  On a server started with `parallel_chunks` W the sentences of a request run up to W at a time.

FastAPI's `Form` / `File` need the `python-multipart` package; the two form encodings are parsed here instead, with
`urllib.parse` and the standard library's `email` header parser.
"""

from __future__ import annotations

import email
import math
import os
import re
import tempfile
import threading
import urllib.parse
from contextlib import asynccontextmanager
from pathlib import Path

from fastapi import FastAPI, Request
from fastapi.responses import HTMLResponse, JSONResponse, StreamingResponse
from starlette.concurrency import run_in_threadpool

OFFLINE_PREFIXES = ("hf://", "http://", "https://")
_VOICE_NAME = re.compile(r"[A-Za-z0-9_][A-Za-z0-9_.-]*")

INDEX_HTML = """<!doctype html>
<html><head><meta charset="utf-8"><title>Pocket TTS</title></head>
<body>
<h1>Pocket TTS</h1>
<form action="/tts" method="post" enctype="multipart/form-data">
<p><textarea name="text" rows="4" cols="60">Hello world.</textarea></p>
<p>Voice name <input name="voice_url"> or WAV prompt <input type="file" name="voice_wav" accept=".wav"></p>
<p>Script <input name="script" size="60"> instead of text and voice: a JSON list such as
[{"voice": "alba", "text": "Hello."}, {"voice": "marius", "text": "Hi."}] (clear the text and the voice above to use
it; empty: the text above)</p>
<p>LSD decode steps <input name="lsd_decode_steps" size="3"> (empty: the server's default)</p>
<p>Seed <input name="seed" size="20"> (empty: a take that cannot be repeated)</p>
<p>Sample rate <input name="sample_rate" size="6"> Hz (empty: the model's own rate)</p>
<p>Speed <input name="speed" size="5"> (empty: 1.0)</p>
<p>Pitch <input name="pitch" size="6"> as a frequency ratio, e.g. 17/16 or 0.8 (empty: 1)</p>
<p>Gain <input name="gain_db" size="5"> dB, peak <input name="peak_dbfs" size="5"> dBFS (empty: the model's own level)
or true peak <input name="peak_dbtp" size="5"> dBTP in its place (BS.1770-4, 4x oversampled; as far as the server was started
with true_peak)</p>
<p>Loudness <input name="loudness_lufs" size="5"> LUFS, e.g. -16 or -23, instead of a gain (empty: the model's own level)</p>
<p>Tone <input name="tone" size="20"> a preset or a band list such as hp:120;peak:3000:4, as far as the server was started
with it (empty: none)</p>
<p>Dynamics <input name="dynamics" size="20"> a compressor preset such as speech or pairs such as threshold=-24;ratio=4, as
far as the server was started with it (empty: none)</p>
<p>Encoding <input name="encoding" size="10"> pcm_s16le, pcm_f32le, mulaw or alaw, as far as the server was started with
them (empty: pcm_s16le), container <select name="container"><option>wav</option><option>raw</option></select></p>
<p><button type="submit">Speak</button></p>
</form>
</body></html>
"""


class FormError(ValueError):
    """the request body is not a form this server can read (answered with 400)"""


def _header_params(value: str) -> email.message.Message:
    """a one-header message, so that `get_param` / `get_filename` parse the header's parameters"""
    return email.message_from_string(f"Content-Type: {value}\n\n")


def parse_form(content_type: str | None, body: bytes) -> tuple[dict, dict]:
    """(fields, files) of an `application/x-www-form-urlencoded` or `multipart/form-data` body: fields maps a name to
    its first value (str), files maps a name to (filename, bytes).  Raises FormError on anything else."""
    ctype = (content_type or "").split(";", 1)[0].strip().lower()
    if ctype == "application/x-www-form-urlencoded":
        try:
            text = body.decode("utf-8")
            pairs = urllib.parse.parse_qsl(text, keep_blank_values=True, strict_parsing=bool(text), errors="strict")
        except (UnicodeDecodeError, ValueError) as e:
            raise FormError(f"malformed form body: {e}") from None
        fields: dict = {}
        for k, v in pairs:
            fields.setdefault(k, v)
        return fields, {}
    if ctype == "multipart/form-data":
        boundary = _header_params(content_type).get_param("boundary")
        if not boundary or not isinstance(boundary, str):
            raise FormError("multipart body without a boundary")
        parts = body.split(b"--" + boundary.encode("latin-1"))
        # preamble, the parts, then the close delimiter "--" (and an optional epilogue)
        if len(parts) < 2 or not parts[-1].startswith(b"--"):
            raise FormError("malformed multipart body: no closing boundary")
        fields, files = {}, {}
        for raw in parts[1:-1]:
            head, sep, data = raw.partition(b"\r\n\r\n")
            if not raw.startswith(b"\r\n") or not sep or not data.endswith(b"\r\n"):
                raise FormError("malformed multipart body: a part without headers or line breaks")
            data = data[:-2]
            try:
                hdrs = email.message_from_bytes(head[2:] + b"\r\n\r\n")
            except Exception as e:  # noqa: BLE001  (the parser's errors are not one family)
                raise FormError(f"malformed multipart part headers: {e}") from None
            disp = hdrs.get("content-disposition")
            if disp is None:
                raise FormError("malformed multipart body: a part without Content-Disposition")
            params = _header_params(disp)
            name = params.get_param("name", header="content-type")
            if not name or not isinstance(name, str):
                raise FormError("malformed multipart body: a part without a name")
            filename = params.get_param("filename", header="content-type")
            if filename is not None:
                files.setdefault(name, (str(filename), data))
            else:
                try:
                    fields.setdefault(name, data.decode("utf-8"))
                except UnicodeDecodeError:
                    raise FormError(f"form field {name!r} is not UTF-8") from None
        return fields, files
    raise FormError("expected an application/x-www-form-urlencoded or multipart/form-data body")


def parse_settings(fields: dict) -> dict:
    """the optional per-request settings as `ContinuousBatcher.submit` keywords (absent or empty field: None)"""
    out = {}
    for name, lo, integer in (("temperature", 0.0, False), ("noise_clamp", 0.0, False), ("eos_threshold", None, False),
                              ("frames_after_eos", 0, True)):
        raw = fields.get(name)
        if raw is None or raw.strip() == "":
            out[name] = None
            continue
        try:
            v = int(raw) if integer else float(raw)
        except ValueError:
            raise FormError(f"{name} must be {'an integer' if integer else 'a number'}, got {raw!r}") from None
        if not math.isfinite(v) or (lo is not None and v < lo) or (integer and v > 1000):
            raise FormError(f"{name} is out of range: {raw!r}")
        out[name] = v
    return out


def parse_lsd_steps(fields: dict, max_lsd_decode_steps: int) -> int | None:
    """the optional `lsd_decode_steps` field: an integer in [1, max_lsd_decode_steps] (absent or empty: None)"""
    raw = fields.get("lsd_decode_steps")
    if raw is None or raw.strip() == "":
        return None
    try:
        v = int(raw)
    except ValueError:
        raise FormError(f"lsd_decode_steps must be an integer, got {raw!r}") from None
    if not 1 <= v <= max_lsd_decode_steps:
        raise FormError(f"lsd_decode_steps must be in [1, {max_lsd_decode_steps}], got {raw!r}")
    return v


def parse_seed(fields: dict) -> int | None:
    """the optional `seed` field: an integer in [0, 2**63) (absent or empty: None)"""
    raw = fields.get("seed")
    if raw is None or raw.strip() == "":
        return None
    try:
        v = int(raw.strip(), 10)
    except ValueError:
        raise FormError(f"seed must be an integer, got {raw!r}") from None
    if not 0 <= v < 2 ** 63:
        raise FormError(f"seed must be in [0, 2**63), got {raw!r}")
    return v


def parse_sample_rate(fields: dict, native: int, sample_rates) -> int | None:
    """the optional `sample_rate` field: the native rate or one of the configured `sample_rates` (absent or empty: None)"""
    raw = fields.get("sample_rate")
    if raw is None or raw.strip() == "":
        return None
    try:
        v = int(raw.strip(), 10)
    except ValueError:
        raise FormError(f"sample_rate must be an integer, got {raw!r}") from None
    allowed = [int(native), *[int(r) for r in sample_rates or () if int(r) != int(native)]]
    if v not in allowed:
        raise FormError(f"sample_rate {v} is not configured (this server offers {allowed})")
    return v


def speed_table(speeds, native: int, sample_rates, frame_samples: int = 1920) -> dict:
    """{rate: [speeds admissible at that rate, 1.0 first]} for the native rate and every configured rate; ValueError for a
    speed that is no fraction in range, or that the plan rule admits at none of the rates"""
    from .output_chain import ChainTable

    return ChainTable(native, frame_samples, sample_rates, speeds).speeds_of()


def parse_speed(fields: dict, rate: int, table: dict | None) -> float | None:
    """the optional `speed` field: 1.0 or one of the configured speeds admissible at the request's `rate` (absent or
    empty: None).  `table`: what `speed_table` returns, or None on a server started without speeds"""
    raw = fields.get("speed")
    if raw is None or raw.strip() == "":
        return None
    try:
        v = float(raw.strip())
    except ValueError:
        raise FormError(f"speed must be a number, got {raw!r}") from None
    if not math.isfinite(v):
        raise FormError(f"speed must be a finite number, got {raw!r}")
    if table is None:
        if v != 1.0:
            raise FormError(f"speed {v} is not configured (this server speaks at 1.0 only)")
        return v
    configured = sorted({s for row in table.values() for s in row})
    near = [s for s in configured if abs(s - v) <= 1e-9]
    if not near:
        raise FormError(f"speed {v} is not configured (this server offers {configured})")
    if near[0] not in table[int(rate)]:
        raise FormError(f"speed {v} is not admissible at {int(rate)} Hz (admissible there: {table[int(rate)]})")
    return near[0]


def parse_pitch(fields: dict, rate, speed, table) -> float | None:
    """the optional `pitch` field, a number or "P/Q": 1 or one of the configured pitches admissible behind the request's
    `rate` and `speed` (absent or empty: None).  `table`: the server's `ChainTable` (rates, speeds, pitches).  FormError
    with the admissible list for a pitch that is not configured, that the plan rule refuses on the request's line, or that
    is sent to a server started without pitches"""
    from . import pitch as pitch_rule

    raw = fields.get("pitch")
    if raw is None or raw.strip() == "":
        return None
    try:
        v = float(pitch_rule.fraction(raw))
        table.route(rate, speed, None, None, v)
    except ValueError as e:
        raise FormError(str(e)) from None
    return v


def parse_tone(fields: dict, rate, speed, table):
    """the optional `tone` field: the canonical string of one of the configured tones admissible at the request's rate, None
    where absent, empty or "flat".  `table`: the server's `ChainTable`, without tones (or None) on a server started without.
    FormError with the configured list for a tone that is not configured, with the admissible list for one the request's
    rate refuses, for what the grammar refuses, and for any tone on a server started without tones"""
    from . import tone as tone_rule

    raw = fields.get("tone")
    if raw is None or raw.strip() == "":
        return None
    try:
        canon = tone_rule.normalise(raw)
        if canon is None:
            return None
        if table is None or table.tones is None:
            raise FormError("tone is not available (this server was started without tones)")
        table.route(rate, speed, tone=canon)
    except ValueError as e:
        raise FormError(str(e)) from None
    return canon


def parse_dynamics(fields: dict, rate, speed, table):
    """the optional `dynamics` field: the canonical string of one of the configured compressor settings, None where absent,
    empty or "off".  `table`: the server's `ChainTable`, without dynamics (or None) on a server started without.  FormError
    with the configured list for a setting that is not configured, with the admissible list for one the request's line
    refuses, for what the grammar refuses, and for any setting on a server started without dynamics"""
    from . import dynamics as dyn_rule

    raw = fields.get("dynamics")
    if raw is None or raw.strip() == "":
        return None
    try:
        canon = dyn_rule.normalise(raw)
        if canon is None:
            return None
        if table is None or table.dynamics is None:
            raise FormError("dynamics is not available (this server was started without dynamics)")
        table.route(rate, speed, dynamics=canon)
    except ValueError as e:
        raise FormError(str(e)) from None
    return canon


def parse_ceiling(fields: dict):
    """the optional `peak_dbfs` field of a request with a tone or a compressor setting and no gain: the limiter's ceiling, None where absent or empty;
    FormError for a value `level.check` refuses"""
    from . import level

    raw = (fields.get("peak_dbfs") or "").strip()
    if not raw:
        return None
    try:
        peak = float(raw)
    except ValueError:
        raise FormError(f"peak_dbfs must be a number, got {raw!r}") from None
    try:
        return level.check(0.0, peak)[1]
    except ValueError as e:
        raise FormError(str(e)) from None


def parse_true_peak(fields: dict, enabled: bool, settings: dict, table):
    """the optional `peak_dbtp` field, the request's ceiling as a true peak, None where absent or empty.  `settings`: what the
    request's other fields came to; `table`: the server's `ChainTable`.  FormError for the field on a server started without
    true_peak, beside `peak_dbfs`, for a value `level.check` refuses, on a request without a gain, a loudness target, a tone
    or a compressor setting (it has no limiter), and on a line the mode's rule refuses"""
    from . import level

    raw = (fields.get("peak_dbtp") or "").strip()
    if not raw:
        return None
    if not enabled:
        raise FormError("peak_dbtp is not available (this server was started without true_peak)")
    try:
        peak = float(raw)
    except ValueError:
        raise FormError(f"peak_dbtp must be a number, got {raw!r}") from None
    limited = any(settings.get(k) is not None for k in ("gain_db", "loudness_lufs", "tone", "dynamics"))
    try:
        peak_dbfs = (fields.get("peak_dbfs") or "").strip() or None
        peak = level.check(0.0 if limited else None, None if peak_dbfs is None else 0.0, peak)[1]
        keys = ("sample_rate", "speed", "pitch", "tone", "dynamics", "loudness_lufs", "gain_db")
        table.route(**{k: settings[k] for k in keys if k in settings}, peak_dbtp=peak)
    except ValueError as e:
        raise FormError(str(e)) from None
    return peak


def parse_level(fields: dict, enabled: bool):
    """the optional `gain_db` and `peak_dbfs` fields as (gain_db, peak_dbfs), each None where absent or empty; FormError for
    a value `level.check` refuses (its message names the rule) and for either field on a server started without level"""
    from . import level

    vals = {}
    for name in ("gain_db", "peak_dbfs"):
        raw = fields.get(name)
        if raw is None or raw.strip() == "":
            vals[name] = None
            continue
        if not enabled:
            raise FormError(f"{name} is not available (this server was started without level)")
        try:
            vals[name] = float(raw.strip())
        except ValueError:
            raise FormError(f"{name} must be a number, got {raw!r}") from None
    try:
        return level.check(vals["gain_db"], vals["peak_dbfs"])
    except ValueError as e:
        raise FormError(str(e)) from None


def parse_loudness(fields: dict, enabled: bool):
    """the optional `loudness_lufs` field with its ceiling as (loudness_lufs, peak_dbfs), (None, None) where absent or empty;
    FormError for a value `loudness.check` or `level.check` refuses (the message names the rule), for `gain_db` beside it and
    for the field on a server started without loudness"""
    from . import level, loudness

    raw = fields.get("loudness_lufs")
    if raw is None or raw.strip() == "":
        return None, None
    if not enabled:
        raise FormError("loudness_lufs is not available (this server was started without loudness)")
    vals = {}
    for name in ("loudness_lufs", "peak_dbfs", "gain_db"):
        text = (fields.get(name) or "").strip()
        try:
            vals[name] = float(text) if text else None
        except ValueError:
            raise FormError(f"{name} must be a number, got {text!r}") from None
    try:
        return loudness.check_with(vals["loudness_lufs"], vals["gain_db"]), level.check(0.0, vals["peak_dbfs"])[1]
    except ValueError as e:
        raise FormError(str(e)) from None


def parse_encoding(fields: dict, encodings):
    """the optional `encoding` field: its name, None where absent or empty.  `encodings`: what the server was started with
    (None: without the encoder; `pcm_s16le` is then the one name it takes).  FormError listing what is configured for any
    other name"""
    from .encoding import DEFAULT, normalise_encodings

    raw = fields.get("encoding")
    if raw is None or raw.strip() == "":
        return None
    name = raw.strip()
    configured = [DEFAULT] if encodings is None else normalise_encodings(encodings)
    if name not in configured:
        hint = "" if encodings is not None else "; this server was started without encodings"
        raise FormError(f"encoding {name!r} is not configured (this server has {configured}{hint})")
    return name


def parse_container(fields: dict, compressions=None) -> str:
    """the optional `container` field: "wav" (absent or empty) or "raw", and on a server started with `compressions` one of
    them ("flac"); FormError for anything else"""
    raw = (fields.get("container") or "").strip()
    if raw in ("", "wav"):
        return "wav"
    if raw == "raw":
        return "raw"
    if compressions is not None:
        if raw in compressions:
            return raw
        raise FormError(f"container must be 'wav', 'raw' or one of {list(compressions)}, got {raw!r}")
    raise FormError(f"container must be 'wav' or 'raw', got {raw!r}")


MAX_SCRIPT_ENTRIES = 256


def parse_script(fields: dict, files: dict | None = None):
    """the optional `script` field, a JSON list of {"voice": <name>, "text": <text>} objects, as [(voice name or None,
    text)] (absent or empty field: None).  It excludes `text`, `voice_url` and `voice_wav`.  FormError, naming the entry
    at fault, for a value that is no JSON, no list, an empty list, more than `MAX_SCRIPT_ENTRIES` entries, an entry that
    is no object, has no text or whose voice is no string"""
    import json

    raw = fields.get("script")
    if raw is None or raw.strip() == "":
        return None
    for name in ("text", "voice_url"):
        if (fields.get(name) or "").strip():
            raise FormError(f"script excludes {name}: the entries of the script carry their own")
    upload = (files or {}).get("voice_wav")
    if upload is not None and upload[1]:
        raise FormError("script excludes voice_wav: the entries of the script name voices of the server")
    try:
        entries = json.loads(raw)
    except ValueError as e:
        raise FormError(f"script is not valid JSON: {e}") from None
    if not isinstance(entries, list):
        raise FormError("script must be a JSON list of {\"voice\": ..., \"text\": ...} objects")
    if not entries:
        raise FormError("script is an empty list")
    if len(entries) > MAX_SCRIPT_ENTRIES:
        raise FormError(f"script has {len(entries)} entries; at most {MAX_SCRIPT_ENTRIES} are accepted")
    out = []
    for i, entry in enumerate(entries):
        if not isinstance(entry, dict):
            raise FormError(f"script[{i}] is not an object with \"voice\" and \"text\"")
        text, voice = entry.get("text"), entry.get("voice")
        if not isinstance(text, str) or not text.strip():
            raise FormError(f"script[{i}] has no text")
        if voice is not None and (not isinstance(voice, str) or not voice.strip()):
            raise FormError(f"script[{i}]: voice must be the name of a voice, got {voice!r}")
        out.append((voice, text))
    return out


def create_app(model, *, slots: int, capacity: int, voices_dir=None, default_voice: str | None = None,
               batcher_factory=None, max_lsd_decode_steps: int | None = None, parallel_chunks: int = 1, **chain):
    """FastAPI app serving `model` through one `ContinuousBatcher(pcm_format="i16")` of `slots` rows of `capacity` KV
    positions, started and closed by the app's lifespan.  `voice_url=<name>` reads `<voices_dir>/<name>.safetensors`
    once; requests without a voice use `default_voice`.  The model's `noise_clamp` (if any) is every request's default
    noise clamp.  A request's `lsd_decode_steps` may be 1 .. `max_lsd_decode_steps` (default: the model's
    `lsd_decode_steps`; a larger maximum gives the batcher per-row LSD schedules).  `**chain`: the options of
    `output_chain.ChainSpec`, what a request may choose with the form fields of the same names as `ChainTable.route`'s;
    without one of them a request that sends its field gets a 400, and the batcher's graphs are those of before.  What the
    rules refuse in a list is a ValueError here, not at the first request; a request with a value that is not configured, or
    that its rate or line does not admit, gets a 400 with the list of what is.  The WAV header and the trailing silence
    follow the request's rate and encoding.  With `encodings` the batcher is built with its default `pcm_format`: every
    request's samples leave the GPU in its own encoding.  With `compressions` a request may send `container=flac`: the
    answer is `audio/flac`, the stream header, one frame per codec frame as each is decoded and the silent tail
    (`main.flac_stream_bytes`), which decodes to the samples of the `container=wav` answer; it takes `encoding` pcm_s16le or
    none, and a line `flac.plan` admits (400 with the rule's message otherwise).  `parallel_chunks` = W: every request runs up to
    W chunks of its text at a time in slots of their own (`ContinuousBatcher`; 1: one after the other).  The form field
    `script`, a JSON list of {"voice": <name>, "text": <text>} objects, makes one request of several segments, each with a voice
    of the voices directory (`parse_script`, `ContinuousBatcher.submit_script`); every other field applies to the whole script.
    `batcher_factory(model, slots, capacity)` replaces the batcher (tests)."""
    from .main import flac_stream_bytes, wav_stream_bytes

    from .output_chain import ChainSpec

    for name, number in (("sample_rates", int), ("speeds", float)):
        if chain.get(name) is not None:
            chain[name] = [number(v) for v in chain[name]]
    spec = ChainSpec(**chain)
    # the one table every request is checked against: the rules of every stage on every line (ValueError at start-up)
    table = spec.table(model.sample_rate, getattr(getattr(model, "engine", None), "frame_samples", 1920))
    # true_peak brings the leveler as level does: such a server takes gain_db too
    sample_rates, level, loudness, encodings = spec.sample_rates, spec.level or spec.true_peak, spec.loudness, table.encodings
    compressions = table.compressions
    speeds_of = None if spec.speeds is None else table.speeds_of()

    from .batching import check_parallel_chunks

    parallel_chunks = check_parallel_chunks(parallel_chunks)  # ValueError at start-up
    own_lsd = getattr(model, "lsd_decode_steps", 1)
    max_lsd = own_lsd if max_lsd_decode_steps is None else int(max_lsd_decode_steps)
    if batcher_factory is None:
        from .batching import ContinuousBatcher

        # no per-row capacity when the maximum is the model's own count: the batcher's graphs are those of before
        reserve = max_lsd if max_lsd != own_lsd else None

        def batcher_factory(model, slots, capacity):  # the encoder writes every request's format, pcm_s16le included
            return ContinuousBatcher(model, slots=slots, capacity=capacity, max_lsd_decode_steps=reserve, spec=spec,
                                     pcm_format="f32" if encodings is not None else "i16", parallel_chunks=parallel_chunks)

    voices_dir = Path(voices_dir) if voices_dir is not None else None
    voices: dict = {}  # name -> voice state dict: one object per voice, so the batcher's voice cache hits
    voices_lock = threading.Lock()

    @asynccontextmanager
    async def lifespan(app):
        import anyio.to_thread

        # every streaming response waits for its frames on a worker thread: let all slots' streams (and as many queued
        # requests) wait at once instead of capping them at anyio's default of 40
        limiter = anyio.to_thread.current_default_thread_limiter()
        limiter.total_tokens = max(limiter.total_tokens, 2 * slots + 8)
        batcher = batcher_factory(model, slots, capacity)
        batcher.start()
        app.state.batcher = batcher
        try:
            yield
        finally:
            app.state.batcher = None
            batcher.close()

    app = FastAPI(title="Pocket TTS", lifespan=lifespan)
    app.state.batcher = None

    def load_voice(name: str) -> dict:
        if name.startswith(OFFLINE_PREFIXES):
            raise FormError(f"{name} needs a download; this build runs offline")
        if name.endswith(".safetensors"):
            name = name[: -len(".safetensors")]
        path = voices_dir / f"{name}.safetensors" if voices_dir is not None else None
        if not _VOICE_NAME.fullmatch(name) or path is None or not path.is_file():
            raise FormError(f"unknown voice {name!r}")
        with voices_lock:
            if name not in voices:
                voices[name] = model.get_state_for_audio_prompt(str(path))
            return voices[name]

    def encode_upload(filename: str, data: bytes, batcher) -> dict:
        suffix = Path(filename).suffix or ".wav"
        fd, path = tempfile.mkstemp(suffix=suffix)
        try:
            with os.fdopen(fd, "wb") as f:
                f.write(data)
            # the encoder runs on the engine the scheduler thread drives: between two of its iterations
            return batcher.exclusive(model.get_state_for_audio_prompt, path, truncate=True)
        except (OSError, EOFError, ImportError, ValueError) as e:
            raise FormError(f"could not read the uploaded voice_wav: {e}") from None
        except Exception as e:  # wave.Error and friends: an unreadable file is the client's error
            if type(e).__module__ in ("wave", "struct", "numpy"):
                raise FormError(f"could not read the uploaded voice_wav: {e}") from None
            raise
        finally:
            os.unlink(path)

    def bad(msg) -> JSONResponse:
        return JSONResponse({"detail": str(msg)}, status_code=400)

    @app.get("/", response_class=HTMLResponse)
    async def index():
        return INDEX_HTML

    @app.get("/health")
    async def health():
        b = app.state.batcher
        if b is None:
            return JSONResponse({"status": "unhealthy", "error": "the batcher is not running"}, status_code=503)
        if b.failed is not None:
            return JSONResponse({"status": "unhealthy", "error": str(b.failed)}, status_code=503)
        return {"status": "healthy"}

    @app.post("/tts")
    async def tts(request: Request):
        batcher = app.state.batcher
        if batcher is None:
            return JSONResponse({"detail": "the batcher is not running"}, status_code=503)
        try:
            fields, files = parse_form(request.headers.get("content-type"), await request.body())
            script = parse_script(fields, files)
            text = fields.get("text", "")
            if script is None and not text.strip():
                raise FormError("Text cannot be empty")
            settings = parse_settings(fields)
            lsd = parse_lsd_steps(fields, max_lsd)
            if lsd is not None:
                settings["lsd_decode_steps"] = lsd
            seed = parse_seed(fields)
            if seed is not None:
                settings["seed"] = seed
            rate = parse_sample_rate(fields, model.sample_rate, sample_rates)
            if rate is not None and rate != int(model.sample_rate):
                settings["sample_rate"] = rate
            speed = parse_speed(fields, rate or int(model.sample_rate), speeds_of)
            if speed is not None and speed != 1.0:
                settings["speed"] = speed
            pitch = parse_pitch(fields, settings.get("sample_rate"), settings.get("speed"), table)
            if pitch is not None and pitch != 1.0:
                settings["pitch"] = pitch
            tone = parse_tone(fields, settings.get("sample_rate"), settings.get("speed"), table)
            if tone is not None:
                settings["tone"] = tone
            dyn = parse_dynamics(fields, settings.get("sample_rate"), settings.get("speed"), table)
            if dyn is not None:
                settings["dynamics"] = dyn
            target, ceiling = parse_loudness(fields, loudness)
            if target is not None:
                settings["loudness_lufs"], settings["peak_dbfs"] = target, ceiling
            elif (tone is not None or dyn is not None) and not (fields.get("gain_db") or "").strip():
                ceiling = parse_ceiling(fields)  # the limiter behind the tone or the compressor: no gain of its own
                if ceiling is not None:
                    settings["peak_dbfs"] = ceiling
            else:
                gain_db, peak_dbfs = parse_level(fields, level)
                if gain_db is not None:
                    settings["gain_db"], settings["peak_dbfs"] = gain_db, peak_dbfs
            peak_dbtp = parse_true_peak(fields, spec.true_peak, settings, table)
            if peak_dbtp is not None:
                settings.pop("peak_dbfs", None)
                settings["peak_dbtp"] = peak_dbtp
            enc = parse_encoding(fields, encodings)
            if enc is not None and encodings is not None:
                settings["encoding"] = enc
            container = parse_container(fields, compressions)
            flac_n = None
            if compressions is not None and container in compressions:
                settings["compression"] = container
                # the rule's refusals (an encoding that is not pcm_s16le, a line FLAC does not admit), and the block size
                route_fields = ("sample_rate", "speed", "pitch", "tone", "dynamics", "loudness_lufs", "gain_db", "peak_dbfs",
                                "peak_dbtp", "encoding", "compression")
                try:
                    flac_n = table.route(**{k: settings[k] for k in route_fields if k in settings}).n_out
                except ValueError as e:
                    raise FormError(str(e)) from None
            voice_url = fields.get("voice_url") or None
            upload = files.get("voice_wav")
            if upload is not None and not upload[1]:
                upload = None  # an empty file input (a browser form sends one when no file is chosen)
            if voice_url is not None and upload is not None:
                raise FormError("Cannot provide both voice_url and voice_wav")
            segments = None
            if script is not None:
                segments = []
                for i, (name, part) in enumerate(script):
                    if name is None and default_voice is None:
                        raise FormError(f"script[{i}] names no voice and the server has no default voice")
                    try:
                        segments.append((await run_in_threadpool(load_voice, name or default_voice), part))
                    except FormError as e:
                        raise FormError(f"script[{i}]: {e}") from None
            elif upload is not None:
                state = await run_in_threadpool(encode_upload, upload[0], upload[1], batcher)
            else:
                if voice_url is None:
                    if default_voice is None:
                        raise FormError("no voice given (voice_url or voice_wav) and the server has no default voice")
                    voice_url = default_voice
                state = await run_in_threadpool(load_voice, voice_url)
            fae = settings.pop("frames_after_eos")
            if settings["noise_clamp"] is None and model.noise_clamp is not None:
                settings["noise_clamp"] = model.noise_clamp
            if segments is not None:
                req = await run_in_threadpool(batcher.submit_script, segments, fae, **settings)
            else:
                req = await run_in_threadpool(batcher.submit, state, text, fae, **settings)
        except ValueError as e:  # FormError, and submit's own (empty text, capacity)
            return bad(e)

        import torch

        def frames():  # every chunk that has arrived so far as one: one thread hop per batch of frames
            for chunks in req.iter_batches():
                yield chunks[0] if len(chunks) == 1 else torch.cat(chunks)

        out_rate = rate or model.sample_rate
        if flac_n is not None:  # every frame that has arrived so far as one item: flac_stream_bytes counts them
            return StreamingResponse(flac_stream_bytes(req.iter_batches(), out_rate, flac_n), media_type="audio/flac",
                                     headers={"Content-Disposition": "attachment; filename=generated_speech.flac"})
        if container == "raw":
            return StreamingResponse(wav_stream_bytes(frames(), out_rate, enc, header=False),
                                     media_type="application/octet-stream",
                                     headers={"X-Audio-Encoding": enc or "pcm_s16le", "X-Sample-Rate": str(int(out_rate))})
        return StreamingResponse(wav_stream_bytes(frames(), out_rate, enc), media_type="audio/wav",
                                 headers={"Content-Disposition": "attachment; filename=generated_speech.wav"})

    return app
