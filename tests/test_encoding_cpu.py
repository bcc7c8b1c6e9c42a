"""Per-request output encoding without a GPU: the G.711 reference against the standard library's recorded results, the rule
module, the routes, the WAV headers and the server's form fields."""

import asyncio
import hashlib
import io
import json
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import g711_ref

G = Path(__file__).parent / "golden"
ROOT = Path(__file__).resolve().parent.parent
FIX = json.loads((G / "g711.json").read_text())
NAMES = ["pcm_s16le", "pcm_f32le", "mulaw", "alaw"]


# ---- the reference -------------------------------------------------------------------------------------------------------
def test_the_reference_reproduces_the_recorded_compressors():
    s = np.arange(-32768, 32768)
    assert hashlib.sha256(g711_ref.lin2ulaw(s).tobytes()).hexdigest() == FIX["lin2ulaw_sha256"]
    assert hashlib.sha256(g711_ref.lin2alaw(s).tobytes()).hexdigest() == FIX["lin2alaw_sha256"]
    assert FIX["lin2ulaw_sha256"].startswith("81d633c9e6972a18") and FIX["lin2alaw_sha256"].startswith("38488f6fd710f468")


def test_the_reference_reproduces_the_recorded_expanders():
    codes = np.arange(256)
    assert g711_ref.ulaw2lin(codes).tolist() == FIX["ulaw2lin"]
    assert g711_ref.alaw2lin(codes).tolist() == FIX["alaw2lin"]


def test_fixed_points():
    s = np.array([0, -1, 32767, -32767])
    assert g711_ref.lin2ulaw(s).tolist() == [0xFF, 0x7E, 0x80, 0x00]
    assert g711_ref.lin2alaw(s).tolist() == [0xD5, 0x55, 0xAA, 0x2A]


def test_every_code_survives_decode_then_encode():
    codes = np.arange(256)
    assert np.array_equal(g711_ref.lin2alaw(g711_ref.alaw2lin(codes)), codes)
    back = g711_ref.lin2ulaw(g711_ref.ulaw2lin(codes))
    assert np.nonzero(back != codes)[0].tolist() == [0x7F] and back[0x7F] == 0xFF  # negative zero, and no other


def test_the_ramp_truncates_back_to_every_sample():
    s, x = g711_ref.ramp()
    assert s.shape == (65535,) and x.dtype == np.float32 and np.array_equal(g711_ref.s16(x), s)
    assert g711_ref.s16([np.nan, 1.5, -1.5, np.inf, -np.inf, 0.99999]).tolist() == [-32767, 32767, -32767, 32767, -32767, 32766]


def test_the_kernel_header_on_the_host_gives_the_recorded_codes(tmp_path):
    """csrc/ptts_encode.h is ordinary C++: its conversions, compiled for the host under ASan and UBSan, over every 16-bit
    sample, and its index functions over every (width, n) of the kernel's grid"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path / "encode_sweep"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-I", str(ROOT / "pocket_tts_amd" / "csrc"), "-o", str(exe),
                        str(ROOT / "tests" / "cpp" / "encode_sweep.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # the leak checker needs ptrace, which build sandboxes often deny
    r = subprocess.run([str(exe)], capture_output=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    out = r.stdout
    assert len(out) == 2 * 65536 + 65535 * 2
    assert hashlib.sha256(out[:65536]).hexdigest() == FIX["lin2ulaw_sha256"]
    assert hashlib.sha256(out[65536:131072]).hexdigest() == FIX["lin2alaw_sha256"]
    assert np.array_equal(np.frombuffer(out[131072:], np.int16), g711_ref.ramp()[0])
    assert r.stderr.decode().strip() == "ok"


# ---- the rule module --------------------------------------------------------------------------------------------------------
def test_the_table_of_encodings():
    from pocket_tts_amd import encoding as e

    assert list(e.NAMES) == NAMES and [e.CODE[n] for n in NAMES] == [0, 1, 2, 3]
    assert [e.BYTES_PER_SAMPLE[n] for n in NAMES] == [2, 4, 1, 1]
    assert [e.WAV_FORMAT_TAG[n] for n in NAMES] == [1, 3, 7, 6]
    assert [e.SILENCE[n] for n in NAMES] == [b"\0\0", b"\0\0\0\0", b"\xff", b"\xd5"]
    assert [e.torch_dtype(n) for n in NAMES] == [torch.int16, torch.float32, torch.uint8, torch.uint8]
    assert [e.pitch(w) for w in (1, 4, 5, 882, 1920)] == [16, 16, 32, 3536, 7680]
    # silence decodes to zero (A-law: to the smallest step)
    assert g711_ref.ulaw2lin([0xFF]).tolist() == [0] and abs(int(g711_ref.alaw2lin([0xD5])[0])) == 8


def test_normalise_and_check():
    from pocket_tts_amd.encoding import check, normalise_encodings

    assert normalise_encodings([]) == ["pcm_s16le"]
    assert normalise_encodings(["mulaw", "alaw", "pcm_f32le"]) == ["pcm_s16le", "mulaw", "alaw", "pcm_f32le"]
    assert normalise_encodings(("alaw", "pcm_s16le", "alaw")) == ["pcm_s16le", "alaw"]
    with pytest.raises(ValueError, match=r"'opus' is not known \(known: \['pcm_s16le', 'pcm_f32le', 'mulaw', 'alaw'\]\)"):
        normalise_encodings(["mulaw", "opus"])
    with pytest.raises(ValueError, match="list of names"):
        normalise_encodings("mulaw")
    assert check(None) == "pcm_s16le" and check("alaw") == "alaw" and check("mulaw", ["pcm_s16le", "mulaw"]) == "mulaw"
    with pytest.raises(ValueError, match=r"'alaw' is not configured \(this pipeline has \['pcm_s16le', 'mulaw'\]\)"):
        check("alaw", ["pcm_s16le", "mulaw"])
    for bad in (3, "MULAW", ""):
        with pytest.raises(ValueError, match="not configured"):
            check(bad)


def test_routes():
    from pocket_tts_amd.output_chain import ChainTable, Route

    r = Route(0, 24000, None, False, None, 1920, 0, 0, None)
    assert r.encoding is None and r.bytes_per_sample is None
    plain = ChainTable(24000, 1920)
    assert plain.empty and plain.encodings is None
    assert plain.route().encoding is None and plain.route().bytes_per_sample is None
    with pytest.raises(ValueError, match="build it with encodings"):
        plain.route(encoding="mulaw")
    with pytest.raises(ValueError, match="build it with encodings"):
        plain.route(encoding="pcm_s16le")
    only = ChainTable(24000, 1920, encodings=[])  # the encoder alone makes a chain
    assert not only.empty and only.encodings == ["pcm_s16le"] and only.width == 1920
    r = only.route()
    assert (r.encoding, r.bytes_per_sample, r.n_out, r.preroll, r.drain_frames, r.drain_stage) == ("pcm_s16le", 2, 1920, 0, 0, None)
    with pytest.raises(ValueError, match=r"'mulaw' is not configured \(this pipeline has \['pcm_s16le'\]\)"):
        only.route(encoding="mulaw")
    t = ChainTable(24000, 1920, sample_rates=[8000], level=True, encodings=["mulaw", "pcm_f32le"])
    assert t.width == 1920
    r = t.route(sample_rate=8000, gain_db=6, encoding="mulaw")
    same = ChainTable(24000, 1920, sample_rates=[8000], level=True).route(sample_rate=8000, gain_db=6)
    assert (r.encoding, r.bytes_per_sample, r.n_out) == ("mulaw", 1, 640)
    assert (r.preroll, r.drain_frames, r.drain_stage, r.level) == (same.preroll, same.drain_frames, same.drain_stage, same.level)
    assert r.take(0, None) == same.take(0, None) and r.take(640, 3) == same.take(640, 3)  # take counts samples
    assert t.route(encoding="pcm_f32le").bytes_per_sample == 4 and t.route().encoding == "pcm_s16le"
    with pytest.raises(ValueError, match="'alaw' is not configured"):
        t.route(encoding="alaw")
    with pytest.raises(ValueError, match="not known"):
        ChainTable(24000, 1920, encodings=["g722"])


# ---- WAV ----------------------------------------------------------------------------------------------------------------------
def test_the_pcm_header_is_the_one_of_before():
    from pocket_tts_amd.main import _wav_header

    for n, rate in ((0, 24000), (12345, 8000)):
        old = struct.pack("<4sL4s4sLHHLLHH4sL", b"RIFF", 36 + 2 * n, b"WAVE", b"fmt ", 16, 1, 1, rate, 2 * rate, 2, 16, b"data", 2 * n)
        assert _wav_header(n, rate) == _wav_header(n, rate, "pcm_s16le") == old and len(old) == 44


@pytest.mark.parametrize("name,tag,bits,align", [("pcm_f32le", 3, 32, 4), ("mulaw", 7, 8, 1), ("alaw", 6, 8, 1)])
def test_the_extended_header_field_by_field(name, tag, bits, align):
    from pocket_tts_amd.main import _wav_header

    n, rate = 4321, 8000
    h = _wav_header(n, rate, name)
    assert len(h) == 58
    riff, size, wave_ = struct.unpack_from("<4sL4s", h, 0)
    assert (riff, size, wave_) == (b"RIFF", 50 + align * n, b"WAVE")
    cid, clen, ftag, ch, sr, byte_rate, block, bps, cb = struct.unpack_from("<4sLHHLLHHH", h, 12)
    assert (cid, clen, ftag, ch, sr, byte_rate, block, bps, cb) == (b"fmt ", 18, tag, 1, rate, align * rate, align, bits, 0)
    cid, clen, samples = struct.unpack_from("<4sLL", h, 38)
    assert (cid, clen, samples) == (b"fact", 4, n)
    assert struct.unpack_from("<4sL", h, 50) == (b"data", align * n)


@pytest.mark.parametrize("name", NAMES)
def test_the_stream_ends_in_the_silence_of_its_encoding(name):
    from pocket_tts_amd import encoding as e
    from pocket_tts_amd.main import _wav_header, wav_stream_bytes

    chunks = [torch.arange(1, 6).to(e.torch_dtype(name)), torch.arange(6, 9).to(e.torch_dtype(name))]
    parts = list(wav_stream_bytes(chunks, 8000, name))
    head = 44 if name == "pcm_s16le" else 58
    assert parts[0] == _wav_header(1_000_000_000, 8000, name) and len(parts[0]) == head
    body = b"".join(parts[1:-1])
    assert body == b"".join(c.numpy().tobytes() for c in chunks) and len(body) == 8 * e.BYTES_PER_SAMPLE[name]
    assert parts[-1] == e.SILENCE[name] * 1600
    assert list(wav_stream_bytes(chunks, 8000, name, header=False)) == parts[1:]
    if name != "pcm_s16le":
        with pytest.raises(ValueError, match="chunks"):
            list(wav_stream_bytes([torch.zeros(4, dtype=torch.int16)], 8000, name))


def test_without_an_encoding_the_stream_is_the_one_of_before():
    from pocket_tts_amd.main import wav_stream_bytes

    x = torch.tensor([0.0, 0.5, -2.0, 1.0])
    parts = list(wav_stream_bytes([x, torch.tensor([7, -7], dtype=torch.int16)], 24000))
    assert len(parts[0]) == 44 and parts[-1] == bytes(2 * 4800)
    assert np.frombuffer(parts[1], np.int16).tolist() == [0, 16383, -32767, 32767]
    assert np.frombuffer(parts[2], np.int16).tolist() == [7, -7]
    assert parts == list(wav_stream_bytes([x, torch.tensor([7, -7], dtype=torch.int16)], 24000, "pcm_s16le"))


def test_written_files_have_their_lengths_patched(tmp_path):
    from scipy.io import wavfile

    from pocket_tts_amd.main import write_wav_stream

    x = np.linspace(-1.5, 1.5, 1000).astype(np.float32)
    x[3] = 0.25
    p = tmp_path / "f.wav"
    n = write_wav_stream(str(p), [torch.from_numpy(x[:300]), torch.from_numpy(x[300:])], 8000, "pcm_f32le")
    assert n == 1000 + 1600
    rate, data = wavfile.read(str(p))
    assert rate == 8000 and data.dtype == np.float32 and data.shape == (2600,)
    assert np.array_equal(data[:1000].view(np.uint32), x.view(np.uint32)) and not data[1000:].any()
    for name, ref in (("mulaw", g711_ref.lin2ulaw), ("alaw", g711_ref.lin2alaw)):
        codes = ref(g711_ref.s16(x))
        p = tmp_path / f"{name}.wav"
        assert write_wav_stream(str(p), [torch.from_numpy(codes)], 8000, name) == 2600
        raw = p.read_bytes()
        assert len(raw) == 58 + 2600
        assert struct.unpack_from("<L", raw, 4)[0] == 50 + 2600 and struct.unpack_from("<L", raw, 46)[0] == 2600
        assert struct.unpack_from("<L", raw, 54)[0] == 2600 and raw[58:1058] == codes.tobytes()
        assert set(raw[1058:]) == {0xFF if name == "mulaw" else 0xD5}
    p = tmp_path / "s.wav"
    assert write_wav_stream(str(p), [torch.from_numpy(x)], 24000) == 1000 + 4800  # as before: 44 bytes, 16 bits
    rate, data = wavfile.read(str(p))
    assert rate == 24000 and data.dtype == np.int16 and np.array_equal(data[:1000], g711_ref.s16(x))


def test_the_commands_take_the_new_flags():
    from pocket_tts_amd.main import build_parser

    ap = build_parser()
    assert ap.parse_args(["generate"]).encoding is None
    assert ap.parse_args(["generate", "--sample-rate", "8000", "--encoding", "mulaw"]).encoding == "mulaw"
    assert ap.parse_args(["serve"]).encodings is None
    assert ap.parse_args(["serve", "--encodings", "mulaw,alaw,pcm_f32le"]).encodings == ["mulaw", "alaw", "pcm_f32le"]
    for bad in (["generate", "--encoding", "opus"], ["serve", "--encodings", "mulaw,opus"], ["serve", "--encodings", ","]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)


# ---- the server's form fields ----------------------------------------------------------------------------------------------
def test_parse_encoding_and_container():
    from pocket_tts_amd.server import FormError, parse_container, parse_encoding

    conf = ["mulaw", "alaw"]
    assert parse_encoding({}, conf) is None and parse_encoding({"encoding": " "}, conf) is None
    assert parse_encoding({"encoding": "alaw"}, conf) == "alaw" and parse_encoding({"encoding": "pcm_s16le"}, conf) == "pcm_s16le"
    with pytest.raises(FormError, match=r"'pcm_f32le' is not configured \(this server has \['pcm_s16le', 'mulaw', 'alaw'\]\)"):
        parse_encoding({"encoding": "pcm_f32le"}, conf)
    assert parse_encoding({"encoding": "pcm_s16le"}, None) == "pcm_s16le"
    with pytest.raises(FormError, match=r"this server has \['pcm_s16le'\]; this server was started without encodings"):
        parse_encoding({"encoding": "mulaw"}, None)
    assert parse_container({}) == "wav" and parse_container({"container": ""}) == "wav"
    assert parse_container({"container": "wav"}) == "wav" and parse_container({"container": " raw "}) == "raw"
    with pytest.raises(FormError, match="'wav' or 'raw'"):
        parse_container({"container": "ogg"})


class _Request:
    def __init__(self, dtype):
        self.dtype = dtype

    def iter_batches(self):
        for i in range(3):
            yield [torch.full((4,), i + 1, dtype=self.dtype)]


class _Batcher:
    """what the server sees of a batcher built with `encodings`: typed chunks by the request's encoding"""

    def __init__(self, typed):
        self.failed, self.submitted, self.typed = None, [], typed

    def start(self):
        pass

    def close(self):
        pass

    def submit(self, state, text, fae=None, **settings):
        from pocket_tts_amd.encoding import torch_dtype

        self.submitted.append(settings)
        return _Request(torch_dtype(settings.get("encoding") or "pcm_s16le") if self.typed else torch.int16)


class _Model:
    sample_rate = 24000
    noise_clamp = None

    def get_state_for_audio_prompt(self, path, truncate=False):
        return {"voice": str(path)}


def _post(tmp_path, forms, **kw):
    import httpx

    from pocket_tts_amd.server import create_app

    (tmp_path / "v1.safetensors").write_bytes(b"x")
    stub = _Batcher(typed=kw.get("encodings") is not None)
    app = create_app(_Model(), slots=4, capacity=64, voices_dir=tmp_path, default_voice="v1",
                     batcher_factory=lambda m, s, c: stub, **kw)

    async def go():
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t") as cl:
                return [await cl.post("/tts", data=d) for d in forms] + [await cl.get("/")]

    return asyncio.run(go()), stub


def test_the_server_with_encodings(tmp_path):
    res, stub = _post(tmp_path, [{"text": "hi", "encoding": "alaw", "sample_rate": "8000"},
                                 {"text": "hi", "encoding": "alaw", "sample_rate": "8000", "container": "raw"},
                                 {"text": "hi"},
                                 {"text": "hi", "encoding": "pcm_f32le", "container": "raw"},
                                 {"text": "hi", "encoding": "mulaw"},
                                 {"text": "hi", "container": "zip"}],
                      sample_rates=[8000], encodings=["alaw", "pcm_f32le"])
    wav, raw, plain, f32, bad, bad_c, index = res
    assert wav.status_code == 200 and wav.headers["content-type"] == "audio/wav"
    assert len(wav.content) == 58 + 12 + 1600 and struct.unpack_from("<HHL", wav.content, 20) == (6, 1, 8000)
    assert wav.content[58:70] == bytes([1] * 4 + [2] * 4 + [3] * 4) and set(wav.content[70:]) == {0xD5}
    assert raw.status_code == 200 and raw.headers["content-type"] == "application/octet-stream"
    assert raw.headers["x-audio-encoding"] == "alaw" and raw.headers["x-sample-rate"] == "8000"
    assert raw.content == wav.content[58:]
    assert plain.status_code == 200 and len(plain.content) == 44 + 24 + 2 * 4800 and plain.content[:4] == b"RIFF"
    assert f32.status_code == 200 and f32.headers["x-audio-encoding"] == "pcm_f32le" and f32.headers["x-sample-rate"] == "24000"
    assert np.frombuffer(f32.content, np.float32)[:12].tolist() == [1.0] * 4 + [2.0] * 4 + [3.0] * 4
    assert len(f32.content) == 48 + 4 * 4800 and not any(f32.content[48:])
    assert bad.status_code == 400 and "['pcm_s16le', 'alaw', 'pcm_f32le']" in bad.json()["detail"]
    assert bad_c.status_code == 400 and "'wav' or 'raw'" in bad_c.json()["detail"]
    assert [s.get("encoding") for s in stub.submitted] == ["alaw", "alaw", None, "pcm_f32le"]
    assert 'name="encoding"' in index.text and 'name="container"' in index.text


def test_a_server_without_encodings(tmp_path):
    res, stub = _post(tmp_path, [{"text": "hi", "encoding": "mulaw"},
                                 {"text": "hi", "encoding": "pcm_s16le", "container": "raw"},
                                 {"text": "hi"}])
    bad, raw, plain, _ = res
    assert bad.status_code == 400 and "['pcm_s16le']" in bad.json()["detail"] and "without encodings" in bad.json()["detail"]
    assert raw.status_code == 200 and raw.headers["content-type"] == "application/octet-stream"
    assert raw.headers["x-audio-encoding"] == "pcm_s16le" and raw.headers["x-sample-rate"] == "24000"
    assert plain.status_code == 200 and plain.headers["content-type"] == "audio/wav" and raw.content == plain.content[44:]
    assert all("encoding" not in s for s in stub.submitted) and len(stub.submitted) == 2
    with pytest.raises(ValueError, match="not known"):
        _post(tmp_path, [], encodings=["opus"])
