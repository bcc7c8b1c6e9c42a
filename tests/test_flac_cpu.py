"""The FLAC packer without a GPU: the rule module `flac.py` (known answers, plan rule, pitch, stream pieces), the reference
encoder against the independent reference decoder (`flac_ref.py`), the routing through `ChainTable`, the stream helper of
`main.py`, the server's form handling, and what the kernel's lanes do with csrc/ptts_flac.h as a sanitizer-built host program
(tests/cpp/flac_sweep.cpp), byte for byte against the reference encoder."""

import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import flac_ref
from pocket_tts_amd import flac
from pocket_tts_amd.output_chain import ChainSpec, ChainTable, RequestError, Route

ROOT = Path(__file__).resolve().parents[1]
NS = (16, 17, 640, 882, 1920, 4608)
NUMBERS = (0, 127, 128, 2047, 2048, 65536)


def signals(n, seed=0):
    """{name: int16 block of n samples}: the sweep of the issue"""
    rng = np.random.default_rng(seed + n)
    t = np.arange(n)
    impulse = np.zeros(n, np.int16)
    impulse[n // 2] = 32767
    e = rng.standard_normal(n + 64) * 900.0
    ar = np.zeros(n + 64)
    for i in range(2, n + 64):  # AR(2), poles at 0.95 exp(+-0.15 i): speech-like spectrum
        ar[i] = 2 * 0.95 * np.cos(0.15) * ar[i - 1] - 0.95 ** 2 * ar[i - 2] + e[i]
    return {
        "silence": np.zeros(n, np.int16),
        "dc": np.full(n, -1234, np.int16),
        "square": np.where((t // 7) % 2 == 0, 32767, -32767).astype(np.int16),
        "sine": np.round(40.0 * np.sin(2 * np.pi * t / 50.0)).astype(np.int16),
        "noise": rng.integers(-32768, 32768, n).astype(np.int16),
        "impulse": impulse,
        "ar2": np.clip(ar[64:], -32768, 32767).astype(np.int16),
    }


# ---- known answers ----------------------------------------------------------------------------------------------------
def test_known_answers():
    assert flac.crc8(b"123456789") == 0xF4
    assert flac.crc16(b"123456789") == 0xFEE8
    assert flac.silent_frame(0, 1920, 24000) == bytes.fromhex("FFF8770800077F22000000B57A")
    assert flac.silent_frame(128, 640, 8000) == bytes.fromhex("FFF87408C280027F3F000000BBFC")


def test_crc_tables_match_a_bit_serial_crc():
    def serial(data, poly, bits):
        c = 0
        for byte in data:
            for i in range(7, -1, -1):
                top = (c >> (bits - 1)) & 1
                c = ((c << 1) & ((1 << bits) - 1)) | ((byte >> i) & 1)
                if top:
                    c ^= poly
        for _ in range(bits):  # flush: the message times x^bits
            top = (c >> (bits - 1)) & 1
            c = (c << 1) & ((1 << bits) - 1)
            if top:
                c ^= poly
        return c

    data = bytes(range(256)) + b"123456789"
    assert flac.crc8(data) == serial(data, 0x07, 8)
    assert flac.crc16(data) == serial(data, 0x8005, 16)


def test_utf8_numbers():
    assert flac.utf8_number(0) == b"\x00" and flac.utf8_number(127) == b"\x7f"
    assert flac.utf8_number(128) == b"\xc2\x80" and flac.utf8_number(2047) == b"\xdf\xbf"
    assert flac.utf8_number(2048) == b"\xe0\xa0\x80" and flac.utf8_number(65536) == b"\xf0\x90\x80\x80"
    assert len(flac.utf8_number((1 << 21) - 1)) == 4 and len(flac.utf8_number(1 << 21)) == 5
    assert len(flac.utf8_number((1 << 26) - 1)) == 5 and len(flac.utf8_number(1 << 26)) == 6
    assert flac.utf8_number((1 << 31) - 1) == b"\xfd\xbf\xbf\xbf\xbf\xbf"
    for v in (0, 127, 128, 2047, 2048, 65535, 65536, (1 << 21) - 1, 1 << 21, (1 << 26) + 5, (1 << 31) - 1):
        assert flac_ref._read_number(flac.utf8_number(v), 0) == (v, len(flac.utf8_number(v)))
        assert flac_ref._number(v) == flac.utf8_number(v)
    with pytest.raises(ValueError):
        flac.utf8_number(1 << 31)


# ---- the plan rule, the pitch, the stream pieces ---------------------------------------------------------------------------
def test_plan_rule():
    assert flac.plan(24000, 1920) == (24000, 1920)
    assert flac.plan(8000, 16, "pcm_s16le") == (8000, 16) and flac.plan(48000, 4608) == (48000, 4608)
    with pytest.raises(ValueError, match="16 to 4608"):
        flac.plan(24000, 15)
    with pytest.raises(ValueError, match="16 to 4608"):
        flac.plan(48000, 4609)
    with pytest.raises(ValueError, match="65535"):
        flac.plan(88200, 1920)
    for enc in ("mulaw", "alaw", "pcm_f32le"):
        with pytest.raises(ValueError, match="pcm_s16le"):
            flac.plan(24000, 1920, enc)
    assert flac.COMPRESSIONS == ("flac",)
    assert flac.normalise_compressions(["flac", "flac"]) == ["flac"]
    with pytest.raises(ValueError, match="not known"):
        flac.normalise_compressions(["mp3"])
    with pytest.raises(ValueError, match="list"):
        flac.normalise_compressions("flac")


def test_pitch():
    for w in (1, 8, 9, 16, 640, 1920, 4608, 5000):
        p = flac.pitch(w)
        assert p % 16 == 0 and p >= 16 + 4 * w and p >= 16 + 2 * w + 18 and p < 16 + max(4 * w, 2 * w + 18) + 16
    assert flac.pitch(1920) == 16 + 7680 and flac.pitch(4) == 16 + 32


def test_stream_header_layout():
    h = flac.stream_header(24000, 1920)
    assert len(h) == 42 and h[:4] == b"fLaC" and h[4:8] == bytes([0x80, 0, 0, 34])
    assert h[8:10] == h[10:12] == (1920).to_bytes(2, "big") and h[12:18] == bytes(6)
    packed = int.from_bytes(h[18:26], "big")
    assert packed >> 44 == 24000 and (packed >> 41) & 7 == 0 and (packed >> 36) & 31 == 15 and packed & ((1 << 36) - 1) == 0
    assert h[26:] == bytes(16)
    h2 = flac.stream_header(8000, 640, total_samples=(1 << 35) + 7)
    assert int.from_bytes(h2[18:26], "big") & ((1 << 36) - 1) == (1 << 35) + 7
    assert flac.patch_total(flac.stream_header(8000, 640), (1 << 35) + 7) == h2
    assert flac.patch_total(h2, 0) == flac.stream_header(8000, 640)


@pytest.mark.parametrize("rate,n", [(8000, 640), (11025, 882), (24000, 1920), (48000, 3840)])
def test_silence_tail(rate, n):
    tail = flac.silence(5, rate, n)
    frames = flac_ref.decode_frames(tail)
    assert [f[1] for f in frames] == list(range(5, 5 + len(frames))) and len(frames) == flac.silence_frames(rate, n)
    assert [f[3] for f in frames] == [n] * (rate // 5 // n) + ([rate // 5 % n] if rate // 5 % n else [])
    assert all(f[2] == rate and f[5] == "constant" and not f[0].any() for f in frames)
    assert sum(f[3] for f in frames) == rate // 5
    pcm, r, info = flac_ref.decode_stream(flac.stream_header(rate, n) + flac.silence(0, rate, n))
    assert r == rate and len(pcm) == rate // 5 and info["block"] == n


def test_frame_header_against_the_reference_encoder():
    for number in NUMBERS:
        for rate in (8000, 16000, 22050, 24000, 32000, 44100, 48000, 11025, 65535):
            x = np.full(64, 3, np.int16)
            f = flac_ref.encode_frame(x, number, rate)
            h = flac.frame_header(number, 64, rate)
            assert f[:len(h)] == h
            got = flac_ref.decode_frame(f)
            assert (got[1], got[2], got[3], got[4]) == (number, rate, 64, len(f))


# ---- encode, then decode ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_encode_decode_identity(n):
    kinds = {}
    for i, (name, x) in enumerate(signals(n).items()):
        number = NUMBERS[i % len(NUMBERS)]
        f = flac_ref.encode_frame(x, number, 24000 if n != 882 else 11025)
        assert len(f) <= 2 * n + 18
        y, num, rate, block, used, kind = flac_ref.decode_frame(f)
        assert np.array_equal(y, x) and num == number and block == n and used == len(f)
        kinds[name] = kind
    assert kinds["silence"] == kinds["dc"] == "constant" and kinds["noise"] == "verbatim"
    assert kinds["sine"] == kinds["impulse"] == "fixed"
    if n >= 640:
        assert kinds["ar2"] == "fixed"


def test_decoder_refuses_damage():
    x = signals(640)["ar2"]
    f = bytearray(flac_ref.encode_frame(x, 7, 8000))
    for at in (0, 1, 2, 3, 5, 8, 40, len(f) - 1):
        bad = bytearray(f)
        bad[at] ^= 0x10
        with pytest.raises(flac_ref.FlacError):
            flac_ref.decode_frame(bytes(bad))
    with pytest.raises(flac_ref.FlacError):
        flac_ref.decode_frame(bytes(f[:-3]))
    with pytest.raises(flac_ref.FlacError):
        flac_ref.decode_stream(b"fLaX" + bytes(f))


def test_decoder_reads_partitioned_rice():
    """a frame this project never writes: FIXED order 2, partition order 2, one escaped partition"""
    n, x = 64, (np.arange(64) ** 2 % 97 - 40).astype(np.int16)
    e = flac_ref.residuals(x, 2)
    u = ((e << 1) ^ (e >> 63)).tolist()
    bits = format(0x10 | (2 << 1), "08b") + "".join(format(int(v) & 0xFFFF, "016b") for v in x[:2]) + "00" + "0010"
    at = 0
    for part in range(4):
        count = 16 - (2 if part == 0 else 0)
        if part == 2:  # escape: raw 9-bit residuals
            bits += "1111" + format(9, "05b") + "".join(format(int(v) & 0x1FF, "09b") for v in e[at:at + count])
        else:
            k = part + 1
            bits += format(k, "04b") + "".join("0" * (v >> k) + "1" + format(v & ((1 << k) - 1), f"0{k}b") for v in u[at:at + count])
        at += count
    bits += "0" * (-len(bits) % 8)
    body = flac.frame_header(3, n, 8000) + int(bits, 2).to_bytes(len(bits) // 8, "big")
    f = body + flac.crc16(body).to_bytes(2, "big")
    y = flac_ref.decode_frame(f)[0]
    assert np.array_equal(y, x)


# ---- routing ----------------------------------------------------------------------------------------------------------
def test_route_and_its_refusals():
    t = ChainTable(24000, 1920, sample_rates=[8000], level=True, encodings=["mulaw"], compressions=["flac"])
    assert t.compressions == ["flac"] and t.encodings == ["pcm_s16le", "mulaw"] and not t.empty
    r = t.route(sample_rate=8000, gain_db=6.0, compression="flac")
    assert r.compression == "flac" and r.encoding == "pcm_s16le" and r.n_out == 640 and r.preroll > 0
    assert r.drain_frames == -(-r.preroll // 640)
    assert t.route().compression is None and t.route(encoding="mulaw").compression is None
    with pytest.raises(ValueError, match="pcm_s16le"):
        t.route(encoding="mulaw", compression="flac")
    with pytest.raises(ValueError, match="not configured"):
        t.route(compression="mp3")
    plain = ChainTable(24000, 1920, encodings=["mulaw"])
    with pytest.raises(ValueError, match="build it with\\s+compressions"):
        plain.route(compression="flac")
    assert plain.route().compression is None
    # the packer brings the encoder
    assert ChainTable(24000, 1920, compressions=["flac"]).encodings == ["pcm_s16le"]
    # a line the plan rule refuses: 48 kHz doubles the frame to 3840 samples, 96 kHz would pass both limits
    wide = ChainTable(24000, 6000, compressions=["flac"])
    with pytest.raises(ValueError, match="16 to 4608"):
        wide.route(compression="flac")
    with pytest.raises(ValueError, match="no compression"):
        ChainTable(24000, 1920, compressions=[])
    # Route keeps its positional order: compression is appended with a default
    assert Route(0, 24000, None, False, None, 1920, 0, 0, None).compression is None


def test_spec_and_for_request():
    spec = ChainSpec(sample_rates=[8000], compressions=["flac"])
    assert spec.compressions == ("flac",) and spec.tags() == ("rate", 8000, "comp")
    assert ChainSpec().tags() == () and list(ChainSpec.TAGS)[-1] == "compressions"
    spec, req = ChainTable.for_request(24000, 1920, sample_rate=8000, gain_db=6, compression="flac")
    assert spec == ChainSpec(sample_rates=(8000,), level=True, compressions=("flac",)) and req["compression"] == "flac"
    route = spec.table(24000, 1920).route(**req)
    assert route.compression == "flac" and route.encoding == "pcm_s16le"
    spec, req = ChainTable.for_request(24000, 1920, encoding="pcm_s16le", compression="flac")
    assert spec.encodings is not None and spec.compressions == ("flac",)
    with pytest.raises(RequestError, match="pcm_s16le") as e:
        ChainTable.for_request(24000, 1920, encoding="mulaw", compression="flac")
    assert e.value.field == "compression"
    with pytest.raises(RequestError, match="not configured"):
        ChainTable.for_request(24000, 1920, compression="ogg")
    # without the field the request is the dict it always was
    assert "compression" not in ChainTable.for_request(24000, 1920, sample_rate=8000)[1]


# ---- the stream helper ----------------------------------------------------------------------------------------------------
def test_flac_stream_bytes():
    from pocket_tts_amd.main import flac_stream_bytes

    rate, n = 8000, 640
    blocks = [signals(n, seed=s)["ar2"] for s in range(3)]
    chunks = [np.frombuffer(flac_ref.encode_frame(x, i, rate), np.uint8) for i, x in enumerate(blocks)]
    parts = list(flac_stream_bytes(iter(chunks), rate, n))
    assert parts[0] == flac.stream_header(rate, n) and parts[1:4] == [c.tobytes() for c in chunks]
    assert parts[4] == flac.silence(3, rate, n) and len(parts) == 5
    pcm, r, info = flac_ref.decode_stream(b"".join(parts))
    assert r == rate and np.array_equal(pcm, np.concatenate([*blocks, np.zeros(rate // 5, np.int16)]))
    # a stream without frames is the header and the tail
    pcm, _, _ = flac_ref.decode_stream(b"".join(flac_stream_bytes(iter(()), rate, n)))
    assert len(pcm) == rate // 5 and not pcm.any()


# ---- the server's form handling, with the stub batcher of test_server_cpu.py ------------------------------------------------
def test_server_container_flac(tmp_path):
    import asyncio

    import httpx
    import torch

    import test_server_cpu as ts
    from pocket_tts_amd.server import create_app

    rate, n = 8000, 640
    blocks = [signals(n, seed=s)["ar2"] for s in range(3)]

    class Req:
        def iter_batches(self):  # two frames in one batch, then one
            f = [torch.from_numpy(np.frombuffer(flac_ref.encode_frame(x, i, rate), np.uint8).copy()) for i, x in enumerate(blocks)]
            yield f[:2]
            yield f[2:]

    class Batcher(ts._StubBatcher):
        def submit(self, state, text, fae=None, **settings):
            self.submitted.append(settings)
            return Req() if settings.get("compression") else ts._StubRequest(3)

    (tmp_path / "v1.safetensors").write_bytes(b"x")

    def run(forms, **chain):
        stub = Batcher()
        app = create_app(ts._StubModel(), slots=4, capacity=64, voices_dir=tmp_path, default_voice="v1",
                         batcher_factory=lambda m, s, c: stub, **chain)

        async def go():
            async with app.router.lifespan_context(app):
                async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t") as cl:
                    return [await cl.post("/tts", data=d) for d in forms]

        return asyncio.run(go()), stub

    res, stub = run([{"text": "hi", "container": "flac", "sample_rate": "8000"},
                     {"text": "hi", "container": "flac", "sample_rate": "8000", "encoding": "mulaw"},
                     {"text": "hi", "container": "flac", "sample_rate": "8000", "encoding": "pcm_s16le"},
                     {"text": "hi", "container": "ogg"}, {"text": "hi"}],
                    sample_rates=[8000], encodings=["mulaw"], compressions=["flac"])
    assert res[0].status_code == 200 and res[0].headers["content-type"] == "audio/flac"
    pcm, r, info = flac_ref.decode_stream(res[0].content)
    assert r == rate and info["block"] == n and np.array_equal(pcm, np.concatenate([*blocks, np.zeros(rate // 5, np.int16)]))
    assert stub.submitted[0]["compression"] == "flac" and stub.submitted[0]["sample_rate"] == 8000
    assert res[1].status_code == 400 and "pcm_s16le" in res[1].json()["detail"]
    assert res[2].status_code == 200 and res[2].headers["content-type"] == "audio/flac"
    assert res[3].status_code == 400 and "flac" in res[3].json()["detail"]
    assert res[4].status_code == 200 and res[4].headers["content-type"] == "audio/wav" and "compression" not in stub.submitted[-1]
    # a server started without it answers as before, word for word
    res, stub = run([{"text": "hi", "container": "flac"}])
    assert res[0].status_code == 400 and res[0].json()["detail"] == "container must be 'wav' or 'raw', got 'flac'"
    assert not stub.submitted


# ---- the kernel's lanes as a host program ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path_factory.mktemp("flac_sweep") / "flac_sweep"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-static-libasan", "-static-libubsan", "-I", str(ROOT / "pocket_tts_amd" / "csrc"), "-o", str(exe),
                        str(ROOT / "tests" / "cpp" / "flac_sweep.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_sweep(exe, tmp_path, cases):
    """cases: [(n, preroll, first_block, rate, lines int16 [L, n])] -> per case the list of each line's bytes"""
    blob = struct.pack("<i", len(cases))
    for n, preroll, first, rate, lines in cases:
        lines = np.ascontiguousarray(lines, dtype=np.int16)
        assert lines.shape[1] == n
        blob += struct.pack("<5i", n, preroll, first, rate, len(lines)) + lines.tobytes()
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # the leak checker needs ptrace, which build sandboxes often deny
    r = subprocess.run([str(exe), str(path)], capture_output=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    out, at, got = r.stdout, 0, []
    for n, preroll, first, rate, lines in cases:
        frames = []
        for _ in range(len(lines)):
            (nbytes,) = struct.unpack_from("<I", out, at)
            frames.append(out[at + 4:at + 4 + nbytes])
            at += 4 + nbytes
        got.append(frames)
    assert at == len(out)
    return got


def expected_lines(n, preroll, first, rate, lines):
    """what the contract says each line of a row emits: nothing while it leads, then the blocks cut at the pre-roll"""
    flat = np.concatenate(list(lines))
    lead = -(-preroll // n)
    return [b"" if f < lead else flac_ref.encode_frame(flat[preroll + (f - lead) * n:preroll + (f - lead + 1) * n], first + f - lead, rate)
            for f in range(len(lines))]


def test_host_sweep_signals(sweep_exe, tmp_path):
    cases = []
    for n in NS:
        sig = signals(n)
        cases.append((n, 0, NUMBERS[NS.index(n)], 24000 if n != 882 else 11025, np.stack(list(sig.values()))))
    got = run_sweep(sweep_exe, tmp_path, cases)
    for case, frames in zip(cases, got):
        assert frames == expected_lines(*case), f"n = {case[0]}"


def test_host_sweep_carry_cut_and_numbers(sweep_exe, tmp_path):
    n = 640
    lines = np.stack([signals(n, seed=s)[name] for s, name in enumerate(("ar2", "sine", "impulse", "ar2", "noise", "square"))])
    cases = [(n, p, first, 8000, lines) for p, first in ((0, 0), (1, 127), (639, 2047), (640, 65535), (1000, 5))]
    got = run_sweep(sweep_exe, tmp_path, cases)
    for case, frames in zip(cases, got):
        want = expected_lines(*case)
        assert [len(f) for f in frames] == [len(f) for f in want]
        assert frames == want, f"preroll = {case[1]}"
        assert [f == b"" for f in frames] == [i < -(-case[1] // n) for i in range(len(lines))]


def test_host_sweep_last_word_edges(sweep_exe, tmp_path):
    """frames of every length modulo 4: the bit buffer of the host program ends with the frame's last word, so a code, a
    sample or the CRC written one word too far is a sanitizer error"""
    rng = np.random.default_rng(5)
    cases, lengths = [], set()
    for n in range(16, 48):
        x = np.cumsum(rng.integers(-6, 7, n)).astype(np.int16)
        cases.append((n, 0, n, 16000, x[None, :]))
        cases.append((n, 0, n, 12345, rng.integers(-32768, 32768, n).astype(np.int16)[None, :]))
    got = run_sweep(sweep_exe, tmp_path, cases)
    for case, frames in zip(cases, got):
        assert frames == expected_lines(*case)
        lengths.add(len(frames[0]) % 4)
    assert lengths == {0, 1, 2, 3}
