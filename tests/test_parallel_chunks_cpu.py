"""Text chunks of one request in parallel rows, the parts that need no GPU: the chunk order (`chunk_order.ChunkOrder`), the
host-side FLAC renumbering (`flac.renumber`), and what the batcher, the server and the command line accept."""

import asyncio
import itertools
import json
import queue
import random

import numpy as np
import pytest

import flac_ref
from pocket_tts_amd import flac
from pocket_tts_amd.chunk_order import ChunkOrder

# ---- the chunk order ------------------------------------------------------------------------------------------------------
SIZES = (3, 1, 4)
SERIAL = [(k, i) for k, n in enumerate(SIZES) for i in range(n)]
# an order is a string of events: a digit pushes the chunk's next item, the letter (a, b, c) finishes chunk 0, 1, 2
ORDERS = {
    "serial": "000a1b2222c",
    "round robin": "0120202a2bc",
    "last chunk finishes first": "2222c01b00a",
    "chunk 1 finishes before chunk 0 has produced anything": "1b000a2222c",
    "all later chunks done before chunk 0 starts": "22122bc000a",
    "every chunk finishes in reverse": "22221000cba",
    "chunk 0 ends early, 2 overtakes 1": "000a22221cb",
    "interleaved, middle finishes first": "01b20202a2c",
}


def _play(order, on_push=None):
    got, nxt = [], [0, 0, 0]
    co = ChunkOrder(len(SIZES), got.append)
    for ev in order:
        if ev.isdigit():
            k = int(ev)
            item = (k, nxt[k])
            nxt[k] += 1
            before = len(got)
            co.push(k, item)
            if on_push is not None:
                on_push(co, k, item, got, before)
        else:
            co.finish("abc".index(ev))
    assert nxt == list(SIZES), "the order does not push every item"
    return got


def test_the_orders_are_what_their_names_say():
    assert len(ORDERS) >= 6 and len(set(ORDERS.values())) == len(ORDERS)
    for name, order in ORDERS.items():
        assert sorted(order) == sorted("0" * 3 + "1" + "2" * 4 + "abc"), name
        for k, letter in enumerate("abc"):  # a chunk finishes behind its last item
            assert order.index(letter) > order.rindex(str(k)), name
    o = ORDERS["last chunk finishes first"]
    assert o.index("c") < o.index("a") and o.index("c") < o.index("b")
    o = ORDERS["chunk 1 finishes before chunk 0 has produced anything"]
    assert o.index("b") < o.index("0")


@pytest.mark.parametrize("name", list(ORDERS))
def test_every_interleaving_gives_the_serial_sequence(name):
    def on_push(co, k, item, got, before):
        if k == 0:  # chunk 0 is never held
            assert got[before:] == [item]
        assert None not in got

    got = _play(ORDERS[name], on_push)
    assert got == SERIAL + [None], name


def test_every_interleaving_of_a_small_case():
    """two chunks of two items: all 20 orders of the six events in which a chunk finishes behind its items"""
    events, n = "0011ab", 0
    for perm in set(itertools.permutations(events)):
        if perm.index("a") < max(i for i, e in enumerate(perm) if e == "0") or \
                perm.index("b") < max(i for i, e in enumerate(perm) if e == "1"):
            continue
        got, nxt = [], [0, 0]
        co = ChunkOrder(2, got.append)
        for ev in perm:
            if ev.isdigit():
                co.push(int(ev), (int(ev), nxt[int(ev)]))
                nxt[int(ev)] += 1
            else:
                co.finish("ab".index(ev))
        assert got == [(0, 0), (0, 1), (1, 0), (1, 1), None], perm
        n += 1
    assert n == 20


def test_items_behind_a_flush_pass_straight_through():
    got = []
    co = ChunkOrder(2, got.append)
    co.push(1, "b0")
    co.push(0, "a0")
    assert got == ["a0"]
    co.finish(0)
    assert got == ["a0", "b0"]
    co.push(1, "b1")  # chunk 1 is the head now
    assert got == ["a0", "b0", "b1"]
    co.finish(1)
    assert got == ["a0", "b0", "b1", None]


def test_the_queue_of_a_request_is_what_it_feeds():
    q = queue.Queue()
    co = ChunkOrder(2, q.put)
    co.push(1, "y")
    co.push(0, "x")
    co.finish(1)
    co.finish(0)
    assert [q.get_nowait() for _ in range(3)] == ["x", "y", None] and q.empty()


def test_cancel_in_the_middle():
    got = []
    co = ChunkOrder(3, got.append)
    co.push(0, "a0")
    co.push(1, "b0")
    co.push(2, "c0")
    co.cancel()
    assert got == ["a0", None]
    co.push(0, "a1")   # rows still in flight: dropped
    co.finish(0)
    co.push(1, "b1")
    co.finish(1)
    co.finish(2)
    co.cancel()
    assert got == ["a0", None]


def test_cancel_after_the_end_does_nothing():
    got = []
    co = ChunkOrder(1, got.append)
    co.push(0, "a")
    co.finish(0)
    co.cancel()
    assert got == ["a", None]


def test_misuse_is_refused():
    co = ChunkOrder(2, lambda item: None)
    with pytest.raises(ValueError):
        co.push(2, "x")
    co.finish(1)
    with pytest.raises(ValueError):
        co.push(1, "x")
    with pytest.raises(ValueError):
        co.finish(1)
    with pytest.raises(ValueError):
        ChunkOrder(0, lambda item: None)


# ---- flac.renumber --------------------------------------------------------------------------------------------------------
NUMBERS = (0, 1, 127, 128, 2047, 2048, 65535, 65536)


@pytest.mark.parametrize("rate", [8000, 24000])
@pytest.mark.parametrize("n", [16, 1920, 4608])
def test_renumber_silent_frames(n, rate):
    for a in NUMBERS:
        frame = flac.silent_frame(a, n, rate)
        for b in NUMBERS:
            assert flac.renumber(frame, b) == flac.silent_frame(b, n, rate), (a, b)


def test_renumber_equals_the_full_rebuild():
    rng = random.Random(20)
    sizes = [1, 2, 3, 15, 16, 17, 255, 256, 3000] + [rng.randrange(1, 3001) for _ in range(12)]
    for size in sizes:
        body = rng.randbytes(size)
        for n, rate in ((1920, 24000), (640, 8000), (1764, 22051)):  # 22051: the rate travels in the header
            a, b = rng.choice(NUMBERS), rng.choice(NUMBERS)
            old = flac.frame_header(a, n, rate) + body
            old += flac.crc16(old).to_bytes(2, "big")
            new = flac.frame_header(b, n, rate) + body
            new += flac.crc16(new).to_bytes(2, "big")
            assert flac.renumber(old, b) == new, (size, n, rate, a, b)


def test_renumbered_frames_decode_to_the_same_samples():
    rng = np.random.default_rng(3)
    t = np.arange(1920)
    blocks = {"constant": np.full(1920, -7, np.int16),
              "verbatim": rng.integers(-32768, 32768, 1920).astype(np.int16),
              "fixed": (8000 * np.sin(t / 40.0)).astype(np.int16)}
    for kind, x in blocks.items():
        for a, b in ((0, 5), (5, 128), (130, 3), (2047, 65536), (70000, 0)):
            frame = flac_ref.encode_frame(x, a, 24000)
            y, number, rate, size, used, got_kind = flac_ref.decode_frame(frame)
            assert number == a and got_kind == kind
            out = flac.renumber(frame, b)
            y2, number2, rate2, size2, used2, kind2 = flac_ref.decode_frame(out)  # checks both CRCs
            assert (number2, rate2, size2, kind2, used2) == (b, rate, size, kind, len(out))
            assert np.array_equal(y2, x) and np.array_equal(y, x)
            assert out == flac_ref.encode_frame(x, b, 24000)


def test_renumber_refuses_what_is_no_frame():
    frame = flac.silent_frame(3, 1920, 24000)
    for bad in (b"", frame[:5], b"\x00" + frame[1:], frame[:4] + b"\x80" + frame[5:], frame[:6] + b"\xff" + frame[7:]):
        with pytest.raises(ValueError):
            flac.renumber(bad, 1)
    with pytest.raises(ValueError):
        flac.renumber(frame, -1)
    with pytest.raises(ValueError):
        flac.renumber(frame, 1 << 31)


# ---- validation -----------------------------------------------------------------------------------------------------------
BAD = (0, -1, 1.5, True)


@pytest.mark.parametrize("bad", BAD)
def test_constructor_refuses_a_bad_window(bad):
    from pocket_tts_amd.batching import ContinuousBatcher, check_parallel_chunks

    with pytest.raises(ValueError, match="parallel_chunks"):
        ContinuousBatcher(None, parallel_chunks=bad)  # refused before the model or the GPU is touched
    with pytest.raises(ValueError, match="parallel_chunks"):
        check_parallel_chunks(bad)


@pytest.mark.parametrize("bad", BAD + (5,))
def test_submit_refuses_a_bad_window(bad):
    """`submit` checks the window before it looks at the model: a bare object with the constructor's bound is enough"""
    from pocket_tts_amd.batching import ContinuousBatcher, check_parallel_chunks

    cb = object.__new__(ContinuousBatcher)
    cb.model, cb._failed, cb.parallel_chunks = None, None, 4
    with pytest.raises(ValueError, match="parallel_chunks"):
        cb.submit({}, "Hello.", parallel_chunks=bad)
    with pytest.raises(ValueError, match="parallel_chunks"):
        cb.submit_script([({}, "Hello.")], parallel_chunks=bad)
    with pytest.raises(ValueError, match="parallel_chunks"):
        check_parallel_chunks(bad, 4)
    assert [check_parallel_chunks(v, 4) for v in (1, 4, np.int64(2))] == [1, 4, 2]
    with pytest.raises(ValueError, match="empty"):
        cb.submit_script([({}, "Hello."), ({}, "  ")])
    with pytest.raises(ValueError, match="segment"):
        cb.submit_script([])


def test_command_line_flags():
    from pocket_tts_amd.main import build_parser

    p = build_parser()
    assert p.parse_args(["generate"]).parallel_chunks == 1
    assert p.parse_args(["serve"]).parallel_chunks == 1
    assert p.parse_args(["generate", "--parallel-chunks", "4"]).parallel_chunks == 4
    assert p.parse_args(["serve", "--parallel-chunks", "16"]).parallel_chunks == 16
    with pytest.raises(SystemExit):
        p.parse_args(["generate", "--parallel-chunks", "many"])


def test_create_app_refuses_a_bad_window():
    from pocket_tts_amd.server import create_app
    from test_server_cpu import _StubModel

    for bad in BAD:
        with pytest.raises(ValueError, match="parallel_chunks"):
            create_app(_StubModel(), slots=4, capacity=64, parallel_chunks=bad)


def _post(tmp_path, forms):
    import httpx

    from pocket_tts_amd.server import create_app
    from test_server_cpu import _StubBatcher, _StubModel, _StubRequest

    class Stub(_StubBatcher):
        def submit_script(self, segments, fae=None, **settings):
            self.submitted.append((segments, fae, settings))
            return _StubRequest(2)

    for name in ("v1", "v2"):
        (tmp_path / f"{name}.safetensors").write_bytes(b"x")
    stub = Stub()
    app = create_app(_StubModel(), slots=4, capacity=64, voices_dir=tmp_path, default_voice="v1", parallel_chunks=4,
                     batcher_factory=lambda m, s, c: stub)

    async def go():
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t") as cl:
                return [await cl.post("/tts", data=d) for d in forms]

    return asyncio.run(go()), stub


def test_script_reaches_submit_script(tmp_path):
    script = [{"voice": "v1", "text": "Hello."}, {"voice": "v2", "text": "Hi there."}, {"text": "Bye."}]
    res, stub = _post(tmp_path, [{"script": json.dumps(script), "seed": "3"}, {"text": "plain"}])
    assert [r.status_code for r in res] == [200, 200], [r.text for r in res]
    segments, fae, settings = stub.submitted[0]
    v1, v2 = {"voice": str(tmp_path / "v1.safetensors")}, {"voice": str(tmp_path / "v2.safetensors")}
    assert segments == [(v1, "Hello."), (v2, "Hi there."), (v1, "Bye.")] and fae is None and settings["seed"] == 3
    assert segments[0][0] is segments[2][0]  # one object per voice: the batcher's voice cache hits
    assert "parallel_chunks" not in settings  # the batcher's own window applies
    assert len(res[0].content) == 44 + 2 * 8 + 2 * 4800
    assert stub.submitted[1][1] == "plain"


def test_script_400s_name_the_entry(tmp_path):
    ok = {"voice": "v1", "text": "Hello."}
    cases = [
        ({"script": "[{"}, "JSON"),
        ({"script": "{\"voice\": \"v1\"}"}, "list"),
        ({"script": "[]"}, "empty"),
        ({"script": json.dumps([ok, {"voice": "v2"}])}, "script[1]"),
        ({"script": json.dumps([ok, ok, {"voice": "v2", "text": "  "}])}, "script[2]"),
        ({"script": json.dumps([ok, "Hello."])}, "script[1]"),
        ({"script": json.dumps([{"voice": "nobody", "text": "Hello."}])}, "script[0]"),
        ({"script": json.dumps([ok, {"voice": 7, "text": "Hello."}])}, "script[1]"),
        ({"script": json.dumps([ok] * 257)}, "256"),
        ({"script": json.dumps([ok]), "text": "Hello."}, "text"),
        ({"script": json.dumps([ok]), "voice_url": "v1"}, "voice_url"),
    ]
    res, stub = _post(tmp_path, [c[0] for c in cases] + [{"script": json.dumps([ok] * 256)}])
    assert res[-1].status_code == 200
    for r, (_, word) in zip(res, cases):
        assert r.status_code == 400 and word in r.json()["detail"], (word, r.text)
    assert "unknown voice" in res[6].json()["detail"]
    assert len(stub.submitted) == 1


def test_script_excludes_an_upload():
    from pocket_tts_amd.server import FormError, parse_script

    good = json.dumps([{"voice": "v1", "text": "Hello."}])
    assert parse_script({"script": good}, {}) == [("v1", "Hello.")]
    assert parse_script({"text": "x"}, {}) is None and parse_script({"script": " "}, {}) is None
    with pytest.raises(FormError, match="voice_wav"):
        parse_script({"script": good}, {"voice_wav": ("p.wav", b"RIFF")})
