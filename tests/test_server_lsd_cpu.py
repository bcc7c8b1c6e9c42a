"""The server's `lsd_decode_steps` form field without a GPU: parsed and range-checked against the server's maximum,
handed to the batcher's `submit` as an int, absent or empty passes nothing (the model's count)."""

import asyncio

import pytest

from test_server_cpu import _StubBatcher, _StubModel


def _post(tmp_path, forms, max_lsd=4):
    import httpx

    from pocket_tts_amd.server import create_app

    (tmp_path / "v1.safetensors").write_bytes(b"x")
    stub = _StubBatcher()
    app = create_app(_StubModel(), slots=4, capacity=64, voices_dir=tmp_path, default_voice="v1",
                     batcher_factory=lambda m, s, c: stub, max_lsd_decode_steps=max_lsd)

    async def go():
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t") as cl:
                return [await cl.post("/tts", data=f) for f in forms]

    return asyncio.run(go()), stub


def test_lsd_decode_steps_reaches_submit(tmp_path):
    res, stub = _post(tmp_path, [{"text": "hi", "lsd_decode_steps": "3"}, {"text": "hi", "lsd_decode_steps": "4"},
                                 {"text": "hi", "lsd_decode_steps": "1", "temperature": "0.2"}])
    assert [r.status_code for r in res] == [200, 200, 200]
    got = [s[3]["lsd_decode_steps"] for s in stub.submitted]
    assert got == [3, 4, 1] and all(type(v) is int for v in got)
    assert stub.submitted[2][3]["temperature"] == 0.2


@pytest.mark.parametrize("raw", ["0", "5", "2.5", "x", "-1", "nan"])
def test_bad_lsd_decode_steps_gets_400(tmp_path, raw):
    res, stub = _post(tmp_path, [{"text": "hi", "lsd_decode_steps": raw}])
    assert res[0].status_code == 400 and "lsd_decode_steps" in res[0].json()["detail"]
    assert stub.submitted == []


def test_absent_or_empty_lsd_decode_steps_passes_none(tmp_path):
    res, stub = _post(tmp_path, [{"text": "hi"}, {"text": "hi", "lsd_decode_steps": ""},
                                 {"text": "hi", "lsd_decode_steps": "  "}])
    assert [r.status_code for r in res] == [200, 200, 200]
    assert [s[3].get("lsd_decode_steps") for s in stub.submitted] == [None, None, None]


def test_default_maximum_is_the_model_count(tmp_path):
    res, stub = _post(tmp_path, [{"text": "hi", "lsd_decode_steps": "1"}, {"text": "hi", "lsd_decode_steps": "2"}],
                      max_lsd=None)
    assert [r.status_code for r in res] == [200, 400]


def test_parse_lsd_steps():
    from pocket_tts_amd.server import FormError, parse_lsd_steps

    assert parse_lsd_steps({}, 4) is None and parse_lsd_steps({"lsd_decode_steps": ""}, 4) is None
    assert parse_lsd_steps({"lsd_decode_steps": " 2 "}, 4) == 2
    for raw in ("0", "5", "2.5", "x"):
        with pytest.raises(FormError):
            parse_lsd_steps({"lsd_decode_steps": raw}, 4)


def test_serve_flag():
    from pocket_tts_amd.main import build_parser

    a = build_parser().parse_args(["serve", "--lsd-decode-steps", "2", "--max-lsd-decode-steps", "5"])
    assert a.lsd_decode_steps == 2 and a.max_lsd_decode_steps == 5
    a = build_parser().parse_args(["serve"])
    assert a.max_lsd_decode_steps is None
