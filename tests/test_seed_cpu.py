"""Per-request seeds without a GPU: the chunk-seed helper against a numpy restatement, the server's `seed` form field
down to the batcher's `submit` keywords, and `generate --seed`."""

import asyncio

import numpy as np
import pytest

from test_server_cpu import _StubBatcher, _StubModel

C_GOLDEN = 0x9E3779B97F4A7C15  # the multiplier of the device generator's hash key (counter_normal in ptts_kernels.h)
SEEDS = [0, 1, 7, 12345, 2 ** 31 - 1, 2 ** 62 + 3, 2 ** 63 - 1]


def _np_mix64(z):
    z = np.uint64(z)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _np_chunk_seed(seed: int, i: int) -> int:
    if i == 0:
        return seed
    return int(_np_mix64(_np_mix64(seed) ^ np.uint64(i)))


def test_chunk_seed_matches_numpy_and_chunk_zero_is_the_seed():
    from noise_ref import _mix64
    from pocket_tts_amd.engine import chunk_seed

    with np.errstate(over="ignore"):
        assert int(_np_mix64(12345)) == int(_mix64(np.uint64(12345)))  # the restatement is the generator's mix64
    for s in SEEDS:
        assert chunk_seed(s, 0) == s
        for i in range(12):
            v = chunk_seed(s, i)
            assert type(v) is int and 0 <= v < 2 ** 64
            assert v == _np_chunk_seed(s, i), (s, i)


@pytest.mark.parametrize("seed", SEEDS)
def test_chunk_seeds_are_distinct_and_not_shifted_copies(seed):
    """seeds a and b with a - b = n C (mod 2^64) hash the same keys n steps apart: no two chunk seeds of a request may
    be related by a multiplier below 2^32 (n = d * C^-1 mod 2^64, either sign)"""
    from pocket_tts_amd.engine import chunk_seed

    cs = [chunk_seed(seed, i) for i in range(8)]
    assert len(set(cs)) == 8
    c_inv = pow(C_GOLDEN, -1, 2 ** 64)
    assert (C_GOLDEN * c_inv) % 2 ** 64 == 1
    for i in range(8):
        for j in range(8):
            if i != j:
                n = ((cs[i] - cs[j]) % 2 ** 64) * c_inv % 2 ** 64
                assert n >= 2 ** 32, (i, j, n)


@pytest.mark.parametrize("bad", [True, False, 1.0, 0.5, -1, 2 ** 63, 2 ** 64, "3", None, float("nan")])
def test_invalid_seeds_raise(bad):
    from pocket_tts_amd.engine import check_seed, chunk_seed

    with pytest.raises(ValueError):
        chunk_seed(bad, 0)
    with pytest.raises(ValueError):
        chunk_seed(bad, 1)
    with pytest.raises(ValueError):
        check_seed(bad)


def test_numpy_integers_are_seeds_and_bad_chunk_indices_raise():
    from pocket_tts_amd.engine import chunk_seed

    assert chunk_seed(np.int64(5), 0) == 5 and chunk_seed(np.int64(5), 2) == chunk_seed(5, 2)
    for bad in (-1, 1.0, True, 2 ** 32):
        with pytest.raises(ValueError):
            chunk_seed(1, bad)


def test_parse_seed():
    from pocket_tts_amd.server import FormError, parse_seed

    assert parse_seed({}) is None and parse_seed({"seed": ""}) is None and parse_seed({"seed": "  "}) is None
    assert parse_seed({"seed": "7"}) == 7 and parse_seed({"seed": " 0 "}) == 0
    assert parse_seed({"seed": str(2 ** 63 - 1)}) == 2 ** 63 - 1
    for raw in ("-1", "1.5", "x", "nan", "1e3", str(2 ** 63), "0x10", "True"):
        with pytest.raises(FormError):
            parse_seed({"seed": raw})


def test_parse_settings_keys_do_not_grow():
    from pocket_tts_amd.server import parse_settings

    assert "seed" not in parse_settings({"seed": "7"})


def _post(tmp_path, forms):
    import httpx

    from pocket_tts_amd.server import create_app

    (tmp_path / "v1.safetensors").write_bytes(b"x")
    stub = _StubBatcher()
    app = create_app(_StubModel(), slots=4, capacity=64, voices_dir=tmp_path, default_voice="v1",
                     batcher_factory=lambda m, s, c: stub)

    async def go():
        async with app.router.lifespan_context(app):
            async with httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t") as cl:
                return [await cl.post("/tts", data=f) for f in forms], await cl.get("/")

    (res, index), = [asyncio.run(go())]
    return res, index, stub


def test_seed_reaches_submit_and_absence_passes_no_keyword(tmp_path):
    res, index, stub = _post(tmp_path, [{"text": "hi", "seed": "7"}, {"text": "hi"}, {"text": "hi", "seed": ""},
                                        {"text": "hi", "seed": str(2 ** 63 - 1), "temperature": "0.2"}])
    assert [r.status_code for r in res] == [200, 200, 200, 200]
    kw = [s[3] for s in stub.submitted]
    assert kw[0]["seed"] == 7 and type(kw[0]["seed"]) is int
    assert "seed" not in kw[1] and "seed" not in kw[2]
    assert kw[3]["seed"] == 2 ** 63 - 1 and kw[3]["temperature"] == 0.2
    assert 'name="seed"' in index.text


@pytest.mark.parametrize("raw", ["-1", "2.5", "x", str(2 ** 63), "nan"])
def test_bad_seed_gets_400(tmp_path, raw):
    res, _, stub = _post(tmp_path, [{"text": "hi", "seed": raw}])
    assert res[0].status_code == 400 and "seed" in res[0].json()["detail"]
    assert stub.submitted == []


def test_generate_seed_flag():
    from pocket_tts_amd.main import build_parser

    a = build_parser().parse_args(["generate", "--seed", "42"])
    assert a.seed == 42
    assert build_parser().parse_args(["generate"]).seed is None
    with pytest.raises(SystemExit):
        build_parser().parse_args(["generate", "--seed", "x"])


def test_entry_points_take_a_seed():
    import inspect

    from pocket_tts_amd.batching import ContinuousBatcher
    from pocket_tts_amd.engine import LMState
    from pocket_tts_amd.tts_model import TTSModel

    for fn, name in ((TTSModel.generate_audio, "seed"), (TTSModel.generate_audio_stream, "seed"),
                     (TTSModel.generate_audio_batch, "seeds"), (ContinuousBatcher.submit, "seed")):
        p = inspect.signature(fn).parameters
        named = [k for k, v in p.items() if v.kind is not v.VAR_KEYWORD]  # behind them only `**request`, the chain's fields
        assert name in p and p[name].default is None and named[-1] == name, fn  # a new trailing keyword
    assert hasattr(LMState, "set_row_seed") and hasattr(LMState, "clear_row_seed")
