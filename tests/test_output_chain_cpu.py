"""The planning half of the output chain (pocket_tts_amd/output_chain.py) against the rule modules composed directly:
no GPU, no library."""

import itertools

import numpy as np
import pytest

from pocket_tts_amd import encoding, level, loudness, pitch, resample, stretch
from pocket_tts_amd import tone as tone_rule
from pocket_tts_amd.output_chain import ChainSpec, ChainTable, RequestError, Route

NATIVE, FS = 24000, 1920
RATES = [None, 8000, 16000, 22050, 44100, 48000]
SPEEDS = [None, 0.5, 0.8, 0.9, 1.0, 1.25, 1.5, 2.0]
GAINS = [None, (6, None), (-3, -6)]
# what the plan rule refuses: 0.9 wherever 9 divides no frame, 1.5 at 8 and 16 kHz, 1.25 at 22.05 and 44.1 kHz
REFUSED = {(0.9, r) for r in (24000, 8000, 16000, 48000)} | {(1.5, 8000), (1.5, 16000), (1.25, 22050), (1.25, 44100)}


@pytest.fixture(scope="module")
def table():
    return ChainTable(NATIVE, FS, [r for r in RATES if r], [s for s in SPEEDS if s], level=True)


def _compose(rate, speed, gain):
    """resample.plan -> stretch.plan -> level.plan of one request, composed by hand"""
    rp = resample.plan(rate or NATIVE, NATIVE, FS)
    sp = stretch.identity(rp.rate, rp.out_n) if speed in (None, 1.0) else stretch.plan(speed, rp.rate, rp.out_n)
    lp = None if gain is None else level.plan(rp.rate, sp.n_out)
    return rp, sp, lp


def _admitted(table):
    for rate, speed, gain in itertools.product(RATES, SPEEDS, GAINS):
        if (speed, rate or NATIVE) not in REFUSED:
            yield rate, speed, gain, table.route(rate, speed, *(gain or (None, None)))


def test_routes_equal_the_rules_composed_directly(table):
    seen = set()
    for rate, speed, gain in itertools.product(RATES, SPEEDS, GAINS):
        args = (rate, speed, *(gain or (None, None)))
        try:
            rp, sp, lp = _compose(rate, speed, gain)
        except ValueError as e:
            assert (speed, rate or NATIVE) in REFUSED and "whole number of hops" in str(e)  # the rule's own message
            with pytest.raises(ValueError, match=f"not admissible at {rate or NATIVE} Hz"):
                table.route(*args)
            seen.add((rate or NATIVE, False))
            continue
        assert (speed, rate or NATIVE) not in REFUSED
        seen.add((rate or NATIVE, True))
        r = table.route(*args)
        pre = sp.preroll + (lp.LA if lp else 0)
        assert (r.rate, r.rate_index, r.n_out, r.preroll) == (rp.rate, table.rates.index(rp.rate), sp.n_out, pre)
        assert table.rate_plans[r.rate_index].out_n == rp.out_n
        assert table.stretch_plans[r.stretch_plan].ints() == sp.ints() and table.stretch_plans[r.stretch_plan].rate == rp.rate
        assert r.stretched == (not sp.identity)
        if gain is None:
            assert r.level is None
        else:
            assert r.level[1:] == level.check(*gain)
            assert table.level_plans[r.level[0]].ints() == lp.ints() and table.level_plans[r.level[0]].rate == rp.rate
        assert r.drain_frames == -(-pre // sp.n_out) and (r.drain_frames == 0) == (pre == 0)
        assert r.drain_stage == ("stretch" if not sp.identity else "level" if gain else None)
    assert seen == {(r or NATIVE, ok) for r in RATES for ok in (True, False)}  # both outcomes at every rate


def test_rule_refusals_keep_their_messages(table):
    for args, msg in [((12345,), "not configured"), ((None, 0.75), "not configured"), ((None, 3.0), "not configured"),
                      ((None, 0.77), "fraction"), ((None, float("nan")), "finite"), ((None, None, 30), r"\[-40, 24\]"),
                      ((None, None, 6, 1), r"\[-20, 0\]"), ((None, None, None, -3), "together with gain_db"),
                      ((8000, 1.5), r"not admissible at 8000 Hz \(admissible there: \[1.0, 0.5, 0.8, 1.25, 2.0\]\)")]:
        with pytest.raises(ValueError, match=msg):
            table.route(*args)
    for kw, msg in [(dict(sample_rates=[10560]), "whole number of output samples"), (dict(sample_rates=[7000]), "must be in"),
                    (dict(speeds=[0.9]), "no multiple of 9"), (dict(speeds=[3.0]), "must be in"),
                    (dict(sample_rates=[8000, 16000], speeds=[0.9]), "no multiple of 9")]:
        with pytest.raises(ValueError, match=msg):
            ChainTable(NATIVE, FS, **kw)


def test_the_combined_drain_rule(table):
    r = table.route(None, 0.8, 6)
    assert (r.n_out, r.preroll, r.drain_frames, r.drain_stage) == (2400, 2400 + 120, 2, "stretch")
    assert table.route(None, 0.8).drain_frames == 1 and table.route(None, None, 6).drain_frames == 1  # each stage alone
    r = table.route(None, 0.5, 6)
    assert (r.n_out, r.preroll, r.drain_frames, r.drain_stage) == (3840, 3360 + 120, 1, "stretch")
    r = table.route()
    assert (r.preroll, r.drain_frames, r.drain_stage, r.stretched, r.level) == (0, 0, None, False, None)
    assert table.route(16000, 1.0) == table.route(16000) and table.route(16000).drain_stage is None
    r = table.route(8000, None, 6)
    assert (r.preroll, r.drain_frames, r.drain_stage) == (40, 1, "level")


@pytest.mark.parametrize("F", [1, 2, 7])
def test_clipping_conserves_samples(table, F):
    for rate, speed, gain, r in _admitted(table):
        total = F + r.drain_frames
        counter = np.arange(total * r.n_out)  # the row's lines one after the other
        got, pos = [], 0
        for f in range(total):
            lo, hi = r.take(pos, None if f < F else F)  # the frame count is known once the last frame has been queued
            assert 0 <= lo <= hi <= r.n_out
            got.append(counter[pos + lo:pos + hi])
            pos += r.n_out
        got = np.concatenate(got)
        assert np.array_equal(got, np.arange(r.preroll, r.preroll + F * r.n_out)), (rate, speed, gain)
        # known from the start, the frame count changes nothing
        pos = 0
        for f in range(total):
            lo, hi = r.take(pos, F)
            assert np.array_equal(counter[pos + lo:pos + hi], got[:hi - lo])
            got, pos = got[hi - lo:], pos + r.n_out
        assert not got.size
        lo, hi = r.take(pos, F)
        assert lo == hi  # nothing past the end


@pytest.mark.parametrize("lvl", [True, False])
def test_table_identity(lvl):
    """plan order is behaviour: the captured graphs bake plan indices into device tables"""
    t = ChainTable(NATIVE, FS, [8000, 16000, 48000], [0.8, 1.25, 1.5], level=lvl)
    rp = resample.plans([8000, 16000, 48000], NATIVE, FS)
    assert t.rates == [p.rate for p in rp] == [24000, 8000, 16000, 48000]
    for a, b in zip(t.rate_plans, rp):
        assert np.array_equal(a.table, b.table) and (a.up, a.down, a.taps) == (b.up, b.down, b.taps)
    rates = [(p.rate, p.out_n) for p in rp]
    assert t.speeds == stretch.normalise_speeds([0.8, 1.25, 1.5]) == [1.0, 0.8, 1.25, 1.5]
    sp, index = stretch.table(rates, t.speeds)
    assert t.stretch_index == index and [p.ints() for p in t.stretch_plans] == [p.ints() for p in sp]
    assert [(p.rate, p.speed) for p in t.stretch_plans] == [(p.rate, p.speed) for p in sp]
    if not lvl:
        assert t.level_plans is None and t.level_index is None
        with pytest.raises(ValueError, match="no level stage"):
            t.route(None, None, 6)
        return
    lp, lindex = level.table([(rates[r][0], sp[i].n_out) for r, row in enumerate(index) for i in row if i is not None])
    assert t.level_index == lindex and [p.ints() for p in t.level_plans] == [p.ints() for p in lp]
    # without speeds the leveler's lines are the resampler's, without rates the codec's
    assert ChainTable(NATIVE, FS, [8000, 16000, 48000], level=True).level_index == level.table(rates)[1]
    assert ChainTable(NATIVE, FS, level=True).level_index == {(NATIVE, FS): 0}


def test_messages_on_tables_without_the_stage():
    bare = ChainTable(NATIVE, FS)
    assert bare.empty and bare.route() == bare.route(NATIVE, 1.0) == Route(0, NATIVE, None, False, None, FS, 0, 0, None)
    for args, msg in [((16000,), "24000 Hz only"), ((True,), "24000 Hz only"), ((None, 1.25), "1.0 only"),
                      ((None, True), "1.0 only"), ((None, None, 6), "no level stage"),
                      ((None, None, None, -3), "no level stage")]:
        with pytest.raises(ValueError, match=msg):
            bare.route(*args)
    t = ChainTable(NATIVE, FS, [8000], [0.8, 1.5])
    assert not t.empty and t.speeds_of() == {24000: [1.0, 0.8, 1.5], 8000: [1.0, 0.8]}
    for args, msg in [((16000,), "not configured"), ((None, 1.25), "not configured"),
                      ((8000, 1.5), r"not admissible at 8000 Hz \(admissible there: \[1.0, 0.8\]\)"),
                      ((None, None, 6), "no level stage")]:
        with pytest.raises(ValueError, match=msg):
            t.route(*args)
    with pytest.raises(ValueError, match="together with gain_db"):
        ChainTable(NATIVE, FS, level=True).route(None, None, None, -3)


def test_single_request_validation_names_the_rule():
    def one(*a):
        got = ChainTable.for_request(NATIVE, FS, *a)[1]
        return got["sample_rate"], got["speed"], got["gain_db"], got["peak_dbfs"]

    assert one() == (None, None, None, None) and one(24000, 1.0) == (None, None, None, None)
    assert one(16000, 0.8, 6) == (16000, 0.8, 6.0, -1.0) and one(None, 1.25, -3, -6) == (None, 1.25, -3.0, -6.0)
    assert one(48000, None, 0) == (48000, None, 0.0, -1.0)  # 0 is not None: it limits at the ceiling
    for args, msg in [((10560,), "whole number of output samples"), ((None, 0.9), "no multiple of 9"),
                      ((8000, 1.5), "no multiple of 3"), ((None, 0.77), "fraction"), ((None, None, 30), r"\[-40, 24\]"),
                      ((None, None, None, -3), "together with gain_db")]:
        with pytest.raises(ValueError, match=msg):
            one(*args)
    with pytest.raises(TypeError):
        ChainTable.for_request(NATIVE, FS, volume=3)


def test_a_single_request_is_what_a_table_of_exactly_its_stages_routes():
    """every point of the grid: `for_request` refuses it, or the table of its spec routes its canonical form to what the
    rules composed directly give"""
    levels = [{}, dict(gain_db=6), dict(gain_db=6, peak_dbfs=-3), dict(loudness_lufs=-16)]
    grid = list(itertools.product([None, 8000, 16000, 48000], [None, 0.8, 1.25], [None, "5/4", "17/16"],
                                  [None, "telephone", "hp:120"], levels, [None, "mulaw"]))
    admitted = 0
    for rate, speed, ratio, tone, lvl, enc in grid:
        asked = dict(sample_rate=rate, speed=speed, pitch=ratio, tone=tone, encoding=enc, **lvl)
        try:
            spec, request = ChainTable.for_request(NATIVE, FS, **asked)
        except ValueError:
            continue
        admitted += 1
        assert list(request) == ["sample_rate", "speed", "gain_db", "peak_dbfs", "pitch", "loudness_lufs", "encoding", "tone"]
        assert spec == ChainSpec(sample_rates=rate and (rate,), speeds=speed and (speed,), level="gain_db" in lvl or (
            tone is not None and not lvl), pitches=ratio and (float(pitch.fraction(ratio)),), loudness="loudness_lufs" in lvl,
            encodings=enc and encoding.NAMES, tones=tone and (tone_rule.normalise(tone),)), asked
        r = spec.table(NATIVE, FS).route(**request)
        rp, sp, _ = _compose(rate, speed, None)
        pre = sp.preroll
        if ratio is not None:
            pre += pitch.plan(pitch.fraction(ratio), rp.rate, sp.n_out).preroll
        if "loudness_lufs" in lvl:
            pre += loudness.plan(rp.rate, sp.n_out).D
        if lvl or tone is not None:
            pre += level.plan(rp.rate, sp.n_out).LA
        assert (r.rate, r.n_out, r.preroll) == (rp.rate, sp.n_out, pre), asked
        assert (r.encoding, r.toned, r.loud is not None, r.level is not None) == (enc, tone is not None, "loudness_lufs" in lvl,
                                                                                 bool(lvl) or tone is not None), asked
    assert 2 * admitted >= len(grid)  # it cannot pass by refusing everything


@pytest.mark.parametrize("field,asked,msg", [
    ("sample_rate", dict(sample_rate=10560), "whole number of output samples"),
    ("speed", dict(sample_rate=8000, speed=1.5), "no multiple of 3 divides 640"),
    ("pitch", dict(sample_rate=8000, pitch="2/3"), "no multiple of 3"),
    ("tone", dict(sample_rate=8000, tone="bright"), "not admissible at 8000 Hz"),
    ("loudness_lufs", dict(loudness_lufs=-16, peak_dbfs=1.0), r"\[-20, 0\]"),
    ("loudness_lufs", dict(loudness_lufs=-16, gain_db=3.0), "exclude each other"),
    ("gain_db", dict(peak_dbfs=-3), "together with gain_db"),
    ("gain_db", dict(tone="telephone", peak_dbfs=1.0), r"\[-20, 0\]"),
    ("encoding", dict(encoding="mp3"), "not configured")])
def test_a_refusal_names_the_request_field(field, asked, msg):
    with pytest.raises(RequestError, match=msg) as e:
        ChainTable.for_request(NATIVE, FS, **asked)
    assert e.value.field == field and isinstance(e.value, ValueError)


def test_the_first_field_in_chain_order_is_named_and_the_line_is_exposed():
    with pytest.raises(RequestError) as e:
        ChainTable.for_request(NATIVE, FS, speed=0.9, pitch="8/9", gain_db=30)
    assert e.value.field == "speed"
    assert ChainTable.line_of(NATIVE, FS, 8000, 1.25) == (8000, 1.25, (8000, 512))
    assert ChainTable.line_of(NATIVE, FS, NATIVE, 1) == (None, None, (NATIVE, FS))


@pytest.mark.parametrize("asked,tags", [
    ({}, ()),
    (dict(sample_rate=8000), ("rate", 8000)),
    (dict(speed=1.25), ("speed", 1.25)),
    (dict(gain_db=6), ("level",)),
    (dict(gain_db=-3, peak_dbfs=-6), ("level",)),
    (dict(pitch="5/4"), ("pitch", 1.25)),
    (dict(loudness_lufs=-16), ("loud",)),
    (dict(loudness_lufs=-23, peak_dbfs=-3), ("loud",)),
    (dict(encoding="mulaw"), ("enc",)),
    (dict(encoding="pcm_f32le"), ("enc",)),
    (dict(tone="Telephone"), ("level", "tone", "telephone")),
    (dict(tone="telephone", gain_db=6), ("level", "tone", "telephone")),
    (dict(tone="telephone", loudness_lufs=-16), ("loud", "tone", "telephone")),
    (dict(sample_rate=8000, speed=0.8, gain_db=6, pitch="17/16", encoding="alaw", tone="telephone"),
     ("rate", 8000, "speed", 0.8, "level", "pitch", 1.0625, "enc", "tone", "telephone")),
    (dict(sample_rate=8000, speed=0.8, pitch="17/16", loudness_lufs=-16, encoding="alaw", tone="telephone"),
     ("rate", 8000, "speed", 0.8, "pitch", 1.0625, "loud", "enc", "tone", "telephone"))])
def test_the_tags_of_a_spec_tell_cached_contexts_apart(asked, tags):
    """what `TTSModel` appends to a context's four leading key entries: one context serves every gain, ceiling, target and
    encoding; a toned request has "level" with or without a gain of its own, unless the normaliser brings the limiter"""
    spec, _ = ChainTable.for_request(NATIVE, FS, **asked)
    assert spec.tags() == tags and hash(spec) == hash(ChainTable.for_request(NATIVE, FS, **asked)[0])
    assert ChainSpec(sample_rates=[8000, 16000], encodings=["mulaw"], loudness=True).tags() == ("rate", 8000, 16000, "loud", "enc")
    with pytest.raises(TypeError):
        ChainSpec(volume=True)
