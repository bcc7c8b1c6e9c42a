"""The output chain as one object: what a pipeline's stages are (`ChainTable`), what a request's row does in them (`Route`),
and the stage objects and buffers on the device (`OutputChain`).

The order, which is also the launch order behind the codec's last kernel:

    codec -> resampler -> stretcher -> pitcher -> toner -> normaliser -> leveler -> encoder

A pipeline has any subset of the seven stages; the toner and the normaliser bring the leveler with them.  The buffer rule: the
first stage present reads the frame's PCM; between two consecutive stages present there is one f32 device buffer [batch, input
width of the later one], which must be the output width of the earlier one; the last stage writes the pinned ring.

The first half is pure Python over the rule modules `resample.py`, `stretch.py`, `pitch.py`, `tone.py`, `loudness.py` and
`level.py`: it needs no library, no GPU and no device memory.  Everything a caller has to know about a row - its plan indices, how many samples a frame
yields, how many leading samples to drop, how many drain frames flush its tail and which stage's drain flag to raise - is a
`Route`; nothing outside this module composes the six plan rules.

The drain rule: a row's pre-roll is the SUM of its stages' pre-rolls (the stretcher's and the pitcher's, 0 on an identity plan,
plus the normaliser's delay and the leveler's look-ahead, each 0 on bypass), it delivers the samples [preroll, preroll + frames * n_out) of its line and needs
ceil(preroll / n_out) further frames, which it reads as zeros, to get there - a count of the sum, not of any one stage.  The
zeros enter at the first lagging stage: through the stretcher's flag where the row is stretched (what the stretcher emits
past its tail is zero, which is what the stages behind it then read), else through the pitcher's where the row is pitched,
else through the normaliser's where the row has a loudness target, else through the leveler's.

The toner (`tone.py`) sits between the pitcher and the normaliser.  It has state but no lag and no drain flag: it adds nothing
to a row's pre-roll, the zeros of a draining row ring out through it, and `drain_stage` never names it.  A toned row always
runs the limiter behind it, because a boost creates peaks; so its pre-roll is what the stages behind the tone add.

The encoder (`encoding.py`) is the last stage where a table has one.  It has no state and no lag: it adds nothing to a row's
pre-roll, and the zeros of a draining row reach it like any other sample.  Everything above counts samples; only the ring the
encoder writes is in bytes, `bytes_per_sample` of the row's encoding to a sample.
"""

from __future__ import annotations

import numbers
from dataclasses import dataclass

from . import encoding as encoding_rule
from . import level as level_rule
from . import loudness as loud_rule
from . import pitch as pitch_rule
from . import resample, stretch
from . import tone as tone_rule


def rate_index(rates, rate) -> int:
    """index of `rate` in `rates` (None: 0, the native rate); ValueError for a rate that is not configured"""
    if rate is None:
        return 0
    if isinstance(rate, bool) or not isinstance(rate, numbers.Integral) or int(rate) not in rates:
        raise ValueError(f"sample rate {rate!r} is not configured (this resampler has {rates})")
    return rates.index(int(rate))


@dataclass(frozen=True)
class Route:
    """One row's way through the chain.  `rate_index`, `rate`: the row's output rate; `stretch_plan`: its plan index in
    the stretcher (None without one), `stretched`: that plan is no identity plan; `level`: (plan index in the leveler,
    gain_db, peak_dbfs), None for bypass; `n_out`: samples its frame yields at the end of the chain; `preroll`, `drain_frames`,
    `drain_stage` ("stretch", "pitch", "loud", "level" or None): the drain rule of the module's docstring; `pitch_plan`: its
    plan index in the pitcher (None without one), `pitched`: that plan is no identity plan; `loud`: (plan index in the
    normaliser, loudness_lufs), None for bypass; `encoding`: the name of the row's output encoding, None on a table without
    the encoder, and `bytes_per_sample`: what a sample of it takes in the encoder's ring (None likewise: the ring's dtype
    says); `tone_plan`: its plan index in the toner (None: bypass, or no toner), `toned`: it has one."""

    rate_index: int
    rate: int
    stretch_plan: int | None
    stretched: bool
    level: tuple | None
    n_out: int
    preroll: int
    drain_frames: int
    drain_stage: str | None
    pitch_plan: int | None = None
    pitched: bool = False
    loud: tuple | None = None
    encoding: str | None = None
    bytes_per_sample: int | None = None
    tone_plan: int | None = None
    toned: bool = False

    def take(self, pos: int, frames: int | None):
        """(lo, hi): the part of the row's line that belongs to its job, which has produced `pos` samples so far (lines are
        read in order, `n_out` each) and consists of `frames` frames (None: not known yet) - everything behind the
        pre-roll, up to frames * n_out samples in all"""
        lo = min(max(self.preroll - pos, 0), self.n_out)
        hi = self.n_out if frames is None else min(self.n_out, self.preroll + frames * self.n_out - pos)
        return lo, max(hi, lo)


class ChainTable:
    """The plans of a pipeline's stages, built once: `rate_plans` (`resample.plans`: the native rate first), and with
    `speeds` the stretcher's `stretch_plans` / `stretch_index[rate index][speed index]` (`stretch.table`), with `level`
    the leveler's `level_plans` / `level_index[(rate, n)]` (`level.table` over every (rate, samples per frame) the rates x
    speeds can produce), with `pitches` the pitcher's `pitch_plans` / `pitch_index[(rate, n)][pitch index]` (`pitch.table`
    over the same lines; the pitcher keeps a line's length, so the leveler's lines are unchanged), with `loudness` the
    normaliser's `loud_plans` / `loud_index[(rate, n)]` (`loudness.table` over the lines the leveler gets; the leveler's
    plans are then built whatever `level` says, because the normaliser is always followed by the limiter).  The graphs bake plan indices into device tables, so the order is part of the contract.  A rate,
    speed, pitch or line the rules refuse raises their ValueError here, before anything is allocated.  `sample_rates` /
    `speeds` / `pitches` None and `level` / `loudness` False: that stage does not exist (`has_rates` tells a resampler of the native rate alone from none).
    With `encodings` (a list of names of `encoding.py`) the chain ends with the encoder and `encodings` is the configured
    list, `pcm_s16le` first; None: that stage does not exist.  A list makes the table non-empty even when the encoder is the
    only stage.  `width` is the widest line that leaves the last stage before the encoder.  With `tones` (a list of tones of
    `tone.py`) the toner's `tone_plans` / `tone_index[(rate, n)][tone index]` (`tone.table` over the lines the pitcher leaves,
    None where the rate refuses a tone) and `tones`, the configured list in canonical form; the leveler's plans are then built
    whatever `level` says, because a toned row is always followed by the limiter.  None: that stage does not exist."""

    def __init__(self, native_rate: int, frame_samples: int, sample_rates=None, speeds=None, level: bool = False,
                 pitches=None, loudness: bool = False, encodings=None, tones=None):
        self.native_rate, self.frame_samples = int(native_rate), int(frame_samples)
        self.has_rates = sample_rates is not None
        self.sample_rates = list(sample_rates) if self.has_rates else None
        self.speeds = None if speeds is None else stretch.normalise_speeds(speeds)
        self.pitches = None if pitches is None else pitch_rule.normalise_pitches(pitches)
        self.rate_plans = resample.plans(self.sample_rates or (), self.native_rate, self.frame_samples)
        self.rates = [p.rate for p in self.rate_plans]
        lines = [(p.rate, p.out_n) for p in self.rate_plans]
        self.stretch_plans = self.stretch_index = self.level_plans = self.level_index = None
        self.pitch_plans = self.pitch_index = None
        if self.speeds is not None:
            self.stretch_plans, self.stretch_index = stretch.table(lines, self.speeds)
            lines = [(self.rates[r], self.stretch_plans[i].n_out) for r, row in enumerate(self.stretch_index)
                     for i in row if i is not None]
        if self.pitches is not None:
            self.pitch_plans, self.pitch_index = pitch_rule.table(lines, self.pitches)
        self.tones = None if tones is None else tone_rule.normalise_tones(tones)
        self.tone_plans = self.tone_index = None
        if self.tones is not None:
            if not self.tones:
                raise ValueError("tones: the list holds no tone but the bypass, which every request has anyway")
            self.tone_plans, self.tone_index = tone_rule.table(lines, self.tones)
        self.loud_plans = self.loud_index = None
        if loudness:
            self.loud_plans, self.loud_index = loud_rule.table(lines)
        if level or loudness or self.tones is not None:
            self.level_plans, self.level_index = level_rule.table(lines)
        self.encodings = None if encodings is None else encoding_rule.normalise_encodings(encodings)
        self.width = max(n for _, n in lines)

    @property
    def empty(self) -> bool:
        return (not self.has_rates and self.speeds is None and self.pitches is None and self.level_plans is None
                and self.encodings is None)

    def speeds_of(self) -> dict:
        """{rate: [the configured speeds admissible at that rate, 1.0 first]}"""
        return {rate: [s for j, s in enumerate(self.speeds) if self.stretch_index[r][j] is not None]
                for r, rate in enumerate(self.rates)}

    def pitches_of(self, rate: int, n: int) -> list:
        """the configured pitches admissible on frames of `n` samples at `rate` Hz, 1.0 first"""
        return [p for j, p in enumerate(self.pitches) if self.pitch_index[(rate, n)][j] is not None]

    def tones_of(self, rate: int, n: int) -> list:
        """the configured tones admissible on frames of `n` samples at `rate` Hz"""
        return [t for j, t in enumerate(self.tones) if self.tone_index[(rate, n)][j] is not None]

    def route(self, sample_rate=None, speed=None, gain_db=None, peak_dbfs=None, pitch=None, loudness_lufs=None,
              encoding=None, tone=None) -> Route:
        """The `Route` of a request; None is the native rate, speed 1.0, no gain, pitch 1.0, no loudness target and, on a
        table with the encoder, `pcm_s16le` (an encoding that is not configured, or any on a table without the encoder,
        raises ValueError).  A request
        with a target gets the normaliser's plan and a leveler entry at gain 0 dB under its `peak_dbfs` (default -1).
        ValueError for a rate, speed or pitch that is not configured, a speed or pitch the plan rule refuses on the
        request's line (the message lists those it admits), a level `level.check` or a target `loudness.check` refuses,
        `loudness_lufs` together with `gain_db`, and for any of them on a table without that stage.  `tone` (None, "" or
        "flat": bypass) must be one of the configured tones (compared in canonical form) that the row's rate admits; a toned
        request gets a leveler entry at gain 0 dB under its `peak_dbfs` (default -1) unless it has a gain or a loudness
        target, with both of which it combines freely."""
        r = 0
        if self.has_rates:
            r = rate_index(self.rates, sample_rate)
        elif sample_rate is not None and (isinstance(sample_rate, bool) or sample_rate != self.native_rate):
            raise ValueError(f"sample rate {sample_rate!r}: this batcher writes {self.native_rate} Hz only (build it "
                             "with sample_rates for per-request rates)")
        rate, n_out, plan, preroll = self.rates[r], self.rate_plans[r].out_n, None, 0
        if self.speeds is not None:
            f = 1.0 if speed is None else float(stretch.fraction(speed))
            if f not in self.speeds:
                raise ValueError(f"speed {speed!r} is not configured (this pipeline has {self.speeds})")
            plan = self.stretch_index[r][self.speeds.index(f)]
            if plan is None:
                raise ValueError(f"speed {speed!r} is not admissible at {rate} Hz (admissible there: {self.speeds_of()[rate]})")
            n_out, preroll = self.stretch_plans[plan].n_out, self.stretch_plans[plan].preroll
        elif speed is not None and (isinstance(speed, bool) or not isinstance(speed, numbers.Real) or speed != 1.0):
            raise ValueError(f"speed {speed!r}: this batcher speaks at 1.0 only (build it with speeds for per-request speeds)")
        stretched = plan is not None and not self.stretch_plans[plan].identity
        pplan, pitched = None, False
        if self.pitches is not None:
            f = 1.0 if pitch is None else float(pitch_rule.fraction(pitch))
            if f not in self.pitches:
                raise ValueError(f"pitch {pitch!r} is not configured (this pipeline has {self.pitches})")
            pplan = self.pitch_index[(rate, n_out)][self.pitches.index(f)]
            if pplan is None:
                raise ValueError(f"pitch {pitch!r} is not admissible on frames of {n_out} samples at {rate} Hz (admissible "
                                 f"there: {self.pitches_of(rate, n_out)})")
            pitched = not self.pitch_plans[pplan].identity
            preroll += self.pitch_plans[pplan].preroll
        elif pitch is not None and float(pitch_rule.fraction(pitch)) != 1.0:
            raise ValueError(f"pitch {pitch!r}: this batcher speaks at pitch 1.0 only (build it with pitches for per-request "
                             "pitches)")
        tplan, canon = None, tone_rule.normalise(tone)
        if self.tones is not None:
            if canon is not None:
                if canon not in self.tones:
                    raise ValueError(f"tone {tone!r} is not configured (this pipeline has {self.tones})")
                tplan = self.tone_index[(rate, n_out)][self.tones.index(canon)]
                if tplan is None:
                    raise ValueError(f"tone {tone!r} is not admissible at {rate} Hz (admissible there: "
                                     f"{self.tones_of(rate, n_out)})")
                if gain_db is None and loudness_lufs is None:
                    gain_db = 0.0  # the limiter behind the tone
        elif canon is not None:
            raise ValueError(f"tone {tone!r}: this batcher has no tone stage (build it with tones for per-request tones)")
        lvl = loud = None
        if self.loud_plans is not None:
            target = loud_rule.check_with(loudness_lufs, gain_db)
            if target is not None:
                loud = (self.loud_index[(rate, n_out)], target)
                preroll += self.loud_plans[loud[0]].D
                gain_db = 0.0  # the limiter behind the normaliser
        elif loudness_lufs is not None:
            raise ValueError("loudness_lufs: this batcher has no loudness stage (build it with loudness=True)")
        if self.level_plans is not None:
            g_db, p_db = level_rule.check(gain_db, peak_dbfs)
            if g_db is not None:
                lvl = (self.level_index[(rate, n_out)], g_db, p_db)
                preroll += self.level_plans[lvl[0]].LA
        elif gain_db is not None or peak_dbfs is not None:
            raise ValueError("gain_db / peak_dbfs: this batcher has no level stage (build it with level=True)")
        bps = None
        if self.encodings is not None:
            encoding = encoding_rule.check(encoding, self.encodings)
            bps = encoding_rule.BYTES_PER_SAMPLE[encoding]
        elif encoding is not None:
            raise ValueError(f"encoding {encoding!r}: this batcher writes one sample format for all (build it with encodings "
                             "for per-request encodings)")
        return Route(r, rate, plan, stretched, lvl, n_out, preroll, -(-preroll // n_out),
                     "stretch" if stretched else "pitch" if pitched else "loud" if loud is not None
                     else "level" if lvl is not None else None, pplan, pitched, loud, encoding, bps, tplan, tplan is not None)

    @staticmethod
    def single(native_rate: int, frame_samples: int, sample_rate=None, speed=None, gain_db=None, peak_dbfs=None):
        """One request that gets a chain of its own: (sample_rate, speed, gain_db, peak_dbfs) with the native rate, speed
        1.0 and no gain as None, the speed as the float of its fraction and peak_dbfs defaulted - what a `ChainTable` of
        exactly these stages is built from and routes.  ValueError with the message of the rule that refuses."""
        native = int(native_rate)
        n = int(frame_samples)
        if sample_rate is not None:
            p = resample.plan(sample_rate, native, frame_samples)
            sample_rate, n = (None if p.rate == native else p.rate), p.out_n
        if speed is not None:
            speed = float(stretch.fraction(speed))
            if speed == 1.0:
                speed = None
            else:
                n = stretch.plan(speed, sample_rate or native, n).n_out
        gain_db, peak_dbfs = level_rule.check(gain_db, peak_dbfs)
        if gain_db is not None:
            level_rule.plan(sample_rate or native, n)
        return sample_rate, speed, gain_db, peak_dbfs

    @staticmethod
    def single_line(native_rate: int, frame_samples: int, sample_rate=None, speed=None):
        """(rate, n): the line that leaves the stretcher of one request's own chain - what its pitcher reads"""
        sample_rate, speed, _, _ = ChainTable.single(native_rate, frame_samples, sample_rate, speed)
        rate, n = sample_rate or int(native_rate), int(frame_samples)
        if sample_rate is not None:
            n = resample.plan(sample_rate, int(native_rate), frame_samples).out_n
        if speed is not None:
            n = stretch.plan(speed, rate, n).n_out
        return rate, n

    @staticmethod
    def single_pitch(native_rate: int, frame_samples: int, sample_rate=None, speed=None, pitch=None):
        """The pitch of one request that gets a chain of its own, behind that request's rate and speed: the float of its
        fraction, None for 1.0.  ValueError with the message of the rule that refuses."""
        if pitch is None:
            return None
        f = pitch_rule.fraction(pitch)
        if f == 1:
            return None
        return pitch_rule.plan(f, *ChainTable.single_line(native_rate, frame_samples, sample_rate, speed)).pitch

    @staticmethod
    def single_tone(native_rate: int, frame_samples: int, sample_rate=None, speed=None, tone=None):
        """The tone of one request that gets a chain of its own, behind that request's rate and speed (the pitcher keeps the
        line): its canonical string, None for the bypass.  ValueError with the message of the rule that refuses."""
        canon = tone_rule.normalise(tone)
        if canon is None:
            return None
        rate, n = ChainTable.single_line(native_rate, frame_samples, sample_rate, speed)
        tone_rule.plan(rate, n, canon)
        level_rule.plan(rate, n)
        return canon

    @staticmethod
    def single_loudness(native_rate: int, frame_samples: int, sample_rate=None, speed=None, gain_db=None, peak_dbfs=None,
                        loudness_lufs=None):
        """The loudness target of one request that gets a chain of its own, behind that request's rate and speed (the
        pitcher keeps the line): (loudness_lufs as a float, peak_dbfs defaulted), (None, None) without a target.
        ValueError with the message of the rule that refuses."""
        target = loud_rule.check_with(loudness_lufs, gain_db)
        if target is None:
            return None, None
        rate, n = ChainTable.single_line(native_rate, frame_samples, sample_rate, speed)
        loud_rule.plan(rate, n)
        level_rule.plan(rate, n)
        return target, level_rule.check(0.0, peak_dbfs)[1]


class OutputChain:
    """The stages of `table` for `batch` rows on `engine`'s device: `rs` / `ts` / `ps` / `tn` / `ln` / `lv` / `en`
    (`engine.Resampler`, `Stretcher`, `Pitcher`, `Toner`, `Normalizer`, `Leveler`, `Encoder`; None where the table has no
    such stage), the device buffers between them and the pinned ring `out` of `nb` tensors, which the last stage writes.
    The buffer rule of the module's docstring gives them: without the encoder a ring slot is [batch, widest line], int16
    with `pcm_i16`, else float32; on a table with `encodings` it is uint8 [batch, encoding.pitch(widest line)], row b's
    n_out * bytes_per_sample bytes at the start of its row, and `pcm_i16` must be left False (ValueError).  An empty table
    creates nothing: `out` is None and the codec writes its PCM as without a chain."""

    def __init__(self, engine, batch: int, table: ChainTable, nb: int, pcm_i16: bool = False):
        import torch

        from .engine import Encoder, Leveler, Normalizer, Pitcher, Resampler, Stretcher, Toner

        if table.encodings is not None and pcm_i16:
            raise ValueError("pcm_i16 and encodings exclude each other: with encodings a row asks for pcm_s16le itself")
        self.table = table
        self.rs = Resampler(engine, batch, table.sample_rates, table.rate_plans) if table.has_rates else None
        self.ts = Stretcher(engine, batch, table.stretch_plans) if table.speeds is not None else None
        self.ps = Pitcher(engine, batch, table.pitch_plans) if table.pitches is not None else None
        self.tn = Toner(engine, batch, table.tone_plans, table.width) if table.tone_plans is not None else None
        self.ln = Normalizer(engine, batch, table.loud_plans) if table.loud_plans is not None else None
        self.lv = Leveler(engine, batch, table.level_plans) if table.level_plans is not None else None
        self.en = Encoder(engine, batch, table.width) if table.encodings is not None else None
        self._stages = [s for s in self.per_kind() if s is not None]
        self._between = []  # one device buffer between two stages serves every ring slot: the codec graphs run one after the other
        self.out = None
        if not self._stages:
            return
        for before, s in zip(self._stages, self._stages[1:]):
            if before._out_width != s._in_width:
                raise ValueError(f"{s._field}: the {s._name}'s line is not the line of the stage before it")
            self._between.append(torch.zeros(batch, s._in_width, device=engine.device))
        if self.en is not None:
            shape, dtype = (batch, self.en.pitch), torch.uint8
        else:
            shape, dtype = (batch, self._stages[-1]._out_width), torch.int16 if pcm_i16 else torch.float32
        self.out = [torch.zeros(*shape, dtype=dtype).pin_memory() for _ in range(nb)]

    def per_kind(self):
        """(rs, ts, ps, tn, ln, lv, en) in chain order, None where the table has no such stage"""
        return self.rs, self.ts, self.ps, self.tn, self.ln, self.lv, self.en

    def stages(self):
        return list(self._stages)

    def attach(self, mimi_state, p: int):
        """the decodes / graph captures of `mimi_state` issued after this call end with the chain's launches and write
        ring slot `p` (the frame's PCM must then be a device tensor)"""
        bufs = [None, *self._between, self.out[p]]  # stage i reads bufs[i] (None: the frame's PCM) and writes bufs[i + 1]
        for i, s in enumerate(self._stages):
            mimi_state._set_stage(type(s), s, bufs[i + 1], bufs[i])

    def detach(self, mimi_state):
        for s in reversed(self._stages):
            mimi_state._set_stage(type(s), None)

    def reset(self, stream=None):
        """every row's state back to zero in every stage (new utterances); the rows keep their routes"""
        for s in self._stages:
            s.reset(stream)

    def set_row(self, row: int, route: Route, stream=None):
        """a new sequence joins `row` on `route` with a zero state in every stage, not draining; a stage the route does not
        use runs its identity plan or bypass.  Stream-ordered"""
        for s in self._stages:
            s.set_row(row, *s._route_args(route), stream)

    def drain_row(self, row: int, route: Route, stream=None):
        """from now on (stream-ordered) the row's incoming frames count as zeros at the stage `route.drain_stage` names"""
        for s in self._stages:
            if s._drain_name is not None and s._drain_name == route.drain_stage:
                s.set_row_drain(row, True, stream)

    def close(self):
        for s in reversed(self._stages):
            s.close()
