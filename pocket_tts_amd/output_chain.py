"""The output chain as one object: the options a pipeline is built with (`ChainSpec`), what its stages are (`ChainTable`),
what a request's row does in them (`Route`, and `ChainTable.for_request` for a request that gets a pipeline of its own), and
the stage objects and buffers on the device (`OutputChain`).

The order, which is also the launch order behind the codec's last kernel:

    codec -> resampler -> stretcher -> pitcher -> toner -> compressor -> normaliser -> leveler -> encoder -> packer

A pipeline has any subset of the nine stages; the toner, the compressor and the normaliser bring the leveler with them, the
packer the encoder.  The buffer rule: the first stage present reads the frame's PCM; between two consecutive stages present there is one
device buffer [batch, input width of the later one], which must be the output width of the earlier one, f32 but for the
encoder's bytes before the packer, which are uint8 [batch, encoding.pitch(width)]; the last stage writes the pinned ring.

The first half is pure Python over the rule modules `resample.py`, `stretch.py`, `pitch.py`, `tone.py`, `dynamics.py`,
`loudness.py` and `level.py`: it needs no library, no GPU and no device memory.  Everything a caller has to know about a row - its plan indices, how many samples a frame
yields, how many leading samples to drop, how many drain frames flush its tail and which stage's drain flag to raise - is a
`Route`; nothing outside this module composes the seven plan rules.

The drain rule: a row's pre-roll is the SUM of its stages' pre-rolls (the stretcher's and the pitcher's, 0 on an identity plan,
plus the normaliser's delay and the leveler's look-ahead, each 0 on bypass), it delivers the samples [preroll, preroll + frames * n_out) of its line and needs
ceil(preroll / n_out) further frames, which it reads as zeros, to get there - a count of the sum, not of any one stage.  The
zeros enter at the first lagging stage: through the stretcher's flag where the row is stretched (what the stretcher emits
past its tail is zero, which is what the stages behind it then read), else through the pitcher's where the row is pitched,
else through the normaliser's where the row has a loudness target, else through the leveler's.

The toner (`tone.py`) sits between the pitcher and the normaliser.  It has state but no lag and no drain flag: it adds nothing
to a row's pre-roll, the zeros of a draining row ring out through it, and `drain_stage` never names it.  A toned row always
runs the limiter behind it, because a boost creates peaks; so its pre-roll is what the stages behind the tone add.

The compressor (`dynamics.py`) sits between the toner and the normaliser, so that the loudness is measured on what the
listener hears.  Like the toner it has state but no lag and no drain flag, adds nothing to a row's pre-roll, and a row with
a setting always runs the limiter behind it, which catches what the make-up gain and the attack time let through.

The encoder (`encoding.py`) is the last stage where a table has one.  It has no state and no lag: it adds nothing to a row's
pre-roll, and the zeros of a draining row reach it like any other sample.  Everything above counts samples; only the ring the
encoder writes is in bytes, `bytes_per_sample` of the row's encoding to a sample.

The packer (`flac.py`) is the last stage where a table has one: it turns the encoder's bytes into ring lines with a 16-byte
prefix that says how many bytes follow, a row's encoded bytes as they are or, for a row whose `compression` is "flac", one
FLAC frame per line.  A compressed frame cannot be sliced on the host, so a flac row's pre-roll is cut on the device: its
first `drain_frames` lines carry nothing and every later line carries one whole block of the samples behind the pre-roll.
"""

from __future__ import annotations

import numbers
from dataclasses import dataclass

from . import encoding as encoding_rule
from . import flac as flac_rule
from . import dynamics as dyn_rule
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
    says); `tone_plan`: its plan index in the toner (None: bypass, or no toner), `toned`: it has one;
    `compression`: None or "flac", the row's lines leave the packer as FLAC frames; `dyn_plan`: its plan index in the
    compressor (None: bypass, or no compressor), `dynamic`: it has one; `true_peak`: the ceiling in `level` is a true peak
    (dBTP), the leveler runs the row in true-peak mode, whose 10 samples of detector delay `preroll` includes."""

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
    compression: str | None = None
    dyn_plan: int | None = None
    dynamic: bool = False
    true_peak: bool = False

    def take(self, pos: int, frames: int | None):
        """(lo, hi): the part of the row's line that belongs to its job, which has produced `pos` samples so far (lines are
        read in order, `n_out` each) and consists of `frames` frames (None: not known yet) - everything behind the
        pre-roll, up to frames * n_out samples in all"""
        lo = min(max(self.preroll - pos, 0), self.n_out)
        hi = self.n_out if frames is None else min(self.n_out, self.preroll + frames * self.n_out - pos)
        return lo, max(hi, lo)


class RequestError(ValueError):
    """A rule's refusal of one request field: `field` names it, the message is the rule's own."""

    def __init__(self, field: str, message: str):
        super().__init__(message)
        self.field = field


def _ask(field: str, rule, *args):
    """rule(*args); its ValueError as the `RequestError` of `field`"""
    try:
        return rule(*args)
    except ValueError as e:
        raise RequestError(field, str(e)) from None


@dataclass(frozen=True)
class ChainSpec:
    """What a pipeline's output chain is built with: the ten options that `StepPipeline`, `ContinuousBatcher` and
    `server.create_app` take as keywords, one per stage but the leveler's, which five bring.  The default of each is "that
    stage does not exist": with all ten nothing changes, same buffers, same graph nodes.  Lists are kept as tuples, so a
    spec is hashable.

    `sample_rates`: the output rates a row may choose besides the native one, each a rate `resample.plan` admits, e.g. [8000,
    16000, 48000]; the streaming polyphase resampler (`resample.py`) is the first stage and a frame then holds
    frame_samples * rate / native samples.
    `speeds`: the speaking rates a row may choose besides 1.0, e.g. [0.8, 1.25, 1.5]; each must be one `stretch.plan` admits
    at one of the rates at least.  The streaming WSOLA time-stretch (`stretch.py`) at constant pitch; a frame then holds
    n_out = samples / speed samples.
    `level`: True lets a row choose its output level, a gain and a look-ahead peak limiter (`level.py`).
    `pitches`: the frequency ratios a row may choose besides 1, numbers or "P/Q" strings, e.g. ["17/16", "5/4", "4/5"]; each
    must be one `pitch.plan` admits on one of the lines at least.  The pitch shifter (`pitch.py`) keeps a line's length.
    `loudness`: True lets a row choose a loudness target, a streaming BS.1770 normaliser (`loudness.py`); it brings the
    leveler with it as its peak limiter.
    `encodings`: the sample encodings a row may choose besides "pcm_s16le", names of `encoding.py`, e.g. ["mulaw", "alaw",
    "pcm_f32le"]; the encoder ends the chain and writes bytes.  Not together with a 16-bit ring (`pcm_i16`, `pcm_format`).
    `tones`: the tones a row may choose, presets or band lists of `tone.py`, e.g. ["telephone", "hp:120;peak:3000:4"]; the
    parametric equaliser, which brings the leveler with it as its peak limiter.
    `compressions`: the compressions a row may choose, names of `flac.py`, i.e. ["flac"]; the packer ends the chain behind
    the encoder, which it brings with it, and writes ring lines with a length prefix.
    `dynamics`: the compressor settings a row may choose, presets or key=value lists of `dynamics.py`, e.g. ["speech",
    "threshold=-24;ratio=4"]; the speech compressor, which brings the leveler with it as its peak limiter.
    `true_peak`: True lets a row state its ceiling as a true peak, `peak_dbtp` (`level.py`, "True-peak mode"); it brings the
    leveler with it, like `level`, with the mode's carries and meters.  Rows that do not use it compute what they compute
    without the option, bit for bit.

    What the rules refuse raises their ValueError when the table is built (`table`), before anything is allocated."""

    sample_rates: tuple | None = None
    speeds: tuple | None = None
    level: bool = False
    pitches: tuple | None = None
    loudness: bool = False
    encodings: tuple | None = None
    tones: tuple | None = None
    compressions: tuple | None = None
    dynamics: tuple | None = None
    true_peak: bool = False

    TAGS = dict(sample_rates="rate", speeds="speed", level="level", true_peak="tp", pitches="pitch", loudness="loud",
                encodings="enc", tones="tone", dynamics="dyn", compressions="comp")  # what `tags` calls each option

    def __post_init__(self):
        for name in ("sample_rates", "speeds", "pitches", "encodings", "tones", "compressions", "dynamics"):
            v = getattr(self, name)
            if v is not None and not isinstance(v, (tuple, str)):  # a string is no list: the rules say so
                object.__setattr__(self, name, tuple(v))

    @classmethod
    def of(cls, spec=None, **chain):
        """`spec`, or the spec of the ten options given as keywords; TypeError for another keyword, or for both"""
        if spec is None:
            return cls(**chain)
        if chain:
            raise TypeError(f"a ChainSpec and the options {sorted(chain)} exclude each other")
        return spec

    def table(self, native_rate: int, frame_samples: int) -> "ChainTable":
        return ChainTable(native_rate, frame_samples, **vars(self))

    def tags(self) -> tuple:
        """The stages of the spec as the words that tell cached contexts apart: each option that is set as its tag in
        `TAGS`, a list other than the encoder's and the packer's followed by its values.  ("rate", 8000, "level", "enc") is a resampler to 8
        kHz, the leveler and the encoder: a context serves every gain, ceiling and target and all encodings, but one list
        of rates, speeds, pitches, tones and compressor settings."""
        out = []
        for name, tag in self.TAGS.items():
            v = getattr(self, name)
            if v is not None and v is not False:
                out += [tag, *(v if isinstance(v, tuple) and name not in ("encodings", "compressions") else ())]
        return tuple(out)


class ChainTable:
    """The plans of a pipeline's stages, built once from the options of a `ChainSpec`: `rate_plans` (`resample.plans`: the
    native rate first; `has_rates` tells a resampler of the native rate alone from none), and with `speeds` the stretcher's
    `stretch_plans` / `stretch_index[rate index][speed index]` (`stretch.table`), with `pitches` the pitcher's `pitch_plans`
    / `pitch_index[(rate, n)][pitch index]` (`pitch.table` over every (rate, samples per frame) the rates x speeds can
    produce), with `tones` the toner's `tone_plans` / `tone_index[(rate, n)][tone index]` (`tone.table` over the same lines,
    None where the rate refuses a tone) and `tones`, the configured list in canonical form, with `loudness` the normaliser's
    `loud_plans` / `loud_index[(rate, n)]` (`loudness.table`), with `dynamics` the compressor's `dyn_plans` /
    `dyn_index[(rate, n)][setting index]` (`dynamics.table` over the same lines) and `dynamics`, the configured list in
    canonical form, and with `level`, `loudness`, `tones`, `dynamics` or `true_peak` the leveler's
    `level_plans` / `level_index[(rate, n)]` (`level.table`); `true_peak` says whether it has the true-peak mode.  With `encodings` the chain ends with the encoder and
    `encodings` is the configured list, `pcm_s16le` first; a list makes the table non-empty even when the encoder is the only
    stage.  With `compressions` it ends with the packer behind the encoder (which the option brings: `encodings` is then at
    least ["pcm_s16le"]) and `compressions` is the configured list.  `width` is the widest line that leaves the last stage
    before the encoder.  The graphs bake plan indices into
    device tables, so the order is part of the contract."""

    def __init__(self, native_rate: int, frame_samples: int, sample_rates=None, speeds=None, level: bool = False,
                 pitches=None, loudness: bool = False, encodings=None, tones=None, compressions=None, dynamics=None,
                 true_peak: bool = False):
        self.true_peak = bool(true_peak)
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
        self.dynamics = None if dynamics is None else dyn_rule.normalise_dynamics(dynamics)
        self.dyn_plans = self.dyn_index = None
        if self.dynamics is not None:
            self.dyn_plans, self.dyn_index = dyn_rule.table(lines, self.dynamics)
        self.loud_plans = self.loud_index = None
        if loudness:
            self.loud_plans, self.loud_index = loud_rule.table(lines)
        if level or loudness or self.tones is not None or self.dynamics is not None or self.true_peak:
            self.level_plans, self.level_index = level_rule.table(lines)
        self.compressions = None if compressions is None else flac_rule.normalise_compressions(compressions)
        if self.compressions is not None:
            if not self.compressions:
                raise ValueError("compressions: the list holds no compression")
            if encodings is None:
                encodings = ()  # the packer brings the encoder
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

    def dynamics_of(self, rate: int, n: int) -> list:
        """the configured compressor settings admissible on frames of `n` samples at `rate` Hz"""
        return [s for j, s in enumerate(self.dynamics) if self.dyn_index[(rate, n)][j] is not None]

    def route(self, sample_rate=None, speed=None, gain_db=None, peak_dbfs=None, pitch=None, loudness_lufs=None,
              encoding=None, tone=None, compression=None, dynamics=None, peak_dbtp=None) -> Route:
        """The `Route` of a request.  Its eleven fields, which `ContinuousBatcher.submit`, `TTSModel.generate_audio` and
        `generate_audio_stream` take as keywords and hand on as they came; None is always "as without the stage":

        `sample_rate`: the rate of the request's audio, the native one (None) or one of the configured; a frame then yields
        frame_samples * rate / native samples.
        `speed`: its speaking rate at constant pitch, 1.0 (None) or one of the configured that the plan rule admits at its
        rate; a frame then yields n_out = samples / speed samples, and F frames exactly F * n_out.
        `pitch`: a frequency ratio P / Q with P, Q <= 20 in [0.5, 2], a number or a "P/Q" string such as "17/16" for a
        semitone up, 1 (None) or one of the configured that the plan rule admits on the line behind its rate and speed.
        Every frequency moves by it, the formants too.
        `tone`: a preset such as "telephone", "warm", "bright", "presence", "small_speaker" or "deess", or a band list such as
        "hp:120;peak:3000:4" (at most eight biquad sections, none above 0.45 x the rate), compared in the canonical form of
        `tone.normalise`; None, "" or "flat": bypass.  A toned request runs the limiter behind it, at gain 0 dB under its
        `peak_dbfs` unless it has a gain or a target, with both of which it combines freely.
        `dynamics`: a compressor preset, "speech", "gentle", "broadcast" or "telephone", or a key=value list such as
        "threshold=-24;ratio=4" (keys threshold, ratio, knee, attack, release, makeup; what is left out is that of `speech`),
        compared in the canonical form of `dynamics.normalise`; None, "" or "off": bypass.  The compressor sits behind the
        tone and in front of the loudness measurement; such a request runs the limiter behind it, like a toned one.
        `loudness_lufs`: a loudness target in [-40, -10], e.g. -16 or -23.  The gain follows the running gated BS.1770
        loudness of the text chunk so far, clamped to +-20 dB, 400 ms late, with the limiter at `peak_dbfs` behind it; it
        excludes `gain_db`.  Each text chunk is measured on its own, so the gain can differ between the chunks of a long text.
        `gain_db` (in [-40, 24]) and `peak_dbfs` (in [-20, 0], default -1, only together with a gain, a target, a tone or a compressor
        setting):
        the samples are amplified and peak-limited to 10^(peak_dbfs / 20).  0 is not None: it limits at the ceiling.
        `peak_dbtp` (same range, same default, accepted wherever `peak_dbfs` is and excluding it): the ceiling as a true
        peak, the peak of the reconstructed waveform as a BS.1770-4 meter reads it by 4x oversampling; the limiter then
        runs in true-peak mode, 10 samples later still, on a line with LA + 10 <= n.
        `encoding`: "pcm_s16le" (None on a table with the encoder), "pcm_f32le", "mulaw" or "alaw", among the configured:
        the chunks are int16, float32 or uint8 (ITU-T G.711) tensors, one element per sample.
        `compression`: "flac" where configured, only with `encoding` None or "pcm_s16le" and on a line `flac.plan` admits:
        the chunks are uint8 tensors, one whole FLAC frame each, which decode to the samples "pcm_s16le" would deliver.

        A stage that lags (all but the resampler, the toner, the compressor and the encoder) delays the output, not the count: the samples
        delivered in all stay those of the same request without it (the drain rule of the module's docstring).  ValueError for
        a value that is not configured, that a rule refuses on the request's line (the message lists what it admits there),
        and for any but None on a table without that stage (the message names the option to build it with)."""
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
        dplan, canon = None, dyn_rule.normalise(dynamics)
        if self.dynamics is not None:
            if canon is not None:
                if canon not in self.dynamics:
                    raise ValueError(f"dynamics {dynamics!r} is not configured (this pipeline has {self.dynamics})")
                dplan = self.dyn_index[(rate, n_out)][self.dynamics.index(canon)]
                if dplan is None:
                    raise ValueError(f"dynamics {dynamics!r} is not admissible at {rate} Hz (admissible there: "
                                     f"{self.dynamics_of(rate, n_out)})")
                if gain_db is None and loudness_lufs is None:
                    gain_db = 0.0  # the limiter behind the compressor
        elif canon is not None:
            raise ValueError(f"dynamics {dynamics!r}: this batcher has no dynamics stage (build it with dynamics for "
                             "per-request dynamics)")
        lvl = loud = None
        if peak_dbtp is not None and not self.true_peak:
            raise ValueError("peak_dbtp: this batcher has no true-peak mode (build it with true_peak=True)")
        if self.loud_plans is not None:
            target = loud_rule.check_with(loudness_lufs, gain_db)
            if target is not None:
                loud = (self.loud_index[(rate, n_out)], target)
                preroll += self.loud_plans[loud[0]].D
                gain_db = 0.0  # the limiter behind the normaliser
        elif loudness_lufs is not None:
            raise ValueError("loudness_lufs: this batcher has no loudness stage (build it with loudness=True)")
        if self.level_plans is not None:
            g_db, p_db = level_rule.check(gain_db, peak_dbfs, peak_dbtp)
            if g_db is not None:
                lvl = (self.level_index[(rate, n_out)], g_db, p_db)
                preroll += level_rule.plan(rate, n_out, peak_dbtp is not None).preroll  # LA, and 10 more in true-peak mode
        elif gain_db is not None or peak_dbfs is not None:
            raise ValueError("gain_db / peak_dbfs: this batcher has no level stage (build it with level=True)")
        bps = None
        if self.encodings is not None:
            encoding = encoding_rule.check(encoding, self.encodings)
            bps = encoding_rule.BYTES_PER_SAMPLE[encoding]
        elif encoding is not None:
            raise ValueError(f"encoding {encoding!r}: this batcher writes one sample format for all (build it with encodings "
                             "for per-request encodings)")
        if self.compressions is not None:
            if flac_rule.check(compression, self.compressions) is not None:
                flac_rule.plan(rate, n_out, encoding)
        elif compression is not None:
            raise ValueError(f"compression {compression!r}: this batcher writes uncompressed samples only (build it with "
                             "compressions for per-request compression)")
        return Route(r, rate, plan, stretched, lvl, n_out, preroll, -(-preroll // n_out),
                     "stretch" if stretched else "pitch" if pitched else "loud" if loud is not None
                     else "level" if lvl is not None else None, pplan, pitched, loud, encoding, bps, tplan, tplan is not None,
                     compression, dplan, dplan is not None, lvl is not None and peak_dbtp is not None)

    @staticmethod
    def line_of(native_rate: int, frame_samples: int, sample_rate=None, speed=None):
        """(sample_rate, speed, (rate, n)) of one request that gets a chain of its own: its rate and speed in canonical form
        (the native rate and speed 1.0 as None, the speed as the float of its fraction) and the line that leaves its
        stretcher, which the pitcher keeps.  `RequestError` with the message of the rule that refuses."""
        rate, n = int(native_rate), int(frame_samples)
        if sample_rate is not None:
            p = _ask("sample_rate", resample.plan, sample_rate, rate, frame_samples)
            sample_rate, rate, n = (None if p.rate == rate else p.rate), p.rate, p.out_n
        if speed is not None:
            speed = float(_ask("speed", stretch.fraction, speed))
            if speed == 1.0:
                speed = None
            else:
                n = _ask("speed", stretch.plan, speed, rate, n).n_out
        return sample_rate, speed, (rate, n)

    @staticmethod
    def for_request(native_rate: int, frame_samples: int, sample_rate=None, speed=None, gain_db=None, peak_dbfs=None,
                    pitch=None, loudness_lufs=None, encoding=None, tone=None, compression=None, dynamics=None,
                    peak_dbtp=None):
        """One request that gets a chain of its own (the fields of `route`): (spec, request), the `ChainSpec` of exactly the
        stages it uses and the request in canonical form, the dict that `spec.table(native_rate, frame_samples).route`
        takes - the native rate, speed 1.0 and pitch 1.0 as None, speed and pitch as the floats of their fractions, the tone
        and the compressor setting as their canonical strings, `peak_dbfs` defaulted, and `gain_db` 0.0 behind a tone or a
        compressor without a gain or a loudness target of its own; a ceiling given as `peak_dbtp` stays under that name (the
        dict then has `peak_dbfs` None, and the spec `true_peak`).  One walk in chain order over the request's own line, stage by stage through the plan rules themselves,
        so a refusal is the rule's: a `RequestError` with its message, whose `field` names the request field at fault."""
        sample_rate, speed, line = ChainTable.line_of(native_rate, frame_samples, sample_rate, speed)
        if pitch is not None:
            f = _ask("pitch", pitch_rule.fraction, pitch)
            pitch = None if f == 1 else _ask("pitch", pitch_rule.plan, f, *line).pitch
        tone = _ask("tone", tone_rule.normalise, tone)
        if tone is not None:
            _ask("tone", tone_rule.plan, *line, tone)
            _ask("tone", level_rule.plan, *line)
        dynamics = _ask("dynamics", dyn_rule.normalise, dynamics)
        if dynamics is not None:
            _ask("dynamics", dyn_rule.plan, *line, dynamics)
            _ask("dynamics", level_rule.plan, *line)
        tp = peak_dbtp is not None
        ceiling = "peak_dbtp" if tp else "loudness_lufs"  # the field a refusal of the ceiling names
        loudness_lufs = _ask("loudness_lufs", loud_rule.check_with, loudness_lufs, gain_db)
        if loudness_lufs is not None:  # the limiter behind the normaliser: no gain of its own, the request's ceiling
            _ask("loudness_lufs", loud_rule.plan, *line)
            _ask("loudness_lufs", level_rule.plan, *line)
            peak = _ask(ceiling, level_rule.check, 0.0, peak_dbfs, peak_dbtp)[1]
        else:
            if (tone is not None or dynamics is not None) and gain_db is None:
                gain_db = 0.0  # the limiter behind the tone or the compressor: no gain of its own, the request's ceiling
            gain_db, peak = _ask("gain_db" if tp is False else ceiling, level_rule.check, gain_db, peak_dbfs, peak_dbtp)
            if gain_db is not None:
                _ask("gain_db", level_rule.plan, *line)
        if tp:
            _ask("peak_dbtp", level_rule.plan, *line, True)
        peak_dbfs, peak_dbtp = (None, peak) if tp else (peak, None)
        if encoding is not None:
            _ask("encoding", encoding_rule.check, encoding)
        if compression is not None:
            _ask("compression", flac_rule.check, compression)
            _ask("compression", flac_rule.plan, *line, encoding)
        one = lambda v: None if v is None else (v,)  # noqa: E731
        spec = ChainSpec(one(sample_rate), one(speed), gain_db is not None, one(pitch), loudness_lufs is not None,
                         None if encoding is None else encoding_rule.NAMES, one(tone), one(compression), one(dynamics), tp)
        req = dict(sample_rate=sample_rate, speed=speed, gain_db=gain_db, peak_dbfs=peak_dbfs, pitch=pitch,
                   loudness_lufs=loudness_lufs, encoding=encoding, tone=tone)
        if compression is not None:  # only then: a request without it is the dict it always was
            req["compression"] = compression
        if dynamics is not None:  # likewise
            req["dynamics"] = dynamics
        if tp:  # likewise
            req["peak_dbtp"] = peak_dbtp
        return spec, req


class OutputChain:
    """The stages of `table` for `batch` rows on `engine`'s device: `rs` / `ts` / `ps` / `tn` / `dy` / `ln` / `lv` / `en` / `pk`
    (`engine.Resampler`, `Stretcher`, `Pitcher`, `Toner`, `Dynamics`, `Normalizer`, `Leveler`, `Encoder`, `Packer`; None where the table has no
    such stage), the device buffers between them and the pinned ring `out` of `nb` tensors, which the last stage writes.
    The buffer rule of the module's docstring gives them: without the encoder a ring slot is [batch, widest line], int16
    with `pcm_i16`, else float32; on a table with `encodings` it is uint8 [batch, encoding.pitch(widest line)], row b's
    n_out * bytes_per_sample bytes at the start of its row, and `pcm_i16` must be left False (ValueError); with `compressions`
    it is uint8 [batch, flac.pitch(widest line)], a row's prefix and bytes (`flac.py`, "the ring").  An empty table
    creates nothing: `out` is None and the codec writes its PCM as without a chain."""

    def __init__(self, engine, batch: int, table: ChainTable, nb: int, pcm_i16: bool = False):
        import torch

        from .engine import Dynamics, Encoder, Leveler, Normalizer, Packer, Pitcher, Resampler, Stretcher, Toner

        if table.encodings is not None and pcm_i16:
            raise ValueError("pcm_i16 and encodings exclude each other: with encodings a row asks for pcm_s16le itself")
        self.table = table
        self.rs = Resampler(engine, batch, table.sample_rates, table.rate_plans) if table.has_rates else None
        self.ts = Stretcher(engine, batch, table.stretch_plans) if table.speeds is not None else None
        self.ps = Pitcher(engine, batch, table.pitch_plans) if table.pitches is not None else None
        self.tn = Toner(engine, batch, table.tone_plans, table.width) if table.tone_plans is not None else None
        self.dy = Dynamics(engine, batch, table.dyn_plans, table.width) if table.dyn_plans is not None else None
        self.ln = Normalizer(engine, batch, table.loud_plans) if table.loud_plans is not None else None
        self.lv = Leveler(engine, batch, table.level_plans, table.true_peak) if table.level_plans is not None else None
        self.en = Encoder(engine, batch, table.width) if table.encodings is not None else None
        self.pk = Packer(engine, batch, table.width) if table.compressions is not None else None
        self._stages = [s for s in (*self.per_kind(), self.pk) if s is not None]
        self._between = []  # one device buffer between two stages serves every ring slot: the codec graphs run one after the other
        self.out = None
        if not self._stages:
            return
        for before, s in zip(self._stages, self._stages[1:]):
            if before._out_width != s._in_width:
                raise ValueError(f"{s._field}: the {s._name}'s line is not the line of the stage before it")
            self._between.append(torch.zeros(batch, s._in_width, device=engine.device,
                                             dtype=torch.uint8 if s is self.pk else torch.float32))
        if self.pk is not None:
            shape, dtype = (batch, self.pk.pitch), torch.uint8
        elif self.en is not None:
            shape, dtype = (batch, self.en.pitch), torch.uint8
        else:
            shape, dtype = (batch, self._stages[-1]._out_width), torch.int16 if pcm_i16 else torch.float32
        self.out = [torch.zeros(*shape, dtype=dtype).pin_memory() for _ in range(nb)]

    def per_kind(self):
        """(rs, ts, ps, tn, dy, ln, lv, en) in chain order, None where the table has no such stage; the packer is `pk`"""
        return self.rs, self.ts, self.ps, self.tn, self.dy, self.ln, self.lv, self.en

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

    def set_row(self, row: int, route: Route, stream=None, first_block: int = 0):
        """a new sequence joins `row` on `route` with a zero state in every stage, not draining; a stage the route does not
        use runs its identity plan or bypass.  `first_block`: the number of a flac row's first frame, what its request has
        delivered so far.  Stream-ordered"""
        for s in self._stages:
            if s is self.pk:
                s.set_row(row, route.n_out, route.encoding, route.compression, route.preroll, first_block, route.rate, stream)
            else:
                s.set_row(row, *s._route_args(route), stream)

    def drain_row(self, row: int, route: Route, stream=None):
        """from now on (stream-ordered) the row's incoming frames count as zeros at the stage `route.drain_stage` names"""
        for s in self._stages:
            if s._drain_name is not None and s._drain_name == route.drain_stage:
                s.set_row_drain(row, True, stream)

    def close(self):
        for s in reversed(self._stages):
            s.close()
