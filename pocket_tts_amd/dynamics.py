"""Per-request dynamics: a streaming speech compressor, the stage of the output chain
codec -> resampler -> stretcher -> pitcher -> toner -> dynamics -> normaliser -> leveler -> encoder -> packer that sits behind
the equaliser and in front of the loudness measurement, so that the target loudness holds for what the listener hears and
the limiter catches what the make-up gain and the attack time let through (the kernel is csrc/ptts_dyn.hip; numpy only,
nothing here touches the GPU).

A setting is a preset's name or a list of key=value pairs joined by ";":

  setting := preset | pair (";" pair)*
  pair    := key "=" number

  threshold  in [-60, 0] dBFS     T
  ratio      in [1, 20]           R
  knee       in [0, 24] dB        W, the full width of the soft knee
  attack     in [0.1, 100] ms
  release    in [10, 2000] ms
  makeup     in [0, 24] dB        M
  None, "" and "off" are the bypass: `normalise` returns None.

A key that is left out takes the value of the preset `speech`; a key given twice and a key that is none of the six are
refused.  `normalise(spec)` is the canonical string that tables and caches key on: a preset stays its (lowercased) name, a
pair list is printed with all six keys in the order above and numbers as repr(float).  The presets (`PRESETS`) are `speech`,
`gentle`, `broadcast` and `telephone`.

The streaming definition.  Everything is float64; the output is rounded to fp32 once.  A row's input stream x is whatever
leaves the stage before it for that row, n samples per frame.  The row carries two doubles, p and s, both zero when the row
is set.  With K = ln(10) / 20, aA = exp(-1 / (attack_ms rate / 1000)), aR = exp(-1 / (release_ms rate / 1000)) and
k = 1 - 1 / R:

  a[i] = |x[i]| > 1e-6 ? |x[i]| : 1e-6 ;  a[i] = a[i] < 1e6 ? a[i] : 1e6     (a NaN compares false: 1e-6)
  L[i] = ln(a[i]) / K                                                        (dBFS, in [-120, 120])
  d    = L[i] - T
  c[i] = 0                          if 2d <= -W
       = k (d + W/2)^2 / (2W)       if -W < 2d < W
       = k d                        if 2d >= W                               (the wanted reduction in dB, >= 0)
  p[i] = max(c[i], aR p[i-1])                                                (instant rise, release decay)
  s[i] = aA s[i-1] + (1 - aA) p[i]                                           (attack smoothing)
  y[i] = fp32( exp((M - s[i]) K) * x[i] )

This is the log-domain feed-forward compressor with the decoupled smooth peak detector: the release decay runs on p and the
attack smoothing on s behind it, so a falling level is smoothed by both and the effective release is attack + release.  The
clamp at 1e6 keeps one Inf from pinning p at infinity for the rest of the request.  s >= 0 always, so the gain never exceeds
the make-up.  A NaN sample comes out as NaN and counts as the floor for p and s.

There is no look-ahead: the stage has no lag, no pre-roll and no drain flag.  The zeros of a draining row pass through it
like any sample, and the release rings out on them.  A row without a setting is on bypass: its whole line is copied bit for
bit.  A row with a setting always runs the limiter behind it.

The two recurrences are written so that a frame is two associative scans: p is the leveler's max(c, A d) form, s is a
one-state linear recurrence.  The kernel gives each thread CHUNK = ceil(n / THREADS) samples, runs them from zero (thread 0
from the carried state), combines the chunk ends over the threads in a log-step scan, E[t] = max(E[t], aR^(CHUNK 2^j)
E[t - 2^j]) for p and E[t] += aA^(CHUNK 2^j) E[t - 2^j] for s, and re-runs each chunk from its true start.  A plan therefore
holds the ten powers of aA and the ten of aR, each computed directly as exp(-CHUNK 2^j / tau) in float64, not by squaring.
"""

from __future__ import annotations

import math

import numpy as np

RATE_MIN, RATE_MAX = 8000, 48000  # PTTS_DY_MIN_RATE, PTTS_DY_MAX_RATE in csrc/ptts_dyn.h
MAX_N = 8192                      # PTTS_DY_MAX_N
THREADS = 1024                    # PTTS_DY_THREADS
SCAN_STEPS = 10                   # PTTS_DY_SCAN: 2^10 = THREADS
K = math.log(10.0) / 20.0         # PTTS_DY_K: dB to nepers
A_MIN, A_MAX = 1e-6, 1e6          # the clamp of |x|: L in [-120, 120]
KEYS = ("threshold", "ratio", "knee", "attack", "release", "makeup")
RANGES = dict(threshold=(-60.0, 0.0), ratio=(1.0, 20.0), knee=(0.0, 24.0), attack=(0.1, 100.0), release=(10.0, 2000.0),
              makeup=(0.0, 24.0))
DOUBLES_PER_PLAN = 6 + 2 * SCAN_STEPS

PRESETS = {
    "speech": "threshold=-20;ratio=3;knee=6;attack=5;release=100;makeup=4",
    "gentle": "threshold=-16;ratio=2;knee=10;attack=10;release=200;makeup=2",
    "broadcast": "threshold=-24;ratio=4;knee=8;attack=3;release=150;makeup=8",
    "telephone": "threshold=-18;ratio=6;knee=4;attack=2;release=60;makeup=6",
}
BYPASS = ("", "off")


def _pairs(spec: str, text: str, defaults=None) -> dict:
    """the six values of the pair list `text`, keys left out taken from `defaults`; `spec` is what the messages quote"""
    out = {}
    for pair in text.split(";"):
        key, eq, value = pair.partition("=")
        key = key.strip().lower()
        if not eq or key not in KEYS:
            raise ValueError(f"dynamics {spec!r}: {pair.strip()!r} is neither a preset ({', '.join(PRESETS)}) nor a "
                             f"key=value pair with a key of {', '.join(KEYS)}")
        if key in out:
            raise ValueError(f"dynamics {spec!r}: the key {key} is given twice")
        lo, hi = RANGES[key]
        try:
            v = float(value)
        except ValueError:
            raise ValueError(f"dynamics {spec!r}: {key} must be a number in [{lo:g}, {hi:g}], got {value.strip()!r}") from None
        if not math.isfinite(v) or not lo <= v <= hi:
            raise ValueError(f"dynamics {spec!r}: {key} must be in [{lo:g}, {hi:g}], got {value.strip()}")
        out[key] = v
    return {k: out.get(k, None if defaults is None else defaults[k]) for k in KEYS}


_SPEECH = _pairs("speech", PRESETS["speech"])


def normalise(spec):
    """The canonical string of a setting, None for the bypass (None, "", "off").  ValueError naming the key and the range
    the spec fails"""
    if spec is None:
        return None
    if not isinstance(spec, str):
        raise ValueError(f"dynamics must be a preset's name or a list of key=value pairs, got {spec!r}")
    text = spec.strip()
    if text.lower() in BYPASS:
        return None
    if text.lower() in PRESETS:
        return text.lower()
    v = _pairs(spec, text, _SPEECH)
    return ";".join(f"{k}={v[k]!r}" for k in KEYS)


def values(spec) -> dict:
    """the six values of a setting after preset expansion, {key: float}; ValueError for the bypass"""
    canon = normalise(spec)
    if canon is None:
        raise ValueError("dynamics: the bypass has no values")
    return _pairs(canon, PRESETS.get(canon, canon), _SPEECH)


def curve(L: float, T: float, k: float, W: float) -> float:
    """The static curve: the wanted reduction in dB, >= 0, of a sample at L dBFS (dy_curve in csrc/ptts_dyn.h)"""
    d = L - T
    if 2.0 * d <= -W:
        return 0.0
    if 2.0 * d < W:
        return k * (d + W / 2.0) * (d + W / 2.0) / (2.0 * W)
    return k * d


def level(x: float) -> float:
    """|x| in dBFS, clamped to [-120, 120]; a NaN is the floor (dy_level)"""
    a = abs(x)
    a = a if a > A_MIN else A_MIN
    a = a if a < A_MAX else A_MAX
    return math.log(a) / K


def chunk_of(n: int) -> int:
    """samples a thread runs: ceil(n / THREADS)"""
    return -(-int(n) // THREADS)


class DynPlan:
    """What the compressor needs for one (setting, rate, n): the canonical `setting`, `chunk`, the curve's `T`, `k`, `W`,
    the make-up `M`, the per-sample decays `aA` and `aR` and the scan's powers `pow_a[j]` = aA^(chunk 2^j) and `pow_r[j]`
    = aR^(chunk 2^j), all float64."""

    __slots__ = ("setting", "rate", "n", "chunk", "T", "k", "W", "M", "aA", "aR", "pow_a", "pow_r")

    def __init__(self, setting, rate, n, v):
        self.setting, self.rate, self.n = setting, rate, n
        self.chunk = chunk_of(n)
        self.T, self.k, self.W, self.M = v["threshold"], 1.0 - 1.0 / v["ratio"], v["knee"], v["makeup"]
        tau_a, tau_r = v["attack"] * rate / 1000.0, v["release"] * rate / 1000.0  # in samples
        self.aA, self.aR = math.exp(-1.0 / tau_a), math.exp(-1.0 / tau_r)
        self.pow_a = np.array([math.exp(-(self.chunk << j) / tau_a) for j in range(SCAN_STEPS)], dtype=np.float64)
        self.pow_r = np.array([math.exp(-(self.chunk << j) / tau_r) for j in range(SCAN_STEPS)], dtype=np.float64)

    def ints(self):
        """the plan's integers as the C ABI takes them; the library derives the chunk itself"""
        return (self.rate, self.n)

    def doubles(self) -> np.ndarray:
        """the plan's float64 values as the C ABI takes them: T, k, W, M, aA, aR, then the SCAN_STEPS powers of aA and the
        SCAN_STEPS powers of aR"""
        return np.concatenate([[self.T, self.k, self.W, self.M, self.aA, self.aR], self.pow_a, self.pow_r]).astype(np.float64)


def plan(rate: int, n: int, spec) -> DynPlan:
    """The `DynPlan` of the setting `spec` for frames of `n` samples at `rate` Hz, or ValueError naming the rule it fails.
    The bypass has no plan (ValueError): a row without a setting is dealt the index -1"""
    rate, n = int(rate), int(n)
    canon = normalise(spec)
    if canon is None:
        raise ValueError("dynamics: the bypass has no plan")
    if not RATE_MIN <= rate <= RATE_MAX:
        raise ValueError(f"dynamics at {rate} Hz: the rate must be in [{RATE_MIN}, {RATE_MAX}]")
    if not 1 <= n <= MAX_N:
        raise ValueError(f"dynamics at {rate} Hz: a frame of {n} samples is not in [1, {MAX_N}]")
    return DynPlan(canon, rate, n, values(canon))


def normalise_dynamics(settings) -> list:
    """a configured list of settings as canonical strings, each once, in the order given (the bypass needs no entry and is
    left out); ValueError for a setting the grammar refuses and for a list that holds none"""
    if isinstance(settings, str):
        raise ValueError(f"dynamics must be a list of settings, got the string {settings!r}")
    out = []
    for s in settings:
        c = normalise(s)
        if c is not None and c not in out:
            out.append(c)
    if not out:
        raise ValueError("dynamics: the list holds no setting but the bypass, which every request has anyway")
    return out


def table(lines, settings):
    """The plan table of (each distinct (rate, n) among `lines`, in their order) x (each setting).  `settings`: a list as
    `normalise_dynamics` returns it.  Returns (plans, index) with index[(rate, n)][setting index] = the plan's position in
    `plans`, or None where `plan` refuses the line.  ValueError for a setting that is admissible on none of the lines."""
    plans, index = [], {}
    for rate, n in lines:
        key = (int(rate), int(n))
        if key in index:
            continue
        row = []
        for s in settings:
            try:
                pl = plan(*key, s)
            except ValueError:
                pl = None
            row.append(None if pl is None else len(plans))
            if pl is not None:
                plans.append(pl)
        index[key] = row
    for j, s in enumerate(settings):
        if all(row[j] is None for row in index.values()):
            plan(*next(iter(index)), s)  # raises with the rule the setting fails on the first line
            raise ValueError(f"dynamics {s!r}: not admissible on any of the configured lines")
    return plans, index


def step(pl: DynPlan, state, x: float) -> float:
    """One sample (dy_step in csrc/ptts_dyn.h).  `state` is the list [p, s], changed in place; returns y in float64, not
    yet rounded"""
    c = curve(level(x), pl.T, pl.k, pl.W)
    q = pl.aR * state[0]
    state[0] = c if c > q else q
    state[1] = pl.aA * state[1] + (1.0 - pl.aA) * state[0]
    return math.exp((pl.M - state[1]) * K) * x


def run(pl: DynPlan, x, state=None):
    """The serial definition: the stream `x` through the plan from `state` ((p, s), None: zero).  Returns (y float64, not
    yet rounded; the state after)"""
    st = [0.0, 0.0] if state is None else [float(state[0]), float(state[1])]
    y = np.array(x, dtype=np.float64)
    for i in range(len(y)):
        y[i] = step(pl, st, float(y[i]))
    return y, (st[0], st[1])
