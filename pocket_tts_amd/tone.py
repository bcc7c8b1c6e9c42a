"""Per-request tone: a streaming parametric equaliser, the stage of the output chain
codec -> resampler -> stretcher -> pitcher -> tone -> normaliser -> level -> encoder that sits before the normaliser, so that
the loudness is measured on what the listener hears and the limiter catches the peaks a boost creates (the kernel is
csrc/ptts_tone.hip; numpy only, nothing here touches the GPU).

A tone is a cascade of at most MAX_SECTIONS biquad sections, chosen by a preset's name or given as a band list:

  tone := preset | band (";" band)*
  band := kind ":" f0 [":" gain_db [":" q]]        kind = peak | lowshelf | highshelf
        | kind ":" f0 [":" q]                      kind = hp | lp: no gain

  f0        in [F0_MIN, 0.45 rate] Hz; the upper limit depends on the row's rate, so it is checked by `plan`, not by `normalise`
  gain_db   in [-24, 24]; required for peak, lowshelf and highshelf
  q         in [0.1, 16]; 1 / sqrt(2) where left out, 1.0 for a peak
  None, "" and "flat" are the bypass: `normalise` returns None.

`normalise(spec)` is the canonical string that tables and caches key on: a preset stays its (lowercased) name, a band list is
printed with every field, kinds lowercased and numbers as repr(float).  A preset expands to its band list (`PRESETS`); a
preset one of whose bands lies above 0.45 rate is NOT admissible at that rate (`bright` at 8 kHz) - it is refused with the
list of presets that rate admits, and no band is ever dropped silently.

Coefficients (`section`) are float64, divided by a0, in the audio-EQ-cookbook forms.  With w = 2 pi f0 / rate, c = cos w,
alpha = sin w / (2 q), A = 10^(gain_db / 40), r = 2 sqrt(A) alpha:

  hp         b = (1+c)/2, -(1+c), (1+c)/2                                   a = 1+alpha, -2c, 1-alpha
  lp         b = (1-c)/2, 1-c, (1-c)/2                                      a = 1+alpha, -2c, 1-alpha
  peak       b = 1+alpha A, -2c, 1-alpha A                                  a = 1+alpha/A, -2c, 1-alpha/A
  lowshelf   b = A((A+1)-(A-1)c+r), 2A((A-1)-(A+1)c), A((A+1)-(A-1)c-r)     a = (A+1)+(A-1)c+r, -2((A-1)+(A+1)c), (A+1)+(A-1)c-r
  highshelf  b = A((A+1)+(A-1)c+r), -2A((A-1)+(A+1)c), A((A+1)+(A-1)c-r)    a = (A+1)-(A-1)c+r, 2((A-1)-(A+1)c), (A+1)-(A-1)c-r

The streaming definition.  A row's input stream x is whatever leaves the previous stage for that row, n samples per frame.
Section k runs in transposed direct form II in float64 (`step`) on the output of section k - 1; every state is zero when the
row is set; y is rounded to fp32 once, after the last section.  There is no lag, no pre-roll and no drain flag: the zeros that
reach the stage once a row drains ring out like any other sample.  A row without a tone is on bypass: its whole line is copied
bit for bit.

The kernel walks a frame section by section.  A section is the 2-state linear recurrence s' = A s + B x with
A = [[-a1, 1], [-a2, 0]]: each thread runs CHUNK = ceil(n / THREADS) samples from a zero state (thread 0 from the row's carried
state), the chunk end states are combined by a log-step scan E[t] += A^(CHUNK 2^j) E[t - 2^j] with the powers of `powers`,
and each thread re-runs its chunk from its true state.  On the device a power is one float64 matrix: the normaliser
(`loudness.py`) hands each of its powers over as a high and a low part, because its high-pass at 38 Hz is all but a double
pole at z = 1 and it squares and sums what it filters, down to digital silence; here a section has two states, not four,
and the output is rounded to fp32 once, so a power rounded to float64 is enough.  It must be rounded ONCE, though.  Next to
z = 1 the entries of A^k grow like k and cancel by as much when a power is squared, so powers squared in float64 carry k eps
each and put k^2 eps into a state: 7e-9 of the running peak at 20 Hz and q = 16 at 48 kHz, three digits above the serial
recurrence.  `powers` therefore multiplies in integers, 256 bits wide, and rounds the result; the chunked scheme then stays
within 4e-13 of the running peak for every preset and within 8e-11 at the corners of the grammar (measured by
tests/cpp/tone_sweep.cpp), against the 6e-8 of the fp32 rounding that follows.
"""

from __future__ import annotations

import functools
import math
from fractions import Fraction

import numpy as np

RATE_MIN, RATE_MAX = 8000, 48000  # PTTS_TN_MIN_RATE, PTTS_TN_MAX_RATE in csrc/ptts_tone.h
MAX_N = 8192                      # PTTS_TN_MAX_N
THREADS = 1024                    # PTTS_TN_THREADS
SCAN_STEPS = 10                   # PTTS_TN_SCAN: 2^10 = THREADS
MAX_SECTIONS = 8                  # PTTS_TN_MAX_SECTIONS
F0_MIN, F0_MAX_OF_RATE = 20.0, 0.45
GAIN_MIN, GAIN_MAX = -24.0, 24.0
Q_MIN, Q_MAX = 0.1, 16.0
KINDS = ("hp", "lp", "peak", "lowshelf", "highshelf")
NO_GAIN = ("hp", "lp")
DOUBLES_PER_PLAN = MAX_SECTIONS * 5 + MAX_SECTIONS * SCAN_STEPS * 4

PRESETS = {
    "telephone": "hp:300:0.5411961;hp:300:1.3065630;lp:3400:0.5411961;lp:3400:1.3065630",  # a 4th-order Butterworth pair
    "warm": "lowshelf:200:3;highshelf:6000:-3",
    "bright": "highshelf:5000:4",
    "presence": "hp:80;peak:3000:4:1",
    "small_speaker": "hp:180;peak:2500:3:0.8",
    "deess": "peak:6500:-6:2",
}
BYPASS = ("", "flat")


def _number(spec, band, name, text, lo, hi):
    try:
        v = float(text)
    except ValueError:
        raise ValueError(f"tone {spec!r}: {name} of band {band!r} must be a number, got {text!r}") from None
    if not math.isfinite(v) or not lo <= v <= hi:
        raise ValueError(f"tone {spec!r}: {name} of band {band!r} must be in [{lo:g}, {hi:g}], got {text.strip()}")
    return v


def _bands(spec: str, text: str) -> list:
    """the bands of the band list `text` as (kind, f0, gain_db or None, q); `spec` is what the messages quote"""
    out = []
    for band in text.split(";"):
        parts = [p.strip() for p in band.split(":")]
        kind = parts[0].lower()
        if kind not in KINDS:
            raise ValueError(f"tone {spec!r}: {parts[0]!r} is neither a preset ({', '.join(PRESETS)}) nor a band kind "
                             f"({', '.join(KINDS)})")
        most = 3 if kind in NO_GAIN else 4
        if len(parts) < 2 or len(parts) > most or parts[1] == "":
            raise ValueError(f"tone {spec!r}: band {band.strip()!r} must read "
                             + (f"{kind}:f0[:q]" if kind in NO_GAIN else f"{kind}:f0:gain_db[:q]"))
        f0 = _number(spec, band.strip(), "f0", parts[1], F0_MIN, F0_MAX_OF_RATE * RATE_MAX)
        gain = None
        if kind not in NO_GAIN:
            if len(parts) < 3 or parts[2] == "":
                raise ValueError(f"tone {spec!r}: band {band.strip()!r} needs a gain, {kind}:f0:gain_db[:q]")
            gain = _number(spec, band.strip(), "gain_db", parts[2], GAIN_MIN, GAIN_MAX)
        q = 1.0 if kind == "peak" else math.sqrt(0.5)
        if len(parts) == most and parts[-1] != "":
            q = _number(spec, band.strip(), "q", parts[-1], Q_MIN, Q_MAX)
        out.append((kind, f0, gain, q))
    if len(out) > MAX_SECTIONS:
        raise ValueError(f"tone {spec!r}: {len(out)} sections, at most {MAX_SECTIONS}")
    return out


def _print(bands) -> str:
    return ";".join(":".join([k, repr(f0)] + ([] if g is None else [repr(g)]) + [repr(q)]) for k, f0, g, q in bands)


def normalise(spec):
    """The canonical string of a tone, None for the bypass (None, "", "flat").  ValueError naming the rule the spec fails;
    the upper limit of f0 is the rate's business (`plan`)."""
    if spec is None:
        return None
    if not isinstance(spec, str):
        raise ValueError(f"tone must be a preset's name or a band list, got {spec!r}")
    text = spec.strip()
    if text.lower() in BYPASS:
        return None
    if text.lower() in PRESETS:
        return text.lower()
    return _print(_bands(spec, text))


def bands(spec) -> list:
    """the sections of a tone after preset expansion: [(kind, f0, gain_db or None, q)], [] for the bypass"""
    canon = normalise(spec)
    if canon is None:
        return []
    return _bands(canon, PRESETS.get(canon, canon))


def section(kind: str, f0: float, gain_db, q: float, rate: int) -> np.ndarray:
    """(b0, b1, b2, a1, a2) of one section at `rate` Hz, float64, divided by a0: the table of the module's docstring"""
    w = 2.0 * math.pi * f0 / rate
    c, alpha = math.cos(w), math.sin(w) / (2.0 * q)
    if kind == "hp":
        b, a = ((1.0 + c) / 2.0, -(1.0 + c), (1.0 + c) / 2.0), (1.0 + alpha, -2.0 * c, 1.0 - alpha)
    elif kind == "lp":
        b, a = ((1.0 - c) / 2.0, 1.0 - c, (1.0 - c) / 2.0), (1.0 + alpha, -2.0 * c, 1.0 - alpha)
    else:
        A = 10.0 ** (gain_db / 40.0)
        r = 2.0 * math.sqrt(A) * alpha
        if kind == "peak":
            b, a = (1.0 + alpha * A, -2.0 * c, 1.0 - alpha * A), (1.0 + alpha / A, -2.0 * c, 1.0 - alpha / A)
        elif kind == "lowshelf":
            b = (A * ((A + 1.0) - (A - 1.0) * c + r), 2.0 * A * ((A - 1.0) - (A + 1.0) * c), A * ((A + 1.0) - (A - 1.0) * c - r))
            a = ((A + 1.0) + (A - 1.0) * c + r, -2.0 * ((A - 1.0) + (A + 1.0) * c), (A + 1.0) + (A - 1.0) * c - r)
        elif kind == "highshelf":
            b = (A * ((A + 1.0) + (A - 1.0) * c + r), -2.0 * A * ((A - 1.0) + (A + 1.0) * c), A * ((A + 1.0) + (A - 1.0) * c - r))
            a = ((A + 1.0) - (A - 1.0) * c + r, 2.0 * ((A - 1.0) - (A + 1.0) * c), (A + 1.0) - (A - 1.0) * c - r)
        else:
            raise ValueError(f"tone: {kind!r} is not a band kind ({', '.join(KINDS)})")
    return np.array([b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0]], dtype=np.float64)


def presets_at(rate: int) -> list:
    """the presets admissible at `rate` Hz, in the order of `PRESETS`"""
    return [name for name in PRESETS if all(f0 <= F0_MAX_OF_RATE * rate for _, f0, _, _ in bands(name))]


def coefficients(spec, rate: int) -> np.ndarray:
    """[K, 5] float64: (b0, b1, b2, a1, a2) of the tone's sections at `rate` Hz ([0, 5] for the bypass).  ValueError for a
    rate out of range and for a band above 0.45 rate: the message says what that rate admits"""
    rate = int(rate)
    if not RATE_MIN <= rate <= RATE_MAX:
        raise ValueError(f"tone at {rate} Hz: the rate must be in [{RATE_MIN}, {RATE_MAX}]")
    canon = normalise(spec)
    top = F0_MAX_OF_RATE * rate
    for kind, f0, _, _ in bands(canon):
        if f0 > top:
            what = (f"the presets admissible there: {presets_at(rate)}" if canon in PRESETS
                    else f"f0 must be in [{F0_MIN:g}, {top:g}] there")
            raise ValueError(f"tone {canon!r} is not admissible at {rate} Hz: its band {kind} at {f0:g} Hz lies above "
                             f"0.45 x the rate ({what})")
    return np.array([section(*b, rate) for b in bands(canon)], dtype=np.float64).reshape(-1, 5)


def step(coef, s, x):
    """One sample of one section in transposed direct form II (tn_step in csrc/ptts_tone.h).  `s` is a list of two floats,
    changed in place; returns y"""
    b0, b1, b2, a1, a2 = coef
    y = b0 * x + s[0]
    s[0] = b1 * x - a1 * y + s[1]
    s[1] = b2 * x - a2 * y
    return y


def chunk_of(n: int) -> int:
    """samples a thread runs: ceil(n / THREADS)"""
    return -(-int(n) // THREADS)


_KEEP = 256  # bits of the largest entry kept after a product


def _trim(M, e):
    """M 2^-e with the largest entry cut to _KEEP bits"""
    cut = max(abs(v).bit_length() for v in M) - _KEEP
    return (M, e) if cut <= 0 else ([v >> cut for v in M], e - cut)


def _mul(P, Q):
    return [P[0] * Q[0] + P[1] * Q[2], P[0] * Q[1] + P[1] * Q[3], P[2] * Q[0] + P[3] * Q[2], P[2] * Q[1] + P[3] * Q[3]]


@functools.lru_cache(maxsize=1024)
def _powers(a1: float, a2: float, chunk: int) -> np.ndarray:
    fa1, fa2 = Fraction(-a1), Fraction(-a2)  # a double is a dyadic rational
    E = max(fa1.denominator.bit_length(), fa2.denominator.bit_length()) - 1
    A = [int(fa1 * (1 << E)), 1 << E, int(fa2 * (1 << E)), 0]  # A 2^E, exactly
    M, e = [1, 0, 0, 1], 0
    for _ in range(chunk):
        M, e = _trim(_mul(M, A), e + E)
    out = np.empty((SCAN_STEPS, 2, 2), dtype=np.float64)
    for t in range(SCAN_STEPS):
        for i in range(4):
            out[t, i // 2, i % 2] = float(Fraction(M[i], 1 << e) if e >= 0 else Fraction(M[i] << -e))
        M, e = _trim(_mul(M, M), 2 * e)
    out.setflags(write=False)
    return out


def powers(coef, chunk: int) -> np.ndarray:
    """[SCAN_STEPS, 2, 2] float64: A^(chunk 2^t), t = 0 .. SCAN_STEPS - 1, of one section's state transition
    A = [[-a1, 1], [-a2, 0]] with the float64 coefficients: computed in integers cut to _KEEP bits after every product and
    rounded to float64 once (the docstring says why).  Read-only: shared by the plans of one (section, chunk)"""
    return _powers(float(coef[3]), float(coef[4]), int(chunk))


class TonePlan:
    """What the toner needs for one (tone, rate, n): the canonical `tone`, the section count `K`, `chunk`, the coefficients
    `coef` [K, 5] and the scan's `powers` [K, SCAN_STEPS, 2, 2], all float64."""

    __slots__ = ("tone", "rate", "n", "K", "chunk", "coef", "powers")

    def __init__(self, tone, rate, n, coef):
        self.tone, self.rate, self.n = tone, rate, n
        self.K = len(coef)
        self.chunk = chunk_of(n)
        self.coef = coef
        self.powers = np.array([powers(c, self.chunk) for c in coef], dtype=np.float64).reshape(self.K, SCAN_STEPS, 2, 2)

    def ints(self):
        """the plan's integers as the C ABI takes them; the library derives the chunk itself"""
        return (self.rate, self.n, self.K)

    def doubles(self) -> np.ndarray:
        """the plan's float64 values as the C ABI takes them: MAX_SECTIONS x 5 coefficients, then MAX_SECTIONS x SCAN_STEPS
        x 4 powers, zero behind the K-th section"""
        c = np.zeros((MAX_SECTIONS, 5), dtype=np.float64)
        p = np.zeros((MAX_SECTIONS, SCAN_STEPS, 2, 2), dtype=np.float64)
        c[:self.K], p[:self.K] = self.coef, self.powers
        return np.concatenate([c.reshape(-1), p.reshape(-1)])


def plan(rate: int, n: int, spec) -> TonePlan:
    """The `TonePlan` of the tone `spec` for frames of `n` samples at `rate` Hz, or ValueError naming the rule it fails.
    The bypass has no plan (ValueError): a row without a tone is dealt the index -1"""
    rate, n = int(rate), int(n)
    canon = normalise(spec)
    if canon is None:
        raise ValueError("tone: the bypass has no plan")
    coef = coefficients(canon, rate)
    if not 1 <= n <= MAX_N:
        raise ValueError(f"tone at {rate} Hz: a frame of {n} samples is not in [1, {MAX_N}]")
    return TonePlan(canon, rate, n, coef)


def normalise_tones(tones) -> list:
    """a configured tone list as canonical strings, each once, in the order given (the bypass needs no entry and is left
    out); ValueError for a tone the grammar refuses"""
    if isinstance(tones, str):
        raise ValueError(f"tones must be a list of tones, got the string {tones!r}")
    out = []
    for t in tones:
        c = normalise(t)
        if c is not None and c not in out:
            out.append(c)
    return out


def table(lines, tones):
    """The plan table of (each distinct (rate, n) among `lines`, in their order) x (each tone).  `tones`: a list as
    `normalise_tones` returns it.  Returns (plans, index) with index[(rate, n)][tone index] = the plan's position in
    `plans`, or None where `plan` refuses the pair.  ValueError for a tone that is admissible on none of the lines."""
    plans, index = [], {}
    for rate, n in lines:
        key = (int(rate), int(n))
        if key in index:
            continue
        row = []
        for t in tones:
            try:
                pl = plan(*key, t)
            except ValueError:
                pl = None
            row.append(None if pl is None else len(plans))
            if pl is not None:
                plans.append(pl)
        index[key] = row
    for j, t in enumerate(tones):
        if all(row[j] is None for row in index.values()):
            plan(*next(iter(index)), t)  # raises with the rule the tone fails on the first line
            raise ValueError(f"tone {t!r}: not admissible on any of the configured lines")
    return plans, index


def run(coef, x, state=None):
    """The serial definition: the float64 stream `x` through the sections `coef` [K, 5] from `state` ([K, 2], None: zero).
    Returns (y float64, not yet rounded; the state after)"""
    coef = np.asarray(coef, dtype=np.float64).reshape(-1, 5)
    s = np.zeros((len(coef), 2)) if state is None else np.array(state, dtype=np.float64)
    y = np.array(x, dtype=np.float64)
    for k, c in enumerate(coef):
        c, sk = [float(v) for v in c], [float(s[k, 0]), float(s[k, 1])]
        for i in range(len(y)):
            y[i] = step(c, sk, float(y[i]))
        s[k] = sk
    return y, s
