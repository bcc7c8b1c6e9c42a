"""Per-request output encoding: the last stage of the output chain, behind the leveler (`output_chain.py` gives its order;
the kernel is csrc/ptts_encode.hip; pure Python, nothing here touches the GPU).

A row's input `x` is whatever leaves the previous stage for that row, `n` fp32 samples per frame.  The stage writes
n * bytes_per_sample bytes at the start of the row's line of the output and nothing behind them.  It has no state, no
pre-roll and no drain flag: the zeros a draining stage emits before it are simply encoded.

  name        code  bytes  WAV tag  silence
  pcm_s16le   0     2      1        00 00
  pcm_f32le   1     4      3        00 00 00 00
  mulaw       2     1      7        FF
  alaw        3     1      6        D5

The contract of each encoding is exact:

  pcm_f32le   the four bytes of x, bit for bit (NaN and infinities included)
  pcm_s16le   s = (int16)(clamp(x, -1, 1) * 32767.0f), truncated towards zero, little-endian: the conversion every stage's own
              16-bit output uses.  The clamp drops a NaN for -1, so a NaN gives -32767; -32768 is never produced
  mulaw       ITU-T G.711 mu-law of the 14-bit value s >> 2 (arithmetic shift): the magnitude plus the bias 33, its segment
              (the position of its leading one) and the four bits below it, all eight bits inverted
  alaw        ITU-T G.711 A-law of the 13-bit value s >> 3 (arithmetic shift), the even bits inverted (0x55)

Both G.711 encodings are byte for byte what CPython's `audioop.lin2ulaw(b, 2)` / `audioop.lin2alaw(b, 2)` give for the
same s.  Fixed points: mu-law 0 -> FF, -1 -> 7E, 32767 -> 80, -32767 -> 00; A-law 0 -> D5, -1 -> 55, 32767 -> AA,
-32767 -> 2A.  Digital silence is therefore FF in mu-law and D5 in A-law: a zero byte there is a full-scale sample.

A row's line in the output is `pitch(width)` bytes: the widest encoding of the widest frame, rounded up to 16 bytes, so
that every lane of the kernel stores whole 16-byte words wherever a row's n allows it.
"""

from __future__ import annotations

PCM_S16LE, PCM_F32LE, MULAW, ALAW = "pcm_s16le", "pcm_f32le", "mulaw", "alaw"
NAMES = (PCM_S16LE, PCM_F32LE, MULAW, ALAW)          # NAMES[code]
CODE = {name: code for code, name in enumerate(NAMES)}  # what ptts_encoder_set_row takes
BYTES_PER_SAMPLE = {PCM_S16LE: 2, PCM_F32LE: 4, MULAW: 1, ALAW: 1}
WAV_FORMAT_TAG = {PCM_S16LE: 1, PCM_F32LE: 3, MULAW: 7, ALAW: 6}
SILENCE = {PCM_S16LE: b"\x00\x00", PCM_F32LE: b"\x00\x00\x00\x00", MULAW: b"\xff", ALAW: b"\xd5"}  # one sample of silence
DEFAULT = PCM_S16LE


def pitch(width: int) -> int:
    """bytes between two rows of an encoder's output for frames of up to `width` samples (en_pitch in csrc/ptts_encode.h)"""
    return (4 * int(width) + 15) // 16 * 16


def normalise_encodings(encodings) -> list:
    """The configured list: `pcm_s16le`, which is always available, first, then the others in the order given, each once.
    ValueError for a name that is no encoding."""
    if isinstance(encodings, str):
        raise ValueError(f"encodings must be a list of names, got the string {encodings!r}")
    out = [DEFAULT]
    for name in encodings:
        if not isinstance(name, str) or name not in CODE:
            raise ValueError(f"encoding {name!r} is not known (known: {list(NAMES)})")
        if name not in out:
            out.append(name)
    return out


def check(name, configured=NAMES) -> str:
    """`name` if it is one of `configured`, `pcm_s16le` for None; ValueError listing what is configured otherwise"""
    if name is None:
        return DEFAULT
    if not isinstance(name, str) or name not in configured:
        raise ValueError(f"encoding {name!r} is not configured (this pipeline has {list(configured)})")
    return name


def torch_dtype(name: str):
    """the dtype a job's chunks are typed as: int16, float32, uint8, uint8"""
    import torch

    return {PCM_S16LE: torch.int16, PCM_F32LE: torch.float32, MULAW: torch.uint8, ALAW: torch.uint8}[name]


def silence(name: str, n_samples: int) -> bytes:
    """`n_samples` samples of digital silence in the encoding `name`"""
    return SILENCE[name] * int(n_samples)
