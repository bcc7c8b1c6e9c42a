"""Per-request FLAC output: the packer, the eighth link of the output chain, behind the encoder (`output_chain.py` gives the
order; the kernel is csrc/ptts_flac.hip, what it shares with a host program csrc/ptts_flac.h; pure Python, nothing here
touches the GPU).

The packer compresses the `pcm_s16le` bytes the encoder wrote for a row.  The contract is exact: the FLAC stream decodes to
the very samples `pcm_s16le` would have delivered.  One line of the row (one codec frame, `n` samples) becomes one FLAC frame,
which is self-contained, so a stream starts as early as without it.  A request's `compression` is None or "flac".

The bitstream.  A block is n int16 samples x (16 <= n <= 4608, the FLAC subset's limit up to 48 kHz), mono, 16 bits, in a
fixed-blocksize stream.

  frame header   FF F8, then 0111 ssss (the blocksize always follows as 16 bits; ssss is the rate code: 8000 0100, 16000 0101,
                 22050 0110, 24000 0111, 32000 1000, 44100 1001, 48000 1010, any other rate 1101 with the rate in Hz as 16 bits
                 behind the blocksize), then 08 (mono, 16 bits), the frame number in FLAC's UTF-8-like coding (1 to 6 bytes,
                 numbers below 2^31), n - 1 as 16 bits, the 16-bit rate where the code is 1101, and the CRC-8 (polynomial 0x07,
                 initial value 0) of everything before it
  subframe       all samples equal: CONSTANT, the byte 00 and the value as 16 bits.  Otherwise, for each fixed predictor order
                 o in 0..4 the residuals e_o[i], i in [o, n):
                   e_0 = x[i]                     e_1 = x[i] - x[i-1]                 e_2 = x[i] - 2 x[i-1] + x[i-2]
                   e_3 = x[i] - 3 x[i-1] + 3 x[i-2] - x[i-3]     e_4 = x[i] - 4 x[i-1] + 6 x[i-2] - 4 x[i-3] + x[i-4]
                 are folded, u = (e << 1) ^ (e >> 31), and for each Rice parameter k in 0..14
                   bits(o, k) = 16 o + 10 + sum((u >> k) + 1 + k)
                 in 64-bit sums.  The smallest wins; ties go to the smaller o, then the smaller k.  If it is >= 16 n: VERBATIM,
                 the byte 02 and the n samples as 16 bits.  Otherwise FIXED: the byte 0x10 | (o << 1), o warm-up samples of 16
                 bits, 2 bits 00 (4-bit Rice parameters), 4 bits 0000 (partition order 0), 4 bits k, and each residual as u >> k
                 zero bits, a one bit and the low k bits of u, most significant first.  All values are big-endian two's
                 complement.  No wasted-bits detection, no LPC subframes, no Rice partitions beyond order 0.
  footer         zero bits up to the byte boundary, then the CRC-16 (polynomial 0x8005, initial value 0, not reflected,
                 big-endian) of the whole frame, header and CRC-8 included

A frame is therefore at most 15 + (1 + 2 n) + 2 = 2 n + 18 bytes.

The ring.  On a table with the packer a row's ring line is `pitch(width)` bytes: a 16-byte prefix {u32 nbytes, 0, 0, 0},
then nbytes bytes - a pass-through row's n * bytes_per_sample encoded bytes, or a flac row's frame - and nothing behind 16 +
nbytes rounded up to 16.

The cut.  A row with pre-roll p delivers the samples [p, p + frames * n) of its line sequence.  The host cannot slice a
compressed frame, so the kernel cuts: with off = p % n and lead = ceil(p / n) the first `lead` lines emit nothing (nbytes 0),
and line f >= lead emits block f - lead, the previous line's [off, n) followed by the current line's [0, off), as frame number
first_block + f - lead.  A request of F frames thus yields exactly F blocks of n samples.

A stream is `stream_header`, the frames, and `silence`, the 200 ms tail every container gets, as CONSTANT frames.
"""

from __future__ import annotations

from . import encoding as encoding_rule

FLAC = "flac"
COMPRESSIONS = (FLAC,)
MIN_N, MAX_N = 16, 4608
MAX_RATE = 65535
PREFIX = 16  # bytes of a ring line's prefix
RATE_CODES = {8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10}


def normalise_compressions(compressions) -> list:
    """The configured list, each name once in the order given.  ValueError for a name that is no compression."""
    if isinstance(compressions, str):
        raise ValueError(f"compressions must be a list of names, got the string {compressions!r}")
    out = []
    for name in compressions:
        if not isinstance(name, str) or name not in COMPRESSIONS:
            raise ValueError(f"compression {name!r} is not known (known: {list(COMPRESSIONS)})")
        if name not in out:
            out.append(name)
    return out


def check(name, configured=COMPRESSIONS):
    """`name` if it is None or one of `configured`; ValueError listing what is configured otherwise"""
    if name is None:
        return None
    if not isinstance(name, str) or name not in configured:
        raise ValueError(f"compression {name!r} is not configured (this pipeline has {list(configured)})")
    return name


def plan(rate: int, n: int, encoding=None):
    """(rate, n) of a line of `n` samples per frame at `rate` Hz that FLAC admits; ValueError naming the limit otherwise"""
    rate, n = int(rate), int(n)
    if encoding is not None and encoding != encoding_rule.PCM_S16LE:
        raise ValueError(f"flac compresses pcm_s16le only, not encoding {encoding!r}")
    if not MIN_N <= n <= MAX_N:
        raise ValueError(f"flac needs frames of {MIN_N} to {MAX_N} samples, not {n} (at {rate} Hz)")
    if not 1 <= rate <= MAX_RATE:
        raise ValueError(f"flac frames carry rates up to {MAX_RATE} Hz, not {rate}")
    return rate, n


def pitch(width: int) -> int:
    """bytes between two rows of a packer's ring for frames of up to `width` samples (fl_pitch in csrc/ptts_flac.h): the
    prefix, then the widest pass-through line or the largest frame, rounded up to 16"""
    w = int(width)
    return PREFIX + (max(4 * w, 2 * w + 18) + 15) // 16 * 16


def _crc_table(poly: int, bits: int):
    top, mask = 1 << (bits - 1), (1 << bits) - 1
    table = []
    for b in range(256):
        c = b << (bits - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        table.append(c)
    return table


CRC8_TABLE = _crc_table(0x07, 8)
CRC16_TABLE = _crc_table(0x8005, 16)


def crc8(data: bytes) -> int:
    c = 0
    for b in data:
        c = CRC8_TABLE[c ^ b]
    return c


def crc16(data: bytes) -> int:
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ CRC16_TABLE[(c >> 8) ^ b]
    return c


def utf8_number(v: int) -> bytes:
    """FLAC's UTF-8-like coding of a frame number below 2^31: 1 to 6 bytes"""
    v = int(v)
    if not 0 <= v < 1 << 31:
        raise ValueError(f"frame number {v} is not in [0, 2^31)")
    if v < 0x80:
        return bytes([v])
    n = 2 if v < 0x800 else 3 if v < 0x10000 else 4 if v < 0x200000 else 5 if v < 0x4000000 else 6
    out = [((0xFF00 >> n) & 0xFF) | (v >> (6 * (n - 1)))]
    out += [0x80 | ((v >> (6 * (n - 1 - i))) & 0x3F) for i in range(1, n)]
    return bytes(out)


def frame_header(number: int, n: int, rate: int) -> bytes:
    """the header of frame `number` of `n` samples at `rate` Hz, its CRC-8 included"""
    n, rate = int(n), int(rate)
    if not 1 <= n <= 65536 or not 1 <= rate <= MAX_RATE:
        raise ValueError(f"frame header: {n} samples at {rate} Hz do not fit 16 bits each")
    code = RATE_CODES.get(rate, 13)
    h = bytes([0xFF, 0xF8, 0x70 | code, 0x08]) + utf8_number(number) + (n - 1).to_bytes(2, "big")
    if code == 13:
        h += rate.to_bytes(2, "big")
    return h + bytes([crc8(h)])


def silent_frame(number: int, n: int, rate: int) -> bytes:
    """one frame of `n` samples of digital silence: a CONSTANT subframe of value 0"""
    f = frame_header(number, n, rate) + b"\x00\x00\x00"
    return f + crc16(f).to_bytes(2, "big")


def _mul16(a: int, b: int) -> int:
    """the product of two remainders modulo the CRC-16 polynomial x^16 + x^15 + x^2 + 1 (bit i: the coefficient of x^i)"""
    r = 0
    while b:
        if b & 1:
            r ^= a
        b >>= 1
        a <<= 1
        if a & 0x10000:
            a ^= 0x18005
    return r


def _xpow16(n: int) -> int:
    """x^n modulo the CRC-16 polynomial, by square-and-multiply"""
    r, b = 1, 2
    while n:
        if n & 1:
            r = _mul16(r, b)
        b = _mul16(b, b)
        n >>= 1
    return r


def header_length(frame: bytes) -> int:
    """bytes of the header of `frame`, its CRC-8 included; ValueError where `frame` does not begin with a frame header of a
    fixed-blocksize stream whose CRC-8 holds"""
    if len(frame) < 6 or frame[0] != 0xFF or frame[1] != 0xF8:
        raise ValueError("not a FLAC frame of a fixed-blocksize stream: no FF F8 sync")
    b = frame[4]
    digits = 1 if b < 0x80 else 8 - (b ^ 0xFF).bit_length()
    if not 1 <= digits <= 6 or (b >= 0x80 and digits < 2):
        raise ValueError("not a FLAC frame: malformed frame number")
    size, rate = frame[2] >> 4, frame[2] & 15
    n = 4 + digits + (1 if size == 6 else 2 if size == 7 else 0) + (1 if rate == 12 else 2 if rate in (13, 14) else 0) + 1
    if len(frame) < n + 2 or crc8(frame[:n - 1]) != frame[n - 1]:
        raise ValueError("not a FLAC frame: the header's CRC-8 does not hold")
    return n


def renumber(frame: bytes, number: int) -> bytes:
    """`frame`, one whole frame, as frame `number` of its stream: the header with the new number (its length may change)
    and CRC-8, the same subframe, the CRC-16 that belongs to them.

    Both CRCs start at 0 and have no final xor, so they are linear: with header A, the rest B of the frame and the CRC-16
    taken as the remainder of the message times x^16, crc16(A | B) = crc16(A) * x^(8 |B|) + crc16(B).  The new CRC-16 is the
    old one plus (crc16(A_old) + crc16(A_new)) * x^(8 |B|), which costs the two headers and a square-and-multiply, not a
    pass over the frame."""
    frame = bytes(frame)
    n = header_length(frame)
    at = 4 + (1 if frame[4] < 0x80 else 8 - (frame[4] ^ 0xFF).bit_length())
    head = frame[:4] + utf8_number(number) + frame[at:n - 1]
    head += bytes([crc8(head)])
    body = frame[n:-2]
    crc = int.from_bytes(frame[-2:], "big") ^ _mul16(crc16(frame[:n]) ^ crc16(head), _xpow16(8 * len(body)))
    return head + body + crc.to_bytes(2, "big")


def silence(first_number: int, rate: int, n: int) -> bytes:
    """the frames of the 200 ms tail, numbered from `first_number`: rate // 5 samples as whole blocks of `n` and one
    shorter last block (the last block of a fixed-blocksize stream may be shorter)"""
    total, out, number = int(rate) // 5, b"", int(first_number)
    while total > 0:
        m = min(int(n), total)
        out += silent_frame(number, m, rate)
        number, total = number + 1, total - m
    return out


def silence_frames(rate: int, n: int) -> int:
    """how many frames `silence` makes"""
    return -(-(int(rate) // 5) // int(n))


def stream_header(rate: int, n: int, total_samples: int = 0) -> bytes:
    """`fLaC`, one last-metadata-block header (0x80, length 34) and the STREAMINFO: both block sizes `n`, both frame sizes 0
    (unknown), 20-bit rate, 3-bit channels - 1 = 0, 5-bit bits - 1 = 15, 36-bit total samples (0: unknown), all-zero MD5"""
    rate, n, total = int(rate), int(n), int(total_samples)
    if not MIN_N <= n <= 65535 or not 1 <= rate < 1 << 20 or not 0 <= total < 1 << 36:
        raise ValueError(f"stream header: block size {n}, rate {rate} or total {total} out of range")
    packed = (rate << 44) | (0 << 41) | (15 << 36) | total
    info = n.to_bytes(2, "big") * 2 + b"\x00" * 6 + packed.to_bytes(8, "big") + b"\x00" * 16
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + info


TOTAL_SAMPLES_AT = 4 + 4 + 10 + 3  # the byte of `stream_header` whose low nibble begins the 36-bit total sample count


def patch_total(header: bytes, total_samples: int) -> bytes:
    """`header` (a `stream_header`) with its total sample count replaced"""
    total = int(total_samples)
    if not 0 <= total < 1 << 36:
        raise ValueError(f"total samples {total} do not fit 36 bits")
    h = bytearray(header)
    at = TOTAL_SAMPLES_AT
    h[at] = (h[at] & 0xF0) | (total >> 32)
    h[at + 1:at + 5] = (total & 0xFFFFFFFF).to_bytes(4, "big")
    return bytes(h)
