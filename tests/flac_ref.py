"""Reference FLAC encoder and decoder for the packer's tests (`pocket_tts_amd/flac.py` states the bitstream).

`encode_frame` is written from the contract, with numpy and Python integers.  `decode_frames` / `decode_stream` are written
from the FLAC format rules as a general reader of fixed-blocksize mono 16-bit streams with CONSTANT, VERBATIM and FIXED
subframes and Rice partitions of any order; they share nothing with the encoder but the CRC tables, and raise `FlacError` on
any sync, CRC, reserved-bit or length violation."""

import numpy as np

from pocket_tts_amd.flac import CRC8_TABLE, CRC16_TABLE


# ---- the encoder --------------------------------------------------------------------------------------------------------
def _crc(data, table, bits):
    c = 0
    if bits == 8:
        for b in data:
            c = table[c ^ b]
    else:
        for b in data:
            c = ((c << 8) & 0xFFFF) ^ table[(c >> 8) ^ b]
    return c


_RATE_CODE = {8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10}


def _number(v):
    if v < 0x80:
        return bytes([v])
    for n, lim in ((2, 1 << 11), (3, 1 << 16), (4, 1 << 21), (5, 1 << 26), (6, 1 << 31)):
        if v < lim:
            lead = (0xFF << (8 - n)) & 0xFF
            return bytes([lead | (v >> (6 * (n - 1)))] + [0x80 | ((v >> (6 * i)) & 0x3F) for i in range(n - 2, -1, -1)])
    raise ValueError(v)


def residuals(x, o):
    """e_o[i] for i in [o, n) as int64"""
    e = np.asarray(x, dtype=np.int64)
    for _ in range(o):
        e = np.diff(e)
    return e


def choose(x):
    """("constant" | "verbatim" | "fixed", o, k, bits) by the contract's rule"""
    x = np.asarray(x, dtype=np.int64)
    n = len(x)
    if np.all(x == x[0]):
        return "constant", 0, 0, 16
    best = None
    for o in range(5):
        e = residuals(x, o)
        u = (e << 1) ^ (e >> 63)
        for k in range(15):
            bits = 16 * o + 10 + int(np.sum((u >> k) + 1 + k))
            if best is None or bits < best[2]:
                best = (o, k, bits)
    o, k, bits = best
    return ("verbatim" if bits >= 16 * n else "fixed"), o, k, bits


def encode_frame(x, number, rate):
    """the frame of the int16 block `x` as bytes"""
    x = np.asarray(x)
    assert x.dtype == np.int16 and x.ndim == 1
    n = len(x)
    code = _RATE_CODE.get(rate, 13)
    head = bytes([0xFF, 0xF8, 0x70 | code, 0x08]) + _number(number) + (n - 1).to_bytes(2, "big")
    if code == 13:
        head += rate.to_bytes(2, "big")
    head += bytes([_crc(head, CRC8_TABLE, 8)])
    kind, o, k, _ = choose(x)
    bits = []  # strings of '0' / '1'
    if kind == "constant":
        bits.append("00000000" + format(int(x[0]) & 0xFFFF, "016b"))
    elif kind == "verbatim":
        bits.append("00000010")
        bits.append("".join(format(int(v) & 0xFFFF, "016b") for v in x))
    else:
        bits.append(format(0x10 | (o << 1), "08b"))
        bits.append("".join(format(int(v) & 0xFFFF, "016b") for v in x[:o]))
        bits.append("00" + "0000" + format(k, "04b"))
        e = residuals(x, o)
        u = (e << 1) ^ (e >> 63)
        parts = []
        for v in u.tolist():
            parts.append("0" * (v >> k) + "1" + (format(v & ((1 << k) - 1), f"0{k}b") if k else ""))
        bits.append("".join(parts))
    s = "".join(bits)
    s += "0" * (-len(s) % 8)
    body = head + int(s, 2).to_bytes(len(s) // 8, "big")
    return body + _crc(body, CRC16_TABLE, 16).to_bytes(2, "big")


# ---- the decoder --------------------------------------------------------------------------------------------------------
class FlacError(ValueError):
    pass


class _Bits:
    def __init__(self, data, at):
        self.data, self.pos = data, 8 * at

    def take(self, n):
        v = 0
        for _ in range(n):
            byte = self.pos >> 3
            if byte >= len(self.data):
                raise FlacError("the stream ends inside a frame")
            v = (v << 1) | ((self.data[byte] >> (7 - (self.pos & 7))) & 1)
            self.pos += 1
        return v

    def signed(self, n):
        v = self.take(n)
        return v - (1 << n) if v >> (n - 1) else v

    def unary(self):
        q = 0
        while self.take(1) == 0:
            q += 1
        return q


def _check8(data):
    c = 0
    for b in data:
        c = CRC8_TABLE[c ^ b]
    return c


def _check16(data):
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ CRC16_TABLE[(c >> 8) ^ b]
    return c


_BLOCK = {1: 192, 2: 576, 3: 1152, 4: 2304, 5: 4608, 8: 256, 9: 512, 10: 1024, 11: 2048, 12: 4096, 13: 8192, 14: 16384, 15: 32768}
_RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}
_FIXED = {0: (), 1: (1,), 2: (2, -1), 3: (3, -3, 1), 4: (4, -6, 4, -1)}


def _read_number(data, at):
    if at >= len(data):
        raise FlacError("the stream ends inside a frame header")
    b0 = data[at]
    if b0 < 0x80:
        return b0, 1
    n = 0
    while n < 8 and (b0 << n) & 0x80:
        n += 1
    if n < 2 or n > 7:
        raise FlacError("bad first byte of a coded number")
    v = b0 & (0x7F >> n)
    if at + n > len(data):
        raise FlacError("the stream ends inside a coded number")
    for i in range(1, n):
        c = data[at + i]
        if c & 0xC0 != 0x80:
            raise FlacError("bad continuation byte of a coded number")
        v = (v << 6) | (c & 0x3F)
    return v, n


def decode_frame(data, at=0, stream_rate=None):
    """One frame of `data` from byte `at`: (samples int16, number, rate, blocksize, bytes consumed, subframe kind)"""
    if at + 4 > len(data):
        raise FlacError("the stream ends inside a frame header")
    if data[at] != 0xFF or data[at + 1] & 0xFC != 0xF8:
        raise FlacError(f"no sync code at byte {at}")
    if data[at + 1] & 0x02:
        raise FlacError("reserved bit set in the frame header")
    if data[at + 1] & 0x01:
        raise FlacError("variable-blocksize frame in a fixed-blocksize stream")
    bcode, rcode = data[at + 2] >> 4, data[at + 2] & 0x0F
    ch, scode, rsv = data[at + 3] >> 4, (data[at + 3] >> 1) & 7, data[at + 3] & 1
    if rsv:
        raise FlacError("reserved bit set in the frame header")
    if bcode == 0 or rcode == 15 or scode in (3, 7):
        raise FlacError("reserved code in the frame header")
    if ch != 0:
        raise FlacError("not a mono frame")
    bps = {0: None, 1: 8, 2: 12, 4: 16, 5: 20, 6: 24}[scode]
    if bps != 16:
        raise FlacError("not a 16-bit frame")
    p = at + 4
    number, used = _read_number(data, p)
    p += used
    if bcode == 6:
        n, p = data[p] + 1, p + 1
    elif bcode == 7:
        if p + 2 > len(data):
            raise FlacError("the stream ends inside a frame header")
        n, p = int.from_bytes(data[p:p + 2], "big") + 1, p + 2
    else:
        n = _BLOCK[bcode]
    if rcode == 0:
        rate = stream_rate
    elif rcode == 12:
        rate, p = data[p] * 1000, p + 1
    elif rcode == 13:
        rate, p = int.from_bytes(data[p:p + 2], "big"), p + 2
    elif rcode == 14:
        rate, p = int.from_bytes(data[p:p + 2], "big") * 10, p + 2
    else:
        rate = _RATES[rcode]
    if p >= len(data):
        raise FlacError("the stream ends inside a frame header")
    if _check8(data[at:p]) != data[p]:
        raise FlacError("frame header CRC-8 mismatch")
    bits = _Bits(data, p + 1)
    if bits.take(1):
        raise FlacError("subframe padding bit set")
    kind = bits.take(6)
    if bits.take(1):
        raise FlacError("wasted bits are not expected in this stream")
    if kind == 0:
        out, name = [bits.signed(16)] * n, "constant"
    elif kind == 1:
        out, name = [bits.signed(16) for _ in range(n)], "verbatim"
    elif 8 <= kind <= 12:
        order, name = kind - 8, "fixed"
        if order > n:
            raise FlacError("predictor order above the blocksize")
        out = [bits.signed(16) for _ in range(order)]
        method = bits.take(2)
        if method > 1:
            raise FlacError("reserved residual coding method")
        pbits, escape = (4, 15) if method == 0 else (5, 31)
        porder = bits.take(4)
        parts = 1 << porder
        if n % parts or (n >> porder) < order and porder:
            raise FlacError("partition order does not fit the blocksize")
        coef = _FIXED[order]
        for part in range(parts):
            count = (n >> porder) - (order if part == 0 else 0)
            if count < 0:
                raise FlacError("partition shorter than the predictor order")
            k = bits.take(pbits)
            raw = bits.take(5) if k == escape else None
            for _ in range(count):
                if raw is not None:
                    e = bits.signed(raw) if raw else 0
                else:
                    u = (bits.unary() << k) | (bits.take(k) if k else 0)
                    e = (u >> 1) ^ -(u & 1)
                out.append(e + sum(c * out[-1 - j] for j, c in enumerate(coef)))
    else:
        raise FlacError(f"subframe type {kind} is reserved or not supported")
    if len(out) != n:
        raise FlacError("subframe length is not the blocksize")
    while bits.pos & 7:
        if bits.take(1):
            raise FlacError("non-zero padding before the frame CRC")
    end = bits.pos >> 3
    if end + 2 > len(data):
        raise FlacError("the stream ends before the frame CRC")
    if _check16(data[at:end]) != int.from_bytes(data[end:end + 2], "big"):
        raise FlacError("frame CRC-16 mismatch")
    arr = np.array(out, dtype=np.int64)
    if arr.min() < -32768 or arr.max() > 32767:
        raise FlacError("sample out of the 16-bit range")
    return arr.astype(np.int16), number, rate, n, end + 2 - at, name


def decode_frames(data, stream_rate=None):
    """every frame of `data`, which must hold whole frames only: [(samples, number, rate, blocksize, nbytes, kind)]"""
    data, at, out = bytes(data), 0, []
    while at < len(data):
        f = decode_frame(data, at, stream_rate)
        out.append(f)
        at += f[4]
    return out


def decode_stream(data):
    """A whole stream: (samples int16, rate, info) with info = dict(block, total, frames=[...]).  Checks the marker, the
    STREAMINFO, consecutive frame numbers, the fixed blocksize (only the last frame may be shorter), each frame's rate and,
    where STREAMINFO gives it, the total"""
    data = bytes(data)
    if data[:4] != b"fLaC":
        raise FlacError("no fLaC marker")
    at, info, last = 4, None, False
    while not last:
        if at + 4 > len(data):
            raise FlacError("the stream ends inside the metadata")
        last, kind, size = bool(data[at] & 0x80), data[at] & 0x7F, int.from_bytes(data[at + 1:at + 4], "big")
        if kind == 127:
            raise FlacError("invalid metadata block type")
        body = data[at + 4:at + 4 + size]
        if len(body) != size:
            raise FlacError("the stream ends inside the metadata")
        if kind == 0:
            if info is not None or size != 34 or at != 4:
                raise FlacError("bad STREAMINFO")
            packed = int.from_bytes(body[10:18], "big")
            info = dict(min_block=int.from_bytes(body[0:2], "big"), block=int.from_bytes(body[2:4], "big"),
                        min_frame=int.from_bytes(body[4:7], "big"), max_frame=int.from_bytes(body[7:10], "big"),
                        rate=packed >> 44, channels=((packed >> 41) & 7) + 1, bits=((packed >> 36) & 31) + 1,
                        total=packed & ((1 << 36) - 1), md5=body[18:34])
        at += 4 + size
    if info is None:
        raise FlacError("no STREAMINFO")
    if info["channels"] != 1 or info["bits"] != 16 or info["min_block"] != info["block"] or info["block"] < 16:
        raise FlacError("STREAMINFO is not that of a fixed-blocksize mono 16-bit stream")
    frames = decode_frames(data[at:], info["rate"])
    for i, f in enumerate(frames):
        if f[1] != i:
            raise FlacError(f"frame {i} carries the number {f[1]}")
        if f[2] != info["rate"]:
            raise FlacError("a frame's rate is not the stream's")
        if f[3] != info["block"] and not (i == len(frames) - 1 and f[3] < info["block"]):
            raise FlacError("a frame's blocksize is not the stream's")
    pcm = np.concatenate([f[0] for f in frames]) if frames else np.zeros(0, np.int16)
    if info["total"] and info["total"] != len(pcm):
        raise FlacError("STREAMINFO's total is not the number of samples")
    info["frames"] = frames
    return pcm, info["rate"], info
