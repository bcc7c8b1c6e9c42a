// Per-request FLAC output: the packer, the link behind the encoder.  What the kernel (ptts_flac.hip) and a plain C++ program
// (tests/cpp/flac_sweep.cpp) share.  Ordinary C++: compiles with g++ as well as under hipcc.  Contract: pocket_tts_amd/flac.py.
//
// A block is n int16 samples x (16 <= n <= 4608), mono, 16 bits, in a fixed-blocksize stream.
//
//   frame header   FF F8 | 0111 ssss | 08 | frame number, UTF-8-like, 1 .. 6 bytes | n - 1 as 16 bits | the rate in Hz as 16
//                  bits where ssss = 1101 | CRC-8 (0x07, initial value 0) of all that
//                  ssss: 8000 0100, 16000 0101, 22050 0110, 24000 0111, 32000 1000, 44100 1001, 48000 1010, any other 1101
//   subframe       all samples equal: CONSTANT, 00 and the value as 16 bits.  Else for the fixed predictors o = 0 .. 4 with
//                  residuals e_o[i], i in [o, n), folded u = (e << 1) ^ (e >> 31), and the Rice parameters k = 0 .. 14:
//                  bits(o, k) = 16 o + 10 + sum((u >> k) + 1 + k); the smallest wins, ties to the smaller o, then the smaller k.
//                  Smallest >= 16 n: VERBATIM, 02 and n samples of 16 bits.  Else FIXED: 0x10 | o << 1, o warm-up samples of 16
//                  bits, 00 (4-bit parameters) 0000 (partition order 0) kkkk, and per residual u >> k zero bits, a one bit and
//                  the low k bits of u, most significant first.  All multi-bit values are big-endian.
//   footer         zero bits to the byte boundary, CRC-16 (0x8005, initial value 0, not reflected, big-endian) of the whole frame
//
// The sums of bits(o, k) need 64 bits: at k = 0 one residual can be 2^20 and 4608 of them pass 2^32.  A lane's own partial
// sum (at most 18 residuals of a 256-lane block) and a wave's (64 lanes) stay below 2^32.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PTTS_FL_HD __host__ __device__
#else
#define PTTS_FL_HD
#endif

#define PTTS_FL_MIN_N 16      // the FLAC subset's block sizes up to 48 kHz
#define PTTS_FL_MAX_N 4608
#define PTTS_FL_ORDERS 5      // fixed predictors 0 .. 4
#define PTTS_FL_KS 15         // Rice parameters 0 .. 14 (15 is the escape code of 4-bit parameters)
#define PTTS_FL_SUMS (PTTS_FL_ORDERS * PTTS_FL_KS)
#define PTTS_FL_PREFIX 16     // bytes of a ring line's prefix {u32 nbytes, 0, 0, 0}
#define PTTS_FL_HEADER_MAX 15 // 2 sync + 1 + 1 + 6 number + 2 blocksize + 2 rate + 1 CRC-8
#define PTTS_FL_LANES 256     // lanes that share a block: the kernel's workgroup

enum { PTTS_FL_CONSTANT = 0, PTTS_FL_VERBATIM = 1, PTTS_FL_FIXED = 2 };

// the largest frame of n samples: header, verbatim subframe (1 + 2 n), CRC-16
PTTS_FL_HD inline int fl_frame_max(int n) { return PTTS_FL_HEADER_MAX + 1 + 2 * n + 2; }
// bytes between two rows of the packer's ring: the prefix, then the widest pass-through line (4 bytes a sample) or the
// largest frame, rounded up to a 16-byte store
PTTS_FL_HD inline int64_t fl_pitch(int width) {
  const int64_t a = (int64_t)4 * width, b = (int64_t)2 * width + 18;
  return PTTS_FL_PREFIX + ((a > b ? a : b) + 15) / 16 * 16;
}

PTTS_FL_HD inline uint32_t fl_fold(int32_t e) { return ((uint32_t)e << 1) ^ (uint32_t)(e >> 31); }

// the residual of predictor o at sample i >= o; |e| <= 16 * 32768
PTTS_FL_HD inline int32_t fl_resid(const int32_t *x, int i, int o) {
  switch (o) {
    case 0: return x[i];
    case 1: return x[i] - x[i - 1];
    case 2: return x[i] - 2 * x[i - 1] + x[i - 2];
    case 3: return x[i] - 3 * x[i - 1] + 3 * x[i - 2] - x[i - 3];
    default: return x[i] - 4 * x[i - 1] + 6 * x[i - 2] - 4 * x[i - 3] + x[i - 4];
  }
}

// bits(o, k) from sum = the sum of u >> k over the n - o residuals
PTTS_FL_HD inline uint64_t fl_bits(int o, int k, int n, uint64_t sum) {
  return (uint64_t)(16 * o + 10) + sum + (uint64_t)(n - o) * (uint64_t)(1 + k);
}

// the subframe of a block that is not constant, from sums[o * PTTS_FL_KS + k]; *o and *k are the winner's (also for VERBATIM)
PTTS_FL_HD inline int fl_choose(const uint64_t *sums, int n, int *o, int *k) {
  uint64_t best = ~(uint64_t)0;
  *o = *k = 0;
  for (int oo = 0; oo < PTTS_FL_ORDERS; ++oo)
    for (int kk = 0; kk < PTTS_FL_KS; ++kk) {
      const uint64_t b = fl_bits(oo, kk, n, sums[oo * PTTS_FL_KS + kk]);
      if (b < best) { best = b; *o = oo; *k = kk; }  // strictly smaller: ties stay with the smaller o, then the smaller k
    }
  return best >= (uint64_t)16 * n ? PTTS_FL_VERBATIM : PTTS_FL_FIXED;
}

// ---- CRCs: byte-wise from 256-entry tables that the user fills once -----------------------------------------------------
PTTS_FL_HD inline uint8_t fl_crc8_entry(int b) {
  uint32_t c = (uint32_t)b;
  for (int i = 0; i < 8; ++i) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) : (c << 1);
  return (uint8_t)c;
}
PTTS_FL_HD inline uint16_t fl_crc16_entry(int b) {
  uint32_t c = (uint32_t)b << 8;
  for (int i = 0; i < 8; ++i) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) : (c << 1);
  return (uint16_t)c;
}
PTTS_FL_HD inline uint8_t fl_crc8(const uint8_t *t8, uint8_t crc, uint8_t byte) { return t8[crc ^ byte]; }
PTTS_FL_HD inline uint16_t fl_crc16(const uint16_t *t16, uint16_t crc, uint8_t byte) {
  return (uint16_t)((crc << 8) ^ t16[((crc >> 8) ^ byte) & 0xFF]);
}
// a(x) b(x) mod x^16 + x^15 + x^2 + 1
PTTS_FL_HD inline uint16_t fl_gfmul16(uint16_t a, uint16_t b) {
  uint32_t r = 0;
  for (int i = 15; i >= 0; --i) {
    r = (r & 0x8000u) ? ((r << 1) ^ 0x8005u) : (r << 1);
    if ((b >> i) & 1u) r ^= a;
  }
  return (uint16_t)r;
}
// x^(8 m) mod the CRC-16 polynomial.  With initial value 0 and no final XOR the CRC is linear, so for a message A | B of
// which B has m bytes: crc(A | B) = fl_gfmul16(crc(A), fl_xpow8(m)) ^ crc(B)
PTTS_FL_HD inline uint16_t fl_xpow8(uint32_t m) {
  uint16_t r = 1, p = 0x0100;  // x^8
  for (; m; m >>= 1) {
    if (m & 1u) r = fl_gfmul16(r, p);
    p = fl_gfmul16(p, p);
  }
  return r;
}

// ---- the frame header -------------------------------------------------------------------------------------------------
PTTS_FL_HD inline int fl_rate_code(int rate) {
  return rate == 8000 ? 4 : rate == 16000 ? 5 : rate == 22050 ? 6 : rate == 24000 ? 7 : rate == 32000 ? 8 : rate == 44100 ? 9
         : rate == 48000 ? 10 : 13;
}
// FLAC's UTF-8-like coding of v < 2^31 into 1 .. 6 bytes; returns the length
PTTS_FL_HD inline int fl_utf8(uint32_t v, uint8_t *out) {
  if (v < 0x80u) { out[0] = (uint8_t)v; return 1; }
  int len = v < 0x800u ? 2 : v < 0x10000u ? 3 : v < 0x200000u ? 4 : v < 0x4000000u ? 5 : 6;
  out[0] = (uint8_t)((0xFF00u >> len) | (v >> (6 * (len - 1))));
  for (int i = 1; i < len; ++i) out[i] = (uint8_t)(0x80u | ((v >> (6 * (len - 1 - i))) & 0x3Fu));
  return len;
}
// the header of frame `number` with its CRC-8 into h[PTTS_FL_HEADER_MAX]; returns its length
PTTS_FL_HD inline int fl_header(uint8_t *h, uint32_t number, int n, int rate, const uint8_t *t8) {
  const int code = fl_rate_code(rate);
  int len = 0;
  h[len++] = 0xFF; h[len++] = 0xF8;
  h[len++] = (uint8_t)(0x70 | code);
  h[len++] = 0x08;
  len += fl_utf8(number, h + len);
  h[len++] = (uint8_t)((n - 1) >> 8); h[len++] = (uint8_t)((n - 1) & 0xFF);
  if (code == 13) { h[len++] = (uint8_t)((rate >> 8) & 0xFF); h[len++] = (uint8_t)(rate & 0xFF); }
  uint8_t crc = 0;
  for (int i = 0; i < len; ++i) crc = fl_crc8(t8, crc, h[i]);
  h[len++] = crc;
  return len;
}

// ---- bit positions ----------------------------------------------------------------------------------------------------
// The frame is built in 32-bit words, most significant bit first: bit p of the stream is bit 31 - (p & 31) of word p >> 5,
// and byte j is bits [24 - 8 (j & 3), +8) of word j >> 2.
// The L <= 32 low bits of v at stream position p: word index *w gets *m0, word *w + 1 gets *m1, which is 0 where the value
// ends inside word *w.  A word whose mask is 0 must not be touched: it can lie behind the buffer.
PTTS_FL_HD inline void fl_split(uint32_t p, uint32_t v, int L, uint32_t *w, uint32_t *m0, uint32_t *m1) {
  const int room = 32 - (int)(p & 31u);
  *w = p >> 5;
  if (L < 32) v &= (1u << L) - 1u;
  if (L <= room) { *m0 = L == 32 ? v : v << (room - L); *m1 = 0; }
  else { const int r = L - room; *m0 = v >> r; *m1 = v << (32 - r); }
}
PTTS_FL_HD inline uint8_t fl_byte(const uint32_t *words, uint32_t j) { return (uint8_t)(words[j >> 2] >> (24 - 8 * (j & 3u))); }
// the Rice code of u under k without its leading zeros: they are `*zeros` bits the zeroed buffer already holds, then the
// L = k + 1 bits of v, a one and the low k bits of u
PTTS_FL_HD inline void fl_code(uint32_t u, int k, uint32_t *zeros, uint32_t *v, int *L) {
  *zeros = u >> k;
  *v = (1u << k) | (u & ((1u << k) - 1u));
  *L = k + 1;
}
// where the residual codes begin in a FIXED subframe behind a header of hlen bytes: subframe byte, o warm-up samples, 10 bits
PTTS_FL_HD inline uint32_t fl_codes_at(int hlen, int o) { return 8u * (uint32_t)hlen + 8u + 16u * (uint32_t)o + 10u; }
// lane t of PTTS_FL_LANES owns the items [*lo, *hi) of `count`: consecutive ranges of ceil(count / lanes), the last ones empty
PTTS_FL_HD inline void fl_range(int t, int count, int *lo, int *hi) {
  const int per = (count + PTTS_FL_LANES - 1) / PTTS_FL_LANES;
  const int a = t * per, b = a + per;
  *lo = a < count ? a : count;
  *hi = b < count ? b : count;
}
// the block of a row whose samples are cut `off` behind a line's start: sample i is the previous line's [off + i] up to
// n - off, then the current line's
PTTS_FL_HD inline int32_t fl_cut(const int16_t *prev, const int16_t *cur, int n, int off, int i) {
  return off == 0 ? cur[i] : (i < n - off ? prev[off + i] : cur[i - (n - off)]);
}
