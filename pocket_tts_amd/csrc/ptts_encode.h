// Per-request output encoding: the last output stage, behind whichever stage ended the chain before it.  What the kernel
// (ptts_encode.hip) and a plain C++ program (the sweep of tests/test_encoding_cpu.py) share.  Ordinary C++: compiles with g++
// as well as under hipcc.  Contract: pocket_tts_amd/encoding.py.
//
//   code 0  pcm_s16le  s = (int16)(clamp(x, -1, 1) * 32767.0f), truncated: the conversion of every stage's 16-bit output
//   code 1  pcm_f32le  the four bytes of x
//   code 2  mulaw      ITU-T G.711 mu-law of the 14-bit value s >> 2
//   code 3  alaw       ITU-T G.711 A-law of the 13-bit value s >> 3
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PTTS_EN_HD __host__ __device__
#else
#define PTTS_EN_HD
#endif

#define PTTS_EN_CODES 4  // encodings: codes 0 .. 3
#define PTTS_EN_RUN 16   // consecutive samples of a row that one lane converts: 16 / 32 / 64 bytes of output

// bytes per sample of a code in [0, PTTS_EN_CODES): 2, 4, 1, 1
PTTS_EN_HD inline int en_bps(int code) { return code == 0 ? 2 : code == 1 ? 4 : 1; }
// bytes between two rows of the output: the widest encoding of a whole line, rounded up to a 16-byte store
PTTS_EN_HD inline int64_t en_pitch(int width) { return ((int64_t)4 * width + 15) / 16 * 16; }

// the 16-bit sample of x: fmaxf drops a NaN for -1, as in every stage's own 16-bit output
PTTS_EN_HD inline int en_s16(float x) { return (int)(int16_t)(fminf(fmaxf(x, -1.0f), 1.0f) * 32767.0f); }

// number of leading zeros of v != 0
PTTS_EN_HD inline int en_clz(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __clz((int)v);
#else
  return __builtin_clz(v);
#endif
}

// mu-law of the 16-bit sample s.  The 14-bit magnitude m <= 8192 plus the bias 33 lies in [33, 8225]: segment e is the
// position of its leading one above bit 5 (chord e holds [2^(e + 5), 2^(e + 6))), the mantissa the four bits below that one;
// 8224 and 8225 (|s| >= 32764) are past the last chord and saturate at its last step.  All eight bits are inverted.
PTTS_EN_HD inline uint8_t en_mulaw(int s) {
  const int v = s >> 2;
  const uint32_t m = (uint32_t)(v < 0 ? -v : v) + 33u;
  const int e = 26 - en_clz(m);  // 0 .. 8
  const uint32_t code = e > 7 ? 0x7Fu : ((uint32_t)e << 4) | ((m >> (e + 1)) & 0xFu);
  return (uint8_t)(code ^ (v < 0 ? 0x7Fu : 0xFFu));
}

// A-law of the 16-bit sample s.  The 13-bit magnitude m (|v| for v >= 0, |v| - 1 below: 0 .. 4095) is linear over [0, 32) in
// steps of 2 (segment 0) and [32, 64) likewise (segment 1); from there segment e holds [2^(e + 4), 2^(e + 5)) in 16 steps.
// Even bits are inverted (0x55), the sign bit is set for v >= 0.
PTTS_EN_HD inline uint8_t en_alaw(int s) {
  const int v = s >> 3;
  const uint32_t m = (uint32_t)(v < 0 ? -v - 1 : v);
  const int e = m < 32u ? 0 : 27 - en_clz(m);  // 0 .. 7
  const uint32_t code = ((uint32_t)e << 4) | ((m >> (e < 2 ? 1 : e)) & 0xFu);
  return (uint8_t)(code ^ (v < 0 ? 0x55u : 0xD5u));
}

// A row of n samples (1 <= n <= width) is walked in runs of PTTS_EN_RUN: run r covers samples [16 r, 16 r + 16).
//   en_runs(width)     runs a row of the widest line has: the grid's extent
//   en_full(r, n)      the whole run lies inside the row: 16 r + 16 <= n, so its loads end at sample n - 1 <= width - 1 and its
//                      stores at byte (16 r + 16) bps <= n bps <= 4 width <= pitch of the row
//   en_tail(r, n)      samples of a run that is not full: n - 16 r in [1, 15], or <= 0 for a run past the row's end
PTTS_EN_HD inline int en_runs(int width) { return (width + PTTS_EN_RUN - 1) / PTTS_EN_RUN; }
PTTS_EN_HD inline bool en_full(int r, int n) { return PTTS_EN_RUN * r + PTTS_EN_RUN <= n; }
PTTS_EN_HD inline int en_tail(int r, int n) { return n - PTTS_EN_RUN * r; }
