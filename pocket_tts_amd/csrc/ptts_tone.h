// Per-request tone (a cascade of biquad sections): the output stage between the pitcher and the normaliser.  What the kernel
// (ptts_tone.hip) and a plain C++ program (the sweep of tests/test_tone_cpu.py, compiled with a host sanitizer) share.
// Ordinary C++: compiles with g++ as well as under hipcc.
//
// A plan is (rate, n, K): K <= PTTS_TN_MAX_SECTIONS sections of five float64 coefficients (b0 b1 b2 a1 a2, a0 = 1) and, per
// section, the scan's PTTS_TN_SCAN matrix powers A^(chunk 2^j) of its 2 x 2 state transition (contract and plan rule:
// pocket_tts_amd/tone.py).  A row carries its sections' states, 2 K doubles, from frame to frame; nothing else.
#pragma once
#include <stdint.h>

#include "ptts_scan.h"

#if defined(__HIPCC__)
#define PTTS_TN_HD __host__ __device__
#else
#define PTTS_TN_HD
#endif

#define PTTS_TN_MIN_RATE 8000
#define PTTS_TN_MAX_RATE 48000
#define PTTS_TN_MAX_N 8192        // largest frame
#define PTTS_TN_THREADS 1024      // threads of the workgroup: one chunk of the frame each
#define PTTS_TN_SCAN 10           // scan steps: 2^PTTS_TN_SCAN == PTTS_TN_THREADS
#define PTTS_TN_MAX_CHUNK (PTTS_TN_MAX_N / PTTS_TN_THREADS)  // 8 samples
#define PTTS_TN_MAX_SECTIONS 8
#define PTTS_TN_COEFS 5
#define PTTS_TN_PLAN_INTS 3       // rate, n, K
#define PTTS_TN_PLAN_DOUBLES (PTTS_TN_MAX_SECTIONS * PTTS_TN_COEFS + PTTS_TN_MAX_SECTIONS * PTTS_TN_SCAN * 4)
#define PTTS_TN_ROW_DOUBLES (2 * PTTS_TN_MAX_SECTIONS)  // a row's carried state: s[k][0], s[k][1]

struct TnPlan {
  int32_t rate, n, K, chunk, threads, pad;
  double coef[PTTS_TN_MAX_SECTIONS][PTTS_TN_COEFS];   // b0 b1 b2 a1 a2 of section k
  double pw[PTTS_TN_MAX_SECTIONS][PTTS_TN_SCAN][4];   // A_k^(chunk 2^j), row-major 2 x 2
};

// The admission rules, as the library applies them before a plan reaches the device (tone.py applies the same ones with a
// message per rule, and the grammar's on top).
PTTS_TN_HD inline bool tn_plan_ok(int rate, int n, int K) {
  if (rate < PTTS_TN_MIN_RATE || rate > PTTS_TN_MAX_RATE) return false;
  return n >= 1 && n <= PTTS_TN_MAX_N && K >= 1 && K <= PTTS_TN_MAX_SECTIONS;
}
// The frame's partition over the threads (ptts_scan.h): chunk <= PTTS_TN_MAX_CHUNK, scan_steps <= PTTS_TN_SCAN
PTTS_TN_HD inline int tn_chunk(int n) { return scan_chunk(n, PTTS_TN_THREADS); }
PTTS_TN_HD inline int tn_threads(int n) { return scan_threads(n, PTTS_TN_THREADS); }
PTTS_TN_HD inline int tn_begin(int t, int chunk) { return scan_begin(t, chunk); }
PTTS_TN_HD inline int tn_end(int t, int chunk, int n) { return scan_end(t, chunk, n); }
PTTS_TN_HD inline int tn_steps(int threads) { return scan_steps(threads); }

// One sample of one section in transposed direct form II.  Returns y.
PTTS_TN_HD inline double tn_step(const double *c, double *s, double x) {
  const double y = c[0] * x + s[0];
  s[0] = c[1] * x - c[3] * y + s[1];
  s[1] = c[2] * x - c[4] * y;
  return y;
}
// acc += M v for a row-major 2 x 2 matrix, the columns in ascending order
PTTS_TN_HD inline void tn_mat_acc(const double *M, const double *v, double *acc) {
  acc[0] += M[0] * v[0] + M[1] * v[1];
  acc[1] += M[2] * v[0] + M[3] * v[1];
}
// Section k of a plan as the chunked scan's recurrence (ptts_scan.h): c = coef[k], pw = pw[k]
struct TnSection {
  static constexpr int W = 2;
  double c[PTTS_TN_COEFS];
  const double *pw;  // [PTTS_TN_SCAN][4]
  PTTS_TN_HD double step(double *s, double x) const { return tn_step(c, s, x); }
  PTTS_TN_HD void join(int j, const double *e, double *s) const { tn_mat_acc(pw + 4 * j, e, s); }
};
