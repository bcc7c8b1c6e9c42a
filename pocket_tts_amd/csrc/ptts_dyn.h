// Per-request dynamics (a feed-forward speech compressor): the output stage between the toner and the normaliser.  What the
// kernel (ptts_dyn.hip) and a plain C++ program (the sweep of tests/test_dynamics_cpu.py, compiled with a host sanitizer)
// share.  Ordinary C++: compiles with g++ as well as under hipcc.
//
// A plan is (rate, n) with the curve's T, k = 1 - 1 / ratio and W, the make-up M, the per-sample decays aA and aR and, for
// the two scans, the PTTS_DY_SCAN powers aA^(chunk 2^j) and aR^(chunk 2^j) (contract and plan rule:
// pocket_tts_amd/dynamics.py).  A row carries two doubles, p and s, from frame to frame; nothing else.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ptts_scan.h"

#if defined(__HIPCC__)
#define PTTS_DY_HD __host__ __device__
#else
#define PTTS_DY_HD
#endif

#define PTTS_DY_MIN_RATE 8000
#define PTTS_DY_MAX_RATE 48000
#define PTTS_DY_MAX_N 8192        // largest frame
#define PTTS_DY_THREADS 1024      // threads of the workgroup: one chunk of the frame each
#define PTTS_DY_SCAN 10           // scan steps: 2^PTTS_DY_SCAN == PTTS_DY_THREADS
#define PTTS_DY_MAX_CHUNK (PTTS_DY_MAX_N / PTTS_DY_THREADS)  // 8 samples
#define PTTS_DY_PLAN_INTS 2       // rate, n
#define PTTS_DY_PLAN_DOUBLES (6 + 2 * PTTS_DY_SCAN)  // T k W M aA aR, the powers of aA, the powers of aR
#define PTTS_DY_ROW_DOUBLES 2     // a row's carried state: p, s
#define PTTS_DY_K 0.11512925464970229  // dB to nepers: the double that log(10.0) / 20.0 gives, as dynamics.py computes it
#define PTTS_DY_A_MIN 1e-6        // the clamp of |x|: -120 dBFS ..
#define PTTS_DY_A_MAX 1e6         // .. 120 dBFS

struct DyPlan {
  int32_t rate, n, chunk, threads;
  double T, k, W, M, aA, aR;
  double pwA[PTTS_DY_SCAN];  // aA^(chunk 2^j)
  double pwR[PTTS_DY_SCAN];  // aR^(chunk 2^j)
};

// The admission rules, as the library applies them before a plan reaches the device (dynamics.py applies the same ones
// with a message per rule, and the grammar's on top).
PTTS_DY_HD inline bool dyn_plan_ok(int rate, int n) {
  if (rate < PTTS_DY_MIN_RATE || rate > PTTS_DY_MAX_RATE) return false;
  return n >= 1 && n <= PTTS_DY_MAX_N;
}
// The ranges of the grammar for a plan's values.  The curve is total, so the kernel is safe with any finite value; these
// keep a caller of the C ABI from handing over an expander (k < 0) or a decay that grows (a >= 1).
PTTS_DY_HD inline bool dyn_values_ok(double T, double k, double W, double M, double aA, double aR) {
  return T >= -60.0 && T <= 0.0 && k >= 0.0 && k < 1.0 && W >= 0.0 && W <= 24.0 && M >= 0.0 && M <= 24.0 && aA > 0.0 &&
         aA < 1.0 && aR > 0.0 && aR < 1.0;
}
// The frame's partition over the threads (ptts_scan.h): chunk <= PTTS_DY_MAX_CHUNK, scan_steps <= PTTS_DY_SCAN
PTTS_DY_HD inline int dy_chunk(int n) { return scan_chunk(n, PTTS_DY_THREADS); }
PTTS_DY_HD inline int dy_threads(int n) { return scan_threads(n, PTTS_DY_THREADS); }
PTTS_DY_HD inline int dy_begin(int t, int chunk) { return scan_begin(t, chunk); }
PTTS_DY_HD inline int dy_end(int t, int chunk, int n) { return scan_end(t, chunk, n); }
PTTS_DY_HD inline int dy_steps(int threads) { return scan_steps(threads); }

// |x| in dBFS, clamped to [-120, 120]; a NaN compares false and is the floor
PTTS_DY_HD inline double dy_level(double x) {
  double a = fabs(x);
  a = a > PTTS_DY_A_MIN ? a : PTTS_DY_A_MIN;
  a = a < PTTS_DY_A_MAX ? a : PTTS_DY_A_MAX;
  return log(a) / PTTS_DY_K;
}
// The static curve: the wanted reduction in dB, >= 0, of a sample at L dBFS
PTTS_DY_HD inline double dy_curve(double L, double T, double k, double W) {
  const double d = L - T;
  if (2.0 * d <= -W) return 0.0;
  if (2.0 * d < W) return k * (d + W / 2.0) * (d + W / 2.0) / (2.0 * W);
  return k * d;
}
// The two recurrences, one sample each: the peak detector (instant rise, release decay) and the attack smoothing
PTTS_DY_HD inline double dy_peak(double c, double aR, double p) {
  const double q = aR * p;
  return c > q ? c : q;
}
PTTS_DY_HD inline double dy_smooth(double p, double aA, double s) { return aA * s + (1.0 - aA) * p; }
// The two as the chunked scan's recurrences (ptts_scan.h): max-plus with pw = pwR, linear with pw = pwA
struct DyPeak {
  static constexpr int W = 1;
  double aR;
  const double *pw;  // [PTTS_DY_SCAN]
  PTTS_DY_HD double step(double *s, double c) const { return s[0] = dy_peak(c, aR, s[0]); }
  PTTS_DY_HD void join(int j, const double *e, double *s) const { s[0] = dy_peak(s[0], pw[j], e[0]); }
};
struct DySmooth {
  static constexpr int W = 1;
  double aA;
  const double *pw;  // [PTTS_DY_SCAN]
  PTTS_DY_HD double step(double *s, double p) const { return s[0] = dy_smooth(p, aA, s[0]); }
  PTTS_DY_HD void join(int j, const double *e, double *s) const { s[0] += pw[j] * e[0]; }
};
// The gain of a sample whose smoothed reduction is s dB
PTTS_DY_HD inline double dy_gain(double M, double s) { return exp((M - s) * PTTS_DY_K); }
// One sample of the serial definition.  st = {p, s}; returns y.
PTTS_DY_HD inline float dy_step(const DyPlan &P, double *st, float x) {
  st[0] = dy_peak(dy_curve(dy_level((double)x), P.T, P.k, P.W), P.aR, st[0]);
  st[1] = dy_smooth(st[0], P.aA, st[1]);
  return (float)(dy_gain(P.M, st[1]) * (double)x);
}
