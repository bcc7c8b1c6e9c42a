// Per-request loudness target (ITU-R BS.1770-4): the output stage between the pitcher and the leveler.  What the kernel
// (ptts_loud.hip) and a plain C++ program (the index sweep of tests/test_loudness_cpu.py, compiled with a host sanitizer)
// share.  Ordinary C++: compiles with g++ as well as under hipcc.
//
// A plan is (rate, n): S = rate / 10 samples per sub-block, D = 4 S samples of delay, ten K-weighting coefficients and the
// scan's matrix powers (contract and plan rule: pocket_tts_amd/loudness.py).  A row carries, from frame to frame, its filter
// state s[4], the partial sum and the position `pos` of the open sub-block, the number `cnt` of completed sub-blocks, the
// last four sub-block energies, up to PTTS_LD_HIST gating-block energies, the last three gains c and a ring of D delayed
// samples with its head.
#pragma once
#include <stdint.h>

#include "ptts_scan.h"

#if defined(__HIPCC__)
#define PTTS_LD_HD __host__ __device__
#else
#define PTTS_LD_HD
#endif

#define PTTS_LD_MIN_RATE 8000
#define PTTS_LD_MAX_RATE 48000
#define PTTS_LD_MAX_N 8192     // largest frame
#define PTTS_LD_THREADS 1024   // threads of the workgroup: one chunk of the frame each
#define PTTS_LD_SCAN 10        // scan steps: 2^PTTS_LD_SCAN == PTTS_LD_THREADS
#define PTTS_LD_MAX_CHUNK (PTTS_LD_MAX_N / PTTS_LD_THREADS)  // 8 samples
#define PTTS_LD_MAX_D (4 * (PTTS_LD_MAX_RATE / 10))          // 19,200 samples: a row's delay ring
#define PTTS_LD_HIST 1024      // gating-block energies a row keeps
// most sub-blocks a frame can complete: pos <= S - 1, so (pos + n) / S <= (S - 1 + MAX_N) / S <= 1 + 8191 / 800 = 11
#define PTTS_LD_MAX_DONE 11
#define PTTS_LD_SEGS (PTTS_LD_MAX_DONE + 1)  // sub-blocks a frame can touch: the completed ones and the one left open
#define PTTS_LD_CC (3 + PTTS_LD_MAX_DONE)    // gains a frame's output pass can see: three carried, then one per completion
#define PTTS_LD_COEFS 10
#define PTTS_LD_PLAN_DOUBLES (PTTS_LD_COEFS + PTTS_LD_SCAN * 32)

struct LdPlan {
  int32_t rate, n, S, D, chunk, threads;
  double coef[PTTS_LD_COEFS];       // b0 b1 b2 a1 a2 of the shelf, then of the high-pass
  double pw[PTTS_LD_SCAN][32];      // A^(chunk 2^t), row-major: its high part, then its low part (exact power - high)
};

// The admission rules, as the library applies them before a plan reaches the device (loudness.py applies the same ones with
// a message per rule).
PTTS_LD_HD inline bool ld_plan_ok(int rate, int n) {
  if (rate < PTTS_LD_MIN_RATE || rate > PTTS_LD_MAX_RATE) return false;
  return n >= 1 && n <= PTTS_LD_MAX_N;
}
PTTS_LD_HD inline int ld_sub(int rate) { return rate / 10; }                 // 800 <= S <= 4800
PTTS_LD_HD inline int ld_delay(int rate) { return 4 * (rate / 10); }         // 3200 <= D <= PTTS_LD_MAX_D
// The frame's partition over the threads (ptts_scan.h): chunk <= PTTS_LD_MAX_CHUNK, scan_steps <= PTTS_LD_SCAN
PTTS_LD_HD inline int ld_chunk(int n) { return scan_chunk(n, PTTS_LD_THREADS); }
PTTS_LD_HD inline int ld_threads(int n) { return scan_threads(n, PTTS_LD_THREADS); }
PTTS_LD_HD inline int ld_begin(int t, int chunk) { return scan_begin(t, chunk); }
PTTS_LD_HD inline int ld_end(int t, int chunk, int n) { return scan_end(t, chunk, n); }

// One sample of the 4-state recurrence: both biquads in transposed direct form II.  Returns w.
PTTS_LD_HD inline double ld_step(const double *c, double *s, double x) {
  const double v = c[0] * x + s[0];
  s[0] = c[1] * x - c[3] * v + s[1];
  s[1] = c[2] * x - c[4] * v;
  const double w = c[5] * v + s[2];
  s[2] = c[6] * v - c[8] * w + s[3];
  s[3] = c[7] * v - c[9] * w;
  return w;
}
// acc += M v for M = high + low (two row-major 4 x 4 matrices, 32 doubles), the columns in ascending order.  A^k v cancels
// by a factor of about k (the high-pass poles are nearly a double pole), so a power rounded to one double would leave
// k 2^-53 in every state; the low part takes that away.
PTTS_LD_HD inline void ld_mat_acc(const double *M, const double *v, double *acc) {
  for (int r = 0; r < 4; ++r) {
    const double hi = M[4 * r] * v[0] + M[4 * r + 1] * v[1] + M[4 * r + 2] * v[2] + M[4 * r + 3] * v[3];
    const double lo = M[16 + 4 * r] * v[0] + M[16 + 4 * r + 1] * v[1] + M[16 + 4 * r + 2] * v[2] + M[16 + 4 * r + 3] * v[3];
    acc[r] += hi + lo;
  }
}
// The K-weighting as the chunked scan's recurrence (ptts_scan.h)
struct LdWeighting {
  static constexpr int W = 4;
  double c[PTTS_LD_COEFS];
  const double *pw;  // [PTTS_LD_SCAN][32]
  PTTS_LD_HD double step(double *s, double x) const { return ld_step(c, s, x); }
  PTTS_LD_HD void join(int j, const double *e, double *s) const { ld_mat_acc(pw + 32 * j, e, s); }
};

// Sample i of a frame (0 <= i < n) that begins at position pos of the open sub-block (0 <= pos < S) lies in the frame's
// segment ld_seg: 0 <= seg <= (S - 1 + n - 1) / S <= PTTS_LD_MAX_DONE < PTTS_LD_SEGS.  A thread's chunk (<= 8 < S samples)
// touches at most the segments ld_seg(first) and ld_seg(first) + 1.  The frame completes ld_done sub-blocks.
PTTS_LD_HD inline int ld_seg(int pos, int i, int S) { return (pos + i) / S; }
PTTS_LD_HD inline int ld_phase(int pos, int i, int S) { return (pos + i) % S; }
PTTS_LD_HD inline int ld_done(int pos, int n, int S) { return (pos + n) / S; }

// Output sample i of a frame whose row has completed cnt sub-blocks before it: the delayed sample belongs to delayed
// sub-block j = cnt + ld_seg - 4 (negative: still pre-roll, the output is zero) and is ramped from knot j to knot j + 1.
// Knot j is c_{max(j + 2, 3)}; the frame's gains sit in cc[PTTS_LD_CC]: cc[0 .. 2] = c_{cnt-3 .. cnt-1} as carried, cc[3 + g]
// = c_{cnt + g} of the frame's g-th completion.  Gain c_m is therefore cc[m - cnt + 3].  For j >= 0 and seg = ld_seg:
//   lower knot  m = max(j + 2, 3) >= cnt + seg - 2:  index >= seg + 1 >= 1
//   upper knot  m = j + 3 = cnt + seg - 1:           index = seg + 2 <= PTTS_LD_MAX_DONE + 2 < PTTS_LD_CC
// and sub-block cnt + seg - 1 is complete before sample i's segment begins, so both entries are written.
PTTS_LD_HD inline int ld_block(int cnt, int seg) { return cnt + seg - 4; }
PTTS_LD_HD inline int ld_knot_lo(int cnt, int j) { return (j + 2 > 3 ? j + 2 : 3) - cnt + 3; }
PTTS_LD_HD inline int ld_knot_hi(int cnt, int j) { return j + 3 - cnt + 3; }

// The delay ring of D floats with head h (0 <= h < D): output sample i < D reads ld_ring(h, i, D); an output sample i >= D
// reads input sample i - D of the same frame.  Input sample i is kept when i + D >= n, in ld_ring(h, i, D); the new head is
// ld_ring(h, n, D).  All indices lie in [0, D).
PTTS_LD_HD inline int ld_ring(int h, int i, int D) { return (int)(((int64_t)h + i) % D); }

// The history of gating-block energies: block q >= 3 sits at q - 3, kept while q - 3 < PTTS_LD_HIST.
PTTS_LD_HD inline int ld_hist(int q) { return q - 3; }
