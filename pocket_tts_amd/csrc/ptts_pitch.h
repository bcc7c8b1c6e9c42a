// Per-request pitch: a streaming WSOLA time-stretch by r = P / Q followed by a polyphase resampling by Q / P, in one launch
// behind the stretcher (or whatever stage comes before).  What the kernel (ptts_pitch.hip) and a plain C++ program (the index
// sweep of tests/test_pitch_cpu.py, compiled with a host sanitizer) share.  Ordinary C++: compiles with g++ as well as under
// hipcc.
//
// A plan is (n, Ha, Hs, D, L, P, Q, T).  (n, Ha, Hs, D, L) is a WSOLA plan of ptts_stretch.h with Ha = Q u, Hs = P u: every
// index of the WSOLA part is formed by that header's functions, under that header's bounds.  A frame's K = n / Ha hops emit
// n_mid = K Hs = n P / Q "mid" samples.  The FIR part is the causal polyphase filter of ptts_resample.h with (up, down) =
// (Q, P) and T taps per phase over the mid stream; a frame yields n_mid Q / P = n outputs, and the phase of output 0 of every
// frame is 0.  P == Q (== 1) is the identity plan: a copy, no state.
#pragma once
#include <stdint.h>

#include "ptts_stretch.h"

#define PTTS_PT_HIST 40       // mid samples a row carries from frame to frame (pitch.py: HIST); T - 1 <= 40 for P, Q <= 20
#define PTTS_PT_MAX_TERM 20   // largest P and Q
#define PTTS_PT_MAX_MID 16384 // largest n_mid (twice the largest frame)

struct PtPlan {
  TsPlan ts;      // the WSOLA part; ts.n_out is n_mid
  int32_t P, Q, T;
  int32_t toff;   // offset of the plan's [Q][T] table in the pitcher's table buffer (floats)
};

PTTS_TS_HD inline int pt_taps(int P, int Q) { return (20 * (P > Q ? P : Q) + 1 + Q - 1) / Q; }

// The admission rules, as the library applies them before a plan reaches the device (pitch.py applies the same ones with a
// message per rule).  `max_in`: largest frame, `max_mid`: largest n_mid the caller accepts.
PTTS_TS_HD inline bool pt_plan_ok(int n, int Ha, int Hs, int D, int L, int P, int Q, int T, int max_in, int max_mid) {
  if (P < 1 || Q < 1 || P > PTTS_PT_MAX_TERM || Q > PTTS_PT_MAX_TERM) return false;
  if (!ts_plan_ok(n, Ha, Hs, D, L, max_in)) return false;
  if (ts_identity(Ha, Hs)) return P == 1 && Q == 1 && T == 1;
  if (P == Q) return false;
  for (int g = 2; g <= PTTS_PT_MAX_TERM; ++g)
    if (P % g == 0 && Q % g == 0) return false;     // reduced: the tap count is that of the reduced ratio
  if (Ha % Q != 0 || Hs % P != 0 || Ha / Q != Hs / P) return false;  // Ha = Q u, Hs = P u: n_mid Q / P == n exactly
  if (T != pt_taps(P, Q) || T - 1 > PTTS_PT_HIST) return false;
  return n / Ha * Hs <= max_mid;
}

// The mid line of a row: m = history || frame, PTTS_PT_HIST + n_mid floats (a line of the pitcher holds PTTS_PT_HIST +
// mid_max >= that); m[PTTS_PT_HIST + i] = mid sample i of this frame, m[PTTS_PT_HIST - 1 - i] = mid sample i before its
// start (zero before the stream's start).
//
//   pt_mid(j, i)     where sample i (0 <= i < Hs) of hop j (0 <= j < K) goes:
//     PTTS_PT_HIST <= PTTS_PT_HIST + j Hs + i <= PTTS_PT_HIST + (K - 1) Hs + Hs - 1 < PTTS_PT_HIST + n_mid
PTTS_TS_HD inline int pt_mid(int j, int i, int Hs) { return PTTS_PT_HIST + ts_out(j, i, Hs); }
//   pt_tap(N, j)     the mid sample that tap j (0 <= j < T) of output N (0 <= N < n) reads, i0 = floor(N P / Q):
//     upper bound  i0 <= floor((n - 1) P / Q) < n P / Q = n_mid        =>  PTTS_PT_HIST + i0 - j <= PTTS_PT_HIST + n_mid - 1
//     lower bound  j <= T - 1 <= PTTS_PT_HIST, i0 >= 0                 =>  PTTS_PT_HIST + i0 - j >= 0
//   N P < 8192 * 20 fits an int.
PTTS_TS_HD inline int pt_tap(int N, int j, int P, int Q) { return PTTS_PT_HIST + N * P / Q - j; }
//   pt_phase(N)      the row of the [Q][T] table output N uses: 0 <= (N P) % Q < Q, so pt_phase * T + j < Q T
PTTS_TS_HD inline int pt_phase(int N, int P, int Q) { return N * P % Q; }
//   pt_keep(i)       the history after the frame: m'[i] = m[n_mid + i], i < PTTS_PT_HIST (the last PTTS_PT_HIST floats of m):
//     n_mid <= n_mid + i <= n_mid + PTTS_PT_HIST - 1 < PTTS_PT_HIST + n_mid
PTTS_TS_HD inline int pt_keep(int i, int n_mid) { return n_mid + i; }

// Output sample N of one frame: the taps in index order, one fused multiply-add each.
PTTS_TS_HD inline float pt_output(const float *table, const float *m, int N, int P, int Q, int T) {
  const float *hp = table + pt_phase(N, P, Q) * T;
  float acc = 0.f;
  for (int j = 0; j < T; ++j) acc = __builtin_fmaf(hp[j], m[pt_tap(N, j, P, Q)], acc);
  return acc;
}
