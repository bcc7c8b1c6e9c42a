// Per-request speaking rate: streaming WSOLA time-stretch behind the codec (or behind the resampler).  What the kernel
// (ptts_stretch.hip) and a plain C++ program (the index sweep of tests/test_stretch_cpu.py, compiled with a host
// sanitizer) share.  Ordinary C++: compiles with g++ as well as under hipcc.
//
// A plan is (n_in, Ha, Hs, D, L): n_in input samples per frame, analysis hop Ha, synthesis hop Hs, search radius D, lag L;
// window W = 2 Hs, K = n_in / Ha hops per frame, n_out = K Hs outputs per frame.  Hop k of a row's stream reads the segment
//   x[p_k .. p_k + W),  p_k = k Ha - L + delta_k,  delta_k in [-D, D]
// chosen against the template x[p_{k-1} + Hs .. p_{k-1} + 2 Hs).  With L >= D + W + Hs no read passes the end of the frame
// that holds hop k, and the oldest sample a frame reads lies ts_reach = L + D + Ha before its first one: that many input
// samples are carried from frame to frame (at most PTTS_TS_HIST).  Ha == Hs is the identity plan: a copy, no state.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PTTS_TS_HD __host__ __device__
#else
#define PTTS_TS_HD
#endif

#define PTTS_TS_HIST 8192     // most input samples a row carries from frame to frame (stretch.py: HIST)
#define PTTS_TS_WINDOW 12288  // most floats of (carried samples || frame) the kernel stages in LDS (48 KB)
#define PTTS_TS_MAX_HS 2048   // largest synthesis hop: the carry line of a row (second half of the last segment)
#define PTTS_TS_MAX_CAND 1024 // largest 2 D + 1: the scores of one hop fit the kernel's score line

struct TsPlan {
  int32_t n_in, Ha, Hs, D, L;
  int32_t K;      // n_in / Ha hops per frame
  int32_t n_out;  // K * Hs outputs per frame
  int32_t reach;  // L + D + Ha carried input samples (0 for the identity plan)
  int32_t woff;   // offset of the plan's W = 2 Hs window floats in the stretcher's window buffer
};

PTTS_TS_HD inline bool ts_identity(int Ha, int Hs) { return Ha == Hs; }

// The admission rules, as the library applies them before a plan reaches the device (stretch.py applies the same ones
// with a message per rule).  `max_in`: largest frame the caller accepts.
PTTS_TS_HD inline bool ts_plan_ok(int n_in, int Ha, int Hs, int D, int L, int max_in) {
  if (n_in < 1 || n_in > max_in || Ha < 1 || Hs < 1 || D < 0 || L < 0) return false;
  if (Ha > n_in || n_in % Ha != 0) return false;
  if (ts_identity(Ha, Hs)) return true;  // a copy: nothing staged, nothing carried
  if (Hs > PTTS_TS_MAX_HS) return false;
  if (2 * Hs < Ha || Hs > 2 * Ha) return false;  // speed = Ha / Hs in [0.5, 2]
  if (2 * D + 1 > PTTS_TS_MAX_CAND) return false;
  if (L % Ha != 0 || L < D + 3 * Hs) return false;  // causal: L >= D + W + Hs
  if (L > PTTS_TS_HIST || L + D + Ha > PTTS_TS_HIST) return false;
  return L + D + Ha + n_in <= PTTS_TS_WINDOW;
}

PTTS_TS_HD inline int ts_reach(int Ha, int D, int L) { return L + D + Ha; }

// The staged window of a row: w = carried || frame, reach + n_in floats; w[reach + i] = input sample i of this frame,
// w[reach - 1 - i] = sample i before its start (zero before the stream's start).  Hop j (0 <= j < K) of the frame:
//
//   ts_seg(j, delta)   index in w of the segment's first sample, p = reach + j Ha - L + delta
//     lower bound  delta >= -D, j >= 0                  =>  p >= reach - L - D = Ha > 0
//     upper bound  delta <= D, j <= K - 1, n < W        =>  p + n <= reach + n_in - Ha - L + D + W - 1
//                  L >= D + W + Hs                      =>  p + n <= reach + n_in - Ha - Hs - 1 < reach + n_in
//   ts_tmpl(j, dprev)  index in w of the template's first sample, (segment of the hop before) + Hs, dprev = the delta of
//                      the hop before (the row's carried delta for j = 0):  q = reach + (j - 1) Ha - L + dprev + Hs
//     lower bound  j = 0, dprev >= -D                   =>  q >= reach - Ha - L - D + Hs = Hs > 0
//     upper bound  q + i <= ts_seg(j - 1, D) + W - 1 (i < Hs), inside w by the line above (j >= 1), and for j = 0
//                  q + i < reach - Ha - L + D + 2 Hs <= reach - Ha - Hs < reach
// The scores read w[ts_seg(j, delta) + i], i < Hs; the overlap-add reads w[ts_seg(j, delta_j) + n], n < W.
PTTS_TS_HD inline int ts_seg(int j, int delta, int Ha, int D, int L) { return ts_reach(Ha, D, L) + j * Ha - L + delta; }
PTTS_TS_HD inline int ts_tmpl(int j, int dprev, int Ha, int Hs, int D, int L) { return ts_seg(j - 1, dprev, Ha, D, L) + Hs; }

// Candidate c (0 <= c <= 2 D) <-> delta, in the order of preference among equal scores: 0, -1, +1, -2, +2, ...
PTTS_TS_HD inline int ts_delta_of(int c) { return (c & 1) ? -((c + 1) >> 1) : (c >> 1); }

// The carried samples after the frame: carried'[i] = w[n_in + i], i < reach (the last `reach` floats of w).
PTTS_TS_HD inline int ts_carry_src(int i, int n_in) { return n_in + i; }
// Output sample n (0 <= n < Hs) of hop j within the row's line of out_max >= n_out = K Hs samples: j Hs + n < K Hs.
PTTS_TS_HD inline int ts_out(int j, int n, int Hs) { return j * Hs + n; }
