// Streaming polyphase resampler behind the codec's last kernel: what the kernels (ptts_resample.hip) and a plain C++
// program (the index sweep of tests/test_resample_cpu.py, compiled with a host sanitizer) share.  Ordinary C++: compiles
// with g++ as well as under hipcc.
//
// One codec frame is `fs` = frame_samples input samples.  A rate is (up, down, T): the causal FIR
//   y[N] = sum_k h[k] * x_up[N * down - k]            (x_up: x with up - 1 zeros between samples)
// in polyphase form, h_poly[ph][j] = h[ph + j * up] zero-padded to [up][T].  A rate is admitted (rs_rate_ok) only when
//   fs * up % down == 0   every frame yields the whole number out_n = fs * up / down of outputs, and the phase of output 0
//                         of every frame is 0: a frame needs nothing from earlier frames but their last input samples
//   T - 1 <= PTTS_RS_HIST the oldest input an output reads lies within the carried history
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PTTS_RS_HD __host__ __device__
#else
#define PTTS_RS_HD
#endif

#define PTTS_RS_HIST 64  // input samples carried from frame to frame (resample.py: HIST)

struct RsRate {
  int32_t up, down, T;  // reduced ratio, taps per phase
  int32_t out_n;        // fs * up / down outputs per frame
  int32_t off;          // offset of the rate's [up][T] table in the resampler's table buffer (floats)
};

// The admission rules, as the library applies them before a rate reaches the device (resample.py applies the same ones
// with a message per rule).  `max_out`: largest out_n the caller accepts.
PTTS_RS_HD inline bool rs_rate_ok(int up, int down, int T, int fs, int max_out) {
  if (up < 1 || down < 1 || T < 1 || fs < PTTS_RS_HIST) return false;
  if (up > 4096 || down > 4096 || T - 1 > PTTS_RS_HIST) return false;
  if ((long long)fs * up % down != 0) return false;
  return (long long)fs * up / down <= max_out;
}

// Output sample n (0 <= n < out_n) of one frame.  w = history || frame: PTTS_RS_HIST + fs floats, w[PTTS_RS_HIST + i] =
// input sample i of this frame, w[PTTS_RS_HIST - 1 - i] = sample i before its start (zero before the stream's start);
// h_poly: the rate's up * T floats.
//
// Bounds, by the admission rules and n < out_n (no run-time clamp anywhere):
//   i0 = floor(n * down / up) <= floor((out_n - 1) * down / up) < out_n * down / up = fs       =>  i0 <= fs - 1
//   0 <= j <= T - 1 <= PTTS_RS_HIST                                                           =>  0 <= PTTS_RS_HIST + i0 - j
//   so 0 <= PTTS_RS_HIST + i0 - j < PTTS_RS_HIST + fs for every j < T, and ph * T + j < up * T since ph < up.
// n * down < out_n * down = fs * up fits an int for every admitted rate (fs * up <= 4096 * fs).
PTTS_RS_HD inline float rs_output(const float *h_poly, const float *w, int n, int up, int down, int T) {
  const int t = n * down;
  const int i0 = t / up, ph = t % up;
  const float *hp = h_poly + ph * T;
  const float *wp = w + PTTS_RS_HIST + i0;
  float acc = 0.f;
  for (int j = 0; j < T; ++j) acc = __builtin_fmaf(hp[j], wp[-j], acc);
  return acc;
}

// The part [*lo, *hi] of w that the outputs n0 .. n1 (0 <= n0 <= n1 < out_n) read: i0 grows with n, so every
// w[PTTS_RS_HIST + i0(n) - j], j < T, of these outputs lies between PTTS_RS_HIST + i0(n0) - (T - 1) >= 0 and
// PTTS_RS_HIST + i0(n1) <= PTTS_RS_HIST + fs - 1 (the bounds above).  A block of resample_kernel stages this part only,
// every entry at its own index of w; the sweep checks every index rs_output forms against it.
PTTS_RS_HD inline void rs_window(int n0, int n1, int up, int down, int T, int *lo, int *hi) {
  *lo = PTTS_RS_HIST + n0 * down / up - (T - 1);
  *hi = PTTS_RS_HIST + n1 * down / up;
}
