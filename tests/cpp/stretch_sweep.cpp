// Index sweep of the time-stretch's index functions (pocket_tts_amd/csrc/ptts_stretch.h) on the CPU, meant to be compiled
// with -fsanitize=address,undefined.  For every plan of the table file, on heap buffers of exactly the sizes the kernel
// stages and owns (one element outside any of them is a sanitizer report):
//   * for every hop j and every delta / previous delta in [-D, D], the first and last index of the candidate's Hs samples, of
//     the segment's W samples and of the template's Hs samples are checked against the staged window w = carried || frame
//     (reach + n_in floats) and read; the ranges are contiguous, so their ends cover every index in between
//   * ts_delta_of is a bijection of [0, 2 D] onto [-D, D] in the order 0, -1, +1, ...
//   * two frames run hop by hop as the kernel runs them - scores over every candidate, argmax with the tie-break, overlap-add
//     into a line of exactly n_out floats, carry of exactly Hs floats, carried samples of exactly `reach` floats - so every
//     index the header forms is also dereferenced
//
// usage: stretch_sweep <file>      file: int32 n_plans, then per plan int32 n_in, Ha, Hs, D, L and 2 Hs float32 (the window);
//                                  written by tests/test_stretch_cpu.py
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ptts_stretch.h"

static bool rd(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n_plans = 0;
  if (!rd(f, &n_plans, 4) || n_plans < 1) return 2;
  long hops = 0, identities = 0;
  uint32_t lcg = 12345u;
  volatile float sink = 0.f;
  for (int r = 0; r < n_plans; ++r) {
    int32_t n_in, Ha, Hs, D, L;
    if (!rd(f, &n_in, 4) || !rd(f, &Ha, 4) || !rd(f, &Hs, 4) || !rd(f, &D, 4) || !rd(f, &L, 4)) return 2;
    if (!ts_plan_ok(n_in, Ha, Hs, D, L, 8192)) {
      printf("plan %d (n_in %d Ha %d Hs %d D %d L %d) is not admitted\n", r, n_in, Ha, Hs, D, L);
      return 1;
    }
    const int W = 2 * Hs;
    float *win = new float[(size_t)W];
    if (!rd(f, win, (size_t)W * 4)) return 2;
    if (ts_identity(Ha, Hs)) {  // a copy of n_in samples into a line of n_out = n_in
      if (n_in / Ha * Hs != n_in) { printf("plan %d: the identity plan does not emit n_in samples\n", r); return 1; }
      ++identities;
      delete[] win;
      continue;
    }
    const int reach = ts_reach(Ha, D, L), K = n_in / Ha, n_out = K * Hs, nw = reach + n_in;
    if (reach > PTTS_TS_HIST || nw > PTTS_TS_WINDOW || Hs > PTTS_TS_MAX_HS || 2 * D + 1 > PTTS_TS_MAX_CAND) {
      printf("plan %d: an admitted plan exceeds a buffer of the kernel\n", r);
      return 1;
    }
    // exact-size heap buffers: new[] so that the sanitizer's red zones sit right at both ends
    float *w = new float[(size_t)nw];
    float *hist = new float[(size_t)reach]();
    float *cy = new float[(size_t)Hs]();
    float *out = new float[(size_t)n_out];
    for (int i = 0; i < nw; ++i) w[i] = 0.f;
    // 1. the ends of every range
    for (int j = 0; j < K; ++j)
      for (int d = -D; d <= D; ++d) {
        const int s = ts_seg(j, d, Ha, D, L), t = ts_tmpl(j, d, Ha, Hs, D, L);
        if (s < 0 || s + W - 1 >= nw || t < 0 || t + Hs - 1 >= nw) {
          printf("plan %d hop %d delta %d: segment [%d, %d] or template [%d, %d] outside w of %d\n", r, j, d, s, s + W - 1, t,
                 t + Hs - 1, nw);
          return 1;
        }
        if (j == 0 && t + Hs - 1 >= reach) { printf("plan %d: the first template leaves the carried samples\n", r); return 1; }
        sink = sink + w[s] + w[s + Hs - 1] + w[s + W - 1] + w[t] + w[t + Hs - 1];
      }
    // 2. candidates <-> deltas
    std::vector<int> seen(2 * D + 1, 0);
    for (int c = 0; c <= 2 * D; ++c) {
      const int d = ts_delta_of(c);
      if (d < -D || d > D || seen[d + D]++) { printf("plan %d: candidate %d -> delta %d\n", r, c, d); return 1; }
      if (c > 0) {
        const int dp = ts_delta_of(c - 1);
        const int a = d < 0 ? -d : d, b = dp < 0 ? -dp : dp;
        if (a < b || (a == b && !(dp < 0 && d > 0))) { printf("plan %d: candidates are not in the order of preference\n", r); return 1; }
      }
    }
    // 3. two frames, hop by hop
    int dprev = 0;
    bool started = false;
    for (int frame = 0; frame < 2; ++frame) {
      for (int i = 0; i < nw; ++i) {
        if (i < reach) { w[i] = hist[i]; continue; }
        lcg = lcg * 1664525u + 1013904223u;
        w[i] = ((lcg >> 8) / 8388608.0f - 1.0f);
      }
      for (int j = 0; j < K; ++j) {
        int delta = 0;
        if (started) {
          const float *t = w + ts_tmpl(j, dprev, Ha, Hs, D, L);
          float best = 0.f;
          int bc = -1;
          for (int c = 0; c <= 2 * D; ++c) {
            const float *s = w + ts_seg(j, ts_delta_of(c), Ha, D, L);
            float acc = 0.f;
            for (int i = 0; i < Hs; ++i) acc += t[i] * s[i];
            if (bc < 0 || acc > best) { best = acc; bc = c; }
          }
          delta = ts_delta_of(bc);
        }
        const float *s = w + ts_seg(j, delta, Ha, D, L);
        for (int n = 0; n < Hs; ++n) {
          out[ts_out(j, n, Hs)] = cy[n] + win[n] * s[n];
          cy[n] = win[Hs + n] * s[Hs + n];
        }
        dprev = delta;
        started = true;
        ++hops;
      }
      for (int i = 0; i < reach; ++i) hist[i] = w[ts_carry_src(i, n_in)];
      sink = sink + out[0] + out[n_out - 1];
    }
    delete[] win; delete[] w; delete[] hist; delete[] cy; delete[] out;
  }
  fclose(f);
  printf("ok %d plans %ld identities %ld hops\n", n_plans, identities, hops);
  return 0;
}
