// Index sweep of the pitch shifter's index functions (pocket_tts_amd/csrc/ptts_pitch.h and the ptts_stretch.h it includes)
// on the CPU, meant to be compiled with -fsanitize=address,undefined.  For every plan of the table file, on heap buffers of
// exactly the sizes the kernel stages and owns (one element outside any of them is a sanitizer report):
//   * the WSOLA part as tests/cpp/stretch_sweep.cpp checks it: for every hop and every delta / previous delta in [-D, D] the
//     ends of the candidate's, the segment's and the template's range against w = carried || frame (reach + n floats)
//   * the mid line m = history || frame of exactly PTTS_PT_HIST + n_mid floats: pt_mid of every (hop, sample) is written, every
//     entry behind the history exactly once; pt_tap of every (output, tap) and pt_phase * T + tap of the table of exactly Q T
//     floats are checked and read; pt_keep of every history sample is read
//   * two frames run as the kernel runs them - hops with scores, argmax and overlap-add into the mid line, then every output
//     through pt_output into a line of exactly n floats, then the carried samples, the carry and the line's history
//
// usage: pitch_sweep <file>      file: int32 n_plans, then per plan int32 n, Ha, Hs, D, L, P, Q, T, 2 Hs float32 (the window)
//                                and Q T float32 (the table); written by tests/test_pitch_cpu.py
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ptts_pitch.h"

static bool rd(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n_plans = 0;
  if (!rd(f, &n_plans, 4) || n_plans < 1) return 2;
  long hops = 0, identities = 0, outputs = 0;
  uint32_t lcg = 12345u;
  volatile float sink = 0.f;
  for (int r = 0; r < n_plans; ++r) {
    int32_t v[8];
    if (!rd(f, v, sizeof v)) return 2;
    const int n = v[0], Ha = v[1], Hs = v[2], D = v[3], L = v[4], P = v[5], Q = v[6], T = v[7];
    if (!pt_plan_ok(n, Ha, Hs, D, L, P, Q, T, 8192, PTTS_PT_MAX_MID)) {
      printf("plan %d (n %d Ha %d Hs %d D %d L %d P %d Q %d T %d) is not admitted\n", r, n, Ha, Hs, D, L, P, Q, T);
      return 1;
    }
    const int W = 2 * Hs;
    float *win = new float[(size_t)W];
    float *tab = new float[(size_t)Q * T];
    if (!rd(f, win, (size_t)W * 4) || !rd(f, tab, (size_t)Q * T * 4)) return 2;
    if (ts_identity(Ha, Hs)) {  // a copy of n samples into a line of n
      if (n / Ha * Hs != n) { printf("plan %d: the identity plan does not emit n samples\n", r); return 1; }
      ++identities;
      delete[] win; delete[] tab;
      continue;
    }
    const int reach = ts_reach(Ha, D, L), K = n / Ha, n_mid = K * Hs, nw = reach + n, nm = PTTS_PT_HIST + n_mid;
    if (reach > PTTS_TS_HIST || nw > PTTS_TS_WINDOW || Hs > PTTS_TS_MAX_HS || 2 * D + 1 > PTTS_TS_MAX_CAND ||
        n_mid > PTTS_PT_MAX_MID || T - 1 > PTTS_PT_HIST || (long long)n_mid * Q != (long long)n * P) {
      printf("plan %d: an admitted plan exceeds a buffer of the kernel, or n_mid Q != n P\n", r);
      return 1;
    }
    // exact-size heap buffers: new[] so that the sanitizer's red zones sit right at both ends
    float *w = new float[(size_t)nw]();
    float *hist = new float[(size_t)reach]();
    float *cy = new float[(size_t)Hs]();
    float *m = new float[(size_t)nm]();
    float *out = new float[(size_t)n];
    // 1. the ends of every WSOLA range
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
    // 2. the mid line: every entry behind the history is written exactly once, every tap lies inside
    std::vector<int> hit(nm, 0);
    for (int j = 0; j < K; ++j)
      for (int i = 0; i < Hs; ++i) {
        const int a = pt_mid(j, i, Hs);
        if (a < PTTS_PT_HIST || a >= nm || hit[a]++) { printf("plan %d: pt_mid(%d, %d) = %d\n", r, j, i, a); return 1; }
      }
    for (int a = PTTS_PT_HIST; a < nm; ++a)
      if (hit[a] != 1) { printf("plan %d: mid sample %d is not written\n", r, a - PTTS_PT_HIST); return 1; }
    int last = -1;
    for (int N = 0; N < n; ++N) {
      const int ph = pt_phase(N, P, Q);
      if (ph < 0 || ph >= Q) { printf("plan %d: phase %d of output %d\n", r, ph, N); return 1; }
      if (N == 0 && ph != 0) { printf("plan %d: the frame does not start at phase 0\n", r); return 1; }
      for (int j = 0; j < T; ++j) {
        const int a = pt_tap(N, j, P, Q);
        if (a < 0 || a >= nm) { printf("plan %d: tap %d of output %d reads %d of %d\n", r, j, N, a, nm); return 1; }
        sink = sink + m[a] + tab[ph * T + j];
      }
      last = pt_tap(N, 0, P, Q);
    }
    if ((long long)n * P % Q != 0 || last > nm - 1) { printf("plan %d: the next frame does not start at phase 0\n", r); return 1; }
    for (int i = 0; i < PTTS_PT_HIST; ++i) {
      const int a = pt_keep(i, n_mid);
      if (a < 0 || a >= nm) { printf("plan %d: pt_keep(%d) = %d\n", r, i, a); return 1; }
    }
    // 3. two frames, as the kernel runs them
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
        for (int i = 0; i < Hs; ++i) {
          m[pt_mid(j, i, Hs)] = cy[i] + win[i] * s[i];
          cy[i] = win[Hs + i] * s[Hs + i];
        }
        dprev = delta;
        started = true;
        ++hops;
      }
      for (int N = 0; N < n; ++N) out[N] = pt_output(tab, m, N, P, Q, T);
      outputs += n;
      for (int i = 0; i < reach; ++i) hist[i] = w[ts_carry_src(i, n)];
      float keep[PTTS_PT_HIST];
      for (int i = 0; i < PTTS_PT_HIST; ++i) keep[i] = m[pt_keep(i, n_mid)];
      for (int i = 0; i < PTTS_PT_HIST; ++i) m[i] = keep[i];
      sink = sink + out[0] + out[n - 1];
    }
    delete[] win; delete[] tab; delete[] w; delete[] hist; delete[] cy; delete[] m; delete[] out;
  }
  fclose(f);
  printf("ok %d plans %ld identities %ld hops %ld outputs\n", n_plans, identities, hops, outputs);
  return 0;
}
