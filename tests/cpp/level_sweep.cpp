// Index sweep of the leveler's index functions (pocket_tts_amd/csrc/ptts_level.h) on the CPU, meant to be compiled with
// -fsanitize=address,undefined.  For every plan of the table file, on heap buffers of exactly the sizes the kernel stages and
// owns (one element outside any of them is a sanitizer report):
//   * the tiles partition [0, n): each begins where the one before ends, holds 1 .. PTTS_LV_TILE samples, the last ends at n
//   * for every sample of every tile the first and last index of its minimum window and of its box window, its own entry and
//     its delayed entry are checked against the staged line of LA + T floats and read; the carried line's sources likewise
//   * three frames run tile by tile with the plain statement of the contract in fp32 - stage, r, minimum, the recurrence on d
//     sample by sample, e, box sum, output into a line of exactly n floats, carried lines of exactly LA floats - so every index
//     the header forms is also dereferenced; the result is compared with the contract evaluated over the whole stream at once
//
// usage: level_sweep <file>      file: int32 n_plans, then per plan int32 n, LA and float32 a, k; written by
//                                tests/test_level_cpu.py
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ptts_level.h"

static bool rd(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n_plans = 0;
  if (!rd(f, &n_plans, 4) || n_plans < 1) return 2;
  long tiles_run = 0;
  uint32_t lcg = 12345u;
  volatile float sink = 0.f;
  const float G = 3.98107171f, C = 0.89125094f;
  for (int p = 0; p < n_plans; ++p) {
    int32_t n, LA;
    float a, k;
    if (!rd(f, &n, 4) || !rd(f, &LA, 4) || !rd(f, &a, 4) || !rd(f, &k, 4)) return 2;
    if (!lv_plan_ok(n, LA)) { printf("plan %d (n %d LA %d) is not admitted\n", p, n, LA); return 1; }
    if (LA > PTTS_LV_MAX_LA || n > PTTS_LV_MAX_N) { printf("plan %d: an admitted plan exceeds a buffer of the kernel\n", p); return 1; }
    // 1. the tiles
    const int tiles = lv_tiles(n);
    int end = 0;
    for (int j = 0; j < tiles; ++j) {
      const int b = lv_tile_begin(j), T = lv_tile_len(j, n);
      if (b != end || T < 1 || T > PTTS_LV_TILE || LA + T > PTTS_LV_LINE) { printf("plan %d tile %d: [%d, %d + %d)\n", p, j, b, b, T); return 1; }
      end = b + T;
    }
    if (end != n) { printf("plan %d: the tiles end at %d, not at n = %d\n", p, end, n); return 1; }
    // exact-size heap buffers: new[] so that the sanitizer's red zones sit right at both ends
    float *cu = new float[(size_t)LA]();
    float *ce = new float[(size_t)LA];
    float *tmp = new float[(size_t)LA];
    for (int c = 0; c < LA; ++c) ce[c] = 1.f;
    float dcar = 0.f;
    const int frames = 3;
    std::vector<float> xs((size_t)frames * n), ys((size_t)frames * n);
    for (int fr = 0; fr < frames; ++fr) {
      float *in = new float[(size_t)n];
      float *out = new float[(size_t)n];
      for (int i = 0; i < n; ++i) {
        lcg = lcg * 1664525u + 1013904223u;
        in[i] = ((lcg >> 8) / 8388608.0f - 1.0f) * 0.5f;
        xs[(size_t)fr * n + i] = in[i];
      }
      for (int j = 0; j < tiles; ++j) {
        const int T = lv_tile_len(j, n), nl = LA + T;
        float *U = new float[(size_t)nl];
        float *E = new float[(size_t)nl];
        float *m = new float[(size_t)T];
        for (int c = 0; c < LA; ++c) U[c] = cu[c];
        for (int i = 0; i < T; ++i) {
          const int q = lv_cur(i, LA), s = lv_io(j, i);
          if (q < LA || q >= nl || s < 0 || s >= n) { printf("plan %d tile %d sample %d: entry %d, line index %d\n", p, j, i, q, s); return 1; }
          U[q] = G * in[s];
        }
        for (int q = 0; q < nl; ++q) { const float au = std::fabs(U[q]); E[q] = au > C ? C / au : 1.f; }
        for (int i = 0; i < T; ++i) {
          const int lo = lv_min_lo(i), hi = lv_min_hi(i, LA);
          if (lo < 0 || hi >= nl || hi - lo != LA) { printf("plan %d tile %d sample %d: minimum window [%d, %d] of %d\n", p, j, i, lo, hi, nl); return 1; }
          float v = E[lo];
          for (int q = lo + 1; q <= hi; ++q) v = E[q] < v ? E[q] : v;
          m[i] = v;
        }
        for (int c = 0; c < LA; ++c) E[c] = ce[c];
        float d = dcar;
        for (int i = 0; i < T; ++i) {
          const float c = 1.f - m[i], ad = a * d;
          d = c > ad ? c : ad;
          E[lv_cur(i, LA)] = 1.f - d;
        }
        dcar = d;
        for (int i = 0; i < T; ++i) {
          const int lo = lv_box_lo(i), hi = lv_box_hi(i, LA), dl = lv_delayed(i);
          if (lo < 1 || hi >= nl || hi - lo != LA - 1 || dl < 0 || dl + LA != lv_cur(i, LA)) {
            printf("plan %d tile %d sample %d: box window [%d, %d] of %d, delayed %d\n", p, j, i, lo, hi, nl, dl);
            return 1;
          }
          float s = 0.f;
          for (int q = lo; q <= hi; ++q) s += E[q];
          out[lv_io(j, i)] = k * s * U[dl];
        }
        for (int c = 0; c < LA; ++c) {
          const int s = lv_carry_src(c, T);
          if (s < 0 || s >= nl) { printf("plan %d tile %d: carried entry %d from %d of %d\n", p, j, c, s, nl); return 1; }
          tmp[c] = U[s];
        }
        for (int c = 0; c < LA; ++c) cu[c] = tmp[c];
        for (int c = 0; c < LA; ++c) tmp[c] = E[lv_carry_src(c, T)];
        for (int c = 0; c < LA; ++c) ce[c] = tmp[c];
        sink = sink + U[0] + U[nl - 1] + E[0] + E[nl - 1];
        delete[] U; delete[] E; delete[] m;
        ++tiles_run;
      }
      for (int i = 0; i < n; ++i) ys[(size_t)fr * n + i] = out[i];
      sink = sink + out[0] + out[n - 1];
      delete[] in; delete[] out;
    }
    delete[] cu; delete[] ce; delete[] tmp;
    // 2. the same stream at once, in double
    const long N = (long)frames * n;
    std::vector<double> r(N), e(N);
    double d = 0.0, worst = 0.0;
    for (long i = 0; i < N; ++i) {
      const double au = std::fabs((double)G * xs[i]);
      r[i] = au > C ? C / au : 1.0;
      double mm = 1.0;
      for (long t = 0; t <= LA && t <= i; ++t) mm = r[i - t] < mm ? r[i - t] : mm;
      const double c = 1.0 - mm, ad = (double)a * d;
      d = c > ad ? c : ad;
      e[i] = 1.0 - d;
      double s = 0.0;
      for (long t = 0; t < LA; ++t) s += i - t >= 0 ? e[i - t] : 1.0;
      const double y = (double)k * s * (i >= LA ? (double)G * xs[i - LA] : 0.0);
      const double err = std::fabs(y - (double)ys[i]);
      worst = err > worst ? err : worst;
      if (std::fabs((double)ys[i]) > C * (1.0 + (LA + 8) / 16777216.0)) { printf("plan %d: sample %ld = %g exceeds the ceiling\n", p, i, ys[i]); return 1; }
    }
    if (worst > (LA + 64) / 16777216.0 * G * 0.5) { printf("plan %d: tile by tile differs from the whole stream by %g\n", p, worst); return 1; }
  }
  fclose(f);
  printf("ok %d plans %ld tiles\n", n_plans, tiles_run);
  return 0;
}
