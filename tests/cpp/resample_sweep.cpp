// Index sweep of the resampler's index function (pocket_tts_amd/csrc/ptts_resample.h) on the CPU, meant to be compiled
// with -fsanitize=address,undefined: for every rate of the table file and every output n < out_n, rs_output runs on heap
// buffers of exactly PTTS_RS_HIST + frame_samples and up * T floats (one element outside either is a sanitizer report)
// and is compared with the direct form y[N] = sum_k h[k] * x_up[N * down - k] in double.
//
// usage: resample_sweep <file>      file: int32 n_rates, int32 frame_samples, then per rate int32 up, down, T and
//                                   up * T float32 (h_poly[ph][j] = h[ph + j * up]); written by tests/test_resample_cpu.py
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ptts_resample.h"

static bool rd(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n_rates = 0, fs = 0;
  if (!rd(f, &n_rates, 4) || !rd(f, &fs, 4) || n_rates < 1 || fs < 1) return 2;
  long total = 0;
  uint32_t lcg = 12345u;
  for (int r = 0; r < n_rates; ++r) {
    int32_t up, down, T;
    if (!rd(f, &up, 4) || !rd(f, &down, 4) || !rd(f, &T, 4)) return 2;
    if (!rs_rate_ok(up, down, T, fs, 4 * fs)) {
      printf("rate %d (up %d down %d T %d) is not admitted\n", r, up, down, T);
      return 1;
    }
    // exact-size heap buffers: new[] so that the sanitizer's red zones sit right at both ends
    float *h = new float[(size_t)up * T];
    float *w = new float[(size_t)PTTS_RS_HIST + fs];
    if (!rd(f, h, (size_t)up * T * 4)) return 2;
    for (int i = 0; i < PTTS_RS_HIST + fs; ++i) {
      lcg = lcg * 1664525u + 1013904223u;
      w[i] = ((lcg >> 8) / 8388608.0f - 1.0f) * 1.2f;
    }
    const int out_n = (int)((long long)fs * up / down);
    for (int n = 0; n < out_n; ++n) {
      // the part of w that the kernel's block of 256 outputs around n stages (rs_window): inside w, and every index that
      // rs_output forms for n, PTTS_RS_HIST + i0 - j with j < T, inside it
      const int n0 = n / 256 * 256, n1 = n0 + 255 < out_n - 1 ? n0 + 255 : out_n - 1;
      int lo, hi;
      rs_window(n0, n1, up, down, T, &lo, &hi);
      const int i0 = (int)((long long)n * down / up);
      if (lo < 0 || hi > PTTS_RS_HIST + fs - 1 || PTTS_RS_HIST + i0 - (T - 1) < lo || PTTS_RS_HIST + i0 > hi) {
        printf("rate %d n %d: reads w[%d .. %d] outside the staged part [%d, %d]\n", r, n, PTTS_RS_HIST + i0 - (T - 1),
               PTTS_RS_HIST + i0, lo, hi);
        return 1;
      }
      const float got = rs_output(h, w, n, up, down, T);
      // direct form over the prototype taps h[k] = h_poly[k % up][k / up], k < up * T, and the zero-stuffed input
      double want = 0.0, mag = 0.0;
      for (long k = 0; k < (long)up * T; ++k) {
        const long m = (long)n * down - k;  // position in the upsampled stream; a multiple of up holds an input sample
        if (((m % up) + up) % up != 0) continue;
        const long i = (m - (((m % up) + up) % up)) / up;  // floor division; i >= -PTTS_RS_HIST since k / up <= T - 1
        if (i < -PTTS_RS_HIST || i >= fs) {
          printf("rate %d n %d k %ld: direct form leaves the window (i = %ld)\n", r, n, k, i);
          return 1;
        }
        const double p = (double)h[(k % up) * T + k / up] * (double)w[PTTS_RS_HIST + i];
        want += p;
        mag += std::fabs(p);
      }
      const double tol = (T + 2) * std::ldexp(1.0, -24) * mag + std::ldexp(1.0, -24);
      if (!(std::fabs((double)got - want) <= tol)) {
        printf("rate %d (up %d down %d T %d) n %d: got %.9g want %.17g tol %.3g\n", r, up, down, T, n, got, want, tol);
        return 1;
      }
      ++total;
    }
    delete[] h;
    delete[] w;
  }
  fclose(f);
  printf("ok %d rates %ld outputs\n", n_rates, total);
  return 0;
}
