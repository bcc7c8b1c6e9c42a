// The toner's index functions and chunked recurrence (csrc/ptts_tone.h) on exact-size heap buffers, for every plan in the
// file given as argv[1], against the serial recurrence.  Compiled with a host sanitizer by tests/test_tone_cpu.py: an index
// out of bounds or a chunked sample that leaves the serial one fails.
//
// The file: int32 count, then per plan int32 rate, int32 n, int32 K and PTTS_TN_PLAN_DOUBLES doubles (coefficients, matrix
// powers).  Every plan runs FRAMES frames of a deterministic signal the way the kernel walks them, section by section: chunk,
// scan over two buffers, re-run, carried state.  The signal is noise-like at 0.25 with digital silence over frames 3 to 6, so
// that the sections ring out and the scan's powers must carry a decaying state as the serial recurrence does.  Every chunked
// output sample (float64, before the rounding to fp32) is compared with the serial one; the program prints the largest
// |chunked - serial| / (running peak of |serial|), "e64", and fails where it exceeds 2^-25 = 3e-8: rounding to fp32 moves a
// sample by at most half a unit in its last place, 2^-25 of its size, so a scheme within 2^-25 of the peak keeps a sample
// at the peak within one unit of fp32 of the serial definition.  With powers rounded once (tone.py) the presets stay below
// 4e-13 and the corners of the grammar (20 Hz at q = 16, a 24 dB shelf at 20 Hz) below 8e-11; eight peaks of 24 dB at 20 Hz
// in a row reach 4e-10.  Powers squared in float64 gave 7e-9 at those corners and 3.5e-8 for the eight.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ptts_tone.h"

#define CHECK(c, ...) do { if (!(c)) { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

static const int FRAMES = 12;

static float signal(long long i, int n) {
  const long long frame = i / n;
  if (frame >= 3 && frame < 7) return 0.f;
  return 0.15f * (float)std::sin(0.05 * (double)i) + 0.1f * (float)((i * 7919) % 13 - 6) / 6.0f;
}

static int run_plan(int rate, int n, int K, const double *dbl, double *e64) {
  CHECK(tn_plan_ok(rate, n, K), "plan (%d, %d, %d) is not admissible", rate, n, K);
  const int chunk = tn_chunk(n), nT = tn_threads(n), steps = tn_steps(nT);
  CHECK(chunk >= 1 && chunk <= PTTS_TN_MAX_CHUNK && nT >= 1 && nT <= PTTS_TN_THREADS, "chunk %d threads %d", chunk, nT);
  CHECK((nT - 1) * chunk < n && n <= nT * chunk, "chunks do not cover the frame");
  CHECK(steps >= 0 && steps <= PTTS_TN_SCAN && (1 << steps) >= nT && (steps == 0 || (1 << (steps - 1)) < nT), "steps %d", steps);
  const double *coef = dbl;
  const double *pw = dbl + PTTS_TN_MAX_SECTIONS * PTTS_TN_COEFS;
  double *xc = new double[n], *xs = new double[n];                 // the frame through the sections: chunked, serial
  double *E = new double[2 * 2 * nT], *s_all = new double[2 * nT];  // E[buf][t][2]; the threads' running states
  double *carry = new double[2 * K], *serial = new double[2 * K];
  std::memset(carry, 0, sizeof(double) * 2 * K);
  std::memset(serial, 0, sizeof(double) * 2 * K);
  double peak = 0.0, worst = 0.0;
  for (int f = 0; f < FRAMES; ++f) {
    for (int i = 0; i < n; ++i) xc[i] = xs[i] = (double)signal((long long)f * n + i, n);
    for (int k = 0; k < K; ++k) {
      const double *c = coef + PTTS_TN_COEFS * k;
      // chunk
      for (int t = 0; t < nT; ++t) {
        double s[2] = {0.0, 0.0};
        if (t == 0) { s[0] = carry[2 * k]; s[1] = carry[2 * k + 1]; }
        const int i0 = tn_begin(t, chunk), i1 = tn_end(t, chunk, n);
        CHECK(i0 >= 0 && i0 < i1 && i1 <= n && i1 - i0 <= PTTS_TN_MAX_CHUNK, "thread %d: [%d, %d)", t, i0, i1);
        for (int i = i0; i < i1; ++i) tn_step(c, s, xc[i]);
        s_all[2 * t] = E[2 * t] = s[0]; s_all[2 * t + 1] = E[2 * t + 1] = s[1];
      }
      // scan: a step reads one half of E and writes the other
      int cur = 0;
      for (int j = 0; j < steps; ++j) {
        const int off = 1 << j;
        const double *src = E + (size_t)cur * 2 * nT;
        double *dst = E + (size_t)(cur ^ 1) * 2 * nT;
        for (int t = 0; t < nT; ++t) {
          if (t >= off) tn_mat_acc(pw + ((size_t)k * PTTS_TN_SCAN + j) * 4, src + 2 * (t - off), s_all + 2 * t);
          dst[2 * t] = s_all[2 * t]; dst[2 * t + 1] = s_all[2 * t + 1];
        }
        cur ^= 1;
      }
      // re-run, and the serial recurrence beside it
      const double *Ef = E + (size_t)cur * 2 * nT;
      for (int t = 0; t < nT; ++t) {
        double s[2] = {carry[2 * k], carry[2 * k + 1]};
        if (t > 0) { s[0] = Ef[2 * (t - 1)]; s[1] = Ef[2 * (t - 1) + 1]; }
        const int i0 = tn_begin(t, chunk), i1 = tn_end(t, chunk, n);
        for (int i = i0; i < i1; ++i) xc[i] = tn_step(c, s, xc[i]);
        if (t == nT - 1) { carry[2 * k] = s[0]; carry[2 * k + 1] = s[1]; }
      }
      for (int i = 0; i < n; ++i) xs[i] = tn_step(c, serial + 2 * k, xs[i]);
    }
    for (int i = 0; i < n; ++i) {
      CHECK(std::isfinite(xc[i]) && std::isfinite(xs[i]), "rate %d n %d frame %d sample %d is not finite", rate, n, f, i);
      peak = std::fmax(peak, std::fabs(xs[i]));
      const double d = std::fabs(xc[i] - xs[i]);
      if (peak > 0.0) worst = std::fmax(worst, d / peak);
      else CHECK(d == 0.0, "rate %d n %d frame %d sample %d: %g against silence", rate, n, f, i, xc[i]);
    }
  }
  CHECK(worst <= 1.0 / 33554432.0, "rate %d n %d K %d: chunked leaves serial by %.3g of the running peak", rate, n, K, worst);
  *e64 = std::fmax(*e64, worst);
  delete[] xc; delete[] xs; delete[] E; delete[] s_all; delete[] carry; delete[] serial;
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t count = 0;
  if (std::fread(&count, 4, 1, f) != 1) return 2;
  double e64 = 0.0;
  for (int p = 0; p < count; ++p) {
    int32_t h[PTTS_TN_PLAN_INTS];
    double *dbl = new double[PTTS_TN_PLAN_DOUBLES];
    if (std::fread(h, 4, PTTS_TN_PLAN_INTS, f) != PTTS_TN_PLAN_INTS ||
        std::fread(dbl, 8, PTTS_TN_PLAN_DOUBLES, f) != PTTS_TN_PLAN_DOUBLES)
      return 2;
    const int rc = run_plan(h[0], h[1], h[2], dbl, &e64);
    delete[] dbl;
    if (rc) return rc;
  }
  std::fclose(f);
  std::printf("ok %d plans %d frames e64 %.3e\n", (int)count, (int)count * FRAMES, e64);
  return 0;
}
