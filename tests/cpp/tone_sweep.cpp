// The toner's index functions and chunked recurrence (csrc/ptts_tone.h) on exact-size heap buffers, for every plan in the
// file given as argv[1], against the serial recurrence.  Compiled with a host sanitizer by tests/test_tone_cpu.py: an index
// out of bounds or a chunked sample that leaves the serial one fails.
//
// The file: int32 count, then per plan int32 rate, int32 n, int32 K and PTTS_TN_PLAN_DOUBLES doubles (coefficients, matrix
// powers).  Every plan runs FRAMES frames of a deterministic signal the way the kernel walks them, section by section: chunk,
// scan over two buffers, re-run, carried state (scan_walk.h over the pieces the kernel runs).  The signal is noise-like at 0.25 with digital silence over frames 3 to 6, so
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
#include "scan_walk.h"

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
  double *carry = new double[2 * K], *serial = new double[2 * K];
  std::memset(carry, 0, sizeof(double) * 2 * K);
  std::memset(serial, 0, sizeof(double) * 2 * K);
  double peak = 0.0, worst = 0.0;
  for (int f = 0; f < FRAMES; ++f) {
    for (int i = 0; i < n; ++i) xc[i] = xs[i] = (double)signal((long long)f * n + i, n);
    for (int k = 0; k < K; ++k) {
      const double *c = coef + PTTS_TN_COEFS * k;
      TnSection sec;
      for (int q = 0; q < PTTS_TN_COEFS; ++q) sec.c[q] = c[q];
      sec.pw = pw + (size_t)k * PTTS_TN_SCAN * 4;
      const int bad = scan_walk<PTTS_TN_MAX_CHUNK>(sec, n, chunk, nT, carry + 2 * k, xc, [&](int i, double y) { xc[i] = y; });
      CHECK(bad < 0, "thread %d: [%d, %d)", bad, tn_begin(bad, chunk), tn_end(bad, chunk, n));
      // the serial recurrence beside it
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
  delete[] xc; delete[] xs; delete[] carry; delete[] serial;
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
