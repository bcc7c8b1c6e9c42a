// The compressor's index functions and chunked recurrences (csrc/ptts_dyn.h) on exact-size heap buffers, for every plan in
// the file given as argv[1], against the header's serial sample step.  Compiled with a host sanitizer by
// tests/test_dynamics_cpu.py: an index out of bounds or a chunked sample that leaves the serial one fails.
//
// The file: int32 count, then per plan int32 rate, int32 n and PTTS_DY_PLAN_DOUBLES doubles (T k W M aA aR, the powers of aA,
// the powers of aR).  Every plan runs FRAMES frames of a deterministic signal the way the kernel walks them: the curve, then
// for p and for s chunk, scan over two buffers, re-run, carried state (scan_walk.h over DyPeak and DySmooth, the
// kernel's two recurrences in the shared scheme's terms).  The signal is noise-like, gated between two levels,
// with digital silence over frames 3 to 6 and one full-scale sample, so that the detector rises, decays and rings out on the
// floor.  Every chunked s (float64, in dB) is compared with the serial one; the program prints the largest |chunked -
// serial|, "e_db", and fails above 1e-9 dB: that is 1.2e-10 of the gain, three orders below the 6e-8 of the rounding to fp32.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ptts_dyn.h"
#include "scan_walk.h"

#define CHECK(c, ...) do { if (!(c)) { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

static const int FRAMES = 12;

static float signal(long long i, int n) {
  const long long frame = i / n;
  if (frame >= 3 && frame < 7) return 0.f;
  if (i == 8LL * n + n / 2) return -1.0f;
  const float level = (i / 97) % 2 ? 0.004f : 1.0f;
  return level * (0.15f * (float)std::sin(0.05 * (double)i) + 0.1f * (float)((i * 7919) % 13 - 6) / 6.0f);
}

static int run_plan(int rate, int n, const double *d, double *e_db) {
  CHECK(dyn_plan_ok(rate, n), "plan (%d, %d) is not admissible", rate, n);
  DyPlan P;
  P.rate = rate; P.n = n; P.chunk = dy_chunk(n); P.threads = dy_threads(n);
  P.T = d[0]; P.k = d[1]; P.W = d[2]; P.M = d[3]; P.aA = d[4]; P.aR = d[5];
  std::memcpy(P.pwA, d + 6, sizeof(P.pwA));
  std::memcpy(P.pwR, d + 6 + PTTS_DY_SCAN, sizeof(P.pwR));
  CHECK(dyn_values_ok(P.T, P.k, P.W, P.M, P.aA, P.aR), "plan (%d, %d): a value outside its range", rate, n);
  const int chunk = P.chunk, nT = P.threads, steps = dy_steps(nT);
  CHECK(chunk >= 1 && chunk <= PTTS_DY_MAX_CHUNK && nT >= 1 && nT <= PTTS_DY_THREADS, "chunk %d threads %d", chunk, nT);
  CHECK((nT - 1) * chunk < n && n <= nT * chunk, "chunks do not cover the frame");
  CHECK(steps >= 0 && steps <= PTTS_DY_SCAN && (1 << steps) >= nT && (steps == 0 || (1 << (steps - 1)) < nT), "steps %d", steps);
  float *x = new float[n];
  double *v = new double[n];
  double carry[2] = {0.0, 0.0}, serial[2] = {0.0, 0.0}, worst = 0.0;
  for (int f = 0; f < FRAMES; ++f) {
    for (int i = 0; i < n; ++i) {
      x[i] = signal((long long)f * n + i, n);
      v[i] = dy_curve(dy_level((double)x[i]), P.T, P.k, P.W);
      CHECK(v[i] >= 0.0 && v[i] <= 180.0, "rate %d n %d frame %d sample %d: reduction %g", rate, n, f, i, v[i]);
    }
    const auto keep = [&](int i, double a) { v[i] = a; };  // p in place of c, then s in place of p
    int bad = scan_walk<PTTS_DY_MAX_CHUNK>(DyPeak{P.aR, P.pwR}, n, chunk, nT, carry, v, keep);
    if (bad < 0) bad = scan_walk<PTTS_DY_MAX_CHUNK>(DySmooth{P.aA, P.pwA}, n, chunk, nT, carry + 1, v, keep);
    CHECK(bad < 0, "thread %d: [%d, %d)", bad, dy_begin(bad, chunk), dy_end(bad, chunk, n));
    for (int i = 0; i < n; ++i) {
      const float y = dy_step(P, serial, x[i]);
      CHECK(std::isfinite(v[i]) && v[i] >= 0.0 && std::isfinite(y), "rate %d n %d frame %d sample %d is not finite", rate, n, f, i);
      worst = std::fmax(worst, std::fabs(v[i] - serial[1]));
      const float yc = (float)(dy_gain(P.M, v[i]) * (double)x[i]);
      CHECK(std::fabs((double)yc - (double)y) <= 1.2e-7 * std::fabs((double)y), "rate %d n %d frame %d sample %d: %g against %g",
            rate, n, f, i, yc, y);
    }
  }
  CHECK(worst <= 1e-9, "rate %d n %d: chunked leaves serial by %.3g dB", rate, n, worst);
  *e_db = std::fmax(*e_db, worst);
  delete[] x; delete[] v;
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t count = 0;
  if (std::fread(&count, 4, 1, f) != 1) return 2;
  double e_db = 0.0;
  for (int p = 0; p < count; ++p) {
    int32_t h[PTTS_DY_PLAN_INTS];
    double *dbl = new double[PTTS_DY_PLAN_DOUBLES];
    if (std::fread(h, 4, PTTS_DY_PLAN_INTS, f) != PTTS_DY_PLAN_INTS ||
        std::fread(dbl, 8, PTTS_DY_PLAN_DOUBLES, f) != PTTS_DY_PLAN_DOUBLES)
      return 2;
    const int rc = run_plan(h[0], h[1], dbl, &e_db);
    delete[] dbl;
    if (rc) return rc;
  }
  std::fclose(f);
  std::printf("ok %d plans %d frames e_db %.3e\n", (int)count, (int)count * FRAMES, e_db);
  return 0;
}
