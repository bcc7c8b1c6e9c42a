// The partition and the chunked scan of csrc/ptts_scan.h on their own, compiled with a host sanitizer by
// tests/test_scan_cpu.py.
//
// The partition: for every n in 1 .. 8192 at 1024 threads, 1 <= chunk <= 8, (threads - 1) chunk < n <= threads chunk, the
// [begin, end) ranges tile [0, n) exactly once, and steps is the least j with 2^j >= threads.
// The scheme: scan_walk.h against a serial run, over exact-size heap buffers, for a scalar linear recurrence
// s' = a s + (1 - a) x and a scalar max-plus recurrence s' = max(x, a s), three frames with a carried state, at
// n in {1, 2, 63, 1023, 1024, 1025, 8191, 8192}.  The powers a^(chunk 2^j) come from repeated squaring in long double,
// rounded once.  Max-plus is exact up to the rounding of the products, and a product of at most 8192 factors is within
// 8192 2^-53 of the power rounded once: 1e-12 relative.  The linear scan adds at most 13 terms of that accuracy to values
// of at most 1: 1e-11 absolute.
#include <cmath>
#include <cstdio>
#include <vector>

#include "scan_walk.h"

#define CHECK(c, ...) do { if (!(c)) { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

static const int THREADS = 1024, MAX_N = 8192, MAX_CHUNK = 8, SCAN = 10;

struct Linear {
  static constexpr int W = 1;
  double a, pw[SCAN];
  double step(double *s, double x) const { return s[0] = a * s[0] + (1.0 - a) * x; }
  void join(int j, const double *e, double *s) const { s[0] += pw[j] * e[0]; }
};
struct MaxPlus {
  static constexpr int W = 1;
  double a, pw[SCAN];
  double step(double *s, double x) const { return s[0] = x > a * s[0] ? x : a * s[0]; }
  void join(int j, const double *e, double *s) const { s[0] = s[0] > pw[j] * e[0] ? s[0] : pw[j] * e[0]; }
};

static int partition() {
  for (int n = 1; n <= MAX_N; ++n) {
    const int chunk = scan_chunk(n, THREADS), used = scan_threads(n, THREADS), steps = scan_steps(used);
    CHECK(chunk >= 1 && chunk <= MAX_CHUNK, "n %d: chunk %d", n, chunk);
    CHECK(used >= 1 && used <= THREADS && (used - 1) * chunk < n && n <= used * chunk, "n %d: %d threads of %d", n, used, chunk);
    int next = 0;
    for (int t = 0; t < used; ++t) {
      CHECK(scan_begin(t, chunk) == next && scan_end(t, chunk, n) > next, "n %d thread %d: [%d, %d) after %d", n, t,
            scan_begin(t, chunk), scan_end(t, chunk, n), next);
      next = scan_end(t, chunk, n);
    }
    CHECK(next == n, "n %d: the ranges end at %d", n, next);
    CHECK(steps >= 0 && steps <= SCAN && (1 << steps) >= used && (steps == 0 || (1 << (steps - 1)) < used), "n %d: steps %d", n, steps);
  }
  return 0;
}

static double signal(long long i) { return 0.5 + 0.4 * std::sin(0.05 * (double)i) + 0.1 * (double)((i * 7919) % 13 - 6) / 6.0; }

template <class R>
static int scheme(const char *name, double a, double bound, double *worst) {
  for (int n : {1, 2, 63, 1023, 1024, 1025, 8191, 8192}) {
    const int chunk = scan_chunk(n, THREADS), used = scan_threads(n, THREADS);
    R r;
    r.a = a;
    long double p = 1.0L;
    for (int q = 0; q < chunk; ++q) p *= (long double)a;
    for (int j = 0; j < SCAN; ++j, p *= p) r.pw[j] = (double)p;
    double carry = 0.0, serial = 0.0;
    for (int f = 0; f < 3; ++f) {
      double *x = new double[n], *y = new double[n];
      for (int i = 0; i < n; ++i) x[i] = f == 1 ? 0.0 : signal((long long)f * n + i);  // the middle frame decays
      const int bad = scan_walk<MAX_CHUNK>(r, n, chunk, used, &carry, x, [&](int i, double v) { y[i] = v; });
      CHECK(bad < 0, "%s n %d: thread %d has no range", name, n, bad);
      for (int i = 0; i < n; ++i) {
        const double want = r.step(&serial, x[i]), d = std::fabs(y[i] - want);
        CHECK(d <= bound, "%s n %d frame %d sample %d: %.17g against %.17g", name, n, f, i, y[i], want);
        *worst = std::fmax(*worst, d);
      }
      CHECK(std::fabs(carry - serial) <= bound, "%s n %d frame %d: carried %.17g against %.17g", name, n, f, carry, serial);
      delete[] x; delete[] y;
    }
  }
  return 0;
}

int main() {
  if (partition()) return 1;
  double lin = 0.0, mx = 0.0;
  if (scheme<Linear>("linear", 0.999, 1e-11, &lin) || scheme<MaxPlus>("max-plus", 0.9995, 1e-12, &mx)) return 1;
  std::printf("ok %d sizes linear %.3e max-plus %.3e\n", MAX_N, lin, mx);
  return 0;
}
