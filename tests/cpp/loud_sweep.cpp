// The loudness normaliser's index functions (csrc/ptts_loud.h) on exact-size heap buffers, for every plan in the file given
// as argv[1], and its chunked recurrence against the serial one.  Compiled with a host sanitizer by
// tests/test_loudness_cpu.py: an index out of bounds, an unwritten gain or a chunked sample that leaves the serial one fails.
//
// The file: int32 count, then per plan int32 rate, int32 n and PTTS_LD_PLAN_DOUBLES doubles (coefficients, matrix powers).
// Every plan runs frames of a deterministic signal until the pre-roll and three further sub-blocks have passed, the way the
// kernel walks them: chunk, scan, energy (scan_walk.h over the pieces the kernel runs), segment sums, completions, output
// from the ring, ring update.  Every chunked sample
// is compared with the serial one (1e-10 of 1 + |w|), and every sub-block's energy with the serial one's, 1e-9 relative: the
// second check is the one that sees the silence.  Every scan level multiplies a state by a power whose product cancels by
// about its span in samples (up to 4096), so a frame leaves some 1e-12 in a state and the frames of the silence add up; 1e-9
// holds a factor of ten over what that gives here (1.0e-10 at 32 kHz, n = 882).  The low parts of the powers matter deeper in
// a decay than this sweep goes: the GPU test's tap, 1e-10 on Z through 400 ms of silence, is the check that needs them.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ptts_loud.h"
#include "scan_walk.h"

#define CHECK(c, ...) do { if (!(c)) { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

// digital silence over sub-blocks 1 and 2: there the filters ring out to 1e-20 of the signal's energy, and the scan's matrix
// powers must still carry the state as the serial recurrence does
static float signal(long long i, int S) {
  if (i >= S && i < 3LL * S) return 0.f;
  return 0.25f * (float)std::sin(0.05 * (double)i) + 0.1f * (float)((i * 7919) % 13 - 6) / 6.0f;
}

static int run_plan(int rate, int n, const double *dbl, long long *frames_out) {
  CHECK(ld_plan_ok(rate, n), "plan (%d, %d) is not admissible", rate, n);
  const int S = ld_sub(rate), D = ld_delay(rate), chunk = ld_chunk(n), nT = ld_threads(n);
  CHECK(chunk >= 1 && chunk <= PTTS_LD_MAX_CHUNK && nT >= 1 && nT <= PTTS_LD_THREADS, "chunk %d threads %d", chunk, nT);
  CHECK((nT - 1) * chunk < n && n <= nT * chunk, "chunks do not cover the frame");
  CHECK(D >= 1 && D <= PTTS_LD_MAX_D, "delay %d", D);
  CHECK(scan_steps(nT) <= PTTS_LD_SCAN, "scan steps %d", scan_steps(nT));
  LdWeighting kw;
  for (int q = 0; q < PTTS_LD_COEFS; ++q) kw.c[q] = dbl[q];
  kw.pw = dbl + PTTS_LD_COEFS;
  float *x = new float[n], *y = new float[n], *ring = new float[D];
  double *hist = new double[PTTS_LD_HIST], *P = new double[2 * nT], *xd = new double[n];
  std::memset(ring, 0, sizeof(float) * D);
  double s_carry[4] = {0, 0, 0, 0}, s_serial[4] = {0, 0, 0, 0}, part = 0.0;
  int pos = 0, cnt = 0, head = 0;
  float c3[3] = {1.f, 1.f, 1.f};
  std::vector<float> all_x, all_c;  // the whole input, the gain of every completed sub-block
  std::vector<double> zc, zs;       // per sub-block: the sum of w^2, chunked and serial
  const long long total = (long long)D + 3LL * S + n;
  long long frames = 0;
  for (long long start = 0; start < total; start += n, ++frames) {
    for (int i = 0; i < n; ++i) { x[i] = signal(start + i, S); all_x.push_back(x[i]); }
    const int done = ld_done(pos, n, S);
    CHECK(done >= 0 && done <= PTTS_LD_MAX_DONE, "done %d", done);
    // chunk, scan, re-run: w in place of x
    for (int i = 0; i < n; ++i) xd[i] = (double)x[i];
    const int bad = scan_walk<PTTS_LD_MAX_CHUNK>(kw, n, chunk, nT, s_carry, xd, [&](int i, double w) { xd[i] = w; });
    CHECK(bad < 0, "thread %d: [%d, %d)", bad, ld_begin(bad, chunk), ld_end(bad, chunk, n));
    // energy, against the serial recurrence
    for (int t = 0; t < nT; ++t) {
      const int i0 = ld_begin(t, chunk), i1 = ld_end(t, chunk, n), seg0 = ld_seg(pos, i0, S);
      double pa = 0.0, pb = 0.0;
      for (int i = i0; i < i1; ++i) {
        const double w = xd[i], ws = ld_step(kw.c, s_serial, (double)x[i]);
        CHECK(std::fabs(w - ws) <= 1e-10 * (1.0 + std::fabs(ws)), "rate %d n %d sample %lld: chunked %.17g serial %.17g", rate, n,
              start + i, w, ws);
        const int sg = ld_seg(pos, i, S);
        CHECK(sg == seg0 || sg == seg0 + 1, "a chunk touches three sub-blocks");
        CHECK(sg >= 0 && sg <= done && sg < PTTS_LD_SEGS, "segment %d of %d", sg, done);
        (sg == seg0 ? pa : pb) += w * w;
        const size_t blk = (size_t)((start + i) / S);
        if (zc.size() <= blk) { zc.resize(blk + 1, 0.0); zs.resize(blk + 1, 0.0); }
        zc[blk] += w * w; zs[blk] += ws * ws;
      }
      P[2 * t] = pa; P[2 * t + 1] = pb;
    }
    double segsum[PTTS_LD_SEGS];
    for (int g = 0; g <= done; ++g) {
      double a = 0.0;
      for (int t = 0; t < nT; ++t) {
        const int sg = ld_seg(pos, ld_begin(t, chunk), S);
        a += sg == g ? P[2 * t] : (sg + 1 == g ? P[2 * t + 1] : 0.0);
      }
      segsum[g] = a;
    }
    // completions: the gains of the frame
    float cc[PTTS_LD_CC];
    bool written[PTTS_LD_CC] = {};
    for (int q = 0; q < 3; ++q) { cc[q] = c3[q]; written[q] = true; }
    for (int g = 0; g < done; ++g) {
      const int m = cnt + g;
      const double z = ((g == 0 ? part : 0.0) + segsum[g]) / (double)S;
      CHECK(z >= 0.0 && std::isfinite(z), "energy %g", z);
      if (m >= 3 && ld_hist(m) < PTTS_LD_HIST) {
        CHECK(ld_hist(m) >= 0, "history index %d", ld_hist(m));
        hist[ld_hist(m)] = z;
      }
      CHECK(3 + g < PTTS_LD_CC, "gain index %d", 3 + g);
      cc[3 + g] = 0.5f + 0.001f * (float)(m % 500);  // a gain that differs from block to block
      written[3 + g] = true;
      all_c.push_back(cc[3 + g]);
    }
    // output
    for (int i = 0; i < n; ++i) {
      const int seg = ld_seg(pos, i, S), j = ld_block(cnt, seg);
      float v = 0.f;
      const long long gi = start + i;
      CHECK((j >= 0) == (gi >= D), "sample %lld: block %d", gi, j);
      if (j >= 0) {
        const int lo = ld_knot_lo(cnt, j), hi = ld_knot_hi(cnt, j);
        CHECK(lo >= 0 && lo < PTTS_LD_CC && hi >= 0 && hi < PTTS_LD_CC && written[lo] && written[hi], "knots %d %d of block %d",
              lo, hi, j);
        CHECK(cc[lo] == all_c[j + 2 > 3 ? j + 2 : 3] && cc[hi] == all_c[j + 3], "block %d reads the wrong gains", j);
        const int r = ld_ring(head, i, D);
        CHECK(r >= 0 && r < D, "ring index %d", r);
        const float xd = i < D ? ring[r] : x[i - D];
        CHECK(xd == all_x[gi - D], "sample %lld: the delay line holds the wrong sample", gi);
        CHECK(ld_phase(pos, i, S) == (int)((gi - D) % S), "sample %lld: phase", gi);
        v = (cc[lo] + (cc[hi] - cc[lo]) * ((float)ld_phase(pos, i, S) / (float)S)) * xd;
      }
      y[i] = v;
    }
    for (int i = 0; i < n; ++i)
      if (i + D >= n) {
        const int r = ld_ring(head, i, D);
        CHECK(r >= 0 && r < D, "ring index %d", r);
        ring[r] = x[i];
      }
    part = (done == 0 ? part : 0.0) + segsum[done];
    for (int q = 0; q < 3; ++q) {
      CHECK(done + q < PTTS_LD_CC && written[done + q], "carried gain %d", done + q);
      c3[q] = cc[done + q];
    }
    head = ld_ring(head, n, D);
    cnt += done;
    pos = ld_phase(pos, n, S);
    CHECK(pos >= 0 && pos < S && head >= 0 && head < D, "pos %d head %d", pos, head);
    CHECK((long long)cnt * S + pos == start + n, "position bookkeeping");
  }
  for (size_t b = 0; b + 1 < zc.size(); ++b)
    CHECK(std::fabs(zc[b] - zs[b]) <= 1e-9 * zs[b], "rate %d n %d sub-block %zu: energy chunked %.17g serial %.17g", rate, n, b,
          zc[b], zs[b]);
  CHECK(zs.size() > 3 && zs[2] > 0.0 && zs[2] < 1e-12 * zs[0], "the silence did not ring out: %g of %g", zs[2], zs[0]);
  delete[] x; delete[] y; delete[] ring; delete[] hist; delete[] P; delete[] xd;
  *frames_out += frames;
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t count = 0;
  if (std::fread(&count, 4, 1, f) != 1) return 2;
  long long frames = 0;
  for (int p = 0; p < count; ++p) {
    int32_t rn[2];
    double *dbl = new double[PTTS_LD_PLAN_DOUBLES];
    if (std::fread(rn, 4, 2, f) != 2 || std::fread(dbl, 8, PTTS_LD_PLAN_DOUBLES, f) != PTTS_LD_PLAN_DOUBLES) return 2;
    const int rc = run_plan(rn[0], rn[1], dbl, &frames);
    delete[] dbl;
    if (rc) return rc;
  }
  std::fclose(f);
  std::printf("ok %d plans %lld frames\n", (int)count, frames);
  return 0;
}
