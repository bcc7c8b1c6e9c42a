// The chunked scan of csrc/ptts_scan.h walked on the host, thread by thread, the way scan_block walks it on the device: the
// same per-thread pieces (scan_run, scan_join, scan_rerun) over exact-size heap buffers, two halves of chunk ends with a
// step reading one and writing the other.  Shared by the sweeps of this directory, which run under a host sanitizer.
#pragma once
#include <vector>

#include "ptts_scan.h"

// One recurrence over a frame of n samples in x, split as scan_chunk / scan_threads split it; keep(i, y) receives what
// sample i gives, after which x[i] may be overwritten.  carry: the R::W doubles a row carries from frame to frame.
// Returns -1, or the first thread whose range is not 1 .. MAXC samples inside the frame.
template <int MAXC, class R, class Keep>
int scan_walk(const R &r, int n, int chunk, int used, double *carry, const double *x, Keep &&keep) {
  constexpr int W = R::W;
  std::vector<double> E(2 * (size_t)used * W), s_all((size_t)used * W, 0.0);
  for (int t = 0; t < used; ++t) {
    const int i0 = scan_begin(t, chunk), i1 = scan_end(t, chunk, n);
    if (!(i0 >= 0 && i0 < i1 && i1 <= n && i1 - i0 <= MAXC)) return t;
    double *s = s_all.data() + (size_t)t * W;
    if (t == 0) for (int q = 0; q < W; ++q) s[q] = carry[q];
    scan_run<MAXC>(r, s, x + i0, i1 - i0);
    for (int q = 0; q < W; ++q) E[(size_t)t * W + q] = s[q];
  }
  const int steps = scan_steps(used);
  int cur = 0;
  for (int j = 0; j < steps; ++j) {
    const double *src = E.data() + (size_t)cur * used * W;
    double *dst = E.data() + (size_t)(cur ^ 1) * used * W;
    for (int t = 0; t < used; ++t) {
      double *s = s_all.data() + (size_t)t * W;
      scan_join(r, j, t, src, s);
      for (int q = 0; q < W; ++q) dst[(size_t)t * W + q] = s[q];
    }
    cur ^= 1;
  }
  const double *Ef = E.data() + (size_t)cur * used * W;
  std::vector<double> first(carry, carry + W);
  for (int t = 0; t < used; ++t) {
    double s0[W];
    for (int q = 0; q < W; ++q) s0[q] = t > 0 ? Ef[(size_t)(t - 1) * W + q] : first[q];
    const int i0 = scan_begin(t, chunk), i1 = scan_end(t, chunk, n);
    scan_rerun<MAXC>(r, s0, x + i0, i1 - i0, [&](int q, double y) { keep(i0 + q, y); });
    if (t == used - 1) for (int q = 0; q < W; ++q) carry[q] = s0[q];
  }
  return -1;
}
