// Index sweep of the true-peak mode's index functions (pocket_tts_amd/csrc/ptts_level.h, "True-peak mode") on the CPU, meant
// to be compiled with -fsanitize=address,undefined.  Stand-alone: it takes no arguments.
//   1. for EVERY pair (n, LA) that lv_tp_plan_ok admits and every tile of it, the extreme indices of each function - the
//      first and last sample, the first and last entry of the r line, tap 0 and tap T - 1, the first and last carried entry -
//      are checked against the sizes of the lines the kernel stages (LA + H + T floats of u, LA + T of r, H + T of y) and
//      against the LDS arrays it declares; pairs just outside the rule are checked to be refused
//   2. for a set of plans at the corners (LA 1 and 512, odd LA, n = LA + 10, frames of one tile, of two with a last tile
//      shorter than the carried lines, and of four) three frames and a drain frame run tile by tile with the plain statement
//      of the mode in fp32 on heap buffers of exactly those sizes, so every index the header forms is also dereferenced (one
//      element outside is a sanitizer report); output and meter are compared with the definition evaluated over the whole
//      stream at once in double
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ptts_level.h"

static const int H = PTTS_LV_TP_H, D = PTTS_LV_TP_D, NT = PTTS_LV_TP_T;

static int extremes(int n, int LA) {
  const int tiles = lv_tiles(n);
  for (int j = 0; j < tiles; ++j) {
    const int T = lv_tile_len(j, n), ul = LA + H + T, rl = LA + T, yl = H + T;
    if (T < 1 || ul > PTTS_LV_TP_ULINE || rl > PTTS_LV_LINE || yl > PTTS_LV_TP_YLINE) return 1;
    if (lv_tp_cur(0, LA) != LA + H || lv_tp_cur(T - 1, LA) != ul - 1) return 2;
    for (int q : {0, rl - 1}) {
      if (lv_tp_tap(q, 0) != q + H || lv_tp_tap(q, NT - 1) != q || lv_tp_tap(q, 0) >= ul || lv_tp_tap(q, NT - 1) < 0) return 3;
      if (lv_tp_centre(q) != lv_tp_tap(q, D) || lv_tp_centre(q) < 0 || lv_tp_centre(q) >= ul) return 4;
    }
    for (int i : {0, T - 1}) {
      // y[i] multiplies the sample LA + D before sample i
      if (lv_tp_delayed(i) != lv_tp_cur(i, LA) - LA - D || lv_tp_delayed(i) < 0 || lv_tp_delayed(i) >= ul) return 5;
      if (lv_tp_ycur(i) != H + i || lv_tp_ycur(i) >= yl) return 6;
      if (lv_tp_ytap(i, 0) != lv_tp_ycur(i) || lv_tp_ytap(i, NT - 1) != i || lv_tp_ytap(i, 0) >= yl) return 7;
      if (lv_tp_ycentre(i) != lv_tp_ytap(i, D) || lv_tp_ycentre(i) < 0 || lv_tp_ycentre(i) >= yl) return 8;
      if (lv_io(j, i) < 0 || lv_io(j, i) >= n) return 9;
    }
    if (lv_tp_carry_src(0, T) != T || lv_tp_carry_src(LA + H - 1, T) != ul - 1) return 10;
    if (lv_tp_ycarry_src(0, T) != T || lv_tp_ycarry_src(H - 1, T) != yl - 1) return 11;
    if (lv_carry_src(0, T) != T || lv_carry_src(LA - 1, T) != rl - 1) return 12;  // the e line keeps the sample-peak layout
  }
  return 0;
}

static float taps[PTTS_LV_TP_PHASES][PTTS_LV_TP_T];

static void make_taps() {  // a 4x windowed sinc of the same shape as level.TP_TAPS; the sweep needs indices, not these values
  const double pi = 3.14159265358979323846;
  for (int p = 1; p <= 3; ++p)
    for (int j = 0; j < NT; ++j) {
      const int idx = p + 4 * j;
      const double t = (idx - 40) / 4.0, w = 0.5 + 0.5 * std::cos(pi * (idx - 40) / 41.0);
      taps[p - 1][j] = idx > 80 ? 0.f : (float)(std::sin(pi * t) / (pi * t) * w);
    }
}

static int run(int n, int LA, long *tiles_run) {
  static uint32_t lcg = 12345u;
  volatile float sink = 0.f;
  const float G = 3.98107171f, C = 0.89125094f, a = 0.999f, k = 1.0f / LA;
  const int tiles = lv_tiles(n), CU = LA + H, frames = 4;  // the last frame drains
  float *cu = new float[(size_t)CU]();
  float *ce = new float[(size_t)LA];
  float *cy = new float[(size_t)H]();
  float *tmp = new float[(size_t)CU];
  for (int c = 0; c < LA; ++c) ce[c] = 1.f;
  float dcar = 0.f, M = 0.f;
  std::vector<float> xs((size_t)frames * n), ys((size_t)frames * n);
  for (int fr = 0; fr < frames; ++fr) {
    float *in = new float[(size_t)n];
    float *out = new float[(size_t)n];
    for (int i = 0; i < n; ++i) {
      lcg = lcg * 1664525u + 1013904223u;
      in[i] = fr == frames - 1 ? 0.f : ((lcg >> 8) / 8388608.0f - 1.0f) * 0.5f;
      xs[(size_t)fr * n + i] = in[i];
    }
    for (int j = 0; j < tiles; ++j) {
      const int T = lv_tile_len(j, n), ul = CU + T, rl = LA + T, yl = H + T;
      float *U = new float[(size_t)ul];
      float *E = new float[(size_t)rl];
      float *Y = new float[(size_t)yl];
      float *m = new float[(size_t)T];
      for (int c = 0; c < CU; ++c) U[c] = cu[c];
      for (int c = 0; c < H; ++c) Y[c] = cy[c];
      for (int i = 0; i < T; ++i) U[lv_tp_cur(i, LA)] = G * in[lv_io(j, i)];
      for (int q = 0; q < rl; ++q) {
        float pk = std::fabs(U[lv_tp_centre(q)]);
        for (int p = 0; p < PTTS_LV_TP_PHASES; ++p) {
          float v = 0.f;
          for (int t = 0; t < NT; ++t) v = std::fmaf(taps[p][t], U[lv_tp_tap(q, t)], v);
          pk = std::fmax(pk, std::fabs(v));
        }
        E[q] = pk > C ? C / pk : 1.f;
      }
      for (int i = 0; i < T; ++i) {
        float v = E[lv_min_lo(i)];
        for (int q = lv_min_lo(i) + 1; q <= lv_min_hi(i, LA); ++q) v = E[q] < v ? E[q] : v;
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
        float s = 0.f;
        for (int q = lv_box_lo(i); q <= lv_box_hi(i, LA); ++q) s += E[q];
        const float y = k * s * U[lv_tp_delayed(i)];
        out[lv_io(j, i)] = y;
        Y[lv_tp_ycur(i)] = y;
      }
      for (int i = 0; i < T; ++i) {
        float pk = std::fabs(Y[lv_tp_ycentre(i)]);
        for (int p = 0; p < PTTS_LV_TP_PHASES; ++p) {
          float w = 0.f;
          for (int t = 0; t < NT; ++t) w = std::fmaf(taps[p][t], Y[lv_tp_ytap(i, t)], w);
          pk = std::fmax(pk, std::fabs(w));
        }
        M = std::fmax(M, pk);
      }
      for (int c = 0; c < CU; ++c) tmp[c] = U[lv_tp_carry_src(c, T)];
      for (int c = 0; c < CU; ++c) cu[c] = tmp[c];
      for (int c = 0; c < LA; ++c) tmp[c] = E[lv_carry_src(c, T)];
      for (int c = 0; c < LA; ++c) ce[c] = tmp[c];
      for (int c = 0; c < H; ++c) tmp[c] = Y[lv_tp_ycarry_src(c, T)];
      for (int c = 0; c < H; ++c) cy[c] = tmp[c];
      sink = sink + U[0] + U[ul - 1] + E[0] + E[rl - 1] + Y[0] + Y[yl - 1];
      delete[] U; delete[] E; delete[] Y; delete[] m;
      ++*tiles_run;
    }
    for (int i = 0; i < n; ++i) ys[(size_t)fr * n + i] = out[i];
    delete[] in; delete[] out;
  }
  delete[] cu; delete[] ce; delete[] cy; delete[] tmp;
  // the same stream at once, in double
  const long N = (long)frames * n;
  std::vector<double> u(N), r(N), e(N), y(N);
  for (long i = 0; i < N; ++i) u[i] = (double)G * xs[i];
  auto at = [](const std::vector<double> &v, long i) { return i >= 0 ? v[i] : 0.0; };
  auto peak = [&](const std::vector<double> &v, long i) {
    double pk = std::fabs(at(v, i - D));
    for (int p = 0; p < PTTS_LV_TP_PHASES; ++p) {
      double s = 0.0;
      for (int t = 0; t < NT; ++t) s += (double)taps[p][t] * at(v, i - t);
      pk = std::fmax(pk, std::fabs(s));
    }
    return pk;
  };
  double d = 0.0, worst = 0.0, M64 = 0.0;
  for (long i = 0; i < N; ++i) {
    const double pk = peak(u, i);
    r[i] = pk > C ? C / pk : 1.0;
    double mm = 1.0;
    for (long t = 0; t <= LA && t <= i; ++t) mm = r[i - t] < mm ? r[i - t] : mm;
    const double c = 1.0 - mm, ad = (double)a * d;
    d = c > ad ? c : ad;
    e[i] = 1.0 - d;
    double s = 0.0;
    for (long t = 0; t < LA; ++t) s += i - t >= 0 ? e[i - t] : 1.0;
    y[i] = (double)k * s * at(u, i - LA - D);
    worst = std::fmax(worst, std::fabs(y[i] - (double)ys[i]));
    if (std::fabs((double)ys[i]) > C * (1.0 + (LA + 8) / 16777216.0)) { printf("n %d LA %d: sample %ld = %g exceeds the ceiling\n", n, LA, i, ys[i]); return 1; }
    if (i >= N - n + LA + D && ys[i] != 0.f) { printf("n %d LA %d: sample %ld behind the drained tail is %g\n", n, LA, i, ys[i]); return 1; }
  }
  for (long i = 0; i < N; ++i) M64 = std::fmax(M64, peak(y, i));
  const double umax = G * 0.5, bound = ((LA + 64) + 22 * 2.3 * umax / C) / 16777216.0 * umax;
  if (worst > bound) { printf("n %d LA %d: tile by tile differs from the whole stream by %g (bound %g)\n", n, LA, worst, bound); return 1; }
  if (std::fabs(M64 - M) > 3.3 * bound) { printf("n %d LA %d: the meter reads %g, the whole stream %g\n", n, LA, (double)M, M64); return 1; }
  return 0;
}

int main() {
  make_taps();
  long pairs = 0, tiles_run = 0;
  for (int LA = 1; LA <= PTTS_LV_MAX_LA; ++LA) {
    if (lv_tp_plan_ok(LA + D - 1, LA) || lv_tp_plan_ok(PTTS_LV_MAX_N + 1, LA)) { printf("LA %d: a frame outside the rule is admitted\n", LA); return 1; }
    for (int n = LA + D; n <= PTTS_LV_MAX_N; ++n) {
      if (!lv_tp_plan_ok(n, LA) || !lv_plan_ok(n, LA)) { printf("n %d LA %d is not admitted\n", n, LA); return 1; }
      const int rc = extremes(n, LA);
      if (rc) { printf("n %d LA %d: check %d fails\n", n, LA, rc); return 1; }
      ++pairs;
    }
  }
  if (lv_tp_plan_ok(1000, 0) || lv_tp_plan_ok(1000, PTTS_LV_MAX_LA + 1)) { printf("a look-ahead outside the rule is admitted\n"); return 1; }
  int plans = 0;
  for (int LA : {1, 2, 40, 55, 56, 120, 221, 240, 511, 512})
    for (int n : {LA + D, LA + D + 1, LA + 2 * H + D, 640, 882, 1920, 2047, 2048, 2049, 2048 + H - 1, 2048 + LA, 3840, 4097, 8192}) {
      if (!lv_tp_plan_ok(n, LA)) continue;
      if (run(n, LA, &tiles_run)) return 1;
      ++plans;
    }
  printf("ok %ld pairs %d plans %ld tiles\n", pairs, plans, tiles_run);
  return 0;
}
