// Per-request output gain with a look-ahead peak limiter: the last output stage, behind the codec, the resampler or the
// stretcher.  What the kernel (ptts_level.hip) and a plain C++ program (the index sweep of tests/test_level_cpu.py, compiled
// with a host sanitizer) share.  Ordinary C++: compiles with g++ as well as under hipcc.
//
// A plan is (n, LA, a, k): n samples per frame, look-ahead LA, release factor a per sample, k = 1 / LA.  With u = G x:
//   r[i] = |u[i]| > C ? C / |u[i]| : 1        m[i] = min r[i - LA .. i]        d[i] = max(1 - m[i], a d[i - 1])
//   e[i] = 1 - d[i]                            g[i] = k sum e[i - LA + 1 .. i]  y[i] = g[i] u[i - LA]
// Sample i reads u and e at most LA samples back: a row carries its last LA samples of u, its last LA of e and its last d
// from frame to frame (contract: pocket_tts_amd/level.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PTTS_LV_HD __host__ __device__
#else
#define PTTS_LV_HD
#endif

#define PTTS_LV_MAX_LA 512  // largest look-ahead: the carried lines of a row (u and e)
#define PTTS_LV_TILE 2048   // most samples of a frame the kernel works on at a time
#define PTTS_LV_MAX_N 8192  // largest frame
#define PTTS_LV_LINE (PTTS_LV_MAX_LA + PTTS_LV_TILE)  // floats of one staged line: carried || tile

struct LvPlan {
  int32_t n, LA;
  float a, k;
};

// The admission rules, as the library applies them before a plan reaches the device (level.py applies the same ones with a
// message per rule).
PTTS_LV_HD inline bool lv_plan_ok(int n, int LA) {
  if (LA < 1 || LA > PTTS_LV_MAX_LA) return false;
  return n >= LA && n <= PTTS_LV_MAX_N;
}

// A frame of n samples is walked in tiles [lv_tile_begin(j), lv_tile_begin(j) + lv_tile_len(j, n)), 0 <= j < lv_tiles(n):
//   begin = j TILE <= (tiles - 1) TILE < n, so 1 <= len <= TILE and begin + len <= n: nothing past n of a line is touched.
PTTS_LV_HD inline int lv_tiles(int n) { return (n + PTTS_LV_TILE - 1) / PTTS_LV_TILE; }
PTTS_LV_HD inline int lv_tile_begin(int j) { return j * PTTS_LV_TILE; }
PTTS_LV_HD inline int lv_tile_len(int j, int n) { return n - j * PTTS_LV_TILE < PTTS_LV_TILE ? n - j * PTTS_LV_TILE : PTTS_LV_TILE; }

// The staged lines of a tile of T samples, each LA + T <= MAX_LA + TILE = PTTS_LV_LINE floats: entries [0, LA) are the
// carried line (the LA samples before the tile, oldest first), entry LA + i belongs to sample i of the tile (0 <= i < T).
//   lv_cur(i, LA)      index of sample i itself:                   LA <= LA + i <= LA + T - 1
//   lv_delayed(i)      index of the sample LA before sample i:     0 <= i <= T - 1 (what y[i] multiplies)
//   lv_min_lo / hi     the window of m[i], r[i - LA .. i]:         [i, LA + i], inside [0, LA + T - 1]
//   lv_box_lo / hi     the window of g[i], e[i - LA + 1 .. i]:     [i + 1, LA + i], inside [1, LA + T - 1]
PTTS_LV_HD inline int lv_cur(int i, int LA) { return LA + i; }
PTTS_LV_HD inline int lv_delayed(int i) { return i; }
PTTS_LV_HD inline int lv_min_lo(int i) { return i; }
PTTS_LV_HD inline int lv_min_hi(int i, int LA) { return LA + i; }
PTTS_LV_HD inline int lv_box_lo(int i) { return i + 1; }
PTTS_LV_HD inline int lv_box_hi(int i, int LA) { return LA + i; }

// The carried line after a tile of T samples: carried'[c] = line[T + c], 0 <= c < LA: T <= T + c <= LA + T - 1 (the last LA
// entries of the staged line).  Source and destination overlap when T < LA: the kernel reads every entry into a register,
// waits at a barrier and writes then.
PTTS_LV_HD inline int lv_carry_src(int c, int T) { return T + c; }

// Output (and input) sample i of tile j within the row's line of n samples: begin + i <= begin + len - 1 <= n - 1.
PTTS_LV_HD inline int lv_io(int j, int i) { return lv_tile_begin(j) + i; }

// ---- True-peak mode (level.py, "True-peak mode") ----------------------------------------------------------------------
// The gain computer sees P[i] = max(|u[i - D]|, |v_1[i]|, |v_2[i]|, |v_3[i]|), v_p[i] = sum_j h_p[j] u[i - j] over T taps, the
// output is y[i] = g[i] u[i - D - LA], and a meter runs the same FIR over y.  r[i - LA], the oldest the minimum of sample i
// reads, reaches u[i - LA - (T - 1)]: such a row carries its last LA + H samples of u, H = T - 1, and its last H samples of y.
#define PTTS_LV_TP_D 10                     // the interpolator's group delay in input samples
#define PTTS_LV_TP_T 21                     // taps per phase
#define PTTS_LV_TP_PHASES 3                 // phases 1, 2, 3 of 4: phase 0 is the sample itself, D late
#define PTTS_LV_TP_H (PTTS_LV_TP_T - 1)     // samples the FIR reaches back
#define PTTS_LV_TP_ULINE (PTTS_LV_MAX_LA + PTTS_LV_TP_H + PTTS_LV_TILE)  // floats of the staged u line in this mode
#define PTTS_LV_TP_YLINE (PTTS_LV_TP_H + PTTS_LV_TILE)                   // floats of the staged y line: carried || tile
#define PTTS_LV_TP_CARRY (2 * PTTS_LV_TP_H)  // floats a row carries on top of the sample-peak ones: H of u, then H of y

// A plan serves a true-peak row only when the pre-roll LA + D fits one frame: one drain frame then flushes the tail.
PTTS_LV_HD inline bool lv_tp_plan_ok(int n, int LA) { return lv_plan_ok(n, LA) && LA + PTTS_LV_TP_D <= n; }

// The staged u line of a tile of T samples in this mode, LA + H + T <= PTTS_LV_TP_ULINE floats: entries [0, LA + H) are the
// carried line, oldest first, entry LA + H + i is sample i of the tile.  The r line keeps the sample-peak layout (entry q is
// the sample q - LA of the tile, 0 <= q < LA + T), so the minimum, the scan and the box are the sample-peak ones.
//   lv_tp_cur(i, LA)    index of sample i itself:                        LA + H <= . <= LA + H + T - 1
//   lv_tp_tap(q, j)     what tap j of r-line entry q multiplies:         q + H - j, 0 <= j < T: inside [q, q + H], and
//                       q + H <= LA + T - 1 + H, the last staged entry
//   lv_tp_centre(q)     the sample D before r-line entry q's:            q + H - D = lv_tp_tap(q, D)
//   lv_tp_delayed(i)    the sample LA + D before sample i (y[i]'s):      i + H - D, inside [H - D, T - 1 + H - D]
//   lv_tp_carry_src     carried'[c] = line[T + c], 0 <= c < LA + H:      T <= . <= LA + H + T - 1
PTTS_LV_HD inline int lv_tp_cur(int i, int LA) { return LA + PTTS_LV_TP_H + i; }
PTTS_LV_HD inline int lv_tp_tap(int q, int j) { return q + PTTS_LV_TP_H - j; }
PTTS_LV_HD inline int lv_tp_centre(int q) { return q + PTTS_LV_TP_H - PTTS_LV_TP_D; }
PTTS_LV_HD inline int lv_tp_delayed(int i) { return i + PTTS_LV_TP_H - PTTS_LV_TP_D; }
PTTS_LV_HD inline int lv_tp_carry_src(int c, int T) { return T + c; }

// The staged y line of a tile of T samples, H + T <= PTTS_LV_TP_YLINE floats: entries [0, H) are the last H samples of y
// before the tile, entry H + i is y of sample i.  The meter of sample i reads
//   lv_tp_ytap(i, j)    what tap j multiplies:                           i + H - j, 0 <= j < T: inside [i, i + H]
//   lv_tp_ycentre(i)    y[i - D]:                                        i + H - D
//   lv_tp_ycarry_src    carried'[c] = line[T + c], 0 <= c < H:           T <= . <= H + T - 1
PTTS_LV_HD inline int lv_tp_ycur(int i) { return PTTS_LV_TP_H + i; }
PTTS_LV_HD inline int lv_tp_ytap(int i, int j) { return i + PTTS_LV_TP_H - j; }
PTTS_LV_HD inline int lv_tp_ycentre(int i) { return i + PTTS_LV_TP_H - PTTS_LV_TP_D; }
PTTS_LV_HD inline int lv_tp_ycarry_src(int c, int T) { return T + c; }
