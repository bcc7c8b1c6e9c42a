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
