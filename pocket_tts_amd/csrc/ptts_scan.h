// The chunked scan of a recurrence over one frame: what the toner, the compressor and the normaliser (ptts_tone.h, ptts_dyn.h,
// ptts_loud.h) share, and what the host sweeps under tests/cpp/ drive thread by thread (scan_walk.h there).  Ordinary C++17:
// compiles with g++ as well as under hipcc.
//
// A workgroup of `threads` threads walks a frame of n samples in three steps:
//   chunk    thread t runs its samples [begin, end) from the neutral state (thread 0 from the row's carried state)
//   scan     the chunk end states are combined over the threads in log steps, s[t] <- s[t] (+) P_j s[t - 2^j], j = 0, 1, ..:
//            s[t - 1] is then the true state in front of thread t's first sample
//   re-run   each thread runs its chunk again from that state and keeps what the recurrence gives; the last thread's end
//            state is the row's carried state
// The recurrence is described by a small struct R:
//   R::W                      doubles of its state; all zeros is the neutral state
//   double step(s, x) const   advance s by one sample x, return what the re-run keeps
//   void join(j, e, s) const  s <- s (+) P_j e, with P_j the transition over chunk 2^j samples
#pragma once

#if defined(__HIPCC__)
#define PTTS_SCAN_HD __host__ __device__
#else
#define PTTS_SCAN_HD
#endif

// The partition.  Thread t of the first scan_threads(n, threads) works on samples [t chunk, min((t + 1) chunk, n)):
// 1 <= chunk <= ceil(MAX_N / threads), (used - 1) chunk < n <= used chunk and used <= threads.  A thread t >= used has no
// sample.
PTTS_SCAN_HD inline int scan_chunk(int n, int threads) { return (n + threads - 1) / threads; }
PTTS_SCAN_HD inline int scan_threads(int n, int threads) { return (n + scan_chunk(n, threads) - 1) / scan_chunk(n, threads); }
PTTS_SCAN_HD inline int scan_begin(int t, int chunk) { return t * chunk; }
PTTS_SCAN_HD inline int scan_end(int t, int chunk, int n) { return (t + 1) * chunk < n ? (t + 1) * chunk : n; }
// scan steps a frame of `used` chunks needs: the smallest j with 2^j >= used
PTTS_SCAN_HD inline int scan_steps(int used) {
  int j = 0;
  while ((1 << j) < used) ++j;
  return j;
}

// The per-thread pieces.  x: the thread's cnt <= MAXC samples.
// chunk: s, the state in front of the thread's first sample, becomes the state behind its last
template <int MAXC, class R>
PTTS_SCAN_HD inline void scan_run(const R &r, double *s, const double *x, int cnt) {
#pragma unroll
  for (int q = 0; q < MAXC; ++q)
    if (q < cnt) r.step(s, x[q]);
}
// one scan step of thread t: `ends` holds the threads' states [.][R::W] as the step before left them
template <class R>
PTTS_SCAN_HD inline void scan_join(const R &r, int j, int t, const double *ends, double *s) {
  const int off = 1 << j;
  if (t >= off) r.join(j, ends + (t - off) * R::W, s);
}
// re-run: as scan_run, and keep(q, y) receives what sample q gives
template <int MAXC, class R, class Keep>
PTTS_SCAN_HD inline void scan_rerun(const R &r, double *s, const double *x, int cnt, Keep &&keep) {
#pragma unroll
  for (int q = 0; q < MAXC; ++q)
    if (q < cnt) keep(q, r.step(s, x[q]));
}

#if defined(__HIPCC__)
// The three steps for a whole workgroup of THREADS threads, every thread calling with its own x and cnt (cnt == 0 for
// t >= used) and steps = scan_steps(used).  E is LDS, [2][THREADS][R::W] doubles: a scan step reads one half and writes the
// other.  carry: the row's R::W carried doubles, read by thread 0 and written by thread used - 1.  The caller puts a barrier
// between this call's return and the next write of E.
template <int MAXC, int THREADS, class R, class Keep>
__device__ inline void scan_block(const R &r, double *E, int t, int used, int steps, double *carry, const double *x, int cnt,
                                  Keep &&keep) {
  constexpr int W = R::W, half = THREADS * W;
  const bool on = t < used;
  double s[W] = {}, s0[W];
  if (t == 0) for (int q = 0; q < W; ++q) s[q] = carry[q];
  for (int q = 0; q < W; ++q) s0[q] = s[q];
  if (on) {
    scan_run<MAXC>(r, s, x, cnt);
    for (int q = 0; q < W; ++q) E[t * W + q] = s[q];
  }
  __syncthreads();
  int cur = 0;
  for (int j = 0; j < steps; ++j) {
    if (on) {
      scan_join(r, j, t, E + cur * half, s);
      for (int q = 0; q < W; ++q) E[(cur ^ 1) * half + t * W + q] = s[q];
    }
    __syncthreads();
    cur ^= 1;
  }
  if (on) {
    if (t > 0) for (int q = 0; q < W; ++q) s0[q] = E[cur * half + (t - 1) * W + q];
    scan_rerun<MAXC>(r, s0, x, cnt, keep);
    if (t == used - 1) for (int q = 0; q < W; ++q) carry[q] = s0[q];
  }
}
#endif
