// Per-request loudness target: a streaming ITU-R BS.1770-4 normaliser, the output stage between the pitcher and the leveler
// (include/ptts.h, "loudness"; contract and plan rule: pocket_tts_amd/loudness.py; index functions and their bounds:
// ptts_loud.h).
//
// One launch per frame, one workgroup per row.  The K-weighting (two cascaded biquads) is one 4-state linear recurrence
// s' = A s + B x in float64:
//   chunk    thread t runs samples [t chunk, (t + 1) chunk) from a zero state (thread 0 from the row's carried state)
//   scan     the chunk end states are combined over the threads, E[t] += A^(chunk 2^k) E[t - 2^k], k = 0, 1, ..: E[t - 1]
//            is then the true state at thread t's first sample
//   energy   each thread re-runs its chunk from that state and adds w^2 to the one or two sub-blocks its chunk touches;
//            wave g sums the threads' shares of the frame's g-th sub-block
//   gate     for every sub-block the frame completes: z, the gating block Z into the row's history, L over the history by
//            two block reductions (absolute gate, relative gate), the gain c
//   output   y[i] = (k_j + (k_{j+1} - k_j) phase / S) x[i - D] in fp32 from the row's delay ring, then the frame's last D
//            input samples into the ring
// The order of every sum is fixed by the sample's index in its frame and the row's position in its own stream, so a row's
// output does not depend on its slot or on the batch.  Bypass rows copy their line and exit.
#include <cmath>
#include <cstring>

#include "ptts_stage.h"
#include "ptts_loud.h"

constexpr int kLdDoubles = 12;  // per row: s[4], the open sub-block's partial sum, z[4], last L, last Z, the target T
constexpr int kLdInts = 3;      // per row: pos, cnt, the ring's head
constexpr int kLdWaves = PTTS_LD_THREADS / 64;
static_assert((1 << PTTS_LD_SCAN) == PTTS_LD_THREADS, "the scan covers every thread");
static_assert(PTTS_LD_SEGS <= kLdWaves, "one wave per sub-block a frame touches");
static_assert(PTTS_LD_HIST <= PTTS_LD_THREADS, "one history entry per thread");

struct ptts_loudnorm : StageBase {  // row_plan < 0: bypass
  LdPlan *plans = nullptr;    // [n_plans]
  double *row_d = nullptr;    // [B][kLdDoubles]
  int *row_i = nullptr;       // [B][kLdInts]
  float *row_c = nullptr;     // [B][3]: the gains of the last three completed sub-blocks
  double *hist = nullptr;     // [B][PTTS_LD_HIST]: gating-block energies
  float *ring = nullptr;      // [B][PTTS_LD_MAX_D]: delayed samples
};

__device__ inline double ld_wave_sum(double v) {
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ inline int ld_wave_sum(int v) {
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ inline double ld_lufs(double Z) { return -0.691 + 10.0 * log10(Z); }

__global__ __launch_bounds__(PTTS_LD_THREADS) void loud_kernel(const float *__restrict__ in, float *__restrict__ out, int width,
                                                               const LdPlan *__restrict__ plans, int n_plans,
                                                               const int *__restrict__ row_plan,
                                                               const int *__restrict__ row_drain, double *__restrict__ row_d,
                                                               int *__restrict__ row_i, float *__restrict__ row_c,
                                                               double *__restrict__ hist, float *__restrict__ ring,
                                                               double *__restrict__ tap) {
  // chunk end states (scan_block): two halves of 32 KB, one barrier per scan step where one half scanned in place took two.
  // With P and the small arrays below the workgroup holds 82,552 B of LDS, more than the 64 KB of older parts and within the
  // 160 KB of a gfx950 CU, which the kernel's 123 VGPRs limit to one such workgroup anyway
  __shared__ double E[2 * PTTS_LD_THREADS * LdWeighting::W];
  static_assert(sizeof(E) + sizeof(double) * 2 * PTTS_LD_THREADS <= 96 * 1024, "E and P leave room in a CU's 160 KB of LDS");
  __shared__ double P[PTTS_LD_THREADS][2];  // a thread's share of its first and its second sub-block
  __shared__ double segsum[kLdWaves];
  __shared__ double wsum[2][kLdWaves];
  __shared__ int wcnt[2][kLdWaves];
  __shared__ double zr[4], shZ, shL, shLastZ;
  __shared__ int shAppend;
  __shared__ float cc[PTTS_LD_CC];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float *x = in + (size_t)row * width;  // n <= width (ptts_loudnorm_create)
  float *y = out + (size_t)row * width;
  const int pi = row_plan[row];
  if (pi < 0) {  // bypass (uniform: the whole block leaves): a row without a plan has no n, its whole line is copied
    for (int i = tid; i < width; i += PTTS_LD_THREADS) y[i] = x[i];
    return;
  }
  const LdPlan &Pl = plans[min(pi, n_plans - 1)];
  const int n = Pl.n, S = Pl.S, D = Pl.D, chunk = Pl.chunk, nT = Pl.threads;  // ld_plan_ok, ptts_loudnorm_create
  const bool drain = row_drain[row] != 0;
  double *rd = row_d + (size_t)row * kLdDoubles;
  int *ri = row_i + (size_t)row * kLdInts;
  float *rc = row_c + (size_t)row * 3;
  double *hrow = hist + (size_t)row * PTTS_LD_HIST;
  float *rrow = ring + (size_t)row * PTTS_LD_MAX_D;
  const int pos = ri[0], cnt = ri[1], head = ri[2];
  const double part = rd[4], T = rd[11];
  LdWeighting kw;
  for (int q = 0; q < PTTS_LD_COEFS; ++q) kw.c[q] = Pl.coef[q];
  kw.pw = Pl.pw[0];
  if (tid == 0) {
    for (int q = 0; q < 4; ++q) zr[q] = rd[5 + q];
    shL = rd[9]; shLastZ = rd[10];
    for (int q = 0; q < 3; ++q) cc[q] = rc[q];
  }
  const int done = ld_done(pos, n, S);  // <= PTTS_LD_MAX_DONE

  // chunk, scan, energy: the thread's samples; the re-run from the true state adds w^2 to the thread's two shares, and the
  // last thread leaves the row's state after the frame in rd[0 .. 3]
  const int i0 = ld_begin(tid, chunk), i1 = tid < nT ? ld_end(tid, chunk, n) : i0;
  double xr[PTTS_LD_MAX_CHUNK];
#pragma unroll
  for (int q = 0; q < PTTS_LD_MAX_CHUNK; ++q) xr[q] = (!drain && i0 + q < i1) ? (double)x[i0 + q] : 0.0;
  const int seg0 = ld_seg(pos, i0, S);
  double pa = 0.0, pb = 0.0;
  scan_block<PTTS_LD_MAX_CHUNK, PTTS_LD_THREADS>(kw, E, tid, nT, scan_steps(nT), rd, xr, i1 - i0, [&](int q, double w) {
    if (ld_seg(pos, i0 + q, S) == seg0) pa += w * w;
    else pb += w * w;
  });
  P[tid][0] = pa; P[tid][1] = pb;
  __syncthreads();
  if (wave <= done) {  // wave g: the frame's g-th sub-block, threads in ascending order per lane, then across the lanes
    double a = 0.0;
    for (int t = lane; t < nT; t += 64) {
      const int sg = ld_seg(pos, ld_begin(t, chunk), S);
      a += sg == wave ? P[t][0] : (sg + 1 == wave ? P[t][1] : 0.0);
    }
    a = ld_wave_sum(a);
    if (lane == 0) segsum[wave] = a;
  }
  __syncthreads();

  // gate: one round per completed sub-block; thread t holds history entry t
  const int have = min(max(cnt - 3, 0), PTTS_LD_HIST);
  double hz = tid < have ? hrow[tid] : 0.0;
  bool hon = tid < have;
  for (int g = 0; g < done; ++g) {
    const int m = cnt + g;  // the sub-block's number
    if (tid == 0) {
      const double z = ((g == 0 ? part : 0.0) + segsum[g]) / (double)S;
      zr[0] = zr[1]; zr[1] = zr[2]; zr[2] = zr[3]; zr[3] = z;
      shAppend = 0;
      if (m >= 3 && ld_hist(m) < PTTS_LD_HIST) {
        shZ = (((zr[0] + zr[1]) + zr[2]) + zr[3]) / 4.0;
        shLastZ = shZ;
        hrow[ld_hist(m)] = shZ;
        shAppend = 1;
      }
    }
    __syncthreads();
    const bool app = shAppend != 0;  // uniform
    if (app) {
      if (tid == ld_hist(m)) { hz = shZ; hon = true; }
      const double l = hon ? ld_lufs(hz) : 0.0;
      const bool inA = hon && l > -70.0;
      double a = ld_wave_sum(inA ? hz : 0.0);
      int c = ld_wave_sum(inA ? 1 : 0);
      if (lane == 0) { wsum[0][wave] = a; wcnt[0][wave] = c; }
      __syncthreads();
      a = 0.0; c = 0;
      for (int w = 0; w < kLdWaves; ++w) { a += wsum[0][w]; c += wcnt[0][w]; }
      double L = 0.0;
      bool defined = c > 0;  // uniform
      if (defined) {
        const double gamma = ld_lufs(a / (double)c) - 10.0;
        const bool inR = inA && l > gamma;
        a = ld_wave_sum(inR ? hz : 0.0);
        c = ld_wave_sum(inR ? 1 : 0);
        if (lane == 0) { wsum[1][wave] = a; wcnt[1][wave] = c; }
        __syncthreads();
        a = 0.0; c = 0;
        for (int w = 0; w < kLdWaves; ++w) { a += wsum[1][w]; c += wcnt[1][w]; }
        L = ld_lufs(a / (double)c);  // the loudest block of A passes the relative gate: c >= 1
      }
      if (tid == 0) {
        if (defined) {
          shL = L;
          cc[3 + g] = (float)fmin(fmax(pow(10.0, (T - L) / 20.0), 0.1), 10.0);
        } else {
          cc[3 + g] = cc[2 + g];
        }
      }
    } else if (tid == 0) {
      cc[3 + g] = cc[2 + g];
    }
    __syncthreads();
  }

  // output: the delayed samples under the ramped gain
  const float fS = (float)S;
  for (int i = tid; i < n; i += PTTS_LD_THREADS) {
    const int seg = ld_seg(pos, i, S), j = ld_block(cnt, seg);
    float v = 0.f;
    if (j >= 0) {
      const float xd = i < D ? rrow[ld_ring(head, i, D)] : (drain ? 0.f : x[i - D]);
      const float k0 = cc[ld_knot_lo(cnt, j)], k1 = cc[ld_knot_hi(cnt, j)];
      v = (k0 + (k1 - k0) * ((float)ld_phase(pos, i, S) / fS)) * xd;
    }
    y[i] = v;
  }
  __syncthreads();  // every read of the ring is done
  for (int i = tid; i < n; i += PTTS_LD_THREADS)
    if (i + D >= n) rrow[ld_ring(head, i, D)] = drain ? 0.f : x[i];
  if (tid == 0) {
    ri[0] = ld_phase(pos, n, S); ri[1] = cnt + done; ri[2] = ld_ring(head, n, D);
    rd[4] = (done == 0 ? part : 0.0) + segsum[done];
    for (int q = 0; q < 4; ++q) rd[5 + q] = zr[q];
    rd[9] = shL; rd[10] = shLastZ;
    for (int q = 0; q < 3; ++q) rc[q] = cc[done + q];
    if (tap) {
      tap[4 * row] = (double)(cnt + done); tap[4 * row + 1] = shL; tap[4 * row + 2] = (double)cc[done + 2];
      tap[4 * row + 3] = shLastZ;
    }
  }
}

__global__ __launch_bounds__(PTTS_LD_THREADS) void loud_set_row_kernel(int *row_plan, int *row_drain, double *row_d, int *row_i,
                                                                       float *row_c, float *ring, int row, int plan_index,
                                                                       double target) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    row_plan[row] = plan_index; row_drain[row] = 0;
    double *rd = row_d + (size_t)row * kLdDoubles;
    for (int q = 0; q < kLdDoubles; ++q) rd[q] = 0.0;
    rd[9] = nan("");  // L is undefined until a gating block passes the absolute gate
    rd[11] = target;
    for (int q = 0; q < kLdInts; ++q) row_i[row * kLdInts + q] = 0;
    for (int q = 0; q < 3; ++q) row_c[row * 3 + q] = 1.f;
  }
  for (int i = tid; i < PTTS_LD_MAX_D; i += PTTS_LD_THREADS) ring[(size_t)row * PTTS_LD_MAX_D + i] = 0.f;
}

int loud_enqueue(hipStream_t st, ptts_loudnorm *ln, const float *d_in, float *d_out, double *d_tap) {
  if (!ln || !d_in || !d_out) return fail(-1, "loudnorm: null argument");
  if (d_in == d_out) return fail(-1, "loudnorm: the stage does not work in place");
  const int B = ln->B;
  {
    ProfScope ps(st, "loudnorm", 4.0 * B * (3.0 * ln->in_width + 2.0 * PTTS_LD_MAX_D) + 8.0 * B * PTTS_LD_HIST, 0);
    loud_kernel<<<B, PTTS_LD_THREADS, 0, st>>>(d_in, d_out, ln->in_width, ln->plans, ln->n_plans, ln->row_plan, ln->row_drain,
                                               ln->row_d, ln->row_i, ln->row_c, ln->hist, ln->ring, d_tap);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int ptts_loudnorm_create(ptts_engine *e, int32_t batch, const int32_t *h_plans, int32_t n_plans,
                                    const double *h_doubles, int64_t n_doubles, ptts_loudnorm **out) {
  if (!e || !out || !h_plans || !h_doubles) return fail(-1, "loudnorm_create: null argument");
  if (batch < 1 || n_plans < 1 || n_plans > 256) return fail(-1, "loudnorm_create: batch or number of plans out of range");
  if (n_doubles != (int64_t)n_plans * PTTS_LD_PLAN_DOUBLES)
    return fail(-1, "loudnorm_create: expected " + std::to_string(PTTS_LD_PLAN_DOUBLES) + " doubles per plan");
  std::vector<LdPlan> plans(n_plans);
  int width = 0;
  for (int i = 0; i < n_plans; ++i) {
    LdPlan &P = plans[i];
    P.rate = h_plans[2 * i]; P.n = h_plans[2 * i + 1];
    if (!ld_plan_ok(P.rate, P.n))
      return fail(-1, "loudnorm_create: plan " + std::to_string(i) + " (rate " + std::to_string(P.rate) + ", n " +
                          std::to_string(P.n) + ") is not admissible");
    P.S = ld_sub(P.rate); P.D = ld_delay(P.rate); P.chunk = ld_chunk(P.n); P.threads = ld_threads(P.n);
    const double *d = h_doubles + (size_t)i * PTTS_LD_PLAN_DOUBLES;
    for (int q = 0; q < PTTS_LD_PLAN_DOUBLES; ++q)
      if (!std::isfinite(d[q])) return fail(-1, "loudnorm_create: plan " + std::to_string(i) + " holds a value that is not finite");
    std::memcpy(P.coef, d, sizeof(P.coef));
    std::memcpy(P.pw, d + PTTS_LD_COEFS, sizeof(P.pw));
    width = std::max(width, (int)P.n);
  }
  StageLock lock;
  ptts_loudnorm *ln;
  CHK(stage_new(e, batch, n_plans, width, width, lock, &ln));
  stage_copy(*ln, ln->plans, plans.data(), n_plans);
  stage_fill(*ln, ln->row_plan, batch, -1);
  stage_zeros(*ln, ln->row_drain, batch);
  stage_zeros(*ln, ln->row_d, (size_t)batch * kLdDoubles);
  stage_zeros(*ln, ln->row_i, (size_t)batch * kLdInts);
  stage_zeros(*ln, ln->row_c, (size_t)batch * 3);
  stage_zeros(*ln, ln->hist, (size_t)batch * PTTS_LD_HIST);
  stage_zeros(*ln, ln->ring, (size_t)batch * PTTS_LD_MAX_D);
  return stage_finish(ln, out, "loudnorm_create");
}

extern "C" void ptts_loudnorm_destroy(ptts_loudnorm *ln) { stage_destroy(ln); }

extern "C" int ptts_loudnorm_set_row(ptts_loudnorm *ln, int32_t row, int32_t plan_index, double target_lufs, void *stream) {
  CHK(stage_row_ok(ln, "loudnorm_set_row", "normaliser", row, "plan", plan_index, -1));
  if (plan_index >= 0 && !(target_lufs >= -40.0 && target_lufs <= -10.0))
    return fail(-1, "loudnorm_set_row: the target must be in [-40, -10] LUFS");
  StageLock lock;
  CHK(stage_enter(ln->e, lock));
  loud_set_row_kernel<<<1, PTTS_LD_THREADS, 0, S(ln->e, stream)>>>(ln->row_plan, ln->row_drain, ln->row_d, ln->row_i, ln->row_c,
                                                                  ln->ring, row, plan_index, plan_index < 0 ? 0.0 : target_lufs);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int ptts_loudnorm_set_row_drain(ptts_loudnorm *ln, int32_t row, int32_t on, void *stream) {
  return stage_set_row_drain(ln, "loudnorm_set_row_drain", "normaliser", row, on, stream);
}

extern "C" int ptts_loudnorm_frame(ptts_loudnorm *ln, const float *d_in, float *d_out, double *d_tap, void *stream) {
  return stage_frame(ln, d_in && d_out, "loudnorm_frame", stream,
                     [&](hipStream_t st) { return loud_enqueue(st, ln, d_in, d_out, d_tap); });
}
