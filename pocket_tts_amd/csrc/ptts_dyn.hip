// Per-request dynamics: a streaming feed-forward speech compressor, the output stage between the toner and the normaliser
// (include/ptts.h, "dynamics"; contract and plan rule: pocket_tts_amd/dynamics.py; index functions, the curve and the sample
// step: ptts_dyn.h).
//
// One launch per frame, one workgroup per row.  Thread t holds samples [t chunk, (t + 1) chunk) in registers and computes
// their wanted reduction c; then the two recurrences run one after the other, each in three steps:
//   chunk    the thread runs its samples from 0 (thread 0 from the row's carried state) and leaves the end value in LDS
//   scan     the chunk ends are combined over the threads in log steps, j = 0, 1, ..:
//              p:  E[t] = max(E[t], aR^(chunk 2^j) E[t - 2^j])      (the leveler's max(c, A d) form)
//              s:  E[t] += aA^(chunk 2^j) E[t - 2^j]                (a one-state linear recurrence)
//            E[t - 1] is then the true value in front of thread t's first sample
//   re-run   each thread runs its chunk again from that value and keeps p in place of c, then s in place of p
// and y = fp32(exp((M - s) K) x) is written.  The last active thread stores p and s as the row's carried state.
//
// The order of every operation is fixed by the sample's index in its frame, so a row's output does not depend on its slot
// or on the batch.  Bypass rows copy their line and exit.
#include <cmath>
#include <cstring>

#include "ptts_stage.h"
#include "ptts_dyn.h"

static_assert((1 << PTTS_DY_SCAN) == PTTS_DY_THREADS, "the scan covers every thread");
static_assert(PTTS_DY_MAX_CHUNK * PTTS_DY_THREADS == PTTS_DY_MAX_N, "a frame of the largest size is covered");

struct ptts_dynamics : StageBase {  // row_plan < 0: bypass
  DyPlan *plans = nullptr;   // [n_plans]
  double *row_s = nullptr;   // [B][PTTS_DY_ROW_DOUBLES]: p, s
};

// The two scans are written out here and do not go through scan_block (ptts_scan.h): through it the same operations came
// out in another schedule, 0.3 us slower at n = 1920.  The partition is the shared one, and DyPeak / DySmooth (ptts_dyn.h)
// state the two recurrences for the shared scheme, which the host sweep walks.
__global__ __launch_bounds__(PTTS_DY_THREADS) void dyn_kernel(const float *__restrict__ in, float *__restrict__ out, int width,
                                                              const DyPlan *__restrict__ plans, int n_plans,
                                                              const int *__restrict__ row_plan, double *__restrict__ row_s) {
  __shared__ double E[2][PTTS_DY_THREADS];  // chunk end values: a scan step reads one half and writes the other
  const int row = blockIdx.x, tid = threadIdx.x;
  const float *x = in + (size_t)row * width;  // n <= width (ptts_dynamics_create)
  float *y = out + (size_t)row * width;
  const int pi = row_plan[row];
  if (pi < 0) {  // bypass (uniform: the whole block leaves): a row without a plan has no n, its whole line is copied
    for (int i = tid; i < width; i += PTTS_DY_THREADS) y[i] = x[i];
    return;
  }
  const DyPlan &Pl = plans[min(pi, n_plans - 1)];
  const int n = Pl.n, chunk = Pl.chunk, nT = Pl.threads;  // dyn_plan_ok, ptts_dynamics_create
  const int steps = dy_steps(nT);                         // <= PTTS_DY_SCAN
  const double T = Pl.T, k = Pl.k, W = Pl.W, M = Pl.M, aA = Pl.aA, aR = Pl.aR;
  double *rs = row_s + (size_t)row * PTTS_DY_ROW_DOUBLES;
  const bool on = tid < nT;
  const int i0 = dy_begin(tid, chunk), i1 = on ? dy_end(tid, chunk, n) : i0;  // i1 <= n
  float xr[PTTS_DY_MAX_CHUNK];
  double v[PTTS_DY_MAX_CHUNK];  // c, then p, then s of the thread's samples
#pragma unroll
  for (int q = 0; q < PTTS_DY_MAX_CHUNK; ++q) {
    xr[q] = i0 + q < i1 ? x[i0 + q] : 0.0f;
    v[q] = i0 + q < i1 ? dy_curve(dy_level((double)xr[q]), T, k, W) : 0.0;
  }

  // ---- p[i] = max(c[i], aR p[i - 1]) ----
  double a = tid == 0 ? rs[0] : 0.0, a0 = a;
  if (on) {
#pragma unroll
    for (int q = 0; q < PTTS_DY_MAX_CHUNK; ++q) if (i0 + q < i1) a = dy_peak(v[q], aR, a);
    E[0][tid] = a;
  }
  __syncthreads();
  int cur = 0;
  for (int j = 0; j < steps; ++j) {
    const int off = 1 << j;
    if (on) {
      if (tid >= off) a = dy_peak(a, Pl.pwR[j], E[cur][tid - off]);
      E[cur ^ 1][tid] = a;
    }
    __syncthreads();
    cur ^= 1;
  }
  if (on) {
    if (tid > 0) a0 = E[cur][tid - 1];
#pragma unroll
    for (int q = 0; q < PTTS_DY_MAX_CHUNK; ++q) if (i0 + q < i1) v[q] = a0 = dy_peak(v[q], aR, a0);
    if (tid == nT - 1) rs[0] = a0;  // p after the frame
  }
  __syncthreads();  // every read of E is done before the second scan writes it

  // ---- s[i] = aA s[i - 1] + (1 - aA) p[i] ----
  a = tid == 0 ? rs[1] : 0.0;
  a0 = a;
  if (on) {
#pragma unroll
    for (int q = 0; q < PTTS_DY_MAX_CHUNK; ++q) if (i0 + q < i1) a = dy_smooth(v[q], aA, a);
    E[0][tid] = a;
  }
  __syncthreads();
  cur = 0;
  for (int j = 0; j < steps; ++j) {
    const int off = 1 << j;
    if (on) {
      if (tid >= off) a += Pl.pwA[j] * E[cur][tid - off];
      E[cur ^ 1][tid] = a;
    }
    __syncthreads();
    cur ^= 1;
  }
  if (on) {
    if (tid > 0) a0 = E[cur][tid - 1];
#pragma unroll
    for (int q = 0; q < PTTS_DY_MAX_CHUNK; ++q)
      if (i0 + q < i1) {
        a0 = dy_smooth(v[q], aA, a0);
        y[i0 + q] = (float)(dy_gain(M, a0) * (double)xr[q]);
      }
    if (tid == nT - 1) rs[1] = a0;  // s after the frame
  }
}

__global__ void dyn_set_row_kernel(int *row_plan, double *row_s, int row, int plan_index) {
  const int tid = threadIdx.x;
  if (tid == 0) row_plan[row] = plan_index;
  if (tid < PTTS_DY_ROW_DOUBLES) row_s[(size_t)row * PTTS_DY_ROW_DOUBLES + tid] = 0.0;
}

int dyn_enqueue(hipStream_t st, ptts_dynamics *dy, const float *d_in, float *d_out) {
  if (!dy || !d_in || !d_out) return fail(-1, "dynamics: null argument");
  if (d_in == d_out) return fail(-1, "dynamics: the stage does not work in place");
  const int B = dy->B;
  {
    ProfScope ps(st, "dynamics", 4.0 * B * 2.0 * dy->in_width + 8.0 * B * 2.0 * PTTS_DY_ROW_DOUBLES, 0);
    dyn_kernel<<<B, PTTS_DY_THREADS, 0, st>>>(d_in, d_out, dy->in_width, dy->plans, dy->n_plans, dy->row_plan, dy->row_s);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int ptts_dynamics_create(ptts_engine *e, int32_t batch, int32_t line, const int32_t *h_plans, int32_t n_plans,
                                    const double *h_doubles, int64_t n_doubles, ptts_dynamics **out) {
  if (!e || !out || !h_plans || !h_doubles) return fail(-1, "dynamics_create: null argument");
  if (batch < 1 || n_plans < 1 || n_plans > 1024) return fail(-1, "dynamics_create: batch or number of plans out of range");
  if (n_doubles != (int64_t)n_plans * PTTS_DY_PLAN_DOUBLES)
    return fail(-1, "dynamics_create: expected " + std::to_string(PTTS_DY_PLAN_DOUBLES) + " doubles per plan");
  std::vector<DyPlan> plans(n_plans);
  if (line < 0 || line > PTTS_DY_MAX_N) return fail(-1, "dynamics_create: the line's width is out of range");
  int width = line;
  for (int i = 0; i < n_plans; ++i) {
    DyPlan &P = plans[i];
    const int32_t *h = h_plans + (size_t)i * PTTS_DY_PLAN_INTS;
    P.rate = h[0]; P.n = h[1];
    if (!dyn_plan_ok(P.rate, P.n))
      return fail(-1, "dynamics_create: plan " + std::to_string(i) + " (rate " + std::to_string(P.rate) + ", n " +
                          std::to_string(P.n) + ") is not admissible");
    P.chunk = dy_chunk(P.n); P.threads = dy_threads(P.n);
    const double *d = h_doubles + (size_t)i * PTTS_DY_PLAN_DOUBLES;
    for (int q = 0; q < PTTS_DY_PLAN_DOUBLES; ++q)
      if (!std::isfinite(d[q]))
        return fail(-1, "dynamics_create: plan " + std::to_string(i) + " holds a value that is not finite");
    P.T = d[0]; P.k = d[1]; P.W = d[2]; P.M = d[3]; P.aA = d[4]; P.aR = d[5];
    std::memcpy(P.pwA, d + 6, sizeof(P.pwA));
    std::memcpy(P.pwR, d + 6 + PTTS_DY_SCAN, sizeof(P.pwR));
    bool ok = dyn_values_ok(P.T, P.k, P.W, P.M, P.aA, P.aR);
    for (int j = 0; j < PTTS_DY_SCAN; ++j) ok = ok && P.pwA[j] >= 0.0 && P.pwA[j] < 1.0 && P.pwR[j] >= 0.0 && P.pwR[j] < 1.0;
    if (!ok) return fail(-1, "dynamics_create: plan " + std::to_string(i) + " holds a value outside the range of its key");
    if (line > 0 && P.n > line)
      return fail(-1, "dynamics_create: plan " + std::to_string(i) + " has frames of " + std::to_string(P.n) +
                          " samples, longer than the line of " + std::to_string(line));
    width = std::max(width, (int)P.n);
  }
  StageLock lock;
  ptts_dynamics *dy;
  CHK(stage_new(e, batch, n_plans, width, width, lock, &dy));
  stage_copy(*dy, dy->plans, plans.data(), n_plans);
  stage_fill(*dy, dy->row_plan, batch, -1);
  stage_zeros(*dy, dy->row_s, (size_t)batch * PTTS_DY_ROW_DOUBLES);
  return stage_finish(dy, out, "dynamics_create");
}

extern "C" void ptts_dynamics_destroy(ptts_dynamics *dy) { stage_destroy(dy); }

extern "C" int ptts_dynamics_set_row(ptts_dynamics *dy, int32_t row, int32_t plan_index, void *stream) {
  CHK(stage_row_ok(dy, "dynamics_set_row", "compressor", row, "plan", plan_index, -1));
  StageLock lock;
  CHK(stage_enter(dy->e, lock));
  dyn_set_row_kernel<<<1, 64, 0, S(dy->e, stream)>>>(dy->row_plan, dy->row_s, row, plan_index);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int ptts_dynamics_frame(ptts_dynamics *dy, const float *d_in, float *d_out, void *stream) {
  return stage_frame(dy, d_in && d_out, "dynamics_frame", stream, [&](hipStream_t st) { return dyn_enqueue(st, dy, d_in, d_out); });
}
