// Per-request tone: a streaming cascade of at most eight biquad sections, the output stage between the pitcher and the
// normaliser (include/ptts.h, "tone"; contract and plan rule: pocket_tts_amd/tone.py; index functions and their bounds:
// ptts_tone.h).
//
// One launch per frame, one workgroup per row.  The cascade is walked section by section, each a 2-state linear recurrence
// s' = A s + B x in float64 over the frame the section before it left in the threads' registers:
//   chunk    thread t runs samples [t chunk, (t + 1) chunk) from a zero state (thread 0 from the row's carried state)
//   scan     the chunk end states are combined over the threads, E[t] += A^(chunk 2^j) E[t - 2^j], j = 0, 1, ..: E[t - 1]
//            is then the true state at thread t's first sample
//   re-run   each thread runs its chunk again from that state and keeps y in place of x; the last thread's end state is the
//            row's carried state of the section
// and after the last section y is rounded to fp32 once and written.
//
// Per section, not as one 2K-state system: the scan of a 16-state system costs a 16 x 16 matrix-vector product per thread
// and step (256 float64 FMAs against 4 here, 2560 doubles of powers per plan against 40 per section) and 128 KB of LDS for
// the end states against 32 KB; and the powers of a single section, two poles of one band, are as well conditioned as the
// band itself, where the powers of the cascade mix the decay rates of every band.  The price is one scan per section, which
// a tone of one to four sections, as every preset is, pays one to four times.
//
// The order of every sum is fixed by the sample's index in its frame, so a row's output does not depend on its slot or on
// the batch.  Bypass rows copy their line and exit.
#include <cmath>
#include <cstring>

#include "ptts_stage.h"
#include "ptts_tone.h"

static_assert((1 << PTTS_TN_SCAN) == PTTS_TN_THREADS, "the scan covers every thread");
static_assert(PTTS_TN_MAX_CHUNK * PTTS_TN_THREADS == PTTS_TN_MAX_N, "a frame of the largest size is covered");

struct ptts_tone : StageBase {  // row_plan < 0: bypass
  TnPlan *plans = nullptr;   // [n_plans]
  double *row_s = nullptr;   // [B][PTTS_TN_ROW_DOUBLES]: the sections' states
};

__global__ __launch_bounds__(PTTS_TN_THREADS) void tone_kernel(const float *__restrict__ in, float *__restrict__ out, int width,
                                                               const TnPlan *__restrict__ plans, int n_plans,
                                                               const int *__restrict__ row_plan, double *__restrict__ row_s) {
  __shared__ double E[2 * PTTS_TN_THREADS * TnSection::W];  // chunk end states (scan_block)
  const int row = blockIdx.x, tid = threadIdx.x;
  const float *x = in + (size_t)row * width;  // n <= width (ptts_tone_create)
  float *y = out + (size_t)row * width;
  const int pi = row_plan[row];
  if (pi < 0) {  // bypass (uniform: the whole block leaves): a row without a plan has no n, its whole line is copied
    for (int i = tid; i < width; i += PTTS_TN_THREADS) y[i] = x[i];
    return;
  }
  const TnPlan &Pl = plans[min(pi, n_plans - 1)];
  const int n = Pl.n, K = Pl.K, chunk = Pl.chunk, nT = Pl.threads;  // tn_plan_ok, ptts_tone_create
  const int steps = tn_steps(nT);                                 // <= PTTS_TN_SCAN
  double *rs = row_s + (size_t)row * PTTS_TN_ROW_DOUBLES;
  const int i0 = tn_begin(tid, chunk), i1 = tid < nT ? tn_end(tid, chunk, n) : i0;  // i1 <= n
  double xr[PTTS_TN_MAX_CHUNK];
#pragma unroll
  for (int q = 0; q < PTTS_TN_MAX_CHUNK; ++q) xr[q] = i0 + q < i1 ? (double)x[i0 + q] : 0.0;

  for (int k = 0; k < K; ++k) {  // k < PTTS_TN_MAX_SECTIONS
    TnSection sec;
    for (int q = 0; q < PTTS_TN_COEFS; ++q) sec.c[q] = Pl.coef[k][q];
    sec.pw = Pl.pw[k][0];
    // chunk, scan, re-run: y in place of x; the last thread leaves the section's state after the frame in rs
    scan_block<PTTS_TN_MAX_CHUNK, PTTS_TN_THREADS>(sec, E, tid, nT, steps, rs + 2 * k, xr, i1 - i0,
                                                   [&](int q, double y) { xr[q] = y; });
    __syncthreads();  // every read of E is done before the next section writes it
  }
#pragma unroll
  for (int q = 0; q < PTTS_TN_MAX_CHUNK; ++q) if (i0 + q < i1) y[i0 + q] = (float)xr[q];
}

__global__ void tone_set_row_kernel(int *row_plan, double *row_s, int row, int plan_index) {
  const int tid = threadIdx.x;
  if (tid == 0) row_plan[row] = plan_index;
  if (tid < PTTS_TN_ROW_DOUBLES) row_s[(size_t)row * PTTS_TN_ROW_DOUBLES + tid] = 0.0;
}

int tone_enqueue(hipStream_t st, ptts_tone *tn, const float *d_in, float *d_out) {
  if (!tn || !d_in || !d_out) return fail(-1, "tone: null argument");
  if (d_in == d_out) return fail(-1, "tone: the stage does not work in place");
  const int B = tn->B;
  {
    ProfScope ps(st, "tone", 4.0 * B * 2.0 * tn->in_width + 8.0 * B * 2.0 * PTTS_TN_ROW_DOUBLES, 0);
    tone_kernel<<<B, PTTS_TN_THREADS, 0, st>>>(d_in, d_out, tn->in_width, tn->plans, tn->n_plans, tn->row_plan, tn->row_s);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int ptts_tone_create(ptts_engine *e, int32_t batch, int32_t line, const int32_t *h_plans, int32_t n_plans,
                                const double *h_doubles, int64_t n_doubles, ptts_tone **out) {
  if (!e || !out || !h_plans || !h_doubles) return fail(-1, "tone_create: null argument");
  if (batch < 1 || n_plans < 1 || n_plans > 1024) return fail(-1, "tone_create: batch or number of plans out of range");
  if (n_doubles != (int64_t)n_plans * PTTS_TN_PLAN_DOUBLES)
    return fail(-1, "tone_create: expected " + std::to_string(PTTS_TN_PLAN_DOUBLES) + " doubles per plan");
  std::vector<TnPlan> plans(n_plans);
  if (line < 0 || line > PTTS_TN_MAX_N) return fail(-1, "tone_create: the line's width is out of range");
  int width = line;
  for (int i = 0; i < n_plans; ++i) {
    TnPlan &P = plans[i];
    const int32_t *h = h_plans + (size_t)i * PTTS_TN_PLAN_INTS;
    P.rate = h[0]; P.n = h[1]; P.K = h[2]; P.pad = 0;
    if (!tn_plan_ok(P.rate, P.n, P.K))
      return fail(-1, "tone_create: plan " + std::to_string(i) + " (rate " + std::to_string(P.rate) + ", n " +
                          std::to_string(P.n) + ", " + std::to_string(P.K) + " sections) is not admissible");
    P.chunk = tn_chunk(P.n); P.threads = tn_threads(P.n);
    const double *d = h_doubles + (size_t)i * PTTS_TN_PLAN_DOUBLES;
    for (int q = 0; q < PTTS_TN_PLAN_DOUBLES; ++q)
      if (!std::isfinite(d[q])) return fail(-1, "tone_create: plan " + std::to_string(i) + " holds a value that is not finite");
    std::memcpy(P.coef, d, sizeof(P.coef));
    std::memcpy(P.pw, d + PTTS_TN_MAX_SECTIONS * PTTS_TN_COEFS, sizeof(P.pw));
    if (line > 0 && P.n > line)
      return fail(-1, "tone_create: plan " + std::to_string(i) + " has frames of " + std::to_string(P.n) +
                          " samples, longer than the line of " + std::to_string(line));
    width = std::max(width, (int)P.n);
  }
  StageLock lock;
  ptts_tone *tn;
  CHK(stage_new(e, batch, n_plans, width, width, lock, &tn));
  stage_copy(*tn, tn->plans, plans.data(), n_plans);
  stage_fill(*tn, tn->row_plan, batch, -1);
  stage_zeros(*tn, tn->row_s, (size_t)batch * PTTS_TN_ROW_DOUBLES);
  return stage_finish(tn, out, "tone_create");
}

extern "C" void ptts_tone_destroy(ptts_tone *tn) { stage_destroy(tn); }

extern "C" int ptts_tone_set_row(ptts_tone *tn, int32_t row, int32_t plan_index, void *stream) {
  CHK(stage_row_ok(tn, "tone_set_row", "toner", row, "plan", plan_index, -1));
  StageLock lock;
  CHK(stage_enter(tn->e, lock));
  tone_set_row_kernel<<<1, 64, 0, S(tn->e, stream)>>>(tn->row_plan, tn->row_s, row, plan_index);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int ptts_tone_frame(ptts_tone *tn, const float *d_in, float *d_out, void *stream) {
  return stage_frame(tn, d_in && d_out, "tone_frame", stream, [&](hipStream_t st) { return tone_enqueue(st, tn, d_in, d_out); });
}
