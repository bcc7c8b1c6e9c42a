// Per-request speaking rate: a streaming WSOLA time-stretch behind the codec's last kernel, or behind the resampler
// (include/ptts.h, "speaking rate"; plan rule: pocket_tts_amd/stretch.py; index functions and their bounds: ptts_stretch.h).
//
// One launch per frame, one workgroup per row (a row's hops depend on each other):
//   stage      w = carried || frame of the row in LDS, the carry (second half of the last segment) beside it
//   per hop    the 2 D + 1 candidate scores in parallel from LDS (each dot product in Q fixed chunks, summed in a fixed
//              order), a workgroup argmax over (score, preference), overlap-add, emit Hs samples
//   state      after the last read the same workgroup writes the row's carried samples, carry and delta: no other block
//              reads them, so there is no second launch
// Rows on an identity plan copy their frame and exit.
#include "ptts_stage.h"
#include "ptts_stretch.h"

struct ptts_stretcher : StageBase {  // in_width: in_max, out_width: out_max
  int k_max = 0, lds_floats = 0;
  float *windows = nullptr;  // the plans' W = 2 Hs window floats, one after the other
  TsPlan *plans = nullptr;   // [n_plans]
  int *row_delta = nullptr;  // [B][2]: delta of the row's last hop, and whether the row has had a hop at all
  float *hist = nullptr;     // [B][PTTS_TS_HIST]: the row's last `reach` input samples at the front of its line
  float *carry = nullptr;    // [B][PTTS_TS_MAX_HS]: second half of the row's last segment
};

constexpr int kTsMaxPlans = 256;
constexpr int kTsMaxFrame = 8192;
constexpr int kTsThreads = 1024;
constexpr int kTsMaxChunks = 16;
static_assert(PTTS_TS_MAX_CAND <= kTsThreads, "one thread per candidate in the argmax");

__device__ inline bool ts_better(float sa, int ca, float sb, int cb) { return sa > sb || (sa == sb && ca < cb); }

__global__ __launch_bounds__(kTsThreads) void stretch_kernel(const float *__restrict__ in, int in_max,
                                                             const TsPlan *__restrict__ plans, int n_plans,
                                                             const float *__restrict__ windows, const int *__restrict__ row_plan,
                                                             const int *__restrict__ row_drain, int *__restrict__ row_delta,
                                                             float *__restrict__ hist, float *__restrict__ carry,
                                                             float *__restrict__ out_f, int16_t *__restrict__ out_i, int out_max,
                                                             int *__restrict__ d_delta, int k_max) {
  extern __shared__ float w[];  // reach + n_in of the row's plan (<= the launch's request, ptts_stretcher_create)
  __shared__ float part[PTTS_TS_MAX_CAND];  // [Q][2 D + 1] partial scores, Q (2 D + 1) <= kTsThreads
  __shared__ float cy[PTTS_TS_MAX_HS];
  __shared__ float red_s[kTsThreads / 64];
  __shared__ int red_c[kTsThreads / 64];
  __shared__ int best_c;
  const int row = blockIdx.x, tid = threadIdx.x;
  const TsPlan P = plans[min(max(row_plan[row], 0), n_plans - 1)];
  const bool drain = row_drain[row] != 0;
  const float *x = in + (size_t)row * in_max;  // n_in <= in_max (ptts_stretcher_create)
  const size_t o0 = (size_t)row * out_max;     // n_out <= out_max
  if (ts_identity(P.Ha, P.Hs)) {               // uniform: the whole block leaves
    for (int i = tid; i < P.n_in; i += kTsThreads) {
      const float v = drain ? 0.f : x[i];
      if (out_i) out_i[o0 + i] = (int16_t)(fminf(fmaxf(v, -1.0f), 1.0f) * 32767.0f);
      else out_f[o0 + i] = v;
    }
    return;
  }
  const int Ha = P.Ha, Hs = P.Hs, D = P.D, L = P.L, reach = P.reach;
  float *hrow = hist + (size_t)row * PTTS_TS_HIST;   // reach <= PTTS_TS_HIST
  float *crow = carry + (size_t)row * PTTS_TS_MAX_HS;  // Hs <= PTTS_TS_MAX_HS
  for (int i = tid; i < reach + P.n_in; i += kTsThreads) w[i] = i < reach ? hrow[i] : (drain ? 0.f : x[i - reach]);
  for (int n = tid; n < Hs; n += kTsThreads) cy[n] = crow[n];
  int dprev = row_delta[2 * row];
  bool started = row_delta[2 * row + 1] != 0;
  __syncthreads();
  const float *win = windows + P.woff;
  const int nc = 2 * D + 1;                                       // <= PTTS_TS_MAX_CAND = kTsThreads
  const int Q = max(1, min(kTsThreads / nc, kTsMaxChunks));       // Q * nc <= kTsThreads
  const int chunk = (Hs + Q - 1) / Q;
  for (int j = 0; j < P.K; ++j) {
    int delta = 0;  // hop 0 of a stream
    if (started) {
      const float *t = w + ts_tmpl(j, dprev, Ha, Hs, D, L);
      if (tid < Q * nc) {
        const int c = tid % nc, q = tid / nc;
        const float *s = w + ts_seg(j, ts_delta_of(c), Ha, D, L);
        const int i1 = min(Hs, (q + 1) * chunk);
        float acc = 0.f;
        for (int i = q * chunk; i < i1; ++i) acc = __builtin_fmaf(t[i], s[i], acc);
        part[q * nc + c] = acc;
      }
      __syncthreads();
      float sc = -INFINITY;
      int c = 0x7fffffff;
      if (tid < nc) {
        c = tid;
        sc = part[c];
        for (int q = 1; q < Q; ++q) sc += part[q * nc + c];
      }
      // (score, preference) is a total order on finite scores: the result does not depend on the order of the reduction
      for (int off = 32; off > 0; off >>= 1) {
        const float so = __shfl_down(sc, off, 64);
        const int co = __shfl_down(c, off, 64);
        if (ts_better(so, co, sc, c)) { sc = so; c = co; }
      }
      if ((tid & 63) == 0) { red_s[tid >> 6] = sc; red_c[tid >> 6] = c; }
      __syncthreads();
      if (tid == 0) {
        for (int v = 1; v < kTsThreads / 64; ++v)
          if (ts_better(red_s[v], red_c[v], sc, c)) { sc = red_s[v]; c = red_c[v]; }
        best_c = (c >= 0 && c < nc) ? c : 0;  // scores that do not compare (NaN input): still a delta in [-D, D]
      }
      __syncthreads();
      delta = ts_delta_of(best_c);
    }
    const float *s = w + ts_seg(j, delta, Ha, D, L);
    for (int n = tid; n < Hs; n += kTsThreads) {  // sample n of the carry belongs to thread n % kTsThreads throughout
      const float v = cy[n] + win[n] * s[n];
      cy[n] = win[Hs + n] * s[Hs + n];
      const size_t o = o0 + ts_out(j, n, Hs);
      if (out_i) out_i[o] = (int16_t)(fminf(fmaxf(v, -1.0f), 1.0f) * 32767.0f);
      else out_f[o] = v;
    }
    if (tid == 0 && d_delta) d_delta[(size_t)row * k_max + j] = delta;  // K <= k_max
    dprev = delta;
    started = true;
    __syncthreads();  // part, best_c and the red_ lines are written again by the next hop
  }
  // every read of the row's state is done (w and cy are LDS copies): write it back
  for (int i = tid; i < reach; i += kTsThreads) hrow[i] = w[ts_carry_src(i, P.n_in)];
  for (int n = tid; n < Hs; n += kTsThreads) crow[n] = cy[n];
  if (tid == 0) { row_delta[2 * row] = dprev; row_delta[2 * row + 1] = 1; }
}

__global__ __launch_bounds__(kTsThreads) void stretch_set_row_kernel(int *row_plan, int *row_drain, int *row_delta, float *hist,
                                                                     float *carry, int row, int plan_index) {
  const int tid = threadIdx.x;
  if (tid == 0) { row_plan[row] = plan_index; row_drain[row] = 0; row_delta[2 * row] = 0; row_delta[2 * row + 1] = 0; }
  for (int i = tid; i < PTTS_TS_HIST; i += kTsThreads) hist[(size_t)row * PTTS_TS_HIST + i] = 0.f;
  for (int i = tid; i < PTTS_TS_MAX_HS; i += kTsThreads) carry[(size_t)row * PTTS_TS_MAX_HS + i] = 0.f;
}

int stretch_enqueue(hipStream_t st, ptts_stretcher *ts, const float *d_in, void *out, int is_i16, int *d_delta) {
  if (!ts || !d_in || !out) return fail(-1, "stretch: null argument");
  const int B = ts->B;
  {
    ProfScope ps(st, "stretch", 4.0 * B * (ts->in_width + 2.0 * PTTS_TS_HIST) + (is_i16 ? 2.0 : 4.0) * B * ts->out_width, 0);
    stretch_kernel<<<B, kTsThreads, (size_t)ts->lds_floats * sizeof(float), st>>>(
        d_in, ts->in_width, ts->plans, ts->n_plans, ts->windows, ts->row_plan, ts->row_drain, ts->row_delta, ts->hist, ts->carry,
        is_i16 ? nullptr : (float *)out, is_i16 ? (int16_t *)out : nullptr, ts->out_width, d_delta, ts->k_max);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int ptts_stretcher_create(ptts_engine *e, int32_t batch, const int32_t *h_plans, int32_t n_plans,
                                     const float *h_windows, int64_t n_window_floats, ptts_stretcher **out) {
  if (!e || !out || !h_plans || !h_windows) return fail(-1, "stretcher_create: null argument");
  if (batch < 1 || n_plans < 1 || n_plans > kTsMaxPlans) return fail(-1, "stretcher_create: batch or number of plans out of range");
  std::vector<TsPlan> plans(n_plans);
  int64_t off = 0;
  int in_max = 0, out_max = 0, k_max = 1, lds = 1;
  for (int i = 0; i < n_plans; ++i) {
    const int32_t *p = h_plans + 5 * i;
    const int n_in = p[0], Ha = p[1], Hs = p[2], D = p[3], L = p[4];
    if (!ts_plan_ok(n_in, Ha, Hs, D, L, kTsMaxFrame))
      return fail(-1, "stretcher_create: plan " + std::to_string(i) + " (n_in " + std::to_string(n_in) + ", Ha " +
                          std::to_string(Ha) + ", Hs " + std::to_string(Hs) + ", D " + std::to_string(D) + ", L " +
                          std::to_string(L) + ") is not admissible");
    const bool id = ts_identity(Ha, Hs);
    plans[i] = TsPlan{n_in, Ha, Hs, D, L, n_in / Ha, n_in / Ha * Hs, id ? 0 : ts_reach(Ha, D, L), (int32_t)off};
    off += 2 * (int64_t)Hs;
    in_max = std::max(in_max, n_in);
    out_max = std::max(out_max, (int)plans[i].n_out);
    if (!id) k_max = std::max(k_max, (int)plans[i].K);
    if (!id) lds = std::max(lds, plans[i].reach + n_in);  // <= PTTS_TS_WINDOW (ts_plan_ok)
  }
  if (off != n_window_floats) return fail(-1, "stretcher_create: the windows do not hold sum(2 * Hs) floats");
  StageLock lock;
  ptts_stretcher *ts;
  CHK(stage_new(e, batch, n_plans, in_max, out_max, lock, &ts));
  ts->k_max = k_max; ts->lds_floats = lds;
  stage_copy(*ts, ts->windows, h_windows, (size_t)off);
  stage_copy(*ts, ts->plans, plans.data(), n_plans);
  stage_zeros(*ts, ts->row_plan, batch);
  stage_zeros(*ts, ts->row_drain, batch);
  stage_zeros(*ts, ts->row_delta, (size_t)batch * 2);
  stage_zeros(*ts, ts->hist, (size_t)batch * PTTS_TS_HIST);
  stage_zeros(*ts, ts->carry, (size_t)batch * PTTS_TS_MAX_HS);
  return stage_finish(ts, out, "stretcher_create");
}

extern "C" void ptts_stretcher_destroy(ptts_stretcher *ts) { stage_destroy(ts); }

extern "C" int ptts_stretcher_set_row(ptts_stretcher *ts, int32_t row, int32_t plan_index, void *stream) {
  CHK(stage_row_ok(ts, "stretcher_set_row", "stretcher", row, "plan", plan_index, 0));
  StageLock lock;
  CHK(stage_enter(ts->e, lock));
  stretch_set_row_kernel<<<1, kTsThreads, 0, S(ts->e, stream)>>>(ts->row_plan, ts->row_drain, ts->row_delta, ts->hist, ts->carry,
                                                                row, plan_index);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int ptts_stretcher_set_row_drain(ptts_stretcher *ts, int32_t row, int32_t on, void *stream) {
  return stage_set_row_drain(ts, "stretcher_set_row_drain", "stretcher", row, on, stream);
}

extern "C" int ptts_stretch_frame(ptts_stretcher *ts, const float *d_in, void *out, int32_t is_i16, int32_t *d_delta,
                                  void *stream) {
  return stage_frame(ts, d_in && out, "stretch_frame", stream,
                     [&](hipStream_t st) { return stretch_enqueue(st, ts, d_in, out, is_i16 != 0, d_delta); });
}
