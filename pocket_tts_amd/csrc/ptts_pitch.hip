// Per-request pitch: a streaming pitch shift by r = P / Q behind the stretcher (or whatever stage comes before it):
// WSOLA by r, then a polyphase FIR by Q / P (include/ptts.h, "pitch"; plan rule: pocket_tts_amd/pitch.py; index functions
// and their bounds: ptts_pitch.h and, for the WSOLA part, ptts_stretch.h).
//
// One launch per frame, one workgroup per row (a row's hops depend on each other):
//   stage      w = carried || frame of the row in LDS, the carry (second half of the last segment) beside it
//   per hop    as stretch_kernel: the 2 D + 1 candidate scores from LDS, a workgroup argmax over (score, preference),
//              overlap-add; the hop's Hs samples go to the row's mid line in device memory, behind its PTTS_PT_HIST
//              history samples (w, the carry and the scores fill the 64 KB of LDS; a mid line is up to 31 KB more)
//   FIR        after the last hop's barrier every thread computes outputs from the mid line, taps in index order.  The
//              line is row-private: the workgroup that wrote it reads it back, no other block touches it
//   state      the same workgroup writes the row's carried samples, carry, delta and the line's new history
// Rows on an identity plan copy their frame and exit.
#include "ptts_stage.h"
#include "ptts_pitch.h"

struct ptts_pitcher : StageBase {
  int mid_max = 0, k_max = 0, lds_floats = 0;
  float *windows = nullptr;  // the plans' W = 2 Hs window floats, one after the other
  float *tables = nullptr;   // the plans' [Q][T] polyphase tables, one after the other
  PtPlan *plans = nullptr;   // [n_plans]
  int *row_delta = nullptr;  // [B][2]: delta of the row's last hop, and whether the row has had a hop at all
  float *hist = nullptr;     // [B][PTTS_TS_HIST]: the row's last `reach` input samples at the front of its line
  float *carry = nullptr;    // [B][PTTS_TS_MAX_HS]: second half of the row's last segment
  float *mid = nullptr;      // [B][PTTS_PT_HIST + mid_max]: the row's mid line, its history at the front
};

constexpr int kPtMaxPlans = 256;
constexpr int kPtMaxFrame = 8192;
constexpr int kPtThreads = 1024;
constexpr int kPtMaxChunks = 16;
static_assert(PTTS_TS_MAX_CAND <= kPtThreads, "one thread per candidate in the argmax");
static_assert(PTTS_PT_HIST <= kPtThreads, "one thread per history sample");

__device__ inline bool pt_better(float sa, int ca, float sb, int cb) { return sa > sb || (sa == sb && ca < cb); }

__device__ inline void pt_store(float *out_f, int16_t *out_i, size_t o, float v) {
  if (out_i) out_i[o] = (int16_t)(fminf(fmaxf(v, -1.0f), 1.0f) * 32767.0f);
  else out_f[o] = v;
}

__global__ __launch_bounds__(kPtThreads) void pitch_kernel(const float *__restrict__ in, int width,
                                                           const PtPlan *__restrict__ plans, int n_plans,
                                                           const float *__restrict__ windows, const float *__restrict__ tables,
                                                           const int *__restrict__ row_plan, const int *__restrict__ row_drain,
                                                           int *__restrict__ row_delta, float *__restrict__ hist,
                                                           float *__restrict__ carry, float *mid, int mid_max,
                                                           float *__restrict__ out_f, int16_t *__restrict__ out_i,
                                                           int *__restrict__ d_delta, int k_max, float *__restrict__ d_mid) {
  extern __shared__ float w[];  // reach + n of the row's plan (<= the launch's request, ptts_pitcher_create)
  __shared__ float part[PTTS_TS_MAX_CAND];  // [Q][2 D + 1] partial scores, Q (2 D + 1) <= kPtThreads
  __shared__ float cy[PTTS_TS_MAX_HS];
  __shared__ float red_s[kPtThreads / 64];
  __shared__ int red_c[kPtThreads / 64];
  __shared__ int best_c;
  const int row = blockIdx.x, tid = threadIdx.x;
  const PtPlan PP = plans[min(max(row_plan[row], 0), n_plans - 1)];
  const TsPlan P = PP.ts;
  const bool drain = row_drain[row] != 0;
  const float *x = in + (size_t)row * width;  // n <= width (ptts_pitcher_create)
  const size_t o0 = (size_t)row * width;      // n_out = n
  if (ts_identity(P.Ha, P.Hs)) {              // uniform: the whole block leaves
    for (int i = tid; i < P.n_in; i += kPtThreads) pt_store(out_f, out_i, o0 + i, drain ? 0.f : x[i]);
    return;
  }
  const int Ha = P.Ha, Hs = P.Hs, D = P.D, L = P.L, reach = P.reach, n_mid = P.n_out;
  float *hrow = hist + (size_t)row * PTTS_TS_HIST;               // reach <= PTTS_TS_HIST
  float *crow = carry + (size_t)row * PTTS_TS_MAX_HS;            // Hs <= PTTS_TS_MAX_HS
  float *m = mid + (size_t)row * (PTTS_PT_HIST + mid_max);       // n_mid <= mid_max
  for (int i = tid; i < reach + P.n_in; i += kPtThreads) w[i] = i < reach ? hrow[i] : (drain ? 0.f : x[i - reach]);
  for (int n = tid; n < Hs; n += kPtThreads) cy[n] = crow[n];
  int dprev = row_delta[2 * row];
  bool started = row_delta[2 * row + 1] != 0;
  __syncthreads();
  const float *win = windows + P.woff;
  const int nc = 2 * D + 1;                                       // <= PTTS_TS_MAX_CAND = kPtThreads
  const int Qc = max(1, min(kPtThreads / nc, kPtMaxChunks));      // Qc * nc <= kPtThreads
  const int chunk = (Hs + Qc - 1) / Qc;
  for (int j = 0; j < P.K; ++j) {
    int delta = 0;  // hop 0 of a stream
    if (started) {
      const float *t = w + ts_tmpl(j, dprev, Ha, Hs, D, L);
      if (tid < Qc * nc) {
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
        for (int q = 1; q < Qc; ++q) sc += part[q * nc + c];
      }
      // (score, preference) is a total order on finite scores: the result does not depend on the order of the reduction
      for (int off = 32; off > 0; off >>= 1) {
        const float so = __shfl_down(sc, off, 64);
        const int co = __shfl_down(c, off, 64);
        if (pt_better(so, co, sc, c)) { sc = so; c = co; }
      }
      if ((tid & 63) == 0) { red_s[tid >> 6] = sc; red_c[tid >> 6] = c; }
      __syncthreads();
      if (tid == 0) {
        for (int v = 1; v < kPtThreads / 64; ++v)
          if (pt_better(red_s[v], red_c[v], sc, c)) { sc = red_s[v]; c = red_c[v]; }
        best_c = (c >= 0 && c < nc) ? c : 0;  // scores that do not compare (NaN input): still a delta in [-D, D]
      }
      __syncthreads();
      delta = ts_delta_of(best_c);
    }
    const float *s = w + ts_seg(j, delta, Ha, D, L);
    for (int n = tid; n < Hs; n += kPtThreads) {  // sample n of the carry belongs to thread n % kPtThreads throughout
      const float v = cy[n] + win[n] * s[n];
      cy[n] = win[Hs + n] * s[Hs + n];
      m[pt_mid(j, n, Hs)] = v;
      if (d_mid) d_mid[(size_t)row * mid_max + ts_out(j, n, Hs)] = v;  // K Hs = n_mid <= mid_max
    }
    if (tid == 0 && d_delta) d_delta[(size_t)row * k_max + j] = delta;  // K <= k_max
    dprev = delta;
    started = true;
    __syncthreads();  // part, best_c and the red_ lines are written again by the next hop; the mid line is read below
  }
  // the barrier that ends the last hop orders every write of the mid line before these reads (same workgroup)
  const float *tab = tables + PP.toff;
  for (int N = tid; N < P.n_in; N += kPtThreads) pt_store(out_f, out_i, o0 + N, pt_output(tab, m, N, PP.P, PP.Q, PP.T));
  // every read of the row's state but the mid line's is done (w and cy are LDS copies): write it back
  for (int i = tid; i < reach; i += kPtThreads) hrow[i] = w[ts_carry_src(i, P.n_in)];
  for (int n = tid; n < Hs; n += kPtThreads) crow[n] = cy[n];
  if (tid == 0) { row_delta[2 * row] = dprev; row_delta[2 * row + 1] = 1; }
  float keep = 0.f;
  if (tid < PTTS_PT_HIST) keep = m[pt_keep(tid, n_mid)];
  __syncthreads();  // the FIR's reads of the line's front, and the reads of `keep`, are done
  if (tid < PTTS_PT_HIST) m[tid] = keep;
}

__global__ __launch_bounds__(kPtThreads) void pitch_set_row_kernel(int *row_plan, int *row_drain, int *row_delta, float *hist,
                                                                   float *carry, float *mid, int mid_max, int row,
                                                                   int plan_index) {
  const int tid = threadIdx.x;
  if (tid == 0) { row_plan[row] = plan_index; row_drain[row] = 0; row_delta[2 * row] = 0; row_delta[2 * row + 1] = 0; }
  for (int i = tid; i < PTTS_TS_HIST; i += kPtThreads) hist[(size_t)row * PTTS_TS_HIST + i] = 0.f;
  for (int i = tid; i < PTTS_TS_MAX_HS; i += kPtThreads) carry[(size_t)row * PTTS_TS_MAX_HS + i] = 0.f;
  for (int i = tid; i < PTTS_PT_HIST; i += kPtThreads) mid[(size_t)row * (PTTS_PT_HIST + mid_max) + i] = 0.f;
}

int pitch_enqueue(hipStream_t st, ptts_pitcher *ps, const float *d_in, void *out, int is_i16, int *d_delta, float *d_mid) {
  if (!ps || !d_in || !out) return fail(-1, "pitch: null argument");
  const int B = ps->B;
  {
    ProfScope prof(st, "pitch", 4.0 * B * (ps->in_width + 2.0 * PTTS_TS_HIST + 2.0 * ps->mid_max) + (is_i16 ? 2.0 : 4.0) * B * ps->in_width,
                   0);
    pitch_kernel<<<B, kPtThreads, (size_t)ps->lds_floats * sizeof(float), st>>>(
        d_in, ps->in_width, ps->plans, ps->n_plans, ps->windows, ps->tables, ps->row_plan, ps->row_drain, ps->row_delta, ps->hist,
        ps->carry, ps->mid, ps->mid_max, is_i16 ? nullptr : (float *)out, is_i16 ? (int16_t *)out : nullptr, d_delta, ps->k_max,
        d_mid);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int ptts_pitcher_create(ptts_engine *e, int32_t batch, const int32_t *h_plans, int32_t n_plans, const float *h_windows,
                                   int64_t n_window_floats, const float *h_tables, int64_t n_table_floats, ptts_pitcher **out) {
  if (!e || !out || !h_plans || !h_windows || !h_tables) return fail(-1, "pitcher_create: null argument");
  if (batch < 1 || n_plans < 1 || n_plans > kPtMaxPlans) return fail(-1, "pitcher_create: batch or number of plans out of range");
  std::vector<PtPlan> plans(n_plans);
  int64_t off = 0, toff = 0;
  int width = 0, mid_max = 1, k_max = 1, lds = 1;
  for (int i = 0; i < n_plans; ++i) {
    const int32_t *p = h_plans + 8 * i;
    const int n = p[0], Ha = p[1], Hs = p[2], D = p[3], L = p[4], P = p[5], Q = p[6], T = p[7];
    if (!pt_plan_ok(n, Ha, Hs, D, L, P, Q, T, kPtMaxFrame, PTTS_PT_MAX_MID))
      return fail(-1, "pitcher_create: plan " + std::to_string(i) + " (n " + std::to_string(n) + ", Ha " + std::to_string(Ha) +
                          ", Hs " + std::to_string(Hs) + ", D " + std::to_string(D) + ", L " + std::to_string(L) + ", P " +
                          std::to_string(P) + ", Q " + std::to_string(Q) + ", T " + std::to_string(T) + ") is not admissible");
    const bool id = ts_identity(Ha, Hs);
    plans[i].ts = TsPlan{n, Ha, Hs, D, L, n / Ha, n / Ha * Hs, id ? 0 : ts_reach(Ha, D, L), (int32_t)off};
    plans[i].P = P; plans[i].Q = Q; plans[i].T = T; plans[i].toff = (int32_t)toff;
    off += 2 * (int64_t)Hs;
    toff += (int64_t)Q * T;
    width = std::max(width, n);
    if (!id) mid_max = std::max(mid_max, (int)plans[i].ts.n_out);  // <= PTTS_PT_MAX_MID (pt_plan_ok)
    if (!id) k_max = std::max(k_max, (int)plans[i].ts.K);
    if (!id) lds = std::max(lds, plans[i].ts.reach + n);  // <= PTTS_TS_WINDOW (ts_plan_ok)
  }
  if (off != n_window_floats) return fail(-1, "pitcher_create: the windows do not hold sum(2 * Hs) floats");
  if (toff != n_table_floats) return fail(-1, "pitcher_create: the tables do not hold sum(Q * T) floats");
  StageLock lock;
  ptts_pitcher *ps;
  CHK(stage_new(e, batch, n_plans, width, width, lock, &ps));
  ps->mid_max = mid_max; ps->k_max = k_max; ps->lds_floats = lds;
  stage_copy(*ps, ps->windows, h_windows, (size_t)off);
  stage_copy(*ps, ps->tables, h_tables, (size_t)toff);
  stage_copy(*ps, ps->plans, plans.data(), n_plans);
  stage_zeros(*ps, ps->row_plan, batch);
  stage_zeros(*ps, ps->row_drain, batch);
  stage_zeros(*ps, ps->row_delta, (size_t)batch * 2);
  stage_zeros(*ps, ps->hist, (size_t)batch * PTTS_TS_HIST);
  stage_zeros(*ps, ps->carry, (size_t)batch * PTTS_TS_MAX_HS);
  stage_zeros(*ps, ps->mid, (size_t)batch * (PTTS_PT_HIST + mid_max));
  return stage_finish(ps, out, "pitcher_create");
}

extern "C" void ptts_pitcher_destroy(ptts_pitcher *ps) { stage_destroy(ps); }

extern "C" int ptts_pitcher_set_row(ptts_pitcher *ps, int32_t row, int32_t plan_index, void *stream) {
  CHK(stage_row_ok(ps, "pitcher_set_row", "pitcher", row, "plan", plan_index, 0));
  StageLock lock;
  CHK(stage_enter(ps->e, lock));
  pitch_set_row_kernel<<<1, kPtThreads, 0, S(ps->e, stream)>>>(ps->row_plan, ps->row_drain, ps->row_delta, ps->hist, ps->carry,
                                                              ps->mid, ps->mid_max, row, plan_index);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int ptts_pitcher_set_row_drain(ptts_pitcher *ps, int32_t row, int32_t on, void *stream) {
  return stage_set_row_drain(ps, "pitcher_set_row_drain", "pitcher", row, on, stream);
}

extern "C" int ptts_pitch_frame(ptts_pitcher *ps, const float *d_in, void *out, int32_t is_i16, int32_t *d_delta, float *d_mid,
                                void *stream) {
  return stage_frame(ps, d_in && out, "pitch_frame", stream,
                     [&](hipStream_t st) { return pitch_enqueue(st, ps, d_in, out, is_i16 != 0, d_delta, d_mid); });
}
