// Per-request output gain with a streaming look-ahead peak limiter: the last output stage, behind the codec's last kernel,
// the resampler or the stretcher (include/ptts.h, "output level"; contract and plan rule: pocket_tts_amd/level.py; index
// functions and their bounds: ptts_level.h).
//
// One launch per frame, one workgroup per row (a row's recurrence is serial across tiles, rows are independent).  A limiting
// row walks its frame in tiles of at most PTTS_LV_TILE samples, two neighbouring samples per thread:
//   stage    U = carried u || G x of the tile in LDS (zeros for the tile when the row drains: the input is then not read)
//   r        R = |U| > C ? C / |U| : 1 over the whole line
//   minimum  m[i] = min R[i .. i + LA]: exact, so the two samples of a thread share the entries both windows hold
//   scan     d[i] = max(1 - m[i], a d[i - 1]) as an associative scan over pairs (A, c), f(d) = max(c, A d): the thread's two
//            samples, an inclusive scan over the wave (shuffles), the 16 wave totals through LDS seeded with the d carried
//            from the tile before.  The order of the combines is fixed by the sample's index in the frame.
//   e        E = carried e || 1 - d of the tile, in the line R leaves
//   box      g[i] = k (E[i + 1] + .. + E[i + LA]), added in ascending order of the index
//   store    y[i] = g[i] U[i]
// After the last tile the same workgroup writes the row's carried u, carried e and d back: no other block reads them, so there
// is no second launch.  Bypass rows copy their line and exit.
//
// True-peak mode (level.py, "True-peak mode"; indices: ptts_level.h) is the TPK = true instance of the same kernel, which a
// leveler launches once ptts_leveler_enable_true_peak has run; TPK = false is the kernel of before, statement for statement.
// The mode is per row and uniform for the block.  A true-peak row differs in three places:
//   stage    the carried line is LA + H samples of u (H = 20, what the FIR reaches back)
//   r        R[q] comes from P = fmax(|u D back|, |v_1|, |v_2|, |v_3|): 3 x 21 taps out of LDS, consecutive lanes on
//            consecutive words (no bank conflict), the taps through scalar loads; terms in ascending j, one fma each
//   store    y[i] = g[i] U[i + H - D]; y also goes to a third line, carried y || tile, over which the same FIR runs for the
//            meter: a thread's maximum, a butterfly over the wave, 16 wave maxima through LDS into thread 0's M
// A sample-peak row of that instance runs H = 0 through the same statements as in the other one.
#include <cstring>

#include "ptts_stage.h"
#include "ptts_level.h"

struct ptts_leveler : StageBase {  // row_plan < 0: bypass
  LvPlan *plans = nullptr;   // [n_plans]
  float *row_gc = nullptr;   // [B][2]: G, C
  float *cu = nullptr;       // [B][PTTS_LV_MAX_LA]: the row's last LA samples of u at the front of its line
  float *ce = nullptr;       // [B][PTTS_LV_MAX_LA]: its last LA samples of e
  float *row_d = nullptr;    // [B]: its last d
  // true-peak mode: null until ptts_leveler_enable_true_peak
  float *taps = nullptr;     // [3][PTTS_LV_TP_T]: phases 1, 2, 3 of the 4x interpolator
  int *row_mode = nullptr;   // [B]: != 0: the row limits the true peak
  float *ctp = nullptr;      // [B][PTTS_LV_TP_CARRY]: a true-peak row's H samples of u before those in cu, then its last H of y
  float *row_tp = nullptr;   // [B]: its meter M
  std::vector<LvPlan> h_plans;  // the plans on the host: what set_row_tp checks a row's plan against
};

constexpr int kLvMaxPlans = 256;
constexpr int kLvThreads = 1024;
constexpr int kLvWaves = kLvThreads / 64;
static_assert(2 * kLvThreads >= PTTS_LV_TILE, "two samples of a tile per thread");
static_assert(PTTS_LV_MAX_LA <= kLvThreads, "one carried sample per thread");

__device__ inline float lv_i16(float v) { return fminf(fmaxf(v, -1.0f), 1.0f) * 32767.0f; }

struct LvTruePeak {  // what the TPK = true instance reads on top: the fields of ptts_leveler of the same names
  const float *taps;
  const int *row_mode;
  float *ctp, *row_tp;
};

template <bool TPK>
__global__ __launch_bounds__(kLvThreads) void level_kernel(const float *__restrict__ in, int width,
                                                           const LvPlan *__restrict__ plans, int n_plans,
                                                           const int *__restrict__ row_plan, const int *__restrict__ row_drain,
                                                           const float *__restrict__ row_gc, float *__restrict__ cu,
                                                           float *__restrict__ ce, float *__restrict__ row_d,
                                                           float *__restrict__ out_f, int16_t *__restrict__ out_i, LvTruePeak tpk) {
  __shared__ float U[TPK ? PTTS_LV_TP_ULINE : PTTS_LV_LINE];  // carried u || u of the tile
  __shared__ float E[PTTS_LV_LINE];  // r of the same samples, then carried e || e of the tile
  __shared__ float Y[TPK ? PTTS_LV_TP_YLINE : 1];  // a true-peak row's carried y || y of the tile
  __shared__ float wM[kLvWaves];
  __shared__ float wA[kLvWaves], wc[kLvWaves], wseed[kLvWaves];
  __shared__ float dlast;
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float *x = in + (size_t)row * width;  // n <= width (ptts_leveler_create)
  const size_t o0 = (size_t)row * width;
  const int pi = row_plan[row];
  if (pi < 0) {  // bypass (uniform: the whole block leaves): a row without a plan has no n, its whole line is copied
    for (int i = tid; i < width; i += kLvThreads) {
      const float v = x[i];
      if (out_i) out_i[o0 + i] = (int16_t)lv_i16(v);
      else out_f[o0 + i] = v;
    }
    return;
  }
  const LvPlan P = plans[min(pi, n_plans - 1)];
  const int n = P.n, LA = P.LA;  // 1 <= LA <= PTTS_LV_MAX_LA, LA <= n <= width (lv_plan_ok, ptts_leveler_create)
  const float a = P.a, k = P.k, G = row_gc[2 * row], C = row_gc[2 * row + 1];
  const bool drain = row_drain[row] != 0;
  float *curow = cu + (size_t)row * PTTS_LV_MAX_LA;
  float *cerow = ce + (size_t)row * PTTS_LV_MAX_LA;
  bool tp = false;  // uniform: the row's mode
  if constexpr (TPK) tp = tpk.row_mode[row] != 0;
  const int H = tp ? PTTS_LV_TP_H : 0, CU = LA + H;  // LA + 10 <= n for such a row (lv_tp_plan_ok, ptts_leveler_set_row_tp)
  float *xrow = nullptr;  // the row's PTTS_LV_TP_CARRY floats
  if constexpr (TPK) xrow = tpk.ctp + (size_t)row * PTTS_LV_TP_CARRY;
  float ucar = 0.f, ecar = 1.f;  // thread c < LA + H: entry c of the carried u line; c < LA: of the carried e line
  float ycar = 0.f, M = 0.f;     // thread c < H: entry c of the carried y line; thread 0: the meter
  if (tid < CU) { ucar = tid < H ? xrow[tid] : curow[tid - H]; U[tid] = ucar; }
  if (tid < LA) ecar = cerow[tid];
  if (tp) {
    if (tid < H) { ycar = xrow[PTTS_LV_TP_H + tid]; Y[tid] = ycar; }
    if (tid == 0) M = tpk.row_tp[row];
  }
  float dcar = row_d[row];
  const int tiles = lv_tiles(n);
  for (int j = 0; j < tiles; ++j) {
    const int T = lv_tile_len(j, n);
    for (int i = tid; i < T; i += kLvThreads) U[tp ? lv_tp_cur(i, LA) : lv_cur(i, LA)] = drain ? 0.f : G * x[lv_io(j, i)];
    __syncthreads();
    for (int i = tid; i < LA + T; i += kLvThreads) {
      float au;
      if (tp) {  // fmaxf drops a NaN operand: P is NaN only where the sample D back is
        float v1 = 0.f, v2 = 0.f, v3 = 0.f;
#pragma unroll
        for (int t = 0; t < PTTS_LV_TP_T; ++t) {
          const float s = U[lv_tp_tap(i, t)];
          v1 = fmaf(tpk.taps[t], s, v1);
          v2 = fmaf(tpk.taps[PTTS_LV_TP_T + t], s, v2);
          v3 = fmaf(tpk.taps[2 * PTTS_LV_TP_T + t], s, v3);
        }
        au = fmaxf(fmaxf(fabsf(U[lv_tp_centre(i)]), fabsf(v1)), fmaxf(fabsf(v2), fabsf(v3)));
      } else {
        au = fabsf(U[i]);
      }
      E[i] = au > C ? C / au : 1.0f;  // a NaN compares false
    }
    __syncthreads();
    const int i0 = 2 * tid, i1 = 2 * tid + 1;
    const bool on0 = i0 < T, on1 = i1 < T;
    float m0 = 1.f, m1 = 1.f;
    if (on0) {
      float common = 1.f;  // the entries both windows hold: [i0 + 1, i0 + LA]
      for (int q = lv_min_lo(i0) + 1; q <= lv_min_hi(i0, LA); ++q) common = fminf(common, E[q]);
      m0 = fminf(common, E[lv_min_lo(i0)]);
      if (on1) m1 = fminf(common, E[lv_min_hi(i1, LA)]);
    }
    __syncthreads();  // every read of r is done: the line takes e below
    // f_i(d) = max(c_i, A_i d); a sample past the tile's end is the identity (1, 0): d >= 0 throughout
    const float A0 = on0 ? a : 1.f, c0 = on0 ? 1.0f - m0 : 0.f;
    const float A1 = on1 ? a : 1.f, c1 = on1 ? 1.0f - m1 : 0.f;
    float A = A1 * A0, c = fmaxf(c1, A1 * c0);
    for (int off = 1; off < 64; off <<= 1) {
      const float Ao = __shfl_up(A, off, 64), co = __shfl_up(c, off, 64);
      if (lane >= off) { c = fmaxf(c, A * co); A = A * Ao; }
    }
    if (lane == 63) { wA[wave] = A; wc[wave] = c; }
    __syncthreads();
    if (tid == 0) {
      float d = dcar;
      for (int w = 0; w < kLvWaves; ++w) { wseed[w] = d; d = fmaxf(wc[w], wA[w] * d); }
    }
    __syncthreads();
    const float Ae = __shfl_up(A, 1, 64), cex = __shfl_up(c, 1, 64), seed = wseed[wave];
    const float dprev = lane == 0 ? seed : fmaxf(cex, Ae * seed);
    const float d0 = fmaxf(c0, A0 * dprev), d1 = fmaxf(c1, A1 * d0);
    if (on0 && i0 == T - 1) dlast = d0;
    if (on1 && i1 == T - 1) dlast = d1;
    if (tid < LA) E[tid] = ecar;
    if (on0) E[lv_cur(i0, LA)] = 1.0f - d0;
    if (on1) E[lv_cur(i1, LA)] = 1.0f - d1;
    __syncthreads();
    if (on0) {
      float s = 0.f;  // the entries both sums hold: [i0 + 2, i0 + LA], ascending
      for (int q = lv_box_lo(i0) + 1; q <= lv_box_hi(i0, LA); ++q) s += E[q];
      const float y0 = (k * (E[lv_box_lo(i0)] + s)) * U[tp ? lv_tp_delayed(i0) : lv_delayed(i0)];
      if (tp) Y[lv_tp_ycur(i0)] = y0;
      const size_t o = o0 + lv_io(j, i0);  // lv_io < n <= width
      if (out_i) out_i[o] = (int16_t)lv_i16(y0);
      else out_f[o] = y0;
      if (on1) {
        const float y1 = (k * (s + E[lv_box_hi(i1, LA)])) * U[tp ? lv_tp_delayed(i1) : lv_delayed(i1)];
        if (tp) Y[lv_tp_ycur(i1)] = y1;
        if (out_i) out_i[o + 1] = (int16_t)lv_i16(y1);
        else out_f[o + 1] = y1;
      }
    }
    if (tid < CU) ucar = U[tp ? lv_tp_carry_src(tid, T) : lv_carry_src(tid, T)];
    if (tid < LA) ecar = E[lv_carry_src(tid, T)];
    dcar = dlast;
    if (tp) {  // the meter: the same FIR over carried y || y of the tile
      __syncthreads();  // the tile's y is in its line
      float mx = 0.f;
      for (int i = tid; i < T; i += kLvThreads) {
        float w1 = 0.f, w2 = 0.f, w3 = 0.f;
#pragma unroll
        for (int t = 0; t < PTTS_LV_TP_T; ++t) {
          const float s = Y[lv_tp_ytap(i, t)];
          w1 = fmaf(tpk.taps[t], s, w1);
          w2 = fmaf(tpk.taps[PTTS_LV_TP_T + t], s, w2);
          w3 = fmaf(tpk.taps[2 * PTTS_LV_TP_T + t], s, w3);
        }
        mx = fmaxf(mx, fmaxf(fmaxf(fabsf(Y[lv_tp_ycentre(i)]), fabsf(w1)), fmaxf(fabsf(w2), fabsf(w3))));
      }
      for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
      if (lane == 0) wM[wave] = mx;
      if (tid < H) ycar = Y[lv_tp_ycarry_src(tid, T)];
    }
    __syncthreads();  // every read of the lines is done
    if (tid < CU) U[tid] = ucar;
    if (tp) {
      if (tid < H) Y[tid] = ycar;
      if (tid == 0)
        for (int w = 0; w < kLvWaves; ++w) M = fmaxf(M, wM[w]);  // wM is next written two barriers on
    }
  }
  if (tid < CU) {
    if (tid < H) xrow[tid] = ucar;
    else curow[tid - H] = ucar;
  }
  if (tid < LA) cerow[tid] = ecar;
  if (tid == 0) row_d[row] = dcar;
  if (tp) {
    if (tid < H) xrow[PTTS_LV_TP_H + tid] = ycar;
    if (tid == 0) tpk.row_tp[row] = M;
  }
}

__global__ __launch_bounds__(PTTS_LV_MAX_LA) void level_set_row_kernel(int *row_plan, int *row_drain, float *row_gc, float *cu,
                                                                       float *ce, float *row_d, int row, int plan_index,
                                                                       float G, float C, int *row_mode, float *ctp,
                                                                       float *row_tp, int mode) {
  const int tid = threadIdx.x;
  if (row_mode) {  // a leveler with true-peak mode: the row's mode, its extra carries and its meter
    if (tid == 0) { row_mode[row] = mode; row_tp[row] = 0.f; }
    if (tid < PTTS_LV_TP_CARRY) ctp[(size_t)row * PTTS_LV_TP_CARRY + tid] = 0.f;
  }
  if (tid == 0) {
    row_plan[row] = plan_index; row_drain[row] = 0; row_gc[2 * row] = G; row_gc[2 * row + 1] = C; row_d[row] = 0.f;
  }
  cu[(size_t)row * PTTS_LV_MAX_LA + tid] = 0.f;  // u = 0 and e = 1 before the stream's start
  ce[(size_t)row * PTTS_LV_MAX_LA + tid] = 1.f;
}

int level_enqueue(hipStream_t st, ptts_leveler *lv, const float *d_in, void *out, int is_i16) {
  if (!lv || !d_in || !out) return fail(-1, "level: null argument");
  const int B = lv->B;
  {
    ProfScope ps(st, "level", 4.0 * B * (lv->in_width + 4.0 * PTTS_LV_MAX_LA) + (is_i16 ? 2.0 : 4.0) * B * lv->in_width, 0);
    const LvTruePeak tpk{lv->taps, lv->row_mode, lv->ctp, lv->row_tp};
    auto kernel = lv->taps ? level_kernel<true> : level_kernel<false>;
    kernel<<<B, kLvThreads, 0, st>>>(d_in, lv->in_width, lv->plans, lv->n_plans, lv->row_plan, lv->row_drain, lv->row_gc, lv->cu,
                                     lv->ce, lv->row_d, is_i16 ? nullptr : (float *)out, is_i16 ? (int16_t *)out : nullptr, tpk);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int ptts_leveler_create(ptts_engine *e, int32_t batch, const int32_t *h_plans, int32_t n_plans, ptts_leveler **out) {
  if (!e || !out || !h_plans) return fail(-1, "leveler_create: null argument");
  if (batch < 1 || n_plans < 1 || n_plans > kLvMaxPlans) return fail(-1, "leveler_create: batch or number of plans out of range");
  std::vector<LvPlan> plans(n_plans);
  int width = 0;
  for (int i = 0; i < n_plans; ++i) {
    const int32_t *p = h_plans + 4 * i;
    LvPlan P;
    P.n = p[0]; P.LA = p[1];
    std::memcpy(&P.a, p + 2, sizeof(float));
    std::memcpy(&P.k, p + 3, sizeof(float));
    if (!lv_plan_ok(P.n, P.LA) || !(P.a >= 0.f && P.a < 1.f) || !(P.k > 0.f && P.k <= 1.f))
      return fail(-1, "leveler_create: plan " + std::to_string(i) + " (n " + std::to_string(P.n) + ", LA " +
                          std::to_string(P.LA) + ", a " + std::to_string(P.a) + ", k " + std::to_string(P.k) +
                          ") is not admissible");
    plans[i] = P;
    width = std::max(width, (int)P.n);
  }
  StageLock lock;
  ptts_leveler *lv;
  CHK(stage_new(e, batch, n_plans, width, width, lock, &lv));
  const size_t line = (size_t)batch * PTTS_LV_MAX_LA;
  lv->h_plans = plans;
  stage_copy(*lv, lv->plans, plans.data(), n_plans);
  stage_fill(*lv, lv->row_plan, batch, -1);
  stage_zeros(*lv, lv->row_drain, batch);
  stage_zeros(*lv, lv->row_gc, (size_t)batch * 2);
  stage_zeros(*lv, lv->cu, line);
  stage_fill(*lv, lv->ce, line, 1.0f);
  stage_zeros(*lv, lv->row_d, batch);
  return stage_finish(lv, out, "leveler_create");
}

extern "C" void ptts_leveler_destroy(ptts_leveler *lv) { stage_destroy(lv); }

extern "C" int ptts_leveler_enable_true_peak(ptts_leveler *lv, const float *taps63) {
  if (!lv || !taps63) return fail(-1, "leveler_enable_true_peak: null argument");
  if (lv->taps) return fail(-1, "leveler_enable_true_peak: the leveler has the mode already");
  for (int i = 0; i < PTTS_LV_TP_PHASES * PTTS_LV_TP_T; ++i)
    if (!(taps63[i] >= -4.f && taps63[i] <= 4.f)) return fail(-1, "leveler_enable_true_peak: a tap is not in [-4, 4]");
  StageLock lock;
  CHK(stage_enter(lv->e, lock));
  float *taps = nullptr;  // lv->taps is set last: it is what level_enqueue and set_row_tp take the mode from
  int *row_mode = nullptr;
  stage_zeros(*lv, row_mode, lv->B);
  stage_zeros(*lv, lv->ctp, (size_t)lv->B * PTTS_LV_TP_CARRY);
  stage_zeros(*lv, lv->row_tp, lv->B);
  stage_copy(*lv, taps, taps63, (size_t)PTTS_LV_TP_PHASES * PTTS_LV_TP_T);
  if (lv->er == hipSuccess) lv->er = hipDeviceSynchronize();
  if (lv->er != hipSuccess) {  // what was allocated stays owned and is freed with the leveler, which goes on without the mode
    const hipError_t er = lv->er;
    lv->er = hipSuccess;
    return fail(-2, std::string("leveler_enable_true_peak: ") + hipGetErrorString(er));
  }
  lv->row_mode = row_mode;
  lv->taps = taps;
  return 0;
}

static int level_set_row(ptts_leveler *lv, const char *fn, int row, int plan_index, float gain, float ceiling, int mode,
                         void *stream) {
  CHK(stage_row_ok(lv, fn, "leveler", row, "plan", plan_index, mode ? 0 : -1));
  if (plan_index >= 0 && !(gain > 0.f && gain <= 16.f && ceiling > 0.f && ceiling <= 1.f))
    return fail(-1, std::string(fn) + ": the gain must be in (0, 16] and the ceiling in (0, 1]");
  if (mode) {
    if (!lv->taps) return fail(-1, std::string(fn) + ": the leveler has no true-peak mode (ptts_leveler_enable_true_peak)");
    const LvPlan &P = lv->h_plans[plan_index];
    if (!lv_tp_plan_ok(P.n, P.LA))
      return fail(-1, std::string(fn) + ": plan " + std::to_string(plan_index) + " (n " + std::to_string(P.n) + ", LA " +
                          std::to_string(P.LA) + ") is not admissible in true-peak mode: LA + 10 exceeds n");
  }
  StageLock lock;
  CHK(stage_enter(lv->e, lock));
  level_set_row_kernel<<<1, PTTS_LV_MAX_LA, 0, S(lv->e, stream)>>>(lv->row_plan, lv->row_drain, lv->row_gc, lv->cu, lv->ce,
                                                                  lv->row_d, row, plan_index, plan_index < 0 ? 1.f : gain,
                                                                  plan_index < 0 ? 1.f : ceiling, lv->row_mode, lv->ctp,
                                                                  lv->row_tp, mode);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int ptts_leveler_set_row(ptts_leveler *lv, int32_t row, int32_t plan_index, float gain, float ceiling, void *stream) {
  return level_set_row(lv, "leveler_set_row", row, plan_index, gain, ceiling, 0, stream);
}

extern "C" int ptts_leveler_set_row_tp(ptts_leveler *lv, int32_t row, int32_t plan_index, float gain, float ceiling,
                                       void *stream) {
  return level_set_row(lv, "leveler_set_row_tp", row, plan_index, gain, ceiling, 1, stream);
}

extern "C" int ptts_leveler_row_true_peak(ptts_leveler *lv, int32_t row, float *host_out, void *stream) {
  CHK(stage_row_ok(lv, "leveler_row_true_peak", "leveler", row));
  if (!host_out) return fail(-1, "leveler_row_true_peak: null argument");
  if (!lv->taps) return fail(-1, "leveler_row_true_peak: the leveler has no true-peak mode (ptts_leveler_enable_true_peak)");
  StageLock lock;
  CHK(stage_enter(lv->e, lock));
  hipStream_t st = S(lv->e, stream);
  HIPCHK(hipMemcpyAsync(host_out, lv->row_tp + row, sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int ptts_leveler_set_row_drain(ptts_leveler *lv, int32_t row, int32_t on, void *stream) {
  return stage_set_row_drain(lv, "leveler_set_row_drain", "leveler", row, on, stream);
}

extern "C" int ptts_level_frame(ptts_leveler *lv, const float *d_in, void *out, int32_t is_i16, void *stream) {
  return stage_frame(lv, d_in && out, "level_frame", stream,
                     [&](hipStream_t st) { return level_enqueue(st, lv, d_in, out, is_i16 != 0); });
}
