// Per-request output sample rates: a streaming polyphase resampler behind the codec's last kernel (include/ptts.h,
// "output sample rates"; filter design and admission rules: pocket_tts_amd/resample.py; index function: ptts_resample.h).
//
// Two launches per frame on one stream:
//   resample_kernel        grid (ceil(out_max / 256), B): every block stages the part of w = history || frame of its row
//                          that its outputs read in LDS and each thread computes at most one output n < out_n of the
//                          row's rate
//   resample_carry_kernel  hist[row] <- the frame's last PTTS_RS_HIST samples
// The history is never written by the launch that reads it: the blocks of one row run concurrently.
#include "ptts_stage.h"
#include "ptts_resample.h"

struct ptts_resampler : StageBase {  // a plan is a rate; in_width: the codec's frame_samples, out_width: out_max
  float *tables = nullptr;  // the rates' [up][T] tables, one after the other
  RsRate *rates = nullptr;  // [n_plans]
  float *hist = nullptr;    // [B][PTTS_RS_HIST]
};

constexpr int kRsMaxRates = 64;
constexpr int kRsMaxFrame = 8128;  // (PTTS_RS_HIST + fs) floats of LDS per block stay under 32 KB

__global__ __launch_bounds__(256) void resample_kernel(const float *__restrict__ pcm, const float *__restrict__ hist,
                                                       const float *__restrict__ tables, const RsRate *__restrict__ rates,
                                                       const int *__restrict__ row_rate, int n_rates, int fs, int out_max,
                                                       float *__restrict__ out_f, int16_t *__restrict__ out_i) {
  extern __shared__ float w[];  // PTTS_RS_HIST + fs
  const int row = blockIdx.y;
  const int r = min(max(row_rate[row], 0), n_rates - 1);
  const RsRate R = rates[r];
  const int n0 = blockIdx.x * 256;
  if (n0 >= R.out_n) return;  // the whole block lies past the row's outputs (uniform: nobody waits at the barrier below)
  // only the part [lo, hi] of w that this block's outputs read is staged, every entry at its own index of w (rs_window:
  // 0 <= lo <= hi <= PTTS_RS_HIST + fs - 1); the native rate has T = 1 and i0(n) = n
  int lo, hi;
  rs_window(n0, min(n0 + 255, R.out_n - 1), R.up, R.down, R.T, &lo, &hi);
  for (int i = lo + threadIdx.x; i <= hi; i += 256)
    w[i] = i < PTTS_RS_HIST ? hist[(size_t)row * PTTS_RS_HIST + i] : pcm[(size_t)row * fs + (i - PTTS_RS_HIST)];
  __syncthreads();
  const int n = n0 + threadIdx.x;
  if (n >= R.out_n) return;  // out_n <= out_max (ptts_resampler_create): o below stays inside the row
  // the native rate is a copy, not a filter (out_n == fs: n < fs)
  const float v = (R.up == 1 && R.down == 1) ? w[PTTS_RS_HIST + n] : rs_output(tables + R.off, w, n, R.up, R.down, R.T);
  const size_t o = (size_t)row * out_max + n;
  if (out_i) out_i[o] = (int16_t)(fminf(fmaxf(v, -1.0f), 1.0f) * 32767.0f);
  else out_f[o] = v;
}

__global__ __launch_bounds__(PTTS_RS_HIST) void resample_carry_kernel(const float *__restrict__ pcm, float *__restrict__ hist,
                                                                      int fs) {
  const int row = blockIdx.x, t = threadIdx.x;  // fs >= PTTS_RS_HIST (ptts_resampler_create)
  hist[(size_t)row * PTTS_RS_HIST + t] = pcm[(size_t)row * fs + (fs - PTTS_RS_HIST) + t];
}

__global__ __launch_bounds__(PTTS_RS_HIST) void resample_set_row_kernel(int *row_rate, float *hist, int row, int rate_index) {
  if (threadIdx.x == 0) row_rate[row] = rate_index;
  hist[(size_t)row * PTTS_RS_HIST + threadIdx.x] = 0.f;
}

int resample_enqueue(hipStream_t st, ptts_resampler *rs, const float *d_pcm, void *out, int is_i16) {
  if (!rs || !d_pcm || !out) return fail(-1, "resample: null argument");
  const int B = rs->B, fs = rs->in_width, out_max = rs->out_width;
  {
    ProfScope ps(st, "resample", 4.0 * B * (fs + PTTS_RS_HIST) + (is_i16 ? 2.0 : 4.0) * B * out_max, 0);
    resample_kernel<<<dim3(cdiv(out_max, 256), B), 256, (size_t)(PTTS_RS_HIST + fs) * sizeof(float), st>>>(
        d_pcm, rs->hist, rs->tables, rs->rates, rs->row_plan, rs->n_plans, fs, out_max, is_i16 ? nullptr : (float *)out,
        is_i16 ? (int16_t *)out : nullptr);
  }
  {
    ProfScope ps(st, "resample_carry", 8.0 * B * PTTS_RS_HIST, 0);
    resample_carry_kernel<<<B, PTTS_RS_HIST, 0, st>>>(d_pcm, rs->hist, fs);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int ptts_resampler_create(ptts_engine *e, int32_t batch, const int32_t *h_up, const int32_t *h_down,
                                     const int32_t *h_taps, int32_t n_rates, const float *h_tables, int64_t n_table_floats,
                                     ptts_resampler **out) {
  if (!e || !out || !h_up || !h_down || !h_taps || !h_tables) return fail(-1, "resampler_create: null argument");
  if (batch < 1 || n_rates < 1 || n_rates > kRsMaxRates) return fail(-1, "resampler_create: batch or number of rates out of range");
  const ptts_config &c = e->cfg;
  const int fs = 16 * c.ratios[0] * c.ratios[1] * c.ratios[2];  // samples per codec frame (ptts_mimi_state::rows[3])
  if (fs < PTTS_RS_HIST || fs > kRsMaxFrame) return fail(-1, "resampler_create: unsupported frame length");
  std::vector<RsRate> rates(n_rates);
  int64_t off = 0;
  int out_max = 0;
  for (int i = 0; i < n_rates; ++i) {
    if (!rs_rate_ok(h_up[i], h_down[i], h_taps[i], fs, 4 * fs))
      return fail(-1, "resampler_create: rate " + std::to_string(i) + " (up " + std::to_string(h_up[i]) + ", down " +
                          std::to_string(h_down[i]) + ", taps " + std::to_string(h_taps[i]) + ") is not admissible for frames of " +
                          std::to_string(fs) + " samples");
    rates[i] = RsRate{h_up[i], h_down[i], h_taps[i], (int32_t)((int64_t)fs * h_up[i] / h_down[i]), (int32_t)off};
    off += (int64_t)h_up[i] * h_taps[i];
    out_max = std::max(out_max, (int)rates[i].out_n);
  }
  if (off != n_table_floats) return fail(-1, "resampler_create: the tables do not hold sum(up * taps) floats");
  StageLock lock;
  ptts_resampler *rs;
  CHK(stage_new(e, batch, n_rates, fs, out_max, lock, &rs));
  stage_copy(*rs, rs->tables, h_tables, (size_t)off);
  stage_copy(*rs, rs->rates, rates.data(), n_rates);
  stage_zeros(*rs, rs->row_plan, batch);
  stage_zeros(*rs, rs->hist, (size_t)batch * PTTS_RS_HIST);
  return stage_finish(rs, out, "resampler_create");
}

extern "C" void ptts_resampler_destroy(ptts_resampler *rs) { stage_destroy(rs); }

extern "C" int ptts_resampler_set_row(ptts_resampler *rs, int32_t row, int32_t rate_index, void *stream) {
  CHK(stage_row_ok(rs, "resampler_set_row", "resampler", row, "rate", rate_index, 0));
  StageLock lock;
  CHK(stage_enter(rs->e, lock));
  resample_set_row_kernel<<<1, PTTS_RS_HIST, 0, S(rs->e, stream)>>>(rs->row_plan, rs->hist, row, rate_index);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int ptts_resample_frame(ptts_resampler *rs, const float *d_pcm_in, void *out, int32_t is_i16, void *stream) {
  return stage_frame(rs, d_pcm_in && out, "resample_frame", stream,
                     [&](hipStream_t st) { return resample_enqueue(st, rs, d_pcm_in, out, is_i16 != 0); });
}
