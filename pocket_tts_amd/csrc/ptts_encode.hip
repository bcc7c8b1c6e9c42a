// Per-request output encoding: the last output stage, behind the codec's last kernel or whichever stage ended the chain
// before it (include/ptts.h, "output encoding"; contract: pocket_tts_amd/encoding.py; conversions, index functions and
// their bounds: ptts_encode.h).
//
// One launch per frame, no state, no LDS.  Row b holds n_b samples and a code; blockIdx.y is the row and every lane owns one
// run of PTTS_EN_RUN = 16 consecutive samples of it:
//   load     a full run as four 16-byte loads where the run's address allows it (a width that is no multiple of 4 shifts the
//            rows), else as 16 dword loads
//   convert  pcm_f32le: the bits as they are; else s = en_s16(x), then s, en_mulaw(s) or en_alaw(s), packed little-endian
//   store    whole 16-byte stores: four (pcm_f32le), two (pcm_s16le) or one (mulaw, alaw).  The output may be pinned host
//            memory, where a byte or short store costs many times the time per byte of a 16-byte one
// Only the run that holds the row's end (n_b no multiple of 16) stores sample by sample, and a run past it stores nothing:
// behind its n_b * bytes_per_sample bytes a row's line is not touched.
#include "ptts_stage.h"
#include "ptts_encode.h"

struct ptts_encoder : StageBase {  // no plans; in_width = out_width: the line's width in samples
  int *row_nc = nullptr;  // [B][2]: n, code
};

constexpr int kEnThreads = 128;

__device__ inline uint32_t en_pack2(int lo, int hi) { return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16); }
__device__ inline uint32_t en_pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return a | (b << 8) | (c << 16) | (d << 24); }
__device__ inline uint32_t en_g711(int code, float x) { return code == 2 ? en_mulaw(en_s16(x)) : en_alaw(en_s16(x)); }

__global__ __launch_bounds__(kEnThreads) void encode_kernel(const float *__restrict__ in, int width,
                                                            const int *__restrict__ row_nc, uint8_t *__restrict__ out,
                                                            long pitch) {
  const int row = blockIdx.y, r = blockIdx.x * kEnThreads + threadIdx.x;
  const int n = min(max(row_nc[2 * row], 0), width);  // 1 <= n <= width by ptts_encoder_set_row
  const int code = row_nc[2 * row + 1] & (PTTS_EN_CODES - 1);
  const int tail = en_tail(r, n);
  if (tail <= 0) return;  // a run past the row's end
  const int bps = en_bps(code);
  const float *x = in + (size_t)row * width + (size_t)PTTS_EN_RUN * r;      // samples [16 r, min(16 r + 16, n)) are read
  uint8_t *o = out + (size_t)row * pitch + (size_t)PTTS_EN_RUN * r * bps;  // 16-byte aligned: base, pitch and 16 r bps are
  if (!en_full(r, n)) {  // the run with the row's end: tail in [1, 15] samples, each stored on its own
    for (int i = 0; i < tail; ++i) {
      const float v = x[i];
      if (code == 1) ((uint32_t *)o)[i] = __float_as_uint(v);
      else if (code == 0) ((uint16_t *)o)[i] = (uint16_t)en_s16(v);
      else o[i] = (uint8_t)en_g711(code, v);
    }
    return;
  }
  float v[PTTS_EN_RUN];
  if (((uintptr_t)x & 15) == 0) {
#pragma unroll
    for (int q = 0; q < PTTS_EN_RUN / 4; ++q) {
      const float4 f = ((const float4 *)x)[q];
      v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < PTTS_EN_RUN; ++i) v[i] = x[i];
  }
  uint4 *o4 = (uint4 *)o;
  if (code == 1) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      o4[q] = make_uint4(__float_as_uint(v[4 * q]), __float_as_uint(v[4 * q + 1]), __float_as_uint(v[4 * q + 2]),
                         __float_as_uint(v[4 * q + 3]));
  } else if (code == 0) {
    uint32_t w[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) w[q] = en_pack2(en_s16(v[2 * q]), en_s16(v[2 * q + 1]));
    o4[0] = make_uint4(w[0], w[1], w[2], w[3]);
    o4[1] = make_uint4(w[4], w[5], w[6], w[7]);
  } else {
    uint32_t w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      w[q] = en_pack4(en_g711(code, v[4 * q]), en_g711(code, v[4 * q + 1]), en_g711(code, v[4 * q + 2]), en_g711(code, v[4 * q + 3]));
    o4[0] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

__global__ void encode_set_row_kernel(int *row_nc, int row, int n, int code) {
  row_nc[2 * row] = n;
  row_nc[2 * row + 1] = code;
}

int encode_enqueue(hipStream_t st, ptts_encoder *en, const float *d_in, void *out_bytes) {
  if (!en || !d_in || !out_bytes) return fail(-1, "encode: null argument");
  if ((uintptr_t)out_bytes & 15) return fail(-1, "encode: the output is not aligned to 16 bytes");
  if ((uintptr_t)d_in & 3) return fail(-1, "encode: the input is not aligned to 4 bytes");
  const int B = en->B;
  {
    ProfScope ps(st, "encode", 8.0 * B * en->in_width + 8.0 * B, 0);
    encode_kernel<<<dim3(cdiv(en_runs(en->in_width), kEnThreads), B), kEnThreads, 0, st>>>(d_in, en->in_width, en->row_nc,
                                                                                        (uint8_t *)out_bytes, en_pitch(en->in_width));
  }
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int ptts_encoder_create(ptts_engine *e, int32_t batch, int32_t width, ptts_encoder **out) {
  if (!e || !out) return fail(-1, "encoder_create: null argument");
  if (batch < 1 || batch > 65535 || width < 1 || width > (1 << 20)) return fail(-1, "encoder_create: batch or width out of range");
  StageLock lock;
  ptts_encoder *en;
  CHK(stage_new(e, batch, 0, width, width, lock, &en));
  std::vector<int> rows(2 * (size_t)batch);
  for (int b = 0; b < batch; ++b) { rows[2 * b] = width; rows[2 * b + 1] = 0; }  // (width, pcm_s16le)
  stage_copy(*en, en->row_nc, rows.data(), rows.size());
  return stage_finish(en, out, "encoder_create");
}

extern "C" void ptts_encoder_destroy(ptts_encoder *en) { stage_destroy(en); }

extern "C" int ptts_encoder_set_row(ptts_encoder *en, int32_t row, int32_t n, int32_t code, void *stream) {
  CHK(stage_row_ok(en, "encoder_set_row", "encoder", row));
  if (n < 1 || n > en->in_width)
    return fail(-1, "encoder_set_row: n " + std::to_string(n) + " is not in [1, " + std::to_string(en->in_width) + "]");
  if (code < 0 || code >= PTTS_EN_CODES) return fail(-1, "encoder_set_row: code " + std::to_string(code) + " is not in [0, 3]");
  StageLock lock;
  CHK(stage_enter(en->e, lock));
  encode_set_row_kernel<<<1, 1, 0, S(en->e, stream)>>>(en->row_nc, row, n, code);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int ptts_encode_frame(ptts_encoder *en, const float *d_in, void *out_bytes, void *stream) {
  return stage_frame(en, d_in && out_bytes, "encode_frame", stream,
                     [&](hipStream_t st) { return encode_enqueue(st, en, d_in, out_bytes); });
}
