// Per-request FLAC output: the packer, the eighth output stage, behind the encoder (include/ptts.h, "output compression";
// contract: pocket_tts_amd/flac.py; bitstream, choice rule, CRCs and bit positions: ptts_flac.h).
//
// One launch per frame.  blockIdx.y is the row and each row gets one workgroup of PTTS_FL_LANES = 256 lanes.  The input is
// the encoder's byte buffer, en_pitch(width) bytes a row on the device; the output is a ring line of fl_pitch(width) bytes
// that begins with the prefix {u32 nbytes, 0, 0, 0}.  Every store to the line is a 16-byte store: it may be pinned host memory.
//
//   pass-through row  the encoder's n * bps bytes behind the prefix, in whole 16-byte words
//   flac row          line f of the row (its counter) emits nothing while f < lead, then block j = f - lead as frame
//                     first_block + j: the previous line's samples [off, n) and the current line's [0, off), so that a row
//                     with pre-roll p = (lead - 1) n + off (off > 0) or lead n (off = 0) delivers the samples from p on in
//                     whole frames.  The current line then replaces the carry.
//
// A block is encoded in LDS: the samples as int32, the 75 sums of u >> k per lane over its own consecutive residuals, wave and
// block reduction, the choice by one lane, a zeroed bit buffer, an exclusive block scan of the lanes' code lengths, the codes
// ORed in with LDS atomics (two lanes can share a word), the header by one lane, the CRC-16 as the XOR of each lane's table
// CRC of its byte range times x^(8 * bytes behind it), and the stores.  Static LDS: 18.0 KB of samples, 9.1 KB of bit
// buffer and 3 KB of tables and partial sums, whatever the row's n.
#include "ptts_stage.h"
#include "ptts_encode.h"
#include "ptts_flac.h"

struct ptts_flac : StageBase {  // no plans; in_width = out_width: the line's width in samples
  int *rows = nullptr;       // [B][kFlRow]
  int16_t *carry = nullptr;  // [B][width]: the previous line of a flac row
};

enum { FL_MODE, FL_N, FL_BPS, FL_OFF, FL_LEAD, FL_FIRST, FL_COUNT, FL_RATE, kFlRow };

constexpr int kFlThreads = PTTS_FL_LANES;
constexpr int kFlWaves = kFlThreads / 64;
constexpr int kFlWords = ((2 * PTTS_FL_MAX_N + 18 + 15) / 16 * 16) / 4;  // the largest frame, rounded up to a 16-byte store

__device__ inline uint32_t fl_bswap(uint32_t v) { return __builtin_bswap32(v); }

// ORs the L low bits of v into the bit buffer at stream position p
__device__ inline void fl_put(uint32_t *buf, uint32_t p, uint32_t v, int L) {
  uint32_t w, m0, m1;
  fl_split(p, v, L, &w, &m0, &m1);
  if (m0 && w < (uint32_t)kFlWords) atomicOr(&buf[w], m0);
  if (m1 && w + 1 < (uint32_t)kFlWords) atomicOr(&buf[w + 1], m1);
}

__global__ __launch_bounds__(kFlThreads) void flac_kernel(const uint8_t *__restrict__ in, long in_pitch, int width,
                                                          int *__restrict__ rows, int16_t *__restrict__ carry,
                                                          uint8_t *__restrict__ out, long pitch) {
  __shared__ int32_t x[PTTS_FL_MAX_N];
  __shared__ uint32_t buf[kFlWords];
  __shared__ uint16_t t16[256];
  __shared__ uint8_t t8[256];
  __shared__ uint32_t wsum[kFlWaves][PTTS_FL_SUMS];
  __shared__ uint64_t sums[PTTS_FL_SUMS];
  __shared__ uint32_t wscan[kFlWaves];
  __shared__ int choice[4];  // type, o, k, header length
  __shared__ uint32_t wcrc[kFlWaves];

  const int row = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int *rd = rows + (size_t)row * kFlRow;
  const int mode = rd[FL_MODE];
  uint4 *line = (uint4 *)(out + (size_t)row * pitch);
  const uint8_t *src = in + (size_t)row * in_pitch;

  if (mode == 0) {  // pass-through: n * bps <= 4 width <= in_pitch, and 16 + in_pitch <= pitch
    const int n = min(max(rd[FL_N], 0), width), bps = min(max(rd[FL_BPS], 1), 4);
    const int nbytes = n * bps, nq = (nbytes + 15) / 16;
    if (t == 0) line[0] = make_uint4((uint32_t)nbytes, 0u, 0u, 0u);
    for (int q = t; q < nq; q += kFlThreads) line[1 + q] = ((const uint4 *)src)[q];
    return;
  }

  const int n = rd[FL_N], off = rd[FL_OFF], lead = rd[FL_LEAD], f = rd[FL_COUNT], rate = rd[FL_RATE];
  const uint32_t number = (uint32_t)rd[FL_FIRST] + (uint32_t)(f - lead);
  // ptts_flac_set_row admits only such rows; a row that is not one emits nothing
  const bool sane = n >= PTTS_FL_MIN_N && n <= PTTS_FL_MAX_N && n <= width && off >= 0 && off < n && lead >= 0 && f >= 0;
  const int16_t *cur = (const int16_t *)src;
  int16_t *prev = carry + (size_t)row * width;
  const bool emit = sane && f >= lead;
  if (emit)
    for (int i = t; i < n; i += kFlThreads) x[i] = fl_cut(prev, cur, n, off, i);
  t8[t] = fl_crc8_entry(t);
  t16[t] = fl_crc16_entry(t);
  for (int w = t; w < kFlWords; w += kFlThreads) buf[w] = 0u;
  __syncthreads();  // x is complete before the carry changes
  if (sane)
    for (int i = t; i < n; i += kFlThreads) prev[i] = cur[i];
  if (t == 0 && f < 0x7FFFFFFF) rd[FL_COUNT] = f + 1;
  if (!emit) {
    if (t == 0) line[0] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }

  // all equal?
  int differs = 0;
  for (int i = t; i < n; i += kFlThreads) differs |= x[i] != x[0];
  const bool constant = !__syncthreads_or(differs);

  int type = PTTS_FL_CONSTANT, o = 0, k = 0;
  if (!constant) {
    // the 75 sums of u >> k: each lane over the samples t, t + 256, .. (at most 18), then the wave, then the block
    uint32_t acc[PTTS_FL_ORDERS][PTTS_FL_KS];
#pragma unroll
    for (int oo = 0; oo < PTTS_FL_ORDERS; ++oo)
#pragma unroll
      for (int kk = 0; kk < PTTS_FL_KS; ++kk) acc[oo][kk] = 0u;
    for (int i = t; i < n; i += kFlThreads) {
#pragma unroll
      for (int oo = 0; oo < PTTS_FL_ORDERS; ++oo) {
        if (i < oo) continue;
        const uint32_t u = fl_fold(fl_resid(x, i, oo));
#pragma unroll
        for (int kk = 0; kk < PTTS_FL_KS; ++kk) acc[oo][kk] += u >> kk;
      }
    }
#pragma unroll
    for (int oo = 0; oo < PTTS_FL_ORDERS; ++oo)
#pragma unroll
      for (int kk = 0; kk < PTTS_FL_KS; ++kk) {
        uint32_t v = acc[oo][kk];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
        if (lane == 0) wsum[wave][oo * PTTS_FL_KS + kk] = v;
      }
    __syncthreads();
    if (t < PTTS_FL_SUMS) {
      uint64_t s = 0;
      for (int w = 0; w < kFlWaves; ++w) s += wsum[w][t];
      sums[t] = s;
    }
    __syncthreads();
    if (t == 0) {
      int oo, kk;
      choice[0] = fl_choose(sums, n, &oo, &kk);
      choice[1] = oo;
      choice[2] = kk;
    }
  } else if (t == 0) {
    choice[0] = PTTS_FL_CONSTANT; choice[1] = 0; choice[2] = 0;
  }
  // the header and the subframe's first byte, by one lane; no other lane writes below bit 8 * hlen + 8
  if (t == 0) {
    uint8_t h[PTTS_FL_HEADER_MAX];
    const int hlen = fl_header(h, number, n, rate, t8);
    for (int i = 0; i < hlen; ++i) fl_put(buf, 8u * i, h[i], 8);
    choice[3] = hlen;
  }
  __syncthreads();
  type = choice[0]; o = choice[1]; k = choice[2];
  const int hlen = choice[3];
  const uint32_t sub = 8u * (uint32_t)hlen;  // the subframe's first bit
  uint32_t total_bits;
  if (type == PTTS_FL_CONSTANT) {
    if (t == 0) fl_put(buf, sub + 8u, (uint32_t)x[0] & 0xFFFFu, 16);  // the subframe byte 00 is there already
    total_bits = sub + 24u;
  } else if (type == PTTS_FL_VERBATIM) {
    if (t == 0) fl_put(buf, sub, 0x02u, 8);
    for (int i = t; i < n; i += kFlThreads) fl_put(buf, sub + 8u + 16u * (uint32_t)i, (uint32_t)x[i] & 0xFFFFu, 16);
    total_bits = sub + 8u + 16u * (uint32_t)n;
  } else {
    if (t == 0) {
      fl_put(buf, sub, 0x10u | ((uint32_t)o << 1), 8);
      fl_put(buf, sub + 8u + 16u * (uint32_t)o, (uint32_t)k, 10);  // 00 0000 kkkk
    }
    if (t < o) fl_put(buf, sub + 8u + 16u * (uint32_t)t, (uint32_t)x[t] & 0xFFFFu, 16);
    // each lane's consecutive residuals, the exclusive scan of their lengths, then the codes
    int lo, hi;
    fl_range(t, n - o, &lo, &hi);
    uint32_t mine = 0;
    for (int r = lo; r < hi; ++r) mine += (fl_fold(fl_resid(x, o + r, o)) >> k) + 1u + (uint32_t)k;
    uint32_t incl = mine;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const uint32_t up = __shfl_up(incl, s);
      if (lane >= s) incl += up;
    }
    if (lane == 63) wscan[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int w = 0; w < kFlWaves; ++w) {
      if (w < wave) before += wscan[w];
      all += wscan[w];
    }
    uint32_t p = fl_codes_at(hlen, o) + before + incl - mine;
    for (int r = lo; r < hi; ++r) {
      uint32_t zeros, v;
      int L;
      fl_code(fl_fold(fl_resid(x, o + r, o)), k, &zeros, &v, &L);
      fl_put(buf, p + zeros, v, L);
      p += zeros + (uint32_t)L;
    }
    total_bits = fl_codes_at(hlen, o) + all;  // < 8 hlen + 8 + 16 n: FIXED is chosen only below VERBATIM's size
  }
  const uint32_t body = (total_bits + 7u) / 8u;  // bytes before the CRC-16
  __syncthreads();
  // CRC-16: each lane's byte range, shifted behind the ranges after it
  {
    int lo, hi;
    fl_range(t, (int)body, &lo, &hi);
    uint16_t c = 0;
    for (int j = lo; j < hi; ++j) c = fl_crc16(t16, c, fl_byte(buf, (uint32_t)j));
    uint32_t v = hi > lo ? fl_gfmul16(c, fl_xpow8(body - (uint32_t)hi)) : 0u;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v ^= __shfl_xor(v, s);
    if (lane == 0) wcrc[wave] = v;
  }
  __syncthreads();
  if (t == 0) {
    uint32_t c = 0;
    for (int w = 0; w < kFlWaves; ++w) c ^= wcrc[w];
    fl_put(buf, 8u * body, c & 0xFFFFu, 16);
  }
  __syncthreads();
  const uint32_t nbytes = body + 2u, nq = (nbytes + 15u) / 16u;  // nbytes <= fl_frame_max(n) <= 4 kFlWords
  if (t == 0) line[0] = make_uint4(nbytes, 0u, 0u, 0u);
  for (uint32_t q = t; q < nq; q += kFlThreads)
    line[1 + q] = make_uint4(fl_bswap(buf[4 * q]), fl_bswap(buf[4 * q + 1]), fl_bswap(buf[4 * q + 2]), fl_bswap(buf[4 * q + 3]));
}

__global__ void flac_set_row_kernel(int *rows, int row, int mode, int n, int bps, int off, int lead, int first, int rate) {
  int *rd = rows + (size_t)row * kFlRow;
  rd[FL_MODE] = mode; rd[FL_N] = n; rd[FL_BPS] = bps; rd[FL_OFF] = off; rd[FL_LEAD] = lead; rd[FL_FIRST] = first;
  rd[FL_COUNT] = 0; rd[FL_RATE] = rate;
}

int flac_enqueue(hipStream_t st, ptts_flac *pk, const void *d_in_bytes, void *out_bytes) {
  if (!pk || !d_in_bytes || !out_bytes) return fail(-1, "flac: null argument");
  if (((uintptr_t)out_bytes | (uintptr_t)d_in_bytes) & 15) return fail(-1, "flac: the input or the output is not aligned to 16 bytes");
  {
    ProfScope ps(st, "flac", 6.0 * pk->B * pk->in_width, 0);
    flac_kernel<<<dim3(1, pk->B), kFlThreads, 0, st>>>((const uint8_t *)d_in_bytes, en_pitch(pk->in_width), pk->in_width, pk->rows,
                                                       pk->carry, (uint8_t *)out_bytes, fl_pitch(pk->in_width));
  }
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int ptts_flac_create(ptts_engine *e, int32_t batch, int32_t width, ptts_flac **out) {
  if (!e || !out) return fail(-1, "flac_create: null argument");
  if (batch < 1 || batch > 65535 || width < 1 || width > (1 << 20)) return fail(-1, "flac_create: batch or width out of range");
  StageLock lock;
  ptts_flac *pk;
  CHK(stage_new(e, batch, 0, width, width, lock, &pk));
  std::vector<int> rows(kFlRow * (size_t)batch, 0);
  for (int b = 0; b < batch; ++b) { rows[kFlRow * b + FL_N] = width; rows[kFlRow * b + FL_BPS] = 2; }  // pass-through, pcm_s16le
  stage_copy(*pk, pk->rows, rows.data(), rows.size());
  stage_zeros(*pk, pk->carry, (size_t)batch * width);
  return stage_finish(pk, out, "flac_create");
}

extern "C" void ptts_flac_destroy(ptts_flac *pk) { stage_destroy(pk); }

extern "C" int ptts_flac_set_row(ptts_flac *pk, int32_t row, int32_t mode, int32_t n, int32_t bps, int32_t rate, int32_t preroll,
                                 int32_t first_block, void *stream) {
  CHK(stage_row_ok(pk, "flac_set_row", "packer", row));
  if (mode != 0 && mode != 1) return fail(-1, "flac_set_row: mode " + std::to_string(mode) + " is not 0 (pass-through) or 1 (flac)");
  int off = 0, lead = 0;
  if (mode == 0) {
    if (n < 1 || n > pk->in_width)
      return fail(-1, "flac_set_row: n " + std::to_string(n) + " is not in [1, " + std::to_string(pk->in_width) + "]");
    if (bps != 1 && bps != 2 && bps != 4) return fail(-1, "flac_set_row: bytes per sample " + std::to_string(bps) + " is not 1, 2 or 4");
    rate = preroll = first_block = 0;
  } else {
    const int hi = pk->in_width < PTTS_FL_MAX_N ? pk->in_width : PTTS_FL_MAX_N;
    if (n < PTTS_FL_MIN_N || n > hi)
      return fail(-1, "flac_set_row: n " + std::to_string(n) + " is not in [" + std::to_string(PTTS_FL_MIN_N) + ", " +
                          std::to_string(hi) + "]");
    if (rate < 1 || rate > 65535) return fail(-1, "flac_set_row: rate " + std::to_string(rate) + " is not in [1, 65535]");
    if (preroll < 0) return fail(-1, "flac_set_row: negative pre-roll");
    if (first_block < 0 || first_block > 0x3FFFFFFF) return fail(-1, "flac_set_row: first block out of range");
    bps = 2;
    off = preroll % n;
    lead = (preroll + n - 1) / n;
  }
  StageLock lock;
  CHK(stage_enter(pk->e, lock));
  flac_set_row_kernel<<<1, 1, 0, S(pk->e, stream)>>>(pk->rows, row, mode, n, bps, off, lead, first_block, rate);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int ptts_flac_frame(ptts_flac *pk, const void *d_in_bytes, void *out_bytes, void *stream) {
  return stage_frame(pk, d_in_bytes && out_bytes, "flac_frame", stream,
                     [&](hipStream_t st) { return flac_enqueue(st, pk, d_in_bytes, out_bytes); });
}
