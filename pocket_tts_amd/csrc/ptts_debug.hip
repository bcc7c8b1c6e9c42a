// Test hooks of the C ABI (include/ptts.h: ptts_debug_read, ptts_debug_gemm, ptts_debug_attn, ptts_debug_codec_gemm) in a unit
// of their own: the layout kernels between plain row-major buffers and the kernels' operand layouts, poison / guard
// buffers and case validation.  Production code is reached through ptts_host.h only, so this unit instantiates none of the
// GEMM / attention templates and compiles in seconds.
#include "ptts_bf16.h"
#include "ptts_host.h"

#include <algorithm>
#include <cstring>

// ------------------------------------------------------------------------------------------------
// The frame every ptts_debug_* case shares

static constexpr unsigned kDbgUnwritten = 0x7fc00000u;  // quiet NaN: an output tile the kernel never wrote
static constexpr unsigned kDbgGuard = 0x7fa5a5a5u;      // the guard regions around the outputs
static constexpr long kDbgGuardFloats = 16384;          // 64 KB behind each GEMM / codec output
static constexpr long kAttnGuard = 16 * 64;             // one key tile on both sides of each attention buffer

static __global__ void dbg_guard_kernel(const unsigned *p, long n, unsigned pattern, int *bad) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && p[i] != pattern) atomicOr(bad, 1);
}
__device__ __forceinline__ float dbg_e4m3(uint8_t b) { return __builtin_amdgcn_cvt_f32_fp8((int)b, 0); }
// FMH (fmt 0: bf16, KB 32-column blocks per row tile) / FM8 (fmt 1: e4m3, decoded, unscaled) -> [M][N] f32
static __global__ void dbg_from_codec_kernel(const void *src, float *dst, int M, int N, int KB, int fmt) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)M * N) return;
  const int m = i / N, n = i - (long)m * N;
  const size_t o = fmh_off(m, n & ~3, KB) + (n & 3);
  dst[i] = fmt == 0 ? (float)((const __bf16 *)src)[o] : dbg_e4m3(((const uint8_t *)src)[o]);
}

static __global__ void dbg_unpack_codec_weight_kernel(const void *img, const float *scale, int fmt, float *dst, int N, int KBt);
static __global__ void dbg_unpack_weight_kernel(const void *img, const float *scale, int fmt, float *dst, int N, int KF);
// ptts_debug_read on a Mimi state: the element type of a tap, and the two buffers that are fp32 in every codec format
enum { TAP_F32, TAP_BF16, TAP_E4M3 };
// the query blocks [B * H][QB][4][64 lanes][4] -> [B * Tq][H * 64] (Tq = 16 QB)
static __global__ void dbg_from_q_kernel(const float *Q, float *dst, int M, int H, int Tq, int QB) {
  const int D = H * 64;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)M * D) return;
  const int m = i / D, n = i - (long)m * D, h = n >> 6, d = n & 63;
  const int b = m / Tq, t = m - b * Tq;
  const size_t bh = (size_t)b * H + h;
  dst[i] = Q[(((bh * QB + (t >> 4)) * 4 + (d >> 4)) * 64 + 16 * ((d & 15) >> 2) + (t & 15)) * 4 + (d & 3)];
}
// one plane [B][H][cap][64] of the key / value ring -> [B * cap][H * 64], row b * cap + slot
static __global__ void dbg_from_kv_kernel(const float *Kc, float *dst, int B, int H, int cap) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * cap * H * 64) return;
  const int d = i & 63, h = (i >> 6) % H;
  const long r = (i >> 6) / H;
  const int slot = r % cap, b = r / cap;
  dst[i] = Kc[(((size_t)b * H + h) * cap + slot) * 64 + d];
}

// Runs one case on the engine's stream (or `stream`) under the engine lock, with a scratch engine that owns whatever the
// case packs and allocates: freed here whatever the outcome
template <typename Fn>
static int run_case(ptts_engine *e, void *stream, Fn fn) {
  ENGINE_LOCK(e);
  HIPCHK(hipSetDevice(e->device));
  bind_engine(e);
  hipStream_t st = S(e, stream);
  AllocScope as(st);
  ptts_engine scr;
  scr.stream = st;
  scr.device = e->device;
  const int rc = fn(st, scr);
  (void)hipStreamSynchronize(st);
  for (void *p : scr.allocs) (void)hipFree(p);
  return rc;
}
static void put_label(const std::string &label, char *dst, int cap) {
  if (!dst || cap <= 0) return;
  const size_t n = std::min<size_t>(label.size(), (size_t)cap - 1);
  memcpy(dst, label.data(), n);
  dst[n] = 0;
}
// Every guard (n words of kDbgGuard each) must still hold its pattern: synchronises, -6 with `what` when one does not
static int check_guards(ptts_engine &scr, hipStream_t st, const std::vector<const void *> &guards, long n, const std::string &what) {
  int *bad = nullptr;  // zero-filled by dalloc
  CHK(dallocT(&scr, &bad, 1));
  for (const void *g : guards) dbg_guard_kernel<<<cdiv(n, 256), 256, 0, st>>>((const unsigned *)g, n, kDbgGuard, bad);
  LAUNCHCHK();
  int h_bad = 0;
  HIPCHK(hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (h_bad) return fail(-6, what);
  return 0;
}

extern "C" int64_t ptts_debug_read(ptts_engine *e, void *state, int32_t is_mimi, const char *name, float *d_out,
                                   int64_t capacity, int32_t *rows, int32_t *cols, void *stream) {
  hipStream_t st = S(e, stream);
  const ptts_config &c = e->cfg;
  const float *src = nullptr;
  int M = 0, K = 0, F = 0;
  std::string n(name);
  if (!is_mimi) {
    ptts_lm_state *s = (ptts_lm_state *)state;
    if (n == "x") { src = s->dec.x; M = s->B; K = c.d_model; }
    else if (n == "ce") { src = s->ce; M = s->B; K = c.flow_dim; }
    else if (n == "fx") { src = s->fx; M = s->B; K = c.flow_dim; }
    else if (n == "mod") {  // AdaLN modulations of the last step's first LSD iteration, [B][(3 depth + 2) flow_dim]
      if (s->mod_stale) return fail(-1, "debug_read: mod is not materialised by a step with the flow fold (ptts_lm_state_set_flow_fold): the cluster computes it on chip");
      if (!s->mod) return fail(-1, "debug_read: mod is not allocated");
      src = s->mod; M = s->B; K = e->adaln.NT * 16;
    }
    else if (n == "prefill_x") { src = s->pre.x; M = s->pre.MT * 16; K = c.d_model; }
    else if (n == "noise") {  // the last step's LSD start point (noise), [B][ldim]
      if (!s->latfm_noise) return fail(-1, "debug_read: noise is only kept by steps that ran the flow cluster");
      src = s->latfm; M = s->B; K = c.ldim;
    }
    else return fail(-1, "unknown buffer " + n);
    F = K / 16;
  } else {
    ptts_mimi_state *s = (ptts_mimi_state *)state;
    const int par = (s->h_frame - 1) & 1;  // parity of the frame decoded last
    const int B = s->B;
    // the element type a buffer really has: the transformer's buffers and SEANet's skip / last-block buffers follow the
    // codec format (fp32 or bf16), the inputs of the fp8 convolutions are e4m3 (build_mimi_state's e_tr / e_sn)
    const int f_tr = e->codec_bf16 ? TAP_BF16 : TAP_F32, f_sn = e->codec_fp8 ? TAP_E4M3 : f_tr;
    const int trM = B * 16 * s->h_tr_last;  // rows of the last transformer launch
    int fmt = f_tr;
    const void *p = nullptr;
    auto index_of = [&](size_t prefix, int lo, int hi) {  // the decimal index behind the prefix, or -1
      if (n.size() <= prefix || n.size() > prefix + 2) return -1;
      for (size_t i = prefix; i < n.size(); ++i)
        if (n[i] < '0' || n[i] > '9') return -1;
      const int k = atoi(n.c_str() + prefix);
      return k >= lo && k <= hi ? k : -1;
    };
    auto plain = [&](int r, int k) -> int64_t {  // d_out already holds f32[r][k]
      LAUNCHCHK();
      *rows = r; *cols = k;
      return (int64_t)r * k;
    };
    if (n == "upsample" || n == "tr_in0") { p = s->u0; M = n == "upsample" ? B * 16 : trM; K = c.m_dim; }
    else if (n == "dec_tr") { p = s->tr_out.slot((s->h_frame - 1) & (s->tr_out.slots - 1)); M = B * 16; K = c.m_dim; }
    else if (n.compare(0, 11, "dec_tr_slot") == 0) {  // slot k of the hand-over ring (frame f lies in slot f & (slots - 1))
      const int k = index_of(11, 0, 3);
      if (k < 0) return fail(-1, "unknown buffer " + n);
      if (k >= s->tr_out.slots) return fail(-1, "debug_read: " + n + ": the hand-over ring of this codec format has " + std::to_string(s->tr_out.slots) + " slots");
      p = s->tr_out.slot(k); M = B * 16; K = c.m_dim;
    }
    else if (n == "seanet0") { p = s->a0.slot(par); fmt = f_sn; M = B * 16; K = 8 * c.n_filters; }
    else if (n == "tr_attn") { p = s->ao; M = B * 16; K = c.m_dim; }       // last layer's attention output
    else if (n == "tr_resid") { p = s->u; M = B * 16; K = c.m_dim; }       // last layer's stream after attention
    else if (n == "tr_ff") { p = s->ff; M = B * 16; K = c.m_ff; }          // last layer's GELU(linear1)
    else if (n.compare(0, 5, "tr_in") == 0 || n.compare(0, 7, "tr_attn") == 0 || n.compare(0, 8, "tr_resid") == 0 ||
             n.compare(0, 5, "tr_ff") == 0 || n.compare(0, 4, "tr_q") == 0) {
      // the same of layer l: the last layer's are the buffers themselves, an earlier layer's (and the input of a layer
      // >= 1) the copies made while "debug_taps" is set
      const size_t pre = n[3] == 'i' ? 5 : n[3] == 'a' ? 7 : n[3] == 'r' ? 8 : n[3] == 'f' ? 5 : 4;
      const char kind = n[3];
      const int last = c.m_layers - 1;
      const int l = n.size() == pre && kind == 'q' ? last : index_of(pre, kind == 'i' ? 1 : 0, last);
      if (l < 0) return fail(-1, "unknown buffer " + n);
      const bool copy = kind == 'i' || l < last;
      if (copy && (!s->tap_tr || !e->opt_debug_taps))
        return fail(-1, "debug_read: " + n + " is only kept with the engine option \"debug_taps\" set before decoding");
      if (copy && s->tap_frame != s->h_tr - s->h_tr_last)
        return fail(-1, "debug_read: " + n + " is stale: the last frame was not decoded eagerly with \"debug_taps\" set");
      const ptts_mimi_state::TrTap t = copy ? s->tr_tap(kind == 'i' ? l : l + 1) : ptts_mimi_state::TrTap{nullptr, s->u, s->ao, s->ff, s->q};
      M = trM; K = kind == 'f' ? c.m_ff : c.m_dim;
      p = kind == 'i' ? t.in : kind == 'a' ? t.ao : kind == 'r' ? t.resid : t.ff;
      if (kind == 'q') {  // the query blocks after RoPE: fp32 in every format
        K = c.m_heads * 64;
        if ((int64_t)M * K > capacity) return fail(-1, "debug_read: capacity too small");
        dbg_from_q_kernel<<<cdiv((long)M * K, 256), 256, 0, st>>>(t.q, d_out, M, c.m_heads, 16 * s->h_tr_last, s->h_tr_last);
        return plain(M, K);
      }
    }
    else if (n.compare(0, 4, "tr_k") == 0 || n.compare(0, 4, "tr_v") == 0) {  // every slot of a layer's ring, row b * ring + slot
      const int l = index_of(4, 0, c.m_layers - 1);
      if (l < 0) return fail(-1, "unknown buffer " + n);
      M = B * e->ring; K = c.m_heads * 64;
      if ((int64_t)M * K > capacity) return fail(-1, "debug_read: capacity too small");
      dbg_from_kv_kernel<<<cdiv((long)M * K, 256), 256, 0, st>>>(n[3] == 'k' ? s->K(l) : s->V(l), d_out, B, c.m_heads, e->ring);
      return plain(M, K);
    }
    else if (n.compare(0, 2, "w_") == 0 || n.compare(0, 3, "ws_") == 0 || n.compare(0, 3, "wh_") == 0 || n.compare(0, 3, "wl_") == 0 ||
             n.compare(0, 4, "lns_") == 0 || n.compare(0, 4, "lnc_") == 0) {
      // the weight image a reduced-precision launch multiplies by, [16 NT][ntaps * C] (k = tap * C + c in the packer's tap
      // order): bf16 values, or at the fp8 convolutions of an fp8 engine e4m3 codes, whose per-row scales are "ws_<site>";
      // "wh_<site>" / "wl_<site>": the hi and lo images of a split-bf16 engine, in the same order; "lns_<site>" /
      // "lnc_<site>": the LayerNorm fold vectors of a +ln site of the fp32 and split-bf16 codecs, [1][16 NT]
      const bool split_img = n[0] == 'w' && (n[1] == 'h' || n[1] == 'l'), fold = n[0] == 'l';
      if (split_img && !e->codec_split) return fail(-1, "debug_read: " + n + ": only a split-bf16 engine has hi / lo weight images");
      if (fold && e->codec_bf16) return fail(-1, "debug_read: " + n + ": the reduced-precision codecs keep their own fold vectors");
      if (!split_img && !fold && !e->codec_bf16) return fail(-1, "debug_read: " + n + ": the fp32 codec has no reduced-precision weight image");
      const bool scale = n[1] == 's';
      const size_t off = fold ? 4 : scale || split_img ? 3 : 2;
      const std::string site = n.substr(off);
      const Lin *L = nullptr;
      bool conv = false;  // a SEANet convolution that the fp8 codec runs on e4m3
      auto layer = [&](const char *pre) {
        const size_t k = strlen(pre);
        return site.compare(0, k, pre) == 0 ? index_of(off + k, 0, c.m_layers - 1) : -1;
      };
      auto stage = [&](const char *pre) {
        const size_t k = strlen(pre);
        return site.compare(0, k, pre) == 0 ? index_of(off + k, 1, 3) - 1 : -1;
      };
      int i;
      if ((i = layer("qkv")) >= 0) L = &e->mm[i].qkv;
      else if ((i = layer("out")) >= 0) L = &e->mm[i].out;
      else if ((i = layer("ff1")) >= 0) L = &e->mm[i].ff1;
      else if ((i = layer("ff2")) >= 0) L = &e->mm[i].ff2;
      else if (site == "conv0") L = &e->conv0;
      else if ((i = stage("convtr")) >= 0) { L = &e->convtr[i]; conv = true; }
      else if ((i = stage("res_a")) >= 0) { L = &e->res_a[i]; conv = true; }
      else if ((i = stage("res_b")) >= 0) { L = &e->res_b[i]; conv = true; }
      if (!L) return fail(-1, "unknown buffer " + n);
      if (fold) {
        if (!L->ln_s || !L->ln_c) return fail(-1, "debug_read: " + n + ": the site folds no LayerNorm");
        if (capacity < L->NT * 16) return fail(-1, "debug_read: capacity too small");
        HIPCHK(hipMemcpyAsync(d_out, n[2] == 's' ? L->ln_s : L->ln_c, (size_t)L->NT * 16 * 4, hipMemcpyDeviceToDevice, st));
        return plain(1, L->NT * 16);
      }
      if (split_img) {
        if (!L->wsh || !L->wsl) return fail(-1, "debug_read: " + n + ": the site has no split image");
        const long nk = (long)L->NT * 16 * L->KF * 16;
        if (nk > capacity) return fail(-1, "debug_read: capacity too small");
        dbg_unpack_weight_kernel<<<cdiv(nk, 256), 256, 0, st>>>(n[1] == 'h' ? L->wsh : L->wsl, nullptr, 2, d_out, L->NT * 16, L->KF);
        return plain(L->NT * 16, L->KF * 16);
      }
      const bool f8w = conv && e->codec_fp8;
      if (scale && !f8w) return fail(-1, "debug_read: " + n + ": the site has no e4m3 weight image in this codec format");
      const int Nn = L->NT * 16, KBt = (L->C / 32) * L->ntaps;
      if (scale) {
        if (capacity < Nn) return fail(-1, "debug_read: capacity too small");
        HIPCHK(hipMemcpyAsync(d_out, L->wscale8, (size_t)Nn * 4, hipMemcpyDeviceToDevice, st));
        return plain(1, Nn);
      }
      if ((int64_t)Nn * KBt * 32 > capacity) return fail(-1, "debug_read: capacity too small");
      dbg_unpack_codec_weight_kernel<<<cdiv((long)Nn * KBt * 32, 256), 256, 0, st>>>(f8w ? L->wf8 : (const void *)L->wh, nullptr, f8w ? 2 : 0,
                                                                                    d_out, Nn, KBt);
      return plain(Nn, KBt * 32);
    }
    else if (n == "f8_scales") {  // the activation scales the fp8 convolutions run with (the host mirror the launches read)
      if (!e->codec_fp8) return fail(-1, "debug_read: f8_scales: the engine has no fp8 codec");
      if (capacity < 16) return fail(-1, "debug_read: capacity too small");
      HIPCHK(hipMemcpyAsync(d_out, e->f8s, sizeof(e->f8s), hipMemcpyHostToDevice, st));
      return plain(1, 16);
    }
    else if (n.compare(0, 12, "calib_latent") == 0) {  // what calibrate_fp8_codec fed in frame f (its state has batch 8)
      const int f = index_of(12, 0, 5);
      if (f < 0) return fail(-1, "unknown buffer " + n);
      if (B != 8) return fail(-1, "debug_read: " + n + " needs a state of batch 8, the calibration run's");
      if (capacity < (int64_t)B * c.ldim) return fail(-1, "debug_read: capacity too small");
      calib_latent(st, d_out, B * c.ldim, (unsigned)f);
      return plain(B, c.ldim);
    }
    else if (n == "seanet11") {
      M = B; K = s->rows[3];
      if ((int64_t)M * K > capacity) return fail(-1, "capacity");
      if (hipMemcpyAsync(d_out, s->pcm_dbg, (size_t)M * K * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return fail(-2, "memcpy");
      *rows = M; *cols = K;
      return (int64_t)M * K;
    } else if (n.compare(0, 8, "seanet_c") == 0 || n.compare(0, 8, "seanet_h") == 0) {
      // stage i's transposed-conv output as the k3 conv reads it (ELU'd; the fp32 codec's "single_store" keeps it raw), and
      // the block's hidden activation
      const int i = index_of(8, 1, 3) - 1;
      if (i < 0) return fail(-1, "unknown buffer " + n);
      const int cout = (8 >> i) * c.n_filters / 2;
      M = B * s->rows[i + 1]; fmt = f_sn;
      if (n[7] == 'c') { p = s->cbuf[i].slot(par); K = cout; }
      else {
        if (!e->codec_bf16 && resblock_fused(s, i)) return fail(-1, "debug_read: " + n + " stays on chip in the fused residual block");
        p = s->rbuf[i]; K = cout / c.compress;
      }
    } else {
      int idx = atoi(n.c_str() + 6);
      if (n.compare(0, 6, "seanet") != 0 || idx < 2 || idx > 9) return fail(-1, "unknown buffer " + n);
      int stage = (idx - 2) / 3;
      bool is_res = (idx - 2) % 3 == 1;
      if ((idx - 2) % 3 == 2) return fail(-1, "unknown buffer " + n);
      int mult = 8 >> stage;
      K = mult * c.n_filters / 2;
      M = B * s->rows[stage + 1];
      if (is_res && stage == 2 && seanet_fuses_pcm(s) && !s->e->opt_debug_taps)
        return fail(-1, "debug_read: " + n + " stays on chip with \"fuse_pcm\"; set the engine option \"debug_taps\" before decoding");
      // the reduced-precision codecs always keep the raw skip input in craw (bf16); their block outputs are e4m3 where an
      // fp8 convolution reads them (stages 1 and 2) and bf16 in front of the last conv
      if (is_res) { p = s->sbuf[stage].slot(par); fmt = stage == 2 ? f_tr : f_sn; }
      else p = e->codec_bf16 ? s->craw[stage] : seanet_single_store(s->e, stage) ? s->cbuf[stage].slot(par) : s->craw[stage];
    }
    if (fmt != TAP_F32) {  // FMH bf16 / FM8 e4m3 (decoded codes, unscaled: the reader applies the scale)
      if (K % 32) return fail(-1, "debug_read: " + n + ": the reduced-precision layouts hold 32-column blocks");
      if ((int64_t)M * K > capacity) return fail(-1, "debug_read: capacity too small");
      dbg_from_codec_kernel<<<cdiv((long)M * K, 256), 256, 0, st>>>(p, d_out, M, K, K / 32, fmt == TAP_BF16 ? 0 : 1);
      return plain(M, K);
    }
    src = (const float *)p;
    F = K / 16;
  }
  if ((int64_t)M * K > capacity) return fail(-1, "debug_read: capacity too small");
  long n4 = (long)M * (K / 4);
  from_fm_kernel<<<cdiv(n4, 256), 256, 0, st>>>(src, d_out, M, K, F, 0);
  *rows = M;
  *cols = K;
  return (int64_t)M * K;
}

// ------------------------------------------------------------------------------------------------
// ptts_debug_gemm (test hook, include/ptts.h): one GEMM of the kernel family, packed by pack_lin and launched by
// launch_gemm_cfg, between plain row-major buffers and the FM layout

// [M][K] row-major -> FM with MT x KF fragments (rows >= M and columns >= K are zero); one thread per float
static __global__ void dbg_to_fm_kernel(const float *src, float *dst, int M, int K, int MT, int KF) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)MT * KF * 256) return;
  const int j = i & 3, lane = (i >> 2) & 63;
  const long f = i >> 8;
  const int kf = f % KF, mt = f / KF;
  const int m = 16 * mt + (lane & 15), k = 16 * kf + 4 * (lane >> 4) + j;
  dst[i] = (m < M && k < K) ? src[(size_t)m * K + k] : 0.f;
}
// FM (NF fragments per row tile) -> [M][N] row-major
static __global__ void dbg_from_fm_kernel(const float *src, float *dst, int M, int N, int NF) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)M * N) return;
  const int m = i / N, n = i - (long)m * N;
  dst[i] = src[(((size_t)(m >> 4) * NF + (n >> 4)) * 64 + 16 * ((n & 15) >> 2) + (m & 15)) * 4 + (n & 3)];
}
// weights a packed image holds, as [N][KF * 16] fp32 (k = tap * C + c): fmt 0 = fp32 image, 1 = int8 image times its
// per-row scale, 2 = bf16 image ([NT][KF/2][64][8], also each half of a split pair)
static __global__ void dbg_unpack_weight_kernel(const void *img, const float *scale, int fmt, float *dst, int N, int KF) {
  const long K = (long)KF * 16;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)N * K) return;
  const int n = i / K, k = i - (long)n * K;
  const int nt = n >> 4, kf = k >> 4, j = k & 3, lane = 16 * ((k & 15) >> 2) + (n & 15);
  float v;
  if (fmt == 0) v = ((const float *)img)[(((size_t)nt * KF + kf) * 64 + lane) * 4 + j];
  else if (fmt == 1) v = ((float)((const uint8_t *)img)[(size_t)nt * KF * 256 + (size_t)(kf >> 2) * 1024 + lane * 16 + 4 * (kf & 3) + j] - 128.f) * scale[n];
  else v = (float)((const __bf16 *)img)[(((size_t)nt * (KF / 2) + (kf >> 1)) * 64 + lane) * 8 + (kf & 1) * 4 + j];
  dst[i] = v;
}

static int debug_gemm(ptts_engine *e, ptts_gemm_case *c, hipStream_t st, ptts_engine &scr) {
  const int M = c->M, N = c->N, C = c->C, ntaps = c->ntaps, pre = c->pre;
  c->cfg_used = -1;
  if (!c->x || !c->w || !c->y) return fail(-1, "debug_gemm: x, w and y are required");
  if (M < 1 || N < 1 || C < 16 || C % 16 || ntaps < 1) return fail(-1, "debug_gemm: bad shape");
  if (c->wfmt < 0 || c->wfmt > 3 || pre < PRE_NONE || pre > PRE_LNMOD || c->epi < EPI_STORE || c->epi > EPI_GATE ||
      c->act < ACT_NONE || c->act > ACT_ELU || c->cfg < -1 || c->cfg >= kNumCfg)
    return fail(-1, "debug_gemm: enumeration out of range");
  if (c->lds_target < 0 || c->lds_target > 64 * 1024) return fail(-1, "debug_gemm: lds_target above 64 KB");
  int rows_in = M;
  if (ntaps > 1) {
    // every input row the kernel addresses lies in the sequence's own rows of x or x_prev
    if (c->T < 16 || c->T % 16 || M % c->T || c->xstride < 1 || c->halo < 0 || c->halo > c->T * c->xstride ||
        ntaps - 1 - c->halo >= c->xstride || c->halo_mode < 0 || c->halo_mode > 2 || (c->halo_mode == 0 && !c->x_prev))
      return fail(-1, "debug_gemm: bad convolution geometry");
    if (pre == PRE_LNFOLD || pre == PRE_LNMOD || pre == PRE_ADDSILU) return fail(-1, "debug_gemm: per-channel prologues are for Linear layers");
    rows_in = M * c->xstride;
  } else if (c->xstride != 1) {
    return fail(-1, "debug_gemm: a Linear has xstride 1");
  }
  if ((pre == PRE_LNFOLD && (!c->ln_w || !c->ln_b)) || (pre == PRE_ADDSILU && !c->prevec) ||
      (pre == PRE_LNMOD && (!c->mod_shift || !c->mod_scale || !c->ln_w != !c->ln_b)))
    return fail(-1, "debug_gemm: missing prologue operand");
  if ((c->epi == EPI_RES && !c->r) || (c->epi == EPI_GATE && (!c->r || !c->g))) return fail(-1, "debug_gemm: missing epilogue operand");
  if (c->wfmt >= 2 && (C / 16) * ntaps % 2) return fail(-1, "debug_gemm: bf16 images need an even number of k-fragments");

  // pack with the engine's own code: a scratch engine whose tensor map holds the case's operands
  const ptts_tensor tw{"w", c->w, (int64_t)N * C * ntaps}, tb{"b", c->bias, N}, tg{"ln_w", c->ln_w, C}, tbe{"ln_b", c->ln_b, C};
  scr.tmap["w"] = &tw;
  if (c->bias) scr.tmap["b"] = &tb;
  if (pre == PRE_LNFOLD) { scr.tmap["ln_w"] = &tg; scr.tmap["ln_b"] = &tbe; }
  Lin L;
  const bool fold = pre == PRE_LNFOLD;
  CHK(pack_lin(&scr, &L, {{"w", c->bias ? "b" : "", N}}, C, ntaps, 0, 0, 0, fold ? "ln_w" : "", fold ? "ln_b" : "", 0,
               c->wfmt == 3 ? 0 : c->wfmt));
  if (c->wfmt == 3) {
    CHK(dalloc(&scr, &L.wsh, (size_t)L.NT * L.KF * 512));
    CHK(dalloc(&scr, &L.wsl, (size_t)L.NT * L.KF * 512));
    pack_weight_split(st, L.w, L.wsh, L.wsl, L.NT, L.KF);
  }
  const int NT = L.NT, MT = cdiv(M, 16), MTin = cdiv(rows_in, 16), CF = L.CF;
  // x: current frame, then the previous one (the kernel's frame-parity double buffer with parity 0)
  float *xfm = nullptr;
  const long xfl = (long)MTin * CF * 256;
  CHK(dallocT(&scr, &xfm, 2 * xfl));
  dbg_to_fm_kernel<<<cdiv(xfl, 256), 256, 0, st>>>(c->x, xfm, rows_in, C, MTin, CF);
  if (c->x_prev) dbg_to_fm_kernel<<<cdiv(xfl, 256), 256, 0, st>>>(c->x_prev, xfm + xfl, rows_in, C, MTin, CF);
  auto to_fm = [&](const float *src, int rows, int cols, int mt, int kf, float **out) -> int {
    CHK(dallocT(&scr, out, (size_t)mt * kf * 256));
    dbg_to_fm_kernel<<<cdiv((long)mt * kf * 256, 256), 256, 0, st>>>(src, *out, rows, cols, mt, kf);
    return 0;
  };
  auto copy_pad = [&](const float *src, int n, int pad, float **out) -> int {  // [n] -> zero-padded [pad]
    CHK(dallocT(&scr, out, (size_t)pad));
    HIPCHK(hipMemcpyAsync(*out, src, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    return 0;
  };
  const long yfl = (long)MT * NT * 256;
  float *yfm = nullptr;
  CHK(dallocT(&scr, &yfm, yfl + kDbgGuardFloats));
  HIPCHK(hipMemsetD32Async((hipDeviceptr_t)yfm, (int)kDbgUnwritten, yfl, st));
  HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(yfm + yfl), (int)kDbgGuard, kDbgGuardFloats, st));

  GemmArgs a = mk_gemm(L, xfm, CF, MT, M);
  if (c->wfmt == 3) { a.Wq = (const uint8_t *)L.wsh; a.W = (const float *)L.wsl; a.wfmt = 3; }
  a.Xdstride = xfl;
  a.T = ntaps > 1 ? c->T : 16;
  a.xstride = c->xstride;
  a.halo = c->halo;
  a.halo_mode = c->halo_mode;
  a.zeros = e->zeros;
  a.krot = c->krot;
  a.epi = c->epi;
  a.act = c->act;
  a.Y = yfm;
  a.YF = NT;
  float *tmp = nullptr;
  if (pre == PRE_ADDSILU) { CHK(copy_pad(c->prevec, C, C, &tmp)); a.prevec = tmp; }
  if (pre == PRE_LNMOD) {
    if (c->ln_w) {
      CHK(copy_pad(c->ln_w, C, C, &tmp)); a.lnm_w = tmp;
      CHK(copy_pad(c->ln_b, C, C, &tmp)); a.lnm_b = tmp;
    }
    CHK(to_fm(c->mod_shift, M, C, MT, CF, &tmp)); a.mod_shift = tmp;
    CHK(to_fm(c->mod_scale, M, C, MT, CF, &tmp)); a.mod_scale = tmp;
    a.modF = CF;
  }
  if (c->epi == EPI_RES || c->epi == EPI_GATE) { CHK(to_fm(c->r, M, N, MT, NT, &tmp)); a.R = tmp; a.RF = NT; }
  if (c->epi == EPI_GATE) { CHK(to_fm(c->g, M, N, MT, NT, &tmp)); a.G = tmp; a.GF = NT; }
  if (c->epi == EPI_RES && c->ls) { CHK(copy_pad(c->ls, N, NT * 16, &tmp)); a.ls = tmp; }

  KnobScope knobs(c->lds_target, c->krot);  // the dispatcher's per-thread knobs for this one launch
  int cfg = c->cfg;
  if (cfg >= 0 ? !(pre_supported(a.wfmt, pre) && cfg_valid(cfg, a, pre)) : (cfg = choose_cfg(st, a, pre)) < 0) {
    HIPCHK(hipStreamSynchronize(st));
    return 1;
  }
  std::string label;
  launch_gemm_cfg(st, a, pre, cfg, &label);
  LAUNCHCHK();
  c->cfg_used = cfg;
  put_label(label, c->label, c->label_cap);
  dbg_from_fm_kernel<<<cdiv((long)M * N, 256), 256, 0, st>>>(yfm, c->y, M, N, NT);
  const long nk = (long)N * L.KF * 16;
  if (c->w_eff) {
    if (c->wfmt == 0) dbg_unpack_weight_kernel<<<cdiv(nk, 256), 256, 0, st>>>(L.w, nullptr, 0, c->w_eff, N, L.KF);
    else if (c->wfmt == 1) dbg_unpack_weight_kernel<<<cdiv(nk, 256), 256, 0, st>>>(L.wq, L.wscale, 1, c->w_eff, N, L.KF);
    else dbg_unpack_weight_kernel<<<cdiv(nk, 256), 256, 0, st>>>(c->wfmt == 2 ? L.wb16 : L.wsh, nullptr, 2, c->w_eff, N, L.KF);
  }
  if (c->w_eff_lo && c->wfmt == 3) dbg_unpack_weight_kernel<<<cdiv(nk, 256), 256, 0, st>>>(L.wsl, nullptr, 2, c->w_eff_lo, N, L.KF);
  if (fold && c->ln_s) HIPCHK(hipMemcpyAsync(c->ln_s, L.ln_s, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
  if (fold && c->ln_c) HIPCHK(hipMemcpyAsync(c->ln_c, L.ln_c, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
  return check_guards(scr, st, {yfm + yfl}, kDbgGuardFloats, "debug_gemm: " + label + " wrote past its output");
}

extern "C" int ptts_debug_gemm(ptts_engine *e, ptts_gemm_case *c, void *stream) {
  if (!e || !c) return fail(-1, "debug_gemm: null argument");
  return run_case(e, stream, [&](hipStream_t st, ptts_engine &scr) { return debug_gemm(e, c, st, scr); });
}

// ------------------------------------------------------------------------------------------------
// ptts_debug_attn (test hook, include/ptts.h): one attention launch (+ combine) through launch_attention, between plain
// row-major buffers and the kernels' Q block / cache / FM layouts.  Every slot the case must not read holds the case's
// poison, and every buffer has a poisoned guard of one key tile (1024 floats) on both sides.

// q [B][Tq][H][64] -> Q blocks [B * H][QB][4][64 lanes][4]: lane c + 16 g of fragment df holds query 16 qb + c, d = 16 df
// + 4 g + j (queries >= Tq of the last block hold poison)
static __global__ void dbg_attn_q_kernel(const float *q, float *Q, int B, int Tq, int H, int QB, float poison) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * H * QB * 1024) return;
  const int j = i & 3, lane = (i >> 2) & 63, df = (i >> 8) & 3;
  const long r = i >> 10;
  const int qb = r % QB, bh = r / QB, b = bh / H, h = bh - b * H;
  const int t = 16 * qb + (lane & 15), d = 16 * df + 4 * (lane >> 4) + j;
  Q[i] = t < Tq ? q[(((size_t)b * Tq + t) * H + h) * 64 + d] : poison;
}

// the position whose key a row's cache slot holds when the row's queries are at off .. off + Tq - 1, or -1 (poison):
// ring slots hold the newest position of their class below off + Tq; keys before every query's window, past the last
// query, and under a borrowed prefix tile (positions < 16 * (len / 16)) are never read
static __device__ int dbg_attn_slot_pos(int s, int off, int Tq, int ring, int ctx, int len) {
  const int top = off + Tq - 1;
  int p = s;
  if (ring) {
    if (s >= ring) return -1;
    p = top - (((top - s) % ring) + ring) % ring;
  }
  if (p < 0 || p > top || (ctx > 0 && p < off - ctx + 1) || p < 16 * (len >> 4)) return -1;
  return p;
}
// K and V caches [B][H][cap][64] of the rows (one thread per float)
static __global__ void dbg_attn_cache_kernel(const float *k, const float *v, const float *pk, const float *pv, float *Kc,
                                             float *Vc, const int *offset, const int *pre_len, const int *pre_id, int B,
                                             int T, int pre_T, int H, int cap, int Tq, int ring, int ctx, float poison_k,
                                             float poison_v) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * H * cap * 64) return;
  const int d = i & 63;
  const long r = i >> 6;
  const int s = r % cap, bh = r / cap, b = bh / H, h = bh - b * H;
  const int id = pre_id ? pre_id[b] : -1, len = id >= 0 ? pre_len[id] : 0;
  const int p = dbg_attn_slot_pos(s, offset[b], Tq, ring, ctx, len);
  if (p < 0) {
    Kc[i] = poison_k;
    Vc[i] = poison_v;
  } else if (p < len) {  // the part of the prefix's last, partial tile the row holds itself
    Kc[i] = pk[(((size_t)id * pre_T + p) * H + h) * 64 + d];
    Vc[i] = pv[(((size_t)id * pre_T + p) * H + h) * 64 + d];
  } else {
    Kc[i] = k[(((size_t)b * T + p) * H + h) * 64 + d];
    Vc[i] = v[(((size_t)b * T + p) * H + h) * 64 + d];
  }
}
// the prefix owners' caches: bank `id` = [L][2][1][H][pcap][64] at bank + id * bstride, layer `layer` positions < len
// from pk / pv, every other float poison (K planes poison_k, V planes poison_v)
static __global__ void dbg_attn_owner_kernel(const float *pk, const float *pv, float *bank, long bstride, const int *pre_len,
                                             int nbank, int L, int layer, int H, int pcap, int pre_T, float poison_k,
                                             float poison_v) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per = (long)L * 2 * H * pcap * 64;
  if (i >= nbank * per) return;
  const int id = i / per;
  const long e = i - id * per;
  const int d = e & 63;
  const long r = e >> 6;
  const int s = r % pcap, pl = r / pcap, h = pl % H, which = (pl / H) & 1, l = pl / (2 * H);
  float x = which ? poison_v : poison_k;
  if (l == layer && s < pre_len[id]) x = (which ? pv : pk)[(((size_t)id * pre_T + s) * H + h) * 64 + d];
  bank[id * bstride + kAttnGuard + e] = x;
}

static int debug_attn(ptts_attn_case *c, hipStream_t st, ptts_engine &scr) {
  const int B = c->B, Tq = c->Tq, H = c->H, T = c->T, cap = c->cap, ring = c->ring, ctx = c->ctx, NB = c->n_pre;
  const int pcap = c->pre_cap > 0 ? c->pre_cap : cap;
  c->kernel_used = -1;
  c->splits_used = 0;
  if (!c->q || !c->k || !c->v || !c->y || !c->offset) return fail(-1, "debug_attn: q, k, v, offset and y are required");
  if (B < 1 || Tq < 1 || H < 1 || T < Tq || cap < 16 || c->layer < 0 || NB < 0 || c->splits < -1 || c->splits == 0 ||
      c->kernel < -1 || c->kernel >= kNumAttn || (c->h16 != 0 && c->h16 != 1))
    return fail(-1, "debug_attn: bad shape or enumeration");
  if (NB > 0 && (!c->pk || !c->pv || !c->pre_len || !c->pre_id || c->pre_T < 1 || pcap % 16))
    return fail(-1, "debug_attn: prefixes need pk, pv, pre_len, pre_id, pre_T and a capacity % 16 == 0");
  for (int j = 0; j < NB; ++j)
    if (c->pre_len[j] < 0 || c->pre_len[j] > c->pre_T || c->pre_len[j] > pcap) return fail(-1, "debug_attn: prefix length out of range");
  for (int b = 0; b < B; ++b) {
    const int off = c->offset[b];
    if (off < 0 || off + Tq > T || (!ring && off + Tq > cap)) return fail(-1, "debug_attn: a row's queries lie outside k / v or its cache");
    if (NB > 0 && (c->pre_id[b] < -1 || c->pre_id[b] >= NB || (c->pre_id[b] >= 0 && c->pre_len[c->pre_id[b]] > off)))
      return fail(-1, "debug_attn: a row's prefix is unknown or longer than its first query's position");
  }
  const int QB = cdiv(Tq, 16), BH = B * H, M = B * Tq, MT = cdiv(M, 16);
  int splits = c->splits;
  if (splits < 0) {  // the production rule of the launch shape the case has
    if (Tq == 1 && !ring) splits = 1;                                                   // FlowLM decode step
    else if (ring) splits = attn_splits(BH, ring / 16);                                 // codec frame (the state's splits)
    else if (ctx > 0) splits = attn_splits(BH * QB, std::min(QB, cdiv(ctx, 16) + 2));   // encoder transformer
    else splits = attn_splits(BH * QB, cdiv(cap, 16));                                  // FlowLM prefill
  }
  const long G = kAttnGuard;
  auto poisoned = [&](long n, float val, float **out) -> int {  // n floats between two guards, all `val`
    CHK(dallocT(&scr, out, (size_t)(n + 2 * G)));
    fill_kernel<<<cdiv(n + 2 * G, 256), 256, 0, st>>>(*out, n + 2 * G, val);
    *out += G;
    return 0;
  };
  auto patterned = [&](long n, unsigned inner, float **out) -> int {  // guards kDbgGuard, inside `inner`
    CHK(dallocT(&scr, out, (size_t)(n + 2 * G)));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)*out, (int)kDbgGuard, G, st));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(*out + G), (int)inner, n, st));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(*out + G + n), (int)kDbgGuard, G, st));
    *out += G;
    return 0;
  };
  int *d_ints = nullptr;  // offset [B], pre_id [B], pre_len [NB]
  CHK(dallocT(&scr, &d_ints, (size_t)2 * B + NB + 1));
  HIPCHK(hipMemcpyAsync(d_ints, c->offset, (size_t)B * 4, hipMemcpyHostToDevice, st));
  if (NB > 0) {
    HIPCHK(hipMemcpyAsync(d_ints + B, c->pre_id, (size_t)B * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_ints + 2 * B, c->pre_len, (size_t)NB * 4, hipMemcpyHostToDevice, st));
  }
  float *Q, *Kc, *Vc, *Y, *part = nullptr;
  const long nq = (long)BH * QB * 1024, nkv = (long)BH * cap * 64;
  CHK(poisoned(nq, c->poison_k, &Q));
  dbg_attn_q_kernel<<<cdiv(nq, 256), 256, 0, st>>>(c->q, Q, B, Tq, H, QB, c->poison_k);
  CHK(poisoned(nkv, c->poison_k, &Kc));
  CHK(poisoned(nkv, c->poison_v, &Vc));
  dbg_attn_cache_kernel<<<cdiv(nkv, 256), 256, 0, st>>>(c->k, c->v, c->pk, c->pv, Kc, Vc, d_ints, NB > 0 ? d_ints + 2 * B : nullptr,
                                                         NB > 0 ? d_ints + B : nullptr, B, T, c->pre_T, H, cap, Tq, ring, ctx,
                                                         c->poison_k, c->poison_v);
  KvPrefix *d_pre = nullptr;
  if (NB > 0) {
    // owners: one allocation, bank id at id * bstride, each bank between guards of poison; layers 0 .. layer + 1
    const int L = c->layer + 2;
    const long per = (long)L * 2 * H * pcap * 64, bstride = per + 2 * G;
    float *bank = nullptr;
    CHK(dallocT(&scr, &bank, (size_t)NB * bstride));
    fill_kernel<<<cdiv(NB * bstride, 256), 256, 0, st>>>(bank, NB * bstride, c->poison_k);
    dbg_attn_owner_kernel<<<cdiv(NB * per, 256), 256, 0, st>>>(c->pk, c->pv, bank, bstride, d_ints + 2 * B, NB, L, c->layer, H,
                                                               pcap, c->pre_T, c->poison_k, c->poison_v);
    std::vector<KvPrefix> h_pre(B, KvPrefix{nullptr, 0, 0});
    for (int b = 0; b < B; ++b)
      if (c->pre_id[b] >= 0) h_pre[b] = KvPrefix{bank + c->pre_id[b] * bstride + G, pcap, c->pre_len[c->pre_id[b]]};
    CHK(dallocT(&scr, &d_pre, (size_t)B));
    HIPCHK(hipMemcpyAsync(d_pre, h_pre.data(), (size_t)B * sizeof(KvPrefix), hipMemcpyHostToDevice, st));
  }
  // output: FM (fp32, 4 H fragments per row tile) or FMH (bf16, 2 H blocks), NaN-filled between guards
  const int YF = c->h16 ? 2 * H : 4 * H;
  const long ny = (long)MT * YF * 256;  // floats (an FMH block of 32 columns holds 512 bf16)
  CHK(patterned(ny, c->h16 ? 0x7fc07fc0u : kDbgUnwritten, &Y));
  const long npart = (long)BH * QB * splits * 16 * ATT_PSTRIDE;
  if (splits > 1) CHK(patterned(npart, kDbgUnwritten, &part));

  AttnArgs at;
  at.Q = Q; at.Kc = Kc; at.Vc = Vc; at.pre = d_pre; at.layer = c->layer; at.offset = d_ints;
  at.H = H; at.Tq = Tq; at.QB = QB; at.cap = cap; at.ring = ring; at.ctx = ctx; at.splits = splits;
  at.part = part; at.Y = Y; at.YF = YF; at.h16 = c->h16; at.nseq = B;
  int k = c->kernel >= 0 ? c->kernel : choose_attn(at, BH, c->cascade);
  if (!attn_valid(k, at)) {
    HIPCHK(hipStreamSynchronize(st));
    if (c->kernel >= 0) return 1;
    return fail(-1, std::string("debug_attn: the dispatcher chose ") + kAttn[k].name + ", which attn_valid rejects");
  }
  std::string label;
  k = launch_attention(st, at, BH, c->cascade, k, 0, 0, &label);
  LAUNCHCHK();
  c->kernel_used = k;
  c->splits_used = splits;
  put_label(label, c->label, c->label_cap);
  if (c->h16) dbg_from_codec_kernel<<<cdiv((long)M * H * 64, 256), 256, 0, st>>>(Y, c->y, M, H * 64, YF, 0);
  else dbg_from_fm_kernel<<<cdiv((long)M * H * 64, 256), 256, 0, st>>>(Y, c->y, M, H * 64, YF);
  std::vector<const void *> guards = {Y - G, Y + ny};
  if (part) guards.insert(guards.end(), {part - G, part + npart});
  return check_guards(scr, st, guards, G, "debug_attn: " + label + " wrote past its output or partial buffer");
}

extern "C" int ptts_debug_attn(ptts_engine *e, ptts_attn_case *c, void *stream) {
  if (!e || !c) return fail(-1, "debug_attn: null argument");
  return run_case(e, stream, [&](hipStream_t st, ptts_engine &scr) { return debug_attn(c, st, scr); });
}

// ------------------------------------------------------------------------------------------------
// ptts_debug_codec_gemm (test hook, include/ptts.h): one GEMM of the reduced-precision codec (gemm_h_kernel /
// gemm_f8_kernel) or its last conv (pcm_conv_h_kernel), packed by pack_lin_h / pack_weight_f8 and launched by
// launch_h_tile / launch_f8_tile, between plain row-major buffers and the FMH / FM8 layouts

// [M][C] row-major -> FMH (fmt 0) / FM8 (fmt 1, saturate(x * inv_xs)) with `rows` rows (rows >= M are zero); eff != null
// receives the values the kernel reads (e4m3: decoded times xs).  One thread per 4 columns of a row.
static __global__ void dbg_to_codec_kernel(const float *src, void *dst, float *eff, int M, int C, int rows, int fmt, float inv_xs, float xs) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)rows * (C / 4)) return;
  const int m = i / (C / 4), c0 = 4 * (int)(i - (long)m * (C / 4));
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (src && m < M) v = *(const f32x4 *)(src + (size_t)m * C + c0);
  const size_t o = fmh_off(m, c0, C / 32);
  f32x4 d;
  if (fmt == 0) {
    const bf16x4 h = to_bf16x4(v);
    *(bf16x4 *)((__bf16 *)dst + o) = h;
    d = from_bf16x4(h);
  } else {
    const unsigned q = to_f8x4(v * inv_xs);
    *(unsigned *)((uint8_t *)dst + o) = q;
    d = (f32x4){dbg_e4m3(q & 255), dbg_e4m3((q >> 8) & 255), dbg_e4m3((q >> 16) & 255), dbg_e4m3(q >> 24)} * xs;
  }
  if (eff && m < M) *(f32x4 *)(eff + (size_t)m * C + c0) = d;
}
// weights of a codec image [NT][KBt][64][8] as [N][KBt * 32] f32 (k = tap * C + c): fmt 0 bf16, 1 e4m3 times scale[n], 2 e4m3
// codes
static __global__ void dbg_unpack_codec_weight_kernel(const void *img, const float *scale, int fmt, float *dst, int N, int KBt) {
  const long K = (long)KBt * 32;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)N * K) return;
  const int n = i / K, k = i - (long)n * K;
  const size_t o = (((size_t)(n >> 4) * KBt + (k >> 5)) * 64 + 16 * ((k & 31) >> 3) + (n & 15)) * 8 + (k & 7);
  dst[i] = fmt == 0 ? (float)((const __bf16 *)img)[o] : fmt == 2 ? dbg_e4m3(((const uint8_t *)img)[o]) : dbg_e4m3(((const uint8_t *)img)[o]) * scale[n];
}
// EPI_QKV outputs -> [M][3 * H * 64]: q from its block layout, k / v from cache slot pos % ring (ring 0: pos)
static __global__ void dbg_from_qkv_kernel(const float *Q, const float *Kc, const float *Vc, const int *offset, float *dst, int M,
                                           int H, int Tq, int QB, int cap, int ring) {
  const int D = H * 64;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)M * 3 * D) return;
  const int m = i / (3 * D), n = i - (long)m * 3 * D;
  const int which = n / D, hn = n - which * D, h = hn >> 6, d = hn & 63;
  const int b = m / Tq, t = m - b * Tq;
  const size_t bh = (size_t)b * H + h;
  if (which == 0) {
    dst[i] = Q[(((bh * QB + (t >> 4)) * 4 + (d >> 4)) * 64 + 16 * ((d & 15) >> 2) + (t & 15)) * 4 + (d & 3)];
  } else {
    const int pos = offset[b] + t, slot = ring ? pos % ring : pos;
    dst[i] = (which == 1 ? Kc : Vc)[(bh * cap + slot) * 64 + d];
  }
}

static int debug_codec_gemm(ptts_engine *e, ptts_codec_gemm_case *c, hipStream_t st, ptts_engine &scr) {
  const int M = c->M, N = c->N, C = c->C, ntaps = c->ntaps, pre = c->pre, epi = c->epi, fmt = c->fmt;
  const bool pcm = c->kind == 1;
  c->cfg_used = -1;
  if (!c->x || !c->w || !c->y) return fail(-1, "debug_codec_gemm: x, w and y are required");
  if (fmt < 0 || fmt > 1 || c->kind < 0 || c->kind > 1 || (pre != PRE_NONE && pre != PRE_LNFOLD) || c->act < ACT_NONE || c->act > ACT_ELU ||
      (epi != EPI_STORE && epi != EPI_RES && epi != EPI_QKV && epi != EPI_CONVTR) || c->cfg < -1 || c->cfg > 3 || c->mode < 0 ||
      c->mode > 1 || c->par < 0 || c->par > 1)
    return fail(-1, "debug_codec_gemm: enumeration out of range");
  if (M < 1 || N < 1 || C < 32 || ntaps < 1) return fail(-1, "debug_codec_gemm: bad shape");
  if (ntaps > 1 || pcm) {
    if (c->T < 16 || c->T % 16 || M % c->T || c->halo < 0 || c->halo > ntaps - 1 || c->halo > c->T)
      return fail(-1, "debug_codec_gemm: bad convolution geometry");
  } else if (c->halo) {
    return fail(-1, "debug_codec_gemm: a Linear has halo 0");
  }
  if (c->mode == 1 && (ntaps != 2 || c->cout < 1 || c->stride < 1 || N != c->cout * c->stride))
    return fail(-1, "debug_codec_gemm: a ConvTranspose image needs ntaps 2 and N = stride * cout");
  if (epi == EPI_CONVTR && (c->cout < 1 || c->stride < 1 || N != c->cout * c->stride)) return fail(-1, "debug_codec_gemm: ConvTranspose needs N = stride * cout");
  if ((epi == EPI_RES && !c->r) || (pre == PRE_LNFOLD && (!c->ln_w || !c->ln_b))) return fail(-1, "debug_codec_gemm: missing operand");
  if (epi == EPI_QKV && (c->H < 1 || N != 3 * c->H * 64 || c->Tq < 1 || M % c->Tq || !c->offset || c->cap < 1 || c->ring < 0 ||
                         c->ring > c->cap || (c->ring && c->Tq > c->ring)))
    return fail(-1, "debug_codec_gemm: bad QKV geometry");
  if (fmt == 1 && c->xs <= 0.f) return fail(-1, "debug_codec_gemm: the e4m3 activation scale xs must be positive");
  if (c->yf8 && c->yinv <= 0.f) return fail(-1, "debug_codec_gemm: yinv must be positive");
  // combinations no kernel implements: nothing launched
  const bool unsupported =
      C % 32 || (pcm ? (fmt != 0 || N != 1 || pre != PRE_NONE) :
                 (N % 32 || (epi == EPI_CONVTR && c->cout % 32) || (pre == PRE_LNFOLD && (fmt != 0 || ntaps != 1)) ||
                  (epi == EPI_QKV && (fmt != 0 || c->yf8 || c->yraw || c->act != ACT_NONE)) ||
                  (epi == EPI_RES && (c->yraw || (c->ls && fmt != 0) || (c->yf8 && fmt == 0))) ||  // gemm_h's RES / CONVTR store bf16 only
                  (epi == EPI_CONVTR && c->yf8 && fmt == 0)));
  if (unsupported) return 1;

  const int MT = cdiv(M, 16), CB = C / 32;
  const int rows_in = 16 * cdiv(M + ntaps, 16);  // rows past the end of x (halo < ntaps - 1) read zeros
  const long half = (long)rows_in * C;           // elements per parity half
  const int esz = fmt == 0 ? 2 : 1;
  void *xbuf = nullptr;
  CHK(dalloc(&scr, &xbuf, 2 * half * esz));
  const float inv_xs = fmt == 1 ? 1.0f / c->xs : 1.f;
  const long nq = (long)rows_in * (C / 4);
  dbg_to_codec_kernel<<<cdiv(nq, 256), 256, 0, st>>>(c->x, (char *)xbuf + (size_t)c->par * half * esz, c->x_eff, M, C, rows_in, fmt, inv_xs, c->xs);
  dbg_to_codec_kernel<<<cdiv(nq, 256), 256, 0, st>>>(c->x_prev, (char *)xbuf + (size_t)(c->par ^ 1) * half * esz, c->xp_eff, M, C, rows_in, fmt,
                                                     inv_xs, c->xs);
  int *dpar = nullptr;
  CHK(dallocT(&scr, &dpar, 1));
  HIPCHK(hipMemcpyAsync(dpar, &c->par, 4, hipMemcpyHostToDevice, st));

  // outputs: NaN-filled (bf16 0x7fc0, e4m3 0x7f, f32 quiet NaN), each followed by a guard
  std::vector<const void *> guards;
  auto out_buf = [&](size_t elems, int bytes_per, void **p) -> int {
    const size_t main = (elems * bytes_per + 255) / 256 * 256;
    CHK(dalloc(&scr, p, main + kDbgGuardFloats * 4));
    if (bytes_per == 4) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)*p, (int)kDbgUnwritten, main / 4, st));
    else if (bytes_per == 2) HIPCHK(hipMemsetD16Async((hipDeviceptr_t)*p, 0x7fc0, main / 2, st));
    else HIPCHK(hipMemsetD8Async((hipDeviceptr_t)*p, 0x7f, main, st));
    unsigned *g = (unsigned *)((char *)*p + main);
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)g, (int)kDbgGuard, kDbgGuardFloats, st));
    guards.push_back(g);
    return 0;
  };

  GemmArgs a;
  memset(&a, 0, sizeof(a));
  std::string label;
  Lin L;
  if (pcm) {
    a.M = M; a.MT = MT; a.CF = CB; a.XF = CB; a.ntaps = ntaps; a.T = c->T; a.halo = c->halo;
    a.X = (const float *)xbuf; a.Xdstride = half; a.par = dpar; a.epi = EPI_PCM;
    void *py = nullptr, *pi = nullptr;
    CHK(out_buf(M, 4, &py));
    CHK(out_buf(M, 2, &pi));
    a.pcm = (float *)py;
    a.pcm_i16 = (int16_t *)pi;
    label = "pcm_conv_h";
    {
      ProfScope ps(st, label, 2.0 * M * C + 4.0 * M, 2.0 * M * C * ntaps);
      pcm_conv_h_kernel<<<cdiv(M, 256), 256, 0, st>>>(a, c->w, c->bias);
    }
    LAUNCHCHK();
    c->cfg_used = 0;
    HIPCHK(hipMemcpyAsync(c->y, py, (size_t)M * 4, hipMemcpyDeviceToDevice, st));
    if (c->y_i16) {
      std::vector<int16_t> h(M);
      HIPCHK(hipMemcpyAsync(h.data(), pi, (size_t)M * 2, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      std::vector<float> f(h.begin(), h.end());
      HIPCHK(hipMemcpyAsync(c->y_i16, f.data(), (size_t)M * 4, hipMemcpyHostToDevice, st));
      HIPCHK(hipStreamSynchronize(st));
    }
  } else {
    // pack with the engine's own code: a scratch engine whose tensor map holds the case's operands.  pack_lin builds the
    // fp32 image as production does; here (as in production) it is only the source of the padded bias and of the
    // LayerNorm fold's ln_c: the codec kernels read pack_lin_h's bf16 image or pack_weight_f8's e4m3 one
    const int nb = epi == EPI_CONVTR || c->mode == 1 ? c->cout : N;
    const ptts_tensor tw{"w", c->w, (int64_t)N * C * ntaps}, tb{"b", c->bias, nb}, tg{"ln_w", c->ln_w, C}, tbe{"ln_b", c->ln_b, C};
    scr.tmap["w"] = &tw;
    if (c->bias) scr.tmap["b"] = &tb;
    const bool fold = pre == PRE_LNFOLD;
    if (fold) { scr.tmap["ln_w"] = &tg; scr.tmap["ln_b"] = &tbe; }
    CHK(pack_lin(&scr, &L, {{"w", c->bias ? "b" : "", N}}, C, ntaps, c->mode, c->cout, c->stride, fold ? "ln_w" : "", fold ? "ln_b" : ""));
    const int KBt = CB * ntaps;
    if (fmt == 0) {
      CHK(pack_lin_h(&scr, &L, "w", N, C, ntaps, c->mode, c->cout, c->stride, fold ? "ln_w" : ""));
    } else {
      CHK(dalloc(&scr, &L.wf8, (size_t)L.NT * KBt * 512));
      CHK(dallocT(&scr, &L.wscale8, (size_t)L.NT * 16));
      pack_weight_f8(st, c->w, L.wf8, L.wscale8, N, C, ntaps, c->mode, c->cout, c->stride);
    }
    LAUNCHCHK();
    a = mk_gemm(L, (const float *)xbuf, CB, MT, M);
    a.ntaps = ntaps; a.T = ntaps > 1 ? c->T : 16; a.halo = c->halo; a.Xdstride = half; a.par = dpar;
    a.epi = epi; a.act = c->act;
    const int YF = (epi == EPI_CONVTR ? c->cout : N) / 32;
    const long yrows = epi == EPI_CONVTR ? (long)MT * 16 * c->stride : (long)MT * 16, yrows_out = epi == EPI_CONVTR ? (long)M * c->stride : M;
    void *y = nullptr, *yraw = nullptr;
    float *Q = nullptr, *Kc = nullptr, *Vc = nullptr, *rope = nullptr, *tmp = nullptr;
    int *doff = nullptr;
    const int B = epi == EPI_QKV ? M / c->Tq : 0, QB = epi == EPI_QKV ? cdiv(c->Tq, 16) : 0;
    if (epi == EPI_QKV) {
      const size_t qn = (size_t)B * c->H * QB * 4 * 64 * 4, kn = (size_t)B * c->H * c->cap * 64;
      CHK(out_buf(qn, 4, (void **)&Q));
      CHK(out_buf(kn, 4, (void **)&Kc));
      CHK(out_buf(kn, 4, (void **)&Vc));
      CHK(dallocT(&scr, &doff, (size_t)B));
      HIPCHK(hipMemcpyAsync(doff, c->offset, (size_t)B * 4, hipMemcpyHostToDevice, st));
      CHK(dallocT(&scr, &rope, (size_t)MT * 16 * 64));
      rope_table_kernel<<<cdiv(M * 32, 256), 256, 0, st>>>(doff, e->freq_mimi, rope, M, c->Tq);
      a.Q = Q; a.Kc = Kc; a.Vc = Vc; a.offset = doff; a.rope = rope;
      a.H = c->H; a.Tq = c->Tq; a.QB = QB; a.cap = c->cap; a.ring = c->ring;
    } else {
      CHK(out_buf((size_t)yrows * YF * 32, c->yf8 ? 1 : 2, &y));
      a.Y = (float *)y; a.YF = YF;
      a.yf8 = c->yf8; a.yinv = c->yf8 ? c->yinv : 1.0f;
      if (c->yraw) { CHK(out_buf((size_t)yrows * YF * 32, 2, &yraw)); a.Yraw = (float *)yraw; }
      if (epi == EPI_CONVTR) { a.cout = c->cout; a.stride = c->stride; }
    }
    if (epi == EPI_RES) {
      CHK(dalloc(&scr, (void **)&tmp, (size_t)MT * 16 * N * 2));
      dbg_to_codec_kernel<<<cdiv((long)MT * 16 * (N / 4), 256), 256, 0, st>>>(c->r, tmp, nullptr, M, N, MT * 16, 0, 1.f, 1.f);
      a.R = tmp; a.RF = N / 32;
      if (c->ls) {
        float *ls = nullptr;
        CHK(dallocT(&scr, &ls, (size_t)L.NT * 16));
        HIPCHK(hipMemcpyAsync(ls, c->ls, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
        a.ls = ls;
      }
    }
    int cfg = c->cfg;
    if (fmt == 0) {
      a = gemm_h_args(a, pre, L);
      if (cfg < 0) cfg = choose_h_tile(a);
      launch_h_tile(st, a, pre, cfg, &label);
    } else {
      a.W = (const float *)L.wf8; a.wscale = L.wscale8; a.CF = CB; a.KF = KBt; a.swz = 0; a.xs = c->xs;
      if (cfg < 0) cfg = choose_f8_tile(a);
      launch_f8_tile(st, a, cfg, &label);
    }
    LAUNCHCHK();
    c->cfg_used = cfg;
    if (epi == EPI_QKV) {
      dbg_from_qkv_kernel<<<cdiv((long)M * N, 256), 256, 0, st>>>(Q, Kc, Vc, doff, c->y, M, c->H, c->Tq, QB, c->cap, c->ring);
      if (c->rope) HIPCHK(hipMemcpyAsync(c->rope, rope, (size_t)M * 64 * 4, hipMemcpyDeviceToDevice, st));
    } else {
      const int Nout = YF * 32;
      dbg_from_codec_kernel<<<cdiv(yrows_out * Nout, 256), 256, 0, st>>>(y, c->y, yrows_out, Nout, YF, c->yf8 ? 1 : 0);
      if (c->yraw) dbg_from_codec_kernel<<<cdiv(yrows_out * Nout, 256), 256, 0, st>>>(yraw, c->yraw, yrows_out, Nout, YF, 0);
    }
    const long nk = (long)N * KBt * 32;
    if (c->w_eff) dbg_unpack_codec_weight_kernel<<<cdiv(nk, 256), 256, 0, st>>>(fmt == 0 ? (const void *)L.wh : L.wf8, L.wscale8, fmt, c->w_eff, N, KBt);
    if (c->wscale && fmt == 1) HIPCHK(hipMemcpyAsync(c->wscale, L.wscale8, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
    if (fold && c->ln_s) HIPCHK(hipMemcpyAsync(c->ln_s, L.ln_s_h, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
    if (fold && c->ln_c) HIPCHK(hipMemcpyAsync(c->ln_c, L.ln_c, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
  }
  put_label(label, c->label, c->label_cap);
  return check_guards(scr, st, guards, kDbgGuardFloats, "debug_codec_gemm: " + label + " wrote past an output");
}

extern "C" int ptts_debug_codec_gemm(ptts_engine *e, ptts_codec_gemm_case *c, void *stream) {
  if (!e || !c) return fail(-1, "debug_codec_gemm: null argument");
  return run_case(e, stream, [&](hipStream_t st, ptts_engine &scr) { return debug_codec_gemm(e, c, st, scr); });
}

// ------------------------------------------------------------------------------------------------
// ptts_debug_read_encoder (test hook, include/ptts.h): the intermediates of the last ptts_encode_voice that ran with
// "debug_taps".  FM buffers, but for "tr_qkv": the last layer's query blocks and key / value caches
extern "C" int64_t ptts_debug_read_encoder(ptts_engine *e, const char *name, float *d_out, int64_t capacity, int32_t *rows,
                                           int32_t *cols, void *stream) {
  if (!e || !name || !d_out || !rows || !cols) return fail(-1, "debug_read_encoder: null argument");
  ENGINE_LOCK(e);
  HIPCHK(hipSetDevice(e->device));
  if (e->enc_taps.empty())
    return fail(-1, "debug_read_encoder: nothing kept; set the engine option \"debug_taps\" before ptts_encode_voice");
  hipStream_t st = S(e, stream);
  for (const ptts_engine::EncTap &t : e->enc_taps) {
    if (t.name != name) continue;
    const long n = (long)t.rows * t.cols;
    if (n > capacity) return fail(-1, "debug_read_encoder: capacity too small");
    if (t.H) dbg_from_qkv_kernel<<<cdiv(n, 256), 256, 0, st>>>(t.p, t.kc, t.vc, t.offset, d_out, t.rows, t.H, t.rows, t.QB, t.cap, 0);
    else from_fm_kernel<<<cdiv(n / 4, 256), 256, 0, st>>>(t.p, d_out, t.rows, t.cols, t.cols / 16, 0);
    LAUNCHCHK();
    *rows = t.rows;
    *cols = t.cols;
    return n;
  }
  return fail(-1, std::string("debug_read_encoder: unknown buffer ") + name);
}
