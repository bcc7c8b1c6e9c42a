// The Mimi codec's host side: the codec state, the frame walks, the hand-over ring's bookkeeping, the output chain behind
// the codec, the decode entry points, the voice-prompt encoder and the fp8 calibration run.
#include "ptts_host.h"
#include "ptts_stage.h"
#include "ptts_bf16.h"

#include <algorithm>

#define SITE(x) set_launch_site(x)

static int build_mimi_state(ptts_engine *e, ptts_mimi_state *s) {
  const ptts_config &c = e->cfg;
  const int B = s->B;
  AllocScope alloc_scope(e->stream);
  s->MTb = cdiv(B, 16);
  s->MT16 = B;  // one 16-row tile per sequence
  const int C = c.m_dim, CF = C / 16;
  CHK(dallocT(nullptr, &s->frame, 4));  // frame, trf, trl
  CHK(dallocT(nullptr, &s->offset, B));
  CHK(dallocT(nullptr, &s->kv, (size_t)c.m_layers * 2 * s->kv_plane()));
  CHK(dallocT(nullptr, &s->zl, (size_t)s->MTb * 256 * (c.ldim / 16)));
  // a ring's element size follows the codec format: the transformer hands over fp32 or bf16, SEANet's convs read fp32,
  // bf16 or (fp8 codec) e4m3, but for the last block's output, which feeds the bf16-input last conv
  const int e_tr = e->codec_bf16 ? 2 : 4, e_sn = e->codec_fp8 ? 1 : e_tr;
  auto ring = [&](Ring &r, int slots, long stride, int esz) {
    r.slots = slots; r.stride = stride; r.esz = esz;
    return dallocT(nullptr, &r.p, (size_t)slots * stride);
  };
  CHK(ring(s->zq, 2, (long)s->MTb * 256 * CF, 4));
  const size_t r16 = (size_t)s->MT16 * 256;
  // the transformer's buffers hold a frame pair (32 rows per sequence) on the fp32 codec, whose transformer takes pairs
  const bool pairs = !e->codec_bf16;
  const size_t r32 = pairs ? 2 * r16 : r16;
  CHK(dallocT(nullptr, &s->u0, r32 * CF));
  CHK(dallocT(nullptr, &s->u, r32 * CF));
  CHK(dallocT(nullptr, &s->h, r32 * CF));
  CHK(dallocT(nullptr, &s->ao, r32 * CF));
  CHK(dallocT(nullptr, &s->ff, r32 * (c.m_ff / 16)));
  CHK(dallocT(nullptr, &s->q, (size_t)B * c.m_heads * 4 * 256 * (pairs ? 2 : 1)));
  CHK(dallocT(nullptr, &s->rope, (size_t)B * 16 * 64 * (pairs ? 2 : 1)));
  // key tiles a 16-query block attends at most: the context in whole frames plus its own (the ring holds one frame more)
  s->splits = attn_splits(B * c.m_heads, e->ring / 16 - 1);
  s->splits2 = attn_splits(B * c.m_heads * 2, e->ring / 16 - 1);
  CHK(dallocT(nullptr, &s->part, (size_t)B * c.m_heads * std::max(s->splits, pairs ? 2 * s->splits2 : 0) * 16 * ATT_PSTRIDE));
  CHK(ring(s->tr_out, pairs ? 4 : 2, (long)r16 * CF, e_tr));
  int mult = 8, rows = 16;
  s->rows[0] = rows;
  CHK(ring(s->a0, 2, (long)r16 * (mult * c.n_filters / 16), e_sn));
  for (int i = 0; i < 3; ++i) {
    const int cout = mult * c.n_filters / 2, hid = cout / c.compress;
    rows *= c.ratios[i];
    s->rows[i + 1] = rows;
    const size_t rt = (size_t)B * (rows / 16) * 256;
    CHK(ring(s->cbuf[i], 2, (long)rt * (cout / 16), e_sn));
    CHK(dallocT(nullptr, &s->craw[i], rt * (cout / 16)));
    CHK(ring(s->sbuf[i], 2, (long)rt * (cout / 16), i == 2 ? e_tr : e_sn));
    CHK(dallocT(nullptr, &s->rbuf[i], rt * (hid / 16)));
    mult /= 2;
  }
  CHK(dallocT(nullptr, &s->pcm_dbg, (size_t)B * rows));
  CHK(dallocT(nullptr, &s->pcm_part, (size_t)B * rows));
  CHK(ring(s->pcm_carry, 2, (long)cdiv(B * rows, 64) * 2, 4));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

extern "C" int ptts_mimi_state_create(ptts_engine *e, int32_t B, ptts_mimi_state **out) {
  if (!e || !out || B < 1) return fail(-1, "bad argument");
  ENGINE_LOCK(e);
  HIPCHK(hipSetDevice(e->device));
  ptts_mimi_state *s = new ptts_mimi_state();
  s->e = e;
  s->B = B;
  const int rc = build_mimi_state(e, s);
  if (rc < 0) {
    const std::string msg = ptts_last_error();
    ptts_mimi_state_destroy(s);
    return fail(rc, msg);
  }
  *out = s;
  return 0;
}

extern "C" void ptts_mimi_state_destroy(ptts_mimi_state *s) {
  if (!s) return;
  hipSetDevice(s->e->device);
  hipDeviceSynchronize();
  hipFree(s->frame); hipFree(s->offset); hipFree(s->kv); hipFree(s->zl); hipFree(s->u0);
  hipFree(s->u); hipFree(s->h); hipFree(s->ao); hipFree(s->ff); hipFree(s->q); hipFree(s->part);
  hipFree(s->pcm_dbg); hipFree(s->pcm_part); hipFree(s->rope); hipFree(s->tap_tr);
  for (const Ring *r : s->rings()) hipFree(r->p);
  for (int i = 0; i < 3; ++i) { hipFree(s->craw[i]); hipFree(s->rbuf[i]); }
  delete s;
}

extern "C" int ptts_mimi_state_reset(ptts_mimi_state *s, void *stream) {
  hipStream_t st = S(s->e, stream);
  // zero-initialised carries == `previous` / `partial` zeros of init_state (conv.py:84-91,145-149)
  HIPCHK(hipMemsetAsync(s->frame, 0, 4 * sizeof(int), st));
  HIPCHK(hipMemsetAsync(s->offset, 0, s->B * sizeof(int), st));
  for (const Ring *r : s->rings()) HIPCHK(hipMemsetAsync(r->p, 0, (size_t)r->slots * r->stride * sizeof(float), st));  // the whole allocation
  HIPCHK(hipMemsetAsync(s->kv, 0, (size_t)s->e->cfg.m_layers * 2 * s->kv_plane() * 4, st));
  s->h_frame = s->h_tr = 0;
  return 0;
}

// Continuous batching: zero the streaming carries of ONE sequence (a new utterance joins in `row`): the
// previous-frame buffers its first frame will read as halo, and its position in the decoder transformer.
extern "C" int ptts_mimi_state_reset_row(ptts_mimi_state *s, int32_t row, void *stream) {
  if (!s || row < 0 || row >= s->B) return fail(-1, "reset_row: row out of range");
  hipStream_t st = S(s->e, stream);
  const int CF = s->e->cfg.m_dim / 16;
  set_int_kernel<<<1, 64, 0, st>>>(s->offset + row, 1, 0);
  // A sequence owns whole 16-row tiles, i.e. one contiguous block of every slot of every ring, the row-th of B.  Two rings
  // differ: 16 sequences share a tile of zq, which zero_row_fm_kernel clears, and a sequence owns whole 64-row tiles of
  // pcm_carry (the row's tile carries) only when rows[3] % 64 == 0
  for (const Ring *r : s->rings()) {
    if (r == &s->pcm_carry && s->rows[3] % 64 != 0) continue;
    for (int k = 0; k < r->slots; ++k) {
      if (r == &s->zq) { zero_row_fm_kernel<<<cdiv(CF * 16, 256), 256, 0, st>>>(r->slot(k), CF, row); continue; }
      const size_t per_seq = r->bytes() / s->B;
      HIPCHK(hipMemsetAsync((char *)r->slot(k) + row * per_seq, 0, per_seq, st));
    }
  }
  LAUNCHCHK();
  return 0;
}

// Optional 16-bit PCM output of the codec's last kernel (device or pinned host memory, [B, frame_samples]);
// applies to the decodes / graph captures issued after the call.  NULL switches it off.
extern "C" int ptts_mimi_set_pcm_i16(ptts_mimi_state *s, int16_t *d_pcm_i16) {
  if (!s) return fail(-1, "null state");
  s->pcm_i16 = d_pcm_i16;
  return 0;
}

static const char *const kSeanetSite[3][3] = {{"seanet.convtr1", "seanet.res1a", "seanet.res1b"},
                                              {"seanet.convtr2", "seanet.res2a", "seanet.res2b"},
                                              {"seanet.convtr3", "seanet.res3a", "seanet.res3b"}};

// SEANet stage i's residual block runs as one launch
bool resblock_fused(const ptts_mimi_state *s, int i) {
  const ptts_engine *e = s->e;
  const int MTout = s->B * s->rows[i + 1] / 16;
  return e->opt_fuse_res && resblock_fusable(e->res_a[i], e->res_b[i], MTout) && (long)MTout * 16 >= e->fuse_res_min_rows;
}
bool seanet_single_store(const ptts_engine *e, int i) {
  return e->opt_single_store && !e->codec_split && !e->res_a[i].wq && !e->res_a[i].wb16;
}
bool seanet_fuses_pcm(const ptts_mimi_state *s) {
  const ptts_engine *e = s->e;
  const Lin &CL = e->conv_last;
  const int Tout = s->rows[3], MTout = s->B * Tout / 16;
  return !e->codec_bf16 && resblock_fused(s, 2) && e->opt_fuse_pcm && e->res_a[2].NT == 2 && Tout % 64 == 0 && MTout % 4 == 0 &&
         e->cfg.n_filters == 64 /* the last stage's cout */ && CL.ntaps == 3 && CL.NT == 1 && !CL.wq && !CL.wb16 && !e->codec_split && s->pcm_carry.p;
}

// the bookkeeping launch that ends a part: positions advance by `rows`, the frame counters by `tr_frames` and `seanet`
static void mimi_tail(hipStream_t st, const ptts_mimi_state *s, int rows, int tr_frames, int seanet) {
  SITE("mimi.tail");
  ProfScope ps(st, "step_tail", 8.0 * s->B, 0);
  mimi_tail_kernel<<<cdiv(s->B, 256), 256, 0, st>>>(s->offset, s->B, rows, s->frame, tr_frames, seanet);
}

// "debug_taps": a transformer of two or more layers overwrites u, ao, ff and q layer by layer; ptts_debug_read reaches the
// earlier layers' through copies (ptts_mimi_state::tr_tap).  The buffer exists only after an eager decode with the option
// (ensure_tr_taps): without it nothing is allocated or enqueued
static int ensure_tr_taps(ptts_engine *e, ptts_mimi_state *s) {
  const ptts_config &c = e->cfg;
  if (!e->opt_debug_taps || s->tap_tr || c.m_layers < 2) return 0;
  AllocScope alloc_scope(e->stream);
  const size_t pair = e->codec_bf16 ? 1 : 2;  // as build_mimi_state sizes u, ff and q
  s->tap_nu = (size_t)s->MT16 * 256 * pair * (c.m_dim / 16);
  s->tap_nff = (size_t)s->MT16 * 256 * pair * (c.m_ff / 16);
  s->tap_nq = (size_t)s->B * c.m_heads * 4 * 256 * pair;
  s->tap_stride = 3 * s->tap_nu + s->tap_nff + s->tap_nq;
  CHK(dallocT(nullptr, &s->tap_tr, (size_t)(c.m_layers - 1) * s->tap_stride));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}
static bool tr_taps_on(const ptts_engine *e, const ptts_mimi_state *s) { return e->opt_debug_taps && s->tap_tr; }
static int tap_copy(hipStream_t st, float *dst, const float *src, size_t n) {
  HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st));
  return 0;
}
// before layer l >= 1 reads u
static int tap_layer_input(hipStream_t st, ptts_engine *e, ptts_mimi_state *s, int l) {
  if (l < 1 || !tr_taps_on(e, s)) return 0;
  s->tap_frame = s->h_tr;  // host stamp of an eager enqueue: a replayed graph does not renew it, its copies are refused
  return tap_copy(st, s->tr_tap(l).in, s->u, s->tap_nu);
}
// after the last launch of layer l < layers - 1 (its stream after attention is copied before linear2 overwrites it)
static int tap_layer_end(hipStream_t st, ptts_engine *e, ptts_mimi_state *s, int l) {
  if (l >= e->cfg.m_layers - 1 || !tr_taps_on(e, s)) return 0;
  const ptts_mimi_state::TrTap t = s->tr_tap(l + 1);
  CHK(tap_copy(st, t.ao, s->ao, s->tap_nu));
  CHK(tap_copy(st, t.ff, s->ff, s->tap_nff));
  return tap_copy(st, t.q, s->q, s->tap_nq);
}

// the codec frame with bf16 activations: same dataflow, buffers and carries as mimi_enqueue (the fp32 buffers are
// reused, half filled); block counts are per 32 channels
// parts: 1 = the transformer, 2 = SEANet, 3 = the whole frame (mimi_enqueue); single frames, tr_out's two parity halves
static int mimi_enqueue_h(hipStream_t st, ptts_engine *e, ptts_mimi_state *s, const float *d_latent, float *d_pcm, int parts = 3) {
  const ptts_config &c = e->cfg;
  bind_engine(e);
  KnobScope knobs(e->opt_codec_lds_target, e->opt_k_rotate);
  const int B = s->B, C = c.m_dim, CB = C / 32, st16 = c.upsample_stride;
  const int M16 = B * st16, MT16 = s->MT16;
  GemmArgs a;
  if (parts & 1) {
  SITE("mimi.prologue");
  {
    ProfScope ps(st, "mimi_prologue", 4.0 * (B * c.ldim + (double)C * c.ldim) + B * C * (8.0 + 2.0 * st16), 2.0 * B * C * (c.ldim + 2.0 * st16));
    const int nb_main = cdiv((long)B * (C / 4) * st16, 256);
    mimi_prologue_kernel<<<nb_main + cdiv(B * st16 * 32, 256), 256, 0, st>>>(
        d_latent, nullptr, e->emb_std, e->emb_mean, e->quant_w, e->up_w, s->zq.p, s->zq.step(), s->trl(), s->u0, B, c.ldim, C,
        st16, nb_main, RopeArgs{s->offset, e->freq_mimi, s->rope, B * st16, st16}, 1);
  }
  for (int l = 0; l < c.m_layers; ++l) {
    const TrLayer &T = e->mm[l];
    float *x_in = l == 0 ? s->u0 : s->u;
    const bool last = l == c.m_layers - 1;
    CHK(tap_layer_input(st, e, s, l));
    SITE("mimi.qkv");
    a = mk_gemm(T.qkv, x_in, CB, MT16, M16);
    a.epi = EPI_QKV;
    a.Q = s->q; a.Kc = s->K(l); a.Vc = s->V(l); a.offset = s->offset; a.rope = s->rope;
    a.H = c.m_heads; a.Tq = st16; a.QB = 1; a.cap = e->ring; a.ring = e->ring;
    launch_gemm_h(st, a, PRE_LNFOLD, T.qkv);
    AttnArgs at;
    at.Q = s->q; at.Kc = s->K(l); at.Vc = s->V(l); at.offset = s->offset; at.H = c.m_heads; at.Tq = st16; at.QB = 1;
    at.cap = e->ring; at.ring = e->ring; at.ctx = c.m_context; at.splits = s->splits; at.part = s->part; at.Y = s->ao; at.YF = CB;
    at.h16 = 1;
    const int BH = B * c.m_heads;
    at.nseq = B;
    SITE("mimi.attn");
    {
      const double keys = (double)B * std::min(e->ring, (s->h_tr + 1) * st16);
      launch_attention(st, at, BH, 0, -1, keys * c.m_heads * 64 * 4 * 2 + 6.0 * M16 * C, 4.0 * keys * c.m_heads * 64 * 16);
    }
    SITE("mimi.out");
    a = mk_gemm(T.out, s->ao, CB, MT16, M16);
    a.epi = EPI_RES; a.R = x_in; a.RF = CB; a.Y = s->u; a.YF = CB; a.ls = T.ls1;
    launch_gemm_h(st, a, PRE_NONE, T.out);
    if (!last && tr_taps_on(e, s)) CHK(tap_copy(st, s->tr_tap(l + 1).resid, s->u, s->tap_nu));
    SITE("mimi.ff1");
    a = mk_gemm(T.ff1, s->u, CB, MT16, M16);
    a.epi = EPI_STORE; a.act = ACT_GELU; a.Y = s->ff; a.YF = c.m_ff / 32;
    launch_gemm_h(st, a, PRE_LNFOLD, T.ff1);
    SITE("mimi.ff2");
    a = mk_gemm(T.ff2, s->ff, c.m_ff / 32, MT16, M16);
    a.epi = EPI_RES; a.R = s->u; a.RF = CB; a.ls = T.ls2;
    a.Y = last ? s->tr_out.p : s->u; a.YF = CB; a.Ydstride = last ? s->tr_out.step() : 0; a.par = last ? s->trf() : nullptr;
    launch_gemm_h(st, a, PRE_NONE, T.ff2);
    CHK(tap_layer_end(st, e, s, l));
  }
  if (parts == 1) mimi_tail(st, s, st16, 1, 0);
  }
  if (!(parts & 2)) { SITE(""); return 0; }
  // the rings hold bf16 or, for the inputs of the fp8 convolutions, e4m3 bytes (Ring::step)
  const bool f8 = e->codec_fp8;
  const float *f8s = e->f8s;
  // fp8 conv: operand images, scales and output format (sc_in / sc_out index e->f8s; sc_out < 0: bf16 output)
  auto f8_conv = [&](GemmArgs &g, const Lin &L, int sc_in, int sc_out) {
    g.W = (const float *)L.wf8;
    g.wscale = L.wscale8;
    g.CF = L.C / 32;
    g.KF = g.CF * L.ntaps;
    g.swz = 0;
    g.xs = f8s[sc_in];
    g.yf8 = sc_out >= 0;
    g.yinv = sc_out >= 0 ? 1.0f / f8s[sc_out] : 1.0f;
    launch_f8_tile(st, g, choose_f8_tile(g));
  };
  int mult = 8;
  SITE("seanet.conv0");
  a = mk_gemm(e->conv0, s->tr_out.p, CB, MT16, M16);
  a.Xdstride = s->tr_out.step(); a.T = s->rows[0]; a.par = s->frame;
  a.Y = s->a0.p; a.Ydstride = s->a0.step(); a.YF = mult * c.n_filters / 32; a.act = ACT_ELU;
  if (f8) { a.yf8 = 1; a.yinv = 1.0f / f8s[0]; }  // bf16 in (the transformer's output), e4m3 out
  launch_gemm_h(st, a, PRE_NONE, e->conv0);
  const Ring *xin = &s->a0;
  for (int i = 0; i < 3; ++i) {
    const int cin = mult * c.n_filters, cout = cin / 2, hid = cout / c.compress;
    const int Tin = s->rows[i], Tout = s->rows[i + 1];
    const int MTin = B * Tin / 16, MTout = B * Tout / 16;
    SITE(kSeanetSite[i][0]);
    a = mk_gemm(e->convtr[i], xin->p, cin / 32, MTin, B * Tin);
    a.Xdstride = xin->step(); a.T = Tin; a.par = s->frame;
    a.epi = EPI_CONVTR; a.cout = cout; a.stride = c.ratios[i];
    a.Y = s->cbuf[i].p; a.Ydstride = s->cbuf[i].step(); a.YF = cout / 32; a.act = ACT_ELU;
    a.Yraw = s->craw[i]; a.Yrawdstride = 0;
    if (f8) f8_conv(a, e->convtr[i], i == 0 ? 0 : 3 * i, 1 + 3 * i);
    else launch_gemm_h(st, a, PRE_NONE, e->convtr[i]);
    SITE(kSeanetSite[i][1]);
    a = mk_gemm(e->res_a[i], s->cbuf[i].p, cout / 32, MTout, B * Tout);
    a.Xdstride = s->cbuf[i].step(); a.T = Tout; a.par = s->frame;
    a.Y = s->rbuf[i]; a.YF = hid / 32; a.act = ACT_ELU;
    if (f8) f8_conv(a, e->res_a[i], 1 + 3 * i, 2 + 3 * i);
    else launch_gemm_h(st, a, PRE_NONE, e->res_a[i]);
    SITE(kSeanetSite[i][2]);
    a = mk_gemm(e->res_b[i], s->rbuf[i], hid / 32, MTout, B * Tout);
    a.T = Tout; a.par = s->frame;
    a.epi = EPI_RES; a.R = s->craw[i]; a.Rdstride = 0; a.RF = cout / 32; a.act = ACT_ELU;
    a.Y = s->sbuf[i].p; a.Ydstride = s->sbuf[i].step(); a.YF = cout / 32;
    if (f8) f8_conv(a, e->res_b[i], 2 + 3 * i, i == 2 ? -1 : 3 + 3 * i);  // the last block's output feeds the (bf16-input) last conv
    else launch_gemm_h(st, a, PRE_NONE, e->res_b[i]);
    xin = &s->sbuf[i];
    mult /= 2;
  }
  const int Tl = s->rows[3];
  SITE("seanet.conv_last");
  a = mk_gemm(e->conv_last, xin->p, c.n_filters / 32, B * Tl / 16, B * Tl);
  a.CF = c.n_filters / 32;
  a.Xdstride = xin->step(); a.T = Tl; a.par = s->frame;
  a.epi = EPI_PCM; a.pcm = d_pcm ? d_pcm : s->pcm_dbg; a.pcm_i16 = s->pcm_i16;
  {
    ProfScope ps(st, "pcm_conv_h", 2.0 * a.M * c.n_filters + 4.0 * a.M, 2.0 * a.M * c.n_filters * c.last_kernel_size);
    pcm_conv_h_kernel<<<cdiv(a.M, 256), 256, 0, st>>>(a, e->conv_last_w, e->conv_last_b);
  }
  mimi_tail(st, s, st16, parts == 3 ? 1 : 0, 1);
  SITE("");
  return 0;
}

// The codec frame of the fp32 codec in two parts that meet in tr_out, a ring of 4 frame slots (frame f in slot f & 3):
// the transformer part, for one frame or for a PAIR of consecutive frames in one launch sequence (rows b * 32 + t, the
// T-general path of the prefills: twice the rows per GEMM, half the launches and weight reads per frame), and the SEANet
// part, always one frame.  `tail`: the part ends with its own bookkeeping launch; the whole frame (mimi_enqueue) leaves
// both parts' bookkeeping to ONE launch at its end, as before the split.
static int mimi_tr_enqueue(hipStream_t st, ptts_engine *e, ptts_mimi_state *s, const float *d_latent, const float *d_latent2,
                           bool tail) {
  const ptts_config &c = e->cfg;
  bind_engine(e);
  KnobScope knobs(e->opt_codec_lds_target, e->opt_k_rotate, e->codec_split);
  const int frames = d_latent2 ? 2 : 1;
  const int B = s->B, C = c.m_dim, st16 = c.upsample_stride, Tq = st16 * frames;
  SITE("mimi.prologue");  // de-normalise + quantizer 1x1 conv + depthwise x16 upsample + RoPE table: one launch
  {
    ProfScope ps(st, "mimi_prologue", 4.0 * (frames * B * c.ldim + (double)C * c.ldim + frames * B * C * (2.0 + st16)),
                 2.0 * frames * B * C * (c.ldim + 2.0 * st16));
    const int nb_main = cdiv((long)B * (C / 4) * Tq, 256);
    mimi_prologue_kernel<<<nb_main + cdiv(B * Tq * 32, 256), 256, 0, st>>>(
        d_latent, d_latent2, e->emb_std, e->emb_mean, e->quant_w, e->up_w, s->zq.p, s->zq.step(), s->trl(), s->u0, B, c.ldim, C,
        st16, nb_main, RopeArgs{s->offset, e->freq_mimi, s->rope, B * Tq, Tq}, 0);
  }
  const int M = B * Tq;
  for (int l = 0; l < c.m_layers; ++l) {
    TrCtx t;
    t.D = C; t.H = c.m_heads; t.FF = c.m_ff; t.MT = s->MT16 * frames; t.M = M; t.Tq = Tq; t.QB = frames;
    t.cap = e->ring; t.ring = e->ring; t.ctx = c.m_context; t.splits = frames == 2 ? s->splits2 : s->splits;
    t.x_in = l == 0 ? s->u0 : s->u; t.x = s->u;
    const bool last = l == c.m_layers - 1;
    t.x_out = last ? s->tr_out.p : s->u; t.out_ds = last ? s->tr_out.step() : 0; t.par = last ? s->trf() : nullptr;
    t.out_ring = last ? frames : 0;
    t.h = s->h; t.ao = s->ao; t.ff = s->ff; t.q = s->q; t.part = s->part;
    t.Kc = s->K(l); t.Vc = s->V(l); t.offset = s->offset; t.rope = s->rope;
    t.kv_keys = (double)B * std::min(e->ring, (s->h_tr + frames) * st16);
    t.tag = "mimi";
    CHK(tap_layer_input(st, e, s, l));
    if (!last && tr_taps_on(e, s)) t.tap_x = s->tr_tap(l + 1).resid;
    run_tr_layer(st, e->mm[l], t);
    CHK(tap_layer_end(st, e, s, l));
  }
  if (tail) mimi_tail(st, s, Tq, frames, 0);
  SITE("");
  return 0;
}

// `tail`: 1 = the part's own bookkeeping, 2 = a whole frame's (the transformer's single frame before it included)
static int mimi_seanet_enqueue(hipStream_t st, ptts_engine *e, ptts_mimi_state *s, float *d_pcm, int tail) {
  const ptts_config &c = e->cfg;
  bind_engine(e);
  KnobScope knobs(e->opt_codec_lds_target, e->opt_k_rotate, e->codec_split);
  const int B = s->B, C = c.m_dim, CF = C / 16, st16 = c.upsample_stride;
  GemmArgs a;
  const int M16 = B * st16;
  // SEANet decoder (seanet.py:141-180) as implicit GEMMs over (sequence, time) rows
  int mult = 8;
  const bool fused_pcm = seanet_fuses_pcm(s);
  SITE("seanet.conv0");
  a = mk_gemm(e->conv0, s->tr_out.p, CF, s->MT16, M16);
  a.Xdstride = s->tr_out.step(); a.T = s->rows[0]; a.par = s->frame; a.xmask = 3;  // frame f and its halo f - 1 in the hand-over ring
  a.Y = s->a0.p; a.Ydstride = s->a0.step(); a.YF = mult * c.n_filters / 16;
  a.act = ACT_ELU;  // every SEANet conv input is ELU(previous output): apply it once, in the producer
  launch_gemm(st, a, PRE_NONE);
  const Ring *xin = &s->a0;
  for (int i = 0; i < 3; ++i) {
    const int cin = mult * c.n_filters, cout = cin / 2, hid = cout / c.compress;
    const int Tin = s->rows[i], Tout = s->rows[i + 1];
    const int MTin = B * Tin / 16, MTout = B * Tout / 16;
    SITE(kSeanetSite[i][0]);
    a = mk_gemm(e->convtr[i], xin->p, cin / 16, MTin, B * Tin);
    a.Xdstride = xin->step(); a.T = Tin; a.par = s->frame;
    a.epi = EPI_CONVTR; a.cout = cout; a.stride = c.ratios[i];
    a.Y = s->cbuf[i].p; a.Ydstride = s->cbuf[i].step(); a.YF = cout / 16; a.act = ACT_ELU;
    a.Yraw = s->craw[i]; a.Yrawdstride = 0;  // raw value = the resnet block's skip input
    // "single_store": the transposed conv stores its RAW output once (the block's skip input); the k3 conv that follows
    // applies ELU to its operand fragments as it reads them (PRE_ELU).  Saves one write and one read of every stage output
    // (107 MB per 64-sequence frame): +1.x % pipelined; fp32 weights only
    const bool single = seanet_single_store(e, i);
    const int pre_a = single ? PRE_ELU : PRE_NONE;
    if (single) { a.act = ACT_NONE; a.Yraw = nullptr; }
    launch_gemm(st, a, PRE_NONE);
    if (resblock_fused(s, i)) {
      SITE(kSeanetSite[i][1]);
      a = mk_gemm(e->res_a[i], s->cbuf[i].p, cout / 16, MTout, B * Tout);
      a.Xdstride = s->cbuf[i].step(); a.T = Tout; a.par = s->frame; a.act = ACT_ELU;
      a.R = s->craw[i]; a.Rdstride = 0; a.RF = cout / 16; a.act2 = ACT_ELU;
      if (single) { a.R = s->cbuf[i].p; a.Rdstride = s->cbuf[i].step(); }
      a.Y = s->sbuf[i].p; a.Ydstride = s->sbuf[i].step(); a.YF = cout / 16;
      // a split-bf16 engine keeps the FUSED fp32 residual blocks: the unfused split pair is slower (stage 3: 34 + 35 us
      // against 43 us fused, stage 2: 25 + 21 against 32; gpurun_out r3 profile), the block is bound by its activations
      a.W = e->res_a[i].w; a.Wq = nullptr; a.wfmt = 0;
      // last stage: SEANet's final conv (k = 3, n_filters -> 1 sample) rides in the block's epilogue: the block's output
      // (31 MB per 64-sequence frame, written and read back by a separate conv before) never leaves the CU
      if (i == 2 && fused_pcm) {
        a.pcm_w = e->conv_last.w; a.pcm_part = s->pcm_part; a.pcm_carry = s->pcm_carry.p; a.pcm_cstride = s->pcm_carry.step();
        if (!e->opt_debug_taps) a.Y = nullptr;
      }
      launch_resblock(st, a, e->res_b[i], pre_a);
      xin = &s->sbuf[i];
      mult /= 2;
      continue;
    }
    SITE(kSeanetSite[i][1]);
    a = mk_gemm(e->res_a[i], s->cbuf[i].p, cout / 16, MTout, B * Tout);
    a.Xdstride = s->cbuf[i].step(); a.T = Tout; a.par = s->frame;
    a.Y = s->rbuf[i]; a.YF = hid / 16; a.act = ACT_ELU;
    launch_gemm(st, a, pre_a);
    SITE(kSeanetSite[i][2]);
    a = mk_gemm(e->res_b[i], s->rbuf[i], hid / 16, MTout, B * Tout);
    a.T = Tout; a.par = s->frame;
    a.epi = EPI_RES; a.R = s->craw[i]; a.Rdstride = 0; a.RF = cout / 16; a.act = ACT_ELU;
    if (single) { a.R = s->cbuf[i].p; a.Rdstride = s->cbuf[i].step(); }
    a.Y = s->sbuf[i].p; a.Ydstride = s->sbuf[i].step(); a.YF = cout / 16;
    launch_gemm(st, a, PRE_NONE);
    xin = &s->sbuf[i];
    mult /= 2;
  }
  const int Tl = s->rows[3];
  SITE("seanet.conv_last");
  if (fused_pcm) {
    ProfScope ps(st, "pcm_fix", 4.0 * (2.0 * B * Tl + B * Tl / 32.0), 0);
    pcm_fix_kernel<<<cdiv(B * Tl, 256), 256, 0, st>>>(s->pcm_part, s->pcm_carry.p, s->pcm_carry.step(), s->frame, e->conv_last.bias,
                                                      d_pcm ? d_pcm : s->pcm_dbg, s->pcm_i16, B * Tl, Tl / 64);
  } else {
    a = mk_gemm(e->conv_last, xin->p, c.n_filters / 16, B * Tl / 16, B * Tl);
    a.Xdstride = xin->step(); a.T = Tl; a.par = s->frame;
    a.epi = EPI_PCM; a.pcm = d_pcm ? d_pcm : s->pcm_dbg; a.pcm_i16 = s->pcm_i16;
    launch_gemm(st, a, PRE_NONE);
  }
  mimi_tail(st, s, st16, tail == 2 ? 1 : 0, 1);
  SITE("");
  return 0;
}

static int mimi_enqueue(hipStream_t st, ptts_engine *e, ptts_mimi_state *s, const float *d_latent, const float *d_latent2,
                        float *d_pcm, int parts) {
  if (d_latent2 && (e->codec_bf16 || !(parts & PART_TR))) return fail(-1, "frame pairs: fp32 codec transformer only");
  if (e->codec_bf16) return mimi_enqueue_h(st, e, s, d_latent, d_pcm, parts);
  if (parts & PART_TR) CHK(mimi_tr_enqueue(st, e, s, d_latent, d_latent2, parts == PART_TR));
  if (parts & PART_SEANET) CHK(mimi_seanet_enqueue(st, e, s, d_pcm, parts == PART_ALL ? 2 : 1));
  return 0;
}
// host bookkeeping of an enqueued (or replayed) part, and what must hold before it: tr_out is a ring, a transformer launch
// must not overwrite a slot that a waiting SEANet frame still reads (its own or its halo), SEANet needs a frame waiting
int mimi_parts_check(const ptts_mimi_state *s, int parts, int frames) {
  int wait = s->h_tr - s->h_frame;  // frames in tr_out that SEANet has not read
  if (parts & PART_TR) {
    // writing frames n .. n + frames - 1 frees slots (n - 4 ..): the oldest waiting frame f reads f and f - 1
    if (wait + frames + 1 > s->tr_out.slots) return fail(-1, "codec: the transformer is too far ahead of SEANet for the hand-over ring");
    wait += frames;
  }
  if ((parts & PART_SEANET) && wait < 1) return fail(-1, "codec: SEANet has no transformer frame to decode");
  return 0;
}
void mimi_parts_done(ptts_mimi_state *s, int parts, int frames) {
  if (parts & PART_TR) { s->h_tr += frames; s->h_tr_last = frames; }
  if (parts & PART_SEANET) s->h_frame += 1;
}

// The static activation scales of the fp8 codec (e->d_f8s) from a calibration run of the bf16 codec: 8 sequences x 6 frames
// of N(0, 1) latents; scale = 2 x amax / 448, saturating
__global__ void calib_latent_kernel(float *lat, int n, unsigned frame) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) lat[i] = counter_normal(0x5EEDull, frame, (unsigned)i);
}
void calib_latent(hipStream_t st, float *lat, int n, unsigned frame) {
  calib_latent_kernel<<<cdiv(n, 256), 256, 0, st>>>(lat, n, frame);
}
int calibrate_fp8_codec(ptts_engine *e) {
  const ptts_config &c = e->cfg;
  hipStream_t st = e->stream;
  const int B = 8, frames = 6;
  ptts_mimi_state *ms = nullptr;
  CHK(ptts_mimi_state_create(e, B, &ms));
  float *lat = nullptr, *amax = nullptr;
  int rc = 0;
  if (hipMalloc((void **)&lat, (size_t)B * c.ldim * 4) != hipSuccess || hipMalloc((void **)&amax, 64) != hipSuccess) rc = fail(-2, "hipMalloc (fp8 calibration)");
  if (rc == 0) {
    (void)hipMemsetAsync(amax, 0, 64, st);
    for (int f = 0; f < frames && rc == 0; ++f) {
      calib_latent(st, lat, B * c.ldim, (unsigned)f);
      rc = mimi_enqueue_h(st, e, ms, lat, nullptr);
      mimi_parts_done(ms, PART_ALL, 1);
      // both parity slots hold bf16 data in their first half (see mimi_enqueue_h); scan them after every frame
      auto scan = [&](const Ring &r, int slot) {
        for (int par = 0; par < 2; ++par) amax_bf16(st, r.slot(par), r.stride, amax + slot);
      };
      scan(ms->a0, 0);
      for (int i = 0; i < 3; ++i) {
        scan(ms->cbuf[i], 1 + 3 * i);
        amax_bf16(st, ms->rbuf[i], (long)B * (ms->rows[i + 1] / 16) * 256 * ((8 >> i) * c.n_filters / 2 / c.compress / 16), amax + 2 + 3 * i);
        if (i < 2) scan(ms->sbuf[i], 3 + 3 * i);
      }
    }
  }
  float h[16] = {};
  if (rc == 0 && (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(h, amax, 64, hipMemcpyDeviceToHost) != hipSuccess)) rc = fail(-2, "fp8 calibration failed");
  if (rc == 0) {
    for (float &v : h) v = v > 0.f ? 2.0f * v / 448.0f : 1.0f;
    if (hipMemcpy(e->d_f8s, h, 64, hipMemcpyHostToDevice) != hipSuccess) rc = fail(-2, "hipMemcpy (fp8 scales)");
  }
  if (lat) (void)hipFree(lat);
  if (amax) (void)hipFree(amax);
  ptts_mimi_state_destroy(ms);
  return rc;
}

// ---- the output chain -------------------------------------------------------------------------------------------------
// The stages behind the codec: one row per kind of ptts_mimi_state::chain, in launch order, with the words the kind's
// messages use, its SITE and thin adapters over what ptts_ext.h declares (the test taps are not fed from here).  While a
// link is set its stage's launch follows the codec's last kernel on the same stream.  It reads the link's `in`, which the
// caller has given the stage before it as its output, or without one the frame's fp32 PCM (d_pcm, or the state's own
// buffer), and writes the link's `out`.  A NULL stage clears the link: decodes and captures are then launch for launch what
// they were.
struct ChainKind {
  const char *setter, *noun, *site;
  bool f32_only;  // writes f32 into a device buffer that must not be its input, and a leveler must follow it
  int (*enqueue)(hipStream_t st, void *stage, const float *in, void *out, int i16);
};
#define ENQ(T, ...)                                                          \
  [](hipStream_t st, void *p, const float *in, void *out, int i16) {         \
    (void)i16;                                                               \
    T *stage = (T *)p;                                                       \
    return __VA_ARGS__;                                                      \
  }
static const ChainKind kChain[CH_N] = {
    {"set_resampler", "resampler", "resample", false, ENQ(ptts_resampler, resample_enqueue(st, stage, in, out, i16))},
    {"set_stretcher", "stretcher", "stretch", false, ENQ(ptts_stretcher, stretch_enqueue(st, stage, in, out, i16, nullptr))},
    {"set_pitcher", "pitcher", "pitch", false, ENQ(ptts_pitcher, pitch_enqueue(st, stage, in, out, i16, nullptr, nullptr))},
    {"set_tone", "toner", "tone", true, ENQ(ptts_tone, tone_enqueue(st, stage, in, (float *)out))},
    {"set_dynamics", "compressor", "dynamics", true, ENQ(ptts_dynamics, dyn_enqueue(st, stage, in, (float *)out))},
    {"set_loudnorm", "normaliser", "loudnorm", true, ENQ(ptts_loudnorm, loud_enqueue(st, stage, in, (float *)out, nullptr))},
    {"set_leveler", "leveler", "level", false, ENQ(ptts_leveler, level_enqueue(st, stage, in, out, i16))},
    {"set_encoder", "encoder", "encode", false, ENQ(ptts_encoder, encode_enqueue(st, stage, in, out))},
    {"set_packer", "packer", "flac", false, ENQ(ptts_flac, flac_enqueue(st, stage, (const void *)in, out))},
};
#undef ENQ
// what the chain reads of a stage: its batch and the widths of its lines (a stage's address is its StageBase's, ptts_stage.h)
static const StageBase *base(const void *stage) { return (const StageBase *)stage; }

// The stage that writes the encoder's input: the last one set of leveler, pitcher, stretcher, resampler; -1: none.  The
// toner and the normaliser do not count, a leveler always follows them.
static int before_encoder(const ptts_mimi_state *s) {
  int last = -1;
  for (int k : {CH_RS, CH_TS, CH_PS, CH_LV})
    if (s->chain[k].stage) last = k;
  return last;
}

// What the eight setters share, in this order: the state, the output, not in place (f32_only), the batch, then `own()`, the
// calling setter's own refusals (a whole message, or nullptr), then the frame length of a stage that reads the frame's PCM,
// and for an input buffer that some stage of a lower kind is set on the state NOW, which is why setters are called in
// chain order.
template <class Own>
static int set_link(ptts_mimi_state *s, int kind, void *stage, float *in, void *out, int i16, Own own) {
  if (!s) return fail(-1, "null state");
  const ChainKind &k = kChain[kind];
  const std::string set = std::string(k.setter) + ": ", its = set + "the " + k.noun + "'s ";
  if (stage) {
    if (!out) return fail(-1, set + "null output");
    if (k.f32_only && in == out) return fail(-1, set + "the stage does not work in place");
    if (base(stage)->B != s->B) return fail(-1, its + "batch is not the state's");
    if (const char *msg = own()) return fail(-1, msg);
    if (!in && base(stage)->in_width != s->rows[3]) return fail(-1, its + "frame length is not the state's");
    bool fed = false;
    for (int i = 0; i < kind; i++) fed |= s->chain[i].stage != nullptr;
    if (in && !fed) {
      std::string kinds;  // "a resampler, a stretcher or a pitcher"
      for (int i = 0; i < kind; i++) kinds += std::string(i == 0 ? "a " : i == kind - 1 ? " or a " : ", a ") + kChain[i].noun;
      return fail(-1, set + "an input buffer needs " + kinds + " on the state");
    }
  }
  s->chain[kind] = stage ? ChainLink{stage, in, out, i16 != 0} : ChainLink{};
  return 0;
}
static int set_link(ptts_mimi_state *s, int kind, void *stage, float *in, void *out, int i16) {
  return set_link(s, kind, stage, in, out, i16, [] { return (const char *)nullptr; });
}

// out [B][out_max] is f32 or i16, device or pinned host
extern "C" int ptts_mimi_set_resampler(ptts_mimi_state *s, ptts_resampler *rs, void *out, int32_t is_i16) {
  // its own: one message for the batch and the frame length, in place of the two of set_link
  if (s && rs && out && (base(rs)->B != s->B || base(rs)->in_width != s->rows[3]))
    return fail(-1, "set_resampler: the resampler's batch or frame length is not the state's");
  return set_link(s, CH_RS, rs, nullptr, out, is_i16);
}

// its own: with d_in the resampler writes f32 into d_in instead of its own output, so its longest frame must be the stretcher's
extern "C" int ptts_mimi_set_stretcher(ptts_mimi_state *s, ptts_stretcher *ts, float *d_in, void *out, int32_t is_i16) {
  return set_link(s, CH_TS, ts, d_in, out, is_i16, [&]() -> const char * {
    const StageBase *rs = base(s->chain[CH_RS].stage);
    if (d_in && (!rs || rs->out_width != base(ts)->in_width))
      return "set_stretcher: an input buffer needs a resampler on the state whose longest frame is the stretcher's";
    return nullptr;
  });
}

extern "C" int ptts_mimi_set_pitcher(ptts_mimi_state *s, ptts_pitcher *ps, float *d_in, void *out, int32_t is_i16) {
  return set_link(s, CH_PS, ps, d_in, out, is_i16);
}

// a frame enqueued with a toner but no leveler fails
extern "C" int ptts_mimi_set_tone(ptts_mimi_state *s, ptts_tone *tn, float *d_in, float *d_out) {
  return set_link(s, CH_TN, tn, d_in, d_out, 0);
}

// a frame enqueued with a compressor but no leveler fails
extern "C" int ptts_mimi_set_dynamics(ptts_mimi_state *s, ptts_dynamics *dy, float *d_in, float *d_out) {
  return set_link(s, CH_DY, dy, d_in, d_out, 0);
}

// a frame enqueued with a normaliser but no leveler fails
extern "C" int ptts_mimi_set_loudnorm(ptts_mimi_state *s, ptts_loudnorm *ln, float *d_in, float *d_out) {
  return set_link(s, CH_LN, ln, d_in, d_out, 0);
}

extern "C" int ptts_mimi_set_leveler(ptts_mimi_state *s, ptts_leveler *lv, float *d_in, void *out, int32_t is_i16) {
  return set_link(s, CH_LV, lv, d_in, out, is_i16);
}

// its own: the stage before_encoder() names writes f32 into d_in instead of its own output, so the encoder has an input
// buffer exactly when there is such a stage, and is as wide as that stage's widest line
extern "C" int ptts_mimi_set_encoder(ptts_mimi_state *s, ptts_encoder *en, float *d_in, void *out_bytes) {
  return set_link(s, CH_EN, en, d_in, out_bytes, 0, [&]() -> const char * {
    const int before = before_encoder(s);
    if (!d_in && before >= 0) return "set_encoder: the state has output stages, the encoder needs an input buffer";
    if (d_in && before < 0)
      return "set_encoder: an input buffer needs a resampler, a stretcher, a pitcher or a leveler on the state";
    if (d_in && base(s->chain[before].stage)->out_width != base(en)->in_width)
      return "set_encoder: the encoder's width is not the widest line of the stage before it";
    return nullptr;
  });
}

// its own: the packer reads the bytes of an encoder of its width, which must be on the state; ChainLink::in holds the byte
// buffer's address
extern "C" int ptts_mimi_set_packer(ptts_mimi_state *s, ptts_flac *pk, void *d_in_bytes, void *out_bytes) {
  return set_link(s, CH_PK, pk, (float *)d_in_bytes, out_bytes, 0, [&]() -> const char * {
    const StageBase *en = base(s->chain[CH_EN].stage);
    if (!en) return "set_packer: a packer needs an encoder on the state";
    if (!d_in_bytes) return "set_packer: null input";
    if (en->out_width != base(pk)->in_width) return "set_packer: the packer's width is not the encoder's";
    return nullptr;
  });
}

// the codec frame, then the launches of the links the state has; every refusal comes before the first launch
// (parts without PART_SEANET: the transformer alone, no stage launches)
int mimi_frame_enqueue(hipStream_t st, ptts_engine *e, ptts_mimi_state *s, const float *d_latent, float *d_pcm, int parts,
                       const float *d_latent2) {
  if (!(parts & PART_SEANET)) return mimi_enqueue(st, e, s, d_latent, d_latent2, nullptr, parts);
  const ChainLink *c = s->chain, &ts = c[CH_TS], &en = c[CH_EN];
  for (int i = 0; i < CH_N; i++) {  // from the normaliser round: it is refused first, then the toner, then the compressor
    const int k = (CH_LN + i) % CH_N;
    if (kChain[k].f32_only && c[k].stage && !c[CH_LV].stage)
      return fail(-1, std::string("the ") + kChain[k].noun + " must be followed by a leveler, but the state has none");
  }
  const int before = en.stage ? before_encoder(s) : -1;
  if (en.stage && (before >= 0) != (en.in != nullptr))
    return fail(-1, "the encoder's input buffer and the state's output stages do not go together");
  if (c[CH_PK].stage && !en.stage) return fail(-1, "the packer reads an encoder's bytes, but the state has no encoder");
  if (c[CH_PK].stage && (void *)c[CH_PK].in != en.out)
    return fail(-1, "the packer's input is not the buffer the encoder writes");
  const bool chained = ts.stage && ts.in;  // resampler -> ts.in -> stretcher
  if (chained && !c[CH_RS].stage) return fail(-1, "the stretcher reads a resampler's output, but the state has no resampler");
  CHK(mimi_enqueue(st, e, s, d_latent, d_latent2, d_pcm, parts));
  for (int k = 0; k < CH_N; k++) {
    if (!c[k].stage) continue;
    // a stage writes its own output, but for two that write f32 into the next one's input buffer: the stage before the
    // encoder, and the resampler before a stretcher that has one
    float *next = k == before ? en.in : k == CH_RS && chained ? ts.in : nullptr;
    const float *in = c[k].in ? c[k].in : (d_pcm ? d_pcm : s->pcm_dbg);
    SITE(kChain[k].site);
    const int r = kChain[k].enqueue(st, c[k].stage, in, next ? (void *)next : c[k].out, next ? 0 : c[k].i16);
    SITE("");
    if (r != 0) return r;
  }
  return 0;
}

extern "C" int ptts_mimi_decode(ptts_engine *e, ptts_mimi_state *s, const float *d_latent, float *d_pcm, void *stream) {
  ENGINE_LOCK(e);
  HIPCHK(hipSetDevice(e->device));
  if (!d_latent) return fail(-1, "null latent");
  CHK(mimi_parts_check(s, PART_ALL, 1));
  CHK(ensure_tr_taps(e, s));
  CHK(mimi_frame_enqueue(S(e, stream), e, s, d_latent, d_pcm));
  mimi_parts_done(s, PART_ALL, 1);
  LAUNCHCHK();
  return 0;
}

// The codec frame in its two parts (see mimi_tr_enqueue), for callers that schedule them apart: the transformer of one
// frame, or of a pair of consecutive frames (d_latent_b != NULL; fp32 codec), then one SEANet decode per frame, oldest first
extern "C" int ptts_mimi_decode_tr(ptts_engine *e, ptts_mimi_state *s, const float *d_latent, const float *d_latent_b, void *stream) {
  ENGINE_LOCK(e);
  HIPCHK(hipSetDevice(e->device));
  if (!d_latent) return fail(-1, "null latent");
  const int frames = d_latent_b ? 2 : 1;
  CHK(mimi_parts_check(s, PART_TR, frames));
  CHK(ensure_tr_taps(e, s));
  CHK(mimi_frame_enqueue(S(e, stream), e, s, d_latent, nullptr, PART_TR, d_latent_b));
  mimi_parts_done(s, PART_TR, frames);
  LAUNCHCHK();
  return 0;
}
extern "C" int ptts_mimi_decode_seanet(ptts_engine *e, ptts_mimi_state *s, float *d_pcm, void *stream) {
  ENGINE_LOCK(e);
  HIPCHK(hipSetDevice(e->device));
  CHK(mimi_parts_check(s, PART_SEANET, 0));
  CHK(mimi_frame_enqueue(S(e, stream), e, s, nullptr, d_pcm, PART_SEANET));
  mimi_parts_done(s, PART_SEANET, 0);
  LAUNCHCHK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Voice-prompt encode path (one-off per voice): MimiModel.encode_to_latent + speaker projection
// (reference mimi.py:96-119, tts_model.py:379-388).  Whole-signal causal convs = the same implicit GEMMs with
// zero / replicate left padding and an input stride.
extern "C" int ptts_encode_voice(ptts_engine *e, const float *d_audio, int64_t n_samples, float *d_latent_out,
                                 float *d_cond_out, int32_t *h_frames, void *stream) {
  ENGINE_LOCK(e);
  if (!e->has_encoder) return fail(-3, "the checkpoint passed to ptts_create has no Mimi encoder tensors");
  if (n_samples < 1) return fail(-1, "empty audio");
  HIPCHK(hipSetDevice(e->device));
  for (void *p : e->enc_keep) hipFree(p);  // the taps of the call before this one ("debug_taps")
  e->enc_keep.clear();
  e->enc_taps.clear();
  const ptts_config &c = e->cfg;
  hipStream_t st = S(e, stream);
  bind_engine(e);
  AllocScope alloc_scope(st);
  // "debug_taps": every intermediate is named here and outlives the call (ptts_debug_read_encoder); without it this
  // function allocates, copies and launches nothing more than it needs
  const bool keep = e->opt_debug_taps != 0;
  std::vector<ptts_engine::EncTap> taps;
  auto tap = [&](const std::string &name, const float *p, long n_rows, int cols) {
    if (keep) taps.push_back({name, p, (int)n_rows, cols});
  };
  const int hop = c.ratios[0] * c.ratios[1] * c.ratios[2];
  const long fs = (long)hop * c.upsample_stride;  // 1920
  const long R0 = (n_samples + fs - 1) / fs * fs;  // pad_for_conv1d(x, frame_size, frame_size)
  const int Tf = (int)(R0 / fs);
  const int C = c.m_dim, nf = c.n_filters;
  std::vector<void *> tmp;
  auto talloc = [&](float **p, size_t n) { int r = dallocT(nullptr, p, n); if (r == 0) tmp.push_back(*p); return r; };
  float *x0, *cur_r, *cur_e;
  CHK(talloc(&x0, (size_t)R0 * 16));
  CHK(talloc(&cur_r, (size_t)R0 * nf));
  CHK(talloc(&cur_e, (size_t)R0 * nf));
  audio_to_fm_kernel<<<cdiv(R0 / 16 * 64, 256), 256, 0, st>>>(d_audio, x0, (int)n_samples, (int)R0);
  tap("audio", x0, R0, 16);  // column 0: the samples, zero from n_samples on; columns 1..15 zero
  long rows = R0;
  auto conv = [&](const Lin &L, const float *X, int XF, long out_rows, int xstride, int halo, int mode) {
    GemmArgs a = mk_gemm(L, X, XF, (int)cdiv(out_rows, 16), (int)out_rows);
    a.T = cdiv(out_rows, 16) * 16;  // one sequence: t == row
    a.xstride = xstride; a.halo = halo; a.halo_mode = mode;
    return a;
  };
  SITE("enc.conv0");
  GemmArgs a = conv(e->enc_conv0, x0, 1, rows, 1, c.kernel_size - 1, 1);
  a.Y = cur_e; a.YF = nf / 16; a.act = ACT_ELU; a.Yraw = cur_r;
  launch_gemm(st, a, PRE_NONE);
  tap("conv0_raw", cur_r, rows, nf);
  tap("conv0", cur_e, rows, nf);
  int dim = nf;
  for (int i = 0; i < 3; ++i) {
    const int r = c.ratios[2 - i], hid = dim / c.compress;
    float *rb, *se, *nr, *ne;
    CHK(talloc(&rb, (size_t)rows * hid));
    CHK(talloc(&se, (size_t)rows * dim));
    SITE("enc.res_a");
    a = conv(e->enc_res_a[i], cur_e, dim / 16, rows, 1, c.res_kernel_size - 1, 1);
    a.Y = rb; a.YF = hid / 16; a.act = ACT_ELU;
    launch_gemm(st, a, PRE_NONE);
    SITE("enc.res_b");
    a = conv(e->enc_res_b[i], rb, hid / 16, rows, 1, 0, 1);
    a.epi = EPI_RES; a.R = cur_r; a.RF = dim / 16; a.Y = se; a.YF = dim / 16; a.act = ACT_ELU;
    launch_gemm(st, a, PRE_NONE);
    const long nrows = rows / r;
    CHK(talloc(&nr, (size_t)nrows * 2 * dim));
    CHK(talloc(&ne, (size_t)nrows * 2 * dim));
    SITE("enc.down");
    a = conv(e->enc_down[i], se, dim / 16, nrows, r, r, 1);  // kernel 2r, stride r: left context r
    a.Y = ne; a.YF = 2 * dim / 16; a.act = ACT_ELU; a.Yraw = nr;
    launch_gemm(st, a, PRE_NONE);
    const std::string n = std::to_string(i + 1);
    tap("rb" + n, rb, rows, hid);
    tap("se" + n, se, rows, dim);
    tap("down" + n + "_raw", nr, nrows, 2 * dim);
    tap("down" + n, ne, nrows, 2 * dim);
    cur_r = nr; cur_e = ne; rows = nrows; dim *= 2;
  }
  // final conv -> encoder-transformer input (rows = R0 / hop, a multiple of 16)
  const int M2 = (int)rows, MT2 = M2 / 16;
  const long ds_rows_in = (long)cdiv(Tf, 16) * 16 * c.upsample_stride;  // rows the downsample may touch
  float *tx;
  CHK(talloc(&tx, (size_t)std::max<long>(M2, ds_rows_in) * C));
  SITE("enc.final");
  a = conv(e->enc_final, cur_e, dim / 16, M2, 1, c.last_kernel_size - 1, 1);
  a.Y = tx; a.YF = C / 16;
  launch_gemm(st, a, PRE_NONE);
  float *tx_in = nullptr, *resid = nullptr;  // the transformer works in place: its input and the last layer's inner stream are copied
  if (keep) {
    CHK(talloc(&tx_in, (size_t)M2 * C));
    CHK(talloc(&resid, (size_t)M2 * C));
    HIPCHK(hipMemcpyAsync(tx_in, tx, (size_t)M2 * C * 4, hipMemcpyDeviceToDevice, st));
    tap("final", tx_in, M2, C);
  }
  // encoder transformer, whole sequence, RoPE offset 0, window = context (transformer.py:63-75)
  {
    const int H = c.m_heads, QB = MT2, cap = MT2 * 16;
    float *ao, *ff, *q, *part, *rope, *kv;
    int *off;
    const int splits = attn_splits(H * QB, std::min(MT2, cdiv(c.m_context, 16) + 2));
    CHK(talloc(&ao, (size_t)M2 * C));
    CHK(talloc(&ff, (size_t)M2 * c.m_ff));
    CHK(talloc(&q, (size_t)H * QB * 4 * 256));
    CHK(talloc(&part, (size_t)H * QB * splits * 16 * ATT_PSTRIDE));
    CHK(talloc(&rope, (size_t)M2 * 64));
    CHK(talloc(&kv, (size_t)2 * H * cap * 64));
    CHK(talloc((float **)&off, 4));
    rope_table_kernel<<<cdiv(M2 * 32, 256), 256, 0, st>>>(off, e->freq_mimi, rope, M2, M2);
    for (int l = 0; l < c.m_layers; ++l) {
      TrCtx t;
      t.D = C; t.H = H; t.FF = c.m_ff; t.MT = MT2; t.M = M2; t.Tq = M2; t.QB = QB;
      t.cap = cap; t.ring = 0; t.ctx = c.m_context; t.splits = splits;
      t.x_in = tx; t.x = tx; t.x_out = tx; t.out_ds = 0; t.par = nullptr;
      t.h = nullptr; t.ao = ao; t.ff = ff; t.q = q; t.part = part;
      t.Kc = kv; t.Vc = kv + (size_t)H * cap * 64; t.offset = off; t.rope = rope;
      t.kv_keys = (double)M2 * std::min(M2, c.m_context) / 16.0;
      t.tag = "enc";
      t.tap_x = l == c.m_layers - 1 ? resid : nullptr;
      run_tr_layer(st, e->enc_tr[l], t);
    }
    if (keep) taps.push_back({"tr_qkv", q, M2, 3 * C, kv, kv + (size_t)H * cap * 64, off, H, QB, cap});
    tap("tr_attn", ao, M2, C);
    tap("tr_resid", resid, M2, C);
    tap("tr_ff", ff, M2, c.m_ff);
    tap("enc_tr", tx, M2, C);
  }
  // ConvDownsample1d: kernel 2s, stride s, replicate padding, no bias (resample.py:7-29)
  float *lat, *cond;
  const int MT3 = cdiv(Tf, 16);
  CHK(talloc(&lat, (size_t)MT3 * 16 * c.ldim));
  CHK(talloc(&cond, (size_t)MT3 * 16 * c.d_model));
  SITE("enc.downsample");
  a = conv(e->enc_downsample, tx, C / 16, Tf, c.upsample_stride, c.upsample_stride, 2);
  a.Y = lat; a.YF = c.ldim / 16;
  launch_gemm(st, a, PRE_NONE);
  SITE("enc.speaker_proj");
  a = mk_gemm(e->speaker_proj, lat, c.ldim / 16, MT3, Tf);
  a.Y = cond; a.YF = c.d_model / 16;
  launch_gemm(st, a, PRE_NONE);
  SITE("");
  if (d_latent_out) from_fm_kernel<<<cdiv((long)Tf * c.ldim / 4, 256), 256, 0, st>>>(lat, d_latent_out, Tf, c.ldim, c.ldim / 16, 0);
  if (d_cond_out) from_fm_kernel<<<cdiv((long)Tf * c.d_model / 4, 256), 256, 0, st>>>(cond, d_cond_out, Tf, c.d_model, c.d_model / 16, 0);
  LAUNCHCHK();
  HIPCHK(hipStreamSynchronize(st));
  if (keep) {
    tap("latent", lat, Tf, c.ldim);
    tap("cond", cond, Tf, c.d_model);
    e->enc_keep.swap(tmp);
    e->enc_taps.swap(taps);
  }
  for (void *p : tmp) hipFree(p);
  if (h_frames) *h_frames = Tf;
  return 0;
}
