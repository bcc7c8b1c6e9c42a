// Host side of libptts: engine construction (weight packing), FlowLM / Mimi step orchestration,
// hipGraph capture and the C ABI declared in include/ptts.h.
#include "ptts_host.h"
#include "ptts_flow.h"
#include "ptts_bf16.h"
#include "ptts_lm.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>

static thread_local std::string g_err;
int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}
static thread_local std::string g_launch_err;  // see LAUNCHCHK (ptts_host.h)
bool launch_err_pending() { return !g_launch_err.empty(); }
int take_launch_err() {
  std::string m;
  m.swap(g_launch_err);
  return fail(-4, m);
}
void note_launch_err(const std::string &msg) { if (g_launch_err.empty()) g_launch_err = msg; }

// Per-call context: every entry point binds its engine's profiler / tuner / zero line in the CALLING thread
// (bind_engine), so two engines driven from two threads never see each other's state.  One engine is driven by one
// thread at a time (entry points take the engine mutex; see the threading contract in include/ptts.h).
static thread_local Profiler *g_prof = nullptr;
static thread_local const char *g_site = "";
ProfScope::ProfScope(hipStream_t st_, const std::string &kernel, double bytes, double flops) : st(st_), pr(g_prof && g_prof->on ? g_prof : nullptr), idx(0) {
  if (!pr) return;
  ProfRec r{g_site, kernel, bytes, flops, nullptr, nullptr};
  if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) { pr = nullptr; return; }
  (void)hipEventRecord(r.a, st);
  idx = pr->recs.size();
  pr->recs.push_back(r);
}
ProfScope::~ProfScope() { if (pr) (void)hipEventRecord(pr->recs[idx].b, st); }
#define SITE(x) g_site = (x)
const char *launch_site() { return g_site; }
void set_launch_site(const char *site) { g_site = site; }

// ------------------------------------------------------------------------------------------------
struct ptts_graph {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  // second capture of an LM step for states whose rows share a prefix (attn_cascade_kernel instead of the per-row decode
  // attention): ptts_graph_launch picks by the state's borrow count, which the host knows
  hipGraph_t graph_c = nullptr;
  hipGraphExec_t exec_c = nullptr;
  ptts_lm_state *lm = nullptr;
  ptts_mimi_state *mimi = nullptr;
  int mimi_parts = 3, mimi_frames = 1;  // what of the codec frame the graph holds (PART_*), transformer frames per launch
  hipStream_t cap_stream = nullptr;
  int coop_wgs = 0;  // workgroups of the largest cooperative launch inside (0: none): the launch stream needs that many CUs
  hipStream_t cu_checked = nullptr;  // the last launch stream whose CU mask was found large enough (checked once per stream)
};

// ------------------------------------------------------------------------------------------------
// allocation helpers
// Zero-filled device allocation.  The fill is queued on `st` (the engine stream, which is
// non-blocking and therefore NOT ordered against the null stream a plain hipMemset would use).
// The zero fill is queued on the stream of the innermost AllocScope of the CALLING thread (thread-local: a
// concurrent call on another engine / thread can no longer redirect it).
static thread_local hipStream_t t_alloc_stream = nullptr;
AllocScope::AllocScope(hipStream_t st) : prev(t_alloc_stream) { t_alloc_stream = st; }
AllocScope::~AllocScope() { t_alloc_stream = prev; }
int dalloc(ptts_engine *e, void **p, size_t bytes) {
  hipStream_t st = t_alloc_stream ? t_alloc_stream : (e ? e->stream : nullptr);
  if (!st) return fail(-1, "internal: allocation outside an AllocScope");
  if (bytes == 0) bytes = 256;
  *p = nullptr;
  const hipError_t err = hipMalloc(p, bytes);
  if (err != hipSuccess) {
    (void)hipGetLastError();  // the error is reported here; do not leave it sticky for the next hipGetLastError()
    *p = nullptr;
    return fail(-2, "hipMalloc of " + std::to_string(bytes) + " bytes: " + hipGetErrorString(err));
  }
  HIPCHK(hipMemsetAsync(*p, 0, bytes, st));
  if (e) { e->allocs.push_back(*p); e->alloc_bytes[*p] = bytes; }
  return 0;
}

static const ptts_tensor *find_tensor(ptts_engine *e, const std::string &name, int64_t numel, int *err) {
  if (e->blob_dummy) return e->blob_dummy;  // loading a packed engine: the packing kernels run on zeros, the real images follow
  auto it = e->tmap.find(name);
  if (it == e->tmap.end()) {
    *err = fail(-3, "missing tensor: " + name);
    return nullptr;
  }
  if (numel >= 0 && it->second->numel != numel) {
    *err = fail(-3, "tensor " + name + ": expected " + std::to_string(numel) + " elements, got " +
                        std::to_string(it->second->numel));
    return nullptr;
  }
  return it->second;
}

// copies a small fp32 vector (norm gains, biases, ...) into engine-owned memory, padded
static int copy_vec(ptts_engine *e, const std::string &name, int64_t n, float **out, int64_t pad_to = 0) {
  int err = 0;
  const ptts_tensor *t = find_tensor(e, name, n, &err);
  if (!t) return err;
  CHK(dallocT(e, out, std::max<int64_t>(pad_to, n)));
  HIPCHK(hipMemcpyAsync(*out, t->d_data, n * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
  return 0;
}

// packs one or several [N_i][C][ntaps] matrices (stacked along N) into one Lin
int pack_lin(ptts_engine *e, Lin *L, const std::vector<PackPart> &parts, int C, int ntaps, int mode, int cout, int stride,
             const std::string &ln_w, const std::string &ln_b, int creal, int wfmt) {
  const bool q8 = wfmt == 1, b16 = wfmt == 2;
  if (C % 16) return fail(-4, "channel count must be a multiple of 16: " + parts[0].w);
  if (b16 && (parts.size() != 1 || mode != 0 || ntaps != 1 || (C / 16) % 2))
    return fail(-4, "bf16 LM weights need a single Linear matrix with in_features % 32 == 0: " + parts[0].w);
  if (q8 && (parts.size() != 1 || mode != 0 || ntaps != 1 || (C / 16) % 4))
    return fail(-4, "int8 weights need a single Linear matrix with in_features % 64 == 0: " + parts[0].w);
  int ntot = 0;
  for (auto &p : parts) ntot += cdiv(p.N, 16);
  L->NT = ntot;
  L->C = C;
  L->CF = C / 16;
  L->ntaps = ntaps;
  L->KF = L->CF * ntaps;
  L->cout = cout;
  L->stride = stride;
  L->N = 0;
  CHK(dallocT(e, &L->w, (size_t)L->NT * L->KF * 256));
  bool any_bias = false;
  for (auto &p : parts) any_bias |= !p.b.empty();
  const float *gam = nullptr, *bet = nullptr;
  if (!ln_w.empty()) {
    // fold the preceding LayerNorm: gain into the weights, mean / bias terms into two per-row vectors
    int err = 0;
    const ptts_tensor *tg = find_tensor(e, ln_w, C, &err), *tb = find_tensor(e, ln_b, C, &err);
    if (!tg || !tb) return err;
    gam = tg->d_data;
    bet = tb->d_data;
    CHK(dallocT(e, &L->ln_s, (size_t)L->NT * 16));
    CHK(dallocT(e, &L->ln_c, (size_t)L->NT * 16));
    any_bias = false;  // the bias is absorbed into ln_c
  }
  if (any_bias) CHK(dallocT(e, &L->bias, (size_t)L->NT * 16));
  int nt_off = 0;
  for (auto &p : parts) {
    int err = 0;
    const ptts_tensor *t = find_tensor(e, p.w, (int64_t)(mode == 0 ? p.N : (p.N / stride)) * (creal > 0 ? creal : C) * (mode == 0 ? ntaps : 2 * stride), &err);
    if (!t) return err;
    int nt = cdiv(p.N, 16);
    long total = (long)nt * L->KF * 256;
    pack_weight_kernel<<<cdiv(total, 256), 256, 0, e->stream>>>(t->d_data, L->w, p.N, C, ntaps, mode, cout, stride,
                                                                nt_off, L->KF, total, q8 ? nullptr : gam, creal > 0 ? creal : C);
    if (gam && !q8) {
      const float *bsrc = nullptr;
      if (!p.b.empty()) {
        const ptts_tensor *tb2 = find_tensor(e, p.b, p.N, &err);
        if (!tb2) return err;
        bsrc = tb2->d_data;
      }
      fold_ln_kernel<<<p.N, 64, 0, e->stream>>>(t->d_data, gam, bet, bsrc, L->ln_s, L->ln_c, p.N, C, nt_off * 16);
    }
    if (any_bias) {
      const float *bsrc = nullptr;
      if (!p.b.empty()) {
        const ptts_tensor *tb = find_tensor(e, p.b, mode == 0 ? p.N : cout, &err);
        if (!tb) return err;
        bsrc = tb->d_data;
      }
      pack_bias_kernel<<<cdiv(nt * 16, 256), 256, 0, e->stream>>>(bsrc, L->bias, p.N, mode, cout, nt_off * 16, nt * 16);
    }
    nt_off += nt;
    L->N += p.N;
  }
  if (q8) {
    int err = 0;
    const float *bsrc = nullptr;
    if (gam && !parts[0].b.empty()) {
      const ptts_tensor *tb2 = find_tensor(e, parts[0].b, parts[0].N, &err);
      if (!tb2) return err;
      bsrc = tb2->d_data;
    }
    CHK(dalloc(e, (void **)&L->wq, (size_t)L->NT * L->KF * 256));
    CHK(dallocT(e, &L->wscale, (size_t)L->NT * 16));
    if (gam) CHK(copy_vec(e, ln_w, C, &L->ln_g));
    quantize_packed_kernel<<<L->NT, 256, 0, e->stream>>>(L->w, L->wq, L->wscale, L->KF, gam, bet, bsrc, L->N, L->ln_s, L->ln_c);
    LAUNCHCHK();
    // the fp32 image is only the quantiser's input
    HIPCHK(hipStreamSynchronize(e->stream));
    e->allocs.erase(std::remove(e->allocs.begin(), e->allocs.end(), (void *)L->w), e->allocs.end());
    e->alloc_bytes.erase((void *)L->w);
    HIPCHK(hipFree(L->w));
    L->w = nullptr;
  }
  if (b16) {
    // bf16 image from the fp32 one (LayerNorm gain already multiplied in); the fold vector s comes from the ROUNDED rows
    CHK(dalloc(e, &L->wb16, (size_t)L->NT * L->KF * 512));
    pack_weight_b16(e->stream, L->w, L->wb16, gam ? L->ln_s : nullptr, L->NT, L->KF);
    LAUNCHCHK();
    HIPCHK(hipStreamSynchronize(e->stream));
    e->allocs.erase(std::remove(e->allocs.begin(), e->allocs.end(), (void *)L->w), e->allocs.end());
    e->alloc_bytes.erase((void *)L->w);
    HIPCHK(hipFree(L->w));
    L->w = nullptr;
  }
  LAUNCHCHK();
  return 0;
}

// bf16 twin of a packed matrix for the reduced-precision codec path (single-part matrices only)
int pack_lin_h(ptts_engine *e, Lin *L, const std::string &wname, int N, int C, int ntaps, int mode, int cout, int stride,
               const std::string &ln_w) {
  if (C % 32) return fail(-4, "bf16 codec path: channel count must be a multiple of 32: " + wname);
  int err = 0;
  const ptts_tensor *t = find_tensor(e, wname, -1, &err);
  if (!t) return err;
  const float *gam = nullptr;
  if (!ln_w.empty()) {
    const ptts_tensor *tg = find_tensor(e, ln_w, C, &err);
    if (!tg) return err;
    gam = tg->d_data;
  }
  const int KBt = (C / 32) * ntaps;
  const long total = (long)L->NT * KBt * 512;
  CHK(dalloc(e, (void **)&L->wh, (size_t)total * 2));
  pack_weight_h_kernel<<<cdiv(total, 256), 256, 0, e->stream>>>(t->d_data, L->wh, N, C, ntaps, mode, cout, stride, KBt, total, gam);
  if (gam) {
    CHK(dallocT(e, &L->ln_s_h, (size_t)L->NT * 16));
    fold_s_h_kernel<<<N, 64, 0, e->stream>>>(L->wh, L->ln_s_h, N, KBt);
  }
  LAUNCHCHK();
  e->mimi_bytes_h += total * 2;
  return 0;
}

static int pack_tr_layer(ptts_engine *e, TrLayer *T, const std::string &p, int d, int ff, bool ls, int quant = 0) {
  const int qa = (quant & PTTS_LM_BF16) ? 2 : (quant & PTTS_QUANT_ATTENTION) ? 1 : 0;
  const int qf = (quant & PTTS_LM_BF16) ? 2 : (quant & PTTS_QUANT_FFN) ? 1 : 0;
  CHK(copy_vec(e, p + ".norm1.weight", d, &T->ln1_w));
  CHK(copy_vec(e, p + ".norm1.bias", d, &T->ln1_b));
  CHK(copy_vec(e, p + ".norm2.weight", d, &T->ln2_w));
  CHK(copy_vec(e, p + ".norm2.bias", d, &T->ln2_b));
  if (ls) {
    CHK(copy_vec(e, p + ".layer_scale_1.scale", d, &T->ls1));
    CHK(copy_vec(e, p + ".layer_scale_2.scale", d, &T->ls2));
  }
  CHK(pack_lin(e, &T->qkv, {{p + ".self_attn.in_proj.weight", "", 3 * d}}, d, 1, 0, 0, 0, p + ".norm1.weight", p + ".norm1.bias", 0, qa));
  CHK(pack_lin(e, &T->out, {{p + ".self_attn.out_proj.weight", "", d}}, d, 1, 0, 0, 0, "", "", 0, qa));
  CHK(pack_lin(e, &T->ff1, {{p + ".linear1.weight", "", ff}}, d, 1, 0, 0, 0, p + ".norm2.weight", p + ".norm2.bias", 0, qf));
  CHK(pack_lin(e, &T->ff2, {{p + ".linear2.weight", "", d}}, ff, 1, 0, 0, 0, "", "", 0, qf));
  return 0;
}

static int make_freq(ptts_engine *e, float **out, float max_period) {
  // freqs = exp(ds * (-ln(max_period) * 2 / D)) in fp32, D = 64 (reference rope.py:28-29)
  float h[32];
  const float coef = (float)(-std::log((double)max_period) * 2.0 / 64.0);
  for (int i = 0; i < 32; ++i) h[i] = std::exp((float)i * coef);
  CHK(dallocT(e, out, 32));
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(*out, h, sizeof(h), hipMemcpyHostToDevice));
  return 0;
}

void bind_engine(ptts_engine *e) {
  bind_dispatch(e);
  g_prof = &e->prof;
}

// One pre-LN transformer layer on M rows (reference mimi_transformer.py:39-54, transformer.py:135-158)
void run_tr_layer(hipStream_t st, const TrLayer &T, const TrCtx &c) {
  const int DF = c.D / 16;
  const std::string tg(c.tag);
  std::string s1 = tg + ".ln1", s2 = tg + ".qkv", s3 = tg + ".attn", s4 = tg + ".out", s5 = tg + ".ln2", s6 = tg + ".ff1", s7 = tg + ".ff2";
  // norm1 is folded into the QKV projection, norm2 into linear1 (PRE_LNFOLD): no LayerNorm launches
  SITE(s2.c_str());
  GemmArgs a = mk_gemm(T.qkv, c.x_in, DF, c.MT, c.M);
  a.epi = EPI_QKV;
  a.Q = c.q; a.Kc = c.Kc; a.Vc = c.Vc; a.offset = c.offset; a.rope = c.rope;
  a.H = c.H; a.Tq = c.Tq; a.QB = c.QB; a.cap = c.cap; a.ring = c.ring; a.qlen = c.qlen;
  launch_gemm(st, a, PRE_LNFOLD);
  AttnArgs at;
  at.Q = c.q; at.Kc = c.Kc; at.Vc = c.Vc; at.offset = c.offset; at.H = c.H; at.Tq = c.Tq; at.QB = c.QB;
  at.cap = c.cap; at.ring = c.ring; at.ctx = c.ctx; at.splits = c.splits; at.part = c.part; at.Y = c.ao; at.YF = DF; at.h16 = 0;
  at.pre = c.pre; at.layer = c.layer; at.qlen = c.qlen;
  const int BH = (c.M / c.Tq) * c.H;
  at.nseq = BH / c.H;
  SITE(s3.c_str());
  // K and V rows of every attended key once per head + q in + o out.  bytes: SURVEY 8d's per-sequence figure (every
  // sequence reads all of its keys), also for the cascade kernel, which fetches a shared prefix once per R sequences -
  // bench.py reports the unique bytes next to it
  launch_attention(st, at, BH, c.cascade, -1, c.kv_keys * c.H * 64 * 4 * 2 + 8.0 * c.M * c.D,
                   4.0 * c.kv_keys * c.H * 64 * std::min(c.Tq, 16));
  SITE(s4.c_str());
  a = mk_gemm(T.out, c.ao, DF, c.MT, c.M);
  a.epi = EPI_RES; a.R = c.x_in; a.RF = DF; a.Y = c.x; a.YF = DF; a.ls = T.ls1;
  launch_gemm(st, a, PRE_NONE);
  if (c.tap_x) (void)hipMemcpyAsync(c.tap_x, c.x, (size_t)c.M * c.D * 4, hipMemcpyDeviceToDevice, st);
  SITE(s6.c_str());
  a = mk_gemm(T.ff1, c.x, DF, c.MT, c.M);
  a.epi = EPI_STORE; a.act = ACT_GELU; a.Y = c.ff; a.YF = c.FF / 16;
  launch_gemm(st, a, PRE_LNFOLD);
  SITE(s7.c_str());
  a = mk_gemm(T.ff2, c.ff, c.FF / 16, c.MT, c.M);
  a.epi = EPI_RES; a.R = c.x; a.RF = DF; a.Y = c.x_out; a.YF = DF; a.Ydstride = c.out_ds; a.par = c.par; a.ls = T.ls2;
  a.yring = c.out_ring;
  launch_gemm(st, a, PRE_NONE);
  SITE("");
}

// ------------------------------------------------------------------------------------------------
extern "C" int ptts_abi_version(void) { return PTTS_ABI_VERSION; }
extern "C" const char *ptts_last_error(void) { return g_err.c_str(); }

static int seanet_check(const ptts_config &c) {
  // an untrusted config (a packed-engine file) reaches this function: no division before the divisors are checked
  if (c.d_model < 64 || c.num_heads < 1 || c.num_layers < 1 || c.m_dim < 64 || c.m_heads < 1 || c.m_layers < 1 || c.ldim < 16 ||
      c.flow_dim < 16 || c.flow_depth < 1 || c.ff_dim < 16 || c.m_ff < 16 || c.n_filters < 1 || c.compress < 1 ||
      c.kernel_size < 1 || c.res_kernel_size < 1 || c.last_kernel_size < 1 || c.ratios[0] < 1 || c.ratios[1] < 1 || c.ratios[2] < 1)
    return fail(-4, "model dimensions must be positive");
  if (c.d_model % 64 || c.d_model / c.num_heads != 64 || c.d_model % c.num_heads) return fail(-4, "FlowLM head dim must be 64");
  if (c.m_dim % c.m_heads || c.m_dim / c.m_heads != 64) return fail(-4, "Mimi head dim must be 64");
  if (c.d_model > 1024 || c.m_dim > 1024 || c.flow_dim > 1024) return fail(-4, "LayerNorm width > 1024 unsupported");
  if (c.ldim % 16 || c.flow_dim % 16 || c.ff_dim % 16 || c.m_ff % 16) return fail(-4, "dims must be multiples of 16");
  if (c.upsample_stride != 16) return fail(-4, "upsample stride must be 16 (one row tile per frame)");
  if ((c.n_filters / c.compress) % 16) return fail(-4, "n_filters/compress must be a multiple of 16");
  return 0;
}

static int build_engine(ptts_engine *e, const ptts_tensor *tensors, int32_t n);
static int build_fp8_codec(ptts_engine *e);
static int sync_host_tables(ptts_engine *e);

// device properties + the option defaults from the environment: shared by ptts_create_ex and ptts_create_from_file
static int init_engine_options(ptts_engine *e, int device) {
  e->device = device;
  e->tuner = new Tuner();
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  e->n_cus = std::max(1, prop.multiProcessorCount);
  if (const char *v = getenv("PTTS_FLOW_CLUSTER")) e->opt_flow_cluster = atoi(v) != 0;
  if (const char *v = getenv("PTTS_LM_CLUSTER")) e->opt_lm_cluster = atoi(v) != 0;
  if (const char *v = getenv("PTTS_K_ROTATE")) e->opt_k_rotate = atoi(v) != 0;
  if (const char *v = getenv("PTTS_FUSE_RES")) e->opt_fuse_res = atoi(v) != 0;
  if (const char *v = getenv("PTTS_SHARE_PREFIX")) e->opt_share_prefix = atoi(v) != 0;
  if (const char *v = getenv("PTTS_SINGLE_STORE")) e->opt_single_store = atoi(v) != 0;
  if (const char *v = getenv("PTTS_FUSE_PCM")) e->opt_fuse_pcm = atoi(v) != 0;
  if (const char *v = getenv("PTTS_CASCADE")) e->opt_cascade = atoi(v);
  if (const char *v = getenv("PTTS_FLOW_MAX_CUS")) e->opt_flow_max_cus = std::max(8, atoi(v));
  e->opt_flow_max_cus = std::min(e->opt_flow_max_cus, e->n_cus);  // a cooperative grid never exceeds the device
  if (const char *v = getenv("PTTS_CODEC_LDS_TARGET")) e->opt_codec_lds_target = std::max(0, std::min(atoi(v), 64 * 1024));
  return 0;
}

extern "C" int ptts_create(const ptts_config *cfg, const ptts_tensor *tensors, int32_t n, int32_t device,
                           ptts_engine **out) {
  return ptts_create_ex(cfg, tensors, n, device, 0, out);
}

extern "C" int ptts_create_ex(const ptts_config *cfg, const ptts_tensor *tensors, int32_t n, int32_t device,
                              int32_t quant_flags, ptts_engine **out) {
  if (!cfg || !tensors || !out) return fail(-1, "null argument");
  if (quant_flags & ~(PTTS_QUANT_ATTENTION | PTTS_QUANT_FFN | PTTS_CODEC_BF16 | PTTS_CODEC_FP8 | PTTS_LM_BF16 | PTTS_CODEC_SPLIT)) return fail(-1, "unknown quantisation group");
  if ((quant_flags & PTTS_CODEC_BF16) && (quant_flags & PTTS_CODEC_FP8)) return fail(-1, "PTTS_CODEC_BF16 and PTTS_CODEC_FP8 are exclusive");
  if ((quant_flags & PTTS_CODEC_SPLIT) && (quant_flags & (PTTS_CODEC_BF16 | PTTS_CODEC_FP8))) return fail(-1, "PTTS_CODEC_SPLIT and the bf16 / fp8 codec are exclusive");
  if ((quant_flags & PTTS_LM_BF16) && (quant_flags & (PTTS_QUANT_ATTENTION | PTTS_QUANT_FFN))) return fail(-1, "PTTS_LM_BF16 and the int8 groups are exclusive");
  CHK(seanet_check(*cfg));
  HIPCHK(hipSetDevice(device));
  ptts_engine *e = new ptts_engine();
  e->cfg = *cfg;
  e->quant_flags = quant_flags;
  int rc = init_engine_options(e, device);
  if (rc == 0) rc = build_engine(e, tensors, n);
  if (rc < 0) {  // missing / ill-shaped tensor, HIP error: release what was built so far
    const std::string msg = g_err;
    ptts_destroy(e);
    return fail(rc, msg);
  }
  *out = e;
  return 0;
}

static int build_engine(ptts_engine *e, const ptts_tensor *tensors, int32_t n) {
  HIPCHK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  AllocScope alloc_scope(e->stream);
  HIPCHK(hipEventCreate(&e->ev0));
  HIPCHK(hipEventCreate(&e->ev1));
  for (int i = 0; i < n; ++i) e->tmap[tensors[i].name] = &tensors[i];
  const ptts_config &c = e->cfg;
  const int D = c.d_model, FD = c.flow_dim;
  std::string p = "flow_lm.";
  CHK(copy_vec(e, p + "bos_emb", c.ldim, &e->bos));
  CHK(make_freq(e, &e->freq_lm, c.max_period));
  CHK(pack_lin(e, &e->in_linear, {{p + "input_linear.weight", "", D}}, c.ldim, 1));
  e->lm.resize(c.num_layers);
  for (int l = 0; l < c.num_layers; ++l)
    CHK(pack_tr_layer(e, &e->lm[l], p + "transformer.layers." + std::to_string(l), D, c.ff_dim, false, e->quant_flags));
  CHK(copy_vec(e, p + "out_norm.weight", D, &e->outnorm_w));
  CHK(copy_vec(e, p + "out_norm.bias", D, &e->outnorm_b));
  std::string f = p + "flow_net.";
  // head = [cond_embed ; out_eos]: both read the out_norm output (flow_lm.py:129, mlp.py:209)
  CHK(pack_lin(e, &e->head, {{f + "cond_embed.weight", f + "cond_embed.bias", FD}, {p + "out_eos.weight", p + "out_eos.bias", 1}}, D, 1,
               0, 0, 0, p + "out_norm.weight", p + "out_norm.bias"));
  {
    std::vector<PackPart> parts;
    for (int i = 0; i < c.flow_depth; ++i) {
      std::string r = f + "res_blocks." + std::to_string(i) + ".adaLN_modulation.1.";
      parts.push_back({r + "weight", r + "bias", 3 * FD});
    }
    parts.push_back({f + "final_layer.adaLN_modulation.1.weight", f + "final_layer.adaLN_modulation.1.bias", 2 * FD});
    CHK(pack_lin(e, &e->adaln, parts, FD, 1));
  }
  CHK(pack_lin(e, &e->input_proj, {{f + "input_proj.weight", f + "input_proj.bias", FD}}, c.ldim, 1));
  e->res.resize(c.flow_depth);
  for (int i = 0; i < c.flow_depth; ++i) {
    std::string r = f + "res_blocks." + std::to_string(i) + ".";
    CHK(copy_vec(e, r + "in_ln.weight", FD, &e->res[i].ln_w));
    CHK(copy_vec(e, r + "in_ln.bias", FD, &e->res[i].ln_b));
    CHK(pack_lin(e, &e->res[i].l0, {{r + "mlp.0.weight", r + "mlp.0.bias", FD}}, FD, 1));
    CHK(pack_lin(e, &e->res[i].l2, {{r + "mlp.2.weight", r + "mlp.2.bias", FD}}, FD, 1));
  }
  CHK(pack_lin(e, &e->fin, {{f + "final_layer.linear.weight", f + "final_layer.linear.bias", c.ldim}}, FD, 1));
  for (int i = 0; i < 2; ++i) {
    std::string t = f + "time_embed." + std::to_string(i) + ".";
    CHK(copy_vec(e, t + "freqs", 128, &e->te_freqs[i]));
    CHK(copy_vec(e, t + "mlp.3.alpha", FD, &e->te_alpha[i]));
    CHK(pack_lin(e, &e->te_l0[i], {{t + "mlp.0.weight", t + "mlp.0.bias", FD}}, 256, 1));
    CHK(pack_lin(e, &e->te_l2[i], {{t + "mlp.2.weight", t + "mlp.2.bias", FD}}, FD, 1));
  }
  CHK(dallocT(e, &e->te_scratch, (size_t)4 * 1024 * 16));
  e->lm_bytes = e->in_linear.bytes() + e->head.bytes() + e->adaln.bytes() + e->input_proj.bytes() + e->fin.bytes();
  for (auto &L : e->lm) e->lm_bytes += L.qkv.bytes() + L.out.bytes() + L.ff1.bytes() + L.ff2.bytes();
  for (auto &R : e->res) e->lm_bytes += R.l0.bytes() + R.l2.bytes();
  {
    // layer table of the single-launch transformer stack: fp32 weights, no LayerScale, head dim 64 (4 column tiles per
    // head), linear1 at most 4 column tiles per workgroup
    const int DF = D / 16, FFF = c.ff_dim / 16;
    bool ok = DF <= 64 && DF % 4 == 0 && c.num_heads * 4 == DF && FFF % DF == 0 && FFF / DF <= 4 && c.num_layers <= 64;
    for (auto &L : e->lm) ok = ok && L.qkv.w && L.out.w && L.ff1.w && L.ff2.w && !L.ls1 && !L.ls2 && L.qkv.ln_s && L.ff1.ln_s;
    if (ok) {
      std::vector<LmLayerP> h(c.num_layers);
      for (int l = 0; l < c.num_layers; ++l) {
        const TrLayer &T = e->lm[l];
        h[l] = LmLayerP{T.qkv.w, T.qkv.ln_s, T.qkv.ln_c, T.out.w, T.ff1.w, T.ff1.ln_s, T.ff1.ln_c, T.ff2.w};
      }
      CHK(dalloc(e, (void **)&e->lm_table, h.size() * sizeof(LmLayerP)));
      HIPCHK(hipStreamSynchronize(e->stream));
      HIPCHK(hipMemcpy(e->lm_table, h.data(), h.size() * sizeof(LmLayerP), hipMemcpyHostToDevice));
    }
  }

  // ---- Mimi decode side
  CHK(copy_vec(e, p + "emb_std", c.ldim, &e->emb_std));
  CHK(copy_vec(e, p + "emb_mean", c.ldim, &e->emb_mean));
  const int C = c.m_dim;
  CHK(copy_vec(e, "mimi.quantizer.output_proj.weight", (int64_t)C * c.ldim, &e->quant_w));
  CHK(copy_vec(e, "mimi.upsample.convtr.convtr.weight", (int64_t)C * 2 * c.upsample_stride, &e->up_w));
  CHK(make_freq(e, &e->freq_mimi, c.m_max_period));
  e->mm.resize(c.m_layers);
  for (int l = 0; l < c.m_layers; ++l)
    CHK(pack_tr_layer(e, &e->mm[l], "mimi.decoder_transformer.transformer.layers." + std::to_string(l), C, c.m_ff, true));
  // the context in whole 16-row frames plus TWO frames being written: a frame pair's 32 queries per sequence need
  // ring >= context + 31 (attn_valid).  The window mask decides what a query attends, not the ring's size
  e->ring = c.m_context > 0 ? (cdiv(c.m_context - 1, 16) + 2) * 16 : 0;
  if (e->ring == 0) return fail(-4, "Mimi decoder transformer needs a finite context");
  int mult = 8, idx = 1;
  const int nf = c.n_filters;
  CHK(pack_lin(e, &e->conv0, {{"mimi.decoder.model.0.conv.weight", "mimi.decoder.model.0.conv.bias", mult * nf}}, C, c.kernel_size));
  if (C != mult * nf && false) return fail(-4, "unexpected seanet dims");
  for (int i = 0; i < 3; ++i) {
    const int cin = mult * nf, cout = cin / 2, s = c.ratios[i], hid = cout / c.compress;
    std::string m = "mimi.decoder.model." + std::to_string(idx + 1);
    CHK(pack_lin(e, &e->convtr[i], {{m + ".convtr.weight", m + ".convtr.bias", s * cout}}, cin, 2, 1, cout, s));
    std::string r = "mimi.decoder.model." + std::to_string(idx + 2);
    CHK(pack_lin(e, &e->res_a[i], {{r + ".block.1.conv.weight", r + ".block.1.conv.bias", hid}}, cout, c.res_kernel_size));
    CHK(pack_lin(e, &e->res_b[i], {{r + ".block.3.conv.weight", r + ".block.3.conv.bias", cout}}, hid, 1));
    idx += 3;
    mult /= 2;
  }
  {
    std::string m = "mimi.decoder.model." + std::to_string(idx + 1);
    CHK(pack_lin(e, &e->conv_last, {{m + ".conv.weight", m + ".conv.bias", 1}}, nf, c.last_kernel_size));
  }
  CHK(dallocT(e, &e->zeros, 64));
  if (e->quant_flags & (PTTS_CODEC_BF16 | PTTS_CODEC_FP8)) {
    // bf16 images of every codec GEMM (reference modules: mimi_transformer.py:12-54, seanet.py:141-180, conv.py:93-163)
    for (int l = 0; l < c.m_layers; ++l) {
      const std::string q = "mimi.decoder_transformer.transformer.layers." + std::to_string(l);
      TrLayer &T = e->mm[l];
      CHK(pack_lin_h(e, &T.qkv, q + ".self_attn.in_proj.weight", 3 * C, C, 1, 0, 0, 0, q + ".norm1.weight"));
      CHK(pack_lin_h(e, &T.out, q + ".self_attn.out_proj.weight", C, C, 1));
      CHK(pack_lin_h(e, &T.ff1, q + ".linear1.weight", c.m_ff, C, 1, 0, 0, 0, q + ".norm2.weight"));
      CHK(pack_lin_h(e, &T.ff2, q + ".linear2.weight", C, c.m_ff, 1));
    }
    CHK(pack_lin_h(e, &e->conv0, "mimi.decoder.model.0.conv.weight", 8 * nf, C, c.kernel_size));
    int m2 = 8, i2 = 1;
    for (int i = 0; i < 3; ++i) {
      const int cin = m2 * nf, cout = cin / 2, sr = c.ratios[i], hid = cout / c.compress;
      CHK(pack_lin_h(e, &e->convtr[i], "mimi.decoder.model." + std::to_string(i2 + 1) + ".convtr.weight", sr * cout, cin, 2, 1, cout, sr));
      const std::string r = "mimi.decoder.model." + std::to_string(i2 + 2);
      CHK(pack_lin_h(e, &e->res_a[i], r + ".block.1.conv.weight", hid, cout, c.res_kernel_size));
      CHK(pack_lin_h(e, &e->res_b[i], r + ".block.3.conv.weight", cout, hid, 1));
      i2 += 3;
      m2 /= 2;
    }
    const std::string lc = "mimi.decoder.model." + std::to_string(i2 + 1);
    CHK(copy_vec(e, lc + ".conv.weight", (int64_t)nf * c.last_kernel_size, &e->conv_last_w));
    CHK(copy_vec(e, lc + ".conv.bias", 1, &e->conv_last_b, 4));
    e->codec_bf16 = true;
    e->mimi_bytes_h += (int64_t)C * c.ldim * 4;
  }
  if (e->quant_flags & PTTS_CODEC_FP8) CHK(build_fp8_codec(e));
  if (e->quant_flags & PTTS_CODEC_SPLIT) {
    std::vector<Lin *> ls = {&e->conv0};
    for (auto &T : e->mm) { ls.push_back(&T.qkv); ls.push_back(&T.out); ls.push_back(&T.ff1); ls.push_back(&T.ff2); }
    for (int i = 0; i < 3; ++i) { ls.push_back(&e->convtr[i]); ls.push_back(&e->res_a[i]); ls.push_back(&e->res_b[i]); }
    for (Lin *L : ls) {
      if (L->KF % 2) return fail(-4, "split-bf16 codec: every codec matrix needs an even number of 16-wide k-fragments");
      CHK(dalloc(e, &L->wsh, (size_t)L->NT * L->KF * 512));
      CHK(dalloc(e, &L->wsl, (size_t)L->NT * L->KF * 512));
      pack_weight_split(e->stream, L->w, L->wsh, L->wsl, L->NT, L->KF);
    }
    LAUNCHCHK();
    e->codec_split = true;
  }
  if (e->blob_dummy ? e->blob_has_encoder != 0
                    : (e->tmap.count("mimi.encoder.model.0.conv.weight") && e->tmap.count("flow_lm.speaker_proj_weight"))) {
    // reference mimi.py:96-119, seanet.py:63-104, resample.py:7-29, tts_model.py:379-388
    int em = 1, eidx = 1;
    CHK(pack_lin(e, &e->enc_conv0, {{"mimi.encoder.model.0.conv.weight", "mimi.encoder.model.0.conv.bias", nf}}, 16,
                 c.kernel_size, 0, 0, 0, "", "", 1));  // mono input padded to 16 channels
    for (int i = 0; i < 3; ++i) {
      const int dim = em * nf, r = c.ratios[2 - i], hid = dim / c.compress;
      std::string rb = "mimi.encoder.model." + std::to_string(eidx);
      CHK(pack_lin(e, &e->enc_res_a[i], {{rb + ".block.1.conv.weight", rb + ".block.1.conv.bias", hid}}, dim, c.res_kernel_size));
      CHK(pack_lin(e, &e->enc_res_b[i], {{rb + ".block.3.conv.weight", rb + ".block.3.conv.bias", dim}}, hid, 1));
      std::string dn = "mimi.encoder.model." + std::to_string(eidx + 2);
      CHK(pack_lin(e, &e->enc_down[i], {{dn + ".conv.weight", dn + ".conv.bias", 2 * dim}}, dim, 2 * r));
      e->enc_down[i].stride = r;
      eidx += 3;
      em *= 2;
    }
    std::string fn = "mimi.encoder.model." + std::to_string(eidx + 1);
    CHK(pack_lin(e, &e->enc_final, {{fn + ".conv.weight", fn + ".conv.bias", C}}, em * nf, c.last_kernel_size));
    e->enc_tr.resize(c.m_layers);
    for (int l = 0; l < c.m_layers; ++l)
      CHK(pack_tr_layer(e, &e->enc_tr[l], "mimi.encoder_transformer.transformer.layers." + std::to_string(l), C, c.m_ff, true));
    CHK(pack_lin(e, &e->enc_downsample, {{"mimi.downsample.conv.conv.weight", "", c.ldim}}, C, 2 * c.upsample_stride));
    e->enc_downsample.stride = c.upsample_stride;
    CHK(pack_lin(e, &e->speaker_proj, {{"flow_lm.speaker_proj_weight", "", D}}, c.ldim, 1));
    e->has_encoder = true;
  }
  e->mimi_bytes = (int64_t)C * c.ldim * 4 + e->conv0.bytes() + e->conv_last.bytes();
  for (auto &L : e->mm) e->mimi_bytes += L.qkv.bytes() + L.out.bytes() + L.ff1.bytes() + L.ff2.bytes();
  for (int i = 0; i < 3; ++i) e->mimi_bytes += e->convtr[i].bytes() + e->res_a[i].bytes() + e->res_b[i].bytes();
  HIPCHK(hipStreamSynchronize(e->stream));
  e->tmap.clear();
  e->n_build_allocs = e->allocs.size();
  return sync_host_tables(e);
}

// PTTS_CODEC_FP8: e4m3 images of the SEANet convolutions that run on the fp8 MFMA, and their scales (calibrate_fp8_codec)
static int build_fp8_codec(ptts_engine *e) {
  const ptts_config &c = e->cfg;
  const int nf = c.n_filters;
  hipStream_t st = e->stream;
  int mult = 8, idx = 1;
  e->mimi_bytes_f8 = e->mimi_bytes_h;
  for (int i = 0; i < 3; ++i) {
    const int cin = mult * nf, cout = cin / 2, sr = c.ratios[i], hid = cout / c.compress;
    if (cin % 32 || cout % 32 || hid % 32) return fail(-4, "fp8 codec path: channel counts must be multiples of 32");
    struct Job { Lin *L; std::string name; int N, C, ntaps, mode, cout, stride; };
    const std::string r = "mimi.decoder.model." + std::to_string(idx + 2);
    const Job jobs[3] = {{&e->convtr[i], "mimi.decoder.model." + std::to_string(idx + 1) + ".convtr.weight", sr * cout, cin, 2, 1, cout, sr},
                         {&e->res_a[i], r + ".block.1.conv.weight", hid, cout, c.res_kernel_size, 0, 0, 0},
                         {&e->res_b[i], r + ".block.3.conv.weight", cout, hid, 1, 0, 0, 0}};
    for (const Job &j : jobs) {
      int err = 0;
      const ptts_tensor *t = find_tensor(e, j.name, -1, &err);
      if (!t) return err;
      const size_t bytes = (size_t)j.L->NT * (j.C / 32) * j.ntaps * 512;
      CHK(dalloc(e, &j.L->wf8, bytes));
      CHK(dallocT(e, &j.L->wscale8, (size_t)j.L->NT * 16));
      pack_weight_f8(st, t->d_data, j.L->wf8, j.L->wscale8, j.N, j.C, j.ntaps, j.mode, j.cout, j.stride);
      LAUNCHCHK();
      e->mimi_bytes_f8 += (int64_t)bytes - 2 * (int64_t)bytes;  // e4m3 instead of bf16 for this matrix
    }
    idx += 3;
    mult /= 2;
  }
  CHK(dallocT(e, &e->d_f8s, 16));
  CHK(calibrate_fp8_codec(e));
  e->codec_fp8 = true;
  return 0;
}

// host mirrors of small device tables (after build_engine and again after a packed file has replaced the device images)
static int sync_host_tables(ptts_engine *e) {
  if (e->codec_fp8) {
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(e->f8s, e->d_f8s, sizeof(e->f8s), hipMemcpyDeviceToHost));
    for (float &v : e->f8s)
      if (!(v > 0.f)) v = 1.0f;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Packed-engine files (SURVEY 8(f).4 "offline packer"): everything build_engine leaves on the device - weights in MFMA
// fragment order, int8 / bf16 images, LayerNorm-fold vectors, small tables - as one file, so a deployment neither
// needs the fp32 checkpoint on the device nor re-packs / re-quantises at every start (reference load-time hook:
// quantization.py:60-88).  Layout: header, sizes, then the allocations in build order, each padded to 256 bytes.
struct PackHeader {
  char magic[8];
  int32_t abi, tune_version;
  ptts_config cfg;
  int32_t quant_flags, has_encoder;
  int64_t n_allocs;
};
static const char kPackMagic[8] = {'P', 'T', 'T', 'S', 'P', 'K', '1', 0};

extern "C" int ptts_engine_save(ptts_engine *e, const char *path) {
  if (!e || !path) return fail(-1, "null argument");
  ENGINE_LOCK(e);
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipDeviceSynchronize());
  FILE *f = fopen(path, "wb");
  if (!f) return fail(-1, std::string("cannot open ") + path);
  PackHeader h;
  memset(&h, 0, sizeof h);
  memcpy(h.magic, kPackMagic, 8);
  h.abi = PTTS_ABI_VERSION; h.tune_version = ptts_tune_version(); h.cfg = e->cfg; h.quant_flags = e->quant_flags;
  h.has_encoder = e->has_encoder ? 1 : 0; h.n_allocs = (int64_t)e->n_build_allocs;
  bool ok = fwrite(&h, sizeof h, 1, f) == 1;
  std::vector<int64_t> sizes;
  for (size_t i = 0; i < e->n_build_allocs; ++i) sizes.push_back((int64_t)e->alloc_bytes[e->allocs[i]]);
  ok = ok && fwrite(sizes.data(), 8, sizes.size(), f) == sizes.size();
  std::vector<char> buf;
  for (size_t i = 0; i < e->n_build_allocs && ok; ++i) {
    const size_t n = (size_t)sizes[i], padded = (n + 255) / 256 * 256;
    buf.assign(padded, 0);
    if (hipMemcpy(buf.data(), e->allocs[i], n, hipMemcpyDeviceToHost) != hipSuccess) { ok = false; break; }
    ok = fwrite(buf.data(), 1, padded, f) == padded;
  }
  ok = (fclose(f) == 0) && ok;
  return ok ? 0 : fail(-2, std::string("writing ") + path + " failed");
}

extern "C" int ptts_create_from_file(const char *path, int32_t device, ptts_engine **out) {
  if (!path || !out) return fail(-1, "null argument");
  FILE *f = fopen(path, "rb");
  if (!f) return fail(-1, std::string("cannot open ") + path);
  PackHeader h;
  if (fread(&h, sizeof h, 1, f) != 1 || memcmp(h.magic, kPackMagic, 8) != 0 || h.abi != PTTS_ABI_VERSION || h.n_allocs < 1 ||
      h.n_allocs > 100000) {
    fclose(f);
    return fail(-3, std::string(path) + " is not a packed engine of this library version");
  }
  std::vector<int64_t> sizes((size_t)h.n_allocs);
  if (fread(sizes.data(), 8, sizes.size(), f) != sizes.size()) { fclose(f); return fail(-3, "truncated packed engine (sizes)"); }
  if (h.quant_flags & ~(PTTS_QUANT_ATTENTION | PTTS_QUANT_FFN | PTTS_CODEC_BF16 | PTTS_CODEC_FP8 | PTTS_LM_BF16 | PTTS_CODEC_SPLIT)) {
    fclose(f);
    return fail(-3, "packed engine carries unknown weight-format flags");
  }
  if (seanet_check(h.cfg) < 0) { fclose(f); return -4; }
  if (hipSetDevice(device) != hipSuccess) { fclose(f); return fail(-2, "hipSetDevice"); }
  // the largest checkpoint tensor any packing kernel reads (a zero stand-in: the images it produces are overwritten)
  const ptts_config &c = h.cfg;
  const int64_t big = std::max<int64_t>({(int64_t)c.ff_dim * c.d_model, (int64_t)3 * c.d_model * c.d_model, (int64_t)c.m_ff * c.m_dim,
                                         (int64_t)c.m_dim * c.m_dim * c.kernel_size, (int64_t)16 * c.n_filters * c.n_filters * 16,
                                         (int64_t)3 * c.flow_dim * c.flow_dim, (int64_t)c.m_dim * c.ldim * 2 * c.upsample_stride}) * 2;
  float *zeros = nullptr;
  if (hipMalloc((void **)&zeros, (size_t)big * 4) != hipSuccess || hipMemset(zeros, 0, (size_t)big * 4) != hipSuccess) {
    (void)hipGetLastError();
    fclose(f);
    return fail(-2, "out of device memory");
  }
  ptts_tensor dummy{"<packed>", zeros, -1};
  ptts_engine *e = new ptts_engine();
  e->cfg = h.cfg;
  e->quant_flags = h.quant_flags;
  e->blob_dummy = &dummy;
  e->blob_has_encoder = h.has_encoder;
  int rc = init_engine_options(e, device);
  if (rc == 0) rc = build_engine(e, nullptr, 0);
  e->blob_dummy = nullptr;
  std::string msg = g_err;
  if (rc == 0 && (int64_t)e->n_build_allocs != h.n_allocs) { rc = -3; msg = "packed engine does not match this build's layout"; }
  std::vector<char> buf;
  for (size_t i = 0; rc == 0 && i < e->n_build_allocs; ++i) {
    const size_t n = (size_t)sizes[i], padded = (n + 255) / 256 * 256;
    if (e->alloc_bytes[e->allocs[i]] != n) { rc = -3; msg = "packed engine does not match this build's layout (allocation size)"; break; }
    buf.resize(padded);
    if (fread(buf.data(), 1, padded, f) != padded) { rc = -3; msg = "truncated packed engine"; break; }
    if (hipMemcpy(e->allocs[i], buf.data(), n, hipMemcpyHostToDevice) != hipSuccess) { rc = -2; msg = "hipMemcpy"; break; }
  }
  fclose(f);
  (void)hipFree(zeros);
  if (rc == 0 && sync_host_tables(e) < 0) { rc = -2; msg = g_err; }
  if (rc < 0) {
    ptts_destroy(e);
    return fail(rc, msg);
  }
  *out = e;
  return 0;
}

extern "C" void ptts_destroy(ptts_engine *e) {
  if (!e) return;
  hipSetDevice(e->device);
  hipDeviceSynchronize();
  for (void *p : e->allocs) hipFree(p);
  for (void *p : e->enc_keep) hipFree(p);
  if (e->ev0) hipEventDestroy(e->ev0);
  if (e->ev1) hipEventDestroy(e->ev1);
  if (e->stream) hipStreamDestroy(e->stream);
  unbind_dispatch(e);
  if (g_prof == &e->prof) g_prof = nullptr;
  for (auto &r : e->prof.recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  delete e->tuner;
  delete e;
}

hipStream_t S(ptts_engine *e, void *stream) { return stream ? (hipStream_t)stream : e->stream; }

// time-embedding constant for a given LSD schedule (reference mlp.py:203-206): computed once on device
static int prepare_lsd(ptts_engine *e, int steps) {
  if (e->tcomb.count(steps)) return 0;
  bind_engine(e);
  if (steps < 1 || steps > 64) return fail(-1, "lsd_decode_steps out of range");
  const int FD = e->cfg.flow_dim;
  float *tab;
  AllocScope alloc_scope(e->stream);
  CHK(dallocT(e, &tab, (size_t)steps * FD));
  hipStream_t st = e->stream;
  float *efm = e->te_scratch, *h = efm + 16 * 1024, *h0 = h + 16 * 1024, *h1 = h0 + 16 * 1024;
  for (int i = 0; i < steps; ++i) {
    const float tv[2] = {(float)((double)i / steps), (float)((double)(i + 1) / steps)};
    float *ho[2] = {h0, h1};
    for (int k = 0; k < 2; ++k) {
      timestep_embed_kernel<<<1, 256, 0, st>>>(e->te_freqs[k], tv[k], efm, 128);
      GemmArgs a = mk_gemm(e->te_l0[k], efm, 16, 1, 1);
      a.act = ACT_SILU; a.Y = h; a.YF = FD / 16;
      launch_gemm(st, a, PRE_NONE);
      a = mk_gemm(e->te_l2[k], h, FD / 16, 1, 1);
      a.Y = ho[k]; a.YF = FD / 16;
      launch_gemm(st, a, PRE_NONE);
    }
    tcomb_kernel<<<1, 64, 0, st>>>(h0, h1, e->te_alpha[0], e->te_alpha[1], tab + (size_t)i * FD, FD);
  }
  HIPCHK(hipStreamSynchronize(st));
  LAUNCHCHK();
  e->tcomb[steps] = tab;
  return 0;
}

// the tables of schedules 1..K in one buffer (per-row LSD schedules): copies of tcomb[N], so bitwise the same values
static int prepare_lsd_pack(ptts_engine *e, int K) {
  if (e->tpack.count(K)) return 0;
  for (int n = 1; n <= K; ++n) CHK(prepare_lsd(e, n));
  const size_t FD = e->cfg.flow_dim;
  float *tab;
  AllocScope alloc_scope(e->stream);
  CHK(dallocT(e, &tab, (size_t)K * (K + 1) / 2 * FD));
  for (int n = 1; n <= K; ++n)
    HIPCHK(hipMemcpyAsync(tab + (size_t)n * (n - 1) / 2 * FD, e->tcomb[n], (size_t)n * FD * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->tpack[K] = tab;
  return 0;
}

// ------------------------------------------------------------------------------------------------
// FlowLM state
static int alloc_scratch(ptts_engine *e, Scratch *s, int B, int Tq, int D, int H, int FF, int cap) {
  const int M = B * Tq;
  s->MT = cdiv(M, 16);
  s->QB = cdiv(Tq, 16);
  const size_t rowt = (size_t)s->MT * 256;
  CHK(dallocT(nullptr, &s->x, rowt * (D / 16)));
  CHK(dallocT(nullptr, &s->h, rowt * (D / 16)));
  CHK(dallocT(nullptr, &s->ao, rowt * (D / 16)));
  CHK(dallocT(nullptr, &s->ff, rowt * (FF / 16)));
  CHK(dallocT(nullptr, &s->q, (size_t)B * H * s->QB * 4 * 256));
  CHK(dallocT(nullptr, &s->rope, (size_t)s->MT * 16 * 64));
  s->splits_cap = attn_splits(B * H * s->QB, cdiv(cap, 16));
  CHK(dallocT(nullptr, &s->part, (size_t)B * H * s->QB * s->splits_cap * 16 * ATT_PSTRIDE));
  return 0;
}
static void free_scratch(Scratch *s) {
  hipFree(s->x); hipFree(s->h); hipFree(s->ao); hipFree(s->ff); hipFree(s->q); hipFree(s->part); hipFree(s->rope);
  *s = Scratch();
}

static int build_lm_state(ptts_engine *e, ptts_lm_state *s);
static int ensure_flow(ptts_engine *e, ptts_lm_state *s, int steps, hipStream_t st);

extern "C" int ptts_lm_state_create(ptts_engine *e, int32_t B, int32_t t_cap, ptts_lm_state **out) {
  if (!e || !out || B < 1 || t_cap < 1) return fail(-1, "bad argument");
  ENGINE_LOCK(e);
  HIPCHK(hipSetDevice(e->device));
  ptts_lm_state *s = new ptts_lm_state();
  s->e = e;
  s->B = B;
  s->cap = cdiv(t_cap, 16) * 16;
  s->MT = cdiv(B, 16);
  const int rc = build_lm_state(e, s);
  if (rc < 0) {  // typically out of device memory for the KV cache: free the partial state
    const std::string msg = g_err;
    ptts_lm_state_destroy(s);
    return fail(rc, msg);
  }
  *out = s;
  return 0;
}

static int build_lm_state(ptts_engine *e, ptts_lm_state *s) {
  const ptts_config &c = e->cfg;
  const int B = s->B;
  AllocScope alloc_scope(e->stream);
  CHK(dallocT(nullptr, &s->kv, (size_t)c.num_layers * 2 * s->kv_plane()));
  CHK(dallocT(nullptr, &s->offset, B));
  CHK(dallocT(nullptr, &s->qlen, B));
  s->h_off.assign(B, 0);
  CHK(dalloc(nullptr, (void **)&s->d_pre, (size_t)B * sizeof(KvPrefix)));
  s->h_pre.assign(B, KvPrefix{nullptr, 0, 0});
  s->pre_owner.assign(B, nullptr);
  CHK(alloc_scratch(e, &s->dec, B, 1, c.d_model, c.num_heads, c.ff_dim, s->cap));
  const size_t rt = (size_t)s->MT * 256;
  const int FD = c.flow_dim;
  CHK(dallocT(nullptr, &s->xlat, rt * (c.ldim / 16)));
  CHK(dallocT(nullptr, &s->latfm, rt * (c.ldim / 16)));
  CHK(dallocT(nullptr, &s->c, rt * (c.d_model / 16)));
  CHK(dallocT(nullptr, &s->ce, rt * (FD / 16)));
  CHK(dallocT(nullptr, &s->ferr, 1));
  CHK(dallocT(nullptr, &s->fx, rt * (FD / 16)));
  CHK(dallocT(nullptr, &s->fh, rt * (FD / 16)));
  CHK(dallocT(nullptr, &s->f1, rt * (FD / 16)));
  CHK(dallocT(nullptr, &s->fstat, (size_t)s->MT * (FD / 16) * 32));
  CHK(dallocT(nullptr, &s->lat, (size_t)B * c.ldim));
  CHK(dallocT(nullptr, &s->lat_prev, (size_t)B * c.ldim));
  CHK(dallocT(nullptr, &s->eos_logit, B));
  CHK(dallocT(nullptr, &s->is_eos, B));
  CHK(dallocT(nullptr, &s->rng_ctr, 1));
  CHK(dallocT(nullptr, &s->active, B));
  CHK(dallocT(nullptr, &s->samp_on, B));
  CHK(dallocT(nullptr, &s->samp_noise, B));
  CHK(dallocT(nullptr, &s->samp_eos, B));
  CHK(dallocT(nullptr, &s->seed_on, B));
  CHK(dallocT(nullptr, &s->seed_val, B));
  CHK(dallocT(nullptr, &s->seed_ctr, B));
  CHK(dallocT(nullptr, &s->lsd_n, B));
  s->h_active.assign(B, 1);
  set_int_kernel<<<cdiv(B, 256), 256, 0, e->stream>>>(s->active, B, 1);
  set_int_kernel<<<cdiv(B, 256), 256, 0, e->stream>>>(s->lsd_n, B, 0);
  fill_kernel<<<cdiv(B * c.ldim, 256), 256, 0, e->stream>>>(s->lat_prev, (long)B * c.ldim, NAN);
  HIPCHK(hipStreamSynchronize(e->stream));
  CHK(ensure_flow(e, s, 1, e->stream));  // AdaLN modulation buffer + flow-cluster exchange slots for lsd_decode_steps = 1
  return 0;
}

// ---- shared prefixes: bookkeeping (host side; the device table is updated by set_prefix_kernel on the caller's stream)
static void lm_state_free(ptts_lm_state *s) {
  hipFree(s->kv); hipFree(s->offset); hipFree(s->qlen); hipFree(s->d_pre);
  free_scratch(&s->dec);
  if (s->pre.x) free_scratch(&s->pre);
  hipFree(s->xlat); hipFree(s->latfm); hipFree(s->c); hipFree(s->ce); hipFree(s->mod); hipFree(s->fx);
  hipFree(s->fh); hipFree(s->f1); hipFree(s->lat); hipFree(s->lat_prev); hipFree(s->eos_logit); hipFree(s->is_eos); hipFree(s->rng_ctr); hipFree(s->active); hipFree(s->fstat);
  hipFree(s->samp_on); hipFree(s->samp_noise); hipFree(s->samp_eos); hipFree(s->lsd_n);
  hipFree(s->seed_on); hipFree(s->seed_val); hipFree(s->seed_ctr);
  hipFree(s->fexch); hipFree(s->fflags); hipFree(s->ferr); hipFree(s->lexch); hipFree(s->lflags);
  delete s;
}
static void prefix_release(ptts_lm_state *s, int row) {  // the row stops reading its owner's cache
  ptts_lm_state *o = s->pre_owner[row];
  if (!o) return;
  s->pre_owner[row] = nullptr;
  s->h_pre[row] = KvPrefix{nullptr, 0, 0};
  s->n_pre -= 1;
  o->borrowers -= 1;
  if (o->zombie && o->borrowers == 0) {  // its destroy was deferred until now; the GPU may still be reading it
    hipDeviceSynchronize();
    lm_state_free(o);
  }
}
static void prefix_borrow(ptts_lm_state *s, int row, ptts_lm_state *owner, int len) {
  if (s->pre_owner[row] == owner && s->h_pre[row].len == len) return;
  owner->borrowers += 1;  // before the release: re-borrowing from the same (zombie) owner must not free it in between
  prefix_release(s, row);
  s->pre_owner[row] = owner;
  s->h_pre[row] = KvPrefix{owner->kv, owner->cap, len};
  s->n_pre += 1;
}
// a state whose cache other states read as their prefix must not have it rewritten under them
static int refuse_if_lent(const ptts_lm_state *s, const char *what) {
  if (s->borrowers > 0) return fail(-1, std::string(what) + ": this state's cache is the shared prefix of " + std::to_string(s->borrowers) +
                                           " sequence(s) cloned from it; destroy or re-clone them first");
  return 0;
}

extern "C" void ptts_lm_state_destroy(ptts_lm_state *s) {
  if (!s) return;
  ENGINE_LOCK(s->e);  // the borrow counts of OTHER states (prefix owners) change here
  hipSetDevice(s->e->device);
  hipDeviceSynchronize();
  for (int b = 0; b < (int)s->pre_owner.size(); ++b) prefix_release(s, b);  // (empty after a failed creation)
  if (s->borrowers > 0) {  // clones still read this cache: the memory goes when the last of them lets go
    s->zombie = true;
    return;
  }
  lm_state_free(s);
}

extern "C" int ptts_lm_state_reset(ptts_lm_state *s, void *stream) {
  hipStream_t st = S(s->e, stream);
  ENGINE_LOCK(s->e);
  CHK(refuse_if_lent(s, "reset"));
  for (int b = 0; b < s->B; ++b) prefix_release(s, b);
  set_prefix_kernel<<<cdiv(s->B, 256), 256, 0, st>>>(s->d_pre, s->B, nullptr, 0, 0);
  set_int_kernel<<<cdiv(s->B, 256), 256, 0, st>>>(s->offset, s->B, 0);
  fill_kernel<<<cdiv(s->B * s->e->cfg.ldim, 256), 256, 0, st>>>(s->lat_prev, (long)s->B * s->e->cfg.ldim, NAN);
  std::fill(s->h_off.begin(), s->h_off.end(), 0);
  std::fill(s->h_active.begin(), s->h_active.end(), 1);
  set_int_kernel<<<cdiv(s->B, 256), 256, 0, st>>>(s->active, s->B, 1);
  set_int_kernel<<<cdiv(s->B, 256), 256, 0, st>>>(s->samp_on, s->B, 0);
  set_int_kernel<<<cdiv(s->B, 256), 256, 0, st>>>(s->lsd_n, s->B, 0);
  set_int_kernel<<<cdiv(s->B, 256), 256, 0, st>>>(s->seed_on, s->B, 0);
  LAUNCHCHK();
  return 0;
}

extern "C" int ptts_lm_state_import(ptts_lm_state *s, int32_t layer, const float *d_cache, int32_t src_batch,
                                    int32_t t, void *stream) {
  const ptts_config &c = s->e->cfg;
  if (layer < 0 || layer >= c.num_layers) return fail(-1, "layer out of range");
  if (t > s->cap) return fail(-5, "import: t exceeds cache capacity");
  if (src_batch != 1 && src_batch != s->B) return fail(-1, "import: src_batch must be 1 or B");
  hipStream_t st = S(s->e, stream);
  ENGINE_LOCK(s->e);
  CHK(refuse_if_lent(s, "import"));
  if (s->n_pre > 0) {  // the imported rows are complete copies
    for (int b = 0; b < s->B; ++b) prefix_release(s, b);
    set_prefix_kernel<<<cdiv(s->B, 256), 256, 0, st>>>(s->d_pre, s->B, nullptr, 0, 0);
  }
  if (t > 0) {
    long total = 2L * s->B * t * c.num_heads * 16;
    kv_import_kernel<<<cdiv(total, 256), 256, 0, st>>>(d_cache, s->K(layer), s->V(layer), s->B, src_batch, t,
                                                        c.num_heads, s->cap);
  }
  set_int_kernel<<<cdiv(s->B, 256), 256, 0, st>>>(s->offset, s->B, t);
  std::fill(s->h_off.begin(), s->h_off.end(), t);
  LAUNCHCHK();
  return 0;
}

extern "C" int ptts_lm_state_export(ptts_lm_state *s, int32_t layer, float *d_cache, int32_t t, void *stream) {
  const ptts_config &c = s->e->cfg;
  if (layer < 0 || layer >= c.num_layers) return fail(-1, "layer out of range");
  if (t > s->cap) return fail(-5, "export: t exceeds cache capacity");
  hipStream_t st = S(s->e, stream);
  long total = 2L * s->B * t * c.num_heads * 16;
  if (total) kv_export_kernel<<<cdiv(total, 256), 256, 0, st>>>(d_cache, s->K(layer), s->V(layer), s->B, t, c.num_heads, s->cap,
                                                                 s->n_pre > 0 ? s->d_pre : nullptr, layer);
  LAUNCHCHK();
  return 0;
}

// KV rows of (src, src_row) -> (dst, row).  With "share_prefix" the destination row BORROWS the leading positions instead
// of copying them: from src itself when src is a one-sequence state (a cached voice state: every clone of it reads the same
// [0, T & ~15) keys, so the clones' attention fetches them once through L2 instead of once per row), or from the state
// src's row already borrows from.  Only the private positions behind the prefix are copied.  Without the option a
// borrowed prefix is materialised into dst.  Host table only; the caller updates dst->d_pre.
static int kv_clone_row(ptts_lm_state *dst, int row, const ptts_lm_state *src, int src_row, int T, hipStream_t st) {
  const ptts_config &c = dst->e->cfg;
  const int planes = c.num_layers * 2, H = c.num_heads;
  ptts_lm_state *owner = src->pre_owner[src_row];
  int plen = owner ? src->h_pre[src_row].len : 0;
  if (plen > T) plen = 0, owner = nullptr;  // cannot happen (offsets only grow past a prefix); a full copy is always right
  bool share = dst->e->opt_share_prefix && !dst->e->opt_lm_cluster && dst != src;  // (the single-launch stack reads own caches only)
  if (share && !owner && src->B == 1 && !src->zombie && T >= 16) owner = const_cast<ptts_lm_state *>(src), plen = T & ~15;
  if (!owner || owner == dst) share = false;
  int t0 = 0;
  if (share) {
    prefix_borrow(dst, row, owner, plen);
    t0 = owner == src ? plen : src->h_pre[src_row].len;
  } else {
    prefix_release(dst, row);
    if (src->pre_owner[src_row]) {  // materialise the part src only borrows
      const ptts_lm_state *o = src->pre_owner[src_row];
      t0 = src->h_pre[src_row].len;
      const long total = (long)planes * H * t0 * 16;
      kv_copy_row_kernel<<<cdiv(total, 256), 256, 0, st>>>(dst->kv, o->kv, planes, H, t0, o->cap, dst->cap, dst->B, row, o->B, 0, 0);
    }
  }
  if (T > t0) {
    const long total = (long)planes * H * (T - t0) * 16;
    kv_copy_row_kernel<<<cdiv(total, 256), 256, 0, st>>>(dst->kv, src->kv, planes, H, T - t0, src->cap, dst->cap, dst->B, row, src->B, src_row, t0);
  }
  return 0;
}
static int upload_prefixes(ptts_lm_state *s, hipStream_t st) {
  bool uniform = true;
  for (int b = 1; b < s->B; ++b) uniform &= s->h_pre[b].kv == s->h_pre[0].kv && s->h_pre[b].len == s->h_pre[0].len && s->h_pre[b].cap == s->h_pre[0].cap;
  if (uniform) {
    set_prefix_kernel<<<cdiv(s->B, 256), 256, 0, st>>>(s->d_pre, s->B, s->h_pre[0].kv, s->h_pre[0].cap, s->h_pre[0].len);
  } else {
    HIPCHK(hipMemcpyAsync(s->d_pre, s->h_pre.data(), s->B * sizeof(KvPrefix), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // pageable host memory
  }
  return 0;
}

extern "C" int ptts_lm_state_copy(ptts_lm_state *dst, const ptts_lm_state *src, void *stream) {
  if (!dst || !src) return fail(-1, "null state");
  if (dst->e != src->e) return fail(-1, "states belong to different engines");
  if (src->B != 1 && src->B != dst->B) return fail(-1, "copy: src batch must be 1 or equal");
  if (dst == src) return 0;
  const ptts_config &c = dst->e->cfg;
  hipStream_t st = S(dst->e, stream);
  ENGINE_LOCK(dst->e);
  CHK(refuse_if_lent(dst, "copy"));
  const int T = *std::max_element(src->h_off.begin(), src->h_off.end());
  if (T > dst->cap) return fail(-5, "copy: destination capacity too small");
  const bool had_pre = dst->n_pre > 0;
  const bool plain = src->n_pre == 0 && !(dst->e->opt_share_prefix && !dst->e->opt_lm_cluster && src->B == 1 && T >= 16);
  if (plain) {
    // full copies: ONE kernel over the T written positions of every row (not the whole capacity: a batch-64 clone of 126
    // positions in a 284-position cache moved 1.8 GB instead of 0.8 GB), whatever the two capacities are
    for (int b = 0; b < dst->B; ++b) prefix_release(dst, b);
    if (T > 0) {
      const long total = (long)c.num_layers * 2 * dst->B * c.num_heads * T * 16;
      kv_copy_t_kernel<<<cdiv(total, 256), 256, 0, st>>>(dst->kv, src->kv, c.num_layers * 2, dst->B, src->B, c.num_heads, T, src->cap, dst->cap);
    }
  } else if (src->B == 1 && !src->pre_owner[0] && !src->zombie && dst->e->opt_share_prefix && !dst->e->opt_lm_cluster && T >= 16) {
    // the common case, a plain voice state cloned into every row: all rows borrow its first T & ~15 positions and ONE
    // kernel copies the (< 16) positions behind them
    ptts_lm_state *owner = const_cast<ptts_lm_state *>(src);
    const int plen = T & ~15;
    for (int b = 0; b < dst->B; ++b) prefix_borrow(dst, b, owner, plen);
    if (T > plen) {
      const long total = (long)c.num_layers * 2 * dst->B * c.num_heads * (T - plen) * 16;
      kv_copy_t_kernel<<<cdiv(total, 256), 256, 0, st>>>(dst->kv, src->kv, c.num_layers * 2, dst->B, 1, c.num_heads, T - plen, src->cap, dst->cap, plen);
    }
  } else {
    // row by row: one copy kernel per destination row for the positions it does not share
    for (int b = 0; b < dst->B; ++b) {
      const int sb = src->B == 1 ? 0 : b;
      CHK(kv_clone_row(dst, b, src, sb, src->h_off[sb], st));
    }
  }
  if (had_pre || dst->n_pre > 0) CHK(upload_prefixes(dst, st));
  for (int b = 0; b < dst->B; ++b) dst->h_off[b] = src->h_off[src->B == 1 ? 0 : b];
  if (*std::min_element(dst->h_off.begin(), dst->h_off.end()) == T) {
    set_int_kernel<<<cdiv(dst->B, 256), 256, 0, st>>>(dst->offset, dst->B, T);
  } else {
    HIPCHK(hipMemcpyAsync(dst->offset, dst->h_off.data(), dst->B * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // h_off.data() is pageable host memory
  }
  // a cloned state starts a new generation: next input is BOS (NaN), reference tts_model.py:748-753
  fill_kernel<<<cdiv(dst->B * c.ldim, 256), 256, 0, st>>>(dst->lat_prev, (long)dst->B * c.ldim, NAN);
  LAUNCHCHK();
  return 0;
}

// Row `row` of dst <- the single sequence of src (B = 1): KV rows, offset and a BOS pending input.  Lets a batch
// be assembled from utterances prefilled one by one with different prompt lengths (per-row offsets).
extern "C" int ptts_lm_state_copy_row(ptts_lm_state *dst, int32_t row, const ptts_lm_state *src, void *stream) {
  if (src && src->B != 1) return fail(-1, "copy_row: src must have batch 1 (use ptts_lm_state_copy_row_from)");
  return ptts_lm_state_copy_row_from(dst, row, src, 0, stream);
}
extern "C" int ptts_lm_state_copy_row_from(ptts_lm_state *dst, int32_t row, const ptts_lm_state *src, int32_t src_row, void *stream) {
  if (!dst || !src) return fail(-1, "null state");
  if (dst->e != src->e) return fail(-1, "states belong to different engines");
  if (src_row < 0 || src_row >= src->B || row < 0 || row >= dst->B) return fail(-1, "copy_row: row out of range");
  if (dst == src) return fail(-1, "copy_row: source and destination are the same state");
  const ptts_config &c = dst->e->cfg;
  hipStream_t st = S(dst->e, stream);
  HIPCHK(hipSetDevice(dst->e->device));
  ENGINE_LOCK(dst->e);
  CHK(refuse_if_lent(dst, "copy_row"));
  const int T = src->h_off[src_row];
  if (T > dst->cap) return fail(-5, "copy_row: destination capacity too small");
  const bool had_pre = dst->pre_owner[row] != nullptr;
  CHK(kv_clone_row(dst, row, src, src_row, T, st));
  if (had_pre || dst->pre_owner[row]) {
    const KvPrefix &p = dst->h_pre[row];
    set_prefix_kernel<<<1, 64, 0, st>>>(dst->d_pre + row, 1, p.kv, p.cap, p.len);
  }
  dst->h_off[row] = T;
  dst->h_active[row] = 1;
  set_int_kernel<<<1, 64, 0, st>>>(dst->active + row, 1, 1);
  set_int_kernel<<<1, 64, 0, st>>>(dst->offset + row, 1, T);
  fill_kernel<<<cdiv(c.ldim, 256), 256, 0, st>>>(dst->lat_prev + (size_t)row * c.ldim, (long)c.ldim, NAN);
  LAUNCHCHK();
  return 0;
}

// Continuous batching: park / unpark one row.  A parked row still flows through the batched kernels (its
// outputs are ignored by the caller) but its position is pinned to 0, so it never exhausts the KV capacity
// and its attention reads one key.
extern "C" int ptts_lm_state_set_row_active(ptts_lm_state *s, int32_t row, int32_t active, void *stream) {
  if (!s || row < 0 || row >= s->B) return fail(-1, "set_row_active: row out of range");
  hipStream_t st = S(s->e, stream);
  ENGINE_LOCK(s->e);
  s->h_active[row] = active ? 1 : 0;
  set_int_kernel<<<1, 64, 0, st>>>(s->active + row, 1, active ? 1 : 0);
  if (!active) {
    s->h_off[row] = 0;
    set_int_kernel<<<1, 64, 0, st>>>(s->offset + row, 1, 0);
    if (s->pre_owner[row]) {  // a parked row reads key 0 of its own cache only
      prefix_release(s, row);
      set_prefix_kernel<<<1, 64, 0, st>>>(s->d_pre + row, 1, nullptr, 0, 0);
    }
  }
  LAUNCHCHK();
  return 0;
}

extern "C" int ptts_lm_state_offsets(ptts_lm_state *s, int32_t *h, void *stream) {
  hipStream_t st = S(s->e, stream);
  HIPCHK(hipMemcpyAsync(h, s->offset, s->B * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" const float *ptts_lm_latent_ptr(ptts_lm_state *s) { return s->lat_prev; }

extern "C" int ptts_lm_set_noise(ptts_lm_state *s, float temp, uint64_t seed) {
  if (temp < 0) return fail(-1, "temperature must be >= 0");
  s->rng_std = std::sqrt(temp);  // std = temp ** 0.5 (reference flow_lm.py:132)
  s->rng_seed = seed;
  return 0;
}

static __global__ void set_row_sampling_kernel(int *on, f32x4 *noise, float *eos, int v_on, f32x4 v_noise, float v_eos) {
  if (threadIdx.x == 0) {
    *on = v_on;
    *noise = v_noise;
    *eos = v_eos;
  }
}

extern "C" int ptts_lm_state_set_row_sampling(ptts_lm_state *s, int32_t row, float temp, float noise_clamp,
                                              float eos_threshold, void *stream) {
  if (!s || row < 0 || row >= s->B) return fail(-1, "set_row_sampling: row out of range");
  if (!std::isfinite(temp) || temp < 0) return fail(-1, "set_row_sampling: temperature must be finite and >= 0");
  if (std::isnan(noise_clamp) || std::isnan(eos_threshold)) return fail(-1, "set_row_sampling: NaN clamp or EOS threshold");
  const float sd = std::sqrt(temp);  // as ptts_lm_set_noise: bitwise the same draws at the same temperature
  f32x4 p = {sd, 0.f, 0.f, 0.f};
  if (noise_clamp > 0 && sd > 0) {
    // [2 Phi(-c / std) - 1, 2 Phi(c / std) - 1] = [-a, a] with a = erf(c / (std sqrt 2))
    const float a = (float)std::erf((double)noise_clamp / ((double)sd * 1.4142135623730950488));
    p = (f32x4){sd, noise_clamp, -a, 2.f * a};
  }
  hipStream_t st = S(s->e, stream);
  ENGINE_LOCK(s->e);
  set_row_sampling_kernel<<<1, 64, 0, st>>>(s->samp_on + row, s->samp_noise + row, s->samp_eos + row, 1, p, eos_threshold);
  LAUNCHCHK();
  return 0;
}

extern "C" int ptts_lm_state_clear_row_sampling(ptts_lm_state *s, int32_t row, void *stream) {
  if (!s || row < 0 || row >= s->B) return fail(-1, "clear_row_sampling: row out of range");
  hipStream_t st = S(s->e, stream);
  ENGINE_LOCK(s->e);
  set_int_kernel<<<1, 64, 0, st>>>(s->samp_on + row, 1, 0);
  LAUNCHCHK();
  return 0;
}

static __global__ void set_row_seed_kernel(int *on, unsigned long long *seed, int *ctr, int v_on, unsigned long long v_seed) {
  if (threadIdx.x == 0) {
    *on = v_on;
    *seed = v_seed;
    *ctr = 0;
  }
}

extern "C" int ptts_lm_state_set_row_seed(ptts_lm_state *s, int32_t row, uint64_t seed, void *stream) {
  if (!s || row < 0 || row >= s->B) return fail(-1, "set_row_seed: row out of range");
  hipStream_t st = S(s->e, stream);
  ENGINE_LOCK(s->e);
  set_row_seed_kernel<<<1, 64, 0, st>>>(s->seed_on + row, s->seed_val + row, s->seed_ctr + row, 1, (unsigned long long)seed);
  LAUNCHCHK();
  return 0;
}

extern "C" int ptts_lm_state_clear_row_seed(ptts_lm_state *s, int32_t row, void *stream) {
  if (!s || row < 0 || row >= s->B) return fail(-1, "clear_row_seed: row out of range");
  hipStream_t st = S(s->e, stream);
  ENGINE_LOCK(s->e);
  set_int_kernel<<<1, 64, 0, st>>>(s->seed_on + row, 1, 0);
  LAUNCHCHK();
  return 0;
}

static int ensure_flow(ptts_engine *e, ptts_lm_state *s, int steps, hipStream_t st);

extern "C" int ptts_lm_state_reserve_row_lsd(ptts_lm_state *s, int32_t K, void *stream) {
  if (!s || K < 1 || K > 64) return fail(-1, "reserve_row_lsd: capacity must be in [1, 64]");
  ptts_engine *e = s->e;
  ENGINE_LOCK(e);
  HIPCHK(hipSetDevice(e->device));
  if (s->n_graphs > 0) return fail(-1, "reserve_row_lsd: the state has captured graphs (they hold its flow buffers): reserve before capturing");
  K = std::max(K, (int32_t)s->lsd_cap);  // never shrinks
  CHK(ensure_flow(e, s, K, S(e, stream)));
  CHK(prepare_lsd_pack(e, K));
  s->lsd_tab = e->tpack[K];
  s->lsd_cap = K;
  return 0;
}

// Per-state switch of the folded flow cluster (flow_cluster_mod_kernel): the exchange slots grow to FLOW_MOD_FRAGS
// fragments, so the buffers are re-allocated here and the switch cannot change under captured graphs
extern "C" int ptts_lm_state_set_flow_fold(ptts_lm_state *s, int32_t on, void *stream) {
  if (!s) return fail(-1, "set_flow_fold: null state");
  ptts_engine *e = s->e;
  ENGINE_LOCK(e);
  HIPCHK(hipSetDevice(e->device));
  if ((on != 0) == s->flow_fold) return 0;
  if (s->n_graphs > 0) return fail(-1, "set_flow_fold: the state has captured graphs (they hold its flow buffers): set it before capturing");
  const int steps = s->flow_steps;
  s->flow_fold = on != 0;
  s->flow_steps = 0;  // ensure_flow re-allocates the exchange at the new slot size
  return ensure_flow(e, s, std::max(1, steps), S(e, stream));
}

extern "C" int64_t ptts_flow_slot_offset(int32_t fdf, int32_t rt, int32_t nph, int32_t nf, int32_t grp, int32_t p, int32_t t,
                                         int32_t j, int32_t f) {
  return (int64_t)flow_slot(fdf, rt, nph, nf, grp, p, t, j, f);
}

extern "C" int32_t ptts_flow_mod_tiles(int32_t fdf, int32_t depth, int32_t ph, int32_t j, int32_t *n) {
  int nn = 0;
  const int t0 = flow_mod_tiles(fdf, depth, ph, j, &nn);
  if (n) *n = nn;
  return t0;
}

extern "C" int ptts_lm_state_set_row_lsd(ptts_lm_state *s, int32_t row, int32_t n, void *stream) {
  if (!s || row < 0 || row >= s->B) return fail(-1, "set_row_lsd: row out of range");
  if (s->lsd_cap < 1) return fail(-1, "set_row_lsd: the state has no per-row LSD capacity (ptts_lm_state_reserve_row_lsd)");
  if (n < 1 || n > s->lsd_cap) return fail(-1, "set_row_lsd: lsd_decode_steps must be in [1, " + std::to_string(s->lsd_cap) + "]");
  hipStream_t st = S(s->e, stream);
  ENGINE_LOCK(s->e);
  set_int_kernel<<<1, 64, 0, st>>>(s->lsd_n + row, 1, n);
  LAUNCHCHK();
  return 0;
}

extern "C" int ptts_lm_state_clear_row_lsd(ptts_lm_state *s, int32_t row, void *stream) {
  if (!s || row < 0 || row >= s->B) return fail(-1, "clear_row_lsd: row out of range");
  hipStream_t st = S(s->e, stream);
  ENGINE_LOCK(s->e);
  set_int_kernel<<<1, 64, 0, st>>>(s->lsd_n + row, 1, 0);
  LAUNCHCHK();
  return 0;
}

extern "C" int ptts_profile_start(ptts_engine *e) {
  if (!e) return fail(-1, "null engine");
  ENGINE_LOCK(e);
  for (auto &r : e->prof.recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  e->prof.recs.clear();
  e->prof.on = true;
  return 0;
}

// Stops profiling and writes one line per (site, kernel): "site kernel count total_ms bytes flops\n"
extern "C" int64_t ptts_profile_stop(ptts_engine *e, char *h_out, int64_t capacity) {
  if (!e) return fail(-1, "null engine");
  ENGINE_LOCK(e);
  e->prof.on = false;
  if (hipDeviceSynchronize() != hipSuccess) return fail(-2, "sync failed");
  std::map<std::pair<std::string, std::string>, std::array<double, 4>> agg;
  std::vector<std::pair<std::string, std::string>> order;
  for (auto &r : e->prof.recs) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, r.a, r.b);
    auto key = std::make_pair(r.site, r.kernel);
    if (!agg.count(key)) { agg[key] = {0, 0, 0, 0}; order.push_back(key); }
    auto &v = agg[key];
    v[0] += 1; v[1] += ms; v[2] += r.bytes; v[3] += r.flops;
    (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b);
  }
  e->prof.recs.clear();
  std::string out;
  char line[512];
  for (auto &k : order) {
    auto &v = agg[k];
    snprintf(line, sizeof line, "%s %s %.0f %.6f %.0f %.0f\n", k.first.empty() ? "-" : k.first.c_str(), k.second.c_str(), v[0], v[1], v[2], v[3]);
    out += line;
  }
  if ((int64_t)out.size() + 1 > capacity) return fail(-1, "profile buffer too small");
  memcpy(h_out, out.c_str(), out.size() + 1);
  return (int64_t)out.size();
}


// ------------------------------------------------------------------------------------------------
// Single-launch flow MLP (ptts_flow.h).  Geometry per state: RT row tiles per cluster, NG clusters of FDF workgroups.
static bool flow_cluster_ok(const ptts_engine *e, const ptts_lm_state *s) {
  const ptts_config &c = e->cfg;
  const int FDF = c.flow_dim / 16, LF = c.ldim / 16;
  if (!e->opt_flow_cluster || c.flow_depth > FLOW_MAX_DEPTH || FDF > 64 || LF > FDF) return false;
  const int kpw = cdiv(std::max(FDF, LF), FLOW_WORKERS);
  if (kpw != 1 && kpw != 2 && kpw != 4) return false;  // flow_dim <= 512
  if (!e->input_proj.bias || !e->fin.bias) return false;
  for (auto &r : e->res) if (!r.l0.bias || !r.l2.bias) return false;
  // every workgroup of the launch must be resident at once (they wait for each other) and a 9-wave workgroup fills a
  // CU: the grid is capped at opt_flow_max_cus workgroups (default 128: half the chip, so a codec kernel always has CUs left) (larger batches loop over row groups inside the kernel)
  return FDF <= std::min(e->opt_flow_max_cus, e->n_cus);
}
// the state's steps run flow_cluster_mod_kernel: its switch is on, one schedule for all rows, one row tile per cluster
// and a plain fp32 AdaLN matrix in the tile order the kernel assumes.  Anything else takes the flow.adaln launch.
static bool flow_fold_ok(const ptts_engine *e, const ptts_lm_state *s) {
  const int FDF = e->cfg.flow_dim / 16;
  const Lin &m = e->adaln;
  return s->flow_fold && flow_cluster_ok(e, s) && s->lsd_cap == 0 && s->flow_rt == 1 && m.w && m.bias && !m.wq && !m.wb16 &&
         m.KF == FDF && m.NT == (3 * e->cfg.flow_depth + 2) * FDF;
}
// (re)allocates the per-state buffers whose size depends on the number of LSD steps; never called during capture
static int ensure_flow(ptts_engine *e, ptts_lm_state *s, int steps, hipStream_t st) {
  if (steps <= s->flow_steps) return 0;
  if (s->n_graphs > 0)
    return fail(-1, "lsd_decode_steps grows beyond what this state's captured graphs were built for: destroy the graphs first "
                    "(they hold the old AdaLN / exchange buffers)");
  const ptts_config &c = e->cfg;
  const int FDF = c.flow_dim / 16;
  // row tiles per cluster.  1 (default): one cluster per 16 rows, the clusters' weight re-reads stay in L2 / Infinity Cache.
  // 2 (PTTS_FLOW_RT=2, A/B knob): half the clusters, half the weight fetches and CUs, twice the exchange payload per phase.
  static const int rt_env = [] { const char *v = getenv("PTTS_FLOW_RT"); return v ? atoi(v) : 1; }();
  s->flow_rt = (rt_env == 2 && s->MT >= 2) ? 2 : 1;
  s->flow_ng = cdiv(s->MT, s->flow_rt);
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipStreamSynchronize(e->stream));
  AllocScope alloc_scope(st);
  hipFree(s->mod); hipFree(s->fexch); hipFree(s->fflags);
  s->mod = nullptr; s->fexch = nullptr; s->fflags = nullptr;
  const size_t rt = (size_t)s->MT * 256;
  const int nph = steps * (2 * c.flow_depth + 2);
  CHK(dallocT(nullptr, &s->mod, (size_t)steps * rt * e->adaln.NT));
  CHK(dallocT(nullptr, &s->fexch, flow_slot(FDF, s->flow_rt, nph, s->flow_fold ? FLOW_MOD_FRAGS : 1, s->flow_ng, 0, 0, 0, 0)));
  CHK(dallocT(nullptr, &s->fflags, (size_t)s->flow_ng * nph * FDF));
  HIPCHK(hipStreamSynchronize(st));
  s->flow_steps = steps;
  return 0;
}

template <int RT, bool ROWLSD>
static void launch_flow_rt(hipStream_t st, const FlowArgs &fa, int kpw) {
  const dim3 grid(fa.NCL * fa.FDF), block(FLOW_THREADS);
  switch (kpw) {
    case 1: flow_cluster_kernel<RT, 1, ROWLSD><<<grid, block, 0, st>>>(fa); break;
    case 2: flow_cluster_kernel<RT, 2, ROWLSD><<<grid, block, 0, st>>>(fa); break;
    default: flow_cluster_kernel<RT, 4, ROWLSD><<<grid, block, 0, st>>>(fa); break;
  }
}

// LSD steps the flow buffers of a step must hold: the step's own count, or the per-row capacity when it is larger
static int flow_steps_of(const ptts_lm_state *s, int lsd_steps) { return std::max(lsd_steps, s->lsd_cap); }

// with per-row schedules (s->lsd_cap > 0) `lsd_steps` is the count of rows without an override and the slots are laid out
// for flow_steps_of(s, lsd_steps) steps
// `fold` (flow_fold_ok): flow_cluster_mod_kernel, which reads `ce` and the AdaLN matrix instead of `mod`; ce_silu: `ce`
// already holds silu(ce + tcomb[0])
static void launch_flow_cluster(hipStream_t st, ptts_engine *e, ptts_lm_state *s, int lsd_steps, float *d_latent_out,
                                bool fold = false, const float *tcomb = nullptr, bool ce_silu = false) {
  const ptts_config &c = e->cfg;
  const int FDF = c.flow_dim / 16, LF = c.ldim / 16;
  FlowArgs fa;
  memset(&fa, 0, sizeof fa);
  fa.MT = s->MT; fa.M = s->B; fa.NG = s->flow_ng; fa.NCL = std::max(1, std::min(s->flow_ng, std::min(e->opt_flow_max_cus, e->n_cus) / FDF)); fa.FDF = FDF; fa.LF = LF; fa.AF = e->adaln.NT;
  const bool rowlsd = s->lsd_cap > 0;
  fa.depth = c.flow_depth; fa.steps = rowlsd ? flow_steps_of(s, lsd_steps) : lsd_steps; fa.ldim = c.ldim;
  fa.w_in = e->input_proj.w; fa.b_in = e->input_proj.bias;
  for (int r = 0; r < c.flow_depth; ++r) {
    fa.w_l0[r] = e->res[r].l0.w; fa.b_l0[r] = e->res[r].l0.bias;
    fa.w_l2[r] = e->res[r].l2.w; fa.b_l2[r] = e->res[r].l2.bias;
    fa.ln_w[r] = e->res[r].ln_w; fa.ln_b[r] = e->res[r].ln_b;
  }
  fa.w_fin = e->fin.w; fa.b_fin = e->fin.bias;
  fa.mod = s->mod; fa.mod_step = (long)s->MT * 256 * e->adaln.NT;
  fa.latfm = s->latfm;
  fa.lat = s->lat; fa.lat_out1 = s->lat_prev; fa.lat_out2 = d_latent_out;
  fa.inv_steps = 1.0f / (float)lsd_steps;
  fa.exch = s->fexch; fa.flags = s->fflags; fa.ctr = s->rng_ctr; fa.err = s->ferr;
  fa.row_n = rowlsd ? s->lsd_n : nullptr; fa.row_ndef = lsd_steps;
  if (fold) { fa.mod = nullptr; fa.ce = s->ce; fa.w_mod = e->adaln.w; fa.b_mod = e->adaln.bias; fa.tcomb = tcomb; fa.ce_silu = ce_silu; }
  // weights of the chain once per cluster-set (L2 / Infinity Cache absorb the clusters' re-reads) + modulations + io
  // folded: + the AdaLN matrix, and `ce` in place of the modulations
  const double wbytes = 4.0 * 256 * ((double)FDF * LF + 2.0 * c.flow_depth * FDF * FDF + (double)LF * FDF + (fold ? (double)e->adaln.NT * FDF : 0.0));
  const double flops = 2.0 * s->B * 256.0 * ((double)FDF * LF + 2.0 * c.flow_depth * FDF * FDF + (double)LF * FDF + (fold ? (double)e->adaln.NT * FDF : 0.0)) * lsd_steps;
  ProfScope ps(st, std::string(fold ? "flow_cluster_mod@" : rowlsd ? "flow_cluster_rowlsd@" : "flow_cluster@") + std::to_string((long)fa.NCL * FDF * FLOW_THREADS),
               lsd_steps * (wbytes + 4.0 * s->B * 16.0 * (fold ? FDF : e->adaln.NT)), flops);
  const int kpw = cdiv(std::max(FDF, LF), FLOW_WORKERS);
  s->coop_wgs = std::max(s->coop_wgs, fa.NCL * FDF);
  if (fold) {
    const dim3 grid(fa.NCL * fa.FDF), block(FLOW_THREADS);
    switch (kpw) {
      case 1: flow_cluster_mod_kernel<1><<<grid, block, 0, st>>>(fa); break;
      case 2: flow_cluster_mod_kernel<2><<<grid, block, 0, st>>>(fa); break;
      default: flow_cluster_mod_kernel<4><<<grid, block, 0, st>>>(fa); break;
    }
    return;
  }
  if (rowlsd) {
    if (s->flow_rt == 2) launch_flow_rt<2, true>(st, fa, kpw);
    else launch_flow_rt<1, true>(st, fa, kpw);
  } else {
    if (s->flow_rt == 2) launch_flow_rt<2, false>(st, fa, kpw);
    else launch_flow_rt<1, false>(st, fa, kpw);
  }
}


// ------------------------------------------------------------------------------------------------
// Single-launch transformer stack (ptts_lm.h)
static constexpr int kLmMaxWGs = 256;  // resident workgroups of one launch (one per CU)
static bool lm_cluster_ok(const ptts_engine *e, const ptts_lm_state *s) {
  if (!e->opt_lm_cluster || !e->lm_table) return false;
  if (e->cfg.d_model / 16 > std::min(kLmMaxWGs, e->n_cus)) return false;  // one cluster must be resident at once
  if (s->n_pre > 0) return false;  // the single-launch stack reads its keys from the state's own cache only
  return (double)s->kv_plane() * 4.0 < 2.0e9;  // 32-bit buffer offsets into a K / V plane
}
static int ensure_lm_cluster(ptts_engine *e, ptts_lm_state *s, hipStream_t st) {
  if (s->lexch || !e->lm_table) return 0;
  const ptts_config &c = e->cfg;
  const int DF = c.d_model / 16, FFF = c.ff_dim / 16;
  AllocScope alloc_scope(st);
  CHK(dallocT(nullptr, &s->lexch, (size_t)s->MT * c.num_layers * (4 * DF + FFF) * 256));
  CHK(dallocT(nullptr, &s->lflags, (size_t)s->MT * c.num_layers * 5 * DF));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}
static void launch_lm_cluster(hipStream_t st, ptts_engine *e, ptts_lm_state *s, Scratch &sc) {
  const ptts_config &c = e->cfg;
  LmArgs la;
  memset(&la, 0, sizeof la);
  la.MT = s->MT; la.M = s->B; la.NG = s->MT; la.DF = c.d_model / 16; la.FFF = c.ff_dim / 16; la.H = c.num_heads;
  la.NCL = std::max(1, std::min(la.NG, std::min(kLmMaxWGs, e->n_cus) / la.DF));
  s->coop_wgs = std::max(s->coop_wgs, la.NCL * la.DF);
  la.L = c.num_layers; la.cap = s->cap;
  la.layers = e->lm_table; la.kv = s->kv; la.kv_plane = (long)s->kv_plane();
  la.offset = s->offset; la.freq = e->freq_lm; la.x = sc.x; la.exch = s->lexch; la.flags = s->lflags;
  la.ctr = s->rng_ctr; la.err = s->ferr; la.ln_eps = 1e-5f;
  double keys = 0;
  for (int b = 0; b < s->B; ++b) keys += s->h_off[b] + 1;
  const double wbytes = 4.0 * 256.0 * c.num_layers * ((double)4 * la.DF * la.DF + 2.0 * la.DF * la.FFF);
  ProfScope ps(st, "lm_cluster@" + std::to_string((long)la.NCL * la.DF * FLOW_THREADS),
               wbytes + c.num_layers * keys * c.num_heads * 64 * 4 * 2,
               c.num_layers * (2.0 * s->B * 256.0 * ((double)4 * la.DF * la.DF + 2.0 * la.DF * la.FFF) + 4.0 * keys * c.num_heads * 64));
  lm_cluster_kernel<0><<<dim3(la.NCL * la.DF), dim3(FLOW_THREADS), 0, st>>>(la);
}

// Cooperative kernels (flow / transformer clusters) need all their workgroups resident: a launch of W workgroups (one per
// CU, see flow_cluster_ok) may share the GPU with other cooperative launches only while the SUM of their grids fits the
// device - beyond that two half-resident grids could wait for each other.  Steps that contain such a launch therefore take
// one of N = floor(CUs / W) per-device SLOTS: step k (in launch order, all states and streams of the device) waits on the GPU
// for step k - N and records its slot's event when it ends.  N = 2 for the flow cluster's default 128 workgroups, so the
// FlowLM steps of two states queued on two streams overlap (round 2 chained them all, lm || lm = 2.16x one alone); the
// 256-workgroup transformer cluster gets N = 1, i.e. the old strict chain.  GPU-side order only, the host never waits.
static constexpr int kCoopMaxSlots = 4;
struct CoopSlots { hipEvent_t ev[kCoopMaxSlots] = {}; bool used[kCoopMaxSlots] = {}; unsigned long long next = 0; };
static std::mutex g_coop_mu;
static CoopSlots g_coop[64];
struct CoopGuard {
  CoopSlots *cs = nullptr;
  hipStream_t st;
  int slot = 0, rc = 0;
  // `wgs` = workgroups of the step's cooperative launch (0: none, the guard does nothing); `n_cus` = CUs of the device
  CoopGuard(int device, hipStream_t stream, int wgs, int n_cus) : st(stream) {
    if (wgs <= 0) return;
    g_coop_mu.lock();
    cs = &g_coop[device & 63];
    // the events belong to the device of the engine, whatever device the calling thread had current (a scheduler thread
    // of an engine on cuda:N > 0): the callers have run hipSetDevice(e->device)
    const int n = std::max(1, std::min(kCoopMaxSlots, n_cus / wgs));
    slot = (int)(cs->next++ % (unsigned)n);
    if (!cs->ev[slot] && hipEventCreateWithFlags(&cs->ev[slot], hipEventDisableTiming) != hipSuccess) { rc = -2; cs->ev[slot] = nullptr; return; }
    // a launch that needs more than its share (n shrank: e.g. the transformer cluster after flow-only steps) waits for ALL slots
    for (int i = 0; i < kCoopMaxSlots; ++i)
      if (cs->ev[i] && cs->used[i] && (i == slot || i >= n))
        if (hipStreamWaitEvent(st, cs->ev[i], 0) != hipSuccess) rc = -2;
  }
  int finish() {  // call after the step is enqueued; returns < 0 when the chain could not be established
    if (!cs) return 0;
    if (cs->ev[slot]) {
      if (hipEventRecord(cs->ev[slot], st) != hipSuccess) rc = -2;
      else cs->used[slot] = true;
    }
    CoopSlots *c = cs;
    cs = nullptr;
    (void)c;
    g_coop_mu.unlock();
    return rc;
  }
  ~CoopGuard() { if (cs) { cs = nullptr; g_coop_mu.unlock(); } }
};
// CUs a stream may use (hipExtStreamCreateWithCUMask streams: the bits of its mask; else the whole device)
static int stream_cu_count(hipStream_t st, int n_cus) {
  uint32_t mask[16] = {};
  if (!st || hipExtStreamGetCUMask(st, 16, mask) != hipSuccess) { (void)hipGetLastError(); return n_cus; }
  int bits = 0;
  for (uint32_t w : mask) bits += __builtin_popcount(w);
  return bits > 0 ? std::min(bits, n_cus) : n_cus;
}

// qlen / h_len (ragged prefill): device and host copy of the real rows per sequence, the other Tq - len are padding
static void lm_layers(hipStream_t st, ptts_engine *e, ptts_lm_state *s, Scratch &sc, int M, int Tq, bool rope_done = false,
                      const int *qlen = nullptr, const int32_t *h_len = nullptr) {
  const ptts_config &c = e->cfg;
  bind_engine(e);
  if (!rope_done) {  // decode steps build the table in their prologue kernel
    SITE("lm.rope");
    ProfScope ps(st, "rope_table", 256.0 * M, 0);
    rope_table_kernel<<<cdiv(M * 32, 256), 256, 0, st>>>(s->offset, e->freq_lm, sc.rope, M, Tq);
  }
  for (int l = 0; l < c.num_layers; ++l) {
    TrCtx t;
    t.D = c.d_model; t.H = c.num_heads; t.FF = c.ff_dim; t.MT = sc.MT; t.M = M; t.Tq = Tq; t.QB = sc.QB;
    t.cap = s->cap; t.ring = 0; t.ctx = 0;
    // decode steps split the keys over the waves of a workgroup (decode_attn_waves): no key splits, no combine launch
    t.splits = Tq == 1 ? 1 : std::min(sc.splits_cap, attn_splits(s->B * c.num_heads * sc.QB, cdiv(s->cap, 16)));
    t.x_in = sc.x; t.x = sc.x; t.x_out = sc.x; t.out_ds = 0; t.par = nullptr;
    t.h = sc.h; t.ao = sc.ao; t.ff = sc.ff; t.q = sc.q; t.part = sc.part;
    t.Kc = s->K(l); t.Vc = s->V(l); t.offset = s->offset; t.rope = sc.rope;
    t.pre = s->d_pre; t.layer = l; t.cascade = e->opt_share_prefix && (s->casc_mode < 0 ? s->n_pre > 0 : s->casc_mode > 0) ? e->opt_cascade : 0;
    t.kv_keys = 0;
    for (int b = 0; b < s->B; ++b) t.kv_keys += h_len ? (h_len[b] ? s->h_off[b] + h_len[b] : 0) : s->h_off[b] + Tq;
    t.qlen = qlen;
    t.tag = "lm";
    run_tr_layer(st, e->lm[l], t);
  }
}

extern "C" int ptts_lm_prefill(ptts_engine *e, ptts_lm_state *s, const float *d_emb, int32_t T, void *stream) {
  ENGINE_LOCK(e);
  if (T < 1) return 0;
  HIPCHK(hipSetDevice(e->device));
  const ptts_config &c = e->cfg;
  for (int b = 0; b < s->B; ++b)
    if (s->h_off[b] + T > s->cap) return fail(-5, "prefill: KV cache capacity exceeded");
  hipStream_t st = S(e, stream);
  const int M = s->B * T;
  if (!s->pre.x || s->pre.MT < cdiv(M, 16) || s->pre.QB != cdiv(T, 16)) {
    HIPCHK(hipStreamSynchronize(st));
    if (s->pre.x) free_scratch(&s->pre);
    AllocScope alloc_scope(st);
    CHK(alloc_scratch(e, &s->pre, s->B, T, c.d_model, c.num_heads, c.ff_dim, s->cap));
  }
  Scratch &sc = s->pre;
  const int MT = cdiv(M, 16);
  sc.MT = MT;
  long n4 = (long)MT * (c.d_model / 16) * 64;
  to_fm_kernel<<<cdiv(n4, 256), 256, 0, st>>>(d_emb, sc.x, M, c.d_model, MT);
  lm_layers(st, e, s, sc, M, T);
  add_int_kernel<<<cdiv(s->B, 256), 256, 0, st>>>(s->offset, s->B, T);
  for (auto &o : s->h_off) o += T;
  LAUNCHCHK();
  return 0;
}

// Rows of different lengths in one pass (include/ptts.h).  The layer stack runs on B * t_max rows; the padding behind a row's
// h_len[b] real positions stores no key or value, is attended by nobody and attends nothing (GemmArgs::qlen, AttnArgs::qlen),
// and every other kernel of the stack is row-independent, so what the padding holds never reaches a real row.
extern "C" int ptts_lm_prefill_ragged(ptts_engine *e, ptts_lm_state *s, const float *d_emb, const int32_t *h_len, int32_t t_max,
                                      void *stream) {
  if (!e || !s || !h_len) return fail(-1, "prefill_ragged: null argument");
  ENGINE_LOCK(e);
  if (t_max < 1) return fail(-1, "prefill_ragged: t_max must be >= 1");
  bool any = false;
  for (int b = 0; b < s->B; ++b) {
    if (h_len[b] < 0 || h_len[b] > t_max) return fail(-1, "prefill_ragged: row " + std::to_string(b) + " has length " + std::to_string(h_len[b]) +
                                                              ", expected 0 .. " + std::to_string(t_max));
    any |= h_len[b] > 0;
  }
  for (int b = 0; b < s->B; ++b)
    if (s->h_off[b] + h_len[b] > s->cap) return fail(-5, "prefill: KV cache capacity exceeded");
  if (!any) return 0;
  if (!d_emb) return fail(-1, "prefill_ragged: null argument");
  HIPCHK(hipSetDevice(e->device));
  const ptts_config &c = e->cfg;
  hipStream_t st = S(e, stream);
  const int M = s->B * t_max;
  if (!s->pre.x || s->pre.MT < cdiv(M, 16) || s->pre.QB != cdiv(t_max, 16)) {
    HIPCHK(hipStreamSynchronize(st));
    if (s->pre.x) free_scratch(&s->pre);
    AllocScope alloc_scope(st);
    CHK(alloc_scratch(e, &s->pre, s->B, t_max, c.d_model, c.num_heads, c.ff_dim, s->cap));
  }
  Scratch &sc = s->pre;
  const int MT = cdiv(M, 16);
  sc.MT = MT;
  for (int b0 = 0; b0 < s->B; b0 += 64) {  // the lengths ride in the launch arguments: h_len is free on return
    IntPack pk;
    const int n = std::min(64, s->B - b0);
    for (int i = 0; i < 64; ++i) pk.v[i] = i < n ? h_len[b0 + i] : 0;
    set_ints_kernel<<<1, 64, 0, st>>>(s->qlen + b0, n, pk);
  }
  long n4 = (long)MT * (c.d_model / 16) * 64;
  to_fm_kernel<<<cdiv(n4, 256), 256, 0, st>>>(d_emb, sc.x, M, c.d_model, MT);
  lm_layers(st, e, s, sc, M, t_max, false, s->qlen, h_len);
  add_rows_kernel<<<cdiv(s->B, 256), 256, 0, st>>>(s->offset, s->qlen, s->B);
  for (int b = 0; b < s->B; ++b) s->h_off[b] += h_len[b];
  LAUNCHCHK();
  return 0;
}

// workgroups of the largest cooperative launch a decode step of this state contains (0: per-layer launches only)
static int coop_wgs_of_step(const ptts_engine *e, const ptts_lm_state *s, int lsd_steps) {
  int w = 0;
  const ptts_config &c = e->cfg;
  if (flow_cluster_ok(e, s) && flow_steps_of(s, lsd_steps) <= s->flow_steps) {
    const int FDF = c.flow_dim / 16;
    w = std::max(1, std::min(s->flow_ng, std::min(e->opt_flow_max_cus, e->n_cus) / FDF)) * FDF;
  }
  if (lm_cluster_ok(e, s) && s->lexch) {
    const int DF = c.d_model / 16;
    w = std::max(w, std::max(1, std::min(s->MT, std::min(kLmMaxWGs, e->n_cus) / DF)) * DF);
  }
  return w;
}

static int lm_step_enqueue(hipStream_t st, ptts_engine *e, ptts_lm_state *s, const float *d_latent_in,
                           const float *d_noise, int lsd_steps, float eos_thr, float *d_latent_out,
                           float *d_eos_logit, uint8_t *d_is_eos) {
  const ptts_config &c = e->cfg;
  bind_engine(e);
  const int B = s->B, MT = s->MT, D = c.d_model, FD = c.flow_dim, DF = D / 16, FDF = FD / 16, LF = c.ldim / 16;
  Scratch &sc = s->dec;
  s->coop_wgs = 0;
  const float *tcomb = e->tcomb[lsd_steps];
  SITE("lm.prep");  // BOS substitution + input_linear + noise / LSD start point + RoPE table: one launch
  if (e->in_linear.w && !e->in_linear.bias && e->in_linear.KF == LF) {
    ProfScope ps(st, "prep_in", 16.0 * B * c.ldim + 4.0 * (D * c.ldim + B * D), 2.0 * B * D * c.ldim);
    const int nb_gemm = cdiv(DF * MT, 4), nb_prep = cdiv(MT * LF * 64, 256);
    prep_in_kernel<<<nb_gemm + nb_prep + cdiv(B * 32, 256), 256, 0, st>>>(
        d_latent_in ? d_latent_in : s->lat_prev, e->bos, d_noise, e->in_linear.w, sc.x, s->lat, s->latfm, B, c.ldim, MT, DF, s->rng_std,
        s->rng_seed, s->rng_ctr, s->rsamp(), nb_gemm, nb_prep, RopeArgs{s->offset, e->freq_lm, sc.rope, B, 1});
  } else {
    {
      ProfScope ps(st, "prep_lm", 16.0 * B * c.ldim, 0);
      const int nb_prep = cdiv(MT * LF * 64, 256);
      prep_lm_kernel<<<nb_prep + cdiv(B * 32, 256), 256, 0, st>>>(d_latent_in ? d_latent_in : s->lat_prev, e->bos, d_noise,
                                                                   s->xlat, s->lat, s->latfm, B, c.ldim, MT, s->rng_std,
                                                                   s->rng_seed, s->rng_ctr, s->rsamp(), nb_prep,
                                                                   RopeArgs{s->offset, e->freq_lm, sc.rope, B, 1});
    }
    SITE("lm.in_linear");
    GemmArgs a0 = mk_gemm(e->in_linear, s->xlat, LF, MT, B);
    a0.Y = sc.x; a0.YF = DF;
    launch_gemm(st, a0, PRE_NONE);
  }
  GemmArgs a;
  if (lm_cluster_ok(e, s) && s->lexch) {
    SITE("lm.cluster");
    launch_lm_cluster(st, e, s, sc);
  } else {
    lm_layers(st, e, s, sc, B, 1, true);
  }
  SITE("flow.head");  // out_norm is folded into [cond_embed ; out_eos]
  a = mk_gemm(e->head, sc.x, DF, MT, B);
  a.epi = EPI_HEAD; a.Y = s->ce; a.YF = FDF; a.head_nt = FDF; a.eos_thr = eos_thr;
  a.eos_on = s->samp_on; a.eos_row = s->samp_eos;
  a.eos_logit = s->eos_logit; a.is_eos = s->is_eos;
  a.eos_logit2 = d_eos_logit; a.is_eos2 = d_is_eos;  // caller's buffers are written by the epilogue itself
  a.tail_offset = s->offset; a.tail_ctr = s->rng_ctr; a.tail_rctr = s->seed_ctr; a.tail_active = s->active;  // the step's bookkeeping rides along (was a launch)
  // s->ce then holds silu(t_emb + cond) and the modulation GEMM loads it as is (not with per-row schedules: rows differ)
  const bool silu_in_head = lsd_steps == 1 && s->lsd_cap == 0;
  if (silu_in_head) { a.act = ACT_SILU; a.prevec = tcomb; }
  launch_gemm(st, a, PRE_LNFOLD);
  const int AF = e->adaln.NT;
  const bool rowlsd = s->lsd_cap > 0;
  const int nit = rowlsd ? flow_steps_of(s, lsd_steps) : lsd_steps;  // LSD iterations enqueued
  auto row_lsd = [&](GemmArgs &g, int i) {  // per-row schedules of step i (GemmArgs::row_n)
    g.row_n = s->lsd_n; g.row_tab = s->lsd_tab; g.row_ndef = lsd_steps; g.row_i = i;
  };
  s->mod_stale = false;
  if (flow_fold_ok(e, s) && nit <= s->flow_steps) {
    // the modulations are computed inside the cluster's hand-off waits: no flow.adaln launch, `mod` is not written
    SITE("flow.cluster");
    launch_flow_cluster(st, e, s, lsd_steps, d_latent_out, true, tcomb, silu_in_head);
    s->latfm_noise = true;
    s->mod_stale = true;
  } else if (flow_cluster_ok(e, s) && nit <= s->flow_steps) {
    // the AdaLN modulations of every LSD step (they depend on the step's (s, t) only through t_emb), then the whole
    // chain + Euler loop in ONE launch
    if (rowlsd) {  // every step in one launch (grid.z), each row with its own schedule
      SITE("flow.adaln");
      a = mk_gemm(e->adaln, s->ce, FDF, MT, B);
      a.prevec = tcomb; a.Y = s->mod; a.YF = AF;
      row_lsd(a, 0);
      a.row_nz = nit; a.row_zstride = (long)MT * 256 * AF;
      launch_gemm(st, a, PRE_ADDSILU_ROW);
    } else {
      for (int i = 0; i < lsd_steps; ++i) {
        SITE("flow.adaln");
        a = mk_gemm(e->adaln, s->ce, FDF, MT, B);
        a.prevec = tcomb + (size_t)i * FD; a.Y = s->mod + (size_t)i * MT * 256 * AF; a.YF = AF;
        launch_gemm(st, a, silu_in_head ? PRE_NONE : PRE_ADDSILU);
      }
    }
    SITE("flow.cluster");
    launch_flow_cluster(st, e, s, lsd_steps, d_latent_out);
    s->latfm_noise = true;  // the cluster reads latfm, never writes it
  } else {
  s->latfm_noise = false;  // the per-layer path keeps the FM copy of the running latent there
  for (int i = 0; i < nit; ++i) {
    // all AdaLN modulations of the step in one GEMM on silu(t_emb + cond)  (mlp.py:107,127,210)
    SITE("flow.adaln");
    a = mk_gemm(e->adaln, s->ce, FDF, MT, B);
    a.prevec = tcomb + (size_t)i * FD; a.Y = s->mod; a.YF = AF;
    if (rowlsd) {  // row m adds its own schedule's embedding of step i (rows past their count: tiles exit or are unused)
      a.prevec = tcomb;
      row_lsd(a, i);
      launch_gemm(st, a, PRE_ADDSILU_ROW);
    } else {
      launch_gemm(st, a, silu_in_head ? PRE_NONE : PRE_ADDSILU);
    }
    SITE("flow.input_proj");
    a = mk_gemm(e->input_proj, s->latfm, LF, MT, B);
    a.Y = s->fx; a.YF = FDF;
    a.stat_out = s->fstat;  // row statistics of x for the first block's LayerNorm
    launch_gemm(st, a, PRE_NONE);
    for (int r = 0; r < c.flow_depth; ++r) {
      const float *shift = s->mod + (size_t)(r * 3 * FDF) * 256;
      const float *scale = shift + (size_t)FDF * 256;
      const float *gate = scale + (size_t)FDF * 256;
      SITE("flow.res.l0");  // in_ln + AdaLN modulate are applied to the operand on load (PRE_LNMOD)
      a = mk_gemm(e->res[r].l0, s->fx, FDF, MT, B);
      a.act = ACT_SILU; a.Y = s->f1; a.YF = FDF;
      a.lnm_w = e->res[r].ln_w; a.lnm_b = e->res[r].ln_b; a.mod_shift = shift; a.mod_scale = scale; a.modF = AF;
      a.ln_eps = 1e-6f;  // flow-MLP LayerNorm eps (mlp.py:95)
      a.stat_in = s->fstat; a.stat_nt = FDF;
      launch_gemm(st, a, PRE_LNMOD);
      SITE("flow.res.l2");
      a = mk_gemm(e->res[r].l2, s->f1, FDF, MT, B);
      a.epi = EPI_GATE; a.R = s->fx; a.RF = FDF; a.G = gate; a.GF = AF; a.Y = s->fx; a.YF = FDF;
      a.stat_out = s->fstat;  // ... of the updated x for the next block / the final layer
      launch_gemm(st, a, PRE_NONE);
    }
    const float *shift = s->mod + (size_t)(c.flow_depth * 3 * FDF) * 256;
    const float *scale = shift + (size_t)FDF * 256;
    SITE("flow.final");  // norm_final (no affine) + modulate on load
    a = mk_gemm(e->fin, s->fx, FDF, MT, B);
    a.lnm_w = nullptr; a.lnm_b = nullptr; a.mod_shift = shift; a.mod_scale = scale; a.modF = AF; a.ln_eps = 1e-6f;
    a.stat_in = s->fstat; a.stat_nt = FDF;
    a.epi = EPI_LATENT; a.lat = s->lat; a.ldim = c.ldim; a.inv_steps = 1.0f / (float)lsd_steps; a.Y = s->latfm; a.YF = LF;
    if (i == lsd_steps - 1) { a.lat_out1 = s->lat_prev; a.lat_out2 = d_latent_out; }  // next step's input + caller's copy
    if (rowlsd) {  // every row writes them at its own last step
      row_lsd(a, i);
      a.lat_out1 = s->lat_prev; a.lat_out2 = d_latent_out;
    }
    launch_gemm(st, a, rowlsd ? PRE_LNMOD_ROW : PRE_LNMOD);
  }
  }
  SITE("");
  return 0;
}

extern "C" int ptts_lm_decode_step(ptts_engine *e, ptts_lm_state *s, const float *d_latent_in, const float *d_noise,
                                   int32_t lsd_steps, float eos_threshold, float *d_latent_out, float *d_eos_logit,
                                   uint8_t *d_is_eos, void *stream) {
  ENGINE_LOCK(e);
  HIPCHK(hipSetDevice(e->device));
  CHK(prepare_lsd(e, lsd_steps));
  CHK(ensure_flow(e, s, flow_steps_of(s, lsd_steps), S(e, stream)));
  CHK(ensure_lm_cluster(e, s, S(e, stream)));
  for (int b = 0; b < s->B; ++b)
    if (s->h_off[b] + 1 > s->cap) return fail(-5, "decode: KV cache capacity exceeded");
  {
    // grid of the cooperative launch this step will contain (the enqueue records the exact value in s->coop_wgs)
    const int wgs = coop_wgs_of_step(e, s, lsd_steps);
    if (wgs > stream_cu_count(S(e, stream), e->n_cus))
      return fail(-1, "decode: the stream's CU mask is smaller than the cooperative flow launch (lower the flow_max_cus option)");
    CoopGuard guard(e->device, S(e, stream), wgs, e->n_cus);
    CHK(lm_step_enqueue(S(e, stream), e, s, d_latent_in, d_noise, lsd_steps, eos_threshold, d_latent_out, d_eos_logit, d_is_eos));
    if (guard.finish() < 0) return fail(-2, "decode: could not chain the cooperative launch behind its predecessor");
  }
  for (int b = 0; b < s->B; ++b) s->h_off[b] += s->h_active[b];
  LAUNCHCHK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Tile autotuning for one batch size (see Tuner).  Runs on scratch states; the caller's states are untouched.
extern "C" int ptts_tune(ptts_engine *e, int32_t B, void *stream) { return ptts_tune_streams(e, B, stream, stream); }
// The FlowLM step is tuned on `lm_stream`, the codec frame on `codec_stream`: with CU-masked streams
// (ptts_stream_create_masked) each stage gets the tiles that are fastest on ITS share of the chip.
extern "C" int ptts_tune_streams(ptts_engine *e, int32_t B, void *lm_stream, void *codec_stream) {
  if (!e || B < 1) return fail(-1, "bad argument");
  ENGINE_LOCK(e);
  HIPCHK(hipSetDevice(e->device));
  hipStream_t st = S(e, lm_stream), st2 = S(e, codec_stream);
  Tuner &t = *e->tuner;
  ptts_lm_state *ls = nullptr;
  ptts_mimi_state *ms = nullptr;
  int rc = ptts_lm_state_create(e, B, 32, &ls);
  if (rc == 0) rc = ptts_mimi_state_create(e, B, &ms);
  t.flush_bytes = (size_t)320 << 20;  // > Infinity Cache (256 MiB)
  if (rc == 0) {
    if (hipMalloc(&t.flush, t.flush_bytes) != hipSuccess) { t.flush = nullptr; (void)hipGetLastError(); }  // tune warm if memory is short
    else (void)hipMemsetAsync(t.flush, 0, t.flush_bytes, st);
  }
  if (rc == 0 && (hipEventCreate(&t.e0) != hipSuccess || hipEventCreate(&t.e1) != hipSuccess)) rc = fail(-2, "hipEventCreate");
  if (rc == 0) {
    HIPCHK(hipStreamSynchronize(e->stream));  // state zero-fills
    const bool prof = e->prof.on;
    e->prof.on = false;
    t.active = true;
    rc = ptts_lm_decode_step(e, ls, nullptr, nullptr, 1, 1e30f, nullptr, nullptr, nullptr, st);
    if (hipStreamSynchronize(st) != hipSuccess && rc == 0) rc = fail(-2, "tune: stream error");
    if (rc == 0) rc = ptts_mimi_decode(e, ms, ls->lat, nullptr, st2);
    // the transformer's GEMMs at a frame pair's row count (the throughput pipeline decodes pairs)
    if (rc == 0 && !e->codec_bf16) rc = ptts_mimi_decode_tr(e, ms, ls->lat, ls->lat, st2);
    t.active = false;
    e->prof.on = prof;
    if (hipStreamSynchronize(st2) != hipSuccess && rc == 0) rc = fail(-2, "tune: stream error");
  }
  if (t.e0) hipEventDestroy(t.e0);
  if (t.e1) hipEventDestroy(t.e1);
  t.e0 = t.e1 = nullptr;
  if (t.flush) hipFree(t.flush);
  t.flush = nullptr;
  if (ms) ptts_mimi_state_destroy(ms);
  if (ls) ptts_lm_state_destroy(ls);
  return rc;
}

// Same for the prefill GEMM shapes of `batch` sequences x `t` positions (first-chunk path: text prefill of a chunk).
extern "C" int ptts_tune_prefill(ptts_engine *e, int32_t B, int32_t T, void *stream) {
  if (!e || B < 1 || T < 1) return fail(-1, "bad argument");
  ENGINE_LOCK(e);
  HIPCHK(hipSetDevice(e->device));
  hipStream_t st = S(e, stream);
  Tuner &t = *e->tuner;
  ptts_lm_state *ls = nullptr;
  float *emb = nullptr;
  int rc = ptts_lm_state_create(e, B, T + 16, &ls);
  t.flush_bytes = (size_t)320 << 20;
  if (rc == 0 && hipMalloc((void **)&emb, (size_t)B * T * e->cfg.d_model * 4) != hipSuccess) { (void)hipGetLastError(); rc = fail(-2, "hipMalloc"); }
  if (rc == 0) {
    (void)hipMemsetAsync(emb, 0, (size_t)B * T * e->cfg.d_model * 4, st);
    if (hipMalloc(&t.flush, t.flush_bytes) != hipSuccess) { t.flush = nullptr; (void)hipGetLastError(); }
    else (void)hipMemsetAsync(t.flush, 0, t.flush_bytes, st);
  }
  if (rc == 0 && (hipEventCreate(&t.e0) != hipSuccess || hipEventCreate(&t.e1) != hipSuccess)) rc = fail(-2, "hipEventCreate");
  if (rc == 0) {
    HIPCHK(hipStreamSynchronize(e->stream));
    const bool prof = e->prof.on;
    e->prof.on = false;
    t.active = true;
    rc = ptts_lm_prefill(e, ls, emb, T, st);
    t.active = false;
    e->prof.on = prof;
    if (hipStreamSynchronize(st) != hipSuccess && rc == 0) rc = fail(-2, "tune_prefill: stream error");
  }
  if (t.e0) hipEventDestroy(t.e0);
  if (t.e1) hipEventDestroy(t.e1);
  t.e0 = t.e1 = nullptr;
  if (t.flush) hipFree(t.flush);
  t.flush = nullptr;
  if (emb) hipFree(emb);
  if (ls) ptts_lm_state_destroy(ls);
  return rc;
}

// ------------------------------------------------------------------------------------------------
// hipGraph capture
template <typename F>
static int capture_into(ptts_graph *g, hipGraph_t *graph, hipGraphExec_t *exec, F &&body) {
  if (!g->cap_stream) HIPCHK(hipStreamCreateWithFlags(&g->cap_stream, hipStreamNonBlocking));
  HIPCHK(hipStreamBeginCapture(g->cap_stream, hipStreamCaptureModeThreadLocal));
  int r = body(g->cap_stream);
  if (r >= 0 && !g_launch_err.empty()) r = take_launch_err();
  hipError_t er = hipStreamEndCapture(g->cap_stream, graph);
  if (r < 0) return r;
  HIPCHK(er);
  HIPCHK(hipGraphInstantiate(exec, *graph, nullptr, nullptr, 0));
  return 0;
}
// a graph with an FlowLM step inside is captured twice when its state may come to share prefixes: rows on their own / cascade
template <class F>
static int capture(ptts_engine *e, ptts_graph *g, F &&body) {
  ptts_lm_state *s = g->lm;
  const bool two = s && e->opt_share_prefix && e->opt_cascade && !e->opt_lm_cluster && s->B >= 16;
  if (s) s->casc_mode = 0;
  int r = capture_into(g, &g->graph, &g->exec, body);
  if (r >= 0 && two) {
    s->casc_mode = 1;
    r = capture_into(g, &g->graph_c, &g->exec_c, body);
  }
  if (s) s->casc_mode = -1;
  return r;
}

extern "C" int ptts_graph_capture_lm_step(ptts_engine *e, ptts_lm_state *s, const float *d_noise, int32_t lsd_steps,
                                          float eos_threshold, float *d_latent_out, float *d_eos_logit,
                                          uint8_t *d_is_eos, ptts_graph **out) {
  ENGINE_LOCK(e);
  HIPCHK(hipSetDevice(e->device));
  CHK(prepare_lsd(e, lsd_steps));
  CHK(ensure_flow(e, s, flow_steps_of(s, lsd_steps), e->stream));
  CHK(ensure_lm_cluster(e, s, e->stream));
  ptts_graph *g = new ptts_graph();
  g->lm = s;
  const int rc = capture(e, g, [&](hipStream_t st) {
    return lm_step_enqueue(st, e, s, nullptr, d_noise, lsd_steps, eos_threshold, d_latent_out, d_eos_logit, d_is_eos);
  });
  if (rc < 0) { g->lm = nullptr; ptts_graph_destroy(g); return rc; }
  g->coop_wgs = s->coop_wgs;
  s->n_graphs += 1;
  *out = g;
  return 0;
}

extern "C" int ptts_graph_capture_mimi(ptts_engine *e, ptts_mimi_state *s, const float *d_latent, float *d_pcm,
                                       ptts_graph **out) {
  ENGINE_LOCK(e);
  HIPCHK(hipSetDevice(e->device));
  ptts_graph *g = new ptts_graph();
  g->mimi = s;
  const int rc = capture(e, g, [&](hipStream_t st) { return mimi_frame_enqueue(st, e, s, d_latent, d_pcm); });
  if (rc < 0) { g->mimi = nullptr; ptts_graph_destroy(g); return rc; }
  *out = g;
  return 0;
}

// The codec frame's parts as graphs of their own (ptts_mimi_decode_tr / _seanet): the transformer of one frame or, with
// d_latent_b, of a frame pair; SEANet of one frame with the state's output stages behind it
static int capture_mimi_parts(ptts_engine *e, ptts_mimi_state *s, const float *d_latent, const float *d_latent_b, float *d_pcm,
                              int parts, ptts_graph **out) {
  ENGINE_LOCK(e);
  HIPCHK(hipSetDevice(e->device));
  ptts_graph *g = new ptts_graph();
  g->mimi = s;
  g->mimi_parts = parts;
  g->mimi_frames = d_latent_b ? 2 : 1;
  const int rc = capture(e, g, [&](hipStream_t st) { return mimi_frame_enqueue(st, e, s, d_latent, d_pcm, parts, d_latent_b); });
  if (rc < 0) { g->mimi = nullptr; ptts_graph_destroy(g); return rc; }
  *out = g;
  return 0;
}
extern "C" int ptts_graph_capture_mimi_tr(ptts_engine *e, ptts_mimi_state *s, const float *d_latent, ptts_graph **out) {
  if (!d_latent) return fail(-1, "null latent");
  return capture_mimi_parts(e, s, d_latent, nullptr, nullptr, PART_TR, out);
}
extern "C" int ptts_graph_capture_mimi_tr_pair(ptts_engine *e, ptts_mimi_state *s, const float *d_latent_a,
                                               const float *d_latent_b, ptts_graph **out) {
  if (!d_latent_a || !d_latent_b) return fail(-1, "null latent");
  return capture_mimi_parts(e, s, d_latent_a, d_latent_b, nullptr, PART_TR, out);
}
extern "C" int ptts_graph_capture_mimi_seanet(ptts_engine *e, ptts_mimi_state *s, float *d_pcm, ptts_graph **out) {
  return capture_mimi_parts(e, s, nullptr, nullptr, d_pcm, PART_SEANET, out);
}

// One graph, two parallel branches: FlowLM step (writes d_latent_out) || Mimi decode of the PREVIOUS frame
// (reads d_mimi_latent_in, a different buffer).  Fork/join inside the capture, so a replay needs no
// cross-stream events: consecutive launches on one stream give step t+1 || frame t.
extern "C" int ptts_graph_capture_pipelined(ptts_engine *e, ptts_lm_state *s, ptts_mimi_state *m, const float *d_noise,
                                            int32_t lsd_steps, float eos_threshold, float *d_latent_out,
                                            float *d_eos_logit, uint8_t *d_is_eos, const float *d_mimi_latent_in,
                                            float *d_pcm, ptts_graph **out) {
  ENGINE_LOCK(e);
  HIPCHK(hipSetDevice(e->device));
  CHK(prepare_lsd(e, lsd_steps));
  CHK(ensure_flow(e, s, flow_steps_of(s, lsd_steps), e->stream));
  CHK(ensure_lm_cluster(e, s, e->stream));
  ptts_graph *g = new ptts_graph();
  g->lm = s;
  g->mimi = m;
  hipStream_t side;
  hipEvent_t fork, join;
  HIPCHK(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&fork, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&join, hipEventDisableTiming));
  int rc = capture(e, g, [&](hipStream_t st) {
    if (hipEventRecord(fork, st) != hipSuccess) return fail(-2, "fork record");
    if (hipStreamWaitEvent(side, fork, 0) != hipSuccess) return fail(-2, "fork wait");
    int r = lm_step_enqueue(st, e, s, nullptr, d_noise, lsd_steps, eos_threshold, d_latent_out, d_eos_logit, d_is_eos);
    if (r < 0) return r;
    r = mimi_frame_enqueue(side, e, m, d_mimi_latent_in, d_pcm);
    if (r < 0) return r;
    if (hipEventRecord(join, side) != hipSuccess) return fail(-2, "join record");
    if (hipStreamWaitEvent(st, join, 0) != hipSuccess) return fail(-2, "join wait");
    return 0;
  });
  hipEventDestroy(fork);
  hipEventDestroy(join);
  hipStreamDestroy(side);
  if (rc < 0) { g->lm = nullptr; g->mimi = nullptr; ptts_graph_destroy(g); return rc; }
  g->coop_wgs = s->coop_wgs;
  s->n_graphs += 1;
  *out = g;
  return 0;
}

extern "C" int ptts_graph_launch(ptts_graph *g, void *stream) {
  ptts_engine *e = g->lm ? g->lm->e : g->mimi->e;
  ENGINE_LOCK(e);
  HIPCHK(hipSetDevice(e->device));  // the calling thread may have another device current (scheduler threads of cuda:N > 0)
  if (g->lm) {
    for (int b = 0; b < g->lm->B; ++b)
      if (g->lm->h_off[b] + 1 > g->lm->cap) return fail(-5, "decode: KV cache capacity exceeded");
  }
  if (g->mimi) CHK(mimi_parts_check(g->mimi, g->mimi_parts, g->mimi_frames));
  {
    if (g->coop_wgs > 0 && g->cu_checked != S(e, stream)) {
      if (g->coop_wgs > stream_cu_count(S(e, stream), e->n_cus))
        return fail(-1, "graph launch: the stream's CU mask is smaller than the cooperative launch captured in this graph");
      g->cu_checked = S(e, stream);
    }
    CoopGuard guard(e->device, S(e, stream), g->coop_wgs, e->n_cus);
    HIPCHK(hipGraphLaunch(g->exec_c && g->lm && g->lm->n_pre > 0 ? g->exec_c : g->exec, S(e, stream)));
    if (guard.finish() < 0) return fail(-2, "graph launch: could not chain the cooperative launch behind its predecessor");
  }
  if (g->lm) for (int b = 0; b < g->lm->B; ++b) g->lm->h_off[b] += g->lm->h_active[b];
  if (g->mimi) mimi_parts_done(g->mimi, g->mimi_parts, g->mimi_frames);
  return 0;
}

extern "C" void ptts_graph_destroy(ptts_graph *g) {
  if (!g) return;
  if (g->lm && g->exec && g->lm->n_graphs > 0) g->lm->n_graphs -= 1;
  if (g->exec) hipGraphExecDestroy(g->exec);
  if (g->graph) hipGraphDestroy(g->graph);
  if (g->exec_c) hipGraphExecDestroy(g->exec_c);
  if (g->graph_c) hipGraphDestroy(g->graph_c);
  if (g->cap_stream) hipStreamDestroy(g->cap_stream);
  delete g;
}

// ------------------------------------------------------------------------------------------------
extern "C" int ptts_set_option(ptts_engine *e, const char *key, int32_t value) {
  if (!e || !key) return fail(-1, "null argument");
  ENGINE_LOCK(e);
  const std::string k(key);
  if (k == "flow_cluster") e->opt_flow_cluster = value != 0;
  else if (k == "lm_cluster") e->opt_lm_cluster = value != 0;
  else if (k == "k_rotate") e->opt_k_rotate = value != 0;
  else if (k == "fuse_res") e->opt_fuse_res = value != 0;
  else if (k == "share_prefix") e->opt_share_prefix = value != 0;
  else if (k == "single_store") e->opt_single_store = value != 0;
  else if (k == "fuse_pcm") e->opt_fuse_pcm = value != 0;
  else if (k == "debug_taps") e->opt_debug_taps = value != 0;
  else if (k == "prefix_cascade") e->opt_cascade = value == 1 ? 423 : value;
  else if (k == "codec_lds_target") {
    if (value < 0 || value > 64 * 1024) return fail(-1, "codec_lds_target must be in [0, 65536]");
    e->opt_codec_lds_target = value;
  }
  else if (k == "flow_max_cus") {
    if (value < 8 || value > e->n_cus) return fail(-1, "flow_max_cus must be in [8, CUs of the device = " + std::to_string(e->n_cus) + "]");
    e->opt_flow_max_cus = value;
  }
  else return fail(-1, "unknown option " + k);
  return 0;
}
extern "C" int ptts_lm_state_error(ptts_lm_state *s, void *stream) {
  if (!s) return fail(-1, "null state");
  int h = 0;
  hipStream_t st = S(s->e, stream);
  HIPCHK(hipSetDevice(s->e->device));
  HIPCHK(hipMemcpyAsync(&h, s->ferr, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemsetAsync(s->ferr, 0, sizeof(int), st));  // read AND clear: one transient timeout is reported once
  HIPCHK(hipStreamSynchronize(st));
  return h != 0;
}
extern "C" int ptts_debug_set_error(ptts_lm_state *s, int32_t value, void *stream) {
  if (!s) return fail(-1, "null state");
  hipStream_t st = S(s->e, stream);
  HIPCHK(hipSetDevice(s->e->device));
  HIPCHK(hipMemsetAsync(s->ferr, value ? 1 : 0, 1, st));  // little endian: byte 0 = the word's low byte
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}
// A stream whose kernels run on a subset of the CUs (hipExtStreamCreateWithCUMask): CUs [cu_lo, cu_hi) of EVERY XCD.
// Measured on MI355X / ROCm 7.2 (tools/cu_mask_probe.py): mask bit i addresses CU i / 8 of XCD i % 8, a kernel runs
// at the speed of its most-masked XCD (workgroups are dealt round-robin over the XCDs), and the mask applies to graph
// launches on the stream as well.  Lets the codec stream leave a slice of every XCD to the latency-bound FlowLM stream.
extern "C" int ptts_stream_create_masked(ptts_engine *e, int32_t cu_lo, int32_t cu_hi, void **out) {
  if (!e || !out) return fail(-1, "bad argument");
  HIPCHK(hipSetDevice(e->device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, e->device));
  const int ncu = prop.multiProcessorCount, nxcd = 8, per = ncu / nxcd, words = (ncu + 31) / 32;
  if (cu_lo < 0 || cu_hi > per || cu_lo >= cu_hi) return fail(-1, "CU range must lie inside [0, CUs per XCD)");
  std::vector<uint32_t> mask(words, 0u);
  for (int i = 0; i < ncu; ++i) {
    const int c = i / nxcd;
    if (c >= cu_lo && c < cu_hi) mask[i >> 5] |= 1u << (i & 31);
  }
  hipStream_t st = nullptr;
  HIPCHK(hipExtStreamCreateWithCUMask(&st, (uint32_t)words, mask.data()));
  *out = (void *)st;
  return 0;
}
// Do two streams run concurrently?  HIP multiplexes streams onto a few hardware queues (GPU_MAX_HW_QUEUES, default 4,
// assigned round-robin at creation): two streams that share a queue execute strictly one after the other, and a
// pipeline whose FlowLM and codec streams collide loses its whole overlap (measured: 0.88 -> 1.15 ms per step, in about
// one of four stream pairs).  Two 200 us single-workgroup spin kernels released together: 1 = overlapped, 0 = serialised.
__global__ void spin_kernel(long long ticks) {
  const long long t0 = wall_clock64();  // 100 MHz
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
}
extern "C" int ptts_streams_overlap(ptts_engine *e, void *stream_a, void *stream_b) {
  if (!e) return fail(-1, "null engine");
  HIPCHK(hipSetDevice(e->device));
  hipStream_t a = S(e, stream_a), b = S(e, stream_b);
  if (a == b) return 0;
  struct Events {  // destroyed on every exit path
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
  } ev;
  for (hipEvent_t &x : ev.e) HIPCHK(hipEventCreate(&x));
  hipEvent_t e0 = ev.e[0], e1 = ev.e[1], e2 = ev.e[2];
  HIPCHK(hipStreamSynchronize(a)); HIPCHK(hipStreamSynchronize(b));
  float worst = 0.f;
  for (int rep = 0; rep < 2; ++rep) {  // first round also warms the kernel up
    HIPCHK(hipEventRecord(e0, a));
    HIPCHK(hipStreamWaitEvent(b, e0, 0));
    spin_kernel<<<1, 64, 0, a>>>(20000);
    spin_kernel<<<1, 64, 0, b>>>(20000);
    HIPCHK(hipEventRecord(e1, a));
    HIPCHK(hipEventRecord(e2, b));
    HIPCHK(hipStreamSynchronize(a)); HIPCHK(hipStreamSynchronize(b));
    float t1 = 0.f, t2 = 0.f;
    HIPCHK(hipEventElapsedTime(&t1, e0, e1));
    HIPCHK(hipEventElapsedTime(&t2, e0, e2));
    worst = std::max(t1, t2);
  }
  return worst < 0.33f ? 1 : 0;  // 0.2 ms each: ~0.21 overlapped, ~0.41 serialised
}
extern "C" int ptts_stream_destroy(void *stream) {
  if (stream) HIPCHK(hipStreamDestroy((hipStream_t)stream));
  return 0;
}
extern "C" int ptts_sync(ptts_engine *e, void *stream) {
  HIPCHK(hipStreamSynchronize(S(e, stream)));
  return 0;
}
extern "C" void *ptts_engine_stream(ptts_engine *e) { return (void *)e->stream; }
// Text-embedding gather of the prefill (reference text.py:74-76, tts_model.py:722-725): d_out[i, :] = d_table[d_tokens[i], :].
// The table stays the caller's tensor (checkpoint "flow_lm.conditioner.embed.weight", f32[n_bins, d_model]).  Asynchronous;
// ids outside [0, n_bins) give zero rows (callers validate ids on the host, where the tokenizer produced them).
extern "C" int ptts_embed_tokens(ptts_engine *e, const float *d_table, int32_t n_bins, const int64_t *d_tokens, int64_t n,
                                 float *d_out, void *stream) {
  if (!e || !d_table || !d_tokens || !d_out || n < 0 || n_bins < 1) return fail(-1, "embed_tokens: bad argument");
  if (n == 0) return 0;
  ENGINE_LOCK(e);
  HIPCHK(hipSetDevice(e->device));
  const int D = e->cfg.d_model;
  embed_gather_kernel<<<cdiv(n * (D / 4), 256), 256, 0, S(e, stream)>>>(d_table, n_bins, D, (const long long *)d_tokens, n, d_out);
  LAUNCHCHK();
  return 0;
}
extern "C" int ptts_copy_to_host_async(ptts_engine *e, void *h_dst, const void *d_src, int64_t bytes, void *stream) {
  HIPCHK(hipMemcpyAsync(h_dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost, S(e, stream)));
  return 0;
}
extern "C" int ptts_timer_start(ptts_engine *e, void *stream) {
  HIPCHK(hipEventRecord(e->ev0, S(e, stream)));
  return 0;
}
extern "C" int ptts_timer_stop_ms(ptts_engine *e, void *stream, float *ms) {
  HIPCHK(hipEventRecord(e->ev1, S(e, stream)));
  HIPCHK(hipEventSynchronize(e->ev1));
  HIPCHK(hipEventElapsedTime(ms, e->ev0, e->ev1));
  return 0;
}
extern "C" int64_t ptts_lm_weight_bytes(ptts_engine *e) { return e->lm_bytes; }
extern "C" int64_t ptts_mimi_weight_bytes(ptts_engine *e) { return e->codec_fp8 ? e->mimi_bytes_f8 : e->codec_bf16 ? e->mimi_bytes_h : e->mimi_bytes; }
