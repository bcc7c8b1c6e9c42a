// The boundary between the four units that share the engine's structures.  Internal (never installed, not part of
// include/ptts.h).
//   ptts.hip           defines the error plumbing, the profiler, the entry-point frame, allocation and packing sections and
//                      the transformer layer: engine construction, the FlowLM states and step, graph capture, the C ABI.
//   ptts_codec.hip     defines the Mimi codec section: the codec state, the frame walks, the output chain behind them, the
//                      decode entry points, the voice-prompt encoder and the fp8 calibration run.
//   ptts_dispatch.hip  defines the dispatcher sections (GEMM, tuner table, attention, reduced-precision codec tiles).  It
//                      alone instantiates gemm_kernel, gemm_lds_kernel, gemm_h_kernel and attn_*: every other unit launches
//                      them through the functions declared here.
//   ptts_debug.hip     the test hooks; defines nothing declared here, and this list is all that test code may reach into.
// Per-thread state (last error, pending launch error, profiler and site, allocation stream in ptts.hip; launch knobs,
// bound tuner and zero line in ptts_dispatch.hip) stays `static` in its one unit and is reached through the functions and
// scopes below, so no unit ever holds a second copy of it.
#pragma once
#include "ptts_kernels.h"
#include "ptts_ext.h"

#include <array>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ptts.h"

#pragma GCC visibility push(hidden)  // links the four units; libptts.so exports none of it

// ---- error plumbing ---------------------------------------------------------------------------------------------------
int fail(int code, const std::string &msg);  // records the calling thread's ptts_last_error(), returns code
#define HIPCHK(x)                                                                                      \
  do {                                                                                                 \
    hipError_t e_ = (x);                                                                               \
    if (e_ != hipSuccess)                                                                              \
      return fail(-2, std::string(#x) + ": " + hipGetErrorString(e_) + " @" + std::to_string(__LINE__)); \
  } while (0)
#define CHK(x)            \
  do {                    \
    int r_ = (x);         \
    if (r_ < 0) return r_; \
  } while (0)
// A launch for which no kernel exists (the dispatchers return nothing: they record the message and launch nothing),
// reported by the entry point's LAUNCHCHK, or by the graph capture that enqueued it
bool launch_err_pending();
int take_launch_err();
void note_launch_err(const std::string &msg);  // kept if none is pending (the first missing kernel is the one reported)
#define LAUNCHCHK()                                     \
  do {                                                  \
    if (launch_err_pending()) return take_launch_err(); \
    HIPCHK(hipGetLastError());                          \
  } while (0)

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// ------------------------------------------------------------------------------------------------
// Optional per-launch profiler: every kernel launch is bracketed by two HIP events on the stream it is
// launched on and tagged with its call site, its kernel name and its ALGORITHMIC bytes / flops.
// Off by default (and always off during graph capture); bench.py switches it on for a few eager steps.
struct ProfRec { std::string site, kernel; double bytes, flops; hipEvent_t a, b; };
struct Profiler { bool on = false; std::vector<ProfRec> recs; };
struct ProfScope {
  hipStream_t st; Profiler *pr; size_t idx;
  ProfScope(hipStream_t st_, const std::string &kernel, double bytes, double flops);
  ~ProfScope();
};
const char *launch_site();  // the call site (SITE in ptts.hip) the calling thread is enqueueing for; "" outside one
void set_launch_site(const char *site);  // SITE of ptts_codec.hip

// ------------------------------------------------------------------------------------------------
struct Lin {  // one packed weight matrix
  float *w = nullptr, *bias = nullptr;
  int N = 0, NT = 0, C = 0, CF = 0, ntaps = 1, KF = 0;
  int cout = 0, stride = 0;  // transposed-conv view
  float *ln_s = nullptr, *ln_c = nullptr;  // LayerNorm folded into this matrix (PRE_LNFOLD)
  // int8 weight-only variant (PTTS_QUANT_*): wq replaces w; ln_g = the LayerNorm gain applied to x on load
  uint8_t *wq = nullptr;
  float *wscale = nullptr, *ln_g = nullptr;
  // bf16 weight variant of a FlowLM Linear (PTTS_LM_BF16): replaces w; packed [NT][KF/2][64][8] (GemmArgs::wfmt == 2)
  void *wb16 = nullptr;
  // split-bf16 twin of a codec matrix (PTTS_CODEC_SPLIT): hi = bf16(w), lo = bf16(w - hi) images beside the fp32 one
  void *wsh = nullptr, *wsl = nullptr;
  // bf16 twin for the reduced-precision codec path (PTTS_CODEC_BF16): packed [NT][ntaps * C/32][64][8], ln_s from the rounded image
  __bf16 *wh = nullptr;
  float *ln_s_h = nullptr;
  // e4m3 twin of a SEANet conv for the fp8 path (PTTS_CODEC_FP8): packed [NT][ntaps * C/32][64][8 bytes] + per-channel scale
  void *wf8 = nullptr;
  float *wscale8 = nullptr;
  size_t bytes() const { return wq ? (size_t)NT * KF * 256 + (size_t)NT * 64 : wb16 ? (size_t)NT * KF * 512 : (size_t)NT * KF * 1024; }
};

struct TrLayer {
  float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *ls1 = nullptr, *ls2 = nullptr;
  Lin qkv, out, ff1, ff2;
};

// Per-engine table of measured tile choices.  `ptts_tune` runs one FlowLM step and one codec frame of a given
// batch on scratch states with `active` set: every GEMM shape met for the first time is timed with every valid
// configuration (caches flushed before each timed launch, as in the real step where ~1 GB streams between two
// uses of a weight) and the fastest is remembered.  Shapes never tuned fall back to pick_cfg.
typedef std::array<int, 13> TuneKey;
struct Tuner {
  std::map<TuneKey, int> table;
  bool active = false;
  void *flush = nullptr;
  size_t flush_bytes = 0;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  std::string log;
};
struct LmLayerP;  // ptts_lm.h
struct ptts_engine {
  ptts_config cfg;
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<void *> allocs;
  std::map<void *, size_t> alloc_bytes;  // engine-owned allocations and their sizes (packed-engine files)
  size_t n_build_allocs = 0;             // allocs[0 .. n) were made by build_engine, in a deterministic order
  const ptts_tensor *blob_dummy = nullptr;  // ptts_create_from_file: every checkpoint lookup resolves to this zero tensor
  int blob_has_encoder = 0;
  std::map<std::string, const ptts_tensor *> tmap;
  // FlowLM
  float *bos = nullptr, *freq_lm = nullptr;
  Lin in_linear;
  std::vector<TrLayer> lm;
  float *outnorm_w, *outnorm_b;
  Lin head, adaln, input_proj, fin;
  struct Res { float *ln_w, *ln_b; Lin l0, l2; };
  std::vector<Res> res;
  Lin te_l0[2], te_l2[2];
  float *te_freqs[2], *te_alpha[2];
  std::map<int, float *> tcomb;  // lsd_steps -> [S][flow_dim]
  std::map<int, float *> tpack;  // K -> the tables of schedules 1..K packed: entry (N, i) at N (N - 1) / 2 + i
  float *te_scratch = nullptr;
  // Mimi
  float *emb_std, *emb_mean, *up_w, *freq_mimi;
  float *quant_w = nullptr;  // quantizer.output_proj weight [C][ldim], plain (mimi_prologue_kernel)
  std::vector<TrLayer> mm;
  Lin conv0, convtr[3], res_a[3], res_b[3], conv_last;
  float *conv_last_w = nullptr, *conv_last_b = nullptr;  // plain checkpoint tensors (bf16 path's last conv)
  bool codec_bf16 = false;
  int64_t mimi_bytes_h = 0;
  // fp8 SEANet convolutions: static activation scales (device copy lives in an engine allocation, so packed-engine files
  // carry it; f8s is its host mirror).  Index: 0 = conv0 output, 1 + 3 i = convtr_i output (ELU'd), 2 + 3 i = hidden
  // activation of residual block i, 3 + 3 i = output of block i (i < 2: the next transposed conv's input)
  bool codec_split = false;  // PTTS_CODEC_SPLIT: the fp32 codec's GEMM launches use the split-bf16 images
  bool codec_fp8 = false;
  float *d_f8s = nullptr;
  float f8s[16] = {};
  int64_t mimi_bytes_f8 = 0;
  int ring = 0;
  // voice-prompt encode path (SEANet encoder, encoder transformer, downsample, speaker projection)
  bool has_encoder = false;
  Lin enc_conv0, enc_res_a[3], enc_res_b[3], enc_down[3], enc_final, enc_downsample, speaker_proj;
  std::vector<TrLayer> enc_tr;
  // test hook (ptts_debug_read_encoder): with "debug_taps" the intermediates of the last ptts_encode_voice stay allocated
  // (enc_keep) until the next call or ptts_destroy; each tap is an FM buffer of `rows` rows and `cols` (% 16 == 0) columns,
  // or (H > 0) the query blocks p, the key / value caches kc / vc of `cap` slots and their offset word: [rows][q | k | v]
  struct EncTap {
    std::string name;
    const float *p;
    int rows, cols;
    const float *kc = nullptr, *vc = nullptr;
    const int *offset = nullptr;
    int H = 0, QB = 0, cap = 0;
  };
  std::vector<EncTap> enc_taps;
  std::vector<void *> enc_keep;
  float *zeros = nullptr;
  int64_t lm_bytes = 0, mimi_bytes = 0;
  Tuner *tuner = nullptr;
  Profiler prof;
  int opt_flow_cluster = 1;
  int opt_lm_cluster = 0;  // measured slower than five launches per layer: kept as an experiment
  LmLayerP *lm_table = nullptr;  // device table of the FlowLM layers for lm_cluster_kernel (null: not eligible)
  int opt_k_rotate = 0;
  long fuse_res_min_rows = 0;
  int opt_codec_lds_target = 56 * 1024;  // see lds_pad()
  int opt_fuse_pcm = 1;      // SEANet's last conv inside the last stage's fused residual block (its output tile never leaves the CU)
  int opt_debug_taps = 0;    // materialise buffers that fused kernels keep on chip (ptts_debug_read of every stage)
  int opt_single_store = 1;  // SEANet transposed convs store their raw output once; the next conv applies ELU on its operand read
  int opt_fuse_res = 1;  // SEANet residual blocks of stages 2 and 3 as one launch each (gemm_lds_kernel<.., NT2>)
  int opt_flow_max_cus = 128;  // resident workgroups of the single-launch flow MLP (<= the CUs its stream may use)
  int opt_share_prefix = 1;    // clones of a batch-1 state share its keys / values (KvPrefix) instead of copying them
  int opt_cascade = 423;       // decode attention of such clones: 10 R + PW of attn_cascade_kernel (0: every sequence on its own)
  int n_cus = 256;             // hipDeviceProp_t::multiProcessorCount of `device` (cooperative grids never exceed it)
  std::recursive_mutex mu;  // entry points that enqueue work or touch tuner / profiler / LSD tables hold it
  int quant_flags = 0;
};
#define ENGINE_LOCK(e) std::lock_guard<std::recursive_mutex> lock_((e)->mu)

struct Scratch {
  float *x = nullptr, *h = nullptr, *ao = nullptr, *ff = nullptr, *q = nullptr, *part = nullptr, *rope = nullptr;
  int MT = 0, QB = 0, splits_cap = 0;
};

struct ptts_lm_state {
  ptts_engine *e;
  int B, cap, MT;
  float *kv = nullptr;  // [L][2][B][H][cap][64]
  int *offset = nullptr;
  int *qlen = nullptr;  // [B] row lengths of the last ragged prefill (ptts_lm_prefill_ragged)
  std::vector<int> h_off;
  Scratch dec, pre;
  // flow head scratch (FM) + io
  float *xlat, *c, *ce, *mod, *latfm, *fx, *fh, *f1;
  float *fstat = nullptr;  // per-tile row statistics of fx (GemmArgs::stat_out / stat_in)
  // single-launch flow MLP (flow_cluster_kernel): exchange slots, flags, error word; sized for `flow_steps` LSD steps
  float *fexch = nullptr;
  unsigned long long *fflags = nullptr;
  int *ferr = nullptr;
  int flow_steps = 0, flow_rt = 1, flow_ng = 1;
  // ptts_lm_state_set_flow_fold: steps of this state compute the AdaLN modulations inside the cluster launch
  // (flow_cluster_mod_kernel) where flow_fold_ok() holds; the exchange slots are then FLOW_MOD_FRAGS fragments wide
  bool flow_fold = false;
  bool mod_stale = false;  // the last enqueued step was folded: `mod` was not written
  // per-row LSD schedules (ptts_lm_state_reserve_row_lsd): capacity K (0: none), packed time-embedding table of
  // schedules 1..K, each row's own step count (0: the step's lsd_steps)
  int lsd_cap = 0;
  const float *lsd_tab = nullptr;
  int *lsd_n = nullptr;
  // shared prefixes (KvPrefix): device table read by the attention kernels, its host mirror, and who owns each row's prefix.
  // An owner with borrowers is not freed by ptts_lm_state_destroy until the last borrower lets go (`zombie`).
  KvPrefix *d_pre = nullptr;
  std::vector<KvPrefix> h_pre;
  std::vector<ptts_lm_state *> pre_owner;
  int casc_mode = -1;   // decode attention: -1 = cascade kernel iff rows borrow prefixes now (eager steps), 0 / 1 forced (captures)
  int n_pre = 0;        // rows of this state that have a prefix
  int borrowers = 0;    // rows of OTHER states whose prefix is this state's cache
  bool zombie = false;
  int n_graphs = 0;   // captured graphs that hold this state's buffer pointers (ensure_flow must not re-allocate under them)
  int coop_wgs = 0;   // workgroups of the cooperative launch of the last enqueued step (0: per-layer launches)
  // single-launch transformer stack (lm_cluster_kernel): exchange slots + flags, allocated on first use
  float *lexch = nullptr;
  unsigned long long *lflags = nullptr;
  float *lat, *lat_prev;  // plain [B][ldim]
  float *eos_logit;
  uint8_t *is_eos;
  // device noise source for perf runs (d_noise == NULL and rng_std > 0): N(0, rng_std^2), counter-based
  float rng_std = 0.f;
  unsigned long long rng_seed = 0;
  int *rng_ctr = nullptr;
  // per-row sampling overrides (ptts_lm_state_set_row_sampling; RowSampling in ptts_kernels.h): marker, {std, clamp, lo,
  // width} of the device generator's draw, EOS threshold
  int *samp_on = nullptr;
  f32x4 *samp_noise = nullptr;
  float *samp_eos = nullptr;
  // per-row seeds (ptts_lm_state_set_row_seed): marker, seed, steps the row has taken since the seed was set
  int *seed_on = nullptr;
  unsigned long long *seed_val = nullptr;
  int *seed_ctr = nullptr;
  bool latfm_noise = false;  // the last enqueued step left its LSD start point in latfm (debug_read "noise")
  RowSampling rsamp() const { return RowSampling{samp_on, samp_noise, samp_eos, seed_on, seed_val, seed_ctr}; }
  // continuous batching: parked rows (active[b] == 0) keep computing but do not advance their position
  int *active = nullptr;
  std::vector<int> h_active;
  size_t kv_plane() const { return (size_t)B * e->cfg.num_heads * cap * 64; }
  float *K(int l) { return kv + (size_t)(2 * l) * kv_plane(); }
  float *V(int l) { return kv + (size_t)(2 * l + 1) * kv_plane(); }
};

// the kinds of output stage in launch order: resampler, stretcher, pitcher, toner, compressor, normaliser, leveler, encoder,
// packer
enum { CH_RS, CH_TS, CH_PS, CH_TN, CH_DY, CH_LN, CH_LV, CH_EN, CH_PK, CH_N };
struct ChainLink {
  void *stage = nullptr;
  float *in = nullptr;
  void *out = nullptr;
  int i16 = 0;
};

// One streaming buffer of the codec: a ring of `slots` frames.  A slot is `stride` floats of allocation and holds `stride`
// elements of `esz` bytes (4 fp32, 2 bf16, 1 e4m3; build_mimi_state decides): a reduced-precision ring is partly filled
struct Ring {
  float *p = nullptr;
  long stride = 0;
  int slots = 0, esz = 4;
  float *slot(int k) const { return p + (size_t)k * stride; }
  long step() const { return stride * 4 / esz; }          // from one slot to the next, in elements (GemmArgs::Xdstride)
  size_t bytes() const { return (size_t)stride * esz; }   // what a slot's elements fill
};

struct ptts_mimi_state {
  ptts_engine *e;
  int B, MTb, MT16;
  // device counters, three ints at `frame` (mimi_tail_kernel): frames through SEANet (frame parity of every conv carry),
  // frames through the transformer (trf = frame + 1: the slot of the hand-over ring), transformer launches (trl = frame + 2:
  // the parity of zq, which a frame pair writes once)
  int *frame = nullptr, *offset = nullptr;
  int *trf() const { return frame + 1; }
  int *trl() const { return frame + 2; }
  int h_frame = 0;  // frames through SEANet, host copy
  int h_tr = 0;     // frames through the transformer, host copy (h_tr - h_frame frames wait in tr_out)
  int splits, splits2 = 1;  // key splits of a frame's attention, and of a frame pair's (32 queries per sequence)
  float *kv = nullptr;  // [ML][2][B][H][ring][64]
  float *zl, *u0, *u, *h, *ao, *ff, *q, *part, *rope;
  // The rings.  tr_out: the transformer's hand-over to SEANet's first conv (fp32 codec: 4 slots, frame f in slot f & 3, so
  // that a frame pair fits beside the frame before it; reduced-precision codecs: the two parity halves).  The others have
  // two slots, the frame parities: zq, SEANet's conv inputs a0 / cbuf / sbuf (ELU'd values), and the fused last stage's
  // ("fuse_pcm") pcm_carry, what each 64-row tile leaves for the first two rows of the next
  Ring zq, tr_out, a0, cbuf[3], sbuf[3], pcm_carry;
  std::array<Ring *, 10> rings() { return {&zq, &tr_out, &a0, &cbuf[0], &sbuf[0], &cbuf[1], &sbuf[1], &cbuf[2], &sbuf[2], &pcm_carry}; }
  float *craw[3], *rbuf[3];  // the raw skip input of a residual block, its hidden activation
  // test hook ("debug_taps", ptts_debug_read "tr_in<l>", "tr_resid<l>", ...): what the next transformer layer overwrites,
  // copied aside.  Block l - 1 of tap_tr (tap_stride floats) holds the input of layer l >= 1 and layer l - 1's stream after
  // attention, attention output, GELU(linear1) and query blocks: tr_tap().  Allocated by the first eager decode that runs
  // with the option; without it nothing is allocated, copied or launched
  float *tap_tr = nullptr;
  size_t tap_nu = 0, tap_nff = 0, tap_nq = 0, tap_stride = 0;  // floats of u / ff / q as build_mimi_state allocates them
  struct TrTap { float *in, *resid, *ao, *ff, *q; };
  TrTap tr_tap(int l) const {  // l = 1 .. layers - 1
    float *p = tap_tr + (size_t)(l - 1) * tap_stride;
    return TrTap{p, p + tap_nu, p + 2 * tap_nu, p + 3 * tap_nu, p + 3 * tap_nu + tap_nff};
  }
  int h_tr_last = 1;  // frames of the last transformer launch (the query blocks hold that many 16-query blocks per head)
  int tap_frame = -1;  // h_tr when the copies in tap_tr were last enqueued: they are the last launch's iff == h_tr - h_tr_last
  int rows[4];  // rows per sequence at each SEANet stage
  float *pcm_dbg;
  int16_t *pcm_i16 = nullptr;
  float *pcm_part = nullptr;  // fused last stage: per-row partial PCM
  // the output stages behind the codec (ptts_mimi_set_*), one link per kind in launch order.  A link is empty (stage == nullptr)
  // or holds the stage, the f32 device buffer it reads (`in`; nullptr: the frame's PCM) and what it writes (`out`, int16 with
  // `i16`, else f32; the encoder's bytes; the packer reads the encoder's bytes through `in` and writes ring lines).
  // mimi_frame_enqueue in ptts_codec.hip states the two cases in which a stage writes another link's `in` instead
  ChainLink chain[CH_N];
  size_t kv_plane() const { return (size_t)B * e->cfg.m_heads * e->ring * 64; }
  float *K(int l) { return kv + (size_t)(2 * l) * kv_plane(); }
  float *V(int l) { return kv + (size_t)(2 * l + 1) * kv_plane(); }
};

// ---- the Mimi codec (ptts_codec.hip) ----------------------------------------------------------------------------------
// parts of a frame: PART_TR the transformer (one frame, or a pair with a second latent), PART_SEANET one SEANet frame
// (with the PCM and the int16 copy); both = the whole frame.  The reduced-precision codecs take single frames only.
enum { PART_TR = 1, PART_SEANET = 2, PART_ALL = 3 };
int mimi_frame_enqueue(hipStream_t st, ptts_engine *e, ptts_mimi_state *s, const float *d_latent, float *d_pcm,
                       int parts = PART_ALL, const float *d_latent2 = nullptr);
int mimi_parts_check(const ptts_mimi_state *s, int parts, int frames);
void mimi_parts_done(ptts_mimi_state *s, int parts, int frames);
int calibrate_fp8_codec(ptts_engine *e);  // build_fp8_codec: fills e->d_f8s from a run of the bf16 codec
bool seanet_single_store(const ptts_engine *e, int i);  // stage i's transposed conv stores its raw output only
bool seanet_fuses_pcm(const ptts_mimi_state *s);  // the last conv rides in the last block: sbuf[2] is written with "debug_taps" only
bool resblock_fused(const ptts_mimi_state *s, int i);  // fp32 codec: stage i's residual block is one launch, rbuf[i] is not written
void calib_latent(hipStream_t st, float *lat, int n, unsigned frame);  // the latents of calibration frame `frame`, [8][ldim]

// ---- the transformer layer (ptts.hip; the FlowLM, the codec and the voice encoder run it) -----------------------------
struct TrCtx {
  int D, H, FF, MT, M, Tq, QB, cap, ring, ctx, splits;
  float *x_in;       // residual stream input (FM, F = D/16)
  float *x;          // residual stream after attention (may equal x_in)
  float *x_out;      // residual stream output of the layer (dbl-buffered if out_ds != 0)
  long out_ds;
  const int *par;
  int out_ring = 0;  // x_out is the codec's hand-over ring (GemmArgs::yring): frames in the launch, 0: parity halves
  float *h, *ao, *ff, *q, *part;
  float *Kc, *Vc;
  const int *offset;
  const KvPrefix *pre = nullptr;  // shared voice prefixes of the sequences (FlowLM states) or null
  int layer = 0;
  int cascade = 0;                // decode steps: attn_cascade_kernel tile shape (10 R + PW) or 0
  const int *qlen = nullptr;      // ragged prefill: real rows of each sequence (GemmArgs::qlen, AttnArgs::qlen) or null
  const float *rope;  // [M][32][2]
  float *tap_x = nullptr;  // test hook: receives a copy of the stream after attention (x), which x_out may overwrite
  double kv_keys;  // sum over sequences of the keys attended (profiling only)
  const char *tag;
};

void run_tr_layer(hipStream_t st, const TrLayer &T, const TrCtx &c);

// ---- entry-point frame, allocation and packing ------------------------------------------------------------------------
hipStream_t S(ptts_engine *e, void *stream);
void bind_engine(ptts_engine *e);
struct AllocScope {  // dalloc's zero fill is queued on the stream of the calling thread's innermost AllocScope
  hipStream_t prev;
  explicit AllocScope(hipStream_t st);
  ~AllocScope();
};
int dalloc(ptts_engine *e, void **p, size_t bytes);
template <typename T>
static int dallocT(ptts_engine *e, T **p, size_t n) {
  return dalloc(e, (void **)p, n * sizeof(T));
}
struct PackPart { std::string w, b; int N; };
int pack_lin(ptts_engine *e, Lin *L, const std::vector<PackPart> &parts, int C, int ntaps, int mode = 0, int cout = 0,
             int stride = 0, const std::string &ln_w = "", const std::string &ln_b = "", int creal = 0, int wfmt = 0);
int pack_lin_h(ptts_engine *e, Lin *L, const std::string &wname, int N, int C, int ntaps, int mode = 0, int cout = 0,
               int stride = 0, const std::string &ln_w = "");

// ---- the fp32 / int8 / bf16 / split GEMM dispatcher -------------------------------------------------------------------
constexpr int kNumCfg = 18;  // 16, 17 appended in round 2 (older cache files stay valid)
// the dispatcher's per-thread knobs for the launches inside the scope: dynamic-LDS target (see lds_pad), "k_rotate", and
// whether mk_gemm hands out the split-bf16 images of a PTTS_CODEC_SPLIT engine; the previous values return at its end
struct KnobScope {
  int lds, krot;
  bool split;
  KnobScope(int lds_target, int k_rotate, bool use_split = false);
  ~KnobScope();
};
void bind_dispatch(const ptts_engine *e);    // the calling thread's tuner, zero line and "k_rotate" (bind_engine calls it)
void unbind_dispatch(const ptts_engine *e);  // ptts_destroy: the calling thread forgets e's tuner
bool pre_supported(int wfmt, int pre);
bool cfg_valid(int cfg, const GemmArgs &a, int pre);
int choose_cfg(hipStream_t st, const GemmArgs &a, int pre);
void launch_gemm_cfg(hipStream_t st, const GemmArgs &a, int pre, int cfg, std::string *label = nullptr);
GemmArgs mk_gemm(const Lin &L, const float *X, int XF, int MT, int M);
void launch_gemm(hipStream_t st, const GemmArgs &a_in, int pre);  // choose_cfg + launch_gemm_cfg, or the launch error
bool resblock_fusable(const Lin &A, const Lin &Bl, int MT);
void launch_resblock(hipStream_t st, GemmArgs a, const Lin &Bl, int pre = PRE_NONE);

// ---- the attention dispatcher -----------------------------------------------------------------------------------------
struct AttnKernelInfo { int family, nw, pw, depth, ns, code; const char *name; };
constexpr int kNumAttn = 17;
extern const AttnKernelInfo kAttn[kNumAttn];
int attn_splits(int base, int max_tiles);
bool attn_valid(int k, const AttnArgs &a);
int choose_attn(const AttnArgs &a, int BH, int cascade);
int launch_attention(hipStream_t st, const AttnArgs &at, int BH, int cascade, int kernel, double bytes, double flops,
                     std::string *label = nullptr);

// ---- the reduced-precision codec's tiles ------------------------------------------------------------------------------
int choose_h_tile(const GemmArgs &a);
GemmArgs gemm_h_args(const GemmArgs &a_in, int pre, const Lin &L);
void launch_h_tile(hipStream_t st, const GemmArgs &a, int pre, int cfg, std::string *label = nullptr);
void launch_gemm_h(hipStream_t st, const GemmArgs &a_in, int pre, const Lin &L);  // gemm_h_args + choose_h_tile + launch_h_tile
void launch_f8_tile(hipStream_t st, const GemmArgs &g, int cfg, std::string *label = nullptr);

#pragma GCC visibility pop
