/*
 * ptts.h -- C ABI of the MI355X (gfx950) Pocket-TTS decode hot path.
 *
 * The reference (kyutai-labs/pocket-tts) is pure Python and has no FFI; the seam this
 * library replaces is the set of Python call sites listed per entry point below
 * (paths relative to the reference checkout).  All pointers named `d_*` are DEVICE
 * pointers to fp32 data (e.g. torch `tensor.data_ptr()` on a ROCm device); `h_*` are host
 * pointers.  `stream` is a `hipStream_t` passed as `void*` (NULL = the engine's own
 * stream).  Every function returns 0 on success or a negative error code;
 * `ptts_last_error()` returns the message (per calling thread).  No exceptions cross the ABI.
 *
 * Threading contract.  The library keeps NO process-global mutable state: profiler, tile table, LSD tables and the
 * allocation stream live in the engine or in the calling thread.  Engines are independent: any number of engines
 * (one per GPU, or several on one GPU) may be driven from different threads at the same time.  Entry points that
 * enqueue work on an engine serialise on that engine's mutex, so two threads MAY share one engine (e.g. a batching
 * scheduler thread and a request thread); device-side ordering between their calls is the caller's business
 * (streams / events).  A state or graph handle is not re-entrant: one thread per ptts_lm_state / ptts_mimi_state /
 * ptts_graph at a time.  Decode steps contain cooperative kernels (the single-launch flow MLP: all its workgroups must
 * be resident together).  Such a launch never exceeds the device's CU count or the `flow_max_cus` option, a launch on a
 * CU-masked stream with fewer CUs than its grid is refused (-1), and the library admits only as many of these steps at a
 * time per DEVICE as their grids fit the chip together (two for the default 128-workgroup grid): step k waits ON THE GPU
 * for step k - 2 through a small per-device ring of events (no host wait), so steps of different states queued on
 * different streams are safe and overlap pairwise.  The one process-wide object is that per-device ring (with its mutex).
 */
#ifndef PTTS_H_
#define PTTS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTTS_ABI_VERSION 1

typedef struct ptts_engine ptts_engine;         /* weights + kernels for one GPU         */
typedef struct ptts_lm_state ptts_lm_state;     /* FlowLM KV caches of B sequences       */
typedef struct ptts_mimi_state ptts_mimi_state; /* Mimi streaming state of B sequences   */
typedef struct ptts_graph ptts_graph;           /* a captured hipGraph of one step       */
typedef struct ptts_resampler ptts_resampler;   /* output sample rates of B sequences    */
typedef struct ptts_stretcher ptts_stretcher;   /* speaking rates of B sequences         */
typedef struct ptts_pitcher ptts_pitcher;       /* pitches of B sequences                */
typedef struct ptts_leveler ptts_leveler;       /* output levels of B sequences          */
typedef struct ptts_loudnorm ptts_loudnorm;     /* loudness targets of B sequences       */
typedef struct ptts_tone ptts_tone;             /* tones (equaliser) of B sequences      */
typedef struct ptts_dynamics ptts_dynamics;     /* dynamics (compressor) of B sequences  */
typedef struct ptts_encoder ptts_encoder;       /* output encodings of B sequences       */
typedef struct ptts_flac ptts_flac;             /* output compression of B sequences     */

/* Model dimensions: pocket_tts/config/english.yaml:7-61 (schema utils/config.py:15-118). */
typedef struct ptts_config {
  int32_t d_model, num_heads, num_layers, ff_dim, ldim; /* flow_lm.transformer, quantizer.dimension */
  int32_t flow_dim, flow_depth;                         /* flow_lm.flow                              */
  float max_period;                                     /* flow_lm.transformer.max_period            */
  int32_t m_dim, m_heads, m_layers, m_ff, m_context;    /* mimi.transformer (d_model == seanet dim)  */
  float m_max_period;
  int32_t n_filters, ratios[3], kernel_size, res_kernel_size, last_kernel_size, compress;
  int32_t upsample_stride;                              /* encoder_frame_rate / frame_rate = 16      */
} ptts_config;

/* One checkpoint tensor, name as in TTSModel.state_dict() (tts_model.py:206-210). */
typedef struct ptts_tensor {
  const char *name;
  const float *d_data;
  int64_t numel;
} ptts_tensor;

int ptts_abi_version(void);
const char *ptts_last_error(void);

/* Builds the engine: packs the checkpoint tensors it needs into MFMA-fragment order on
 * `device`.  Replaces TTSModel._from_pydantic_config_with_weights (tts_model.py:129-230)
 * for the decode-side modules.  The caller may free the source tensors afterwards. */
int ptts_create(const ptts_config *cfg, const ptts_tensor *tensors, int32_t n_tensors, int32_t device,
                ptts_engine **out);
/* Same, with int8 weights for layer groups of the FlowLM transformer: replaces
 * quantization.apply_dynamic_int8(flow_lm, groups) (quantization.py:60-128; load_model(quantize=True) uses
 * {"attention", "ffn"}, tts_model.py:312-315).  The reference quantises activations dynamically as well (torch.ao /
 * torchao CPU kernels); here the weights are int8 per output channel (symmetric) and activations and accumulation
 * stay fp32, so the result is closer to the fp32 model than the reference's int8 path.  flags = 0 == ptts_create. */
#define PTTS_QUANT_ATTENTION 1 /* self_attn.in_proj, self_attn.out_proj */
#define PTTS_QUANT_FFN 2       /* linear1, linear2 */
/* Reduced-precision CODEC (BASELINE.json config #5, second half; no reference counterpart, parity unpinned): the Mimi
 * decoder-transformer GEMMs and the SEANet decoder convolutions run with bf16 weights and bf16 activations, fp32
 * accumulation (v_mfma_f32_16x16x32_bf16) and fp32 epilogue math; attention, the KV ring and the FlowLM stay fp32, so
 * EOS decisions / frame counts are those of the fp32 model.  Quality: tests/test_gpu_bf16.py (SNR vs the fp32 path). */
#define PTTS_CODEC_BF16 4
/* fp8 CODEC CONVOLUTIONS (BASELINE.json config #5: "fp8 MFMA codec convs"; no reference counterpart - the reference never
 * quantises Mimi, docs/quantization.md:67-76 - parity unpinned, judged by SNR and frame-count equality): the SEANet decoder
 * convolutions (seanet.py:141-180, conv.py:93-163) run on v_mfma_f32_16x16x32_fp8_fp8 with OCP e4m3 weights (one fp32
 * scale per output channel) and e4m3 activations (one fp32 scale per tensor, fixed at load time from a calibration
 * frame), fp32 accumulation and epilogue math; the Mimi decoder transformer runs as under PTTS_CODEC_BF16 (bf16), the
 * FlowLM stays fp32.  Exclusive with PTTS_CODEC_BF16.  Quality: tests/test_gpu_fp8.py. */
#define PTTS_CODEC_FP8 8
/* bf16 WEIGHTS for the FlowLM transformer's Linear layers (SURVEY 8(f).4 "bf16 / int8 per-channel LM weights"; same
 * hook as the int8 groups: quantization.py:91-128): weights rounded to bf16 once at load (a LayerNorm gain multiplied in
 * first), and the activation operand of each of the four Linear layers rounded to bf16 in registers, both fed to
 * v_mfma_f32_16x16x32_bf16; the residual stream, the LayerNorm statistics (taken from the unrounded row), q / k / v, the
 * KV cache, attention, accumulation and every epilogue stay fp32.  Half the weight bytes of a decode step.  The
 * single-launch stack (lm_cluster) is fp32 only: with this flag or an int8 group the option falls back to the per-layer
 * launches.  Exclusive with the int8 groups.  Quality: tests/test_gpu_quant.py; every call against fp64:
 * tests/test_gpu_lm_formats.py. */
#define PTTS_LM_BF16 16
/* ERROR-COMPENSATED bf16 for the codec's GEMMs (an experiment reported beside the fp32 headline): every Linear / conv of the
 * Mimi decoder as hi*hi + hi*lo + lo*hi of bf16 halves (hi = bf16(v), lo = bf16(v - hi)) on the bf16 MFMA with fp32
 * accumulation; activations, buffers, attention and epilogues stay fp32.  ~2^-16 relative error per product; passes the fp32
 * codec's parity tests at their tolerance (tests/test_gpu_split.py).  Exclusive with the bf16 / fp8 codec. */
#define PTTS_CODEC_SPLIT 32
int ptts_create_ex(const ptts_config *cfg, const ptts_tensor *tensors, int32_t n_tensors, int32_t device,
                   int32_t quant_flags, ptts_engine **out);
/* Packed-engine files ("offline packer"): ptts_engine_save writes everything ptts_create[_ex] built on
 * the device (MFMA-fragment-ordered weights, int8 / bf16 images, LayerNorm-fold vectors) to one file;
 * ptts_create_from_file rebuilds the engine from it without the checkpoint and without packing or quantising again
 * (the reference re-quantises at every load: quantization.py:60-88, tts_model.py:312-313).  The file is tied to this
 * library's ABI version and layout; a mismatch is reported (-3), never loaded. */
int ptts_engine_save(ptts_engine *e, const char *path);
int ptts_create_from_file(const char *path, int32_t device, ptts_engine **out);
void ptts_destroy(ptts_engine *e);

/* ---- FlowLM state: init_states(flow_lm, B, T) (stateful_module.py:7-16, transformer.py:46-57) */
int ptts_lm_state_create(ptts_engine *e, int32_t batch, int32_t t_cap, ptts_lm_state **out);
void ptts_lm_state_destroy(ptts_lm_state *s);
/* zero offsets (fresh init_states); also clears every row's sampling override (ptts_lm_state_set_row_sampling), LSD
 * override (ptts_lm_state_set_row_lsd) and seed (ptts_lm_state_set_row_seed) */
int ptts_lm_state_reset(ptts_lm_state *s, void *stream);
/* Import / export one layer in the reference layout cache f32[2, src_batch, t, H, 64] (device) with
 * `t` valid positions (transformer.py:32-36; voice files tts_model.py:1047-1072).  On import,
 * src_batch == 1 broadcasts to every row of the state, and every row's offset is set to t. */
int ptts_lm_state_import(ptts_lm_state *s, int32_t layer, const float *d_cache, int32_t src_batch,
                         int32_t t, void *stream);
int ptts_lm_state_export(ptts_lm_state *s, int32_t layer, float *d_cache, int32_t t, void *stream);
/* dst <- src (replaces copy.deepcopy(model_state), tts_model.py:637-638); src batch 1 broadcasts.
 * The clone starts a new generation: its pending input latent is BOS (tts_model.py:748-753).
 * With "share_prefix" (default) a clone of a one-sequence state borrows its leading keys instead of copying them: see
 * ptts_set_option.  These calls, destroy, reset, import and set_row_active serialise on the engine's mutex. */
int ptts_lm_state_copy(ptts_lm_state *dst, const ptts_lm_state *src, void *stream);
/* row `row` of dst <- the single sequence of src (batch 1): assembles a batch from utterances prefilled one by
 * one with different prompt lengths; every kernel reads per-row offsets, so rows need not be in sync (the
 * reference requires equal offsets across the batch: transformer.py:12-13). */
int ptts_lm_state_copy_row(ptts_lm_state *dst, int32_t row, const ptts_lm_state *src, void *stream);
/* the same from row `src_row` of a batch state: a group of utterances with the same voice and text length is prefilled
 * as ONE batch (one GEMM pass instead of one per utterance) and its rows are then dealt to their slots */
int ptts_lm_state_copy_row_from(ptts_lm_state *dst, int32_t row, const ptts_lm_state *src, int32_t src_row, void *stream);
/* offsets of all rows to host (transformer.py:14 `.item()`; synchronises the stream) */
int ptts_lm_state_offsets(ptts_lm_state *s, int32_t *h_offsets, void *stream);

/* Text or voice conditioning d_emb f32[B, t, d_model] run through every layer; only the KV cache
 * is kept.  Replaces _run_flow_lm_and_increment_step(text_tokens=.. | audio_conditioning=..)
 * (tts_model.py:317-346, call sites :723, :899). */
int ptts_lm_prefill(ptts_engine *e, ptts_lm_state *s, const float *d_emb, int32_t t, void *stream);
/* Ragged prefill: rows of different lengths in one pass.  d_emb f32[B, t_max, d_model]; h_len = HOST array [B] with
 * 0 <= h_len[b] <= t_max.  The first h_len[b] positions of row b are real, the rest is padding whose contents are arbitrary.
 *   Result: row b ends as if ptts_lm_prefill had run on it alone with t = h_len[b]: its keys and values land at positions
 *     [offset[b], offset[b] + h_len[b]), and offset[b] and its host mirror advance by h_len[b].
 *   Zero length: a row with h_len[b] == 0 is not touched at all.
 *   Cache isolation: no cache slot at or beyond offset[b] + h_len[b] is written, and none of another row or head.
 *   Padding independence: padding never influences a real position or the cache; the valid outputs are bitwise independent
 *     of what the padding of d_emb holds (any bit pattern, NaN included).
 *   Capacity: checked per row, offset[b] + h_len[b] <= capacity, else -5 and nothing is enqueued; t_max plays no part in it.
 *     A row that ends exactly at the capacity while offset[b] + t_max lies past it works, and nothing past the capacity is read.
 *   Errors: -1 for an h_len[b] outside [0, t_max] or t_max < 1.  All lengths 0: returns 0 and enqueues nothing.
 *   Ordering: asynchronous on `stream`, like ptts_lm_prefill; h_len may be freed or overwritten as soon as the call returns.
 * The layer stack still runs on B * t_max rows (padding rows cost GEMM time, no weight traffic); ptts_lm_prefill itself,
 * its launches and its results are unchanged. */
int ptts_lm_prefill_ragged(ptts_engine *e, ptts_lm_state *s, const float *d_emb, const int32_t *h_len, int32_t t_max,
                           void *stream);
/* The text-embedding gather in front of a text prefill (LUTConditioner._get_condition, conditioners/text.py:74-76):
 * d_out f32[n, d_model] <- d_table[d_tokens[i]] for int64 ids; d_table = the checkpoint tensor
 * "flow_lm.conditioner.embed.weight" f32[n_bins, d_model], which stays the caller's.  Asynchronous on `stream`; an id outside
 * [0, n_bins) gives a zero row (validate ids on the host, where the tokenizer made them). */
int ptts_embed_tokens(ptts_engine *e, const float *d_table, int32_t n_bins, const int64_t *d_tokens, int64_t n,
                      float *d_out, void *stream);

/* One autoregressive step = _run_flow_lm_and_increment_step(backbone_input_latents=..)
 * (tts_model.py:758-760 -> flow_lm.py:96-139).
 *   d_latent_in  f32[B, ldim]  rows of NaN mean BOS; NULL = previous step's output (or BOS after reset)
 *   d_noise      f32[B, ldim]  starting point of the LSD flow (flow_lm.py:131-137); NULL = zeros (temp 0)
 *   d_latent_out f32[B, ldim], d_eos_logit f32[B], d_is_eos u8[B] (logit > eos_threshold); any may be NULL */
int ptts_lm_decode_step(ptts_engine *e, ptts_lm_state *s, const float *d_latent_in, const float *d_noise,
                        int32_t lsd_steps, float eos_threshold, float *d_latent_out, float *d_eos_logit,
                        uint8_t *d_is_eos, void *stream);
/* Perf-run noise source: when d_noise is NULL and temp > 0 the step draws N(0, temp) itself from a
 * counter-based device generator (the reference draws from torch's global CPU generator,
 * flow_lm.py:131-135, which cannot be reproduced on device; parity runs pass d_noise or temp 0). */
int ptts_lm_set_noise(ptts_lm_state *s, float temp, uint64_t seed);
/* Per-row seeds (a request's own random stream, wherever the request runs).  The generator above keys the draw of row m,
 * column k by (the state's seed, the state's step counter, m * ldim + k): what a sequence draws depends on the row it sits
 * in and on how many steps the state has run.  After ptts_lm_state_set_row_seed(s, row, seed) the draws of `row` are
 * keyed by (seed, j, k) instead, j = the number of steps the row has taken, while active, since the call (the call zeroes
 * it; it advances once per step whatever the row's number of LSD steps).  The same hash, Box-Muller / inverse-CDF
 * truncated normal and std / clamp selection (the row's sampling override, else the state's temperature) apply, so a
 * seeded row at its j-th step draws what row 0 of a one-row state seeded `seed` draws at its step counter j.  The draws do
 * not depend on the row index, the batch size, the other rows or the state's own seed and counter.  Rows without a seed
 * draw exactly as before; d_noise != NULL is still used as given, for every row.  The kernels read seed and counter from
 * device memory at run time: graphs captured before the call pick them up.  set / clear are stream-ordered on `stream`
 * and reject a row out of range (-1).  ptts_lm_state_reset clears every seed; the copy calls leave the destination's seeds
 * as they are (set the seed after ptts_lm_state_copy_row_from, before the row's first step).  Seeds that differ by a
 * multiple of 0x9E3779B97F4A7C15 (mod 2^64) give shifted copies of one stream: derive related seeds by hashing. */
int ptts_lm_state_set_row_seed(ptts_lm_state *s, int32_t row, uint64_t seed, void *stream);
/* row `row` returns to the state's seed and step counter; stream-ordered */
int ptts_lm_state_clear_row_seed(ptts_lm_state *s, int32_t row, void *stream);
/* Per-row sampling override (a server's per-request settings in one continuous batch; the reference takes them per model,
 * flow_lm.py:131-137, tts_model.py:756-760).  Row `row` of later steps then uses, instead of the state's ptts_lm_set_noise
 * temperature and the step's eos_threshold argument:
 *   temp           its own std = sqrt(temp) for the device generator (d_noise == NULL only; external noise is used as
 *                  given).  Without a clamp the draws are bitwise those of a state whose ptts_lm_set_noise used `temp`
 *                  (same seed, same row); temp 0 gives zeros.
 *   noise_clamp    > 0: a truncated normal on [-noise_clamp, noise_clamp], drawn by the inverse CDF like
 *                  torch.nn.init.trunc_normal_ (flow_lm.py:134-137); <= 0: no clamp
 *   eos_threshold  the row's EOS flag is logit > eos_threshold
 * The kernels read the values from device memory at run time: graphs captured before the call pick them up.  The write
 * is stream-ordered on `stream`, like ptts_lm_state_copy_row_from.  Rejects a row out of range and a temp that is
 * negative or not finite (-1).  ptts_lm_state_reset clears every override; ptts_lm_state_copy / _copy_row / _copy_row_from
 * leave the destination's overrides as they are (they copy sequences, not sampling settings). */
int ptts_lm_state_set_row_sampling(ptts_lm_state *s, int32_t row, float temp, float noise_clamp, float eos_threshold,
                                   void *stream);
/* row `row` returns to the state's defaults (ptts_lm_set_noise temperature, the step's eos_threshold); stream-ordered */
int ptts_lm_state_clear_row_sampling(ptts_lm_state *s, int32_t row, void *stream);
/* Per-row LSD schedules (a server's per-request lsd_decode_steps in one continuous batch; the reference takes it per model,
 * flow_lm.py:19-40).  ptts_lm_state_reserve_row_lsd gives the state a capacity K (1 <= K <= 64): its flow buffers are sized
 * for K Euler steps and the time embeddings of every schedule 1..K are built.  Afterwards
 * ptts_lm_state_set_row_lsd makes row `row` of later steps run its own `n` Euler steps (1 <= n <= K) instead of the
 * step's lsd_steps; rows without an override keep the step's lsd_steps.  Each row's latent is bitwise that of a state
 * without the capacity stepped with lsd_steps = n when n >= 2 (n = 1: within fp32 rounding).  A step of a state with a
 * capacity takes as long as its slowest group of 16 rows.
 *   reserve   -1 for K out of range and for a state with captured graphs (reserve before capturing); never shrinks the
 *             capacity.  A state without a capacity enqueues exactly the steps it did before.
 *   set       -1 for a row out of range, n < 1, n > K, or a state without a capacity.
 * The kernels read the counts from device memory at run time: graphs captured after the reservation pick up later
 * calls.  set / clear are stream-ordered on `stream`.  ptts_lm_state_reset clears every override; the copy calls leave the
 * destination's overrides as they are. */
int ptts_lm_state_reserve_row_lsd(ptts_lm_state *s, int32_t K, void *stream);
int ptts_lm_state_set_row_lsd(ptts_lm_state *s, int32_t row, int32_t n, void *stream);
/* row `row` returns to the step's lsd_steps; stream-ordered */
int ptts_lm_state_clear_row_lsd(ptts_lm_state *s, int32_t row, void *stream);
/* Flow fold (per state, default off): with on != 0 later steps of the state skip the AdaLN modulation GEMM (`flow.adaln`)
 * and the single-launch flow MLP computes the modulations itself while its workgroups wait for each other (kernel label
 * `flow_cluster_mod@<threads>` under the site `flow.cluster`).  Taken only where the single-launch flow MLP runs with one
 * row tile per cluster, flow_dim <= 256 or in 400..512 (1, 2 or 4 k-fragments per worker wave), fp32 flow weights and no per-row LSD capacity; a state
 * outside of that enqueues exactly the launches it did before.  Results agree with the unfolded step within fp32
 * rounding (another summation order).  The state's exchange buffers are re-allocated, so:
 *   -1 for a state with captured graphs when the call would change the switch (set it before capturing). */
int ptts_lm_state_set_flow_fold(ptts_lm_state *s, int32_t on, void *stream);
/* Offset, in floats, of fragment `f` (of `nf` per slot) of producer `j`'s exchange slot for (row group, phase, row tile) of
 * the single-launch flow MLP, with `fdf` producers, `rt` row tiles per group and `nph` phases; (fdf, rt, nph, nf, grp = number
 * of groups, 0, 0, 0, 0) is the buffer's size.  The function the kernels and the allocation use; no GPU needed. */
int64_t ptts_flow_slot_offset(int32_t fdf, int32_t rt, int32_t nph, int32_t nf, int32_t grp, int32_t p, int32_t t, int32_t j,
                              int32_t f);
/* The folded kernel's schedule: the 16-column tiles of the AdaLN output (blocks' [shift | scale | gate], then the final
 * layer's [shift | scale], `fdf` tiles each) that workgroup `j` computes at the top of phase `ph` (0 .. 2 depth + 1) of an
 * LSD step: *n tiles (0 .. 2), the first at the returned tile, the second `fdf` tiles later.  No GPU needed. */
int32_t ptts_flow_mod_tiles(int32_t fdf, int32_t depth, int32_t ph, int32_t j, int32_t *n);
/* device pointer of the state's own copy of the latest latent f32[B, ldim] */
const float *ptts_lm_latent_ptr(ptts_lm_state *s);

/* ---- Mimi streaming decode: init_states(mimi, B, ..) + _decode_audio_worker body
 *      (tts_model.py:444-455 -> mimi.py:89-94) */
int ptts_mimi_state_create(ptts_engine *e, int32_t batch, ptts_mimi_state **out);
void ptts_mimi_state_destroy(ptts_mimi_state *s);
int ptts_mimi_state_reset(ptts_mimi_state *s, void *stream);
/* ---- continuous batching (the reference serves one request at a time, main.py:80-181) ----
 * A batch state is a set of slots.  An utterance JOINS slot `row` with ptts_lm_state_copy_row (its prefilled
 * batch-1 state) + ptts_mimi_state_reset_row (zero conv carries == init_states for that sequence,
 * stateful_module.py:7-16) and LEAVES with ptts_lm_state_set_row_active(row, 0): a parked row keeps flowing
 * through the batched kernels but stays at position 0.  Captured graphs stay valid across joins / leaves. */
int ptts_mimi_state_reset_row(ptts_mimi_state *s, int32_t row, void *stream);
int ptts_lm_state_set_row_active(ptts_lm_state *s, int32_t row, int32_t active, void *stream);
/* 16-bit PCM straight from the codec's last kernel: (clamp(x, -1, 1) * 32767) truncated, the conversion of
 * StreamingWAVWriter.write_pcm_data (data/audio.py:79).  i16[B, frame_samples], device or pinned host. */
int ptts_mimi_set_pcm_i16(ptts_mimi_state *s, int16_t *d_pcm_i16);
/* ---- Output sample rates (no reference counterpart: the reference writes the codec's own rate, data/audio.py:69-72).
 * A resampler holds, for B sequences, the polyphase tables of a list of rates, each row's rate and each row's history of
 * PTTS_RS_HIST = 64 input samples; it turns one codec frame f32[B, frame_samples] into out[B, out_max] with row b's
 * out_n(rate of b) = frame_samples * up / down samples at the front of its line (the rest of the line is not written).
 * Rate i is the causal polyphase FIR y[N] = sum_k h[k] x_up[N down_i - k] (scipy.signal.upfirdn(h, x, up, down); input
 * before the stream's start is zero) with h_poly[ph][j] = h[ph + j * up] given as h_up[i] * h_taps[i] floats; the tables
 * follow each other in h_tables (n_table_floats in all).  up = down = 1 is an exact copy whatever its table holds.  A rate
 * is refused (-1) unless frame_samples * up % down == 0 (whole outputs per frame, phase 0 at every frame start),
 * taps - 1 <= 64 (the history covers the filter's reach) and out_n <= 4 * frame_samples: with these every index the kernel
 * forms is in bounds by construction (csrc/ptts_resample.h).  Filter design: pocket_tts_amd/resample.py.  Every row starts
 * at rate 0 with a zero history. */
int ptts_resampler_create(ptts_engine *e, int32_t batch, const int32_t *h_up, const int32_t *h_down, const int32_t *h_taps,
                          int32_t n_rates, const float *h_tables, int64_t n_table_floats, ptts_resampler **out);
/* after every decode / graph that uses it has finished, and after ptts_mimi_set_resampler(state, NULL, ..) on its states */
void ptts_resampler_destroy(ptts_resampler *rs);
/* a new utterance joins `row`: its rate from now on, and a zero history.  Stream-ordered on `stream`; captured graphs pick
 * the rate up (the kernel reads it from device memory).  -1 for a row or a rate index out of range; nothing is enqueued. */
int ptts_resampler_set_row(ptts_resampler *rs, int32_t row, int32_t rate_index, void *stream);
/* One frame: d_pcm_in f32[B, frame_samples] (DEVICE memory) -> out [B, out_max], f32 or (is_i16) int16 converted as
 * ptts_mimi_set_pcm_i16 converts, device or pinned host; then every row's history <- the frame's last 64 samples (a second
 * launch: the blocks of a row read the history concurrently).  out_max = the largest out_n of the rates. */
int ptts_resample_frame(ptts_resampler *rs, const float *d_pcm_in, void *out, int32_t is_i16, void *stream);
/* ---- The output chain.  The nine ptts_mimi_set_* below follow one rule, stated here once.  While a stage is set on a
 * state, ptts_mimi_decode and the graph captures append its ptts_*_frame launches behind the codec's last kernel, in the order
 *   resampler -> stretcher -> pitcher -> toner -> compressor -> normaliser -> leveler -> encoder -> packer
 * whichever of them are set.  d_in == NULL: the stage reads d_pcm (which must then be device memory; NULL = the state's own
 * buffer), and its input width must be frame_samples.  Otherwise it reads the f32 device buffer d_in [B, its input width],
 * which the caller has given the stage before it as its `out`; some stage of an earlier kind must be set on the state at
 * the time of the call, so the setters are called in chain order.  It writes `out` [B, its output width], f32 or (is_i16)
 * int16 converted as ptts_mimi_set_pcm_i16 converts, device or pinned host.  -1 for a null state or output, for a batch that
 * is not the state's, and for what the rule or the setter's own comment asks and does not get.  A NULL stage switches it off:
 * decodes and captures are then launch for launch those of a state that never had one.  What follows each setter is only what
 * is particular to it.
 * The resampler is always first and has no d_in; its two launches are those of ptts_resample_frame. */
int ptts_mimi_set_resampler(ptts_mimi_state *s, ptts_resampler *rs, void *out, int32_t is_i16);
/* ---- Speaking rate (no reference counterpart).  A stretcher holds, for B sequences, a table of WSOLA plans, each row's
 * plan and each row's streaming state; it turns one frame f32[B, in_max] of the previous output stage (the codec's PCM or the
 * resampler's output; row b's n_in samples at the front of its line) into out[B, out_max] with row b's n_out samples at the
 * front of its line (the rest of the line is not written).  Plan i is h_plans[5 i ..] = (n_in, Ha, Hs, D, L): window W = 2 Hs,
 * K = n_in / Ha hops per frame, n_out = K Hs.  Hop k = 0, 1, .. of a row's input stream x (zero before its start and after
 * the row is set to drain):
 *   p_k = k Ha - L + delta_k; delta_0 = 0, else delta_k in [-D, D] maximises the fp32 dot product
 *         sum_{i < Hs} x[p_{k-1} + Hs + i] x[k Ha - L + delta + i]  (equal maxima: the smallest |delta|, then the negative one)
 *   y[k Hs + n] += w[n] x[p_k + n], n < W, with the plan's window w (its 2 Hs floats in h_windows, the plans' windows one
 *         after the other, n_window_floats in all); y[k Hs .. (k + 1) Hs) is then final and emitted
 * Ha == Hs is the identity plan: an exact copy of the first n_in samples, no lag, no state.  A plan is refused (-1) unless
 * n_in % Ha == 0, 1/2 <= Ha / Hs <= 2, L % Ha == 0, L >= D + 3 Hs (no read past the frame's end), L + D + Ha <= 8192 (the
 * samples a row carries), L + D + Ha + n_in <= 12288 (the window staged in LDS), Hs <= 2048 and 2 D + 1 <= 1024: with these
 * every index the kernel forms is in bounds by construction (csrc/ptts_stretch.h).  Plan rule: pocket_tts_amd/stretch.py.
 * in_max and out_max are the largest n_in and n_out of the plans, K_max the largest K of those that are not the identity
 * (at least 1).  Every row starts on plan 0 with a zero state. */
int ptts_stretcher_create(ptts_engine *e, int32_t batch, const int32_t *h_plans, int32_t n_plans, const float *h_windows,
                          int64_t n_window_floats, ptts_stretcher **out);
/* after every decode / graph that uses it has finished, and after ptts_mimi_set_stretcher(state, NULL, ..) on its states */
void ptts_stretcher_destroy(ptts_stretcher *ts);
/* a new utterance joins `row`: its plan from now on; carried samples, carry, delta and the drain flag are zeroed.
 * Stream-ordered on `stream`; captured graphs pick it up (the kernel reads all of it from device memory).  -1 for a row or
 * a plan index out of range; nothing is enqueued. */
int ptts_stretcher_set_row(ptts_stretcher *ts, int32_t row, int32_t plan_index, void *stream);
/* from now on (stream-ordered) the row's incoming frames count as zeros (on != 0), until set_row or on == 0 */
int ptts_stretcher_set_row_drain(ptts_stretcher *ts, int32_t row, int32_t on, void *stream);
/* One frame, one launch: d_in f32[B, in_max] (DEVICE memory) -> out [B, out_max], f32 or (is_i16) int16 converted as
 * ptts_mimi_set_pcm_i16 converts, device or pinned host; then the rows' states advance.  d_delta (i32 [B, K_max], device, or
 * NULL) receives the delta_k of the frame's hops of every row that is not on an identity plan: the test tap. */
int ptts_stretch_frame(ptts_stretcher *ts, const float *d_in, void *out, int32_t is_i16, int32_t *d_delta, void *stream);
/* The output chain's rule (ptts_mimi_set_resampler), with one difference: with d_in [B, in_max] the resampler set on the
 * state writes f32 into d_in INSTEAD of its own output, so there must be one and in_max must be its out_max; a frame enqueued
 * with d_in and no resampler fails (-1). */
int ptts_mimi_set_stretcher(ptts_mimi_state *s, ptts_stretcher *ts, float *d_in, void *out, int32_t is_i16);
/* ---- Pitch (no reference counterpart).  A pitcher holds, for B sequences, a table of plans, each row's plan and each row's
 * streaming state; it turns one frame f32[B, width] of the previous output stage (row b's n samples at the front of its line)
 * into out[B, width] with row b's n samples at the front of its line (the rest of the line is not written), every frequency
 * moved by r = P / Q.  Plan i is h_plans[8 i ..] = (n, Ha, Hs, D, L, P, Q, T):
 *   WSOLA part  (n, Ha, Hs, D, L) is a stretcher plan with Ha = Q u, Hs = P u, under the stretcher's contract word for word
 *               (positions, score, tie-break, the plan's window of 2 Hs floats in h_windows, zero before the stream's start
 *               and after the row is set to drain); a frame's K = n / Ha hops emit n_mid = n P / Q "mid" samples
 *   FIR part    y[N] = sum_{j < T} table[(N P) % Q][j] mid[(N P) / Q - j], N < n, the taps in index order; the plan's table is
 *               its Q T floats in h_tables (the plans' tables one after the other), mid = 0 before the stream's start
 * The output lags by L samples (the WSOLA part's (L / Ha) Hs mid samples, times Q / P) plus the FIR's group delay of
 * 10 max(P, Q) / P samples, which is not compensated.  Ha == Hs is the identity plan (P = Q = T = 1): an exact copy of the
 * first n samples, no lag, no state.  A plan is refused (-1) unless the stretcher admits (n, Ha, Hs, D, L), P and Q are
 * coprime and at most 20, Ha / Q == Hs / P, T == ceil((20 max(P, Q) + 1) / Q) <= 41 and n_mid <= 16384: with these every
 * index the kernel forms is in bounds by construction (csrc/ptts_pitch.h, csrc/ptts_stretch.h).  Plan rule:
 * pocket_tts_amd/pitch.py.  width is the largest n of the plans, mid_max the largest n_mid and K_max the largest K of those
 * that are not the identity (at least 1).  The mid samples of a frame live in a row-private device buffer the pitcher owns.
 * Every row starts on plan 0 with a zero state. */
int ptts_pitcher_create(ptts_engine *e, int32_t batch, const int32_t *h_plans, int32_t n_plans, const float *h_windows,
                        int64_t n_window_floats, const float *h_tables, int64_t n_table_floats, ptts_pitcher **out);
/* after every decode / graph that uses it has finished, and after ptts_mimi_set_pitcher(state, NULL, ..) on its states */
void ptts_pitcher_destroy(ptts_pitcher *ps);
/* a new utterance joins `row`: its plan from now on; carried samples, carry, delta, mid history and the drain flag are zeroed.
 * Stream-ordered on `stream`; captured graphs pick it up (the kernel reads all of it from device memory).  -1 for a row or
 * a plan index out of range; nothing is enqueued. */
int ptts_pitcher_set_row(ptts_pitcher *ps, int32_t row, int32_t plan_index, void *stream);
/* from now on (stream-ordered) the row's incoming frames count as zeros (on != 0), until set_row or on == 0 */
int ptts_pitcher_set_row_drain(ptts_pitcher *ps, int32_t row, int32_t on, void *stream);
/* One frame, one launch: d_in f32[B, width] (DEVICE memory) -> out [B, width], f32 or (is_i16) int16 converted as
 * ptts_mimi_set_pcm_i16 converts, device or pinned host; then the rows' states advance.  The test taps, device or NULL:
 * d_delta (i32 [B, K_max]) receives the delta_k of the frame's hops and d_mid (f32 [B, mid_max]) the frame's n_mid mid samples
 * of every row that is not on an identity plan; nothing else of them is written. */
int ptts_pitch_frame(ptts_pitcher *ps, const float *d_in, void *out, int32_t is_i16, int32_t *d_delta, float *d_mid,
                     void *stream);
/* The output chain's rule (ptts_mimi_set_resampler), nothing of its own. */
int ptts_mimi_set_pitcher(ptts_mimi_state *s, ptts_pitcher *ps, float *d_in, void *out, int32_t is_i16);
/* ---- Output level (no reference counterpart).  A leveler holds, for B sequences, a table of plans, each row's plan, gain G,
 * ceiling C and streaming state; it turns one frame f32[B, width] of the previous output stage (row b's n samples at the front
 * of its line) into out[B, width] with row b's n samples at the front of its line (the rest of the line is not written).
 * Plan i is h_plans[4 i ..] = (n, LA, the bits of the float a, the bits of the float k): n samples per frame, look-ahead LA,
 * release factor a per sample, k = 1 / LA.  With x the row's input stream (zero before its start and after the row is set
 * to drain) and u = G x:
 *   r[i] = |u[i]| > C ? C / |u[i]| : 1      m[i] = min r[i - LA .. i]         d[i] = max(1 - m[i], a d[i - 1]), d[-1] = 0
 *   e[i] = 1 - d[i]                          g[i] = k sum e[i - LA + 1 .. i]   y[i] = g[i] u[i - LA]
 * (r = e = 1 before the stream's start): |y| <= C up to fp32 rounding, the output lags by LA samples.  A plan is refused
 * (-1) unless 1 <= LA <= 512, LA <= n <= 8192, 0 <= a < 1 and 0 < k <= 1: with these every index the kernel forms is in
 * bounds by construction (csrc/ptts_level.h).  Plan rule: pocket_tts_amd/level.py.  width is the largest n of the plans.
 * Every row starts on bypass: an exact copy of its whole line, no lag, no state. */
int ptts_leveler_create(ptts_engine *e, int32_t batch, const int32_t *h_plans, int32_t n_plans, ptts_leveler **out);
/* after every decode / graph that uses it has finished, and after ptts_mimi_set_leveler(state, NULL, ..) on its states */
void ptts_leveler_destroy(ptts_leveler *lv);
/* a new utterance joins `row`: its plan (-1: bypass), gain G in (0, 16] and ceiling C in (0, 1] from now on; carried samples,
 * d and the drain flag are zeroed.  Stream-ordered on `stream`; captured graphs pick it up (the kernel reads all of it from
 * device memory).  -1 for a row, a plan index, a gain or a ceiling out of range; nothing is enqueued. */
int ptts_leveler_set_row(ptts_leveler *lv, int32_t row, int32_t plan_index, float gain, float ceiling, void *stream);
/* from now on (stream-ordered) the row's incoming frames count as zeros (on != 0), until set_row or on == 0 */
int ptts_leveler_set_row_drain(ptts_leveler *lv, int32_t row, int32_t on, void *stream);
/* True-peak mode (pocket_tts_amd/level.py, "True-peak mode").  taps63 is float[3][21], phases 1, 2, 3 of the 4x interpolator
 * h_p[j] (level.TP_TAPS).  A row in this mode limits on P[i] = max(|u[i - 10]|, |v_1[i]|, |v_2[i]|, |v_3[i]|), v_p[i] =
 * sum over j < 21 of h_p[j] u[i - j], in place of |u[i]|: r[i] = P[i] > C ? C / P[i] : 1, m, d, e, g as above and y[i] =
 * g[i] u[i - 10 - LA]; the output lags by LA + 10 samples, and the row keeps a meter M = max(M, |y[i - 10]|, |w_p[i]|), w_p
 * the same FIR over y.  enable allocates the mode's carries and meters, once per leveler and before its first frame or
 * graph capture: from then on level_frame launches the kernel that knows the mode, in which a row that does not use it
 * computes bit for bit what it computed before.  -1 for a null argument, a second call or a tap outside [-4, 4]. */
int ptts_leveler_enable_true_peak(ptts_leveler *lv, const float *taps63);
/* ptts_leveler_set_row for a row in true-peak mode, its meter at 0 (ptts_leveler_set_row puts a row in sample-peak mode).
 * -1 additionally for a leveler without the mode, for plan_index -1 and for a plan with LA + 10 > n. */
int ptts_leveler_set_row_tp(ptts_leveler *lv, int32_t row, int32_t plan_index, float gain, float ceiling, void *stream);
/* the row's meter after everything enqueued on `stream` so far, into *host_out; waits for the stream, so not inside a
 * capture.  0.0 for a row that is not in the mode.  -1 for a row out of range, a null argument, a leveler without the mode. */
int ptts_leveler_row_true_peak(ptts_leveler *lv, int32_t row, float *host_out, void *stream);
/* One frame, one launch: d_in f32[B, width] (DEVICE memory) -> out [B, width], f32 or (is_i16) int16 converted as
 * ptts_mimi_set_pcm_i16 converts, device or pinned host; then the rows' states advance. */
int ptts_level_frame(ptts_leveler *lv, const float *d_in, void *out, int32_t is_i16, void *stream);
/* The output chain's rule (ptts_mimi_set_resampler), nothing of its own. */
int ptts_mimi_set_leveler(ptts_mimi_state *s, ptts_leveler *lv, float *d_in, void *out, int32_t is_i16);
/* ---- Loudness (no reference counterpart).  A normaliser holds, for B sequences, a table of plans, each row's plan, target T
 * in LUFS and streaming state; it turns one frame f32[B, width] of the previous output stage (row b's n samples at the front of
 * its line) into d_out f32[B, width] with row b's n samples at the front of its line (the rest of the line is neither read nor
 * written).  It measures the running gated loudness of the row's own stream by ITU-R BS.1770-4 (K-weighting, 400 ms blocks
 * every 100 ms, absolute and relative gate) and applies the gain, clamped to +-20 dB and ramped linearly over each 100 ms,
 * that brings it to T; the output lags by D = 4 (rate / 10) samples (contract: pocket_tts_amd/loudness.py).  Plan i is
 * h_plans[2 i ..] = (rate, n) and h_doubles[330 i ..] = the ten K-weighting coefficients (b0 b1 b2 a1 a2 of the shelf, then of
 * the high-pass) followed by the ten matrices A^(chunk 2^t), chunk = ceil(n / 1024), of the recurrence the kernel scans, each
 * as two row-major 4 x 4 matrices: the power rounded to double, then what the exact power leaves.  A plan is refused (-1) unless 8000 <= rate <= 48000, 1 <= n <= 8192 and every double is finite: with these
 * every index the kernel forms is in bounds by construction (csrc/ptts_loud.h).  width is the largest n of the plans.  Every
 * row starts on bypass: an exact copy of its whole line, no lag, no state. */
int ptts_loudnorm_create(ptts_engine *e, int32_t batch, const int32_t *h_plans, int32_t n_plans, const double *h_doubles,
                         int64_t n_doubles, ptts_loudnorm **out);
/* after every decode / graph that uses it has finished, and after ptts_mimi_set_loudnorm(state, NULL, ..) on its states */
void ptts_loudnorm_destroy(ptts_loudnorm *ln);
/* a new utterance joins `row`: its plan (-1: bypass) and target in [-40, -10] LUFS from now on; the filter state, the
 * measurement, the delayed samples and the drain flag are zeroed.  Stream-ordered on `stream`; captured graphs pick it up.
 * -1 for a row, a plan index or a target out of range; nothing is enqueued. */
int ptts_loudnorm_set_row(ptts_loudnorm *ln, int32_t row, int32_t plan_index, double target_lufs, void *stream);
/* from now on (stream-ordered) the row's incoming frames count as zeros (on != 0), until set_row or on == 0 */
int ptts_loudnorm_set_row_drain(ptts_loudnorm *ln, int32_t row, int32_t on, void *stream);
/* One frame, one launch: d_in f32[B, width] -> d_out f32[B, width], both DEVICE memory and distinct; then the rows' states
 * advance.  The test tap d_tap, device or NULL: f64[B, 4] receives, for every row that is not on bypass, the sub-blocks it
 * has completed, its last L (NaN while undefined), its last c and its last Z. */
int ptts_loudnorm_frame(ptts_loudnorm *ln, const float *d_in, float *d_out, double *d_tap, void *stream);
/* The output chain's rule (ptts_mimi_set_resampler).  Its own: d_out is f32 device memory and not d_in (-1), and the caller
 * gives it to the leveler as its d_in: a frame enqueued with a normaliser but no leveler fails (-1). */
int ptts_mimi_set_loudnorm(ptts_mimi_state *s, ptts_loudnorm *ln, float *d_in, float *d_out);
/* ---- Tone (no reference counterpart).  A toner holds, for B sequences, a table of plans, each row's plan and streaming
 * state; it turns one frame f32[B, width] of the previous output stage (row b's n samples at the front of its line) into d_out
 * f32[B, width] with row b's n samples at the front of its line (the rest of the line is neither read nor written).  A plan
 * is a cascade of K <= 8 biquad sections for frames of n samples: section k runs in transposed direct form II in float64 on
 * the output of section k - 1 from a zero state, and y is rounded to f32 once, after the last one; no lag, no pre-roll, no
 * drain flag (contract, grammar and presets: pocket_tts_amd/tone.py).  Plan i is h_plans[3 i ..] = (rate, n, K) and
 * h_doubles[360 i ..] = 8 x (b0 b1 b2 a1 a2), a0 = 1, followed by 8 x 10 row-major 2 x 2 matrices A_k^(chunk 2^j), j = 0 .. 9,
 * chunk = ceil(n / 1024), A_k = [[-a1, 1], [-a2, 0]]: the powers of section k's state transition that the kernel's scan
 * uses; the sections behind the K-th are zero.  A plan is refused (-1) unless 8000 <= rate <= 48000, 1 <= n <= 8192,
 * 1 <= K <= 8 and every double is finite: with these every index the kernel forms is in bounds by construction
 * (csrc/ptts_tone.h).  The plans are copied to the device once; a row is dealt one by its index, so a captured graph follows
 * ptts_tone_set_row without recapture.  width is `line`, which no plan's n may exceed (-1), or with line == 0 the largest n
 * of the plans (a tone need not be admissible on the widest line of the chain it sits in).  Every row starts on bypass: an exact copy of
 * its whole line, no state.  A row's output depends on its own stream alone, bit for bit: not on its slot, not on the batch. */
int ptts_tone_create(ptts_engine *e, int32_t batch, int32_t line, const int32_t *h_plans, int32_t n_plans,
                     const double *h_doubles, int64_t n_doubles, ptts_tone **out);
/* after every decode / graph that uses it has finished, and after ptts_mimi_set_tone(state, NULL, ..) on its states */
void ptts_tone_destroy(ptts_tone *tn);
/* a new utterance joins `row`: its plan (-1: bypass) from now on; the sections' states are zeroed.  Stream-ordered on
 * `stream`; captured graphs pick it up.  -1 for a row or a plan index out of range; nothing is enqueued. */
int ptts_tone_set_row(ptts_tone *tn, int32_t row, int32_t plan_index, void *stream);
/* One frame, one launch: d_in f32[B, width] -> d_out f32[B, width], both DEVICE memory and distinct (-1 otherwise); then
 * the rows' states advance. */
int ptts_tone_frame(ptts_tone *tn, const float *d_in, float *d_out, void *stream);
/* The output chain's rule (ptts_mimi_set_resampler).  Its own: d_out is f32 device memory and not d_in (-1), and the caller
 * gives it to the normaliser or the leveler as its d_in: a frame enqueued with a toner but no leveler fails (-1). */
int ptts_mimi_set_tone(ptts_mimi_state *s, ptts_tone *tn, float *d_in, float *d_out);
/* ---- Dynamics (no reference counterpart).  A compressor holds, for B sequences, a table of plans, each row's plan and
 * streaming state; it turns one frame f32[B, width] of the previous output stage (row b's n samples at the front of its
 * line) into d_out f32[B, width] with row b's n samples at the front of its line (the rest of the line is neither read nor
 * written).  A plan is a log-domain feed-forward compressor with a soft knee and a decoupled smooth peak detector, in float64,
 * y rounded to f32 once; no look-ahead, no lag, no pre-roll, no drain flag (contract, grammar and presets:
 * pocket_tts_amd/dynamics.py).  Plan i is h_plans[2 i ..] = (rate, n) and h_doubles[26 i ..] = T, k = 1 - 1 / ratio, W, M, aA,
 * aR, followed by the ten powers aA^(chunk 2^j) and the ten powers aR^(chunk 2^j), j = 0 .. 9, chunk = ceil(n / 1024), that
 * the kernel's two scans use.  A plan is refused (-1) unless 8000 <= rate <= 48000, 1 <= n <= 8192, every double is finite,
 * T, W and M lie in the ranges of the grammar, 0 <= k < 1, 0 < aA, aR < 1 and every power is in [0, 1): with these every
 * index the kernel forms is in bounds by construction (csrc/ptts_dyn.h).  The plans are copied to the device once; a row is
 * dealt one by its index, so a captured graph follows ptts_dynamics_set_row without recapture.  width is `line`, which no
 * plan's n may exceed (-1), or with line == 0 the largest n of the plans.  Every row starts on bypass: an exact copy of its
 * whole line, no state.  A row's output depends on its own stream alone, bit for bit: not on its slot, not on the batch. */
int ptts_dynamics_create(ptts_engine *e, int32_t batch, int32_t line, const int32_t *h_plans, int32_t n_plans,
                         const double *h_doubles, int64_t n_doubles, ptts_dynamics **out);
/* after every decode / graph that uses it has finished, and after ptts_mimi_set_dynamics(state, NULL, ..) on its states */
void ptts_dynamics_destroy(ptts_dynamics *dy);
/* a new utterance joins `row`: its plan (-1: bypass) from now on; p and s are zeroed.  Stream-ordered on `stream`; captured
 * graphs pick it up.  -1 for a row or a plan index out of range; nothing is enqueued. */
int ptts_dynamics_set_row(ptts_dynamics *dy, int32_t row, int32_t plan_index, void *stream);
/* One frame, one launch: d_in f32[B, width] -> d_out f32[B, width], both DEVICE memory and distinct (-1 otherwise); then
 * the rows' states advance. */
int ptts_dynamics_frame(ptts_dynamics *dy, const float *d_in, float *d_out, void *stream);
/* The output chain's rule (ptts_mimi_set_resampler).  Its own: d_out is f32 device memory and not d_in (-1), and the caller
 * gives it to the normaliser or the leveler as its d_in: a frame enqueued with a compressor but no leveler fails (-1). */
int ptts_mimi_set_dynamics(ptts_mimi_state *s, ptts_dynamics *dy, float *d_in, float *d_out);
/* ---- Output encoding (no reference counterpart).  An encoder holds, for B sequences, each row's number of samples n and
 * encoding code: 0 pcm_s16le, 1 pcm_f32le, 2 mulaw, 3 alaw (contract: pocket_tts_amd/encoding.py).  It turns one frame
 * f32[B, width] of the previous output stage (row b's n samples at the front of its line) into out_bytes u8[B, pitch],
 * pitch = 4 width rounded up to 16: row b gets exactly n * bytes_per_sample(code) bytes (2, 4, 1, 1) at the start of its row
 * and NOTHING behind them.  pcm_f32le: the sample's four bytes, bit for bit.  pcm_s16le: s = (int16)(clamp(x, -1, 1) * 32767.0f),
 * truncated, as ptts_mimi_set_pcm_i16 converts (a NaN gives -32767).  mulaw / alaw: ITU-T G.711 of that s, mu-law from the
 * 14-bit value s >> 2 with all bits inverted, A-law from the 13-bit value s >> 3 with the even bits inverted (0x55).  The
 * stage has no state, no lag and no drain flag.  Every row starts as (width, pcm_s16le). */
int ptts_encoder_create(ptts_engine *e, int32_t batch, int32_t width, ptts_encoder **out);
/* after every decode / graph that uses it has finished, and after ptts_mimi_set_encoder(state, NULL, ..) on its states */
void ptts_encoder_destroy(ptts_encoder *en);
/* `row` holds n samples (1 <= n <= width) in the encoding `code` (0 .. 3) from now on.  Stream-ordered on `stream`; captured
 * graphs pick it up (the kernel reads both from device memory).  -1 for a row, an n or a code out of range; nothing is
 * enqueued. */
int ptts_encoder_set_row(ptts_encoder *en, int32_t row, int32_t n, int32_t code, void *stream);
/* One frame, one launch: d_in f32[B, width] (DEVICE memory) -> out_bytes u8[B, pitch], device or pinned host, aligned to 16
 * bytes (-1 otherwise). */
int ptts_encode_frame(ptts_encoder *en, const float *d_in, void *out_bytes, void *stream);
/* The output chain's rule (ptts_mimi_set_resampler), writing out_bytes, with one difference: the last stage set on the state
 * (leveler, else pitcher, else stretcher, else resampler; its widest line must be width) writes f32 into d_in INSTEAD of its
 * own `out`.  So d_in must be NULL exactly when the state has none of these four, at the time of the call (-1) and when a
 * frame is enqueued (-1). */
int ptts_mimi_set_encoder(ptts_mimi_state *s, ptts_encoder *en, float *d_in, void *out_bytes);
/* ---- Output compression (no reference counterpart): the packer, the eighth stage, behind the encoder.  A packer holds, for B
 * sequences, each row's mode (0 pass-through, 1 flac), its data and the previous line of a flac row.  It reads the encoder's
 * bytes, u8[B, 4 width rounded up to 16] in DEVICE memory, and writes ring lines u8[B, pitch], pitch = 16 + (max(4 width, 2 width
 * + 18) rounded up to 16): the prefix {u32 nbytes, 0, 0, 0}, then nbytes bytes, and nothing behind 16 + nbytes rounded up to 16.
 * A pass-through row's bytes are the encoder's n * bps.  A flac row's are one FLAC frame of n samples of the row's pcm_s16le
 * line sequence (bitstream and choice rule: pocket_tts_amd/flac.py, csrc/ptts_flac.h), or none (nbytes 0) for the first
 * ceil(preroll / n) lines after set_row: line f emits the n samples that begin preroll + (f - lead) n samples into the row's
 * sequence, as frame first_block + f - lead, cut from the previous line and the current one.  Every row starts as
 * pass-through (width, 2 bytes a sample). */
int ptts_flac_create(ptts_engine *e, int32_t batch, int32_t width, ptts_flac **out);
/* after every decode / graph that uses it has finished, and after ptts_mimi_set_packer(state, NULL, ..) on its states */
void ptts_flac_destroy(ptts_flac *pk);
/* `row` is from now on pass-through (mode 0: n in [1, width] samples of bps = 1, 2 or 4 bytes; the other arguments are not
 * read) or flac (mode 1: n in [16, min(width, 4608)], rate in [1, 65535] Hz, preroll >= 0 samples, first_block in [0, 2^30),
 * bps is not read), with its line counter at 0.  Stream-ordered on `stream`; captured graphs pick it up (the kernel reads
 * all of it from device memory).  -1 for a value out of range; nothing is enqueued. */
int ptts_flac_set_row(ptts_flac *pk, int32_t row, int32_t mode, int32_t n, int32_t bps, int32_t rate, int32_t preroll,
                      int32_t first_block, void *stream);
/* One frame, one launch: d_in_bytes (DEVICE memory) -> out_bytes, device or pinned host, both aligned to 16 bytes (-1
 * otherwise); the flac rows' line counters advance. */
int ptts_flac_frame(ptts_flac *pk, const void *d_in_bytes, void *out_bytes, void *stream);
/* The output chain's rule (ptts_mimi_set_resampler), with these differences: the packer needs an encoder of its width on the
 * state, at the time of the call (-1) and when a frame is enqueued (-1); d_in_bytes is the device buffer the caller has given
 * that encoder as its out_bytes, which is checked when a frame is enqueued (-1). */
int ptts_mimi_set_packer(ptts_mimi_state *s, ptts_flac *pk, void *d_in_bytes, void *out_bytes);
/* d_latent f32[B, ldim] (normalised FlowLM output) -> d_pcm f32[B, frame_samples]; includes the
 * emb_std/emb_mean de-normalisation, the quantizer 1x1 conv and increment_steps(mimi, 16). */
int ptts_mimi_decode(ptts_engine *e, ptts_mimi_state *s, const float *d_latent, float *d_pcm, void *stream);
/* The same frame in its two parts, for callers that schedule them apart.  ptts_mimi_decode_tr: the de-normalisation, the
 * quantizer conv, the upsample and the decoder transformer of ONE frame (d_latent_b NULL) or of a PAIR of consecutive
 * frames (d_latent, then d_latent_b; fp32 codec only, -1 otherwise): a pair runs the transformer once on twice the rows.
 * ptts_mimi_decode_seanet: SEANet, the PCM and the state's output stages of the oldest frame the transformer has handed
 * over and SEANet has not decoded.  The hand-over holds a pair beside the frame before it: -1 when the transformer would
 * run further ahead than that, or when SEANet has no frame to decode; nothing is enqueued then.  Parts and whole frames
 * mix freely on one state; results are those of ptts_mimi_decode called once per frame. */
int ptts_mimi_decode_tr(ptts_engine *e, ptts_mimi_state *s, const float *d_latent, const float *d_latent_b, void *stream);
int ptts_mimi_decode_seanet(ptts_engine *e, ptts_mimi_state *s, float *d_pcm, void *stream);

/* ---- Voice-prompt encode path (one-off per voice): MimiModel.encode_to_latent + F.linear(speaker_proj_weight)
 *      (mimi.py:96-119, tts_model.py:379-388).  d_audio f32[n_samples] mono at the model rate; the signal is
 *      zero-padded to a whole number of frames.  Outputs (either may be NULL): d_latent_out f32[frames, ldim],
 *      d_cond_out f32[frames, d_model] (feed it to ptts_lm_prefill after bos_before_voice).  Synchronises. */
int ptts_encode_voice(ptts_engine *e, const float *d_audio, int64_t n_samples, float *d_latent_out,
                      float *d_cond_out, int32_t *h_frames, void *stream);

/* ---- hipGraph capture of one step (north star: "each decode step hipGraph-captured").
 * The captured step uses the same argument pointers on every launch. */
int ptts_graph_capture_lm_step(ptts_engine *e, ptts_lm_state *s, const float *d_noise, int32_t lsd_steps,
                               float eos_threshold, float *d_latent_out, float *d_eos_logit,
                               uint8_t *d_is_eos, ptts_graph **out);
int ptts_graph_capture_mimi(ptts_engine *e, ptts_mimi_state *s, const float *d_latent, float *d_pcm,
                            ptts_graph **out);
/* The parts of the codec frame as graphs of their own (ptts_mimi_decode_tr / ptts_mimi_decode_seanet; the same refusals, at
 * ptts_graph_launch): the transformer of one frame, of a frame pair, and SEANet of one frame with the output stages the
 * state has when it is captured. */
int ptts_graph_capture_mimi_tr(ptts_engine *e, ptts_mimi_state *s, const float *d_latent, ptts_graph **out);
int ptts_graph_capture_mimi_tr_pair(ptts_engine *e, ptts_mimi_state *s, const float *d_latent_a, const float *d_latent_b,
                                    ptts_graph **out);
int ptts_graph_capture_mimi_seanet(ptts_engine *e, ptts_mimi_state *s, float *d_pcm, ptts_graph **out);
/* One graph with two parallel branches: the FlowLM step (as ptts_graph_capture_lm_step) and the Mimi decode of
 * the PREVIOUS frame (reads d_mimi_latent_in, which must differ from d_latent_out).  Replaying such graphs
 * back to back on one stream overlaps step t+1 with frame t without cross-stream events (the reference
 * pipelines the same two stages with two threads: tts_model.py:651-658). */
int ptts_graph_capture_pipelined(ptts_engine *e, ptts_lm_state *s, ptts_mimi_state *m, const float *d_noise,
                                 int32_t lsd_steps, float eos_threshold, float *d_latent_out, float *d_eos_logit,
                                 uint8_t *d_is_eos, const float *d_mimi_latent_in, float *d_pcm, ptts_graph **out);
int ptts_graph_launch(ptts_graph *g, void *stream);
void ptts_graph_destroy(ptts_graph *g);

/* ---- tile autotuning (no reference counterpart: torch picks its CPU kernels at dispatch time).
 * Runs one FlowLM step + one codec frame of `batch` rows on scratch states and, for every GEMM shape on the
 * path, times each valid tile configuration (cache flushed before every timed launch) and remembers the
 * fastest for this engine.  Call it before capturing graphs for that batch; shapes never tuned use the static
 * heuristic.  Results are numerically equivalent up to fp32 summation order.  Synchronises.
 * ptts_tune_log: one text line per tuned shape (valid until the next tune/clear). */
int ptts_tune(ptts_engine *e, int32_t batch, void *stream);
/* the same with the FlowLM step tuned on `lm_stream` and the codec frame on `codec_stream`: with CU-masked streams
 * (ptts_stream_create_masked) each stage gets the tiles that are fastest on its own share of the chip */
int ptts_tune_streams(ptts_engine *e, int32_t batch, void *lm_stream, void *codec_stream);
/* the same for the prefill GEMM shapes of `batch` sequences x `t` positions (text prefill of a chunk: first-chunk path) */
int ptts_tune_prefill(ptts_engine *e, int32_t batch, int32_t t, void *stream);
const char *ptts_tune_log(ptts_engine *e);
void ptts_tune_clear(ptts_engine *e);
/* The tuned table as text (one line per GEMM shape) so that a deployment tunes once: export after ptts_tune,
 * import (returns the number of entries accepted) before capturing graphs in a later process. */
int64_t ptts_tune_export(ptts_engine *e, char *h_out, int64_t capacity);
/* version of the table format + configuration list: a cache file written by another version must not be imported */
int ptts_tune_version(void);
int ptts_tune_import(ptts_engine *e, const char *text);

/* ---- utilities */
/* Engine options (experiments / A-B tests; defaults come from the environment variable in brackets):
 *   "flow_cluster"  [PTTS_FLOW_CLUSTER, 1]  1 = the flow MLP of a decode step runs as ONE cooperative launch
 *                                           (ptts_flow.h), 0 = one GEMM launch per layer
 *   "lm_cluster"    [PTTS_LM_CLUSTER, 0]    1 = all transformer layers of a decode step run as ONE cooperative launch
 *                                           (ptts_lm.h; fp32 weights only; correct, but measured SLOWER than the default:
 *                                           DESIGN.md section 3), 0 = five launches per layer
 *   "k_rotate"      [PTTS_K_ROTATE, 0]      1 = K-split GEMM workgroups start their K loop at a column-block dependent
 *                                           chunk (spreads the re-reads of the shared activation rows over L2 channels)
 *   "fuse_res"      [PTTS_FUSE_RES, 1]      1 = a SEANet residual block (k3 conv, ELU, 1x1 conv, skip) of decoder stages 2 and 3
 *                                           is ONE launch, the hidden activation staying in LDS; 0 = two launches
 *   "codec_lds_target" [PTTS_CODEC_LDS_TARGET, 57344]  the codec's GEMM launches pad their LDS request to this many bytes
 *                                           per workgroup (0 = off): fewer codec workgroups per CU, so the FlowLM stream's
 *                                           short dependent kernels find free wave slots and registers (+5 % pipelined throughput at batch 64)
 *   "flow_max_cus"  [PTTS_FLOW_MAX_CUS, 128] resident workgroups of the cooperative flow launch (8..CUs of the device): at most the number
 *                                           of CUs its stream may use (a CU-masked FlowLM stream needs it lowered; fewer is
 *                                           slower in the shared pipeline too: 128 -> 0.852, 64 -> 0.904, 32 -> 1.010 ms per step)
 *   "single_store"  [PTTS_SINGLE_STORE, 1]  1 = a SEANet transposed conv stores its RAW output once (it is the residual block's skip
 *                                           input) and the k3 conv that follows applies ELU to its operand fragments as it reads
 *                                           them; 0 = the producer stores raw + ELU'd copies (rounds 1-2).  fp32 codec only;
 *                                           -107 MB of HBM traffic per 64-sequence frame, +1.4 % pipelined throughput
 *   "fuse_pcm"      [PTTS_FUSE_PCM, 1]      1 = SEANet's last conv (n_filters -> 1 sample) runs in the epilogue of the last stage's fused
 *                                           residual block (per 64-row tile: partial sums + a carry for the next tile's first two
 *                                           samples; a small kernel adds carries and bias and writes the PCM); 0 = a separate
 *                                           conv over the stored block output.  fp32 codec, en100m-shaped last stage only
 *   "debug_taps"    [-, 0]                  1 = buffers that fused kernels keep on chip are also stored, so that ptts_debug_read can
 *                                           return every stage (parity tests); reading such a buffer without it fails (-1)
 *   "share_prefix"  [PTTS_SHARE_PREFIX, 1]  1 = ptts_lm_state_copy / _copy_row(_from) from a ONE-sequence state (a voice state) do
 *                                           not copy its first T & ~15 keys / values: the clone's rows BORROW them (the
 *                                           attention kernels read those key tiles from the owner's cache), so the
 *                                           utterances of one voice fetch them through L2 once instead of once per row, and a
 *                                           clone copies < 16 positions.  Bitwise the same results as full copies.  While
 *                                           lent, the owner refuses ptts_lm_state_reset / _import / being a copy
 *                                           destination (-1); it may be prefilled further (appends only) and destroyed (its
 *                                           memory is released when the last borrower is destroyed, re-cloned or reset).
 *                                           Export materialises the borrowed positions.
 *   "prefix_cascade" [PTTS_CASCADE, 1]      decode steps of >= 16 sequences: 1 = the scores against a prefix shared by 4
 *                                           neighbouring rows are MFMA tiles computed once for the 4 (attn_cascade_kernel),
 *                                           their private keys per row, merged in LDS; 0 = every row on its own.  Equal to
 *                                           fp32 summation order, not bitwise; a row's bits then depend on whether its 4-row
 *                                           group shares a prefix (a row next to other voices takes the per-row path)
 * Applies to steps enqueued / graphs captured after the call.  Returns -1 for an unknown key. */
int ptts_set_option(ptts_engine *e, const char *key, int32_t value);
/* 1 after a cooperative kernel of this state gave up waiting for a peer workgroup since the last call (the outputs of
 * the steps in between are then invalid); READS AND CLEARS the word, synchronises the stream.  Never 1 unless the GPU was
 * oversubscribed beyond the contract above. */
int ptts_lm_state_error(ptts_lm_state *s, void *stream);
/* Test hook: sets (value != 0) or clears the word ptts_lm_state_error reports. */
int ptts_debug_set_error(ptts_lm_state *s, int32_t value, void *stream);
/* A HIP stream restricted to CUs [cu_lo, cu_hi) of every XCD (hipExtStreamCreateWithCUMask; 32 CUs per XCD on
 * MI355X): work queued on it - eager launches and graph launches alike - leaves the other CUs to the other streams.
 * Destroy with ptts_stream_destroy after the work queued on it has finished. */
int ptts_stream_create_masked(ptts_engine *e, int32_t cu_lo, int32_t cu_hi, void **out_stream);
int ptts_stream_destroy(void *stream);
/* 1 if work queued on the two streams runs concurrently, 0 if the runtime put them on the same hardware queue (HIP
 * multiplexes streams onto GPU_MAX_HW_QUEUES queues, default 4, round-robin at creation; such a pair executes strictly
 * in turn).  Callers that pipeline the FlowLM step and the codec frame on two streams check the pair once and pick
 * another stream on 0.  Synchronises both streams; costs ~0.5 ms. */
int ptts_streams_overlap(ptts_engine *e, void *stream_a, void *stream_b);
int ptts_sync(ptts_engine *e, void *stream);
void *ptts_engine_stream(ptts_engine *e);
/* asynchronous device -> pinned-host copy on `stream` (PCM chunks, EOS flags) */
int ptts_copy_to_host_async(ptts_engine *e, void *h_dst, const void *d_src, int64_t bytes, void *stream);
/* HIP-event timing on `stream` (bench.py measures on the stream the kernels run on) */
int ptts_timer_start(ptts_engine *e, void *stream);
int ptts_timer_stop_ms(ptts_engine *e, void *stream, float *h_ms);
/* The test hooks from here on (ptts_debug_read / _gemm / _codec_gemm / _attn) are built from csrc/ptts_debug.hip, a unit of
 * their own beside the production host side (csrc/ptts.hip). */
/* Test hook: copies an internal activation buffer, converted to row-major f32[rows, cols], to
 * d_out (capacity in floats).  Names: see DESIGN.md; FlowLM name "noise" = the last step's LSD start point (the noise)
 * f32[B, ldim] (only kept when that step ran the single-launch flow MLP, "flow_cluster"; -1 otherwise); FlowLM name "mod" =
 * the AdaLN modulations of the last step's first LSD iteration, f32[B, (3 flow_depth + 2) flow_dim] (-1 after a step that
 * ran with the flow fold, ptts_lm_state_set_flow_fold: it computes them on chip and the buffer would be stale).
 * Mimi names (every codec format; B sequences, rows b * T + t).  A tap is decoded from the layout and element type its
 * buffer has in the engine's codec format: fp32 fragments, bf16 blocks, or e4m3 bytes, which come back as the decoded
 * CODES, unscaled (the reader multiplies by the scale "f8_scales" holds for the tap).  A name whose buffer the format or
 * the options do not keep is refused with a message (-1), never reinterpreted:
 *   "upsample"            [16 B, m_dim]        the transformer's input (fp32 | bf16)
 *   "tr_in<l>"            [16 B, m_dim]        the input of layer l; l = 0 is "upsample", l >= 1 is a copy made only while
 *                                              the engine option "debug_taps" is set (the next layer overwrites the stream)
 *   "tr_q"                [16 B, 64 heads]     the LAST layer's queries after RoPE (fp32 in every format)
 *   "tr_k<l>", "tr_v<l>"  [ring B, 64 heads]   EVERY slot of layer l's key / value ring, row b * ring + slot (fp32)
 *   "tr_attn", "tr_resid", "tr_ff"             the LAST layer's attention output, stream after attention, GELU(linear1)
 *   "tr_q<l>", "tr_attn<l>", "tr_resid<l>", "tr_ff<l>"  the same of layer l: an earlier layer's are copies made only while
 *                                              "debug_taps" is set, like "tr_in<l>"
 *   "dec_tr", "dec_tr_slot<k>" [16 B, m_dim]   the transformer's output of the last frame; slot k of the hand-over ring
 *                                              (fp32: 4 slots, reduced precision: the 2 parity halves)
 *   "seanet0"             [16 B, 8 nf]         ELU(conv0) (fp32 | bf16 | e4m3, scale index 0)
 *   "seanet2/5/8"         [rows_i B, cout_i]   stage i's transposed conv, RAW: the block's skip input (fp32 | bf16)
 *   "seanet_c<i>"         [rows_i B, cout_i]   the same as the k3 conv reads it: ELU'd (fp32 | bf16 | e4m3, index 3 i - 2);
 *                                              the fp32 codec's "single_store" keeps the raw value there
 *   "seanet_h<i>"         [rows_i B, cout_i / compress]  the block's hidden activation (fp32 | bf16 | e4m3, index 3 i - 1);
 *                                              refused where the fp32 codec's fused block keeps it on chip
 *   "seanet3/6/9"         [rows_i B, cout_i]   the block's output, ELU'd (fp32 | bf16 | e4m3 for i < 3, index 3 i; the last
 *                                              block's is bf16 on the fp8 codec too: the last conv reads bf16)
 *   "seanet11"            [B, frame samples]   the PCM (fp32)
 *   "w_<site>"            [N, taps C]          the weight image a reduced-precision launch multiplies by (refused on the fp32
 *                                              codec), site = qkv<l> | out<l> | ff1<l> | ff2<l> | conv0 | convtr<i> | res_a<i> |
 *                                              res_b<i>; k = tap C + c in the packer's tap order (a transposed conv: tap 0 the
 *                                              previous input row); bf16 values, or at the fp8 convolutions of an fp8 engine the
 *                                              e4m3 codes, whose per-row scales are "ws_<site>" [1, N]
 *   "wh_<site>", "wl_<site>" [N, taps C]       the hi = bf16(w) and lo = bf16(w - hi) images a PTTS_CODEC_SPLIT engine's
 *                                              launches multiply by, same sites and tap order (refused on every other engine)
 *   "lns_<site>", "lnc_<site>" [1, N]          the LayerNorm fold vectors ln_s, ln_c of site = qkv<l> | ff1<l> of the fp32 and
 *                                              split-bf16 codecs (fp32; refused on the reduced-precision codecs)
 *   "f8_scales"           [1, 16]            the activation scales of an fp8 codec engine (refused on any other)
 *   "calib_latent<f>"     [8, ldim]            f = 0..5, on a state of batch 8: the latents the fp8 calibration run decoded
 *                                              in frame f, generated again by the same kernel
 * Returns rows*cols or <0. */
int64_t ptts_debug_read(ptts_engine *e, void *state, int32_t is_mimi, const char *name, float *d_out,
                        int64_t capacity, int32_t *rows, int32_t *cols, void *stream);
/* Test hook: the intermediates of the voice-prompt encoder.  A ptts_encode_voice that runs with the engine option
 * "debug_taps" set keeps them in the engine until the next ptts_encode_voice or ptts_destroy (without the option it
 * allocates, copies and launches nothing for them, and this function returns -1).  Same conversion and return value as
 * ptts_debug_read.  With R = the padded sample count (a multiple of the frame size), r = 4, 5, 6 the strides of rounds
 * i = 1, 2, 3 and dim = n_filters * 2^(i-1), each name holds what the NEXT kernel reads:
 *   "audio"       [R, 16]            column 0 = the samples, zero from n_samples on; columns 1..15 zero
 *   "conv0_raw"   [R, n_filters]     k7 conv, RAW (the first block's skip input)
 *   "conv0"       [R, n_filters]     the same, ELU'd
 *   "rb<i>"       [rows, dim / compress]  the block's hidden activation: k3 conv of the ELU'd input, ELU'd
 *   "se<i>"       [rows, dim]        the block's output raw skip + 1x1 conv, ELU'd (nothing reads the raw sum)
 *   "down<i>_raw" [rows / r, 2 dim]  the strided conv, RAW (the next block's skip input)
 *   "down<i>"     [rows / r, 2 dim]  the same, ELU'd
 *   "final"       [R / 120, m_dim]   the k3 conv, raw: the transformer's input (a copy; the transformer works in place)
 *   "tr_qkv"      [R / 120, 3 m_dim] the LAST layer's queries and keys after RoPE and its values, [q | k | v] per position,
 *                                    read from the query blocks and the key / value cache the attention kernel reads
 *   "tr_attn", "tr_resid", "tr_ff"   the LAST layer's attention output before out_proj, stream after attention (a copy)
 *                                    and GELU(linear1)
 *   "enc_tr"      [R / 120, m_dim]   the transformer's output
 *   "latent"      [frames, ldim]     the replicate-padded downsample
 *   "cond"        [frames, d_model]  the speaker projection */
int64_t ptts_debug_read_encoder(ptts_engine *e, const char *name, float *d_out, int64_t capacity, int32_t *rows,
                                int32_t *cols, void *stream);
/* Test hook: ONE GEMM of the hot path's kernel family (gemm_kernel / gemm_lds_kernel), packed by the engine's own
 * packers and launched through the production dispatcher, on plain row-major device buffers:
 *   y[m][n] = epilogue( sum_tap sum_c pre(x[row(m, tap)][c]) * w[n][c][tap] ),  row(b * T + t, tap) = b * T * xstride + t * xstride + tap - halo
 * (ntaps == 1: a Linear, row(m) = m).  Rows before a sequence's start come from x_prev (halo_mode 0: the previous frame,
 * row b * T * xstride + T * xstride + (t * xstride + tap - halo)), are zero (1) or repeat the sequence's first row (2).
 * Enumerations as in the kernels: wfmt 0 fp32, 1 int8, 2 bf16, 3 split bf16; pre 0 none, 1 ELU, 2 add + SiLU, 3 LayerNorm
 * (folded), 4 modulated LayerNorm; epi 0 store, 1 residual (+ layer scale), 2 gate; act 0 none, 1 GELU, 2 SiLU, 3 ELU.
 * Returns 0 when the GEMM ran, 1 when no kernel exists for the combination (an explicit cfg that the dispatcher does not
 * admit for it, or a (wfmt, pre) pair no kernel implements), < 0 on an error, e.g. a kernel that wrote past its output.
 * Tiles the kernel leaves unwritten read back as NaN.  Synchronises `stream`. */
typedef struct ptts_gemm_case {
  int32_t M, N, C, ntaps;                  /* output rows, output channels, input channels (% 16 == 0), taps */
  int32_t T, xstride, halo, halo_mode;     /* convolutions (ntaps > 1): rows per sequence (% 16 == 0, divides M), see above */
  int32_t wfmt, pre, epi, act;
  int32_t cfg;                             /* configuration 0..17 of the dispatcher's table, -1 = its own choice */
  int32_t krot, lds_target;                /* engine option "k_rotate"; dynamic-LDS target of the codec's launches (bytes) */
  const float *x, *x_prev;                 /* [rows][C], rows = M * xstride (x_prev: halo_mode 0 only) */
  const float *w, *bias;                   /* [N][C][ntaps], [N] or null */
  const float *ln_w, *ln_b;                /* pre 3: LayerNorm gain / bias [C]; pre 4: affine [C] or null */
  const float *prevec;                     /* pre 2: [C] */
  const float *mod_shift, *mod_scale;      /* pre 4: [M][C] */
  const float *r, *g, *ls;                 /* epi 1 / 2: residual, gate [M][N]; epi 1: layer scale [N] or null */
  float *y;                                /* out: [M][N] */
  float *w_eff, *w_eff_lo;                 /* optional out: [N][ntaps * C] weights the kernel consumed, k = tap * C + c (int8:
                                              q * scale; bf16: the bf16 values; split: hi in w_eff, lo in w_eff_lo) */
  float *ln_s, *ln_c;                      /* optional out (pre 3): [N] fold vectors */
  char *label;                             /* optional out: the launch's profiler label */
  int32_t label_cap;
  int32_t cfg_used;                        /* out: the configuration that ran */
} ptts_gemm_case;
int ptts_debug_gemm(ptts_engine *e, ptts_gemm_case *c, void *stream);
/* Test hook: ONE GEMM of the reduced-precision codec (gemm_h_kernel on bf16 operands, fmt 0; gemm_f8_kernel on e4m3
 * operands, fmt 1) or its last conv (pcm_conv_h_kernel, kind 1), packed by the engine's own packers and launched by the
 * production launchers, on plain row-major device buffers:
 *   acc[m][n] = sum_tap sum_c x_eff[row(m, tap)][c] * w_eff[n][tap * C + c],  row(b * T + t, tap) = b * T + t + tap - halo
 * (ntaps == 1: row(m) = m).  Rows before a sequence's start come from the previous frame x_prev (row + T), rows past
 * the end of x read as zero.  x goes into parity half `par` of the kernels' frame-parity double buffer, x_prev into the
 * other, each converted as production converts it (bf16: round to nearest even; e4m3: saturate(x / xs)).
 * w: mode 0 [N][C][ntaps]; mode 1 (ConvTranspose, ntaps 2, N = stride * cout) [C][cout][2 * stride].
 * pre 3 = folded LayerNorm (bf16 Linear only).  epi 0 store (act 0 none / 1 GELU / 3 ELU; yraw = bf16 pre-activation;
 * yf8 = e4m3 output of y * yinv), 1 residual (bf16 r; ls: bf16 only), 3 QKV (bf16 only: RoPE from the table the hook
 * builds with rope_table_kernel, y = [M][q | k | v] with k / v read back from cache slot pos % ring), 6 ConvTranspose
 * (output row m * stride + j takes columns j * cout ..; y [M * stride][cout]).  kind 1: y [M] fp32 PCM, y_i16 its int16
 * twin (widened), w [1][C][ntaps], fmt 0.  cfg: tile 0..3 ({2,4,2,2}, {2,2,2,2}, {1,2,2,2}, {1,1,2,2}), -1 = the
 * dispatcher's choice.  Returns 0 when the kernel ran, 1 when no kernel implements the combination (nothing launched),
 * < 0 on an error, e.g. a kernel that wrote past an output.  Outputs the kernel leaves unwritten read back as NaN.
 * Synchronises `stream`. */
typedef struct ptts_codec_gemm_case {
  int32_t M, N, C, ntaps;                  /* output rows, output channels, input channels (% 32 == 0), taps */
  int32_t T, halo, par;                    /* rows per sequence (ntaps > 1 or kind 1; % 16 == 0, divides M), halo, parity */
  int32_t fmt, kind, pre, epi, act, cfg;
  int32_t mode, cout, stride;              /* weight packing mode; ConvTranspose: cout, stride */
  int32_t yf8, H, Tq, ring, cap;           /* e4m3 output; QKV: heads, rows per sequence, ring (0: linear), cache slots */
  float xs, yinv;                          /* e4m3: activation scale of x, 1 / scale of an e4m3 y */
  const float *x, *x_prev;                 /* [M][C] (x_prev: null = zeros) */
  const float *w, *bias, *ln_w, *ln_b;     /* weights (see above), [N] / [cout] or null, pre 3: LayerNorm gain / bias [C] */
  const float *r, *ls;                     /* epi 1: residual [M][N] (rounded to bf16), layer scale [N] or null */
  const int32_t *offset;                   /* QKV: host [M / Tq] positions of each sequence's first row */
  float *y, *yraw, *y_i16;                 /* out: see above; optional out: yraw (epi 0 / 5), y_i16 (kind 1) */
  float *x_eff, *xp_eff;                   /* optional out: [M][C] activations the kernel consumed (e4m3: decoded * xs) */
  float *w_eff, *wscale;                   /* optional out: [N][ntaps * C] weights consumed (e4m3: decoded * wscale), [N] */
  float *ln_s, *ln_c, *rope;               /* optional out: pre 3 fold vectors [N]; QKV: RoPE table [M][32][2] (cos, sin) */
  char *label;                             /* optional out: the launch's profiler label */
  int32_t label_cap;
  int32_t cfg_used;                        /* out: the tile that ran */
} ptts_codec_gemm_case;
int ptts_debug_codec_gemm(ptts_engine *e, ptts_codec_gemm_case *c, void *stream);
/* Test hook: ONE attention launch of the hot path (attn_kernel / attn_decode_kernel / attn_decode2_kernel /
 * attn_cascade_kernel, + attn_combine_kernel when the keys are split) through the production dispatcher, on plain
 * row-major device buffers.  Row b's queries sit at positions offset[b] .. offset[b] + Tq - 1; its key / value at
 * position p is pk / pv[pre_id[b]][p] when p < pre_len[pre_id[b]] (a shared prefix), else k / v[b][p]:
 *   y[b][t][h * 64 + d] = sum_p softmax_p(q[b][t][h] . key(p) / 8) value(p)[d],  over p <= offset[b] + t and, when ctx > 0,
 *   offset[b] + t - p < ctx.
 * The hook writes each row's keys into cache slots (ring > 0: slot p % ring), builds the prefix table over owner caches
 * of layers 0 .. layer + 1 (the prefix in plane `layer`), and fills every slot a row must not read - and a guard of one
 * key tile on both sides of each buffer - with poison_k / poison_v.  splits -1 = the production rule for the case's
 * shape; kernel -1 = the dispatcher's choice, else an index into its table (ptts.hip kAttn).  Returns 0 when the kernel
 * ran, 1 when the forced kernel does not support the case (nothing launched), < 0 on an error, e.g. a kernel that wrote
 * past its output or partial buffer.  Queries the kernel leaves unwritten read back as NaN.  Synchronises `stream`. */
typedef struct ptts_attn_case {
  int32_t B, Tq, H, T;                     /* rows, queries per row, heads, positions per row in k / v */
  int32_t cap, ring, ctx, splits, h16;     /* cache slots (% 16 == 0), ring (0: linear cache), window (0: none), key
                                              splits (-1: production's), bf16 output (rounded, returned widened) */
  int32_t layer, n_pre, pre_T, pre_cap;    /* prefix plane, prefix banks, positions per bank, owners' capacity (0: cap) */
  int32_t cascade, kernel;                 /* engine option "prefix_cascade" value; kernel table index or -1 */
  float poison_k, poison_v;
  const float *q;                          /* [B][Tq][H][64] */
  const float *k, *v;                      /* [B][T][H][64] */
  const float *pk, *pv;                    /* [n_pre][pre_T][H][64] or null */
  const int32_t *offset;                   /* host [B] */
  const int32_t *pre_len, *pre_id;         /* host [n_pre] (<= offset of every row using it), host [B] (-1: none) */
  float *y;                                /* out: [B][Tq][H * 64] */
  char *label;                             /* optional out: the launch's profiler label */
  int32_t label_cap;
  int32_t kernel_used, splits_used;        /* out */
} ptts_attn_case;
int ptts_debug_attn(ptts_engine *e, ptts_attn_case *c, void *stream);
/* Per-launch profiler (HIP events around every kernel launch on its own stream, tagged with call site,
 * kernel and algorithmic bytes / flops).  stop() writes text lines "site kernel count total_ms bytes flops"
 * to h_out and returns the length.  Never active inside a captured graph. */
int ptts_profile_start(ptts_engine *e);
int64_t ptts_profile_stop(ptts_engine *e, char *h_out, int64_t capacity);
/* Packed weight bytes streamed by one LM decode step / one Mimi frame (roofline accounting) */
int64_t ptts_lm_weight_bytes(ptts_engine *e);
int64_t ptts_mimi_weight_bytes(ptts_engine *e);

#ifdef __cplusplus
}
#endif
#endif /* PTTS_H_ */
