// Launchers of the kernel families that live in their own translation units (compiled in parallel with ptts.hip, see
// pocket_tts_amd/_lib.py::build).  Plain C++ functions: their callers (ptts.hip, ptts_dispatch.hip) never instantiate these
// kernels themselves.  Of an output stage only its enqueue is declared here: what the stages' host sides share, and what
// the output chain reads of a stage (batch, widths), is ptts_stage.h; the chunked scan of the toner's, the compressor's and
// the normaliser's kernels is ptts_scan.h.
#pragma once
#include "ptts_kernels.h"

// ---- ptts_lmh.hip: FlowLM Linear layers with bf16 weights (PTTS_LM_BF16) ------------------------------------------
// register-staged K-split / 2-D tile configurations of gemm_kernel<.., WF = 2>; `cfg` indexes the same table as
// launch_by_cfg in ptts_dispatch.hip (only the b16_cfg() subset exists), `pre` is PRE_NONE or PRE_LNFOLD
void launch_gemm_b16(hipStream_t st, const GemmArgs &a, int pre, int cfg, unsigned dyn_lds);
// fp32 packed image [NT][KF][64][4] (LayerNorm gain already multiplied in) -> bf16 image [NT][KF/2][64][8]; with
// ln_s != null also the fold vector s[n] = sum_k W'[n][k] of the ROUNDED weights (NT * 16 floats)
void pack_weight_b16(hipStream_t st, const float *src, void *dst, float *ln_s, int NT, int KF);

// ---- ptts_fp8.hip: SEANet decoder convolutions on the fp8 MFMA (PTTS_CODEC_FP8) --------------------------------------
// checkpoint conv weight -> e4m3 image [NT][ntaps * C/32][64][8 bytes] + one fp32 scale per output channel (padded to
// NT * 16); same (mode, cout, stride) conventions as pack_weight_kernel
void pack_weight_f8(hipStream_t st, const float *src, void *dst, float *wscale, int N, int C, int ntaps, int mode, int cout, int stride);
// implicit GEMM on e4m3 operands (GemmArgs::X = e4m3 activations in the "FM8" layout, W = e4m3 weights, wscale = per-channel
// weight scale, xs = activation scale of X, yinv = 1 / scale of Y when Y is e4m3 (yf8 = 1), else Y is bf16 FMH);
// choose_f8_tile = the production tile (0..3 of {2,4,2,2}, {2,2,2,2}, {1,2,2,2}, {1,1,2,2}), launch_gemm_f8 runs tile `cfg`
int choose_f8_tile(const GemmArgs &a);
void launch_gemm_f8(hipStream_t st, const GemmArgs &a, int cfg, unsigned dyn_lds);
// max |x| over n bf16 values (calibration of the static activation scales), atomically max-ed into *out (as float bits)
void amax_bf16(hipStream_t st, const void *x, long n, float *out);

// ---- ptts_split.hip: codec GEMMs on error-compensated ("split") bf16 (PTTS_CODEC_SPLIT) ----------------------------------
// every register-staged configuration of gemm_kernel<.., WF = 3> (cfg = index into ptts_dispatch.hip's table; LDS-staged ones do not exist)
void launch_gemm_split(hipStream_t st, const GemmArgs &a, int pre, int cfg, unsigned dyn_lds);
bool split_cfg(int cfg);
// fp32 packed image [NT][KF][64][4] -> hi = bf16(w) and lo = bf16(w - hi) images, each [NT][KF/2][64][8]
void pack_weight_split(hipStream_t st, const float *src, void *hi, void *lo, int NT, int KF);

// ---- ptts_resample.hip: per-request output sample rates (streaming polyphase resampler behind the codec) ---------------
// the frame's two launches on `st`: d_pcm f32[B][frame_samples] (device) -> out f32 / i16 [B][out_max] (device or pinned host),
// then the rows' histories <- the frame's tail.  Returns 0 or a negative error code (message recorded).
struct ptts_resampler;
int resample_enqueue(hipStream_t st, ptts_resampler *rs, const float *d_pcm, void *out, int is_i16);

// ---- ptts_stretch.hip: per-request speaking rate (streaming WSOLA time-stretch behind the codec or the resampler) -------
// the frame's launch on `st`: d_in f32[B][in_max] (device) -> out f32 / i16 [B][out_max] (device or pinned host); d_delta
// (i32 [B][k_max], or null) receives the hops' deltas.  Returns 0 or a negative error code (message recorded).
struct ptts_stretcher;
int stretch_enqueue(hipStream_t st, ptts_stretcher *ts, const float *d_in, void *out, int is_i16, int *d_delta);

// ---- ptts_level.hip: per-request output gain with a look-ahead peak limiter (the last output stage) ---------------------
// the frame's launch on `st`: d_in f32[B][width] (device) -> out f32 / i16 [B][width] (device or pinned host).  Returns 0 or
// a negative error code (message recorded).
struct ptts_leveler;
int level_enqueue(hipStream_t st, ptts_leveler *lv, const float *d_in, void *out, int is_i16);

// ---- ptts_loud.hip: per-request loudness target (streaming BS.1770 normaliser, between the pitcher and the leveler) ------
// the frame's launch on `st`: d_in f32[B][width] (device) -> d_out f32[B][width] (device, never d_in); d_tap (f64 [B][4], or
// null) receives each normalising row's completed sub-blocks, last L, last c and last Z.  Returns 0 or a negative error code.
struct ptts_loudnorm;
int loud_enqueue(hipStream_t st, ptts_loudnorm *ln, const float *d_in, float *d_out, double *d_tap);

// ---- ptts_tone.hip: per-request tone (a streaming cascade of biquad sections, between the pitcher and the normaliser) -----
// the frame's launch on `st`: d_in f32[B][width] (device) -> d_out f32[B][width] (device, never d_in).  Returns 0 or a
// negative error code (message recorded).
struct ptts_tone;
int tone_enqueue(hipStream_t st, ptts_tone *tn, const float *d_in, float *d_out);

// ---- ptts_dyn.hip: per-request dynamics (a streaming feed-forward compressor, between the toner and the normaliser) ------
// the frame's launch on `st`: d_in f32[B][width] (device) -> d_out f32[B][width] (device, never d_in).  Returns 0 or a
// negative error code (message recorded).
struct ptts_dynamics;
int dyn_enqueue(hipStream_t st, ptts_dynamics *dy, const float *d_in, float *d_out);

// ---- ptts_pitch.hip: per-request pitch (streaming WSOLA + polyphase FIR, between the stretcher and the leveler) ---------
// the frame's launch on `st`: d_in f32[B][width] (device) -> out f32 / i16 [B][width] (device or pinned host); d_delta
// (i32 [B][k_max], or null) and d_mid (f32 [B][mid_max], or null) receive the hops' deltas and the frame's mid samples.
// Returns 0 or a negative error code (message recorded).
struct ptts_pitcher;
int pitch_enqueue(hipStream_t st, ptts_pitcher *ps, const float *d_in, void *out, int is_i16, int *d_delta, float *d_mid);

// ---- ptts_encode.hip: per-request output encoding (pcm_s16le, pcm_f32le, G.711 mu-law / A-law; the last output stage) -------
// the frame's launch on `st`: d_in f32[B][width] (device) -> out_bytes u8[B][pitch] (device or pinned host, 16-byte aligned),
// pitch = 4 width rounded up to 16; row b gets n_b * bytes_per_sample(code_b) bytes and nothing behind them.  Returns 0 or a
// negative error code (message recorded).
struct ptts_encoder;
int encode_enqueue(hipStream_t st, ptts_encoder *en, const float *d_in, void *out_bytes);

// ---- ptts_flac.hip: per-request output compression (FLAC frames; the packer behind the encoder) ----------------------------
// the frame's launch on `st`: d_in_bytes u8[B][en_pitch(width)] (device, the encoder's output) -> out_bytes u8[B][fl_pitch(width)]
// (device or pinned host, 16-byte aligned); row b gets the prefix {u32 nbytes, 0, 0, 0}, nbytes bytes and nothing behind 16 +
// nbytes rounded up to 16.  Returns 0 or a negative error code (message recorded).
struct ptts_flac;
int flac_enqueue(hipStream_t st, ptts_flac *pk, const void *d_in_bytes, void *out_bytes);
