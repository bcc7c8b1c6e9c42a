// The dispatchers of libptts: which tile of gemm_kernel / gemm_lds_kernel / gemm_h_kernel / the fp8 family and which attn_*
// kernel a launch gets, the tuner that times the GEMM tiles, and the per-thread knobs they read.  The only unit that
// instantiates those templates; the host side (ptts.hip) and the test hooks (ptts_debug.hip) call it through ptts_host.h.
#include "ptts_host.h"
#include "ptts_bf16.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

// ------------------------------------------------------------------------------------------------
// GEMM dispatch
// int8-weight variants exist for these tiles and for plain / LN-folded operands only
template <int TN, int TM, int WK, int WN, int WM>
static void launch_cfg_q8(hipStream_t st, const GemmArgs &a, int pre) {
  dim3 grid(cdiv(a.NT, TN * WN), cdiv(a.MT, TM * WM));
  dim3 block(64 * WK * WN * WM);
  if (pre == PRE_LNFOLD) gemm_kernel<TN, TM, WK, WN, WM, PRE_LNFOLD, true><<<grid, block, 0, st>>>(a);
  else gemm_kernel<TN, TM, WK, WN, WM, PRE_NONE, true><<<grid, block, 0, st>>>(a);
}

// Occupancy cap of the codec's GEMM launches (engine option "codec_lds_target", bytes <= 64 KB; 0 = off): they request
// dynamic LDS up to this total per workgroup, which limits their workgroups per CU to 160 KB / target and leaves wave slots
// and registers for the FlowLM stream's kernels, whose dependent chain is what the pipelined step waits for.  Measured at
// batch 64 (tools/ab.sh env PTTS_CODEC_LDS_TARGET, final kernels): 0 -> 0.893 ms per step, 36 KB (4 per CU) -> 0.882,
// 44 KB (3) -> 0.864, 56 KB (2) -> 0.851; the codec graph alone 0.548 -> 0.554 (44 KB) -> 0.589 ms (56 KB).
static thread_local int g_lds_target = 0;
static unsigned lds_pad(int static_bytes) { return g_lds_target > static_bytes ? (unsigned)(g_lds_target - static_bytes) : 0u; }
#define LDS_LAUNCH(kernel, grid, block, dyn, st, arg) (kernel)<<<(grid), (block), (dyn), (st)>>>(arg)

template <int TN, int TM, int WK, int WN, int WM>
static void launch_cfg(hipStream_t st, const GemmArgs &a, int pre) {
  dim3 grid(cdiv(a.NT, TN * WN), cdiv(a.MT, TM * WM), pre == PRE_ADDSILU_ROW ? std::max(1, a.row_nz) : 1);
  dim3 block(64 * WK * WN * WM);
  const unsigned dyn = lds_pad(WK > 1 ? WK * WN * WM * TN * TM * 1024 : 0);
  switch (pre) {
    case PRE_NONE: LDS_LAUNCH((gemm_kernel<TN, TM, WK, WN, WM, PRE_NONE>), grid, block, dyn, st, a); break;
    case PRE_LNFOLD: LDS_LAUNCH((gemm_kernel<TN, TM, WK, WN, WM, PRE_LNFOLD>), grid, block, dyn, st, a); break;
    case PRE_LNMOD: LDS_LAUNCH((gemm_kernel<TN, TM, WK, WN, WM, PRE_LNMOD>), grid, block, dyn, st, a); break;
    case PRE_ELU: LDS_LAUNCH((gemm_kernel<TN, TM, WK, WN, WM, PRE_ELU>), grid, block, dyn, st, a); break;
    case PRE_ADDSILU_ROW: LDS_LAUNCH((gemm_kernel<TN, TM, WK, WN, WM, PRE_ADDSILU_ROW>), grid, block, dyn, st, a); break;
    case PRE_LNMOD_ROW: LDS_LAUNCH((gemm_kernel<TN, TM, WK, WN, WM, PRE_LNMOD_ROW>), grid, block, dyn, st, a); break;
    default: LDS_LAUNCH((gemm_kernel<TN, TM, WK, WN, WM, PRE_ADDSILU>), grid, block, dyn, st, a); break;
  }
}

template <int BMT, int BNT>
static void launch_lds(hipStream_t st, const GemmArgs &a, int pre) {
  dim3 grid(cdiv(a.NT, BNT), cdiv(a.MT, BMT));
  // Under the occupancy cap the padded LDS is free, so the capped launches run a THREE-stage ring (two stages in flight
  // with two workgroups per CU): 0.862 -> 0.857 ms per pipelined step; four k-fragments per stage instead: 0.909
  // (tools/ab.sh env PTTS_LDS_VARIANT 0 / 1 / 2).  Uncapped launches keep two stages (never slower, round 1).
  static const int variant = [] { const char *v = getenv("PTTS_LDS_VARIANT"); return v ? atoi(v) : 1; }();
  if constexpr (BMT == 4 && BNT <= 4) {
    if (variant == 1 && g_lds_target) {
      const unsigned dyn3 = lds_pad(3 * (BMT + BNT) * 2 * 1024);
      if (pre == PRE_LNFOLD) gemm_lds_kernel<BMT, BNT, 2, PRE_LNFOLD, 3><<<grid, 256, dyn3, st>>>(a);
      else if (pre == PRE_ELU) gemm_lds_kernel<BMT, BNT, 2, PRE_ELU, 3><<<grid, 256, dyn3, st>>>(a);
      else gemm_lds_kernel<BMT, BNT, 2, PRE_NONE, 3><<<grid, 256, dyn3, st>>>(a);
      return;
    }
    if (variant == 2 && g_lds_target && a.KF % 4 == 0 && pre != PRE_ELU) {
      const unsigned dyn4 = lds_pad(2 * (BMT + BNT) * 4 * 1024);
      if (pre == PRE_LNFOLD) gemm_lds_kernel<BMT, BNT, 4, PRE_LNFOLD><<<grid, 256, dyn4, st>>>(a);
      else gemm_lds_kernel<BMT, BNT, 4, PRE_NONE><<<grid, 256, dyn4, st>>>(a);
      return;
    }
  }
  const unsigned dyn = lds_pad(2 * (BMT + BNT) * 2 * 1024);
  if (pre == PRE_LNFOLD) LDS_LAUNCH((gemm_lds_kernel<BMT, BNT, 2, PRE_LNFOLD>), grid, dim3(256), dyn, st, a);
  else if (pre == PRE_ELU) LDS_LAUNCH((gemm_lds_kernel<BMT, BNT, 2, PRE_ELU>), grid, dim3(256), dyn, st, a);
  else LDS_LAUNCH((gemm_lds_kernel<BMT, BNT, 2, PRE_NONE>), grid, dim3(256), dyn, st, a);
}

// Tile selection.  K-split configs (TM row tiles per wave, 4 waves split K, LDS-reduced) give NT x ceil(MT/TM)
// workgroups and stream each weight fragment ceil(MT/TM) times (L2 / Infinity Cache absorb the re-reads);
// the 2-D tiled configs amortise operand loads over 2x4 tiles per wave but need a large grid to fill 256 CUs.
// Pick the K-split row-tile count TM that still yields >= ~256 workgroups, and use 2-D tiles only when
// their grid is large.
static int pick_cfg(const GemmArgs &a) {
  const long tiled = (long)cdiv(a.NT, 4) * cdiv(a.MT, 8);
  // many rows (codec convs at batch >= 16): LDS-staged kernel, each operand fragment DMA'd once per workgroup
  // (tests/hip/sweep_gemm.hip: 5-12 % faster than the register-staged tiles on these shapes)
  if (a.MT >= 256 && a.NT >= 4 && a.KF % 2 == 0 && a.epi != EPI_QKV && !a.mod_scale) return a.NT >= 8 ? 8 : 9;
  if (a.MT > 4 && tiled >= 192) return a.NT >= 4 ? 3 : a.NT >= 2 ? 4 : 5;
  // few output tiles but a long K (Mimi FFN2 / conv k7 / out_proj at moderate batch): 2x4 tiles per wave,
  // the 4 waves of a workgroup split K -> 4x the workgroups of the 2-D tiling at the same operand reuse
  if (a.MT >= 8 && a.NT >= 2 && a.KF >= 32 && (long)cdiv(a.NT, 2) * cdiv(a.MT, 4) >= 128) return 7;
  if (a.MT > 64) {  // K-split would re-stream weights too often
    if (tiled < 192) return 6;  // small problem, many rows: one tile per wave for the largest grid
    return a.NT >= 4 ? 3 : a.NT >= 2 ? 4 : 5;
  }
  int tm = a.MT >= 4 ? 4 : a.MT >= 2 ? 2 : 1;
  while (tm > 1 && (long)a.NT * cdiv(a.MT, tm) < 256) tm >>= 1;
  return tm == 4 ? 2 : tm == 2 ? 1 : 0;
}
static const char *const kCfgName[kNumCfg] = {
    "gemm<1,1,8,1,1>", "gemm<1,2,4,1,1>", "gemm<1,4,4,1,1>", "gemm<2,4,1,2,2>", "gemm<2,4,1,1,4>", "gemm<1,4,1,1,4>",
    "gemm<1,1,1,1,4>", "gemm<2,4,4,1,1>", "gemm_lds<4,8,2>", "gemm_lds<4,4,2>", "gemm<2,2,4,1,1>", "gemm<1,1,4,1,1>",
    "gemm_lds<4,2,2>", "gemm<1,2,1,2,2>", "gemm<2,4,2,2,1>", "gemm_lds<8,8,2>", "gemm_lds<8,4,2>", "gemm_lds<8,2,2>"};
// {TN, TM, WK, WN, WM} of the register-staged configs, {BNT, BMT, 0, 0, 0} of the LDS-staged ones
static const int kCfgShape[kNumCfg][5] = {{1, 1, 8, 1, 1}, {1, 2, 4, 1, 1}, {1, 4, 4, 1, 1}, {2, 4, 1, 2, 2}, {2, 4, 1, 1, 4},
                                          {1, 4, 1, 1, 4}, {1, 1, 1, 1, 4}, {2, 4, 4, 1, 1}, {8, 4, 0, 0, 0}, {4, 4, 0, 0, 0},
                                          {2, 2, 4, 1, 1}, {1, 1, 4, 1, 1}, {2, 4, 0, 0, 0}, {1, 2, 1, 2, 2}, {2, 4, 2, 2, 1},
                                          {8, 8, 0, 0, 0}, {4, 8, 0, 0, 0}, {2, 8, 0, 0, 0}};

static bool q8_cfg(int cfg) { return cfg == 0 || cfg == 1 || cfg == 2 || cfg == 3 || cfg == 7 || cfg == 10 || cfg == 11; }
// bf16 weights: the int8 set without the 8-wave single tile.  Its bf16 instantiation returned non-finite garbage whenever a
// wave owned more than one chunk of k-fragments (K >= 1024 in tests/test_gpu_gemm_matrix.py; exact at K <= 512), while the
// 4-wave K-split, the 2-D tilings and the fp32 / int8 8-wave instantiations are exact on every shape there.  The cause is not
// known, so the instantiation does not exist (launch_gemm_b16).
static bool b16_cfg(int cfg) { return cfg != 0 && q8_cfg(cfg); }

bool cfg_valid(int cfg, const GemmArgs &a, int pre) {
  const int *s = kCfgShape[cfg];
  if (a.wfmt == 3) {  // split bf16: every register-staged configuration, whole pairs of k-fragments per wave
    if (!split_cfg(cfg) || (pre != PRE_NONE && pre != PRE_LNFOLD)) return false;
    if (a.KF % (2 * s[2])) return false;
  } else if (a.wfmt) {  // whole groups of four (int8) / two (bf16) k-fragments per wave
    if (!(a.wfmt == 2 ? b16_cfg(cfg) : q8_cfg(cfg)) || (pre != PRE_NONE && pre != PRE_LNFOLD)) return false;
    if (a.KF % ((a.wfmt == 1 ? 4 : 2) * s[2])) return false;
  }
  if (s[2] == 0) {  // LDS-staged: two k-fragments per stage, plain or LN-folded operand only
    if (a.KF % 2 || (pre != PRE_NONE && pre != PRE_LNFOLD && pre != PRE_ELU)) return false;
    return a.MT >= s[1] && 2 * a.NT >= s[0];
  }
  const int tn = s[0] * s[3], tm = s[1] * s[4];
  if (tm > 1 && tm > 2 * a.MT) return false;  // mostly padding
  if (tn > 1 && tn > 2 * a.NT) return false;
  if (s[2] > 1 && a.KF < 2) return false;  // nothing to split
  return true;
}

// XCD-aware mapping (tile_of_block) when the activations outweigh the weights and several column blocks re-read them
// (PMC: conv k7 with 7.3 MB of weights and 2 MB of activations fetched 112 MB when it was swizzled by rows)
static int swz_for(int cfg, const GemmArgs &a) {
  static const int swz_env = [] { const char *v = getenv("PTTS_SWZ"); return v ? atoi(v) : -1; }();
  const int *sh = kCfgShape[cfg];
  const int gx = sh[2] == 0 ? cdiv(a.NT, sh[0]) : cdiv(a.NT, sh[0] * sh[3]);
  if (gx <= 1) return 0;
  // swizzle when the activations (M x C) outweigh the weights (N x K, K = taps x C)
  return swz_env >= 0 ? swz_env : ((double)a.M * a.CF > (double)a.NT * 16 * a.KF && a.MT >= 64);
}

static void launch_by_cfg(hipStream_t st, const GemmArgs &a_in, int pre, int cfg) {
  GemmArgs a = a_in;
  a.swz = swz_for(cfg, a);
  if (a.wfmt == 2) {
    launch_gemm_b16(st, a, pre, cfg, 0);
    return;
  }
  if (a.wfmt == 3) {
    const int *sh = kCfgShape[cfg];
    launch_gemm_split(st, a, pre, cfg, lds_pad(sh[2] > 1 ? sh[2] * sh[3] * sh[4] * sh[0] * sh[1] * 1024 : 0));
    return;
  }
  if (a.wfmt == 1) {
    switch (cfg) {
      case 0: launch_cfg_q8<1, 1, 8, 1, 1>(st, a, pre); break;
      case 1: launch_cfg_q8<1, 2, 4, 1, 1>(st, a, pre); break;
      case 2: launch_cfg_q8<1, 4, 4, 1, 1>(st, a, pre); break;
      case 7: launch_cfg_q8<2, 4, 4, 1, 1>(st, a, pre); break;
      case 10: launch_cfg_q8<2, 2, 4, 1, 1>(st, a, pre); break;
      case 11: launch_cfg_q8<1, 1, 4, 1, 1>(st, a, pre); break;
      default: launch_cfg_q8<2, 4, 1, 2, 2>(st, a, pre); break;  // 3: no K split, any KF % 4 == 0
    }
    return;
  }
  switch (cfg) {
    case 0: launch_cfg<1, 1, 8, 1, 1>(st, a, pre); break;  // 8 waves: most bytes in flight per CU for cold weights
    case 1: launch_cfg<1, 2, 4, 1, 1>(st, a, pre); break;
    case 2: launch_cfg<1, 4, 4, 1, 1>(st, a, pre); break;
    case 3: launch_cfg<2, 4, 1, 2, 2>(st, a, pre); break;
    case 4: launch_cfg<2, 4, 1, 1, 4>(st, a, pre); break;
    case 5: launch_cfg<1, 4, 1, 1, 4>(st, a, pre); break;
    case 6: launch_cfg<1, 1, 1, 1, 4>(st, a, pre); break;
    case 7: launch_cfg<2, 4, 4, 1, 1>(st, a, pre); break;
    case 8: launch_lds<4, 8>(st, a, pre); break;
    case 9: launch_lds<4, 4>(st, a, pre); break;
    case 10: launch_cfg<2, 2, 4, 1, 1>(st, a, pre); break;
    case 11: launch_cfg<1, 1, 4, 1, 1>(st, a, pre); break;
    case 12: launch_lds<4, 2>(st, a, pre); break;
    case 13: launch_cfg<1, 2, 1, 2, 2>(st, a, pre); break;
    case 14: launch_cfg<2, 4, 2, 2, 1>(st, a, pre); break;
    case 16: launch_lds<8, 4>(st, a, pre); break;
    case 17: launch_lds<8, 2>(st, a, pre); break;
    default: launch_lds<8, 8>(st, a, pre); break;
  }
}

// The tuner (struct Tuner, ptts_host.h) and the other per-thread state of the dispatchers
static constexpr int kTuneVersion = 2;  // bump when the key or the configuration list changes (cache files carry it)
static thread_local bool g_use_split = false;  // set around the codec's enqueue by engines built with PTTS_CODEC_SPLIT
static thread_local Tuner *g_tuner = nullptr;
static thread_local const float *g_zeros = nullptr;  // both set by the entry points from the engine
static thread_local int g_krot = 1;
KnobScope::KnobScope(int lds_target, int k_rotate, bool use_split) : lds(g_lds_target), krot(g_krot), split(g_use_split) {
  g_krot = k_rotate; g_use_split = use_split; g_lds_target = lds_target;
}
KnobScope::~KnobScope() { g_lds_target = lds; g_use_split = split; g_krot = krot; }
void bind_dispatch(const ptts_engine *e) {
  g_zeros = e->zeros;
  g_tuner = e->tuner;
  g_krot = e->opt_k_rotate;
}
void unbind_dispatch(const ptts_engine *e) {
  if (g_tuner == e->tuner) g_tuner = nullptr;
}

static TuneKey tune_key(const GemmArgs &a, int pre) {
  return TuneKey{a.NT, a.KF, a.CF, a.ntaps, a.MT, a.epi, pre, a.act, a.xstride, a.halo_mode, a.Yraw ? 1 : 0, a.R ? 1 : 0, a.wfmt};
}

// Evicts L2 and the Infinity Cache by READING a large buffer (a write flush would leave dirty lines whose
// write-back then competes with the timed kernel).
__global__ void flush_read_kernel(const f32x4 *p, size_t n, float *sink) {
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) s += p[i];
  if (s.x + s.y + s.z + s.w == 123.456f) *sink = s.x;  // never true for a zero buffer; keeps the loads alive
}

static int tune_one(hipStream_t st, const GemmArgs &a, int pre, Tuner &t) {
  // tiles are timed WITHOUT the codec's occupancy cap: under it the LDS-staged tiles look slower alone and the search drifts
  // to the register-heavy K-split tiles, which cost the pipelined step 6 % (tools/ab.sh cache)
  struct NoCap { int keep; NoCap() : keep(g_lds_target) { g_lds_target = 0; } ~NoCap() { g_lds_target = keep; } } nocap;
  int best = pick_cfg(a);
  float best_ms = 1e30f, heur_ms = 0.f;
  const int heur = best;
  // PTTS_TUNE_EXCLUDE="9,12": experiment knob, drops configurations from the search
  static const unsigned excl = [] {
    unsigned m = 0;
    if (const char *v = getenv("PTTS_TUNE_EXCLUDE"))
      for (const char *p = v; *p;) { m |= 1u << (atoi(p) & 31); while (*p && *p != ',') ++p; if (*p) ++p; }
    return m;
  }();
  static const bool verbose = getenv("PTTS_TUNE_VERBOSE") != nullptr;  // log every configuration's time
  std::string all;
  for (int cfg = 0; cfg < kNumCfg; ++cfg) {
    if (!cfg_valid(cfg, a, pre) || ((excl >> cfg) & 1)) continue;
    float ms_min = 1e30f;
    for (int r = 0; r < 4; ++r) {
      if (t.flush) flush_read_kernel<<<4096, 256, 0, st>>>((const f32x4 *)t.flush, t.flush_bytes / 16, (float *)t.flush);
      (void)hipEventRecord(t.e0, st);
      launch_by_cfg(st, a, pre, cfg);
      (void)hipEventRecord(t.e1, st);
      if (hipEventSynchronize(t.e1) != hipSuccess) return heur;
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, t.e0, t.e1);
      ms_min = std::min(ms_min, ms);
    }
    if (cfg == heur) heur_ms = ms_min;
    if (ms_min < best_ms) { best_ms = ms_min; best = cfg; }
    if (verbose) { char b[64]; snprintf(b, sizeof b, " %d:%.1f", cfg, ms_min * 1e3); all += b; }
  }
  if (best_ms > 1e29f) return heur;
  char line[256];
  snprintf(line, sizeof line, "%s NT=%d KF=%d taps=%d MT=%d epi=%d pre=%d: %s %.1f us (heuristic %s %.1f us)\n", launch_site(), a.NT,
           a.KF, a.ntaps, a.MT, a.epi, pre, kCfgName[best], best_ms * 1e3, kCfgName[heur], heur_ms * 1e3);
  t.log += line;
  if (verbose) t.log += "   all (cfg:us)" + all + "\n";
  return best;
}

// The int8, bf16 and split-bf16 kernels exist for plain and LN-folded operands only: any other operand pre-processing with
// those weights has no kernel (never a fall-back to one that would ignore `pre`)
bool pre_supported(int wfmt, int pre) { return wfmt == 0 || pre == PRE_NONE || pre == PRE_LNFOLD; }

// The dispatcher's configuration for one GEMM: the tuner's table (or a live tuning run), PTTS_FORCE_CFG, else pick_cfg,
// then the weight formats' fall-backs among the admitted configurations.  -1: no kernel implements (wfmt, pre).
int choose_cfg(hipStream_t st, const GemmArgs &a, int pre) {
  if (!pre_supported(a.wfmt, pre)) return -1;
  int cfg = -1;
  if (g_tuner) {
    const TuneKey key = tune_key(a, pre);
    auto it = g_tuner->table.find(key);
    if (it != g_tuner->table.end()) cfg = it->second;
    else if (g_tuner->active) cfg = g_tuner->table[key] = tune_one(st, a, pre, *g_tuner);
  }
  {
    // PTTS_FORCE_CFG="NT:MT:cfg[,NT:MT:cfg...]": experiment knob, pins the configuration of one GEMM shape
    static const std::vector<std::array<int, 3>> forced = [] {
      std::vector<std::array<int, 3>> v;
      if (const char *e = getenv("PTTS_FORCE_CFG")) {
        std::array<int, 3> t;
        const char *p = e;
        while (sscanf(p, "%d:%d:%d", &t[0], &t[1], &t[2]) == 3) {
          v.push_back(t);
          while (*p && *p != ',') ++p;
          if (!*p) break;
          ++p;
        }
      }
      return v;
    }();
    for (auto &f : forced)
      if (f[0] == a.NT && f[1] == a.MT && f[2] >= 0 && f[2] < kNumCfg && cfg_valid(f[2], a, pre)) cfg = f[2];
  }
  if (cfg < 0 || !cfg_valid(cfg, a, pre)) cfg = pick_cfg(a);
  if (a.wfmt == 3 && !cfg_valid(cfg, a, pre)) {  // the heuristic may name an LDS-staged tile: nearest register-staged one
    cfg = a.MT >= 8 ? 3 : 13;
    for (int c : {3, 13, 4, 6, 11}) if (cfg_valid(c, a, pre)) { cfg = c; break; }
  }
  if (a.wfmt && a.wfmt != 3 && !cfg_valid(cfg, a, pre)) cfg = (a.wfmt == 2 && !cfg_valid(3, a, pre) && cfg_valid(11, a, pre)) ? 11 : 3;
  return cfg;
}

// Launches configuration `cfg` (admitted by cfg_valid), bracketed by the profiler under its label; `label` != null receives it
void launch_gemm_cfg(hipStream_t st, const GemmArgs &a, int pre, int cfg, std::string *label) {
  // algorithmic traffic: weights once + input rows once (x taps re-read from cache, not counted) + output
  const double K = (double)a.KF * 16, N = (double)a.NT * 16, M = (double)a.M;
  double bytes = 4.0 * (N * K + M * (double)a.CF * 16 + M * N);
  if (a.epi == EPI_RES || a.epi == EPI_GATE) bytes += 4.0 * M * N;
  if (a.wfmt == 1) bytes -= 3.0 * N * K;  // one byte per weight
  if (a.wfmt == 2) bytes -= 2.0 * N * K;  // two
  // label = configuration + operand variant + "@<work-items>" (what rocprofv3 reports as Grid_Size), so that the
  // launches of one label are GEMMs of one grid, i.e. of one (NT, MT) shape class
  const int *sh = kCfgShape[cfg];
  const long wgs = sh[2] == 0 ? (long)cdiv(a.NT, sh[0]) * cdiv(a.MT, sh[1])
                              : (long)cdiv(a.NT, sh[0] * sh[3]) * cdiv(a.MT, sh[1] * sh[4]);
  const long threads = wgs * (sh[2] == 0 ? 256 : 64 * sh[2] * sh[3] * sh[4]);
  std::string name = std::string(kCfgName[cfg]) + (pre == PRE_NONE ? "" : pre == PRE_LNFOLD ? "+ln" : pre == PRE_LNMOD ? "+lnmod" : pre == PRE_ELU ? "+elu" : pre == PRE_ADDSILU_ROW ? "+addsilu_row" : pre == PRE_LNMOD_ROW ? "+lnmod_row" : "+addsilu") +
                     (a.wfmt == 1 ? "+q8" : a.wfmt == 2 ? "+b16" : a.wfmt == 3 ? "+split" : "") + "@" + std::to_string(threads);
  if (label) *label = name;
  ProfScope ps(st, name, bytes, 2.0 * M * N * K);
  launch_by_cfg(st, a, pre, cfg);
}

void launch_gemm(hipStream_t st, const GemmArgs &a_in, int pre) {
  GemmArgs a = a_in;
  a.zeros = g_zeros;
  a.krot = g_krot;
  if (a.epi == EPI_PCM && a.NT == 1 && pre == PRE_NONE && !a.Wq && a.CF == 4 && a.ntaps <= 4) {  // one output channel: vector-ALU kernel
    const double K = (double)a.KF * 16, M = (double)a.M;
    ProfScope ps(st, "pcm_conv", 4.0 * (M * (double)a.CF * 16 + M), 2.0 * M * K);
    pcm_conv_kernel<<<cdiv(a.MT, 4), 256, 0, st>>>(a);
    return;
  }
  int cfg;
  if (pre == PRE_ADDSILU_ROW || pre == PRE_LNMOD_ROW) {  // the tile of the plain GEMM: per-row schedules sum in the same order
    GemmArgs b = a;
    b.row_nz = 0;
    cfg = choose_cfg(st, b, pre == PRE_LNMOD_ROW ? PRE_LNMOD : PRE_ADDSILU);
  } else {
    cfg = choose_cfg(st, a, pre);
  }
  if (cfg < 0) {
    note_launch_err(std::string("no GEMM kernel for weight format ") + std::to_string(a.wfmt) + " with operand pre-processing " +
                    std::to_string(pre) + " (site " + launch_site() + ")");
    return;
  }
  launch_gemm_cfg(st, a, pre, cfg);
}

// k3 conv + ELU + 1x1 conv + skip of a SEANet residual block in one launch (a = the k3 conv's arguments with Y / R
// already describing the block's output and skip input)
bool resblock_fusable(const Lin &A, const Lin &Bl, int MT) {
  return !A.wq && !Bl.wq && A.bias && Bl.bias && Bl.ntaps == 1 && Bl.KF == A.NT && A.KF % 2 == 0 && MT >= 4 &&
         ((A.NT == 2 && Bl.NT == 4) || (A.NT == 4 && Bl.NT == 8));
}
void launch_resblock(hipStream_t st, GemmArgs a, const Lin &Bl, int pre) {
  a.zeros = g_zeros;
  a.W2 = Bl.w; a.bias2 = Bl.bias;
  const double M = a.M, K = a.KF * 16.0, N = a.NT * 16.0, N2 = Bl.NT * 16.0;
  ProfScope ps(st, std::string(a.NT == 2 ? "resblock<2,4>" : "resblock<4,8>") + (pre == PRE_ELU ? "+elu" : "") + "@" + std::to_string((long)cdiv(a.MT, 4) * 256),
               4.0 * (N * K + N2 * N + M * a.CF * 16.0 + (pre == PRE_ELU ? 1.0 : 2.0) * M * N2), 2.0 * M * N * K + 2.0 * M * N2 * N);
  dim3 grid(1, cdiv(a.MT, 4));
  if (pre == PRE_ELU) {
    if (a.NT == 2) LDS_LAUNCH((gemm_lds_kernel<4, 2, 2, PRE_ELU, 2, 4>), grid, dim3(256), lds_pad(24 * 1024), st, a);
    else LDS_LAUNCH((gemm_lds_kernel<4, 4, 2, PRE_ELU, 2, 8>), grid, dim3(256), lds_pad(32 * 1024), st, a);
    return;
  }
  if (a.NT == 2) LDS_LAUNCH((gemm_lds_kernel<4, 2, 2, PRE_NONE, 2, 4>), grid, dim3(256), lds_pad(24 * 1024), st, a);
  else LDS_LAUNCH((gemm_lds_kernel<4, 4, 2, PRE_NONE, 2, 8>), grid, dim3(256), lds_pad(32 * 1024), st, a);
}

GemmArgs mk_gemm(const Lin &L, const float *X, int XF, int MT, int M) {
  GemmArgs a;
  memset(&a, 0, sizeof(a));
  a.W = L.w;
  a.Wq = L.wq ? L.wq : (const uint8_t *)L.wb16;
  a.wfmt = L.wq ? 1 : L.wb16 ? 2 : 0;
  if (g_use_split && L.wsh) {  // codec launches of a PTTS_CODEC_SPLIT engine: hi image in Wq, lo image in W
    a.Wq = (const uint8_t *)L.wsh;
    a.W = (const float *)L.wsl;
    a.wfmt = 3;
  }
  a.wscale = L.wscale;
  a.ln_g = L.ln_g;
  a.bias = L.bias;
  a.ln_s = L.ln_s;
  a.ln_c = L.ln_c;
  a.ln_eps = 1e-5f;  // nn.LayerNorm(eps=1e-5): mimi_transformer.py:26-27, flow_lm.py:89
  a.NT = L.NT;
  a.KF = L.KF;
  a.CF = L.CF;
  a.ntaps = L.ntaps;
  a.X = X;
  a.XF = XF;
  a.MT = MT;
  a.M = M;
  a.T = 16;
  a.xstride = 1;
  a.halo = L.ntaps - 1;  // streaming causal conv: kernel - 1 rows of left context (stride 1)
  a.halo_mode = 0;
  a.epi = EPI_STORE;
  a.act = ACT_NONE;
  return a;
}

// waves per (sequence, head) in the decode attention: enough to reach the wave target, at most 8 (one workgroup)
static int decode_attn_waves(int BH) {
  static const int forced = [] { const char *v = getenv("PTTS_ATTN_NW"); return v ? atoi(v) : 0; }();
  if (forced) return forced;
  int nw = 1;
  while (nw < 8 && BH * nw * 2 <= 1024) nw *= 2;
  return nw;
}
static int attn_wave_target() {
  static int t = [] { const char *v = getenv("PTTS_ATTN_WAVES"); return v ? atoi(v) : 1024; }();
  return t;
}
// waves per workgroup of attn_kernel (they split the workgroup's key tiles and merge in LDS, no combine launch).
// Only for small launches: on the codec frame at batch 64 (512 (sequence, head) pairs, 17 key tiles) 4 waves x 1 split
// is faster alone (18.2 us against 19.8 us + the combine launch, tests/hip/sweep_attn.hip) but SLOWER in the two-stream
// pipeline (0.958 vs 0.947 ms per step, 2 waves 0.963 vs 0.955; tools/ab.sh env PTTS_ATTN_KERNEL_NW): the extra resident waves delay
// the FlowLM stream's kernels.  At batch 8 / 1 it saves 1.5 / 1.1 us per layer.
static int attn_nw(int base) {
  static const int forced = [] { const char *v = getenv("PTTS_ATTN_KERNEL_NW"); return v ? atoi(v) : 0; }();  // A/B knob
  if (forced) return forced;
  return base <= 128 ? 4 : (base <= 256 ? 2 : 1);
}
int attn_splits(int base, int max_tiles) {
  // `base` = (sequence, head, query block) triples.  Keys are split over workgroups only until ~1024 waves exist
  // (measured at batch 64: 1024 -> 1.139 ms/step, 4096 -> 1.168, 8192 -> 1.211; more splits only add combine launches);
  // a wave never gets less than ~1 key tile.  PTTS_ATTN_WAVES overrides the target for experiments.
  const int nw = attn_nw(base);
  const int tiles = cdiv(max_tiles, nw);
  int s = std::max(1, cdiv(attn_wave_target(), std::max(1, base * nw)));
  return std::max(1, std::min(s, tiles));
}
// Every compiled attention instantiation: the dispatcher's table (ptts_debug_attn's `kernel` indexes it, tests/
// test_gpu_attn_matrix.py mirrors it).  family 0 = attn_kernel<nw, depth>, 1 = attn_decode_kernel<nw>, 2 =
// attn_decode2_kernel<nw, depth>, 3 = attn_cascade_kernel<R = nw, pw, depth, ns>; `code` = the "prefix_cascade" /
// PTTS_CASCADE value that names a cascade shape (every shape besides the default <4, 2, 3, 1> is an A/B knob: all shapes
// measured are in profiles/r03_experiments.txt, more waves per workgroup or a fourth register tile lose beside the codec stream)
enum {
  AK_ATTN4, AK_ATTN2, AK_ATTN1, AK_ATTN1_D2, AK_DEC1, AK_DEC2_1_2, AK_DEC2_1_3, AK_DEC2_2_3, AK_DEC2_4_3, AK_DEC2_8_3,
  AK_CASC, AK_CASC_442, AK_CASC_222, AK_CASC_42, AK_CASC_44, AK_CASC_84, AK_CASC_22, AK_COUNT
};
static_assert(AK_COUNT == kNumAttn, "ptts_host.h declares the table's size");
const AttnKernelInfo kAttn[kNumAttn] = {
    {0, 4, 0, 3, 0, 0, "attn<4,3>"}, {0, 2, 0, 3, 0, 0, "attn<2,3>"}, {0, 1, 0, 3, 0, 0, "attn<1,3>"}, {0, 1, 0, 2, 0, 0, "attn<1,2>"},
    {1, 1, 0, 3, 0, 0, "attn_decode<1>"}, {2, 1, 0, 2, 0, 0, "attn_decode2<1,2>"}, {2, 1, 0, 3, 0, 0, "attn_decode2<1,3>"},
    {2, 2, 0, 3, 0, 0, "attn_decode2<2,3>"}, {2, 4, 0, 3, 0, 0, "attn_decode2<4,3>"}, {2, 8, 0, 3, 0, 0, "attn_decode2<8,3>"},
    {3, 4, 2, 3, 1, 423, "attn_cascade<4,2,3,1>"}, {3, 4, 4, 2, 2, 442, "attn_cascade<4,4,2,2>"},
    {3, 2, 2, 2, 2, 222, "attn_cascade<2,2,2,2>"}, {3, 4, 2, 2, 1, 42, "attn_cascade<4,2,2,1>"},
    {3, 4, 4, 2, 1, 44, "attn_cascade<4,4,2,1>"}, {3, 8, 4, 2, 1, 84, "attn_cascade<8,4,2,1>"},
    {3, 2, 2, 2, 1, 22, "attn_cascade<2,2,2,1>"},
};

// What each kernel supports (production and ptts_debug_attn both ask this before a launch):
//   every kernel: Tq >= 1 queries in QB = ceil(Tq / 16) blocks, a cache of cap % 16 == 0 slots per (sequence, head), at
//   least one split (a partial buffer when more);
//   a ring (slot = position % ring) holds whole tiles (ring % 16 == 0, ring <= cap), has a window (ctx > 0) and keeps
//   every key a query block attends (ring >= ctx + Tq - 1); shared prefixes (KvPrefix) are for linear caches only;
//   decode and cascade kernels: one query per sequence, fp32 output (they ignore h16), no per-sequence query count (qlen);
//   cascade: additionally one split, no ring, no window and a prefix table.
bool attn_valid(int k, const AttnArgs &a) {
  if (k < 0 || k >= kNumAttn) return false;
  if (a.H < 1 || a.Tq < 1 || a.QB != cdiv(a.Tq, 16) || a.cap < 16 || a.cap % 16 || a.splits < 1 || a.nseq < 1) return false;
  if (a.splits > 1 && !a.part) return false;
  if (a.ring && (a.ring % 16 || a.ring > a.cap || a.ctx <= 0 || a.ring < a.ctx + a.Tq - 1 || a.pre)) return false;
  const AttnKernelInfo &K = kAttn[k];
  if (K.family != 0 && (a.Tq != 1 || a.h16 || a.qlen)) return false;
  if (K.family == 3 && (a.splits != 1 || a.ring || a.ctx > 0 || !a.pre)) return false;
  return true;
}

// The production choice for a launch of BH = nseq * H (sequence, head) pairs; `cascade` = the engine's "prefix_cascade"
// value when the sequences may share prefixes (0: never the cascade kernel)
int choose_attn(const AttnArgs &a, int BH, int cascade) {
  if (a.Tq == 1 && !a.qlen && cascade && a.pre && a.splits == 1 && !a.ring && a.ctx <= 0 && a.nseq >= 16) {
    // sequences cloned from one voice: prefix keys as MFMA tiles shared by R sequences, private keys per sequence,
    // merged in LDS.  Tile shape: tools/ab.sh env PTTS_CASCADE
    for (int k = AK_CASC + 1; k < kNumAttn; ++k)
      if (kAttn[k].code == cascade) return k;
    return AK_CASC;
  }
  if (a.Tq == 1 && !a.qlen) {  // (a ragged prefill of one position: attn_kernel, which skips the sequences without a query)
    // one query: vector ALU + wave reductions.  The keys of a (sequence, head) are split over the nw waves of ONE
    // workgroup and merged in LDS, so small batches reach ~1024 waves without partial buffers or a combine launch.
    // The row-state kernel (no cross-row traffic in its loop).  Small batches: three register tiles (6.0 vs 7.2 us per
    // layer at batch 1, 221 keys).  >= 1024 (sequence, head) pairs: TWO register tiles - alone it streams at the rate of
    // the first kernel (attn_decode_kernel, 188 VGPRs, still selectable with PTTS_ATTN_V=1), but at ~110 registers per wave
    // it leaves the codec stream its occupancy: 0.904 -> 0.877 ms per pipelined step at batch 64 (tools/ab.sh env
    // PTTS_ATTN_V; three tiles: 0.881)
    const int nw = decode_attn_waves(BH);
    if (nw >= 8) return AK_DEC2_8_3;
    if (nw == 4) return AK_DEC2_4_3;
    if (nw == 2) return AK_DEC2_2_3;
    static const int v = [] { const char *e = getenv("PTTS_ATTN_V"); return e ? atoi(e) : 2; }();  // A/B knob
    return v == 1 ? AK_DEC1 : v == 3 ? AK_DEC2_1_3 : AK_DEC2_1_2;
  }
  const int nw = attn_nw(BH * a.QB);
  // large launches (one wave per workgroup) keep two register tiles instead of three: 32 registers less per wave, 0.854 ->
  // 0.850 ms per pipelined step at batch 64 (tools/ab.sh env PTTS_ATTN_DEPTH)
  static const int depth = [] { const char *v = getenv("PTTS_ATTN_DEPTH"); return v ? atoi(v) : 2; }();  // A/B knob
  if (nw == 4) return AK_ATTN4;
  if (nw == 2) return AK_ATTN2;
  return depth == 2 ? AK_ATTN1_D2 : AK_ATTN1;
}

// Launches kernel `k` (admitted by attn_valid) for BH (sequence, head) pairs, bracketed by the profiler; label = kernel
// family + "@<work-items>" (what rocprofv3 reports as Grid_Size)
static void launch_attn_kernel(hipStream_t st, const AttnArgs &at, int BH, int k, double bytes, double flops, std::string *label) {
  const AttnKernelInfo &K = kAttn[k];
  const long wgs = K.family == 3 ? (long)cdiv(at.nseq, K.nw) * at.H : K.family == 0 ? (long)BH * at.QB * at.splits : (long)BH * at.splits;
  const int threads = 64 * (K.family == 3 ? K.nw * K.ns + K.pw : K.nw);
  const std::string name = std::string(K.family == 0 ? "attn" : K.family == 3 ? "attn_cascade" : "attn_decode") + "@" + std::to_string(wgs * threads);
  if (label) *label = name;
  ProfScope ps(st, name, bytes, flops);
  const dim3 grid(BH, at.QB, at.splits), dgrid(BH, 1, at.splits);
  switch (k) {
    case AK_ATTN4: attn_kernel<4><<<grid, threads, 0, st>>>(at); break;
    case AK_ATTN2: attn_kernel<2><<<grid, threads, 0, st>>>(at); break;
    case AK_ATTN1: attn_kernel<1><<<grid, threads, 0, st>>>(at); break;
    case AK_ATTN1_D2: attn_kernel<1, 2><<<grid, threads, 0, st>>>(at); break;
    case AK_DEC1: attn_decode_kernel<1><<<dgrid, threads, 0, st>>>(at); break;
    case AK_DEC2_1_2: attn_decode2_kernel<1, 2><<<dgrid, threads, 0, st>>>(at); break;
    case AK_DEC2_1_3: attn_decode2_kernel<1, 3><<<dgrid, threads, 0, st>>>(at); break;
    case AK_DEC2_2_3: attn_decode2_kernel<2, 3><<<dgrid, threads, 0, st>>>(at); break;
    case AK_DEC2_4_3: attn_decode2_kernel<4, 3><<<dgrid, threads, 0, st>>>(at); break;
    case AK_DEC2_8_3: attn_decode2_kernel<8, 3><<<dgrid, threads, 0, st>>>(at); break;
    case AK_CASC: attn_cascade_kernel<4, 2, 3, 1><<<wgs, threads, 0, st>>>(at); break;
    case AK_CASC_442: attn_cascade_kernel<4, 4, 2, 2><<<wgs, threads, 0, st>>>(at); break;
    case AK_CASC_222: attn_cascade_kernel<2, 2, 2, 2><<<wgs, threads, 0, st>>>(at); break;
    case AK_CASC_42: attn_cascade_kernel<4, 2, 2, 1><<<wgs, threads, 0, st>>>(at); break;
    case AK_CASC_44: attn_cascade_kernel<4, 4, 2, 1><<<wgs, threads, 0, st>>>(at); break;
    case AK_CASC_84: attn_cascade_kernel<8, 4, 2, 1><<<wgs, threads, 0, st>>>(at); break;
    case AK_CASC_22: attn_cascade_kernel<2, 2, 2, 1><<<wgs, threads, 0, st>>>(at); break;
  }
}

// The one attention launch site of the library: kernel `kernel` (-1: choose_attn's choice) on BH (sequence, head) pairs,
// then the combine kernel when the keys are split.  bytes / flops: the profiler's figures for the attention launch.
// Returns the kernel launched, or -1 when attn_valid does not admit it (nothing launched, the entry point reports it).
int launch_attention(hipStream_t st, const AttnArgs &at, int BH, int cascade, int kernel, double bytes, double flops,
                     std::string *label) {
  const int k = kernel >= 0 ? kernel : choose_attn(at, BH, cascade);
  if (!attn_valid(k, at)) {
    note_launch_err(std::string("no attention kernel ") + (k >= 0 && k < kNumAttn ? kAttn[k].name : std::to_string(k)) + " for Tq " +
                    std::to_string(at.Tq) + ", ring " + std::to_string(at.ring) + ", splits " + std::to_string(at.splits) + " (site " + launch_site() + ")");
    return -1;
  }
  launch_attn_kernel(st, at, BH, k, bytes, flops, label);
  if (at.splits > 1) {
    ProfScope ps(st, "attn_combine", (double)BH * at.QB * at.splits * 16 * ATT_PSTRIDE * 4, 0);
    attn_combine_kernel<<<dim3(BH, at.QB), 256, 0, st>>>(at);
  }
  return k;
}

// ------------------------------------------------------------------------------------------------
// Reduced-precision codec (ptts_bf16.h): tile choice is static (the kernels are bandwidth / launch bound: bf16 MFMA
// runs at 16x the fp32 rate) - the largest workgroup tile that still yields >= ~2 workgroups per CU.
template <int TN, int TM, int WN, int WM>
static void launch_h_cfg(hipStream_t st, const GemmArgs &a, int pre) {
  const dim3 grid(cdiv(a.NT, TN * WN), cdiv(a.MT, TM * WM)), block(64 * WN * WM);
  const unsigned dyn = lds_pad(0);  // occupancy cap of the codec stream (the kernel itself uses no LDS)
  if (pre == PRE_LNFOLD) gemm_h_kernel<TN, TM, WN, WM, PRE_LNFOLD><<<grid, block, dyn, st>>>(a);
  else gemm_h_kernel<TN, TM, WN, WM, PRE_NONE><<<grid, block, dyn, st>>>(a);
}
// The production tile of a bf16 codec GEMM: index into kTileH
static const int kTileH[4][4] = {{2, 4, 2, 2}, {2, 2, 2, 2}, {1, 2, 2, 2}, {1, 1, 2, 2}};
int choose_h_tile(const GemmArgs &a) {
  int pick = 3;
  for (int i = 0; i < 4; ++i) {
    const int *t = kTileH[i];
    if (t[0] * t[2] > 2 * a.NT && i < 3) continue;  // mostly padding
    if ((long)cdiv(a.NT, t[0] * t[2]) * cdiv(a.MT, t[1] * t[3]) >= 512 || i == 3) { pick = i; break; }
  }
  return pick;
}
// Launches tile `cfg` of gemm_h_kernel on operands a (W, CF, KF, ln_s set), bracketed by the profiler under its label;
// `label` != null receives it
void launch_h_tile(hipStream_t st, const GemmArgs &a, int pre, int cfg, std::string *label) {
  const double K = (double)a.KF * 32, N = (double)a.NT * 16, M = (double)a.M;
  double bytes = 2.0 * (N * K + M * (double)a.CF * 32 + M * N * (a.Yraw ? 2 : 1)) + (a.epi == EPI_RES ? 2.0 * M * N : 0.0);
  if (a.epi == EPI_QKV) bytes += 2.0 * M * N;  // q / k / v leave as fp32
  static const char *const names[4] = {"gemm_h<2,4,2,2>", "gemm_h<2,2,2,2>", "gemm_h<1,2,2,2>", "gemm_h<1,1,2,2>"};
  const int *t = kTileH[cfg];
  const std::string name = std::string(names[cfg]) + (pre == PRE_LNFOLD ? "+ln" : "") + "@" +
                           std::to_string((long)cdiv(a.NT, t[0] * t[2]) * cdiv(a.MT, t[1] * t[3]) * 256);
  if (label) *label = name;
  ProfScope ps(st, name, bytes, 2.0 * M * N * K);
  switch (cfg) {
    case 0: launch_h_cfg<2, 4, 2, 2>(st, a, pre); break;
    case 1: launch_h_cfg<2, 2, 2, 2>(st, a, pre); break;
    case 2: launch_h_cfg<1, 2, 2, 2>(st, a, pre); break;
    default: launch_h_cfg<1, 1, 2, 2>(st, a, pre); break;
  }
}
GemmArgs gemm_h_args(const GemmArgs &a_in, int pre, const Lin &L) {
  GemmArgs a = a_in;
  a.W = (const float *)L.wh;
  a.CF = L.C / 32;
  a.KF = a.CF * L.ntaps;
  if (pre == PRE_LNFOLD) a.ln_s = L.ln_s_h;
  a.swz = 0;
  return a;
}
void launch_gemm_h(hipStream_t st, const GemmArgs &a_in, int pre, const Lin &L) {
  const GemmArgs a = gemm_h_args(a_in, pre, L);
  launch_h_tile(st, a, pre, choose_h_tile(a));
}
// fp8 conv tile `cfg` (ptts_fp8.hip) on operands g, bracketed by the profiler under its label (one label for every tile)
void launch_f8_tile(hipStream_t st, const GemmArgs &g, int cfg, std::string *label) {
  const double K = (double)g.KF * 32, N = (double)g.NT * 16, M = (double)g.M;
  const std::string name = "gemm_f8@" + std::to_string((long)g.NT * g.MT);
  if (label) *label = name;
  ProfScope ps(st, name, N * K + M * g.CF * 32.0 + M * N * (g.yf8 ? 1 : 2) + (g.Yraw ? 2.0 * M * N : 0.0) + (g.epi == EPI_RES ? 2.0 * M * N : 0.0),
               2.0 * M * N * K);
  launch_gemm_f8(st, g, cfg, lds_pad(0));
}

// ------------------------------------------------------------------------------------------------
// The tuner's table through the C ABI (ptts_tune* that run steps on states: ptts.hip)
extern "C" int ptts_tune_version(void) { return kTuneVersion; }
extern "C" const char *ptts_tune_log(ptts_engine *e) { return e ? e->tuner->log.c_str() : ""; }

// The tuned table as text, one line per shape: the 13 key integers (tune_key) then the configuration index.
extern "C" int64_t ptts_tune_export(ptts_engine *e, char *h_out, int64_t capacity) {
  if (!e) return fail(-1, "null engine");
  ENGINE_LOCK(e);
  std::string out;
  char line[256];
  for (auto &kv : e->tuner->table) {
    int n = 0;
    for (int v : kv.first) n += snprintf(line + n, sizeof line - n, "%d ", v);
    snprintf(line + n, sizeof line - n, "%d\n", kv.second);
    out += line;
  }
  if ((int64_t)out.size() + 1 > capacity) return fail(-1, "tune_export: buffer too small");
  memcpy(h_out, out.c_str(), out.size() + 1);
  return (int64_t)out.size();
}

extern "C" int ptts_tune_import(ptts_engine *e, const char *text) {
  if (!e || !text) return fail(-1, "null argument");
  ENGINE_LOCK(e);
  const char *p = text;
  int n_ok = 0;
  while (*p) {
    TuneKey k;
    int cfg = -1, consumed = 0, ok = 1;
    for (int i = 0; i < 13 && ok; ++i) {
      if (sscanf(p, "%d%n", &k[i], &consumed) != 1) ok = 0;
      else p += consumed;
    }
    if (ok && sscanf(p, "%d%n", &cfg, &consumed) == 1) {
      p += consumed;
      if (cfg >= 0 && cfg < kNumCfg) { e->tuner->table[k] = cfg; ++n_ok; }
    } else {
      ok = 0;
    }
    while (*p && *p != '\n') ++p;
    if (*p) ++p;
    if (!ok && !*p) break;
  }
  return n_ok;
}

extern "C" void ptts_tune_clear(ptts_engine *e) {
  if (e) { e->tuner->table.clear(); e->tuner->log.clear(); }
}
