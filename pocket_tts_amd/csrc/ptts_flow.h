// The flow MLP of one FlowLM step as ONE launch (reference mlp.py:188-215 inside the LSD loop of flow_lm.py:19-40).
//
// The chain  input_proj -> depth x [AdaLN-LN -> Linear -> SiLU -> Linear -> gate + residual] -> final layer -> Euler
// is 2 * depth + 2 dependent GEMMs on 512-wide rows: 1 MB of weights and a few hundred kFLOP per row tile each, i.e.
// nothing but dependent-launch latency when every GEMM is its own kernel (16 launches, 193 us per step at batch 64).
// Here a CLUSTER of FDF = flow_dim / 16 workgroups owns RT row tiles (16 rows each) for the whole chain; workgroup j
// owns output columns 16 j .. 16 j + 15 of every layer.  Rows are independent, so clusters never talk to each other
// and a batch is covered by ceil(MT / RT) clusters (batch 64: 4 clusters x 32 workgroups = 128 CUs, the rest of the
// chip stays free for the codec stream).  Between two layers the cluster exchanges the layer output (RT x 512 floats)
// through L2: every workgroup publishes its 16 columns as ONE 1 KiB fragment per row tile - lane for lane the MFMA
// operand fragment kf = j of the next layer (FM layout, see ptts_kernels.h) - with write-through (`sc1`) stores, drains
// them and raises a flag; consumers poll the flags of their cluster and read the fragments with `sc1` loads
// (MI355X_MICROARCH.md, "Valid forms": every payload byte stored sc1 and drained before the flag, every load of it a
// buffer_load sc1 behind the matched poll and a workgroup barrier).  Every (phase, producer) has its own slot and flag,
// so nothing is overwritten inside a launch; the flag value carries the state's step counter, so a replayed graph
// needs no memset node and stale flags of earlier steps never match.
//
// Workgroup = 1 coordinator wave + 8 worker waves.  Workers split K eight ways: each loads its k-fragments of the
// operand (and of the AdaLN shift / scale), the LayerNorm statistics meet in LDS, the partial accumulators too.  The
// coordinator polls, sums the partials, runs the epilogue, publishes and holds the residual stream tile in registers;
// it issues no weight loads, so its polls and drains never queue behind an HBM miss.  Workers fetch the NEXT phase's
// weight fragments right after handing over their partials: the 32 KB a workgroup needs per layer are in flight
// while the hand-off completes.
#pragma once
#include "ptts_kernels.h"

#define FLOW_MAX_DEPTH 12
#define FLOW_WORKERS 8
#define FLOW_THREADS (64 * (FLOW_WORKERS + 1))
#define FLOW_SPIN_LIMIT 400000u  // ~0.1-0.3 s per phase before a workgroup gives up (never reached when all blocks run)

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

struct FlowArgs {
  int MT, M, NG, NCL, FDF, LF, AF, depth, steps, ldim;  // NG row groups of RT tiles, served by NCL resident clusters
  const float *w_in, *b_in;  // input_proj, packed [FDF][LF][64][4]
  const float *w_l0[FLOW_MAX_DEPTH], *b_l0[FLOW_MAX_DEPTH], *w_l2[FLOW_MAX_DEPTH], *b_l2[FLOW_MAX_DEPTH];
  const float *ln_w[FLOW_MAX_DEPTH], *ln_b[FLOW_MAX_DEPTH];
  const float *w_fin, *b_fin;  // final linear, packed [LF][FDF][64][4]
  const float *mod;            // AdaLN modulations of every LSD step, FM [steps][MT][AF]
  long mod_step;               // floats per LSD step in `mod`
  const float *latfm;          // FM [MT][LF]: start point of the LSD integration (noise), written by prep_lm_kernel
  float *lat, *lat_out1, *lat_out2;  // plain [M][ldim] outputs (state copy, next step's input, caller's buffer)
  float inv_steps;
  float *exch;         // [NG][steps * (2 depth + 2)][RT][FDF][256]
  u64 *flags;          // [NG][steps * (2 depth + 2)][FDF]
  const int *ctr;      // the state's step counter (incremented by step_tail_kernel after this launch)
  int *err;            // set to 1 when a poll gave up
  // per-row LSD schedules (flow_cluster_kernel<.., true>): row m runs row_lsd_n(row_n, row_ndef, m) <= steps Euler steps
  const int *row_n;
  int row_ndef;
  // flow_cluster_mod_kernel only: the modulations are computed inside the launch from the conditioning `ce` (FM [MT][FDF])
  const float *ce, *w_mod, *b_mod;  // AdaLN linear, packed [AF][FDF][64][4], and its bias
  const float *tcomb;               // time embeddings of the LSD steps [steps][flow_dim], added before the SiLU
  int ce_silu;                      // 1: `ce` already holds silu(ce + tcomb[0]) (the head's epilogue, lsd_steps 1)
};

// Exchange layout, in floats from the start of the buffer: every (row group, phase, row tile, producer) owns one slot of
// `nf` fragments of 256 floats.  nf = 1: the layer output (flow_cluster_kernel); nf = FLOW_MOD_FRAGS: layer output, then
// the AdaLN shift and scale fragments the next phase's LayerNorm consumes (flow_cluster_mod_kernel).
#define FLOW_MOD_FRAGS 3
__host__ __device__ inline size_t flow_slot(int FDF, int RT, int NPH, int nf, int grp, int p, int t, int j, int f) {
  return ((((((size_t)grp * NPH + p) * RT + t) * FDF + j) * nf) + f) * 256;
}

// flow_cluster_mod_kernel: the modulation column tiles workgroup j computes at the top of phase ph (0 .. 2 depth + 1) of an
// LSD step: *n of them (0 .. 2), the first at the returned tile of the AdaLN output, the second FDF tiles later.  The
// AdaLN output is [block 0: shift | scale | gate] .. [block depth - 1: ..] [final layer: shift | scale], FDF tiles each.
//   phase 0 (input_proj): shift, scale of block 0;  linear 0 of block r: gate of block r;
//   linear 2 of block r: shift, scale of block r + 1, or of the final layer;  final layer: none
__host__ __device__ inline int flow_mod_tiles(int FDF, int depth, int ph, int j, int *n) {
  const int r = (ph - 1) >> 1;
  if (ph == 0) { *n = 2; return j; }
  if (ph == 2 * depth + 1) { *n = 0; return 0; }
  if ((ph - 1) & 1) { *n = 2; return (r + 1) * 3 * FDF + j; }
  *n = 1;
  return r * 3 * FDF + 2 * FDF + j;
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t flow_rsrc(const void *p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, 0x7ffffff0, 0x00020000);
}
__device__ __forceinline__ f32x4 flow_ld_sc1(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)byte_off, 0, 16));  // aux 16 = sc1
}
__device__ __forceinline__ void flow_st_sc1(__amdgpu_buffer_rsrc_t r, unsigned byte_off, f32x4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, (int)byte_off, 0, 16);
}

// 16 bytes per lane at a wave-uniform address + the lane's byte offset, as buffer loads / stores: the address takes no vector
// registers, and nothing per-lane is left for the compiler to hoist out of the phase loop (flow_cluster_mod_kernel: with
// plain pointers it kept some forty 64-bit addresses alive around the loop and spilled them)
__device__ __forceinline__ f32x4 flow_ldu(const void *base, unsigned voff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(flow_rsrc(base), (int)voff, 0, 0));
}
__device__ __forceinline__ f32x4 flow_ldu_sc1(__amdgpu_buffer_rsrc_t r, unsigned soff, unsigned voff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 16));
}
__device__ __forceinline__ void flow_stu_sc1(__amdgpu_buffer_rsrc_t r, unsigned soff, unsigned voff, f32x4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, (int)voff, (int)soff, 16);
}

// one wave polls the flags of `np` producers (np <= 64) until all carry `epoch`; bounded
__device__ __forceinline__ bool flow_wait(const u64 *f, int np, u64 epoch, int lane, int *err) {
  for (unsigned spins = 0;; ++spins) {
    const u64 v = lane < np ? __hip_atomic_load(f + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : epoch;
    if (__all(v == epoch)) return true;
    if (spins > FLOW_SPIN_LIMIT) {
      if (lane == 0) atomicExch(err, 1);
      return false;
    }
    __builtin_amdgcn_s_sleep(2);
  }
}

// RT = row tiles per cluster (the host uses 1: one cluster per 16 rows keeps the worker waves within the 168
// registers a 9-wave workgroup leaves per lane), KPW = k-fragments per worker wave (>= ceil(max(FDF, LF) / 8)).
// ROWLSD: per-row schedules.  `steps` is then the capacity the slots are laid out for; a row group runs the phases of
// max n over its rows (every workgroup reads the same words, written before the launch), each row's Euler update uses
// its own 1 / n, a row past its count is frozen and writes its outputs at its own last step.  Phases past a group's
// bound never run, so their flags and slots are simply not touched.
template <int RT, int KPW, bool ROWLSD = false>
__global__ __launch_bounds__(FLOW_THREADS) void flow_cluster_kernel(FlowArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int FDF = a.FDF, LF = a.LF;
  // workgroups with the same column tile j (they stream the SAME weight tiles) sit 8 apart in blockIdx, i.e. on one XCD
  // under round-robin placement (speed only): the clusters' weight re-reads are then L2 hits instead of fabric reads
  const int cl = blockIdx.x / a.FDF, j = blockIdx.x % a.FDF;  // resident cluster, column tile
  const bool coord = wave == FLOW_WORKERS;
  const int PPS = 2 * a.depth + 2, NPH = a.steps * PPS;
  __shared__ f32x4 red[FLOW_WORKERS][RT][64];
  __shared__ float st[FLOW_WORKERS][RT][16][2];
  const u64 ebase = ((u64)(unsigned)(*a.ctr) + 1ull) << 16;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  bool dead = false;  // coordinator only: a poll gave up; finish without waiting (outputs are garbage, *err is set)
  // a resident cluster serves row groups cl, cl + NCL, ..: at most NCL * FDF workgroups wait for each other, however
  // large the batch is (a 9-wave workgroup of this kernel fills a CU: residency is one workgroup per CU)
  for (int grp = cl; grp < a.NG; grp += a.NCL) {
  const int mt0 = grp * RT;
  float *ex = a.exch + (size_t)grp * NPH * RT * FDF * 256;
  u64 *fl = a.flags + (size_t)grp * NPH * FDF;
  const __amdgpu_buffer_rsrc_t rs = flow_rsrc(ex);
  __syncthreads();  // LDS of the previous group is free

  int mtc[RT];  // clamped row tiles (a partially filled last cluster computes duplicates and stores nothing for them)
#pragma unroll
  for (int t = 0; t < RT; ++t) mtc[t] = min(mt0 + t, a.MT - 1);
  int nph = NPH;  // phases this group runs
  int nrow[RT];   // ROWLSD: LSD steps of this lane's row of each tile
  if constexpr (ROWLSD) {
    int mx = 0;
    const int mg = 16 * mt0 + lane;  // RT * 16 <= 64 rows of the group, one per lane
    if (lane < RT * 16 && mg < a.M) mx = row_lsd_n(a.row_n, a.row_ndef, mg);
#pragma unroll
    for (int o = 32; o; o >>= 1) mx = max(mx, __shfl_xor(mx, o));
    nph = __builtin_amdgcn_readfirstlane(mx) * PPS;  // the same in every lane: a scalar loop bound
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      const int m = 16 * (mt0 + t) + (lane & 15);
      nrow[t] = m < a.M ? row_lsd_n(a.row_n, a.row_ndef, m) : 1;
    }
  }

  // phase p of the launch: kind 0 = input_proj, 1 = block linear 0 (AdaLN-LN on load, SiLU), 2 = block linear 2
  // (gate + residual), 3 = final layer (no-affine LN + modulation on load, Euler update)
  auto kind_of = [&](int ph) { return ph == 0 ? 0 : ph == PPS - 1 ? 3 : 1 + ((ph - 1) & 1); };
  auto wtile = [&](int ph, int &KF, bool &use) -> const float * {
    const int k = kind_of(ph), r = (ph - 1) >> 1;
    use = true;
    if (k == 0) { KF = LF; return a.w_in + (size_t)j * LF * 256; }
    KF = FDF;
    if (k == 1) return a.w_l0[r] + (size_t)j * FDF * 256;
    if (k == 2) return a.w_l2[r] + (size_t)j * FDF * 256;
    use = j < LF;
    return a.w_fin + (size_t)(use ? j : 0) * FDF * 256;
  };
  auto bias_of = [&](int ph) -> const float * {
    const int k = kind_of(ph), r = (ph - 1) >> 1;
    return (k == 0 ? a.b_in : k == 1 ? a.b_l0[r] : k == 2 ? a.b_l2[r] : a.b_fin) + (k == 3 && j >= LF ? 0 : 16 * j) + 4 * (lane >> 4);
  };

  // ---- worker state: weight fragments of the current phase
  f32x4 w[KPW];
  auto load_w = [&](int ph) {
    int KF;
    bool use;
    const float *Wt = wtile(ph, KF, use);
#pragma unroll
    for (int u = 0; u < KPW; ++u) {
      const int kf = wave * KPW + u;
      // plain loads: the clusters of a batch read the same tiles, L2 / Infinity Cache serve the re-reads
      const f32x4 v = *(const f32x4 *)(Wt + (size_t)min(kf, KF - 1) * 256 + lane * 4);
      w[u] = (use && kf < KF) ? v : zero4;
    }
  };
  // ---- coordinator state: residual stream tile, latent tile, epilogue operands of the current and the next phase
  f32x4 xres[RT], latv[RT], e_bias = zero4, e_gate[RT], n_bias = zero4, n_gate[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) xres[t] = latv[t] = e_gate[t] = n_gate[t] = zero4;
  auto load_epi = [&](int p, f32x4 &bias, f32x4 *gate) {  // bias (+ gate tiles) of phase p
    const int i = p / PPS, ph = p - i * PPS;
    bias = *(const f32x4 *)bias_of(ph);
    if (kind_of(ph) == 2) {
      const int r = (ph - 1) >> 1;
#pragma unroll
      for (int t = 0; t < RT; ++t)
        gate[t] = *(const f32x4 *)(a.mod + (size_t)i * a.mod_step + (((size_t)mtc[t] * a.AF + r * 3 * FDF + 2 * FDF + j) * 64 + lane) * 4);
    }
  };
  if (coord) {
    load_epi(0, e_bias, e_gate);
    if (j < LF) {
#pragma unroll
      for (int t = 0; t < RT; ++t) latv[t] = *(const f32x4 *)(a.latfm + (((size_t)mtc[t] * LF + j) * 64 + lane) * 4);
    }
  } else {
    load_w(0);
  }

  for (int p = 0; p < nph; ++p) {
    const int i = p / PPS, ph = p - i * PPS;
    const int kind = kind_of(ph);
    const int KF = kind == 0 ? LF : FDF;
    const bool lnmod = kind == 1 || kind == 3;
    // ---- A: the inputs of phase p are published (slot p - 1)
    if (coord && p > 0 && !dead) {
      const int np = ph == 0 ? LF : FDF;
      if (!flow_wait(fl + (size_t)(p - 1) * FDF, np, ebase | (u64)p, lane, a.err)) dead = true;
    }
    __syncthreads();
    f32x4 x[RT][KPW], ma[RT][KPW], mb[RT][KPW];  // operand fragments; modulation as x' = LN0(x) * ma + mb
    const int r = (ph - 1) >> 1;
    if (!coord) {
      if (p == 0) {
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
          for (int u = 0; u < KPW; ++u) {
            const int kf = wave * KPW + u;
            const f32x4 v = *(const f32x4 *)(a.latfm + (((size_t)mtc[t] * LF + min(kf, KF - 1)) * 64 + lane) * 4);
            x[t][u] = kf < KF ? v : zero4;
          }
      } else {
        const unsigned sbase = (unsigned)(p - 1) * RT * FDF * 1024u;
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
          for (int u = 0; u < KPW; ++u) {
            const int kf = wave * KPW + u;
            const f32x4 v = flow_ld_sc1(rs, sbase + ((unsigned)(t * FDF + min(kf, KF - 1)) * 64u + lane) * 16u);
            x[t][u] = kf < KF ? v : zero4;
          }
      }
      if (lnmod) {
        // AdaLN-modulated LayerNorm on load (reference mlp.py:107-109, 127-129): statistics over the whole row
        const float *mbase = a.mod + (size_t)i * a.mod_step;
        const int sh0 = kind == 1 ? r * 3 * FDF : a.depth * 3 * FDF;
#pragma unroll
        for (int u = 0; u < KPW; ++u) {
          const int kf = min(wave * KPW + u, KF - 1);
          f32x4 lw = {1.f, 1.f, 1.f, 1.f}, lb = zero4;
          if (kind == 1) {
            lw = *(const f32x4 *)(a.ln_w[r] + 16 * kf + 4 * (lane >> 4));
            lb = *(const f32x4 *)(a.ln_b[r] + 16 * kf + 4 * (lane >> 4));
          }
#pragma unroll
          for (int t = 0; t < RT; ++t) {
            const float *mp = mbase + (((size_t)mtc[t] * a.AF + sh0 + kf) * 64 + lane) * 4;
            const f32x4 shv = *(const f32x4 *)mp, scv = 1.0f + *(const f32x4 *)(mp + (size_t)FDF * 256);
            // (n * w + b) * (1 + scale) + shift  ==  n * [w (1 + scale)] + [b (1 + scale) + shift]
            ma[t][u] = lw * scv;
            mb[t][u] = lb * scv + shv;
          }
        }
#pragma unroll
        for (int t = 0; t < RT; ++t) {
          float s1 = 0.f, s2 = 0.f;
#pragma unroll
          for (int u = 0; u < KPW; ++u) {
            const f32x4 v = x[t][u];
            s1 += (v.x + v.y) + (v.z + v.w);
            s2 += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
          }
          s1 += __shfl_xor(s1, 16); s1 += __shfl_xor(s1, 32);
          s2 += __shfl_xor(s2, 16); s2 += __shfl_xor(s2, 32);
          if (lane < 16) { st[wave][t][lane][0] = s1; st[wave][t][lane][1] = s2; }
        }
      }
    } else if (p + 1 < nph) {
      load_epi(p + 1, n_bias, n_gate);  // lands while the workers compute
    }
    if (lnmod) __syncthreads();  // B: row statistics of all workers are in LDS
    if (!coord) {
      if (lnmod) {
        const float invK = 1.0f / (float)(KF * 16);
#pragma unroll
        for (int t = 0; t < RT; ++t) {
          float t0 = 0.f, t1 = 0.f;
#pragma unroll
          for (int q = 0; q < FLOW_WORKERS; ++q) { t0 += st[q][t][lane & 15][0]; t1 += st[q][t][lane & 15][1]; }
          const float mu = t0 * invK;
          const float rsd = 1.0f / sqrtf(fmaxf(t1 * invK - mu * mu, 0.f) + 1e-6f);  // flow-MLP LayerNorm eps (mlp.py:95)
#pragma unroll
          for (int u = 0; u < KPW; ++u) {
            const f32x4 v = ((x[t][u] - mu) * rsd) * ma[t][u] + mb[t][u];
            x[t][u] = (wave * KPW + u) < KF ? v : zero4;
          }
        }
      }
      f32x4 acc[RT];
#pragma unroll
      for (int t = 0; t < RT; ++t) acc[t] = zero4;
#pragma unroll
      for (int u = 0; u < KPW; ++u)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int t = 0; t < RT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[u][c], x[t][u][c], acc[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < RT; ++t) red[wave][t][lane] = acc[t];
    }
    __syncthreads();  // C: partial accumulators are in LDS
    if (!coord) {
      if (p + 1 < nph) load_w((p + 1) % PPS);  // in flight while the hand-off completes
      continue;
    }
    // ---- coordinator: reduce (fixed order), epilogue, publish
    const bool last_step = i == a.steps - 1;
    const bool publish = p + 1 < nph && (kind != 3 || j < LF);
#pragma unroll
    for (int t = 0; t < RT; ++t) {
      f32x4 s = red[0][t][lane];
#pragma unroll
      for (int q = 1; q < FLOW_WORKERS; ++q) s += red[q][t][lane];
      s += e_bias;
      f32x4 out;
      if (kind == 0) { xres[t] = s; out = s; }
      else if (kind == 1) out = act4(s, ACT_SILU);
      else if (kind == 2) { xres[t] = xres[t] + e_gate[t] * s; out = xres[t]; }
      else {
        // Euler update of lsd_decode: current += flow_dir / num_steps (reference flow_lm.py:39)
        bool last = last_step;
        if constexpr (ROWLSD) {
          if (i < nrow[t]) latv[t] = latv[t] + s * (1.0f / (float)nrow[t]);
          last = i == nrow[t] - 1;
        } else {
          latv[t] = latv[t] + s * a.inv_steps;
        }
        out = latv[t];
        const int m = 16 * (mt0 + t) + (lane & 15);
        if (last && j < LF && mt0 + t < a.MT && m < a.M) {
          const size_t o = (size_t)m * a.ldim + 16 * j + 4 * (lane >> 4);
          *(f32x4 *)(a.lat + o) = out;
          if (a.lat_out1) *(f32x4 *)(a.lat_out1 + o) = out;
          if (a.lat_out2) *(f32x4 *)(a.lat_out2 + o) = out;
        }
      }
      if (publish) flow_st_sc1(rs, ((unsigned)((p * RT + t) * FDF + j) * 64u + lane) * 16u, out);
    }
    if (publish) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the write-through stores have left the CU
      if (lane == 0) __hip_atomic_store(fl + (size_t)p * FDF + j, ebase | (u64)(p + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    e_bias = n_bias;
#pragma unroll
    for (int t = 0; t < RT; ++t) e_gate[t] = n_gate[t];
  }
  }  // row groups
}

// The same chain with the AdaLN modulation GEMM (mod = Linear(silu(ce + t_emb)), reference mlp.py:107,127,210) folded
// into the hand-off waits: no `mod` buffer, no launch in front of the cluster.  Same geometry, flags, epochs, spin limit
// and error word as flow_cluster_kernel<1, KPW>; one row tile per cluster, one schedule for all rows.
//
// Workgroup j owns column tile j of each of the 3 depth + 2 modulation vectors (tile r 3 FDF + j = shift of block r,
// + FDF = scale, + 2 FDF = gate; depth 3 FDF + j and + FDF = the final layer's shift and scale).  A tile is a K = flow_dim
// product like a layer's, split over the workers the same way; its operand silu(ce + t_emb) stays on chip (LDS).  Workers
// compute, at the top of phase p and before the barrier behind the coordinator's poll (i.e. while they would wait):
//   kind 0 (input_proj): shift and scale of block 0          -> published with slot p, read by phase p + 1
//   kind 1 (linear 0 of block r): gate of block r            -> stays in the coordinator's registers for phase p + 1
//   kind 2 (linear 2 of block r): shift and scale of the next LayerNorm (block r + 1 or the final layer) -> slot p
// Their weight fragments are requested with load_w of the phase before.  The coordinator sums the partials in fixed
// order, adds the bias and issues the write-through stores of shift and scale BEFORE it waits for the layer partials;
// the one flag per (phase, producer) is raised behind `s_waitcnt vmcnt(0)` over all three fragments of the slot.
template <int KPW>
__global__ __launch_bounds__(FLOW_THREADS) void flow_cluster_mod_kernel(FlowArgs a) {
  // the wave index as a scalar: the coordinator / worker branches are then uniform branches, and the registers of one
  // role are not kept alive through the code of the other
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int FDF = a.FDF, LF = a.LF;
  const int cl = blockIdx.x / a.FDF, j = blockIdx.x % a.FDF;  // resident cluster, column tile (see flow_cluster_kernel)
  const bool coord = wave == FLOW_WORKERS;
  const int PPS = 2 * a.depth + 2, NPH = a.steps * PPS;
  __shared__ f32x4 red[FLOW_WORKERS][64];
  __shared__ f32x4 mred[FLOW_WORKERS][2][64];  // partial sums of the phase's modulation tiles
  // the modulation operand silu(ce + t_emb) of the row group, each worker's own k-fragments: written and read by that
  // wave only; in LDS, not in registers: the LayerNorm part of a KPW = 4 phase has none to spare
  __shared__ f32x4 cxs[FLOW_WORKERS][KPW][64];
  __shared__ float st[FLOW_WORKERS][16][2];
  const u64 ebase = ((u64)(unsigned)(*a.ctr) + 1ull) << 16;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  bool dead = false;
  // byte offset of fragment f of producer q's slot of phase p inside the row group's part of the exchange (a scalar)
  auto slot = [&](int p, int q, int f) { return (unsigned)flow_slot(FDF, 1, NPH, FLOW_MOD_FRAGS, 0, p, 0, q, f) * 4u; };
  const unsigned l16 = (unsigned)lane * 16u, q16 = (unsigned)(lane >> 4) * 16u;  // a lane's bytes in a fragment / in 16 columns
  for (int grp = cl; grp < a.NG; grp += a.NCL) {
  float *ex = a.exch + flow_slot(FDF, 1, NPH, FLOW_MOD_FRAGS, grp, 0, 0, 0, 0);
  u64 *fl = a.flags + (size_t)grp * NPH * FDF;
  const __amdgpu_buffer_rsrc_t rs = flow_rsrc(ex);
  __syncthreads();  // LDS of the previous group is free
  const int mtc = min(grp, a.MT - 1);
  const int nph = NPH;

  auto kind_of = [&](int ph) { return ph == 0 ? 0 : ph == PPS - 1 ? 3 : 1 + ((ph - 1) & 1); };
  auto wtile = [&](int ph, int &KF, bool &use) -> const float * {
    const int k = kind_of(ph), r = (ph - 1) >> 1;
    use = true;
    if (k == 0) { KF = LF; return a.w_in + (size_t)j * LF * 256; }
    KF = FDF;
    if (k == 1) return a.w_l0[r] + (size_t)j * FDF * 256;
    if (k == 2) return a.w_l2[r] + (size_t)j * FDF * 256;
    use = j < LF;
    return a.w_fin + (size_t)(use ? j : 0) * FDF * 256;
  };
  auto bias_of = [&](int ph) -> const float * {
    const int k = kind_of(ph), r = (ph - 1) >> 1;
    return (k == 0 ? a.b_in : k == 1 ? a.b_l0[r] : k == 2 ? a.b_l2[r] : a.b_fin) + (k == 3 && j >= LF ? 0 : 16 * j);
  };
  // modulation tiles of phase ph: n of them, the first at the returned column tile, the second FDF tiles later
  auto mtiles = [&](int ph, int &n) { return flow_mod_tiles(FDF, a.depth, ph, j, &n); };

  // ---- worker state: weight fragments of the current phase and of its modulation tiles
  f32x4 w[KPW], mw[2][KPW];
  auto load_w = [&](int ph) {
    int n;
    const int t0 = mtiles(ph, n);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int u = 0; u < KPW; ++u) mw[s][u] = zero4;  // (assigned on every path: nothing is carried from phase to phase)
      if (s < n) {  // the same in every lane
#pragma unroll
        for (int u = 0; u < KPW; ++u) {
          const int kf = wave * KPW + u;
          const f32x4 v = flow_ldu(a.w_mod + ((size_t)(t0 + s * FDF) * FDF + min(kf, FDF - 1)) * 256, l16);
          if (kf < FDF) mw[s][u] = v;
        }
      }
    }
    int KF;
    bool use;
    const float *Wt = wtile(ph, KF, use);
#pragma unroll
    for (int u = 0; u < KPW; ++u) {
      const int kf = wave * KPW + u;
      const f32x4 v = flow_ldu(Wt + (size_t)min(kf, KF - 1) * 256, l16);
      w[u] = (use && kf < KF) ? v : zero4;
    }
  };
  // The two roles run their own copy of the phase loop, each with the phase's barriers A, (B,) C in it: the branch is
  // uniform per wave and all nine waves meet every barrier, but no register of one role is live in the other's code.
  if (coord) {
    // ---- coordinator state: residual stream tile, latent tile, the gate of the next epilogue (the biases are requested
    // in front of the poll, phase by phase)
    f32x4 xres = zero4, latv = zero4, e_gate = zero4;
    if (j < LF) latv = flow_ldu(a.latfm + ((size_t)mtc * LF + j) * 256, l16);
    for (int p = 0; p < nph; ++p) {
      const int i = p / PPS, ph = p - i * PPS;
      const int kind = kind_of(ph);
      const bool lnmod = kind == 1 || kind == 3;
      int nmt;
      const int t0 = mtiles(ph, nmt);
      // ---- A: the inputs of phase p are published (slot p - 1)
      const f32x4 e_bias = flow_ldu(bias_of(ph), q16);
      f32x4 mbias[2] = {zero4, zero4};  // biases of the phase's modulation tiles
#pragma unroll
      for (int s = 0; s < 2; ++s)
        if (s < nmt) mbias[s] = flow_ldu(a.b_mod + 16 * (t0 + s * FDF), q16);
      if (p > 0 && !dead) {
        const int np = ph == 0 ? LF : FDF;
        if (!flow_wait(fl + (size_t)(p - 1) * FDF, np, ebase | (u64)p, lane, a.err)) dead = true;
      }
      __syncthreads();
      // the phase's modulation tiles: fixed-order sum + bias; shift and scale leave before the layer partials are waited for
      if (nmt > 0) {
        auto msum = [&](int s) {
          f32x4 m = mred[0][s][lane];
#pragma unroll
          for (int q = 1; q < FLOW_WORKERS; ++q) m += mred[q][s][lane];
          return m + mbias[s];
        };
        const f32x4 m0 = msum(0);
        if (nmt == 2) {
          flow_stu_sc1(rs, slot(p, j, 1), l16, m0);
          flow_stu_sc1(rs, slot(p, j, 2), l16, msum(1));
        } else {
          e_gate = m0;  // the gate of this block: the next phase's epilogue (this phase's has none)
        }
      }
      if (lnmod) __syncthreads();  // B
      __syncthreads();             // C: partial accumulators are in LDS
      // ---- reduce (fixed order), epilogue, publish
      const bool publish = p + 1 < nph && (kind != 3 || j < LF);
      f32x4 s = red[0][lane];
#pragma unroll
      for (int q = 1; q < FLOW_WORKERS; ++q) s += red[q][lane];
      s += e_bias;
      f32x4 out;
      if (kind == 0) { xres = s; out = s; }
      else if (kind == 1) out = act4(s, ACT_SILU);
      else if (kind == 2) { xres = xres + e_gate * s; out = xres; }
      else {
        latv = latv + s * a.inv_steps;  // Euler update of lsd_decode (reference flow_lm.py:39)
        out = latv;
        const int m = 16 * grp + (lane & 15);
        if (i == a.steps - 1 && j < LF && m < a.M) {
          const size_t o = (size_t)m * a.ldim + 16 * j + 4 * (lane >> 4);
          *(f32x4 *)(a.lat + o) = out;
          if (a.lat_out1) *(f32x4 *)(a.lat_out1 + o) = out;
          if (a.lat_out2) *(f32x4 *)(a.lat_out2 + o) = out;
        }
      }
      if (publish) {
        flow_stu_sc1(rs, slot(p, j, 0), l16, out);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // all three fragments of the slot have left the CU
        if (lane == 0) __hip_atomic_store(fl + (size_t)p * FDF + j, ebase | (u64)(p + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  } else {
    load_w(0);
    for (int p = 0; p < nph; ++p) {
      const int i = p / PPS, ph = p - i * PPS;
      const int kind = kind_of(ph);
      const int KF = kind == 0 ? LF : FDF;
      const bool lnmod = kind == 1 || kind == 3;
      int nmt;
      mtiles(ph, nmt);
      // ---- in front of A: the wait for the phase's inputs is filled with the modulation tiles
      if (ph == 0) {  // the operand of this LSD step's modulations: silu(ce + t_emb_i), this wave's k-fragments
#pragma unroll
        for (int u = 0; u < KPW; ++u) {
          const int kf = wave * KPW + u, kc = min(kf, FDF - 1);
          f32x4 v = flow_ldu(a.ce + ((size_t)mtc * FDF + kc) * 256, l16);
          if (!a.ce_silu) {
            const f32x4 t = flow_ldu(a.tcomb + (size_t)i * FDF * 16 + 16 * kc, q16);
            v.x = silu_f(v.x + t.x); v.y = silu_f(v.y + t.y); v.z = silu_f(v.z + t.z); v.w = silu_f(v.w + t.w);
          }
          cxs[wave][u][lane] = kf < FDF ? v : zero4;
        }
      }
      if (nmt > 0) {
        f32x4 m0 = zero4, m1 = zero4, cx[KPW];
#pragma unroll
        for (int u = 0; u < KPW; ++u) cx[u] = cxs[wave][u][lane];
#pragma unroll
        for (int u = 0; u < KPW; ++u)
#pragma unroll
          for (int c = 0; c < 4; ++c) m0 = __builtin_amdgcn_mfma_f32_16x16x4f32(mw[0][u][c], cx[u][c], m0, 0, 0, 0);
        mred[wave][0][lane] = m0;
        if (nmt == 2) {
#pragma unroll
          for (int u = 0; u < KPW; ++u)
#pragma unroll
            for (int c = 0; c < 4; ++c) m1 = __builtin_amdgcn_mfma_f32_16x16x4f32(mw[1][u][c], cx[u][c], m1, 0, 0, 0);
          mred[wave][1][lane] = m1;
        }
      }
      __syncthreads();  // A
      f32x4 x[KPW], ma[KPW], mb[KPW];  // operand fragments; modulation as x' = LN0(x) * ma + mb
      const int r = (ph - 1) >> 1;
      if (p == 0) {
#pragma unroll
        for (int u = 0; u < KPW; ++u) {
          const int kf = wave * KPW + u;
          const f32x4 v = flow_ldu(a.latfm + ((size_t)mtc * LF + min(kf, KF - 1)) * 256, l16);
          x[u] = kf < KF ? v : zero4;
        }
      } else {
#pragma unroll
        for (int u = 0; u < KPW; ++u) {
          const int kf = wave * KPW + u;
          const f32x4 v = flow_ldu_sc1(rs, slot(p - 1, min(kf, KF - 1), 0), l16);
          x[u] = kf < KF ? v : zero4;
        }
      }
      if (lnmod) {
        // AdaLN-modulated LayerNorm on load (reference mlp.py:107-109, 127-129): statistics over the whole row; shift
        // and scale fragment kf come from producer kf's slot, behind the same poll as the operand
#pragma unroll
        for (int u = 0; u < KPW; ++u) {
          const int kf = min(wave * KPW + u, KF - 1);
          f32x4 lw = {1.f, 1.f, 1.f, 1.f}, lb = zero4;
          if (kind == 1) {
            lw = flow_ldu(a.ln_w[r] + 16 * kf, q16);
            lb = flow_ldu(a.ln_b[r] + 16 * kf, q16);
          }
          const f32x4 shv = flow_ldu_sc1(rs, slot(p - 1, kf, 1), l16), scv = 1.0f + flow_ldu_sc1(rs, slot(p - 1, kf, 2), l16);
          // (n * w + b) * (1 + scale) + shift  ==  n * [w (1 + scale)] + [b (1 + scale) + shift]
          ma[u] = lw * scv;
          mb[u] = lb * scv + shv;
        }
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int u = 0; u < KPW; ++u) {
          const f32x4 v = x[u];
          s1 += (v.x + v.y) + (v.z + v.w);
          s2 += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
        }
        s1 += __shfl_xor(s1, 16); s1 += __shfl_xor(s1, 32);
        s2 += __shfl_xor(s2, 16); s2 += __shfl_xor(s2, 32);
        if (lane < 16) { st[wave][lane][0] = s1; st[wave][lane][1] = s2; }
      }
      if (lnmod) __syncthreads();  // B: row statistics of all workers are in LDS
      if (lnmod) {
        const float invK = 1.0f / (float)(KF * 16);
        float t0 = 0.f, t1 = 0.f;
#pragma unroll
        for (int q = 0; q < FLOW_WORKERS; ++q) { t0 += st[q][lane & 15][0]; t1 += st[q][lane & 15][1]; }
        const float mu = t0 * invK;
        const float rsd = 1.0f / sqrtf(fmaxf(t1 * invK - mu * mu, 0.f) + 1e-6f);  // flow-MLP LayerNorm eps (mlp.py:95)
#pragma unroll
        for (int u = 0; u < KPW; ++u) {
          const f32x4 v = ((x[u] - mu) * rsd) * ma[u] + mb[u];
          x[u] = (wave * KPW + u) < KF ? v : zero4;
        }
      }
      f32x4 acc = zero4;
#pragma unroll
      for (int u = 0; u < KPW; ++u)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w[u][c], x[u][c], acc, 0, 0, 0);
      red[wave][lane] = acc;
      __syncthreads();  // C: partial accumulators are in LDS
      if (p + 1 < nph) {
        load_w((p + 1) % PPS);  // in flight while the hand-off completes
      } else {  // (assigned on every path: no fragment is carried around the loop, which would pin 48 registers)
#pragma unroll
        for (int u = 0; u < KPW; ++u) w[u] = mw[0][u] = mw[1][u] = zero4;
      }
    }  // phases
  }  // worker
  }  // row groups
}
