// Kernel choice of the grouped GEMM (afx_gemm.hip): which kernel family and tile shape a GemmBatch runs on, as host arithmetic on the batch, the
// settings and the CU count.  No HIP runtime call: plan_gemm() runs without a GPU (tests/gemm_plan_check.hip); launch_gemm() only switches on its result.
#pragma once
#include "afx_kernels.h"

namespace afx {

constexpr int BM = 256, BN = 256, BK = 64;
constexpr int GROUP_M = 6;                              // super-row height of the tile order

// The GEMM's settings (afx_gemm.hip gemm_mode() reads the environment ONCE; the launcher and the predicates below agree on every launch):
//   AFX_GEMM_IMPL       2 = the 8-phase kernel only, 3 (default; any other value) = the one-wave-per-SIMD kernels for the launches they take
//   AFX_GEMM_TILE       (impl 3) 0 = pick per launch, 1 ... 6 = force 256x256 / 288x192 / 320x192 / 128x128 / 256x224 / 224x256
//   AFX_QK_FUSE=0       keep the separate kv_prep launch (A/B)
//   AFX_FP8_V3=0        fp8 launches on the 8-phase kernel (A/B);  AFX_FP8_V3_MIN: fewest 256x256 tiles of a launch for the fp8 v3 kernel;
//   AFX_FP8_TILE        1 / 2 force its 256x256 / 224x256 shape
//   AFX_GEMM_GROUP_M    tile-order super-row height;  AFX_GEMM_PEN224 / AFX_GEMM_PEN_QK224: cost factors of the 256x224 / 224x256 shapes (1e9 = never)
//   AFX_GEMM_PERSIST    1 / 2: launches with more tiles than resident work-groups run the persistent tile walk (grid = CUs x resident work-groups
//                       per CU); off by default -- see DESIGN 4.1 for the same-box A/B
// afx_gemm_set_mode() overrides impl and tile, afx_gemm_set_fp8_tile() fp8_tile (parity tests, A/B runs).
struct GemmMode {
  int impl = 3, tile = 0;
  bool qk_fuse = true, fp8_v3 = true;
  int fp8_v3_min = -1;            // < 0: half the CUs
  int fp8_tile = 0, group_m = 0;  // group_m 0: the tile shape's own
  double pen224 = 1.03, pen_qk224 = 1.03;
  int persist = 0;
};

// ---- what the settings allow: each condition once, for plan_gemm() and for the predicates callers ask before they build a batch ----------------
inline bool gemm_v3_mode(const GemmMode& m) { return m.impl == 3; }                                   // the one-wave-per-SIMD bf16 kernels take launches
inline bool gemm_fp8_v3_mode(const GemmMode& m) { return m.fp8_v3 && gemm_v3_mode(m); }               // ... and the one-wave-per-SIMD fp8 kernel
inline bool gemm_fp8_mx_k(int K) { return K % 512 == 0 && K >= 512; }                                 // K of a block-scaled fp8 problem
inline bool gemm_conv_stats_available(const GemmMode& m) { return gemm_v3_mode(m) && m.tile == 0; }   // convolution launches go to the kernel whose epilogue accumulates GroupNorm sums
inline bool gemm_qk_fusion_available(const GemmMode& m) { return gemm_v3_mode(m) && m.qk_fuse; }
inline bool gemm_dropres_available(const GemmMode& m) { return gemm_v3_mode(m); }                     // the masked residual add exists in the one-wave-per-SIMD kernel's permlane-paired epilogue only
inline bool gemm_fp8_mx_ok(const GemmMode& m, int K) { return gemm_fp8_v3_mode(m) && gemm_fp8_mx_k(K); }      // a block-scaled launch always takes the one-wave-per-SIMD kernel, whatever its tile count

struct TileCfg { int tm, tn, group_m; };
// {4,4} = 128x128: 64 accumulators and 80 KiB of LDS, TWO work-groups per CU -- for launches that would leave most CUs without a
// 256x256 tile (the rank-256 LoRA products of the distillation step: N = 256 or M = 256, 12-84 tiles at 256x256)
// {8,7} = 256x224: the shape that makes the forward's N = 3072 launches (18 row tiles of the 4096 + 512 row problems x 14 column
// tiles = 252) and the N = 12288 launch (990 tiles = 3.87 rounds of 7/8-size tiles) fill their last round -- what hipBLASLt's
// MT256x224 kernels do for these shapes (1295 vs 1161 TF at 4608 x 3072 x 3072 in profiles/r02s_microbench.log)
// {7,8} = 224x256: the k|q|v^T launch of the Qwen-Image shape (4096 + 128 rows: 612 tiles of 256x256 = 2.39 rounds -> 718 tiles of 7/8 the size =
// 2.8 rounds); a wave keeps its 128 columns = one head, so the fused q / k epilogue works unchanged (FLUX's 4096 + 512 rows stay 256x256: 648 tiles)
static const TileCfg kTileCfg[6] = {{256, 256, GROUP_M}, {288, 192, 5}, {320, 192, 4}, {128, 128, 8}, {256, 224, GROUP_M}, {224, 256, GROUP_M}};

inline int count_tiles(GemmBatch& batch, int tm, int tn, bool fill) {
  int total = 0;
  for (int i = 0; i < batch.nprob; ++i) {
    GemmProblem& p = batch.p[i];
    const int tiles_m = (p.M + tm - 1) / tm, tiles_n = (p.N + tn - 1) / tn;
    const int sk = (p.split_k < 1 || p.out_f32 != 3) ? 1 : p.split_k;
    if (fill) {
      p.tiles_m = tiles_m;
      p.tiles_n = tiles_n;
      p.tile_start = total;
      p.split_k = sk;
    }
    total += tiles_m * tiles_n * sk;
  }
  return total;
}

// What launch_gemm() does with a batch.  EMPTY: no tile, success without a launch;  INVALID: hipErrorInvalidValue.
struct GemmPlan {
  enum Status { OK, EMPTY, INVALID } status;
  enum Family { V3_BF16, V3_CONV, V3_FP8, PHASE8 } family;      // gemm_kernel_v3 / v3s<MI, NJ, false, persist>, gemm_kernel_v3<MI, NJ, true, 0>, gemm_kernel_v3f8<MI, NJ, flag>, gemm_kernel_v2<flag>
  bool flag;              // V3_FP8: block-scaled activations (MX);  PHASE8: fp8 operands
  int mi, nj;             // the tile is 32 mi x 32 nj
  int total;              // tiles of the launch (= batch.total_tiles)
  int persist;            // V3_BF16: 0 = one work-group per tile, 1 / 2 = `grid` work-groups walk the tiles
  int grid;
};

// The launch of `family` on tm x tn tiles: fills the batch (tiles_m, tiles_n, tile_start, the normalised split_k, total_tiles, group_m).
inline GemmPlan gemm_plan_tiles(GemmBatch& batch, const GemmMode& mode, int cus, GemmPlan::Family family, bool flag, int tm, int tn, int group_m) {
  const int total = count_tiles(batch, tm, tn, true);
  batch.total_tiles = total;
  GemmPlan pl{GemmPlan::OK, family, flag, tm / 32, tn / 32, total, 0, total};
  if (total == 0) {
    pl.status = GemmPlan::EMPTY;
    return pl;
  }
  batch.group_m = mode.group_m ? mode.group_m : group_m;
  // (The VAE's convolutions ran the persistent walk as an A/B in round 5 -- AFX_CONV_PERSIST, measured level, profiles/r05*: with the accumulator file asm-owned
  // (round 6) those instances no longer fit hipcc's arch VGPRs and it parked values in accumulator registers: dropped rather than shipped unsafe.)
  if (family == GemmPlan::V3_BF16) {
    const int slots = cus * (4 * pl.mi * pl.nj <= 64 ? 2 : 1);
    if ((mode.persist == 1 || mode.persist == 2) && total > slots && slots % 8 == 0) {
      pl.persist = mode.persist;
      pl.grid = slots;
    }
  }
  return pl;
}

inline GemmPlan plan_gemm(GemmBatch& batch, const GemmMode& mode, int cus) {
  const GemmPlan invalid{GemmPlan::INVALID, GemmPlan::PHASE8, false, 0, 0, 0, 0, 0};
  GemmPlan empty = invalid;
  empty.status = GemmPlan::EMPTY;
  const int tile_env = mode.tile;
  // ---- one-wave-per-SIMD kernel: bf16 launches whose every problem is in a fast epilogue mode.  The tile shape is the one with
  // the least (rounds of `cus` tiles) x (tile area): the launch is as long as its fullest CU.
  bool v3_ok = gemm_v3_mode(mode);
  for (int i = 0; i < batch.nprob; ++i) {
    const GemmProblem& p = batch.p[i];
    const bool bf16_out = p.out_f32 == 0, f32_out = (p.out_f32 == 1 || p.out_f32 == 2) && p.epi == EPI_NONE;     // (3 = split-K slabs: 8-phase)
    v3_ok = v3_ok && (bf16_out || f32_out) && p.fp8 == 0 && p.conv_cin_tiles == 0 && p.conv_wp == 0 && p.pre == nullptr && p.K >= BK;
    if (p.drop_on && (p.epi != EPI_GATE_RES || p.gate != nullptr || p.out_f32 != 0)) return invalid;
  }
  for (int i = 0; i < batch.nprob; ++i)
    if (batch.p[i].drop_on && !v3_ok) return invalid;        // the masked residual add lives in the one-wave-per-SIMD kernel's epilogue only
  // ---- the VAE decoders' 3x3 convolutions: the same kernel with the implicit-GEMM address stream and the border-zeroing epilogue;
  // 256x128 tiles for the <= 128-channel layers (the full-resolution stage and conv_out, half of a 256-wide tile otherwise)
  bool conv_all = gemm_conv_stats_available(mode) && batch.nprob >= 1;
  for (int i = 0; i < batch.nprob; ++i) {
    const GemmProblem& p = batch.p[i];
    conv_all = conv_all && p.conv_cin_tiles > 0 && p.conv_wp > 0 && p.out_f32 == 0 && p.fp8 == 0 && p.pre == nullptr && p.epi != EPI_GELU &&
               p.split_k <= 1 && p.N == batch.p[0].N && (p.up_phase == 0 || (p.epi == EPI_NONE && p.gn_stats == nullptr));
  }
  if (conv_all) {
    // 256x128 tiles for the <= 128-channel layers only: for the 128^2 stage (134 tiles of 256x256 for 256 CUs, K = 4608) 268 narrow tiles measured
    // 116 us per launch against 93
    const bool narrow = batch.p[0].N <= 128;
    return gemm_plan_tiles(batch, mode, cus, GemmPlan::V3_CONV, false, 256, narrow ? 128 : 256, GROUP_M);
  }
  bool qk = false;
  for (int i = 0; i < batch.nprob; ++i) {
    const GemmProblem& p = batch.p[i];
    if (p.qk_D > 0) {
      qk = true;
      if (p.qk_D % 128 || p.N < p.qk_D || !p.qk_wk || !p.qk_wq || !p.rope_cos || !p.rope_sin || p.rope_period < 1 || p.rope_rows < 1 ||
          p.epi == EPI_GATE_RES)
        return invalid;
    }
  }
  for (int i = 0; i < batch.nprob; ++i)
    if (batch.p[i].w_perm16 || batch.p[i].bias_rows) {
      qk = true;                                         // same kernel requirement (and the 256x256 shape: tested there)
      if (batch.p[i].out_f32 != 0 || batch.p[i].epi != EPI_NONE || (batch.p[i].w_perm16 && batch.p[i].N % 16)) return invalid;
    }
  bool all_fp8 = batch.nprob >= 1;
  for (int i = 0; i < batch.nprob; ++i) all_fp8 = all_fp8 && batch.p[i].fp8 != 0;
  if (qk && !v3_ok && !all_fp8) return invalid;        // callers ask gemm_qk_fusion_available() first (fp8: checked below)
  if (v3_ok) {
    int best = 0;
    bool f32_any = false;                               // fp32-output launches: the shapes with an even number of column tiles per wave only
    for (int i = 0; i < batch.nprob; ++i) f32_any = f32_any || batch.p[i].out_f32 != 0;
    if (qk) {                                           // one head = one wave's 128 columns: the two 256-wide shapes only
      best = 0;
      if (tile_env == 6) best = 5;
      else if (tile_env == 0) {
        const int t0 = count_tiles(batch, 256, 256, false), t5 = count_tiles(batch, 224, 256, false);
        if (t0 == 0) return empty;
        const double c0 = (double)((t0 + cus - 1) / cus) * 256, c5 = (double)((t5 + cus - 1) / cus) * 224 * mode.pen_qk224;
        if (c5 < c0) best = 5;
      }
    } else if (tile_env >= 1 && tile_env <= 6) best = (tile_env == 5 && f32_any) ? 0 : tile_env - 1;
    else {
      double best_cost = 0;
      int tiles256 = 0;
      for (int c = 0; c < 5; ++c) {
        const int tiles = count_tiles(batch, kTileCfg[c].tm, kTileCfg[c].tn, false);
        if (tiles == 0) return empty;
        if (c == 0) tiles256 = tiles;
        if (c == 3 && tiles256 * 2 > cus) continue;   // 128x128 only where 256x256 leaves half the CUs idle (measured: the 864-tile
                                                      // mlp GEMM as 3456 small tiles takes 362 us against 287)
        const int slots = c == 3 ? 2 * cus : cus;
        const int rounds = (tiles + slots - 1) / slots;
        // 256x256 has the best MFMA : LDS-read ratio (4 : 1 against 3.6 : 1 / 3.75 : 1) and the chip is power-capped: a tile
        // shape that fills the last round only makes every CU clock lower.  Measured with weights streaming from HBM
        // (tools/gemm_trace.hip TRACE_COLD=1, r02s): 288x192 wins 4-6 % at K = 3072 where it saves a round or fills a 216-tile
        // launch, is level at K = 12288 and loses 3 % at K = 15360 (its W slots leave the DMA the shorter lead); 320x192 never won.
        double pen = 1.0;
        if (c == 1) pen = batch.p[0].K <= 8192 ? 1.05 : 1.5;
        if (c == 2) pen = 1.10;
        if (c == 3) pen = 2.0;          // 16 MFMAs per 8 fragment reads and 4 DMA issues per k-half: the loop runs at about half rate
        if (c == 4) pen = f32_any ? 1e9 : mode.pen224;   // 56 MFMAs per 15 fragment reads (256x256: 64 per 16); bf16 epilogues only
        const double cost = (double)rounds * kTileCfg[c].tm * kTileCfg[c].tn * pen;
        if (c == 0 || cost < best_cost) { best = c; best_cost = cost; }
      }
    }
    return gemm_plan_tiles(batch, mode, cus, GemmPlan::V3_BF16, false, kTileCfg[best].tm, kTileCfg[best].tn, kTileCfg[best].group_m);
  }
  // ---- fp8 launches with at least one full round of 256x256 tiles: the one-wave-per-SIMD fp8 kernel (AFX_FP8_V3=0: 8-phase kernel, A/B)
  {
    bool ok = gemm_fp8_v3_mode(mode) && batch.nprob >= 1;
    bool mx_any = false, mx_all = true, c8_any = false, qk_any = false;
    for (int i = 0; i < batch.nprob; ++i) {
      const GemmProblem& p = batch.p[i];
      ok = ok && p.fp8 != 0 && p.out_f32 == 0 && p.conv_cin_tiles == 0 && p.conv_wp == 0 && p.pre == nullptr && p.K % 128 == 0 && p.K >= 256 &&
           !p.w_perm16 && !p.bias_rows && p.split_k <= 1;
      qk_any = qk_any || p.qk_D > 0;
      mx_any = mx_any || p.a_mx != nullptr;
      if (p.c8 != nullptr && (p.epi == EPI_GATE_RES || p.c8_col0 % 128 || !p.c_mx || p.ldc8 % 8 || (p.gelu_col0 != 0 && p.gelu_col0 != p.c8_col0))) return invalid;
      c8_any = c8_any || p.c8 != nullptr;
      mx_all = mx_all && p.a_mx != nullptr && gemm_fp8_mx_k(p.K) && p.ld_mx % 4 == 0;
    }
    // fewest 256x256 tiles of a launch that takes this kernel: by default half a round -- 216-tile launches (N = 3072): 2.1-2.2 -> 2.7 PF; below half a
    // round the 8-phase kernel's 2 waves per SIMD win
    const int min_tiles = mode.fp8_v3_min >= 0 ? mode.fp8_v3_min : cus / 2;
    if (mx_any && !(ok && mx_all)) return invalid;      // block scales are this kernel's format only (callers ask gemm_fp8_mx_ok() first)
    if ((c8_any || qk_any) && !ok) return invalid;     // (the fused q / k epilogue: this kernel only; the engine asks for it with block scales only)
    if (ok && (mx_any || c8_any || qk_any || count_tiles(batch, 256, 256, false) >= min_tiles)) {
      // 224x256 (round 5): a launch costs ceil(rounds) x tile area and the fp8 kernel had ONE shape -- Qwen-Image's 4096 + 128 rows are 17 + 1
      // row tiles of 256 (N = 3072: 216 tiles = 0.84 round, N = 12288: 864 = 3.4 -> 4 rounds, N = 9216: 648 = 2.5 -> 3) but 19 + 1 of 224 (240 tiles = 0.94,
      // 960 = 3.75 -> 4, 720 = 2.8 -> 3 rounds of tiles 7/8 the size); FLUX's joint 4608 rows of the single blocks likewise (out-projection: 252 tiles).
      // AFX_FP8_TILE=1 / 2 force 256x256 / 224x256 (A/B).  The fused q / k epilogue keeps 256x256 (one head = one wave's 128 columns either way, but its
      // row-tile loop is written for 8).
      const int tile_env8 = mode.fp8_tile;
      const int t8 = count_tiles(batch, 256, 256, false), t7 = count_tiles(batch, 224, 256, false);
      const int r8 = (t8 + cus - 1) / cus, r7 = (t7 + cus - 1) / cus;
      bool use7 = !qk_any && (tile_env8 == 2 || (tile_env8 == 0 && (double)r7 * 224 * 1.02 < (double)r8 * 256));
      return gemm_plan_tiles(batch, mode, cus, GemmPlan::V3_FP8, mx_any, use7 ? 224 : 256, 256, GROUP_M);
    }
  }
  bool fp8 = false;
  for (int i = 0; i < batch.nprob; ++i) fp8 = fp8 || batch.p[i].fp8 != 0;     // a launch is all-bf16 or all-fp8
  return gemm_plan_tiles(batch, mode, cus, GemmPlan::PHASE8, fp8, BM, BN, GROUP_M);
}

}  // namespace afx
