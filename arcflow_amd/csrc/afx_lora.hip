// afx_lora_fold: fold up to 8 weighted low-rank adapters into one bf16 linear on the device (style LoRAs next to the ArcFlow adapter,
// arcflow_amd/pipelines/arcflow_loader.py):
//
//   dst[o, i] = bf16_rne( float(base[o, i]) + sum_j s_j * ( sum_r B_j[o, r] * A_j[r, i] ) )
//
// base / dst are row slices of packed weight matrices (own leading dimensions), A_j [r_j, I] and B_j [O, r_j] are bf16, s_j is fp32 and
// multiplies the fp32-accumulated product of adapter j: it is never folded into a bf16 operand, so the only rounding is the one at the store.
//
// One work-group of 4 waves owns a 64 x 64 tile of dst.  Per adapter and per 32 ranks it stages B_j[64 rows, 32] and A_j[32, 64 columns]^T in
// LDS (ranks past r_j are zeros: any rank >= 1 runs, no padded copies on the host) and every wave multiplies its 16 rows by the four column
// tiles on the 16x16x32 bf16 MFMA.  The whole rank of every adapter is summed inside the one work-group that owns the tile, in a fixed order:
// no split over the rank, no atomics, the result is bit-reproducible.  The fp32 sum goes through LDS once so that base is read and dst written
// in 16-byte words along the rows; there is no weight-sized fp32 temporary.
//
// HBM traffic: 2 B read + 2 B written per element; the A / B panels (2 (O + I) r_j bytes per adapter) are re-read per tile out of L2.
// 2 sum(r_j) flop per element is far below the MFMA / HBM ridge at the ranks in use: the kernel's roofline is the HBM one.
//
// DoRA adapters (a magnitude m[o] per output row next to A / B) are no sum of low-rank products: adapter j turns row o of the base into
// g_j[o] (w + s_j B_j A_j)[o, :] with g_j[o] = m_j[o] / || (w + s_j B_j A_j)[o, :] ||, so the whole row has to be seen before any element can be
// written.  Two launches.  afx_lora_row_gain forms every 64 x 64 tile of w + s B A exactly as the fold does (lora_tile_product is the one copy of
// the staging and the MFMA loop) and sums its squares per row: one work-group per 64-row strip walks the column tiles in order, every thread
// keeps the running sum of its 8 columns of a row, and the 8 partial sums of a row are added in column order at the end -- a fixed order, no
// atomics, no workspace, bit-reproducible.  afx_lora_fold_rows is the fold with a per-row factor on every product and on the base:
//
//   dst[o, i] = bf16_rne( c[o] float(base[o, i]) + sum_j (g_j[o] s_j) * ( sum_r B_j[o, r] * A_j[r, i] ) ),   c[o] = 1 + sum_{j with gain} (g_j[o] - 1)
//
// (g_j = 1 where adapter j has no gain vector; c in fp32 in adapter order).  Without any gain vector every factor is s_j and c is 1: fma(1, w, d)
// is w + d, the bits of afx_lora_fold.
//
// LyCORIS LoHa and LoKr adapters are no sums of low-rank products either (rules restated from memory, NOT PINNED against LyCORIS / ComfyUI):
// LoHa's delta is (w1_a w1_b) (*) (w2_a w2_b) element by element, LoKr's is kron(w1, w2).  afx_lora_fold_terms is afx_lora_fold_rows over a list of
// terms of three kinds: a LoRA term as above; a LoHa term, whose two products come out of lora_tile_product one after the other in the same
// accumulator layout and are multiplied in fp32 registers (never rounded to bf16); a LoKr term, one fp32 product w1[r / c, i / d] w2[r % c, i % d]
// per element from two dense fp32 matrices out of L2, r = row0 + o so that a row slice of a fused tensor folds without splitting the Kronecker
// product.  Every term enters the running fp32 total by one fused multiply-add with its scale, in term order; the store is still the one rounding.
#include "afx_api_util.h"
#include "afx_common.h"

namespace afx {

struct LoraFoldArgs {
  const bf16_t* A[AFX_LORA_MAX_ADAPTERS];
  const bf16_t* B[AFX_LORA_MAX_ADAPTERS];
  int32_t r[AFX_LORA_MAX_ADAPTERS];
  float s[AFX_LORA_MAX_ADAPTERS];
};

struct LoraGainArgs {
  const float* g[AFX_LORA_MAX_ADAPTERS];      // per adapter: fp32 [O] row gains, null = a plain LoRA
};

constexpr int LF_T = 64;          // tile edge (rows and columns of dst)
constexpr int LF_K = 32;          // ranks per MFMA step
constexpr int LF_LDK = LF_K + 8;  // bf16 per LDS operand row: 80 bytes keep every 8-rank fragment 16-byte aligned
constexpr int LF_LDC = LF_T + 4;  // floats per row of the fp32 tile

// acc = B_j[o0 .. o0 + 63, :] . A_j[:, i0 .. i0 + 63] in fp32 for the calling work-group of 256 threads: accumulator element e of column tile n is row
// 16 wave + 4 (lane / 16) + e, column 16 n + lane % 16 of the tile.  Begins with a barrier (every wave is done with what sA / sB held before).
__device__ __forceinline__ void lora_tile_product(const bf16_t* __restrict__ Aj, const bf16_t* __restrict__ Bj, int r, int I, int64_t o0, int i0,
                                                  bf16_t* sA, bf16_t* sB, f32x4_t (&acc)[4]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b_row = tid >> 2, b_k = (tid & 3) * 8;          // staging of B: 8 ranks of one row per thread
  const int a_k = tid >> 3, a_c = (tid & 7) * 8;            // staging of A: 8 columns of one rank per thread
  const int fi = lane & 15, fk = (lane >> 4) * 8;           // MFMA operand: row / column fi, ranks fk .. fk + 7
  const bool b_vec = (r & 7) == 0 && (reinterpret_cast<uintptr_t>(Bj) & 15) == 0;      // rows of B_j start on 16 bytes
#pragma unroll
  for (int n = 0; n < 4; ++n) acc[n] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < r; k0 += LF_K) {
    __syncthreads();                                      // every wave is done with the previous step's operands
    {
      const bf16_t* p = Bj + (o0 + b_row) * (int64_t)r + k0 + b_k;
      u32x4_t v = (u32x4_t){0u, 0u, 0u, 0u};
      if (b_vec) {
        if (k0 + b_k < r) v = *reinterpret_cast<const u32x4_t*>(p);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (k0 + b_k + e < r) v[e >> 1] |= (uint32_t)p[e] << (16 * (e & 1));
      }
      *reinterpret_cast<u32x4_t*>(&sB[b_row * LF_LDK + b_k]) = v;
    }
    {
      u32x4_t v = (u32x4_t){0u, 0u, 0u, 0u};
      if (k0 + a_k < r) v = *reinterpret_cast<const u32x4_t*>(Aj + (int64_t)(k0 + a_k) * I + i0 + a_c);
#pragma unroll
      for (int e = 0; e < 8; ++e) sA[(a_c + e) * LF_LDK + a_k] = (bf16_t)(v[e >> 1] >> (16 * (e & 1)));
    }
    __syncthreads();
    const bf16x8_t bf = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u32x4_t*>(&sB[(16 * wave + fi) * LF_LDK + fk]));
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const bf16x8_t af = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u32x4_t*>(&sA[(16 * n + fi) * LF_LDK + fk]));
      acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf, af, acc[n], 0, 0, 0);      // rows: B_j (operand A), columns: A_j (operand B)
    }
  }
}

// the accumulator layout of lora_tile_product into the [row][column] fp32 tile
__device__ __forceinline__ void lora_tile_to_lds(const f32x4_t (&tot)[4], float* sC) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int e = 0; e < 4; ++e) sC[(16 * wave + 4 * (lane >> 4) + e) * LF_LDC + 16 * n + (lane & 15)] = tot[n][e];
}

// ROWS = false: afx_lora_fold (gn is not read).  ROWS = true: afx_lora_fold_rows.
template <bool ROWS>
__global__ __launch_bounds__(256) void lora_fold_kernel(const bf16_t* __restrict__ base, int64_t ld_base, bf16_t* __restrict__ dst,
                                                        int64_t ld_dst, int I, int J, LoraFoldArgs a, LoraGainArgs gn) {
  __shared__ __attribute__((aligned(16))) bf16_t sB[LF_T * LF_LDK];     // [row of the tile][rank]
  __shared__ __attribute__((aligned(16))) bf16_t sA[LF_T * LF_LDK];     // [column of the tile][rank]: A^T
  __shared__ __attribute__((aligned(16))) float sC[LF_T * LF_LDC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_i = I / LF_T;
  const int64_t o0 = (int64_t)(blockIdx.x / tiles_i) * LF_T;
  const int i0 = (int)(blockIdx.x % tiles_i) * LF_T;

  // the tile of base: two 16-byte words per thread, in flight while the products are formed
  u32x4_t bw[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int idx = tid + 256 * c, row = idx >> 3, c8 = (idx & 7) * 8;
    bw[c] = *reinterpret_cast<const u32x4_t*>(base + (o0 + row) * ld_base + i0 + c8);
  }
  if (J == 0) {                                             // (uniform) a plain copy: no add, so that -0 stays -0
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int idx = tid + 256 * c, row = idx >> 3, c8 = (idx & 7) * 8;
      *reinterpret_cast<u32x4_t*>(dst + (o0 + row) * ld_dst + i0 + c8) = bw[c];
    }
    return;
  }

  f32x4_t tot[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) tot[n] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  for (int j = 0; j < J; ++j) {
    f32x4_t acc[4];
    lora_tile_product(a.A[j], a.B[j], a.r[j], I, o0, i0, sA, sB, acc);
    const float s = a.s[j];
    float gs[4] = {s, s, s, s};                             // the factor of accumulator element e: row 16 wave + 4 (lane / 16) + e
    if (ROWS && gn.g[j] != nullptr) {                       // (uniform)
      const float* g = gn.g[j] + o0 + 16 * wave + 4 * (lane >> 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) gs[e] = g[e] * s;
    }
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int e = 0; e < 4; ++e) tot[n][e] = fmaf(gs[e], acc[n][e], tot[n][e]);
  }

  lora_tile_to_lds(tot, sC);
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int idx = tid + 256 * c, row = idx >> 3, c8 = (idx & 7) * 8;
    float f[8];
    unpack8(bw[c], f);
    const float* d = &sC[row * LF_LDC + c8];
    if (ROWS) {
      float cr = 1.f;                                       // c[o] = 1 + sum_j (g_j[o] - 1), in adapter order
      for (int j = 0; j < J; ++j)
        if (gn.g[j] != nullptr) cr += gn.g[j][o0 + row] - 1.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = fmaf(cr, f[e], d[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] += d[e];
    }
    *reinterpret_cast<u32x4_t*>(dst + (o0 + row) * ld_dst + i0 + c8) = pack8(f);       // the one rounding
  }
}

// afx_lora_fold_terms: the fold over terms of three kinds (include/arcflow_hip.h).  Passed by value; the fields follow afx_lora_term.
struct LoraTermArgs {
  const bf16_t* down[AFX_LORA_MAX_ADAPTERS];   // LoRA A / LoHa hada_w1_b: [rank, I]
  const bf16_t* up[AFX_LORA_MAX_ADAPTERS];     // LoRA B / LoHa hada_w1_a: [O, rank]
  const bf16_t* down2[AFX_LORA_MAX_ADAPTERS];  // LoHa hada_w2_b
  const bf16_t* up2[AFX_LORA_MAX_ADAPTERS];    // LoHa hada_w2_a
  const float* w1[AFX_LORA_MAX_ADAPTERS];      // LoKr [ka, kb]
  const float* w2[AFX_LORA_MAX_ADAPTERS];      // LoKr [kc, kd]
  const float* g[AFX_LORA_MAX_ADAPTERS];       // LoRA: row gains or null
  int32_t kind[AFX_LORA_MAX_ADAPTERS];
  int32_t r[AFX_LORA_MAX_ADAPTERS];
  int32_t r2[AFX_LORA_MAX_ADAPTERS];
  int32_t kb[AFX_LORA_MAX_ADAPTERS];
  int32_t kc[AFX_LORA_MAX_ADAPTERS];
  int32_t kd[AFX_LORA_MAX_ADAPTERS];
  int32_t row0[AFX_LORA_MAX_ADAPTERS];         // (row0 + O <= ka kc < 2^31 is checked on the host)
  float s[AFX_LORA_MAX_ADAPTERS];
};

// lora_fold_kernel<true> with a delta per term instead of a low-rank product per adapter.  A LoRA term takes lora_fold_kernel<true>'s instructions
// in its order (the same bits); a LoHa term forms its two products one after the other through lora_tile_product -- the same accumulator layout, so
// the element-wise product is a register product -- and a LoKr term forms its element of kron(w1, w2) in that layout from two loads out of L2.
__global__ __launch_bounds__(256) void lora_fold_terms_kernel(const bf16_t* __restrict__ base, int64_t ld_base, bf16_t* __restrict__ dst,
                                                              int64_t ld_dst, int I, int J, LoraTermArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t sB[LF_T * LF_LDK];
  __shared__ __attribute__((aligned(16))) bf16_t sA[LF_T * LF_LDK];
  __shared__ __attribute__((aligned(16))) float sC[LF_T * LF_LDC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_i = I / LF_T;
  const int64_t o0 = (int64_t)(blockIdx.x / tiles_i) * LF_T;
  const int i0 = (int)(blockIdx.x % tiles_i) * LF_T;

  u32x4_t bw[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int idx = tid + 256 * c, row = idx >> 3, c8 = (idx & 7) * 8;
    bw[c] = *reinterpret_cast<const u32x4_t*>(base + (o0 + row) * ld_base + i0 + c8);
  }
  if (J == 0) {                                             // (uniform) a plain copy: no add, so that -0 stays -0
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int idx = tid + 256 * c, row = idx >> 3, c8 = (idx & 7) * 8;
      *reinterpret_cast<u32x4_t*>(dst + (o0 + row) * ld_dst + i0 + c8) = bw[c];
    }
    return;
  }

  f32x4_t tot[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) tot[n] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const int er = 16 * wave + 4 * (lane >> 4);               // accumulator element e of column tile n: row er + e, column 16 n + lane % 16 of the tile

  for (int j = 0; j < J; ++j) {                             // (every branch on the term is uniform)
    const float s = a.s[j];
    if (a.kind[j] == AFX_LORA_TERM_LOKR) {
      const int kc = a.kc[j], kd = a.kd[j], kb = a.kb[j];
      const float* w1 = a.w1[j];
      const float* w2 = a.w2[j];
      int p[4], q[4], u[4], v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = a.row0[j] + (int)o0 + er + e;       // < ka kc < 2^31
        p[e] = row / kc;
        q[e] = row - p[e] * kc;
      }
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int col = i0 + 16 * n + (lane & 15);          // < I = kb kd
        u[n] = col / kd;
        v[n] = col - u[n] * kd;
      }
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = __fmul_rn(w1[(int64_t)p[e] * kb + u[n]], w2[(int64_t)q[e] * kd + v[n]]);
          tot[n][e] = fmaf(s, d, tot[n][e]);
        }
      continue;
    }
    f32x4_t acc[4];
    lora_tile_product(a.down[j], a.up[j], a.r[j], I, o0, i0, sA, sB, acc);
    if (a.kind[j] == AFX_LORA_TERM_LOHA) {
      f32x4_t acc2[4];
      lora_tile_product(a.down2[j], a.up2[j], a.r2[j], I, o0, i0, sA, sB, acc2);
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int e = 0; e < 4; ++e) tot[n][e] = fmaf(s, __fmul_rn(acc[n][e], acc2[n][e]), tot[n][e]);
      continue;
    }
    float gs[4] = {s, s, s, s};
    if (a.g[j] != nullptr) {
      const float* g = a.g[j] + o0 + er;
#pragma unroll
      for (int e = 0; e < 4; ++e) gs[e] = g[e] * s;
    }
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int e = 0; e < 4; ++e) tot[n][e] = fmaf(gs[e], acc[n][e], tot[n][e]);
  }

  lora_tile_to_lds(tot, sC);
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int idx = tid + 256 * c, row = idx >> 3, c8 = (idx & 7) * 8;
    float f[8];
    unpack8(bw[c], f);
    const float* d = &sC[row * LF_LDC + c8];
    float cr = 1.f;                                         // c[o] = 1 + sum_j (g_j[o] - 1), in term order
    for (int j = 0; j < J; ++j)
      if (a.g[j] != nullptr) cr += a.g[j][o0 + row] - 1.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = fmaf(cr, f[e], d[e]);
    *reinterpret_cast<u32x4_t*>(dst + (o0 + row) * ld_dst + i0 + c8) = pack8(f);       // the one rounding
  }
}

// gain[o] = m[o] / sqrt( sum_i (w[o, i] + s (B A)[o, i])^2 ), 0 where the sum is 0.  One work-group per 64 rows.
__global__ __launch_bounds__(256) void lora_row_gain_kernel(const bf16_t* __restrict__ base, int64_t ld_base, int I, const bf16_t* __restrict__ A,
                                                            const bf16_t* __restrict__ B, int r, float s, const float* __restrict__ m,
                                                            float* __restrict__ gain) {
  __shared__ __attribute__((aligned(16))) bf16_t sB[LF_T * LF_LDK];
  __shared__ __attribute__((aligned(16))) bf16_t sA[LF_T * LF_LDK];
  __shared__ __attribute__((aligned(16))) float sC[LF_T * LF_LDC];
  __shared__ float sR[LF_T * 8];                            // [row of the strip][8-column group of a tile]: the partial sums of squares
  const int tid = threadIdx.x;
  const int64_t o0 = (int64_t)blockIdx.x * LF_T;
  float ss[2] = {0.f, 0.f};                                 // rows tid / 8 and 32 + tid / 8, columns 8 (tid % 8) .. + 7 of every tile
  for (int i0 = 0; i0 < I; i0 += LF_T) {
    u32x4_t bw[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int idx = tid + 256 * c, row = idx >> 3, c8 = (idx & 7) * 8;
      bw[c] = *reinterpret_cast<const u32x4_t*>(base + (o0 + row) * ld_base + i0 + c8);
    }
    f32x4_t acc[4], tot[4];
    lora_tile_product(A, B, r, I, o0, i0, sA, sB, acc);     // its first barrier also ends the previous tile's reads of sC
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int e = 0; e < 4; ++e) tot[n][e] = fmaf(s, acc[n][e], 0.f);        // as the fold's first adapter
    lora_tile_to_lds(tot, sC);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int idx = tid + 256 * c, row = idx >> 3, c8 = (idx & 7) * 8;
      float f[8];
      unpack8(bw[c], f);
      const float* d = &sC[row * LF_LDC + c8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float v = f[e] + d[e];
        ss[c] = fmaf(v, v, ss[c]);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) sR[tid + 256 * c] = ss[c];    // = [row (tid + 256 c) / 8][group tid % 8]
  __syncthreads();
  if (tid < LF_T) {
    float sum = sR[tid * 8];
#pragma unroll
    for (int q = 1; q < 8; ++q) sum += sR[tid * 8 + q];
    gain[o0 + tid] = sum == 0.f ? 0.f : __fdiv_rn(m[o0 + tid], __fsqrt_rn(sum));
  }
}

// what every fold asks of its two row slices: 0, or AFX_E_INVALID with the message set
static int lora_slice_guards(const char* what, const void* base, int64_t ld_base, void* dst, int64_t ld_dst, int32_t O, int32_t I) {
  if (O < 64 || I < 64 || O % 64 || I % 64) return fail(AFX_E_INVALID, "%s: O = %d and I = %d must be positive multiples of 64", what, O, I);
  if (ld_base < I || ld_dst < I) return fail(AFX_E_INVALID, "%s: leading dimension below I = %d", what, I);
  if (ld_base % 8 || ld_dst % 8 || ((uintptr_t)base & 15) || ((uintptr_t)dst & 15))
    return fail(AFX_E_INVALID, "%s: base / dst must be 16-byte aligned with leading dimensions that are multiples of 8", what);
  if (ranges_overlap(base, ((int64_t)(O - 1) * ld_base + I) * 2, dst, ((int64_t)(O - 1) * ld_dst + I) * 2))
    return fail(AFX_E_INVALID, "%s: dst overlaps base", what);
  if ((int64_t)(O / 64) * (I / 64) > 0x7fffffff) return fail(AFX_E_INVALID, "%s: %lld tiles", what, (long long)(O / 64) * (I / 64));
  return AFX_OK;
}

// the guards and the launch of afx_lora_fold (row_gain == nullptr, `rows` false) and afx_lora_fold_rows
static int lora_fold_launch(const char* what, bool rows, const void* base, int64_t ld_base, void* dst, int64_t ld_dst, int32_t O, int32_t I, int32_t J,
                            const void* const* A, const void* const* B, const int32_t* ranks, const float* scales, const float* const* row_gain,
                            void* stream) {
  if (!base || !dst) return fail(AFX_E_INVALID, "%s: null base / dst", what);
  if (J < 0 || J > AFX_LORA_MAX_ADAPTERS) return fail(AFX_E_INVALID, "%s: %d adapters (0 .. %d)", what, J, AFX_LORA_MAX_ADAPTERS);
  if (J > 0 && (!A || !B || !ranks || !scales)) return fail(AFX_E_INVALID, "%s: null adapter array", what);
  if (int rc = lora_slice_guards(what, base, ld_base, dst, ld_dst, O, I)) return rc;
  const int64_t dst_bytes = ((int64_t)(O - 1) * ld_dst + I) * 2;
  LoraFoldArgs args{};
  LoraGainArgs gains{};
  for (int j = 0; j < J; ++j) {
    if (!A[j] || !B[j]) return fail(AFX_E_INVALID, "%s: null A / B of adapter %d", what, j);
    if (ranks[j] < 1) return fail(AFX_E_INVALID, "%s: rank %d of adapter %d (>= 1)", what, ranks[j], j);
    if ((uintptr_t)A[j] & 15) return fail(AFX_E_INVALID, "%s: A of adapter %d must be 16-byte aligned", what, j);
    if ((uintptr_t)B[j] & 1) return fail(AFX_E_INVALID, "%s: B of adapter %d must be 2-byte aligned", what, j);
    args.A[j] = (const bf16_t*)A[j];
    args.B[j] = (const bf16_t*)B[j];
    args.r[j] = ranks[j];
    args.s[j] = scales[j];
    if (row_gain && row_gain[j]) {
      if ((uintptr_t)row_gain[j] & 3) return fail(AFX_E_INVALID, "%s: the row gains of adapter %d must be 4-byte aligned", what, j);
      if (ranges_overlap(row_gain[j], (int64_t)O * 4, dst, dst_bytes)) return fail(AFX_E_INVALID, "%s: dst overlaps the row gains of adapter %d", what, j);
      gains.g[j] = row_gain[j];
    }
  }
  const int64_t tiles = (int64_t)(O / 64) * (I / 64);
  hipLaunchKernelGGL(rows ? lora_fold_kernel<true> : lora_fold_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)base, ld_base, (bf16_t*)dst, ld_dst, (int)I, (int)J, args, gains);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

// the guards and the launch of afx_lora_fold_terms
static int lora_fold_terms_launch(const void* base, int64_t ld_base, void* dst, int64_t ld_dst, int32_t O, int32_t I, int32_t J, const afx_lora_term* terms,
                                  void* stream) {
  const char* what = "afx_lora_fold_terms";
  if (!base || !dst) return fail(AFX_E_INVALID, "%s: null base / dst", what);
  if (J < 0 || J > AFX_LORA_MAX_ADAPTERS) return fail(AFX_E_INVALID, "%s: %d terms (0 .. %d)", what, J, AFX_LORA_MAX_ADAPTERS);
  if (J > 0 && !terms) return fail(AFX_E_INVALID, "%s: null term array", what);
  if (int rc = lora_slice_guards(what, base, ld_base, dst, ld_dst, O, I)) return rc;
  const int64_t dst_bytes = ((int64_t)(O - 1) * ld_dst + I) * 2;
  LoraTermArgs args{};
  for (int j = 0; j < J; ++j) {
    const afx_lora_term& t = terms[j];
    args.kind[j] = t.kind;
    args.s[j] = t.scale;
    if (t.kind != AFX_LORA_TERM_LORA && t.kind != AFX_LORA_TERM_LOHA && t.kind != AFX_LORA_TERM_LOKR)
      return fail(AFX_E_INVALID, "%s: unknown kind %d of term %d", what, t.kind, j);
    if (t.kind != AFX_LORA_TERM_LORA && t.row_gain) return fail(AFX_E_INVALID, "%s: term %d has row gains but is no LoRA term", what, j);
    if (t.kind == AFX_LORA_TERM_LOKR) {
      if (!t.w1 || !t.w2) return fail(AFX_E_INVALID, "%s: null w1 / w2 of LoKr term %d", what, j);
      if (((uintptr_t)t.w1 & 3) || ((uintptr_t)t.w2 & 3)) return fail(AFX_E_INVALID, "%s: w1 / w2 of LoKr term %d must be 4-byte aligned", what, j);
      if (t.ka < 1 || t.kb < 1 || t.kc < 1 || t.kd < 1)
        return fail(AFX_E_INVALID, "%s: LoKr term %d factors [%d, %d] x [%d, %d] (all >= 1)", what, j, t.ka, t.kb, t.kc, t.kd);
      if ((int64_t)t.kb * t.kd != I) return fail(AFX_E_INVALID, "%s: LoKr term %d has kb kd = %lld columns, I = %d", what, j, (long long)t.kb * t.kd, I);
      const int64_t vrows = (int64_t)t.ka * t.kc;
      if (vrows > 0x7fffffff || t.row0 < 0 || t.row0 + O > vrows)
        return fail(AFX_E_INVALID, "%s: LoKr term %d: row0 = %lld with O = %d outside the %lld rows of kron(w1, w2) (< 2^31)", what, j, (long long)t.row0, O,
                    (long long)vrows);
      args.w1[j] = t.w1;
      args.w2[j] = t.w2;
      args.kb[j] = t.kb;
      args.kc[j] = t.kc;
      args.kd[j] = t.kd;
      args.row0[j] = (int32_t)t.row0;
      continue;
    }
    const bool loha = t.kind == AFX_LORA_TERM_LOHA;
    if (!t.down || !t.up || (loha && (!t.down2 || !t.up2))) return fail(AFX_E_INVALID, "%s: null down / up of term %d", what, j);
    if (t.rank < 1 || (loha && t.rank2 < 1)) return fail(AFX_E_INVALID, "%s: rank %d of term %d (>= 1)", what, t.rank < 1 ? t.rank : t.rank2, j);
    if (((uintptr_t)t.down & 15) || (loha && ((uintptr_t)t.down2 & 15))) return fail(AFX_E_INVALID, "%s: down of term %d must be 16-byte aligned", what, j);
    if (((uintptr_t)t.up & 1) || (loha && ((uintptr_t)t.up2 & 1))) return fail(AFX_E_INVALID, "%s: up of term %d must be 2-byte aligned", what, j);
    args.down[j] = (const bf16_t*)t.down;
    args.up[j] = (const bf16_t*)t.up;
    args.r[j] = t.rank;
    if (loha) {
      args.down2[j] = (const bf16_t*)t.down2;
      args.up2[j] = (const bf16_t*)t.up2;
      args.r2[j] = t.rank2;
    } else if (t.row_gain) {
      if ((uintptr_t)t.row_gain & 3) return fail(AFX_E_INVALID, "%s: the row gains of term %d must be 4-byte aligned", what, j);
      if (ranges_overlap(t.row_gain, (int64_t)O * 4, dst, dst_bytes)) return fail(AFX_E_INVALID, "%s: dst overlaps the row gains of term %d", what, j);
      args.g[j] = t.row_gain;
    }
  }
  const int64_t tiles = (int64_t)(O / 64) * (I / 64);
  hipLaunchKernelGGL(lora_fold_terms_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)base, ld_base, (bf16_t*)dst, ld_dst,
                     (int)I, (int)J, args);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

}  // namespace afx

using namespace afx;

extern "C" {

int afx_lora_fold(const void* base, int64_t ld_base, void* dst, int64_t ld_dst, int32_t O, int32_t I, int32_t J,
                  const void* const* A, const void* const* B, const int32_t* ranks, const float* scales, void* stream) {
  return lora_fold_launch("afx_lora_fold", false, base, ld_base, dst, ld_dst, O, I, J, A, B, ranks, scales, nullptr, stream);
}

int afx_lora_fold_rows(const void* base, int64_t ld_base, void* dst, int64_t ld_dst, int32_t O, int32_t I, int32_t J,
                       const void* const* A, const void* const* B, const int32_t* ranks, const float* scales, const float* const* row_gain,
                       void* stream) {
  return lora_fold_launch("afx_lora_fold_rows", true, base, ld_base, dst, ld_dst, O, I, J, A, B, ranks, scales, row_gain, stream);
}

int afx_lora_fold_terms(const void* base, int64_t ld_base, void* dst, int64_t ld_dst, int32_t O, int32_t I, int32_t J,
                        const afx_lora_term* terms, void* stream) {
  return lora_fold_terms_launch(base, ld_base, dst, ld_dst, O, I, J, terms, stream);
}

int afx_lora_row_gain(const void* base, int64_t ld_base, int32_t O, int32_t I, const void* A, const void* B, int32_t r, float s,
                      const float* m, float* gain, void* stream) {
  if (!base || !A || !B || !m || !gain) return fail(AFX_E_INVALID, "afx_lora_row_gain: null argument");
  if (O < 64 || I < 64 || O % 64 || I % 64)
    return fail(AFX_E_INVALID, "afx_lora_row_gain: O = %d and I = %d must be positive multiples of 64", O, I);
  if (ld_base < I) return fail(AFX_E_INVALID, "afx_lora_row_gain: leading dimension below I = %d", I);
  if (ld_base % 8 || ((uintptr_t)base & 15))
    return fail(AFX_E_INVALID, "afx_lora_row_gain: base must be 16-byte aligned with a leading dimension that is a multiple of 8");
  if (r < 1) return fail(AFX_E_INVALID, "afx_lora_row_gain: rank %d (>= 1)", r);
  if ((uintptr_t)A & 15) return fail(AFX_E_INVALID, "afx_lora_row_gain: A must be 16-byte aligned");
  if ((uintptr_t)B & 1) return fail(AFX_E_INVALID, "afx_lora_row_gain: B must be 2-byte aligned");
  if (((uintptr_t)m & 3) || ((uintptr_t)gain & 3)) return fail(AFX_E_INVALID, "afx_lora_row_gain: m / gain must be 4-byte aligned");
  const int64_t gain_bytes = (int64_t)O * 4;
  if (ranges_overlap(gain, gain_bytes, base, ((int64_t)(O - 1) * ld_base + I) * 2) || ranges_overlap(gain, gain_bytes, A, (int64_t)r * I * 2) ||
      ranges_overlap(gain, gain_bytes, B, (int64_t)O * r * 2) || ranges_overlap(gain, gain_bytes, m, gain_bytes))
    return fail(AFX_E_INVALID, "afx_lora_row_gain: gain overlaps base / A / B / m");
  hipLaunchKernelGGL(lora_row_gain_kernel, dim3((unsigned)(O / 64)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)base, ld_base, (int)I,
                     (const bf16_t*)A, (const bf16_t*)B, (int)r, s, m, gain);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

}  // extern "C"
