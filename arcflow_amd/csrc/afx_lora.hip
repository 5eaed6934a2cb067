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
#include "afx_api_util.h"
#include "afx_common.h"

namespace afx {

struct LoraFoldArgs {
  const bf16_t* A[AFX_LORA_MAX_ADAPTERS];
  const bf16_t* B[AFX_LORA_MAX_ADAPTERS];
  int32_t r[AFX_LORA_MAX_ADAPTERS];
  float s[AFX_LORA_MAX_ADAPTERS];
};

constexpr int LF_T = 64;          // tile edge (rows and columns of dst)
constexpr int LF_K = 32;          // ranks per MFMA step
constexpr int LF_LDK = LF_K + 8;  // bf16 per LDS operand row: 80 bytes keep every 8-rank fragment 16-byte aligned
constexpr int LF_LDC = LF_T + 4;  // floats per row of the fp32 tile

__global__ __launch_bounds__(256) void lora_fold_kernel(const bf16_t* __restrict__ base, int64_t ld_base, bf16_t* __restrict__ dst,
                                                        int64_t ld_dst, int I, int J, LoraFoldArgs a) {
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
  const int b_row = tid >> 2, b_k = (tid & 3) * 8;          // staging of B: 8 ranks of one row per thread
  const int a_k = tid >> 3, a_c = (tid & 7) * 8;            // staging of A: 8 columns of one rank per thread
  const int fi = lane & 15, fk = (lane >> 4) * 8;           // MFMA operand: row / column fi, ranks fk .. fk + 7

  for (int j = 0; j < J; ++j) {
    const bf16_t* __restrict__ Aj = a.A[j];
    const bf16_t* __restrict__ Bj = a.B[j];
    const int r = a.r[j];
    const bool b_vec = (r & 7) == 0 && (reinterpret_cast<uintptr_t>(Bj) & 15) == 0;      // rows of B_j start on 16 bytes
    f32x4_t acc[4];
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
    const float s = a.s[j];
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int e = 0; e < 4; ++e) tot[n][e] = fmaf(s, acc[n][e], tot[n][e]);
  }

  // accumulator element e of column tile n: row 16 wave + 4 (lane / 16) + e, column 16 n + lane % 16
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int e = 0; e < 4; ++e) sC[(16 * wave + 4 * (lane >> 4) + e) * LF_LDC + 16 * n + fi] = tot[n][e];
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int idx = tid + 256 * c, row = idx >> 3, c8 = (idx & 7) * 8;
    float f[8];
    unpack8(bw[c], f);
    const float* d = &sC[row * LF_LDC + c8];
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] += d[e];
    *reinterpret_cast<u32x4_t*>(dst + (o0 + row) * ld_dst + i0 + c8) = pack8(f);       // the one rounding
  }
}

}  // namespace afx

using namespace afx;

extern "C" {

int afx_lora_fold(const void* base, int64_t ld_base, void* dst, int64_t ld_dst, int32_t O, int32_t I, int32_t J,
                  const void* const* A, const void* const* B, const int32_t* ranks, const float* scales, void* stream) {
  if (!base || !dst) return fail(AFX_E_INVALID, "afx_lora_fold: null base / dst");
  if (J < 0 || J > AFX_LORA_MAX_ADAPTERS) return fail(AFX_E_INVALID, "afx_lora_fold: %d adapters (0 .. %d)", J, AFX_LORA_MAX_ADAPTERS);
  if (J > 0 && (!A || !B || !ranks || !scales)) return fail(AFX_E_INVALID, "afx_lora_fold: null adapter array");
  if (O < 64 || I < 64 || O % 64 || I % 64) return fail(AFX_E_INVALID, "afx_lora_fold: O = %d and I = %d must be positive multiples of 64", O, I);
  if (ld_base < I || ld_dst < I) return fail(AFX_E_INVALID, "afx_lora_fold: leading dimension below I = %d", I);
  if (ld_base % 8 || ld_dst % 8 || ((uintptr_t)base & 15) || ((uintptr_t)dst & 15))
    return fail(AFX_E_INVALID, "afx_lora_fold: base / dst must be 16-byte aligned with leading dimensions that are multiples of 8");
  LoraFoldArgs args{};
  for (int j = 0; j < J; ++j) {
    if (!A[j] || !B[j]) return fail(AFX_E_INVALID, "afx_lora_fold: null A / B of adapter %d", j);
    if (ranks[j] < 1) return fail(AFX_E_INVALID, "afx_lora_fold: rank %d of adapter %d (>= 1)", ranks[j], j);
    if ((uintptr_t)A[j] & 15) return fail(AFX_E_INVALID, "afx_lora_fold: A of adapter %d must be 16-byte aligned", j);
    if ((uintptr_t)B[j] & 1) return fail(AFX_E_INVALID, "afx_lora_fold: B of adapter %d must be 2-byte aligned", j);
    args.A[j] = (const bf16_t*)A[j];
    args.B[j] = (const bf16_t*)B[j];
    args.r[j] = ranks[j];
    args.s[j] = scales[j];
  }
  const uintptr_t b0 = (uintptr_t)base, b1 = b0 + (uintptr_t)(((int64_t)(O - 1) * ld_base + I) * 2);
  const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + (uintptr_t)(((int64_t)(O - 1) * ld_dst + I) * 2);
  if (b0 < d1 && d0 < b1) return fail(AFX_E_INVALID, "afx_lora_fold: dst overlaps base");
  const int64_t tiles = (int64_t)(O / 64) * (I / 64);
  if (tiles > 0x7fffffff) return fail(AFX_E_INVALID, "afx_lora_fold: %lld tiles", (long long)tiles);
  hipLaunchKernelGGL(lora_fold_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)base, ld_base, (bf16_t*)dst,
                     ld_dst, (int)I, (int)J, args);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

}  // extern "C"
