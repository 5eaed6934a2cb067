// HBM-bound helper kernels of the MMDiT trunk and its velocity head (gfx950, wave64; the ArcFlow policy math is afx_policy.hip).
// Everything here streams 16 B per lane and reduces with wave shuffles; fp32 math, bf16 storage.
#include <cstdlib>

#include "afx_common.h"
#include "afx_kernels.h"

namespace afx {

// ------------------------------------------------------------------------------------------------
// AdaLN modulate:  out = LN(x) * (1 + scale[b]) + shift[b]      (LN: no affine, eps 1e-6)
// RMS mode:        out = x * rsqrt(mean(x^2) + 1e-6) * scale    (scale = weight vector)
// One wave per row, D <= 4096, D % 8 == 0; each lane owns chunks lane, lane+64, ... of 8 elements.
constexpr int NM_MAX_CHUNKS = 8;

// Joint mode (scale_txt != nullptr): the rows are the joint [text n_txt | image] token matrix of rows_per_batch = S rows per
// sample and the two streams of a double block carry different modulation vectors -- one launch instead of one per stream.
__global__ __launch_bounds__(256) void norm_modulate_kernel(
    const bf16_t* __restrict__ x, int64_t ldx, bf16_t* __restrict__ out, int64_t ldo, int rows, int D,
    const float* __restrict__ scale, const float* __restrict__ shift, int64_t ldmod, int rows_per_batch,
    int rms, const float* __restrict__ scale_txt, const float* __restrict__ shift_txt, int n_txt) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nchunk = D >> 3;
  const bf16_t* xr = x + (int64_t)row * ldx;
  float v[NM_MAX_CHUNKS][8];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NM_MAX_CHUNKS; ++i) {
    const int c = lane + i * 64;
    if (c < nchunk) {
      const u32x4_t w = *reinterpret_cast<const u32x4_t*>(xr + c * 8);
      unpack8(w, v[i]);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += rms ? v[i][e] * v[i][e] : v[i][e];
    }
  }
  s = wave_sum(s);
  float mean = 0.f, rstd;
  if (rms) {
    rstd = rsqrtf(s / (float)D + 1e-6f);
  } else {
    mean = s / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NM_MAX_CHUNKS; ++i) {
      const int c = lane + i * 64;
      if (c < nchunk) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d = v[i][e] - mean;
          q += d * d;
        }
      }
    }
    q = wave_sum(q);
    rstd = rsqrtf(q / (float)D + 1e-6f);
  }
  const int64_t moff = rms ? 0 : (int64_t)(row / rows_per_batch) * ldmod;
  if (scale_txt != nullptr && row % rows_per_batch < n_txt) {      // wave-uniform: one wave = one row
    scale = scale_txt;
    shift = shift_txt;
  }
  bf16_t* orow = out + (int64_t)row * ldo;
#pragma unroll
  for (int i = 0; i < NM_MAX_CHUNKS; ++i) {
    const int c = lane + i * 64;
    if (c < nchunk) {
      const f32x4_t s0 = *reinterpret_cast<const f32x4_t*>(scale + moff + c * 8);
      const f32x4_t s1 = *reinterpret_cast<const f32x4_t*>(scale + moff + c * 8 + 4);
      const float sc[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
      float r[8];
      if (rms) {
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = v[i][e] * rstd * sc[e];
      } else {
        const f32x4_t h0 = *reinterpret_cast<const f32x4_t*>(shift + moff + c * 8);
        const f32x4_t h1 = *reinterpret_cast<const f32x4_t*>(shift + moff + c * 8 + 4);
        const float sh[8] = {h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = (v[i][e] - mean) * rstd * (1.0f + sc[e]) + sh[e];
      }
      *reinterpret_cast<u32x4_t*>(orow + c * 8) = pack8(r);
    }
  }
}

// LayerNorm + modulate for D = 512 * NCH (3072: both model families), R consecutive rows per wave.  The one-row kernel above reads 8 bytes of
// modulation vector (scale + shift, fp32) for every 2 bytes of x it normalises -- out of L1 / L2, but through the same 64 B/clk address path; here a
// lane keeps (1 + scale, shift) of its NCH chunks in registers across the wave's rows and reloads them only when the (sample, stream) of a row
// differs from the previous one's.  The next row's chunks are requested before the current one is reduced.  Same arithmetic, same order: bit-identical.
// MX8: the row leaves as the next fp8 GEMM's block-scaled operand instead of bf16 (afx_common.h mx_exp / mx_pack8; a lane's chunk i and its 15
// neighbours are one 128-column block): e4m3 bytes to q8[row][.] and one E8M0 byte per block to mx[row][.] -- no quantisation pass behind the LayerNorm.
// QOUT 2: e4m3 bytes with ONE fp32 scale per row (absmax / 448, afx_quant_rows_fp8's format) to q8 / rowscale: a LayerNorm row sits in one wave, so the
// row-wise format is as cheap here as the block-wise one -- and its consumer is the plain fp8 MFMA (the scaled one costs 3-7 % per GEMM).
template <int NCH, int R, int QOUT = 0>
__global__ __launch_bounds__(256) void norm_modulate_rows_kernel(
    const bf16_t* __restrict__ x, int64_t ldx, bf16_t* __restrict__ out, int64_t ldo, int rows,
    const float* __restrict__ scale, const float* __restrict__ shift, int64_t ldmod, int rows_per_batch,
    const float* __restrict__ scale_txt, const float* __restrict__ shift_txt, int n_txt, uint8_t* __restrict__ q8 = nullptr, int64_t ldq = 0,
    uint8_t* __restrict__ mx = nullptr, int64_t ld_mx = 0, float* __restrict__ rowscale = nullptr) {
  constexpr bool MX8 = QOUT == 1;
  constexpr int D = 512 * NCH;
  const int lane = threadIdx.x & 63;
  const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * R;
  if (row0 >= rows) return;
  const int nrows = min(R, rows - row0);
  float sc[NCH][8], sh[NCH][8];
  int key = -1;
  u32x4_t cur[NCH], nxt[NCH];
  {
    const bf16_t* xr = x + (int64_t)row0 * ldx;
#pragma unroll
    for (int i = 0; i < NCH; ++i) cur[i] = *reinterpret_cast<const u32x4_t*>(xr + (lane + i * 64) * 8);
  }
#pragma unroll 1
  for (int rr = 0; rr < nrows; ++rr) {
    const int row = row0 + rr;
    if (rr + 1 < nrows) {
      const bf16_t* xn = x + (int64_t)(row + 1) * ldx;
#pragma unroll
      for (int i = 0; i < NCH; ++i) nxt[i] = *reinterpret_cast<const u32x4_t*>(xn + (lane + i * 64) * 8);
    }
    const int b = row / rows_per_batch;
    const bool txt = scale_txt != nullptr && row - b * rows_per_batch < n_txt;
    const int k = 2 * b + (txt ? 1 : 0);
    if (k != key) {                                              // wave-uniform
      key = k;
      const float* sp = (txt ? scale_txt : scale) + (int64_t)b * ldmod;
      const float* hp = (txt ? shift_txt : shift) + (int64_t)b * ldmod;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int c = (lane + i * 64) * 8;
        const f32x4_t s0 = *reinterpret_cast<const f32x4_t*>(sp + c), s1 = *reinterpret_cast<const f32x4_t*>(sp + c + 4);
        const f32x4_t h0 = *reinterpret_cast<const f32x4_t*>(hp + c), h1 = *reinterpret_cast<const f32x4_t*>(hp + c + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          sc[i][e] = 1.0f + s0[e]; sc[i][4 + e] = 1.0f + s1[e];
          sh[i][e] = h0[e];        sh[i][4 + e] = h1[e];
        }
      }
    }
    float v[NCH][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      unpack8(cur[i], v[i]);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += v[i][e];
    }
    s = wave_sum(s);
    const float mean = s / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = v[i][e] - mean;
        q += d * d;
      }
    q = wave_sum(q);
    const float rstd = rsqrtf(q / (float)D + 1e-6f);
    bf16_t* orow = out + (int64_t)row * ldo;
    if constexpr (QOUT == 2) {
      float amax = 0.f;
#pragma unroll
      for (int i = 0; i < NCH; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          v[i][e] = (v[i][e] - mean) * rstd * sc[i][e] + sh[i][e];
          amax = fmaxf(amax, fabsf(v[i][e]));
        }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
      const float s_ = fmaxf(amax, 1e-12f) / 448.0f;
      const float inv = 1.0f / s_;
      if (lane == 0) rowscale[row] = s_;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        uint32_t w0, w1;
        mx_pack8(v[i], inv, w0, w1);
        *reinterpret_cast<u32x2_t*>(q8 + (int64_t)row * ldq + (lane + i * 64) * 8) = (u32x2_t){w0, w1};
      }
    } else
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      float r[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] = (v[i][e] - mean) * rstd * sc[i][e] + sh[i][e];
      if constexpr (MX8) {
        float amax = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(r[e]));
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
        const int eb = mx_exp(amax);
        uint32_t w0, w1;
        mx_pack8(r, mx_inv(eb), w0, w1);
        *reinterpret_cast<u32x2_t*>(q8 + (int64_t)row * ldq + (lane + i * 64) * 8) = (u32x2_t){w0, w1};
        if ((lane & 15) == 0) mx[(int64_t)row * ld_mx + 4 * i + (lane >> 4)] = (uint8_t)eb;
      } else
      *reinterpret_cast<u32x4_t*>(orow + (lane + i * 64) * 8) = pack8(r);
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) cur[i] = nxt[i];
  }
}

static int nm_rows_per_wave() {
  static int r = -1;
  if (r < 0) {
    const char* e = getenv("AFX_NM_ROWS");
    r = e ? atoi(e) : 2;            // 2 rows per wave: 16.4 -> 14.5 us at 4608 x 3072 (4: 15.1; 0 = the one-row kernel)
  }
  return r;
}

// true when the multi-row kernel took the launch
static bool launch_norm_modulate_rows(const uint16_t* x, int64_t ldx, uint16_t* out, int64_t ldo, int rows, int D, const float* scale,
                                      const float* shift, int64_t ldmod, int rows_per_batch, const float* scale_txt, const float* shift_txt,
                                      int n_txt, hipStream_t stream, uint8_t* q8 = nullptr, int64_t ldq = 0, uint8_t* mx = nullptr, int64_t ld_mx = 0,
                                      float* rowscale = nullptr) {
  const int R = nm_rows_per_wave();
  if (D != 3072 || rows < 1024 || (R != 2 && R != 4)) return false;
  const dim3 grid((rows + 4 * R - 1) / (4 * R));
  if (q8 != nullptr) {
    if (R != 2) return false;
    if (rowscale != nullptr)
      hipLaunchKernelGGL((norm_modulate_rows_kernel<6, 2, 2>), grid, dim3(256), 0, stream, x, ldx, out, ldo, rows, scale, shift, ldmod, rows_per_batch,
                         scale_txt, shift_txt, n_txt, q8, ldq, (uint8_t*)nullptr, (int64_t)0, rowscale);
    else
      hipLaunchKernelGGL((norm_modulate_rows_kernel<6, 2, 1>), grid, dim3(256), 0, stream, x, ldx, out, ldo, rows, scale, shift, ldmod, rows_per_batch,
                         scale_txt, shift_txt, n_txt, q8, ldq, mx, ld_mx, (float*)nullptr);
    return true;
  }
  if (R == 2)
    hipLaunchKernelGGL((norm_modulate_rows_kernel<6, 2, 0>), grid, dim3(256), 0, stream, x, ldx, out, ldo, rows, scale, shift, ldmod, rows_per_batch,
                       scale_txt, shift_txt, n_txt);
  else
    hipLaunchKernelGGL((norm_modulate_rows_kernel<6, 4, 0>), grid, dim3(256), 0, stream, x, ldx, out, ldo, rows, scale, shift, ldmod, rows_per_batch,
                       scale_txt, shift_txt, n_txt);
  return true;
}

hipError_t launch_norm_modulate(const uint16_t* x, int64_t ldx, uint16_t* out, int64_t ldo, int rows,
                                int D, const float* scale, const float* shift, int64_t ldmod,
                                int rows_per_batch, int rms, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  if (D > NM_MAX_CHUNKS * 512 || (D & 7)) return hipErrorInvalidValue;
  if (!rms && launch_norm_modulate_rows(x, ldx, out, ldo, rows, D, scale, shift, ldmod, rows_per_batch > 0 ? rows_per_batch : rows, nullptr, nullptr, 0,
                                        stream))
    return hipGetLastError();
  hipLaunchKernelGGL(norm_modulate_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, x, ldx, out, ldo, rows,
                     D, scale, shift, ldmod, rows_per_batch > 0 ? rows_per_batch : rows, rms, (const float*)nullptr,
                     (const float*)nullptr, 0);
  return hipGetLastError();
}

// LN + modulate straight into the next fp8 GEMM's operand (q8 [rows, ldq] e4m3; scale_txt may be null: one stream) -- block-scaled (mx [rows, ld_mx]
// E8M0 bytes) or, with rowscale != nullptr, one fp32 scale per row (rowscale [rows]; mx unused).  *fused = false: this shape has no fused kernel,
// nothing was launched -- the caller runs the bf16 kernel and a quantisation pass.
hipError_t launch_norm_modulate_mx8(const uint16_t* x, int64_t ldx, uint8_t* q8, int64_t ldq, uint8_t* mx, int64_t ld_mx, int rows, int D,
                                    const float* scale, const float* shift, const float* scale_txt, const float* shift_txt, int64_t ldmod, int S,
                                    int n_txt, hipStream_t stream, bool* fused, float* rowscale) {
  *fused = rows > 0 && launch_norm_modulate_rows(x, ldx, nullptr, 0, rows, D, scale, shift, ldmod, S, scale_txt, shift_txt, n_txt, stream, q8, ldq, mx, ld_mx,
                                                 rowscale);
  return hipGetLastError();
}

// LN + modulate of a whole joint token matrix [B][text T | image N] in ONE launch: image rows use (scale, shift), text rows
// (scale_txt, shift_txt); sample b's vectors sit at + b * ldmod.
hipError_t launch_norm_modulate_joint(const uint16_t* x, int64_t ldx, uint16_t* out, int64_t ldo, int rows, int D, const float* scale,
                                      const float* shift, const float* scale_txt, const float* shift_txt, int64_t ldmod, int S,
                                      int n_txt, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  if (D > NM_MAX_CHUNKS * 512 || (D & 7) || S <= 0) return hipErrorInvalidValue;
  if (launch_norm_modulate_rows(x, ldx, out, ldo, rows, D, scale, shift, ldmod, S, scale_txt, shift_txt, n_txt, stream)) return hipGetLastError();
  hipLaunchKernelGGL(norm_modulate_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, x, ldx, out, ldo, rows, D, scale, shift, ldmod,
                     S, 0, scale_txt, shift_txt, n_txt);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// In-place per-head RMSNorm(128, weight) + interleaved-pair RoPE.  16 lanes x 8 elements = one
// (token, head); the 4 rotation pairs of a lane stay inside its own 16-byte chunk.
// blockIdx.y selects one of up to two tensors handled by the same launch (k and q of a block: same rows, different column
// range and norm weights).
struct QkRopeArgs { bf16_t* x[2]; const float* w_txt[2]; const float* w_img[2]; };

__global__ __launch_bounds__(256) void qk_norm_rope_kernel(
    const QkRopeArgs a, int64_t ldx, const float* __restrict__ cos_t, const float* __restrict__ sin_t, int S, int n_txt, int H,
    int64_t total) {
  bf16_t* __restrict__ x = a.x[blockIdx.y];
  const float* __restrict__ w_txt = a.w_txt[blockIdx.y];
  const float* __restrict__ w_img = a.w_img[blockIdx.y];
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;     // (row, head, chunk)
  if (g >= total) return;                                         // total % 16 == 0: whole groups exit together
  const int c = (int)(g & 15);
  const int64_t th = g >> 4;
  const int h = (int)(th % H);
  const int64_t row = th / H;
  const int s = (int)(row % S);
  bf16_t* p = x + row * ldx + h * 128 + c * 8;
  float v[8];
  unpack8(*reinterpret_cast<const u32x4_t*>(p), v);
  float ss = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) ss += v[e] * v[e];
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  const float rstd = rsqrtf(ss * (1.0f / 128.0f) + 1e-6f);
  const float* w = (s < n_txt ? w_txt : w_img) + c * 8;
  const f32x4_t w0 = *reinterpret_cast<const f32x4_t*>(w);
  const f32x4_t w1 = *reinterpret_cast<const f32x4_t*>(w + 4);
  const float wv[8] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]};
  const f32x4_t cs = *reinterpret_cast<const f32x4_t*>(cos_t + (int64_t)s * 64 + c * 4);
  const f32x4_t sn = *reinterpret_cast<const f32x4_t*>(sin_t + (int64_t)s * 64 + c * 4);
  float r[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float a = v[2 * i] * rstd * wv[2 * i];
    const float b = v[2 * i + 1] * rstd * wv[2 * i + 1];
    r[2 * i] = a * cs[i] - b * sn[i];
    r[2 * i + 1] = a * sn[i] + b * cs[i];
  }
  *reinterpret_cast<u32x4_t*>(p) = pack8(r);
}

hipError_t launch_qk_norm_rope(uint16_t* x, int64_t ldx, const float* w_txt, const float* w_img,
                               const float* cos_t, const float* sin_t, int B, int S, int n_txt, int H,
                               hipStream_t stream) {
  const int64_t total = (int64_t)B * S * H * 16;
  if (total == 0) return hipSuccess;
  QkRopeArgs a{};
  a.x[0] = x; a.w_txt[0] = w_txt; a.w_img[0] = w_img;
  hipLaunchKernelGGL(qk_norm_rope_kernel, dim3((unsigned)((total + 255) / 256), 1), dim3(256), 0, stream, a, ldx, cos_t, sin_t, S,
                     n_txt, H, total);
  return hipGetLastError();
}

// k and q of one block in a single launch
hipError_t launch_qk_norm_rope2(uint16_t* xk, uint16_t* xq, int64_t ldx, const float* wk_txt, const float* wk_img, const float* wq_txt,
                                const float* wq_img, const float* cos_t, const float* sin_t, int B, int S, int n_txt, int H,
                                hipStream_t stream) {
  const int64_t total = (int64_t)B * S * H * 16;
  if (total == 0) return hipSuccess;
  QkRopeArgs a{};
  a.x[0] = xk; a.w_txt[0] = wk_txt; a.w_img[0] = wk_img;
  a.x[1] = xq; a.w_txt[1] = wq_txt; a.w_img[1] = wq_img;
  hipLaunchKernelGGL(qk_norm_rope_kernel, dim3((unsigned)((total + 255) / 256), 2), dim3(256), 0, stream, a, ldx, cos_t, sin_t, S,
                     n_txt, H, total);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Skinny GEMV  y[b,n] (+)= act(sum_k x[b,k] W[n,k] + bias[n])  -- one wave per weight row, the row is
// streamed once (16 B per lane per load) and reused for every batch row (B <= 8).  HBM-bound on W.
constexpr int GEMV_MAXB = 8;

__global__ __launch_bounds__(256) void gemv_kernel(const float* __restrict__ x, const bf16_t* __restrict__ W,
                                                   const bf16_t* __restrict__ bias, float* __restrict__ y,
                                                   int B, int N, int K, int act, int accumulate, int64_t ldy) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const bf16_t* wr = W + (int64_t)n * K;
  float acc[GEMV_MAXB];
#pragma unroll
  for (int b = 0; b < GEMV_MAXB; ++b) acc[b] = 0.f;
  for (int c = lane; c < (K >> 3); c += 64) {
    float w[8];
    unpack8(*reinterpret_cast<const u32x4_t*>(wr + c * 8), w);
#pragma unroll
    for (int b = 0; b < GEMV_MAXB; ++b) {
      if (b < B) {
        const f32x4_t x0 = *reinterpret_cast<const f32x4_t*>(x + (int64_t)b * K + c * 8);
        const f32x4_t x1 = *reinterpret_cast<const f32x4_t*>(x + (int64_t)b * K + c * 8 + 4);
        acc[b] += w[0] * x0[0] + w[1] * x0[1] + w[2] * x0[2] + w[3] * x0[3] + w[4] * x1[0] + w[5] * x1[1] +
                  w[6] * x1[2] + w[7] * x1[3];
      }
    }
  }
  const float bv = bias ? bf16_to_f32(bias[n]) : 0.f;
#pragma unroll
  for (int b = 0; b < GEMV_MAXB; ++b) {
    if (b < B) {
      float r = wave_sum(acc[b]) + bv;
      if (act == 1) r = silu(r);
      if (lane == 0) {
        float* yp = y + (int64_t)b * ldy + n;
        *yp = accumulate ? (*yp + r) : r;
      }
    }
  }
}

hipError_t launch_gemv(const float* x, const uint16_t* W, const uint16_t* bias, float* y, int B, int N,
                       int K, int act, int accumulate, hipStream_t stream, int64_t ldy) {
  if (ldy <= 0) ldy = N;
  if (B > GEMV_MAXB || (K & 7)) return hipErrorInvalidValue;
  if (N == 0 || B == 0) return hipSuccess;
  hipLaunchKernelGGL(gemv_kernel, dim3((N + 3) / 4), dim3(256), 0, stream, x, W, bias, y, B, N, K, act, accumulate, ldy);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Timesteps(256, flip_sin_to_cos=True, downscale_freq_shift=0): out[b] = [cos(a) | sin(a)],
// a_i = scale * t_b * exp(-ln(1e4) * i / 128).
// cast_mode models the reference's explicit casts of the conditioning scalar to the trunk dtype (bf16):
//   1  FLUX  `timestep.to(hidden_states.dtype) * 1000` (arcflux.py:160-162): t and the product are bf16 tensors -- sigma 0.76190
//            reaches the sinusoid as 760.0, guidance 3.5 as 3504;
//   2  Qwen  `timestep.to(hidden_states.dtype)` (arcqwen.py:128), the x1000 is Timesteps(scale=1000) in fp32;
//   0  none (fp32 scalar).
__global__ void sincos_kernel(const float* __restrict__ t, float scale, float* __restrict__ out, int B, int cast_mode) {
  const int i = threadIdx.x;        // 0..127
  const int b = blockIdx.x;
  if (b >= B) return;
  const float f = expf(-9.210340371976184f * (float)i / 128.0f);
  float tb = t[b];
  if (cast_mode != 0) tb = bf16_to_f32(f32_to_bf16(tb));
  float a;
  if (cast_mode == 1) a = bf16_to_f32(f32_to_bf16(tb * scale)) * f;
  else a = scale * (tb * f);
  out[b * 256 + i] = cosf(a);
  out[b * 256 + 128 + i] = sinf(a);
}
hipError_t launch_sincos(const float* t, float scale, float* out, int B, int cast_mode, hipStream_t stream) {
  hipLaunchKernelGGL(sincos_kernel, dim3(B), dim3(128), 0, stream, t, scale, out, B, cast_mode);
  return hipGetLastError();
}

__global__ void silu_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = silu(x[i]);
}
hipError_t launch_silu(const float* x, float* y, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(silu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, y, n);
  return hipGetLastError();
}

__global__ void bf16_to_f32_kernel(const bf16_t* __restrict__ x, float* __restrict__ y, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = bf16_to_f32(x[i]);
}
hipError_t launch_bf16_to_f32(const uint16_t* x, float* y, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(bf16_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, y, n);
  return hipGetLastError();
}

// rows x cols bf16 copy between strided buffers (cols % 8 == 0)
__global__ void copy_rows_kernel(const bf16_t* __restrict__ src, int64_t lds_, bf16_t* __restrict__ dst,
                                 int64_t ldd, int64_t rows, int cols) {
  const int cpr = cols >> 3;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= rows * cpr) return;
  const int64_t r = g / cpr;
  const int c = (int)(g % cpr);
  *reinterpret_cast<u32x4_t*>(dst + r * ldd + c * 8) = *reinterpret_cast<const u32x4_t*>(src + r * lds_ + c * 8);
}
hipError_t launch_copy_rows(const uint16_t* src, int64_t lds_, uint16_t* dst, int64_t ldd, int64_t rows,
                            int cols, hipStream_t stream) {
  const int64_t total = rows * (cols >> 3);
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(copy_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, src, lds_,
                     dst, ldd, rows, cols);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Velocity head split (arcflux.py:243-249): head row = [means K*ch | logw K*lw | logg (K-1)*lw | pad];
// means and logg are copied, logw gets log_softmax over K (fp32 math on the bf16 logits, bf16 out).
__global__ __launch_bounds__(256) void head_split_kernel(const bf16_t* __restrict__ head, int64_t ldh,
                                                         bf16_t* __restrict__ means, bf16_t* __restrict__ logw,
                                                         bf16_t* __restrict__ logg, int64_t rows, int K, int ch,
                                                         int lw) {
  const int64_t row = blockIdx.x;
  const bf16_t* hr = head + row * ldh;
  const int nm = K * ch, nw = K * lw, ng = (K - 1) * lw;
  for (int i = threadIdx.x; i < nm; i += 256) means[row * nm + i] = hr[i];
  for (int i = threadIdx.x; i < ng; i += 256) logg[row * ng + i] = hr[nm + nw + i];
  if (threadIdx.x < lw) {
    const int p = threadIdx.x;
    float mx = -INFINITY;
    for (int k = 0; k < K; ++k) mx = fmaxf(mx, bf16_to_f32(hr[nm + k * lw + p]));
    float se = 0.f;
    for (int k = 0; k < K; ++k) se += expf(bf16_to_f32(hr[nm + k * lw + p]) - mx);
    const float lse = mx + logf(se);
    for (int k = 0; k < K; ++k) logw[row * nw + k * lw + p] = f32_to_bf16(bf16_to_f32(hr[nm + k * lw + p]) - lse);
  }
}
hipError_t launch_head_split(const uint16_t* head, int64_t ldh, uint16_t* means, uint16_t* logw,
                             uint16_t* logg, int64_t rows, int K, int ch, int lw, hipStream_t stream) {
  if (rows == 0) return hipSuccess;
  hipLaunchKernelGGL(head_split_kernel, dim3((unsigned)rows), dim3(256), 0, stream, head, ldh, means, logw, logg,
                     rows, K, ch, lw);
  return hipGetLastError();
}

}  // namespace afx
