// Training-time evaluation (student against teacher samples): the per-sample scoring passes, fp64 and bit-reproducible on the reduction
// scheme of afx_reduce.h.
//   * sample_score_partial_kernel: per-sample agreement sums of two batches, sum (a-b)^2, sum a^2, sum b^2, sum a b over the n elements
//     of a sample: the fixed partition of reduce_parts(), elements widened to fp64 (after the optional image-range transform in fp32),
//     one slot of 4 doubles per work-group, the slots added in index order by the second launch (ordered_finish_kernel).  16 B per lane
//     and operand: 8 bf16 or 4 fp32.
//   * image_ssim_partial_kernel<BF16, MASKED> / image_ssim_finish_kernel: per-sample sum of the structural similarity of two image
//     batches over every valid 11 x 11 Gaussian window (decoded images), fp64 throughout: one work-group and one slot per tile of
//     windows, the slots added in a fixed order by the second launch.  Scheme and LDS use at the kernel.
//   * sample_score_masked_partial_kernel and the MASKED SSIM instances: the two scoring passes weighted by an edit's mask, a repainted
//     (weight m) and a kept (weight 1 - m) set of sums each, on the same partitions and the same ordered second launches.  Weight maps and
//     LDS use at the kernels.
#include <algorithm>
#include <climits>
#include <cmath>

#include "afx_api_util.h"
#include "afx_common.h"
#include "afx_reduce.h"

namespace afx {

// The image range val_step produces: clamp(v / 2 + 0.5, 0, 1) in fp32 (v / 2 is exact, so a contracted multiply-add gives the same value).
AFX_DEV float unit_range(float v) { return fminf(fmaxf(v * 0.5f + 0.5f, 0.f), 1.f); }

// One unit = 16 B of an operand: 8 bf16 or 4 fp32 elements (n % 64 == 0: a unit never straddles two samples).
template <bool BF16>
AFX_DEV void load_unit(const void* p, int64_t unit, float (&v)[BF16 ? 8 : 4]) {
  if constexpr (BF16) {
    unpack8(*reinterpret_cast<const u32x4_t*>(reinterpret_cast<const bf16_t*>(p) + unit * 8), v);
  } else {
    const f32x4_t t = *reinterpret_cast<const f32x4_t*>(reinterpret_cast<const float*>(p) + unit * 4);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  }
}

// grid (parts, B): work-group w of sample s owns the units [w upw, min((w + 1) upw, units_per_sample)) and writes
// ws[(s parts + w) 4 + {0, 1, 2, 3}] = sum (a-b)^2, sum a^2, sum b^2, sum a b.  Every element is widened to fp64 first; the products
// of two widened fp32 values are exact, the difference and its square round once each.
template <bool BF16>
__global__ __launch_bounds__(256) void sample_score_partial_kernel(const void* __restrict__ a, const void* __restrict__ b, int transform,
                                                                   double* __restrict__ ws, int64_t units_per_sample, int64_t upw) {
  constexpr int E = BF16 ? 8 : 4;
  const int64_t s = blockIdx.y;
  const int64_t begin = (int64_t)blockIdx.x * upw;
  const int64_t end = begin + upw < units_per_sample ? begin + upw : units_per_sample;
  const int64_t base = s * units_per_sample;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t u = begin + threadIdx.x; u < end; u += 256) {
    float p[E], q[E];
    load_unit<BF16>(a, base + u, p);
    load_unit<BF16>(b, base + u, q);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const double x = (double)(transform ? unit_range(p[e]) : p[e]);
      const double y = (double)(transform ? unit_range(q[e]) : q[e]);
      const double d = x - y;
      acc[0] += d * d;
      acc[1] += x * x;
      acc[2] += y * y;
      acc[3] += x * y;
    }
  }
  // an empty work-group (upw rounded up) writes zeros: every slot the finish reads is written
  block_slot_sums<4>(acc, ws + (s * gridDim.x + blockIdx.x) * 4);
}

// The masked agreement sums (training-time evaluation of edits: how the student repaints the masked region against the teacher).  A sample
// is viewed as [G, P, R] and the mask as [P, Q], Q | R: element i takes the weight m[(i / R) % P, i % Q]  (i % R % Q == i % Q).  Packed
// latents [N, 64] with the [N, 4] operand of edit_blend_kernel: G = 1, P = N, R = 64, Q = 4 -- element e of token t reads m[t, e & 3], that
// kernel's map.  Decoded images [C, H, W] with a [1, H, W] mask: G = C, P = H W, R = Q = 1.
// grid (parts, B), the partition of sample_score_partial_kernel: work-group w of sample s owns the units [w upw, min((w + 1) upw,
// units_per_sample)) and writes ws[(s parts + w) 10 + 5 g + {0..4}] = sum w, sum w d^2, sum w a^2, sum w b^2, sum w a b, region g = 0
// with w = m (repainted), g = 1 with w = 1 - m formed in fp64 (kept).  d, the squares and the product are sample_score_partial_kernel's
// (x x, y y, x y exact); the square of d takes its weight on one factor, fma(w d, d, acc), so that w = 1 is that kernel's own
// fma(d, d, acc) bit for bit; contraction is off and every multiply-add is written out, so the compiler fuses nothing else.
// A lane keeps (p, r, q) = ((i / R) % P, i % R, i % Q) of its unit's first element and moves it by 256 units per round with adds and
// compares: three divisions per lane, none in the loop.  The mask is read 4 B per element through the caches (0.0625 B per element from
// memory in the latent form, 4 / C B in the image form).
template <bool BF16>
__global__ __launch_bounds__(256) void sample_score_masked_partial_kernel(const void* __restrict__ a, const void* __restrict__ b,
                                                                          const float* __restrict__ mask, int transform, double* __restrict__ ws,
                                                                          int64_t units_per_sample, int64_t upw, int64_t mask_stride, uint32_t P,
                                                                          uint32_t R, uint32_t Q) {
#pragma clang fp contract(off)
  constexpr int E = BF16 ? 8 : 4;
  const int64_t s = blockIdx.y;
  const int64_t begin = (int64_t)blockIdx.x * upw;
  const int64_t end = begin + upw < units_per_sample ? begin + upw : units_per_sample;
  const int64_t base = s * units_per_sample;
  const float* __restrict__ mrow = mask + s * mask_stride;
  const uint32_t first = (uint32_t)(begin + threadIdx.x) * E;          // n < 2^31 (checked by the entry): an index fits 32 bits
  uint32_t p0 = (first / R) % P, r0 = first % R, q0 = first % Q;
  const uint32_t step = 256 * E, sp = (step / R) % P, sr = step % R, sq = step % Q;
  double acc[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t u = begin + threadIdx.x; u < end; u += 256) {
    float f[E], h[E];
    load_unit<BF16>(a, base + u, f);
    load_unit<BF16>(b, base + u, h);
    uint32_t p = p0, r = r0, q = q0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const double w = (double)mrow[p * Q + q], k = 1.0 - w;
      const double x = (double)(transform ? unit_range(f[e]) : f[e]);
      const double y = (double)(transform ? unit_range(h[e]) : h[e]);
      const double d = x - y, xx = x * x, yy = y * y, xy = x * y;
      acc[0] += w;
      acc[1] = fma(w * d, d, acc[1]);
      acc[2] = fma(w, xx, acc[2]);
      acc[3] = fma(w, yy, acc[3]);
      acc[4] = fma(w, xy, acc[4]);
      acc[5] += k;
      acc[6] = fma(k * d, d, acc[6]);
      acc[7] = fma(k, xx, acc[7]);
      acc[8] = fma(k, yy, acc[8]);
      acc[9] = fma(k, xy, acc[9]);
      q = q + 1 == Q ? 0 : q + 1;
      if (++r == R) {
        r = 0;
        p = p + 1 == P ? 0 : p + 1;
      }
    }
    q0 += sq;
    if (q0 >= Q) q0 -= Q;
    r0 += sr;
    p0 += sp;
    if (r0 >= R) {
      r0 -= R;
      ++p0;
    }
    if (p0 >= P) p0 -= P;          // sp < P and one carry: p0 < 2 P
  }
  // an empty work-group (upw rounded up) writes zeros: every slot the finish reads is written
  block_slot_sums<10>(acc, ws + (s * gridDim.x + blockIdx.x) * 10);
}

// ---- SSIM of two image batches (Wang et al. 2004: 11-tap Gaussian window, sigma 1.5, "valid" windows only) -----------------------------
// One work-group = a tile of SSIM_TW x SSIM_TH windows of one (sample, channel) plane.  The (SSIM_TW + 10) x (SSIM_TH + 10) inputs of both
// images are staged in LDS as the fp32 values the transform leaves (widening is exact, so they are widened where they are read); the
// horizontal 11-tap pass of a, b, a a, a b, b b goes to LDS as fp64; the vertical pass, the ratio and the sums are fp64 in registers.
// Positions past the right / bottom edge of the image are staged as zeros and their windows are not counted.
constexpr int SSIM_TAPS = 11, SSIM_TW = 32, SSIM_TH = 16;
constexpr int SSIM_IW = SSIM_TW + SSIM_TAPS - 1, SSIM_IH = SSIM_TH + SSIM_TAPS - 1;          // 42 x 26 staged inputs per image

struct ssim_taps_t { double g[SSIM_TAPS]; };          // the normalised 1-D window, built in fp64 by the host

// The ratio of one window.  The three central moments come from the same sequence of operations (multiply, subtract: contraction is
// off, or the compiler would fuse some products into the additions and not others), so a == b gives num == den bit for bit and 1.0.
AFX_DEV double ssim_ratio(double mu_a, double mu_b, double e_aa, double e_ab, double e_bb, double c1, double c2) {
#pragma clang fp contract(off)
  const double p_aa = mu_a * mu_a, p_ab = mu_a * mu_b, p_bb = mu_b * mu_b;
  const double s_aa = e_aa - p_aa, s_ab = e_ab - p_ab, s_bb = e_bb - p_bb;
  const double num = (2.0 * p_ab + c1) * (2.0 * s_ab + c2);
  const double den = ((p_aa + p_bb) + c1) * ((s_aa + s_bb) + c2);
  return num / den;
}

// grid (C tiles, B), tiles = tiles_x tiles_y, K = MASKED ? 4 : 1 sums per slot: work-group (ch tiles + tile) of sample s writes
// ws[(s gridDim.x + blockIdx.x) K + {0..K-1}] over the valid windows of its tile:
//   plain    the sum of ssim
//   MASKED   sum w ssim, sum w, sum (1 - w) ssim, sum (1 - w)     (training-time evaluation of edits)
// MASKED takes the mask [Bm, 1, H, W] (fp32, shared by the channels) as a sixth quantity: staged beside the two images, taken through the
// same horizontal and vertical 11-tap passes.  A window's weight w is the Gaussian-weighted mean of the mask over the window's own
// 11 x 11 support, clamped to [0, 1] in fp64 (the taps sum to 1 within a few ulp); the ratio is ssim_ratio() on the same five moments
// formed by the same fma chains, so a == b still gives exactly 1.0 per window and then sum w ssim == sum w bit for bit.
// LDS, plain: 2 x 26 x 43 x 4 B staged inputs + 5 x 26 x 32 x 8 B horizontal sums + 32 B = 42256 B, three work-groups per CU.  MASKED:
// the third staged plane and the sixth row of sums cost 4472 + 6656 = 11128 B (+ 96 B for four sums per wave), 53480 B, 53504 B as laid
// out (52.3 KB); three work-groups still fit the CU's 160 KB (3 x 53504 = 160512 <= 163840), so the mask needs no pass of its own.  The
// plain instances declare neither.  138 VGPRs MASKED (3 waves per SIMD: the same three work-groups),
// 114 plain, no scratch.
template <bool BF16, bool MASKED>
__global__ __launch_bounds__(256) void image_ssim_partial_kernel(const void* __restrict__ a, const void* __restrict__ b,
                                                                 const float* __restrict__ mask, int transform, ssim_taps_t taps, double c1,
                                                                 double c2, double* __restrict__ ws, int H, int W, int tiles_x, int tiles,
                                                                 int64_t mask_stride) {
  constexpr int NQ = MASKED ? 6 : 5, K = MASKED ? 4 : 1;
  __shared__ float st[MASKED ? 3 : 2][SSIM_IH][SSIM_IW + 1];          // a, b and, MASKED, the mask
  __shared__ double hq[NQ][SSIM_IH][SSIM_TW];
  const int tile = blockIdx.x % tiles, ch = blockIdx.x / tiles, C = gridDim.x / tiles;
  const int x0 = (tile % tiles_x) * SSIM_TW, y0 = (tile / tiles_x) * SSIM_TH;
  const int64_t base = ((int64_t)blockIdx.y * C + ch) * H * W;
  for (int i = threadIdx.x; i < SSIM_IH * SSIM_IW; i += 256) {
    const int r = i / SSIM_IW, c = i % SSIM_IW;
    const int y = y0 + r, x = x0 + c;
    float p = 0.f, q = 0.f, m = 0.f;
    if (y < H && x < W) {
      const int64_t at = base + (int64_t)y * W + x;
      if constexpr (BF16) {
        p = bf16_to_f32(reinterpret_cast<const bf16_t*>(a)[at]);
        q = bf16_to_f32(reinterpret_cast<const bf16_t*>(b)[at]);
      } else {
        p = reinterpret_cast<const float*>(a)[at];
        q = reinterpret_cast<const float*>(b)[at];
      }
      if (transform) { p = unit_range(p); q = unit_range(q); }
      if constexpr (MASKED) m = mask[(int64_t)blockIdx.y * mask_stride + (int64_t)y * W + x];
    }
    st[0][r][c] = p;
    st[1][r][c] = q;
    if constexpr (MASKED) st[2][r][c] = m;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SSIM_IH * SSIM_TW; i += 256) {          // horizontal pass: x x, x y, y y are exact in fp64
    const int r = i / SSIM_TW, c = i % SSIM_TW;
    double h[NQ] = {};
#pragma unroll
    for (int j = 0; j < SSIM_TAPS; ++j) {
      const double x = (double)st[0][r][c + j], y = (double)st[1][r][c + j], g = taps.g[j];
      h[0] = fma(g, x, h[0]);
      h[1] = fma(g, y, h[1]);
      h[2] = fma(g, x * x, h[2]);
      h[3] = fma(g, x * y, h[3]);
      h[4] = fma(g, y * y, h[4]);
      if constexpr (MASKED) h[5] = fma(g, (double)st[2][r][c + j], h[5]);
    }
#pragma unroll
    for (int k = 0; k < NQ; ++k) hq[k][r][c] = h[k];
  }
  __syncthreads();
  double acc[K] = {};
  for (int i = threadIdx.x; i < SSIM_TH * SSIM_TW; i += 256) {          // vertical pass, ratio, weight; a lane adds its windows in index order
    const int r = i / SSIM_TW, c = i % SSIM_TW;
    if (y0 + r >= H - (SSIM_TAPS - 1) || x0 + c >= W - (SSIM_TAPS - 1)) continue;
    double v[NQ] = {};
#pragma unroll
    for (int j = 0; j < SSIM_TAPS; ++j) {
#pragma unroll
      for (int k = 0; k < NQ; ++k) v[k] = fma(taps.g[j], hq[k][r + j][c], v[k]);
    }
    const double ratio = ssim_ratio(v[0], v[1], v[2], v[3], v[4], c1, c2);
    if constexpr (MASKED) {
      const double w = fmin(fmax(v[NQ - 1], 0.0), 1.0), k = 1.0 - w;
      acc[0] = fma(w, ratio, acc[0]);
      acc[1] += w;
      acc[2] = fma(k, ratio, acc[2]);
      acc[K - 1] += k;
    } else {
      acc[0] += ratio;
    }
  }
  block_slot_sums<K>(acc, ws + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * K);
}

// grid (B, K), one wave per (sample, sum): lane l adds the slots l, l + 64, ... of its sample in index order, then the 64 lanes are
// added by the shuffle tree -- an order that depends on `parts` alone
__global__ __launch_bounds__(64) void image_ssim_finish_kernel(const double* __restrict__ ws, double* __restrict__ out, int parts) {
  const int64_t s = blockIdx.x;
  const int k = blockIdx.y, K = gridDim.y;
  double v = 0.0;
  for (int w = threadIdx.x; w < parts; w += 64) v += ws[(s * parts + w) * K + k];
  v = wave_sum_f64(v);
  if (threadIdx.x == 0) out[s * K + k] = v;
}

}  // namespace afx

using namespace afx;

// What the four scoring entries refuse alike, after their own shape checks: a NULL operand (mask only where `masked`), the dtype, the
// transform, the alignment (a and b to ab_align bytes; 0: to their element) and a workspace below `need` bytes.
static int score_refusals(const char* name, const void* a, const void* b, const float* mask, bool masked, int32_t dtype, int32_t transform,
                          const double* out, const void* ws, int64_t ws_bytes, int64_t need, int ab_align) {
  if (!a || !b || (masked && !mask) || !out || !ws) return fail(AFX_E_INVALID, "null argument to %s", name);
  if (dtype != AFX_DT_BF16 && dtype != AFX_DT_F32) return fail(AFX_E_INVALID, "%s: dtype must be AFX_DT_BF16 or AFX_DT_F32", name);
  if (transform != 0 && transform != 1) return fail(AFX_E_INVALID, "%s: transform must be 0 or 1", name);
  const uintptr_t ab = (ab_align ? ab_align : dtype == AFX_DT_BF16 ? 2 : 4) - 1;
  if (((uintptr_t)a & ab) || ((uintptr_t)b & ab) || ((uintptr_t)mask & 3) || ((uintptr_t)out & 7) || ((uintptr_t)ws & 7))
    return fail(AFX_E_INVALID, "%s: a and b must be aligned to %s, %sout and ws 8-byte aligned", name, ab_align ? "16 bytes" : "their element",
                masked ? "mask 4-byte, " : "");
  if (ws_bytes < need) return fail(AFX_E_INVALID, "%s: workspace smaller than %s_ws_bytes()", name, name);
  return AFX_OK;
}

// work-groups (= workspace slots) per sample of the SSIM pass: one per tile of windows and channel -- a function of the shape alone
static inline int64_t ssim_parts(int32_t C, int32_t H, int32_t W, int* tiles_x, int* tiles) {
  const int64_t tx = ((int64_t)W - (SSIM_TAPS - 1) + SSIM_TW - 1) / SSIM_TW, ty = ((int64_t)H - (SSIM_TAPS - 1) + SSIM_TH - 1) / SSIM_TH;
  if (tiles_x) *tiles_x = (int)tx;
  if (tiles) *tiles = (int)std::min<int64_t>(tx * ty, INT32_MAX);
  return tx * ty * C;
}

// g[i] = exp(-(i - 5)^2 / (2 1.5^2)), normalised to sum 1, in fp64 on the host: the one window of both SSIM entries
static inline ssim_taps_t ssim_window() {
  ssim_taps_t taps;
  double sum = 0.0;
  for (int i = 0; i < SSIM_TAPS; ++i) {
    const double d = (double)(i - SSIM_TAPS / 2);
    taps.g[i] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
    sum += taps.g[i];
  }
  for (int i = 0; i < SSIM_TAPS; ++i) taps.g[i] /= sum;
  return taps;
}

static int64_t ssim_ws_bytes(const char* name, int32_t batch, int32_t C, int32_t H, int32_t W, int K) {
  return ws_bytes_or_fail(name, batch < 1 || C < 1 || H < SSIM_TAPS || W < SSIM_TAPS, " (batch and C at least 1, H and W at least 11)", batch,
                          ssim_parts(C, H, W, nullptr, nullptr), K);
}

// Both SSIM entries: mask == NULL -> afx_image_ssim (one sum per slot), else afx_image_ssim_masked (four)
static int ssim_entry(const char* name, bool masked, const float* mask, int32_t mask_batch, const void* a, const void* b, int32_t dtype,
                      int32_t transform, double data_range, double* out, void* ws, int64_t ws_bytes, int32_t batch, int32_t C, int32_t H,
                      int32_t W, void* stream) {
  if (!(data_range > 0.0) || data_range > 1e150) return fail(AFX_E_INVALID, "%s: data_range must be positive (and finite)", name);
  if (batch < 1 || batch > 65535 || C < 1) return fail(AFX_E_INVALID, "bad argument to %s (1 <= batch <= 65535, C >= 1)", name);
  if (masked && mask_batch != 1 && mask_batch != batch)
    return fail(AFX_E_INVALID, "%s: mask_batch must be 1 or batch = %d, got %d", name, (int)batch, (int)mask_batch);
  if (H < SSIM_TAPS || W < SSIM_TAPS) return fail(AFX_E_INVALID, "%s: H and W must be at least 11 (one window)", name);
  int tiles_x = 0, tiles = 0;
  const int64_t parts = ssim_parts(C, H, W, &tiles_x, &tiles);
  if (parts > INT32_MAX) return fail(AFX_E_INVALID, "%s: more than 2^31 - 1 tiles per sample", name);
  const int K = masked ? 4 : 1;
  AFX_TRY(score_refusals(name, a, b, mask, masked, dtype, transform, out, ws, ws_bytes, (int64_t)batch * parts * K * (int64_t)sizeof(double), 0));
  const ssim_taps_t taps = ssim_window();
  const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
  const int64_t mstride = mask_batch == 1 ? 0 : (int64_t)H * W;
  const bool bf16 = dtype == AFX_DT_BF16;
  auto kernel = masked ? (bf16 ? image_ssim_partial_kernel<true, true> : image_ssim_partial_kernel<false, true>)
                       : (bf16 ? image_ssim_partial_kernel<true, false> : image_ssim_partial_kernel<false, false>);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(kernel, dim3((unsigned)parts, batch), dim3(256), 0, st, a, b, mask, (int)transform, taps, c1, c2, (double*)ws, (int)H, (int)W,
                     tiles_x, tiles, mstride);
  hipLaunchKernelGGL(image_ssim_finish_kernel, dim3(batch, K), dim3(64), 0, st, (const double*)ws, out, (int)parts);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

// Both agreement-sum entries past their shape checks: n elements per sample, K sums per slot; mask == NULL -> the plain kernel
static int score_entry(const char* name, bool masked, const float* mask, int64_t mstride, uint32_t P, uint32_t R, uint32_t Q, const void* a,
                       const void* b, int32_t dtype, int32_t transform, double* out, void* ws, int64_t ws_bytes, int32_t batch, int64_t n,
                       void* stream) {
  const int parts = reduce_parts(n), K = masked ? 10 : 4;
  AFX_TRY(score_refusals(name, a, b, mask, masked, dtype, transform, out, ws, ws_bytes, (int64_t)batch * parts * K * (int64_t)sizeof(double), 16));
  if (batch == 0) return AFX_OK;
  const bool bf16 = dtype == AFX_DT_BF16;
  const int64_t ups = n / (bf16 ? 8 : 4), upw = (ups + parts - 1) / parts;
  const dim3 grid(parts, batch), fin((batch * K + 63) / 64);
  hipStream_t st = (hipStream_t)stream;
  if (masked) {
    hipLaunchKernelGGL(bf16 ? sample_score_masked_partial_kernel<true> : sample_score_masked_partial_kernel<false>, grid, dim3(256), 0, st, a, b,
                       mask, (int)transform, (double*)ws, ups, upw, mstride, P, R, Q);
    hipLaunchKernelGGL(ordered_finish_kernel<10>, fin, dim3(64), 0, st, (const double*)ws, out, (int)batch, parts);
  } else {
    hipLaunchKernelGGL(bf16 ? sample_score_partial_kernel<true> : sample_score_partial_kernel<false>, grid, dim3(256), 0, st, a, b,
                       (int)transform, (double*)ws, ups, upw);
    hipLaunchKernelGGL(ordered_finish_kernel<4>, fin, dim3(64), 0, st, (const double*)ws, out, (int)batch, parts);
  }
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

extern "C" {

int64_t afx_sample_score_ws_bytes(int32_t batch, int64_t n) {
  return ws_bytes_or_fail("afx_sample_score_ws_bytes", batch < 0 || n < 64 || n % 64, "", batch, reduce_parts(n), 4);
}

int afx_sample_score(const void* a, const void* b, int32_t dtype, int32_t transform, double* out, void* ws, int64_t ws_bytes,
                     int32_t batch, int64_t n, void* stream) {
  if (batch < 0 || batch > 65535 || n < 64 || n % 64)
    return fail(AFX_E_INVALID, "bad argument to afx_sample_score (n = elements per sample must be a positive multiple of 64)");
  return score_entry("afx_sample_score", false, nullptr, 0, 0, 0, 0, a, b, dtype, transform, out, ws, ws_bytes, batch, n, stream);
}

int64_t afx_sample_score_masked_ws_bytes(int32_t batch, int64_t n) {
  return ws_bytes_or_fail("afx_sample_score_masked_ws_bytes", batch < 0 || n < 64 || n % 64 || n > INT32_MAX,
                          " (n must be a positive multiple of 64 below 2^31)", batch, reduce_parts(n), 10);
}

int afx_sample_score_masked(const void* a, const void* b, const float* mask, int32_t dtype, int32_t transform, double* out, void* ws,
                            int64_t ws_bytes, int32_t batch, int32_t mask_batch, int32_t G, int32_t P, int32_t R, int32_t Q, void* stream) {
  const char* name = "afx_sample_score_masked";
  if (batch < 0 || batch > 65535 || G < 1 || P < 1 || R < 1 || Q < 1)
    return fail(AFX_E_INVALID, "bad argument to %s (0 <= batch <= 65535; G, P, R, Q >= 1)", name);
  if (R % Q) return fail(AFX_E_INVALID, "%s: Q = %d must divide R = %d", name, (int)Q, (int)R);
  if (mask_batch != 1 && mask_batch != batch)
    return fail(AFX_E_INVALID, "%s: mask_batch must be 1 or batch = %d, got %d", name, (int)batch, (int)mask_batch);
  const int64_t pr = (int64_t)P * R;
  if (pr > INT32_MAX || pr * G > INT32_MAX || (pr * G) % 64)
    return fail(AFX_E_INVALID, "bad argument to %s (n = G P R elements per sample must be a multiple of 64 below 2^31)", name);
  return score_entry(name, true, mask, mask_batch == 1 ? 0 : (int64_t)P * Q, (uint32_t)P, (uint32_t)R, (uint32_t)Q, a, b, dtype, transform, out, ws,
                     ws_bytes, batch, pr * G, stream);
}

int64_t afx_image_ssim_ws_bytes(int32_t batch, int32_t C, int32_t H, int32_t W) {
  return ssim_ws_bytes("afx_image_ssim_ws_bytes", batch, C, H, W, 1);
}

int afx_image_ssim(const void* a, const void* b, int32_t dtype, int32_t transform, double data_range, double* out, void* ws,
                   int64_t ws_bytes, int32_t batch, int32_t C, int32_t H, int32_t W, void* stream) {
  return ssim_entry("afx_image_ssim", false, nullptr, 1, a, b, dtype, transform, data_range, out, ws, ws_bytes, batch, C, H, W, stream);
}

int64_t afx_image_ssim_masked_ws_bytes(int32_t batch, int32_t C, int32_t H, int32_t W) {
  return ssim_ws_bytes("afx_image_ssim_masked_ws_bytes", batch, C, H, W, 4);
}

int afx_image_ssim_masked(const void* a, const void* b, const float* mask, int32_t dtype, int32_t transform, double data_range, double* out,
                          void* ws, int64_t ws_bytes, int32_t batch, int32_t mask_batch, int32_t C, int32_t H, int32_t W, void* stream) {
  return ssim_entry("afx_image_ssim_masked", true, mask, mask_batch, a, b, dtype, transform, data_range, out, ws, ws_bytes, batch, C, H, W, stream);
}

}  // extern "C"
