// Colour matching of a decoded edit to the picture it was made from (afx_color_fix; the pipelines' color_fix=).  Rules: arcflow_hip.h.
//   * wavelet: out = e + L, L = five levels (dilations 1, 2, 4, 8, 16) of the separable [1, 2, 1] / 4 blur with replicate borders on
//     d = s' - e.  Every element goes through the same fixed sequence of fp32 operations (wavelet_tap, below) whatever the launch
//     structure, so the two variants give the same bits:
//       - wavelet_fused_kernel (AFX_COLOR_WAVELET): one launch.  A work-group of 1024 lanes owns a 64 x 64 tile of one plane, loads d of
//         the tile and its 31-pixel apron (clipped to the image: at most 126 x 126) into LDS and carries all five levels between two LDS
//         buffers of 126 x 126 fp32 = 63.5 KB each (127 KB: one work-group = 16 waves per CU).  A pass computes only what the later
//         passes still need (the apron shrinks by the dilation per pass), lanes on consecutive columns of a row (LDS reads and writes of
//         one wave fall on consecutive banks).  The last pass adds e and stores 256-B row segments.  e and s are read once from memory
//         (the aprons again through the caches, (126 / 64)^2 = 3.9 times), out is written once.
//       - wavelet_pass_kernel (AFX_COLOR_WAVELET_LEVELS): ten launches, one per pass, between two fp32 planes of `ws`; the first forms d
//         per tap, the last adds e.  About four times the traffic; kept as the plain form the fused one is tested against bit for bit.
//   * adain: moments_partial_kernel (fp64 sums and sums of squares, one slot per work-group, the partition a function of H W alone),
//     moments_finish_kernel (one wave per (image, channel): the slots in a fixed order, then mu, var, a, b and `stats`) and
//     affine_kernel (out = fma(a, e, b)).  No atomics.
#include "afx_api_util.h"
#include "afx_common.h"
#include "afx_reduce.h"

namespace afx {

// every multiply-add below is written out: the compiler fuses nothing else, so the header's rounding count holds
#pragma clang fp contract(off)

constexpr int kWvTile = 64;                         // output tile side of the fused kernel
constexpr int kWvApron = 31;                         // 1 + 2 + 4 + 8 + 16
constexpr int kWvSide = kWvTile + 2 * kWvApron;      // 126
constexpr int kWvThreads = 1024;
constexpr int kWvLevels = 5;
constexpr int64_t kPassMaxRows = 65535;              // gridDim.y of the per-pass kernels; further rows by their row-stride loop
constexpr int kMomentChunk = 4096;                   // elements per work-group of moments_partial_kernel (16 per lane)
constexpr int kAffineChunk = 2048;                   // elements per work-group of affine_kernel (8 per lane)

template <bool BF16>
AFX_DEV float load_edit(const void* __restrict__ e, int64_t i) {
  if constexpr (BF16) return bf16_to_f32(static_cast<const bf16_t*>(e)[i]);
  else return static_cast<const float*>(e)[i];
}

// s' of the header: a source in [0, 1] is read as fma(2, s, -1)
AFX_DEV float load_src(const float* __restrict__ s, int64_t i, int src01) {
  const float v = s[i];
  return src01 ? __builtin_fmaf(2.0f, v, -1.0f) : v;
}

// One [1, 2, 1] / 4 tap triple, the one formula of both variants: two roundings (the sum and the fma); the scalings are exact.
AFX_DEV float wavelet_tap(float lo, float mid, float hi) { return __builtin_fmaf(0.5f, mid, 0.25f * (lo + hi)); }

// One pass over the rows [ya, yb) x columns [xa, xb) of the region (region coordinates): COLS lanes along a row, kWvThreads / COLS rows
// at a time.  Tap indices are clamped to the region, which is the clamp to the image wherever the result is still needed.
template <int COLS, bool HORIZ>
AFX_DEV void wavelet_lds_pass(const float* __restrict__ in, float* __restrict__ out, int r, int ya, int yb, int xa, int xb, int RH, int RW) {
  const int tx = threadIdx.x % COLS, ty = threadIdx.x / COLS;
  const int x = xa + tx;
  if (x >= xb) return;
  for (int y = ya + ty; y < yb; y += kWvThreads / COLS) {
    float lo, hi;
    if constexpr (HORIZ) {
      lo = in[y * kWvSide + max(x - r, 0)];
      hi = in[y * kWvSide + min(x + r, RW - 1)];
    } else {
      lo = in[max(y - r, 0) * kWvSide + x];
      hi = in[min(y + r, RH - 1) * kWvSide + x];
    }
    out[y * kWvSide + x] = wavelet_tap(lo, in[y * kWvSide + x], hi);
  }
}

// grid: planes * tiles_y * tiles_x work-groups, tile-x fastest.  plane = b C + c; the source's plane is c (src_batch 1) or the same.
template <bool BF16>
__global__ __launch_bounds__(kWvThreads) void wavelet_fused_kernel(const void* __restrict__ edit, const float* __restrict__ src,
                                                                    float* __restrict__ out, int src01, int src_bcast, int C, int H, int W,
                                                                    int tiles_x, int tiles_y) {
  __shared__ float buf[2][kWvSide * kWvSide];
  const unsigned tile = blockIdx.x % ((unsigned)tiles_x * tiles_y);
  const int64_t plane = blockIdx.x / ((unsigned)tiles_x * tiles_y);
  const int64_t splane = src_bcast ? plane % C : plane;
  const int oy0 = (int)(tile / tiles_x) * kWvTile, ox0 = (int)(tile % tiles_x) * kWvTile;
  const int oy1 = min(oy0 + kWvTile, H), ox1 = min(ox0 + kWvTile, W);
  const int gy0 = max(oy0 - kWvApron, 0), gx0 = max(ox0 - kWvApron, 0);
  const int RH = min(oy1 + kWvApron, H) - gy0, RW = min(ox1 + kWvApron, W) - gx0;          // <= kWvSide
  const int64_t ebase = plane * H * W, sbase = splane * H * W;

  {  // d = s' - e over the region
    const int tx = threadIdx.x & 127, ty = threadIdx.x >> 7;
    if (tx < RW) {
      for (int y = ty; y < RH; y += kWvThreads / 128) {
        const int64_t off = (int64_t)(gy0 + y) * W + gx0 + tx;
        buf[0][y * kWvSide + tx] = load_src(src, sbase + off, src01) - load_edit<BF16>(edit, ebase + off);
      }
    }
  }
  __syncthreads();

  // level k, dilation r = 2^k: after its vertical pass the rows and columns within rem = 31 - (2^(k+1) - 1) of the tile are still needed
  // (clipped to the region); its horizontal pass feeds that, so it covers r more rows.
  const int ty0 = oy0 - gy0, ty1 = oy1 - gy0, tx0 = ox0 - gx0, tx1 = ox1 - gx0;           // the tile in region coordinates
#pragma unroll
  for (int k = 0; k < kWvLevels - 1; ++k) {
    const int r = 1 << k, rem = kWvApron - (2 * r - 1);
    const int xa = max(tx0 - rem, 0), xb = min(tx1 + rem, RW), ya = max(ty0 - rem, 0), yb = min(ty1 + rem, RH);
    wavelet_lds_pass<128, true>(buf[0], buf[1], r, max(ya - r, 0), min(yb + r, RH), xa, xb, RH, RW);
    __syncthreads();
    wavelet_lds_pass<128, false>(buf[1], buf[0], r, ya, yb, xa, xb, RH, RW);
    __syncthreads();
  }
  {  // the last level (r = 16, rem = 0): the horizontal pass over the tile's columns, then the vertical taps, + e, to memory
    constexpr int r = 1 << (kWvLevels - 1);
    wavelet_lds_pass<64, true>(buf[0], buf[1], r, max(ty0 - r, 0), min(ty1 + r, RH), tx0, tx1, RH, RW);
    __syncthreads();
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int x = tx0 + tx;
    if (x < tx1) {
      for (int y = ty0 + ty; y < ty1; y += kWvThreads / 64) {
        const float L = wavelet_tap(buf[1][max(y - r, 0) * kWvSide + x], buf[1][y * kWvSide + x], buf[1][min(y + r, RH - 1) * kWvSide + x]);
        const int64_t off = (int64_t)(gy0 + y) * W + gx0 + x;
        out[ebase + off] = load_edit<BF16>(edit, ebase + off) + L;
      }
    }
  }
}

// One pass of the per-level variant over planes of [H, W]: rows = planes H, one lane per column, a work-group on one row at a time.
// FIRST: the input is d = s' - e, formed per tap.  LAST: the output is e + the pass' value.  Otherwise in -> dst, both fp32 planes of ws.
template <bool BF16, bool HORIZ, bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void wavelet_pass_kernel(const void* __restrict__ edit, const float* __restrict__ src,
                                                           const float* __restrict__ in, float* __restrict__ dst, int r, int src01,
                                                           int src_bcast, int C, int64_t rows, int H, int W) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= W) return;
  for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
    const int64_t plane = row / H;
    const int y = (int)(row - plane * H);
    const int64_t base = plane * H * W, sbase = (src_bcast ? plane % C : plane) * H * W;
    int64_t olo, omid = (int64_t)y * W + x, ohi;
    if constexpr (HORIZ) {
      olo = (int64_t)y * W + max(x - r, 0);
      ohi = (int64_t)y * W + min(x + r, W - 1);
    } else {
      olo = (int64_t)max(y - r, 0) * W + x;
      ohi = (int64_t)min(y + r, H - 1) * W + x;
    }
    float lo, mid, hi;
    if constexpr (FIRST) {
      lo = load_src(src, sbase + olo, src01) - load_edit<BF16>(edit, base + olo);
      mid = load_src(src, sbase + omid, src01) - load_edit<BF16>(edit, base + omid);
      hi = load_src(src, sbase + ohi, src01) - load_edit<BF16>(edit, base + ohi);
    } else {
      lo = in[base + olo]; mid = in[base + omid]; hi = in[base + ohi];
    }
    const float q = wavelet_tap(lo, mid, hi);
    if constexpr (LAST) dst[base + omid] = load_edit<BF16>(edit, base + omid) + q;
    else dst[base + omid] = q;
  }
}

// grid: (planes_e + planes_s) * parts work-groups, part fastest.  Work-group (plane, w) owns the elements [w kMomentChunk, min((w + 1)
// kMomentChunk, n)) of its plane and writes slot[(plane parts + w) 2 + {0, 1}] = sum x, sum x^2, x widened to fp64 (x x is exact).  The
// planes of the edit come first, then those of the source (after the s' transform).
template <bool BF16>
__global__ __launch_bounds__(256) void moments_partial_kernel(const void* __restrict__ edit, const float* __restrict__ src, int src01,
                                                              double* __restrict__ slots, int64_t planes_e, int64_t n, int parts) {
  const int64_t plane = blockIdx.x / (unsigned)parts;
  const int w = (int)(blockIdx.x % (unsigned)parts);
  const int64_t begin = (int64_t)w * kMomentChunk, end = begin + kMomentChunk < n ? begin + kMomentChunk : n;
  double acc[2] = {0.0, 0.0};
  if (plane < planes_e) {
    for (int64_t i = begin + threadIdx.x; i < end; i += 256) {
      const double x = (double)load_edit<BF16>(edit, plane * n + i);
      acc[0] += x;
      acc[1] += x * x;
    }
  } else {
    for (int64_t i = begin + threadIdx.x; i < end; i += 256) {
      const double x = (double)load_src(src, (plane - planes_e) * n + i, src01);
      acc[0] += x;
      acc[1] += x * x;
    }
  }
  block_slot_sums<2>(acc, slots + (int64_t)blockIdx.x * 2);
}

// lane l adds the slots l, l + 64, ... of the plane in index order, then the 64 lanes by the shuffle tree (afx_image_ssim's order)
AFX_DEV double plane_sum(const double* __restrict__ slots, int64_t plane, int parts, int k) {
  double v = 0.0;
  for (int w = threadIdx.x; w < parts; w += 64) v += slots[(plane * parts + w) * 2 + k];
  return wave_sum_f64(v);
}

// grid: batch C work-groups of one wave, one per (image, channel): the moments of both planes by the same sequence of operations, then
// coef[plane] = (a, b) and, when asked, stats[plane] = (mu_e, var_e, mu_s, var_s).
__global__ __launch_bounds__(64) void moments_finish_kernel(const double* __restrict__ slots, float* __restrict__ coef,
                                                            double* __restrict__ stats, int64_t planes_e, int src_bcast, int C, int64_t n,
                                                            int parts) {
  const int64_t plane = blockIdx.x;
  const int64_t splane = planes_e + (src_bcast ? plane % C : plane);
  const double dn = (double)n;
  const double mu_e = plane_sum(slots, plane, parts, 0) / dn, q_e = plane_sum(slots, plane, parts, 1) / dn;
  const double mu_s = plane_sum(slots, splane, parts, 0) / dn, q_s = plane_sum(slots, splane, parts, 1) / dn;
  if (threadIdx.x != 0) return;
  const double var_e = q_e - mu_e * mu_e, var_s = q_s - mu_s * mu_s;
  const double ratio = sqrt(var_s + 1e-5) / sqrt(var_e + 1e-5);
  coef[plane * 2 + 0] = (float)ratio;
  coef[plane * 2 + 1] = (float)(mu_s - ratio * mu_e);
  if (stats) {
    stats[plane * 4 + 0] = mu_e; stats[plane * 4 + 1] = var_e; stats[plane * 4 + 2] = mu_s; stats[plane * 4 + 3] = var_s;
  }
}

// grid: planes * chunks work-groups, chunk fastest; a work-group owns kAffineChunk consecutive elements of one plane
template <bool BF16>
__global__ __launch_bounds__(256) void affine_kernel(const void* __restrict__ edit, const float* __restrict__ coef, float* __restrict__ out,
                                                     int64_t n, int chunks) {
  const int64_t plane = blockIdx.x / (unsigned)chunks;
  const int64_t begin = (int64_t)(blockIdx.x % (unsigned)chunks) * kAffineChunk;
  const int64_t end = begin + kAffineChunk < n ? begin + kAffineChunk : n;
  const float a = coef[plane * 2], b = coef[plane * 2 + 1];
  for (int64_t i = begin + threadIdx.x; i < end; i += 256) out[plane * n + i] = __builtin_fmaf(a, load_edit<BF16>(edit, plane * n + i), b);
}

static inline int64_t moment_parts(int64_t n) { return (n + kMomentChunk - 1) / kMomentChunk; }

// the bytes of ws a mode needs, or -1 for a shape past the mode's grid limit (the caller has checked mode, batch, C, H, W)
static int64_t color_ws_need(int32_t mode, int64_t batch, int64_t C, int64_t H, int64_t W) {
  const int64_t n = H * W, planes = batch * C;
  if (mode == AFX_COLOR_WAVELET)
    return planes * ((H + kWvTile - 1) / kWvTile) * ((W + kWvTile - 1) / kWvTile) > INT32_MAX ? -1 : 0;
  if (mode == AFX_COLOR_WAVELET_LEVELS) return 2 * planes * n * 4;
  // adain: the slots of 2 batch C planes (a source batch of 1 leaves some unused), then batch C (a, b) pairs
  if (2 * planes * moment_parts(n) > INT32_MAX || planes * ((n + kAffineChunk - 1) / kAffineChunk) > INT32_MAX) return -1;
  return (2 * planes * moment_parts(n) * 2 + planes) * 8;
}

}  // namespace afx

using namespace afx;

static bool color_shape_bad(int32_t mode, int32_t batch, int32_t C, int32_t H, int32_t W) {
  return (mode != AFX_COLOR_ADAIN && mode != AFX_COLOR_WAVELET && mode != AFX_COLOR_WAVELET_LEVELS) || batch < 1 || C < 1 || H < 1 || W < 1 ||
         (int64_t)batch * C > INT32_MAX || (int64_t)H * W > INT32_MAX;
}

template <bool BF16>
static int wavelet_levels_launch(const void* edit, const float* src, float* out, float* ws, int src01, int bcast, int C, int64_t planes, int H,
                                 int W, hipStream_t st) {
  const int64_t rows = planes * H;
  const dim3 grid((unsigned)((W + 255) / 256), (unsigned)std::min(rows, kPassMaxRows)), block(256);
  float* A = ws;
  float* B = ws + planes * H * W;
  for (int k = 0; k < kWvLevels; ++k) {
    const int r = 1 << k;
    if (k == 0)
      hipLaunchKernelGGL((wavelet_pass_kernel<BF16, true, true, false>), grid, block, 0, st, edit, src, (const float*)nullptr, A, r, src01, bcast,
                         C, rows, H, W);
    else
      hipLaunchKernelGGL((wavelet_pass_kernel<BF16, true, false, false>), grid, block, 0, st, edit, src, (const float*)B, A, r, src01, bcast, C,
                         rows, H, W);
    HIP_TRY(hipGetLastError());
    if (k == kWvLevels - 1)
      hipLaunchKernelGGL((wavelet_pass_kernel<BF16, false, false, true>), grid, block, 0, st, edit, src, (const float*)A, out, r, src01, bcast, C,
                         rows, H, W);
    else
      hipLaunchKernelGGL((wavelet_pass_kernel<BF16, false, false, false>), grid, block, 0, st, edit, src, (const float*)A, B, r, src01, bcast, C,
                         rows, H, W);
    HIP_TRY(hipGetLastError());
  }
  return AFX_OK;
}

extern "C" {

int64_t afx_color_fix_ws_bytes(int32_t mode, int32_t batch, int32_t C, int32_t H, int32_t W) {
  if (color_shape_bad(mode, batch, C, H, W))
    return (int64_t)fail(AFX_E_INVALID, "bad argument to afx_color_fix_ws_bytes (a known mode; batch, C, H, W >= 1; batch C and H W below 2^31)");
  const int64_t need = color_ws_need(mode, batch, C, H, W);
  if (need < 0) return (int64_t)fail(AFX_E_INVALID, "afx_color_fix_ws_bytes: the shape needs more than 2^31 - 1 work-groups");
  return need;
}

int afx_color_fix(const void* edit, int32_t dtype, const float* src, int32_t src_batch, int32_t src01, int32_t mode, float* out, double* stats,
                  void* ws, int64_t ws_bytes, int32_t batch, int32_t C, int32_t H, int32_t W, void* stream) {
  if (!edit || !src || !out) return fail(AFX_E_INVALID, "null argument to afx_color_fix (edit, src and out are required)");
  if (dtype != AFX_DT_BF16 && dtype != AFX_DT_F32) return fail(AFX_E_INVALID, "afx_color_fix: dtype must be AFX_DT_BF16 or AFX_DT_F32");
  if (src01 != 0 && src01 != 1) return fail(AFX_E_INVALID, "afx_color_fix: src01 must be 0 or 1, got %d", (int)src01);
  if (color_shape_bad(mode, batch, C, H, W))
    return fail(AFX_E_INVALID, "bad argument to afx_color_fix (a known mode; batch, C, H, W >= 1; batch C and H W below 2^31)");
  if (src_batch != 1 && src_batch != batch) return fail(AFX_E_INVALID, "afx_color_fix: src_batch must be 1 or batch = %d, got %d", (int)batch, (int)src_batch);
  const int64_t need = color_ws_need(mode, batch, C, H, W);
  if (need < 0) return fail(AFX_E_INVALID, "afx_color_fix: the shape needs more than 2^31 - 1 work-groups");
  const bool bf16 = dtype == AFX_DT_BF16, adain = mode == AFX_COLOR_ADAIN;
  if (!adain) stats = nullptr;
  if (((uintptr_t)edit & (bf16 ? 1 : 3)) || ((uintptr_t)src & 3) || ((uintptr_t)out & 3) || ((uintptr_t)stats & 7) || ((uintptr_t)ws & 7))
    return fail(AFX_E_INVALID, "afx_color_fix: edit must be aligned to its element, src and out to 4 bytes, stats and ws to 8");
  const int64_t n = (int64_t)H * W, planes = (int64_t)batch * C;
  const int64_t ebytes = planes * n * (bf16 ? 2 : 4), sbytes = (int64_t)src_batch * C * n * 4, obytes = planes * n * 4, tbytes = planes * 32;
  const void* wsr = need ? ws : nullptr;              // a mode without a workspace ignores ws
  if (ranges_overlap(out, obytes, edit, ebytes) || ranges_overlap(out, obytes, src, sbytes) || ranges_overlap(stats, tbytes, edit, ebytes) ||
      ranges_overlap(stats, tbytes, src, sbytes) || ranges_overlap(wsr, need, edit, ebytes) || ranges_overlap(wsr, need, src, sbytes) ||
      ranges_overlap(out, obytes, stats, tbytes) || ranges_overlap(out, obytes, wsr, need) || ranges_overlap(stats, tbytes, wsr, need))
    return fail(AFX_E_INVALID, "afx_color_fix: out, stats or ws overlaps an operand, or each other (in-place operation is refused)");
  if (need && (!ws || ws_bytes < need))
    return fail(AFX_E_WORKSPACE, "afx_color_fix: workspace missing or too small (%lld bytes, need afx_color_fix_ws_bytes = %lld)",
                (long long)(ws ? ws_bytes : 0), (long long)need);

  const hipStream_t st = (hipStream_t)stream;
  const int bcast = src_batch == 1 && batch > 1;
  if (mode == AFX_COLOR_WAVELET) {
    const int tiles_x = (W + kWvTile - 1) / kWvTile, tiles_y = (H + kWvTile - 1) / kWvTile;
    const dim3 grid((unsigned)(planes * tiles_x * tiles_y));
    if (bf16)
      hipLaunchKernelGGL(wavelet_fused_kernel<true>, grid, dim3(kWvThreads), 0, st, edit, src, out, (int)src01, bcast, (int)C, (int)H, (int)W, tiles_x,
                         tiles_y);
    else
      hipLaunchKernelGGL(wavelet_fused_kernel<false>, grid, dim3(kWvThreads), 0, st, edit, src, out, (int)src01, bcast, (int)C, (int)H, (int)W, tiles_x,
                         tiles_y);
    HIP_TRY(hipGetLastError());
    return AFX_OK;
  }
  if (mode == AFX_COLOR_WAVELET_LEVELS)
    return bf16 ? wavelet_levels_launch<true>(edit, src, out, (float*)ws, src01, bcast, C, planes, H, W, st)
                : wavelet_levels_launch<false>(edit, src, out, (float*)ws, src01, bcast, C, planes, H, W, st);

  const int parts = (int)moment_parts(n), chunks = (int)((n + kAffineChunk - 1) / kAffineChunk);
  const int64_t planes_s = (int64_t)src_batch * C;
  double* slots = (double*)ws;
  float* coef = (float*)(slots + 2 * planes * parts * 2);
  const dim3 pgrid((unsigned)((planes + planes_s) * parts)), block(256);
  if (bf16)
    hipLaunchKernelGGL(moments_partial_kernel<true>, pgrid, block, 0, st, edit, src, (int)src01, slots, planes, n, parts);
  else
    hipLaunchKernelGGL(moments_partial_kernel<false>, pgrid, block, 0, st, edit, src, (int)src01, slots, planes, n, parts);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(moments_finish_kernel, dim3((unsigned)planes), dim3(64), 0, st, (const double*)slots, coef, stats, planes, bcast, (int)C, n, parts);
  HIP_TRY(hipGetLastError());
  const dim3 agrid((unsigned)(planes * chunks));
  if (bf16)
    hipLaunchKernelGGL(affine_kernel<true>, agrid, block, 0, st, edit, (const float*)coef, out, n, chunks);
  else
    hipLaunchKernelGGL(affine_kernel<false>, agrid, block, 0, st, edit, (const float*)coef, out, n, chunks);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

}  // extern "C"
