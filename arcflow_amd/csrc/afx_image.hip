// Image resampling for the edit pipelines: resize, crop and Gaussian mask feathering as ONE table-driven separable pass pair.
//   out[i] = sum_{k < count[i]} w[i, k] * in[start[i] + k]          per axis, horizontally first, then vertically
// The tables (start, count, w[n_out, taps]) say everything about the filter: afx_resample_table builds them on the host in fp64 by
// Pillow's Image.resize(..., box=) rule (Lanczos-3, triangle) or as a border-clipped, renormalised Gaussian, and rounds the weights
// to fp32 once.  The kernels know no filter formula.
//   * resample_h_kernel: src (uint8 [B, H, W, C] or fp32 [B, C, H, W]) -> ws fp32 [B, C, H, W_out].  One lane per output column of one
//     source row, consecutive lanes on consecutive columns: the lanes of a wave read a span of about 64 * scale source pixels per tap
//     (re-reads between neighbouring windows hit the vector cache), and the store is one coalesced 256-B row segment per wave.  A uint8
//     lane reads the C interleaved bytes of each tap once and keeps C accumulators; uint8 -> fp32 is the IEEE quotient float(x) / 255.0f.
//   * resample_v_kernel: ws -> dst fp32 [B, C, H_out, W_out].  One lane per output pixel; a work-group shares its output row, so start,
//     count and the weights are wave-uniform (scalar loads) and every tap is one coalesced row-segment load.  Optional clamp to [0, 1].
//   Both accumulate in fp32 by fma in tap order.  Every source index is clamped into [0, n_in - 1] and count is capped at taps before
//   any load: a bad table gives wrong pixels, never a read outside the source.
//   Traffic for a 4000 x 3000 x 3 uint8 photo -> 1024 x 1024: 36 MB read, 36.9 MB of ws written and read again, 12.6 MB written = 122 MB.
// The way back, for an edit that ran on a window of a larger photo (afx_mask_bbox finds the window, afx_image_paste returns the edit):
//   * mask_bbox_kernel: the half-open bounding box of the mask's pixels > 0 per image, by integer min / max atomics.
//   * afx_image_paste: resample_h_kernel<false, 1> on the decoded image (and the mask), then paste_kernel: per pixel of the uint8 photo the
//     vertical taps, p = 0.5 v + 0.5, the blend m p + (1 - m) byte / 255 and the rounding to a byte; the source's own bytes outside the
//     window and where m == 0.  The same tables, the same clamped indices: no filter formula, no read outside an operand.
// Tiled editing of a canvas larger than the model's size (the pipelines' enhance; the plan is arcflow_amd.schedule.tile_plan on the host):
//   * tiles_cut_kernel: the canvas fp32 [3, H, W] -> the stack of overlapping tiles [T, 3, th, tw], a bit copy in 16-byte chunks.
//   * tiles_merge_kernel: the decoded tiles -> uint8 [H, W, 3]: per pixel the cross-fade weights of the tiles that cover it (at most
//     AFX_TILE_MAX_TAPS per axis, tables of the resampler's form), p = 0.5 v + 0.5 and ONE rounding to a byte.  No accumulator canvas and no
//     atomics.  Traffic at a 4500 x 6000 canvas in 1024-pixel tiles with overlap 128: 35 tiles = 440 MB read once, 81 MB written.
// Outpainting (the pipelines' outpaint; the plan of windows is arcflow_amd.schedule.outpaint_plan on the host):
//   * canvas_extend_kernel: the photo uint8 [B, H, W, 3] -> the extended canvas uint8 [B, Hc, Wc, 3], every canvas pixel the photo's pixel
//     at the edge-clamped or mirrored index (a bit copy), and the mask state fp32 [Hc, Wc]: 1 on the new pixels, a ramp of `blend` pixels
//     inside every extended side of the photo, 0 deeper inside.  One lane per four consecutive pixels of the flat canvas: 12 bytes of
//     canvas stored as three dwords and 16 bytes of mask as one float4 where the addresses allow.
//     Traffic for a 3000 x 4000 photo extended 512 px on every side: 36 MB read, 60.6 MB of canvas and 80.9 MB of mask written.
//   * canvas_mark_kernel: M = min(M, ramp(d)) in place on the pixels of one window, d the distance to the nearest window side that is not
//     on the canvas border; one lane per aligned quad of columns of one row, 16-byte loads and stores where the quad lies in the window.
#include <algorithm>
#include <cmath>
#include <vector>

#include "afx_api_util.h"
#include "afx_common.h"

namespace afx {

constexpr int kResampleBlock = 256;
constexpr int64_t kResampleMaxRows = 65535;         // gridDim.y; further rows are taken by the row-stride loop
constexpr int64_t kBboxMaxBlocks = 1024;            // work-groups per image of mask_bbox_kernel (4 per CU); further pixels by its grid-stride loop
constexpr int64_t kTilesCutMaxBlocks = 2048;        // work-groups of tiles_cut_kernel (8 per CU); further chunks by its grid-stride loop

// rows: U8 ? B * H (each gives C rows of ws) : B * C * H
template <bool U8, int C>
__global__ __launch_bounds__(kResampleBlock) void resample_h_kernel(const void* __restrict__ src, const int32_t* __restrict__ start,
                                                                    const int32_t* __restrict__ count, const float* __restrict__ w, int taps,
                                                                    float* __restrict__ ws, int64_t rows, int H, int W_in, int W_out) {
  const int x = blockIdx.x * kResampleBlock + threadIdx.x;
  if (x >= W_out) return;
  const int s0 = start[x];
  const int n = min(count[x], taps);
  const float* wx = w + (int64_t)x * taps;
  for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
    if constexpr (U8) {
      const uint8_t* in = static_cast<const uint8_t*>(src) + row * W_in * C;
      float acc[C];
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] = 0.0f;
      for (int k = 0; k < n; ++k) {
        const int sx = min(max(s0 + k, 0), W_in - 1);
        const float wk = wx[k];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = __builtin_fmaf(wk, __fdiv_rn((float)in[(int64_t)sx * C + c], 255.0f), acc[c]);
      }
      const int64_t b = row / H, y = row - b * H;
#pragma unroll
      for (int c = 0; c < C; ++c) ws[((b * C + c) * H + y) * W_out + x] = acc[c];
    } else {
      const float* in = static_cast<const float*>(src) + row * W_in;
      float acc = 0.0f;
      for (int k = 0; k < n; ++k) acc = __builtin_fmaf(wx[k], in[min(max(s0 + k, 0), W_in - 1)], acc);
      ws[row * W_out + x] = acc;
    }
  }
}

// rows = planes * H_out; a work-group works on one output row at a time
__global__ __launch_bounds__(kResampleBlock) void resample_v_kernel(const float* __restrict__ ws, const int32_t* __restrict__ start,
                                                                    const int32_t* __restrict__ count, const float* __restrict__ w, int taps,
                                                                    float* __restrict__ dst, int64_t rows, int H_in, int H_out, int W_out,
                                                                    int clamp) {
  const int x = blockIdx.x * kResampleBlock + threadIdx.x;
  if (x >= W_out) return;
  for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
    const int64_t plane = row / H_out;
    const int y = (int)(row - plane * H_out);
    const int s0 = start[y];
    const int n = min(count[y], taps);
    const float* wy = w + (int64_t)y * taps;
    const float* in = ws + plane * H_in * W_out + x;
    float acc = 0.0f;
    for (int k = 0; k < n; ++k) acc = __builtin_fmaf(wy[k], in[(int64_t)min(max(s0 + k, 0), H_in - 1) * W_out], acc);
    if (clamp) acc = fminf(fmaxf(acc, 0.0f), 1.0f);
    dst[row * W_out + x] = acc;
  }
}

// bbox [B, 4] = (W, H, 0, 0): the identity of the (min, min, max, max) that mask_bbox_kernel folds in
__global__ __launch_bounds__(64) void mask_bbox_init_kernel(int32_t* __restrict__ bbox, int batch, int H, int W) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= batch) return;
  int32_t* o = bbox + 4 * b;
  o[0] = W; o[1] = H; o[2] = 0; o[3] = 0;
}

// One lane per pixel of one image (blockIdx.y), grid-stride over its H * W pixels.  A lane keeps the box of its own pixels, a wave folds
// its 64 boxes by shuffles, and lane 0 of a wave that saw a pixel folds the wave's box into bbox[b] with four integer atomics: integer
// min / max give the same result in every arrival order.  U8: m > 0 is byte != 0.  fp32: the bit pattern as a signed integer is in
// (0, 0x7f800000] exactly for the positive values, denormals and +inf included and every NaN and negative excluded, whatever the
// denormal mode of the float compare.
template <bool U8>
__global__ __launch_bounds__(kResampleBlock) void mask_bbox_kernel(const void* __restrict__ mask, int32_t* __restrict__ bbox, int H, int W) {
  const int64_t n = (int64_t)H * W;
  const int b = blockIdx.y;
  int x0 = W, y0 = H, x1 = 0, y1 = 0;
  for (int64_t i = (int64_t)blockIdx.x * kResampleBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kResampleBlock) {
    bool on;
    if constexpr (U8) {
      on = static_cast<const uint8_t*>(mask)[b * n + i] != 0;
    } else {
      const int32_t bits = static_cast<const int32_t*>(mask)[b * n + i];
      on = bits > 0 && bits <= 0x7f800000;
    }
    if (on) {
      const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
      x0 = min(x0, x); y0 = min(y0, y); x1 = max(x1, x + 1); y1 = max(y1, y + 1);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    x0 = min(x0, __shfl_xor(x0, o, 64)); y0 = min(y0, __shfl_xor(y0, o, 64));
    x1 = max(x1, __shfl_xor(x1, o, 64)); y1 = max(y1, __shfl_xor(y1, o, 64));
  }
  if ((threadIdx.x & 63) == 0 && x1 > 0) {
    int32_t* o = bbox + 4 * b;
    atomicMin(o + 0, x0); atomicMin(o + 1, y0); atomicMax(o + 2, x1); atomicMax(o + 3, y1);
  }
}

// The vertical taps of one output pixel: column x of the horizontal result `in` [H_in, W_out] of one plane, fp32 fma in tap order as in
// resample_v_kernel; s0, n and wy are the row's (wave-uniform) table entries.
AFX_DEV float paste_v_taps(const float* __restrict__ in, int s0, int n, const float* __restrict__ wy, int H_in, int W_out, int x) {
  float acc = 0.0f;
  for (int k = 0; k < n; ++k) acc = __builtin_fmaf(wy[k], in[(int64_t)min(max(s0 + k, 0), H_in - 1) * W_out + x], acc);
  return acc;
}

// The second pass of afx_image_paste: dst uint8 [B, H, W, 3], one lane per pixel, a work-group works on one row of dst at a time (rows =
// B * H), so whether the row crosses the window, and the vertical tables' entries where it does, are wave-uniform.  ws_img [B, 3, h, ww] and
// ws_mask [mask_batch, h, ww] (NULL: m = 1) are the horizontal results, ww = x1 - x0.  Outside the window, and inside it where m == 0, the
// source's bytes are stored as they are: no float stands between them, and nothing of img (a NaN included) can reach them.
__global__ __launch_bounds__(kResampleBlock) void paste_kernel(const float* __restrict__ ws_img, const float* __restrict__ ws_mask,
                                                               const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                               const int32_t* __restrict__ iv_start, const int32_t* __restrict__ iv_count,
                                                               const float* __restrict__ iv_w, int iv_taps,
                                                               const int32_t* __restrict__ mv_start, const int32_t* __restrict__ mv_count,
                                                               const float* __restrict__ mv_w, int mv_taps, int64_t rows, int mask_batch, int h,
                                                               int H, int W, int x0, int y0, int x1, int y1) {
  const int X = blockIdx.x * kResampleBlock + threadIdx.x;
  if (X >= W) return;
  const int ww = x1 - x0, xx = X - x0;
  for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
    const int64_t b = row / H;
    const int Y = (int)(row - b * H);
    const int64_t px = (row * W + X) * 3;
    const uint8_t s0 = src[px], s1 = src[px + 1], s2 = src[px + 2];
    uint8_t q[3] = {s0, s1, s2};
    if (Y >= y0 && Y < y1 && X >= x0 && X < x1) {
      const int yy = Y - y0;
      float m = 1.0f;
      if (ws_mask) {
        const int64_t mb = mask_batch == 1 ? 0 : b;
        m = paste_v_taps(ws_mask + mb * h * ww, mv_start[yy], min(mv_count[yy], mv_taps), mv_w + (int64_t)yy * mv_taps, h, ww, xx);
        m = fminf(fmaxf(m, 0.0f), 1.0f);
      }
      if (m != 0.0f) {
        const int is0 = iv_start[yy], in = min(iv_count[yy], iv_taps);
        const float* wy = iv_w + (int64_t)yy * iv_taps;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float v = paste_v_taps(ws_img + (b * 3 + c) * h * ww, is0, in, wy, h, ww, xx);
          const float p = __builtin_fmaf(0.5f, v, 0.5f);
          const float s = __fdiv_rn((float)q[c], 255.0f);
          const float r = __builtin_fmaf(m, p, (1.0f - m) * s);
          q[c] = (uint8_t)__builtin_rintf(255.0f * fminf(fmaxf(r, 0.0f), 1.0f));
        }
      }
    }
    dst[px] = q[0]; dst[px + 1] = q[1]; dst[px + 2] = q[2];
  }
}

// canvas fp32 [3, H, W] -> tiles fp32 [ky * kx, 3, th, tw], tile iy * kx + ix from the corner (oy[iy], ox[ix]).  One lane per 16-byte chunk
// (four columns) of a tile row, chunks numbered through the whole stack, grid-stride: consecutive lanes store consecutive 16 bytes (tw is
// a multiple of 16, so every chunk lies in one row and is 16-byte aligned when `tiles` is).  The source chunk is loaded as one 16 bytes
// when its address allows (W and ox[ix] multiples of 4 and an aligned canvas), else as four floats.  Values pass as bits.
__global__ __launch_bounds__(kResampleBlock) void tiles_cut_kernel(const float* __restrict__ canvas, const int32_t* __restrict__ oy,
                                                                   const int32_t* __restrict__ ox, float* __restrict__ tiles, int H, int W,
                                                                   int ky, int kx, int th, int tw, int64_t chunks) {
  const int cpr = tw >> 2;                                     // chunks per tile row
  for (int64_t i = (int64_t)blockIdx.x * kResampleBlock + threadIdx.x; i < chunks; i += (int64_t)gridDim.x * kResampleBlock) {
    const int64_t row = i / cpr;                               // ((tile * 3 + c) * th + r)
    const int col = (int)(i - row * cpr) << 2;
    const int64_t plane = row / th;
    const int r = (int)(row - plane * th);
    const int tile = (int)(plane / 3), c = (int)(plane - (int64_t)tile * 3);
    const int iy = min(tile / kx, ky - 1), ix = tile - (tile / kx) * kx;
    const int y = min(max(oy[iy], 0), H - th) + r, x = min(max(ox[ix], 0), W - tw) + col;
    const float* s = canvas + ((int64_t)c * H + y) * W + x;
    float4 v;
    if (((uintptr_t)s & 15) == 0) {
      v = *reinterpret_cast<const float4*>(s);
    } else {
      v.x = s[0]; v.y = s[1]; v.z = s[2]; v.w = s[3];
    }
    *reinterpret_cast<float4*>(tiles + i * 4) = v;
  }
}

// tiles fp32 [ky * kx, 3, th, tw] -> dst uint8 [H, W, 3].  One lane per pixel, a work-group works on a strip of 256 pixels of one row of
// dst at a time (rows beyond the grid's by the row loop), so the row's tiles and weights are wave-uniform and every tap is a coalesced
// row-segment load per tile that the strip crosses.  Tile indices and in-tile coordinates are clamped, counts capped at the taps.
__global__ __launch_bounds__(kResampleBlock) void tiles_merge_kernel(const float* __restrict__ tiles, const int32_t* __restrict__ oy,
                                                                     const int32_t* __restrict__ ox, const int32_t* __restrict__ y_start,
                                                                     const int32_t* __restrict__ y_count, const float* __restrict__ y_w,
                                                                     int y_taps, const int32_t* __restrict__ x_start,
                                                                     const int32_t* __restrict__ x_count, const float* __restrict__ x_w,
                                                                     int x_taps, uint8_t* __restrict__ dst, int H, int W, int ky, int kx,
                                                                     int th, int tw) {
  const int X = blockIdx.x * kResampleBlock + threadIdx.x;
  if (X >= W) return;
  const int nx = min(x_count[X], x_taps), sx = x_start[X];
  int64_t xoff[AFX_TILE_MAX_TAPS];                             // per column tap: the tile's offset in the stack + the column inside it
  float wx[AFX_TILE_MAX_TAPS];
#pragma unroll
  for (int b = 0; b < AFX_TILE_MAX_TAPS; ++b) {
    const int ix = min(max(sx + b, 0), kx - 1);
    xoff[b] = (int64_t)ix * 3 * th * tw + min(max(X - ox[ix], 0), tw - 1);
    wx[b] = b < nx ? x_w[(int64_t)X * x_taps + b] : 0.0f;
  }
  const int64_t plane = (int64_t)th * tw;
  for (int Y = blockIdx.y; Y < H; Y += gridDim.y) {
    const int ny = min(y_count[Y], y_taps), sy = y_start[Y];
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int a = 0; a < ny; ++a) {
      const int iy = min(max(sy + a, 0), ky - 1);
      const float wy = y_w[(int64_t)Y * y_taps + a];
      const float* rowp = tiles + (int64_t)iy * kx * 3 * plane + (int64_t)min(max(Y - oy[iy], 0), th - 1) * tw;
      float inner[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int b = 0; b < AFX_TILE_MAX_TAPS; ++b) {
        if (b < nx) {
#pragma unroll
          for (int c = 0; c < 3; ++c) inner[c] = __builtin_fmaf(wx[b], __builtin_fmaf(0.5f, rowp[xoff[b] + c * plane], 0.5f), inner[c]);
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] = __builtin_fmaf(wy, inner[c], acc[c]);
    }
    const int64_t px = ((int64_t)Y * W + X) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[px + c] = (uint8_t)__builtin_rintf(255.0f * fminf(fmaxf(acc[c], 0.0f), 1.0f));
  }
}

// The photo's index of canvas coordinate i (relative to the photo, any int) along an axis of n pixels: the clamp, or the mirror of period
// p = 2 (n - 1) that does not repeat the border (numpy's pad modes 'edge' and 'reflect').  The result is in [0, n - 1] for every i.
AFX_DEV int canvas_src_index(int i, int n, int fill) {
  if (i >= 0 && i < n) return i;
  if (fill == AFX_FILL_EDGE || n == 1) return min(max(i, 0), n - 1);
  const uint32_t p = 2u * (uint32_t)(n - 1);
  uint32_t j;
  if (i >= 0) {
    j = (uint32_t)i % p;
  } else {
    const uint32_t r = (0u - (uint32_t)i) % p;
    j = r ? p - r : 0u;
  }
  return (int)(j < (uint32_t)n ? j : p - j);
}

constexpr int kCanvasFar = INT_MAX;                  // the distance of a pixel that no counted side bounds

// ramp(d) = max(0, 1 - (d + 1) / (blend + 1)): one correctly rounded quotient, one subtraction; 0 for the infinite distance
AFX_DEV float canvas_ramp(int d, int blend) {
  if (d == kCanvasFar) return 0.0f;
  return fmaxf(0.0f, 1.0f - __fdiv_rn((float)(d + 1), (float)((int64_t)blend + 1)));
}

// src uint8 [B, H, W, 3] -> canvas uint8 [B, Hc, Wc, 3] and mask fp32 [Hc, Wc].  One lane per chunk of four consecutive pixels of the flat
// canvas (a chunk may run over a row's or an image's end; the last one may be short), grid-stride.  vec bit 0: canvas is 4-byte aligned,
// so a whole chunk is stored as three dwords; bit 1: mask is 16-byte aligned, so a chunk of the first image is stored as one float4.  Four
// pixels that lie in one row of the photo are loaded as 12 consecutive bytes.  The mask is written by the lanes of the first image alone.
__global__ __launch_bounds__(kResampleBlock) void canvas_extend_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ canvas,
                                                                       float* __restrict__ mask, int H, int W, int left, int top, int right,
                                                                       int bottom, int Hc, int Wc, int fill, int blend, int64_t pixels,
                                                                       int vec) {
  const int64_t plane = (int64_t)Hc * Wc, chunks = (pixels + 3) >> 2;
  for (int64_t i = (int64_t)blockIdx.x * kResampleBlock + threadIdx.x; i < chunks; i += (int64_t)gridDim.x * kResampleBlock) {
    const int64_t p0 = i << 2;
    const int cnt = (int)min((int64_t)4, pixels - p0);
    const int64_t row = p0 / Wc;                                 // b * Hc + y
    int x = (int)(p0 - row * Wc);
    int64_t b = row / Hc;
    int y = (int)(row - b * Hc);
    uint32_t q[12];
    float m[4];
    const int xx0 = x - left, yy0 = y - top;
    if (cnt == 4 && x + 3 < Wc && xx0 >= 0 && xx0 + 3 < W) {     // four pixels of one photo row, or of its mirror above or below
      const uint8_t* s = src + ((b * H + canvas_src_index(yy0, H, fill)) * W + xx0) * 3;
      uint8_t raw[12];
      __builtin_memcpy(raw, s, 12);
#pragma unroll
      for (int k = 0; k < 12; ++k) q[k] = raw[k];
    } else {
      int xs = x, ys = y;
      int64_t bs = b;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        q[3 * j] = q[3 * j + 1] = q[3 * j + 2] = 0;
        if (j < cnt) {
          const uint8_t* s = src + ((bs * H + canvas_src_index(ys - top, H, fill)) * W + canvas_src_index(xs - left, W, fill)) * 3;
          q[3 * j] = s[0]; q[3 * j + 1] = s[1]; q[3 * j + 2] = s[2];
          if (++xs == Wc) {
            xs = 0;
            if (++ys == Hc) { ys = 0; ++bs; }
          }
        }
      }
    }
    uint8_t* c = canvas + p0 * 3;
    if ((vec & 1) && cnt == 4) {
      uint32_t* c4 = reinterpret_cast<uint32_t*>(c);
#pragma unroll
      for (int k = 0; k < 3; ++k) c4[k] = q[4 * k] | (q[4 * k + 1] << 8) | (q[4 * k + 2] << 16) | (q[4 * k + 3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k)
        if (k < 3 * cnt) c[k] = (uint8_t)q[k];
    }
    if (p0 >= plane) continue;                                   // the mask belongs to the first image's lanes
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                // (b == 0 here; a pixel past the plane is not stored)
      const int yy = y - top, xx = x - left;
      float r = 1.0f;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
        int d = kCanvasFar;
        if (left > 0) d = min(d, xx);
        if (right > 0) d = min(d, W - 1 - xx);
        if (top > 0) d = min(d, yy);
        if (bottom > 0) d = min(d, H - 1 - yy);
        r = canvas_ramp(d, blend);
      }
      m[j] = r;
      if (++x == Wc) { x = 0; ++y; }
    }
    if ((vec & 2) && p0 + 4 <= plane) {
      *reinterpret_cast<float4*>(mask + p0) = make_float4(m[0], m[1], m[2], m[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (p0 + j < plane) mask[p0 + j] = m[j];
    }
  }
}

// M fp32 [Hc, Wc], in place on the window (x0, y0, x1, y1): M = min(M, ramp(d)), d the distance to the nearest window side that does not lie
// on the canvas border.  One lane per quad of columns [4 q, 4 q + 4) of one row, rows beyond the grid's by the row loop; vec: Wc is a
// multiple of 4 and M 16-byte aligned, so a quad inside the window is one 16-byte load and store.  No pixel outside the window is touched.
__global__ __launch_bounds__(kResampleBlock) void canvas_mark_kernel(float* __restrict__ M, int Hc, int Wc, int x0, int y0, int x1, int y1,
                                                                     int blend, int vec) {
  const int64_t xa = ((int64_t)(x0 >> 2) + (int64_t)blockIdx.x * kResampleBlock + threadIdx.x) << 2;
  if (xa >= x1) return;
  const bool whole = vec && xa >= x0 && xa + 4 <= x1;
  int dx[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = (int)min(xa + k, (int64_t)x1 - 1);
    int d = kCanvasFar;
    if (x0 > 0) d = min(d, x - x0);
    if (x1 < Wc) d = min(d, x1 - 1 - x);
    dx[k] = d;
  }
  for (int64_t y = (int64_t)y0 + blockIdx.y; y < y1; y += gridDim.y) {
    int dy = kCanvasFar;
    if (y0 > 0) dy = min(dy, (int)y - y0);
    if (y1 < Hc) dy = min(dy, y1 - 1 - (int)y);
    float* rowp = M + y * Wc + xa;
    if (whole) {
      float4 v = *reinterpret_cast<const float4*>(rowp);
      v.x = fminf(v.x, canvas_ramp(min(dx[0], dy), blend));
      v.y = fminf(v.y, canvas_ramp(min(dx[1], dy), blend));
      v.z = fminf(v.z, canvas_ramp(min(dx[2], dy), blend));
      v.w = fminf(v.w, canvas_ramp(min(dx[3], dy), blend));
      *reinterpret_cast<float4*>(rowp) = v;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (xa + k >= x0 && xa + k < x1) rowp[k] = fminf(rowp[k], canvas_ramp(min(dx[k], dy), blend));
    }
  }
}

static double sinc_pi(double x) {     // sin(pi x) / (pi x); its zeros at the non-zero integers are exact, so a same-size table is the identity
  if (x == 0.0) return 1.0;
  if (x == std::floor(x)) return 0.0;
  const double a = x * 3.14159265358979323846;
  return std::sin(a) / a;
}

static double filter_value(int filter, double x) {
  if (filter == AFX_FILTER_LANCZOS3) return (-3.0 <= x && x < 3.0) ? sinc_pi(x) * sinc_pi(x / 3.0) : 0.0;
  x = std::fabs(x);                     // AFX_FILTER_TRIANGLE
  return x < 1.0 ? 1.0 - x : 0.0;
}

}  // namespace afx

using namespace afx;

extern "C" {

int afx_resample_table(int32_t n_in, int32_t n_out, int32_t filter, double b0, double b1, double sigma, int32_t* start, int32_t* count,
                       float* w, int32_t max_taps) {
  const bool query = !start && !count && !w;
  if (!query && (!start || !count || !w))
    return fail(AFX_E_INVALID, "afx_resample_table: start, count and w are given together (all NULL only asks for the tap count)");
  if (n_in < 1 || n_out < 1 || max_taps < 1)
    return fail(AFX_E_INVALID, "bad argument to afx_resample_table (n_in, n_out and max_taps must be >= 1)");
  if (filter != AFX_FILTER_LANCZOS3 && filter != AFX_FILTER_TRIANGLE && filter != AFX_FILTER_GAUSSIAN)
    return fail(AFX_E_INVALID, "afx_resample_table: unknown filter %d", (int)filter);
  const bool gauss = filter == AFX_FILTER_GAUSSIAN;
  double scale = 1.0, fs = 1.0, support = 0.0;
  if (gauss) {
    if (n_in != n_out) return fail(AFX_E_INVALID, "afx_resample_table: the Gaussian keeps the size, got %d -> %d", (int)n_in, (int)n_out);
    if (!(sigma > 0.0) || !std::isfinite(sigma) || !(sigma * sigma > 0.0))          // (a sigma whose square underflows would give exp(-0 / 0))
      return fail(AFX_E_INVALID, "afx_resample_table: sigma must be positive and finite, and so must its square");
    b0 = 0.0;
    support = std::ceil(3.0 * sigma);
  } else {
    if (!(b0 >= 0.0) || !(b1 > b0) || !(b1 <= (double)n_in))
      return fail(AFX_E_INVALID, "afx_resample_table: the box [%g, %g) must be non-empty and inside [0, %d]", b0, b1, (int)n_in);
    scale = (b1 - b0) / n_out;
    fs = std::max(scale, 1.0);
    support = (filter == AFX_FILTER_LANCZOS3 ? 3.0 : 1.0) * fs;
  }
  if (!(support < 1e9)) return fail(AFX_E_UNSUPPORTED, "afx_resample_table: the filter's support is out of range");
  int32_t taps = 0;
  std::vector<double> row;
  for (int pass = 0; pass < (query ? 1 : 2); ++pass) {         // pass 0: the tap count, pass 1: the tables
    for (int32_t i = 0; i < n_out; ++i) {
      const double c = b0 + (i + 0.5) * scale;
      int64_t lo, hi;
      if (gauss) {
        lo = std::max<int64_t>(0, (int64_t)i - (int64_t)support);
        hi = std::min<int64_t>(n_in, (int64_t)i + (int64_t)support + 1);
      } else {
        lo = std::max<int64_t>(0, (int64_t)(c - support + 0.5));         // the casts truncate, as Pillow's (int)
        hi = std::min<int64_t>(n_in, (int64_t)(c + support + 0.5));
      }
      if (hi <= lo) return fail(AFX_E_INVALID, "afx_resample_table: output %d has an empty window", (int)i);
      if (pass == 0) {
        taps = (int32_t)std::max<int64_t>(taps, std::min<int64_t>(hi - lo, (int64_t)AFX_RESAMPLE_MAX_TAPS + 1));
        continue;
      }
      const int32_t n = (int32_t)(hi - lo);
      row.assign(n, 0.0);
      double sum = 0.0;
      for (int32_t k = 0; k < n; ++k) {
        if (gauss) {
          const double d = (double)(k + lo - i);
          row[k] = std::exp(-d * d / (2.0 * sigma * sigma));
        } else {
          row[k] = filter_value(filter, (k + lo - c + 0.5) / fs);
        }
        sum += row[k];
      }
      if (!(std::fabs(sum) > 0.0) || !std::isfinite(sum))
        return fail(AFX_E_INVALID, "afx_resample_table: the weights of output %d sum to zero or are not finite", (int)i);
      start[i] = (int32_t)lo;
      count[i] = n;
      for (int32_t k = 0; k < max_taps; ++k) w[(int64_t)i * max_taps + k] = k < n ? (float)(row[k] / sum) : 0.0f;
    }
    if (pass == 0) {
      if (taps > AFX_RESAMPLE_MAX_TAPS)
        return fail(AFX_E_UNSUPPORTED, "afx_resample_table: the filter needs more than AFX_RESAMPLE_MAX_TAPS = %d taps (%d -> %d is too large a ratio)",
                    (int)AFX_RESAMPLE_MAX_TAPS, (int)n_in, (int)n_out);
      if (taps > max_taps) return fail(AFX_E_INVALID, "afx_resample_table: the filter needs %d taps, max_taps is %d", (int)taps, (int)max_taps);
    }
  }
  return taps;
}

int64_t afx_image_resample_ws_bytes(int32_t batch, int32_t C, int32_t H_in, int32_t W_out) {
  if (batch < 1 || (C != 1 && C != 3) || H_in < 1 || W_out < 1)
    return fail(AFX_E_INVALID, "bad argument to afx_image_resample_ws_bytes (batch, H_in, W_out >= 1, C 1 or 3)");
  return (int64_t)batch * C * H_in * W_out * 4;
}

int afx_image_resample(const void* src, int32_t src_u8, int32_t batch, int32_t C, int32_t H_in, int32_t W_in, const int32_t* h_start,
                       const int32_t* h_count, const float* h_w, int32_t h_taps, const int32_t* v_start, const int32_t* v_count,
                       const float* v_w, int32_t v_taps, float* dst, int32_t H_out, int32_t W_out, int32_t clamp, void* ws,
                       int64_t ws_bytes, void* stream) {
  if (!src || !dst || !h_start || !h_count || !h_w || !v_start || !v_count || !v_w)
    return fail(AFX_E_INVALID, "null argument to afx_image_resample (src, dst and both axes' start, count and w are required)");
  if (C != 1 && C != 3) return fail(AFX_E_INVALID, "afx_image_resample: C must be 1 or 3, got %d", (int)C);
  if (batch < 1 || H_in < 1 || W_in < 1 || H_out < 1 || W_out < 1)
    return fail(AFX_E_INVALID, "bad argument to afx_image_resample (batch and every size must be >= 1)");
  if (h_taps < 1 || v_taps < 1 || h_taps > AFX_RESAMPLE_MAX_TAPS || v_taps > AFX_RESAMPLE_MAX_TAPS)
    return fail(AFX_E_INVALID, "afx_image_resample: h_taps and v_taps must be in [1, %d], got %d and %d", (int)AFX_RESAMPLE_MAX_TAPS,
                (int)h_taps, (int)v_taps);
  if ((!src_u8 && ((uintptr_t)src & 3)) || ((uintptr_t)dst & 3) || ((uintptr_t)ws & 3) || ((uintptr_t)h_start & 3) || ((uintptr_t)h_count & 3) ||
      ((uintptr_t)h_w & 3) || ((uintptr_t)v_start & 3) || ((uintptr_t)v_count & 3) || ((uintptr_t)v_w & 3))
    return fail(AFX_E_INVALID, "afx_image_resample: an fp32 src, dst, ws and the tables must be 4-byte aligned");
  const int64_t need = (int64_t)batch * C * H_in * W_out * 4;
  if (!ws || ws_bytes < need)
    return fail(AFX_E_WORKSPACE, "afx_image_resample: workspace missing or too small (%lld bytes, need afx_image_resample_ws_bytes = %lld)",
                (long long)(ws ? ws_bytes : 0), (long long)need);
  const int64_t sbytes = (int64_t)batch * C * H_in * W_in * (src_u8 ? 1 : 4), dbytes = (int64_t)batch * C * H_out * W_out * 4;
  const void* ops[] = {src, h_start, h_count, h_w, v_start, v_count, v_w};
  const int64_t obytes[] = {sbytes,          (int64_t)W_out * 4, (int64_t)W_out * 4,         (int64_t)W_out * h_taps * 4,
                            (int64_t)H_out * 4, (int64_t)H_out * 4, (int64_t)H_out * v_taps * 4};
  for (int i = 0; i < 7; ++i)
    if (ranges_overlap(dst, dbytes, ops[i], obytes[i]) || ranges_overlap(ws, need, ops[i], obytes[i]))
      return fail(AFX_E_INVALID, "afx_image_resample: dst or ws overlaps the source or a table");
  if (ranges_overlap(dst, dbytes, ws, need)) return fail(AFX_E_INVALID, "afx_image_resample: dst overlaps ws");

  const hipStream_t st = (hipStream_t)stream;
  const unsigned gx = (unsigned)((W_out + kResampleBlock - 1) / kResampleBlock);
  const int64_t hrows = (int64_t)batch * (src_u8 ? 1 : C) * H_in;
  const dim3 hgrid(gx, (unsigned)std::min(hrows, kResampleMaxRows));
  float* wsf = (float*)ws;
  if (!src_u8)
    hipLaunchKernelGGL((resample_h_kernel<false, 1>), hgrid, dim3(kResampleBlock), 0, st, src, h_start, h_count, h_w, h_taps, wsf, hrows, H_in,
                       W_in, W_out);
  else if (C == 3)
    hipLaunchKernelGGL((resample_h_kernel<true, 3>), hgrid, dim3(kResampleBlock), 0, st, src, h_start, h_count, h_w, h_taps, wsf, hrows, H_in,
                       W_in, W_out);
  else
    hipLaunchKernelGGL((resample_h_kernel<true, 1>), hgrid, dim3(kResampleBlock), 0, st, src, h_start, h_count, h_w, h_taps, wsf, hrows, H_in,
                       W_in, W_out);
  HIP_TRY(hipGetLastError());
  const int64_t vrows = (int64_t)batch * C * H_out;
  hipLaunchKernelGGL(resample_v_kernel, dim3(gx, (unsigned)std::min(vrows, kResampleMaxRows)), dim3(kResampleBlock), 0, st, wsf, v_start,
                     v_count, v_w, v_taps, dst, vrows, H_in, H_out, W_out, clamp);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

int afx_mask_bbox(const void* mask, int32_t mask_u8, int32_t batch, int32_t H, int32_t W, int32_t* bbox, void* stream) {
  if (!mask || !bbox) return fail(AFX_E_INVALID, "null argument to afx_mask_bbox (mask and bbox are required)");
  if (batch < 1 || H < 1 || W < 1) return fail(AFX_E_INVALID, "bad argument to afx_mask_bbox (batch, H and W must be >= 1)");
  if (batch > (int32_t)kResampleMaxRows) return fail(AFX_E_INVALID, "afx_mask_bbox: batch must be <= %d", (int)kResampleMaxRows);
  if ((!mask_u8 && ((uintptr_t)mask & 3)) || ((uintptr_t)bbox & 3))
    return fail(AFX_E_INVALID, "afx_mask_bbox: an fp32 mask and bbox must be 4-byte aligned");
  const int64_t n = (int64_t)H * W;
  if (ranges_overlap(bbox, (int64_t)batch * 16, mask, (int64_t)batch * n * (mask_u8 ? 1 : 4)))
    return fail(AFX_E_INVALID, "afx_mask_bbox: bbox overlaps the mask");
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mask_bbox_init_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, st, bbox, batch, H, W);
  HIP_TRY(hipGetLastError());
  const dim3 grid((unsigned)std::min<int64_t>((n + kResampleBlock - 1) / kResampleBlock, kBboxMaxBlocks), (unsigned)batch);
  if (mask_u8)
    hipLaunchKernelGGL(mask_bbox_kernel<true>, grid, dim3(kResampleBlock), 0, st, mask, bbox, H, W);
  else
    hipLaunchKernelGGL(mask_bbox_kernel<false>, grid, dim3(kResampleBlock), 0, st, mask, bbox, H, W);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

int64_t afx_image_paste_ws_bytes(int32_t batch, int32_t mask_batch, int32_t h, int32_t win_w) {
  if (batch < 1 || mask_batch < 0 || (mask_batch > 1 && mask_batch != batch) || h < 1 || win_w < 1)
    return fail(AFX_E_INVALID, "bad argument to afx_image_paste_ws_bytes (batch, h, win_w >= 1; mask_batch 0 (no mask), 1 or batch)");
  return ((int64_t)batch * 3 + mask_batch) * h * win_w * 4;
}

int afx_image_paste(const float* img, const float* mask, int32_t mask_batch, const void* src, void* dst, int32_t batch, int32_t h, int32_t w,
                    int32_t H, int32_t W, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t n_out_w, int32_t n_out_h,
                    const int32_t* ih_start, const int32_t* ih_count, const float* ih_w, int32_t ih_taps, const int32_t* iv_start,
                    const int32_t* iv_count, const float* iv_w, int32_t iv_taps, const int32_t* mh_start, const int32_t* mh_count,
                    const float* mh_w, int32_t mh_taps, const int32_t* mv_start, const int32_t* mv_count, const float* mv_w, int32_t mv_taps,
                    void* ws, int64_t ws_bytes, void* stream) {
  if (!img || !src || !dst || !ih_start || !ih_count || !ih_w || !iv_start || !iv_count || !iv_w)
    return fail(AFX_E_INVALID, "null argument to afx_image_paste (img, src, dst and both axes' image tables are required)");
  if (mask && (!mh_start || !mh_count || !mh_w || !mv_start || !mv_count || !mv_w))
    return fail(AFX_E_INVALID, "null argument to afx_image_paste (a mask needs both axes' mask tables)");
  if (batch < 1 || h < 1 || w < 1 || H < 1 || W < 1)
    return fail(AFX_E_INVALID, "bad argument to afx_image_paste (batch and every size must be >= 1)");
  if (mask ? (mask_batch != 1 && mask_batch != batch) : mask_batch != 0)
    return fail(AFX_E_INVALID, "afx_image_paste: mask_batch must be 1 or batch with a mask and 0 without, got %d", (int)mask_batch);
  if (x0 < 0 || y0 < 0 || x1 <= x0 || y1 <= y0 || x1 > W || y1 > H)
    return fail(AFX_E_INVALID, "afx_image_paste: the window (%d, %d, %d, %d) must be non-empty and inside the %d x %d source", (int)x0, (int)y0,
                (int)x1, (int)y1, (int)H, (int)W);
  if (x1 - x0 != n_out_w || y1 - y0 != n_out_h)
    return fail(AFX_E_INVALID, "afx_image_paste: the window is %d x %d, the tables are for %d x %d", (int)(y1 - y0), (int)(x1 - x0), (int)n_out_h,
                (int)n_out_w);
  const int32_t taps[] = {ih_taps, iv_taps, mh_taps, mv_taps};
  for (int i = 0; i < (mask ? 4 : 2); ++i)
    if (taps[i] < 1 || taps[i] > AFX_RESAMPLE_MAX_TAPS)
      return fail(AFX_E_INVALID, "afx_image_paste: every tap count must be in [1, %d], got %d", (int)AFX_RESAMPLE_MAX_TAPS, (int)taps[i]);
  const int ww = x1 - x0, wh = y1 - y0;
  const void* tabs[] = {ih_start, ih_count, ih_w, iv_start, iv_count, iv_w, mh_start, mh_count, mh_w, mv_start, mv_count, mv_w};
  const int64_t tbytes[] = {(int64_t)ww * 4, (int64_t)ww * 4, (int64_t)ww * ih_taps * 4, (int64_t)wh * 4, (int64_t)wh * 4, (int64_t)wh * iv_taps * 4,
                            (int64_t)ww * 4, (int64_t)ww * 4, (int64_t)ww * mh_taps * 4, (int64_t)wh * 4, (int64_t)wh * 4, (int64_t)wh * mv_taps * 4};
  const int ntabs = mask ? 12 : 6;
  uintptr_t bits = (uintptr_t)img | (uintptr_t)mask | (uintptr_t)ws;
  for (int i = 0; i < ntabs; ++i) bits |= (uintptr_t)tabs[i];
  if (bits & 3) return fail(AFX_E_INVALID, "afx_image_paste: img, mask, ws and the tables must be 4-byte aligned");
  const int64_t need = ((int64_t)batch * 3 + mask_batch) * h * ww * 4;
  if (!ws || ws_bytes < need)
    return fail(AFX_E_WORKSPACE, "afx_image_paste: workspace missing or too small (%lld bytes, need afx_image_paste_ws_bytes = %lld)",
                (long long)(ws ? ws_bytes : 0), (long long)need);
  const int64_t ibytes = (int64_t)batch * 3 * h * w * 4, mbytes = (int64_t)mask_batch * h * w * 4, sbytes = (int64_t)batch * H * W * 3;
  if (ranges_overlap(dst, sbytes, src, sbytes) || ranges_overlap(dst, sbytes, img, ibytes) || ranges_overlap(dst, sbytes, mask, mbytes) ||
      ranges_overlap(dst, sbytes, ws, need) || ranges_overlap(ws, need, src, sbytes) || ranges_overlap(ws, need, img, ibytes) ||
      ranges_overlap(ws, need, mask, mbytes))
    return fail(AFX_E_INVALID, "afx_image_paste: dst or ws overlaps an operand, or each other");
  for (int i = 0; i < ntabs; ++i)
    if (ranges_overlap(dst, sbytes, tabs[i], tbytes[i]) || ranges_overlap(ws, need, tabs[i], tbytes[i]))
      return fail(AFX_E_INVALID, "afx_image_paste: dst or ws overlaps a table");

  const hipStream_t st = (hipStream_t)stream;
  const dim3 block(kResampleBlock);
  const unsigned gx = (unsigned)((ww + kResampleBlock - 1) / kResampleBlock);
  float* ws_img = (float*)ws;
  float* ws_mask = mask ? ws_img + (int64_t)batch * 3 * h * ww : nullptr;
  const int64_t irows = (int64_t)batch * 3 * h, mrows = (int64_t)mask_batch * h;
  hipLaunchKernelGGL((resample_h_kernel<false, 1>), dim3(gx, (unsigned)std::min(irows, kResampleMaxRows)), block, 0, st, (const void*)img,
                     ih_start, ih_count, ih_w, ih_taps, ws_img, irows, h, w, ww);
  HIP_TRY(hipGetLastError());
  if (mask) {
    hipLaunchKernelGGL((resample_h_kernel<false, 1>), dim3(gx, (unsigned)std::min(mrows, kResampleMaxRows)), block, 0, st, (const void*)mask,
                       mh_start, mh_count, mh_w, mh_taps, ws_mask, mrows, h, w, ww);
    HIP_TRY(hipGetLastError());
  }
  const int64_t rows = (int64_t)batch * H;
  hipLaunchKernelGGL(paste_kernel, dim3((unsigned)((W + kResampleBlock - 1) / kResampleBlock), (unsigned)std::min(rows, kResampleMaxRows)), block,
                     0, st, ws_img, ws_mask, (const uint8_t*)src, (uint8_t*)dst, iv_start, iv_count, iv_w, iv_taps, mv_start, mv_count, mv_w,
                     mv_taps, rows, mask_batch, h, H, W, x0, y0, x1, y1);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

// what afx_tiles_cut and afx_tiles_merge ask of the geometry they share
static int tiles_geometry_check(const char* name, int32_t H, int32_t W, int32_t ky, int32_t kx, int32_t th, int32_t tw) {
  if (H < 1 || W < 1 || ky < 1 || kx < 1 || th < 1 || tw < 1)
    return fail(AFX_E_INVALID, "bad argument to %s (H, W, ky, kx, th and tw must be >= 1)", name);
  if ((th & 15) || (tw & 15) || th > H || tw > W)
    return fail(AFX_E_INVALID, "%s: th and tw must be multiples of 16 inside the %d x %d canvas, got %d x %d", name, (int)H, (int)W, (int)th,
                (int)tw);
  if ((int64_t)ky * kx > INT32_MAX / 3) return fail(AFX_E_INVALID, "%s: too many tiles (%d x %d)", name, (int)ky, (int)kx);
  return AFX_OK;
}

int afx_tiles_cut(const float* canvas, int32_t H, int32_t W, const int32_t* oy, int32_t ky, const int32_t* ox, int32_t kx, int32_t th,
                  int32_t tw, float* tiles, void* stream) {
  if (!canvas || !oy || !ox || !tiles) return fail(AFX_E_INVALID, "null argument to afx_tiles_cut (canvas, oy, ox and tiles are required)");
  AFX_TRY(tiles_geometry_check("afx_tiles_cut", H, W, ky, kx, th, tw));
  if ((((uintptr_t)canvas | (uintptr_t)oy | (uintptr_t)ox) & 3) || ((uintptr_t)tiles & 15))
    return fail(AFX_E_INVALID, "afx_tiles_cut: canvas, oy and ox must be 4-byte aligned and tiles 16-byte aligned");
  const int64_t tbytes = (int64_t)ky * kx * 3 * th * tw * 4;
  if (ranges_overlap(tiles, tbytes, canvas, (int64_t)3 * H * W * 4) || ranges_overlap(tiles, tbytes, oy, (int64_t)ky * 4) ||
      ranges_overlap(tiles, tbytes, ox, (int64_t)kx * 4))
    return fail(AFX_E_INVALID, "afx_tiles_cut: tiles overlaps the canvas or an origin list");
  const int64_t chunks = tbytes / 16;
  const unsigned grid = (unsigned)std::min<int64_t>((chunks + kResampleBlock - 1) / kResampleBlock, kTilesCutMaxBlocks);
  hipLaunchKernelGGL(tiles_cut_kernel, dim3(grid), dim3(kResampleBlock), 0, (hipStream_t)stream, canvas, oy, ox, tiles, H, W, ky, kx, th, tw,
                     chunks);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

int afx_tiles_merge(const float* tiles, int32_t T, int32_t th, int32_t tw, const int32_t* oy, int32_t ky, const int32_t* ox, int32_t kx,
                    const int32_t* y_start, const int32_t* y_count, const float* y_w, int32_t y_taps, const int32_t* x_start,
                    const int32_t* x_count, const float* x_w, int32_t x_taps, void* dst, int32_t H, int32_t W, void* stream) {
  if (!tiles || !oy || !ox || !y_start || !y_count || !y_w || !x_start || !x_count || !x_w || !dst)
    return fail(AFX_E_INVALID, "null argument to afx_tiles_merge (tiles, oy, ox, both axes' start, count and w, and dst are required)");
  AFX_TRY(tiles_geometry_check("afx_tiles_merge", H, W, ky, kx, th, tw));
  if ((int64_t)T != (int64_t)ky * kx) return fail(AFX_E_INVALID, "afx_tiles_merge: T = %d tiles, the plan has ky kx = %d x %d", (int)T, (int)ky, (int)kx);
  if (y_taps < 1 || x_taps < 1 || y_taps > AFX_TILE_MAX_TAPS || x_taps > AFX_TILE_MAX_TAPS)
    return fail(AFX_E_INVALID, "afx_tiles_merge: y_taps and x_taps must be in [1, AFX_TILE_MAX_TAPS = %d], got %d and %d", (int)AFX_TILE_MAX_TAPS,
                (int)y_taps, (int)x_taps);
  const void* ops[] = {tiles, oy, ox, y_start, y_count, y_w, x_start, x_count, x_w};
  const int64_t obytes[] = {(int64_t)T * 3 * th * tw * 4, (int64_t)ky * 4, (int64_t)kx * 4,           (int64_t)H * 4, (int64_t)H * 4,
                            (int64_t)H * y_taps * 4,      (int64_t)W * 4,  (int64_t)W * 4,            (int64_t)W * x_taps * 4};
  uintptr_t bits = 0;
  for (int i = 0; i < 9; ++i) bits |= (uintptr_t)ops[i];
  if (bits & 3) return fail(AFX_E_INVALID, "afx_tiles_merge: tiles, the origin lists and the tables must be 4-byte aligned");
  for (int i = 0; i < 9; ++i)
    if (ranges_overlap(dst, (int64_t)H * W * 3, ops[i], obytes[i])) return fail(AFX_E_INVALID, "afx_tiles_merge: dst overlaps the tiles or a table");
  const dim3 grid((unsigned)((W + kResampleBlock - 1) / kResampleBlock), (unsigned)std::min<int64_t>(H, kResampleMaxRows));
  hipLaunchKernelGGL(tiles_merge_kernel, grid, dim3(kResampleBlock), 0, (hipStream_t)stream, tiles, oy, ox, y_start, y_count, y_w, y_taps, x_start,
                     x_count, x_w, x_taps, (uint8_t*)dst, H, W, ky, kx, th, tw);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

int afx_canvas_extend(const void* src, int32_t batch, int32_t H, int32_t W, int32_t left, int32_t top, int32_t right, int32_t bottom,
                      int32_t fill, int32_t blend, void* canvas, float* mask, void* stream) {
  if (!src || !canvas || !mask) return fail(AFX_E_INVALID, "null argument to afx_canvas_extend (src, canvas and mask are required)");
  if (batch < 1 || H < 1 || W < 1) return fail(AFX_E_INVALID, "bad argument to afx_canvas_extend (batch, H and W must be >= 1)");
  if (fill != AFX_FILL_EDGE && fill != AFX_FILL_REFLECT) return fail(AFX_E_INVALID, "afx_canvas_extend: unknown fill %d", (int)fill);
  if (left < 0 || top < 0 || right < 0 || bottom < 0 || !(left | top | right | bottom))
    return fail(AFX_E_INVALID, "afx_canvas_extend: the extents (%d, %d, %d, %d) must be >= 0 and one of them > 0", (int)left, (int)top,
                (int)right, (int)bottom);
  if (blend < 0) return fail(AFX_E_INVALID, "afx_canvas_extend: blend must be >= 0, got %d", (int)blend);
  const int64_t Hc = (int64_t)H + top + bottom, Wc = (int64_t)W + left + right;
  if (Hc > INT32_MAX || Wc > INT32_MAX || Hc * Wc > INT64_MAX / 16 / batch)
    return fail(AFX_E_INVALID, "afx_canvas_extend: the canvas %lld x %lld is past the launch grid's index range (sides below 2^31, batch Hc Wc below 2^59)",
                (long long)Hc, (long long)Wc);
  if ((uintptr_t)mask & 3) return fail(AFX_E_INVALID, "afx_canvas_extend: mask must be 4-byte aligned");
  const int64_t sbytes = (int64_t)batch * H * W * 3, cbytes = (int64_t)batch * Hc * Wc * 3, mbytes = Hc * Wc * 4;
  if (ranges_overlap(canvas, cbytes, src, sbytes) || ranges_overlap(mask, mbytes, src, sbytes) || ranges_overlap(mask, mbytes, canvas, cbytes))
    return fail(AFX_E_INVALID, "afx_canvas_extend: canvas or mask overlaps src, or each other");
  const int64_t pixels = (int64_t)batch * Hc * Wc, chunks = (pixels + 3) / 4;
  const unsigned grid = (unsigned)std::min<int64_t>((chunks + kResampleBlock - 1) / kResampleBlock, kTilesCutMaxBlocks);
  const int vec = (((uintptr_t)canvas & 3) == 0 ? 1 : 0) | (((uintptr_t)mask & 15) == 0 ? 2 : 0);
  hipLaunchKernelGGL(canvas_extend_kernel, dim3(grid), dim3(kResampleBlock), 0, (hipStream_t)stream, (const uint8_t*)src, (uint8_t*)canvas, mask,
                     H, W, left, top, right, bottom, (int)Hc, (int)Wc, fill, blend, pixels, vec);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

int afx_canvas_mark(float* mask, int32_t Hc, int32_t Wc, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t blend, void* stream) {
  if (!mask) return fail(AFX_E_INVALID, "null argument to afx_canvas_mark (mask is required)");
  if (Hc < 1 || Wc < 1) return fail(AFX_E_INVALID, "bad argument to afx_canvas_mark (Hc and Wc must be >= 1)");
  if (x0 < 0 || y0 < 0 || x1 <= x0 || y1 <= y0 || x1 > Wc || y1 > Hc)
    return fail(AFX_E_INVALID, "afx_canvas_mark: the window (%d, %d, %d, %d) must be non-empty and inside the %d x %d canvas", (int)x0, (int)y0,
                (int)x1, (int)y1, (int)Hc, (int)Wc);
  if (blend < 0) return fail(AFX_E_INVALID, "afx_canvas_mark: blend must be >= 0, got %d", (int)blend);
  if ((uintptr_t)mask & 3) return fail(AFX_E_INVALID, "afx_canvas_mark: mask must be 4-byte aligned");
  const int quads = ((x1 - 1) >> 2) - (x0 >> 2) + 1;
  const dim3 grid((unsigned)((quads + kResampleBlock - 1) / kResampleBlock), (unsigned)std::min<int64_t>(y1 - y0, kResampleMaxRows));
  const int vec = (Wc & 3) == 0 && ((uintptr_t)mask & 15) == 0;
  hipLaunchKernelGGL(canvas_mark_kernel, grid, dim3(kResampleBlock), 0, (hipStream_t)stream, mask, Hc, Wc, x0, y0, x1, y1, blend, vec);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

}  // extern "C"
