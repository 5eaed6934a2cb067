// Image editing (image-to-image and inpainting on the ArcFlow pipelines): the one pass that runs between two student steps, on the
// packed token layout the engine reads and writes.
//   * edit_blend_kernel: the forward diffusion of the source latents to the sigma the step landed on, the per-latent-pixel blend
//     with the sampler's latents, and the bf16 copy the next forward reads:
//       om    = 1 - sigma_to[b]
//       known = noise ? fma(sigma_to[b], noise, om x0) : om x0
//       x_out = mask ? fma(m, x, (1 - m) known) : known
//     (edit_blend8, afx_common.h: the function the fused teacher_edit_step_kernel of afx_sampler.hip calls too)
//     A token is 64 channels = 16 latent channels x the 2 x 2 patch, channel = c*4 + ph*2 + pw, and the mask holds one value per
//     latent pixel of the patch: element e of a token reads mask[b, tok, e & 3].  A chunk of 8 consecutive elements starts at a
//     multiple of 8, so its elements read mask values 0 1 2 3 0 1 2 3: one 16-byte load of the token's mask row per chunk.
//     16 B per lane and operand (two float4 of x, x0, noise, one of the mask), grid-stride, no LDS, no atomics.  Traffic at
//     1024 x 1024 (4096 tokens x 64 channels = 262144 elements per image): 4 (x) + 4 (x0) + 4 (noise) B read, 4 (x') + 2 (bf16 x') B
//     written per element and 16 B of mask per token (0.25 B per element, the re-reads of the 8 chunks of a token hit the cache)
//     = 18 B, about 4.7 MB per image and step.
//   The products are written so that m = 1 returns x, m = 0 returns known, sigma_to = 1 returns noise and sigma_to = 0 returns x0
//   bit for bit (finite inputs): each of them multiplies the other term by an exact 0 and the kept term by an exact 1.
#include "afx_api_util.h"
#include "afx_common.h"

namespace afx {

// One chunk = 8 consecutive elements of one token (64 channels per token: a chunk never straddles two tokens or two samples).
__global__ __launch_bounds__(256) void edit_blend_kernel(const float* x, const float* __restrict__ x0, const float* __restrict__ noise,
                                                         const float* __restrict__ mask, const float* __restrict__ sigma_to, float* x_out,
                                                         bf16_t* __restrict__ x_bf16, int64_t chunks_per_sample, int64_t chunks) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < chunks; c += stride) {
    const int64_t b = c / chunks_per_sample;
    const float sg = sigma_to[b];
    float a[8], z[8], v[8], o[8];
    f32x4_t mk = {0.f, 0.f, 0.f, 0.f};
    load8(x0 + c * 8, a);
    if (noise != nullptr) load8(noise + c * 8, z);
    if (mask != nullptr) {
      load8(x + c * 8, v);          // (x_out may be x: every load precedes every store)
      mk = *reinterpret_cast<const f32x4_t*>(mask + (c >> 3) * 4);
    }
    edit_blend8(v, a, z, mk, noise != nullptr, mask != nullptr, sg, o);
    store8(x_out + c * 8, o);
    if (x_bf16 != nullptr) *reinterpret_cast<u32x4_t*>(x_bf16 + c * 8) = pack8(o);
  }
}

}  // namespace afx

using namespace afx;

extern "C" {

int afx_edit_blend(const float* x, const float* x0, const float* noise, const float* mask, const float* sigma_to, float* x_out,
                   void* x_out_bf16, int32_t batch, int32_t n_tok, int32_t ch, int32_t max_blocks, void* stream) {
  if (!x0 || !x_out || !sigma_to || (mask && !x))
    return fail(AFX_E_INVALID, "null argument to afx_edit_blend (x0, x_out and sigma_to are required, x whenever mask is given)");
  if (ch != 64) return fail(AFX_E_INVALID, "afx_edit_blend: ch must be 64 (16 latent channels x the 2 x 2 patch), got %d", (int)ch);
  if (batch < 1 || n_tok < 1 || max_blocks < 0)
    return fail(AFX_E_INVALID, "bad argument to afx_edit_blend (batch and n_tok must be >= 1, max_blocks >= 0)");
  if (misaligned16({x, x0, noise, mask, sigma_to, x_out, x_out_bf16}))
    return fail(AFX_E_INVALID, "afx_edit_blend: x, x0, noise, mask, sigma_to, x_out and x_out_bf16 must be 16-byte aligned");
  const int64_t elems = (int64_t)batch * n_tok * 64;
  const int64_t fbytes = elems * 4, hbytes = elems * 2, mbytes = (int64_t)batch * n_tok * 16, sbytes = (int64_t)batch * 4;
  // every lane reads its own 8 elements before it writes them, so x_out == x is safe; any other overlap lets one lane's store
  // land in another lane's load
  if ((x != x_out && mask != nullptr && ranges_overlap(x_out, fbytes, x, fbytes)) || ranges_overlap(x_out, fbytes, x0, fbytes) ||
      ranges_overlap(x_out, fbytes, noise, fbytes) || ranges_overlap(x_out, fbytes, mask, mbytes) ||
      ranges_overlap(x_out, fbytes, sigma_to, sbytes) || ranges_overlap(x_out, fbytes, x_out_bf16, hbytes))
    return fail(AFX_E_INVALID, "afx_edit_blend: x_out overlaps another operand (only x_out == x is allowed)");
  if ((mask != nullptr && ranges_overlap(x_out_bf16, hbytes, x, fbytes)) || ranges_overlap(x_out_bf16, hbytes, x0, fbytes) ||
      ranges_overlap(x_out_bf16, hbytes, noise, fbytes) || ranges_overlap(x_out_bf16, hbytes, mask, mbytes) ||
      ranges_overlap(x_out_bf16, hbytes, sigma_to, sbytes))
    return fail(AFX_E_INVALID, "afx_edit_blend: x_out_bf16 overlaps an input");
  return launch_step(edit_blend_kernel, batch, (int64_t)n_tok * 64, max_blocks, stream, mask != nullptr ? x : nullptr, x0, noise, mask, sigma_to,
                     x_out, (bf16_t*)x_out_bf16);
}

}  // extern "C"
