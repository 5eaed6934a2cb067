// Teacher sampling (GaussianFlow.forward_test, lakonlab/models/diffusions/gaussian_flow.py:149-222): what runs between two
// teacher forwards of the sampler's loop, on the packed token layout the engine reads and writes.
//   * teacher_euler_step_kernel: true-CFG combine (guidance_jit, gaussian_flow.py:18-26) + FlowEulerODEScheduler.step
//     (schedulers/flow_euler_ode.py:141-150) + the bf16 copy of the new latents the next forward reads, in one pass:
//     16 B per lane and operand (8 bf16 of pos / neg, two float4 of x), grid-stride, no LDS, no atomics.
//   * teacher_sde_step_kernel: the same combine + FlowSDEScheduler.step (schedulers/flow_sde.py:143-166) + the bf16 copy, in one
//     pass of the same shape.  The scheduler's per-step scalars (sigma, sigma_to, m, c_noise = sqrt(max(1 - m^2, 0))) come from the
//     host (FlowSDEScheduler.coefficients: the pow is evaluated once per step in the reference's arithmetic); the fresh noise z is
//     an fp32 operand drawn by torch, so that a torch.Generator reproduces the run.  Traffic at 1024 x 1024 (4096 tokens x 64
//     channels = 262144 elements per image): 4 (x) + 2 (pos) + 2 (neg) + 4 (z) B read and 4 (x') + 2 (bf16 x') B written per
//     element = 18 B, about 4.7 MB per image and step.
//   * teacher_unipc_step_kernel: the same combine + one predictor-corrector step of the UniPC multistep solver (FlowUniPCScheduler) + the bf16
//     copy + the solver's state (the corrected sample, the clean-sample prediction into the host's history ring), in one pass of the same
//     shape; the host hands over one fp32 weight per operand.  Formula, fma order and traffic at the kernel.
//   * teacher_edit_step_kernel<SDE>: either step + the inpainting blend of afx_edit.hip at the sigma the step lands on + the bf16 copy,
//     in one pass of the same shape (teacher image-to-image / inpainting); formula and traffic at the kernel.
//   * cfg_ortho_partial_kernel / cfg_ortho_finish_kernel: the per-sample projection coefficient of orthogonal guidance,
//     mean(bias pos) / max(mean(pos pos), 1e-6) over all n elements of a sample, on the reduction of afx_reduce.h: a fixed number of
//     work-groups per sample (a function of n alone), every product exact in fp64, one workspace slot per work-group, the slots added
//     in index order by the second launch: bit-reproducible.
#include "afx_api_util.h"
#include "afx_common.h"
#include "afx_reduce.h"

namespace afx {

// The guided velocity of one element, one function for every step kernel so that the CFG arithmetic cannot drift between them:
//   u = pos                                  no guidance on this step
//   u = pos + (pos - neg) (scale - 1)        true CFG (guidance_jit, orthogonal off)
//   u = u - coef pos                         orthogonal guidance: the projection on pos removed (coef from afx_cfg_ortho_coef)
AFX_DEV float cfg_velocity(const float (&p)[8], const float (&q)[8], int e, bool has_neg, bool has_coef, float sm1, float cf) {
  float u = p[e];
  if (has_neg) u = p[e] + (p[e] - q[e]) * sm1;
  if (has_coef) u = u - cf * p[e];
  return u;
}

// FlowEulerODEScheduler.step on one chunk, u formed on the way:  o = x + u (sigma_to - sigma).  (q is read only with has_neg.)
AFX_DEV void euler_update8(const float (&x)[8], const float (&p)[8], const float (&q)[8], bool has_neg, bool has_coef, float sm1, float cf,
                           float sg, float sg_to, float (&o)[8]) {
  const float dt = sg_to - sg;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float u = cfg_velocity(p, q, e, has_neg, has_coef, sm1, cf);
    o[e] = x[e] + u * dt;
  }
}

// FlowSDEScheduler.step, prediction_type 'u', on one chunk:
//   x0 = x - sigma u,   eps = x + (1 - sigma) u,   o = (1 - sigma_to) x0 + sigma_to (m eps + c_noise z)
// has_noise false: the term c_noise z is skipped (z is not read; the host passes no noise when sigma_to c_noise = 0 for every sample).
AFX_DEV void sde_update8(const float (&x)[8], const float (&p)[8], const float (&q)[8], const float (&z)[8], bool has_neg, bool has_coef,
                         bool has_noise, float sm1, float cf, float sg, float sg_to, float mb, float cn, float (&o)[8]) {
  const float alpha = 1.0f - sg, alpha_to = 1.0f - sg_to;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float u = cfg_velocity(p, q, e, has_neg, has_coef, sm1, cf);
    const float clean = x[e] - sg * u;
    const float eps = x[e] + alpha * u;
    float mix = mb * eps;
    if (has_noise) mix = mix + cn * z[e];
    o[e] = alpha_to * clean + sg_to * mix;
  }
}

// One chunk = 8 consecutive elements of one sample (n % 64 == 0: a chunk never straddles two samples, and a sample's first chunk
// is 16-byte aligned in every operand).  x_out may be x: a lane loads its chunk of every operand before it stores.
__global__ __launch_bounds__(256) void teacher_euler_step_kernel(const float* x, const bf16_t* __restrict__ pos,
                                                                 const bf16_t* __restrict__ neg, const float* __restrict__ sigma,
                                                                 const float* __restrict__ sigma_to, const float* __restrict__ coef,
                                                                 float scale, float* x_out, bf16_t* __restrict__ x_bf16,
                                                                 int64_t chunks_per_sample, int64_t chunks) {
  const float sm1 = scale - 1.0f;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < chunks; c += stride) {
    const int64_t b = c / chunks_per_sample;
    const float sg = sigma[b], sg_to = sigma_to[b];
    const float cf = coef != nullptr ? coef[b] : 0.f;
    float p[8], q[8], v[8], o[8];
    unpack8(*reinterpret_cast<const u32x4_t*>(pos + c * 8), p);
    if (neg != nullptr) unpack8(*reinterpret_cast<const u32x4_t*>(neg + c * 8), q);
    load8(x + c * 8, v);
    euler_update8(v, p, q, neg != nullptr, coef != nullptr, sm1, cf, sg, sg_to, o);
    store8(x_out + c * 8, o);
    *reinterpret_cast<u32x4_t*>(x_bf16 + c * 8) = pack8(o);
  }
}

// noise == nullptr: no noise term, nothing read
__global__ __launch_bounds__(256) void teacher_sde_step_kernel(const float* x, const bf16_t* __restrict__ pos,
                                                               const bf16_t* __restrict__ neg, const float* __restrict__ noise,
                                                               const float* __restrict__ sigma, const float* __restrict__ sigma_to,
                                                               const float* __restrict__ m, const float* __restrict__ c_noise,
                                                               const float* __restrict__ coef, float scale, float* x_out,
                                                               bf16_t* __restrict__ x_bf16, int64_t chunks_per_sample, int64_t chunks) {
  const float sm1 = scale - 1.0f;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < chunks; c += stride) {
    const int64_t b = c / chunks_per_sample;
    const float sg = sigma[b], sg_to = sigma_to[b], mb = m[b], cn = c_noise[b];
    const float cf = coef != nullptr ? coef[b] : 0.f;
    float p[8], q[8], v[8], z[8], o[8];
    unpack8(*reinterpret_cast<const u32x4_t*>(pos + c * 8), p);
    if (neg != nullptr) unpack8(*reinterpret_cast<const u32x4_t*>(neg + c * 8), q);
    load8(x + c * 8, v);
    if (noise != nullptr) load8(noise + c * 8, z);
    sde_update8(v, p, q, z, neg != nullptr, coef != nullptr, noise != nullptr, sm1, cf, sg, sg_to, mb, cn, o);
    store8(x_out + c * 8, o);
    *reinterpret_cast<u32x4_t*>(x_bf16 + c * 8) = pack8(o);
  }
}

// One step of the UniPC multistep sampler (FlowUniPCScheduler: the solver behind the reference's FlowAdapterScheduler on its default base
// scheduler; the arithmetic is diffusers' as recalled, DESIGN.md 6.1 "Multistep sampling") on the same chunks, with the same CFG combine.  The
// predictor and the corrector are linear in their operands, and the host (FlowUniPCScheduler.coefficients, fp64) hands over one fp32 weight
// per operand and sample, w[r * batch + b], rows
//   0 s | 1 c_last  2 c_mt  3 c_1  4 c_2  5 c_3 | 6 p_xc  7 p_mt  8 p_1  9 p_2
// Per element, in this order, every product-sum one fused multiply-add (a rounding each):
//   u      = cfg_velocity
//   m_t    = fma(-s, u, x)                                                          the clean-sample prediction, from the uncorrected x
//   x_c    = fma(c_mt, m_t, fma(c_3, h3, fma(c_2, h2, fma(c_1, h1, c_last last))))  last == nullptr (first step of a roll): x_c = x
//   x_next = fma(p_mt, m_t, fma(p_2, h2, fma(p_1, h1, p_xc x_c)))
// h1, h2, h3 = the clean-sample predictions of one, two, three steps ago; a nullptr one is neither read nor multiplied (its fma is skipped).
// On the step that lands on sigma 0 the weights are p_xc = 0, p_mt = 1, p_1 = p_2 = 0: x_next = m_t bit for bit (finite operands).
// Writes x_next (x_out, may be x) and its bf16 copy, x_c (last_out, may be last) and m_t (hist_out, may be one of h1 / h2 / h3: the host
// rotates a ring of solver_order buffers and overwrites the oldest).  A lane loads all of its 8 elements of every operand before it stores
// any, and no two lanes share an element, so these aliases are safe; the operands that may alias carry no __restrict__.
// Traffic per element at order 2 past the warm-up: 4 (x) + 2 (pos) + 2 (neg) + 4 (last) + 4 (h1) + 4 (h2) = 20 B read and 4 (x') + 2 (bf16 x') +
// 4 (x_c) + 4 (m_t) = 14 B written: 34 B, about 8.9 MB per 1024 x 1024 image and step (order 3: 38 B; the Euler step moves 14 B).
__global__ __launch_bounds__(256) void teacher_unipc_step_kernel(const float* x, const bf16_t* __restrict__ pos, const bf16_t* __restrict__ neg,
                                                                 const float* __restrict__ w, const float* last, const float* h1, const float* h2,
                                                                 const float* h3, const float* __restrict__ coef, float scale, float* x_out,
                                                                 bf16_t* __restrict__ x_bf16, float* last_out, float* hist_out, int64_t batch,
                                                                 int64_t chunks_per_sample, int64_t chunks) {
  const float sm1 = scale - 1.0f;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < chunks; c += stride) {
    const int64_t b = c / chunks_per_sample;
    float wv[10];
#pragma unroll
    for (int r = 0; r < 10; ++r) wv[r] = w[r * batch + b];
    const float cf = coef != nullptr ? coef[b] : 0.f;
    float p[8], q[8], v[8], l[8], a1[8], a2[8], a3[8], o[8], xc[8], mt[8];
    unpack8(*reinterpret_cast<const u32x4_t*>(pos + c * 8), p);
    if (neg != nullptr) unpack8(*reinterpret_cast<const u32x4_t*>(neg + c * 8), q);
    load8(x + c * 8, v);
    if (last != nullptr) load8(last + c * 8, l);
    if (h1 != nullptr) load8(h1 + c * 8, a1);
    if (h2 != nullptr) load8(h2 + c * 8, a2);
    if (h3 != nullptr) load8(h3 + c * 8, a3);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float u = cfg_velocity(p, q, e, neg != nullptr, coef != nullptr, sm1, cf);
      const float m = __builtin_fmaf(-wv[0], u, v[e]);
      float cx = v[e];
      if (last != nullptr) {
        cx = wv[1] * l[e];
        if (h1 != nullptr) cx = __builtin_fmaf(wv[3], a1[e], cx);
        if (h2 != nullptr) cx = __builtin_fmaf(wv[4], a2[e], cx);
        if (h3 != nullptr) cx = __builtin_fmaf(wv[5], a3[e], cx);
        cx = __builtin_fmaf(wv[2], m, cx);
      }
      float nx = wv[6] * cx;
      if (h1 != nullptr) nx = __builtin_fmaf(wv[8], a1[e], nx);
      if (h2 != nullptr) nx = __builtin_fmaf(wv[9], a2[e], nx);
      o[e] = __builtin_fmaf(wv[7], m, nx);
      xc[e] = cx;
      mt[e] = m;
    }
    store8(x_out + c * 8, o);
    *reinterpret_cast<u32x4_t*>(x_bf16 + c * 8) = pack8(o);
    store8(last_out + c * 8, xc);
    store8(hist_out + c * 8, mt);
  }
}

// The step of teacher image editing (image-to-image / inpainting with the many-step sampler): the Euler (SDE = false) or FlowSDE
// (SDE = true) update with the CFG combine -- euler_update8 / sde_update8, the same functions the two kernels above call -- rounded to
// fp32, then the re-imposition of the known region at the sigma the step lands on by edit_blend8 (afx_common.h), the same function
// edit_blend_kernel (afx_edit.hip) calls:
//   x'    = the step above                                              (fp32)
//   x_out = edit_blend8(x', x0, noise0, mask row, sigma_to[b])          m = mask[b, tok, e & 3], 1 = repaint, 0 = keep the source
// so that the outputs are, bit for bit, those of the step kernel followed by edit_blend_kernel on its result.  One chunk = 8 consecutive
// elements of one token (64 channels per token), one 16-byte load of the token's mask row per chunk as in edit_blend_kernel.  Traffic
// per element at 1024 x 1024: 4 (x) + 2 (pos) + 2 (neg) [+ 4 (z), SDE] + 4 (x0) + 4 (noise0) B read, 16 B of mask per token (0.25 B), 4 (x') +
// 2 (bf16 x') B written = 22.25 B (SDE 26.25 B); the two launches it replaces move 14 (18) + 18.25 B: the fused step saves the fp32
// write and re-read of x', the first bf16 copy (10 B per element) and a launch.
template <bool SDE>
__global__ __launch_bounds__(256) void teacher_edit_step_kernel(const float* x, const bf16_t* __restrict__ pos, const bf16_t* __restrict__ neg,
                                                                const float* __restrict__ noise, const float* __restrict__ sigma,
                                                                const float* __restrict__ sigma_to, const float* __restrict__ m,
                                                                const float* __restrict__ c_noise, const float* __restrict__ coef, float scale,
                                                                const float* __restrict__ x0, const float* __restrict__ noise0,
                                                                const float* __restrict__ mask, float* x_out, bf16_t* __restrict__ x_bf16,
                                                                int64_t chunks_per_sample, int64_t chunks) {
  const float sm1 = scale - 1.0f;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < chunks; c += stride) {
    const int64_t b = c / chunks_per_sample;
    const float sg = sigma[b], sg_to = sigma_to[b];
    const float cf = coef != nullptr ? coef[b] : 0.f;
    float p[8], q[8], v[8], a[8], z[8], n0[8], o[8];
    unpack8(*reinterpret_cast<const u32x4_t*>(pos + c * 8), p);
    if (neg != nullptr) unpack8(*reinterpret_cast<const u32x4_t*>(neg + c * 8), q);
    load8(x + c * 8, v);
    load8(x0 + c * 8, a);
    const f32x4_t mk = *reinterpret_cast<const f32x4_t*>(mask + (c >> 3) * 4);
    if (SDE && noise != nullptr) load8(noise + c * 8, z);
    if (noise0 != nullptr) load8(noise0 + c * 8, n0);
    if constexpr (SDE)
      sde_update8(v, p, q, z, neg != nullptr, coef != nullptr, noise != nullptr, sm1, cf, sg, sg_to, m[b], c_noise[b], o);
    else
      euler_update8(v, p, q, neg != nullptr, coef != nullptr, sm1, cf, sg, sg_to, o);
    edit_blend8(o, a, n0, mk, noise0 != nullptr, true, sg_to, o);
    store8(x_out + c * 8, o);
    *reinterpret_cast<u32x4_t*>(x_bf16 + c * 8) = pack8(o);
  }
}

// grid (parts, B): work-group w of sample b owns the chunks [w cpw, min((w + 1) cpw, chunks_per_sample)) and writes
// ws[(b parts + w) 2 + {0, 1}] = sum bias pos, sum pos pos  (bias = fl(fl(pos - neg) (scale - 1)), the step kernel's fp32 value)
__global__ __launch_bounds__(256) void cfg_ortho_partial_kernel(const bf16_t* __restrict__ pos, const bf16_t* __restrict__ neg,
                                                                float scale, double* __restrict__ ws, int64_t chunks_per_sample,
                                                                int64_t cpw) {
  const float sm1 = scale - 1.0f;
  const int64_t b = blockIdx.y;
  const int64_t begin = (int64_t)blockIdx.x * cpw;
  const int64_t end = begin + cpw < chunks_per_sample ? begin + cpw : chunks_per_sample;
  const bf16_t* ps = pos + b * chunks_per_sample * 8;
  const bf16_t* ns = neg + b * chunks_per_sample * 8;
  double acc[2] = {0.0, 0.0};          // sum bias pos, sum pos pos
  for (int64_t c = begin + threadIdx.x; c < end; c += 256) {
    float p[8], q[8];
    unpack8(*reinterpret_cast<const u32x4_t*>(ps + c * 8), p);
    unpack8(*reinterpret_cast<const u32x4_t*>(ns + c * 8), q);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float bias = (p[e] - q[e]) * sm1;
      acc[0] += (double)bias * (double)p[e];
      acc[1] += (double)p[e] * (double)p[e];
    }
  }
  block_slot_sums<2>(acc, ws + (b * gridDim.x + blockIdx.x) * 2);
}

__global__ __launch_bounds__(64) void cfg_ortho_finish_kernel(const double* __restrict__ ws, float* __restrict__ coef, int batch,
                                                              int parts, double inv_n) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= batch) return;
  const double s_bp = ordered_slot_sum<2>(ws, b, parts, 0), s_pp = ordered_slot_sum<2>(ws, b, parts, 1);
  const double den = s_pp * inv_n > 1e-6 ? s_pp * inv_n : 1e-6;
  coef[b] = (float)(s_bp * inv_n / den);
}

}  // namespace afx

using namespace afx;

// What every step entry refuses first, by the name of the entry that was called: a missing required pointer (`optional`: the operands
// that may be NULL, or NULL to say nothing), batch, n and max_blocks, and a pointer of `ptrs` (the operands `ptr_names`, read or
// written 16 bytes at a time) that is not 16-byte aligned.
static int step_refusals(const char* name, bool missing, const char* optional, int32_t batch, int64_t n, int32_t max_blocks,
                         std::initializer_list<const void*> ptrs, const char* ptr_names) {
  if (missing && optional) return fail(AFX_E_INVALID, "null argument to %s (only %s may be NULL)", name, optional);
  if (missing) return fail(AFX_E_INVALID, "null argument to %s", name);
  if (batch < 0 || n < 64 || n % 64 || max_blocks < 0)
    return fail(AFX_E_INVALID, "bad argument to %s (n = tokens x channels must be a positive multiple of 64)", name);
  if (misaligned16(ptrs)) return fail(AFX_E_INVALID, "%s: %s must be 16-byte aligned", name, ptr_names);
  return AFX_OK;
}

extern "C" {

int afx_teacher_euler_step(const float* x, const void* pos, const void* neg, const float* sigma, const float* sigma_to,
                           const float* coef, float scale, float* x_out, void* x_out_bf16, int32_t batch, int64_t n,
                           int32_t max_blocks, void* stream) {
  AFX_TRY(step_refusals("afx_teacher_euler_step", !x || !pos || !sigma || !sigma_to || !x_out || !x_out_bf16, nullptr, batch, n, max_blocks,
                        {x, pos, neg, x_out, x_out_bf16}, "x, pos, neg, x_out and x_out_bf16"));
  if (batch == 0) return AFX_OK;
  return launch_step(teacher_euler_step_kernel, batch, n, max_blocks, stream, x, (const bf16_t*)pos, (const bf16_t*)neg, sigma, sigma_to, coef,
                     scale, x_out, (bf16_t*)x_out_bf16);
}

int afx_teacher_sde_step(const float* x, const void* pos, const void* neg, const float* noise, const float* sigma,
                         const float* sigma_to, const float* m, const float* c_noise, const float* coef, float scale, float* x_out,
                         void* x_out_bf16, int32_t batch, int64_t n, int32_t max_blocks, void* stream) {
  AFX_TRY(step_refusals("afx_teacher_sde_step", !x || !pos || !sigma || !sigma_to || !m || !c_noise || !x_out || !x_out_bf16, nullptr, batch, n,
                        max_blocks, {x, pos, neg, noise, x_out, x_out_bf16}, "x, pos, neg, noise, x_out and x_out_bf16"));
  if (batch == 0) return AFX_OK;
  return launch_step(teacher_sde_step_kernel, batch, n, max_blocks, stream, x, (const bf16_t*)pos, (const bf16_t*)neg, noise, sigma, sigma_to, m,
                     c_noise, coef, scale, x_out, (bf16_t*)x_out_bf16);
}

int afx_teacher_unipc_step(const float* x, const void* pos, const void* neg, const float* w, const float* last, const float* h1,
                           const float* h2, const float* h3, const float* coef, float scale, float* x_out, void* x_out_bf16, float* last_out,
                           float* hist_out, int32_t batch, int64_t n, int32_t max_blocks, void* stream) {
  AFX_TRY(step_refusals("afx_teacher_unipc_step", !x || !pos || !w || !x_out || !x_out_bf16 || !last_out || !hist_out,
                        "neg, last, h1, h2, h3 and coef", batch, n, max_blocks, {x, pos, neg, last, h1, h2, h3, x_out, x_out_bf16, last_out, hist_out},
                        "x, pos, neg, last, h1, h2, h3, x_out, x_out_bf16, last_out and hist_out"));
  if ((last && !h1) || (h2 && !h1) || (h3 && !h2))
    return fail(AFX_E_INVALID, "afx_teacher_unipc_step: the corrector (last) needs h1, h2 needs h1 and h3 needs h2");
  if (batch == 0) return AFX_OK;
  // a lane reads its own 8 elements of every operand before it writes them, so an output may BE the input it replaces (x_out == x,
  // last_out == last, hist_out == one history slot); any other overlap lets one lane's store land in another lane's load
  const int64_t fbytes = (int64_t)batch * n * 4, hbytes = (int64_t)batch * n * 2, wbytes = (int64_t)batch * 10 * 4, cbytes = (int64_t)batch * 4;
  const void* fin[] = {x, last, h1, h2, h3};
  struct { const void* p; int64_t bytes; const void* may; const char* name; } outs[] = {
      {x_out, fbytes, x, "x_out"}, {x_out_bf16, hbytes, nullptr, "x_out_bf16"}, {last_out, fbytes, last, "last_out"}, {hist_out, fbytes, nullptr, "hist_out"}};
  for (int k = 0; k < 4; ++k) {
    bool hit = ranges_overlap(outs[k].p, outs[k].bytes, pos, hbytes) || ranges_overlap(outs[k].p, outs[k].bytes, neg, hbytes) ||
               ranges_overlap(outs[k].p, outs[k].bytes, w, wbytes) || ranges_overlap(outs[k].p, outs[k].bytes, coef, cbytes);
    for (int i = 0; i < 5; ++i) {
      const bool same = outs[k].p == fin[i] && (fin[i] == outs[k].may || (k == 3 && i >= 2));      // hist_out: h1, h2 or h3 itself
      hit = hit || (!same && ranges_overlap(outs[k].p, outs[k].bytes, fin[i], fbytes));
    }
    for (int j = 0; j < k; ++j) hit = hit || ranges_overlap(outs[k].p, outs[k].bytes, outs[j].p, outs[j].bytes);
    if (hit)
      return fail(AFX_E_INVALID, "afx_teacher_unipc_step: %s overlaps another operand (only x_out == x, last_out == last and hist_out == h1, h2 or h3 are allowed)",
                  outs[k].name);
  }
  return launch_step(teacher_unipc_step_kernel, batch, n, max_blocks, stream, x, (const bf16_t*)pos, (const bf16_t*)neg, w, last, h1, h2, h3, coef,
                     scale, x_out, (bf16_t*)x_out_bf16, last_out, hist_out, (int64_t)batch);
}

}  // extern "C"

// Both edit-step entries: the refusals (before any launch), then mask == NULL -> the plain step entry itself, else the fused kernel.
// sde = false: the Euler step (noise, m, c_noise are NULL and unused).
static int edit_step(const char* name, bool sde, const float* x, const void* pos, const void* neg, const float* noise, const float* sigma,
                     const float* sigma_to, const float* m, const float* c_noise, const float* coef, float scale, const float* x0,
                     const float* noise0, const float* mask, float* x_out, void* x_out_bf16, int32_t batch, int32_t n_tok, int32_t ch,
                     int32_t max_blocks, void* stream) {
  if (!x || !pos || !sigma || !sigma_to || (sde && (!m || !c_noise)) || !x0 || !x_out || !x_out_bf16)
    return fail(AFX_E_INVALID, "null argument to %s (only neg, noise, coef, noise0 and mask may be NULL)", name);
  if (ch != 64) return fail(AFX_E_INVALID, "%s: ch must be 64 (16 latent channels x the 2 x 2 patch), got %d", name, (int)ch);
  if (batch < 1 || n_tok < 1 || max_blocks < 0)
    return fail(AFX_E_INVALID, "bad argument to %s (batch and n_tok must be >= 1, max_blocks >= 0)", name);
  if (misaligned16({x, pos, neg, noise, x0, noise0, mask, x_out, x_out_bf16}))
    return fail(AFX_E_INVALID, "%s: x, pos, neg, noise, x0, noise0, mask, x_out and x_out_bf16 must be 16-byte aligned", name);
  const int64_t elems = (int64_t)batch * n_tok * 64;
  const int64_t fbytes = elems * 4, hbytes = elems * 2, mbytes = (int64_t)batch * n_tok * 16, sbytes = (int64_t)batch * 4;
  // every lane reads its own 8 elements before it writes them, so x_out == x is safe; any other overlap lets one lane's store
  // land in another lane's load
  const void* fin[] = {x, noise, x0, noise0};
  const void* sin[] = {sigma, sigma_to, m, c_noise, coef};
  bool out_hit = x != x_out && ranges_overlap(x_out, fbytes, x, fbytes), bf_hit = false;
  for (int i = 0; i < 4; ++i) {
    if (i > 0) out_hit = out_hit || ranges_overlap(x_out, fbytes, fin[i], fbytes);
    bf_hit = bf_hit || ranges_overlap(x_out_bf16, hbytes, fin[i], fbytes);
  }
  for (const void* s : sin) {
    out_hit = out_hit || ranges_overlap(x_out, fbytes, s, sbytes);
    bf_hit = bf_hit || ranges_overlap(x_out_bf16, hbytes, s, sbytes);
  }
  out_hit = out_hit || ranges_overlap(x_out, fbytes, pos, hbytes) || ranges_overlap(x_out, fbytes, neg, hbytes) ||
            ranges_overlap(x_out, fbytes, mask, mbytes) || ranges_overlap(x_out, fbytes, x_out_bf16, hbytes);
  bf_hit = bf_hit || ranges_overlap(x_out_bf16, hbytes, pos, hbytes) || ranges_overlap(x_out_bf16, hbytes, neg, hbytes) ||
           ranges_overlap(x_out_bf16, hbytes, mask, mbytes);
  if (out_hit) return fail(AFX_E_INVALID, "%s: x_out overlaps another operand (only x_out == x is allowed)", name);
  if (bf_hit) return fail(AFX_E_INVALID, "%s: x_out_bf16 overlaps an input", name);
  const int64_t n = (int64_t)n_tok * 64;
  if (mask == nullptr)            // nothing to re-impose: the plain step, the very kernel the plain sampler runs
    return sde ? afx_teacher_sde_step(x, pos, neg, noise, sigma, sigma_to, m, c_noise, coef, scale, x_out, x_out_bf16, batch, n, max_blocks, stream)
               : afx_teacher_euler_step(x, pos, neg, sigma, sigma_to, coef, scale, x_out, x_out_bf16, batch, n, max_blocks, stream);
  return launch_step(sde ? teacher_edit_step_kernel<true> : teacher_edit_step_kernel<false>, batch, n, max_blocks, stream, x, (const bf16_t*)pos,
                     (const bf16_t*)neg, noise, sigma, sigma_to, m, c_noise, coef, scale, x0, noise0, mask, x_out, (bf16_t*)x_out_bf16);
}

extern "C" {

int afx_teacher_edit_step(const float* x, const void* pos, const void* neg, const float* sigma, const float* sigma_to, const float* coef,
                          float scale, const float* x0, const float* noise0, const float* mask, float* x_out, void* x_out_bf16,
                          int32_t batch, int32_t n_tok, int32_t ch, int32_t max_blocks, void* stream) {
  return edit_step("afx_teacher_edit_step", false, x, pos, neg, nullptr, sigma, sigma_to, nullptr, nullptr, coef, scale, x0, noise0, mask, x_out,
                   x_out_bf16, batch, n_tok, ch, max_blocks, stream);
}

int afx_teacher_sde_edit_step(const float* x, const void* pos, const void* neg, const float* noise, const float* sigma, const float* sigma_to,
                              const float* m, const float* c_noise, const float* coef, float scale, const float* x0, const float* noise0,
                              const float* mask, float* x_out, void* x_out_bf16, int32_t batch, int32_t n_tok, int32_t ch, int32_t max_blocks,
                              void* stream) {
  return edit_step("afx_teacher_sde_edit_step", true, x, pos, neg, noise, sigma, sigma_to, m, c_noise, coef, scale, x0, noise0, mask, x_out,
                   x_out_bf16, batch, n_tok, ch, max_blocks, stream);
}

int64_t afx_cfg_ortho_ws_bytes(int32_t batch, int64_t n) {
  return ws_bytes_or_fail("afx_cfg_ortho_ws_bytes", batch < 0 || n < 64 || n % 64, "", batch, reduce_parts(n), 2);
}

int afx_cfg_ortho_coef(const void* pos, const void* neg, float scale, float* coef, void* ws, int64_t ws_bytes, int32_t batch,
                       int64_t n, void* stream) {
  if (!pos || !neg || !coef || !ws) return fail(AFX_E_INVALID, "null argument to afx_cfg_ortho_coef");
  if (batch < 0 || batch > 65535 || n < 64 || n % 64)
    return fail(AFX_E_INVALID, "bad argument to afx_cfg_ortho_coef (n = tokens x channels must be a positive multiple of 64)");
  if (((uintptr_t)pos & 15) || ((uintptr_t)neg & 15) || ((uintptr_t)ws & 7))
    return fail(AFX_E_INVALID, "afx_cfg_ortho_coef: pos and neg must be 16-byte aligned, ws 8-byte aligned");
  const int parts = reduce_parts(n);
  if (ws_bytes < (int64_t)batch * parts * 2 * (int64_t)sizeof(double))
    return fail(AFX_E_INVALID, "afx_cfg_ortho_coef: workspace smaller than afx_cfg_ortho_ws_bytes()");
  if (batch == 0) return AFX_OK;
  const int64_t cps = n / 8, cpw = (cps + parts - 1) / parts;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cfg_ortho_partial_kernel, dim3(parts, batch), dim3(256), 0, st, (const bf16_t*)pos, (const bf16_t*)neg, scale,
                     (double*)ws, cps, cpw);
  hipLaunchKernelGGL(cfg_ortho_finish_kernel, dim3((batch + 63) / 64), dim3(64), 0, st, (const double*)ws, coef, batch, parts,
                     1.0 / (double)n);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

}  // extern "C"
