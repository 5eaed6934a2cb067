// Teacher sampling (GaussianFlow.forward_test, lakonlab/models/diffusions/gaussian_flow.py:149-222): what runs between two
// teacher forwards of the Euler ODE loop, on the packed token layout the engine reads and writes.
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
//     mean(bias pos) / max(mean(pos pos), 1e-6) over all n elements of a sample.  A fixed number of work-groups per sample
//     (a function of n alone), every product exact in fp64, one workspace slot per work-group, the slots added in index order
//     by the second launch: bit-reproducible.
//   * sample_score_partial_kernel / sample_score_finish_kernel: per-sample agreement sums of two batches (training-time evaluation:
//     student against teacher samples), sum (a-b)^2, sum a^2, sum b^2, sum a b over the n elements of a sample, on the coefficient's
//     reduction scheme: the same fixed partition, elements widened to fp64 (after the optional image-range transform in fp32), one slot
//     of 4 doubles per work-group, the slots added in index order by the second launch.  16 B per lane and operand: 8 bf16 or 4 fp32.
//   * image_ssim_partial_kernel / image_ssim_finish_kernel: per-sample sum of the structural similarity of two image batches over
//     every valid 11 x 11 Gaussian window (training-time evaluation, decoded images), fp64 throughout: one work-group and one slot per
//     tile of windows, the slots added in a fixed order by the second launch.  Scheme and LDS use at the kernel.
//   * sample_score_masked_* / image_ssim_masked_*: the two scoring passes weighted by an edit's mask, a repainted (weight m) and a kept
//     (weight 1 - m) set of sums each, on the same partitions and the same ordered second launches.  Weight maps and LDS use at the kernels.
#include <algorithm>
#include <climits>
#include <cmath>

#include "afx_api_util.h"
#include "afx_common.h"

namespace afx {

// The guided velocity of one element, shared by both step kernels so that the CFG arithmetic cannot drift between them:
//   u = pos                                  no guidance on this step
//   u = pos + (pos - neg) (scale - 1)        true CFG (guidance_jit, orthogonal off)
//   u = u - coef pos                         orthogonal guidance: the projection on pos removed (coef from afx_cfg_ortho_coef)
AFX_DEV float cfg_velocity(const float (&p)[8], const float (&q)[8], int e, bool has_neg, bool has_coef, float sm1, float cf) {
  float u = p[e];
  if (has_neg) u = p[e] + (p[e] - q[e]) * sm1;
  if (has_coef) u = u - cf * p[e];
  return u;
}

// One chunk = 8 consecutive elements of one sample (n % 64 == 0: a chunk never straddles two samples, and a sample's first chunk
// is 16-byte aligned in every operand).
__global__ __launch_bounds__(256) void teacher_euler_step_kernel(const float* x, const bf16_t* __restrict__ pos,
                                                                 const bf16_t* __restrict__ neg, const float* __restrict__ sigma,
                                                                 const float* __restrict__ sigma_to, const float* __restrict__ coef,
                                                                 float scale, float* x_out, bf16_t* __restrict__ x_bf16,
                                                                 int64_t chunks_per_sample, int64_t chunks) {
  const float sm1 = scale - 1.0f;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < chunks; c += stride) {
    const int64_t b = c / chunks_per_sample;
    const float dt = sigma_to[b] - sigma[b];
    const float cf = coef != nullptr ? coef[b] : 0.f;
    float p[8], q[8], o[8];
    unpack8(*reinterpret_cast<const u32x4_t*>(pos + c * 8), p);
    if (neg != nullptr) unpack8(*reinterpret_cast<const u32x4_t*>(neg + c * 8), q);
    const f32x4_t x0 = *reinterpret_cast<const f32x4_t*>(x + c * 8);        // (x_out may be x: both loads precede both stores)
    const f32x4_t x1 = *reinterpret_cast<const f32x4_t*>(x + c * 8 + 4);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float u = cfg_velocity(p, q, e, neg != nullptr, coef != nullptr, sm1, cf);
      o[e] = (e < 4 ? x0[e & 3] : x1[e & 3]) + u * dt;
    }
    const f32x4_t o0 = {o[0], o[1], o[2], o[3]}, o1 = {o[4], o[5], o[6], o[7]};
    *reinterpret_cast<f32x4_t*>(x_out + c * 8) = o0;
    *reinterpret_cast<f32x4_t*>(x_out + c * 8 + 4) = o1;
    *reinterpret_cast<u32x4_t*>(x_bf16 + c * 8) = pack8(o);
  }
}

// FlowSDEScheduler.step, prediction_type 'u', on the same chunks:
//   x0 = x - sigma u,   eps = x + (1 - sigma) u,   x' = (1 - sigma_to) x0 + sigma_to (m eps + c_noise z)
// noise == nullptr: the term c_noise z is skipped together with its read (the host passes it when sigma_to c_noise = 0 for every sample).
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
    const float alpha = 1.0f - sg, alpha_to = 1.0f - sg_to;
    const float cf = coef != nullptr ? coef[b] : 0.f;
    float p[8], q[8], o[8];
    unpack8(*reinterpret_cast<const u32x4_t*>(pos + c * 8), p);
    if (neg != nullptr) unpack8(*reinterpret_cast<const u32x4_t*>(neg + c * 8), q);
    const f32x4_t x0 = *reinterpret_cast<const f32x4_t*>(x + c * 8);        // (x_out may be x: every load precedes every store)
    const f32x4_t x1 = *reinterpret_cast<const f32x4_t*>(x + c * 8 + 4);
    f32x4_t z0 = {0.f, 0.f, 0.f, 0.f}, z1 = z0;
    if (noise != nullptr) {
      z0 = *reinterpret_cast<const f32x4_t*>(noise + c * 8);
      z1 = *reinterpret_cast<const f32x4_t*>(noise + c * 8 + 4);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float u = cfg_velocity(p, q, e, neg != nullptr, coef != nullptr, sm1, cf);
      const float xe = e < 4 ? x0[e & 3] : x1[e & 3];
      const float clean = xe - sg * u;
      const float eps = xe + alpha * u;
      float mix = mb * eps;
      if (noise != nullptr) mix = mix + cn * (e < 4 ? z0[e & 3] : z1[e & 3]);
      o[e] = alpha_to * clean + sg_to * mix;
    }
    const f32x4_t o0 = {o[0], o[1], o[2], o[3]}, o1 = {o[4], o[5], o[6], o[7]};
    *reinterpret_cast<f32x4_t*>(x_out + c * 8) = o0;
    *reinterpret_cast<f32x4_t*>(x_out + c * 8 + 4) = o1;
    *reinterpret_cast<u32x4_t*>(x_bf16 + c * 8) = pack8(o);
  }
}

AFX_DEV void load8(const float* p, float (&v)[8]) {
  const f32x4_t a = *reinterpret_cast<const f32x4_t*>(p), b = *reinterpret_cast<const f32x4_t*>(p + 4);
  v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
}

AFX_DEV void store8(float* p, const float (&v)[8]) {
  const f32x4_t a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
  *reinterpret_cast<f32x4_t*>(p) = a;
  *reinterpret_cast<f32x4_t*>(p + 4) = b;
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
// (SDE = true) update with the CFG combine, written as the two kernels above write it and rounded to fp32, then the re-imposition of
// the known region at the sigma the step lands on, in edit_blend_kernel's own forms (afx_edit.hip):
//   x'    = the step above                                              (fp32)
//   om    = 1 - sigma_to[b]
//   known = noise0 ? fma(sigma_to[b], noise0, om x0) : om x0
//   x_out = fma(m, x', (1 - m) known)                                   m = mask[b, tok, e & 3], 1 = repaint, 0 = keep the source
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
    float p[8], q[8], o[8];
    unpack8(*reinterpret_cast<const u32x4_t*>(pos + c * 8), p);
    if (neg != nullptr) unpack8(*reinterpret_cast<const u32x4_t*>(neg + c * 8), q);
    const f32x4_t v0 = *reinterpret_cast<const f32x4_t*>(x + c * 8);        // (x_out may be x: every load precedes every store)
    const f32x4_t v1 = *reinterpret_cast<const f32x4_t*>(x + c * 8 + 4);
    const f32x4_t a0 = *reinterpret_cast<const f32x4_t*>(x0 + c * 8);
    const f32x4_t a1 = *reinterpret_cast<const f32x4_t*>(x0 + c * 8 + 4);
    const f32x4_t mk = *reinterpret_cast<const f32x4_t*>(mask + (c >> 3) * 4);
    f32x4_t z0 = {0.f, 0.f, 0.f, 0.f}, z1 = z0, n0 = z0, n1 = z0;
    if (SDE && noise != nullptr) {
      z0 = *reinterpret_cast<const f32x4_t*>(noise + c * 8);
      z1 = *reinterpret_cast<const f32x4_t*>(noise + c * 8 + 4);
    }
    if (noise0 != nullptr) {
      n0 = *reinterpret_cast<const f32x4_t*>(noise0 + c * 8);
      n1 = *reinterpret_cast<const f32x4_t*>(noise0 + c * 8 + 4);
    }
    if constexpr (SDE) {            // teacher_sde_step_kernel's update
      const float mb = m[b], cn = c_noise[b];
      const float alpha = 1.0f - sg, alpha_to = 1.0f - sg_to;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float u = cfg_velocity(p, q, e, neg != nullptr, coef != nullptr, sm1, cf);
        const float xe = e < 4 ? v0[e & 3] : v1[e & 3];
        const float clean = xe - sg * u;
        const float eps = xe + alpha * u;
        float mix = mb * eps;
        if (noise != nullptr) mix = mix + cn * (e < 4 ? z0[e & 3] : z1[e & 3]);
        o[e] = alpha_to * clean + sg_to * mix;
      }
    } else {                        // teacher_euler_step_kernel's update
      const float dt = sg_to - sg;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float u = cfg_velocity(p, q, e, neg != nullptr, coef != nullptr, sm1, cf);
        o[e] = (e < 4 ? v0[e & 3] : v1[e & 3]) + u * dt;
      }
    }
    const float om = 1.0f - sg_to;
#pragma unroll
    for (int e = 0; e < 8; ++e) {   // edit_blend_kernel's blend, on the step's fp32 result
      float known = om * (e < 4 ? a0[e & 3] : a1[e & 3]);
      if (noise0 != nullptr) known = __builtin_fmaf(sg_to, e < 4 ? n0[e & 3] : n1[e & 3], known);
      const float mm = mk[e & 3];
      o[e] = __builtin_fmaf(mm, o[e], (1.0f - mm) * known);
    }
    const f32x4_t o0 = {o[0], o[1], o[2], o[3]}, o1 = {o[4], o[5], o[6], o[7]};
    *reinterpret_cast<f32x4_t*>(x_out + c * 8) = o0;
    *reinterpret_cast<f32x4_t*>(x_out + c * 8 + 4) = o1;
    *reinterpret_cast<u32x4_t*>(x_bf16 + c * 8) = pack8(o);
  }
}

AFX_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// grid (parts, B): work-group w of sample b owns the chunks [w cpw, min((w + 1) cpw, chunks_per_sample)) and writes
// ws[(b parts + w) 2 + {0, 1}] = sum bias pos, sum pos pos  (bias = fl(fl(pos - neg) (scale - 1)), the step kernel's fp32 value)
__global__ __launch_bounds__(256) void cfg_ortho_partial_kernel(const bf16_t* __restrict__ pos, const bf16_t* __restrict__ neg,
                                                                float scale, double* __restrict__ ws, int64_t chunks_per_sample,
                                                                int64_t cpw) {
  __shared__ double red[4][2];
  const float sm1 = scale - 1.0f;
  const int64_t b = blockIdx.y;
  const int64_t begin = (int64_t)blockIdx.x * cpw;
  const int64_t end = begin + cpw < chunks_per_sample ? begin + cpw : chunks_per_sample;
  const bf16_t* ps = pos + b * chunks_per_sample * 8;
  const bf16_t* ns = neg + b * chunks_per_sample * 8;
  double s_bp = 0.0, s_pp = 0.0;
  for (int64_t c = begin + threadIdx.x; c < end; c += 256) {
    float p[8], q[8];
    unpack8(*reinterpret_cast<const u32x4_t*>(ps + c * 8), p);
    unpack8(*reinterpret_cast<const u32x4_t*>(ns + c * 8), q);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float bias = (p[e] - q[e]) * sm1;
      s_bp += (double)bias * (double)p[e];
      s_pp += (double)p[e] * (double)p[e];
    }
  }
  s_bp = wave_sum_f64(s_bp);
  s_pp = wave_sum_f64(s_pp);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[wave][0] = s_bp;
    red[wave][1] = s_pp;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* slot = ws + (b * gridDim.x + blockIdx.x) * 2;
    slot[0] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
    slot[1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
  }
}

__global__ __launch_bounds__(64) void cfg_ortho_finish_kernel(const double* __restrict__ ws, float* __restrict__ coef, int batch,
                                                              int parts, double inv_n) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= batch) return;
  double s_bp = 0.0, s_pp = 0.0;
  for (int w = 0; w < parts; ++w) {            // index order: the sum does not depend on which work-group finished first
    s_bp += ws[((int64_t)b * parts + w) * 2];
    s_pp += ws[((int64_t)b * parts + w) * 2 + 1];
  }
  const double den = s_pp * inv_n > 1e-6 ? s_pp * inv_n : 1e-6;
  coef[b] = (float)(s_bp * inv_n / den);
}

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
  __shared__ double red[4][4];
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
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double v = wave_sum_f64(acc[k]);
    if ((threadIdx.x & 63) == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) {      // an empty work-group (upw rounded up) writes zeros: every slot the finish reads is written
    const int k = threadIdx.x;
    ws[(s * gridDim.x + blockIdx.x) * 4 + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

// one lane per (sample, sum): out[s][k] = the slots of sample s added in index order
__global__ __launch_bounds__(64) void sample_score_finish_kernel(const double* __restrict__ ws, double* __restrict__ out, int batch,
                                                                 int parts) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= batch * 4) return;
  const int s = i >> 2, k = i & 3;
  double v = 0.0;
  for (int w = 0; w < parts; ++w) v += ws[((int64_t)s * parts + w) * 4 + k];
  out[i] = v;
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
  __shared__ double red[4][10];
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
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    const double v = wave_sum_f64(acc[k]);
    if ((threadIdx.x & 63) == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 10) {      // an empty work-group (upw rounded up) writes zeros: every slot the finish reads is written
    const int k = threadIdx.x;
    ws[(s * gridDim.x + blockIdx.x) * 10 + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

// one lane per (sample, region, sum): out[s][g][k] = the slots of sample s added in index order
__global__ __launch_bounds__(64) void sample_score_masked_finish_kernel(const double* __restrict__ ws, double* __restrict__ out, int batch,
                                                                        int parts) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= batch * 10) return;
  const int s = i / 10, k = i % 10;
  double v = 0.0;
  for (int w = 0; w < parts; ++w) v += ws[((int64_t)s * parts + w) * 10 + k];
  out[i] = v;
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

// grid (C tiles, B), tiles = tiles_x tiles_y: work-group (ch tiles + tile) of sample s writes ws[s gridDim.x + blockIdx.x] = the sum
// of ssim over the valid windows of its tile.
template <bool BF16>
__global__ __launch_bounds__(256) void image_ssim_partial_kernel(const void* __restrict__ a, const void* __restrict__ b, int transform,
                                                                 ssim_taps_t taps, double c1, double c2, double* __restrict__ ws, int H,
                                                                 int W, int tiles_x, int tiles) {
  __shared__ float sa[SSIM_IH][SSIM_IW + 1], sb[SSIM_IH][SSIM_IW + 1];
  __shared__ double hq[5][SSIM_IH][SSIM_TW];
  __shared__ double red[4];
  const int tile = blockIdx.x % tiles, ch = blockIdx.x / tiles, C = gridDim.x / tiles;
  const int x0 = (tile % tiles_x) * SSIM_TW, y0 = (tile / tiles_x) * SSIM_TH;
  const int64_t base = ((int64_t)blockIdx.y * C + ch) * H * W;
  for (int i = threadIdx.x; i < SSIM_IH * SSIM_IW; i += 256) {
    const int r = i / SSIM_IW, c = i % SSIM_IW;
    const int y = y0 + r, x = x0 + c;
    float p = 0.f, q = 0.f;
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
    }
    sa[r][c] = p;
    sb[r][c] = q;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SSIM_IH * SSIM_TW; i += 256) {          // horizontal pass: x x, x y, y y are exact in fp64
    const int r = i / SSIM_TW, c = i % SSIM_TW;
    double h[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < SSIM_TAPS; ++j) {
      const double x = (double)sa[r][c + j], y = (double)sb[r][c + j], g = taps.g[j];
      h[0] = fma(g, x, h[0]);
      h[1] = fma(g, y, h[1]);
      h[2] = fma(g, x * x, h[2]);
      h[3] = fma(g, x * y, h[3]);
      h[4] = fma(g, y * y, h[4]);
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) hq[k][r][c] = h[k];
  }
  __syncthreads();
  double acc = 0.0;
  for (int i = threadIdx.x; i < SSIM_TH * SSIM_TW; i += 256) {          // vertical pass, ratio; a lane adds its windows in index order
    const int r = i / SSIM_TW, c = i % SSIM_TW;
    if (y0 + r >= H - (SSIM_TAPS - 1) || x0 + c >= W - (SSIM_TAPS - 1)) continue;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < SSIM_TAPS; ++j) {
#pragma unroll
      for (int k = 0; k < 5; ++k) v[k] = fma(taps.g[j], hq[k][r + j][c], v[k]);
    }
    acc += ssim_ratio(v[0], v[1], v[2], v[3], v[4], c1, c2);
  }
  acc = wave_sum_f64(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) ws[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one wave per sample: lane l adds the slots l, l + 64, ... of its sample in index order, then the 64 lanes are added by the shuffle
// tree -- an order that depends on `parts` alone
__global__ __launch_bounds__(64) void image_ssim_finish_kernel(const double* __restrict__ ws, double* __restrict__ out, int parts) {
  const int64_t s = blockIdx.x;
  double v = 0.0;
  for (int w = threadIdx.x; w < parts; w += 64) v += ws[s * parts + w];
  v = wave_sum_f64(v);
  if (threadIdx.x == 0) out[s] = v;
}

// ---- the same SSIM, every window weighted by the mask it covers (training-time evaluation of edits) ---------------------------------------
// image_ssim_partial_kernel with the mask [Bm, 1, H, W] (fp32, shared by the channels) as a sixth quantity: staged beside the two images,
// taken through the same horizontal and vertical 11-tap passes.  A window's weight w is the Gaussian-weighted mean of the mask over the
// window's own 11 x 11 support, clamped to [0, 1] in fp64 (the taps sum to 1 within a few ulp); the ratio is ssim_ratio() on the same five
// moments formed by the same fma chains, so a == b still gives exactly 1.0 per window and then sum w ssim == sum w bit for bit.
// Work-group (ch tiles + tile) of sample s writes ws[(s gridDim.x + blockIdx.x) 4 + {0..3}] = sum w ssim, sum w, sum (1 - w) ssim, sum (1 - w)
// over the valid windows of its tile.
// LDS: 3 x 26 x 43 x 4 B staged inputs + 6 x 26 x 32 x 8 B horizontal sums + 128 B = 53480 B, 53504 B as laid out (52.3 KB); the sixth
// plane costs 4472 + 6656 = 11128 B over image_ssim_partial_kernel's 42272 B (+ 96 B for four sums per wave).  Three work-groups still fit
// the CU's 160 KB (3 x 53504 = 160512 <= 163840), the occupancy the unmasked kernel has (3 by LDS there too), so the mask needs no pass
// of its own.  138 VGPRs (3 waves per SIMD: the same three work-groups), no scratch; the unmasked kernel has 114.
template <bool BF16>
__global__ __launch_bounds__(256) void image_ssim_masked_partial_kernel(const void* __restrict__ a, const void* __restrict__ b,
                                                                        const float* __restrict__ mask, int transform, ssim_taps_t taps, double c1,
                                                                        double c2, double* __restrict__ ws, int H, int W, int tiles_x, int tiles,
                                                                        int64_t mask_stride) {
  __shared__ float sa[SSIM_IH][SSIM_IW + 1], sb[SSIM_IH][SSIM_IW + 1], sm[SSIM_IH][SSIM_IW + 1];
  __shared__ double hq[6][SSIM_IH][SSIM_TW];
  __shared__ double red[4][4];
  const int tile = blockIdx.x % tiles, ch = blockIdx.x / tiles, C = gridDim.x / tiles;
  const int x0 = (tile % tiles_x) * SSIM_TW, y0 = (tile / tiles_x) * SSIM_TH;
  const int64_t base = ((int64_t)blockIdx.y * C + ch) * H * W;
  const float* __restrict__ mplane = mask + (int64_t)blockIdx.y * mask_stride;
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
      m = mplane[(int64_t)y * W + x];
    }
    sa[r][c] = p;
    sb[r][c] = q;
    sm[r][c] = m;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SSIM_IH * SSIM_TW; i += 256) {          // horizontal pass: the five of image_ssim_partial_kernel, and the mask
    const int r = i / SSIM_TW, c = i % SSIM_TW;
    double h[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < SSIM_TAPS; ++j) {
      const double x = (double)sa[r][c + j], y = (double)sb[r][c + j], g = taps.g[j];
      h[0] = fma(g, x, h[0]);
      h[1] = fma(g, y, h[1]);
      h[2] = fma(g, x * x, h[2]);
      h[3] = fma(g, x * y, h[3]);
      h[4] = fma(g, y * y, h[4]);
      h[5] = fma(g, (double)sm[r][c + j], h[5]);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) hq[k][r][c] = h[k];
  }
  __syncthreads();
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < SSIM_TH * SSIM_TW; i += 256) {          // vertical pass, ratio, weight; a lane adds its windows in index order
    const int r = i / SSIM_TW, c = i % SSIM_TW;
    if (y0 + r >= H - (SSIM_TAPS - 1) || x0 + c >= W - (SSIM_TAPS - 1)) continue;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < SSIM_TAPS; ++j) {
#pragma unroll
      for (int k = 0; k < 6; ++k) v[k] = fma(taps.g[j], hq[k][r + j][c], v[k]);
    }
    const double ratio = ssim_ratio(v[0], v[1], v[2], v[3], v[4], c1, c2);
    const double w = fmin(fmax(v[5], 0.0), 1.0), k = 1.0 - w;
    acc[0] = fma(w, ratio, acc[0]);
    acc[1] += w;
    acc[2] = fma(k, ratio, acc[2]);
    acc[3] += k;
  }
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double v = wave_sum_f64(acc[k]);
    if ((threadIdx.x & 63) == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    ws[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

// one wave per (sample, sum): image_ssim_finish_kernel's order -- lane l adds the slots l, l + 64, ... of its sample in index order, then the
// 64 lanes are added by the shuffle tree
__global__ __launch_bounds__(64) void image_ssim_masked_finish_kernel(const double* __restrict__ ws, double* __restrict__ out, int parts) {
  const int64_t s = blockIdx.x;
  const int k = blockIdx.y;
  double v = 0.0;
  for (int w = threadIdx.x; w < parts; w += 64) v += ws[(s * parts + w) * 4 + k];
  v = wave_sum_f64(v);
  if (threadIdx.x == 0) out[s * 4 + k] = v;
}

}  // namespace afx

using namespace afx;

// work-groups per sample of the coefficient reduction: one per 8192 elements, at most 64 -- a function of n alone
static inline int ortho_parts(int64_t n) { return (int)std::min<int64_t>(64, std::max<int64_t>(1, (n + 8191) / 8192)); }

extern "C" {

int afx_teacher_euler_step(const float* x, const void* pos, const void* neg, const float* sigma, const float* sigma_to,
                           const float* coef, float scale, float* x_out, void* x_out_bf16, int32_t batch, int64_t n,
                           int32_t max_blocks, void* stream) {
  if (!x || !pos || !sigma || !sigma_to || !x_out || !x_out_bf16) return fail(AFX_E_INVALID, "null argument to afx_teacher_euler_step");
  if (batch < 0 || n < 64 || n % 64 || max_blocks < 0)
    return fail(AFX_E_INVALID, "bad argument to afx_teacher_euler_step (n = tokens x channels must be a positive multiple of 64)");
  if (((uintptr_t)x & 15) || ((uintptr_t)pos & 15) || ((uintptr_t)neg & 15) || ((uintptr_t)x_out & 15) || ((uintptr_t)x_out_bf16 & 15))
    return fail(AFX_E_INVALID, "afx_teacher_euler_step: x, pos, neg, x_out and x_out_bf16 must be 16-byte aligned");
  if (batch == 0) return AFX_OK;
  const int64_t cps = n / 8, chunks = cps * batch;
  // 8 work-groups per CU (256 CUs) hide the load latency of a streaming pass; more only add launch work
  const int64_t cap = max_blocks > 0 ? max_blocks : 2048;
  const unsigned grid = (unsigned)std::min<int64_t>((chunks + 255) / 256, cap);
  hipLaunchKernelGGL(teacher_euler_step_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (const bf16_t*)pos,
                     (const bf16_t*)neg, sigma, sigma_to, coef, scale, x_out, (bf16_t*)x_out_bf16, cps, chunks);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

int afx_teacher_sde_step(const float* x, const void* pos, const void* neg, const float* noise, const float* sigma,
                         const float* sigma_to, const float* m, const float* c_noise, const float* coef, float scale, float* x_out,
                         void* x_out_bf16, int32_t batch, int64_t n, int32_t max_blocks, void* stream) {
  if (!x || !pos || !sigma || !sigma_to || !m || !c_noise || !x_out || !x_out_bf16)
    return fail(AFX_E_INVALID, "null argument to afx_teacher_sde_step");
  if (batch < 0 || n < 64 || n % 64 || max_blocks < 0)
    return fail(AFX_E_INVALID, "bad argument to afx_teacher_sde_step (n = tokens x channels must be a positive multiple of 64)");
  if (((uintptr_t)x & 15) || ((uintptr_t)pos & 15) || ((uintptr_t)neg & 15) || ((uintptr_t)noise & 15) || ((uintptr_t)x_out & 15) ||
      ((uintptr_t)x_out_bf16 & 15))
    return fail(AFX_E_INVALID, "afx_teacher_sde_step: x, pos, neg, noise, x_out and x_out_bf16 must be 16-byte aligned");
  if (batch == 0) return AFX_OK;
  const int64_t cps = n / 8, chunks = cps * batch;
  const int64_t cap = max_blocks > 0 ? max_blocks : 2048;          // as afx_teacher_euler_step: 8 work-groups per CU
  const unsigned grid = (unsigned)std::min<int64_t>((chunks + 255) / 256, cap);
  hipLaunchKernelGGL(teacher_sde_step_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (const bf16_t*)pos, (const bf16_t*)neg,
                     noise, sigma, sigma_to, m, c_noise, coef, scale, x_out, (bf16_t*)x_out_bf16, cps, chunks);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

int afx_teacher_unipc_step(const float* x, const void* pos, const void* neg, const float* w, const float* last, const float* h1,
                           const float* h2, const float* h3, const float* coef, float scale, float* x_out, void* x_out_bf16, float* last_out,
                           float* hist_out, int32_t batch, int64_t n, int32_t max_blocks, void* stream) {
  if (!x || !pos || !w || !x_out || !x_out_bf16 || !last_out || !hist_out)
    return fail(AFX_E_INVALID, "null argument to afx_teacher_unipc_step (only neg, last, h1, h2, h3 and coef may be NULL)");
  if ((last && !h1) || (h2 && !h1) || (h3 && !h2))
    return fail(AFX_E_INVALID, "afx_teacher_unipc_step: the corrector (last) needs h1, h2 needs h1 and h3 needs h2");
  if (batch < 0 || n < 64 || n % 64 || max_blocks < 0)
    return fail(AFX_E_INVALID, "bad argument to afx_teacher_unipc_step (n = tokens x channels must be a positive multiple of 64)");
  if (((uintptr_t)x & 15) || ((uintptr_t)pos & 15) || ((uintptr_t)neg & 15) || ((uintptr_t)last & 15) || ((uintptr_t)h1 & 15) ||
      ((uintptr_t)h2 & 15) || ((uintptr_t)h3 & 15) || ((uintptr_t)x_out & 15) || ((uintptr_t)x_out_bf16 & 15) || ((uintptr_t)last_out & 15) ||
      ((uintptr_t)hist_out & 15))
    return fail(AFX_E_INVALID, "afx_teacher_unipc_step: x, pos, neg, last, h1, h2, h3, x_out, x_out_bf16, last_out and hist_out must be 16-byte aligned");
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
  const int64_t cps = n / 8, chunks = cps * batch;
  const int64_t cap = max_blocks > 0 ? max_blocks : 2048;          // as afx_teacher_euler_step: 8 work-groups per CU
  const unsigned grid = (unsigned)std::min<int64_t>((chunks + 255) / 256, cap);
  hipLaunchKernelGGL(teacher_unipc_step_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (const bf16_t*)pos, (const bf16_t*)neg, w, last,
                     h1, h2, h3, coef, scale, x_out, (bf16_t*)x_out_bf16, last_out, hist_out, (int64_t)batch, cps, chunks);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
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
  if (((uintptr_t)x & 15) || ((uintptr_t)pos & 15) || ((uintptr_t)neg & 15) || ((uintptr_t)noise & 15) || ((uintptr_t)x0 & 15) ||
      ((uintptr_t)noise0 & 15) || ((uintptr_t)mask & 15) || ((uintptr_t)x_out & 15) || ((uintptr_t)x_out_bf16 & 15))
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
  const int64_t cps = n / 8, chunks = cps * batch;
  const int64_t cap = max_blocks > 0 ? max_blocks : 2048;          // as afx_teacher_euler_step: 8 work-groups per CU
  const unsigned grid = (unsigned)std::min<int64_t>((chunks + 255) / 256, cap);
  if (sde)
    hipLaunchKernelGGL(teacher_edit_step_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (const bf16_t*)pos, (const bf16_t*)neg,
                       noise, sigma, sigma_to, m, c_noise, coef, scale, x0, noise0, mask, x_out, (bf16_t*)x_out_bf16, cps, chunks);
  else
    hipLaunchKernelGGL(teacher_edit_step_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, (const bf16_t*)pos, (const bf16_t*)neg,
                       (const float*)nullptr, sigma, sigma_to, (const float*)nullptr, (const float*)nullptr, coef, scale, x0, noise0, mask, x_out,
                       (bf16_t*)x_out_bf16, cps, chunks);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
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
  if (batch < 0 || n < 64 || n % 64) return (int64_t)fail(AFX_E_INVALID, "bad argument to afx_cfg_ortho_ws_bytes");
  return (int64_t)batch * ortho_parts(n) * 2 * (int64_t)sizeof(double);
}

int afx_cfg_ortho_coef(const void* pos, const void* neg, float scale, float* coef, void* ws, int64_t ws_bytes, int32_t batch,
                       int64_t n, void* stream) {
  if (!pos || !neg || !coef || !ws) return fail(AFX_E_INVALID, "null argument to afx_cfg_ortho_coef");
  if (batch < 0 || batch > 65535 || n < 64 || n % 64)
    return fail(AFX_E_INVALID, "bad argument to afx_cfg_ortho_coef (n = tokens x channels must be a positive multiple of 64)");
  if (((uintptr_t)pos & 15) || ((uintptr_t)neg & 15) || ((uintptr_t)ws & 7))
    return fail(AFX_E_INVALID, "afx_cfg_ortho_coef: pos and neg must be 16-byte aligned, ws 8-byte aligned");
  const int parts = ortho_parts(n);
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

int64_t afx_sample_score_ws_bytes(int32_t batch, int64_t n) {
  if (batch < 0 || n < 64 || n % 64) return (int64_t)fail(AFX_E_INVALID, "bad argument to afx_sample_score_ws_bytes");
  return (int64_t)batch * ortho_parts(n) * 4 * (int64_t)sizeof(double);
}

int afx_sample_score(const void* a, const void* b, int32_t dtype, int32_t transform, double* out, void* ws, int64_t ws_bytes,
                     int32_t batch, int64_t n, void* stream) {
  if (!a || !b || !out || !ws) return fail(AFX_E_INVALID, "null argument to afx_sample_score");
  if (dtype != AFX_DT_BF16 && dtype != AFX_DT_F32) return fail(AFX_E_INVALID, "afx_sample_score: dtype must be AFX_DT_BF16 or AFX_DT_F32");
  if (transform != 0 && transform != 1) return fail(AFX_E_INVALID, "afx_sample_score: transform must be 0 or 1");
  if (batch < 0 || batch > 65535 || n < 64 || n % 64)
    return fail(AFX_E_INVALID, "bad argument to afx_sample_score (n = elements per sample must be a positive multiple of 64)");
  if (((uintptr_t)a & 15) || ((uintptr_t)b & 15) || ((uintptr_t)out & 7) || ((uintptr_t)ws & 7))
    return fail(AFX_E_INVALID, "afx_sample_score: a and b must be 16-byte aligned, out and ws 8-byte aligned");
  const int parts = ortho_parts(n);
  if (ws_bytes < (int64_t)batch * parts * 4 * (int64_t)sizeof(double))
    return fail(AFX_E_INVALID, "afx_sample_score: workspace smaller than afx_sample_score_ws_bytes()");
  if (batch == 0) return AFX_OK;
  const bool bf16 = dtype == AFX_DT_BF16;
  const int64_t ups = n / (bf16 ? 8 : 4), upw = (ups + parts - 1) / parts;
  hipStream_t st = (hipStream_t)stream;
  if (bf16)
    hipLaunchKernelGGL(sample_score_partial_kernel<true>, dim3(parts, batch), dim3(256), 0, st, a, b, (int)transform, (double*)ws, ups, upw);
  else
    hipLaunchKernelGGL(sample_score_partial_kernel<false>, dim3(parts, batch), dim3(256), 0, st, a, b, (int)transform, (double*)ws, ups, upw);
  hipLaunchKernelGGL(sample_score_finish_kernel, dim3((batch * 4 + 63) / 64), dim3(64), 0, st, (const double*)ws, out, batch, parts);
  HIP_TRY(hipGetLastError());
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

int64_t afx_image_ssim_ws_bytes(int32_t batch, int32_t C, int32_t H, int32_t W) {
  if (batch < 1 || C < 1 || H < SSIM_TAPS || W < SSIM_TAPS) return (int64_t)fail(AFX_E_INVALID, "bad argument to afx_image_ssim_ws_bytes (batch and C at least 1, H and W at least 11)");
  const int64_t parts = ssim_parts(C, H, W, nullptr, nullptr);
  if (parts > INT32_MAX) return (int64_t)fail(AFX_E_INVALID, "afx_image_ssim_ws_bytes: more than 2^31 - 1 tiles per sample");
  return (int64_t)batch * parts * (int64_t)sizeof(double);
}

int afx_image_ssim(const void* a, const void* b, int32_t dtype, int32_t transform, double data_range, double* out, void* ws,
                   int64_t ws_bytes, int32_t batch, int32_t C, int32_t H, int32_t W, void* stream) {
  if (!a || !b || !out || !ws) return fail(AFX_E_INVALID, "null argument to afx_image_ssim");
  if (dtype != AFX_DT_BF16 && dtype != AFX_DT_F32) return fail(AFX_E_INVALID, "afx_image_ssim: dtype must be AFX_DT_BF16 or AFX_DT_F32");
  if (transform != 0 && transform != 1) return fail(AFX_E_INVALID, "afx_image_ssim: transform must be 0 or 1");
  if (!(data_range > 0.0) || data_range > 1e150) return fail(AFX_E_INVALID, "afx_image_ssim: data_range must be positive (and finite)");
  if (batch < 1 || batch > 65535 || C < 1) return fail(AFX_E_INVALID, "bad argument to afx_image_ssim (1 <= batch <= 65535, C >= 1)");
  if (H < SSIM_TAPS || W < SSIM_TAPS) return fail(AFX_E_INVALID, "afx_image_ssim: H and W must be at least 11 (one window)");
  const bool bf16 = dtype == AFX_DT_BF16;
  if (((uintptr_t)a & (bf16 ? 1 : 3)) || ((uintptr_t)b & (bf16 ? 1 : 3)) || ((uintptr_t)out & 7) || ((uintptr_t)ws & 7))
    return fail(AFX_E_INVALID, "afx_image_ssim: a and b must be aligned to their element, out and ws 8-byte aligned");
  int tiles_x = 0, tiles = 0;
  const int64_t parts = ssim_parts(C, H, W, &tiles_x, &tiles);
  if (parts > INT32_MAX) return fail(AFX_E_INVALID, "afx_image_ssim: more than 2^31 - 1 tiles per sample");
  if (ws_bytes < (int64_t)batch * parts * (int64_t)sizeof(double))
    return fail(AFX_E_INVALID, "afx_image_ssim: workspace smaller than afx_image_ssim_ws_bytes()");
  const ssim_taps_t taps = ssim_window();
  const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
  hipStream_t st = (hipStream_t)stream;
  if (bf16)
    hipLaunchKernelGGL(image_ssim_partial_kernel<true>, dim3((unsigned)parts, batch), dim3(256), 0, st, a, b, (int)transform, taps, c1, c2,
                       (double*)ws, (int)H, (int)W, tiles_x, tiles);
  else
    hipLaunchKernelGGL(image_ssim_partial_kernel<false>, dim3((unsigned)parts, batch), dim3(256), 0, st, a, b, (int)transform, taps, c1, c2,
                       (double*)ws, (int)H, (int)W, tiles_x, tiles);
  hipLaunchKernelGGL(image_ssim_finish_kernel, dim3(batch), dim3(64), 0, st, (const double*)ws, out, (int)parts);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

int64_t afx_sample_score_masked_ws_bytes(int32_t batch, int64_t n) {
  if (batch < 0 || n < 64 || n % 64 || n > INT32_MAX) return (int64_t)fail(AFX_E_INVALID, "bad argument to afx_sample_score_masked_ws_bytes (n must be a positive multiple of 64 below 2^31)");
  return (int64_t)batch * ortho_parts(n) * 10 * (int64_t)sizeof(double);
}

int afx_sample_score_masked(const void* a, const void* b, const float* mask, int32_t dtype, int32_t transform, double* out, void* ws,
                            int64_t ws_bytes, int32_t batch, int32_t mask_batch, int32_t G, int32_t P, int32_t R, int32_t Q, void* stream) {
  if (!a || !b || !mask || !out || !ws) return fail(AFX_E_INVALID, "null argument to afx_sample_score_masked");
  if (dtype != AFX_DT_BF16 && dtype != AFX_DT_F32)
    return fail(AFX_E_INVALID, "afx_sample_score_masked: dtype must be AFX_DT_BF16 or AFX_DT_F32");
  if (transform != 0 && transform != 1) return fail(AFX_E_INVALID, "afx_sample_score_masked: transform must be 0 or 1");
  if (batch < 0 || batch > 65535 || G < 1 || P < 1 || R < 1 || Q < 1)
    return fail(AFX_E_INVALID, "bad argument to afx_sample_score_masked (0 <= batch <= 65535; G, P, R, Q >= 1)");
  if (R % Q) return fail(AFX_E_INVALID, "afx_sample_score_masked: Q = %d must divide R = %d", (int)Q, (int)R);
  if (mask_batch != 1 && mask_batch != batch)
    return fail(AFX_E_INVALID, "afx_sample_score_masked: mask_batch must be 1 or batch = %d, got %d", (int)batch, (int)mask_batch);
  const int64_t pr = (int64_t)P * R;
  if (pr > INT32_MAX || pr * G > INT32_MAX || (pr * G) % 64)
    return fail(AFX_E_INVALID, "bad argument to afx_sample_score_masked (n = G P R elements per sample must be a multiple of 64 below 2^31)");
  const int64_t n = pr * G;
  if (((uintptr_t)a & 15) || ((uintptr_t)b & 15) || ((uintptr_t)mask & 3) || ((uintptr_t)out & 7) || ((uintptr_t)ws & 7))
    return fail(AFX_E_INVALID, "afx_sample_score_masked: a and b must be 16-byte aligned, mask 4-byte, out and ws 8-byte aligned");
  const int parts = ortho_parts(n);
  if (ws_bytes < (int64_t)batch * parts * 10 * (int64_t)sizeof(double))
    return fail(AFX_E_INVALID, "afx_sample_score_masked: workspace smaller than afx_sample_score_masked_ws_bytes()");
  if (batch == 0) return AFX_OK;
  const bool bf16 = dtype == AFX_DT_BF16;
  const int64_t ups = n / (bf16 ? 8 : 4), upw = (ups + parts - 1) / parts;          // the partition of afx_sample_score
  const int64_t mstride = mask_batch == 1 ? 0 : (int64_t)P * Q;
  hipStream_t st = (hipStream_t)stream;
  if (bf16)
    hipLaunchKernelGGL(sample_score_masked_partial_kernel<true>, dim3(parts, batch), dim3(256), 0, st, a, b, mask, (int)transform, (double*)ws,
                       ups, upw, mstride, (uint32_t)P, (uint32_t)R, (uint32_t)Q);
  else
    hipLaunchKernelGGL(sample_score_masked_partial_kernel<false>, dim3(parts, batch), dim3(256), 0, st, a, b, mask, (int)transform, (double*)ws,
                       ups, upw, mstride, (uint32_t)P, (uint32_t)R, (uint32_t)Q);
  hipLaunchKernelGGL(sample_score_masked_finish_kernel, dim3((batch * 10 + 63) / 64), dim3(64), 0, st, (const double*)ws, out, batch, parts);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

int64_t afx_image_ssim_masked_ws_bytes(int32_t batch, int32_t C, int32_t H, int32_t W) {
  if (batch < 1 || C < 1 || H < SSIM_TAPS || W < SSIM_TAPS)
    return (int64_t)fail(AFX_E_INVALID, "bad argument to afx_image_ssim_masked_ws_bytes (batch and C at least 1, H and W at least 11)");
  const int64_t parts = ssim_parts(C, H, W, nullptr, nullptr);
  if (parts > INT32_MAX) return (int64_t)fail(AFX_E_INVALID, "afx_image_ssim_masked_ws_bytes: more than 2^31 - 1 tiles per sample");
  return (int64_t)batch * parts * 4 * (int64_t)sizeof(double);
}

int afx_image_ssim_masked(const void* a, const void* b, const float* mask, int32_t dtype, int32_t transform, double data_range, double* out,
                          void* ws, int64_t ws_bytes, int32_t batch, int32_t mask_batch, int32_t C, int32_t H, int32_t W, void* stream) {
  if (!a || !b || !mask || !out || !ws) return fail(AFX_E_INVALID, "null argument to afx_image_ssim_masked");
  if (dtype != AFX_DT_BF16 && dtype != AFX_DT_F32) return fail(AFX_E_INVALID, "afx_image_ssim_masked: dtype must be AFX_DT_BF16 or AFX_DT_F32");
  if (transform != 0 && transform != 1) return fail(AFX_E_INVALID, "afx_image_ssim_masked: transform must be 0 or 1");
  if (!(data_range > 0.0) || data_range > 1e150) return fail(AFX_E_INVALID, "afx_image_ssim_masked: data_range must be positive (and finite)");
  if (batch < 1 || batch > 65535 || C < 1) return fail(AFX_E_INVALID, "bad argument to afx_image_ssim_masked (1 <= batch <= 65535, C >= 1)");
  if (mask_batch != 1 && mask_batch != batch)
    return fail(AFX_E_INVALID, "afx_image_ssim_masked: mask_batch must be 1 or batch = %d, got %d", (int)batch, (int)mask_batch);
  if (H < SSIM_TAPS || W < SSIM_TAPS) return fail(AFX_E_INVALID, "afx_image_ssim_masked: H and W must be at least 11 (one window)");
  const bool bf16 = dtype == AFX_DT_BF16;
  if (((uintptr_t)a & (bf16 ? 1 : 3)) || ((uintptr_t)b & (bf16 ? 1 : 3)) || ((uintptr_t)mask & 3) || ((uintptr_t)out & 7) || ((uintptr_t)ws & 7))
    return fail(AFX_E_INVALID, "afx_image_ssim_masked: a, b and mask must be aligned to their element, out and ws 8-byte aligned");
  int tiles_x = 0, tiles = 0;
  const int64_t parts = ssim_parts(C, H, W, &tiles_x, &tiles);
  if (parts > INT32_MAX) return fail(AFX_E_INVALID, "afx_image_ssim_masked: more than 2^31 - 1 tiles per sample");
  if (ws_bytes < (int64_t)batch * parts * 4 * (int64_t)sizeof(double))
    return fail(AFX_E_INVALID, "afx_image_ssim_masked: workspace smaller than afx_image_ssim_masked_ws_bytes()");
  const ssim_taps_t taps = ssim_window();
  const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
  const int64_t mstride = mask_batch == 1 ? 0 : (int64_t)H * W;
  hipStream_t st = (hipStream_t)stream;
  if (bf16)
    hipLaunchKernelGGL(image_ssim_masked_partial_kernel<true>, dim3((unsigned)parts, batch), dim3(256), 0, st, a, b, mask, (int)transform, taps, c1,
                       c2, (double*)ws, (int)H, (int)W, tiles_x, tiles, mstride);
  else
    hipLaunchKernelGGL(image_ssim_masked_partial_kernel<false>, dim3((unsigned)parts, batch), dim3(256), 0, st, a, b, mask, (int)transform, taps, c1,
                       c2, (double*)ws, (int)H, (int)W, tiles_x, tiles, mstride);
  hipLaunchKernelGGL(image_ssim_masked_finish_kernel, dim3(batch, 4), dim3(64), 0, st, (const double*)ws, out, (int)parts);
  HIP_TRY(hipGetLastError());
  return AFX_OK;
}

}  // extern "C"
