// The analytic ArcFlow policy, forward and backward (lakonlab/models/diffusions/arcflow.py:81-110, policies/arcflow.py:52-76; token layout of
// arcflux_pipeline.py:195-249 + the (un)pack permutes):
//     D[c] = sum_k softmax_k(logw)[k, c % pp] * m[k, c] * e_k
//   step mode:      e_0 = Dt,  e_k = exp(g_k Dp) * Dt * phi(g_k Dt)       (D = displacement, x_end = x - D)
//   velocity mode:  e_0 = 1,   e_k = exp(g_k Dp)                           (D = u)
// with Dp = s_src - s_start, Dt = s_start - s_end and phi(z) = expm1(z) / z on z clamped away from 0.
//   * arcflow_step_kernel:      any (K <= ARC_MAXK, ch, pp), one wave per token, the K terms walked in registers
//   * arcflow_step_k16_kernel:  the shipped shape (K, ch, pp) = (16, 64, 4), one coefficient per lane
//   * arcflow_bwd_kernel:       d/d(means, logw, logg) of D, which the reference leaves to torch autograd
// and their four C entry points.  The pieces of the formula the kernels share are written once, in front of them.
#include <cstdlib>
#include <type_traits>

#include "afx_api_util.h"
#include "afx_common.h"
#include "afx_kernels.h"

namespace afx {

constexpr int ARC_MAXK = 32;      // mixture components a lane can hold in registers: the limit of kernels, launchers and entries

template <typename MixT> AFX_DEV float mix_load(const MixT* p, int64_t i);
template <> AFX_DEV float mix_load<float>(const float* p, int64_t i) { return p[i]; }
template <> AFX_DEV float mix_load<bf16_t>(const bf16_t* p, int64_t i) { return bf16_to_f32(p[i]); }

// The sigma gaps of sample bidx: per-sample triples (s_src, s_start, s_end) in sigma_vec where it is given, else the scalars.
struct SigmaGaps { float d_past, d_step; };
AFX_DEV SigmaGaps sigma_gaps(float s_src, float s_start, float s_end, const float* __restrict__ sigma_vec, int64_t bidx) {
  if (sigma_vec != nullptr) {
    s_src = sigma_vec[3 * bidx];
    s_start = sigma_vec[3 * bidx + 1];
    s_end = sigma_vec[3 * bidx + 2];
  }
  return {s_src - s_start, s_start - s_end};
}

// The step factor of one component: z = g d_step clamped to |zs| >= eps (sign kept), em1 = expm1(zs), phi = em1 / zs.  `clamped` is the one
// place that says the clamp acted (phi does not depend on z there: phi' = 0).  The product decay * d_step * phi is NOT formed here: the
// generic step multiplies m * decay * d_step * phi, the K = 16 step coef *= decay; coef *= d_step * (em1 / zs), the backward
// dec * d_step * phi -- each kernel keeps its own order of multiplications, and with it its bits.
struct StepFactor { float zs, em1, phi; bool clamped; };
AFX_DEV StepFactor step_factor(float g, float d_step, float eps) {
  const float z = g * d_step;
  const float zs = (z < 0.f ? -1.0f : 1.0f) * fmaxf(fabsf(z), eps);
  const float em1 = expm1f(zs);
  return {zs, em1, em1 / zs, fabsf(z) < eps};
}

// Softmax over the K components of sub-pixel q in registers: w[k] = exp(logw[k, q] - max) for k < K, the return value is 1 / sum_k w[k].
// dr != nullptr: GM dropout, component k with dr[k] != 0 is removed (-inf).
template <typename MixT>
AFX_DEV float softmax_k(const MixT* wt, int K, int pp, int q, const uint8_t* dr, float (&w)[ARC_MAXK]) {
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < ARC_MAXK; ++k)
    if (k < K) {
      w[k] = (dr && dr[k]) ? -INFINITY : mix_load<MixT>(wt, k * pp + q);
      mx = fmaxf(mx, w[k]);
    }
  float den = 0.f;
#pragma unroll
  for (int k = 0; k < ARC_MAXK; ++k)
    if (k < K) {
      w[k] = expf(w[k] - mx);
      den += w[k];
    }
  return 1.0f / den;
}

// ------------------------------------------------------------------------------------------------
// The step in the token layout: one wave per token, lane = packed channel (ch = C*p*p = 64 for FLUX/Qwen), the K mixture terms are
// walked in registers.  21 MB of traffic per 1024^2 step -> pure HBM streaming.
template <typename MixT>
__global__ __launch_bounds__(256) void arcflow_step_kernel(
    const float* __restrict__ x_in, const MixT* __restrict__ means, const MixT* __restrict__ logw,
    const MixT* __restrict__ logg, float s_src, float s_start, float s_end,
    const float* __restrict__ sigma_vec, float eps, float* __restrict__ x_out, int64_t tokens, int n_tok, int K,
    int ch, int pp, int velocity_only, const uint8_t* __restrict__ drop) {
  const int lane = threadIdx.x & 63;
  const int64_t tok = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tok >= tokens) return;
  const int64_t bidx = tok / n_tok;
  const auto [d_past, d_step] = sigma_gaps(s_src, s_start, s_end, sigma_vec, bidx);
  const uint8_t* dr = drop ? drop + bidx * K : nullptr;      // GM dropout: component k of sample b removed
  const MixT* mt = means + tok * (int64_t)K * ch;
  const MixT* wt = logw + tok * (int64_t)K * pp;
  const MixT* gt = logg + tok * (int64_t)(K - 1) * pp;
  for (int c = lane; c < ch; c += 64) {
    const int q = c % pp;
    float lw[ARC_MAXK];
    const float inv = softmax_k<MixT>(wt, K, pp, q, dr, lw);
    // k = 0: straight-line component (d = phi = 1)
    float acc = (lw[0] * inv) * mix_load<MixT>(mt, c) * (velocity_only ? 1.0f : d_step);
#pragma unroll
    for (int k = 1; k < ARC_MAXK; ++k)
      if (k < K) {
        const float g = mix_load<MixT>(gt, (k - 1) * pp + q);
        const float m = mix_load<MixT>(mt, (int64_t)k * ch + c);
        const float decay = expf(g * d_past);
        float term;
        if (velocity_only) {
          term = m * decay;
        } else {
          term = m * decay * d_step * step_factor(g, d_step, eps).phi;
        }
        acc += (lw[k] * inv) * term;
      }
    const int64_t xi = tok * ch + c;
    x_out[xi] = velocity_only ? acc : (x_in[xi] - acc);
  }
}

// Fast path for the shipped mixture shape (K = 16 components, ch = C p^2 = 64 packed channels, pp = p^2 = 4 sub-pixels: FLUX and
// Qwen-Image alike).  The step is  x_out[c] = x[c] - sum_k coef[k][c % 4] * mean[k][c]  with
//     coef[k][q] = softmax_k(logw[.][q]) * exp(gamma_k d_past) * d_step * phi(gamma_k d_step)        (k = 0: d = phi = 1)
// -- K * pp = 64 coefficients per token, i.e. exactly ONE per lane: every transcendental of the token is evaluated once
// (the generic kernel above evaluates each of them in all 16 lanes that share a sub-pixel), the softmax over K is a 4-step
// xor-shuffle over the lanes of one sub-pixel, and the token's 1024 means arrive as two 16-byte loads per lane.  Lane l then
// owns 8 channels of components l/8 and 8 + l/8; a 3-step reduce-scatter (4 + 2 + 1 exchanges) over the 8 lanes that share
// l % 8 leaves every lane with ONE fully summed channel, so x is read and written as one coalesced 256-byte row per token.
// TPW tokens per wave with all of their loads issued up front (2 x 2.8 KB in flight per wave): HBM streaming, not latency.
template <typename MixT> struct Mix8;
template <> struct Mix8<bf16_t> {
  AFX_DEV static void load(const bf16_t* p, float (&f)[8]) { unpack8(*reinterpret_cast<const u32x4_t*>(p), f); }
};
template <> struct Mix8<float> {
  AFX_DEV static void load(const float* p, float (&f)[8]) {
    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(p), b = *reinterpret_cast<const f32x4_t*>(p + 4);
    f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3]; f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
  }
};

template <typename MixT, int TPW>
__global__ __launch_bounds__(256) void arcflow_step_k16_kernel(
    const float* __restrict__ x_in, const MixT* __restrict__ means, const MixT* __restrict__ logw,
    const MixT* __restrict__ logg, float s_src0, float s_start0, float s_end0, const float* __restrict__ sigma_vec, float eps,
    float* __restrict__ x_out, int64_t tokens, int n_tok, int velocity_only, const uint8_t* __restrict__ drop) {
  constexpr int K = 16, CH = 64, PP = 4;
  const int lane = threadIdx.x & 63;
  const int64_t tok0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * TPW;
  if (tok0 >= tokens) return;
  const int k = lane >> 2;                       // this lane's coefficient: component k, sub-pixel lane & 3
  float mA[TPW][8], mB[TPW][8], lw[TPW], lg[TPW], xv[TPW];
  // ---- every load of the wave's tokens first -------------------------------------------------------------------------
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int64_t tok = tok0 + t < tokens ? tok0 + t : tokens - 1;      // wave-uniform clamp (the tail token is not stored)
    const MixT* mt = means + tok * (int64_t)(K * CH);
    Mix8<MixT>::load(mt + lane * 8, mA[t]);                             // component lane/8,      channels (lane%8)*8 ..
    Mix8<MixT>::load(mt + (64 + lane) * 8, mB[t]);                      // component 8 + lane/8
    lw[t] = mix_load<MixT>(logw + tok * (K * PP), lane);
    lg[t] = k > 0 ? mix_load<MixT>(logg + tok * ((K - 1) * PP), lane - PP) : 0.f;
  }
  const int e3 = ((lane >> 5) & 1) * 4 + ((lane >> 4) & 1) * 2 + ((lane >> 3) & 1);   // channel (inside the lane's 8) left after the reduce-scatter
  const int cfin = (lane & 7) * 8 + e3;
  if (!velocity_only) {
#pragma unroll
    for (int t = 0; t < TPW; ++t) xv[t] = x_in[(tok0 + t < tokens ? tok0 + t : tokens - 1) * CH + cfin];
  }
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int64_t tok = tok0 + t;
    if (tok >= tokens) break;                    // wave-uniform
    const int64_t bidx = tok / n_tok;
    const auto [d_past, d_step] = sigma_gaps(s_src0, s_start0, s_end0, sigma_vec, bidx);
    float l = lw[t];
    if (drop != nullptr && drop[bidx * K + k]) l = -INFINITY;           // GM dropout: component k of sample b removed
    // softmax over the 16 components of this sub-pixel: lanes q, q+4, ..., q+60
    float mx = l;
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    const float ex = expf(l - mx);
    float den = ex;
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) den += __shfl_xor(den, o, 64);
    float coef = ex / den;
    if (k > 0) {
      const float g = lg[t];
      coef *= expf(g * d_past);
      if (!velocity_only) {
        const StepFactor f = step_factor(g, d_step, eps);
        coef *= d_step * (f.em1 / f.zs);
      }
    } else if (!velocity_only) {
      coef *= d_step;                             // k = 0: straight-line component (d = phi = 1)
    }
    // the 4 coefficients (sub-pixels) of this lane's two components
    float cA[4], cB[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      cA[q] = __shfl(coef, (lane >> 3) * 4 + q, 64);
      cB[q] = __shfl(coef, (8 + (lane >> 3)) * 4 + q, 64);
    }
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = cA[e & 3] * mA[t][e] + cB[e & 3] * mB[t][e];
    // reduce-scatter over the 8 lanes sharing lane % 8 (xor 32, 16, 8): 4 + 2 + 1 exchanges
    const bool h5 = (lane & 32) != 0, h4 = (lane & 16) != 0, h3 = (lane & 8) != 0;
    float w4[4], w2[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float keep = h5 ? v[4 + i] : v[i], send = h5 ? v[i] : v[4 + i];
      w4[i] = keep + __shfl_xor(send, 32, 64);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float keep = h4 ? w4[2 + i] : w4[i], send = h4 ? w4[i] : w4[2 + i];
      w2[i] = keep + __shfl_xor(send, 16, 64);
    }
    const float keep = h3 ? w2[1] : w2[0], send = h3 ? w2[0] : w2[1];
    const float acc = keep + __shfl_xor(send, 8, 64);
    x_out[tok * CH + cfin] = velocity_only ? acc : (xv[t] - acc);
  }
}

// ------------------------------------------------------------------------------------------------
// d/d(means, logw, logg) of D given the upstream gradient gD = gscale[b] * g[c].  One wave per token, lane = packed channel (ch <= 64,
// pp a power of two dividing 64): the reductions over the channels that share a sub-pixel q = c % pp are xor-shuffles over lane
// bits >= log2(pp).

// phi'(z) = sum_n z^n / (n! (n + 2)) for |z| < 1.  The closed form (e^z - phi) / z subtracts two numbers near 1 there and loses u * 4 / |z|
// relative (1e-3 at z = 1e-4, against fp64); from |z| = 1 on nothing cancels and it is kept.  Twelve terms: the first one left out,
// z^12 / (12! * 14) <= 1.5e-10, is 1e-2 u of the smallest value on the interval, phi'(-1) = 0.26; Horner's own roundings stay below 3 u.
AFX_DEV float dphi_series(float z) {
  float p = 1.0f / 518918400.0f;                  // 1 / (11! * 13)
  p = fmaf(p, z, 1.0f / 43545600.0f);             // 1 / (10! * 12)
  p = fmaf(p, z, 1.0f / 3991680.0f);              // 1 / (9! * 11)
  p = fmaf(p, z, 1.0f / 403200.0f);               // 1 / (8! * 10)
  p = fmaf(p, z, 1.0f / 45360.0f);                // 1 / (7! * 9)
  p = fmaf(p, z, 1.0f / 5760.0f);                 // 1 / (6! * 8)
  p = fmaf(p, z, 1.0f / 840.0f);                  // 1 / (5! * 7)
  p = fmaf(p, z, 1.0f / 144.0f);                  // 1 / (4! * 6)
  p = fmaf(p, z, 1.0f / 30.0f);                   // 1 / (3! * 5)
  p = fmaf(p, z, 1.0f / 8.0f);                    // 1 / (2! * 4)
  p = fmaf(p, z, 1.0f / 3.0f);                    // 1 / (1! * 3)
  return fmaf(p, z, 0.5f);                        // 1 / (0! * 2)
}

template <typename MixT>
__global__ __launch_bounds__(256) void arcflow_bwd_kernel(
    const float* __restrict__ g, const MixT* __restrict__ means, const MixT* __restrict__ logw,
    const MixT* __restrict__ logg, float s_src, float s_start, float s_end, const float* __restrict__ sigma_vec,
    const float* __restrict__ gscale_vec, float gscale, float eps, float* __restrict__ d_means,
    float* __restrict__ d_logw, float* __restrict__ d_logg, int64_t tokens, int n_tok, int K, int ch, int pp,
    int velocity_only, int accumulate) {
  const int lane = threadIdx.x & 63;
  const int64_t tok = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tok >= tokens) return;
  const int64_t b = tok / n_tok;
  const auto [d_past, d_step] = sigma_gaps(s_src, s_start, s_end, sigma_vec, b);
  if (gscale_vec != nullptr) gscale *= gscale_vec[b];
  const bool active = lane < ch;
  const int c = active ? lane : 0;
  const int q = c % pp;
  const MixT* mt = means + tok * (int64_t)K * ch;
  const MixT* wt = logw + tok * (int64_t)K * pp;
  const MixT* gt = logg + tok * (int64_t)(K - 1) * pp;
  const float gD = active ? gscale * g[tok * ch + c] : 0.f;

  float w[ARC_MAXK];
  const float inv = softmax_k<MixT>(wt, K, pp, q, nullptr, w);

  float* dm = d_means + tok * (int64_t)K * ch;
  float* dw = d_logw + tok * (int64_t)K * pp;
  float* dg = d_logg + tok * (int64_t)(K - 1) * pp;
  float a[ARC_MAXK];       // a_k = e_k * sum_{c in q} gD_c m_{k,c}
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < ARC_MAXK; ++k)
    if (k < K) {
      w[k] *= inv;
      const float m = mix_load<MixT>(mt, (int64_t)k * ch + c);
      float e, de;
      if (k == 0) {
        e = velocity_only ? 1.0f : d_step;
        de = 0.f;
      } else {
        const float gam = mix_load<MixT>(gt, (k - 1) * pp + q);
        const float dec = expf(gam * d_past);
        if (velocity_only) {
          e = dec;
          de = d_past * dec;
        } else {
          const StepFactor f = step_factor(gam, d_step, eps);
          // phi'(z): 0 inside the clamp, its series below |z| = 1, the closed form above
          const float dphi = f.clamped ? 0.f : (fabsf(f.zs) < 1.0f ? dphi_series(f.zs) : (f.em1 + 1.0f - f.phi) / f.zs);
          e = dec * d_step * f.phi;
          de = d_past * e + dec * d_step * dphi * d_step;
        }
      }
      // gradient w.r.t. the mean of this lane's channel
      if (active) {
        const float v = gD * w[k] * e;
        dm[(int64_t)k * ch + c] = accumulate ? dm[(int64_t)k * ch + c] + v : v;
      }
      // r_k = sum over the channels of sub-pixel q of gD_c m_{k,c}
      float r = gD * m;
      for (int o = pp; o < 64; o <<= 1) r += __shfl_xor(r, o, 64);
      a[k] = e * r;
      s += w[k] * a[k];
      if (k > 0 && lane < pp) {
        const float v = w[k] * de * r;
        dg[(k - 1) * pp + q] = accumulate ? dg[(k - 1) * pp + q] + v : v;
      }
    }
  if (lane < pp) {
#pragma unroll
    for (int k = 0; k < ARC_MAXK; ++k)
      if (k < K) {
        const float v = w[k] * (a[k] - s);
        dw[k * pp + q] = accumulate ? dw[k * pp + q] + v : v;
      }
  }
}

// ------------------------------------------------------------------------------------------------
// f(tag) with a null pointer of the mixture's element type: the body names it as std::remove_pointer_t<decltype(tag)>
template <class F>
static void with_mix_type(int mix_bf16, F&& f) {
  if (mix_bf16) f((bf16_t*)nullptr); else f((float*)nullptr);
}

hipError_t launch_arcflow_step(const float* x_in, const void* means, const void* logw, const void* logg,
                               int mix_bf16, float s_src, float s_start, float s_end,
                               const float* sigma_vec, float eps, float* x_out, int B, int n_tok, int K,
                               int ch, int pp, int velocity_only, const uint8_t* drop, hipStream_t stream) {
  if (K < 1 || K > ARC_MAXK || pp < 1 || ch < 1) return hipErrorInvalidValue;
  const int64_t tokens = (int64_t)B * n_tok;
  if (tokens == 0) return hipSuccess;
  if (K == 16 && ch == 64 && pp == 4) {             // the shipped mixture shape: one coefficient per lane (see above)
    static int tpw = -1;
    if (tpw < 0) {
      const char* e = getenv("AFX_STEP_TPW");       // tokens per wave: 1 | 2 | 4 (cold-cache kernel time at 1024^2, r02p: 6.1 | 6.6 | 8.8 us)
      tpw = e ? atoi(e) : 1;
      if (tpw != 1 && tpw != 2 && tpw != 4) tpw = 1;
    }
    with_mix_type(mix_bf16, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      auto launch = [&](auto tpw_c) {
        constexpr int TPW = decltype(tpw_c)::value;
        hipLaunchKernelGGL((arcflow_step_k16_kernel<T, TPW>), dim3((unsigned)((tokens + 4 * TPW - 1) / (4 * TPW))), dim3(256), 0, stream,
                           x_in, (const T*)means, (const T*)logw, (const T*)logg, s_src, s_start, s_end, sigma_vec, eps, x_out, tokens,
                           n_tok, velocity_only, drop);
      };
      if (tpw == 1) launch(std::integral_constant<int, 1>{});
      else if (tpw == 4) launch(std::integral_constant<int, 4>{});
      else launch(std::integral_constant<int, 2>{});
    });
    return hipGetLastError();
  }
  with_mix_type(mix_bf16, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL(arcflow_step_kernel<T>, dim3((unsigned)((tokens + 3) / 4)), dim3(256), 0, stream, x_in, (const T*)means,
                       (const T*)logw, (const T*)logg, s_src, s_start, s_end, sigma_vec, eps, x_out, tokens, n_tok, K, ch, pp,
                       velocity_only, drop);
  });
  return hipGetLastError();
}

// what arcflow_bwd_kernel can walk: lane = channel, and the sub-pixel reductions are xor-shuffles inside the wave
static bool arcflow_bwd_shape_ok(int K, int ch, int pp) {
  return K >= 1 && K <= ARC_MAXK && ch >= 1 && ch <= 64 && pp >= 1 && !(pp & (pp - 1)) && 64 % pp == 0 && ch % pp == 0;
}

hipError_t launch_arcflow_bwd(const float* g, const void* means, const void* logw, const void* logg, int mix_bf16,
                              float s_src, float s_start, float s_end, const float* sigma_vec,
                              const float* gscale_vec, float gscale, float eps, float* d_means, float* d_logw,
                              float* d_logg, int B, int n_tok, int K, int ch, int pp, int velocity_only,
                              int accumulate, hipStream_t stream) {
  if (!arcflow_bwd_shape_ok(K, ch, pp)) return hipErrorInvalidValue;
  const int64_t tokens = (int64_t)B * n_tok;
  if (tokens == 0) return hipSuccess;
  with_mix_type(mix_bf16, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL(arcflow_bwd_kernel<T>, dim3((unsigned)((tokens + 3) / 4)), dim3(256), 0, stream, g, (const T*)means,
                       (const T*)logw, (const T*)logg, s_src, s_start, s_end, sigma_vec, gscale_vec, gscale, eps, d_means, d_logw,
                       d_logg, tokens, n_tok, K, ch, pp, velocity_only, accumulate);
  });
  return hipGetLastError();
}

}  // namespace afx

using namespace afx;

// the mixture arguments the three forward entry points share
static int arcflow_args(const char* fn, bool operands, int32_t mix_dtype, int32_t batch, int32_t n_tok, int32_t K, int32_t ch, int32_t pp) {
  if (!operands) return fail(AFX_E_INVALID, "null argument to %s", fn);
  if (mix_dtype != AFX_DT_BF16 && mix_dtype != AFX_DT_F32) return fail(AFX_E_INVALID, "bad mix_dtype");
  if (batch < 0 || n_tok < 0 || K < 1 || K > ARC_MAXK || ch < 1 || pp < 1 || ch % pp != 0) return fail(AFX_E_INVALID, "bad shape for %s", fn);
  return AFX_OK;
}

extern "C" {

int afx_arcflow_step(const float* x_in, const void* means, const void* logw, const void* logg, int32_t mix_dtype,
                     float sigma_src, float sigma_start, float sigma_end, const float* sigma_vec, float eps,
                     float* x_out, int32_t batch, int32_t n_tok, int32_t K, int32_t ch, int32_t pp, void* stream) {
  AFX_TRY(arcflow_args("afx_arcflow_step", x_in && means && logw && logg && x_out, mix_dtype, batch, n_tok, K, ch, pp));
  HIP_TRY(launch_arcflow_step(x_in, means, logw, logg, mix_dtype == AFX_DT_BF16, sigma_src, sigma_start, sigma_end,
                              sigma_vec, eps, x_out, batch, n_tok, K, ch, pp, 0, nullptr, (hipStream_t)stream));
  return AFX_OK;
}

int afx_arcflow_step_dropout(const float* x_in, const void* means, const void* logw, const void* logg, int32_t mix_dtype,
                             const float* sigma_vec, const uint8_t* drop_mask, float eps, float* x_out, int32_t batch,
                             int32_t n_tok, int32_t K, int32_t ch, int32_t pp, void* stream) {
  AFX_TRY(arcflow_args("afx_arcflow_step_dropout", x_in && means && logw && logg && x_out && sigma_vec, mix_dtype, batch, n_tok, K, ch, pp));
  HIP_TRY(launch_arcflow_step(x_in, means, logw, logg, mix_dtype == AFX_DT_BF16, 0.f, 0.f, 0.f, sigma_vec, eps, x_out,
                              batch, n_tok, K, ch, pp, 0, drop_mask, (hipStream_t)stream));
  return AFX_OK;
}

int afx_arcflow_velocity(const void* means, const void* logw, const void* logg, int32_t mix_dtype, float sigma_src,
                         float sigma_t, const float* sigma_vec, float* u_out, int32_t batch, int32_t n_tok,
                         int32_t K, int32_t ch, int32_t pp, void* stream) {
  AFX_TRY(arcflow_args("afx_arcflow_velocity", means && logw && logg && u_out, mix_dtype, batch, n_tok, K, ch, pp));
  HIP_TRY(launch_arcflow_step(u_out, means, logw, logg, mix_dtype == AFX_DT_BF16, sigma_src, sigma_t, sigma_t,
                              sigma_vec, 1e-4f, u_out, batch, n_tok, K, ch, pp, 1, nullptr, (hipStream_t)stream));
  return AFX_OK;
}

int afx_arcflow_backward(const float* g, const void* means, const void* logw, const void* logg, int32_t mix_dtype,
                         float sigma_src, float sigma_start, float sigma_end, const float* sigma_vec,
                         const float* gscale_vec, float gscale, float eps, float* d_means, float* d_logw,
                         float* d_logg, int32_t batch, int32_t n_tok, int32_t K, int32_t ch, int32_t pp,
                         int32_t velocity_only, int32_t accumulate, void* stream) {
  if (!g || !means || !logw || !logg || !d_means || !d_logw || !d_logg)
    return fail(AFX_E_INVALID, "null argument to afx_arcflow_backward");
  if (mix_dtype != AFX_DT_BF16 && mix_dtype != AFX_DT_F32) return fail(AFX_E_INVALID, "bad mix_dtype");
  if (batch < 0 || n_tok < 0 || !arcflow_bwd_shape_ok(K, ch, pp))
    return fail(AFX_E_INVALID, "afx_arcflow_backward: need K<=32, ch<=64, pp a power of two dividing ch");
  HIP_TRY(launch_arcflow_bwd(g, means, logw, logg, mix_dtype == AFX_DT_BF16, sigma_src, sigma_start, sigma_end, sigma_vec,
                             gscale_vec, gscale, eps, d_means, d_logw, d_logg, batch, n_tok, K, ch, pp, velocity_only,
                             accumulate, (hipStream_t)stream));
  return AFX_OK;
}

}  // extern "C"
