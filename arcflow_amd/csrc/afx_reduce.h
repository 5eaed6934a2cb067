// The bit-reproducible fp64 reduction of the per-sample passes (afx_sampler.hip: the orthogonal-guidance coefficient; afx_score.hip: the
// agreement sums and SSIM of training-time evaluation).  A fixed number of work-groups per sample, one workspace slot of K doubles per
// work-group, the four waves of a work-group added in wave order, the slots added in index order by a second launch: no atomics, and a
// result that does not depend on which work-group or wave finished first.
#pragma once
#include <algorithm>

#include "afx_common.h"

namespace afx {

AFX_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The tail of a 256-lane work-group: slot[k] = the sum of acc[k] over the work-group, each wave by the shuffle tree, then
// ((wave 0 + wave 1) + wave 2) + wave 3.  Every lane must call it (it holds a barrier); 32 K bytes of LDS.
template <int K>
AFX_DEV void block_slot_sums(const double (&acc)[K], double* slot) {
  __shared__ double red[4][K];
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double v = wave_sum_f64(acc[k]);
    if ((threadIdx.x & 63) == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const int k = threadIdx.x;
    slot[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

// sum k of sample s: its `parts` slots added in index order
template <int K>
AFX_DEV double ordered_slot_sum(const double* __restrict__ ws, int s, int parts, int k) {
  double v = 0.0;
  for (int w = 0; w < parts; ++w) v += ws[((int64_t)s * parts + w) * K + k];
  return v;
}

// one lane per (sample, sum): out[s][k] = ordered_slot_sum
template <int K>
__global__ __launch_bounds__(64) void ordered_finish_kernel(const double* __restrict__ ws, double* __restrict__ out, int batch, int parts) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= batch * K) return;
  out[i] = ordered_slot_sum<K>(ws, i / K, parts, i % K);
}

// work-groups (= workspace slots) per sample of a reduction over n elements: one per 8192 elements, at most 64 -- a function of n alone,
// so that the partition, and with it every rounding of the sum, is the same on every run and for every batch size
static inline int reduce_parts(int64_t n) { return (int)std::min<int64_t>(64, std::max<int64_t>(1, (n + 8191) / 8192)); }

}  // namespace afx
