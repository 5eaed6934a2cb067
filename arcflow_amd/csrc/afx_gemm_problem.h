// The one way host code writes a dense GemmProblem (afx_kernels.h): the operand core, then the field groups a caller needs.  What is not set
// stays zero / null, the launcher's "off".
#pragma once
#include "afx_kernels.h"

namespace afx {

// C [M, N] = A [M, K] . W [N, K]^T + bias
inline GemmProblem dense_problem(const void* A, int64_t lda, const void* W, int64_t ldw, const void* bias, void* C, int64_t ldc, int M, int N, int K) {
  GemmProblem p{};
  p.A = (const uint16_t*)A; p.lda = lda; p.W = (const uint16_t*)W; p.ldw = ldw; p.bias = (const uint16_t*)bias;
  p.C = (uint16_t*)C; p.ldc = ldc; p.M = M; p.N = N; p.K = K;
  return p;
}

// the epilogue: GELU from column gelu_col0 on, or res + gate[row / rows_per_batch] * (.) (gate == nullptr: a unit gate)
inline void set_epilogue(GemmProblem& p, int epi, int gelu_col0, const float* gate, int64_t ldg, int rows_per_batch, const void* res, int64_t ldr) {
  p.epi = epi; p.gelu_col0 = gelu_col0;
  p.gate = gate; p.ldg = ldg; p.rows_per_batch = rows_per_batch; p.res = (const uint16_t*)res; p.ldr = ldr;
}

// e4m3 operands: one scale per row of A and per row of W, and (a_mx != nullptr) one E8M0 byte per row and 128 columns of A
inline void set_fp8(GemmProblem& p, const float* a_scale, const float* w_scale, const void* a_mx = nullptr, int64_t ld_mx = 0) {
  p.fp8 = 1; p.a_scale = a_scale; p.w_scale = w_scale; p.a_mx = (const uint8_t*)a_mx; p.ld_mx = ld_mx;
}

inline hipError_t launch_single(const GemmProblem& p, hipStream_t stream) {
  GemmBatch gb{};
  gb.nprob = 1;
  gb.p[0] = p;
  return launch_gemm(gb, stream);
}

}  // namespace afx
