// C-ABI entry points of the stand-alone operators (see include/arcflow_hip.h for the contract): argument checks, then one launcher of afx_kernels.h.
// None of them takes an afx_ctx; the MMDiT engine is afx_engine.hip.  No kernel lives here.
#include "afx_api_util.h"
#include "afx_gemm_problem.h"

using namespace afx;

namespace {

// What every afx_linear_* entry asks of its arguments, each with its own numbers (in elements): the operands present, M, N >= 0, K a positive
// multiple of k_multiple, N % 8 == 0, lda and ldw multiples of lda_multiple, ldc of ldc_multiple
int check_linear_args(const char* fn, bool operands, int M, int N, int K, int64_t lda, int64_t ldw, int64_t ldc, int k_multiple, int lda_multiple,
                      int ldc_multiple) {
  if (!operands) return fail(AFX_E_INVALID, "null argument to %s", fn);
  if (M < 0 || N < 0 || K <= 0 || K % k_multiple || N % 8 || lda % lda_multiple || ldw % lda_multiple || ldc % ldc_multiple)
    return fail(AFX_E_INVALID, "%s: need K%%%d==0, N%%8==0, lda/ldw%%%d==0, ldc%%%d==0", fn, k_multiple, lda_multiple, ldc_multiple);
  return AFX_OK;
}

// ... and of the epilogue group of the entries that expose it
int check_epilogue_args(const char* fn, int epi, const float* gate, int rows_per_batch, const void* res, int64_t ldr) {
  if (epi < 0 || epi > 2) return fail(AFX_E_INVALID, "%s: bad epilogue", fn);
  if (epi == EPI_GATE_RES && (!res || ldr % 8 || (gate && rows_per_batch < 1)))
    return fail(AFX_E_INVALID, "%s: gated residual epilogue needs res with ldr%%8==0 (and rows_per_batch with a gate)", fn);
  return AFX_OK;
}

int linear_bf16(const char* fn, const void* A, int64_t lda, const void* W, int64_t ldw, const void* bias, void* C, int64_t ldc, int32_t M, int32_t N,
                int32_t K, int32_t epi, int32_t gelu_col0, const float* gate, int64_t ldg, int32_t rows_per_batch, const void* res, int64_t ldr,
                const void* pre, int64_t ldp, void* stream) {
  AFX_TRY(check_linear_args(fn, A && W && C, M, N, K, lda, ldw, ldc, 64, 8, 8));
  if (pre && ldp % 8) return fail(AFX_E_INVALID, "%s: ldp %% 8 == 0", fn);
  AFX_TRY(check_epilogue_args(fn, epi, gate, rows_per_batch, res, ldr));
  GemmProblem p = dense_problem(A, lda, W, ldw, bias, C, ldc, M, N, K);
  set_epilogue(p, epi, gelu_col0, gate, ldg, rows_per_batch > 0 ? rows_per_batch : 1, res, ldr);
  p.pre = (const uint16_t*)pre; p.ldp = ldp;
  HIP_TRY(launch_single(p, (hipStream_t)stream));
  return AFX_OK;
}

// ws == nullptr: one work-group per tile; need_ws: refuse the shapes whose token loop is split over a workspace instead
int linear_tn_f32out(const char* fn, const void* X, int64_t ldx, const void* Y, int64_t ldy, float* C, int64_t ldc, int32_t M, int32_t N1, int32_t N2,
                     int32_t accumulate, void* ws, bool need_ws, void* stream) {
  if (!X || !Y || !C) return fail(AFX_E_INVALID, "null argument to %s", fn);
  if (M < 0 || N1 < 0 || N2 < 0 || N1 % 8 || N2 % 8 || ldx % 8 || ldy % 8 || ldc % 4 || ldx < N1 || ldy < N2 || ldc < N2)
    return fail(AFX_E_INVALID, "%s: need N1%%8==0, N2%%8==0, ldx/ldy%%8==0, ldc%%4==0, leading dimensions >= the widths", fn);
  if (((uintptr_t)X | (uintptr_t)Y | (uintptr_t)C | (uintptr_t)ws) & 15) return fail(AFX_E_INVALID, "%s: operands must be 16-byte aligned", fn);
  if (need_ws && !ws && gemm_tn_ws_bytes(M, N1, N2) > 0) return fail(AFX_E_INVALID, "%s: this shape needs afx_linear_tn_ws_bytes() of workspace", fn);
  HIP_TRY(launch_gemm_tn_f32((const uint16_t*)X, ldx, (const uint16_t*)Y, ldy, C, ldc, M, N1, N2, accumulate, (hipStream_t)stream, (float*)ws));
  return AFX_OK;
}

// V -> V^T, then the attention forward (lse != nullptr: the row log-sum-exps for the backward are kept)
int attention_fwd(const char* fn, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo, float* lse,
                  void* vt_ws, int32_t batch, int32_t heads, int32_t S, void* stream) {
  if (!q || !k || !v || !o || !vt_ws) return fail(AFX_E_INVALID, "null argument to %s", fn);
  if (batch < 1 || heads < 1 || S < 1 || ldq % 8 || ldk % 8 || ldv % 8 || ldo % 4) return fail(AFX_E_INVALID, "%s: bad attention shape / stride", fn);
  HIP_TRY(launch_v_transpose((const uint16_t*)v, ldv, (uint16_t*)vt_ws, batch, heads, S, (hipStream_t)stream));
  HIP_TRY(launch_attention((const uint16_t*)q, ldq, (const uint16_t*)k, ldk, (const uint16_t*)vt_ws, (uint16_t*)o, ldo, batch, heads, S,
                           (hipStream_t)stream, lse));
  return AFX_OK;
}

// shared argument checks of the two AdaLN entry points
int norm_joint_args(const char* fn, const void* x, int64_t ldx, int64_t ldo, int32_t rows, int32_t D, const float* scale, const float* shift,
                    const float* scale_txt, const float* shift_txt, int64_t ldmod, int32_t S, int32_t n_txt) {
  if (!x || !scale || !shift || (!scale_txt) != (!shift_txt)) return fail(AFX_E_INVALID, "null argument to %s", fn);
  if (rows < 0 || D < 8 || D % 8 || D > 4096 || ldx < D || ldx % 8 || ldo < D || ldo % 8 || ldmod < 0 || ldmod % 4 || S < 1 || n_txt < 0 ||
      n_txt > S || (!scale_txt && n_txt != 0))
    return fail(AFX_E_INVALID, "%s: need D %% 8 == 0, D <= 4096, ldx / ldo >= D and multiples of 8, ldmod %% 4 == 0, 0 <= n_txt <= S "
                "(n_txt 0 without text vectors)", fn);
  if (((uintptr_t)x | (uintptr_t)scale | (uintptr_t)shift | (uintptr_t)scale_txt | (uintptr_t)shift_txt) & 15)
    return fail(AFX_E_INVALID, "%s: operands must be 16-byte aligned", fn);
  return AFX_OK;
}

}  // namespace

extern "C" {

// ---- grouped bf16 GEMM  C = epi(A . W^T + bias) -------------------------------------------
int afx_linear_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, const void* bias, void* C, int64_t ldc,
                    int32_t M, int32_t N, int32_t K, int32_t epi, int32_t gelu_col0, const float* gate,
                    int64_t ldg, int32_t rows_per_batch, const void* res, int64_t ldr, void* stream) {
  return linear_bf16("afx_linear_bf16", A, lda, W, ldw, bias, C, ldc, M, N, K, epi, gelu_col0, gate, ldg, rows_per_batch, res, ldr, nullptr, 0, stream);
}

int afx_linear_bf16_pre(const void* A, int64_t lda, const void* W, int64_t ldw, const void* bias, void* C, int64_t ldc,
                        int32_t M, int32_t N, int32_t K, int32_t epi, int32_t gelu_col0, const float* gate,
                        int64_t ldg, int32_t rows_per_batch, const void* res, int64_t ldr, const void* pre, int64_t ldp,
                        void* stream) {
  return linear_bf16("afx_linear_bf16_pre", A, lda, W, ldw, bias, C, ldc, M, N, K, epi, gelu_col0, gate, ldg, rows_per_batch, res, ldr, pre, ldp, stream);
}

int afx_linear_bf16_f32out(const void* A, int64_t lda, const void* W, int64_t ldw, float* C, int64_t ldc, int32_t M,
                           int32_t N, int32_t K, int32_t accumulate, void* stream) {
  AFX_TRY(check_linear_args("afx_linear_bf16_f32out", A && W && C, M, N, K, lda, ldw, ldc, 64, 8, 4));
  GemmProblem p = dense_problem(A, lda, W, ldw, nullptr, C, ldc, M, N, K);
  p.rows_per_batch = 1; p.out_f32 = accumulate ? 2 : 1;
  HIP_TRY(launch_single(p, (hipStream_t)stream));
  return AFX_OK;
}

int afx_linear_splitk_chunks(int32_t M, int32_t N, int32_t K, int32_t split_k) {
  const int tiles = ((M + 255) / 256) * ((N + 255) / 256), nk = K / 64;
  if (split_k <= 0) {                    // ~2 work-groups per CU (512 in flight), at least 4 K-tiles per chunk
    split_k = (512 + tiles / 2) / tiles;
    if (split_k > nk / 4) split_k = nk / 4;
    if (split_k < 1) split_k = 1;
  }
  split_k = split_k < nk ? split_k : nk;
  const int per = (nk + split_k - 1) / split_k;
  return (nk + per - 1) / per;           // no empty chunk
}

int afx_linear_bf16_splitk(const void* A, int64_t lda, const void* W, int64_t ldw, const void* bias, float* partials, int32_t M,
                           int32_t N, int32_t K, int32_t split_k, void* stream) {
  AFX_TRY(check_linear_args("afx_linear_bf16_splitk", A && W && partials, M, N, K, lda, ldw, N, 64, 8, 8));      // the slabs are dense: ldc = N
  if (split_k < 0) return fail(AFX_E_INVALID, "afx_linear_bf16_splitk: need split_k >= 0");
  GemmProblem p = dense_problem(A, lda, W, ldw, bias, partials, N, M, N, K);
  p.rows_per_batch = 1; p.out_f32 = 3;
  p.split_k = afx_linear_splitk_chunks(M, N, K, split_k);
  p.split_stride = (int64_t)M * N;
  HIP_TRY(launch_single(p, (hipStream_t)stream));
  return AFX_OK;
}

int afx_linear_bf16_dropres(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, int32_t M, int32_t N, int32_t K,
                            const void* res, int64_t ldr, float p, uint32_t seed, int64_t row0, void* stream) {
  AFX_TRY(check_linear_args("afx_linear_bf16_dropres", A && W && C && res, M, N, K, lda, ldw, ldc, 64, 8, 8));
  if (ldr % 8 || !(p >= 0.f && p < 1.f)) return fail(AFX_E_INVALID, "afx_linear_bf16_dropres: need ldr%%8==0, 0 <= p < 1");
  GemmProblem q = dense_problem(A, lda, W, ldw, nullptr, C, ldc, M, N, K);
  set_epilogue(q, EPI_GATE_RES, 0, nullptr, 0, M > 0 ? M : 1, res, ldr);
  const DropConsts dc = drop_consts(p);
  q.drop_on = 1; q.drop_thresh = dc.thresh; q.drop_seed = seed; q.drop_inv_keep = dc.inv_keep; q.drop_row0 = row0;
  HIP_TRY(launch_single(q, (hipStream_t)stream));
  return AFX_OK;
}

int afx_linear_tn_f32out(const void* X, int64_t ldx, const void* Y, int64_t ldy, float* C, int64_t ldc, int32_t M, int32_t N1, int32_t N2,
                         int32_t accumulate, void* stream) {
  return linear_tn_f32out("afx_linear_tn_f32out", X, ldx, Y, ldy, C, ldc, M, N1, N2, accumulate, nullptr, false, stream);
}

int64_t afx_linear_tn_ws_bytes(int32_t M, int32_t N1, int32_t N2) {
  if (M < 0 || N1 < 0 || N2 < 0) return fail(AFX_E_INVALID, "bad shape to afx_linear_tn_ws_bytes");
  return gemm_tn_ws_bytes(M, N1, N2);
}

int afx_linear_tn_f32out_ws(const void* X, int64_t ldx, const void* Y, int64_t ldy, float* C, int64_t ldc, int32_t M, int32_t N1, int32_t N2,
                            int32_t accumulate, void* ws, void* stream) {
  return linear_tn_f32out("afx_linear_tn_f32out_ws", X, ldx, Y, ldy, C, ldc, M, N1, N2, accumulate, ws, true, stream);
}

int afx_gemm_dropres_available(void) { return gemm_dropres_available() ? 1 : 0; }
int afx_gemm_set_mode(int32_t impl, int32_t tile) { gemm_set_mode(impl, tile); return 0; }
int afx_gemm_set_fp8_tile(int32_t tile) { return gemm_set_fp8_tile(tile); }

// ... on OCP e4m3 operands (the quantisation kernels are in afx_text.hip)
int afx_quant_rows_fp8(const void* x, int64_t ldx, void* q, int64_t ldq, float* scale, int32_t rows, int32_t K, void* stream) {
  if (!x || !q || !scale || rows < 1 || K % 8 || ldx % 8 || ldq % 8) return fail(AFX_E_INVALID, "bad argument to afx_quant_rows_fp8");
  HIP_TRY(launch_quant_rows_fp8((const uint16_t*)x, ldx, (uint8_t*)q, ldq, scale, rows, K, (hipStream_t)stream));
  return AFX_OK;
}

int afx_quant_rows_mx8(const void* x, int64_t ldx, void* q, int64_t ldq, void* mx, int64_t ld_mx, int32_t rows, int32_t K, void* stream) {
  if (!x || !q || !mx || rows < 1 || K < 128 || K % 128 || ldx % 8 || ldq % 8 || ld_mx < K / 128)
    return fail(AFX_E_INVALID, "afx_quant_rows_mx8: need K %% 128 == 0, ldx / ldq %% 8 == 0, ld_mx >= K / 128");
  HIP_TRY(launch_quant_rows_mx8((const uint16_t*)x, ldx, (uint8_t*)q, ldq, (uint8_t*)mx, ld_mx, rows, K, (hipStream_t)stream));
  return AFX_OK;
}

int afx_linear_fp8(const void* Aq, int64_t lda, const float* a_scale, const void* Wq, int64_t ldw, const float* w_scale, const void* bias,
                   void* C, int64_t ldc, int32_t M, int32_t N, int32_t K, int32_t epi, int32_t gelu_col0, const float* gate, int64_t ldg,
                   int32_t rows_per_batch, const void* res, int64_t ldr, void* stream) {
  AFX_TRY(check_linear_args("afx_linear_fp8", Aq && Wq && C && a_scale && w_scale, M, N, K, lda, ldw, ldc, 128, 16, 8));
  AFX_TRY(check_epilogue_args("afx_linear_fp8", epi, gate, rows_per_batch, res, ldr));
  GemmProblem p = dense_problem(Aq, lda, Wq, ldw, bias, C, ldc, M, N, K);
  set_epilogue(p, epi, gelu_col0, gate, ldg, rows_per_batch > 0 ? rows_per_batch : 1, res, ldr);
  set_fp8(p, a_scale, w_scale);
  HIP_TRY(launch_single(p, (hipStream_t)stream));
  return AFX_OK;
}

int afx_linear_fp8_mx(const void* Aq, int64_t lda, const void* a_mx, int64_t ld_mx, const float* a_scale, const void* Wq, int64_t ldw,
                      const float* w_scale, const void* bias, void* C, int64_t ldc, int32_t M, int32_t N, int32_t K, int32_t epi,
                      int32_t gelu_col0, const float* gate, int64_t ldg, int32_t rows_per_batch, const void* res, int64_t ldr, void* stream) {
  AFX_TRY(check_linear_args("afx_linear_fp8_mx", Aq && a_mx && Wq && C && a_scale && w_scale, M, N, K, lda, ldw, ldc, 512, 16, 8));
  if (ld_mx % 4 || ld_mx < K / 128) return fail(AFX_E_INVALID, "afx_linear_fp8_mx: need ld_mx%%4==0, ld_mx >= K / 128");
  AFX_TRY(check_epilogue_args("afx_linear_fp8_mx", epi, gate, rows_per_batch, res, ldr));
  if (!gemm_fp8_mx_ok(M, N, K)) return fail(AFX_E_INVALID, "afx_linear_fp8_mx: the block-scaled kernel is switched off (AFX_FP8_V3 / AFX_GEMM_IMPL)");
  GemmProblem p = dense_problem(Aq, lda, Wq, ldw, bias, C, ldc, M, N, K);
  set_epilogue(p, epi, gelu_col0, gate, ldg, rows_per_batch > 0 ? rows_per_batch : 1, res, ldr);
  set_fp8(p, a_scale, w_scale, a_mx, ld_mx);
  HIP_TRY(launch_single(p, (hipStream_t)stream));
  return AFX_OK;
}

int afx_linear_fp8_to_mx8(const void* Aq, int64_t lda, const void* a_mx, int64_t ld_mx, const float* a_scale, const void* Wq, int64_t ldw,
                          const float* w_scale, const void* bias, void* C, int64_t ldc, void* c8, int64_t ldc8, void* c_mx, int64_t ld_cmx,
                          int32_t c8_col0, int32_t M, int32_t N, int32_t K, int32_t gelu, void* stream) {
  AFX_TRY(check_linear_args("afx_linear_fp8_to_mx8", Aq && Wq && c8 && c_mx && a_scale && w_scale && (c8_col0 <= 0 || C), M, N, K, lda, ldw, ldc,
                            128, 16, 8));
  if (K < 256 || ldc8 % 8 || c8_col0 < 0 || c8_col0 % 128 || c8_col0 >= N || ld_cmx < (N - c8_col0 + 127) / 128 ||
      (a_mx && (K % 512 || ld_mx % 4 || ld_mx < K / 128)))
    return fail(AFX_E_INVALID, "afx_linear_fp8_to_mx8: need K >= 256 (K%%512==0 with block-scaled A), c8_col0%%128==0, ldc8%%8==0");
  // (the producer epilogue lives in the one-wave-per-SIMD fp8 kernel: the same switches as the block-scaled consumer; K % 512 only binds with a_mx)
  if (!gemm_fp8_mx_ok(M, N, a_mx ? K : 512)) return fail(AFX_E_INVALID, "afx_linear_fp8_to_mx8: the one-wave-per-SIMD fp8 kernel is switched off");
  GemmProblem p = dense_problem(Aq, lda, Wq, ldw, bias, C, ldc, M, N, K);
  p.epi = gelu ? EPI_GELU : EPI_NONE; p.gelu_col0 = gelu ? c8_col0 : 0; p.rows_per_batch = 1;
  set_fp8(p, a_scale, w_scale, a_mx, ld_mx);
  p.c8 = (uint8_t*)c8; p.ldc8 = ldc8; p.c_mx = (uint8_t*)c_mx; p.ld_cmx = ld_cmx; p.c8_col0 = c8_col0;
  HIP_TRY(launch_single(p, (hipStream_t)stream));
  return AFX_OK;
}

// ---- attention ------------------------------------------------------------------------------
int afx_attn_set_impl(int32_t impl) { attn_set_impl(impl); return 0; }
int afx_attn_bwd_set_impl(int32_t impl) { attn_bwd_set_impl(impl); return 0; }

int64_t afx_attention_ws_bytes(int32_t batch, int32_t heads, int32_t S) {
  if (batch < 1 || heads < 1 || S < 1) return fail(AFX_E_INVALID, "bad attention shape");
  return (int64_t)batch * heads * 128 * attn_spad(S) * 2;
}

int afx_attention_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o,
                       int64_t ldo, void* vt_ws, int32_t batch, int32_t heads, int32_t S, void* stream) {
  return attention_fwd("afx_attention_bf16", q, ldq, k, ldk, v, ldv, o, ldo, nullptr, vt_ws, batch, heads, S, stream);
}

int afx_attention_fwd_lse_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o,
                               int64_t ldo, float* lse, void* vt_ws, int32_t batch, int32_t heads, int32_t S, void* stream) {
  if (!lse) return fail(AFX_E_INVALID, "null argument to afx_attention_fwd_lse_bf16");
  return attention_fwd("afx_attention_fwd_lse_bf16", q, ldq, k, ldk, v, ldv, o, ldo, lse, vt_ws, batch, heads, S, stream);
}

int afx_attention_to_mx8(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o8, int64_t ldo8,
                         void* mx, int64_t ld_mx, void* vt_ws, int32_t batch, int32_t heads, int32_t S, void* stream) {
  if (!q || !k || !v || !o8 || !mx || !vt_ws) return fail(AFX_E_INVALID, "null argument to afx_attention_to_mx8");
  if (batch < 1 || heads < 1 || S < 1 || ldq % 8 || ldk % 8 || ldv % 8 || ldo8 % 8 || ld_mx < heads) return fail(AFX_E_INVALID, "bad attention shape / stride");
  if (!attention_v3_eligible(S)) return fail(AFX_E_INVALID, "afx_attention_to_mx8: S > 64 (the one-wave-per-SIMD kernel's epilogue)");
  HIP_TRY(launch_v_transpose((const uint16_t*)v, ldv, (uint16_t*)vt_ws, batch, heads, S, (hipStream_t)stream));
  const AttnMx8 m{(uint8_t*)o8, ldo8, (uint8_t*)mx, ld_mx};
  bool fused = false;
  HIP_TRY(launch_attention((const uint16_t*)q, ldq, (const uint16_t*)k, ldk, (const uint16_t*)vt_ws, nullptr, 0, batch, heads, S, (hipStream_t)stream,
                           nullptr, &m, &fused));
  if (!fused) return fail(AFX_E_INVALID, "afx_attention_to_mx8: the one-wave-per-SIMD attention kernel is switched off (AFX_ATTN_IMPL)");
  return AFX_OK;
}

int64_t afx_attention_ext_ws_bytes(int32_t B, int32_t Hkv, int32_t S, int32_t head_dim) {
  return (int64_t)B * Hkv * head_dim * attn_spad(S) * 2;
}

int afx_attention_ext_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo,
                           void* ws, int32_t B, int32_t H, int32_t Hkv, int32_t S, int32_t head_dim, float scale, int32_t causal,
                           const float* bias, void* stream) {
  if (!q || !k || !v || !o || !ws || B < 1 || S < 1 || H < 1 || Hkv < 1 || H % Hkv || (head_dim != 64 && head_dim != 128) ||
      ldq % 8 || ldk % 8 || ldv % 8 || ldo % 8 || !(scale > 0.f))
    return fail(AFX_E_INVALID, "afx_attention_ext_bf16: head_dim 64 or 128, H %% Hkv == 0, strides %% 8 == 0, scale > 0");
  HIP_TRY(launch_attention_ext((const uint16_t*)q, ldq, (const uint16_t*)k, ldk, (const uint16_t*)v, ldv, (uint16_t*)ws, (uint16_t*)o,
                               ldo, B, H, Hkv, S, head_dim, scale, causal, bias, (hipStream_t)stream));
  return AFX_OK;
}

int64_t afx_attention_bwd_ws_bytes(int32_t batch, int32_t heads, int32_t S) {
  if (batch < 1 || heads < 1 || S < 1) return fail(AFX_E_INVALID, "bad attention shape");
  return attn_bwd_ws_bytes(batch, heads, S);
}

int afx_attention_bwd_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o,
                           int64_t ldo, const void* dout, int64_t lddo, const float* lse, void* dq, int64_t lddq, void* dk,
                           int64_t lddk, void* dv, int64_t lddv, void* ws, int32_t batch, int32_t heads, int32_t S,
                           void* stream) {
  if (!q || !k || !v || !o || !dout || !lse || !dq || !dk || !dv || !ws) return fail(AFX_E_INVALID, "null argument to afx_attention_bwd_bf16");
  if (batch < 1 || heads < 1 || S < 1 || ldq % 8 || ldk % 8 || ldv % 8 || ldo % 8 || lddo % 8 || lddq % 4 || lddk % 4 || lddv % 4)
    return fail(AFX_E_INVALID, "bad attention backward shape / stride");
  HIP_TRY(launch_attention_backward((const uint16_t*)q, ldq, (const uint16_t*)k, ldk, (const uint16_t*)v, ldv,
                                    (const uint16_t*)o, ldo, (const uint16_t*)dout, lddo, lse, (uint16_t*)dq, lddq,
                                    (uint16_t*)dk, lddk, (uint16_t*)dv, lddv, ws, batch, heads, S, (hipStream_t)stream));
  return AFX_OK;
}

// ---- element-wise / reductions -----------------------------------------------------------------
int afx_norm_modulate_bf16(const void* x, int64_t ldx, void* out, int64_t ldo, int32_t rows, int32_t D,
                           const float* scale, const float* shift, int64_t ldmod, int32_t rows_per_batch, int32_t rms,
                           void* stream) {
  if (!x || !out || !scale || (!rms && !shift)) return fail(AFX_E_INVALID, "null argument to afx_norm_modulate_bf16");
  if (rows < 0 || D < 8 || D % 8 || D > 4096 || ldx % 8 || ldo % 8) return fail(AFX_E_INVALID, "bad norm shape");
  HIP_TRY(launch_norm_modulate((const uint16_t*)x, ldx, (uint16_t*)out, ldo, rows, D, scale, shift, ldmod,
                               rows_per_batch, rms, (hipStream_t)stream));
  return AFX_OK;
}

int afx_norm_modulate_joint_bf16(const void* x, int64_t ldx, void* out, int64_t ldo, int32_t rows, int32_t D, const float* scale,
                                 const float* shift, const float* scale_txt, const float* shift_txt, int64_t ldmod, int32_t S,
                                 int32_t n_txt, void* stream) {
  AFX_TRY(norm_joint_args("afx_norm_modulate_joint_bf16", x, ldx, ldo, rows, D, scale, shift, scale_txt, shift_txt, ldmod, S, n_txt));
  if (!out || ((uintptr_t)out & 15)) return fail(AFX_E_INVALID, "afx_norm_modulate_joint_bf16: out null or not 16-byte aligned");
  HIP_TRY(launch_norm_modulate_joint((const uint16_t*)x, ldx, (uint16_t*)out, ldo, rows, D, scale, shift, scale_txt, shift_txt, ldmod, S, n_txt,
                                     (hipStream_t)stream));
  return AFX_OK;
}

int afx_norm_modulate_mx8(const void* x, int64_t ldx, void* q8, int64_t ldq, void* mx, int64_t ld_mx, float* rowscale, int32_t rows, int32_t D,
                          const float* scale, const float* shift, const float* scale_txt, const float* shift_txt, int64_t ldmod, int32_t S,
                          int32_t n_txt, int32_t* fused, void* stream) {
  AFX_TRY(norm_joint_args("afx_norm_modulate_mx8", x, ldx, ldq, rows, D, scale, shift, scale_txt, shift_txt, ldmod, S, n_txt));
  if (!q8 || !fused || ((uintptr_t)q8 & 7) || (!rowscale && (!mx || ld_mx < (D + 127) / 128 || ld_mx % 4)) || ((uintptr_t)rowscale & 3))
    return fail(AFX_E_INVALID, "afx_norm_modulate_mx8: need q8 (8-byte aligned), fused, and rowscale or mx with ld_mx >= D / 128, ld_mx %% 4 == 0");
  bool f = false;
  HIP_TRY(launch_norm_modulate_mx8((const uint16_t*)x, ldx, (uint8_t*)q8, ldq, (uint8_t*)mx, ld_mx, rows, D, scale, shift, scale_txt, shift_txt,
                                   ldmod, S, n_txt, (hipStream_t)stream, &f, rowscale));
  *fused = f ? 1 : 0;
  return AFX_OK;
}

int afx_qk_norm_rope_bf16(void* x, int64_t ldx, const float* w_txt, const float* w_img, const float* rope_cos,
                          const float* rope_sin, int32_t batch, int32_t S, int32_t n_txt, int32_t heads, void* stream) {
  if (!x || !w_txt || !w_img || !rope_cos || !rope_sin) return fail(AFX_E_INVALID, "null argument to afx_qk_norm_rope_bf16");
  if (batch < 1 || S < 1 || heads < 1 || ldx % 8) return fail(AFX_E_INVALID, "bad qk_norm_rope shape");
  HIP_TRY(launch_qk_norm_rope((uint16_t*)x, ldx, w_txt, w_img, rope_cos, rope_sin, batch, S, n_txt, heads,
                              (hipStream_t)stream));
  return AFX_OK;
}

int afx_gemv_bf16(const float* x, const void* W, const void* bias, float* y, int32_t B, int32_t N, int32_t K,
                  int32_t act, int32_t accumulate, void* stream) {
  if (!x || !W || !y) return fail(AFX_E_INVALID, "null argument to afx_gemv_bf16");
  if (B < 1 || B > 8 || N < 1 || K < 8 || K % 8) return fail(AFX_E_INVALID, "bad gemv shape (B<=8, K%%8==0)");
  HIP_TRY(launch_gemv(x, (const uint16_t*)W, (const uint16_t*)bias, y, B, N, K, act, accumulate, (hipStream_t)stream));
  return AFX_OK;
}

}  // extern "C"
