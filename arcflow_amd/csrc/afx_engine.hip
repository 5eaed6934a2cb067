// The MMDiT forward engine behind the afx_ctx entry points (see include/arcflow_hip.h for the contract), and the library's error state.  The
// stand-alone operators' entry points are in afx_ops_api.hip.
//
// The forward is a fixed launch plan over the kernels in afx_gemm / afx_attn / afx_elementwise:
//   temb MLPs (gemv) -> ONE gemv over all stacked AdaLN modulation linears -> embedders (grouped GEMM)
//   -> per block { LN+modulate, k|v|q projection with the q / k / V^T preparation (below),
//                  flash attention (O overwrites Q), out-proj GEMM with fused gate*x+residual,
//                  LN+modulate, MLP-up GEMM + GELU, MLP-down GEMM with fused gate*x+residual }
//   -> norm_out + head GEMM -> log_softmax split.
// The preparation is one of three paths, picked per shape by qkv_path(): AFX_QKV_VT_PROJ (q / k RMSNorm + RoPE in the projection's epilogue, V^T
// computed by the projection itself: no launch in between), AFX_QKV_QK_EPI (that epilogue, then a V transpose launch) or AFX_QKV_KV_PREP (the plain
// projection, then one launch for RMSNorm + RoPE in place and the V transpose).  The steps are fwd_conditioning ... fwd_head below.
// Activations live in the caller-provided workspace in the joint [B][text;image] token layout, so the
// FLUX single-stream blocks run on the same buffers without a concat, and attention / proj_out read
// the [O | mlp] operand in place (lda-strided) from the fused QKV+MLP buffer.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "afx_api_util.h"
#include "afx_gemm_problem.h"

using namespace afx;

thread_local char afx_g_err[512] = "";

int afx_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(afx_g_err, sizeof(afx_g_err), fmt, ap);
  va_end(ap);
  return code;
}

namespace {

struct Weight {
  const void* ptr = nullptr;
  int dtype = 0;
  std::vector<int64_t> shape;
};

inline int64_t align256(int64_t x) { return (x + 255) / 256 * 256; }

}  // namespace

// Weight pointers of one linear / one block, resolved once in afx_finalize (the launch plan does no string work)
struct LinW {
  const uint16_t* w = nullptr;    // bf16 [out, in]
  const uint16_t* b = nullptr;    // bf16 [out]
  const void* wq = nullptr;       // fp8 mode: e4m3 [out, in]
  const float* wscale = nullptr;  //           per-output-channel scale [out]
};
struct DoubleW { LinW qkv[2], out[2], mlp1[2], mlp2[2]; const float* qkn = nullptr; };   // [0] image stream, [1] text stream
struct SingleW { LinW fused, out; const float* qkn = nullptr; };
// ... and of everything around the blocks: the conditioning MLPs (timestep, guidance, pooled text), the stacked modulation linear, a separately
// bound norm_out.linear (mod_final: optional, w stays null), the embedders, Qwen's text RMSNorm weight (f32 [joint_dim]) and the head
struct OuterW { LinW t1, t2, g1, g2, p1, p2, mod, mod_final, x_in, ctx_in, head; const float* txt_norm = nullptr; };

struct afx_ctx {
  afx_model_desc d;
  std::unordered_map<std::string, Weight> w;
  bool finalized = false;
  std::vector<DoubleW> dbl;
  std::vector<SingleW> sgl;
  OuterW ow;
  char* ws = nullptr;
  int64_t ws_bytes = 0;
  int D = 0;
  int64_t n_mod = 0;       // rows of the stacked modulation linear
  int head_n = 0;          // padded head width
  uint16_t* ckpt = nullptr;   // optional [num_blocks][B*S, D] block-input checkpoints (gradient checkpointing)
  bool fp8 = false;            // block linears on the fp8 MFMA (afx_set_fp8_linear)
  int fp8_mx = -1;             // fp8: block-scaled activations, quantisation in the producers' epilogues (AFX_FP8_MX=0: one scale per row + a pass per GEMM)
  const float* temb_override = nullptr;   // optional [B, D] f32 replacing timestep_embedder(t) (training student with its LoRA pair)
  // conditioning of several denoising steps prepared in one pass over the stacked modulation matrix (afx_mmdit_prepare_steps)
  int prep_steps = 0, prep_B = 0, prep_use = -1;
  // optional per-launch-class timing (HIP events on the forward's stream)
  bool prof_on = false;
  int prof_stride = 1;          // time one launch in prof_stride (afx_profile_enable(ctx, N)): an event pair on a dispatch costs ~4 us
  uint64_t prof_count = 0;
  struct ProfRec { hipEvent_t a, b; int klass; double flops; };
  std::vector<ProfRec> prof_pool;
  size_t prof_used = 0;
};

namespace {

template <class T>
const T* wptr(const afx_ctx* c, const std::string& n) {
  auto it = c->w.find(n);
  return it == c->w.end() ? nullptr : (const T*)it->second.ptr;
}

int need(const afx_ctx* c, const std::string& n, int dtype, std::vector<int64_t> shape) {
  auto it = c->w.find(n);
  if (it == c->w.end()) return fail(AFX_E_MISSING, "weight '%s' is not bound", n.c_str());
  if (it->second.dtype != dtype) return fail(AFX_E_INVALID, "weight '%s': wrong dtype", n.c_str());
  if (it->second.shape != shape) {
    std::string got, want;
    for (auto v : it->second.shape) got += std::to_string(v) + ",";
    for (auto v : shape) want += std::to_string(v) + ",";
    return fail(AFX_E_INVALID, "weight '%s': shape [%s] expected [%s]", n.c_str(), got.c_str(), want.c_str());
  }
  return AFX_OK;
}

int need_linear(const afx_ctx* c, const std::string& n, int64_t out_f, int64_t in_f) {
  int r = need(c, n + ".weight", AFX_DT_BF16, {out_f, in_f});
  if (r) return r;
  return need(c, n + ".bias", AFX_DT_BF16, {out_f});
}

// modulation vector offsets inside one row of the stacked modulation output
struct ModLayout {
  int64_t D;
  int nd, ns;
  int64_t dbl(int i, int stream /*0 img, 1 txt*/, int chunk /*0..5*/) const {
    return ((int64_t)i * 12 + stream * 6 + chunk) * D;
  }
  int64_t sgl(int i, int chunk /*0..2*/) const { return (int64_t)nd * 12 * D + ((int64_t)i * 3 + chunk) * D; }
  int64_t fin(int chunk /*0 scale, 1 shift*/) const { return (int64_t)nd * 12 * D + (int64_t)ns * 3 * D + chunk * D; }
  int64_t total() const { return (int64_t)nd * 12 * D + (int64_t)ns * 3 * D + 2 * D; }
};

constexpr int AFX_PREP_ROWS = 8;      // (steps x samples) one modulation pass can serve: the GEMV's batch limit

struct Workspace {
  uint16_t *X, *Xn, *F, *Vt, *head;
  float *sincos, *tmp, *temb, *semb, *mod, *pooled;
  float *prep_temb, *prep_semb, *prep_mod;   // [AFX_PREP_ROWS][D], [..][D], [..][n_mod]: prepared steps (step-major, then sample)
  uint8_t* q8;     // fp8 mode: the quantised A operand of the GEMM about to run [R, <= 5D]
  uint8_t* q8n;    // fp8, block-scaled: the D-wide operands (LayerNorm outputs, the double blocks' attention output) [R, D] -- q8 then holds the
                   // wide ones, written by the producing GEMM's epilogue while that GEMM still reads q8n
  uint8_t* mxn;    // [R, ld_mxn] / [R, ld_mxw] E8M0 scale bytes of q8n / q8
  uint8_t* mxw;
  float* ones;     // [R] 1.0f: a_scale of the block-scaled launches
  int64_t ld_mxn, ld_mxw;
  float* qs;       //           its per-row scales [R]
  int64_t total;
};

Workspace carve(const afx_ctx* c, char* base, int B, int N, int T) {
  const int64_t D = c->D, S = (int64_t)N + T, R = (int64_t)B * S;
  Workspace w;
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align256(bytes);
    return p;
  };
  w.prep_temb = (float*)take((int64_t)AFX_PREP_ROWS * D * 4);       // FIRST (shape-independent offsets: they outlive a forward)
  w.prep_semb = (float*)take((int64_t)AFX_PREP_ROWS * D * 4);
  w.prep_mod = (float*)take((int64_t)AFX_PREP_ROWS * c->n_mod * 4);
  w.X = (uint16_t*)take(R * D * 2);
  w.Xn = (uint16_t*)take(R * D * 2);
  w.F = (uint16_t*)take(R * 7 * D * 2);   // single: fused [k|v|q|mlp]; double: [QKV 3D] then [H 4D]
  w.Vt = (uint16_t*)take((int64_t)B * c->d.heads * 128 * attn_spad((int)S) * 2);
  w.head = (uint16_t*)take((int64_t)B * N * c->head_n * 2);
  w.sincos = (float*)take((int64_t)B * 256 * 4);
  w.tmp = (float*)take((int64_t)B * D * 4);
  w.temb = (float*)take((int64_t)B * D * 4);
  w.semb = (float*)take((int64_t)B * D * 4);
  w.pooled = (float*)take((int64_t)B * (c->d.pooled_dim > 0 ? c->d.pooled_dim : 8) * 4);
  w.mod = (float*)take((int64_t)B * c->n_mod * 4);
  w.q8 = nullptr;
  w.qs = nullptr;
  w.q8n = w.mxn = w.mxw = nullptr;
  w.ones = nullptr;
  w.ld_mxn = (D / 128 + 3) / 4 * 4;
  w.ld_mxw = (5 * D / 128 + 3) / 4 * 4;
  if (c->fp8) {
    w.q8 = (uint8_t*)take(R * 5 * D);
    w.qs = (float*)take(R * 4);
    w.q8n = (uint8_t*)take(R * D);
    w.mxn = (uint8_t*)take(R * w.ld_mxn);
    w.mxw = (uint8_t*)take(R * w.ld_mxw);
    w.ones = (float*)take(R * 4);
  }
  w.total = off;
  return w;
}

// Scoped timer of ONE launch when profiling is enabled: hands an event pair to the launcher, which attaches it to the kernel
// dispatch itself (hipExtLaunchKernelGGL: kernel begin / end timestamps, no extra queue packets).
struct ProfScope {
  afx_ctx* c; hipStream_t st; afx_ctx::ProfRec* r = nullptr;
  ProfScope(afx_ctx* c_, hipStream_t st_, int klass, double flops) : c(c_), st(st_) {
    if (!c->prof_on) return;
    if ((c->prof_count++ % (uint64_t)c->prof_stride) != 0) return;      // sampled: the forward has an odd number of launches, so the sample walks every launch position
    if (c->prof_used == c->prof_pool.size()) {
      afx_ctx::ProfRec n{};
      if (hipEventCreate(&n.a) != hipSuccess || hipEventCreate(&n.b) != hipSuccess) return;
      c->prof_pool.push_back(n);
    }
    r = &c->prof_pool[c->prof_used++];
    r->klass = klass; r->flops = flops;
    launch_timer().start = r->a;
    launch_timer().stop = r->b;
  }
  ~ProfScope() { launch_timer() = LaunchTimer{}; }
};

double gemm_flops(const GemmBatch& gb) {
  double f = 0;
  for (int i = 0; i < gb.nprob; ++i) f += 2.0 * gb.p[i].M * (double)gb.p[i].N * gb.p[i].K;
  return f;
}

// ---- the attention operands of one block: the k|v|q(|mlp) projection and the q / k / V^T preparation -----------------------------
// Three ways (AFX_QKV_* in arcflow_hip.h), picked per shape by qkv_path():
//   VT_PROJ  V^T straight out of the projection: k and q as problems of their own with the q / k epilogue (GemmProblem::qk_D), the V third
//            computed transposed (A = the V rows of the weight, W = the tokens; w_perm16 / bias_rows) into Vt at the rows' key offset.  Needs
//            16-key groups that do not straddle the text / image boundary and no key padding (T % 16 == 0, S % 64 == 0);
//   QK_EPI   RMSNorm + RoPE of q / k in the epilogue of the whole projection, then launch_v_transpose;
//   KV_PREP  the plain projection, then launch_kv_prep (norm, RoPE and transpose of the bf16-rounded projection in one launch).
// The forward and afx_qkv_operands build their launches with the functions below.
struct BlockShape {
  int64_t D;
  int H, B, N, T, S, S_pad;                    // S = N + T joint rows per sample: [text T | image N]
  const float* rope_cos;                       // [S, 64] f32 tables of the joint positions
  const float* rope_sin;
  uint16_t* Vt;                                // [B][H][128][S_pad] key-permuted V^T (afx_attn.hip key_of_pos)
};

BlockShape block_shape(int H, int B, int N, int T, const float* rope_cos, const float* rope_sin, uint16_t* Vt) {
  BlockShape q;
  q.D = (int64_t)H * 128; q.H = H; q.B = B; q.N = N; q.T = T; q.S = N + T; q.S_pad = (int)attn_spad(N + T);
  q.rope_cos = rope_cos; q.rope_sin = rope_sin; q.Vt = Vt;
  return q;
}

bool vt_proj_shape_ok(const BlockShape& q, bool single) {
  return q.T % 16 == 0 && q.S % 64 == 0 && (!single || q.B + 3 <= GEMM_MAX_PROBLEMS);
}

// the forward's choice (fp8: the block linears run on the fp8 MFMA; qk_fuse_fp8: its q / k epilogue is switched on)
int qkv_path(const BlockShape& q, bool single, bool fp8, bool qk_fuse_fp8) {
  const bool qk_fuse = gemm_qk_fusion_available() && (!fp8 || qk_fuse_fp8);
  const bool vt_fuse = qk_fuse && !fp8 && getenv("AFX_VT_FUSE_OFF") == nullptr && vt_proj_shape_ok(q, single);
  return vt_fuse ? AFX_QKV_VT_PROJ : qk_fuse ? AFX_QKV_QK_EPI : AFX_QKV_KV_PREP;
}

// q / k RMSNorm + RoPE in the epilogue of problem p: its row r sits at joint position (row0 + r) % period
void set_qk_epilogue(GemmProblem& p, const BlockShape& q, const float* wq, const float* wk, int row0, int period) {
  p.qk_D = (int)q.D; p.qk_wq = wq; p.qk_wk = wk;
  p.rope_cos = q.rope_cos; p.rope_sin = q.rope_sin; p.rope_row0 = row0; p.rope_period = period; p.rope_rows = q.S;
}

// ... of the image (s = 0) or text (s = 1) rows of a double block: qkn = [img_q, img_k, txt_q, txt_k][128]
void stream_qk_epilogue(GemmProblem& p, const BlockShape& q, const float* qkn, int s) {
  set_qk_epilogue(p, q, qkn + (s == 0 ? 0 : 2) * 128, qkn + (s == 0 ? 1 : 3) * 128, s == 0 ? q.T : 0, 1 << 30);
}

// the plain linear C [M, N] = A [M, K] . W^T + bias over the rows of lw from wrow0 on
void linear_problem(GemmProblem& p, const uint16_t* A, int64_t lda, const LinW& lw, int64_t wrow0, uint16_t* C, int64_t ldc, int M, int N, int K) {
  p = dense_problem(A, lda, lw.w + wrow0 * K, K, lw.b ? lw.b + wrow0 : nullptr, C, ldc, M, N, K);
}

// VT_PROJ: the V third of a k|v|q projection computed transposed -- A = the V rows of the weight, W = `keys` token rows -- into Vt at the keys' offset
void vt_problem(GemmProblem& p, const BlockShape& q, const uint16_t* tokens, int64_t ldt, const LinW& lw, uint16_t* Vt, int keys) {
  const int64_t D = q.D;
  p = dense_problem(lw.w + D * D, D, tokens, ldt, lw.b ? lw.b + D : nullptr, Vt, q.S_pad, (int)D, keys, (int)D);
  p.bias_rows = 1; p.w_perm16 = 1;
}

// the image (s = 0) or text (s = 1) rows of sample b in a per-stream linear over the joint token matrix
void stream_problem(GemmProblem& p, const BlockShape& q, const uint16_t* A, int64_t lda, int K, const LinW& lw, uint16_t* C, int64_t ldc,
                    int Nout, int b, int s) {
  const int64_t row0 = (int64_t)b * q.S + (s == 0 ? q.T : 0);
  linear_problem(p, A + row0 * lda, lda, lw, 0, C + row0 * ldc, ldc, s == 0 ? q.N : q.T, Nout, K);
}

// VT_PROJ: the k, q and transposed-v problems of one k|v|q(|mlp) projection over `rows` joint rows starting at joint row `row0g` of sample b
void kqv_problems(GemmBatch& gb, const BlockShape& q, const uint16_t* A, int64_t lda, const LinW& lw, uint16_t* C, int64_t ldc, int64_t row0g,
                  int rows, int b, int pos0, int period, const float* wq, const float* wk, bool with_v) {
  const int64_t D = q.D;
  for (int part = 0; part < 2; ++part) {        // 0: k (weight rows 0..D), 1: q (2D..3D)
    GemmProblem& p = gb.p[gb.nprob++];
    const int64_t wrow = part == 0 ? 0 : 2 * D;
    linear_problem(p, A + row0g * lda, lda, lw, wrow, C + row0g * ldc + wrow, ldc, rows, (int)D, (int)D);
    set_qk_epilogue(p, q, part == 0 ? wk : wq, part == 0 ? wk : wq, pos0, period);     // a problem of its own: its columns are "region 0"
  }
  if (with_v) vt_problem(gb.p[gb.nprob++], q, A + row0g * lda, lda, lw, q.Vt + (int64_t)b * q.H * 128 * q.S_pad + pos0, rows);      // v^T (D..2D)
}

// VT_PROJ, double block: sample b's image k, q, v^T + text k, q, v^T = 6 problems of one launch
void double_vt_batch(GemmBatch& gb, const BlockShape& q, const uint16_t* A, int64_t lda, const LinW (&lw)[2], uint16_t* QKV, int64_t ldq,
                     const float* qkn, int b) {
  for (int s = 0; s < 2; ++s)
    kqv_problems(gb, q, A, lda, lw[s], QKV, ldq, (int64_t)b * q.S + (s == 0 ? q.T : 0), s == 0 ? q.N : q.T, b, s == 0 ? q.T : 0, 1 << 30,
                 qkn + (s == 0 ? 0 : 2) * 128, qkn + (s == 0 ? 1 : 3) * 128, true);
}

// Single block: the fused [k | v | q | mlp] projection over all B S joint rows (position = row % S, qkn = [q, k][128]), mlp columns through
// GELU.  QK_EPI / KV_PREP: one problem (with / without the q / k epilogue); VT_PROJ: k, q, the mlp columns and one transposed v per sample.
void single_qkv_batch(GemmBatch& gb, int path, const BlockShape& q, const uint16_t* A, int64_t lda, const LinW& lw, uint16_t* F, int64_t ldf,
                      const float* qkn) {
  const int64_t D = q.D;
  const int R = q.B * q.S;
  gb.nprob = 1;
  GemmProblem& f = gb.p[0];
  linear_problem(f, A, lda, lw, 0, F, ldf, R, (int)(7 * D), (int)D);
  f.epi = EPI_GELU; f.gelu_col0 = (int)(3 * D);
  if (path == AFX_QKV_VT_PROJ) {
    gb.nprob = 0;
    kqv_problems(gb, q, A, lda, lw, F, ldf, 0, R, 0, 0, q.S, qkn, qkn + 128, false);
    GemmProblem& m = gb.p[gb.nprob++];
    linear_problem(m, A, lda, lw, 3 * D, F + 3 * D, ldf, R, (int)(4 * D), (int)D);
    m.epi = EPI_GELU; m.gelu_col0 = 0;
    for (int b = 0; b < q.B; ++b) vt_problem(gb.p[gb.nprob++], q, A + (int64_t)b * q.S * lda, lda, lw, q.Vt + (int64_t)b * q.H * 128 * q.S_pad, q.S);
  } else if (path == AFX_QKV_QK_EPI) {
    set_qk_epilogue(f, q, qkn, qkn + 128, 0, q.S);
  }
}

// what is left behind the projection [k | v | q ...] (row stride ldf): QK_EPI transposes V, KV_PREP normalises and rotates k and q in place
// (joint rows < T with the text weights) and transposes V
hipError_t qkv_finish(int path, const BlockShape& q, uint16_t* F, int64_t ldf, const float* wk_txt, const float* wk_img, const float* wq_txt,
                      const float* wq_img, hipStream_t st) {
  if (path == AFX_QKV_QK_EPI) return launch_v_transpose(F + q.D, ldf, q.Vt, q.B, q.H, q.S, st);
  if (path == AFX_QKV_KV_PREP)
    return launch_kv_prep(F, F + 2 * q.D, ldf, wk_txt, wk_img, wq_txt, wq_img, q.rope_cos, q.rope_sin, q.T, F + q.D, ldf, q.Vt, q.B, q.H, q.S, st);
  return hipSuccess;
}

// ---- conditioning: temb = t_mlp(sincos(1000 t)) [+ g_mlp(sincos(1000 g))] [+ p_mlp(pooled)] ------
// ... of nsteps x B rows (step-major, then sample; t == nullptr: temb already holds the timestep part), then their SiLU and modulation vectors.
// sc [B, 256] / pf [B, pooled_dim] take the MLPs' inputs, hid [nsteps B, D] their hidden rows (may be semb: overwritten by the SiLU).
struct CondBufs { float *sc, *pf, *hid, *temb, *semb, *mod; };
int conditioning(const afx_ctx* c, const float* t, int nsteps, const float* g, const void* pooled, int B, const CondBufs& o, hipStream_t st) {
  const afx_model_desc& d = c->d;
  const OuterW& w = c->ow;
  const int D = c->D, rows = B * nsteps;
  for (int k = 0; k < nsteps; ++k) {
    float *hid = o.hid + (int64_t)k * B * D, *temb = o.temb + (int64_t)k * B * D;
    if (t != nullptr) {
      HIP_TRY(launch_sincos(t + (int64_t)k * B, 1000.0f, o.sc, B, d.family == 0 ? 1 : 2, st));
      HIP_TRY(launch_gemv(o.sc, w.t1.w, w.t1.b, hid, B, D, 256, 1, 0, st));
      HIP_TRY(launch_gemv(hid, w.t2.w, w.t2.b, temb, B, D, D, 0, 0, st));
    }
    if (d.guidance_embeds) {
      HIP_TRY(launch_sincos(g, 1000.0f, o.sc, B, 1, st));
      HIP_TRY(launch_gemv(o.sc, w.g1.w, w.g1.b, hid, B, D, 256, 1, 0, st));
      HIP_TRY(launch_gemv(hid, w.g2.w, w.g2.b, temb, B, D, D, 0, 1, st));
    }
    if (d.pooled_dim > 0) {
      HIP_TRY(launch_bf16_to_f32((const uint16_t*)pooled, o.pf, (int64_t)B * d.pooled_dim, st));
      HIP_TRY(launch_gemv(o.pf, w.p1.w, w.p1.b, hid, B, D, d.pooled_dim, 1, 0, st));
      HIP_TRY(launch_gemv(hid, w.p2.w, w.p2.b, temb, B, D, D, 0, 1, st));
    }
  }
  HIP_TRY(launch_silu(o.temb, o.semb, (int64_t)rows * D, st));
  // Every AdaLN modulation vector of the whole network in one weight-streaming pass over the stacked [n_mod, D] matrix
  // (6.5 GB for FLUX: 1.3 ms of pure HBM streaming), on the forward's stream.  (Measured and dropped, r02c: the rows of all but the first blocks
  // on a side stream under the embedders' and first blocks' MFMA work, 140.2 vs 139.5 ms per image -- the GEMMs lose more to the shared HBM / issue
  // slots than the 1.3 ms the stream hides.)
  HIP_TRY(launch_gemv(o.semb, w.mod.w, w.mod.b, o.mod, rows, (int)c->n_mod, D, 0, 0, st, c->n_mod));
  // a separately bound norm_out.linear (the distillation student trains its own copy while the teacher keeps the
  // frozen one inside the stacked matrix: lakonlab/configs/flux/arcflux_2nfe_k16.py:20-25 freeze_exclude 'norm_out')
  if (w.mod_final.w != nullptr)
    HIP_TRY(launch_gemv(o.semb, w.mod_final.w, w.mod_final.b, o.mod + ModLayout{D, d.num_double, d.num_single}.fin(0), rows, 2 * D, D, 0, 0, st, c->n_mod));
  return AFX_OK;
}

// ---- the forward of one micro-batch: one state, named steps ----------------------------------------
// The fp8 switches, resolved once per call (fwd_resolve_fp8).  mx: block-scaled activations; norm_rows: ... except the operands the LayerNorm kernel writes, one scale per row; attn_mx: the
// attention epilogue writes the out-projection's operand; qk_fuse_fp8: the fp8 kernel's q / k epilogue is switched on
struct Fp8Mode { bool mx = false, norm_rows = false, attn_mx = false, qk_fuse_fp8 = false; };
// where the A operand of an fp8 block GEMM is when its launch is built
enum class ASrc {
  Bf16,   // bf16 in memory: a pass in front of the GEMM quantises it
  Wide,   // the wide operand a GEMM epilogue left in q8 / mxw (mlp hidden; the single blocks' [O | mlp], O added by the attention kernel or a pass)
  Norm,   // the LayerNorm kernel left it in q8n, with one scale per row in qs or (AFX_FP8_NORM_MX) block scales in mxn
  Attn,   // the attention kernel of a double block left it in q8n / mxn
};
struct Fwd {
  afx_ctx* c; Workspace ws; hipStream_t st; BlockShape bs; ModLayout ml; int64_t ldm, D, R;
  Fp8Mode fp8; int dpath, spath;          // dpath / spath: how the double / single blocks prepare their attention operands (AFX_QKV_*)
};

int fwd_gemm(Fwd& f, GemmBatch& gb) {
  ProfScope ps_(f.c, f.st, 0, gemm_flops(gb));
  HIP_TRY(launch_gemm(gb, f.st));
  return AFX_OK;
}

int fwd_resolve_fp8(Fwd& f) {
  afx_ctx* c = f.c;
  Fp8Mode& m = f.fp8;
  // fp8 with block-scaled activations: every block GEMM reads e4m3 rows + one E8M0 byte per row and 128 columns.  The D-wide
  // operands are quantised into q8n / mxn (by the pass below until their producers write them), the wide ones (mlp hidden, [O | mlp]) leave
  // the producing GEMM's epilogue in q8 / mxw.
  if (c->fp8 && c->fp8_mx < 0) {          // latched per context on the first fp8 forward; the other switches are read on every call
    const char* e = getenv("AFX_FP8_MX");
    c->fp8_mx = (e && e[0] == '0') ? 0 : 1;
  }
  m.mx = c->fp8 && c->fp8_mx == 1 && f.D % 512 == 0 && gemm_fp8_mx_ok(f.R, (int)f.D, (int)f.D);
  if (m.mx) HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)f.ws.ones, 0x3f800000, (size_t)f.R, f.st));
  // The fused q / k epilogue also exists on the one-wave-per-SIMD fp8 kernel (epi_store_qk<MI, true>; V is then transposed by its own launch), opt-in:
  // measured level with the separate preparation launch (11.30 vs 11.30 images/s) -- with 256 accumulators in the file the fp8 variant of that epilogue
  // has to re-read the weight scales per row tile, which costs what the saved launch gave (AFX_FP8_QK_FUSE=1).
  // LayerNorm-produced operands (a row sits in one wave there) carry ONE scale per row and run on the plain fp8 MFMA; only the operands written by
  // GEMM / attention epilogues need block scales (AFX_FP8_NORM_MX=1: block scales everywhere, A/B)
  m.norm_rows = m.mx && getenv("AFX_FP8_NORM_MX") == nullptr;
  m.attn_mx = m.mx && f.bs.H * 128 == f.D && getenv("AFX_FP8_ATTN_MX_OFF") == nullptr;      // the attention epilogue as the last producer of the format
  const char* qkf8 = getenv("AFX_FP8_QK_FUSE");
  m.qk_fuse_fp8 = m.mx && qkf8 != nullptr && qkf8[0] == '1';
  // how each block prepares its attention operands (see qkv_path): q / k RMSNorm + RoPE in the epilogue of the k|v|q projections when
  // the GEMM kernel in use offers it (not in fp8 mode unless AFX_FP8_QK_FUSE), and V^T straight out of the projection where the shape
  // allows: then no preparation launch is left between the projection and the attention
  f.dpath = qkv_path(f.bs, false, c->fp8, m.qk_fuse_fp8);
  f.spath = qkv_path(f.bs, true, c->fp8, m.qk_fuse_fp8);
  return AFX_OK;
}

// The fp8 operand side of problem p (bf16 mode: nothing): its M rows are the rows from row0 on of the K-wide operand `src`, its weight is lw
void bind_fp8_operand(GemmProblem& p, const Fwd& f, ASrc src, int64_t row0, int K, const LinW& lw) {
  const Workspace& ws = f.ws;
  if (!f.c->fp8) return;
  p.W = (const uint16_t*)lw.wq; p.lda = K;
  if (!f.fp8.mx) {                                     // per-token scales: the pass in front of every GEMM wrote q8 / qs
    p.A = (const uint16_t*)(ws.q8 + row0 * K); set_fp8(p, ws.qs + row0, lw.wscale);
  } else if (src == ASrc::Norm && f.fp8.norm_rows) {   // LayerNorm rows: one scale per row, the plain fp8 MFMA
    p.A = (const uint16_t*)(ws.q8n + row0 * K); set_fp8(p, ws.qs + row0, lw.wscale);
  } else if (src == ASrc::Wide) {
    p.A = (const uint16_t*)(ws.q8 + row0 * K); set_fp8(p, ws.ones + row0, lw.wscale, ws.mxw + row0 * ws.ld_mxw, ws.ld_mxw);
  } else {
    p.A = (const uint16_t*)(ws.q8n + row0 * K); set_fp8(p, ws.ones + row0, lw.wscale, ws.mxn + row0 * ws.ld_mxn, ws.ld_mxn);
  }
}
// ... and the producer side (block-scaled mode): the epilogue of p stores its columns from col0 on as columns dst_col0.. of rows row0.. of
// the wide operand (ld8 bytes per row) instead of bf16 to C
void bind_fp8_producer(GemmProblem& p, const Fwd& f, int64_t row0, int64_t ld8, int64_t dst_col0, int col0) {
  p.c8 = f.ws.q8 + row0 * ld8 + dst_col0; p.ldc8 = ld8; p.c8_col0 = col0;
  p.c_mx = f.ws.mxw + row0 * f.ws.ld_mxw + dst_col0 / 128; p.ld_cmx = f.ws.ld_mxw;
}
// the quantisation pass in front of an fp8 GEMM whose K-wide operand no producer wrote
int fwd_quant_operand(Fwd& f, ASrc src, const uint16_t* A, int64_t lda, int K) {
  const Workspace& ws = f.ws;
  if (f.fp8.mx && src == ASrc::Bf16) HIP_TRY(launch_quant_rows_mx8(A, lda, ws.q8n, K, ws.mxn, ws.ld_mxn, (int)f.R, K, f.st));
  else if (f.c->fp8 && !f.fp8.mx) HIP_TRY(launch_quant_rows_fp8(A, lda, ws.q8, K, ws.qs, (int)f.R, K, f.st));     // per-token scales, all rows at once
  return AFX_OK;
}

// One per-stream linear of a double block: 2 problems per sample in one grouped launch.  wide_out: this GEMM's epilogue writes the wide operand.
// A launch costs ceil(rounds) x tile area, so a SHORT text stream (Qwen-Image: 128 rows) costs the grouped launch a row of half-empty tiles;
// the text problems as a launch of their own were level at best and are gone (docs/DESIGN_HISTORY_r04_r05.md, "short text stream").
int stream_gemm(Fwd& f, const uint16_t* A, int64_t lda, int K, const LinW (&lw)[2], uint16_t* C, int64_t ldc, int Nout, int epi, int blk,
                int gate_chunk, const float* qkn = nullptr, ASrc src = ASrc::Bf16, bool wide_out = false) {
  GemmBatch gb{};
  AFX_TRY(fwd_quant_operand(f, src, A, lda, K));
  for (int b = 0; b < f.bs.B; ++b)
    for (int s = 0; s < 2; ++s) {   // 0 image rows, 1 text rows
      GemmProblem& p = gb.p[gb.nprob++];
      stream_problem(p, f.bs, A, lda, K, lw[s], C, ldc, Nout, b, s);
      const int64_t row0 = (int64_t)b * f.bs.S + (s == 0 ? f.bs.T : 0);
      bind_fp8_operand(p, f, src, row0, K, lw[s]);
      if (wide_out) bind_fp8_producer(p, f, row0, Nout, 0, 0);
      p.epi = epi;
      if (qkn != nullptr) stream_qk_epilogue(p, f.bs, qkn, s);          // [img_q, img_k, txt_q, txt_k][128]
      if (epi == EPI_GATE_RES) set_epilogue(p, epi, 0, f.ws.mod + (int64_t)b * f.ldm + f.ml.dbl(blk, s, gate_chunk), 0, 1 << 30, C + row0 * ldc, ldc);
    }
  return fwd_gemm(f, gb);
}

// LN + modulate of both streams of every sample in one launch (text rows take the text stream's vectors).  *out: where the next GEMM finds
// the rows -- Norm when (block-scaled mode) the kernel wrote the GEMM operand itself, else Bf16 (Xn)
int stream_norm(Fwd& f, int blk, int shift_chunk, int scale_chunk, ASrc* out) {
  const Workspace& ws = f.ws;
  const float *sc_i = ws.mod + f.ml.dbl(blk, 0, scale_chunk), *sh_i = ws.mod + f.ml.dbl(blk, 0, shift_chunk);
  const float *sc_t = ws.mod + f.ml.dbl(blk, 1, scale_chunk), *sh_t = ws.mod + f.ml.dbl(blk, 1, shift_chunk);
  bool fused = false;
  if (f.fp8.mx)
    HIP_TRY(launch_norm_modulate_mx8(ws.X, f.D, ws.q8n, f.D, ws.mxn, ws.ld_mxn, (int)f.R, (int)f.D, sc_i, sh_i, sc_t, sh_t, f.ldm, f.bs.S, f.bs.T, f.st,
                                     &fused, f.fp8.norm_rows ? ws.qs : nullptr));
  if (!fused) HIP_TRY(launch_norm_modulate_joint(ws.X, f.D, ws.Xn, f.D, (int)f.R, (int)f.D, sc_i, sh_i, sc_t, sh_t, f.ldm, f.bs.S, f.bs.T, f.st));
  *out = fused ? ASrc::Norm : ASrc::Bf16;
  return AFX_OK;
}

// the modulation vectors and embeddings of this call: copied from a prepared step, or computed here
int fwd_conditioning(Fwd& f, const void* pooled, const float* t, const float* g) {
  afx_ctx* c = f.c;
  const Workspace& ws = f.ws;
  const int B = f.bs.B;
  const int prep_k = c->prep_use;
  c->prep_use = -1;                              // one-shot
  if (prep_k >= 0 && prep_k < c->prep_steps && c->prep_B == B && c->temb_override == nullptr) {
    // the modulation vectors (and temb, for afx_mmdit_export) of this step were computed by afx_mmdit_prepare_steps
    const int64_t r0 = (int64_t)prep_k * B;
    HIP_TRY(hipMemcpyAsync(ws.mod, ws.prep_mod + r0 * f.ldm, (size_t)B * f.ldm * 4, hipMemcpyDeviceToDevice, f.st));
    HIP_TRY(hipMemcpyAsync(ws.temb, ws.prep_temb + r0 * f.D, (size_t)B * f.D * 4, hipMemcpyDeviceToDevice, f.st));
    HIP_TRY(hipMemcpyAsync(ws.semb, ws.prep_semb + r0 * f.D, (size_t)B * f.D * 4, hipMemcpyDeviceToDevice, f.st));
    return AFX_OK;
  }
  if (c->temb_override != nullptr) HIP_TRY(hipMemcpyAsync(ws.temb, c->temb_override, (size_t)B * f.D * 4, hipMemcpyDeviceToDevice, f.st));
  return conditioning(c, c->temb_override != nullptr ? nullptr : t, 1, g, pooled, B, CondBufs{ws.sincos, ws.pooled, ws.tmp, ws.temb, ws.semb, ws.mod}, f.st);
}

// embedders into the joint layout X[b][text T | image N]
int fwd_embed(Fwd& f, const void* x, const void* ctx_emb) {
  const afx_model_desc& d = f.c->d;
  const OuterW& w = f.c->ow;
  const Workspace& ws = f.ws;
  const int64_t B = f.bs.B, N = f.bs.N, T = f.bs.T, S = f.bs.S, D = f.D;
  const uint16_t* ctx_src = (const uint16_t*)ctx_emb;
  if (d.family == 1) {   // Qwen: RMSNorm(joint_dim) on the text states before txt_in (arcqwen.py:129)
    HIP_TRY(launch_norm_modulate(ctx_src, d.joint_dim, ws.F, d.joint_dim, (int)(B * T), d.joint_dim, w.txt_norm, nullptr, 0, (int)(B * T), 1, f.st));
    ctx_src = ws.F;
  }
  GemmBatch gb{};
  for (int b = 0; b < B; ++b) {
    linear_problem(gb.p[gb.nprob++], (const uint16_t*)x + b * N * d.in_channels, d.in_channels, w.x_in, 0, ws.X + (b * S + T) * D, D, (int)N, (int)D, d.in_channels);
    linear_problem(gb.p[gb.nprob++], ctx_src + b * T * d.joint_dim, d.joint_dim, w.ctx_in, 0, ws.X + b * S * D, D, (int)T, (int)D, d.joint_dim);
  }
  return fwd_gemm(f, gb);
}

// attention over the [k | v | q ...] rows of stride ldf (O overwrites Q).  omx: the fp8 operand the kernel writes too where it can (*o_fused)
int fwd_attention(Fwd& f, uint16_t* F, int64_t ldf, const AttnMx8& omx, bool* o_fused) {
  const BlockShape& bs = f.bs;
  ProfScope ps_(f.c, f.st, 1, 4.0 * bs.B * bs.H * (double)bs.S * bs.S * 128);
  HIP_TRY(launch_attention(F + 2 * f.D, ldf, F, ldf, f.ws.Vt, F + 2 * f.D, ldf, bs.B, bs.H, bs.S, f.st, nullptr, f.fp8.attn_mx ? &omx : nullptr, o_fused));
  return AFX_OK;
}

// dual-stream block i
int fwd_double_block(Fwd& f, int i) {
  const Workspace& ws = f.ws;
  const int64_t D = f.D, R = f.R;
  const bool mx = f.fp8.mx;
  const DoubleW& bw = f.c->dbl[i];
  const float* qkn = bw.qkn;            // [img_q, img_k, txt_q, txt_k][128]
  uint16_t* QKV = ws.F;                 // [R, 3D]  rows k|v|q
  uint16_t* Hb = ws.F + R * 3 * D;      // [R, 4D]  MLP hidden
  if (f.c->ckpt) HIP_TRY(hipMemcpyAsync(f.c->ckpt + (int64_t)i * R * D, ws.X, (size_t)R * D * 2, hipMemcpyDeviceToDevice, f.st));
  ASrc normed;
  AFX_TRY(stream_norm(f, i, 0, 1, &normed));
  if (f.dpath == AFX_QKV_VT_PROJ) {     // per sample: img k, q, v^T + txt k, q, v^T = 6 problems in one launch
    for (int b = 0; b < f.bs.B; ++b) {
      GemmBatch gb{};
      double_vt_batch(gb, f.bs, ws.Xn, D, bw.qkv, QKV, 3 * D, qkn, b);
      AFX_TRY(fwd_gemm(f, gb));
    }
  } else AFX_TRY(stream_gemm(f, ws.Xn, D, (int)D, bw.qkv, QKV, 3 * D, (int)(3 * D), EPI_NONE, i, 0, f.dpath == AFX_QKV_QK_EPI ? qkn : nullptr, normed));
  // V -> V^T (QK_EPI), or k, q: RMSNorm + RoPE in place and V -> V^T in one launch (KV_PREP)
  HIP_TRY(qkv_finish(f.dpath, f.bs, QKV, 3 * D, qkn + 3 * 128, qkn + 1 * 128, qkn + 2 * 128, qkn, f.st));
  bool o_fused = false;                 // mx: the attention kernel wrote the out-projection's operand itself (q8n / mxn)
  AFX_TRY(fwd_attention(f, QKV, 3 * D, AttnMx8{ws.q8n, D, ws.mxn, ws.ld_mxn}, &o_fused));
  AFX_TRY(stream_gemm(f, QKV + 2 * D, 3 * D, (int)D, bw.out, ws.X, D, (int)D, EPI_GATE_RES, i, 2, nullptr, o_fused ? ASrc::Attn : ASrc::Bf16));
  AFX_TRY(stream_norm(f, i, 3, 4, &normed));
  AFX_TRY(stream_gemm(f, ws.Xn, D, (int)D, bw.mlp1, Hb, 4 * D, (int)(4 * D), EPI_GELU, i, 0, nullptr, normed, mx));      // (mx: the hidden leaves as the next GEMM's operand, Hb stays unwritten)
  return stream_gemm(f, Hb, 4 * D, (int)(4 * D), bw.mlp2, ws.X, D, (int)D, EPI_GATE_RES, i, 5, nullptr, mx ? ASrc::Wide : ASrc::Bf16);
}

// single-stream block i on the joint sequence
int fwd_single_block(Fwd& f, int i) {
  const Workspace& ws = f.ws;
  const int64_t D = f.D, R = f.R, ldm = f.ldm;
  const int S = f.bs.S;
  const bool mx = f.fp8.mx;
  const SingleW& bw = f.c->sgl[i];
  const float* qkn = bw.qkn;            // [q, k][128]
  const float *scale = ws.mod + f.ml.sgl(i, 1), *shift = ws.mod + f.ml.sgl(i, 0);
  if (f.c->ckpt)
    HIP_TRY(hipMemcpyAsync(f.c->ckpt + (int64_t)(f.c->d.num_double + i) * R * D, ws.X, (size_t)R * D * 2, hipMemcpyDeviceToDevice, f.st));
  bool sgl_fused = false;
  if (mx) HIP_TRY(launch_norm_modulate_mx8(ws.X, D, ws.q8n, D, ws.mxn, ws.ld_mxn, (int)R, (int)D, scale, shift, nullptr, nullptr, ldm, S, 0, f.st,
                                           &sgl_fused, f.fp8.norm_rows ? ws.qs : nullptr));
  if (!sgl_fused) HIP_TRY(launch_norm_modulate(ws.X, D, ws.Xn, D, (int)R, (int)D, scale, shift, ldm, S, 0, f.st));
  const ASrc normed = sgl_fused ? ASrc::Norm : ASrc::Bf16;
  GemmBatch gb{};
  single_qkv_batch(gb, f.spath, f.bs, ws.Xn, D, bw.fused, ws.F, 7 * D, qkn);      // (VT_PROJ is never taken in fp8 mode)
  AFX_TRY(fwd_quant_operand(f, normed, ws.Xn, D, (int)D));
  bind_fp8_operand(gb.p[0], f, normed, 0, (int)D, bw.fused);
  if (mx) bind_fp8_producer(gb.p[0], f, 0, 5 * D, D, (int)(3 * D));      // the mlp columns leave as columns [D, 5D) of the proj_out operand
  AFX_TRY(fwd_gemm(f, gb));
  HIP_TRY(qkv_finish(f.spath, f.bs, ws.F, 7 * D, qkn + 128, qkn + 128, qkn, qkn, f.st));
  bool o_fused = false;                 // mx: ... columns [0, D) of the [O | mlp] operand (q8 / mxw)
  AFX_TRY(fwd_attention(f, ws.F, 7 * D, AttnMx8{ws.q8, 5 * D, ws.mxw, ws.ld_mxw}, &o_fused));
  GemmBatch go{};
  GemmProblem& o = go.p[go.nprob++];
  linear_problem(o, ws.F + 2 * D, 7 * D, bw.out, 0, ws.X, D, (int)R, (int)D, (int)(5 * D));
  set_epilogue(o, EPI_GATE_RES, 0, ws.mod + f.ml.sgl(i, 2), ldm, S, ws.X, D);
  // mx: the attention output joins the mlp columns the projection's epilogue left in q8 (a pass of D columns unless the attention kernel wrote
  // them); per-token scales: the usual pass over all 5D columns.  Either way the operand is the wide one.
  if (mx && !o_fused) HIP_TRY(launch_quant_rows_mx8(ws.F + 2 * D, 7 * D, ws.q8, 5 * D, ws.mxw, ws.ld_mxw, (int)R, (int)D, f.st));
  if (!mx) AFX_TRY(fwd_quant_operand(f, ASrc::Bf16, ws.F + 2 * D, 7 * D, (int)(5 * D)));
  bind_fp8_operand(o, f, ASrc::Wide, 0, (int)(5 * D), bw.out);
  return fwd_gemm(f, go);
}

// norm_out (scale first) + velocity head on the image tokens
int fwd_head(Fwd& f, void* means, void* logw, void* logg) {
  afx_ctx* c = f.c;
  const afx_model_desc& d = c->d;
  const Workspace& ws = f.ws;
  const int64_t B = f.bs.B, N = f.bs.N, T = f.bs.T, S = f.bs.S, D = f.D, ldm = f.ldm;
  for (int b = 0; b < B; ++b)
    HIP_TRY(launch_norm_modulate(ws.X + (b * S + T) * D, D, ws.Xn + b * N * D, D, (int)N, (int)D, ws.mod + b * ldm + f.ml.fin(0),
                                 ws.mod + b * ldm + f.ml.fin(1), 0, 1 << 30, 0, f.st));
  GemmBatch gb{};      // (teacher: velocity [B*N, in_channels] written directly)
  linear_problem(gb.p[gb.nprob++], ws.Xn, D, c->ow.head, 0, d.head_mode == 0 ? ws.head : (uint16_t*)means, c->head_n, (int)(B * N), c->head_n, (int)D);
  AFX_TRY(fwd_gemm(f, gb));
  if (d.head_mode == 0)
    HIP_TRY(launch_head_split(ws.head, c->head_n, (uint16_t*)means, (uint16_t*)logw, (uint16_t*)logg, B * N,
                              d.num_gaussians, d.in_channels, d.logweights_channels, f.st));
  return AFX_OK;
}

}  // namespace

extern "C" {

const char* afx_last_error(void) { return afx_g_err; }
const char* afx_version(void) { return "arcflow_hip 0.1 (gfx950)"; }

int afx_create(const afx_model_desc* desc, afx_ctx** out) {
  if (!desc || !out) return fail(AFX_E_INVALID, "null argument");
  if (desc->head_dim != 128) return fail(AFX_E_UNSUPPORTED, "head_dim must be 128");
  if (desc->heads <= 0 || desc->num_double < 0 || desc->num_single < 0 || desc->num_gaussians < 1 ||
      desc->num_gaussians > 32)
    return fail(AFX_E_INVALID, "bad model description");
  if (desc->in_channels % 64 != 0 || desc->joint_dim % 64 != 0)
    return fail(AFX_E_UNSUPPORTED, "in_channels and joint_dim must be multiples of 64");
  afx_ctx* c = new afx_ctx();
  c->d = *desc;
  c->D = desc->heads * desc->head_dim;
  ModLayout ml{c->D, desc->num_double, desc->num_single};
  c->n_mod = ml.total();
  const int K = desc->num_gaussians, ch = desc->in_channels, lw = desc->logweights_channels;
  const int raw = desc->head_mode == 0 ? K * ch + K * lw + (K - 1) * lw : ch;
  c->head_n = (raw + 7) / 8 * 8;
  *out = c;
  return AFX_OK;
}

int afx_destroy(afx_ctx* ctx) {
  if (ctx) {
    for (auto& r : ctx->prof_pool) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  }
  delete ctx;
  return AFX_OK;
}

int afx_bind_weight(afx_ctx* ctx, const char* name, const void* dptr, int32_t dtype, int32_t ndim,
                    const int64_t* shape) {
  if (!ctx || !name || !dptr || ndim < 1 || ndim > 4 || !shape) return fail(AFX_E_INVALID, "bad bind_weight argument");
  if (dtype != AFX_DT_BF16 && dtype != AFX_DT_F32 && dtype != AFX_DT_FP8) return fail(AFX_E_INVALID, "bad dtype for '%s'", name);
  Weight w;
  w.ptr = dptr;
  w.dtype = dtype;
  w.shape.assign(shape, shape + ndim);
  ctx->w[name] = w;
  ctx->finalized = false;
  return AFX_OK;
}

int afx_finalize(afx_ctx* c) {
  if (!c) return fail(AFX_E_INVALID, "null ctx");
  const int64_t D = c->D;
  const afx_model_desc& d = c->d;
  AFX_TRY(need_linear(c, "x_in", D, d.in_channels));
  AFX_TRY(need_linear(c, "ctx_in", D, d.joint_dim));
  if (d.family == 1) AFX_TRY(need(c, "txt_norm.weight", AFX_DT_F32, {d.joint_dim}));
  AFX_TRY(need_linear(c, "temb.t.l1", D, 256));
  AFX_TRY(need_linear(c, "temb.t.l2", D, D));
  if (d.guidance_embeds) AFX_TRY(need_linear(c, "temb.g.l1", D, 256));
  if (d.guidance_embeds) AFX_TRY(need_linear(c, "temb.g.l2", D, D));
  if (d.pooled_dim > 0) AFX_TRY(need_linear(c, "temb.p.l1", D, d.pooled_dim));
  if (d.pooled_dim > 0) AFX_TRY(need_linear(c, "temb.p.l2", D, D));
  AFX_TRY(need_linear(c, "mod", c->n_mod, D));
  for (int i = 0; i < d.num_double; ++i) {
    const std::string p = "d" + std::to_string(i) + ".";
    for (const char* s : {"img", "txt"}) {
      AFX_TRY(need_linear(c, p + s + "_qkv", 3 * D, D));
      AFX_TRY(need_linear(c, p + s + "_out", D, D));
      AFX_TRY(need_linear(c, p + s + "_mlp1", 4 * D, D));
      AFX_TRY(need_linear(c, p + s + "_mlp2", D, 4 * D));
    }
    AFX_TRY(need(c, p + "qknorm", AFX_DT_F32, {4, 128}));
  }
  for (int i = 0; i < d.num_single; ++i) {
    const std::string p = "s" + std::to_string(i) + ".";
    AFX_TRY(need_linear(c, p + "fused", 7 * D, D));
    AFX_TRY(need_linear(c, p + "out", D, 5 * D));
    AFX_TRY(need(c, p + "qknorm", AFX_DT_F32, {2, 128}));
  }
  AFX_TRY(need_linear(c, "head", c->head_n, D));
  if (c->w.count("mod_final.weight")) AFX_TRY(need_linear(c, "mod_final", 2 * D, D));
  auto lin = [&](const std::string& n) {
    return LinW{wptr<uint16_t>(c, n + ".weight"), wptr<uint16_t>(c, n + ".bias"), wptr<void>(c, n + ".weight_q"), wptr<float>(c, n + ".wscale")};
  };
  c->dbl.assign(d.num_double, DoubleW{});
  for (int i = 0; i < d.num_double; ++i) {
    const std::string p = "d" + std::to_string(i) + ".";
    for (int s = 0; s < 2; ++s) {
      const std::string q = p + (s == 0 ? "img_" : "txt_");
      c->dbl[i].qkv[s] = lin(q + "qkv"); c->dbl[i].out[s] = lin(q + "out");
      c->dbl[i].mlp1[s] = lin(q + "mlp1"); c->dbl[i].mlp2[s] = lin(q + "mlp2");
    }
    c->dbl[i].qkn = wptr<float>(c, p + "qknorm");
  }
  c->sgl.assign(d.num_single, SingleW{});
  for (int i = 0; i < d.num_single; ++i) {
    const std::string p = "s" + std::to_string(i) + ".";
    c->sgl[i].fused = lin(p + "fused"); c->sgl[i].out = lin(p + "out");
    c->sgl[i].qkn = wptr<float>(c, p + "qknorm");
  }
  c->ow = OuterW{lin("temb.t.l1"), lin("temb.t.l2"), lin("temb.g.l1"), lin("temb.g.l2"), lin("temb.p.l1"), lin("temb.p.l2"), lin("mod"),
                 lin("mod_final"), lin("x_in"), lin("ctx_in"), lin("head"), wptr<float>(c, "txt_norm.weight")};
  c->finalized = true;
  return AFX_OK;
}

int64_t afx_workspace_bytes(const afx_ctx* ctx, int32_t batch, int32_t n_img, int32_t n_txt) {
  if (!ctx || batch < 1 || n_img < 1 || n_txt < 0) return fail(AFX_E_INVALID, "bad workspace query");
  return carve(ctx, nullptr, batch, n_img, n_txt).total;
}

int afx_head_width(const afx_ctx* ctx) {
  if (!ctx) return fail(AFX_E_INVALID, "afx_head_width: null ctx");
  return ctx->head_n;
}

int afx_set_workspace(afx_ctx* ctx, void* dptr, int64_t bytes) {
  if (!ctx || !dptr || bytes <= 0) return fail(AFX_E_INVALID, "bad workspace");
  if (((uintptr_t)dptr & 255) != 0) return fail(AFX_E_INVALID, "workspace must be 256-byte aligned");
  ctx->ws = (char*)dptr;
  ctx->ws_bytes = bytes;
  ctx->prep_steps = 0;                                       // prepared steps lived in the old workspace
  ctx->prep_use = -1;
  return AFX_OK;
}

int afx_mmdit_forward(afx_ctx* c, const void* x, const void* ctx_emb, const void* pooled, const float* t,
                      const float* g, const float* rope_cos, const float* rope_sin, int32_t B, int32_t N,
                      int32_t T, void* means, void* logw, void* logg, void* stream_) {
  return afx_mmdit_forward_stage(c, x, ctx_emb, pooled, t, g, rope_cos, rope_sin, B, N, T, means, logw, logg, 0, stream_);
}

int afx_mmdit_forward_stage(afx_ctx* c, const void* x, const void* ctx_emb, const void* pooled, const float* t,
                            const float* g, const float* rope_cos, const float* rope_sin, int32_t B, int32_t N,
                            int32_t T, void* means, void* logw, void* logg, int32_t stage, void* stream_) {
  if (stage < 0 || stage > 2) return fail(AFX_E_INVALID, "stage must be 0 (all), 1 (conditioning + embedders) or 2 (norm_out + head)");
  if (!c || !x || !ctx_emb || !t || !rope_cos || !rope_sin || !means)
    return fail(AFX_E_INVALID, "null argument to afx_mmdit_forward");
  if (!c->finalized) return fail(AFX_E_MISSING, "afx_finalize() has not succeeded on this context");
  const afx_model_desc& d = c->d;
  if (B < 1 || N < 1 || T < 1) return fail(AFX_E_INVALID, "bad shape: batch, N, T >= 1");
  if (B > AFX_MAX_MICRO_BATCH) {
    // A grouped launch holds 2 problems per sample (GEMM_MAX_PROBLEMS = 8) and the workspace is carved for 4 samples: larger
    // batches run as micro-batches of 4 on the same stream (samples are independent: the reference's batch dimension,
    // arcflux.py:134-257, has no cross-sample op).  The staged (training) calls keep one micro-batch per call.
    if (stage != 0 || c->ckpt) return fail(AFX_E_INVALID, "staged / checkpointed forward: batch must be 1..4 per call");
    const int64_t K = d.num_gaussians, Cc = d.in_channels, lw = d.logweights_channels;
    for (int b0 = 0; b0 < B; b0 += AFX_MAX_MICRO_BATCH) {
      const int nb = B - b0 < AFX_MAX_MICRO_BATCH ? B - b0 : AFX_MAX_MICRO_BATCH;
      const uint16_t* xb = (const uint16_t*)x + (int64_t)b0 * N * Cc;
      const uint16_t* cb = (const uint16_t*)ctx_emb + (int64_t)b0 * T * d.joint_dim;
      const uint16_t* pb = pooled ? (const uint16_t*)pooled + (int64_t)b0 * d.pooled_dim : nullptr;
      uint16_t* mb = (uint16_t*)means + (int64_t)b0 * N * (d.head_mode == 0 ? K * Cc : Cc);
      uint16_t* wb = logw ? (uint16_t*)logw + (int64_t)b0 * N * K * lw : nullptr;
      uint16_t* gb_ = logg ? (uint16_t*)logg + (int64_t)b0 * N * (K - 1) * lw : nullptr;
      const float* temb_all = c->temb_override;
      if (temb_all) c->temb_override = temb_all + (int64_t)b0 * c->D;
      const int rc = afx_mmdit_forward_stage(c, xb, cb, pb, t + b0, g ? g + b0 : nullptr, rope_cos, rope_sin, nb, N, T, mb, wb, gb_, 0, stream_);
      c->temb_override = temb_all;
      if (rc != AFX_OK) return rc;
    }
    return AFX_OK;
  }
  if (d.guidance_embeds && !g) return fail(AFX_E_INVALID, "guidance vector required");
  if (d.pooled_dim > 0 && !pooled) return fail(AFX_E_INVALID, "pooled projections required");
  if (d.head_mode == 0 && (!logw || !logg)) return fail(AFX_E_INVALID, "logw/logg outputs required");
  Workspace ws = carve(c, c->ws, B, N, T);
  if (!c->ws || ws.total > c->ws_bytes)
    return fail(AFX_E_WORKSPACE, "workspace too small: need %lld bytes, have %lld", (long long)ws.total, (long long)c->ws_bytes);
  Fwd f{c, ws, (hipStream_t)stream_, block_shape(d.heads, B, N, T, rope_cos, rope_sin, ws.Vt), ModLayout{c->D, d.num_double, d.num_single},
        c->n_mod, c->D, (int64_t)B * (N + T), Fp8Mode{}, 0, 0};
  if (stage != 2) {
    AFX_TRY(fwd_conditioning(f, pooled, t, g));
    AFX_TRY(fwd_embed(f, x, ctx_emb));
  }
  if (stage == 1) return AFX_OK;       // the caller runs the blocks itself on the exported token matrix
  AFX_TRY(fwd_resolve_fp8(f));
  if (stage == 0) {
    for (int i = 0; i < d.num_double; ++i) AFX_TRY(fwd_double_block(f, i));
    for (int i = 0; i < d.num_single; ++i) AFX_TRY(fwd_single_block(f, i));
  }
  return fwd_head(f, means, logw, logg);
}

int afx_mmdit_prepare_steps(afx_ctx* c, const void* pooled, const float* t_steps, const float* g, int32_t B, int32_t nsteps,
                            void* stream_) {
  if (!c || !t_steps) return fail(AFX_E_INVALID, "null argument to afx_mmdit_prepare_steps");
  if (!c->finalized) return fail(AFX_E_MISSING, "afx_finalize() has not succeeded on this context");
  const afx_model_desc& d = c->d;
  if (B < 1 || nsteps < 1 || B > AFX_MAX_MICRO_BATCH || (int64_t)B * nsteps > AFX_PREP_ROWS)
    return fail(AFX_E_INVALID, "afx_mmdit_prepare_steps: batch <= 4 and batch * steps <= %d", AFX_PREP_ROWS);
  if (d.guidance_embeds && !g) return fail(AFX_E_INVALID, "guidance vector required");
  if (d.pooled_dim > 0 && !pooled) return fail(AFX_E_INVALID, "pooled projections required");
  if (c->temb_override) return fail(AFX_E_INVALID, "afx_mmdit_prepare_steps: not with a timestep-embedding override");
  Workspace ws = carve(c, c->ws, 1, 1, 1);                       // (only the shape-independent head of the workspace is used)
  if (!c->ws || ws.total > c->ws_bytes) return fail(AFX_E_WORKSPACE, "workspace not set / too small");
  c->prep_steps = 0; c->prep_use = -1;
  // temb of every (step, sample): the same three tiny MLPs as the forward, B rows at a time into row block k.  Scratch: the hidden rows live in
  // the semb block until the SiLU overwrites them, the sincos / pooled rows ([B, 256] / [B, pooled_dim]) in the mod block, free until the big pass.
  // Then ONE pass over the stacked [n_mod, D] matrix for all steps: the matrix (6.5 GB for FLUX) is what the time goes into, the
  // number of right-hand sides is free up to the GEMV's 8
  AFX_TRY(conditioning(c, t_steps, nsteps, g, pooled, B, CondBufs{ws.prep_mod, ws.prep_mod, ws.prep_semb, ws.prep_temb, ws.prep_semb, ws.prep_mod},
                       (hipStream_t)stream_));
  c->prep_steps = nsteps; c->prep_B = B;
  return AFX_OK;
}

int afx_mmdit_use_prepared_step(afx_ctx* c, int32_t k) {
  if (!c) return fail(AFX_E_INVALID, "null ctx");
  if (k >= c->prep_steps) return fail(AFX_E_INVALID, "afx_mmdit_use_prepared_step: step %d of %d prepared", k, c->prep_steps);
  c->prep_use = k < 0 ? -1 : k;
  return AFX_OK;
}

int afx_mmdit_import_tokens(afx_ctx* c, const void* src, int32_t batch, int32_t n_img, int32_t n_txt, void* stream) {
  if (!c || !src || !c->ws || batch < 1 || n_img < 1 || n_txt < 0) return fail(AFX_E_INVALID, "bad argument to afx_mmdit_import_tokens");
  Workspace ws = carve(c, c->ws, batch, n_img, n_txt);
  if (ws.total > c->ws_bytes)
    return fail(AFX_E_WORKSPACE, "afx_mmdit_import_tokens: shape (%d, %d, %d) needs %lld workspace bytes, have %lld", batch, n_img, n_txt,
                (long long)ws.total, (long long)c->ws_bytes);
  HIP_TRY(hipMemcpyAsync(ws.X, src, (size_t)batch * (n_img + n_txt) * c->D * 2, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return AFX_OK;
}

int afx_mmdit_export(afx_ctx* c, const char* what, void* dst, int32_t batch, int32_t n_img, int32_t n_txt, void* stream) {
  if (!c || !what || !dst || !c->ws || batch < 1 || n_img < 1 || n_txt < 0) return fail(AFX_E_INVALID, "bad argument to afx_mmdit_export");
  Workspace ws = carve(c, c->ws, batch, n_img, n_txt);
  // the layout is a function of the shape: a shape the bound workspace was not sized for would read past it / from another layout
  if (ws.total > c->ws_bytes)
    return fail(AFX_E_WORKSPACE, "afx_mmdit_export: shape (%d, %d, %d) needs %lld workspace bytes, have %lld", batch, n_img, n_txt,
                (long long)ws.total, (long long)c->ws_bytes);
  const int64_t D = c->D;
  ModLayout ml{D, c->d.num_double, c->d.num_single};
  hipStream_t st = (hipStream_t)stream;
  const std::string w(what);
  if (w == "head_in") {            // [B*N, D] bf16: norm_out output = input of the velocity head
    HIP_TRY(hipMemcpyAsync(dst, ws.Xn, (size_t)batch * n_img * D * 2, hipMemcpyDeviceToDevice, st));
  } else if (w == "x_final") {     // [B*N, D] bf16: image tokens entering norm_out
    for (int b = 0; b < batch; ++b)
      HIP_TRY(hipMemcpyAsync((char*)dst + (size_t)b * n_img * D * 2, ws.X + ((int64_t)b * (n_img + n_txt) + n_txt) * D,
                             (size_t)n_img * D * 2, hipMemcpyDeviceToDevice, st));
  } else if (w == "x_tokens") {    // [B*(T+N), D] bf16: the joint token matrix (after the embedders / after the last block)
    HIP_TRY(hipMemcpyAsync(dst, ws.X, (size_t)batch * (n_img + n_txt) * D * 2, hipMemcpyDeviceToDevice, st));
  } else if (w == "temb") {        // [B, D] f32: the summed conditioning embedding before SiLU
    HIP_TRY(hipMemcpyAsync(dst, ws.temb, (size_t)batch * D * 4, hipMemcpyDeviceToDevice, st));
  } else if (w == "silu_temb") {   // [B, D] f32
    HIP_TRY(hipMemcpyAsync(dst, ws.semb, (size_t)batch * D * 4, hipMemcpyDeviceToDevice, st));
  } else if (w == "mod_all") {     // [B, n_mod] f32: every AdaLN modulation vector of the network
    HIP_TRY(hipMemcpyAsync(dst, ws.mod, (size_t)batch * c->n_mod * 4, hipMemcpyDeviceToDevice, st));
  } else if (w == "mod_final") {   // [B, 2D] f32: (scale | shift) of norm_out
    for (int b = 0; b < batch; ++b)
      HIP_TRY(hipMemcpyAsync((char*)dst + (size_t)b * 2 * D * 4, ws.mod + (int64_t)b * c->n_mod + ml.fin(0), (size_t)2 * D * 4,
                             hipMemcpyDeviceToDevice, st));
  } else {
    return fail(AFX_E_INVALID, "afx_mmdit_export: unknown buffer '%s'", what);
  }
  return AFX_OK;
}

int afx_set_fp8_linear(afx_ctx* c, int32_t on) {
  if (!c) return fail(AFX_E_INVALID, "null ctx");
  if (on) {
    const int64_t D = c->D;
    int r;
    auto chk = [&](const std::string& n, int64_t out_f, int64_t in_f) -> int {
      if ((r = need(c, n + ".weight_q", AFX_DT_FP8, {out_f, in_f})) != AFX_OK) return r;
      return need(c, n + ".wscale", AFX_DT_F32, {out_f});
    };
    for (int i = 0; i < c->d.num_double; ++i)
      for (const char* s : {"img_", "txt_"}) {
        const std::string p = "d" + std::to_string(i) + "." + s;
        if ((r = chk(p + "qkv", 3 * D, D)) || (r = chk(p + "out", D, D)) || (r = chk(p + "mlp1", 4 * D, D)) || (r = chk(p + "mlp2", D, 4 * D))) return r;
      }
    for (int i = 0; i < c->d.num_single; ++i) {
      const std::string p = "s" + std::to_string(i) + ".";
      if ((r = chk(p + "fused", 7 * D, D)) || (r = chk(p + "out", D, 5 * D))) return r;
    }
  }
  c->fp8 = on != 0;
  return AFX_OK;
}

int afx_set_temb_override(afx_ctx* ctx, const float* temb_t) {
  if (!ctx) return fail(AFX_E_INVALID, "null ctx");
  ctx->temb_override = temb_t;
  return AFX_OK;
}

int afx_set_checkpoint_buffer(afx_ctx* ctx, void* dptr) {
  if (!ctx) return fail(AFX_E_INVALID, "null ctx");
  ctx->ckpt = (uint16_t*)dptr;     // nullptr switches checkpointing off
  return AFX_OK;
}

int afx_profile_enable(afx_ctx* ctx, int32_t on) {
  if (!ctx) return fail(AFX_E_INVALID, "null ctx");
  ctx->prof_on = on != 0;
  ctx->prof_stride = on > 1 ? on : 1;
  ctx->prof_count = 0;
  ctx->prof_used = 0;
  return AFX_OK;
}

int afx_profile_read(afx_ctx* ctx, int32_t klass, double* total_ms, int64_t* launches, double* flops) {
  if (!ctx || !total_ms || !launches || !flops) return fail(AFX_E_INVALID, "null argument to afx_profile_read");
  double ms = 0, fl = 0;
  int64_t n = 0;
  for (size_t i = 0; i < ctx->prof_used; ++i) {
    auto& r = ctx->prof_pool[i];
    if (r.klass != klass) continue;
    HIP_TRY(hipEventSynchronize(r.b));
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, r.a, r.b));
    ms += t; fl += r.flops; ++n;
  }
  *total_ms = ms; *launches = n; *flops = fl;
  return AFX_OK;
}

int afx_qkv_operands(int32_t kind, const void* A, int64_t lda, const void* w_img, const void* b_img, const void* w_txt, const void* b_txt,
                     const float* qkn, const float* rope_cos, const float* rope_sin, int32_t B, int32_t N, int32_t T, int32_t heads,
                     int32_t path, void* F, int64_t ldf, void* Vt, void* stream) {
  if (kind != AFX_BLOCK_DOUBLE && kind != AFX_BLOCK_SINGLE) return fail(AFX_E_INVALID, "afx_qkv_operands: kind must be AFX_BLOCK_DOUBLE or AFX_BLOCK_SINGLE");
  const bool single = kind == AFX_BLOCK_SINGLE;
  if (!A || !w_img || !qkn || !rope_cos || !rope_sin || !F || !Vt || (!single && !w_txt) || (!single && (!b_img) != (!b_txt)))
    return fail(AFX_E_INVALID, "null argument to afx_qkv_operands");
  if (B < 1 || B > AFX_MAX_MICRO_BATCH || N < 1 || T < 1 || heads < 1 || path < AFX_QKV_AUTO || path > AFX_QKV_KV_PREP)
    return fail(AFX_E_INVALID, "afx_qkv_operands: need 1 <= batch <= %d, n_img, n_txt, heads >= 1 and a path AFX_QKV_*", AFX_MAX_MICRO_BATCH);
  const int64_t D = (int64_t)heads * 128, width = (single ? 7 : 3) * D;
  if (lda < D || ldf < width || lda % 8 || ldf % 8)
    return fail(AFX_E_INVALID, "afx_qkv_operands: need lda >= %lld, ldf >= %lld, both multiples of 8", (long long)D, (long long)width);
  if (((uintptr_t)A | (uintptr_t)w_img | (uintptr_t)b_img | (uintptr_t)w_txt | (uintptr_t)b_txt | (uintptr_t)qkn | (uintptr_t)rope_cos |
       (uintptr_t)rope_sin | (uintptr_t)F | (uintptr_t)Vt) & 15)
    return fail(AFX_E_INVALID, "afx_qkv_operands: operands must be 16-byte aligned");
  const BlockShape bs = block_shape(heads, B, N, T, rope_cos, rope_sin, (uint16_t*)Vt);
  const int p = path == AFX_QKV_AUTO ? qkv_path(bs, single, false, false) : path;
  if (p != AFX_QKV_KV_PREP && !gemm_qk_fusion_available())
    return fail(AFX_E_INVALID, "afx_qkv_operands: the GEMM kernel in use has no q / k epilogue (afx_gemm_set_mode / AFX_QK_FUSE)");
  if (p == AFX_QKV_VT_PROJ && !vt_proj_shape_ok(bs, single))
    return fail(AFX_E_INVALID, "afx_qkv_operands: V^T from the projection needs n_txt %% 16 == 0 and (n_img + n_txt) %% 64 == 0");
  hipStream_t st = (hipStream_t)stream;
  const uint16_t* a = (const uint16_t*)A;
  uint16_t* f = (uint16_t*)F;
  if (single) {
    const LinW lw{(const uint16_t*)w_img, (const uint16_t*)b_img};
    GemmBatch gb{};
    single_qkv_batch(gb, p, bs, a, lda, lw, f, ldf, qkn);
    HIP_TRY(launch_gemm(gb, st));
    HIP_TRY(qkv_finish(p, bs, f, ldf, qkn + 128, qkn + 128, qkn, qkn, st));
    return AFX_OK;
  }
  const LinW lw[2] = {{(const uint16_t*)w_img, (const uint16_t*)b_img}, {(const uint16_t*)w_txt, (const uint16_t*)b_txt}};
  if (p == AFX_QKV_VT_PROJ) {
    for (int b = 0; b < B; ++b) {
      GemmBatch gb{};
      double_vt_batch(gb, bs, a, lda, lw, f, ldf, qkn, b);
      HIP_TRY(launch_gemm(gb, st));
    }
    return AFX_OK;
  }
  GemmBatch gb{};
  for (int b = 0; b < B; ++b)
    for (int s = 0; s < 2; ++s) {
      GemmProblem& pr = gb.p[gb.nprob++];
      stream_problem(pr, bs, a, lda, (int)D, lw[s], f, ldf, (int)width, b, s);
      if (p == AFX_QKV_QK_EPI) stream_qk_epilogue(pr, bs, qkn, s);
    }
  HIP_TRY(launch_gemm(gb, st));
  HIP_TRY(qkv_finish(p, bs, f, ldf, qkn + 3 * 128, qkn + 1 * 128, qkn + 2 * 128, qkn, st));
  return AFX_OK;
}

}  // extern "C"
