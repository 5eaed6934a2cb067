/*
 * arcflow_hip.h -- C ABI of libarcflow_hip.so, the MI355X (gfx950) engine for the ArcFlow
 * 2-NFE hot path.
 *
 * The reference (pnotp/ArcFlow) has no FFI: its hot path is Python calling torch/diffusers
 * modules.  This header is the boundary a maintainer binds instead (ctypes stub in
 * INTEGRATION.md); every entry point names the reference interface it replaces
 * (paths relative to the reference repository root).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only; no torch types.
 *   - all data pointers are DEVICE pointers owned by the caller (e.g. torch tensors);
 *     the library owns only the opaque afx_ctx (weight table, workspace pointer, plan).
 *   - every call is asynchronous on the given hipStream_t (passed as void*; NULL = default
 *     stream); the library never synchronises, allocates or frees device memory.
 *   - return value: 0 on success, a negative AFX_E_* code otherwise; afx_last_error() returns
 *     a human readable message for the calling thread.  Nothing throws across the boundary.
 *   - a context is thread-compatible, not thread-safe.
 *   - bf16 tensors are raw uint16 bit patterns, row-major, innermost dimension contiguous.
 */
#ifndef ARCFLOW_HIP_H_
#define ARCFLOW_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AFX_OK 0
#define AFX_MAX_MICRO_BATCH 4  /* samples per grouped launch: afx_mmdit_forward splits larger batches itself; staged calls take <= 4 */
#define AFX_E_INVALID (-1)     /* bad argument / shape */
#define AFX_E_MISSING (-2)     /* a required weight is not bound */
#define AFX_E_WORKSPACE (-3)   /* workspace missing or too small */
#define AFX_E_HIP (-4)         /* a HIP runtime call failed */
#define AFX_E_UNSUPPORTED (-5)

#define AFX_DT_BF16 1
#define AFX_DT_F32 2
#define AFX_DT_FP8 3   /* OCP e4m3 bytes (quantised weights of the fp8 linear mode) */

typedef struct afx_ctx afx_ctx;

/* ---- model description -------------------------------------------------------------------
 * Mirrors the constructor arguments of the reference denoisers
 *   lakonlab/models/architecture/arcflow/arcflux.py:27-39   (_ArcFluxTransformer2DModel)
 *   lakonlab/models/architecture/arcflow/arcqwen.py:25-36   (_ArcQwenImageTransformer2DModel)
 */
typedef struct afx_model_desc {
  int32_t family;             /* 0 = FLUX MMDiT (double + single blocks), 1 = Qwen-Image MMDiT */
  int32_t num_double;         /* num_layers: 19 (FLUX) / 60 (Qwen) */
  int32_t num_single;         /* num_single_layers: 38 (FLUX) / 0 (Qwen) */
  int32_t heads;              /* num_attention_heads (24) */
  int32_t head_dim;           /* attention_head_dim (must be 128) */
  int32_t in_channels;        /* 64 */
  int32_t joint_dim;          /* joint_attention_dim: 4096 / 3584 */
  int32_t pooled_dim;         /* pooled_projection_dim: 768 (FLUX) / 0 (Qwen) */
  int32_t guidance_embeds;    /* 1 for FLUX.1-dev */
  int32_t num_gaussians;      /* K = 16 */
  int32_t logweights_channels;/* 4 (= patch_size^2) */
  int32_t head_mode;          /* 0 = ArcFlow 3-head student, 1 = plain proj_out teacher head */
} afx_model_desc;

const char* afx_last_error(void);
const char* afx_version(void);

/* ---- context life cycle ------------------------------------------------------------------ */
int afx_create(const afx_model_desc* desc, afx_ctx** out);
int afx_destroy(afx_ctx* ctx);

/* Bind one packed weight (device pointer stays owned by the caller and must outlive the ctx).
 * Names are the engine's packed names (arcflow_amd/weights.py builds them from the diffusers
 * state-dict keys the reference loads, lakonlab/pipelines/arcflow_loader.py:241-263):
 *   x_in.{weight,bias}  ctx_in.{weight,bias}  txt_norm.weight
 *   temb.{t,g,p}.l{1,2}.{weight,bias}
 *   mod.{weight,bias}                       all AdaLN modulation linears stacked on N
 *   d<i>.{img,txt}_{qkv,out,mlp1,mlp2}.{weight,bias}   d<i>.qknorm   (rows k|v|q in *_qkv)
 *   s<i>.{fused,out}.{weight,bias}          s<i>.qknorm              (rows k|v|q|mlp in fused)
 *   head.{weight,bias}
 *   mod_final.{weight,bias}   optional: a separately owned norm_out.linear [2D, D] that overrides the last 2D rows
 *                             of mod.* (the distillation student trains it while the teacher keeps the frozen copy)
 */
int afx_bind_weight(afx_ctx* ctx, const char* name, const void* dptr, int32_t dtype,
                    int32_t ndim, const int64_t* shape);
/* Verify every weight the description requires is bound with the right shape. */
int afx_finalize(afx_ctx* ctx);

/* Output width of the head GEMM (the stacked ArcFlow heads, padded to a multiple of 8): the N of its launch and the rows of "head.weight". */
int afx_head_width(const afx_ctx* ctx);

/* Scratch memory: size for the largest (batch, image tokens, text tokens) the ctx will see. */
int64_t afx_workspace_bytes(const afx_ctx* ctx, int32_t batch, int32_t n_img, int32_t n_txt);
int afx_set_workspace(afx_ctx* ctx, void* dptr, int64_t bytes);

/* ---- denoiser forward ---------------------------------------------------------------------
 * Replaces  transformer(hidden_states, timestep, guidance, pooled_projections,
 *                        encoder_hidden_states, txt_ids, img_ids)
 *   lakonlab/pipelines/arcflux_pipeline.py:469-479  ->  arcflux.py:134-257
 *   lakonlab/pipelines/arcqwen_pipeline.py:409-418  ->  arcqwen.py:106-174
 * x        [B, N, in_channels]      bf16  packed latents
 * ctx_emb  [B, T, joint_dim]        bf16  text-encoder states (Qwen: only the T real tokens)
 * pooled   [B, pooled_dim]          bf16  (FLUX) or NULL
 * t        [B] f32  sigma in [0,1] (the pipeline's timestep/1000);  g [B] f32 guidance or NULL.  As the reference's forward
 *          does (arcflux.py:160-162 `timestep.to(hidden_states.dtype) * 1000`, arcqwen.py:128), t and g are cast to bf16 in
 *          front of the sinusoid (FLUX: the x1000 product too -- sigma 0.76190 is embedded as 760, guidance 3.5 as 3504)
 * rope_cos/rope_sin [T+N, head_dim/2] f32 rotation tables of the joint [text; image] sequence
 *          (FluxPosEmbed / QwenEmbedRope angles; built by the host, see arcflow_amd/rope.py)
 * outputs (head_mode 0): means [B,N,K,in_channels], logw [B,N,K,lw] (log_softmax over K),
 *          logg [B,N,K-1,lw], all bf16  == ArcFlowModelOutput (arc_output.py:9-25)
 * outputs (head_mode 1): means receives the velocity [B,N,in_channels]; logw/logg unused.
 */
int afx_mmdit_forward(afx_ctx* ctx, const void* x, const void* ctx_emb, const void* pooled,
                      const float* t, const float* g, const float* rope_cos, const float* rope_sin,
                      int32_t batch, int32_t n_img, int32_t n_txt,
                      void* means, void* logw, void* logg, void* stream);

/* The conditioning of SEVERAL denoising steps in one pass.  The AdaLN modulation vectors of a forward depend only on (t, guidance,
 * pooled text) -- the reference recomputes them inside every transformer call (arcflux.py:134-257: time_text_embed, then each
 * block's norm1 / norm linear) -- and computing them means streaming the stacked modulation matrix (6.5 GB for FLUX, 1.3 ms)
 * once per forward.  A sampler knows all its timesteps up front (arcflux_pipeline.py:455-467), so:
 *   afx_mmdit_prepare_steps(ctx, pooled, t_steps [nsteps][batch] f32, g, batch, nsteps, stream)   batch <= 4, batch * nsteps <= 8
 * streams the matrix ONCE for all steps, and afx_mmdit_use_prepared_step(ctx, k) makes the NEXT afx_mmdit_forward (same batch)
 * take step k's vectors instead of recomputing them (one-shot; k = -1 cancels; the t / g / pooled arguments of that forward are
 * not looked at for the conditioning).  Results are bit-identical to the plain call.  The prepared vectors live in the workspace:
 * a new afx_set_workspace or a changed pooled / guidance needs a new prepare. */
int afx_mmdit_prepare_steps(afx_ctx* ctx, const void* pooled, const float* t_steps, const float* g, int32_t batch, int32_t nsteps,
                            void* stream);
int afx_mmdit_use_prepared_step(afx_ctx* ctx, int32_t k);

/* Gradient checkpointing (arcflux.py:181-189,315-316 checkpoint every block): when a buffer of
 * (num_double + num_single) x [B*(T+N), D] bf16 is set, afx_mmdit_forward stores every block's input token matrix
 * there; the training trunk recomputes one block at a time from it.  NULL switches it off. */
int afx_set_checkpoint_buffer(afx_ctx* ctx, void* dptr);

/* Optional instrumentation for bench.py's roofline line: when enabled, afx_mmdit_forward records a HIP
 * event pair on its stream around every GEMM launch (klass 0) and attention launch (klass 1).
 * afx_profile_read waits for the recorded events and returns the summed duration, the number of
 * launches and their algorithmic FLOPs since the last afx_profile_enable(ctx, 1).  on = N > 1 times ONE launch in N (a counter over both
 * classes; a forward has an odd number of launches, so over several forwards the sample covers every launch position): an event pair on a
 * dispatch costs ~4 us, 1.8 % of the FLUX forward when every launch carries one (round 4, profiles/r04a_no_profile_ab.txt). */
int afx_profile_enable(afx_ctx* ctx, int32_t on);
int afx_profile_read(afx_ctx* ctx, int32_t klass, double* total_ms, int64_t* launches, double* flops);

/* ---- analytic ArcFlow step, token layout --------------------------------------------------
 * Replaces _unpack_latents + _unpack_mp + ArcFlowPolicy + momentum_integration + _pack_latents
 *   lakonlab/pipelines/arcflux_pipeline.py:482-510 (:195-249), arcqwen_pipeline.py:421-451
 *   training twin: lakonlab/models/diffusions/arcflow.py:28-79
 * x_in/x_out [B,N,ch] f32 (may alias); means [B,N,K,ch]; logw [B,N,K,pp]; logg [B,N,K-1,pp]
 * (mix_dtype AFX_DT_BF16 or AFX_DT_F32); sigma_* per call scalars, or per-sample device arrays
 * sigma_vec[3*B] = {src,start,end} per sample when sigma_vec != NULL.
 *   x_out = x - D * sum_k softmax(logw)_k m_k d_k phi(g_k D),  D = sigma_start - sigma_end.
 */
int afx_arcflow_step(const float* x_in, const void* means, const void* logw, const void* logg,
                     int32_t mix_dtype, float sigma_src, float sigma_start, float sigma_end,
                     const float* sigma_vec, float eps, float* x_out,
                     int32_t batch, int32_t n_tok, int32_t K, int32_t ch, int32_t pp, void* stream);

/* u = sum_k softmax(logw)_k m_k exp(g_k (sigma_src - sigma_t))
 *   lakonlab/models/diffusions/policies/arcflow.py:52-76 */
int afx_arcflow_velocity(const void* means, const void* logw, const void* logg, int32_t mix_dtype,
                         float sigma_src, float sigma_t, const float* sigma_vec, float* u_out,
                         int32_t batch, int32_t n_tok, int32_t K, int32_t ch, int32_t pp, void* stream);

/* ---- distillation-step kernels (training side) ------------------------------------------------
 * The reference runs these as eager torch + autograd; shapes are the token layout of afx_arcflow_step. */

/* Analytic step with per-sample sigmas sigma_vec[3*B] = {src,start,end} and GM dropout: component k of
 * sample b is removed (log-weight -> -inf) when drop_mask[b*K+k] != 0 (policies/arcflow.py:96-106);
 * roll-outs of the detached policy in piid_segment_momentum (arcflow.py:141-144,176-178,201-205). */
int afx_arcflow_step_dropout(const float* x_in, const void* means, const void* logw, const void* logg,
                             int32_t mix_dtype, const float* sigma_vec, const uint8_t* drop_mask, float eps,
                             float* x_out, int32_t batch, int32_t n_tok, int32_t K, int32_t ch, int32_t pp,
                             void* stream);

/* Gradients of D = sum_k softmax(logw)_k m_k e_k w.r.t. (means, logw, logg) given gD = gscale * gscale_vec[b] * g:
 * step form (velocity_only = 0): e_0 = Dt, e_k = exp(g_k Dp) Dt phi(g_k Dt)  -- x_end = x - D
 * velocity form (1):             e_0 = 1,  e_k = exp(g_k Dp)                  -- u = D
 * = autograd of policy_average_u_momentum (arcflow.py:81-110).  accumulate != 0 adds into the outputs.
 * d_means [B,N,K,ch], d_logw [B,N,K,pp], d_logg [B,N,K-1,pp] fp32.  ch <= 64, pp power of two. */
int afx_arcflow_backward(const float* g, const void* means, const void* logw, const void* logg, int32_t mix_dtype,
                         float sigma_src, float sigma_start, float sigma_end, const float* sigma_vec,
                         const float* gscale_vec, float gscale, float eps, float* d_means, float* d_logw,
                         float* d_logg, int32_t batch, int32_t n_tok, int32_t K, int32_t ch, int32_t pp,
                         int32_t velocity_only, int32_t accumulate, void* stream);

/* *loss_accum += coef * 0.5 * sum (pred-target)^2 ; grad (optional) = coef * (pred-target)
 * (DiffusionMSELoss, losses/diffusion_loss.py:44-83; coef folds the x30 rescale, the mean and the segment size) */
int afx_mse_loss(const float* pred, const float* target, float coef, float* grad, float* loss_accum, int64_t n,
                 void* stream);
/* x_out = x_a + u * (sigma_b[b] - sigma_a[b])   teacher Euler roll (arcflow.py:189-192) */
int afx_euler_roll(const float* x_a, const float* u, const float* sigma_a, const float* sigma_b, float* out,
                   int32_t batch, int64_t per_sample, void* stream);
/* xt = x0 * (1 - sigma[b]) + noise * sigma[b] (fp32), with x0 the cached latents [B,C,H,W] and noise / xt in the engine's token
 * layout [B, (H/2)(W/2), 4C], channel = c*4 + ph*2 + pw: the patchify of latent_diffusion_text_image.py:51 and the forward
 * diffusion of the data-based trainer (gaussian_flow.py:83-88, called at arcflow.py:321-322) in one pass.  xt_bf16 (may be NULL)
 * receives the round-to-nearest-even bf16 copy the engine reads.  4C must be 64, H and W even; x0 8-byte, the others 16-byte aligned. */
int afx_forward_diffuse_pack(const float* x0, const float* noise, const float* sigma, float* xt_f32, void* xt_bf16,
                             int32_t B, int32_t C, int32_t H, int32_t W, void* stream);
/* out = alpha[b] * a + beta[b] * b, per-sample scalars: mean velocity (x_a - x_e) / (sigma_a - sigma_e) and the
 * short/long roll-out select of policy_average_u_momentum (arcflow.py:92-110) */
int afx_axpby_rows(const float* a, const float* alpha, const float* b, const float* beta, float* out, int32_t batch,
                   int64_t per_sample, void* stream);
/* out = pos + (pos - neg) * (scale - 1)   teacher CFG (gaussian_flow.py:18-26, orthogonal=False) */
int afx_cfg_combine(const float* pos, const float* neg, float scale, float* out, int64_t n, void* stream);

/* One step of the teacher's Euler ODE sampler (GaussianFlow.forward_test, gaussian_flow.py:196-215) on the engine's packed
 * token layout: true-CFG combine (guidance_jit, gaussian_flow.py:18-26) + FlowEulerODEScheduler.step, prediction_type 'u'
 * (schedulers/flow_euler_ode.py:141-150) + the bf16 copy of the new latents that the next forward reads, in one launch.
 *   bias  = (pos - neg) (scale - 1)                  (0 when neg is NULL: no guidance on this step)
 *   u     = pos + bias - coef[b] pos                 (coef NULL: no orthogonal term)
 *   x_out = x + u (sigma_to[b] - sigma[b])           all in fp32
 * x, x_out [batch, n] fp32 (x_out may alias x); pos, neg [batch, n] bf16 teacher velocities; sigma, sigma_to, coef [batch] fp32;
 * x_out_bf16 [batch, n] = round-to-nearest-even of x_out.  n = tokens x channels must be a multiple of 64 and every tensor
 * 16-byte aligned, else AFX_E_INVALID.  max_blocks: cap on the grid of the grid-stride loop (0 = the default, 2048). */
int afx_teacher_euler_step(const float* x, const void* pos, const void* neg, const float* sigma, const float* sigma_to,
                           const float* coef, float scale, float* x_out, void* x_out_bf16, int32_t batch, int64_t n,
                           int32_t max_blocks, void* stream);
/* One step of the teacher's stochastic sampler (FlowSDEScheduler.step, prediction_type 'u', schedulers/flow_sde.py:143-166) with the
 * same operands, layout and CFG combine as afx_teacher_euler_step, in one launch:
 *   u     = pos + (pos - neg) (scale - 1) - coef[b] pos          exactly as afx_teacher_euler_step forms it
 *   x0    = x - sigma[b] u,    e = x + (1 - sigma[b]) u
 *   x_out = (1 - sigma_to[b]) x0 + sigma_to[b] (m[b] e + c_noise[b] noise)          all in fp32
 * m, c_noise [batch] fp32: the scheduler's mixing weight (sigma_to alpha / (sigma alpha_to))^(h^2) and sqrt(max(1 - m^2, 0)), computed
 * on the host (FlowSDEScheduler.coefficients); m = 1, c_noise = 0 is the ODE step.  noise [batch, n] fp32 N(0, 1) draws, 16-byte
 * aligned; NULL skips the noise term and its read (every sample's sigma_to c_noise is 0, as on the final step).  neg, coef, x_out
 * aliasing x, x_out_bf16, n, alignment and max_blocks as for afx_teacher_euler_step.  Traffic at 1024 x 1024 (262144 elements per
 * image): 4 + 2 + 2 + 4 B read and 4 + 2 B written per element, about 4.7 MB per image and step. */
int afx_teacher_sde_step(const float* x, const void* pos, const void* neg, const float* noise, const float* sigma,
                         const float* sigma_to, const float* m, const float* c_noise, const float* coef, float scale, float* x_out,
                         void* x_out_bf16, int32_t batch, int64_t n, int32_t max_blocks, void* stream);
/* One step of the teacher's UniPC multistep sampler (FlowUniPCScheduler: the predictor-corrector solver behind the reference's
 * FlowAdapterScheduler on its default base scheduler, schedulers/flow_adapter.py; the multistep arithmetic is diffusers' as recalled and
 * no fixture pins it) with the same operands, layout and CFG combine as afx_teacher_euler_step, in one launch.  The host evaluates the
 * solver's scalars in fp64 (FlowUniPCScheduler.coefficients) and passes one fp32 weight per operand and sample, w [10, batch], rows
 *   0 s | 1 c_last  2 c_mt  3 c_1  4 c_2  5 c_3 | 6 p_xc  7 p_mt  8 p_1  9 p_2.
 * Per element, in fp32, every product-sum one fused multiply-add in exactly this order:
 *   u      = pos + (pos - neg) (scale - 1) - coef[b] pos          exactly as afx_teacher_euler_step forms it
 *   m_t    = fma(-s, u, x)                                         the clean-sample prediction x - s u
 *   x_c    = fma(c_mt, m_t, fma(c_3, h3, fma(c_2, h2, fma(c_1, h1, c_last last))))      the corrector; last NULL: x_c = x
 *   x_next = fma(p_mt, m_t, fma(p_2, h2, fma(p_1, h1, p_xc x_c)))                        the predictor
 * last [batch, n] fp32: the corrected sample the previous step wrote (NULL on the first step of a roll: no corrector); h1, h2, h3
 * [batch, n] fp32: the m_t of one, two and three steps ago, NULL when the step's orders do not reach them -- a NULL operand is neither
 * read nor multiplied.  last needs h1, h2 needs h1, h3 needs h2.  Outputs: x_out = x_next (may be x), x_out_bf16 = its
 * round-to-nearest-even bf16 copy, last_out = x_c (may be last), hist_out = m_t (may be h1, h2 or h3 itself: the caller rotates a ring
 * of solver_order buffers and overwrites the oldest).  With p_xc = 0, p_mt = 1, p_1 = p_2 = 0 (the step that lands on sigma 0)
 * x_next = m_t bit for bit for finite operands.  AFX_E_INVALID before any launch when a required pointer is NULL (all but neg, last,
 * h1, h2, h3, coef), n is not a positive multiple of 64, batch or max_blocks < 0, a tensor is not 16-byte aligned, or an output
 * overlaps another operand other than by the three aliases above.  max_blocks: cap on the grid of the grid-stride loop (0 = the
 * default, 2048).  Traffic at 1024 x 1024 (262144 elements per image) at order 2: 4 + 2 + 2 + 4 + 4 + 4 = 20 B read and 4 + 2 + 4 + 4 =
 * 14 B written per element, about 8.9 MB per image and step. */
int afx_teacher_unipc_step(const float* x, const void* pos, const void* neg, const float* w, const float* last, const float* h1,
                           const float* h2, const float* h3, const float* coef, float scale, float* x_out, void* x_out_bf16, float* last_out,
                           float* hist_out, int32_t batch, int64_t n, int32_t max_blocks, void* stream);
/* The blend of image editing (image-to-image start, inpainting) on the engine's packed token layout, in one launch: the source
 * latents x0 diffused forward to sigma_to with the call's fixed noise, blended per latent pixel with the sampler's latents x, plus the
 * bf16 copy the next forward reads.  Per element, in fp32, exactly:
 *   om    = 1 - sigma_to[b]
 *   known = noise ? fma(sigma_to[b], noise, om x0) : om x0
 *   x_out = mask ? fma(m, x, (1 - m) known) : known                     m = mask[b, tok, e & 3] for element e of the token
 *   x_out_bf16 = round-to-nearest-even of x_out
 * so that, for finite inputs, m = 1 returns x, m = 0 returns known, sigma_to = 1 returns noise and sigma_to = 0 returns x0 bit for bit.
 * x, x0, noise, x_out [batch, n_tok, ch] fp32, x_out_bf16 [batch, n_tok, ch] bf16, ch = 64 with channel = c*4 + ph*2 + pw; mask
 * [batch, n_tok, 4] fp32 in [0, 1], one value per latent pixel of the 2 x 2 patch at index ph*2 + pw (1 = keep x, 0 = keep the source);
 * sigma_to [batch] fp32.  mask NULL: everything is known (the image-to-image start: the noised source and its bf16 copy in one launch);
 * x is then not read and may be NULL.  noise NULL: the noise term and its read are skipped (the final step, sigma_to = 0).  x_out may
 * be x; x_out_bf16 may be NULL.  AFX_E_INVALID before any launch when x0, x_out or sigma_to is NULL, x is NULL with a mask, ch != 64,
 * batch or n_tok < 1, a pointer is not 16-byte aligned, or an output overlaps another operand (other than x_out == x).  max_blocks: cap
 * on the grid of the grid-stride loop (0 = the default, 2048).  Traffic at 1024 x 1024 (262144 elements per image): 4 + 4 + 4 B read and
 * 4 + 2 B written per element, 16 B of mask per token: 18 B per element, about 4.7 MB per image and step. */
int afx_edit_blend(const float* x, const float* x0, const float* noise, const float* mask, const float* sigma_to, float* x_out,
                   void* x_out_bf16, int32_t batch, int32_t n_tok, int32_t ch, int32_t max_blocks, void* stream);
/* One step of teacher image editing (image-to-image / inpainting with the many-step sampler): afx_teacher_euler_step /
 * afx_teacher_sde_step and the re-imposition of the known region at the sigma the step lands on, in one launch.  Per element, in fp32:
 *   x'    = the Euler / FlowSDE update with the CFG combine, exactly as afx_teacher_euler_step / afx_teacher_sde_step compute it
 *   om    = 1 - sigma_to[b]
 *   known = noise0 ? fma(sigma_to[b], noise0, om x0) : om x0
 *   x_out = fma(m, x', (1 - m) known)                                 m = mask[b, tok, e & 3] for element e of the token
 *   x_out_bf16 = round-to-nearest-even of x_out
 * so x_out and x_out_bf16 are, bit for bit, those of the step entry followed by afx_edit_blend(x', x0, noise0, mask, sigma_to): m = 1
 * returns the plain step, m = 0 returns known, and m = 0 with sigma_to = 0 returns x0 (finite inputs).  x0 [batch, n_tok, ch] fp32: the
 * packed source latents; noise0 [batch, n_tok, ch] fp32: the START noise of the edit on every step (never the FlowSDE draw `noise`), NULL on
 * the step whose sigma_to is 0 (the term and its read are skipped); mask [batch, n_tok, 4] fp32 in [0, 1] as for afx_edit_blend (1 =
 * repaint, 0 = keep the source), NULL: nothing is re-imposed and the call IS the plain step entry (same kernel, same bits; x0 and noise0
 * are then not read).  Every other operand as for the step entries with n = n_tok * ch.  These semantics follow the image-to-image /
 * inpainting pipelines of diffusers as recalled; the reference has no image-conditioned sampling, so no fixture pins them.
 * AFX_E_INVALID before any launch when a required pointer is NULL (all but neg, noise, coef, noise0, mask), ch != 64, batch or n_tok < 1,
 * max_blocks < 0, a tensor is not 16-byte aligned, or an output overlaps another operand (other than x_out == x).  max_blocks: cap on
 * the grid of the grid-stride loop (0 = the default, 2048).  Traffic at 1024 x 1024 (262144 elements per image): 4 + 2 + 2 + 4 + 4 B read
 * (+ 4 B of `noise` for FlowSDE), 16 B of mask per token, 4 + 2 B written: 22.25 B per element (26.25 B), about 5.8 MB (6.9 MB) per image
 * and step.  The two launches it replaces move 14 (18) + 18.25 B: fused saves one fp32 write + read of x', one bf16 write and a launch. */
int afx_teacher_edit_step(const float* x, const void* pos, const void* neg, const float* sigma, const float* sigma_to, const float* coef,
                          float scale, const float* x0, const float* noise0, const float* mask, float* x_out, void* x_out_bf16,
                          int32_t batch, int32_t n_tok, int32_t ch, int32_t max_blocks, void* stream);
int afx_teacher_sde_edit_step(const float* x, const void* pos, const void* neg, const float* noise, const float* sigma, const float* sigma_to,
                              const float* m, const float* c_noise, const float* coef, float scale, const float* x0, const float* noise0,
                              const float* mask, float* x_out, void* x_out_bf16, int32_t batch, int32_t n_tok, int32_t ch, int32_t max_blocks,
                              void* stream);
/* coef[b] = mean(bias pos) / max(mean(pos pos), 1e-6) over the n elements of sample b, bias = (pos - neg) (scale - 1) rounded to
 * fp32 as the step kernel computes it: the projection coefficient of orthogonal guidance (gaussian_flow.py:21-25, dim = [1..]).
 * Deterministic: a number of work-groups per sample that depends on n alone, exact fp64 products, one slot of `ws` per
 * work-group, the slots added in index order by a second launch; no atomics.  ws: afx_cfg_ortho_ws_bytes(batch, n) bytes,
 * 8-byte aligned, private to the call until it completes.  n a multiple of 64, pos / neg 16-byte aligned. */
int64_t afx_cfg_ortho_ws_bytes(int32_t batch, int64_t n);
int afx_cfg_ortho_coef(const void* pos, const void* neg, float scale, float* coef, void* ws, int64_t ws_bytes, int32_t batch,
                       int64_t n, void* stream);
/* Per-sample agreement sums of two batches (training-time evaluation: student samples a against teacher samples b):
 *   out[s] = { sum (a-b)^2, sum a^2, sum b^2, sum a b }  over the n elements of sample s, as fp64.
 * a, b [batch, n], both `dtype` (AFX_DT_BF16 or AFX_DT_F32), 16-byte aligned; n a positive multiple of 64; out [batch, 4] fp64.
 * transform 0: the values as they are (packed latents).  transform 1: clamp(v / 2 + 0.5, 0, 1) in fp32 on both operands before
 * anything else -- the image range of the reference's val_step, so decoded images are scored in [0, 1].
 * Every element is widened to fp64 after the transform; differences, products and sums are fp64.  Deterministic on the scheme of
 * afx_cfg_ortho_coef: min(64, ceil(n / 8192)) work-groups per sample (a function of n alone), one slot of 4 doubles of `ws` per
 * work-group, the slots added in index order by a second launch; no atomics, bit-reproducible.  ws: afx_sample_score_ws_bytes(batch,
 * n) bytes, 8-byte aligned, private to the call until it completes.  Traffic: 2 x 2 B (bf16) or 2 x 4 B (fp32) read per element,
 * 32 B written per work-group and per sample: 1 MB per 1024 x 1024 latent pair in bf16 (262144 elements), 12.6 MB per decoded
 * 3 x 1024 x 1024 bf16 image pair. */
int64_t afx_sample_score_ws_bytes(int32_t batch, int64_t n);
int afx_sample_score(const void* a, const void* b, int32_t dtype, int32_t transform, double* out, void* ws, int64_t ws_bytes,
                     int32_t batch, int64_t n, void* stream);
/* Structural similarity of two image batches (training-time evaluation: decoded student images a against teacher images b), Wang et al.
 * 2004 in the common "Gaussian, valid" form:
 *   out[s] = sum over the C channels and the (H - 10)(W - 10) windows of each of
 *            (2 mu_a mu_b + c1)(2 s_ab + c2) / ((mu_a^2 + mu_b^2 + c1)(s_aa + s_bb + c2)),        as fp64;
 * the mean SSIM of sample s is out[s] / (C (H - 10)(W - 10)).  The window is g g^T with g[i] = exp(-(i - 5)^2 / (2 1.5^2)), i = 0..10,
 * normalised to sum 1 in fp64; only windows that lie fully inside the image count.  mu are the weighted means, s_aa = E[a^2] - mu_a^2,
 * s_bb likewise, s_ab = E[a b] - mu_a mu_b (weighted, biased); c1 = (0.01 data_range)^2, c2 = (0.03 data_range)^2.
 * a, b [batch, C, H, W] contiguous, both `dtype` (AFX_DT_BF16 or AFX_DT_F32), aligned to their element; H, W >= 11; batch, C >= 1.
 * transform as in afx_sample_score: 0 the values as they are, 1 clamp(v / 2 + 0.5, 0, 1) in fp32 first.  Every element is widened to
 * fp64 after the transform; both 11-tap passes, the moments and the ratio are fp64, and the three second moments are formed by the same
 * sequence of operations: a == b gives exactly 1.0 per window, i.e. out[s] == C (H - 10)(W - 10).  The values are expected in (about)
 * [0, data_range]: the denominators are positive then.
 * Deterministic on the scheme of afx_sample_score: one work-group per tile of 32 x 16 windows and channel (a function of the shape
 * alone), one fp64 slot of `ws` per work-group, the slots of a sample added in a fixed order by a second launch (lane l of one wave adds
 * the slots l, l + 64, ... in index order, then the 64 lanes by the shuffle tree); no atomics, bit-reproducible.
 * ws: afx_image_ssim_ws_bytes(batch, C, H, W) = 8 batch C ceil((H - 10) / 16) ceil((W - 10) / 32) bytes, 8-byte aligned, private to the
 * call until it completes.  Traffic: every element of a and b is read once from memory (and up to 42 x 26 / (32 x 16) = 2.1 times through the
 * caches: a tile reads its 10-wide apron), 8 B written per tile: 25.2 MB per decoded 3 x 1024 x 1024 fp32 image pair (12.6 MB in bf16), 49 KB
 * of slots. */
int64_t afx_image_ssim_ws_bytes(int32_t batch, int32_t C, int32_t H, int32_t W);
int afx_image_ssim(const void* a, const void* b, int32_t dtype, int32_t transform, double data_range, double* out, void* ws,
                   int64_t ws_bytes, int32_t batch, int32_t C, int32_t H, int32_t W, void* stream);
/* afx_sample_score weighted by an edit's mask (training-time evaluation of edits: does the student repaint the masked region the way the
 * teacher does?).  a, b [batch, n] as afx_sample_score takes them, n = G P R, viewed as [batch, G, P, R]; mask [mask_batch, P, Q] fp32
 * weights in [0, 1], mask_batch 1 (shared by the batch) or batch, Q a divisor of R: element (s, g, p, r) takes the weight
 * m[s, p, r % Q].  Packed latents [batch, N, 64] with the [batch, N, 4] mask of afx_edit_blend: G = 1, P = N, R = 64, Q = 4 (element e
 * of a token reads m[token, e & 3], that kernel's map).  Decoded images [batch, C, H, W] with a [batch, 1, H, W] mask: G = C, P = H W,
 * R = Q = 1.
 *   out[s][0] = { sum w, sum w (a-b)^2, sum w a^2, sum w b^2, sum w a b },  w = m          the repainted region
 *   out[s][1] = the same with w = 1 - m (formed in fp64)                                   the kept region
 * out [batch, 2, 5] fp64.  transform as in afx_sample_score.  w is widened to fp64; the difference, the squares and the product are
 * afx_sample_score's, then weighted; the partition is afx_sample_score's, min(64, ceil(n / 8192)) work-groups per sample, one slot of
 * 10 doubles each, added in index order by a second launch: no atomics, bit-reproducible, and with m = 1 everywhere out[s][0][1..4]
 * equals afx_sample_score's out[s] bit for bit while out[s][1] is exactly 0.
 * n a positive multiple of 64 below 2^31; a, b 16-byte aligned, mask 4-byte, out and ws 8-byte.  ws: afx_sample_score_masked_ws_bytes(
 * batch, n) bytes, private to the call until it completes.  Every refusal precedes the first launch: out is untouched then. */
int64_t afx_sample_score_masked_ws_bytes(int32_t batch, int64_t n);
int afx_sample_score_masked(const void* a, const void* b, const float* mask, int32_t dtype, int32_t transform, double* out, void* ws,
                            int64_t ws_bytes, int32_t batch, int32_t mask_batch, int32_t G, int32_t P, int32_t R, int32_t Q, void* stream);
/* afx_image_ssim weighted by an edit's mask.  a, b, dtype, transform, data_range, the window and the ratio are afx_image_ssim's (a == b
 * gives exactly 1.0 per window).  mask [mask_batch, 1, H, W] fp32 in [0, 1], mask_batch 1 or batch, shared by the C channels.  The
 * weight w of a window is the Gaussian-weighted mean of the mask over the window's own 11 x 11 support (the same two 11-tap passes),
 * clamped to [0, 1] in fp64.
 *   out[s] = { sum w ssim, sum w, sum (1 - w) ssim, sum (1 - w) }  over the C channels and the (H - 10)(W - 10) windows of each, fp64:
 * out[s][0] / out[s][1] is the mean SSIM of the repainted region, out[s][2] / out[s][3] that of the kept region.
 * Deterministic on the scheme of afx_image_ssim: the same tiles, one slot of 4 doubles of `ws` per work-group, each sum added in that
 * entry's fixed order by a second launch.  ws: afx_image_ssim_masked_ws_bytes(batch, C, H, W) = 4 x afx_image_ssim_ws_bytes bytes,
 * 8-byte aligned, private to the call until it completes.  Every refusal precedes the first launch: out is untouched then. */
int64_t afx_image_ssim_masked_ws_bytes(int32_t batch, int32_t C, int32_t H, int32_t W);
int afx_image_ssim_masked(const void* a, const void* b, const float* mask, int32_t dtype, int32_t transform, double data_range, double* out,
                          void* ws, int64_t ws_bytes, int32_t batch, int32_t mask_batch, int32_t C, int32_t H, int32_t W, void* stream);
/* Image resampling for the edit pipelines: resize, crop and Gaussian mask feathering are one table-driven separable operation,
 *   out[i] = sum_{k < count[i]} w[i, k] in[start[i] + k]        per axis, horizontally first, then vertically, fp32 fma in tap order.
 * afx_resample_table is a HOST function on HOST arrays (no GPU needed): it builds one axis' table in fp64, rounds the weights to fp32 once
 * and returns the tap count (the largest count[i]), or a negative AFX_E_* code.  start, count [n_out] int32, w [n_out, max_taps] fp32 with
 * row stride max_taps (entries past count[i] are written as 0); all three NULL only asks for the tap count.
 *   AFX_FILTER_LANCZOS3 (a = 3) / AFX_FILTER_TRIANGLE (a = 1): the rule of Pillow's Image.resize(size, resample, box) along one axis with
 *   box [b0, b1) in source pixels, 0 <= b0 < b1 <= n_in, fractional allowed:
 *     scale = (b1 - b0) / n_out, fs = max(scale, 1), support = a fs, c = b0 + (i + 0.5) scale,
 *     lo = max(0, int(c - support + 0.5)), hi = min(n_in, int(c + support + 0.5)), w_k = f((k + lo - c + 0.5) / fs) / sum.
 *   sin(pi x) / (pi x) is taken as exactly 0 at the non-zero integers, so a same-size table is exactly the identity.  sigma is ignored.
 *   AFX_FILTER_GAUSSIAN: n_out == n_in, b0 / b1 ignored, taps exp(-d^2 / (2 sigma^2)) for |d| <= ceil(3 sigma), the window clipped at the
 *   border and renormalised there (an edge pixel is a weighted mean of the pixels that exist; nothing is padded or reflected).
 * AFX_E_UNSUPPORTED when a window needs more than AFX_RESAMPLE_MAX_TAPS taps (a 16x Lanczos-3 downscale takes 95), AFX_E_INVALID when it
 * needs more than max_taps, for a bad size, filter, box or sigma (sigma and sigma^2 must be positive and finite), for weights whose sum is zero
 * or not finite, or when only some of start / count / w are NULL.
 * afx_image_resample: src uint8 [batch, H_in, W_in, C] (src_u8 = 1; a byte x is read as the IEEE fp32 quotient float(x) / 255.0f) or fp32
 * [batch, C, H_in, W_in] (src_u8 = 0), C 1 or 3; dst fp32 [batch, C, H_out, W_out]; h_* the table of the W axis (n_out = W_out, row stride
 * h_taps), v_* that of the H axis (n_out = H_out, row stride v_taps), all DEVICE pointers; clamp 1: dst is clamped to [0, 1] (Lanczos
 * overshoots).  ws: afx_image_resample_ws_bytes(batch, C, H_in, W_out) = 4 batch C H_in W_out bytes, the fp32 horizontal result, private to
 * the call until it completes.  Two launches.  Every source index is clamped into the source and count[i] is capped at the row stride
 * before any load: a bad table gives wrong pixels, never a read outside src.  AFX_E_INVALID before any launch for a NULL src, dst or
 * table, C outside {1, 3}, a size < 1, taps outside [1, AFX_RESAMPLE_MAX_TAPS], a misaligned pointer (4 bytes; a uint8 src: none), or dst
 * or ws overlapping the source, a table or each other; AFX_E_WORKSPACE for a NULL or short ws. */
#define AFX_RESAMPLE_MAX_TAPS 128
#define AFX_FILTER_LANCZOS3 0
#define AFX_FILTER_TRIANGLE 1
#define AFX_FILTER_GAUSSIAN 2
int afx_resample_table(int32_t n_in, int32_t n_out, int32_t filter, double b0, double b1, double sigma, int32_t* start, int32_t* count,
                       float* w, int32_t max_taps);
int64_t afx_image_resample_ws_bytes(int32_t batch, int32_t C, int32_t H_in, int32_t W_out);
int afx_image_resample(const void* src, int32_t src_u8, int32_t batch, int32_t C, int32_t H_in, int32_t W_in, const int32_t* h_start,
                       const int32_t* h_count, const float* h_w, int32_t h_taps, const int32_t* v_start, const int32_t* v_count,
                       const float* v_w, int32_t v_taps, float* dst, int32_t H_out, int32_t W_out, int32_t clamp, void* ws,
                       int64_t ws_bytes, void* stream);
/* The way back from an edit that ran on a window of a larger photo (the pipelines' padding_mask_crop).
 * afx_mask_bbox: mask uint8 [batch, H, W, 1] (mask_u8 = 1) or fp32 [batch, 1, H, W] -> bbox int32 [batch, 4] = (x0, y0, x1, y1), the half-open
 * bounding box of the pixels with m > 0 (a NaN is not, a positive denormal and +inf are); an image without such a pixel gives (W, H, 0, 0).
 * Integer min / max atomics: the result does not depend on arrival order.  Two launches, all on the device.  AFX_E_INVALID before any
 * launch for a NULL or misaligned (4 bytes; a uint8 mask: none) pointer, a size < 1, batch > 65535, or bbox overlapping the mask.
 * afx_image_paste: img fp32 [batch, 3, h, w] in [-1, 1] (the decoder's output), mask fp32 [mask_batch, 1, h, w] in [0, 1] (mask_batch 1 =
 * shared, or batch) or NULL (mask_batch 0: m = 1 inside the window), src and dst uint8 [batch, H, W, 3], the integer window (x0, y0, x1, y1)
 * inside the source.  ih_* / iv_* are the image's afx_resample_table tables of the W axis (w -> x1 - x0, n_out_w rows of stride ih_taps) and
 * of the H axis (h -> y1 - y0, n_out_h rows), mh_* / mv_* the mask's (same n_out; ignored without a mask), all DEVICE pointers.  Every byte
 * of dst is written: outside the window src's three bytes; inside, per channel,
 *     v = vertical taps of the horizontal taps of img (fp32 fma in tap order, as afx_image_resample), p = fma(0.5, v, 0.5),
 *     m = clamp(the same taps of mask, 0, 1), s = float(byte) / 255.0f, r = fma(m, p, (1 - m) s), byte' = rint(255 clamp(r, 0, 1)), ties to even;
 * where m == 0 src's bytes are stored as they are, and nothing of img (a NaN included) reaches them.  ws: afx_image_paste_ws_bytes(batch,
 * mask_batch, h, x1 - x0) = 4 (3 batch + mask_batch) h (x1 - x0) bytes, the horizontal results, private to the call until it completes.
 * Two launches, three with a mask.  Indices are clamped and counts capped as in afx_image_resample.  AFX_E_INVALID before any launch for a
 * NULL img, src, dst or image table (with a mask: a mask table), a size < 1, a mask_batch other than 0 / 1 / batch, a window that is empty,
 * not inside the source or not n_out_w x n_out_h, taps outside [1, AFX_RESAMPLE_MAX_TAPS], a misaligned fp32 pointer (4 bytes), or dst or ws
 * overlapping an operand, a table or each other; AFX_E_WORKSPACE for a NULL or short ws. */
int afx_mask_bbox(const void* mask, int32_t mask_u8, int32_t batch, int32_t H, int32_t W, int32_t* bbox, void* stream);
int64_t afx_image_paste_ws_bytes(int32_t batch, int32_t mask_batch, int32_t h, int32_t win_w);
int afx_image_paste(const float* img, const float* mask, int32_t mask_batch, const void* src, void* dst, int32_t batch, int32_t h, int32_t w,
                    int32_t H, int32_t W, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t n_out_w, int32_t n_out_h,
                    const int32_t* ih_start, const int32_t* ih_count, const float* ih_w, int32_t ih_taps, const int32_t* iv_start,
                    const int32_t* iv_count, const float* iv_w, int32_t iv_taps, const int32_t* mh_start, const int32_t* mh_count,
                    const float* mh_w, int32_t mh_taps, const int32_t* mv_start, const int32_t* mv_count, const float* mv_w, int32_t mv_taps,
                    void* ws, int64_t ws_bytes, void* stream);
/* Tiled image-to-image (the pipelines' enhance): a canvas of any size is cut into ky x kx overlapping th x tw tiles with their corners at
 * (oy[iy], ox[ix]), tile index iy * kx + ix, each tile is edited on its own, and the decoded tiles are cross-faded back into bytes.
 * oy [ky] and ox [kx] int32, and the axes' tables y_* (H rows) and x_* (W rows) -- start, count [n] int32, w [n, taps] fp32, the tiles
 * start[i] .. start[i] + count[i] - 1 cover pixel i with the weights w[i, :], which sum to 1 -- are DEVICE pointers (host side:
 * arcflow_amd.schedule.tile_plan).  th and tw are multiples of 16.
 * afx_tiles_cut: canvas fp32 [3, H, W] -> tiles fp32 [ky kx, 3, th, tw], values copied bit for bit; 16-byte stores, and 16-byte loads where
 * the source address allows (else four 4-byte loads).  An origin is clamped into [0, H - th] / [0, W - tw] before any load.  One launch.
 * afx_tiles_merge: tiles fp32 [T, 3, th, tw] in the decoder's range [-1, 1] -> dst uint8 [H, W, 3] (the layout afx_image_paste writes), per
 * pixel and channel in fp32, taps in ascending order, rows outer and columns inner, v_ab the value of tile (y_start[y] + a, x_start[x] + b):
 *     acc = sum_a y_w[y, a] ( sum_b x_w[x, b] fma(0.5, v_ab, 0.5) )   (both sums by fma from 0),   byte = rint(255 clamp(acc, 0, 1)), ties to even.
 * No atomics and no accumulator canvas: the same bits on every run.  Every byte of dst is written.  Tile indices and in-tile coordinates
 * are clamped and counts capped at the taps before any load: a bad table gives wrong pixels, never a read outside tiles.  One launch.
 * AFX_E_INVALID before any launch for a NULL pointer, a misaligned one (4 bytes; afx_tiles_cut's tiles: 16), a size < 1, th or tw no
 * multiple of 16 or larger than the canvas, T != ky kx, taps outside [1, AFX_TILE_MAX_TAPS], or an output that overlaps an operand. */
#define AFX_TILE_MAX_TAPS 4
int afx_tiles_cut(const float* canvas, int32_t H, int32_t W, const int32_t* oy, int32_t ky, const int32_t* ox, int32_t kx, int32_t th,
                  int32_t tw, float* tiles, void* stream);
int afx_tiles_merge(const float* tiles, int32_t T, int32_t th, int32_t tw, const int32_t* oy, int32_t ky, const int32_t* ox, int32_t kx,
                    const int32_t* y_start, const int32_t* y_count, const float* y_w, int32_t y_taps, const int32_t* x_start,
                    const int32_t* x_count, const float* x_w, int32_t x_taps, void* dst, int32_t H, int32_t W, void* stream);
/* Outpainting (the pipelines' outpaint): the photo on a larger canvas, and the mask state that the windows of
 * arcflow_amd.schedule.outpaint_plan work through one after the other.
 * afx_canvas_extend: src uint8 [batch, H, W, 3], extents left, top, right, bottom >= 0 (one of them > 0) -> canvas uint8 [batch, Hc, Wc, 3]
 * with Hc = H + top + bottom, Wc = W + left + right, and mask fp32 [Hc, Wc], both in one launch.  Canvas pixel (y, x) is the photo's pixel
 * (iy(y - top), ix(x - left)), a bit copy; inside the photo's rectangle the canvas is the photo.  Along an axis of n pixels,
 *     AFX_FILL_EDGE:     the index is clamp(i, 0, n - 1);
 *     AFX_FILL_REFLECT:  with p = 2 (n - 1), j = ((i mod p) + p) mod p, the index is j if j < n, else p - j; 0 for n == 1
 * (numpy's pad modes 'edge' and 'reflect', for pads of any length).  The mask is 1 outside the photo's rectangle and ramp(d) inside it,
 *     ramp(d) = max(0, 1 - (d + 1) / (blend + 1)),   in fp32: 1.0f - float(d + 1) / float(blend + 1), an IEEE quotient,
 * d the pixel's distance to the nearest side of the rectangle whose extent is > 0 (0 on the side itself): `blend` pixels inside every
 * extended side are partly repainted, blend = 0 gives a binary mask.
 * afx_canvas_mark: mask[y, x] = min(mask[y, x], ramp(d)) in place for the pixels of the integer window (x0, y0, x1, y1) of mask fp32
 * [Hc, Wc], d the distance to the nearest window side that does not lie on the canvas border (none: the window's area becomes 0).  No
 * pixel outside the window is read or written.  The state only decreases, so it does not depend on the order of the marks.  One launch.
 * AFX_E_INVALID before any launch for a NULL pointer, batch, H, W, Hc or Wc < 1, an unknown fill, a negative extent or extents that are
 * all 0, blend < 0, a window that is empty or not inside the canvas, a mask that is not 4-byte aligned, canvas overlapping src, mask
 * overlapping either, or a canvas past the grid's index range (a side above 2^31 - 1, batch Hc Wc above 2^59). */
#define AFX_FILL_EDGE 0
#define AFX_FILL_REFLECT 1
int afx_canvas_extend(const void* src, int32_t batch, int32_t H, int32_t W, int32_t left, int32_t top, int32_t right, int32_t bottom,
                      int32_t fill, int32_t blend, void* canvas, float* mask, void* stream);
int afx_canvas_mark(float* mask, int32_t Hc, int32_t Wc, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t blend, void* stream);
/* Colour matching of a decoded edit to the picture it was made from (the pipelines' color_fix=; "wavelet" and "AdaIN" colour fix of tile
 * upscalers: StableSR's wavelet_reconstruction and adaptive_instance_normalization restated as recalled, parity unpinned).
 * edit e [batch, C, H, W], `dtype` AFX_DT_F32 or AFX_DT_BF16 (widened to fp32, exactly), in the decoder's range [-1, 1]; src s fp32
 * [src_batch, C, H, W], src_batch 1 (shared by the batch) or batch; out fp32 [batch, C, H, W], not clamped.  src01 1: the source is in
 * [0, 1] and is read as s' = fma(2, s, -1), one rounding; src01 0: s' = s.  C, H, W >= 1: an image narrower than a dilation is legal.
 * AFX_COLOR_WAVELET: the low band of the edit is replaced by the low band of the source, as ONE chain on the difference (high(e) =
 * e - low(e) and low is linear): per element, in fp32,
 *     d = s' - e                                                                       (one rounding)
 *     for r in (1, 2, 4, 8, 16), cl = the clamp of an index into the image (replicate borders, at every level):
 *         q(y, x) = fma(0.5, d(y, x), 0.25 (d(y, cl(x - r)) + d(y, cl(x + r))))        (two roundings: the sum and the fma)
 *         d(y, x) = fma(0.5, q(y, x), 0.25 (q(cl(y - r), x) + q(cl(y + r), x)))        (two roundings)
 *     out = e + d                                                                      (one rounding)
 * The per-element order is fixed, so the launch structure cannot change a bit: one launch, every level of a 64 x 64 tile and its
 * 31-pixel apron in LDS; e and s are read once from memory and out is written once (37.7 MB per 3 x 1024 x 1024 fp32 image).  No
 * workspace (afx_color_fix_ws_bytes = 0; ws is ignored).  AFX_COLOR_WAVELET_LEVELS: the same values, bit for bit, by one launch per pass
 * through two fp32 planes of ws (8 batch C H W bytes) -- about four times the traffic; the plain form the fused one is checked against.
 * AFX_COLOR_ADAIN: the edit takes the source's mean and deviation per (image, channel): with n = H W and every element widened to fp64
 * (the source after the s' transform), both images by the same sequence of operations,
 *     mu = sum / n,  var = sumsq / n - mu mu  (population variance),  sd = sqrt(var + 1e-5),
 *     a = float(sd_s / sd_e),  b = float(mu_s - (sd_s / sd_e) mu_e)     (formed in fp64, rounded once each),   out = fma(a, e, b).
 * Identical planes give a == 1 and b == 0 exactly.  The sums are deterministic on the scheme of afx_image_ssim: one work-group and one
 * slot of ws (sum, sumsq) per 4096 consecutive elements of a plane (a function of H W alone), the slots of a plane added by a second
 * launch in that entry's fixed order (lane l of one wave the slots l, l + 64, ... in index order, then the 64 lanes by the shuffle tree);
 * no atomics, bit-reproducible, and a batch gives the bits of its single calls.  With src_batch 1 the source's moments are those of the
 * one source.  stats (may be NULL; ignored by the wavelet modes): fp64 [batch, C, 4] = (mu_e, var_e, mu_s, var_s).  Three launches.
 * ws: afx_color_fix_ws_bytes(mode, batch, C, H, W) bytes (adain: 8 batch C (4 ceil(H W / 4096) + 1)), 8-byte aligned, private to the call
 * until it completes.
 * Grid limit: batch C and H W must be below 2^31, and so must the work-groups of a launch -- batch C ceil(H / 64) ceil(W / 64) (wavelet),
 * 2 batch C ceil(H W / 4096) (adain); the per-pass form walks rows beyond 65535 by a loop.  A shape past it is AFX_E_INVALID.
 * Every refusal precedes the first launch and leaves out untouched: AFX_E_INVALID for a NULL edit, src or out, a bad dtype or mode, a
 * src01 other than 0 / 1, a src_batch outside {1, batch}, a size < 1, a misaligned pointer (edit: its element; src, out: 4 bytes; stats,
 * ws: 8), or out, stats or ws overlapping an operand or each other (in-place operation is refused in every mode); AFX_E_WORKSPACE for a
 * NULL or short ws when the mode needs one. */
#define AFX_COLOR_ADAIN 0
#define AFX_COLOR_WAVELET 1
#define AFX_COLOR_WAVELET_LEVELS 2
int64_t afx_color_fix_ws_bytes(int32_t mode, int32_t batch, int32_t C, int32_t H, int32_t W);
int afx_color_fix(const void* edit, int32_t dtype, const float* src, int32_t src_batch, int32_t src01, int32_t mode, float* out,
                  double* stats, void* ws, int64_t ws_bytes, int32_t batch, int32_t C, int32_t H, int32_t W, void* stream);

/* Head-logit gradient rows dY = [d_means | log_softmax^T(d_logw) | d_logg | 0] as bf16 (arcflux.py:243-249 backward) */
int afx_head_grad(const float* d_means, const float* d_logw, const float* d_logg, const void* logw_out, void* dy,
                  int64_t ldy, int64_t rows, int32_t K, int32_t ch, int32_t lw, void* stream);
/* C(float)[M,N] (+)= A[M,K] . W[N,K]^T, bf16 operands, fp32 result: weight gradients dW = dY^T . X on transposed copies */
int afx_linear_bf16_f32out(const void* A, int64_t lda, const void* W, int64_t ldw, float* C, int64_t ldc, int32_t M,
                           int32_t N, int32_t K, int32_t accumulate, void* stream);
/* C(float)[N1,N2] (+)= X^T . Y with X [M,N1], Y [M,N2] TOKEN-major bf16 (row strides ldx, ldy): the contraction runs over the rows.  The LoRA weight
 * gradients dB += dy^T t, dA += dT^T dropout(x) of peft's adapted linears (reference arcflux.py:294-302) straight from the token-major activations --
 * no transposed copies (ds_read_b64_tr_b16 gathers the MFMA fragments out of LDS).  N1, N2 multiples of 8; deterministic (no atomics). */
int afx_linear_tn_f32out(const void* X, int64_t ldx, const void* Y, int64_t ldy, float* C, int64_t ldc, int32_t M, int32_t N1, int32_t N2,
                         int32_t accumulate, void* stream);
/* The same product with the TOKEN loop split over work-groups (round 6): a [3072, 256] gradient is 48 tiles for 512 work-group slots, so each tile's 4608
 * tokens are cut into afx_linear_tn_ws_bytes() / (4 N1 N2) runs whose fp32 partial tiles go to `ws` and are then added IN ORDER into C by a second launch --
 * deterministic (the summation tree depends on the shape only), no atomics.  ws: afx_linear_tn_ws_bytes(M, N1, N2) bytes, 16-byte aligned, private to the
 * call until it has run (0 bytes = this shape runs unsplit; ws may then be NULL).  Same reference as above (peft lora_A / lora_B gradients, arcflux.py:294-302). */
int64_t afx_linear_tn_ws_bytes(int32_t M, int32_t N1, int32_t N2);
int afx_linear_tn_f32out_ws(const void* X, int64_t ldx, const void* Y, int64_t ldy, float* C, int64_t ldc, int32_t M, int32_t N1, int32_t N2,
                            int32_t accumulate, void* ws, void* stream);
/* C = res + (A . W^T) . keep / (1 - p): the input gradient of peft's LoRA branch with lora_dropout, dx = dx0 + ((dy B) A) . mask, in ONE launch -- the mask
 * (the counter hash of afx_lora_dropout_bf16: seed, row0 + row, column) is applied to the fp32 product in the GEMM's epilogue; res may alias C.  bf16. */
int afx_linear_bf16_dropres(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, int32_t M, int32_t N, int32_t K,
                            const void* res, int64_t ldr, float p, uint32_t seed, int64_t row0, void* stream);
int afx_transpose_bf16(const void* x, int64_t ldx, void* y, int64_t ldy, int32_t rows, int32_t cols, void* stream);
int afx_colsum_bf16(const void* x, int64_t ldx, float* out_accum, int32_t rows, int32_t cols, void* stream);
/* AdaLayerNormContinuous backward w.r.t. (scale, shift): dmod_accum[B,2,D] += sum_rows (dxn * LN(x) | dxn).  Keeps a per-(device, stream)
 * scratch inside the library (grown with hipFree / hipMalloc when a larger shape shows up: not capturable into a graph on that call);
 * long row ranges are folded in 8 splits that meet in float atomics, so the result is reproducible to the rounding of that sum's order. */
int afx_normout_backward(const void* x, int64_t ldx, const void* dxn, int64_t ldd, float* dmod_accum, int32_t rows,
                         int32_t D, int32_t rows_per_batch, void* stream);
/* The same sums for ONE batch entry into two separate fp32 [D] accumulators (d_scale += sum_rows dxn * LN(x), d_shift += sum_rows dxn): the training trunk adds
 * every block's AdaLN modulation gradients straight into its per-sample [n_mod] vector -- no scratch pair, no add passes. */
int afx_normout_backward_split(const void* x, int64_t ldx, const void* dxn, int64_t ldd, float* d_scale_accum, float* d_shift_accum, int32_t rows,
                               int32_t D, void* stream);
/* Modulation gradients of the blocks (needed by the timestep-embedder LoRA pair, configs/flux/arcflux_2nfe_k16.py:46-47):
 * out_accum[c] += sum_r a[r,c] b[r,c] (d_gate = sum_tokens dX_out * branch output);  out = res + gate[c] * y (gated residual kept
 * apart from the GEMM so that y can be stored);  out_accum[b,k] += sum_n x[b,n] W[n,k] (d silu(temb) through the stacked
 * modulation matrix W [n_mod, D], read once; B <= 4) */
int afx_coldot_bf16(const void* a, int64_t lda, const void* b, int64_t ldb, float* out_accum, int32_t rows, int32_t cols, void* stream);
int afx_gate_residual_bf16(const void* y, int64_t ldy, const float* gate, const void* res, int64_t ldr, void* out, int64_t ldo,
                           int64_t rows, int32_t cols, void* stream);
int afx_gemv_t_bf16(const float* x, int64_t ldx, const void* W, int64_t ldw, float* out_accum, int32_t B, int64_t N, int32_t K,
                    void* stream);
/* dW_accum[J,Kd] += sum_b dmod[b,J] x[b,Kd]   (norm_out.linear weight gradient, B <= 8) */
int afx_outer_accum(const float* dmod, const float* x, float* dW_accum, int32_t B, int32_t J, int32_t Kd, void* stream);
/* Staged forward for the training student with LoRA input dropout (lakonlab .../arcflux.py:294-302 lora_dropout): stage 1 runs
 * the conditioning + embedders only, the caller runs the blocks itself on the token matrix (afx_mmdit_export "x_tokens",
 * [B*(T+N), D] bf16, text rows first per sample), puts the result back with afx_mmdit_import_tokens and calls stage 2
 * (norm_out + velocity head).  stage 0 = afx_mmdit_forward. */
int afx_mmdit_forward_stage(afx_ctx* ctx, const void* x, const void* ctx_emb, const void* pooled, const float* t, const float* g,
                            const float* rope_cos, const float* rope_sin, int32_t B, int32_t N, int32_t T, void* means, void* logw,
                            void* logg, int32_t stage, void* stream);
int afx_mmdit_import_tokens(afx_ctx* ctx, const void* src, int32_t batch, int32_t n_img, int32_t n_txt, void* stream);
/* fp8 linear mode (BASELINE.json configs[4] "fp8 MFMA fwd"): every block linear (qkv / out / mlp of the double blocks, fused
 * projection and proj_out of the single blocks) runs on the fp8 MFMA with row-wise scales: activations are quantised per
 * token right before the GEMM, weights come pre-quantised as "<linear>.weight_q" (AFX_DT_FP8 [out, in]) + "<linear>.wscale"
 * (f32 [out]) next to the bf16 ones.  Embedders, modulation, head and attention stay bf16.  Set before afx_workspace_bytes. */
int afx_set_fp8_linear(afx_ctx* ctx, int32_t on);
/* Timestep-embedding override: when set (device pointer to [B, D] f32, NULL to clear) the next forwards use it in place of
 * timestep_embedder(sincos(1000 t)); the guidance / pooled-text embeddings are still added.  The training student computes it
 * host-side with the LoRA pair on the two tiny linears (and their input dropout). */
int afx_set_temb_override(afx_ctx* ctx, const float* temb_t);

/* Copy an activation of the LAST afx_mmdit_forward out of the workspace: "head_in" [B*N,D] bf16,
 * "x_final" [B*N,D] bf16, "silu_temb" [B,D] f32, "mod_final" [B,2D] f32 (scale|shift of norm_out),
 * "mod_all" [B, n_mod] f32 (every modulation vector: per double block img 6D | txt 6D, per single block 3D, final 2D). */
int afx_mmdit_export(afx_ctx* ctx, const char* what, void* dst, int32_t batch, int32_t n_img, int32_t n_txt,
                     void* stream);

/* Element-wise backward kernels of the trunk (gradient checkpointed block recompute + backward):
 * dx = dres + LN^T(dxn (1+scale));  out-of-place RMSNorm+RoPE forward (backward = 0) / backward (dy -> dx, written
 * to y);  GELU(tanh) forward (dh == NULL) / backward;  out = (a (+ b)) * gate[batch] residual-gradient plumbing. */
int afx_ln_modulate_backward(const void* x, int64_t ldx, const void* dxn, int64_t ldd, const float* scale, int64_t ldmod,
                             int32_t rows_per_batch, const void* dres, int64_t ldr, void* dx, int64_t ldo, int32_t rows,
                             int32_t D, void* stream);
int afx_qk_norm_rope_oop_bf16(const void* x, int64_t ldx, void* y, int64_t ldy, const void* dy, int64_t lddy,
                              const float* w_txt, const float* w_img, const float* rope_cos, const float* rope_sin,
                              int32_t batch, int32_t S, int32_t n_txt, int32_t heads, int32_t backward, void* stream);
int afx_gelu_bf16(const void* pre, int64_t ldp, const void* dh, int64_t ldh, void* out, int64_t ldo, int64_t rows,
                  int32_t cols, void* stream);
int afx_add_scale_bf16(const void* a, int64_t lda, const void* b, int64_t ldb, const float* gate, int64_t ldg,
                       int32_t rows_per_batch, void* out, int64_t ldo, int64_t rows, int32_t cols, void* stream);

/* Optimiser step of lakonlab/models/base.py:76-103 + ema_hook.py:86-124 on flat fp32 buffers:
 * global grad-norm (afx_sumsq accumulates sum of squares), AdamW with decoupled decay (grad_scale folds
 * 1/world and the clip factor; step >= 1 for bias correction), Karras EMA  ema = net + (ema - net) * beta. */
int afx_sumsq(const float* x, float* out_accum, int64_t n, void* stream);
int afx_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int32_t step, float grad_scale, int64_t n, void* stream);
/* The same update with block-wise 8-bit moments (the reference's optimizer is bitsandbytes AdamW8bit: _ddp_train.py:18-26,
 * optimizer/builder.py:11-24): state1 / state2 hold one code byte per value, absmax1 / absmax2 one f32 per block of 256 values
 * (ceil(n / 256) entries), qmap1 (signed) / qmap2 (unsigned) the 256-entry sorted code books (arcflow_amd/ops.py dynamic_map).
 * Zero-initialised absmax + any codes = zero moments.  The parameter is updated from the new moments BEFORE they are re-quantised. */
int afx_adamw8bit_step(float* param, const float* grad, void* state1, void* state2, float* absmax1, float* absmax2,
                       const float* qmap1, const float* qmap2, float lr, float beta1, float beta2, float eps, float weight_decay,
                       int32_t step, float grad_scale, int64_t n, void* stream);
int afx_ema_lerp(float* ema, const float* net, float beta, int64_t n, void* stream);
int afx_cast_f32_bf16(const float* x, void* y, int64_t n, void* stream);

/* ---- VAE decoder (AutoencoderKL, the step after the loop: arcflux_pipeline.py:531-534) ---------------------------
 * Activations are NHWC bf16 on ZERO-BORDERED grids [(H+2)*(W+2), C]; a 3x3 convolution is an implicit GEMM on the MFMA
 * kernel (K-tile = (tap, 64-channel chunk) = the same pixel rows shifted by dy*(W+2)+dx, no im2col), the epilogue
 * re-zeroes the border.  x must be readable (W+3) rows before and after the grid.  w: [Cout][3][3][Cin] bf16. */
int afx_conv3x3_bf16(const void* x, const void* w, const void* bias, void* y, int32_t H, int32_t W, int32_t Cin,
                     int32_t Cout, const void* res, void* stream);
#define AFX_GN_SLOTS 64
/* Bytes of the stats_ws scratch afx_groupnorm_nhwc / afx_groupnorm_nhwc_from_stats need for (C, groups): (2 + 2*AFX_GN_SLOTS)*groups + C
 * doubles.  (The requirement GREW in round 3 -- it was 2*groups doubles + 2*C floats -- when the per-slot partial sums moved into it:
 * size the buffer with this call, not with a constant.)  Negative status on bad arguments. */
int64_t afx_groupnorm_ws_bytes(int32_t C, int32_t groups);
/* y = act(GroupNorm(x)) on the interior, 0 on the border; stats_ws: afx_groupnorm_ws_bytes(C, groups) of scratch; act 1 = SiLU;
 * C/8 must divide 256 (C = 64, 128, 256, 512, 1024, 2048) */
int afx_groupnorm_nhwc(const void* x, void* y, double* stats_ws, int32_t H, int32_t W, int32_t C, int32_t groups,
                       const float* gamma, const float* beta, float eps, int32_t act, void* stream);
/* The same convolution, and the GroupNorm sums of ITS OUTPUT accumulated by the GEMM epilogue from the fp32 accumulators BEFORE the bf16
 * rounding of the stored values (mean / variance differ from sums over the stored grid by that rounding: ~2^-9 relative, bounded in
 * tests/test_vae.py): gn_stats = AFX_GN_SLOTS x groups x 2 doubles (zeroed by the call; partial sums spread over the slots by tile), Cout <= 128 (the 256x128-tile kernel: the full-resolution stage, whose
 * grids are the largest), Cout / groups = 4, 8 or a multiple of 8.  afx_groupnorm_nhwc_from_stats
 * then normalises y without a statistics pass of its own (diffusers' ResnetBlock2D order norm -> act -> conv: every GroupNorm input of the
 * decoder except the attention output is a convolution output).  afx_conv_stats_available(): 0 when the GEMM kernel override in force has no
 * such epilogue (AFX_GEMM_IMPL=2 or a forced tile shape). */
int afx_conv3x3_bf16_stats(const void* x, const void* w, const void* bias, void* y, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                           const void* res, double* gn_stats, int32_t groups, void* stream);
int afx_groupnorm_nhwc_from_stats(const void* x, void* y, const double* gn_stats, double* stats_ws, int32_t H, int32_t W, int32_t C,
                                  int32_t groups, const float* gamma, const float* beta, float eps, int32_t act, void* stream);
int afx_conv_stats_available(void);
/* y = conv3x3(nearest-2x upsample(x)) + bias with the upsample FOLDED into the convolution (diffusers Upsample2D: F.interpolate(nearest) then conv,
 * reached through vae.decode, arcflux_pipeline.py:531-534): x = the low-resolution zero-bordered grid [(H+2)*(W+2), Cin], y = [(2H+2)*(2W+2), Cout],
 * w4 = four 2x2 phase kernels [2 py + px][Cout][2][2][Cin] bf16 built from the 3x3 weight (arcflow_amd.vae.phase_weights): 44 % of the flops of the
 * convolution on the upsampled grid, which is never written.  Needs afx_conv_stats_available() (the one-wave-per-SIMD GEMM). */
int afx_upconv3x3_bf16(const void* x, const void* w4, const void* bias, void* y, int32_t H, int32_t W, int32_t Cin, int32_t Cout, void* stream);
int afx_upsample2x_nhwc(const void* x, void* y, int32_t H, int32_t W, int32_t C, void* stream);
/* scatter == 0: compact[H*W, C] = interior(padded);  != 0: interior(padded) = compact (+ interior(res_padded)) */
int afx_interior_nhwc(void* padded, void* compact, const void* res_padded, int32_t H, int32_t W, int32_t C, int32_t scatter,
                      void* stream);
/* P = softmax(scale * S) row-wise, S fp32 [rows, cols], P bf16 (mid-block single-head attention, head dim 512) */
int afx_softmax_rows_f32(const float* s, int64_t lds_, void* p, int64_t ldp, int32_t rows, int32_t cols, float scale,
                         void* stream);
/* packed latent tokens [hp*wp, 64] f32 -> padded NHWC [(2hp+2)*(2wp+2), Cpad] bf16 of lat/scaling + shift; and back to
 * an image [3, H, W] f32 from the first 3 channels of a padded NHWC grid */
int afx_latent_to_nhwc(const float* tokens, void* y, int32_t hp, int32_t wp, int32_t Cpad, float scaling_factor,
                       float shift_factor, void* stream);
int afx_nhwc_to_image(const void* x, float* img, int32_t H, int32_t W, int32_t C, void* stream);
/* AutoencoderKLQwenImage (lakonlab/pipelines/arcqwen_pipeline.py:470-481): the unpack applies v = A . lat + b on the 16
 * latent channels per pixel (A [16][16] row-major = post_quant_conv . diag(latents_std), b = post_quant_conv . mean + bias);
 * the norm is the per-pixel channel RMS norm of that VAE, y = x / max(|x|_2, 1e-12) * sqrt(Creal) * gamma, act 1 = SiLU,
 * Cpad <= 512 */
int afx_latent_to_nhwc_affine(const float* tokens, void* y, int32_t hp, int32_t wp, int32_t Cpad, const float* A, const float* b,
                              void* stream);
int afx_rmsnorm_nhwc(const void* x, void* y, int64_t rows, int32_t Cpad, int32_t Creal, const float* gamma, int32_t act,
                     void* stream);

/* ---- VAE encoders (images -> latents: vae.encode behind lakonlab/models/architecture/diffusers/pretrained.py:60-67 and :133-140) ----
 * The encoders' downsample (diffusers Downsample2D(padding=0) / Qwen Resample('downsample2d')): y = conv3x3(pad(x, (0,1,0,1)), stride 2) + bias,
 * out[y][x] = sum w[dy][dx] in[2y+dy][2x+dx] with input row H / column W read as zero.  x: zero-bordered grid [(H+2)*(W+2), Cin], y: zero-bordered
 * grid [(H/2+2)*(W/2+2), Cout] (border re-zeroed).  An implicit GEMM, no im2col: x is first re-laid space-to-depth into ws, a zero-bordered
 * [(H/2+2)*(W/2+2), 4 Cin] grid with (W/2+3) readable rows before and after it (channel (2 py + px) Cin + c of cell (Y, X) = x[2Y+py][2X+px][c]),
 * on which the stride-2 kernel is a stride-1 3x3 kernel with taps 0 / +1: w = [Cout][3][3][4 Cin] bf16 from arcflow_amd.vae.s2d_weights.
 * H, W even, Cin % 64 == 0, Cout % 8 == 0, else AFX_E_INVALID.  gn_stats / groups as afx_conv3x3_bf16_stats, or null / 0. */
int afx_conv3x3s2_bf16(const void* x, const void* w, const void* bias, void* y, void* ws, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                       double* gn_stats, int32_t groups, void* stream);
/* The encoder's first layer operand (the inverse direction of afx_nhwc_to_image): image [3, H, W] fp32 (img_bf16 0) or bf16 (1), in [-1, 1], or
 * in [0, 1] with from01 != 0 (the images * 2 - 1 of lakonlab/models/latent_diffusion_text_image.py:43 applied here) -> zero-bordered grid
 * [(H+2)*(W+2), 64] bf16 whose interior rows hold the pixel's 3x3x3 neighbourhood, k = (3 dy + dx) * 3 + channel, k = 27 the constant 1, the
 * rest zero: conv_in (3 -> C, padding 1) is then afx_linear_bf16 with K = 64 on the weight from arcflow_amd.vae.conv_in_weights (bias in column 27). */
int afx_image_to_cols27(const void* img, int32_t img_bf16, void* y, int32_t H, int32_t W, int32_t from01, void* stream);
/* DiagonalGaussianDistribution + the latent normalisation of pretrained.py:67 / :140 in one pass.  grid: zero-bordered [(h+2)*(w+2), Cpad >= 32]
 * bf16, channels 0-15 mean, 16-31 logvar (conv_out's output); A [32][32] / b [32] fp32: optional 1x1 quant_conv applied first (both or neither).
 * moments [32, h, w] fp32 = mean | clamp(logvar, -30, 20); z = mean + exp(logvar / 2) * eps (eps [16, h, w] fp32; null: z = mean, the mode);
 * out = (z - sub[c]) * fac[c] (divide 0: FLUX, sub = shift, fac = scaling) or (z - sub[c]) / fac[c] (divide 1: Qwen-Image, latents_mean / latents_std),
 * fp32 as [16, h, w] (packed 0) or packed tokens [(h/2)*(w/2), 64], channel c * 4 + (y & 1) * 2 + (x & 1) (packed 1; h, w even). */
int afx_posterior_latents(const void* grid, int32_t Cpad, int32_t h, int32_t w, const float* A, const float* b, const float* eps, const float* sub,
                          const float* fac, int32_t divide, float* out, int32_t packed, float* moments, void* stream);

/* ---- text encoders: T5-XXL + CLIP-L (FLUX), Qwen2.5-VL language model (Qwen-Image) -----------------------
 * Replaces the transformers modules behind lakonlab/models/architecture/diffusers/pretrained.py:152-238
 * (PretrainedFluxTextEncoder / PretrainedQwenImageTextEncoder -> pipeline.encode_prompt). */
/* out[s, :] = table[ids[s], :] (+ pos[s, :]) */
int afx_embed_rows_bf16(const void* table, const int32_t* ids, const void* pos, void* out, int32_t S, int32_t D, void* stream);
/* rms 0: LayerNorm(x) * w + b;  rms 1: x * rsqrt(mean(x^2) + eps) * w (b ignored).  fp32 statistics, D <= 8192 */
int afx_norm_rows_bf16(const void* x, int64_t ldx, void* y, int64_t ldy, int32_t rows, int32_t D, const float* w, const float* b,
                       float eps, int32_t rms, void* stream);
/* out[m, j] = act(x[m, j]) * (gate_off >= 0 ? x[m, gate_off + j] : 1);  act 0 none, 1 SiLU, 2 GELU(tanh), 3 quick-GELU */
int afx_act_mul_bf16(const void* x, int64_t ldx, void* out, int64_t ldo, int64_t M, int32_t F, int32_t gate_off, int32_t act,
                     void* stream);
/* rotate-half RoPE in place on H heads side by side in a row; cos/sin [S, head_dim / 2] f32 */
int afx_rope_half_bf16(void* x, int64_t ldx, const float* cos_t, const float* sin_t, int32_t S, int32_t H, int32_t head_dim,
                       void* stream);
/* fp8 (OCP e4m3) linear on v_mfma_scale_f32_16x16x128_f8f6f4 (BASELINE.json configs[4]): row-wise
 * quantisation q = round(x / scale[r]), scale[r] = absmax(row) / 448, for activations (per token) and weights (per output
 * channel); C = epi(a_scale[m] w_scale[n] (Aq . Wq^T) + bias), bf16 out, same epilogues as afx_linear_bf16.  K % 128 == 0. */
int afx_quant_rows_fp8(const void* x, int64_t ldx, void* q, int64_t ldq, float* scale, int32_t rows, int32_t K, void* stream);
int afx_linear_fp8(const void* Aq, int64_t lda, const float* a_scale, const void* Wq, int64_t ldw, const float* w_scale, const void* bias,
                   void* C, int64_t ldc, int32_t M, int32_t N, int32_t K, int32_t epi, int32_t gelu_col0, const float* gate, int64_t ldg,
                   int32_t rows_per_batch, const void* res, int64_t ldr, void* stream);
/* Block-scaled activations (the MX layout with 128-value blocks = one K-tile of the one-wave-per-SIMD fp8 kernel): mx[r][j] = E8M0 byte b,
 * scale 2^(b - 127) = the smallest power of two with absmax(x[r, 128 j .. 128 j + 127]) <= 448 * scale; q = round(x / scale), e4m3.
 * afx_linear_fp8_mx consumes it (the matrix instruction applies the block scales); a_scale[m] still multiplies row m (pass ones),
 * weights keep their per-output-channel fp32 scales.  K % 512 == 0, ld_mx % 4 == 0.  No reference counterpart (the reference has no
 * fp8 path): the format exists so that GEMM / attention / LayerNorm epilogues can quantise the 128 columns they hold. */
int afx_quant_rows_mx8(const void* x, int64_t ldx, void* q, int64_t ldq, void* mx, int64_t ld_mx, int32_t rows, int32_t K, void* stream);
int afx_linear_fp8_mx(const void* Aq, int64_t lda, const void* a_mx, int64_t ld_mx, const float* a_scale, const void* Wq, int64_t ldw,
                      const float* w_scale, const void* bias, void* C, int64_t ldc, int32_t M, int32_t N, int32_t K, int32_t epi,
                      int32_t gelu_col0, const float* gate, int64_t ldg, int32_t rows_per_batch, const void* res, int64_t ldr, void* stream);
/* ... and the producer side: the fp8 GEMM whose epilogue writes the NEXT GEMM's block-scaled operand.  Columns [0, c8_col0) leave as bf16 in C
 * (bias only), columns [c8_col0, N) as e4m3 bytes in c8[m][n - c8_col0] with scale bytes c_mx[m][(n - c8_col0) / 128], after bias and
 * (gelu != 0) tanh-GELU -- the mlp hidden of a double block (c8_col0 = 0), the mlp part of a single block's k|v|q|mlp projection
 * (c8_col0 = 3 D).  a_mx may be NULL (per-row a_scale only). */
int afx_linear_fp8_to_mx8(const void* Aq, int64_t lda, const void* a_mx, int64_t ld_mx, const float* a_scale, const void* Wq, int64_t ldw,
                          const float* w_scale, const void* bias, void* C, int64_t ldc, void* c8, int64_t ldc8, void* c_mx, int64_t ld_cmx,
                          int32_t c8_col0, int32_t M, int32_t N, int32_t K, int32_t gelu, void* stream);
/* Split-K GEMM for few-row operands (M <= 1-2 tiles: the prompt encoders): the K range is cut into chunks, chunk c stores
 * its partial A . W^T (+ bias on chunk 0) into the f32 slab partials[c][M][N]; afx_finish_f32_bf16 sums the slabs into bf16
 * (+ residual).  afx_linear_splitk_chunks = number of slabs for (M, N, K, split_k); split_k 0: chosen to fill the chip. */
int afx_linear_splitk_chunks(int32_t M, int32_t N, int32_t K, int32_t split_k);
int afx_linear_bf16_splitk(const void* A, int64_t lda, const void* W, int64_t ldw, const void* bias, float* partials, int32_t M,
                           int32_t N, int32_t K, int32_t split_k, void* stream);
int afx_finish_f32_bf16(const float* partials, int32_t nslab, const void* res, int64_t ldr, void* out, int64_t ldo, int64_t M, int32_t N,
                        void* stream);
/* softmax(scale * Q K^T + scale * bias [, causal]) V with H query heads over Hkv KV heads (H % Hkv == 0), head_dim 64 or 128;
 * bias: [H][2S-1] f32 indexed by key - query + S - 1, ALREADY DIVIDED by scale, or NULL; ws: afx_attention_ext_ws_bytes */
int64_t afx_attention_ext_ws_bytes(int32_t B, int32_t Hkv, int32_t S, int32_t head_dim);
int afx_attention_ext_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo,
                           void* ws, int32_t B, int32_t H, int32_t Hkv, int32_t S, int32_t head_dim, float scale, int32_t causal,
                           const float* bias, void* stream);

/* ---- building-block kernels (exported for the per-kernel parity tests and micro benches) -- */

/* C[M,N] = epi(A[M,K] . W[N,K]^T + bias)   bf16 in/out, fp32 accumulate (nn.Linear semantics).
 * epi 0: none; 1: GELU(tanh) on columns >= gelu_col0; 2: C = res + gate[m / rows_per_batch, n] * (.)  (gate NULL: C = res + (.))
 * K % 64 == 0, N % 8 == 0, lda/ldw/ldc/ldr % 8 == 0. */
int afx_linear_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, const void* bias,
                    void* C, int64_t ldc, int32_t M, int32_t N, int32_t K,
                    int32_t epi, int32_t gelu_col0, const float* gate, int64_t ldg,
                    int32_t rows_per_batch, const void* res, int64_t ldr, void* stream);
/* same, with pre [M,N] bf16 added to A.W^T + bias BEFORE the activation / gate (the LoRA-dropout correction B A (x . delta)) */
int afx_linear_bf16_pre(const void* A, int64_t lda, const void* W, int64_t ldw, const void* bias,
                        void* C, int64_t ldc, int32_t M, int32_t N, int32_t K,
                        int32_t epi, int32_t gelu_col0, const float* gate, int64_t ldg,
                        int32_t rows_per_batch, const void* res, int64_t ldr, const void* pre, int64_t ldp, void* stream);
/* Tuning / test knob of every bf16 GEMM in the library (process-wide, not thread-safe against running launches): impl 3 (default) =
 * one-wave-per-SIMD kernel for the bf16 epilogue modes with the tile shape picked per launch (tile 0) or forced (1: 256x256,
 * 2: 288x192, 3: 320x192, 4: 128x128, 5: 256x224, 6: 224x256); impl 2 = 8-phase 256x256 kernel for everything; any other impl selects 3.  Same meaning
 * as the AFX_GEMM_IMPL / AFX_GEMM_TILE environment variables (read once, on first use), which it overrides.  Returns 0. */
int afx_gemm_set_mode(int32_t impl, int32_t tile);
/* Tile shape of the one-wave-per-SIMD fp8 GEMM kernel (process-wide, like afx_gemm_set_mode): 0 (default) = picked per launch, 1 = 256x256,
 * 2 = 224x256 (launches with the fused q / k epilogue keep 256x256); any other value selects 0.  Same meaning as the AFX_FP8_TILE environment
 * variable, which it overrides.  Returns the setting now in force (0, 1 or 2).  Host-side, no GPU needed. */
int afx_gemm_set_fp8_tile(int32_t tile);
/* 1 when afx_linear_bf16_dropres can run under the current kernel choice (its masked residual add lives in the one-wave-per-SIMD kernel's epilogue: kernel
 * mode 3), 0 otherwise -- the caller then computes the product with afx_linear_bf16 and masks + adds it with afx_lora_dropout_bf16 mode 3
 * (arcflow_amd/ops.py linear_dropres does).  Host-side, no GPU needed. */
int afx_gemm_dropres_available(void);
/* Kernel choice of every joint attention launch (process-wide; same meaning as AFX_ATTN_IMPL, which it overrides): 0 (default) = the
 * one-wave-per-SIMD kernel (afx_attn3.hip: 64 queries per wave, any S > 64: ragged tails handled) where eligible, else the 4-wave kernel; 1 = 4-wave kernel
 * always; 3 = the one-wave-per-SIMD kernel on its plain grid (0 cuts the 256-query blocks of an under-filled last round into one run of key tiles per
 * CU and merges the partial results: afx_attn3.hip); any other value selects 0.  For A/B runs and the parity tests.  Returns 0. */
int afx_attn_set_impl(int32_t impl);
/* LoRA input dropout masks from a counter-based hash of (seed, row0 + row, col), keep probability 1 - p, delta = keep/(1-p) - 1:
 * mode 0: dst = src * delta;  1: dst = src * (1 + delta) (= dropout(src));  2: dst += src * delta;  3: dst += src * (1 + delta) */
int afx_lora_dropout_bf16(const void* src, int64_t lds_, void* dst, int64_t ldd, int64_t M, int32_t N, int64_t row0, float p,
                          uint32_t seed, int32_t mode, void* stream);

/* Joint attention over S tokens, no mask: O = softmax(Q K^T / sqrt(128)) V per (batch, head).
 * q,k,v,o: row (b*S + s), head h at column h*128, row strides ld* (elements).  head_dim = 128.
 * vt_ws: scratch of afx_attention_ws_bytes() bytes (transposed V).  o may alias q. */
int64_t afx_attention_ws_bytes(int32_t batch, int32_t heads, int32_t S);
int afx_attention_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                       int64_t ldv, void* o, int64_t ldo, void* vt_ws,
                       int32_t batch, int32_t heads, int32_t S, void* stream);
/* The same attention with the output as the next fp8 GEMM's block-scaled operand (afx_quant_rows_mx8's layout; a head's 128 columns = one block):
 * o8 [batch * S, ldo8] e4m3 bytes, mx [batch * S, ld_mx] one E8M0 byte per token and head.  S > 64.  vt_ws as afx_attention_bf16. */
int afx_attention_to_mx8(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o8, int64_t ldo8,
                         void* mx, int64_t ld_mx, void* vt_ws, int32_t batch, int32_t heads, int32_t S, void* stream);

/* Training twins: forward that also returns lse [B, H, roundup(S,64)] f32 (log2-domain log-sum-exp of the scaled
 * scores; the caller pre-fills it with +inf so padded queries drop out), and the backward producing dq, dk, dv
 * (same row/head addressing as q, k, v) from o, dout and lse.  ws: afx_attention_bwd_ws_bytes() bytes. */
int afx_attention_fwd_lse_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o,
                               int64_t ldo, float* lse, void* vt_ws, int32_t batch, int32_t heads, int32_t S, void* stream);
int64_t afx_attention_bwd_ws_bytes(int32_t batch, int32_t heads, int32_t S);
/* Kernel generation of afx_attention_bwd_bf16 (reference: the FlashAttention-2 backward SDPA runs under arcflux.py:181-189): 3 (default) = the generated
 * one-wave-per-SIMD dK / dV and dQ streams in one launch (csrc/afx_attn_bwd3.hip; S > 64, row strides multiples of 8), 4 = the same as two launches,
 * 1 = generated dK / dV + round-4 dQ, 2 = the round-4 kernels (also what S <= 64 runs).  For A/B runs and the parity tests.  Returns 0. */
int afx_attn_bwd_set_impl(int32_t impl);
int afx_attention_bwd_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* o,
                           int64_t ldo, const void* dout, int64_t lddo, const float* lse, void* dq, int64_t lddq, void* dk,
                           int64_t lddk, void* dv, int64_t lddv, void* ws, int32_t batch, int32_t heads, int32_t S,
                           void* stream);

/* out = LayerNorm(x, eps=1e-6, no affine) * (1 + scale[b]) + shift[b]   (AdaLN modulate), or with
 * rms != 0: out = x * rsqrt(mean(x^2) + 1e-6) * w  (scale = w as f32[D], shift ignored). */
int afx_norm_modulate_bf16(const void* x, int64_t ldx, void* out, int64_t ldo, int32_t rows,
                           int32_t D, const float* scale, const float* shift, int64_t ldmod,
                           int32_t rows_per_batch, int32_t rms, void* stream);

/* In-place per-head RMSNorm(eps 1e-6, weight) + interleaved-pair RoPE on q or k.
 * x: row (b*S+s), head h at column h*128.  rows s < n_txt use w_txt, others w_img (f32[128]). */
int afx_qk_norm_rope_bf16(void* x, int64_t ldx, const float* w_txt, const float* w_img,
                          const float* rope_cos, const float* rope_sin,
                          int32_t batch, int32_t S, int32_t n_txt, int32_t heads, void* stream);

/* y[b,n] (+)= act(sum_k x[b,k] W[n,k] + bias[n]); x f32 [B,K], W bf16 [N,K], y f32 [B,N];
 * act 0 none, 1 SiLU; accumulate != 0 adds into y. */
int afx_gemv_bf16(const float* x, const void* W, const void* bias, float* y, int32_t B, int32_t N,
                  int32_t K, int32_t act, int32_t accumulate, void* stream);

/* The attention operands of ONE block exactly as afx_mmdit_forward builds them (bf16 linears), for parity tests.
 * A: the AdaLN output [B*S, D] bf16 (row stride lda), the joint layout [text T | image N] per sample, S = N + T, D = heads * 128.
 * kind AFX_BLOCK_DOUBLE: per-stream k|v|q weights w_img / w_txt [3D, D] (+ biases [3D] or both null), qkn [img_q, img_k, txt_q, txt_k][128];
 *   F [B*S, 3D] (row stride ldf) receives k | v | q.
 * kind AFX_BLOCK_SINGLE: the fused weight w_img [7D, D] (+ b_img [7D]; w_txt / b_txt unused), qkn [q, k][128]; F [B*S, 7D] receives
 *   k | v | q | gelu_tanh(mlp).
 * k and q leave as RoPE(RMSNorm_128(.) * w) per head at the row's joint position (the single block: row % S) of rope_cos / rope_sin
 * [S, 64] f32; Vt [B][heads][128][roundup(S, 64)] bf16 receives V^T with the keys of every 16-group in the attention kernel's order and
 * zeros for keys >= S (V itself stays in F for every path but AFX_QKV_VT_PROJ, which leaves F's V columns unwritten).
 * path: AFX_QKV_AUTO = the forward's choice for this shape, or one of the three forced; AFX_E_INVALID when it cannot run on the shape
 * or with the GEMM kernel in use.  batch <= AFX_MAX_MICRO_BATCH. */
#define AFX_BLOCK_DOUBLE 0
#define AFX_BLOCK_SINGLE 1
#define AFX_QKV_AUTO 0
#define AFX_QKV_VT_PROJ 1   /* V^T out of the projection GEMM, q / k epilogue on separate k and q problems: T % 16 == 0, S % 64 == 0 */
#define AFX_QKV_QK_EPI 2    /* q / k RMSNorm + RoPE in the projection's fp32 epilogue, then a V transpose launch */
#define AFX_QKV_KV_PREP 3   /* the plain projection, then norm + RoPE of the bf16 k / q and the V transpose in one launch */
int afx_qkv_operands(int32_t kind, const void* A, int64_t lda, const void* w_img, const void* b_img, const void* w_txt, const void* b_txt,
                     const float* qkn, const float* rope_cos, const float* rope_sin, int32_t batch, int32_t n_img, int32_t n_txt,
                     int32_t heads, int32_t path, void* F, int64_t ldf, void* Vt, void* stream);
/* AdaLN of a joint token matrix in one launch (the forward's double blocks): out = LayerNorm(x) * (1 + scale) + shift, rows of sample
 * b = row / S at scale + b * ldmod, the first n_txt rows of each sample with scale_txt / shift_txt (both null: one stream, n_txt 0). */
int afx_norm_modulate_joint_bf16(const void* x, int64_t ldx, void* out, int64_t ldo, int32_t rows, int32_t D, const float* scale,
                                 const float* shift, const float* scale_txt, const float* shift_txt, int64_t ldmod, int32_t S,
                                 int32_t n_txt, void* stream);
/* ... straight into the next fp8 GEMM's operand: e4m3 bytes q8 [rows, ldq] with one E8M0 byte per row and 128 columns in mx [rows, ld_mx]
 * or, with rowscale != null, one f32 scale per row (absmax / 448).  *fused = 0: no fused kernel for this shape and nothing was
 * launched (the forward then runs the bf16 kernel and a quantisation pass). */
int afx_norm_modulate_mx8(const void* x, int64_t ldx, void* q8, int64_t ldq, void* mx, int64_t ld_mx, float* rowscale, int32_t rows,
                          int32_t D, const float* scale, const float* shift, const float* scale_txt, const float* shift_txt,
                          int64_t ldmod, int32_t S, int32_t n_txt, int32_t* fused, void* stream);

/* Fold J <= AFX_LORA_MAX_ADAPTERS weighted low-rank adapters into one linear (style LoRAs next to the ArcFlow adapter: what peft's
 * side branches y += s (alpha / r) B A x of every active adapter add up to, lakonlab/models/architecture/arcflow/arcflux.py:147-154 with
 * `pipe.set_adapters([...])` of inference_flux.py:9):
 *   dst[o, i] = bf16_rne( float(base[o, i]) + sum_j scales[j] * ( sum_r B[j][o, r] * A[j][r, i] ) )
 * base, dst  bf16 row slices [O, I] of packed weight matrices with leading dimensions ld_base / ld_dst (elements), so a slice may start
 *            at any row of a taller matrix; 16-byte aligned, leading dimensions multiples of 8; the two ranges must not overlap.
 * A, B, ranks, scales  HOST arrays of J entries: A[j] [ranks[j], I] bf16 (16-byte aligned), B[j] [O, ranks[j]] bf16, any rank >= 1 (the
 *            kernel zero-fills the last MFMA K-step itself), scales[j] fp32.  They are read before the call returns.
 * Arithmetic: bf16 MFMAs with fp32 accumulation per adapter; scales[j] multiplies adapter j's fp32 sum (never a bf16 operand); one
 * rounding, at the store.  One work-group owns each 64 x 64 tile of dst and walks the whole rank of every adapter in order: no split
 * over the rank, no atomics, no workspace, bit-reproducible.  J == 0 copies base into dst.
 * AFX_E_INVALID (nothing is launched): a null pointer, J > 8, a rank < 1, O or I not a positive multiple of 64, a leading dimension
 * < I, dst overlapping base, or an alignment above not met.
 * Traffic: 4 B per element of the slice + the A / B panels out of L2; 2 sum(ranks) flop per element: HBM-bound. */
#define AFX_LORA_MAX_ADAPTERS 8
int afx_lora_fold(const void* base, int64_t ld_base, void* dst, int64_t ld_dst, int32_t O, int32_t I, int32_t J,
                  const void* const* A, const void* const* B, const int32_t* ranks, const float* scales, void* stream);
/* DoRA adapters (weight-decomposed LoRA: a magnitude m[o] per output row next to A / B; `dora_scale` of Kohya files, `lora_magnitude_vector` of
 * peft files).  An active DoRA adapter j replaces row o of the base by g_j[o] (w + s_j B_j A_j)[o, :] with the row gain
 *   g_j[o] = m_j[o] / sqrt( sum_i ( w[o, i] + s_j sum_r B_j[o, r] A_j[r, i] )^2 ),
 * and several active adapters add their deltas relative to the base weight, a DoRA adapter's being (g_j - 1) w + g_j s_j B_j A_j (peft's rule for
 * several active adapters as recalled -- not checked against peft).  The whole row is needed before an element can be written: two launches.
 *
 * afx_lora_row_gain: gain[o] (fp32 [O]) of ONE adapter on one linear.  base [O, I] bf16 with leading dimension ld_base, A [r, I] (16-byte aligned),
 * B [O, r] bf16, any rank >= 1, s fp32, m fp32 [O]; O, I positive multiples of 64, base 16-byte aligned with ld_base % 8 == 0, m / gain 4-byte aligned,
 * gain overlapping none of the inputs.  Every 64 x 64 tile of w + s B A is formed as afx_lora_fold forms it (same staging, same 16x16x32 bf16 MFMA,
 * fp32); one work-group owns 64 rows and walks the column tiles in order, the squares are summed in fp32 in a fixed order (no atomics, no
 * workspace): bit-reproducible.  Square root and division are correctly rounded.  A row whose sum of squares is 0 gets gain 0 -- a deviation from
 * peft, which divides by zero there.  Traffic: 2 B per element read, 4 O bytes written.
 *
 * afx_lora_fold_rows: afx_lora_fold's arguments plus row_gain, a HOST array of J device pointers (fp32 [O], 4-byte aligned, not overlapping dst;
 * a null entry -- or a null array -- means a plain LoRA):
 *   dst[o, i] = bf16_rne( c[o] float(base[o, i]) + sum_j (g_j[o] scales[j]) * ( sum_r B[j][o, r] * A[j][r, i] ) )
 *   c[o] = 1 + sum_{j with gain} (g_j[o] - 1)   (fp32, in adapter order),   g_j[o] = 1 where the entry is null
 * g_j[o] scales[j] is one fp32 product and c[o] w is fused with the addition of the adapters' sum: still ONE rounding to bf16, at the store.  With every
 * entry null the result is bit-identical to afx_lora_fold.  Same guards as afx_lora_fold (AFX_E_INVALID, nothing is launched). */
int afx_lora_row_gain(const void* base, int64_t ld_base, int32_t O, int32_t I, const void* A, const void* B, int32_t r, float s,
                      const float* m, float* gain, void* stream);
int afx_lora_fold_rows(const void* base, int64_t ld_base, void* dst, int64_t ld_dst, int32_t O, int32_t I, int32_t J,
                       const void* const* A, const void* const* B, const int32_t* ranks, const float* scales, const float* const* row_gain,
                       void* stream);

/* LyCORIS LoHa and LoKr adapters next to LoRA / DoRA ones: the fold over a list of TERMS of three kinds,
 *   dst[o, i] = bf16_rne( c[o] float(base[o, i]) + sum_j (g_j[o] scale_j) * D_j[o, i] ),   D_j in fp32,
 * c and g_j as afx_lora_fold_rows defines them (g_j = 1 for a term without row gains: every LoHa / LoKr term).  NOT PINNED: the two rules below are
 * LyCORIS' / ComfyUI's arithmetic restated from memory; neither library was at hand to check them.
 *   AFX_LORA_TERM_LORA  D = up . down: `down` [rank, I] bf16 (16-byte aligned), `up` [O, rank] bf16, `row_gain` null or fp32 [O] (a DoRA adapter's gains).
 *                       Exactly afx_lora_fold_rows' arithmetic: a call whose terms are all of this kind returns its bits (afx_lora_fold's without gains).
 *   AFX_LORA_TERM_LOHA  D = (up . down) (*) (up2 . down2), the element-wise product of two low-rank products (LyCORIS hada_w1_a . hada_w1_b and
 *                       hada_w2_a . hada_w2_b): `up` [O, rank], `down` [rank, I], `up2` [O, rank2], `down2` [rank2, I] bf16 as above, any ranks >= 1.
 *                       Both products are formed as a LoRA term's is (bf16 MFMAs, fp32 sums over the whole rank), multiplied element by element in
 *                       fp32 -- neither is rounded to bf16 -- and the fp32 product enters the sum by one fused multiply-add with `scale`.
 *   AFX_LORA_TERM_LOKR  D[o, i] = fl32( w1[(row0 + o) / kc, i / kd] * w2[(row0 + o) % kc, i % kd] ): rows row0 .. row0 + O of kron(w1, w2), `w1` [ka, kb]
 *                       and `w2` [kc, kd] dense fp32 (4-byte aligned), kb kd == I, 0 <= row0, row0 + O <= ka kc < 2^31.  kc and kd are arbitrary (no
 *                       multiples of the tile).  row0 lets one row slice of a fused tensor be folded without splitting the Kronecker product.
 * Fields a kind does not name are ignored, except row_gain, which must be null on a LoHa / LoKr term.  `terms` is a HOST array of J <=
 * AFX_LORA_MAX_ADAPTERS entries read before the call returns.  One work-group owns a 64 x 64 tile and walks the terms in order, each over its whole
 * rank: no split, no atomics, no workspace, bit-reproducible; the store is the one rounding to bf16.  J == 0 copies.  base / dst / O / I / leading
 * dimensions and their guards as afx_lora_fold.  AFX_E_INVALID (nothing is launched) also for: an unknown kind, a null operand of the term's kind, a
 * rank < 1, ka / kb / kc / kd < 1, kb kd != I, row0 out of range, a misaligned operand, row gains on a LoHa / LoKr term or overlapping dst.
 * Traffic: 4 B per element of the slice + the operands out of L2: HBM-bound. */
#define AFX_LORA_TERM_LORA 0
#define AFX_LORA_TERM_LOHA 1
#define AFX_LORA_TERM_LOKR 2
typedef struct afx_lora_term {
  int32_t kind;             /* AFX_LORA_TERM_* */
  int32_t rank;             /* LoRA: rank; LoHa: rank of the first pair */
  int32_t rank2;            /* LoHa: rank of the second pair */
  float scale;              /* fp32 factor of the term's fp32 delta */
  const void* down;         /* LoRA: A [rank, I]; LoHa: hada_w1_b [rank, I] */
  const void* up;           /* LoRA: B [O, rank]; LoHa: hada_w1_a [O, rank] */
  const void* down2;        /* LoHa: hada_w2_b [rank2, I] */
  const void* up2;          /* LoHa: hada_w2_a [O, rank2] */
  const float* row_gain;    /* LoRA: null or fp32 [O] */
  const float* w1;          /* LoKr: fp32 [ka, kb] */
  const float* w2;          /* LoKr: fp32 [kc, kd] */
  int32_t ka;
  int32_t kb;
  int32_t kc;
  int32_t kd;
  int64_t row0;             /* LoKr: the slice's first row in the virtual [ka kc, kb kd] delta */
} afx_lora_term;
int afx_lora_fold_terms(const void* base, int64_t ld_base, void* dst, int64_t ld_dst, int32_t O, int32_t I, int32_t J,
                        const afx_lora_term* terms, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ARCFLOW_HIP_H_ */
