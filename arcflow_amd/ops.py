"""torch-tensor wrappers over the exported building-block kernels of libarcflow_hip.so.

Used by the pipelines (analytic step), the distillation loop and the per-kernel parity tests.
No fallback: every function launches a HIP kernel or raises.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional, Tuple

import torch

from . import _lib


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gpu(*tensors, name: str = '') -> None:
    """Every tensor given (None entries are skipped) must live on the GPU: the kernels take device pointers."""
    for t in tensors:
        if t is not None and t.device.type != 'cuda':
            raise _lib.ArcflowHipError((name and name + ': ') + 'arcflow_amd.ops works on GPU tensors only (no CPU fallback)')


def _cuda(t: torch.Tensor, dtype) -> torch.Tensor:
    _gpu(t)
    return t.to(dtype).contiguous()


# Argument checks of the training-step wrappers: the kernels take a base pointer and a row stride and trust everything else, so a
# transposed view, a wrong dtype or a short accumulator would give wrong numbers (or touch memory past the tensor) without an error.
def _mat(t: torch.Tensor, dtype, name: str, shape=None) -> torch.Tensor:
    """A [rows, cols] operand read row by row: 2-D, on the GPU, ``dtype``, unit inner stride (any row stride)."""
    _gpu(t, name=name)
    if t.dim() != 2 or t.dtype != dtype or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f'{name}: need a 2-D {dtype} tensor with unit inner stride, got {tuple(t.shape)} {t.dtype} strides {t.stride()}')
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f'{name}: shape {tuple(t.shape)} != {tuple(shape)}')
    return t


def _acc(t: torch.Tensor, shape, name: str) -> torch.Tensor:
    """An fp32 accumulator written through a flat index: contiguous, exactly ``shape``."""
    _gpu(t, name=name)
    if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError(f'{name}: need a contiguous float32 accumulator of shape {tuple(shape)}, got {tuple(t.shape)} {t.dtype} '
                         f'strides {t.stride()}')
    return t


def _rows_f32(v: torch.Tensor, R: int, C: int, rows_per_batch: int, name: str) -> torch.Tensor:
    """A per-batch fp32 row vector (gate / scale) [C] or [Bg, C] -> [Bg, C] with unit inner stride.  A row-strided fp32 view is passed
    as it is (its rows 16-byte aligned: the kernels read it in float4); several rows need rows_per_batch with R == rows_per_batch * Bg."""
    _gpu(v, name=name)
    if v.dim() == 1:
        v = v[None]
    if v.dim() != 2 or v.shape[1] != C:
        raise ValueError(f'{name}: need [{C}] or [batch, {C}], got {tuple(v.shape)}')
    if not (v.dtype == torch.float32 and v.stride(1) == 1 and v.stride(0) % 4 == 0 and v.data_ptr() % 16 == 0):
        v = v.to(torch.float32).contiguous()
    if rows_per_batch > 0:
        if R != rows_per_batch * v.shape[0]:
            raise ValueError(f'{name}: {R} rows != rows_per_batch {rows_per_batch} x {v.shape[0]} {name} rows')
    elif v.shape[0] != 1:
        raise ValueError(f'{name}: {v.shape[0]} {name} rows need rows_per_batch')
    return v


def linear(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, epilogue: str = 'none',
           gelu_col0: int = 0, gate: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
           rows_per_batch: int = 0, out: Optional[torch.Tensor] = None, pre: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = epi(a @ w.T + bias + pre); a [M,K] (last-dim contiguous, may be a strided view), w [N,K] bf16.
    epilogue: 'none' | 'gelu' (tanh, on columns >= gelu_col0) | 'gate_res' (residual + gate[b] * (.)).
    pre [M,N] bf16 is added before the activation / gate (LoRA-dropout correction)."""
    lib = _lib.load()
    assert a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and a.stride(-1) == 1 and w.stride(-1) == 1
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    epi = {'none': 0, 'gelu': 1, 'gate_res': 2}[epilogue]
    if gate is not None:
        gate = _cuda(gate, torch.float32)
        if gate.dim() == 1:
            gate = gate[None]
    rpb = rows_per_batch if rows_per_batch > 0 else max(M, 1)
    _lib.check(lib.afx_linear_bf16_pre(_p(a), a.stride(0), _p(w), w.stride(0), _p(bias), _p(out), out.stride(0), M, N, K,
                                       epi, gelu_col0, _p(gate), 0 if gate is None else gate.stride(0), rpb,
                                       _p(residual), 0 if residual is None else residual.stride(0),
                                       _p(pre), 0 if pre is None else pre.stride(0), _s()))
    return out


def set_gemm_mode(impl: int = 3, tile: int = 0) -> None:
    """Kernel / tile-shape override of every bf16 GEMM (``afx_gemm_set_mode``): impl 3 = one-wave-per-SIMD kernel with tile 0 = picked
    per launch, 1 ... 6 = 256x256 / 288x192 / 320x192 / 128x128 / 256x224 / 224x256; impl 2 = 8-phase 256x256 kernel (any other impl: 3)."""
    _lib.check(_lib.load().afx_gemm_set_mode(impl, tile))


def set_fp8_tile(tile: int = 0) -> int:
    """Tile shape of the one-wave-per-SIMD fp8 GEMM (``afx_gemm_set_fp8_tile``): 0 = picked per launch, 1 = 256x256, 2 = 224x256 (any other
    value: 0).  Returns the setting now in force."""
    return _lib.load().afx_gemm_set_fp8_tile(tile)


def set_attn_impl(impl: int = 0) -> None:
    """Kernel choice of the joint attention (``afx_attn_set_impl``): 0 = one-wave-per-SIMD kernel where eligible, the blocks of an under-filled
    last round KV-split (default), 1 = 4-wave kernel always, 3 = as 0 on the plain grid (any other value: 0)."""
    _lib.check(_lib.load().afx_attn_set_impl(impl))


def set_attn_bwd_impl(impl: int = 3) -> None:
    """Kernel generation of ``attention_bwd`` (``afx_attn_bwd_set_impl``): 3 = generated dK / dV + dQ streams in one launch (default), 4 = as two launches,
    1 = generated dK / dV + round-4 dQ, 2 = the round-4 kernels."""
    _lib.check(_lib.load().afx_attn_bwd_set_impl(impl))


def lora_dropout(src: torch.Tensor, p: float, seed: int, row0: int = 0, mode: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Counter-based LoRA input dropout (keep probability 1-p, delta = keep/(1-p) - 1):
    mode 0: out = src * delta;  1: out = src * (1 + delta) = dropout(src);  2: out += src * delta;  3: out += src * (1 + delta)."""
    lib = _lib.load()
    M, N = src.shape
    if out is None:
        assert mode < 2
        out = torch.empty(M, N, dtype=torch.bfloat16, device=src.device)
    _lib.check(lib.afx_lora_dropout_bf16(_p(src), src.stride(0), _p(out), out.stride(0), M, N, row0, float(p), int(seed) & 0xffffffff, mode, _s()))
    return out


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """q,k,v [B,S,H,128] bf16 (last two dims contiguous) -> [B,S,H*128]; softmax(q k^T/sqrt(128)) v."""
    lib = _lib.load()
    B, S, H, Dh = q.shape
    assert Dh == 128 and q.dtype == torch.bfloat16
    q2, k2, v2 = (t.reshape(B * S, H * Dh) for t in (q.contiguous(), k.contiguous(), v.contiguous()))
    o = torch.empty(B * S, H * Dh, dtype=torch.bfloat16, device=q.device)
    ws = torch.empty(lib.afx_attention_ws_bytes(B, H, S), dtype=torch.uint8, device=q.device)
    _lib.check(lib.afx_attention_bf16(_p(q2), H * Dh, _p(k2), H * Dh, _p(v2), H * Dh, _p(o), H * Dh, _p(ws), B, H, S, _s()))
    return o.reshape(B, S, H * Dh)


def attention_to_mx8(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out=None):
    """``attention`` with the output as a block-scaled fp8 operand: (uint8 [B*S, H*128] e4m3, uint8 [B*S, H] E8M0 -- one scale per token and head).
    out: (o8, mx) row-strided views to write into (row strides multiples of 16 / 4)."""
    lib = _lib.load()
    B, S, H, Dh = q.shape
    assert Dh == 128 and q.dtype == torch.bfloat16
    q2, k2, v2 = (t.reshape(B * S, H * Dh) for t in (q.contiguous(), k.contiguous(), v.contiguous()))
    if out is None:
        o8 = torch.empty(B * S, H * Dh, dtype=torch.uint8, device=q.device)
        mx = torch.empty(B * S, (H + 3) // 4 * 4, dtype=torch.uint8, device=q.device)
    else:
        o8, mx = out
        assert o8.shape == (B * S, H * Dh) and mx.shape[0] == B * S and mx.shape[1] >= H and o8.dtype == mx.dtype == torch.uint8
        assert o8.stride(1) == 1 and mx.stride(1) == 1 and o8.stride(0) % 16 == 0 and mx.stride(0) % 4 == 0
    ws = torch.empty(lib.afx_attention_ws_bytes(B, H, S), dtype=torch.uint8, device=q.device)
    _lib.check(lib.afx_attention_to_mx8(_p(q2), H * Dh, _p(k2), H * Dh, _p(v2), H * Dh, _p(o8), o8.stride(0), _p(mx), mx.stride(0), _p(ws), B, H, S, _s()))
    return o8, mx[:, :H]


def norm_modulate(x: torch.Tensor, scale: torch.Tensor, shift: Optional[torch.Tensor], rows_per_batch: int = 0,
                  rms: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [R,D] bf16; AdaLN: scale/shift [B,D] f32 (row r uses batch r // rows_per_batch);
    rms=True: x * rsqrt(mean x^2 + 1e-6) * scale[D].  Two fp32 [B,D] column views of one stacked modulation tensor (unit inner stride, the
    same row stride, 16-byte aligned rows) are read in place, as the forward's single blocks read them; anything else is copied."""
    lib = _lib.load()
    R, D = x.shape
    if out is None:
        out = torch.empty(R, D, dtype=torch.bfloat16, device=x.device)
    _gpu(scale, shift)
    in_place = not rms and shift is not None and all(
        v.dim() == 2 and v.dtype == torch.float32 and v.stride(1) == 1 and v.stride(0) % 4 == 0 and v.data_ptr() % 16 == 0
        for v in (scale, shift)) and scale.stride(0) == shift.stride(0)
    if not in_place:
        scale = _cuda(scale, torch.float32)
        shift = None if shift is None else _cuda(shift, torch.float32)
    ldm = 0 if rms or scale.dim() == 1 else scale.stride(0)
    _lib.check(lib.afx_norm_modulate_bf16(_p(x), x.stride(0), _p(out), out.stride(0), R, D, _p(scale), _p(shift), ldm,
                                          rows_per_batch if rows_per_batch > 0 else max(R, 1), int(rms), _s()))
    return out


def qk_norm_rope_(x: torch.Tensor, w_txt: torch.Tensor, w_img: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                  n_txt: int) -> torch.Tensor:
    """In place on x [B,S,H,128] bf16: per-head RMSNorm (rows < n_txt use w_txt) then pair RoPE."""
    lib = _lib.load()
    B, S, H, Dh = x.shape
    assert x.is_contiguous() and Dh == 128
    _lib.check(lib.afx_qk_norm_rope_bf16(_p(x), H * Dh, _p(_cuda(w_txt, torch.float32)), _p(_cuda(w_img, torch.float32)),
                                         _p(_cuda(cos, torch.float32)), _p(_cuda(sin, torch.float32)), B, S, n_txt, H, _s()))
    return x


def _joint_vectors(vecs, B: int, D: int, name: str) -> int:
    """The AdaLN vectors of a joint launch: each [B, D] fp32 (or [D] when B == 1), unit inner stride, 16-byte aligned rows, all with the
    same row stride (the kernels take one ldmod).  Returns that stride."""
    ld = None
    for v, n in vecs:
        _gpu(v, name=f'{name} {n}')
        v2 = v[None] if v.dim() == 1 else v
        if v2.dim() != 2 or tuple(v2.shape) != (B, D) or v2.dtype != torch.float32 or v2.stride(1) != 1 or v2.data_ptr() % 16:
            raise ValueError(f'{name} {n}: need a [{B}, {D}] float32 tensor with unit inner stride and 16-byte aligned rows, got '
                             f'{tuple(v.shape)} {v.dtype} strides {v.stride()}')
        s = v2.stride(0) if B > 1 else 0
        if s % 4 or (ld is not None and s != ld):
            raise ValueError(f'{name} {n}: every modulation vector needs the same row stride (a multiple of 4), got {v2.stride(0)}')
        ld = s
    return ld


def _joint_norm_args(x, scale, shift, S, scale_txt, shift_txt, n_txt, name):
    _mat(x, torch.bfloat16, f'{name} x')
    R, D = x.shape
    if S < 1 or R % S:
        raise ValueError(f'{name}: {R} rows are not a whole number of samples of S = {S}')
    if (scale_txt is None) != (shift_txt is None) or not 0 <= n_txt <= S or (scale_txt is None and n_txt):
        raise ValueError(f'{name}: text vectors need both scale_txt and shift_txt and 0 <= n_txt <= S (n_txt 0 without them)')
    vecs = [(scale, 'scale'), (shift, 'shift')] + ([] if scale_txt is None else [(scale_txt, 'scale_txt'), (shift_txt, 'shift_txt')])
    return R, D, _joint_vectors(vecs, R // S, D, name)


def norm_modulate_joint(x, scale, shift, S: int, scale_txt=None, shift_txt=None, n_txt: int = 0, out=None):
    """AdaLN of the joint token matrix x [B*S, D] bf16 in one launch (the forward's double blocks): LayerNorm(x) * (1 + scale[b]) + shift[b],
    the first n_txt rows of every sample with (scale_txt, shift_txt).  Vectors [B, D] fp32 views with one common row stride."""
    lib = _lib.load()
    R, D, ldm = _joint_norm_args(x, scale, shift, S, scale_txt, shift_txt, n_txt, 'norm_modulate_joint')
    if out is None:
        out = torch.empty(R, D, dtype=torch.bfloat16, device=x.device)
    _mat(out, torch.bfloat16, 'norm_modulate_joint out', (R, D))
    _lib.check(lib.afx_norm_modulate_joint_bf16(_p(x), x.stride(0), _p(out), out.stride(0), R, D, _p(scale), _p(shift), _p(scale_txt),
                                                _p(shift_txt), ldm, S, n_txt, _s()))
    return out


def norm_modulate_mx8(x, scale, shift, S: int, scale_txt=None, shift_txt=None, n_txt: int = 0, row_scale: bool = False):
    """``norm_modulate_joint`` straight into the next fp8 GEMM's operand: returns (q uint8 [R, D] e4m3, scales, fused) with scales = uint8
    [R, D / 128] E8M0 bytes (block-scaled) or, row_scale=True, fp32 [R] (absmax / 448 per row).  fused False: this shape has no fused
    kernel and nothing was launched (q and scales are uninitialised)."""
    lib = _lib.load()
    R, D, ldm = _joint_norm_args(x, scale, shift, S, scale_txt, shift_txt, n_txt, 'norm_modulate_mx8')
    q = torch.empty(R, D, dtype=torch.uint8, device=x.device)
    nb = (D + 127) // 128
    mx = None if row_scale else torch.empty(R, (nb + 3) // 4 * 4, dtype=torch.uint8, device=x.device)
    rs = torch.empty(R, dtype=torch.float32, device=x.device) if row_scale else None
    fused = C.c_int32(0)
    _lib.check(lib.afx_norm_modulate_mx8(_p(x), x.stride(0), _p(q), D, _p(mx), 0 if mx is None else mx.stride(0), _p(rs), R, D, _p(scale),
                                         _p(shift), _p(scale_txt), _p(shift_txt), ldm, S, n_txt, C.byref(fused), _s()))
    return q, (rs if row_scale else mx[:, :nb]), bool(fused.value)


def qkv_operands(kind: str, a, w, bias, qkn, cos, sin, B: int, N: int, T: int, path: str = 'auto', out=None, vt=None):
    """The attention operands of one block as the forward builds them (``afx_qkv_operands``).  a [B*(N+T), D] bf16 AdaLN rows (joint layout,
    row-strided view allowed); kind 'double': w = (w_img, w_txt) [3D, D], bias = (b_img, b_txt) [3D] or None, qkn [4, 128]
    (img_q, img_k, txt_q, txt_k); kind 'single': w [7D, D], bias [7D] or None, qkn [2, 128] (q, k).  cos / sin [N+T, 64] fp32.
    path: 'auto' (the forward's choice) | 'vt_proj' | 'qk_epi' | 'kv_prep'.  Returns (out [B*(N+T), 3D or 7D] bf16, which may be a
    column view of a wider buffer, vt [B, H, 128, roundup(N+T, 64)] bf16)."""
    lib = _lib.load()
    if kind not in ('double', 'single') or path not in _lib.AFX_QKV_PATHS:
        raise ValueError(f'qkv_operands: kind {kind!r} / path {path!r}')
    single = kind == 'single'
    S = N + T
    _mat(a, torch.bfloat16, 'qkv_operands a')
    R, D = a.shape
    if D % 128 or R != B * S:
        raise ValueError(f'qkv_operands a: need [{B} x {S}, heads x 128], got {tuple(a.shape)}')
    H, width = D // 128, (7 if single else 3) * D
    ws = (w,) if single else tuple(w)
    bs = (bias,) if single else ((None, None) if bias is None else tuple(bias))
    if len(ws) != (1 if single else 2) or len(bs) != len(ws):
        raise ValueError('qkv_operands: a double block takes (w_img, w_txt) and (b_img, b_txt) or None')
    for i, t in enumerate(ws):
        _mat(t, torch.bfloat16, f'qkv_operands w[{i}]', ((width, D)))
        if not t.is_contiguous():
            raise ValueError(f'qkv_operands w[{i}]: the weight rows must be contiguous (row stride D)')
    for i, t in enumerate(bs):
        if t is not None and (t.device.type != 'cuda' or t.dtype != torch.bfloat16 or not t.is_contiguous() or tuple(t.shape) != (width,)):
            raise ValueError(f'qkv_operands bias[{i}]: need a contiguous bf16 [{width}] tensor')
    if sum(t is None for t in bs) not in (0, len(bs)):
        raise ValueError('qkv_operands: both streams with a bias or neither')
    for t, n, shp in ((qkn, 'qkn', (2 if single else 4, 128)), (cos, 'cos', (S, 64)), (sin, 'sin', (S, 64))):
        if t.device.type != 'cuda' or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shp:
            raise ValueError(f'qkv_operands {n}: need a contiguous float32 {list(shp)} tensor, got {tuple(t.shape)} {t.dtype}')
    S_pad = (S + 63) // 64 * 64
    if out is None:
        out = torch.empty(R, width, dtype=torch.bfloat16, device=a.device)
    _mat(out, torch.bfloat16, 'qkv_operands out', (R, width))
    if vt is None:
        vt = torch.empty(B, H, 128, S_pad, dtype=torch.bfloat16, device=a.device)
    if vt.device.type != 'cuda' or vt.dtype != torch.bfloat16 or not vt.is_contiguous() or tuple(vt.shape) != (B, H, 128, S_pad):
        raise ValueError(f'qkv_operands vt: need a contiguous bf16 [{B}, {H}, 128, {S_pad}] workspace, got {tuple(vt.shape)} {vt.dtype}')
    w_img, w_txt = ws[0], (None if single else ws[1])
    b_img, b_txt = bs[0], (None if single else bs[1])
    _lib.check(lib.afx_qkv_operands(_lib.AFX_BLOCK_SINGLE if single else _lib.AFX_BLOCK_DOUBLE, _p(a), a.stride(0), _p(w_img), _p(b_img),
                                    _p(w_txt), _p(b_txt), _p(qkn), _p(cos), _p(sin), B, N, T, H, _lib.AFX_QKV_PATHS[path], _p(out),
                                    out.stride(0), _p(vt), _s()))
    return out, vt


def gemv(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: str = 'none',
         out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    lib = _lib.load()
    x = _cuda(x, torch.float32)
    B, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.zeros(B, N, dtype=torch.float32, device=x.device)
    _lib.check(lib.afx_gemv_bf16(_p(x), _p(w), _p(bias), _p(out), B, N, K, 1 if act == 'silu' else 0, int(accumulate), _s()))
    return out


def _mix_dtype(means, logw, logg) -> Tuple[int, torch.Tensor, torch.Tensor, torch.Tensor]:
    if means.dtype == torch.bfloat16:
        return _lib.AFX_DT_BF16, means.contiguous(), logw.to(torch.bfloat16).contiguous(), logg.to(torch.bfloat16).contiguous()
    return _lib.AFX_DT_F32, means.float().contiguous(), logw.float().contiguous(), logg.float().contiguous()


def _sigma_vec(B, device, *sig):
    cols = [torch.as_tensor(x, dtype=torch.float32, device=device).flatten().expand(B) for x in sig]
    return torch.stack(cols, dim=1).contiguous()


def _mix_operands(means, logw, logg):
    """(B, N, K, ch, pp), the mixture's dtype code and its three tensors, contiguous in that dtype"""
    return (*means.shape, logw.shape[-1]), *_mix_dtype(means, logw, logg)


def arcflow_step(x: torch.Tensor, means: torch.Tensor, logw: torch.Tensor, logg: torch.Tensor, sigma_src, sigma_start,
                 sigma_end, eps: float = 1e-4, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Analytic ArcFlow transport in the token layout: x [B,N,ch] f32, means [B,N,K,ch], logw [B,N,K,pp],
    logg [B,N,K-1,pp]  ->  x_end [B,N,ch] f32.  sigmas: python floats, or [B] tensors (per-sample)."""
    lib = _lib.load()
    (B, N, K, ch, pp), dt, means, logw, logg = _mix_operands(means, logw, logg)
    x = _cuda(x, torch.float32)
    if out is None:
        out = torch.empty_like(x)
    sv = None
    if any(isinstance(s, torch.Tensor) and s.numel() > 1 for s in (sigma_src, sigma_start, sigma_end)):
        sv = _sigma_vec(B, x.device, sigma_src, sigma_start, sigma_end)
        s0 = s1 = s2 = 0.0
    else:
        s0, s1, s2 = (float(s) for s in (sigma_src, sigma_start, sigma_end))
    _lib.check(lib.afx_arcflow_step(_p(x), _p(means), _p(logw), _p(logg), dt, s0, s1, s2, _p(sv), eps, _p(out),
                                    B, N, K, ch, pp, _s()))
    return out


def arcflow_velocity(means: torch.Tensor, logw: torch.Tensor, logg: torch.Tensor, sigma_src, sigma_t) -> torch.Tensor:
    """u(sigma_t) of the momentum mixture, token layout -> [B,N,ch] f32."""
    lib = _lib.load()
    (B, N, K, ch, pp), dt, means, logw, logg = _mix_operands(means, logw, logg)
    out = torch.empty(B, N, ch, dtype=torch.float32, device=means.device)
    sv = None
    if any(isinstance(s, torch.Tensor) and s.numel() > 1 for s in (sigma_src, sigma_t)):
        sv = _sigma_vec(B, out.device, sigma_src, sigma_t, sigma_t)
        s0 = s1 = 0.0
    else:
        s0, s1 = float(sigma_src), float(sigma_t)
    _lib.check(lib.afx_arcflow_velocity(_p(means), _p(logw), _p(logg), dt, s0, s1, _p(sv), _p(out), B, N, K, ch, pp, _s()))
    return out


# ---------------------------------------------------------------------------------------------------
# distillation-step kernels
def arcflow_step_dropout(x, means, logw, logg, sigma_src, sigma_start, sigma_end, drop_mask=None, eps: float = 1e-4):
    """Roll-out step of the detached policy with per-sample sigmas and GM dropout mask [B,K] (bool/uint8)."""
    lib = _lib.load()
    (B, N, K, ch, pp), dt, means, logw, logg = _mix_operands(means, logw, logg)
    x = _cuda(x, torch.float32)
    sv = _sigma_vec(B, x.device, sigma_src, sigma_start, sigma_end)
    dm = None if drop_mask is None else drop_mask.to(device=x.device, dtype=torch.uint8).reshape(B, K).contiguous()
    out = torch.empty_like(x)
    _lib.check(lib.afx_arcflow_step_dropout(_p(x), _p(means), _p(logw), _p(logg), dt, _p(sv), _p(dm), eps, _p(out),
                                            B, N, K, ch, pp, _s()))
    return out


def arcflow_backward(g, means, logw, logg, sigma_src, sigma_start, sigma_end, gscale=None, velocity: bool = False,
                     grads=None, eps: float = 1e-4):
    """Gradients of the displacement (or velocity) w.r.t. the mixture.  g [B,N,ch] upstream gradient, gscale [B]
    optional per-sample factor.  grads = (d_means, d_logw, d_logg) fp32 to accumulate into, else fresh tensors."""
    lib = _lib.load()
    (B, N, K, ch, pp), dt, means, logw, logg = _mix_operands(means, logw, logg)
    g = _cuda(g, torch.float32)
    sv = _sigma_vec(B, g.device, sigma_src, sigma_start, sigma_end)
    gs = None if gscale is None else _cuda(torch.as_tensor(gscale, device=g.device).flatten().expand(B), torch.float32)
    acc = grads is not None
    if not acc:
        grads = (torch.empty(B, N, K, ch, dtype=torch.float32, device=g.device),
                 torch.empty(B, N, K, pp, dtype=torch.float32, device=g.device),
                 torch.empty(B, N, K - 1, pp, dtype=torch.float32, device=g.device))
    _lib.check(lib.afx_arcflow_backward(_p(g), _p(means), _p(logw), _p(logg), dt, 0.0, 0.0, 0.0, _p(sv), _p(gs), 1.0, eps,
                                        _p(grads[0]), _p(grads[1]), _p(grads[2]), B, N, K, ch, pp, int(velocity), int(acc), _s()))
    return grads


def mse_loss(pred, target, coef: float, loss_accum: torch.Tensor, want_grad: bool = True):
    lib = _lib.load()
    pred, target = _cuda(pred, torch.float32), _cuda(target, torch.float32)
    grad = torch.empty_like(pred) if want_grad else None
    _lib.check(lib.afx_mse_loss(_p(pred), _p(target), coef, _p(grad), _p(loss_accum), pred.numel(), _s()))
    return grad


def euler_roll(x_a, u, sigma_a, sigma_b):
    lib = _lib.load()
    x_a, u = _cuda(x_a, torch.float32), _cuda(u, torch.float32)
    B = x_a.shape[0]
    sa = _cuda(sigma_a.flatten().expand(B), torch.float32)
    sb = _cuda(sigma_b.flatten().expand(B), torch.float32)
    out = torch.empty_like(x_a)
    _lib.check(lib.afx_euler_roll(_p(x_a), _p(u), _p(sa), _p(sb), _p(out), B, x_a[0].numel(), _s()))
    return out


def forward_diffuse_pack(x0, noise, sigma, want_bf16: bool = True):
    """x_t = x0 (1 - sigma[b]) + noise sigma[b] in the engine's token layout: x0 [B,16,H,W] fp32 latents, noise [B,N,64] token-major,
    sigma [B] -> (x_t [B,N,64] fp32, its bf16 rounding or None)."""
    lib = _lib.load()
    x0, noise = _cuda(x0, torch.float32), _cuda(noise, torch.float32)
    if x0.dim() != 4 or x0.shape[2] % 2 or x0.shape[3] % 2:
        raise ValueError(f'x0: need [B, C, H, W] latents with even H and W, got {tuple(x0.shape)}')
    B, Cc, H, W = x0.shape
    N = (H // 2) * (W // 2)
    if tuple(noise.shape) != (B, N, 4 * Cc):
        raise ValueError(f'noise: need the token layout {(B, N, 4 * Cc)}, got {tuple(noise.shape)}')
    sg = _cuda(sigma.flatten(), torch.float32)
    if sg.numel() != B:
        raise ValueError(f'sigma: need {B} values, got {sg.numel()}')
    xt = torch.empty_like(noise)
    xt16 = torch.empty(noise.shape, dtype=torch.bfloat16, device=noise.device) if want_bf16 else None
    _lib.check(lib.afx_forward_diffuse_pack(_p(x0), _p(noise), _p(sg), _p(xt), _p(xt16), B, Cc, H, W, _s()))
    return xt, xt16


def axpby_rows(a, alpha, b, beta):
    """alpha[s] * a + beta[s] * b with per-sample scalars alpha, beta [B]."""
    lib = _lib.load()
    a, b = _cuda(a, torch.float32), _cuda(b, torch.float32)
    B = a.shape[0]
    al, be = _cuda(alpha.flatten().expand(B), torch.float32), _cuda(beta.flatten().expand(B), torch.float32)
    out = torch.empty_like(a)
    _lib.check(lib.afx_axpby_rows(_p(a), _p(al), _p(b), _p(be), _p(out), B, a[0].numel(), _s()))
    return out


def cfg_combine(pos, neg, scale: float):
    lib = _lib.load()
    pos, neg = _cuda(pos, torch.float32), _cuda(neg, torch.float32)
    out = torch.empty_like(pos)
    _lib.check(lib.afx_cfg_combine(_p(pos), _p(neg), scale, _p(out), pos.numel(), _s()))
    return out


def _packed(t: torch.Tensor, dtype, shape, name: str) -> torch.Tensor:
    """An operand of the teacher-sampler kernels: on the GPU, ``dtype``, contiguous, exactly ``shape`` -- passed as it is (no copy)."""
    _gpu(t, name=name)
    if t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError(f'{name}: need a contiguous {dtype} tensor of shape {tuple(shape)}, got {tuple(t.shape)} {t.dtype} strides {t.stride()}')
    return t


def _ws(lib_fn, *args, device, min_one: bool) -> torch.Tensor:
    """The float64 workspace of lib_fn(*args) bytes (a *_ws_bytes entry; its refusal raises).  min_one: one element where no bytes are needed."""
    need = lib_fn(*args)
    if need < 0:
        _lib.check(int(need))
    return torch.empty(max(need // 8, 1) if min_one else need // 8, dtype=torch.float64, device=device)


def cfg_ortho_ws(batch: int, n: int, device='cuda') -> torch.Tensor:
    """Workspace of cfg_ortho_coef for [batch, n] velocities (afx_cfg_ortho_ws_bytes): fp64 partial sums, one pair per work-group."""
    return _ws(_lib.load().afx_cfg_ortho_ws_bytes, batch, n, device=device, min_one=True)


def cfg_ortho_coef(pos, neg, scale: float, out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """coef [B] fp32 = mean(bias pos) / max(mean(pos pos), 1e-6) per sample over every other dimension, bias = (pos - neg)(scale - 1):
    the projection coefficient of orthogonal guidance (gaussian_flow.py:21-25).  pos, neg [B, ...] bf16 teacher velocities with
    numel / B a multiple of 64.  Bit-reproducible (fixed partition, exact fp64 products, ordered sum).  out / ws: reuse buffers."""
    lib = _lib.load()
    _gpu(pos, neg)
    B = pos.shape[0]
    n = pos[0].numel() if B else 0
    pos = _packed(pos, torch.bfloat16, pos.shape, 'pos')
    neg = _packed(neg, torch.bfloat16, pos.shape, 'neg')
    out = torch.empty(B, dtype=torch.float32, device=pos.device) if out is None else _packed(out, torch.float32, (B,), 'out')
    if ws is None:
        ws = cfg_ortho_ws(B, n, pos.device)
    elif ws.device.type != 'cuda' or not ws.is_contiguous():
        raise ValueError('ws: need a contiguous GPU buffer (ops.cfg_ortho_ws)')
    _lib.check(lib.afx_cfg_ortho_coef(_p(pos), _p(neg), scale, _p(out), _p(ws), ws.numel() * ws.element_size(), B, n, _s()))
    return out


def _score_operands(a, b, out, out_shape, ws, ws_fn, *ws_args):
    """The operands every scorer shares, checked: -> (a, b, out, ws, dt).  a, b both fp32 or both bf16, contiguous, of one shape; out
    [B, *out_shape] float64 (allocated when None); ws from ws_fn(B, *ws_args, device), one of the *_ws functions below, when None."""
    if a.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f'a: need float32 or bfloat16, got {a.dtype}')
    B = a.shape[0]
    a = _packed(a, a.dtype, a.shape, 'a')
    b = _packed(b, a.dtype, a.shape, 'b')
    out = torch.empty(B, *out_shape, dtype=torch.float64, device=a.device) if out is None else _packed(out, torch.float64, (B, *out_shape), 'out')
    if ws is None:
        ws = ws_fn(B, *ws_args, a.device)
    elif not ws.is_contiguous():
        raise ValueError(f'ws: need a contiguous GPU buffer (ops.{ws_fn.__name__})')
    return a, b, out, ws, _lib.AFX_DT_BF16 if a.dtype == torch.bfloat16 else _lib.AFX_DT_F32


def sample_score_ws(batch: int, n: int, device='cuda') -> torch.Tensor:
    """Workspace of sample_score for [batch, n] operands (afx_sample_score_ws_bytes): fp64 partial sums, 4 per work-group."""
    return _ws(_lib.load().afx_sample_score_ws_bytes, batch, n, device=device, min_one=True)


def sample_score(a, b, transform: bool = False, out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B, 4] float64 = (sum (a-b)^2, sum a^2, sum b^2, sum a b) per sample over every other dimension (afx_sample_score).
    a, b [B, ...], both fp32 or both bf16, contiguous, numel / B a multiple of 64.  transform: score clamp(v / 2 + 0.5, 0, 1)
    (fp32) of both operands, the [0, 1] image range.  Elements are widened to fp64; bit-reproducible (fixed partition, ordered sum).
    Nothing is copied or cast: a wrong dtype or layout raises.  out / ws: reuse buffers (ops.sample_score_ws)."""
    lib = _lib.load()
    _gpu(a, b, out, ws)
    B = a.shape[0]
    n = a[0].numel() if B else 0
    a, b, out, ws, dt = _score_operands(a, b, out, (4,), ws, sample_score_ws, n)
    _lib.check(lib.afx_sample_score(_p(a), _p(b), dt, int(bool(transform)), _p(out), _p(ws), ws.numel() * ws.element_size(), B, n, _s()))
    return out


def image_ssim_ws(batch: int, channels: int, height: int, width: int, device='cuda') -> torch.Tensor:
    """Workspace of image_ssim for [batch, channels, height, width] operands (afx_image_ssim_ws_bytes): one fp64 partial sum per work-group."""
    return _ws(_lib.load().afx_image_ssim_ws_bytes, batch, channels, height, width, device=device, min_one=False)


def image_ssim(a, b, transform: bool = False, data_range: float = 1.0, out: Optional[torch.Tensor] = None,
               ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B] float64 = per sample, the SUM of the structural similarity (11 x 11 Gaussian window, sigma 1.5, valid windows only) over the C
    channels and (H - 10)(W - 10) windows of a, b [B, C, H, W] (afx_image_ssim); the mean SSIM is the sum / (C (H - 10)(W - 10)).
    a, b both fp32 or both bf16, contiguous NCHW, H, W >= 11.  transform: score clamp(v / 2 + 0.5, 0, 1) (fp32) of both operands, the
    [0, 1] image range.  data_range: L of c1 = (0.01 L)^2, c2 = (0.03 L)^2.  Elements are widened to fp64 and everything after is fp64;
    bit-reproducible (fixed partition, fixed order of the sum).  Nothing is copied or cast: a wrong dtype, device, layout or rank raises.
    out / ws: reuse buffers (ops.image_ssim_ws)."""
    lib = _lib.load()
    _gpu(a, b, out, ws)
    if a.dim() != 4:
        raise ValueError(f'a: need [B, C, H, W], got {tuple(a.shape)}')
    B, Cn, H, W = a.shape
    a, b, out, ws, dt = _score_operands(a, b, out, (), ws, image_ssim_ws, Cn, H, W)
    _lib.check(lib.afx_image_ssim(_p(a), _p(b), dt, int(bool(transform)), float(data_range), _p(out), _p(ws), ws.numel() * ws.element_size(),
                                  B, Cn, H, W, _s()))
    return out


def _score_mask_view(a, mask):
    """(G, P, R, Q) of afx_sample_score_masked for operands a [B, ...] and a mask: packed tokens [B, N, 64] with [Bm, N, 4] (the operand of
    edit_blend), or images [B, C, H, W] with [Bm, 1, H, W]."""
    if a.dim() == 3 and mask.dim() == 3 and mask.shape[1] == a.shape[1] and mask.shape[2] >= 1 and a.shape[2] % mask.shape[2] == 0:
        return 1, a.shape[1], a.shape[2], mask.shape[2]
    if a.dim() == 4 and mask.dim() == 4 and mask.shape[1] == 1 and tuple(mask.shape[2:]) == tuple(a.shape[2:]):
        return a.shape[1], a.shape[2] * a.shape[3], 1, 1
    raise ValueError(f'mask: need [B or 1, N, Q] (Q dividing C) for a [B, N, C], or [B or 1, 1, H, W] for a [B, C, H, W]; got {tuple(mask.shape)} '
                     f'for a {tuple(a.shape)}')


def sample_score_masked_ws(batch: int, n: int, device='cuda') -> torch.Tensor:
    """Workspace of sample_score_masked for [batch, n] operands (afx_sample_score_masked_ws_bytes): fp64 partial sums, 10 per work-group."""
    return _ws(_lib.load().afx_sample_score_masked_ws_bytes, batch, n, device=device, min_one=True)


def sample_score_masked(a, b, mask, transform: bool = False, out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B, 2, 5] float64 = per sample and region (sum w, sum w (a-b)^2, sum w a^2, sum w b^2, sum w a b): region 0 the repainted one,
    w = mask, region 1 the kept one, w = 1 - mask (afx_sample_score_masked).  a, b as sample_score takes them, either packed tokens
    [B, N, 64] with the [B or 1, N, 4] fp32 mask of edit_blend / schedule.mask_to_tokens, or images [B, C, H, W] with a [B or 1, 1, H, W]
    fp32 mask; a mask batch of 1 is shared.  Bit-reproducible; with mask = 1 region 0's last four sums are sample_score's bit for bit.
    Nothing is copied or cast: a wrong dtype or layout raises.  out / ws: reuse buffers (ops.sample_score_masked_ws)."""
    lib = _lib.load()
    _gpu(a, b, mask, out, ws)
    G, Pn, R, Q = _score_mask_view(a, mask)
    mask = _packed(mask, torch.float32, mask.shape, 'mask')
    B = a.shape[0]
    a, b, out, ws, dt = _score_operands(a, b, out, (2, 5), ws, sample_score_masked_ws, a[0].numel() if B else 0)
    _lib.check(lib.afx_sample_score_masked(_p(a), _p(b), _p(mask), dt, int(bool(transform)), _p(out), _p(ws), ws.numel() * ws.element_size(),
                                           B, mask.shape[0], G, Pn, R, Q, _s()))
    return out


def image_ssim_masked_ws(batch: int, channels: int, height: int, width: int, device='cuda') -> torch.Tensor:
    """Workspace of image_ssim_masked (afx_image_ssim_masked_ws_bytes): four fp64 partial sums per work-group."""
    return _ws(_lib.load().afx_image_ssim_masked_ws_bytes, batch, channels, height, width, device=device, min_one=False)


def image_ssim_masked(a, b, mask, transform: bool = False, data_range: float = 1.0, out: Optional[torch.Tensor] = None,
                      ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[B, 4] float64 = per sample (sum w ssim, sum w, sum (1 - w) ssim, sum (1 - w)) over the C channels and (H - 10)(W - 10) windows of
    a, b [B, C, H, W] (afx_image_ssim_masked): image_ssim's window SSIM, every window weighted by w = the Gaussian-weighted mean of
    mask [B or 1, 1, H, W] (fp32, in [0, 1]) over the window's own support.  [:, 0] / [:, 1] is the mean SSIM of the repainted region,
    [:, 2] / [:, 3] that of the kept region.  transform, data_range, dtypes and layout as image_ssim; bit-reproducible.  Nothing is
    copied or cast: a wrong dtype, device, layout or rank raises.  out / ws: reuse buffers (ops.image_ssim_masked_ws)."""
    lib = _lib.load()
    _gpu(a, b, mask, out, ws)
    if a.dim() != 4:
        raise ValueError(f'a: need [B, C, H, W], got {tuple(a.shape)}')
    B, Cn, H, W = a.shape
    if mask.dim() != 4 or tuple(mask.shape[1:]) != (1, H, W):
        raise ValueError(f'mask: need [B or 1, 1, {H}, {W}], got {tuple(mask.shape)}')
    mask = _packed(mask, torch.float32, mask.shape, 'mask')
    a, b, out, ws, dt = _score_operands(a, b, out, (4,), ws, image_ssim_masked_ws, Cn, H, W)
    _lib.check(lib.afx_image_ssim_masked(_p(a), _p(b), _p(mask), dt, int(bool(transform)), float(data_range), _p(out), _p(ws),
                                         ws.numel() * ws.element_size(), B, mask.shape[0], Cn, H, W, _s()))
    return out


_FILTERS = {'lanczos3': 'AFX_FILTER_LANCZOS3', 'triangle': 'AFX_FILTER_TRIANGLE'}


def _axis_table(n_in: int, n_out: int, filt: int, b0: float, b1: float, sigma: float):
    """One axis' table from afx_resample_table (a host function: no GPU is touched): (start [n_out] int32, count [n_out] int32,
    w [n_out, taps] float32) on the CPU.  The C function's refusals (bad size, box, sigma, too many taps) are raised as ValueError."""
    lib = _lib.load()
    taps = lib.afx_resample_table(n_in, n_out, filt, b0, b1, sigma, None, None, None, _lib.AFX_RESAMPLE_MAX_TAPS)
    if taps < 0:
        raise ValueError(lib.afx_last_error().decode())
    start = torch.empty(n_out, dtype=torch.int32)
    count = torch.empty(n_out, dtype=torch.int32)
    w = torch.empty(n_out, taps, dtype=torch.float32)
    rc = lib.afx_resample_table(n_in, n_out, filt, b0, b1, sigma, _p(start), _p(count), _p(w), taps)
    if rc != taps:
        _lib.check(rc if rc < 0 else _lib.AFX_E_INVALID)
    return start, count, w


def resample_tables(n_in: int, n_out: int, filter: str = 'lanczos3', box=None):
    """(start, count, w) of one axis of Pillow's ``Image.resize(..., box=)``: output i is sum_k w[i, k] in[start[i] + k], k < count[i].
    ``box`` = (b0, b1) in source pixels (fractional allowed; default the whole axis).  Built in fp64, weights rounded to fp32 once; CPU
    tensors, no GPU needed.  A ratio that needs more than AFX_RESAMPLE_MAX_TAPS taps (Lanczos-3: beyond about 21x down) raises."""
    if filter not in _FILTERS:
        raise ValueError(f"filter: 'lanczos3' or 'triangle', got {filter!r}")
    b0, b1 = (0.0, float(n_in)) if box is None else (float(box[0]), float(box[1]))
    return _axis_table(int(n_in), int(n_out), getattr(_lib, _FILTERS[filter]), b0, b1, 0.0)


def gaussian_tables(n: int, sigma: float):
    """(start, count, w) of a Gaussian blur along an axis of ``n`` pixels: taps exp(-d^2 / (2 sigma^2)) for |d| <= ceil(3 sigma), windows
    clipped at the border and renormalised (every row of w sums to 1).  CPU tensors."""
    return _axis_table(int(n), int(n), _lib.AFX_FILTER_GAUSSIAN, 0.0, float(n), float(sigma))


@functools.lru_cache(maxsize=64)
def _device_table(n_in: int, n_out: int, filt: int, b0: float, b1: float, sigma: float, device: str):
    """``_axis_table`` on the GPU, kept for the next call of the same geometry.  The cache holds at most 64 tables for the life of the
    process (a table is n_out (taps + 2) 4 bytes: 0.4 MB for 1024 outputs of a 4x Lanczos-3 downscale).  A table is uploaded on the
    stream that is current at its first use and that stream is waited for here, once per table, so a later call on ANY stream reads a
    finished upload."""
    tabs = tuple(t.to(device) for t in _axis_table(n_in, n_out, filt, b0, b1, sigma))
    torch.cuda.current_stream(tabs[0].device).synchronize()
    return tabs


def _resample_source(src: torch.Tensor, name: str):
    """-> (B, C, H, W) of a source as afx_image_resample reads it: uint8 [B, H, W, C] or float32 [B, C, H, W], C 1 or 3, non-empty."""
    _gpu(src, name=name)
    if src.dim() != 4 or src.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f'{name}: need uint8 [B, H, W, C] or float32 [B, C, H, W], got {tuple(src.shape)} {src.dtype}')
    B, Cn, H, W = (src.shape[0], src.shape[3], src.shape[1], src.shape[2]) if src.dtype == torch.uint8 else src.shape
    if Cn not in (1, 3) or min(B, H, W) < 1:
        raise ValueError(f'{name}: need 1 or 3 channels and a non-empty image, got {tuple(src.shape)} '
                         f'({"B, H, W, C" if src.dtype == torch.uint8 else "B, C, H, W"})')
    return int(B), int(Cn), int(H), int(W)


def _resample(src: torch.Tensor, dims, out_h: int, out_w: int, tab_h, tab_w, clamp: bool) -> torch.Tensor:
    """afx_image_resample on a checked source (``dims`` from ``_resample_source``) with the device tables ``tab_w`` (W axis) and ``tab_h``
    (H axis) of ``_device_table``: (start, count, w)."""
    B, Cn, H, W = dims
    src = src.contiguous()
    lib = _lib.load()
    need = lib.afx_image_resample_ws_bytes(B, Cn, H, out_w)
    if need < 0:
        _lib.check(int(need))
    ws = torch.empty(need // 4, dtype=torch.float32, device=src.device)
    dst = torch.empty(B, Cn, out_h, out_w, dtype=torch.float32, device=src.device)
    _lib.check(lib.afx_image_resample(_p(src), int(src.dtype == torch.uint8), B, Cn, H, W, _p(tab_w[0]), _p(tab_w[1]), _p(tab_w[2]),
                                      tab_w[2].shape[1], _p(tab_h[0]), _p(tab_h[1]), _p(tab_h[2]), tab_h[2].shape[1], _p(dst), out_h, out_w,
                                      int(bool(clamp)), _p(ws), need, _s()))
    return dst


def image_resample(src: torch.Tensor, out_h: int, out_w: int, filter: str = 'lanczos3', box=None, clamp: bool = True) -> torch.Tensor:
    """Pillow's ``Image.resize((out_w, out_h), filter, box)`` on the GPU (afx_image_resample): src uint8 [B, H, W, C] (read as x / 255, so
    3 B per pixel cross the bus) or float32 [B, C, H, W], C 1 or 3 -> float32 [B, C, out_h, out_w].  ``box`` = (left, upper, right, lower)
    in source pixels, fractional allowed (default the whole image); ``clamp`` to [0, 1] (Lanczos overshoots).  Separable, horizontal
    pass first, fp32 accumulation; a same-size call without a box returns the source's values exactly."""
    if filter not in _FILTERS:
        raise ValueError(f"filter: 'lanczos3' or 'triangle', got {filter!r}")
    dims = _resample_source(src, 'src')
    H, W = dims[2:]
    left, upper, right, lower = (0.0, 0.0, float(W), float(H)) if box is None else (float(v) for v in box)
    filt, dev = getattr(_lib, _FILTERS[filter]), str(src.device)
    tab_w = _device_table(W, int(out_w), filt, left, right, 0.0, dev)
    tab_h = _device_table(H, int(out_h), filt, upper, lower, 0.0, dev)
    return _resample(src, dims, int(out_h), int(out_w), tab_h, tab_w, clamp)


def mask_feather(mask: torch.Tensor, sigma: float) -> torch.Tensor:
    """Gaussian feathering of a float32 [B, C, H, W] mask (C 1 or 3) with ``sigma`` in pixels, on the table-driven resampling kernel
    (ops.gaussian_tables on both axes: border windows are clipped and renormalised), clamped to [0, 1]."""
    if mask.dtype != torch.float32:
        raise ValueError(f'mask: need float32 [B, C, H, W], got {tuple(mask.shape)} {mask.dtype}')
    dims = _resample_source(mask, 'mask')
    H, W = dims[2:]
    dev = str(mask.device)
    tab_w = _device_table(W, W, _lib.AFX_FILTER_GAUSSIAN, 0.0, float(W), float(sigma), dev)
    tab_h = _device_table(H, H, _lib.AFX_FILTER_GAUSSIAN, 0.0, float(H), float(sigma), dev)
    return _resample(mask, dims, H, W, tab_h, tab_w, True)


def mask_bbox(mask: torch.Tensor) -> torch.Tensor:
    """int32 [B, 4] on the device = (x0, y0, x1, y1), the half-open bounding box of the pixels with m > 0 of every image of ``mask``
    (afx_mask_bbox): uint8 [B, H, W, 1] or float32 [B, 1, H, W].  A NaN is not > 0, a positive denormal is; an image without such a pixel
    gives (W, H, 0, 0).  Integer min / max: the same result on every run.  Nothing is copied or cast: a wrong dtype or layout raises."""
    _gpu(mask, name='mask')
    u8 = mask.dtype == torch.uint8
    ok = mask.dim() == 4 and mask.dtype in (torch.uint8, torch.float32) and mask.shape[3 if u8 else 1] == 1 and mask.is_contiguous()
    if not ok or min(mask.shape) < 1:
        raise ValueError(f'mask: need a contiguous, non-empty uint8 [B, H, W, 1] or float32 [B, 1, H, W], got {tuple(mask.shape)} {mask.dtype} '
                         f'strides {mask.stride()}')
    B, H, W = (mask.shape[0], mask.shape[1], mask.shape[2]) if u8 else (mask.shape[0], mask.shape[2], mask.shape[3])
    out = torch.empty(B, 4, dtype=torch.int32, device=mask.device)
    _lib.check(_lib.load().afx_mask_bbox(_p(mask), int(u8), B, H, W, _p(out), _s()))
    return out


def image_paste(img: torch.Tensor, mask: Optional[torch.Tensor], src_u8: torch.Tensor, window, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Paste an edit back into the photo it was cut from (afx_image_paste) -> uint8 [B, H, W, 3].  ``img`` float32 [B, 3, h, w] in [-1, 1]
    (the decoder's output) is resampled to the integer ``window`` = (x0, y0, x1, y1) of ``src_u8`` uint8 [B, H, W, 3] with Lanczos-3,
    ``mask`` float32 [B or 1, 1, h, w] in [0, 1] (None: 1 everywhere in the window) with the triangle filter, and per channel the byte is
    rint(255 clamp(m (0.5 v + 0.5) + (1 - m) byte / 255, 0, 1)).  Outside the window, and inside it where m == 0, the result holds the
    source's own bytes.  The tables are built once per geometry and kept (``_device_table``).  Nothing is copied or cast: a wrong dtype or
    layout raises.  ``out``: a uint8 [B, H, W, 3] buffer to write (not ``src_u8``)."""
    lib = _lib.load()
    _gpu(img, mask, src_u8, out)
    if img.dim() != 4 or img.shape[1] != 3 or min(img.shape) < 1:
        raise ValueError(f'img: need a non-empty float32 [B, 3, h, w], got {tuple(img.shape)}')
    B, _, h, w = img.shape
    img = _packed(img, torch.float32, img.shape, 'img')
    if src_u8.dim() != 4 or src_u8.shape[0] != B or src_u8.shape[3] != 3 or min(src_u8.shape) < 1:
        raise ValueError(f'src_u8: need a non-empty uint8 [{B}, H, W, 3], got {tuple(src_u8.shape)}')
    src_u8 = _packed(src_u8, torch.uint8, src_u8.shape, 'src_u8')
    H, W = src_u8.shape[1:3]
    if mask is not None:
        if mask.dim() != 4 or mask.shape[0] not in (1, B):
            raise ValueError(f'mask: need float32 [{B} or 1, 1, {h}, {w}], got {tuple(mask.shape)}')
        mask = _packed(mask, torch.float32, (mask.shape[0], 1, h, w), 'mask')
    x0, y0, x1, y1 = (int(v) for v in window)
    if any(int(v) != v for v in window) or not (0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H):
        raise ValueError(f'window: need integers (x0, y0, x1, y1) of a non-empty window inside the {H} x {W} source, got {tuple(window)}')
    out = torch.empty_like(src_u8) if out is None else _packed(out, torch.uint8, src_u8.shape, 'out')
    dev = str(img.device)
    itab = (_device_table(w, x1 - x0, _lib.AFX_FILTER_LANCZOS3, 0.0, float(w), 0.0, dev),
            _device_table(h, y1 - y0, _lib.AFX_FILTER_LANCZOS3, 0.0, float(h), 0.0, dev))
    mtab = ((None, None, None),) * 2 if mask is None else (_device_table(w, x1 - x0, _lib.AFX_FILTER_TRIANGLE, 0.0, float(w), 0.0, dev),
                                                         _device_table(h, y1 - y0, _lib.AFX_FILTER_TRIANGLE, 0.0, float(h), 0.0, dev))
    mb = 0 if mask is None else mask.shape[0]
    need = lib.afx_image_paste_ws_bytes(B, mb, h, x1 - x0)
    if need < 0:
        _lib.check(int(need))
    ws = torch.empty(need // 4, dtype=torch.float32, device=img.device)
    tabs = [a for tab in itab + mtab for a in (_p(tab[0]), _p(tab[1]), _p(tab[2]), 0 if tab[2] is None else tab[2].shape[1])]
    _lib.check(lib.afx_image_paste(_p(img), _p(mask), mb, _p(src_u8), _p(out), B, h, w, H, W, x0, y0, x1, y1, x1 - x0, y1 - y0, *tabs,
                                   _p(ws), need, _s()))
    return out


@functools.lru_cache(maxsize=16)
def _device_plan(H: int, W: int, tile: int, overlap: int, device: str):
    """``schedule.tile_plan`` with its origin lists and tables on the GPU, kept for the next call of the same geometry, uploaded and waited
    for in the manner of ``_device_table``: -> (plan, oy, ox, (y_start, y_count, y_w), (x_start, x_count, x_w)).  A plan of a 4500 x 6000
    canvas is 0.25 MB."""
    from .schedule import tile_plan
    plan = tile_plan(H, W, tile, overlap)
    up = lambda a: torch.from_numpy(a).to(device)          # noqa: E731
    dev = (plan, up(plan.oy), up(plan.ox), tuple(up(a) for a in plan.y), tuple(up(a) for a in plan.x))
    torch.cuda.current_stream(dev[1].device).synchronize()
    return dev


def _plan_on(plan, device=None):
    """The checked plan alone, or with a device its ``_device_plan``."""
    from .schedule import TilePlan
    if not isinstance(plan, TilePlan):
        raise ValueError(f'plan: need a schedule.TilePlan (schedule.tile_plan), got {type(plan).__name__}')
    return plan if device is None else _device_plan(plan.H, plan.W, plan.tile, plan.overlap, str(device))


def tiles_cut(canvas: torch.Tensor, plan) -> torch.Tensor:
    """Cut the canvas float32 [3, H, W] (or [1, 3, H, W]) into the overlapping tiles of ``plan`` = ``schedule.tile_plan(H, W, tile, overlap)``
    (afx_tiles_cut) -> float32 [T, 3, th, tw], tile iy * kx + ix from the corner (oy[iy], ox[ix]), values bit for bit.  The plan's lists
    are uploaded once per geometry and kept.  Nothing is copied or cast: a wrong dtype or layout raises."""
    _gpu(canvas, name='canvas')
    plan = _plan_on(plan)
    if canvas.dim() == 4 and canvas.shape[0] == 1:
        canvas = canvas[0]
    if canvas.dim() != 3 or tuple(canvas.shape) != (3, plan.H, plan.W):
        raise ValueError(f'canvas: need float32 [3, H, W] of the plan\'s canvas ({plan.H} x {plan.W}), got {tuple(canvas.shape)}')
    canvas = _packed(canvas, torch.float32, canvas.shape, 'canvas')
    plan, oy, ox, _, _ = _plan_on(plan, canvas.device)
    tiles = torch.empty(plan.T, 3, plan.th, plan.tw, dtype=torch.float32, device=canvas.device)
    _lib.check(_lib.load().afx_tiles_cut(_p(canvas), plan.H, plan.W, _p(oy), plan.ky, _p(ox), plan.kx, plan.th, plan.tw, _p(tiles), _s()))
    return tiles


def tiles_merge(tiles: torch.Tensor, plan, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Cross-fade decoded tiles float32 [T, 3, th, tw] in [-1, 1] back into one image (afx_tiles_merge) -> uint8 [H, W, 3]: per pixel and
    channel, in fp32, taps ascending, rows outer and columns inner, acc = sum_a wy[y, a] (sum_b wx[x, b] fma(0.5, v_ab, 0.5)) over the
    tiles that cover the pixel with the weights of ``plan`` (``schedule.tile_plan``), byte = rint(255 clamp(acc, 0, 1)).  One launch, no
    atomics: the same bits on every run.  ``out``: a uint8 [H, W, 3] buffer to write.  A wrong dtype or layout raises."""
    _gpu(tiles, out, name='tiles')
    plan = _plan_on(plan)
    want = (plan.T, 3, plan.th, plan.tw)
    if tiles.dim() != 4 or tuple(tiles.shape) != want:
        raise ValueError(f'tiles: need float32 {list(want)} (the plan\'s T, 3, th, tw), got {tuple(tiles.shape)}')
    tiles = _packed(tiles, torch.float32, tiles.shape, 'tiles')
    plan, oy, ox, ytab, xtab = _plan_on(plan, tiles.device)
    out = torch.empty(plan.H, plan.W, 3, dtype=torch.uint8, device=tiles.device) if out is None else \
        _packed(out, torch.uint8, (plan.H, plan.W, 3), 'out')
    _lib.check(_lib.load().afx_tiles_merge(_p(tiles), plan.T, plan.th, plan.tw, _p(oy), plan.ky, _p(ox), plan.kx, _p(ytab[0]), _p(ytab[1]),
                                           _p(ytab[2]), ytab[2].shape[1], _p(xtab[0]), _p(xtab[1]), _p(xtab[2]), xtab[2].shape[1], _p(out),
                                           plan.H, plan.W, _s()))
    return out


CANVAS_FILLS = {'edge': _lib.AFX_FILL_EDGE, 'reflect': _lib.AFX_FILL_REFLECT}


def _count(v, name: str) -> int:
    """An integral value >= 0 as an int (a bool, a fraction or a negative value raises)."""
    if isinstance(v, bool) or int(v) != v or v < 0:
        raise ValueError(f'{name}: need an integer >= 0, got {v!r}')
    return int(v)


def canvas_extend(src_u8: torch.Tensor, left: int, top: int, right: int, bottom: int, fill: str = 'reflect',
                  blend: int = 32) -> Tuple[torch.Tensor, torch.Tensor]:
    """The photo ``src_u8`` uint8 [B, H, W, 3] on a canvas extended by ``left``, ``top``, ``right``, ``bottom`` pixels (afx_canvas_extend) ->
    (canvas uint8 [B, Hc, Wc, 3], mask float32 [1, 1, Hc, Wc]), one launch.  The new pixels are filled from the photo, ``fill`` 'edge'
    (the border repeated) or 'reflect' (mirrored without repeating the border: ``np.pad``'s modes, for pads of any length); inside the
    photo's rectangle the canvas holds the photo's bytes.  The mask is 1 on the new pixels, max(0, 1 - (d + 1) / (blend + 1)) inside the
    rectangle at distance d from the nearest extended side, so ``blend`` pixels inside each extended side are partly repainted and
    ``blend=0`` gives a binary mask.  Nothing is copied or cast: a wrong dtype, layout or device raises."""
    if fill not in CANVAS_FILLS:
        raise ValueError(f"fill: 'edge' or 'reflect', got {fill!r}")
    if src_u8.dim() != 4 or src_u8.shape[3] != 3 or min(src_u8.shape) < 1 or src_u8.dtype != torch.uint8 or not src_u8.is_contiguous():
        raise ValueError(f'src_u8: need a contiguous, non-empty uint8 [B, H, W, 3], got {tuple(src_u8.shape)} {src_u8.dtype} '
                         f'strides {src_u8.stride()}')
    left, top, right, bottom = (_count(v, n) for v, n in ((left, 'left'), (top, 'top'), (right, 'right'), (bottom, 'bottom')))
    blend = _count(blend, 'blend')
    if not (left or top or right or bottom):
        raise ValueError('left, top, right, bottom: at least one extent must be > 0')
    _gpu(src_u8, name='src_u8')
    B, H, W = src_u8.shape[:3]
    canvas = torch.empty(B, H + top + bottom, W + left + right, 3, dtype=torch.uint8, device=src_u8.device)
    mask = torch.empty(1, 1, H + top + bottom, W + left + right, dtype=torch.float32, device=src_u8.device)
    _lib.check(_lib.load().afx_canvas_extend(_p(src_u8), B, H, W, left, top, right, bottom, CANVAS_FILLS[fill], blend, _p(canvas), _p(mask),
                                             _s()))
    return canvas, mask


def canvas_mark(mask: torch.Tensor, window, blend: int) -> torch.Tensor:
    """Mark the integer ``window`` = (x0, y0, x1, y1) as painted in the outpainting mask state ``mask`` float32 [1, 1, Hc, Wc] (or [Hc, Wc]),
    in place (afx_canvas_mark): M = min(M, max(0, 1 - (d + 1) / (blend + 1))) on the window's pixels, d the distance to the nearest window
    side that is not on the canvas border -- 0 in the window's interior, a ramp of ``blend`` pixels inside each inner side, which the next
    window cross-fades over.  Pixels outside the window are not touched.  Returns ``mask``.  A wrong dtype, layout or device raises."""
    if mask.dim() not in (2, 4) or (mask.dim() == 4 and tuple(mask.shape[:2]) != (1, 1)) or min(mask.shape) < 1 or \
            mask.dtype != torch.float32 or not mask.is_contiguous():
        raise ValueError(f'mask: need a contiguous, non-empty float32 [1, 1, Hc, Wc] or [Hc, Wc], got {tuple(mask.shape)} {mask.dtype} '
                         f'strides {mask.stride()}')
    Hc, Wc = mask.shape[-2:]
    x0, y0, x1, y1 = (int(v) for v in window)
    if any(int(v) != v for v in window) or not (0 <= x0 < x1 <= Wc and 0 <= y0 < y1 <= Hc):
        raise ValueError(f'window: need integers (x0, y0, x1, y1) of a non-empty window inside the {Hc} x {Wc} canvas, got {tuple(window)}')
    blend = _count(blend, 'blend')
    _gpu(mask, name='mask')
    _lib.check(_lib.load().afx_canvas_mark(_p(mask), Hc, Wc, x0, y0, x1, y1, blend, _s()))
    return mask


COLOR_FIX_MODES = {'adain': _lib.AFX_COLOR_ADAIN, 'wavelet': _lib.AFX_COLOR_WAVELET, 'wavelet_levels': _lib.AFX_COLOR_WAVELET_LEVELS}


def _color_mode(mode) -> int:
    if mode not in COLOR_FIX_MODES:
        raise ValueError(f"mode: 'adain' or 'wavelet' ('wavelet_levels': the per-pass form of 'wavelet', the same bits), got {mode!r}")
    return COLOR_FIX_MODES[mode]


def color_fix_ws(mode: str, batch: int, channels: int, height: int, width: int, device='cuda') -> torch.Tensor:
    """Workspace of color_fix for a [batch, channels, height, width] edit (afx_color_fix_ws_bytes): 'adain' the fp64 partial sums and the
    (a, b) pairs, 'wavelet' nothing (one element), 'wavelet_levels' two fp32 copies of the edit's shape."""
    return _ws(_lib.load().afx_color_fix_ws_bytes, _color_mode(mode), batch, channels, height, width, device=device, min_one=True)


def color_fix(edit: torch.Tensor, source: torch.Tensor, mode: str = 'wavelet', src01: bool = True, out: Optional[torch.Tensor] = None,
              stats: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Give a decoded edit the colours of the picture it was made from (afx_color_fix) -> float32 [B, C, H, W], not clamped.
    ``edit`` [B, C, H, W] fp32 or bf16 in the decoder's range [-1, 1]; ``source`` float32 [Bs, C, H, W], Bs 1 (shared) or B, in [0, 1]
    (``src01``, read as 2 s - 1) or already in [-1, 1].  'wavelet': the edit's low band -- five levels of the [1, 2, 1] / 4 blur at
    dilations 1..16, replicate borders -- is replaced by the source's, out = e + low(s' - e) in one fused launch; 'adain': the edit takes
    the source's per-(image, channel) mean and deviation, out = fma(a, e, b) with fp64 moments.  Both are bit-reproducible and a batch
    gives the bits of its single calls; the full rules are in arcflow_hip.h.  ``stats``: a float64 [B, C, 4] buffer that 'adain' fills
    with (mu_e, var_e, mu_s, var_s).  ``out`` / ``ws``: reuse buffers (ops.color_fix_ws); ``out`` may not be an operand.  Nothing is
    copied or cast: a CPU tensor, a wrong dtype or a wrong layout raises."""
    m = _color_mode(mode)
    _gpu(edit, source, out, stats, ws, name='color_fix')
    if edit.dim() != 4 or edit.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f'edit: need a float32 or bfloat16 [B, C, H, W] tensor, got {tuple(edit.shape)} {edit.dtype}')
    B, Cn, H, W = edit.shape
    if source.dim() != 4 or source.shape[0] not in (1, B) or tuple(source.shape[1:]) != (Cn, H, W):
        raise ValueError(f'source: need float32 [1 or {B}, {Cn}, {H}, {W}] (the edit\'s shape), got {tuple(source.shape)}')
    edit = _packed(edit, edit.dtype, edit.shape, 'edit')
    source = _packed(source, torch.float32, source.shape, 'source')
    out = torch.empty(B, Cn, H, W, dtype=torch.float32, device=edit.device) if out is None else _packed(out, torch.float32, (B, Cn, H, W), 'out')
    if stats is not None:
        stats = _packed(stats, torch.float64, (B, Cn, 4), 'stats')
    if ws is None:
        ws = color_fix_ws(mode, B, Cn, H, W, edit.device)
    elif not ws.is_contiguous():
        raise ValueError('ws: need a contiguous GPU buffer (ops.color_fix_ws)')
    dt = _lib.AFX_DT_BF16 if edit.dtype == torch.bfloat16 else _lib.AFX_DT_F32
    _lib.check(_lib.load().afx_color_fix(_p(edit), dt, _p(source), source.shape[0], int(bool(src01)), m, _p(out), _p(stats), _p(ws),
                                         ws.numel() * ws.element_size(), B, Cn, H, W, _s()))
    return out


def _step_operands(x, pos, neg, sigma, sigma_to, coef, out, out_bf16):
    """The operands every teacher step shares, checked: -> (x, pos, neg, sigma, sigma_to, coef, out, out_bf16, B, n), out and out_bf16
    allocated when None.  sigma and sigma_to may be None (the UniPC step takes its weights instead)."""
    B = x.shape[0]
    x = _packed(x, torch.float32, x.shape, 'x')
    pos = _packed(pos, torch.bfloat16, x.shape, 'pos')
    neg = None if neg is None else _packed(neg, torch.bfloat16, x.shape, 'neg')
    sigma = None if sigma is None else _packed(sigma, torch.float32, (B,), 'sigma')
    sigma_to = None if sigma_to is None else _packed(sigma_to, torch.float32, (B,), 'sigma_to')
    coef = None if coef is None else _packed(coef, torch.float32, (B,), 'coef')
    out = torch.empty_like(x) if out is None else _packed(out, torch.float32, x.shape, 'out')
    out_bf16 = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if out_bf16 is None else _packed(out_bf16, torch.bfloat16, x.shape, 'out_bf16')
    return x, pos, neg, sigma, sigma_to, coef, out, out_bf16, B, x[0].numel() if B else 0


def _sde_operands(x, noise, m, c_noise):
    """What the FlowSDE steps take beside _step_operands, checked against x: -> (noise, m, c_noise)."""
    noise = None if noise is None else _packed(noise, torch.float32, x.shape, 'noise')
    return noise, _packed(m, torch.float32, (x.shape[0],), 'm'), _packed(c_noise, torch.float32, (x.shape[0],), 'c_noise')


def teacher_euler_step(x, pos, neg, sigma, sigma_to, scale: float = 1.0, coef: Optional[torch.Tensor] = None,
                       out: Optional[torch.Tensor] = None, out_bf16: Optional[torch.Tensor] = None, max_blocks: int = 0):
    """One step of the teacher's Euler ODE sampler in one launch (afx_teacher_euler_step):
    x + (pos + (pos - neg)(scale - 1) - coef[b] pos)(sigma_to[b] - sigma[b]) -> (fp32 latents, their bf16 rounding).
    x [B, ...] fp32; pos, neg (None: no guidance) bf16 of the same shape; sigma, sigma_to, coef (None: not orthogonal) [B] fp32.
    out may be x (in place).  numel / B must be a multiple of 64.  Nothing is copied or cast: a wrong dtype or layout raises."""
    lib = _lib.load()
    _gpu(x, pos, neg, sigma, sigma_to, coef, out, out_bf16)
    x, pos, neg, sigma, sigma_to, coef, out, out_bf16, B, n = _step_operands(x, pos, neg, sigma, sigma_to, coef, out, out_bf16)
    _lib.check(lib.afx_teacher_euler_step(_p(x), _p(pos), _p(neg), _p(sigma), _p(sigma_to), _p(coef), scale, _p(out), _p(out_bf16), B, n,
                                          max_blocks, _s()))
    return out, out_bf16


def teacher_sde_step(x, pos, neg, noise, sigma, sigma_to, m, c_noise, scale: float = 1.0, coef: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None, out_bf16: Optional[torch.Tensor] = None, max_blocks: int = 0):
    """One step of the teacher's stochastic sampler (FlowSDEScheduler) in one launch (afx_teacher_sde_step): with
    u = pos + (pos - neg)(scale - 1) - coef[b] pos as teacher_euler_step forms it, x0 = x - sigma[b] u and e = x + (1 - sigma[b]) u,
    (1 - sigma_to[b]) x0 + sigma_to[b] (m[b] e + c_noise[b] noise) -> (fp32 latents, their bf16 rounding).
    x, noise (None: no noise term, nothing read) [B, ...] fp32; pos, neg (None: no guidance) bf16 of the same shape; sigma, sigma_to,
    m, c_noise (FlowSDEScheduler.coefficients), coef (None: not orthogonal) [B] fp32.  out may be x (in place).  numel / B must be a
    multiple of 64.  Nothing is copied or cast: a wrong dtype or layout raises."""
    lib = _lib.load()
    _gpu(x, pos, neg, noise, sigma, sigma_to, m, c_noise, coef, out, out_bf16)
    x, pos, neg, sigma, sigma_to, coef, out, out_bf16, B, n = _step_operands(x, pos, neg, sigma, sigma_to, coef, out, out_bf16)
    noise, m, c_noise = _sde_operands(x, noise, m, c_noise)
    _lib.check(lib.afx_teacher_sde_step(_p(x), _p(pos), _p(neg), _p(noise), _p(sigma), _p(sigma_to), _p(m), _p(c_noise), _p(coef), scale,
                                        _p(out), _p(out_bf16), B, n, max_blocks, _s()))
    return out, out_bf16


def teacher_unipc_step(x, pos, neg, w, last, hist, last_out, hist_out, scale: float = 1.0, coef: Optional[torch.Tensor] = None,
                       out: Optional[torch.Tensor] = None, out_bf16: Optional[torch.Tensor] = None, max_blocks: int = 0):
    """One step of the teacher's UniPC multistep sampler (FlowUniPCScheduler) in one launch (afx_teacher_unipc_step): with u as
    teacher_euler_step forms it and the per-sample weights w [10, B] fp32 (``FlowUniPCScheduler.coefficients(i).row()``: s | c_last, c_mt,
    c_1, c_2, c_3 | p_xc, p_mt, p_1, p_2), m_t = x - s u; x_c = c_last last + c_1 h1 + c_2 h2 + c_3 h3 + c_mt m_t (last None: x_c = x);
    x_next = p_xc x_c + p_1 h1 + p_2 h2 + p_mt m_t -> (fp32 x_next, its bf16 rounding); x_c is written to last_out and m_t to hist_out.
    x, last (None: no corrector) and the up to three tensors of ``hist`` (m_t of one, two, three steps ago; only those given are read)
    [B, ...] fp32; pos, neg (None: no guidance) bf16 of the same shape; coef (None: not orthogonal) [B] fp32.  out may be x, last_out may
    be last, hist_out may be one of ``hist``.  numel / B must be a multiple of 64.  Nothing is copied or cast: a wrong dtype or layout raises."""
    lib = _lib.load()
    hist = list(hist or ())
    if len(hist) > 3:
        raise ValueError(f'hist: at most three past predictions, got {len(hist)}')
    _gpu(x, pos, neg, w, last, *hist, last_out, hist_out, coef, out, out_bf16)
    x, pos, neg, _, _, coef, out, out_bf16, B, n = _step_operands(x, pos, neg, None, None, coef, out, out_bf16)
    w = _packed(w, torch.float32, (10, B), 'w')
    last = None if last is None else _packed(last, torch.float32, x.shape, 'last')
    hist = [_packed(h, torch.float32, x.shape, f'hist[{k}]') for k, h in enumerate(hist)] + [None] * (3 - len(hist))
    last_out = _packed(last_out, torch.float32, x.shape, 'last_out')
    hist_out = _packed(hist_out, torch.float32, x.shape, 'hist_out')
    _lib.check(lib.afx_teacher_unipc_step(_p(x), _p(pos), _p(neg), _p(w), _p(last), _p(hist[0]), _p(hist[1]), _p(hist[2]), _p(coef), scale,
                                          _p(out), _p(out_bf16), _p(last_out), _p(hist_out), B, n, max_blocks, _s()))
    return out, out_bf16


def edit_blend(x, x0, noise, mask, sigma_to, out: Optional[torch.Tensor] = None, out_bf16=None, max_blocks: int = 0):
    """The blend of image editing in one launch (afx_edit_blend): with known = (1 - sigma_to[b]) x0 + sigma_to[b] noise, the source
    latents diffused to sigma_to, mask x + (1 - mask) known -> (fp32 latents, their bf16 rounding).
    x0, noise (None: no noise term, nothing read) [B, N, 64] fp32 packed tokens; mask [B, N, 4] fp32 in [0, 1], one value per latent
    pixel of the 2 x 2 patch (None: everything is known, x is ignored and may be None: the image-to-image start); x [B, N, 64] fp32
    with a mask; sigma_to [B] fp32.  out may be x (in place).  out_bf16=False: no bf16 copy is written, (out, None) is returned.
    m = 1 returns x, m = 0 known, sigma_to = 1 noise and sigma_to = 0 x0 bit for bit.  Nothing is copied or cast: a wrong dtype, device
    or layout raises."""
    lib = _lib.load()
    _gpu(x, x0, noise, mask, sigma_to, out, None if out_bf16 is False else out_bf16)
    if x0.dim() != 3:
        raise ValueError(f'x0: need packed tokens [B, N, 64], got {tuple(x0.shape)}')
    B, N, ch = x0.shape
    x0 = _packed(x0, torch.float32, x0.shape, 'x0')
    if mask is None:
        x = None
    else:
        if x is None:
            raise ValueError('x: required with a mask')
        x = _packed(x, torch.float32, x0.shape, 'x')
        mask = _packed(mask, torch.float32, (B, N, 4), 'mask')
    noise = None if noise is None else _packed(noise, torch.float32, x0.shape, 'noise')
    sigma_to = _packed(sigma_to, torch.float32, (B,), 'sigma_to')
    out = torch.empty_like(x0) if out is None else _packed(out, torch.float32, x0.shape, 'out')
    if out_bf16 is False:
        out_bf16 = None
    else:
        out_bf16 = torch.empty(x0.shape, dtype=torch.bfloat16, device=x0.device) if out_bf16 is None else _packed(out_bf16, torch.bfloat16, x0.shape, 'out_bf16')
    _lib.check(lib.afx_edit_blend(_p(x), _p(x0), _p(noise), _p(mask), _p(sigma_to), _p(out), _p(out_bf16), B, N, ch, max_blocks, _s()))
    return out, out_bf16


def _edit_step_operands(x, pos, neg, sigma, sigma_to, coef, x0, noise0, mask, out, out_bf16):
    """_step_operands for the edit steps, x packed tokens [B, N, 64], with their x0, noise0 and mask, checked:
    -> (x, pos, neg, sigma, sigma_to, coef, x0, noise0, mask, out, out_bf16, B, N, ch)."""
    if x.dim() != 3:
        raise ValueError(f'x: need packed tokens [B, N, 64], got {tuple(x.shape)}')
    B, N, ch = x.shape
    x, pos, neg, sigma, sigma_to, coef, out, out_bf16, _, _ = _step_operands(x, pos, neg, sigma, sigma_to, coef, out, out_bf16)
    x0 = _packed(x0, torch.float32, x.shape, 'x0')
    noise0 = None if noise0 is None else _packed(noise0, torch.float32, x.shape, 'noise0')
    mask = None if mask is None else _packed(mask, torch.float32, (B, N, 4), 'mask')
    return x, pos, neg, sigma, sigma_to, coef, x0, noise0, mask, out, out_bf16, B, N, ch


def teacher_edit_step(x, pos, neg, sigma, sigma_to, x0, noise0, mask, scale: float = 1.0, coef: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None, out_bf16: Optional[torch.Tensor] = None, max_blocks: int = 0):
    """One Euler step of teacher image editing in one launch (afx_teacher_edit_step): teacher_euler_step's x', then with
    known = (1 - sigma_to[b]) x0 + sigma_to[b] noise0 the blend mask x' + (1 - mask) known of edit_blend -> (fp32 latents, their bf16
    rounding), bit for bit teacher_euler_step followed by edit_blend.  x, x0, noise0 (None: no noise term, the step landing on
    sigma_to = 0) [B, N, 64] fp32 packed tokens; mask [B, N, 4] fp32 in [0, 1], 1 = repaint (None: the plain step, the same kernel as
    teacher_euler_step); the other operands as for teacher_euler_step.  out may be x (in place).  Nothing is copied or cast."""
    lib = _lib.load()
    _gpu(x, pos, neg, sigma, sigma_to, coef, x0, noise0, mask, out, out_bf16)
    x, pos, neg, sigma, sigma_to, coef, x0, noise0, mask, out, out_bf16, B, N, ch = _edit_step_operands(
        x, pos, neg, sigma, sigma_to, coef, x0, noise0, mask, out, out_bf16)
    _lib.check(lib.afx_teacher_edit_step(_p(x), _p(pos), _p(neg), _p(sigma), _p(sigma_to), _p(coef), scale, _p(x0), _p(noise0), _p(mask),
                                         _p(out), _p(out_bf16), B, N, ch, max_blocks, _s()))
    return out, out_bf16


def teacher_sde_edit_step(x, pos, neg, noise, sigma, sigma_to, m, c_noise, x0, noise0, mask, scale: float = 1.0,
                          coef: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, out_bf16: Optional[torch.Tensor] = None,
                          max_blocks: int = 0):
    """One FlowSDE step of teacher image editing in one launch (afx_teacher_sde_edit_step): teacher_sde_step's x' with the step's draw
    ``noise``, then edit_blend's blend with the START noise ``noise0`` as in teacher_edit_step -> (fp32 latents, their bf16 rounding),
    bit for bit teacher_sde_step followed by edit_blend.  Operands as for teacher_sde_step and teacher_edit_step."""
    lib = _lib.load()
    _gpu(x, pos, neg, noise, sigma, sigma_to, m, c_noise, coef, x0, noise0, mask, out, out_bf16)
    x, pos, neg, sigma, sigma_to, coef, x0, noise0, mask, out, out_bf16, B, N, ch = _edit_step_operands(
        x, pos, neg, sigma, sigma_to, coef, x0, noise0, mask, out, out_bf16)
    noise, m, c_noise = _sde_operands(x, noise, m, c_noise)
    _lib.check(lib.afx_teacher_sde_edit_step(_p(x), _p(pos), _p(neg), _p(noise), _p(sigma), _p(sigma_to), _p(m), _p(c_noise), _p(coef), scale,
                                             _p(x0), _p(noise0), _p(mask), _p(out), _p(out_bf16), B, N, ch, max_blocks, _s()))
    return out, out_bf16


def head_grad(d_means, d_logw, d_logg, logw_out, ldy: int):
    lib = _lib.load()
    B, N, K, ch = d_means.shape
    lw = d_logw.shape[-1]
    dy = torch.empty(B * N, ldy, dtype=torch.bfloat16, device=d_means.device)
    _lib.check(lib.afx_head_grad(_p(d_means), _p(d_logw), _p(d_logg), _p(logw_out.contiguous()), _p(dy), ldy, B * N, K, ch, lw, _s()))
    return dy


def linear_f32out(a, w, out=None, accumulate: bool = False):
    """out (fp32) [M,N] (+)= a [M,K] @ w[N,K].T, bf16 operands."""
    lib = _lib.load()
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.zeros(M, N, dtype=torch.float32, device=a.device)
    _lib.check(lib.afx_linear_bf16_f32out(_p(a), a.stride(0), _p(w), w.stride(0), _p(out), out.stride(0), M, N, K,
                                          int(accumulate), _s()))
    return out


def linear_dropres(a, w, residual, p: float, seed: int, row0: int = 0, out=None):
    """out = residual + (a @ w.T) * keep/(1-p) with the LoRA-dropout mask of ``lora_dropout`` (seed, row0 + row, column) applied to the fp32 product in
    the GEMM's epilogue (one launch instead of product + mask-and-add pass).  out may be ``residual``."""
    lib = _lib.load()
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    if not lib.afx_gemm_dropres_available():
        # the masked residual add lives in the one-wave-per-SIMD kernel's epilogue only (set_gemm_mode(2) / AFX_GEMM_IMPL=2 select the 8-phase
        # kernel in A/B runs and parity tests): the product to memory, then the mask-and-add pass.  NOT the same bits: the fused epilogue masks
        # the fp32 product and rounds once, this path rounds the product to bf16 and rounds again after the add
        if out.data_ptr() != residual.data_ptr():
            out.copy_(residual)
        return lora_dropout(linear(a, w), p, seed, row0, mode=3, out=out)
    _lib.check(lib.afx_linear_bf16_dropres(_p(a), a.stride(0), _p(w), w.stride(0), _p(out), out.stride(0), M, N, K, _p(residual), residual.stride(0),
                                           float(p), seed & 0xffffffff, row0, _s()))
    return out


def linear_tn_f32out(x, y, out=None, accumulate: bool = False):
    """out (fp32) [N1,N2] (+)= x[M,N1].T @ y[M,N2]: the contraction runs over the ROWS of two token-major bf16 matrices (row strides = their
    stride(0)); the LoRA weight gradients without transposed copies (afx_tn.hip)."""
    lib = _lib.load()
    M, N1 = x.shape
    N2 = y.shape[1]
    assert y.shape[0] == M and x.stride(1) == 1 and y.stride(1) == 1
    if out is None:
        out = torch.zeros(N1, N2, dtype=torch.float32, device=x.device)
    nws = lib.afx_linear_tn_ws_bytes(M, N1, N2)       # > 0: the token loop is cut into runs (fp32 partial tiles in ws, added in a fixed order: deterministic)
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device) if nws > 0 else None      # (from the current stream's pool: private until the launches have run)
    _lib.check(lib.afx_linear_tn_f32out_ws(_p(x), x.stride(0), _p(y), y.stride(0), _p(out), out.stride(0), M, N1, N2, int(accumulate), _p(ws), _s()))
    return out


def quant_rows_fp8(x: torch.Tensor):
    """bf16 [M,K] -> (q uint8 [M,K] OCP e4m3, scale fp32 [M]) with q = round(x / scale[r]), scale = absmax(row) / 448."""
    lib = _lib.load()
    M, K = x.shape
    q = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    scale = torch.empty(M, dtype=torch.float32, device=x.device)
    _lib.check(lib.afx_quant_rows_fp8(_p(x), x.stride(0), _p(q), K, _p(scale), M, K, _s()))
    return q, scale


def linear_fp8(aq, a_scale, wq, w_scale, bias=None, epilogue: str = 'none', gelu_col0: int = 0, gate=None, residual=None,
               rows_per_batch: int = 0, out=None):
    """bf16 out = epi(a_scale[m] w_scale[n] (aq @ wq.T) + bias) on the 2x-rate fp8 MFMA; aq [M,K], wq [N,K] uint8 (e4m3)."""
    lib = _lib.load()
    M, K = aq.shape
    N = wq.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=aq.device)
    epi = {'none': 0, 'gelu': 1, 'gate_res': 2}[epilogue]
    if gate is not None:
        gate = _cuda(gate, torch.float32)
        if gate.dim() == 1:
            gate = gate[None]
    rpb = rows_per_batch if rows_per_batch > 0 else max(M, 1)
    _lib.check(lib.afx_linear_fp8(_p(aq), aq.stride(0), _p(a_scale), _p(wq), wq.stride(0), _p(w_scale), _p(bias), _p(out), out.stride(0),
                                  M, N, K, epi, gelu_col0, _p(gate), 0 if gate is None else gate.stride(0), rpb, _p(residual),
                                  0 if residual is None else residual.stride(0), _s()))
    return out


def quant_rows_mx8(x: torch.Tensor):
    """bf16 [M,K] -> (q uint8 [M,K] OCP e4m3, mx uint8 [M, K/128] E8M0): block-scaled fp8, one power-of-two scale per row and 128 columns
    (q = round(x * 2^(127 - mx)), the smallest scale that keeps the block inside +-448)."""
    lib = _lib.load()
    M, K = x.shape
    q = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    nb = K // 128
    mx = torch.empty(M, (nb + 3) // 4 * 4, dtype=torch.uint8, device=x.device)
    _lib.check(lib.afx_quant_rows_mx8(_p(x), x.stride(0), _p(q), K, _p(mx), mx.stride(0), M, K, _s()))
    return q, mx[:, :nb]


def linear_fp8_mx(aq, a_mx, wq, w_scale, bias=None, epilogue: str = 'none', gelu_col0: int = 0, gate=None, residual=None,
                  rows_per_batch: int = 0, out=None, a_scale=None):
    """bf16 out = epi(w_scale[n] (sum over K-tiles t of 2^(a_mx[m, t] - 127) aq[m, t] . wq[n, t]) + bias): the fp8 GEMM on block-scaled
    activations (``quant_rows_mx8`` / the fused producers).  K % 512 == 0."""
    lib = _lib.load()
    M, K = aq.shape
    N = wq.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=aq.device)
    if a_scale is None:
        a_scale = torch.ones(M, dtype=torch.float32, device=aq.device)
    epi = {'none': 0, 'gelu': 1, 'gate_res': 2}[epilogue]
    if gate is not None:
        gate = _cuda(gate, torch.float32)
        if gate.dim() == 1:
            gate = gate[None]
    rpb = rows_per_batch if rows_per_batch > 0 else max(M, 1)
    _lib.check(lib.afx_linear_fp8_mx(_p(aq), aq.stride(0), _p(a_mx), a_mx.stride(0), _p(a_scale), _p(wq), wq.stride(0), _p(w_scale), _p(bias),
                                     _p(out), out.stride(0), M, N, K, epi, gelu_col0, _p(gate), 0 if gate is None else gate.stride(0), rpb,
                                     _p(residual), 0 if residual is None else residual.stride(0), _s()))
    return out


def linear_fp8_to_mx8(aq, a_mx, wq, w_scale, bias=None, gelu: bool = False, c8_col0: int = 0, a_scale=None, out=None):
    """The fp8 GEMM whose epilogue writes the next GEMM's block-scaled operand: returns (bf16 [M, c8_col0] or None, q uint8 [M, N - c8_col0],
    mx uint8 [M, (N - c8_col0) / 128]).  a_mx None: per-row ``a_scale`` only.  out: (head or None, q, mx) row-strided views to write into
    (q's row stride a multiple of 8, mx's of 4)."""
    lib = _lib.load()
    M, K = aq.shape
    N = wq.shape[0]
    n8 = N - c8_col0
    nb = (n8 + 127) // 128
    if out is None:
        head = torch.empty(M, c8_col0, dtype=torch.bfloat16, device=aq.device) if c8_col0 > 0 else None
        q = torch.empty(M, n8, dtype=torch.uint8, device=aq.device)
        mx = torch.empty(M, (nb + 3) // 4 * 4, dtype=torch.uint8, device=aq.device)
    else:
        head, q, mx = out
        assert (head is None) == (c8_col0 == 0) and (head is None or (head.shape == (M, c8_col0) and head.dtype == torch.bfloat16))
        assert q.shape == (M, n8) and q.dtype == torch.uint8 and mx.shape[0] == M and mx.shape[1] >= nb and mx.dtype == torch.uint8
        assert q.stride(1) == 1 and mx.stride(1) == 1 and q.stride(0) % 8 == 0 and mx.stride(0) % 4 == 0
        assert head is None or (head.stride(1) == 1 and head.stride(0) % 8 == 0)
    if a_scale is None:
        a_scale = torch.ones(M, dtype=torch.float32, device=aq.device)
    _lib.check(lib.afx_linear_fp8_to_mx8(_p(aq), aq.stride(0), _p(a_mx), 0 if a_mx is None else a_mx.stride(0), _p(a_scale), _p(wq), wq.stride(0),
                                         _p(w_scale), _p(bias), _p(head), head.stride(0) if head is not None else 8, _p(q), q.stride(0), _p(mx), mx.stride(0),
                                         c8_col0, M, N, K, int(gelu), _s()))
    return head, q, mx[:, :nb]


def linear_splitk(a, w, bias=None, residual=None, out=None, split_k: int = 0):
    """bf16 out = a @ w.T (+ bias) (+ residual) for few-row operands: split-K GEMM into per-chunk fp32 partial slabs, then one
    summing / converting pass.  Fills the chip when M x N alone gives only a handful of 256x256 tiles."""
    lib = _lib.load()
    M, K = a.shape
    N = w.shape[0]
    n = lib.afx_linear_splitk_chunks(M, N, K, split_k)
    part = torch.empty(n, M, N, dtype=torch.float32, device=a.device)
    _lib.check(lib.afx_linear_bf16_splitk(_p(a), a.stride(0), _p(w), w.stride(0), _p(bias), _p(part), M, N, K, split_k, _s()))
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=a.device)
    _lib.check(lib.afx_finish_f32_bf16(_p(part), n, _p(residual), 0 if residual is None else residual.stride(0), _p(out), out.stride(0),
                                       M, N, _s()))
    return out


def transpose(x, pad_to: int = 1):
    """[R,C] bf16 (row-strided view allowed) -> [C, roundup(R, pad_to)], zero padded."""
    lib = _lib.load()
    R, Cc = x.shape
    Rp = (R + pad_to - 1) // pad_to * pad_to
    y = (torch.zeros if Rp != R else torch.empty)(Cc, Rp, dtype=torch.bfloat16, device=x.device)
    _lib.check(lib.afx_transpose_bf16(_p(x), x.stride(0), _p(y), Rp, R, Cc, _s()))
    return y


def coldot(a, b, out_accum):
    """out_accum[c] += sum_r a[r,c] * b[r,c]   (a, b bf16 row-strided views, out fp32 [C])."""
    lib = _lib.load()
    _mat(a, torch.bfloat16, 'coldot a')
    _mat(b, torch.bfloat16, 'coldot b', a.shape)
    _acc(out_accum, (a.shape[1],), 'coldot out_accum')
    _lib.check(lib.afx_coldot_bf16(_p(a), a.stride(0), _p(b), b.stride(0), _p(out_accum), a.shape[0], a.shape[1], _s()))
    return out_accum


def gate_residual(y, gate, res, out=None):
    """out = res + gate[c] * y   (y, res bf16 [R,C], gate fp32 [C])."""
    lib = _lib.load()
    _mat(y, torch.bfloat16, 'gate_residual y')
    _mat(res, torch.bfloat16, 'gate_residual res', y.shape)
    gate = _cuda(gate, torch.float32)
    if tuple(gate.shape) != (y.shape[1],):
        raise ValueError(f'gate_residual gate: need [{y.shape[1]}], got {tuple(gate.shape)}')
    if out is None:
        out = torch.empty(y.shape[0], y.shape[1], dtype=torch.bfloat16, device=y.device)
    _mat(out, torch.bfloat16, 'gate_residual out', y.shape)
    _lib.check(lib.afx_gate_residual_bf16(_p(y), y.stride(0), _p(gate), _p(res), res.stride(0), _p(out), out.stride(0),
                                          y.shape[0], y.shape[1], _s()))
    return out


def gemv_t(x, w, out_accum):
    """out_accum[b,k] += sum_n x[b,n] w[n,k]   (x fp32 [B<=4, N], w bf16 [N, K], out fp32 [B, K])."""
    lib = _lib.load()
    _mat(x, torch.float32, 'gemv_t x')
    _mat(w, torch.bfloat16, 'gemv_t w')
    if w.shape[0] != x.shape[1]:
        raise ValueError(f'gemv_t: x {tuple(x.shape)} and w {tuple(w.shape)} do not agree on N')
    _acc(out_accum, (x.shape[0], w.shape[1]), 'gemv_t out_accum')
    _lib.check(lib.afx_gemv_t_bf16(_p(x), x.stride(0), _p(w), w.stride(0), _p(out_accum), x.shape[0], x.shape[1], w.shape[1], _s()))
    return out_accum


def colsum(x, out_accum):
    """out_accum[c] += sum_r x[r,c]   (x bf16 row-strided view, out fp32 [C])."""
    lib = _lib.load()
    _mat(x, torch.bfloat16, 'colsum x')
    _acc(out_accum, (x.shape[1],), 'colsum out_accum')
    _lib.check(lib.afx_colsum_bf16(_p(x), x.stride(0), _p(out_accum), x.shape[0], x.shape[1], _s()))
    return out_accum


def normout_backward(x, dxn, dmod_accum, rows_per_batch: int):
    """dmod_accum[b, 0] += sum_rows(b) dxn * LN(x), dmod_accum[b, 1] += sum_rows(b) dxn   (x, dxn bf16 [R, D] views, dmod fp32 [R / rows_per_batch, 2, D])."""
    lib = _lib.load()
    _mat(x, torch.bfloat16, 'normout_backward x')
    _mat(dxn, torch.bfloat16, 'normout_backward dxn', x.shape)
    if rows_per_batch < 1 or x.shape[0] % rows_per_batch:
        raise ValueError(f'normout_backward: {x.shape[0]} rows are not a whole number of batch entries of {rows_per_batch}')
    _acc(dmod_accum, (x.shape[0] // rows_per_batch, 2, x.shape[1]), 'normout_backward dmod_accum')
    _lib.check(lib.afx_normout_backward(_p(x), x.stride(0), _p(dxn), dxn.stride(0), _p(dmod_accum), x.shape[0], x.shape[1],
                                        rows_per_batch, _s()))
    return dmod_accum


def normout_backward_split(x, dxn, d_scale_accum, d_shift_accum):
    """d_scale_accum[D] += sum_rows dxn * LN(x), d_shift_accum[D] += sum_rows dxn (all rows one batch entry; fp32 vectors, e.g. slices of a larger buffer)."""
    lib = _lib.load()
    _mat(x, torch.bfloat16, 'normout_backward_split x')
    _mat(dxn, torch.bfloat16, 'normout_backward_split dxn', x.shape)
    _acc(d_scale_accum, (x.shape[1],), 'normout_backward_split d_scale_accum')
    _acc(d_shift_accum, (x.shape[1],), 'normout_backward_split d_shift_accum')
    _lib.check(lib.afx_normout_backward_split(_p(x), x.stride(0), _p(dxn), dxn.stride(0), _p(d_scale_accum), _p(d_shift_accum), x.shape[0], x.shape[1], _s()))


def outer_accum(dmod, x, dW_accum):
    """dW_accum[j, k] += sum_b dmod[b, j] x[b, k]   (dmod [B, J], x [B, Kd], dW fp32 [J, Kd])."""
    lib = _lib.load()
    dmod, x = _cuda(dmod, torch.float32), _cuda(x, torch.float32)
    if dmod.dim() != 2 or x.dim() != 2 or x.shape[0] != dmod.shape[0]:
        raise ValueError(f'outer_accum: dmod {tuple(dmod.shape)} and x {tuple(x.shape)} need the same batch')
    B, J = dmod.shape
    _acc(dW_accum, (J, x.shape[1]), 'outer_accum dW_accum')
    _lib.check(lib.afx_outer_accum(_p(dmod), _p(x), _p(dW_accum), B, J, x.shape[1], _s()))
    return dW_accum


def sumsq(x, out_accum):
    """out_accum[0] += sum x^2   (x fp32, contiguous)."""
    lib = _lib.load()
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f'sumsq x: need a contiguous float32 tensor, got {x.dtype} strides {x.stride()}')
    _acc(out_accum, (1,), 'sumsq out_accum')
    _lib.check(lib.afx_sumsq(_p(x), _p(out_accum), x.numel(), _s()))
    return out_accum


# The optimizer, EMA and cast wrappers update flat buffers in place through raw pointers and a length: nothing may be converted (a converted
# copy would take the update and be dropped) and nothing may be shorter than the length passed.
def _flat(t, dtype, name: str, n: Optional[int] = None) -> int:
    """A flat operand of an in-place kernel: a GPU tensor of ``dtype``, contiguous, of ``n`` values when given.  -> its numel."""
    if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
        raise ValueError(f'{name}: need a GPU tensor (the kernel takes a device pointer)')
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f'{name}: need a contiguous {dtype} tensor, got {t.dtype} strides {t.stride()}')
    if n is not None and t.numel() != n:
        raise ValueError(f'{name}: {t.numel()} values, need {n}')
    return t.numel()


def _opt_step(step) -> int:
    if int(step) != step or step < 1:
        raise ValueError(f'step: the bias corrections need an integer step >= 1, got {step!r}')
    return int(step)


def adamw_step(param, grad, exp_avg, exp_avg_sq, lr, step, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.0, grad_scale=1.0):
    lib = _lib.load()
    n = _flat(param, torch.float32, 'adamw_step param')
    _flat(grad, torch.float32, 'adamw_step grad', n)
    _flat(exp_avg, torch.float32, 'adamw_step exp_avg', n)
    _flat(exp_avg_sq, torch.float32, 'adamw_step exp_avg_sq', n)
    step = _opt_step(step)
    if n == 0:
        return
    _lib.check(lib.afx_adamw_step(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), lr, betas[0], betas[1], eps,
                                  weight_decay, step, grad_scale, n, _s()))


def dynamic_map(signed: bool = True, max_exponent_bits: int = 7, total_bits: int = 8) -> torch.Tensor:
    """The 256-entry "dynamic" 8-bit code book of bitsandbytes' block-wise optimizers (functional.create_dynamic_map; bitsandbytes
    is an unvendored, unpinned dependency of the reference -- requirements.txt:11 -- so this restates its published construction):
    for every exponent i the interval [0.1, 1] * 10^(i - 6) is cut into 2^i (signed) or 2^(i+1) (unsigned) equal cells whose
    midpoints are codes (mirrored when signed), plus 0 and 1; sorted ascending.  Signed for exp_avg, unsigned for exp_avg_sq."""
    data = []
    non_sign_bits = total_bits - 1
    additional_items = 2 ** (non_sign_bits - max_exponent_bits) - 1
    i = 0
    for i in range(max_exponent_bits):
        fraction_items = int(2 ** (i + non_sign_bits - max_exponent_bits) + 1 if signed else 2 ** (i + non_sign_bits - max_exponent_bits + 1) + 1)
        boundaries = torch.linspace(0.1, 1, fraction_items, dtype=torch.float64)
        means = (boundaries[:-1] + boundaries[1:]) / 2.0
        data += ((10 ** (-(max_exponent_bits - 1) + i)) * means).tolist()
        if signed:
            data += (-(10 ** (-(max_exponent_bits - 1) + i)) * means).tolist()
    if additional_items > 0:
        boundaries = torch.linspace(0.1, 1, additional_items + 1, dtype=torch.float64)
        means = (boundaries[:-1] + boundaries[1:]) / 2.0
        data += ((10 ** (-(max_exponent_bits - 1) + i)) * means).tolist()
        if signed:
            data += (-(10 ** (-(max_exponent_bits - 1) + i)) * means).tolist()
    data += [0.0, 1.0]
    assert len(data) == 2 ** total_bits, len(data)
    return torch.tensor(sorted(data), dtype=torch.float32)


class AdamW8bitState:
    """Block-wise 8-bit moments of ``n`` values: code bytes + one absmax per block of 256 (zero absmax = zero moments)."""
    BLOCK = 256

    def __init__(self, n: int, device):
        nb = (n + self.BLOCK - 1) // self.BLOCK
        self.n = n
        self.state1 = torch.zeros(n, dtype=torch.uint8, device=device)
        self.state2 = torch.zeros(n, dtype=torch.uint8, device=device)
        self.absmax1 = torch.zeros(nb, dtype=torch.float32, device=device)
        self.absmax2 = torch.zeros(nb, dtype=torch.float32, device=device)
        self.qmap1 = dynamic_map(True).to(device)
        self.qmap2 = dynamic_map(False).to(device)

    def moments(self):
        """Dequantised (exp_avg, exp_avg_sq) -- for tests and checkpoint conversion."""
        rep = lambda a: a.repeat_interleave(self.BLOCK)[:self.n]   # noqa: E731
        return self.qmap1[self.state1.long()] * rep(self.absmax1), self.qmap2[self.state2.long()] * rep(self.absmax2)

    def state_dict(self):
        return {k: getattr(self, k).detach().cpu() for k in ('state1', 'state2', 'absmax1', 'absmax2')}

    def load_state_dict(self, sd):
        for k in ('state1', 'state2', 'absmax1', 'absmax2'):
            getattr(self, k).copy_(sd[k])


def adamw8bit_step(param, grad, st: AdamW8bitState, lr, step, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.0, grad_scale=1.0):
    lib = _lib.load()
    n = _flat(param, torch.float32, 'adamw8bit_step param')
    _flat(grad, torch.float32, 'adamw8bit_step grad', n)
    nb = (n + AdamW8bitState.BLOCK - 1) // AdamW8bitState.BLOCK
    if st.n != n:
        raise ValueError(f'adamw8bit_step: the state holds {st.n} values, the parameter {n}')
    _flat(st.state1, torch.uint8, 'adamw8bit_step state1', n)
    _flat(st.state2, torch.uint8, 'adamw8bit_step state2', n)
    _flat(st.absmax1, torch.float32, 'adamw8bit_step absmax1', nb)
    _flat(st.absmax2, torch.float32, 'adamw8bit_step absmax2', nb)
    _flat(st.qmap1, torch.float32, 'adamw8bit_step qmap1', 256)
    _flat(st.qmap2, torch.float32, 'adamw8bit_step qmap2', 256)
    step = _opt_step(step)
    if n == 0:
        return
    _lib.check(lib.afx_adamw8bit_step(_p(param), _p(grad), _p(st.state1), _p(st.state2), _p(st.absmax1), _p(st.absmax2), _p(st.qmap1),
                                      _p(st.qmap2), lr, betas[0], betas[1], eps, weight_decay, step, grad_scale, n, _s()))


def ema_lerp(ema, net, beta: float):
    lib = _lib.load()
    n = _flat(ema, torch.float32, 'ema_lerp ema')
    _flat(net, torch.float32, 'ema_lerp net', n)
    if n == 0:
        return
    _lib.check(lib.afx_ema_lerp(_p(ema), _p(net), beta, n, _s()))


def cast_bf16(x, out=None):
    lib = _lib.load()
    n = _flat(x, torch.float32, 'cast_bf16 x')
    if out is None:
        out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    _flat(out, torch.bfloat16, 'cast_bf16 out', n)
    if out.device != x.device:
        raise ValueError(f'cast_bf16 out: on {out.device}, x on {x.device}')
    if n == 0:
        return out
    _lib.check(lib.afx_cast_f32_bf16(_p(x), _p(out), n, _s()))
    return out


# ---------------------------------------------------------------------------------------------------
# attention with gradient
def attention_fwd_lse(q, k, v):
    """q,k,v [B,S,H,128] bf16 -> (o [B,S,H*128] bf16, lse [B,H,S_pad] f32)."""
    lib = _lib.load()
    B, S, H, Dh = q.shape
    q2, k2, v2 = (t.reshape(B * S, H * Dh) for t in (q.contiguous(), k.contiguous(), v.contiguous()))
    o = torch.empty(B * S, H * Dh, dtype=torch.bfloat16, device=q.device)
    S_pad = (S + 63) // 64 * 64
    lse = torch.full((B, H, S_pad), float('inf'), dtype=torch.float32, device=q.device)
    ws = torch.empty(lib.afx_attention_ws_bytes(B, H, S), dtype=torch.uint8, device=q.device)
    _lib.check(lib.afx_attention_fwd_lse_bf16(_p(q2), H * Dh, _p(k2), H * Dh, _p(v2), H * Dh, _p(o), H * Dh, _p(lse), _p(ws),
                                              B, H, S, _s()))
    return o.reshape(B, S, H * Dh), lse


def attention_bwd(q, k, v, o, dout, lse):
    """-> (dq, dk, dv) each [B,S,H,128] bf16."""
    lib = _lib.load()
    B, S, H, Dh = q.shape
    flat = lambda t: t.contiguous().reshape(B * S, H * Dh)   # noqa: E731
    q2, k2, v2, o2, do2 = flat(q), flat(k), flat(v), flat(o), flat(dout)
    dq, dk, dv = (torch.empty(B * S, H * Dh, dtype=torch.bfloat16, device=q.device) for _ in range(3))
    ws = torch.empty(lib.afx_attention_bwd_ws_bytes(B, H, S), dtype=torch.uint8, device=q.device)
    ld = H * Dh
    _lib.check(lib.afx_attention_bwd_bf16(_p(q2), ld, _p(k2), ld, _p(v2), ld, _p(o2), ld, _p(do2), ld, _p(lse), _p(dq), ld,
                                          _p(dk), ld, _p(dv), ld, _p(ws), B, H, S, _s()))
    return tuple(t.reshape(B, S, H, Dh) for t in (dq, dk, dv))


# ---------------------------------------------------------------------------------------------------
# element-wise trunk backward
def ln_modulate_backward(x, dxn, scale, rows_per_batch: int = 0, dres=None, out=None):
    """dx = dres + LN^T(dxn * (1 + scale[b])); x, dxn [R,D] bf16 (row-strided views allowed), scale [B,D] f32."""
    lib = _lib.load()
    _mat(x, torch.bfloat16, 'ln_modulate_backward x')
    R, D = x.shape
    _mat(dxn, torch.bfloat16, 'ln_modulate_backward dxn', x.shape)
    if dres is not None:
        _mat(dres, torch.bfloat16, 'ln_modulate_backward dres', x.shape)
    if out is None:
        out = torch.empty(R, D, dtype=torch.bfloat16, device=x.device)
    _mat(out, torch.bfloat16, 'ln_modulate_backward out', x.shape)
    scale = _rows_f32(scale, R, D, rows_per_batch, 'scale')
    _lib.check(lib.afx_ln_modulate_backward(_p(x), x.stride(0), _p(dxn), dxn.stride(0), _p(scale), scale.stride(0),
                                            rows_per_batch if rows_per_batch > 0 else max(R, 1), _p(dres),
                                            0 if dres is None else dres.stride(0), _p(out), out.stride(0), R, D, _s()))
    return out


def qk_norm_rope(x, w_txt, w_img, cos, sin, n_txt: int, out=None, dy=None):
    """Out-of-place per-head RMSNorm + RoPE on x [B,S,H*128 view with row stride]; with dy: the backward (dx)."""
    lib = _lib.load()
    B, S, HD = x.shape
    H = HD // 128
    if HD % 128 or not 0 <= n_txt <= S:
        raise ValueError(f'qk_norm_rope: need whole 128-wide heads and 0 <= n_txt <= S, got {tuple(x.shape)}, n_txt {n_txt}')
    x2 = _mat(x.reshape(B * S, HD) if x.is_contiguous() else x.view(B * S, HD), torch.bfloat16, 'qk_norm_rope x')
    if out is None:
        out = torch.empty(B * S, HD, dtype=torch.bfloat16, device=x.device)
    _mat(out, torch.bfloat16, 'qk_norm_rope out', (B * S, HD))
    dy2 = None
    if dy is not None:
        if tuple(dy.shape) != (B, S, HD):
            raise ValueError(f'qk_norm_rope dy: shape {tuple(dy.shape)} != {(B, S, HD)}')
        dy2 = _mat(dy.view(B * S, HD), torch.bfloat16, 'qk_norm_rope dy')
    for t, name in ((cos, 'cos'), (sin, 'sin')):
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (S, 64):
            raise ValueError(f'qk_norm_rope {name}: need a contiguous float32 [{S}, 64] table, got {tuple(t.shape)} {t.dtype}')
    for t, name in ((w_txt, 'w_txt'), (w_img, 'w_img')):
        if t.numel() != 128:
            raise ValueError(f'qk_norm_rope {name}: need 128 weights, got {tuple(t.shape)}')
    _lib.check(lib.afx_qk_norm_rope_oop_bf16(_p(x2), x2.stride(0), _p(out), out.stride(0), _p(dy2),
                                             0 if dy2 is None else dy2.stride(0), _p(_cuda(w_txt, torch.float32)),
                                             _p(_cuda(w_img, torch.float32)), _p(cos), _p(sin), B, S, n_txt, H,
                                             int(dy is not None), _s()))
    return out.view(B, S, HD)


def gelu(pre, dh=None, out=None):
    """h = gelu_tanh(pre) or, with dh, dpre = dh * gelu'(pre); [R,C] bf16 row-strided views."""
    lib = _lib.load()
    _mat(pre, torch.bfloat16, 'gelu pre')
    R, Cc = pre.shape
    if dh is not None:
        _mat(dh, torch.bfloat16, 'gelu dh', pre.shape)
    if out is None:
        out = torch.empty(R, Cc, dtype=torch.bfloat16, device=pre.device)
    _mat(out, torch.bfloat16, 'gelu out', pre.shape)
    _lib.check(lib.afx_gelu_bf16(_p(pre), pre.stride(0), _p(dh), 0 if dh is None else dh.stride(0), _p(out), out.stride(0), R, Cc, _s()))
    return out


def add_scale(a, b=None, gate=None, rows_per_batch: int = 0, out=None):
    """out = (a (+ b)) * gate[batch]; a, b [R,C] bf16 row-strided, gate [B,C] f32."""
    lib = _lib.load()
    _mat(a, torch.bfloat16, 'add_scale a')
    R, Cc = a.shape
    if b is not None:
        _mat(b, torch.bfloat16, 'add_scale b', a.shape)
    if out is None:
        out = torch.empty(R, Cc, dtype=torch.bfloat16, device=a.device)
    _mat(out, torch.bfloat16, 'add_scale out', a.shape)
    if gate is not None:
        gate = _rows_f32(gate, R, Cc, rows_per_batch, 'gate')
    _lib.check(lib.afx_add_scale_bf16(_p(a), a.stride(0), _p(b), 0 if b is None else b.stride(0), _p(gate),
                                      0 if gate is None else gate.stride(0), rows_per_batch if rows_per_batch > 0 else max(R, 1),
                                      _p(out), out.stride(0), R, Cc, _s()))
    return out


def attention_fwd_lse_2d(q, k, v, o, B: int, S: int, H: int):
    """Strided form: q, k, v, o are [B*S, H*128] views (row stride = their stride(0)); returns lse [B,H,S_pad]."""
    lib = _lib.load()
    S_pad = (S + 63) // 64 * 64
    lse = torch.full((B, H, S_pad), float('inf'), dtype=torch.float32, device=q.device)
    ws = torch.empty(lib.afx_attention_ws_bytes(B, H, S), dtype=torch.uint8, device=q.device)
    _lib.check(lib.afx_attention_fwd_lse_bf16(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(o), o.stride(0),
                                              _p(lse), _p(ws), B, H, S, _s()))
    return lse


def attention_bwd_2d(q, k, v, o, dout, lse, dq, dk, dv, B: int, S: int, H: int):
    lib = _lib.load()
    ws = torch.empty(lib.afx_attention_bwd_ws_bytes(B, H, S), dtype=torch.uint8, device=q.device)
    _lib.check(lib.afx_attention_bwd_bf16(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(o), o.stride(0),
                                          _p(dout), dout.stride(0), _p(lse), _p(dq), dq.stride(0), _p(dk), dk.stride(0),
                                          _p(dv), dv.stride(0), _p(ws), B, H, S, _s()))


def lora_fold(base: torch.Tensor, dst: torch.Tensor, A=(), B=(), scales=(), row_gains=None) -> torch.Tensor:
    """dst = bf16(base + sum_j scales[j] * B[j] @ A[j]) (``afx_lora_fold``): base, dst [O, I] bf16 row slices (any row stride >= I) of
    packed weights that do not overlap, A[j] [r_j, I] and B[j] [O, r_j] contiguous bf16 of any rank >= 1, scales[j] python floats applied
    in fp32 to adapter j's fp32-accumulated product.  One rounding, at the store; bit-reproducible; no adapters = a copy.

    row_gains (``afx_lora_fold_rows``): one entry per adapter, None for a plain LoRA or the fp32 [O] row gains of a DoRA adapter
    (``lora_row_gain``): dst = bf16(c * base + sum_j g_j * scales[j] * B[j] @ A[j]) row by row, c = 1 + sum_j (g_j - 1) over the adapters with
    gains.  row_gains=None is the plain fold above, the call it always was."""
    lib = _lib.load()
    _mat(base, torch.bfloat16, 'lora_fold base')
    _mat(dst, torch.bfloat16, 'lora_fold dst', base.shape)
    O, I = base.shape
    J = len(A)
    if len(B) != J or len(scales) != J:
        raise ValueError(f'lora_fold: {J} A, {len(B)} B and {len(scales)} scales')
    for j in range(J):
        _mat(A[j], torch.bfloat16, f'lora_fold A[{j}]')
        _mat(B[j], torch.bfloat16, f'lora_fold B[{j}]')
        r = A[j].shape[0]
        if not (A[j].is_contiguous() and B[j].is_contiguous()) or tuple(A[j].shape) != (r, I) or tuple(B[j].shape) != (O, r):
            raise ValueError(f'lora_fold: adapter {j} needs contiguous A [r, {I}] and B [{O}, r], got {tuple(A[j].shape)} and {tuple(B[j].shape)}')
    n = max(J, 1)
    pa = (C.c_void_p * n)(*[a.data_ptr() for a in A])
    pb = (C.c_void_p * n)(*[b.data_ptr() for b in B])
    rk = (C.c_int32 * n)(*[a.shape[0] for a in A])
    sc = (C.c_float * n)(*[float(s) for s in scales])
    if row_gains is None:
        _lib.check(lib.afx_lora_fold(_p(base), base.stride(0), _p(dst), dst.stride(0), O, I, J, pa, pb, rk, sc, _s()))
        return dst
    if len(row_gains) != J:
        raise ValueError(f'lora_fold: {J} adapters and {len(row_gains)} row_gains')
    for j, g in enumerate(row_gains):
        if g is not None:
            _acc(g, (O,), f'lora_fold row_gains[{j}]')
    pg = (C.c_void_p * n)(*[None if g is None else g.data_ptr() for g in row_gains])
    _lib.check(lib.afx_lora_fold_rows(_p(base), base.stride(0), _p(dst), dst.stride(0), O, I, J, pa, pb, rk, sc, pg, _s()))
    return dst


def lora_fold_terms(base: torch.Tensor, dst: torch.Tensor, terms=()) -> torch.Tensor:
    """dst = bf16(c * base + sum_j g_j * scale_j * D_j) (``afx_lora_fold_terms``): ``lora_fold`` over terms of three kinds, each a dict with
    a python float ``scale`` applied in fp32 to the term's fp32 delta D_j:

    * ``dict(kind='lora', A=[r, I], B=[O, r], scale=s, row_gain=None or fp32 [O])``: D = B @ A, exactly ``lora_fold``'s arithmetic (a call with
      only such terms returns its bits);
    * ``dict(kind='loha', w1_a=[O, r1], w1_b=[r1, I], w2_a=[O, r2], w2_b=[r2, I], scale=s)``: D = (w1_a @ w1_b) * (w2_a @ w2_b), contiguous bf16
      operands of any ranks >= 1, both products kept in fp32;
    * ``dict(kind='lokr', w1=[a, b], w2=[c, d], scale=s, row0=0)``: D = rows row0 .. row0 + O of kron(w1, w2), contiguous fp32 factors with
      b * d == I and row0 + O <= a * c.

    base, dst as for ``lora_fold``; c and g_j are 1 without row gains.  One rounding, at the store; bit-reproducible; no terms = a copy.  The LoHa
    and LoKr rules are LyCORIS' as recalled: not checked against LyCORIS or ComfyUI."""
    lib = _lib.load()
    _mat(base, torch.bfloat16, 'lora_fold_terms base')
    _mat(dst, torch.bfloat16, 'lora_fold_terms dst', base.shape)
    O, I = base.shape
    J = len(terms)
    arr = (_lib.LoraTerm * max(J, 1))()

    def pair(j, up_name, down_name, t):
        up, down = t[up_name], t[down_name]
        _mat(up, torch.bfloat16, f'lora_fold_terms terms[{j}] {up_name}')
        _mat(down, torch.bfloat16, f'lora_fold_terms terms[{j}] {down_name}')
        r = down.shape[0]
        if not (up.is_contiguous() and down.is_contiguous()) or tuple(down.shape) != (r, I) or tuple(up.shape) != (O, r):
            raise ValueError(f'lora_fold_terms: term {j} needs contiguous {down_name} [r, {I}] and {up_name} [{O}, r], got {tuple(down.shape)} and '
                             f'{tuple(up.shape)}')
        return up.data_ptr(), down.data_ptr(), r
    for j, t in enumerate(terms):
        kind = t.get('kind')
        c = arr[j]
        c.scale = float(t['scale'])
        if kind != 'lora' and t.get('row_gain') is not None:
            raise ValueError(f'lora_fold_terms: term {j} is a {kind} term: row gains belong to LoRA terms')
        if kind == 'lora':
            c.kind = _lib.AFX_LORA_TERM_LORA
            c.up, c.down, c.rank = pair(j, 'B', 'A', t)
            if t.get('row_gain') is not None:
                c.row_gain = _acc(t['row_gain'], (O,), f'lora_fold_terms terms[{j}] row_gain').data_ptr()
        elif kind == 'loha':
            c.kind = _lib.AFX_LORA_TERM_LOHA
            c.up, c.down, c.rank = pair(j, 'w1_a', 'w1_b', t)
            c.up2, c.down2, c.rank2 = pair(j, 'w2_a', 'w2_b', t)
        elif kind == 'lokr':
            c.kind = _lib.AFX_LORA_TERM_LOKR
            w1, w2, row0 = t['w1'], t['w2'], int(t.get('row0', 0))
            for name, w in (('w1', w1), ('w2', w2)):
                _gpu(w, name=f'lora_fold_terms terms[{j}] {name}')
                if w.dim() != 2 or w.dtype != torch.float32 or not w.is_contiguous() or 0 in w.shape:
                    raise ValueError(f'lora_fold_terms: term {j} needs a contiguous 2-D float32 {name}, got {tuple(w.shape)} {w.dtype} strides {w.stride()}')
            (ka, kb), (kc, kd) = w1.shape, w2.shape
            if kb * kd != I or row0 < 0 or row0 + O > ka * kc:
                raise ValueError(f'lora_fold_terms: term {j}: kron of w1 {tuple(w1.shape)} and w2 {tuple(w2.shape)} is [{ka * kc}, {kb * kd}], which does '
                                 f'not hold rows {row0} .. {row0 + O} of {I} columns')
            c.w1, c.w2, c.ka, c.kb, c.kc, c.kd, c.row0 = w1.data_ptr(), w2.data_ptr(), ka, kb, kc, kd, row0
        else:
            raise ValueError(f"lora_fold_terms: term {j} has kind {kind!r} (one of 'lora', 'loha', 'lokr')")
    _lib.check(lib.afx_lora_fold_terms(_p(base), base.stride(0), _p(dst), dst.stride(0), O, I, J, C.cast(arr, C.c_void_p), _s()))
    return dst


def lora_row_gain(base: torch.Tensor, A: torch.Tensor, B: torch.Tensor, scale: float, magnitude: torch.Tensor, out=None) -> torch.Tensor:
    """The row gains of one DoRA adapter on one linear (``afx_lora_row_gain``): gain[o] = magnitude[o] / || (base + scale * B @ A)[o, :] ||, fp32
    [O]; base [O, I] bf16 (any row stride >= I), A [r, I] and B [O, r] contiguous bf16 of any rank >= 1, magnitude fp32 [O].  The rows are
    formed as ``lora_fold`` forms them and their squares summed in fp32 in a fixed order: bit-reproducible.  A row of zeros gets gain 0."""
    lib = _lib.load()
    _mat(base, torch.bfloat16, 'lora_row_gain base')
    _mat(A, torch.bfloat16, 'lora_row_gain A')
    _mat(B, torch.bfloat16, 'lora_row_gain B')
    O, I = base.shape
    r = A.shape[0]
    if not (A.is_contiguous() and B.is_contiguous()) or tuple(A.shape) != (r, I) or tuple(B.shape) != (O, r):
        raise ValueError(f'lora_row_gain: needs contiguous A [r, {I}] and B [{O}, r], got {tuple(A.shape)} and {tuple(B.shape)}')
    _acc(magnitude, (O,), 'lora_row_gain magnitude')
    if out is None:
        out = torch.empty(O, dtype=torch.float32, device=base.device)
    _acc(out, (O,), 'lora_row_gain out')
    _lib.check(lib.afx_lora_row_gain(_p(base), base.stride(0), O, I, _p(A), _p(B), r, float(scale), _p(magnitude), _p(out), _s()))
    return out
