"""Prompt encoders on the MI355X engine: the step in front of the denoiser.

The reference gets its prompt embeddings from diffusers' ``encode_prompt`` (lakonlab/models/architecture/diffusers/
pretrained.py:152-238; pipeline call sites arcflux_pipeline.py / arcqwen_pipeline.py ``encode_prompt``), i.e. from three
``transformers`` models:

* ``T5Encoder``         -- T5 v1.1 XXL encoder (FLUX ``text_encoder_2``): ``prompt_embeds`` [B, 512, 4096]
* ``CLIPTextEncoder``   -- CLIP ViT-L/14 text model (FLUX ``text_encoder``): ``pooled_prompt_embeds`` [B, 768]
* ``Qwen25TextEncoder`` -- the language model of Qwen2.5-VL-7B (Qwen-Image ``text_encoder``): last hidden states

Each class takes the ``state_dict`` of the corresponding transformers module (its key names) and runs the forward on the
hand-written kernels: grouped MFMA GEMMs with fused bias / residual epilogues (q|k|v and the gated-MLP pairs are stacked
into one weight), the EXT instantiations of the flash-attention kernel (relative-position bias table for T5, causal mask
for CLIP / Qwen, grouped KV heads for Qwen, head dim 64 / 128), and the row kernels of afx_text.hip.
Parity: tests/test_text_encoders.py runs the real transformers modules (random-init small configs) on the CPU in fp32 as
the oracle -- the third-party dependency itself, not a restatement.  The attention kernel itself is held per element against
fp64 in tests/test_hip_attention_ext_fp64.py (short, ragged and batched lengths, strided operands, the encoders' head counts).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional

import torch

from . import _lib, ops


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Base:
    def __init__(self, device):
        self.lib = _lib.load()
        self.dev = torch.device(device)
        self.w: Dict[str, torch.Tensor] = {}
        self.use_graphs = True
        self.max_graphs = 8
        self._graphs: Dict[int, tuple] = {}

    def _run(self, ids: torch.Tensor) -> torch.Tensor:
        """One sequence through ``self._forward`` (ids int32 on the device -> [S, D]).  A layer is ~10 short launches and
        a prompt has few rows, so the host would be the bottleneck: the launch sequence is captured once per sequence length
        into a HIP graph (torch.cuda.CUDAGraph; every kernel here runs on torch's current stream) and replayed."""
        S = ids.numel()
        ids = ids.to(self.dev, torch.int32).contiguous()
        if not self.use_graphs:
            return self._forward(ids)
        if S not in self._graphs:
            self._prepare(S)
            self._forward(ids)                       # eager warm-up (lazy one-time kernel attribute setup)
            torch.cuda.synchronize()
            static_ids = ids.clone()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                static_out = self._forward(static_ids)
            while len(self._graphs) >= self.max_graphs:      # prompt lengths vary: keep the most recent few (each graph owns
                self._graphs.pop(next(iter(self._graphs)))   # its activation pool)
            self._graphs[S] = (g, static_ids, static_out)
        else:
            self._graphs[S] = self._graphs.pop(S)            # most recently used last
        g, static_ids, static_out = self._graphs[S]
        static_ids.copy_(ids)
        g.replay()
        return static_out.clone()

    def _prepare(self, S: int) -> None:              # per-length tables, built outside the capture
        pass

    def _bf(self, t):
        return t.to(self.dev, torch.bfloat16).contiguous()

    def _f32(self, t):
        return t.to(self.dev, torch.float32).contiguous()

    def _linear(self, x, w, b=None, residual=None):
        """y = x w^T (+ b) (+ residual).  A prompt is one or two 256-row tiles.  Measured on every encoder shape (tools/t5_gemm_probe.py, round 5: the
        rule of round 2 predates the 128x128 / 256x224 shapes of the one-wave-per-SIMD kernel and sent T5-XXL's q|k|v, o and wi launches to split-K at
        1.5-1.9x the plain kernel's time): the plain fused GEMM (the launcher picks 128x128 tiles, two work-groups per CU, when 256x256 would leave half the
        chip idle) costs ~0.6 us per 64-wide K-tile whatever N; splitting K pays only when the K loop itself is long (K >= 8192: T5's wo 85 -> 59 us with 8
        chunks, Qwen2.5-VL's down projection 146 -> 48 us with 16) or when even the small tiles are a handful (<= 80 of them, K >= 3072)."""
        M, N, K = x.shape[0], w.shape[0], w.shape[1]
        t128 = ((M + 127) // 128) * ((N + 127) // 128)
        if K >= 8192:
            return ops.linear_splitk(x, w, b, residual, split_k=8 if K < 16384 else 16)
        if K >= 3072 and t128 <= 80:
            return ops.linear_splitk(x, w, b, residual)
        if residual is not None:
            return ops.linear(x, w, b, epilogue='gate_res', residual=residual)
        return ops.linear(x, w, b)

    def _embed(self, table, ids32, pos=None):
        S, D = ids32.numel(), table.shape[1]
        out = torch.empty(S, D, dtype=torch.bfloat16, device=self.dev)
        _lib.check(self.lib.afx_embed_rows_bf16(_p(table), _p(ids32), _p(pos), _p(out), S, D, _s()))
        return out

    def _norm(self, x, w, b=None, eps=1e-6, rms=True, out=None):
        out = torch.empty_like(x) if out is None else out
        _lib.check(self.lib.afx_norm_rows_bf16(_p(x), x.stride(0), _p(out), out.stride(0), x.shape[0], x.shape[1], _p(w), _p(b),
                                               eps, int(rms), _s()))
        return out

    def _act_mul(self, x, F, gate_off, act):
        out = torch.empty(x.shape[0], F, dtype=torch.bfloat16, device=self.dev)
        _lib.check(self.lib.afx_act_mul_bf16(_p(x), x.stride(0), _p(out), out.stride(0), x.shape[0], F, gate_off, act, _s()))
        return out

    def _attention(self, qkv, Dq, Dk, H, Hkv, d, scale, causal, bias=None):
        """qkv [S, Dq + 2 Dk] rows q | k | v -> [S, Dq]."""
        S = qkv.shape[0]
        o = torch.empty(S, Dq, dtype=torch.bfloat16, device=self.dev)
        ws = torch.empty(self.lib.afx_attention_ext_ws_bytes(1, Hkv, S, d), dtype=torch.uint8, device=self.dev)
        ld = qkv.stride(0)
        _lib.check(self.lib.afx_attention_ext_bf16(_p(qkv), ld, _p(qkv[:, Dq:]), ld, _p(qkv[:, Dq + Dk:]), ld, _p(o), o.stride(0),
                                                   _p(ws), 1, H, Hkv, S, d, scale, int(causal), _p(bias), _s()))
        return o


# ------------------------------------------------------------------------------------------------------------- T5
def t5_relative_buckets(delta: torch.Tensor, num_buckets: int = 32, max_distance: int = 128) -> torch.Tensor:
    """Bidirectional bucket of relative position key - query (transformers T5Attention._relative_position_bucket)."""
    nb = num_buckets // 2
    out = (delta > 0).long() * nb
    n = delta.abs()
    max_exact = nb // 2
    large = max_exact + (torch.log(n.float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)).long()
    large = torch.minimum(large, torch.full_like(large, nb - 1))
    return out + torch.where(n < max_exact, n, large)


class T5Encoder(_Base):
    def __init__(self, state_dict: Dict[str, torch.Tensor], num_layers: int = 24, num_heads: int = 64, d_kv: int = 64,
                 num_buckets: int = 32, max_distance: int = 128, eps: float = 1e-6, device='cuda'):
        super().__init__(device)
        sd = state_dict
        self.L, self.H, self.dkv, self.eps = num_layers, num_heads, d_kv, eps
        self.nb, self.maxd = num_buckets, max_distance
        self.w['embed'] = self._bf(sd['shared.weight'] if 'shared.weight' in sd else sd['encoder.embed_tokens.weight'])
        self.D = self.w['embed'].shape[1]
        for i in range(num_layers):
            a, f = f'encoder.block.{i}.layer.0.', f'encoder.block.{i}.layer.1.'
            self.w[f'{i}.qkv'] = self._bf(torch.cat([sd[a + f'SelfAttention.{n}.weight'] for n in 'qkv']))
            self.w[f'{i}.o'] = self._bf(sd[a + 'SelfAttention.o.weight'])
            self.w[f'{i}.ln1'] = self._f32(sd[a + 'layer_norm.weight'])
            self.w[f'{i}.wi'] = self._bf(torch.cat([sd[f + 'DenseReluDense.wi_0.weight'], sd[f + 'DenseReluDense.wi_1.weight']]))
            self.w[f'{i}.wo'] = self._bf(sd[f + 'DenseReluDense.wo.weight'])
            self.w[f'{i}.ln2'] = self._f32(sd[f + 'layer_norm.weight'])
        self.F = self.w['0.wo'].shape[1]
        self.w['ln_f'] = self._f32(sd['encoder.final_layer_norm.weight'])
        self.rel = sd['encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight'].float()     # [buckets, H]
        self._bias_cache: Dict[int, torch.Tensor] = {}

    def _bias(self, S: int) -> torch.Tensor:
        if S not in self._bias_cache:      # [H][2S-1], index key - query + S - 1; T5 does not scale its scores (scale 1)
            b = t5_relative_buckets(torch.arange(-(S - 1), S), self.nb, self.maxd)
            self._bias_cache[S] = self.rel[b].t().contiguous().to(self.dev)
        return self._bias_cache[S]

    def _prepare(self, S: int) -> None:
        self._bias(S)

    def _forward(self, ids32: torch.Tensor) -> torch.Tensor:
        inner = self.H * self.dkv
        x = self._embed(self.w['embed'], ids32)
        bias = self._bias(ids32.numel())
        for i in range(self.L):
            qkv = self._linear(self._norm(x, self.w[f'{i}.ln1'], eps=self.eps), self.w[f'{i}.qkv'])
            o = self._attention(qkv, inner, inner, self.H, self.H, self.dkv, 1.0, False, bias)
            x = self._linear(o, self.w[f'{i}.o'], residual=x)
            h = self._linear(self._norm(x, self.w[f'{i}.ln2'], eps=self.eps), self.w[f'{i}.wi'])
            x = self._linear(self._act_mul(h, self.F, self.F, 2), self.w[f'{i}.wo'], residual=x)
        return self._norm(x, self.w['ln_f'], eps=self.eps)

    @torch.no_grad()
    def __call__(self, input_ids: torch.Tensor) -> torch.Tensor:
        """input_ids [B, S] -> last_hidden_state [B, S, d_model] bf16 (no attention mask: FLUX passes none, so padding
        tokens attend and are attended like any other -- diffusers ``_get_t5_prompt_embeds``)."""
        return torch.stack([self._run(ids) for ids in input_ids])


# ------------------------------------------------------------------------------------------------------------- CLIP
class CLIPTextEncoder(_Base):
    def __init__(self, state_dict: Dict[str, torch.Tensor], num_layers: int = 12, num_heads: int = 12, eps: float = 1e-5,
                 eos_token_id: int = 2, hidden_act: str = 'quick_gelu', device='cuda'):
        super().__init__(device)
        sd = {k[len('text_model.'):] if k.startswith('text_model.') else k: v for k, v in state_dict.items()}
        self.L, self.H, self.eps, self.eos = num_layers, num_heads, eps, eos_token_id
        self.act = {'quick_gelu': 3, 'gelu': 2, 'gelu_pytorch_tanh': 2}[hidden_act]
        self.w['tok'] = self._bf(sd['embeddings.token_embedding.weight'])
        self.w['pos'] = self._bf(sd['embeddings.position_embedding.weight'])
        self.D = self.w['tok'].shape[1]
        for i in range(num_layers):
            p = f'encoder.layers.{i}.'
            self.w[f'{i}.qkv'] = self._bf(torch.cat([sd[p + f'self_attn.{n}_proj.weight'] for n in 'qkv']))
            self.w[f'{i}.qkv_b'] = self._bf(torch.cat([sd[p + f'self_attn.{n}_proj.bias'] for n in 'qkv']))
            for nm, key in (('o', 'self_attn.out_proj'), ('fc1', 'mlp.fc1'), ('fc2', 'mlp.fc2')):
                self.w[f'{i}.{nm}'], self.w[f'{i}.{nm}_b'] = self._bf(sd[p + key + '.weight']), self._bf(sd[p + key + '.bias'])
            for nm, key in (('ln1', 'layer_norm1'), ('ln2', 'layer_norm2')):
                self.w[f'{i}.{nm}'], self.w[f'{i}.{nm}_b'] = self._f32(sd[p + key + '.weight']), self._f32(sd[p + key + '.bias'])
        self.w['ln_f'], self.w['ln_f_b'] = self._f32(sd['final_layer_norm.weight']), self._f32(sd['final_layer_norm.bias'])

    def _forward(self, ids32: torch.Tensor) -> torch.Tensor:
        d = self.D // self.H
        S = ids32.numel()
        x = self._embed(self.w['tok'], ids32, self.w['pos'][:S])
        for i in range(self.L):
            y = self._norm(x, self.w[f'{i}.ln1'], self.w[f'{i}.ln1_b'], self.eps, rms=False)
            qkv = self._linear(y, self.w[f'{i}.qkv'], self.w[f'{i}.qkv_b'])
            o = self._attention(qkv, self.D, self.D, self.H, self.H, d, d ** -0.5, True)
            x = self._linear(o, self.w[f'{i}.o'], self.w[f'{i}.o_b'], residual=x)
            y = self._norm(x, self.w[f'{i}.ln2'], self.w[f'{i}.ln2_b'], self.eps, rms=False)
            h = self._linear(y, self.w[f'{i}.fc1'], self.w[f'{i}.fc1_b'])
            x = self._linear(self._act_mul(h, h.shape[1], -1, self.act), self.w[f'{i}.fc2'], self.w[f'{i}.fc2_b'], residual=x)
        return self._norm(x, self.w['ln_f'], self.w['ln_f_b'], self.eps, rms=False)

    @torch.no_grad()
    def __call__(self, input_ids: torch.Tensor):
        """input_ids [B, S] -> (last_hidden_state [B, S, D], pooler_output [B, D]); causal attention, no padding mask."""
        hs, pooled = [], []
        for ids in input_ids:
            x = self._run(ids)
            # pooled output = the EOS token's features (transformers CLIPTextTransformer: argmax for the legacy eos id 2)
            pos = int(ids.argmax()) if self.eos == 2 else int((ids == self.eos).int().argmax())
            hs.append(x)
            pooled.append(x[pos])
        return torch.stack(hs), torch.stack(pooled)


# ------------------------------------------------------------------------------------------------------------- Qwen2.5
class Qwen25TextEncoder(_Base):
    def __init__(self, state_dict: Dict[str, torch.Tensor], num_layers: int = 28, num_heads: int = 28, num_kv_heads: int = 4,
                 rope_theta: float = 1e6, eps: float = 1e-6, device='cuda'):
        super().__init__(device)
        sd = {}
        for k, v in state_dict.items():          # language-model tensors under any of the prefixes transformers has used
            for pre in ('model.language_model.', 'language_model.model.', 'model.'):
                if k.startswith(pre) and not k.startswith('model.visual.'):
                    sd.setdefault(k[len(pre):], v)
                    break
        self.L, self.H, self.Hkv, self.theta, self.eps = num_layers, num_heads, num_kv_heads, rope_theta, eps
        self.w['embed'] = self._bf(sd['embed_tokens.weight'])
        self.D = self.w['embed'].shape[1]
        self.d = self.D // num_heads
        for i in range(num_layers):
            p = f'layers.{i}.'
            self.w[f'{i}.qkv'] = self._bf(torch.cat([sd[p + f'self_attn.{n}_proj.weight'] for n in 'qkv']))
            self.w[f'{i}.qkv_b'] = self._bf(torch.cat([sd[p + f'self_attn.{n}_proj.bias'] for n in 'qkv']))
            self.w[f'{i}.o'] = self._bf(sd[p + 'self_attn.o_proj.weight'])
            self.w[f'{i}.gu'] = self._bf(torch.cat([sd[p + 'mlp.gate_proj.weight'], sd[p + 'mlp.up_proj.weight']]))
            self.w[f'{i}.down'] = self._bf(sd[p + 'mlp.down_proj.weight'])
            self.w[f'{i}.ln1'] = self._f32(sd[p + 'input_layernorm.weight'])
            self.w[f'{i}.ln2'] = self._f32(sd[p + 'post_attention_layernorm.weight'])
        self.F = self.w['0.down'].shape[1]
        self.w['ln_f'] = self._f32(sd['norm.weight'])
        self._rope_cache: Dict[int, tuple] = {}

    def _rope(self, S: int):
        # text-only prompts: the three M-RoPE position streams are identical, so the sectioned table is the plain 1-D one
        inv = 1.0 / (self.theta ** (torch.arange(0, self.d, 2, dtype=torch.float32) / self.d))
        ang = torch.arange(S, dtype=torch.float32)[:, None] * inv[None]
        return ang.cos().contiguous().to(self.dev), ang.sin().contiguous().to(self.dev)

    def _prepare(self, S: int) -> None:
        self._rope_cache[S] = self._rope(S)

    def _forward(self, ids32: torch.Tensor) -> torch.Tensor:
        Dq, Dk = self.H * self.d, self.Hkv * self.d
        S = ids32.numel()
        if S not in self._rope_cache:
            self._prepare(S)
        cos, sin = self._rope_cache[S]
        x = self._embed(self.w['embed'], ids32)
        for i in range(self.L):
            qkv = self._linear(self._norm(x, self.w[f'{i}.ln1'], eps=self.eps), self.w[f'{i}.qkv'], self.w[f'{i}.qkv_b'])
            _lib.check(self.lib.afx_rope_half_bf16(_p(qkv), qkv.stride(0), _p(cos), _p(sin), S, self.H + self.Hkv, self.d, _s()))
            o = self._attention(qkv, Dq, Dk, self.H, self.Hkv, self.d, self.d ** -0.5, True)
            x = self._linear(o, self.w[f'{i}.o'], residual=x)
            h = self._linear(self._norm(x, self.w[f'{i}.ln2'], eps=self.eps), self.w[f'{i}.gu'])
            x = self._linear(self._act_mul(h, self.F, self.F, 1), self.w[f'{i}.down'], residual=x)
        return self._norm(x, self.w['ln_f'], eps=self.eps)

    @torch.no_grad()
    def __call__(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """input_ids [B, S] (+ padding mask, either side) -> hidden_states[-1] [B, S, D] (after the final norm).  Only the
        valid tokens are run (positions = running count of valid tokens, as transformers derives them from the mask);
        rows of masked positions are zero (transformers leaves meaningless values there; callers drop them)."""
        outs = []
        for bi, ids_full in enumerate(input_ids):
            keep = attention_mask[bi].bool() if attention_mask is not None else torch.ones_like(ids_full, dtype=torch.bool)
            x = self._run(ids_full[keep])
            full = x.new_zeros(ids_full.numel(), self.D)
            full[keep.to(self.dev)] = x
            outs.append(full)
        return torch.stack(outs)


# ------------------------------------------------------------------------------------------------------------- loading
def _read_dir(path: str):
    """config.json + every safetensors shard of a transformers model directory."""
    import glob
    import json
    import os
    from safetensors import safe_open
    with open(os.path.join(path, 'config.json')) as f:
        cfg = json.load(f)
    sd: Dict[str, torch.Tensor] = {}
    files = sorted(glob.glob(os.path.join(path, '*.safetensors')))
    if not files:
        raise EnvironmentError(f'no safetensors weights under {path}')
    for fn in files:
        with safe_open(fn, framework='pt', device='cpu') as f:
            for k in f.keys():
                sd[k] = f.get_tensor(k)
    return cfg, sd


def load_t5_encoder(path: str, device='cuda') -> T5Encoder:
    c, sd = _read_dir(path)
    return T5Encoder(sd, c['num_layers'], c['num_heads'], c['d_kv'], c.get('relative_attention_num_buckets', 32),
                     c.get('relative_attention_max_distance', 128), c.get('layer_norm_epsilon', 1e-6), device)


def load_clip_text_encoder(path: str, device='cuda') -> CLIPTextEncoder:
    c, sd = _read_dir(path)
    c = c.get('text_config', c)
    return CLIPTextEncoder(sd, c['num_hidden_layers'], c['num_attention_heads'], c.get('layer_norm_eps', 1e-5),
                           c.get('eos_token_id', 2), c.get('hidden_act', 'quick_gelu'), device)


def load_qwen25_text_encoder(path: str, device='cuda') -> Qwen25TextEncoder:
    c, sd = _read_dir(path)
    t = c.get('text_config', c)
    return Qwen25TextEncoder(sd, t['num_hidden_layers'], t['num_attention_heads'], t['num_key_value_heads'],
                             t.get('rope_theta', 1e6), t.get('rms_norm_eps', 1e-6), device)
