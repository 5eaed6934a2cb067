"""AutoencoderKL decoder on the MI355X engine: the ``vae.decode`` step that follows the ArcFlow loop
(reference lakonlab/pipelines/arcflux_pipeline.py:531-534, wrapper lakonlab/models/architecture/diffusers/pretrained.py:22-149).

MI355X-first layout: NHWC bf16 activations on zero-bordered grids; every 3x3 convolution is an implicit GEMM on the
8-phase MFMA kernel (tap = row shift, no im2col, residual add fused in the epilogue); GroupNorm(32)+SiLU, nearest
upsample, softmax and the layout conversions are single-pass streaming kernels; the mid-block attention (one head,
dim 512, 16 384 tokens at 1024^2) is two MFMA GEMMs around an fp32 row softmax.  Weights are re-laid once at load:
conv [Cout,Cin,3,3] -> [Cout][tap][Cin] (K-contiguous), to_q|to_k|to_v stacked.
"""
from __future__ import annotations

import os

import ctypes as C
from typing import Dict, Sequence

import torch

from . import _lib, ops


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Grid:
    """Zero-bordered NHWC activation [(H+2)*(W+2), C] with guard rows on both sides (the shifted taps of the implicit
    GEMM read up to W+3 rows outside the grid; what they produce lands on border rows, which the epilogue zeroes)."""

    def __init__(self, H: int, W: int, Cn: int, device, buf: torch.Tensor = None):
        self.H, self.W, self.C = H, W, Cn
        self.guard = W + 3
        rows = (H + 2) * (W + 2)
        self.buf = torch.zeros(rows + 2 * self.guard, Cn, dtype=torch.bfloat16, device=device) if buf is None else buf
        self.t = self.buf[self.guard:self.guard + rows]
        self.stats = None           # GroupNorm partial sums of this grid, left by the convolution that produced it (afx_conv3x3_bf16_stats)


class _GridPool:
    """Recycles activation grids between layers and decodes.  Every producer kernel rewrites the whole grid INCLUDING its
    zero border (conv / linear epilogues, norm kernels, upsample), and nothing ever writes the guard rows, so a recycled
    buffer needs no re-zeroing.  A ring of 6 buffers per shape covers the longest live range of a ResNet block (input kept
    for the residual while norm1 / conv1 / norm2 / conv2 outputs are produced)."""
    RING = 6

    def __init__(self, device):
        self.dev = device
        self.rings = {}

    def grid(self, H: int, W: int, Cn: int) -> _Grid:
        ring = self.rings.setdefault((H, W, Cn), [[], 0])
        if len(ring[0]) < self.RING:
            g = _Grid(H, W, Cn, self.dev)
            ring[0].append(g.buf)
            return g
        buf = ring[0][ring[1] % self.RING]
        ring[1] += 1
        return _Grid(H, W, Cn, self.dev, buf)


def phase_weights(wp9: torch.Tensor, cin: int) -> torch.Tensor:
    """[Cout, 9 * cin] (tap-major 3x3 kernel, the layout of afx_conv3x3_bf16) -> [4, Cout, 4 * cin]: the four 2x2 kernels of
    conv3x3(nearest-2x upsample(.)) acting on the LOW-resolution grid.  Output pixel (2y + py, 2x + px) reads source rows {y - 1 + py, y + py}:
    for py = 0 the taps dy = -1 | {0, +1} fall on them, for py = 1 the taps {-1, 0} | +1 (the same in x); taps on one source pixel add up
    (in fp32, rounded once to bf16).  Phase index 2 py + px, tap index 2 ty + tx: the layout afx_upconv3x3_bf16 expects."""
    co = wp9.shape[0]
    w = wp9.float().reshape(co, 3, 3, cin)
    rows = {0: ([0], [1, 2]), 1: ([0, 1], [2])}                   # phase -> 3x3 tap indices landing on source row 0 / 1 of the 2x2 footprint
    out = torch.zeros(4, co, 2, 2, cin, dtype=torch.float32, device=wp9.device)
    for py in (0, 1):
        for px in (0, 1):
            for ty in (0, 1):
                for tx in (0, 1):
                    acc = 0
                    for a in rows[py][ty]:
                        for b in rows[px][tx]:
                            acc = acc + w[:, a, b]
                    out[2 * py + px, :, ty, tx] = acc
    return out.reshape(4, co, 4 * cin).to(torch.bfloat16).contiguous()


def _upconv(lib, pool, x: "_Grid", w4: torch.Tensor, b: torch.Tensor) -> "_Grid":
    """conv3x3(nearest-2x upsample(x)) + b through afx_upconv3x3_bf16: the upsampled grid is never written."""
    y = pool.grid(2 * x.H, 2 * x.W, w4.shape[1])
    _lib.check(lib.afx_upconv3x3_bf16(_p(x.t), _p(w4), _p(b), _p(y.t), x.H, x.W, x.C, w4.shape[1], _s()))
    return y


def _single_head_attention(lib, xn: _Grid, x: _Grid, w_qkv, b_qkv, w_out, b_out, scale: float) -> _Grid:
    """x + proj(softmax(q k^T * scale) v) over the H*W pixels of a grid (xn = normalised x): two MFMA GEMMs around an fp32
    row softmax.  The token count is padded to a multiple of 64 for the GEMM contraction; padded keys get P = 0."""
    H, W, Cn = x.H, x.W, x.C
    N = H * W
    dev = x.t.device
    Np = (N + 63) // 64 * 64
    xc = torch.zeros(Np, Cn, dtype=torch.bfloat16, device=dev)
    _lib.check(lib.afx_interior_nhwc(_p(xn.t), _p(xc), None, H, W, Cn, 0, _s()))
    qkv = ops.linear(xc, w_qkv, b_qkv)                                                       # [Np, 3C]
    q, k, v = qkv[:, :Cn], qkv[:, Cn:2 * Cn], qkv[:, 2 * Cn:]
    s = ops.linear_f32out(q, k)                                                              # [Np, Np] fp32 logits
    pm = torch.zeros(Np, Np, dtype=torch.bfloat16, device=dev)
    _lib.check(lib.afx_softmax_rows_f32(_p(s), s.stride(0), _p(pm), Np, N, N, scale, _s()))
    o = ops.linear(pm, ops.transpose(v))                                                     # [N, C] = P V
    oc = ops.linear(o, w_out, b_out)
    y = _Grid(H, W, Cn, dev)
    _lib.check(lib.afx_interior_nhwc(_p(y.t), _p(oc), _p(x.t), H, W, Cn, 1, _s()))
    return y


class _VAEFacade:
    """``pipe.vae`` stays the decoder object; when the snapshot's ``vae/`` also holds ``encoder.*`` weights the pipeline attaches the encoder
    here, so ``pipe.vae.encode(...)`` works as on the reference's ``PretrainedVAE`` wrappers."""
    encoder = None

    def encode(self, images: torch.Tensor, **kw):
        if self.encoder is None:
            raise RuntimeError('this VAE was loaded without encoder.* weights (decoder-only snapshot): encode() needs a snapshot whose vae/ holds them')
        return self.encoder.encode(images, **kw)


class _KLBlocks:
    """What the AutoencoderKL decoder and encoder share: the weight re-layout at load time and the layer primitives on grids
    (3x3 convolution with GroupNorm sums from its epilogue, GroupNorm(+SiLU), ResnetBlock2D, the single-head mid-block attention)."""

    def _setup(self, state_dict: Dict[str, torch.Tensor], prefix: str, norm_num_groups: int, device):
        self.lib = _lib.load()
        self.dev = torch.device(device)
        self.groups = norm_num_groups
        self.w: Dict[str, torch.Tensor] = {}
        sd = state_dict
        for k in [k for k in sd if k.startswith(prefix) and k.endswith('.weight')]:
            name = k[:-len('.weight')]
            wt, b = sd[k], sd.get(name + '.bias')
            if self._relay(name, wt, b):                                  # a layer with a layout of its own (the encoder's conv_in / downsamplers)
                continue
            if wt.dim() == 4 and wt.shape[-1] == 3:                       # 3x3 conv -> [Cout][tap][Cin], K-contiguous
                co, ci = wt.shape[:2]
                cip, cop = max(64, (ci + 63) // 64 * 64), (co + 7) // 8 * 8
                wp = torch.zeros(cop, 9, cip, dtype=torch.bfloat16)
                wp[:co, :, :ci] = wt.permute(0, 2, 3, 1).reshape(co, 9, ci).to(torch.bfloat16)
                bp = torch.zeros(cop, dtype=torch.bfloat16)
                bp[:co] = b.to(torch.bfloat16)
                self.w[name + '.weight'], self.w[name + '.bias'] = wp.reshape(cop, 9 * cip).to(self.dev), bp.to(self.dev)
            elif wt.dim() == 4:                                           # 1x1 conv_shortcut -> linear
                self.w[name + '.weight'] = wt.reshape(wt.shape[0], wt.shape[1]).to(self.dev, torch.bfloat16).contiguous()
                self.w[name + '.bias'] = b.to(self.dev, torch.bfloat16)
            elif wt.dim() == 2:
                self.w[name + '.weight'] = wt.to(self.dev, torch.bfloat16).contiguous()
                self.w[name + '.bias'] = b.to(self.dev, torch.bfloat16)
            else:                                                         # GroupNorm affine
                self.w[name + '.weight'] = wt.to(self.dev, torch.float32)
                self.w[name + '.bias'] = b.to(self.dev, torch.float32)
        a = prefix + 'mid_block.attentions.0.'
        self.w[a + 'qkv.weight'] = torch.cat([self.w[a + n + '.weight'] for n in ('to_q', 'to_k', 'to_v')]).contiguous()
        self.w[a + 'qkv.bias'] = torch.cat([self.w[a + n + '.bias'] for n in ('to_q', 'to_k', 'to_v')]).contiguous()
        self._stats = torch.zeros(int(self.lib.afx_groupnorm_ws_bytes(2048, self.groups)) // 8, dtype=torch.float64, device=self.dev)   # afx_groupnorm_nhwc's scratch, sized by the library
        self._pool = _GridPool(self.dev)
        # GroupNorm sums out of the producing convolution's epilogue: a ring of slotted buffers (a grid's sums live until its norm ran:
        # at most the block input + conv1 output at a time; 4 is generous)
        self._conv_stats = bool(self.lib.afx_conv_stats_available()) and os.environ.get('AFX_VAE_CONV_STATS', '1') != '0'     # (0: A/B runs)
        self._stat_ring = [torch.zeros(64 * 2 * self.groups, dtype=torch.float64, device=self.dev) for _ in range(4)]
        self._stat_i = 0

    def _relay(self, name: str, wt: torch.Tensor, b: torch.Tensor) -> bool:
        return False

    def _stat_slot(self, co: int):
        """The statistics buffer for a convolution output of co channels that feeds a GroupNorm, or None when the epilogue cannot take it."""
        gs = co // self.groups if co % self.groups == 0 else 0
        if not (self._conv_stats and co <= 128 and gs >= 4 and gs % 4 == 0 and (gs <= 8 or gs % 8 == 0)):
            return None
        st = self._stat_ring[self._stat_i % len(self._stat_ring)]
        self._stat_i += 1
        return st

    # ------------------------------------------------------------------ primitives on grids
    def _conv(self, name: str, x: _Grid, cout: int, res: _Grid = None, stats: bool = True) -> _Grid:
        """stats: the output feeds a GroupNorm -> its sums come out of the GEMM epilogue (no statistics pass over the grid later)."""
        w, b = self.w[name + '.weight'], self.w[name + '.bias']
        co = w.shape[0]
        y = self._pool.grid(x.H, x.W, co)
        y.stats = self._stat_slot(co) if stats else None
        if y.stats is not None:
            _lib.check(self.lib.afx_conv3x3_bf16_stats(_p(x.t), _p(w), _p(b), _p(y.t), x.H, x.W, x.C, co, None if res is None else _p(res.t),
                                                       _p(y.stats), self.groups, _s()))
        else:
            _lib.check(self.lib.afx_conv3x3_bf16(_p(x.t), _p(w), _p(b), _p(y.t), x.H, x.W, x.C, co, None if res is None else _p(res.t), _s()))
        return y

    def _gn(self, name: str, x: _Grid, act: bool) -> _Grid:
        y = self._pool.grid(x.H, x.W, x.C)
        g, b = self.w[name + '.weight'], self.w[name + '.bias']
        if x.stats is not None:
            _lib.check(self.lib.afx_groupnorm_nhwc_from_stats(_p(x.t), _p(y.t), _p(x.stats), _p(self._stats), x.H, x.W, x.C, self.groups,
                                                              _p(g), _p(b), 1e-6, int(act), _s()))
        else:
            _lib.check(self.lib.afx_groupnorm_nhwc(_p(x.t), _p(y.t), _p(self._stats), x.H, x.W, x.C, self.groups, _p(g), _p(b), 1e-6, int(act), _s()))
        return y

    def _resnet(self, p: str, x: _Grid) -> _Grid:
        h = self._conv(p + 'conv1', self._gn(p + 'norm1', x, True), 0)
        skip = x
        if p + 'conv_shortcut.weight' in self.w:
            skip = self._pool.grid(x.H, x.W, self.w[p + 'conv_shortcut.weight'].shape[0])
            ops.linear(x.t, self.w[p + 'conv_shortcut.weight'], self.w[p + 'conv_shortcut.bias'], out=skip.t)
        return self._conv(p + 'conv2', self._gn(p + 'norm2', h, True), 0, res=skip)

    def _attention(self, p: str, x: _Grid) -> _Grid:
        xn = self._gn(p + 'group_norm', x, False)
        return _single_head_attention(self.lib, xn, x, self.w[p + 'qkv.weight'], self.w[p + 'qkv.bias'],
                                      self.w[p + 'to_out.0.weight'], self.w[p + 'to_out.0.bias'], x.C ** -0.5)


class AutoencoderKLDecoder(_KLBlocks, _VAEFacade):
    def __init__(self, state_dict: Dict[str, torch.Tensor], block_out_channels: Sequence[int] = (128, 256, 512, 512),
                 norm_num_groups: int = 32, layers_per_block: int = 2, scaling_factor: float = 0.3611,
                 shift_factor: float = 0.1159, device='cuda'):
        self._setup(state_dict, 'decoder.', norm_num_groups, device)
        self.lpb = layers_per_block
        self.rev = list(reversed(block_out_channels))
        self.scaling_factor, self.shift_factor = scaling_factor, shift_factor
        self.config = type('cfg', (), dict(scaling_factor=scaling_factor, shift_factor=shift_factor))()
        # nearest-2x upsample folded into the upsamplers' convolutions (four 2x2 phase kernels on the low-resolution grid)
        self._fold_up = bool(self.lib.afx_conv_stats_available()) and os.environ.get('AFX_VAE_FOLD_UPSAMPLE', '1') != '0'     # (0: A/B runs)
        if self._fold_up:
            for k in [k for k in self.w if '.upsamplers.0.conv.weight' in k]:
                self.w[k[:-len('.weight')] + '.weight4'] = phase_weights(self.w[k], self.w[k].shape[1] // 9)

    # ------------------------------------------------------------------ decode
    @torch.no_grad()
    def decode_tokens(self, tokens: torch.Tensor, hp: int, wp: int) -> torch.Tensor:
        """tokens: packed latents [hp*wp, 64] fp32 (the loop's output for ONE image) -> image [3, 16hp, 16wp] fp32."""
        x = self._pool.grid(2 * hp, 2 * wp, 64)
        _lib.check(self.lib.afx_latent_to_nhwc(_p(tokens.to(self.dev, torch.float32).contiguous()), _p(x.t), hp, wp, 64,
                                               self.scaling_factor, self.shift_factor, _s()))
        x = self._conv('decoder.conv_in', x, 0)
        x = self._resnet('decoder.mid_block.resnets.0.', x)
        x = self._attention('decoder.mid_block.attentions.0.', x)
        x = self._resnet('decoder.mid_block.resnets.1.', x)
        n = len(self.rev)
        for i in range(n):
            for j in range(self.lpb + 1):
                x = self._resnet(f'decoder.up_blocks.{i}.resnets.{j}.', x)
            if i < n - 1:
                un = f'decoder.up_blocks.{i}.upsamplers.0.conv'
                if self._fold_up:
                    x = _upconv(self.lib, self._pool, x, self.w[un + '.weight4'], self.w[un + '.bias'])
                else:
                    up = self._pool.grid(2 * x.H, 2 * x.W, x.C)
                    _lib.check(self.lib.afx_upsample2x_nhwc(_p(x.t), _p(up.t), x.H, x.W, x.C, _s()))
                    x = self._conv(un, up, 0)
        x = self._conv('decoder.conv_out', self._gn('decoder.conv_norm_out', x, True), 0, stats=False)
        img = torch.empty(3, x.H, x.W, dtype=torch.float32, device=self.dev)
        _lib.check(self.lib.afx_nhwc_to_image(_p(x.t), _p(img), x.H, x.W, x.C, _s()))
        return img

    def decode_packed(self, latents: torch.Tensor, hp: int, wp: int) -> torch.Tensor:
        """[B, hp*wp, 64] packed latents -> [B, 3, 16hp, 16wp]."""
        return torch.stack([self.decode_tokens(latents[b], hp, wp) for b in range(latents.shape[0])])


def _c64(c: int) -> int:
    return (c + 63) // 64 * 64


class _QwenBlocks:
    """What the AutoencoderKLQwenImage decoder and encoder share on ONE frame: every causal 3-D convolution reduced to its last temporal tap
    and re-laid as a 2-D kernel on grids padded to multiples of 64 channels, the per-pixel RMS norm, the residual block and the attention."""

    def _setup(self, state_dict: Dict[str, torch.Tensor], prefix: str, narrow: Dict[str, int], device):
        """narrow: layer name -> padded output width for the layers whose output is not a grid the next convolution reads."""
        self.lib = _lib.load()
        self.dev = torch.device(device)
        self.w: Dict[str, torch.Tensor] = {}
        self.creal: Dict[str, int] = {}
        sd = {k: v.detach().cpu() for k, v in state_dict.items()}          # repacked on the host (a few hundred MB, once), then uploaded
        for k in [k for k in sd if k.startswith(prefix) and k.endswith('.weight') and 'time_conv' not in k]:
            name = k[:-len('.weight')]
            wt, b = sd[k].float(), sd[name + '.bias'].float()
            if wt.dim() == 5:
                wt = wt[:, :, -1]                                         # causal: only the last temporal tap sees the frame
            co, ci = wt.shape[:2]
            cop = narrow.get(name, _c64(co))
            cip = _c64(ci)
            bp = torch.zeros(cop, dtype=torch.bfloat16)
            bp[:co] = b.to(torch.bfloat16)
            self.creal[name] = co
            if self._relay(name, wt, b, cop):                             # a layer with a layout of its own (the encoder's conv_in / downsamplers)
                continue
            if wt.shape[-1] == 3:                                         # 3x3 -> [Cout][tap][Cin], K-contiguous
                wp = torch.zeros(cop, 9, cip, dtype=torch.bfloat16)
                wp[:co, :, :ci] = wt.permute(0, 2, 3, 1).reshape(co, 9, ci).to(torch.bfloat16)
                self.w[name + '.weight'] = wp.reshape(cop, 9 * cip).to(self.dev)
            else:                                                         # 1x1 -> linear
                wp = torch.zeros(cop, cip, dtype=torch.bfloat16)
                wp[:co, :ci] = wt.reshape(co, ci).to(torch.bfloat16)
                self.w[name + '.weight'] = wp.to(self.dev)
            self.w[name + '.bias'] = bp.to(self.dev)
        for k in [k for k in sd if k.startswith(prefix) and k.endswith('.gamma')]:
            gm = sd[k].float().flatten()
            gp = torch.zeros(_c64(gm.numel()), dtype=torch.float32)
            gp[:gm.numel()] = gm
            self.w[k], self.creal[k] = gp.to(self.dev), gm.numel()
        self._pool = _GridPool(self.dev)
        return sd

    def _relay(self, name: str, wt: torch.Tensor, b: torch.Tensor, cop: int) -> bool:
        return False

    def _conv(self, name: str, x: _Grid, res: _Grid = None) -> _Grid:
        w, b = self.w[name + '.weight'], self.w[name + '.bias']
        y = self._pool.grid(x.H, x.W, w.shape[0])
        _lib.check(self.lib.afx_conv3x3_bf16(_p(x.t), _p(w), _p(b), _p(y.t), x.H, x.W, x.C, w.shape[0],
                                             None if res is None else _p(res.t), _s()))
        return y

    def _norm(self, name: str, x: _Grid, act: bool) -> _Grid:
        y = self._pool.grid(x.H, x.W, x.C)
        _lib.check(self.lib.afx_rmsnorm_nhwc(_p(x.t), _p(y.t), x.t.shape[0], x.C, self.creal[name + '.gamma'],
                                             _p(self.w[name + '.gamma']), int(act), _s()))
        return y

    def _mid_attention(self, a: str, x: _Grid) -> _Grid:
        return _single_head_attention(self.lib, self._norm(a + 'norm', x, False), x, self.w[a + 'to_qkv.weight'], self.w[a + 'to_qkv.bias'],
                                      self.w[a + 'proj.weight'], self.w[a + 'proj.bias'], self.creal[a + 'norm.gamma'] ** -0.5)

    def _resnet(self, p: str, x: _Grid) -> _Grid:
        skip = x
        if p + 'conv_shortcut.weight' in self.w:
            skip = self._pool.grid(x.H, x.W, self.w[p + 'conv_shortcut.weight'].shape[0])
            ops.linear(x.t, self.w[p + 'conv_shortcut.weight'], self.w[p + 'conv_shortcut.bias'], out=skip.t)
        h = self._conv(p + 'conv1', self._norm(p + 'norm1', x, True))
        return self._conv(p + 'conv2', self._norm(p + 'norm2', h, True), res=skip)


class AutoencoderKLQwenImageDecoder(_QwenBlocks, _VAEFacade):
    """Decoder of AutoencoderKLQwenImage for single images (reference arcqwen_pipeline.py:470-481 and
    lakonlab/models/architecture/diffusers/pretrained.py:142-149).  With one latent frame the causal 3-D convolutions
    see two zero frames in front, so each reduces to its LAST temporal tap as a 2-D kernel and the temporal ``time_conv``
    of the 3-D upsamplers is never reached; those 2-D kernels run as implicit GEMMs like the FLUX decoder's.  Channel
    counts that are not multiples of 64 (96) live on grids padded to the next multiple (zero weights / gamma there).
    The per-channel latent un-normalisation and the 1x1x1 ``post_quant_conv`` are folded into the unpack kernel."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], latents_mean: Sequence[float], latents_std: Sequence[float],
                 dim_mult: Sequence[int] = (1, 2, 4, 4), num_res_blocks: int = 2, z_dim: int = 16, device='cuda'):
        assert z_dim == 16, 'the packed-latent layout of the pipelines has 16 latent channels'
        sd = self._setup(state_dict, 'decoder.', {'decoder.conv_out': 8}, device)
        self.n_up, self.nrb = len(dim_mult), num_res_blocks
        self.latents_mean, self.latents_std = list(latents_mean), list(latents_std)
        self.config = type('cfg', (), dict(latents_mean=self.latents_mean, latents_std=self.latents_std, z_dim=z_dim))()
        # v = post_quant_conv(lat * std + mean) = (Wq diag(std)) lat + (Wq mean + bq)
        wq = sd['post_quant_conv.weight'].float().reshape(16, 16)
        std, mean = torch.tensor(self.latents_std, dtype=torch.float32), torch.tensor(self.latents_mean, dtype=torch.float32)
        self._fold_up = bool(self.lib.afx_conv_stats_available()) and os.environ.get('AFX_VAE_FOLD_UPSAMPLE', '1') != '0'
        if self._fold_up:
            for k in [k for k in self.w if '.upsamplers.0.resample.1.weight' in k]:
                self.w[k[:-len('.weight')] + '.weight4'] = phase_weights(self.w[k], self.w[k].shape[1] // 9)
        self._A = (wq * std[None, :]).contiguous().to(self.dev)
        self._b = (wq @ mean + sd['post_quant_conv.bias'].float()).contiguous().to(self.dev)

    @torch.no_grad()
    def decode_tokens(self, tokens: torch.Tensor, hp: int, wp: int) -> torch.Tensor:
        """tokens: packed latents [hp*wp, 64] fp32 of ONE image -> image [3, 16hp, 16wp] fp32 in [-1, 1]."""
        x = self._pool.grid(2 * hp, 2 * wp, 64)
        _lib.check(self.lib.afx_latent_to_nhwc_affine(_p(tokens.to(self.dev, torch.float32).contiguous()), _p(x.t), hp, wp, 64,
                                                      _p(self._A), _p(self._b), _s()))
        x = self._conv('decoder.conv_in', x)
        x = self._resnet('decoder.mid_block.resnets.0.', x)
        x = self._mid_attention('decoder.mid_block.attentions.0.', x)
        x = self._resnet('decoder.mid_block.resnets.1.', x)
        for i in range(self.n_up):
            for j in range(self.nrb + 1):
                x = self._resnet(f'decoder.up_blocks.{i}.resnets.{j}.', x)
            if i != self.n_up - 1:
                un = f'decoder.up_blocks.{i}.upsamplers.0.resample.1'
                if self._fold_up:
                    x = _upconv(self.lib, self._pool, x, self.w[un + '.weight4'], self.w[un + '.bias'])
                else:
                    up = self._pool.grid(2 * x.H, 2 * x.W, x.C)
                    _lib.check(self.lib.afx_upsample2x_nhwc(_p(x.t), _p(up.t), x.H, x.W, x.C, _s()))
                    x = self._conv(un, up)
        x = self._conv('decoder.conv_out', self._norm('decoder.norm_out', x, True))
        img = torch.empty(3, x.H, x.W, dtype=torch.float32, device=self.dev)
        _lib.check(self.lib.afx_nhwc_to_image(_p(x.t), _p(img), x.H, x.W, x.C, _s()))
        return img.clamp_(-1.0, 1.0)

    def decode_packed(self, latents: torch.Tensor, hp: int, wp: int) -> torch.Tensor:
        return torch.stack([self.decode_tokens(latents[b], hp, wp) for b in range(latents.shape[0])])


# ====================================================================================================== encoders: images -> latents
def s2d_weights(wt: torch.Tensor, cip: int, cop: int) -> torch.Tensor:
    """[Cout, Cin, 3, 3] kernel of the stride-2 convolution on pad(x, (0, 1, 0, 1)) -> [cop, 9 * 4 * cip] bf16: the stride-1 3x3 kernel on the
    space-to-depth grid (cell (Y, X), channel (2 py + px) * cip + c = x[2Y + py][2X + px][c]) that afx_conv3x3s2_bf16 runs.  Source row
    2y + dy is phase dy of cell y for dy = 0, 1 and phase 0 of cell y + 1 for dy = 2 (the same in x), so the taps -1 and the phase-1 blocks of
    the taps +1 stay zero: 9 of the 36 (tap, phase) blocks are live."""
    co, ci = wt.shape[:2]
    cell = {0: (1, 0), 1: (1, 1), 2: (2, 0)}                       # kernel index -> (tap index of the 3x3 kernel on cells, phase)
    out = torch.zeros(cop, 3, 3, 4, cip, dtype=wt.dtype)
    for dy in range(3):
        for dx in range(3):
            (ty, py), (tx, px) = cell[dy], cell[dx]
            out[:co, ty, tx, 2 * py + px, :ci] = wt[:, :, dy, dx]
    return out.reshape(cop, 36 * cip)


def conv_in_weights(wt: torch.Tensor, b: torch.Tensor, cop: int) -> torch.Tensor:
    """[Cout, 3, 3, 3] kernel + bias of conv_in (padding 1) -> [cop, 64]: the matrix applied to the rows of afx_image_to_cols27
    (column (3 dy + dx) * 3 + channel, the bias in column 27, which multiplies that layout's constant 1)."""
    co = wt.shape[0]
    out = torch.zeros(cop, 64, dtype=wt.dtype)
    out[:co, :27] = wt.permute(0, 2, 3, 1).reshape(co, 27)
    out[:co, 27] = b
    return out


def kl_encoder_shapes(block_out_channels: Sequence[int] = (128, 256, 512, 512), layers_per_block: int = 2, latent_channels: int = 16,
                      in_channels: int = 3) -> Dict[str, tuple]:
    """State-dict keys and shapes of the diffusers AutoencoderKL encoder (double_z, mid-block attention, no quant_conv)."""
    sh: Dict[str, tuple] = {}

    def conv(n, co, ci, k=3):
        sh[n + '.weight'], sh[n + '.bias'] = (co, ci, k, k), (co,)

    def norm(n, c):
        sh[n + '.weight'], sh[n + '.bias'] = (c,), (c,)

    def res(p, ci, co):
        norm(p + 'norm1', ci); conv(p + 'conv1', co, ci); norm(p + 'norm2', co); conv(p + 'conv2', co, co)
        if ci != co:
            conv(p + 'conv_shortcut', co, ci, 1)
    c = block_out_channels[0]
    conv('encoder.conv_in', c, in_channels)
    for i, co in enumerate(block_out_channels):
        for j in range(layers_per_block):
            res(f'encoder.down_blocks.{i}.resnets.{j}.', c, co)
            c = co
        if i < len(block_out_channels) - 1:
            conv(f'encoder.down_blocks.{i}.downsamplers.0.conv', c, c)
    res('encoder.mid_block.resnets.0.', c, c)
    a = 'encoder.mid_block.attentions.0.'
    norm(a + 'group_norm', c)
    for n in ('to_q', 'to_k', 'to_v', 'to_out.0'):
        sh[a + n + '.weight'], sh[a + n + '.bias'] = (c, c), (c,)
    res('encoder.mid_block.resnets.1.', c, c)
    norm('encoder.conv_norm_out', c)
    conv('encoder.conv_out', 2 * latent_channels, c)
    return sh


def qwen_encoder_shapes(dim: int = 96, z_dim: int = 16, dim_mult: Sequence[int] = (1, 2, 4, 4), num_res_blocks: int = 2,
                        temporal_downsample: Sequence[bool] = (False, True, True)) -> Dict[str, tuple]:
    """State-dict keys and shapes of the diffusers AutoencoderKLQwenImage encoder + quant_conv (down_blocks is one flat list of residual blocks and
    Resample modules)."""
    sh: Dict[str, tuple] = {}

    def conv3(n, co, ci, k):
        sh[n + '.weight'], sh[n + '.bias'] = (co, ci, k, k, k), (co,)

    def res(p, ci, co):
        sh[p + 'norm1.gamma'] = (ci, 1, 1, 1); conv3(p + 'conv1', co, ci, 3)
        sh[p + 'norm2.gamma'] = (co, 1, 1, 1); conv3(p + 'conv2', co, co, 3)
        if ci != co:
            conv3(p + 'conv_shortcut', co, ci, 1)
    dims = [dim * u for u in [1] + list(dim_mult)]
    conv3('encoder.conv_in', dims[0], 3, 3)
    n = 0
    for i, (ci, co) in enumerate(zip(dims[:-1], dims[1:])):
        for _ in range(num_res_blocks):
            res(f'encoder.down_blocks.{n}.', ci, co)
            ci = co
            n += 1
        if i != len(dim_mult) - 1:
            sh[f'encoder.down_blocks.{n}.resample.1.weight'], sh[f'encoder.down_blocks.{n}.resample.1.bias'] = (co, co, 3, 3), (co,)
            if temporal_downsample[i]:
                sh[f'encoder.down_blocks.{n}.time_conv.weight'], sh[f'encoder.down_blocks.{n}.time_conv.bias'] = (co, co, 3, 1, 1), (co,)
            n += 1
    c = dims[-1]
    res('encoder.mid_block.resnets.0.', c, c)
    a = 'encoder.mid_block.attentions.0.'
    sh[a + 'norm.gamma'] = (c, 1, 1)
    sh[a + 'to_qkv.weight'], sh[a + 'to_qkv.bias'] = (3 * c, c, 1, 1), (3 * c,)
    sh[a + 'proj.weight'], sh[a + 'proj.bias'] = (c, c, 1, 1), (c,)
    res('encoder.mid_block.resnets.1.', c, c)
    sh['encoder.norm_out.gamma'] = (c, 1, 1, 1)
    conv3('encoder.conv_out', 2 * z_dim, c, 3)
    conv3('quant_conv', 2 * z_dim, 2 * z_dim, 1)
    return sh


def _check_keys(state_dict, expected: Dict[str, tuple], prefixes, what: str):
    """Every expected key present with its shape, and no other key under the encoder's prefixes: nothing is skipped silently."""
    have = {k for k in state_dict if k.startswith(tuple(prefixes))}
    missing, extra = sorted(set(expected) - have), sorted(have - set(expected))
    bad = [f'{k}: {tuple(state_dict[k].shape)} != {expected[k]}' for k in sorted(have & set(expected)) if tuple(state_dict[k].shape) != tuple(expected[k])]
    if missing or extra or bad:
        raise KeyError(f'{what}: missing keys {missing[:8]}{" ..." if len(missing) > 8 else ""}, unknown keys {extra[:8]}'
                       f'{" ..." if len(extra) > 8 else ""}, wrong shapes {bad[:8]}')


class _EncodeMixin:
    """The public side both encoders share: batching, the noise, the posterior kernel."""

    def encode(self, images: torch.Tensor, generator=None, noise: torch.Tensor = None, sample: bool = True, packed: bool = False,
               return_moments: bool = False, images01: bool = False):
        """images [B, 3, H, W] fp32 / bf16 in [-1, 1] as the reference passes them to vae.encode (images01: in [0, 1], the ``* 2 - 1`` of
        latent_diffusion_text_image.py:43 is applied by the kernel); H, W multiples of 16.  Returns the latents the reference wrappers return
        (pretrained.py:67 / :140): fp32 [B, 16, H/8, W/8], or packed [B, (H/16)(W/16), 64] tokens, so ``decoder.decode_packed(encoder.encode(x,
        packed=True), H // 16, W // 16)`` is the round trip.  sample: z = mean + std * noise with ``noise`` [B, 16, H/8, W/8] (drawn from
        ``generator`` when not given); sample=False: the mode.  return_moments: also the fp32 moments [B, 32, H/8, W/8] (mean | clamped logvar)."""
        if images.dim() != 4 or images.shape[1] != 3 or images.shape[2] % 16 or images.shape[3] % 16:
            raise ValueError(f'encode: need images [B, 3, H, W] with H, W multiples of 16, got {tuple(images.shape)}')
        B, _, H, W = images.shape
        h, w = H // 8, W // 8
        if images.dtype != torch.bfloat16:
            images = images.to(torch.float32)
        images = images.to(self.dev).contiguous()
        if sample:
            if noise is None:
                gdev = self.dev if generator is None else generator.device
                noise = torch.randn(B, 16, h, w, generator=generator, device=gdev, dtype=torch.float32)
            if tuple(noise.shape) != (B, 16, h, w):
                raise ValueError(f'encode: noise must be {(B, 16, h, w)}, got {tuple(noise.shape)}')
            noise = noise.to(self.dev, torch.float32).contiguous()
        out = torch.empty((B, (h // 2) * (w // 2), 64) if packed else (B, 16, h, w), dtype=torch.float32, device=self.dev)
        mom = torch.empty(B, 32, h, w, dtype=torch.float32, device=self.dev)
        for i in range(B):
            g = self._moments_grid(images[i], images01)
            _lib.check(self.lib.afx_posterior_latents(_p(g.t), g.C, h, w, _p(self._qA), _p(self._qb), _p(noise[i]) if sample else None, _p(self._sub),
                                                      _p(self._fac), self._divide, _p(out[i]), int(packed), _p(mom[i]), _s()))
        return (out, mom) if return_moments else out

    def encode_images01(self, images: torch.Tensor, **kw):
        """``encode`` of images in [0, 1] (the ``images`` branch of a training batch, latent_diffusion_text_image.py:34-45)."""
        return self.encode(images, images01=True, **kw)

    def _first_grid(self, img: torch.Tensor, images01: bool, name: str) -> _Grid:
        """conv_in: the 27-in-64 neighbourhood rows, then a K = 64 GEMM (3 channels padded to 64 for the 3x3 kernel would be 21x the work)."""
        H, W = img.shape[1:]
        cols = self._pool.grid(H, W, 64)
        _lib.check(self.lib.afx_image_to_cols27(_p(img), int(img.dtype == torch.bfloat16), _p(cols.t), H, W, int(images01), _s()))
        w = self.w[name + '.weight']
        x = self._pool.grid(H, W, w.shape[0])
        ops.linear(cols.t, w, None, out=x.t)
        return x

    def _down(self, name: str, x: _Grid, stats) -> _Grid:
        w, b = self.w[name + '.weight'], self.w[name + '.bias']
        ws = self._pool.grid(x.H // 2, x.W // 2, 4 * x.C)
        y = self._pool.grid(x.H // 2, x.W // 2, w.shape[0])
        y.stats = stats
        _lib.check(self.lib.afx_conv3x3s2_bf16(_p(x.t), _p(w), _p(b), _p(y.t), _p(ws.t), x.H, x.W, x.C, w.shape[0], _p(stats),
                                               self.groups if stats is not None else 0, _s()))
        return y


class AutoencoderKLEncoder(_KLBlocks, _EncodeMixin):
    """Encoder of the diffusers AutoencoderKL (FLUX: block_out_channels (128, 256, 512, 512), 2 layers per block, 32 groups, 16 latent channels,
    double_z, no quant_conv) on the decoder's kernels -- the ``vae.encode(img).latent_dist.sample()`` behind
    lakonlab/models/architecture/diffusers/pretrained.py:60-67.  conv_in is a K = 64 GEMM on 27-value neighbourhood rows, the three
    Downsample2D(padding=0) layers are afx_conv3x3s2_bf16, the posterior (clamp, exp, noise, shift / scale, packing) is one fp32 kernel."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], block_out_channels: Sequence[int] = (128, 256, 512, 512),
                 norm_num_groups: int = 32, layers_per_block: int = 2, scaling_factor: float = 0.3611,
                 shift_factor: float = 0.1159, device='cuda'):
        _check_keys(state_dict, kl_encoder_shapes(block_out_channels, layers_per_block), ('encoder.', 'quant_conv.'), 'AutoencoderKLEncoder')
        self._setup(state_dict, 'encoder.', norm_num_groups, device)
        self.chans, self.lpb = list(block_out_channels), layers_per_block
        self.scaling_factor = 1.0 if scaling_factor is None else scaling_factor
        self.shift_factor = 0.0 if shift_factor is None else shift_factor
        self.config = type('cfg', (), dict(scaling_factor=scaling_factor, shift_factor=shift_factor))()
        self._qA = self._qb = None
        self._sub = torch.full((16,), float(self.shift_factor), dtype=torch.float32, device=self.dev)
        self._fac = torch.full((16,), float(self.scaling_factor), dtype=torch.float32, device=self.dev)
        self._divide = 0

    def _relay(self, name, wt, b):
        if name == 'encoder.conv_in':
            self.w[name + '.weight'] = conv_in_weights(wt.float(), b.float(), (wt.shape[0] + 7) // 8 * 8).to(self.dev, torch.bfloat16)
        elif '.downsamplers.0.conv' in name:
            co, ci = wt.shape[:2]
            self.w[name + '.weight'] = s2d_weights(wt.float(), _c64(ci), (co + 7) // 8 * 8).to(self.dev, torch.bfloat16)
            bp = torch.zeros((co + 7) // 8 * 8, dtype=torch.bfloat16)
            bp[:co] = b.to(torch.bfloat16)
            self.w[name + '.bias'] = bp.to(self.dev)
        else:
            return False
        return True

    @torch.no_grad()
    def _moments_grid(self, img: torch.Tensor, images01: bool) -> _Grid:
        x = self._first_grid(img, images01, 'encoder.conv_in')
        n = len(self.chans)
        for i in range(n):
            for j in range(self.lpb):
                x = self._resnet(f'encoder.down_blocks.{i}.resnets.{j}.', x)
            if i < n - 1:
                x = self._down(f'encoder.down_blocks.{i}.downsamplers.0.conv', x, self._stat_slot(x.C))
        x = self._resnet('encoder.mid_block.resnets.0.', x)
        x = self._attention('encoder.mid_block.attentions.0.', x)
        x = self._resnet('encoder.mid_block.resnets.1.', x)
        return self._conv('encoder.conv_out', self._gn('encoder.conv_norm_out', x, True), 0, stats=False)


class AutoencoderKLQwenImageEncoder(_QwenBlocks, _EncodeMixin):
    """Encoder of AutoencoderKLQwenImage for single images -- ``vae.encode(img.unsqueeze(-3)).latent_dist.sample()`` normalised by latents_mean /
    latents_std (lakonlab/models/architecture/diffusers/pretrained.py:133-140).  Two reductions hold on ONE frame and are checked against a real
    conv3d on the one-frame clip by the test oracle: (1) every causal 3x3x3 convolution pads two zero frames in front, so it reduces to its LAST
    temporal tap as a 2-D kernel (as in the decoder); (2) the temporal ``time_conv`` of the ``downsample3d`` stages never runs: the first chunk only
    fills its cache, so those stages are the spatial Resample alone (pad (0, 1, 0, 1) + stride-2 Conv2d).  The 1x1x1 ``quant_conv`` is applied in
    fp32 by the posterior kernel; the 96-channel stage runs on grids padded to 128."""
    groups = 0

    def __init__(self, state_dict: Dict[str, torch.Tensor], latents_mean: Sequence[float], latents_std: Sequence[float], dim: int = None,
                 dim_mult: Sequence[int] = (1, 2, 4, 4), num_res_blocks: int = 2, temporal_downsample: Sequence[bool] = (False, True, True),
                 z_dim: int = 16, device='cuda'):
        assert z_dim == 16, 'the packed-latent layout of the pipelines has 16 latent channels'
        if dim is None:
            dim = state_dict['encoder.conv_in.weight'].shape[0]
        _check_keys(state_dict, qwen_encoder_shapes(dim, z_dim, dim_mult, num_res_blocks, temporal_downsample), ('encoder.', 'quant_conv.'),
                    'AutoencoderKLQwenImageEncoder')
        sd = self._setup(state_dict, 'encoder.', {'encoder.conv_out': 2 * z_dim}, device)
        self.n_down, self.nrb = len(dim_mult), num_res_blocks
        self.latents_mean, self.latents_std = list(latents_mean), list(latents_std)
        self.config = type('cfg', (), dict(latents_mean=self.latents_mean, latents_std=self.latents_std, z_dim=z_dim))()
        self._qA = sd['quant_conv.weight'].float().reshape(32, 32).contiguous().to(self.dev)
        self._qb = sd['quant_conv.bias'].float().contiguous().to(self.dev)
        self._sub = torch.tensor(self.latents_mean, dtype=torch.float32, device=self.dev)
        self._fac = torch.tensor(self.latents_std, dtype=torch.float32, device=self.dev)
        self._divide = 1

    def _relay(self, name, wt, b, cop):
        if name == 'encoder.conv_in':
            self.w[name + '.weight'] = conv_in_weights(wt, b, cop).to(self.dev, torch.bfloat16)
        elif name.endswith('.resample.1'):
            self.w[name + '.weight'] = s2d_weights(wt, _c64(wt.shape[1]), cop).to(self.dev, torch.bfloat16)
            bp = torch.zeros(cop, dtype=torch.bfloat16)
            bp[:wt.shape[0]] = b.to(torch.bfloat16)
            self.w[name + '.bias'] = bp.to(self.dev)
        else:
            return False
        return True

    @torch.no_grad()
    def _moments_grid(self, img: torch.Tensor, images01: bool) -> _Grid:
        x = self._first_grid(img, images01, 'encoder.conv_in')
        n = 0
        for i in range(self.n_down):
            for _ in range(self.nrb):
                x = self._resnet(f'encoder.down_blocks.{n}.', x)
                n += 1
            if i != self.n_down - 1:
                x = self._down(f'encoder.down_blocks.{n}.resample.1', x, None)
                n += 1
        x = self._resnet('encoder.mid_block.resnets.0.', x)
        x = self._mid_attention('encoder.mid_block.attentions.0.', x)
        x = self._resnet('encoder.mid_block.resnets.1.', x)
        return self._conv('encoder.conv_out', self._norm('encoder.norm_out', x, True))
