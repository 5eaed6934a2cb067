"""fp32 torch oracle of the two VAE *encoders* (test helper, not a test module).

Restates the published diffusers 0.35.1 algorithm from its layer list (the reference imports the classes from diffusers, which is not
installed here): AutoencoderKL's Encoder (conv_in -> 4 x DownEncoderBlock2D (2 ResnetBlock2D, Downsample2D(padding=0) = pad (0,1,0,1) +
stride-2 conv on the first three) -> UNetMidBlock2D -> GroupNorm -> SiLU -> conv_out, double_z) and AutoencoderKLQwenImage's encoder on a
one-frame clip (causal conv3d everywhere, RMS norm over channels, Resample = ZeroPad2d((0,1,0,1)) + stride-2 Conv2d; the temporal time_conv of
the downsample3d stages only fills its cache on the first chunk), then quant_conv.  The Qwen path evaluates real conv3d on the 5-D weights with
two zero frames padded in front, so the engine's "last temporal tap" reduction is checked, not assumed.

Parity status: **parity unpinned** for the wiring (tests/test_vae_encoder_thirdparty.py pins it where diffusers is installed); the arithmetic
of every op is torch's.  ``bf16=True`` rounds every op's output to bf16 (what an eager bf16 run of the same graph would hold in memory).
"""
from __future__ import annotations

from typing import Dict, Sequence

import torch
import torch.nn.functional as F

Tensor = torch.Tensor


class _R:
    """Rounds op outputs to bf16 when on (the eager-bf16 comparator), identity otherwise."""

    def __init__(self, on: bool):
        self.on = on

    def __call__(self, x: Tensor) -> Tensor:
        return x.bfloat16().float() if self.on else x


# ------------------------------------------------------------------------------------------------------------- AutoencoderKL (FLUX)
def _gn(w, n, x, groups, r):
    return r(F.group_norm(x, groups, w[n + '.weight'].float(), w[n + '.bias'].float(), 1e-6))


def _conv(w, n, x, r, pad=1):
    return r(F.conv2d(x, w[n + '.weight'].float(), w[n + '.bias'].float(), padding=pad))


def _resnet(w, p, x, groups, r):
    h = _conv(w, p + 'conv1', r(F.silu(_gn(w, p + 'norm1', x, groups, r))), r)
    h = _conv(w, p + 'conv2', r(F.silu(_gn(w, p + 'norm2', h, groups, r))), r)
    if p + 'conv_shortcut.weight' in w:
        x = _conv(w, p + 'conv_shortcut', x, r, pad=0)
    return r(x + h)


def _mid_attention(w, p, x, groups, r):
    b, c, hh, ww = x.shape
    t = _gn(w, p + 'group_norm', x, groups, r).reshape(b, c, hh * ww).transpose(1, 2)
    q, k, v = (r(F.linear(t, w[p + n + '.weight'].float(), w[p + n + '.bias'].float())) for n in ('to_q', 'to_k', 'to_v'))
    a = r(F.scaled_dot_product_attention(q[:, None], k[:, None], v[:, None])[:, 0])
    o = r(F.linear(a, w[p + 'to_out.0.weight'].float(), w[p + 'to_out.0.bias'].float()))
    return r(x + o.transpose(1, 2).reshape(b, c, hh, ww))


def downsample(x: Tensor, wt: Tensor, b: Tensor) -> Tensor:
    """diffusers Downsample2D(padding=0) / Qwen Resample('downsample2d'): zero-pad right and bottom by one, 3x3, stride 2."""
    return F.conv2d(F.pad(x, (0, 1, 0, 1)), wt, b, stride=2)


def flux_moments(w: Dict[str, Tensor], img: Tensor, chans: Sequence[int] = (128, 256, 512, 512), groups: int = 32, layers_per_block: int = 2,
                 bf16: bool = False) -> Tensor:
    """img [B, 3, H, W] in [-1, 1] -> moments [B, 32, H/8, W/8] (mean | logvar, not clamped)."""
    r = _R(bf16)
    x = _conv(w, 'encoder.conv_in', img.float(), r)
    n = len(chans)
    for i in range(n):
        for j in range(layers_per_block):
            x = _resnet(w, f'encoder.down_blocks.{i}.resnets.{j}.', x, groups, r)
        if i < n - 1:
            p = f'encoder.down_blocks.{i}.downsamplers.0.conv'
            x = r(downsample(x, w[p + '.weight'].float(), w[p + '.bias'].float()))
    x = _resnet(w, 'encoder.mid_block.resnets.0.', x, groups, r)
    x = _mid_attention(w, 'encoder.mid_block.attentions.0.', x, groups, r)
    x = _resnet(w, 'encoder.mid_block.resnets.1.', x, groups, r)
    return _conv(w, 'encoder.conv_out', r(F.silu(_gn(w, 'encoder.conv_norm_out', x, groups, r))), r)


def posterior(moments: Tensor, eps: Tensor = None) -> Tensor:
    """DiagonalGaussianDistribution: sample (eps given) or mode."""
    mean, logvar = moments.chunk(2, dim=1)
    logvar = logvar.clamp(-30.0, 20.0)
    return mean if eps is None else mean + torch.exp(0.5 * logvar) * eps


def encode_flux(w, img, chans=(128, 256, 512, 512), groups=32, eps=None, scaling_factor=0.3611, shift_factor=0.1159, bf16=False) -> Tensor:
    """pretrained.py:60-67: (vae.encode(img).latent_dist.sample() - shift) * scale -> [B, 16, H/8, W/8]."""
    return (posterior(flux_moments(w, img, chans, groups, bf16=bf16), eps) - shift_factor) * scaling_factor


def make_encoder_weights(chans=(128, 256, 512, 512), latent_channels=16, layers_per_block=2, seed=0, dtype=torch.bfloat16) -> Dict[str, Tensor]:
    """Random weights with the key names / shapes of diffusers' AutoencoderKL encoder (scaled as oracle/vae_ref.make_decoder_weights)."""
    g = torch.Generator().manual_seed(seed)
    w: Dict[str, Tensor] = {}

    def conv(name, co, ci, k=3):
        w[name + '.weight'] = (torch.randn(co, ci, k, k, generator=g) * (1.2 / (ci * k * k) ** 0.5)).to(dtype)
        w[name + '.bias'] = (torch.randn(co, generator=g) * 0.05).to(dtype)

    def norm(name, c):
        w[name + '.weight'] = (1 + 0.1 * torch.randn(c, generator=g)).to(dtype)
        w[name + '.bias'] = (0.1 * torch.randn(c, generator=g)).to(dtype)

    def res(p, ci, co):
        norm(p + 'norm1', ci); conv(p + 'conv1', co, ci); norm(p + 'norm2', co); conv(p + 'conv2', co, co)
        if ci != co:
            conv(p + 'conv_shortcut', co, ci, 1)
    c = chans[0]
    conv('encoder.conv_in', c, 3)
    for i, co in enumerate(chans):
        for j in range(layers_per_block):
            res(f'encoder.down_blocks.{i}.resnets.{j}.', c, co)
            c = co
        if i < len(chans) - 1:
            conv(f'encoder.down_blocks.{i}.downsamplers.0.conv', c, c)
    res('encoder.mid_block.resnets.0.', c, c)
    p = 'encoder.mid_block.attentions.0.'
    norm(p + 'group_norm', c)
    for nm in ('to_q', 'to_k', 'to_v', 'to_out.0'):
        w[p + nm + '.weight'] = (torch.randn(c, c, generator=g) * (1.0 / c ** 0.5)).to(dtype)
        w[p + nm + '.bias'] = (torch.randn(c, generator=g) * 0.05).to(dtype)
    res('encoder.mid_block.resnets.1.', c, c)
    norm('encoder.conv_norm_out', c)
    conv('encoder.conv_out', 2 * latent_channels, c)
    return w


# ------------------------------------------------------------------------------------------------------------- AutoencoderKLQwenImage
def _causal_conv3d(w, n, x, r):
    wt = w[n + '.weight'].float()
    kt, kh, kw = wt.shape[2:]
    return r(F.conv3d(F.pad(x, (kw // 2, kw // 2, kh // 2, kh // 2, kt - 1, 0)), wt, w[n + '.bias'].float()))


def _rms(w, n, x, r):
    g = w[n + '.gamma'].float().reshape(1, -1, *([1] * (x.dim() - 2)))
    return r(F.normalize(x, dim=1) * (x.shape[1] ** 0.5) * g)


def _qres(w, p, x, r):
    h = _causal_conv3d(w, p + 'conv_shortcut', x, r) if p + 'conv_shortcut.weight' in w else x
    x = _causal_conv3d(w, p + 'conv1', r(F.silu(_rms(w, p + 'norm1', x, r))), r)
    x = _causal_conv3d(w, p + 'conv2', r(F.silu(_rms(w, p + 'norm2', x, r))), r)
    return r(x + h)


def _qattn(w, p, x, r):
    b, c, t, hh, ww = x.shape
    y = _rms(w, p + 'norm', x.permute(0, 2, 1, 3, 4).reshape(b * t, c, hh, ww), r)
    qkv = r(F.conv2d(y, w[p + 'to_qkv.weight'].float(), w[p + 'to_qkv.bias'].float()))
    q, k, v = qkv.reshape(b * t, 1, c * 3, hh * ww).permute(0, 1, 3, 2).chunk(3, dim=-1)
    a = r(F.scaled_dot_product_attention(q, k, v)).squeeze(1).permute(0, 2, 1).reshape(b * t, c, hh, ww)
    a = r(F.conv2d(a, w[p + 'proj.weight'].float(), w[p + 'proj.bias'].float()))
    return r(x + a.reshape(b, t, c, hh, ww).permute(0, 2, 1, 3, 4))


def qwen_moments(w: Dict[str, Tensor], img: Tensor, dim_mult: Sequence[int] = (1, 2, 4, 4), num_res_blocks: int = 2, bf16: bool = False) -> Tensor:
    """img [B, 3, H, W] in [-1, 1] -> moments [B, 32, H/8, W/8] of the one-frame clip img[:, :, None] (quant_conv applied, logvar not clamped)."""
    r = _R(bf16)
    x = _causal_conv3d(w, 'encoder.conv_in', img.float()[:, :, None], r)
    n = 0
    for i in range(len(dim_mult)):
        for _ in range(num_res_blocks):
            x = _qres(w, f'encoder.down_blocks.{n}.', x, r)
            n += 1
        if i != len(dim_mult) - 1:
            p = f'encoder.down_blocks.{n}.resample.1'
            b, c, t, hh, ww = x.shape
            y = downsample(x.permute(0, 2, 1, 3, 4).reshape(b * t, c, hh, ww), w[p + '.weight'].float(), w[p + '.bias'].float())
            x = r(y.reshape(b, t, y.shape[1], hh // 2, ww // 2).permute(0, 2, 1, 3, 4))     # (first chunk: time_conv only fills its cache)
            n += 1
    x = _qres(w, 'encoder.mid_block.resnets.0.', x, r)
    x = _qattn(w, 'encoder.mid_block.attentions.0.', x, r)
    x = _qres(w, 'encoder.mid_block.resnets.1.', x, r)
    x = _causal_conv3d(w, 'encoder.conv_out', r(F.silu(_rms(w, 'encoder.norm_out', x, r))), r)
    return _causal_conv3d(w, 'quant_conv', x, _R(False))[:, :, 0]


def encode_qwen(w, img, latents_mean, latents_std, eps=None, bf16=False) -> Tensor:
    """pretrained.py:133-140: (vae.encode(clip).latent_dist.sample() - latents_mean) / latents_std -> [B, 16, H/8, W/8]."""
    z = posterior(qwen_moments(w, img, bf16=bf16), eps)
    m = torch.as_tensor(latents_mean, dtype=z.dtype, device=z.device).view(1, 16, 1, 1)
    s = torch.as_tensor(latents_std, dtype=z.dtype, device=z.device).view(1, 16, 1, 1)
    return (z - m) / s


def make_qwen_encoder_weights(dim: int = 96, z_dim: int = 16, dim_mult: Sequence[int] = (1, 2, 4, 4), num_res_blocks: int = 2,
                              temporal_downsample: Sequence[bool] = (False, True, True), seed: int = 0, std: float = 0.03) -> Dict[str, Tensor]:
    """Random weights with the key names / shapes of diffusers' AutoencoderKLQwenImage encoder + quant_conv (scaled as
    oracle/vae_qwen_ref.make_decoder_weights; every temporal tap is non-zero, so a wrong tap would show)."""
    g = torch.Generator().manual_seed(seed)
    w: Dict[str, Tensor] = {}

    def conv3(name, co, ci, k, s=None):
        w[name + '.weight'] = torch.randn(co, ci, k, k, k, generator=g) * (s if s is not None else (std if k == 3 else std * 3))
        w[name + '.bias'] = torch.randn(co, generator=g) * 0.02

    def res(p, ci, co):
        w[p + 'norm1.gamma'] = 1.0 + 0.1 * torch.randn(ci, 1, 1, 1, generator=g); conv3(p + 'conv1', co, ci, 3)
        w[p + 'norm2.gamma'] = 1.0 + 0.1 * torch.randn(co, 1, 1, 1, generator=g); conv3(p + 'conv2', co, co, 3)
        if ci != co:
            conv3(p + 'conv_shortcut', co, ci, 1)
    dims = [dim * u for u in [1] + list(dim_mult)]
    conv3('encoder.conv_in', dims[0], 3, 3, 0.2)
    n = 0
    for i, (ci, co) in enumerate(zip(dims[:-1], dims[1:])):
        for _ in range(num_res_blocks):
            res(f'encoder.down_blocks.{n}.', ci, co)
            ci = co
            n += 1
        if i != len(dim_mult) - 1:
            p = f'encoder.down_blocks.{n}.'
            w[p + 'resample.1.weight'] = torch.randn(co, co, 3, 3, generator=g) * std
            w[p + 'resample.1.bias'] = torch.randn(co, generator=g) * 0.02
            if temporal_downsample[i]:
                w[p + 'time_conv.weight'] = torch.randn(co, co, 3, 1, 1, generator=g) * std
                w[p + 'time_conv.bias'] = torch.randn(co, generator=g) * 0.02
            n += 1
    c = dims[-1]
    res('encoder.mid_block.resnets.0.', c, c)
    a = 'encoder.mid_block.attentions.0.'
    w[a + 'norm.gamma'] = 1.0 + 0.1 * torch.randn(c, 1, 1, generator=g)
    for nm, co in (('to_qkv', 3 * c), ('proj', c)):
        w[a + nm + '.weight'] = torch.randn(co, c, 1, 1, generator=g) * std * 2
        w[a + nm + '.bias'] = torch.randn(co, generator=g) * 0.02
    res('encoder.mid_block.resnets.1.', c, c)
    w['encoder.norm_out.gamma'] = 1.0 + 0.1 * torch.randn(c, 1, 1, 1, generator=g)
    conv3('encoder.conv_out', 2 * z_dim, c, 3)
    conv3('quant_conv', 2 * z_dim, 2 * z_dim, 1, 0.2)
    return w
