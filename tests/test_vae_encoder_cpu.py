"""Host side of the VAE encoders, no GPU: the weight re-layouts, the one-frame reductions of the Qwen-Image encoder, the latent cache tool and
the C header."""
import os
import pickle
import re
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vae_encoder_ref as E  # noqa: E402


@pytest.mark.parametrize('H,W,ci,co,cip,cop', [(6, 10, 5, 7, 5, 8), (8, 4, 3, 4, 8, 8)])
def test_s2d_weights_equal_stride2_conv(H, W, ci, co, cip, cop):
    """The stride-1 3x3 convolution on the space-to-depth grid with s2d_weights == F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2), fp64 to 1e-12
    (padded channels / outputs stay zero)."""
    from arcflow_amd.vae import s2d_weights
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, ci, H, W, generator=g, dtype=torch.float64)
    wt = torch.randn(co, ci, 3, 3, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.pad(x, (0, 1, 0, 1)), wt, stride=2)
    xp = F.pad(x, (0, 0, 0, 0, 0, cip - ci))
    s = xp.reshape(1, cip, H // 2, 2, W // 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(1, 4 * cip, H // 2, W // 2)     # channel (2 py + px) * cip + c
    w36 = s2d_weights(wt, cip, cop).reshape(cop, 3, 3, 4 * cip).permute(0, 3, 1, 2)
    got = F.conv2d(s, w36, padding=1)
    assert (got[:, :co] - ref).abs().max().item() < 1e-12
    assert got[:, co:].abs().max().item() == 0
    live = (s2d_weights(torch.ones(1, 1, 3, 3), 1, 1).reshape(9, 4) != 0).sum().item()
    assert live == 9


def test_conv_in_weights_equal_conv():
    """The 27-in-64 neighbourhood rows times conv_in_weights == F.conv2d(img, w, b, padding=1), fp64 to 1e-12."""
    from arcflow_amd.vae import conv_in_weights
    g = torch.Generator().manual_seed(1)
    H, W, co = 5, 7, 6
    img = torch.randn(1, 3, H, W, generator=g, dtype=torch.float64)
    wt, b = torch.randn(co, 3, 3, 3, generator=g, dtype=torch.float64), torch.randn(co, generator=g, dtype=torch.float64)
    xp = F.pad(img, (1, 1, 1, 1))[0]
    cols = torch.zeros(H, W, 64, dtype=torch.float64)
    for dy in range(3):
        for dx in range(3):
            for c in range(3):
                cols[:, :, (3 * dy + dx) * 3 + c] = xp[c, dy:dy + H, dx:dx + W]
    cols[:, :, 27] = 1
    got = (cols @ conv_in_weights(wt, b, 8).T).permute(2, 0, 1)
    assert (got[:co] - F.conv2d(img, wt, b, padding=1)[0]).abs().max().item() < 1e-12 and got[co:].abs().max().item() == 0


def test_qwen_one_frame_reductions_vs_conv3d():
    """On a one-frame clip (two zero frames padded in front) a causal 3x3x3 convolution equals its last temporal tap as a 2-D kernel, and the whole
    encoder oracle (real conv3d) equals the same network evaluated with 2-D last-tap kernels; time_conv weights are never read."""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 4, 6, 8, generator=g, dtype=torch.float64)
    wt, b = torch.randn(5, 4, 3, 3, 3, generator=g, dtype=torch.float64), torch.randn(5, generator=g, dtype=torch.float64)
    ref = F.conv3d(F.pad(x[:, :, None], (1, 1, 1, 1, 2, 0)), wt, b)[:, :, 0]
    assert (F.conv2d(x, wt[:, :, -1], b, padding=1) - ref).abs().max().item() < 1e-12
    w = E.make_qwen_encoder_weights(dim=8, seed=3)
    img = torch.rand(1, 3, 16, 16, generator=g) * 2 - 1
    w2 = {}
    for k, v in w.items():
        if 'time_conv' in k:
            continue
        w2[k] = v[:, :, -1:].clone() if (v.dim() == 5 and v.shape[2] == 3) else v
    a = E.qwen_moments({k: v.float() for k, v in w.items() if 'time_conv' not in k}, img.float())
    b2 = E.qwen_moments({k: v.float() for k, v in w2.items()}, img.float())
    assert a.shape == (1, 32, 2, 2) and (a - b2).abs().max().item() < 1e-5 * a.abs().max().item()


def test_encoder_key_lists_match_the_oracle_weights():
    from arcflow_amd.vae import kl_encoder_shapes, qwen_encoder_shapes
    w = E.make_encoder_weights((64, 128, 128, 128))
    assert {k: tuple(v.shape) for k, v in w.items()} == kl_encoder_shapes((64, 128, 128, 128))
    for dim in (32, 96):
        w = E.make_qwen_encoder_weights(dim=dim)
        assert {k: tuple(v.shape) for k, v in w.items()} == qwen_encoder_shapes(dim)
    assert len(kl_encoder_shapes()) == 106 and kl_encoder_shapes()['encoder.conv_out.weight'] == (32, 512, 3, 3)


def test_cache_latents_round_trip(tmp_path):
    """tools/cache_latents.add_latents writes records PromptEmbedCache(load_latents=True) reads back with identical latents; the default
    arguments return items without the new key."""
    import importlib.util
    import numpy as np
    from PIL import Image
    from arcflow_amd.train.data import PromptEmbedCache
    spec = importlib.util.spec_from_file_location('_cache_latents', os.path.join(ROOT, 'tools', 'cache_latents.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cache, images = tmp_path / 'cache', tmp_path / 'images'
    cache.mkdir(); images.mkdir()
    rng = np.random.RandomState(0)
    for i, (h, w) in enumerate([(32, 48), (37, 64)]):
        item = dict(prompt=f'p{i}', prompt_embed_kwargs=dict(encoder_hidden_states=torch.randn(4, 8).half()), latent_size=(16, 128, 128))
        with open(cache / f'{i:08d}.pkl', 'wb') as f:
            pickle.dump(item, f)
        Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(images / f'{i:08d}.png')
    seen = []

    def fake_encode(im, gen):                       # stands in for the GPU encoder: [1, 3, H, W] in [0, 1] -> [1, 16, H/8, W/8]
        assert im.min() >= 0 and im.max() <= 1 and im.shape[2] % 16 == 0 and im.shape[3] % 16 == 0
        lat = F.avg_pool2d(im, 8).repeat(1, 6, 1, 1)[:, :16] + torch.randn(1, 16, im.shape[2] // 8, im.shape[3] // 8, generator=gen)
        seen.append(lat[0].half())
        return lat
    assert mod.add_latents(fake_encode, str(images), str(cache)) == ['00000000', '00000001']
    plain = PromptEmbedCache(str(cache))
    assert 'latents' not in plain[0] and plain[1]['latent_size'] == (16, 4, 8)
    ds = PromptEmbedCache(str(cache), load_latents=True)
    for i in range(2):
        it = ds[i]
        assert it['latents'].dtype == torch.float32 and torch.equal(it['latents'], seen[i].float()) and it['latent_size'] == tuple(seen[i].shape)
    rec = pickle.load(open(cache / '00000000.pkl', 'rb'))
    rec['latents_scale'] = 2.0
    pickle.dump(rec, open(cache / '00000000.pkl', 'wb'))
    assert torch.equal(ds[0]['latents'], seen[0].float() * 2.0)
    rec.pop('latents'); pickle.dump(rec, open(cache / '00000000.pkl', 'wb'))
    with pytest.raises(KeyError):
        ds[0]


def test_header_declares_every_bound_symbol():
    from arcflow_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'arcflow_hip.h')).read()
    missing = [s for s in _lib.EXPORTS if not re.search(r'\b' + s + r'\s*\(', hdr)]
    assert not missing, missing
    for s in ('afx_conv3x3s2_bf16', 'afx_image_to_cols27', 'afx_posterior_latents'):
        assert s in _lib.EXPORTS
