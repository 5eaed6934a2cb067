"""Third-party pin of the encoder oracle's WIRING (tests/vae_encoder_ref.py restates diffusers' encoders from their published layer list):
diffusers' own AutoencoderKL / AutoencoderKLQwenImage with random weights against the oracle's moments, fp32 on the CPU, <= 2e-5.

diffusers is not installed on the development image or on the GPU pool, so these tests SKIP there (like tests/test_thirdparty_crosscheck.py);
they run wherever `pip install diffusers==0.35.1` is possible and pin the "parity unpinned" row of DESIGN.md section 2."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vae_encoder_ref as E  # noqa: E402


def test_flux_encoder_oracle_vs_diffusers():
    diffusers = pytest.importorskip('diffusers')
    chans = (32, 64, 64, 64)
    vae = diffusers.AutoencoderKL(in_channels=3, out_channels=3, down_block_types=('DownEncoderBlock2D',) * 4, up_block_types=('UpDecoderBlock2D',) * 4,
                                  block_out_channels=chans, layers_per_block=2, latent_channels=16, norm_num_groups=8, use_quant_conv=False,
                                  use_post_quant_conv=False, mid_block_add_attention=True).eval()
    w = {k: v.float() for k, v in E.make_encoder_weights(chans, seed=1, dtype=torch.float32).items()}
    missing, unexpected = vae.load_state_dict(w, strict=False)
    assert not unexpected and all(k.startswith('decoder.') for k in missing)
    img = torch.rand(1, 3, 32, 48, generator=torch.Generator().manual_seed(2)) * 2 - 1
    with torch.no_grad():
        ref = vae.encode(img).latent_dist.parameters
    got = E.flux_moments(w, img, chans, 8)
    assert (got - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())


def test_qwen_encoder_oracle_vs_diffusers():
    diffusers = pytest.importorskip('diffusers')
    cls = getattr(diffusers, 'AutoencoderKLQwenImage', None)
    if cls is None:
        pytest.skip('this diffusers has no AutoencoderKLQwenImage')
    vae = cls(base_dim=16, z_dim=16, dim_mult=[1, 2, 4, 4], num_res_blocks=2, attn_scales=[], temperal_downsample=[False, True, True]).eval()
    w = E.make_qwen_encoder_weights(dim=16, seed=1)
    missing, unexpected = vae.load_state_dict(w, strict=False)
    assert not unexpected and all(k.startswith(('decoder.', 'post_quant_conv.')) for k in missing)
    img = torch.rand(1, 3, 32, 48, generator=torch.Generator().manual_seed(2)) * 2 - 1
    with torch.no_grad():
        ref = vae.encode(img[:, :, None]).latent_dist.parameters[:, :, 0]
    got = E.qwen_moments(w, img)
    assert (got - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())
