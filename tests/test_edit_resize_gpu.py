"""``resize=`` and ``mask_blur=`` of both pipelines, on the tiny synthetic engines and VAEs that tests/test_edit_pipeline_gpu.py uses (D = 256,
2 heads, FLUX 1 double + 1 single block, Qwen-Image 1 layer), at 32 x 32 pixels = a 2 x 2 token grid, 2 NFE, ``prompt_embeds`` given.  Every
check is a bit-equality: the resize is ``ops.image_resample`` in front of the existing edit path, an identity table returns the source's
values exactly, and a feathered mask is exactly 0 farther than ceil(3 sigma) from the mask.  On the parent commit every call here fails
(``resize`` / ``mask_blur`` are unknown keywords, ``ops.image_resample`` does not exist)."""
import numpy as np
import pytest
import torch

import vae_encoder_ref as E

pytestmark = pytest.mark.gpu

HP = WP = 2
SIZE = 16 * HP
NFE, RATIO = 2, 1.0


class Setup:
    def __init__(self, family):
        from arcflow_amd import FlowMatchEulerDiscreteScheduler
        from arcflow_amd import vae as VAE
        from arcflow_amd.pipelines import ArcFluxPipeline, ArcQwenImagePipeline
        from oracle import dit_ref as D
        self.family = family
        sch = FlowMatchEulerDiscreteScheduler(shift=3.2)
        g = torch.Generator().manual_seed(2)
        if family == 'flux':
            from oracle import vae_ref as V
            w = D.make_flux_weights(D.FluxCfg(num_layers=1, num_single_layers=1, heads=2, joint_dim=128, pooled_dim=64), seed=9)
            tcfg = dict(num_layers=1, num_single_layers=1, num_attention_heads=2, attention_head_dim=128, in_channels=64, joint_attention_dim=128,
                        pooled_projection_dim=64, guidance_embeds=True)
            self.pipe = ArcFluxPipeline.from_state_dict(tcfg, w, scheduler=sch)
            jd = 128
            chans = (64, 128, 128, 128)
            dec = VAE.AutoencoderKLDecoder(V.make_decoder_weights(chans, seed=4), chans, norm_num_groups=16)
            dec.encoder = VAE.AutoencoderKLEncoder(E.make_encoder_weights(chans, seed=3), chans, norm_num_groups=16)
        else:
            from oracle import vae_qwen_ref as V
            w = D.make_qwen_weights(D.QwenCfg(num_layers=1, heads=2, joint_dim=192), seed=5)
            tcfg = dict(num_layers=1, num_attention_heads=2, attention_head_dim=128, in_channels=64, joint_attention_dim=192)
            self.pipe = ArcQwenImagePipeline.from_state_dict(tcfg, w, scheduler=sch)
            jd = 192
            mean, std = (torch.randn(16, generator=g) * 0.3).tolist(), (1.0 + 0.5 * torch.rand(16, generator=g)).tolist()
            dec = VAE.AutoencoderKLQwenImageDecoder(V.make_decoder_weights(dim=32, seed=3), mean, std)
            dec.encoder = VAE.AutoencoderKLQwenImageEncoder(E.make_qwen_encoder_weights(dim=32, seed=1), mean, std)
        self.pipe.vae = dec
        self.encoder = dec.encoder
        g = torch.Generator().manual_seed(3)
        self.pe = (torch.randn(1, 12, jd, generator=g) * 0.5).bfloat16()
        self.pooled = (torch.randn(1, 64, generator=g) * 0.5).bfloat16()
        self.noise = torch.randn(1, HP * WP, 64, generator=g)
        self.photo = torch.randint(0, 256, (40, 56, 3), generator=g, dtype=torch.uint8).numpy()           # uint8 [H, W, C], no multiple of 16

    def call(self, output_type='latent', **kw):
        kw.setdefault('latents', self.noise.clone())
        kw.setdefault('strength', 0.6)
        if self.family == 'flux':
            cond = dict(prompt_embeds=self.pe, pooled_prompt_embeds=self.pooled)
        else:
            cond = dict(prompt_embeds=self.pe, prompt_embeds_mask=torch.ones(1, 12, dtype=torch.long))
        out = self.pipe(num_inference_steps=NFE, timestep_ratio=RATIO, output_type=output_type, **cond, **kw).images
        torch.cuda.synchronize()
        return out.cpu() if isinstance(out, torch.Tensor) else out


@pytest.fixture(scope='module', params=['flux', 'qwen'])
def S(request):
    return Setup(request.param)


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_stretch_is_image_resample_then_encode(S):
    from arcflow_amd import ops
    small = ops.image_resample(torch.from_numpy(S.photo)[None].cuda(), SIZE, SIZE)
    assert small.shape == (1, 3, SIZE, SIZE) and small.min() >= 0 and small.max() <= 1
    lat = S.encoder.encode_images01(small, sample=False, packed=True)
    want = S.call(image_latents=lat, height=SIZE, width=SIZE)
    got = S.call(image=S.photo, resize='stretch', height=SIZE, width=SIZE)
    assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want))
    from PIL import Image
    assert torch.equal(_bits(S.call(image=Image.fromarray(S.photo), resize='stretch', height=SIZE, width=SIZE)), _bits(want))      # PIL goes the same way
    # the default size: 40 x 56 rounds to 48 x 64 (both ties, up)
    big = S.call(image=S.photo, resize='stretch', latents=None, generator=torch.Generator().manual_seed(1))
    assert big.shape == (1, 3 * 4, 64)
    with pytest.raises(ValueError, match='resizes nothing'):
        S.call(image=torch.rand(1, 3, 48, 64), height=SIZE, width=SIZE)                # without resize: as before


def test_resize_to_the_own_size_is_no_resize(S):
    from PIL import Image
    own = S.photo[:SIZE, :SIZE].copy()
    plain = S.call(image=Image.fromarray(own))                                          # resize=None: the host path, x / 255 in numpy
    for mode in ('stretch', 'crop'):
        assert torch.equal(_bits(S.call(image=own, resize=mode)), _bits(plain)), mode
        assert torch.equal(_bits(S.call(image=Image.fromarray(own), resize=mode, height=SIZE, width=SIZE)), _bits(plain)), mode


def test_crop_at_the_target_aspect_is_stretch(S):
    square = np.ascontiguousarray(S.photo[:, :40])                                      # 40 x 40 -> 32 x 32: the aspect is the target's already
    a = S.call(image=square, resize='stretch', height=SIZE, width=SIZE)
    assert torch.equal(_bits(S.call(image=square, resize='crop', height=SIZE, width=SIZE)), _bits(a))
    # ... and on the 40 x 56 photo it resamples the centred 40 x 40 window (the filter still reads the pixels next to the box, as Pillow's does)
    from arcflow_amd import ops
    boxed = ops.image_resample(torch.from_numpy(S.photo)[None].cuda(), SIZE, SIZE, box=(8.0, 0.0, 48.0, 40.0))
    lat = S.encoder.encode_images01(boxed, sample=False, packed=True)
    assert torch.equal(_bits(S.call(image=S.photo, resize='crop', height=SIZE, width=SIZE)), _bits(S.call(image_latents=lat, height=SIZE, width=SIZE)))
    assert not torch.equal(S.call(image=S.photo, resize='stretch', height=SIZE, width=SIZE), a)


def test_mask_blur_zero_is_absent_and_feathering_keeps_far_pixels(S):
    from arcflow_amd import ops
    mask = torch.zeros(1, 1, SIZE, SIZE)
    mask[..., :8] = 1.0                                                                 # repaint the 8 left columns
    kw = dict(image=S.photo, resize='stretch', height=SIZE, width=SIZE, mask_image=mask)
    hard = S.call(output_type='pt', **kw)
    assert torch.equal(_bits(S.call(output_type='pt', mask_blur=0.0, **kw).float()), _bits(hard.float()))
    plain = torch.from_numpy(S.photo[:SIZE, :SIZE].copy()).permute(2, 0, 1)[None].float() / 255          # mask_blur without resize
    assert torch.equal(_bits(S.call(image=plain, mask_image=mask, mask_blur=0.0)), _bits(S.call(image=plain, mask_image=mask)))
    sigma = 1.0
    r = int(np.ceil(3 * sigma))
    soft = S.call(output_type='pt', mask_blur=sigma, **kw)
    small = ops.image_resample(torch.from_numpy(S.photo)[None].cuda(), SIZE, SIZE).cpu()
    want = (small * 2 - 1).to(soft.dtype)                                               # the composite pastes back the RESIZED original
    far = torch.zeros(1, 3, SIZE, SIZE, dtype=torch.bool)
    far[..., 8 + r:] = True                                                             # farther than ceil(3 sigma) from the mask
    assert soft.shape == (1, 3, SIZE, SIZE) and torch.equal(soft[far], want[far])
    assert torch.equal(hard[..., 8:], want[..., 8:]) and not torch.equal(soft[..., 8:8 + r], want[..., 8:8 + r])      # the feather band is a blend
    # the feathered mask feeds the tokens and the composite alike: passing it in by hand is the same call
    by_hand = S.call(output_type='pt', image=S.photo, resize='stretch', height=SIZE, width=SIZE, mask_image=ops.mask_feather(mask.cuda(), sigma).cpu())
    assert torch.equal(_bits(by_hand.float()), _bits(soft.float()))
    also = S.call(output_type='pt', image=plain, mask_image=mask, mask_blur=sigma)      # resize=None takes mask_blur too
    assert torch.isfinite(also.float()).all() and torch.equal(also[far], (plain * 2 - 1).to(also.dtype)[far])


def test_mask_is_resized_with_the_triangle_filter_and_stays_soft(S):
    from arcflow_amd import ops
    big = np.zeros((40, 56), dtype=np.uint8)
    big[:, :28] = 255
    got = S.call(image=S.photo, mask_image=big, resize='stretch', height=SIZE, width=SIZE)
    m = ops.image_resample(torch.from_numpy(big)[None, ..., None].cuda(), SIZE, SIZE, filter='triangle').cpu()
    assert ((m > 0) & (m < 1)).any() and (m[..., :14] > 1 - 1e-6).all() and (m[..., 18:] == 0).all()                # soft at the edge, nothing binarised
    small = ops.image_resample(torch.from_numpy(S.photo)[None].cuda(), SIZE, SIZE).cpu()
    assert torch.equal(_bits(got), _bits(S.call(image=small, mask_image=m)))


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_sample_teacher_takes_the_same_path(family, tmp_path):
    from arcflow_amd import ops
    from tests.test_teacher_edit_gpu import _pipeline
    pipe, kw = _pipeline(family, str(tmp_path / 'snap'))
    g = torch.Generator().manual_seed(4)
    photo = torch.randint(0, 256, (40, 56, 3), generator=g, dtype=torch.uint8).numpy()
    noise = torch.randn(2, HP * WP, 64, generator=g)
    kw.update(num_inference_steps=3, output_type='latent', strength=0.6, height=SIZE, width=SIZE)
    small = ops.image_resample(torch.from_numpy(photo)[None].cuda(), SIZE, SIZE)
    lat = pipe.vae.encoder.encode_images01(small, sample=False, packed=True)
    want = pipe.sample_teacher(image_latents=lat, latents=noise.clone(), **kw).images.cpu()
    got = pipe.sample_teacher(image=photo, resize='stretch', latents=noise.clone(), **kw).images.cpu()
    assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want))
    mask = torch.zeros(1, 1, SIZE, SIZE)
    mask[..., :8] = 1.0
    a = pipe.sample_teacher(image=photo, resize='stretch', mask_image=mask, mask_blur=1.0, latents=noise.clone(), **kw).images.cpu()
    b = pipe.sample_teacher(image=small.cpu(), mask_image=ops.mask_feather(mask.cuda(), 1.0).cpu(), latents=noise.clone(), **kw).images.cpu()
    assert torch.equal(_bits(a), _bits(b)) and not torch.equal(a, got)
