"""Image-to-image and inpainting on both pipelines, on the tiny engines of tests/test_lora_adapters_gpu.py (D = 256, 2 heads, FLUX 1 double + 1
single block, Qwen-Image 1 layer, an 8 x 8 token grid = 128 x 128 pixels), 2 NFE, ``prompt_embeds`` given.  Almost everything is a bit-equality:
the edit path adds one kernel (afx_edit_blend) whose m = 0 / m = 1 / sigma = 0 / sigma = 1 cases are exact.

The one bound.  With a mask, the unmasked latent pixels after step i are the kernel's  fl(sigma eps + fl(fl(1 - sigma) x0))  (one fma) and are
held to 2 fp32 ulp of (1 - sigma_i) x0 + sigma_i eps formed in fp64 from the fp32 sigma_i the kernel was handed.  Three roundings: the final one is
<= 0.5 ulp(result); p = fl(om x0) is off by <= 0.5 ulp(p); om = fl(1 - sigma) is off by <= 2^-24 om, i.e. by < 1 ulp(p) after the product.  When x0
and eps have the same sign nothing cancels, |p| <= |result|, and the three add up to < 2 ulp(result).  When they have opposite signs the
result can be arbitrarily smaller than p and NO bound in ulps of the result holds for this (or any) fp32 evaluation of the formula; so the
start noise of that test is given the sign of x0 element by element (its magnitudes stay those of a normal draw)."""
import numpy as np
import pytest
import torch

import vae_encoder_ref as E

pytestmark = pytest.mark.gpu

HP = WP = 8
SIZE = 16 * HP
NFE, RATIO = 2, 1.0


class Setup:
    def __init__(self, family):
        from arcflow_amd import FlowMatchEulerDiscreteScheduler
        from arcflow_amd.pipelines import ArcFluxPipeline, ArcQwenImagePipeline
        from oracle import dit_ref as D
        self.family = family
        sch = FlowMatchEulerDiscreteScheduler(shift=3.2)
        if family == 'flux':
            w = D.make_flux_weights(D.FluxCfg(num_layers=1, num_single_layers=1, heads=2, joint_dim=128, pooled_dim=64), seed=9)
            tcfg = dict(num_layers=1, num_single_layers=1, num_attention_heads=2, attention_head_dim=128, in_channels=64, joint_attention_dim=128,
                        pooled_projection_dim=64, guidance_embeds=True)
            self.pipe = ArcFluxPipeline.from_state_dict(tcfg, w, scheduler=sch)
            jd = 128
        else:
            w = D.make_qwen_weights(D.QwenCfg(num_layers=1, heads=2, joint_dim=192), seed=5)
            tcfg = dict(num_layers=1, num_attention_heads=2, attention_head_dim=128, in_channels=64, joint_attention_dim=192)
            self.pipe = ArcQwenImagePipeline.from_state_dict(tcfg, w, scheduler=sch)
            jd = 192
        g = torch.Generator().manual_seed(3)
        self.pe = (torch.randn(1, 12, jd, generator=g) * 0.5).bfloat16()
        self.pooled = (torch.randn(1, 64, generator=g) * 0.5).bfloat16()
        self.noise = torch.randn(2, HP * WP, 64, generator=g)
        self.x0 = torch.randn(1, HP * WP, 64, generator=g) * 0.8

    def call(self, batch=1, output_type='latent', **kw):
        pe = self.pe.repeat(batch, 1, 1)
        if 'latents' not in kw and 'generator' not in kw:
            kw['latents'] = self.noise[:batch].clone()
        if self.family == 'flux':
            cond = dict(prompt_embeds=pe, pooled_prompt_embeds=self.pooled.repeat(batch, 1))
        else:
            cond = dict(prompt_embeds=pe, prompt_embeds_mask=torch.ones(batch, 12, dtype=torch.long))
        kw.setdefault('height', SIZE)
        kw.setdefault('width', SIZE)
        out = self.pipe(num_inference_steps=NFE, timestep_ratio=RATIO, output_type=output_type, **cond, **kw).images
        torch.cuda.synchronize()
        return out.cpu() if isinstance(out, torch.Tensor) else out

    def sigmas(self, strength):
        """-> (fp32 sigma at the start of every step, fp32 sigma every step lands on), as the pipeline walks them."""
        from arcflow_amd.schedule import edit_raw_timesteps
        raw, per_step, total = edit_raw_timesteps(NFE, 128, RATIO, strength)
        ts = self.pipe._retrieve_timesteps(raw, 'cpu', HP * WP).float().tolist()
        starts = [sum(per_step[:i]) for i in range(NFE)]
        return [np.float32(ts[j] / 1000) for j in starts], [np.float32(ts[j] / 1000) for j in starts[1:]] + [np.float32(0.0)]


@pytest.fixture(scope='module', params=['flux', 'qwen'])
def S(request):
    return Setup(request.param)


def _row_mask(rows):
    """Image-resolution mask [1, 1, 128, 128]: the latent rows listed (8 pixel rows each) are repainted."""
    m = torch.zeros(1, 1, SIZE, SIZE)
    for r in rows:
        m[:, :, 8 * r:8 * r + 8] = 1.0
    return m


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_strength_one_is_text_to_image(S):
    start, _ = S.sigmas(1.0)
    assert float(start[0]) == 1.0                                  # shift 3.2 maps raw time 1 to sigma 1 exactly: the blend returns the noise itself
    t2i = S.call()
    assert torch.isfinite(t2i).all()
    assert torch.equal(_bits(S.call(image_latents=S.x0, strength=1.0)), _bits(t2i))
    assert torch.equal(_bits(S.call()), _bits(t2i))               # ... and the edit call left the text-to-image path as it was


def test_mid_strength_starts_at_the_shifted_sigma(S):
    seen = []

    def cb(pipe, i, t, kw):
        seen.append((i, float(t), pipe._current_timestep))
        return {}
    half = S.call(image_latents=S.x0, strength=0.5, callback_on_step_end=cb)
    start, _ = S.sigmas(0.5)
    assert [s[0] for s in seen] == [0, 1]
    assert np.float32(seen[0][1] / 1000) == start[0] and seen[0][2] == seen[0][1] and np.float32(seen[1][1] / 1000) == start[1]
    assert abs(float(start[0]) - 3.2 * 0.5 / (1 + 2.2 * 0.5)) < 1e-6                      # sigma(0.5) under the static shift 3.2
    assert not torch.equal(half, S.call(image_latents=S.x0, strength=1.0))
    # no mask: the result is not the source, and a lower strength stays closer to it
    d_half, d_full = (half - S.x0).norm().item(), (S.call(image_latents=S.x0, strength=1.0) - S.x0).norm().item()
    assert 0 < d_half and torch.isfinite(half).all()
    print(f'{S.family}: |out - x0| at strength 0.5: {d_half:.3f}, at 1.0: {d_full:.3f}')


def test_all_ones_and_all_zero_masks(S):
    plain = S.call(image_latents=S.x0, strength=0.6)
    ones = S.call(image_latents=S.x0, strength=0.6, mask_image=torch.ones(1, 1, SIZE, SIZE))
    assert torch.equal(_bits(ones), _bits(plain))
    zero = S.call(image_latents=S.x0, strength=0.6, mask_image=torch.zeros(SIZE, SIZE))
    assert torch.equal(_bits(zero), _bits(S.x0))


def test_half_mask_keeps_the_unmasked_half_on_the_source_trajectory(S):
    """Latent rows 0-7 (token rows 0-3) repainted, B = 2 with the image and the mask broadcast from a batch of 1."""
    x0 = S.x0
    eps = S.noise.abs() * torch.where(x0 >= 0, 1.0, -1.0)          # same sign as x0: see the module docstring
    seen = []

    def cb(pipe, i, t, kw):
        seen.append(kw['latents'].cpu().clone())
        return {}
    out = S.call(batch=2, image_latents=x0, strength=0.6, mask_image=_row_mask(range(8)), latents=eps.clone(), callback_on_step_end=cb)
    keep = torch.zeros(HP, WP, 64, dtype=torch.bool)
    keep[4:] = True
    keep = keep.view(HP * WP, 64)
    for b in range(2):
        assert torch.equal(_bits(out[b][keep]), _bits(x0[0][keep]))
        assert (out[b][~keep] != x0[0][~keep]).float().mean().item() > 0.99
    assert not torch.equal(out[0], out[1]) and torch.isfinite(out).all()
    _, ends = S.sigmas(0.6)
    assert len(seen) == NFE and torch.equal(_bits(seen[-1]), _bits(out))
    for i, lat in enumerate(seen):
        sg = float(ends[i])
        ref = (1.0 - sg) * x0.double() + sg * eps.double()
        ulp = torch.from_numpy(np.spacing(ref.abs().float().numpy()))
        err = ((lat.double() - ref).abs() / ulp.double())[:, keep]
        print(f'{S.family} step {i} (sigma_end {sg:.6f}): unmasked max err {err.max().item():.3f} ulp')
        assert err.max().item() <= 2.0


def test_mask_is_honoured_per_sub_pixel(S):
    """One repainted PIXEL: its latent pixel (5, 6) = token (2, 3), sub-pixel ph*2 + pw = 1*2 + 0 = 2, and nothing else, leaves the source."""
    m = torch.zeros(1, 1, SIZE, SIZE)
    m[0, 0, 5 * 8 + 3, 6 * 8 + 2] = 1.0
    out = S.call(image_latents=S.x0, strength=0.6, mask_image=m)
    moved = torch.zeros(HP, WP, 16, 4, dtype=torch.bool)
    moved[2, 3, :, 2] = True
    moved = moved.view(1, HP * WP, 64)
    assert torch.equal(_bits(out[~moved]), _bits(S.x0[~moved]))
    assert (out[moved] != S.x0[moved]).all()
    # a soft mask value is a blend, not a switch: 0.5 on that pixel moves the same elements, to other values
    soft = S.call(image_latents=S.x0, strength=0.6, mask_image=m * 0.5)
    assert torch.equal(_bits(soft[~moved]), _bits(S.x0[~moved])) and (soft[moved] != out[moved]).all() and (soft[moved] != S.x0[moved]).all()


def test_latents_replaced_by_the_callback_feed_the_next_forward(S):
    """The loop hands the blend kernel's own bf16 copy of the latents to the next forward.  A callback that returns other latents after
    step 0 must make that copy stale: the result is, bit for bit, the continuation written out here from the replaced latents -- one
    forward on THEIR bf16 rounding, ``ops.arcflow_step`` to sigma 0, the masked blend."""
    from arcflow_amd import ops
    from arcflow_amd.schedule import edit_raw_timesteps, mask_to_tokens
    mask = _row_mask(range(8))
    repl = torch.randn(1, HP * WP, 64, generator=torch.Generator().manual_seed(21))

    def cb(pipe, i, t, kw):
        return dict(latents=repl.cuda()) if i == 0 else {}
    got = S.call(image_latents=S.x0, strength=0.6, mask_image=mask, callback_on_step_end=cb)
    raw, per_step, total = edit_raw_timesteps(NFE, 128, RATIO, 0.6)
    ts = S.pipe._retrieve_timesteps(raw, 'cuda', HP * WP).float().cpu().tolist()
    assert sum(per_step) == len(ts)                                 # the second step is the last: it lands on sigma 0
    t1, ntt = ts[per_step[0]], S.pipe.scheduler.config.num_train_timesteps
    x, eng = repl.cuda(), S.pipe.transformer
    pooled = S.pooled.cuda() if S.family == 'flux' else None
    guidance = torch.full((1,), 3.5, device='cuda', dtype=torch.float32) if S.family == 'flux' and eng.guidance_embeds else None
    out = eng(x.to(torch.bfloat16), torch.full((1,), t1 / 1000.0, device='cuda'), S.pe.cuda(), pooled, guidance, HP, WP)
    x = ops.arcflow_step(x, out.means, out.logweights, out.loggammas, t1 / ntt, t1 / ntt, 0.0, eps=1e-4)
    want, _ = ops.edit_blend(x, S.x0.cuda(), None, mask_to_tokens(mask.cuda(), HP, WP), torch.zeros(1, device='cuda'))
    assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want.cpu()))
    assert not torch.equal(got, S.call(image_latents=S.x0, strength=0.6, mask_image=mask))           # ... and the replacement was felt


def test_determinism_and_generator_equals_explicit_noise(S):
    kw = dict(image_latents=S.x0, strength=0.6, mask_image=_row_mask(range(8)))
    a = S.call(generator=torch.Generator().manual_seed(7), **kw)
    b = S.call(generator=torch.Generator().manual_seed(7), **kw)
    assert torch.equal(_bits(a), _bits(b))
    noise = torch.randn(1, 16, 2 * HP, 2 * WP, generator=torch.Generator().manual_seed(7))
    packed = noise.view(1, 16, HP, 2, WP, 2).permute(0, 2, 4, 1, 3, 5).reshape(1, HP * WP, 64)
    assert torch.equal(_bits(S.call(latents=packed, **kw)), _bits(a))
    assert not torch.equal(S.call(generator=torch.Generator().manual_seed(8), **kw), a)


def test_image_goes_through_the_encoder_and_composite_restores_pixels(S):
    """A reduced-width synthetic encoder / decoder pair attached as pipe.vae / pipe.vae.encoder."""
    from arcflow_amd import vae as VAE
    g = torch.Generator().manual_seed(2)
    if S.family == 'flux':
        from oracle import vae_ref as V
        chans = (64, 128, 128, 128)
        dec = VAE.AutoencoderKLDecoder(V.make_decoder_weights(chans, seed=4), chans, norm_num_groups=16)
        dec.encoder = VAE.AutoencoderKLEncoder(E.make_encoder_weights(chans, seed=3), chans, norm_num_groups=16)
    else:
        from oracle import vae_qwen_ref as V
        mean, std = (torch.randn(16, generator=g) * 0.3).tolist(), (1.0 + 0.5 * torch.rand(16, generator=g)).tolist()
        dec = VAE.AutoencoderKLQwenImageDecoder(V.make_decoder_weights(dim=32, seed=3), mean, std)
        dec.encoder = VAE.AutoencoderKLQwenImageEncoder(E.make_qwen_encoder_weights(dim=32, seed=1), mean, std)
    img = torch.rand(1, 3, SIZE, SIZE, generator=g)
    S.pipe.vae = dec
    try:
        lat = dec.encoder.encode_images01(img, sample=False, packed=True)
        assert lat.shape == (1, HP * WP, 64)
        by_image = S.call(image=img, strength=0.6, height=None, width=None)           # the size comes from the image
        assert torch.equal(_bits(by_image), _bits(S.call(image_latents=lat, strength=0.6)))
        assert torch.equal(_bits(S.call(image=img.permute(0, 2, 3, 1).numpy(), strength=0.6, height=None, width=None)), _bits(by_image))
        mask = torch.zeros(1, 1, SIZE, SIZE)
        mask[..., :SIZE // 2] = 1.0                                                   # repaint the left half
        keep = (mask == 0).expand(1, 3, SIZE, SIZE)
        out = S.call(image=img, mask_image=mask, strength=0.6, output_type='pt')
        want = (img * 2 - 1).to(out.dtype)                                            # 'pt' is the decoder's own range, [-1, 1]
        assert out.shape == (1, 3, SIZE, SIZE) and torch.equal(out[keep], want[keep])
        assert not torch.equal(out[~keep], want[~keep])
        raw = S.call(image=img, mask_image=mask, strength=0.6, output_type='pt', composite=False)
        assert not torch.equal(raw[keep], want[keep]) and torch.equal(raw[~keep], out[~keep])
        arr = S.call(image=img, mask_image=mask, strength=0.6, output_type='np')
        assert arr.shape == (1, SIZE, SIZE, 3) and np.abs(arr - img.permute(0, 2, 3, 1).numpy())[:, :, SIZE // 2:].max() < 1e-2
    finally:
        S.pipe.vae = None
