"""Teacher image-to-image and inpainting on the GPU: ``TeacherSampler(x0=, mask=, strength=)`` on the tiny engines of
tests/test_teacher_sampler_gpu.py (its ``Model``), ``sample_teacher(image=, image_latents=, strength=, mask_image=, composite=)`` of both
pipelines on the synthetic snapshots of tests/snapshot_util.py, the distiller's pass-through and tools/sample_teacher.py ``--image --mask``.

Everything here is a bit-equality or a count: the edit path adds the start blend (afx_edit_blend, exact at sigma = 1) and the fused edit step,
whose m = 0 / m = 1 / sigma_to = 0 cases are exact and whose general case is DEFINED as the plain step followed by afx_edit_blend
(tests/test_hip_teacher_edit_step_fp64.py holds the kernel to that and to fp64); the sampler is held to the same composition written out by hand.
The semantics (truncation by strength, start noise re-used on every step) are this project's own, after diffusers as recalled: nothing pins them.
"""
import os
import sys

import pytest
import torch

import vae_encoder_ref as E
from tests.test_teacher_sampler_gpu import GUID, ROOT, SCALE, Model, T

pytestmark = pytest.mark.gpu

STEPS = 4
GRIDS = [(4, 4), (3, 5)]


@pytest.fixture(scope='module')
def models():
    cache = {}

    def get(family):
        if family not in cache:
            cache[family] = Model(family)
        return cache[family]
    return get


def _sampler(m, steps=STEPS, **kw):
    from arcflow_amd import TeacherSampler
    kw.setdefault('guidance_scale', SCALE)
    kw.setdefault('shift', 3.2)
    return TeacherSampler(m.engine, steps, distilled_guidance=GUID, **kw)


def _inputs(m, B, hp, wp, seed=3):
    """-> (cond for the grid, start noise, source latents, a soft mask with exact 0 / 1 tokens, FlowSDE draws for every step), on the GPU."""
    g = torch.Generator().manual_seed(seed + 100 * hp + wp)
    n = hp * wp
    cond = dict(m.cond(B, seed=seed), hp=hp, wp=wp)
    noise, x0 = torch.randn(B, n, 64, generator=g), torch.randn(B, n, 64, generator=g) * 0.8
    mask = torch.rand(B, n, 4, generator=g)
    mask[:, 0], mask[:, 1] = 0.0, 1.0
    mask[:, 2] = torch.tensor([0.0, 1.0, 1.0, 0.0])
    draws = torch.randn(STEPS, B, n, 64, generator=g)
    return cond, noise.cuda(), x0.cuda(), mask.cuda(), draws.cuda()


def _take(c, a, b):
    return {k: (v[a:b] if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def _bits(t):
    return t.contiguous().view(torch.int32)


class Counter:
    """Counts ``engine.forward`` calls per prompt branch for the duration of a ``with`` block."""

    def __init__(self, engine, cond):
        self.engine, self.neg_ptr, self.pos, self.neg = engine, cond['negative_prompt_embeds'].data_ptr(), 0, 0

    def __enter__(self):
        inner = self.engine.forward

        def forward(x, sigma, ctx, *a, **k):
            if ctx.data_ptr() == self.neg_ptr:
                self.neg += 1
            else:
                self.pos += 1
            return inner(x, sigma, ctx, *a, **k)
        self.engine.forward = forward
        return self

    def __exit__(self, *exc):
        del self.engine.forward


def _by_hand(sampler, cond, noise, x0, mask, strength, draws=None):
    """The edit roll written out with the kernels of the parent commit: start blend, then per step the sampler's plain step followed by
    afx_edit_blend at the sigma the step landed on, with the START noise (none on the step landing on 0)."""
    from arcflow_amd import ops
    from arcflow_amd.schedule import truncate_by_strength
    B = noise.shape[0]
    sigmas, active = sampler.schedule(cond['hp'], cond['wp'])
    t_start, _ = truncate_by_strength(sigmas, strength)
    row = lambda v: torch.full((B,), float(v), device='cuda')          # noqa: E731
    x, xb = ops.edit_blend(None, x0, noise, None, row(sigmas[t_start]))
    for i in range(t_start, sampler.num_steps):
        extra = {}
        if sampler.sampler == 'FlowSDE':
            _, s_to, mm, cn = sampler.scheduler.coefficients(i)
            extra = dict(m=row(mm), c_noise=row(cn), noise=draws[i - t_start] if float(s_to * cn) != 0 else None)
        sampler.step(x, xb, cond, row(sigmas[i]), row(sigmas[i + 1]), active[i], **extra)
        if mask is not None:
            ops.edit_blend(x, x0, noise if float(sigmas[i + 1]) > 0 else None, mask, row(sigmas[i + 1]), out=x, out_bf16=xb)
    return x


@pytest.mark.parametrize('hp,wp', GRIDS)
@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_sampler_edit_identities(models, family, hp, wp):
    m = models(family)
    B = 2
    cond, noise, x0, mask, draws = _inputs(m, B, hp, wp)
    zeros, ones = torch.zeros_like(mask), torch.ones_like(mask)
    for kind, kw, run in (('ode', {}, {}), ('ode_ortho_interval', dict(orthogonal_guidance=True, guidance_interval=[600.0, 950.0]), {}),
                          ('sde', dict(sampler='FlowSDE', h=1.0), dict(step_noise=draws))):
        sampler = _sampler(m, **kw)
        plain = sampler(cond, noise, **run)
        assert float(sampler.schedule(hp, wp)[0][0]) == 1.0                # shift 3.2 maps raw time 1 to sigma 1 exactly: the start blend returns the noise
        # strength 1, no mask: the plain sampler, bit for bit; and the plain sampler is where it was
        assert torch.equal(_bits(sampler(cond, noise, x0=x0, strength=1.0, **run)), _bits(plain)), kind
        assert torch.equal(_bits(sampler(cond, noise, **run)), _bits(plain)), kind
        for strength in (1.0, 0.5):
            sub = {k: v[:2] if strength == 0.5 else v for k, v in run.items()}          # one draw per step that runs
            nomask = sampler(cond, noise, x0=x0, strength=strength, **sub)
            assert torch.isfinite(nomask).all() and not torch.equal(nomask, x0)
            # m = 1 everywhere: the same call without a mask; m = 0 everywhere: the source, whatever the prompts and the guidance
            assert torch.equal(_bits(sampler(cond, noise, x0=x0, mask=ones, strength=strength, **sub)), _bits(nomask)), (kind, strength)
            assert torch.equal(_bits(sampler(cond, noise, x0=x0, mask=zeros, strength=strength, **sub)), _bits(x0)), (kind, strength)
            # a soft mask: the composition of the parent commit's kernels, written out by hand; kept tokens are the source
            got = sampler(cond, noise, x0=x0, mask=mask, strength=strength, **sub)
            want = _by_hand(sampler, cond, noise, x0, mask, strength, sub.get('step_noise'))
            assert torch.equal(_bits(got), _bits(want)), (kind, strength)
            assert torch.equal(_bits(got[:, 0]), _bits(x0[:, 0])) and not torch.equal(got[:, 1], x0[:, 1])
            assert torch.equal(_bits(got[:, 2, 0::4]), _bits(x0[:, 2, 0::4])) and torch.equal(_bits(got[:, 2, 3::4]), _bits(x0[:, 2, 3::4]))
            assert torch.equal(_bits(nomask), _bits(_by_hand(sampler, cond, noise, x0, None, strength, sub.get('step_noise'))))
        # prepared modulation chunks == the plain path, in an edit too
        off = _sampler(m, prepare_steps=False, **kw)
        assert torch.equal(_bits(off(cond, noise, x0=x0, mask=mask, strength=0.5, **sub)), _bits(got)), kind


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_strength_truncates_the_forwards_and_guidance_still_switches_per_step(models, family):
    m = models(family)
    hp, wp = GRIDS[1]
    cond, noise, x0, mask, draws = _inputs(m, 1, hp, wp)
    for scale, want in ((SCALE, (2, 2)), (1.0, (2, 0))):                  # strength 0.5 of 4 steps: exactly 2 forwards per prompt branch
        sampler = _sampler(m, guidance_scale=scale)
        with Counter(m.engine, cond) as n:
            sampler(cond, noise, x0=x0, mask=mask, strength=0.5)
        assert (n.pos, n.neg) == want, (scale, n.pos, n.neg)
        with Counter(m.engine, cond) as n:
            sampler(cond, noise, x0=x0, strength=1.0)
        assert (n.pos, n.neg) == (4, 4 if scale > 1 else 0)
    for orth in (False, True):                                            # the interval covers some of the steps that run, not all
        sampler = _sampler(m, guidance_interval=[600.0, 950.0], orthogonal_guidance=orth)
        active = sampler.schedule(hp, wp)[1]
        assert active == [False, True, True, False]
        for strength, t_start in ((1.0, 0), (0.75, 1), (0.3, 2)):
            with Counter(m.engine, cond) as n:
                out = sampler(cond, noise, x0=x0, mask=mask, strength=strength)
            assert (n.pos, n.neg) == (STEPS - t_start, sum(active[t_start:])), (orth, strength, n.pos, n.neg)
            assert torch.equal(_bits(out), _bits(_by_hand(sampler, cond, noise, x0, mask, strength)))
        assert not torch.equal(out, _sampler(m, orthogonal_guidance=orth)(cond, noise, x0=x0, mask=mask, strength=0.3))      # the interval matters
    # FlowSDE: one draw per step that runs, none for the skipped ones
    sde = _sampler(m, sampler='FlowSDE', h=1.0)
    g = torch.Generator(device='cuda').manual_seed(7)
    out = sde(cond, noise, x0=x0, mask=mask, strength=0.5, generator=g)
    g2 = torch.Generator(device='cuda').manual_seed(7)
    by_hand = torch.stack([torch.randn(tuple(noise.shape), device='cuda', dtype=torch.float32, generator=g2) for _ in range(2)])
    assert torch.equal(g.get_state(), g2.get_state())
    assert torch.equal(_bits(sde(cond, noise, x0=x0, mask=mask, strength=0.5, step_noise=by_hand)), _bits(out))
    with pytest.raises(ValueError, match='step_noise'):
        sde(cond, noise, x0=x0, strength=0.5, step_noise=draws)          # four draws for two steps
    with pytest.raises(ValueError, match='mask needs x0'):
        sde(cond, noise, mask=mask)
    with pytest.raises(ValueError, match='strength'):
        sde(cond, noise, strength=0.5)
    with pytest.raises(ValueError, match='strength'):
        sde(cond, noise, x0=x0, strength=0.0)
    with pytest.raises(ValueError, match='x0'):
        sde(cond, noise, x0=x0[:, :4])


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_batch_of_five_equals_five_single_runs(models, family):
    m = models(family)
    hp, wp = GRIDS[1]
    B = 5
    cond, noise, x0, mask, draws = _inputs(m, B, hp, wp, seed=9)
    for kw, run in ((dict(orthogonal_guidance=True), {}), (dict(sampler='FlowSDE', h=1.0), dict(step_noise=draws[:3]))):
        sampler = _sampler(m, **kw)
        out = sampler(cond, noise, x0=x0, mask=mask, strength=0.75, **run)          # micro-batches of 4 + 1
        for b in range(B):
            one = sampler(_take(cond, b, b + 1), noise[b:b + 1], x0=x0[b:b + 1], mask=mask[b:b + 1], strength=0.75,
                          **{k: v[:, b:b + 1] for k, v in run.items()})
            assert torch.equal(_bits(out[b:b + 1]), _bits(one)), (kw, b)
    # with a generator the whole batch's draws are made first, one per step that runs
    out = sampler(cond, noise, x0=x0, mask=mask, strength=0.75, generator=torch.Generator(device='cuda').manual_seed(5))
    g = torch.Generator(device='cuda').manual_seed(5)
    by_hand = torch.stack([torch.randn(tuple(noise.shape), device='cuda', dtype=torch.float32, generator=g) for _ in range(3)])
    assert torch.equal(_bits(out), _bits(sampler(cond, noise, x0=x0, mask=mask, strength=0.75, step_noise=by_hand)))


# ------------------------------------------------------------------------------------------------ the pipelines
HP = WP = 8
SIZE = 16 * HP


def _pipeline(family, root):
    from arcflow_amd import vae as VAE
    from arcflow_amd.pipelines import ArcFluxPipeline, ArcQwenImagePipeline
    from tests import snapshot_util as SU
    g = torch.Generator().manual_seed(2)
    B = 2
    if family == 'flux':
        snap = SU.write_flux_snapshot(root, with_text=False)
        pipe = ArcFluxPipeline.from_pretrained(root)
        chans = snap['vae_channels']
        pipe.vae.encoder = VAE.AutoencoderKLEncoder(E.make_encoder_weights(chans, seed=3), chans, norm_num_groups=16)
        pe, ne = (torch.randn(B, T, 128, generator=g) * 0.5).bfloat16(), (torch.randn(B, T, 128, generator=g) * 0.5).bfloat16()
        pooled, npooled = (torch.randn(B, 64, generator=g) * 0.5).bfloat16(), (torch.randn(B, 64, generator=g) * 0.5).bfloat16()
        kw = dict(prompt_embeds=pe, pooled_prompt_embeds=pooled, negative_prompt_embeds=ne, negative_pooled_prompt_embeds=npooled)
    else:
        snap = SU.write_qwen_snapshot(root, with_text=False)
        pipe = ArcQwenImagePipeline.from_pretrained(root)
        pipe.vae.encoder = VAE.AutoencoderKLQwenImageEncoder(E.make_qwen_encoder_weights(dim=32, seed=1), snap['latents_mean'], snap['latents_std'])
        pe, ne = (torch.randn(B, T, 256, generator=g) * 0.5).bfloat16(), (torch.randn(B, T, 256, generator=g) * 0.5).bfloat16()
        ones = torch.ones(B, T, dtype=torch.long)
        kw = dict(prompt_embeds=pe, prompt_embeds_mask=ones, negative_prompt_embeds=ne, negative_prompt_embeds_mask=ones)
    kw.update(num_inference_steps=STEPS, guidance_scale=GUID, true_cfg_scale=SCALE)
    return pipe, kw


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_pipeline_sample_teacher_image_and_mask(family, tmp_path):
    """On the parent commit every call here fails with TypeError (unexpected keyword ``image``): the must-fail-without-the-feature test."""
    from arcflow_amd import TeacherSampler
    pipe, kw = _pipeline(family, str(tmp_path / 'snap'))
    g = torch.Generator().manual_seed(4)
    img = torch.rand(1, 3, SIZE, SIZE, generator=g)
    noise = torch.randn(2, HP * WP, 64, generator=g)
    mask = torch.zeros(1, 1, SIZE, SIZE)
    mask[..., :SIZE // 2] = 1.0                                                       # repaint the left half: token columns 0-3
    lat = pipe.vae.encoder.encode_images01(img, sample=False, packed=True)
    assert lat.shape == (1, HP * WP, 64)

    def run(**more):
        more.setdefault('latents', noise.clone())
        more.setdefault('output_type', 'latent')
        out = pipe.sample_teacher(**kw, **more).images
        return out.cpu() if isinstance(out, torch.Tensor) else out
    i2i = run(image=img, strength=0.6)                                                # the size comes from the image
    assert i2i.shape == (2, HP * WP, 64) and torch.isfinite(i2i).all() and not torch.equal(i2i[0], i2i[1])
    assert torch.equal(_bits(run(image_latents=lat, strength=0.6, height=SIZE, width=SIZE)), _bits(i2i))          # image_latents round-trips
    assert torch.equal(_bits(run(image=img.permute(0, 2, 3, 1).numpy(), strength=0.6)), _bits(i2i))
    plain = run(height=SIZE, width=SIZE)
    if family == 'flux':          # strength 1 starts at sigmas[0]; this schedule's is exactly 1, so the start is the noise and the roll the plain teacher's
        assert torch.equal(_bits(run(image=img, strength=1.0)), _bits(plain))
    else:                         # Qwen-Image's terminal stretch leaves sigmas[0] an ulp or two above 1 in fp32: the start is the noise only to within that
        assert torch.isfinite(run(image=img, strength=1.0)).all()
    # what TeacherSampler makes of the same operands
    cond = dict(prompt_embeds=kw['prompt_embeds'].cuda(), negative_prompt_embeds=kw['negative_prompt_embeds'].cuda(), hp=HP, wp=WP)
    if family == 'flux':
        cond.update(pooled=kw['pooled_prompt_embeds'].cuda(), negative_pooled=kw['negative_pooled_prompt_embeds'].cuda())
    want = TeacherSampler(pipe.transformer, STEPS, guidance_scale=SCALE, distilled_guidance=GUID, tokens_as_seq_len=True,
                          **pipe._euler_scheduler_kwargs())(cond, noise.cuda(), x0=lat.expand(2, -1, -1).contiguous(), strength=0.6)
    assert torch.equal(_bits(i2i), _bits(want.cpu()))
    # inpainting: the kept tokens are the encoded source, bit for bit; the repainted ones are not
    inp = run(image=img, mask_image=mask, strength=0.6)
    keep = torch.zeros(HP, WP, 64, dtype=torch.bool)
    keep[:, WP // 2:] = True
    keep = keep.view(HP * WP, 64)
    for b in range(2):
        assert torch.equal(_bits(inp[b][keep]), _bits(lat[0].cpu()[keep]))
        assert (inp[b][~keep] != lat[0].cpu()[~keep]).float().mean().item() > 0.99
    assert torch.isfinite(inp).all() and not torch.equal(inp, i2i)
    assert torch.equal(_bits(run(image=img, mask_image=mask, strength=0.6, sampler='FlowSDE', h=1.0,
                                 generator=torch.Generator(device='cuda').manual_seed(1))[0][keep]), _bits(lat[0].cpu()[keep]))
    # decoded: with composite the pixels outside the mask are the input image's, without it they are the decoder's
    keep_px = (mask == 0).expand(2, 3, SIZE, SIZE)
    out = run(image=img, mask_image=mask, strength=0.6, output_type='pt')
    want_px = (img * 2 - 1).to(out.dtype).expand(2, -1, -1, -1)                        # 'pt' is the decoder's own range, [-1, 1]
    assert out.shape == (2, 3, SIZE, SIZE) and torch.equal(out[keep_px], want_px[keep_px]) and not torch.equal(out[~keep_px], want_px[~keep_px])
    raw = run(image=img, mask_image=mask, strength=0.6, output_type='pt', composite=False)
    assert not torch.equal(raw[keep_px], want_px[keep_px]) and torch.equal(raw[~keep_px], out[~keep_px])
    with pytest.raises(ValueError, match='mask_image'):
        run(mask_image=mask)
    with pytest.raises(ValueError, match='strength'):
        run(image=img, strength=1e-20)


def test_distiller_passes_the_edit_through_and_tool_caches_it(tmp_path):
    from arcflow_amd import TeacherSampler
    from arcflow_amd.train import data
    from arcflow_amd.train.distill import ArcFlowDistiller, DistillConfig
    from oracle import dit_ref as D
    hp, wp = 4, 4
    cfg = D.FluxCfg(num_layers=1, num_single_layers=1, heads=2, joint_dim=128, pooled_dim=64)
    w = D.make_flux_weights(cfg, seed=2, teacher_head=True)
    dc = DistillConfig(teacher_guidance_scale=SCALE, teacher_guidance=2.5)
    dist = ArcFlowDistiller('flux', dict(num_double=1, num_single=1, heads=2, joint_dim=128, pooled_dim=64), w, dc)
    g = torch.Generator().manual_seed(8)
    cond = dict(prompt_embeds=(torch.randn(2, T, 128, generator=g) * 0.5).bfloat16().cuda(),
                negative_prompt_embeds=(torch.randn(2, T, 128, generator=g) * 0.5).bfloat16().cuda(),
                pooled=(torch.randn(2, 64, generator=g) * 0.5).bfloat16().cuda(),
                negative_pooled=(torch.randn(2, 64, generator=g) * 0.5).bfloat16().cuda(), hp=hp, wp=wp)
    noise, x0 = torch.randn(2, hp * wp, 64, generator=g).cuda(), torch.randn(2, hp * wp, 64, generator=g).cuda()
    mask = (torch.rand(2, hp * wp, 4, generator=g) > 0.5).float().cuda()
    want = TeacherSampler(dist.teacher, 4, guidance_scale=SCALE, distilled_guidance=2.5, shift=dc.shift)(cond, noise, x0=x0, mask=mask, strength=0.5)
    got = dist.sample_teacher(cond, noise, num_steps=4, x0=x0, mask=mask, strength=0.5)
    kept = mask[:, :, torch.arange(64, device='cuda') & 3] == 0
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(got[kept]), _bits(x0[kept]))
    # the tool: --synthetic --image <latents .pt> --mask <latent-resolution .pt> writes records that the data mode reads back
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import sample_teacher as tool
    finally:
        sys.path.pop(0)
    src = torch.randn(16, 2 * hp, 2 * wp, generator=g) * 0.8
    m = torch.zeros(2 * hp, 2 * wp)
    m[:, :wp] = 1.0                                                                  # repaint the left half of the latent
    torch.save(src, str(tmp_path / 'src.pt'))
    torch.save(m, str(tmp_path / 'mask.pt'))
    assert torch.equal(tool.unpack(tool.pack(src[None]), hp, wp)[0], src)

    def write(name, *more):
        cache = str(tmp_path / name)
        done = tool.main(['--family', 'flux', '--synthetic', '--cache-dir', cache, '--count', '2', '--latent-size', '16', str(2 * hp), str(2 * wp),
                          '--steps', '4', '--true-cfg-scale', '4.0', '--image', str(tmp_path / 'src.pt'), *more])
        ds = data.PromptEmbedCache(cache, load_latents=True)
        assert len(ds) == 2 and all(torch.equal(ds[i]['latents'], done[fn].half().float()) for i, fn in enumerate(ds.files))
        return [done[fn] for fn in ds.files]
    inp = write('a', '--mask', str(tmp_path / 'mask.pt'), '--strength', '0.5')
    for lat in inp:
        assert torch.isfinite(lat).all() and torch.equal(_bits(lat[:, :, wp:]), _bits(src[:, :, wp:])) and (lat[:, :, :wp] != src[:, :, :wp]).all()
    assert not torch.equal(inp[0], inp[1])
    i2i = write('b', '--strength', '0.5')
    assert not torch.equal(i2i[0][:, :, wp:], src[:, :, wp:])
    with pytest.raises(SystemExit):
        tool.main(['--family', 'flux', '--synthetic', '--cache-dir', str(tmp_path / 'c'), '--mask', str(tmp_path / 'mask.pt')])
