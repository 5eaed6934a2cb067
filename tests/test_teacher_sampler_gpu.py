"""Teacher sampling on the GPU: ``TeacherSampler`` (Euler ODE + true CFG on the fused step kernel), the pipelines' and the distiller's
``sample_teacher`` and tools/sample_teacher.py, on the tiny engines of tests/test_hip_engine.py: 1 + 1 FLUX blocks / 2 Qwen-Image
blocks, D = 256 (2 heads), 16 image tokens + 8 text tokens.

Bounds.  One fused step against the composed ops (engine -> .float() -> ops.cfg_combine -> ops.euler_roll) runs the SAME forwards,
so only the step arithmetic differs: both sides are within the step bound of tests/test_hip_teacher_step_fp64.py of the exact value
(7 * 2^-24 * M, M = |x| + |dt| (|pos| + |scale - 1| (|pos| + |neg|)); the composed path has the same six roundings), and their
difference is asserted against that bound.  The orthogonal step is checked against tests/teacher_sampler_ref.py in fp64 fed the engine's own
velocities: 9 * 2^-24 * M plus the coefficient's own bound carried to the output, |d coef| |pos| |dt|.

The four-step roll is held to the project's bar (tests/test_full_depth_parity.py): rel-L2 of the HIP latents against the fp32 oracle
<= 1.5 x the eager-bf16 oracle's + 2e-3.
"""
import os
import sys

import pytest
import torch

from tests import teacher_sampler_ref as TS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
HP = WP = 4
T = 8
SCALE = 4.0
GUID = 3.5
FACTOR, FLOOR = 1.5, 2e-3


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp(min=1e-12)).item()


class Model:
    """A tiny teacher: oracle weights + the HIP engine bound to them + the oracle's forward for one conditioning."""

    def __init__(self, family, seed=11):
        from arcflow_amd import MMDiTEngine
        from oracle import dit_ref as D
        self.family, self.D = family, D
        if family == 'flux':
            self.cfg = D.FluxCfg(num_layers=1, num_single_layers=1, heads=2, joint_dim=128, pooled_dim=64)
            self.w = D.make_flux_weights(self.cfg, seed=seed, teacher_head=True)
            self.kw = dict(num_double=1, num_single=1, heads=2, joint_dim=128, pooled_dim=64)
            self.engine = MMDiTEngine('flux', 1, 1, heads=2, joint_dim=128, pooled_dim=64, teacher_head=True)
        else:
            self.cfg = D.QwenCfg(num_layers=2, heads=2, joint_dim=192)
            self.w = D.make_qwen_weights(self.cfg, seed=seed)
            g = torch.Generator().manual_seed(seed + 1)
            self.w['proj_out.weight'] = (torch.randn(64, self.cfg.dim, generator=g) * 0.02).bfloat16()
            self.w['proj_out.bias'] = (torch.randn(64, generator=g) * 0.02).bfloat16()
            self.kw = dict(num_double=2, heads=2, joint_dim=192)
            self.engine = MMDiTEngine('qwen', 2, 0, heads=2, joint_dim=192, teacher_head=True)
        self.engine.load_state_dict(self.w)

    def cond(self, B, seed=5, device='cuda'):
        g = torch.Generator().manual_seed(seed)
        joint = self.cfg.joint_dim
        c = dict(prompt_embeds=(torch.randn(B, T, joint, generator=g) * 0.5).bfloat16().to(device),
                 negative_prompt_embeds=(torch.randn(B, T, joint, generator=g) * 0.5).bfloat16().to(device), hp=HP, wp=WP)
        if self.family == 'flux':
            c['pooled'] = (torch.randn(B, 64, generator=g) * 0.5).bfloat16().to(device)
            c['negative_pooled'] = (torch.randn(B, 64, generator=g) * 0.5).bfloat16().to(device)
        return c

    def oracle(self, cond):
        """denoise(x, sigma, negative) on the CPU oracle: bf16 cast at the transformer input, as the reference's pred()."""
        D, c = self.D, {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in cond.items()}

        def denoise(x, s, negative):
            B = x.shape[0]
            ctx = c['negative_prompt_embeds' if negative else 'prompt_embeds'].float()
            t = torch.full((B,), s)
            xin = x.float().bfloat16().float()
            if self.family == 'flux':
                pooled = c['negative_pooled' if negative else 'pooled'].float()
                return D.flux_teacher_forward(self.w, self.cfg, xin, ctx, pooled, t, torch.full((B,), GUID), HP, WP)
            return TS.qwen_teacher_forward(D, self.w, self.cfg, xin, ctx, t, HP, WP)
        return denoise


@pytest.fixture(scope='module')
def models():
    cache = {}

    def get(family):
        if family not in cache:
            cache[family] = Model(family)
        return cache[family]
    return get


def _noise(B, seed=3):
    return torch.randn(B, HP * WP, 64, generator=torch.Generator().manual_seed(seed))


def _sampler(m, steps=4, **kw):
    from arcflow_amd import TeacherSampler
    kw.setdefault('guidance_scale', SCALE)
    kw.setdefault('shift', 3.2)
    return TeacherSampler(m.engine, steps, distilled_guidance=GUID, **kw)


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_one_step_equals_composed_ops_and_fp64_orthogonal(models, family):
    from arcflow_amd import ops
    m = models(family)
    B = 2
    cond = m.cond(B)
    x0 = _noise(B).cuda()
    sig, sig_to = torch.tensor([0.76, 0.76]).cuda(), torch.tensor([0.52, 0.52]).cuda()
    g = torch.full((B,), GUID).cuda() if family == 'flux' else None
    pos = m.engine(x0.bfloat16(), sig, cond['prompt_embeds'], cond.get('pooled'), g, HP, WP)
    neg = m.engine(x0.bfloat16(), sig, cond['negative_prompt_embeds'], cond.get('negative_pooled'), g, HP, WP)
    composed = ops.euler_roll(x0, ops.cfg_combine(pos.float(), neg.float(), SCALE), sig, sig_to)
    x, xb = x0.clone(), x0.bfloat16()
    _sampler(m).step(x, xb, cond, sig, sig_to, True)
    p, q, dt = pos.double().cpu(), neg.double().cpu(), (sig_to.double() - sig.double()).cpu()[:, None, None]
    M = x0.double().cpu().abs() + dt.abs() * (p.abs() + (SCALE - 1) * (p.abs() + q.abs()))
    diff = (x.double().cpu() - composed.double().cpu()).abs()
    print(f'{family}: fused vs composed max diff / bound {(diff / (7 * EPS * M)).max().item():.3f}')
    assert (diff <= 7 * EPS * M).all()
    assert torch.equal(xb, x.bfloat16())
    # inactive step: the negative forward is skipped and the step is the plain Euler roll
    x1, xb1 = x0.clone(), x0.bfloat16()
    _sampler(m).step(x1, xb1, cond, sig, sig_to, False)
    plain = ops.euler_roll(x0, pos.float(), sig, sig_to)
    assert ((x1.double().cpu() - plain.double().cpu()).abs() <= 7 * EPS * (x0.double().cpu().abs() + dt.abs() * p.abs())).all()
    # orthogonal: fp64 restatement fed the engine's own velocities
    x2, xb2 = x0.clone(), x0.bfloat16()
    _sampler(m, orthogonal_guidance=True).step(x2, xb2, cond, sig, sig_to, True)
    bias = TS.guidance_bias(p, q, SCALE, orthogonal=True)
    ref = TS.euler_step(x0.double().cpu(), p + bias, sig.double().cpu()[:, None, None], sig_to.double().cpu()[:, None, None])
    plain_bias = (p - q) * (SCALE - 1)
    den = (p * p).flatten(1).sum(1).clamp(min=p[0].numel() * 1e-6)
    coef = (plain_bias * p).flatten(1).sum(1) / den
    coef_bound = (3 * EPS * (plain_bias * p).abs().flatten(1).sum(1) / den)[:, None, None]
    bound = 9 * EPS * (M + dt.abs() * (coef[:, None, None] * p).abs()) + coef_bound * p.abs() * dt.abs()
    err = (x2.double().cpu() - ref).abs()
    print(f'{family}: orthogonal step max err / bound {(err / bound).max().item():.3f}  coef {coef.tolist()}')
    assert (err <= bound).all()
    assert ((x2 - x).abs() > 0).float().mean().item() > 0.5            # (the orthogonal term is not a no-op here)


@pytest.mark.parametrize('orthogonal', [False, True], ids=['plain', 'ortho'])
@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_four_step_roll_against_fp32_and_eager_bf16_oracles(models, family, orthogonal):
    m = models(family)
    B = 2
    cond, noise = m.cond(B), _noise(B)
    sampler = _sampler(m, orthogonal_guidance=orthogonal)
    sigmas, active = sampler.schedule(HP, WP)
    assert all(active) and sigmas.numel() == 5
    ref_sig, _ = TS.euler_sigmas(4, shift=3.2)
    assert torch.equal(sigmas, ref_sig)
    denoise = m.oracle(cond)
    with torch.no_grad():
        ref = TS.sample(denoise, noise, sigmas, SCALE, orthogonal=orthogonal)
        with m.D.eager_bf16():
            eager = TS.sample(denoise, noise, sigmas, SCALE, orthogonal=orthogonal)
    hip = sampler(cond, noise.cuda())
    torch.cuda.synchronize()
    e_hip, e_eager = rel_l2(hip, ref), rel_l2(eager, ref)
    print(f'{family} orthogonal={orthogonal}: 4-step CFG {SCALE} latents rel-L2 vs fp32 oracle: hip {e_hip:.3e}  eager-bf16 {e_eager:.3e}')
    assert hip.dtype == torch.float32 and hip.shape == noise.shape and torch.isfinite(hip).all()
    assert e_hip <= FACTOR * e_eager + FLOOR, (e_hip, e_eager)


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_guidance_interval_skips_the_negative_forward(models, family):
    m = models(family)
    cond, noise = m.cond(2), _noise(2).cuda()
    sampler = _sampler(m, guidance_interval=[600, 950])          # t = 1000, 905.7, 761.9, 516.1: active on steps 1 and 2 only
    _, active = sampler.schedule(HP, WP)
    assert active == [False, True, True, False]
    calls = []
    real = m.engine.forward

    def counting(x, t, ctx, *a, **kw):
        calls.append(ctx.data_ptr() == cond['negative_prompt_embeds'].data_ptr())
        return real(x, t, ctx, *a, **kw)
    m.engine.forward = counting
    try:
        out = sampler(cond, noise)
    finally:
        del m.engine.forward
    assert sum(calls) == sum(active) == 2 and len(calls) == 4 + 2
    assert calls == [False, False, True, False, True, False]
    # and the numbers are those of the restated loop on the engine itself: same steps with and without guidance
    full = _sampler(m)(cond, noise)
    none = _sampler(m, guidance_scale=1.0)(cond, noise)
    assert not torch.equal(out, full) and not torch.equal(out, none)


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_prepared_steps_microbatches_and_reproducibility(models, family):
    m = models(family)
    cond5, noise5 = m.cond(5, seed=9), _noise(5, seed=4).cuda()
    take = lambda c, a, b: {k: (v[a:b] if isinstance(v, torch.Tensor) else v) for k, v in c.items()}      # noqa: E731
    for orth in (False, True):
        sampler = _sampler(m, orthogonal_guidance=orth)
        out5 = sampler(cond5, noise5)
        assert torch.equal(sampler(cond5, noise5), out5)                                         # a second run is bit-identical
        out4, out1 = sampler(take(cond5, 0, 4), noise5[:4]), sampler(take(cond5, 4, 5), noise5[4:])
        assert torch.equal(out5, torch.cat([out4, out1]))                                       # B = 5 = micro-batches of 4 + 1
        plain = _sampler(m, orthogonal_guidance=orth, prepare_steps=False)
        assert torch.equal(plain(take(cond5, 0, 2), noise5[:2]), sampler(take(cond5, 0, 2), noise5[:2]))      # prepared modulation chunks == the plain path
    # prepare_steps() returning False (patched: as for a batch it cannot hold) falls back to the plain path
    real = m.engine.prepare_steps
    m.engine.prepare_steps = lambda *a, **k: False
    try:
        fallback = _sampler(m)(take(cond5, 0, 2), noise5[:2])
    finally:
        del m.engine.prepare_steps
    assert real is not None and torch.equal(fallback, _sampler(m)(take(cond5, 0, 2), noise5[:2]))


def test_sampler_argument_errors(models):
    from arcflow_amd import MMDiTEngine, TeacherSampler
    m = models('qwen')
    with pytest.raises(ValueError):
        TeacherSampler(MMDiTEngine('qwen', 1, 0, heads=2, joint_dim=192), 4)             # a student engine
    cond = m.cond(1)
    cond.pop('negative_prompt_embeds')
    with pytest.raises(ValueError):
        _sampler(m)(cond, _noise(1).cuda())                                               # true CFG without a negative prompt
    out = _sampler(m, guidance_scale=1.0)(cond, _noise(1).cuda())                         # no guidance: fine without one
    assert torch.isfinite(out).all()


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_pipeline_sample_teacher(models, family, tmp_path):
    from arcflow_amd import TeacherSampler
    from arcflow_amd.pipelines import ArcFluxPipeline, ArcQwenImagePipeline
    from tests import snapshot_util as SU
    root = str(tmp_path / 'snap')
    if family == 'flux':
        SU.write_flux_snapshot(root, with_text=False, with_vae=False)
        pipe = ArcFluxPipeline.from_pretrained(root)
        joint = 128
    else:
        SU.write_qwen_snapshot(root, with_text=False, with_vae=False)
        pipe = ArcQwenImagePipeline.from_pretrained(root)
        joint = 256
    assert pipe.transformer.teacher_head
    g = torch.Generator().manual_seed(2)
    B = 2
    pe, ne = (torch.randn(B, T, joint, generator=g) * 0.5).bfloat16(), (torch.randn(B, T, joint, generator=g) * 0.5).bfloat16()
    noise = _noise(B).cuda()
    cond = dict(prompt_embeds=pe.cuda(), negative_prompt_embeds=ne.cuda(), hp=HP, wp=WP)
    if family == 'flux':
        pooled, npooled = (torch.randn(B, 64, generator=g) * 0.5).bfloat16(), (torch.randn(B, 64, generator=g) * 0.5).bfloat16()
        cond.update(pooled=pooled.cuda(), negative_pooled=npooled.cuda())
        kw = dict(prompt_embeds=pe, pooled_prompt_embeds=pooled, negative_prompt_embeds=ne, negative_pooled_prompt_embeds=npooled)
    else:
        mask = torch.ones(B, T, dtype=torch.long)
        kw = dict(prompt_embeds=pe, prompt_embeds_mask=mask, negative_prompt_embeds=ne, negative_prompt_embeds_mask=mask)
    got = pipe.sample_teacher(height=16 * HP, width=16 * WP, num_inference_steps=4, guidance_scale=GUID, true_cfg_scale=SCALE,
                              latents=noise, output_type='latent', **kw).images
    want = TeacherSampler(pipe.transformer, 4, guidance_scale=SCALE, distilled_guidance=GUID, tokens_as_seq_len=True,
                          **pipe._euler_scheduler_kwargs())(cond, noise)
    assert torch.equal(got, want) and torch.isfinite(got).all()
    tup = pipe.sample_teacher(height=16 * HP, width=16 * WP, num_inference_steps=4, guidance_scale=GUID, true_cfg_scale=SCALE,
                              latents=noise, output_type='latent', return_dict=False, **kw)
    assert isinstance(tup, tuple) and torch.equal(tup[0], want)
    with pytest.raises(RuntimeError, match='no VAE decoder'):        # decoding is __call__'s: without a VAE only latents come out
        pipe.sample_teacher(height=16 * HP, width=16 * WP, num_inference_steps=1, true_cfg_scale=1.0, latents=noise, output_type='pt', **kw)
    with pytest.raises(RuntimeError, match='load_arcflow_adapter'):         # the student entry is unchanged: no adapter, no sampling
        if family == 'flux':
            pipe(prompt_embeds=pe, pooled_prompt_embeds=pooled, height=16 * HP, width=16 * WP, output_type='latent')
        else:
            pipe(prompt_embeds=pe, prompt_embeds_mask=mask, height=16 * HP, width=16 * WP, output_type='latent')
    # a pipeline that only ever saw student weights has no velocity head to sample
    sd = {k: v for k, v in pipe._base_state_dict.items() if not k.startswith('proj_out.')}
    student_only = type(pipe)()
    student_only._transformer_config, student_only._base_state_dict = pipe._transformer_config, sd
    with pytest.raises(RuntimeError, match='proj_out'):
        student_only.sample_teacher(height=16 * HP, width=16 * WP, latents=noise, output_type='latent', true_cfg_scale=1.0, **kw)


def test_distiller_sample_teacher_and_tool_cache_roundtrip(tmp_path):
    from arcflow_amd import TeacherSampler
    from arcflow_amd.train import data
    from arcflow_amd.train.distill import ArcFlowDistiller, DistillConfig
    from oracle import dit_ref as D
    cfg = D.FluxCfg(num_layers=1, num_single_layers=1, heads=2, joint_dim=128, pooled_dim=64)
    w = D.make_flux_weights(cfg, seed=2, teacher_head=True)
    dc = DistillConfig(teacher_guidance_scale=SCALE, teacher_guidance=2.5)
    dist = ArcFlowDistiller('flux', dict(num_double=1, num_single=1, heads=2, joint_dim=128, pooled_dim=64), w, dc)
    g = torch.Generator().manual_seed(8)
    cond = dict(prompt_embeds=(torch.randn(2, T, 128, generator=g) * 0.5).bfloat16().cuda(),
                negative_prompt_embeds=(torch.randn(2, T, 128, generator=g) * 0.5).bfloat16().cuda(),
                pooled=(torch.randn(2, 64, generator=g) * 0.5).bfloat16().cuda(),
                negative_pooled=(torch.randn(2, 64, generator=g) * 0.5).bfloat16().cuda(), hp=HP, wp=WP)
    noise = _noise(2).cuda()
    got = dist.sample_teacher(cond, noise, num_steps=3)
    want = TeacherSampler(dist.teacher, 3, guidance_scale=SCALE, distilled_guidance=2.5, shift=dc.shift)(cond, noise)
    assert torch.equal(got, want) and torch.isfinite(got).all()
    # the tool: --synthetic writes records that PromptEmbedCache(load_latents=True) reads back bit-equal
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import sample_teacher as tool
    finally:
        sys.path.pop(0)
    cache = str(tmp_path / 'cache')
    done = tool.main(['--family', 'flux', '--synthetic', '--cache-dir', cache, '--count', '3', '--latent-size', '16', str(2 * HP), str(2 * WP),
                      '--steps', '3', '--true-cfg-scale', '4.0'])
    ds = data.PromptEmbedCache(cache, load_latents=True)
    assert len(ds) == 3 and sorted(done) == sorted(ds.files)
    for i, fn in enumerate(ds.files):
        item = ds[i]
        assert item['latent_size'] == (16, 2 * HP, 2 * WP) and item['latents'].dtype == torch.float32
        assert torch.equal(item['latents'], done[fn].half().float()) and torch.isfinite(item['latents']).all()
    assert not torch.equal(ds[0]['latents'], ds[1]['latents'])
    batch = data.collate([ds[0], ds[1]], device='cuda')          # what tools/train.py --data-dir feeds the data mode
    assert batch['latents'].shape == (2, 16, 2 * HP, 2 * WP) and batch['hp'] == HP
