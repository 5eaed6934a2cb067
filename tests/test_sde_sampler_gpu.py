"""Stochastic teacher sampling on the GPU: ``TeacherSampler(sampler='FlowSDE')`` (FlowSDEScheduler + true CFG on the fused step kernel
``afx_teacher_sde_step``), the pipelines' and the distiller's ``sample_teacher`` and tools/sample_teacher.py, on the tiny engines of
tests/test_teacher_sampler_gpu.py (its ``Model``: 1 + 1 FLUX blocks / 2 Qwen-Image blocks, D = 256, 16 image tokens + 8 text tokens).

Bounds.  The four-step roll with explicit per-step draws is held to the project's bar (tests/test_full_depth_parity.py,
as the ODE sampler's roll): rel-L2 of the HIP latents against the fp32 oracle loop (tests/sde_sampler_ref.py, fed the SAME draws)
<= 1.5 x the eager-bf16 oracle's + 2e-3.

h = 0 on the SDE path against the ODE path of the same sampler.  In real arithmetic the two steps are equal; in fp32 they differ by rounding
(tests/test_hip_teacher_sde_step_fp64.py bounds it per step), and a rounding-sized difference of the fp32 state can flip the bf16 rounding
of an element the next forward reads -- one bf16 ulp, 2^-8 relative, on that element -- after which the two rolls see different velocities.
The fp32 oracle rounds its forward's input to bf16 in the same place, so its own h = 0 roll departs from its ODE roll by the same
mechanism: that departure is the yardstick, under the same section-2 rule (<= 1.5 x the oracle's + 2e-3, the floor being what that rule
grants for bf16 roundings that fall differently), not a constant chosen for this test.
"""
import os
import sys

import pytest
import torch

from tests import sde_sampler_ref as SR
from tests import teacher_sampler_ref as TS
from tests.test_teacher_sampler_gpu import FACTOR, FLOOR, GUID, HP, ROOT, SCALE, WP, Model, T, _noise, rel_l2

pytestmark = pytest.mark.gpu

STEPS = 4


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
    kw.setdefault('sampler', 'FlowSDE')
    return TeacherSampler(m.engine, steps, distilled_guidance=GUID, **kw)


def _draws(B, steps=STEPS, seed=21):
    return torch.randn(steps, B, HP * WP, 64, generator=torch.Generator().manual_seed(seed))


def _take(c, a, b):
    return {k: (v[a:b] if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


@pytest.mark.parametrize('orthogonal', [False, True], ids=['plain', 'ortho'])
@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_four_step_sde_roll_against_fp32_and_eager_bf16_oracles(models, family, orthogonal):
    m = models(family)
    B = 2
    cond, noise, draws = m.cond(B), _noise(B), _draws(B)
    sampler = _sampler(m, h=1.0, orthogonal_guidance=orthogonal)
    sigmas, active = sampler.schedule(HP, WP)
    assert all(active) and sigmas.numel() == STEPS + 1
    ref_sig, _ = TS.euler_sigmas(STEPS, shift=3.2)
    assert torch.equal(sigmas, ref_sig)
    denoise = m.oracle(cond)
    with torch.no_grad():
        ref = SR.sample(denoise, noise, sigmas, draws, h=1.0, guidance_scale=SCALE, orthogonal=orthogonal)
        with m.D.eager_bf16():
            eager = SR.sample(denoise, noise, sigmas, draws, h=1.0, guidance_scale=SCALE, orthogonal=orthogonal)
    hip = sampler(cond, noise.cuda(), step_noise=draws.cuda())
    torch.cuda.synchronize()
    e_hip, e_eager = rel_l2(hip, ref), rel_l2(eager, ref)
    print(f'{family} orthogonal={orthogonal}: 4-step FlowSDE h=1 CFG {SCALE} latents rel-L2 vs fp32 oracle: hip {e_hip:.3e}  eager-bf16 {e_eager:.3e}')
    assert hip.dtype == torch.float32 and hip.shape == noise.shape and torch.isfinite(hip).all()
    assert e_hip <= FACTOR * e_eager + FLOOR, (e_hip, e_eager)
    # the same draws again: bit-identical; draws from the CPU work as well as from the device
    assert torch.equal(sampler(cond, noise.cuda(), step_noise=draws.cuda()), hip)
    assert torch.equal(sampler(cond, noise.cuda(), step_noise=draws), hip)
    # the noise matters: the ODE roll of the same sampler is somewhere else
    ode = _sampler(m, sampler='FlowEulerODE', orthogonal_guidance=orthogonal)(cond, noise.cuda())
    assert rel_l2(hip, ode) > FACTOR * e_eager + FLOOR


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_generator_equals_hand_made_draws_and_seeds_differ(models, family):
    m = models(family)
    B = 2
    cond, noise = m.cond(B), _noise(B).cuda()
    sampler = _sampler(m, h=1.0)
    for dev in ('cuda', 'cpu'):
        out = sampler(cond, noise, generator=torch.Generator(device=dev).manual_seed(7))
        g = torch.Generator(device=dev).manual_seed(7)
        by_hand = torch.stack([torch.randn((B, HP * WP, 64), device=dev, dtype=torch.float32, generator=g) for _ in range(STEPS)])
        assert torch.equal(sampler(cond, noise, step_noise=by_hand), out), dev
        assert torch.equal(sampler(cond, noise, generator=torch.Generator(device=dev).manual_seed(7)), out), dev
        other = sampler(cond, noise, generator=torch.Generator(device=dev).manual_seed(8))
        assert torch.isfinite(other).all() and not torch.equal(other, out), dev
    # the generator advances once per step, also on the final step whose draw the kernel does not read (sigma_to = 0)
    g = torch.Generator(device='cuda').manual_seed(7)
    sampler(cond, noise, generator=g)
    g2 = torch.Generator(device='cuda').manual_seed(7)
    for _ in range(STEPS):
        torch.randn((B, HP * WP, 64), device='cuda', dtype=torch.float32, generator=g2)
    assert torch.equal(g.get_state(), g2.get_state())
    # one generator per sample
    gens = [torch.Generator(device='cuda').manual_seed(30 + b) for b in range(B)]
    per_sample = sampler(cond, noise, generator=gens)
    solo = sampler(_take(cond, 1, 2), noise[1:2], generator=torch.Generator(device='cuda').manual_seed(31))
    assert torch.equal(per_sample[1:2], solo)
    # the ODE sampler accepts and ignores both
    ode = _sampler(m, sampler='FlowEulerODE')
    assert torch.equal(ode(cond, noise, generator=torch.Generator(device='cuda').manual_seed(7), step_noise=by_hand.cuda()), ode(cond, noise))


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_h0_on_the_sde_path_against_the_ode_path(models, family):
    m = models(family)
    B = 2
    cond, noise, draws = m.cond(B), _noise(B), _draws(B)
    sigmas, _ = TS.euler_sigmas(STEPS, shift=3.2)
    denoise = m.oracle(cond)
    with torch.no_grad():
        o_ode = TS.sample(denoise, noise, sigmas, SCALE)
        o_sde = SR.sample(denoise, noise, sigmas, draws, h=0.0, guidance_scale=SCALE)
    h_ode = _sampler(m, sampler='FlowEulerODE')(cond, noise.cuda())
    h_sde = _sampler(m, h=0.0)(cond, noise.cuda(), step_noise=draws.cuda())
    d_hip, d_oracle = rel_l2(h_sde, h_ode), rel_l2(o_sde, o_ode)
    print(f'{family}: h = 0 vs ODE latents rel-L2: hip {d_hip:.3e}  fp32 oracle {d_oracle:.3e}')
    assert torch.isfinite(h_sde).all()
    assert d_hip <= FACTOR * d_oracle + FLOOR, (d_hip, d_oracle)
    # c_noise = 0 on every step: the draws are not read, whatever they are
    assert torch.equal(_sampler(m, h=0.0)(cond, noise.cuda(), generator=torch.Generator(device='cuda').manual_seed(1)), h_sde)


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_microbatches_do_not_change_the_samples(models, family):
    m = models(family)
    B = 6
    cond, noise, draws = m.cond(B, seed=9), _noise(B, seed=4).cuda(), _draws(B, seed=22).cuda()
    for orth in (False, True):
        sampler = _sampler(m, h=1.0, orthogonal_guidance=orth)
        out6 = sampler(cond, noise, step_noise=draws)                      # micro-batches of 4 + 2
        a, b = sampler(_take(cond, 0, 3), noise[:3], step_noise=draws[:, :3]), sampler(_take(cond, 3, 6), noise[3:], step_noise=draws[:, 3:])
        assert torch.equal(out6, torch.cat([a, b])), orth                  # = the per-sample results of 3 + 3
    # with a generator the whole batch's draws are made first, step by step: the same draws a single roll would make
    out = sampler(cond, noise, generator=torch.Generator(device='cuda').manual_seed(5))
    g = torch.Generator(device='cuda').manual_seed(5)
    by_hand = torch.stack([torch.randn((B, HP * WP, 64), device='cuda', dtype=torch.float32, generator=g) for _ in range(STEPS)])
    assert torch.equal(out, sampler(cond, noise, step_noise=by_hand))
    # prepared modulation chunks == the plain path, as for the ODE sampler
    plain = _sampler(m, h=1.0, orthogonal_guidance=True, prepare_steps=False)
    assert torch.equal(plain(_take(cond, 0, 2), noise[:2], step_noise=draws[:, :2]), sampler(_take(cond, 0, 2), noise[:2], step_noise=draws[:, :2]))


def test_sampler_argument_errors(models):
    m = models('qwen')
    cond, noise = m.cond(1), _noise(1).cuda()
    with pytest.raises(ValueError, match='step_noise'):
        _sampler(m)(cond, noise, step_noise=torch.zeros(STEPS + 1, 1, HP * WP, 64))
    with pytest.raises(ValueError):                                        # the reference asserts h > 0
        _sampler(m, h=-1.0)(cond, noise)
    out = _sampler(m, h='inf', guidance_scale=1.0)(cond, noise)           # no generator: the default one; h = 'inf' re-noises fully
    assert torch.isfinite(out).all() and out.shape == noise.shape


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_pipeline_sample_teacher_sde(models, family, tmp_path):
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
    g = torch.Generator().manual_seed(2)
    B = 2
    pe, ne = (torch.randn(B, T, joint, generator=g) * 0.5).bfloat16(), (torch.randn(B, T, joint, generator=g) * 0.5).bfloat16()
    cond = dict(prompt_embeds=pe.cuda(), negative_prompt_embeds=ne.cuda(), hp=HP, wp=WP)
    if family == 'flux':
        pooled, npooled = (torch.randn(B, 64, generator=g) * 0.5).bfloat16(), (torch.randn(B, 64, generator=g) * 0.5).bfloat16()
        cond.update(pooled=pooled.cuda(), negative_pooled=npooled.cuda())
        kw = dict(prompt_embeds=pe, pooled_prompt_embeds=pooled, negative_prompt_embeds=ne, negative_pooled_prompt_embeds=npooled)
    else:
        mask = torch.ones(B, T, dtype=torch.long)
        kw = dict(prompt_embeds=pe, prompt_embeds_mask=mask, negative_prompt_embeds=ne, negative_prompt_embeds_mask=mask)
    kw.update(height=16 * HP, width=16 * WP, num_inference_steps=STEPS, guidance_scale=GUID, true_cfg_scale=SCALE, output_type='latent')

    def run(seed, **more):
        return pipe.sample_teacher(generator=torch.Generator(device='cuda').manual_seed(seed), **kw, **more).images
    got = run(3, sampler='FlowSDE', h=1.0)
    assert torch.isfinite(got).all() and got.shape == (B, HP * WP, 64)
    assert torch.equal(run(3, sampler='FlowSDE', h=1.0), got)                         # reproducible under the same seed
    assert not torch.equal(run(4, sampler='FlowSDE', h=1.0), got)
    assert not torch.equal(run(3), got)                                               # the default is still the ODE sampler
    # the generator's stream: the start noise first, then one draw per step -- what TeacherSampler makes of the same stream
    gen = torch.Generator(device='cuda').manual_seed(3)
    latents, hp, wp = pipe._prepare_latents(B, 16 * HP, 16 * WP, gen, None)
    want = TeacherSampler(pipe.transformer, STEPS, guidance_scale=SCALE, distilled_guidance=GUID, tokens_as_seq_len=True, sampler='FlowSDE', h=1.0,
                          **pipe._euler_scheduler_kwargs())(cond, latents, generator=gen)
    assert (hp, wp) == (HP, WP) and torch.equal(got, want)
    with pytest.raises(TypeError):                                                    # h belongs to FlowSDE
        run(3, h=1.0)
    with pytest.raises(ValueError):
        run(3, sampler='FlowAdapter')


def test_distiller_and_tool_sde(tmp_path):
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
    noise, draws = _noise(2).cuda(), _draws(2, steps=3).cuda()
    want = TeacherSampler(dist.teacher, 3, guidance_scale=SCALE, distilled_guidance=2.5, shift=dc.shift, sampler='FlowSDE', h=2.0)(cond, noise, step_noise=draws)
    assert torch.equal(dist.sample_teacher(cond, noise, num_steps=3, sampler='FlowSDE', h=2.0, step_noise=draws), want) and torch.isfinite(want).all()
    a = dist.sample_teacher(cond, noise, num_steps=3, sampler='FlowSDE', generator=torch.Generator(device='cuda').manual_seed(1))
    b = dist.sample_teacher(cond, noise, num_steps=3, sampler='FlowSDE', generator=torch.Generator(device='cuda').manual_seed(1))
    assert torch.equal(a, b) and not torch.equal(a, want)
    # the tool: --sampler FlowSDE --h inf writes records; the same --seed writes the same latents, another seed others
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import sample_teacher as tool
    finally:
        sys.path.pop(0)

    def write(name, seed, *more):
        cache = str(tmp_path / name)
        argv = ['--family', 'flux', '--synthetic', '--cache-dir', cache, '--count', '2', '--latent-size', '16', str(2 * HP), str(2 * WP),
                '--steps', '3', '--true-cfg-scale', '4.0', '--seed', str(seed), *more]
        done = tool.main(argv)
        ds = data.PromptEmbedCache(cache, load_latents=True)
        assert len(ds) == 2 and all(torch.equal(ds[i]['latents'], done[fn].half().float()) for i, fn in enumerate(ds.files))
        return [done[fn] for fn in ds.files]
    inf_a, inf_b = write('a', 0, '--sampler', 'FlowSDE', '--h', 'inf'), write('b', 0, '--sampler', 'FlowSDE', '--h', 'inf')
    assert all(torch.equal(x, y) and torch.isfinite(x).all() for x, y in zip(inf_a, inf_b))
    ode = write('c', 0)
    assert not torch.equal(ode[0], inf_a[0])
    half = write('d', 0, '--sampler', 'FlowSDE', '--h', '0.5')
    assert not torch.equal(half[0], inf_a[0]) and not torch.equal(half[0], ode[0])
