"""The UniPC multistep teacher sampler on the GPU: ``TeacherSampler(sampler='UniPC')`` (FlowUniPCScheduler + true CFG on the fused step kernel
``afx_teacher_unipc_step``), the pipelines' and the distiller's ``sample_teacher`` and tools/sample_teacher.py, on the tiny engines of
tests/test_teacher_sampler_gpu.py (its ``Model``), built as tests/test_sde_sampler_gpu.py builds them.

The roll against ``FlowUniPCScheduler.step()``.  The sampler's roll is replayed by a torch loop over the scheduler's own ``step()``, fed the
engine's own forwards: every (pos, neg) pair the roll's engine returned is recorded, u = pos + (pos - neg)(scale - 1) is formed from them in
fp32 as the kernel forms it, and ``step()`` advances an fp32 state of its own.  (Feeding the replay the forwards of ITS OWN state instead would
let a rounding-sized difference of the state flip a bf16 rounding at the engine's input, after which the two rolls see different velocities --
the mechanism tests/test_sde_sampler_gpu.py describes; what is under test here is the step arithmetic and the state handling, not the engine.)

Bound, per element, accumulated over the roll.  Per step the kernel is within (5, 10, 14) eps times (M_m, S_c, S_p) of exact arithmetic on its
inputs (tests/test_hip_teacher_unipc_step_fp64.py; no orthogonal term here) and ``step()`` -- the same sums unfused, a rounding per product
and per addition -- within (6, 15, 22): m_t = x - s u rounds the product and the difference on top of u's three, 5, +1 for second order; x_c
has up to 5 products and 4 additions, 9, plus m_t's 5, +1; x_next 4 products and 3 additions, 7, plus the larger of x_c's 14 and m_t's 5 (they
weigh different summands of S_p), +1.  So one step from IDENTICAL inputs differs by at most (11, 25, 36) eps (M_m, S_c, S_p).  The inputs are
not identical after the first step: with E_x, E_last, E_k the bounds on the difference of x, last_sample and m[-k] so far, linearity gives
    E(m_t)    = E_x + 11 eps M_m
    E(x_c)    = |c_last| E_last + sum_k |c_k| E_k + |c_mt| E_x + 25 eps S_c              (E(x_c) = E_x without a corrector)
    E(x_next) = |p_xc| (E(x_c) - 25 eps S_c) + sum_k |p_k| E_k + |p_mt| E_x + 36 eps S_p
(the roundings of x_c and m_t are inside the 36 eps S_p already), M_m, S_c, S_p evaluated on the replay's fp64 copy of its state.
"""
import os
import sys

import pytest
import torch

from tests.test_teacher_sampler_gpu import GUID, HP, ROOT, SCALE, WP, Model, T, _noise

pytestmark = pytest.mark.gpu

STEPS = 4
EPS = 2.0 ** -24
K_M, K_C, K_P = 5 + 6, 10 + 15, 14 + 22


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
    kw.setdefault('sampler', 'UniPC')
    return TeacherSampler(m.engine, steps, distilled_guidance=GUID, **kw)


def _take(c, a, b):
    return {k: (v[a:b] if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def _recording(engine):
    """Wrap engine.forward so that every output is kept (a clone: the engine reuses its buffers) -> (list, undo)."""
    seen, real = [], engine.forward

    def forward(*a, **kw):
        out = real(*a, **kw)
        seen.append(out.clone())
        return out
    engine.forward = forward

    def undo():
        del engine.forward
    return seen, undo


def _replay(sampler, noise, forwards, begin=0, E0=None):
    """The torch loop over FlowUniPCScheduler.step() on the recorded forwards -> (latents fp32, accumulated bound fp64), both on the CPU.
    E0: the bound on the difference of the two start states (None: they are the same bits)."""
    from arcflow_amd import FlowUniPCScheduler
    cfgd = dict(sampler.scheduler.config)
    sch = FlowUniPCScheduler(cfgd.pop('num_train_timesteps'), **cfgd)
    sch.set_timesteps(sampler.num_steps, seq_len=noise.shape[1] * 4)
    sch.set_begin_index(begin)
    x = noise.float().cpu().clone()
    E_x, E_last, E_h = torch.zeros_like(x, dtype=torch.float64) if E0 is None else E0.double(), None, []
    for j, i in enumerate(range(begin, sampler.num_steps)):
        pos, neg = forwards[2 * j].float().cpu(), forwards[2 * j + 1].float().cpu()
        u = pos + (pos - neg) * (SCALE - 1.0)
        co = sch.coefficients(i, begin)
        hist = [t.double() for t in sch.model_outputs[::-1]]
        last = None if sch.last_sample is None else sch.last_sample.double()
        U = pos.double().abs() + (SCALE - 1.0) * (pos.double().abs() + neg.double().abs())
        M_m = x.double().abs() + co.sigma * U
        if co.corrector is None:
            S_c, E_c, R_c = x.double().abs(), E_x, 0.0
        else:
            cl, cm, *ch = co.corrector
            S_c = abs(cl) * last.abs() + sum(abs(ch[k]) * hist[k].abs() for k in range(co.corrector_order)) + abs(cm) * M_m
            R_c = K_C * EPS * S_c
            E_c = abs(cl) * E_last + sum(abs(ch[k]) * E_h[k] for k in range(co.corrector_order)) + abs(cm) * E_x + R_c
        px, pm, *ph = co.predictor
        S_p = abs(px) * S_c + sum(abs(ph[k]) * hist[k].abs() for k in range(co.predictor_order - 1)) + abs(pm) * M_m
        E_n = abs(px) * (E_c - R_c) + sum(abs(ph[k]) * E_h[k] for k in range(co.predictor_order - 1)) + abs(pm) * E_x + K_P * EPS * S_p
        E_h = ([E_x + K_M * EPS * M_m] + E_h)[:sch.config.solver_order]
        E_last, E_x = E_c, E_n
        x = sch.step(u, sch.timesteps[i], x).prev_sample
    return x, E_x


@pytest.mark.parametrize('order,steps', [(2, 4), (3, 6)])
@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_roll_equals_the_scheduler_step_loop_on_the_engines_own_forwards(models, family, order, steps):
    """B = 2, 3 x 2 tokens, true CFG on; 4 steps at the default order, and 6 at order 3 (lower_order_final caps the order at the number of
    steps left, so a 4-step roll never gets past order 2)."""
    m = models(family)
    B, hp, wp = 2, 3, 2
    cond = dict(m.cond(B), hp=hp, wp=wp)
    noise = torch.randn(B, hp * wp, 64, generator=torch.Generator().manual_seed(3))
    sampler = _sampler(m, steps, solver_order=order)
    sigmas, active = sampler.schedule(hp, wp)
    assert all(active) and sigmas.numel() == steps + 1 and float(sigmas[0]) == 1.0
    assert max(sampler.scheduler.coefficients(i).predictor_order for i in range(steps)) == order
    seen, undo = _recording(m.engine)
    try:
        hip = sampler(cond, noise.cuda())
        torch.cuda.synchronize()
    finally:
        undo()
    assert len(seen) == 2 * steps                                        # a positive and a negative forward per step, nothing else
    ref, bound = _replay(sampler, noise, seen)
    err = (hip.double().cpu() - ref.double()).abs()
    print(f'{family} order {order}: UniPC roll vs step() loop: max err / bound {(err / bound).max().item():.3f}  (max |err| {err.max().item():.3e}, max bound {bound.max().item():.3e})')
    assert hip.dtype == torch.float32 and hip.shape == noise.shape and torch.isfinite(hip).all()
    assert (err <= bound).all(), (err / bound).max().item()
    # again: bit-identical; the plain path (modulation per forward) = the prepared chunks; generator and step_noise are accepted and ignored
    assert torch.equal(sampler(cond, noise.cuda()), hip)
    assert torch.equal(_sampler(m, steps, solver_order=order, prepare_steps=False)(cond, noise.cuda()), hip)
    assert torch.equal(sampler(cond, noise.cuda(), generator=torch.Generator(device='cuda').manual_seed(1), step_noise=torch.zeros(1)), hip)
    # the solver matters: the Euler roll and the other order are somewhere else
    euler = _sampler(m, steps, sampler='FlowEulerODE')(cond, noise.cuda())
    print(f'{family} order {order}: max |UniPC - Euler| {(hip - euler).abs().max().item():.3e}')
    assert (hip - euler).abs().max().item() > bound.max().item()         # (a rounding bound: below what separates two samplers)
    assert not torch.equal(_sampler(m, steps, solver_order=order - 1)(cond, noise.cuda()), hip)


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_batch_of_five_equals_its_rows_run_singly(models, family):
    m = models(family)
    B = 5
    cond, noise = m.cond(B, seed=9), _noise(B, seed=4).cuda()
    for kw in (dict(), dict(solver_order=3, orthogonal_guidance=True)):
        sampler = _sampler(m, **kw)
        out = sampler(cond, noise)                                         # micro-batches of 4 + 1
        assert torch.isfinite(out).all()
        for b in range(B):
            assert torch.equal(out[b:b + 1], sampler(_take(cond, b, b + 1), noise[b:b + 1])), (kw, b)


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_strength_runs_the_suffix_on_an_empty_history(models, family):
    m = models(family)
    B = 2
    cond, noise = m.cond(B), _noise(B)
    x0 = torch.randn(B, HP * WP, 64, generator=torch.Generator().manual_seed(12)) * 0.7
    sampler = _sampler(m, solver_order=3)
    seen, undo = _recording(m.engine)
    try:
        hip = sampler(cond, noise.cuda(), x0=x0.cuda(), strength=0.5)
        torch.cuda.synchronize()
    finally:
        undo()
    assert len(seen) == 2 * (STEPS // 2)                                  # t_start = 2: steps 2 and 3 run
    sigmas, _ = sampler.schedule(HP, WP)
    s = sigmas[2]
    start = ((1 - s) * x0 + s * noise).float()
    # the start is the source noised to sigmas[2]: afx_edit_blend rounds 1 - s, its product with x0 and the fma (3), the line above 1 - s, two
    # products and the sum (4), each of a term that (1 - s) |x0| + s |noise| bounds: 7 eps of it, + 1 for second order
    ref, bound = _replay(sampler, start, seen, begin=2, E0=8 * EPS * ((1 - s) * x0.abs() + s * noise.abs()))
    err = (hip.double().cpu() - ref.double()).abs()
    print(f'{family}: strength 0.5 suffix vs step() loop: max err / bound {(err / bound).max().item():.3f}')
    assert torch.isfinite(hip).all() and (err <= bound).all(), (err / bound).max().item()
    assert torch.equal(sampler(cond, noise.cuda(), x0=x0.cuda(), strength=0.5), hip)
    assert not torch.equal(sampler(cond, noise.cuda(), x0=x0.cuda(), strength=1.0), hip)
    with pytest.raises(ValueError, match='mask.*UniPC'):
        sampler(cond, noise.cuda(), x0=x0.cuda(), mask=torch.ones(B, HP * WP, 4).cuda(), strength=0.5)


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_pipeline_sample_teacher_unipc_and_the_other_samplers_unchanged(models, family, tmp_path):
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
    got = run(3, sampler='UniPC')
    assert torch.isfinite(got).all() and got.shape == (B, HP * WP, 64)
    assert torch.equal(run(3, sampler='UniPC'), got) and torch.equal(run(3, sampler='UniPC', solver_order=2, solver_type='bh2'), got)
    assert not torch.equal(run(3, sampler='UniPC', solver_order=1), got) and not torch.equal(run(3, sampler='UniPC', solver_type='bh1'), got)
    gen = torch.Generator(device='cuda').manual_seed(3)
    latents, hp, wp = pipe._prepare_latents(B, 16 * HP, 16 * WP, gen, None)
    want = TeacherSampler(pipe.transformer, STEPS, guidance_scale=SCALE, distilled_guidance=GUID, tokens_as_seq_len=True, sampler='UniPC',
                          **pipe._euler_scheduler_kwargs())(cond, latents)
    assert (hp, wp) == (HP, WP) and torch.equal(got, want)
    with pytest.raises(TypeError):                                                    # solver_order belongs to UniPC
        run(3, solver_order=2)
    with pytest.raises(ValueError, match='UniPC'):                                    # the reference's name still raises, and says where to go
        run(3, sampler='FlowAdapter')
    # the Euler and SDE results of the same seeds: what a second call gives, and not the UniPC roll
    for more in (dict(), dict(sampler='FlowSDE', h=1.0)):
        a = run(3, **more)
        assert torch.equal(run(3, **more), a) and not torch.equal(a, got)
    want = TeacherSampler(pipe.transformer, STEPS, guidance_scale=SCALE, distilled_guidance=GUID, tokens_as_seq_len=True,
                          **pipe._euler_scheduler_kwargs())(cond, latents)
    assert torch.equal(run(3), want)


def test_distiller_and_tool_unipc(tmp_path):
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
    want = TeacherSampler(dist.teacher, 3, guidance_scale=SCALE, distilled_guidance=2.5, shift=dc.shift, sampler='UniPC', solver_order=3)(cond, noise)
    assert torch.equal(dist.sample_teacher(cond, noise, num_steps=3, sampler='UniPC', solver_order=3), want) and torch.isfinite(want).all()
    euler = dist.sample_teacher(cond, noise, num_steps=3)
    assert torch.equal(dist.sample_teacher(cond, noise, num_steps=3), euler) and not torch.equal(euler, want)
    # the tool: --sampler UniPC writes records; the same --seed writes the same latents; the order matters; the default is still the ODE sampler
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import sample_teacher as tool
    finally:
        sys.path.pop(0)

    def write(name, *more):
        cache = str(tmp_path / name)
        argv = ['--family', 'flux', '--synthetic', '--cache-dir', cache, '--count', '2', '--latent-size', '16', str(2 * HP), str(2 * WP),
                '--steps', '3', '--true-cfg-scale', '4.0', '--seed', '0', *more]
        done = tool.main(argv)
        ds = data.PromptEmbedCache(cache, load_latents=True)
        assert len(ds) == 2 and all(torch.equal(ds[i]['latents'], done[fn].half().float()) for i, fn in enumerate(ds.files))
        return [done[fn] for fn in ds.files]
    a, b = write('a', '--sampler', 'UniPC'), write('b', '--sampler', 'UniPC', '--solver-order', '2')
    assert all(torch.equal(x, y) and torch.isfinite(x).all() for x, y in zip(a, b))
    third = write('c', '--sampler', 'UniPC', '--solver-order', '3', '--solver-type', 'bh1')
    ode = write('d')
    assert not torch.equal(third[0], a[0]) and not torch.equal(ode[0], a[0])
