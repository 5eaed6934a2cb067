"""Stochastic teacher sampling on the CPU: ``FlowSDEScheduler`` and the restated loop (tests/sde_sampler_ref.py) against fixture G13
(tests/golden/g13_sde_sampler.npz: the reference's own scheduler and ``GaussianFlow.forward_test`` with ``sampler='FlowSDE'`` executed
on the closed-form stub denoiser of G12, every draw recorded; tests/golden/make_golden_sde_sampler.py), the h = 0 identity against
the Euler fixture G12, the test_cfg helper, the constructor checks and the argument checks of ``afx_teacher_sde_step``, which return
before any launch.  No GPU."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import sde_sampler_ref as SR
from tests import teacher_sampler_ref as TS

TOL = 2e-6            # the ODE scheduler's fixture tolerance (tests/test_teacher_sampler_cpu.py)
EPS = 2.0 ** -24
HS = [('h0', 0.0), ('h0p5', 0.5), ('h1', 1.0), ('h2', 2.0), ('hinf', 'inf')]
ROLLS = [('h1_plain', 1.0, False), ('h1_ortho', 1.0, True), ('h0', 0.0, False)]


@pytest.fixture(scope='module')
def g13(golden):
    return golden('g13_sde_sampler')


@pytest.fixture(scope='module')
def g12(golden):
    return golden('g12_teacher_sampler')


def _stub(x, sigma, negative):
    """The closed-form denoiser fixtures G12 and G13 were generated with (t / 1000 = sigma)."""
    if negative:
        return 0.25 * x - 0.5 * sigma + 0.04 * torch.roll(x, 1, dims=-2) + 0.1
    return 0.3 * x - 0.7 * sigma + 0.05 * torch.roll(x, 1, dims=-1)


@pytest.mark.parametrize('tag,h', HS)
def test_tables_and_coefficients_bit_equal(g13, g12, tag, h):
    from arcflow_amd import FlowEulerODEScheduler, FlowSDEScheduler
    sch = FlowSDEScheduler(1000, h=h, shift=3.2)
    ts = sch.set_timesteps(7)
    assert sch.sigmas.dtype == torch.float32 and sch.config.h == h
    assert np.array_equal(sch.sigmas.numpy(), g13['tab_sigmas']) and np.array_equal(ts.numpy(), g13['tab_timesteps'])
    # the ODE scheduler's tables, with the trailing 0: the same code
    ode = FlowEulerODEScheduler(1000, shift=3.2)
    ode.set_timesteps(7)
    assert torch.equal(ode.sigmas, sch.sigmas) and torch.equal(ode.timesteps, sch.timesteps) and float(sch.sigmas[-1]) == 0.0
    assert np.array_equal(g13['tab_sigmas'], g12['tab1_sigmas'])
    co = [sch.coefficients(i) for i in range(7)]
    for i, (sigma, sigma_to, m, c) in enumerate(co):
        assert all(v.dtype == torch.float32 and v.dim() == 0 for v in (sigma, sigma_to, m, c))
        assert sigma.item() == g13['tab_sigmas'][i] and sigma_to.item() == g13['tab_sigmas'][i + 1]
    m, c = np.asarray([v[2].item() for v in co], np.float32), np.asarray([v[3].item() for v in co], np.float32)
    print(f'h={h}: m {m.tolist()}  c_noise {c.tolist()}')
    assert np.array_equal(m, g13[f'step_{tag}_m']) and np.array_equal(c, g13[f'step_{tag}_c'])
    if h not in (0.0,):
        assert m[0] == 0.0 and m[-1] == 0.0 and c[0] == 1.0          # sigma = 1 (alpha = 0) and sigma_to = 0
    # the helper's coefficients are pinned by the same numbers
    hm, hc = SR.sde_coefficients(sch.sigmas[:-1], sch.sigmas[1:], h)
    assert np.array_equal(hm.numpy(), g13[f'step_{tag}_m']) and np.array_equal(hc.numpy(), g13[f'step_{tag}_c'])


@pytest.mark.parametrize('tag,h', HS)
def test_step_matches_reference(g13, tag, h):
    from arcflow_amd import FlowSDEScheduler
    sch = FlowSDEScheduler(1000, h=h, shift=3.2)
    sch.set_timesteps(7)
    x = torch.from_numpy(g13['step_sample'])
    worst = 0.0
    for t, u, z, ref in zip(sch.timesteps, torch.from_numpy(g13['step_model_output']), torch.from_numpy(g13['step_noise']),
                            torch.from_numpy(g13[f'step_{tag}_prev_sample'])):
        x = sch.step(u, t, x, return_dict=False, noise=z)[0]
        worst = max(worst, (x - ref).abs().max().item())
        assert x.dtype == torch.float32
    print(f'h={h}: step max |d prev_sample| {worst:.3e}  (bit-equal is expected)')
    assert worst <= TOL
    assert sch.step_index == 7


def test_scheduler_config_noise_default_and_errors():
    from arcflow_amd import FlowEulerODEScheduler, FlowSDEScheduler
    assert FlowSDEScheduler._DEFAULTS == dict(FlowEulerODEScheduler._DEFAULTS, h=1.0)
    sch = FlowSDEScheduler.from_config(dict(num_train_timesteps=1000, shift=3.0, base_shift=0.5, h=2.0, _class_name='x'), shift=3.2)
    assert sch.config.shift == 3.2 and sch.config.h == 2.0 and sch.config.terminal_sigma is None and len(sch) == 1000 and sch.order == 1
    assert FlowSDEScheduler().config.h == 1.0 and FlowSDEScheduler(h='inf').config.h == 'inf'
    dyn = FlowSDEScheduler(use_dynamic_shifting=True)
    assert abs(dyn.get_shift(seq_len=256) - np.exp(0.5)) < 1e-12 and abs(dyn.get_shift(seq_len=4096) - np.exp(1.15)) < 1e-12
    with pytest.raises(TypeError):
        FlowSDEScheduler(flow_shift=3.0)
    with pytest.raises(TypeError):
        FlowEulerODEScheduler(h=1.0)                        # h is the SDE scheduler's alone
    with pytest.raises(ValueError):
        FlowSDEScheduler(h='lots')
    sch.set_timesteps(3)
    with pytest.raises(ValueError):
        sch.step(torch.zeros(2), 0, torch.zeros(2))
    with pytest.raises(NotImplementedError):
        sch.step(torch.zeros(2), sch.timesteps[0], torch.zeros(2), prediction_type='x0')
    neg = FlowSDEScheduler(h=-0.5)
    neg.set_timesteps(3)
    with pytest.raises(ValueError):                         # where the reference asserts h > 0
        neg.step(torch.zeros(2), neg.timesteps[0], torch.zeros(2))
    with pytest.raises(ValueError):
        neg.coefficients(0)
    # the default draw: torch.randn of model_output's shape from the generator, fp32 -- one draw per step, also on the last one
    u, x = torch.ones(2, 3), torch.zeros(2, 3)
    a, b = FlowSDEScheduler(h=1.0), FlowSDEScheduler(h=1.0)
    a.set_timesteps(3)
    b.set_timesteps(3)
    ga, gb = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    xa, xb = x, x
    for t in a.timesteps:
        xa = a.step(u, t, xa, generator=ga).prev_sample
        xb = b.step(u, t, xb, noise=torch.randn(2, 3, generator=gb), return_dict=False)[0]
    assert torch.equal(xa, xb) and torch.equal(ga.get_state(), gb.get_state())
    assert a.step_index == 3 and not torch.equal(xa, x)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('tag,h,orthogonal', ROLLS)
def test_restated_loop_matches_forward_test(g13, tag, h, orthogonal, dtype):
    noise, draws = torch.from_numpy(g13['roll_noise']), torch.from_numpy(g13['roll_draws'])
    sigmas, _ = TS.euler_sigmas(5, shift=float(g13['roll_shift']))
    trace = {}
    x = SR.sample(_stub, noise, sigmas, draws, h=h, guidance_scale=float(g13['roll_scale']), orthogonal=orthogonal, dtype=dtype, trace=trace)
    ref = torch.from_numpy(g13[f'roll_{tag}_x_t']).double()
    got = torch.stack(trace['x_t']).double()
    assert got.shape == ref.shape and torch.equal(got[-1], x.double())
    excess = ((got - ref).abs() / (1 + ref.abs())).max().item()
    print(f'{tag} {dtype}: max |d x_t| / (1 + |ref|) {excess:.3e}')
    assert excess <= TOL
    assert all(m.dtype == torch.float32 for m in trace['m'])


def test_scheduler_object_reproduces_the_rolls(g13):
    """FlowSDEScheduler itself (not the helper) in the loop of forward_test, fed the recorded draws."""
    from arcflow_amd import FlowSDEScheduler
    noise, draws = torch.from_numpy(g13['roll_noise']), torch.from_numpy(g13['roll_draws'])
    scale = float(g13['roll_scale'])
    for tag, h, orthogonal in ROLLS:
        sch = FlowSDEScheduler(1000, h=h, shift=float(g13['roll_shift']))
        sch.set_timesteps(5, seq_len=16)
        x = noise
        for i, t in enumerate(sch.timesteps):
            s = float(t) / 1000
            pos, neg = _stub(x, s, False), _stub(x, s, True)
            x = sch.step(pos + TS.guidance_bias(pos, neg, scale, orthogonal), t, x, noise=draws[i], return_dict=False)[0]
            ref = torch.from_numpy(g13[f'roll_{tag}_x_t'][i])
            assert ((x - ref).abs() / (1 + ref.abs())).max().item() <= TOL, (tag, i)


def test_h0_roll_agrees_with_the_euler_fixture(g13, g12):
    """h = 0: m = 1 and c_noise = 0, so the SDE step is alpha_to (x - sigma u) + sigma_to (x + alpha u) = x + u (sigma_to - sigma)
    exactly in real arithmetic (alpha_to - 1 = -sigma_to, alpha = 1 - sigma: the u terms are -alpha_to sigma + sigma_to alpha =
    sigma_to - sigma).  G13's h = 0 roll and G12's plain Euler roll (same stub, same start noise, same scale and shift) therefore
    differ by fp32 rounding only, and the bound below is derived from the operations, not fitted.

    Let F(x) = x + u(x) dt be the exact step and g = alpha_to sigma + sigma_to alpha >= |dt|.  One step of either roll is F plus
      * the rounding of the stub + guidance evaluation, E_u, times the weight of u in the step (|dt| <= g for the ODE form; g for the SDE form);
      * the rounding of the step itself: the ODE form rounds dt, u dt and the sum (3 roundings), the SDE form alpha, alpha_to, sigma u,
        x0, alpha u, eps, alpha_to x0, sigma_to (.) and the sum (9; m eps = eps and + 0 z are exact), each at most 2^-24 times a term that
        M = |x| + g |u| bounds.  3 + 9 = 12, and 2 more units for the second-order terms and for evaluating M on one of the two trajectories: 14.
    E_u: pos = 0.3 x - 0.7 s + 0.05 roll(x) takes 6 roundings (t / 1000, three products, two sums) of terms bounded by
    P = 0.3 |x| + 0.7 s + 0.05 |x|; neg 7 of terms bounded by Q = 0.25 |x| + 0.5 s + 0.04 |x| + 0.1; the guidance d = pos - neg, b = 3 d,
    u = pos + b three more of terms bounded by 4 P + 3 Q; u = 4 pos - 3 neg carries the first two with weights 4 and 3:
    E_u <= 2^-24 (4 * 6 P + 3 * 7 Q + 3 (4 P + 3 Q)) = 2^-24 (36 P + 30 Q).
    A difference D between the two states grows through F by at most (1 + |dt| L), L = 4 (0.3 + 0.05) + 3 (0.25 + 0.04) = 2.27 the
    Lipschitz constant of u in the maximum norm.  So, in the maximum norm, with |x|, |u| the maxima over the state,
        D_0 = 0,   D_{i+1} <= (1 + |dt_i| L) D_i + 2 g_i E_u,i + 14 * 2^-24 (|x_i| + g_i |u_i|)."""
    a, b = torch.from_numpy(g13['roll_h0_x_t']).double(), torch.from_numpy(g12['roll_plain_x_t']).double()
    assert a.shape == b.shape and torch.equal(torch.from_numpy(g13['roll_noise']), torch.from_numpy(g12['roll_noise']))
    assert float(g13['roll_scale']) == float(g12['roll_scale']) == 4.0 and float(g13['roll_shift']) == float(g12['roll_shift'])
    sigmas, _ = TS.euler_sigmas(5, shift=float(g13['roll_shift']))
    sig = sigmas.double()
    states = [torch.from_numpy(g12['roll_noise']).double()] + list(b[:-1])
    L, D = 2.27, 0.0
    for i, x in enumerate(states):
        s, s_to = sig[i].item(), sig[i + 1].item()
        g = (1 - s_to) * s + s_to * (1 - s)
        pos, neg = _stub(x, s, False), _stub(x, s, True)
        X, U = x.abs().max().item(), (pos + (pos - neg) * 3.0).abs().max().item()
        P, Q = 0.35 * X + 0.7 * s, 0.29 * X + 0.5 * s + 0.1
        D = (1 + abs(s_to - s) * L) * D + 2 * g * EPS * (36 * P + 30 * Q) + 14 * EPS * (X + g * U)
        diff = (a[i] - b[i]).abs().max().item()
        print(f'step {i}: max |x_sde(h=0) - x_ode| {diff:.3e}  derived bound {D:.3e}')
        assert diff <= D, (i, diff, D)
    # (a rounding bound: orders of magnitude below the distance by which the h = 1 roll departs from the ODE's)
    assert (torch.from_numpy(g13['roll_h1_plain_x_t']).double() - b).abs().max().item() > 100 * D


def test_test_cfg_helper():
    from arcflow_amd import FlowSDEScheduler, TeacherSampler, sampler_kwargs_from_test_cfg
    ts = types.SimpleNamespace(shift=3.2, use_dynamic_shifting=False, base_seq_len=256, max_seq_len=4096, base_logshift=0.5, max_logshift=1.15)
    cfg = dict(sampler='FlowSDE', sampler_kwargs=dict(h='inf'), num_timesteps=28, guidance_interval=[0, 875], orthogonal_guidance=True)
    kw = sampler_kwargs_from_test_cfg(cfg, ts)
    assert kw == dict(sampler='FlowSDE', h='inf', num_steps=28, num_train_timesteps=1000, guidance_interval=[0.0, 875.0], orthogonal_guidance=True,
                      shift=3.2, use_dynamic_shifting=False, base_seq_len=256, max_seq_len=4096, base_logshift=0.5, max_logshift=1.15)
    assert cfg['sampler_kwargs'] == dict(h='inf')                         # the caller's dict is left alone
    sampler = TeacherSampler(types.SimpleNamespace(teacher_head=True), guidance_scale=4.0, **kw)
    assert isinstance(sampler.scheduler, FlowSDEScheduler) and sampler.scheduler.config.h == 'inf' and sampler.scheduler.config.shift == 3.2
    assert sampler.num_steps == 28 and sampler.orthogonal_guidance and sampler.guidance_interval == (0.0, 875.0)
    # precedence of the shift family: sampler_kwargs, then the test_cfg itself, then the timestep sampler (gaussian_flow.py:167-171)
    kw = sampler_kwargs_from_test_cfg(dict(sampler='FlowSDE', sampler_kwargs=dict(shift=2.0), shift=5.0, base_seq_len=1024), ts)
    assert kw['shift'] == 2.0 and kw['base_seq_len'] == 1024 and kw['max_seq_len'] == 4096 and 'h' not in kw and 'guidance_interval' not in kw
    assert kw['num_steps'] == 1000                                        # the reference's default: the model's num_timesteps
    # missing shift keys: from the timestep sampler -- an object, its config dict (absent keys at its class defaults), or nothing
    dyn = dict(type='ContinuousTimeStepSampler', shift=3.0, use_dynamic_shifting=True, max_logshift=2.0)
    kw = sampler_kwargs_from_test_cfg(dict(num_timesteps=4), dyn)
    assert kw['sampler'] == 'FlowEulerODE' and kw['shift'] == 3.0 and kw['use_dynamic_shifting'] is True and kw['max_logshift'] == 2.0
    assert kw['base_logshift'] == 0.5 and kw['base_seq_len'] == 256 and kw['num_steps'] == 4
    assert sampler_kwargs_from_test_cfg(None)['shift'] == 1.0 and sampler_kwargs_from_test_cfg({}, None, 500)['num_train_timesteps'] == 500
    with pytest.raises(ValueError, match='FlowAdapter'):
        sampler_kwargs_from_test_cfg(dict(sampler='FlowAdapter', sampler_kwargs=dict(base_scheduler='UniPCMultistep')), ts)
    with pytest.raises(ValueError):
        sampler_kwargs_from_test_cfg(dict(sampler='FlowMatchEulerDiscrete'), ts)
    with pytest.raises(TypeError):
        sampler_kwargs_from_test_cfg(dict(sampler='FlowEulerODE', sampler_kwargs=dict(h=1.0)), ts)


def test_sampler_constructor_checks():
    from arcflow_amd import FlowEulerODEScheduler, FlowSDEScheduler, TeacherSampler
    eng = types.SimpleNamespace(teacher_head=True)
    with pytest.raises(ValueError, match='FlowEulerODE.*FlowSDE'):
        TeacherSampler(eng, 4, sampler='nope')
    with pytest.raises(TypeError):
        TeacherSampler(eng, 4, h=1.0)                                      # h with the ODE sampler: the scheduler's own TypeError
    with pytest.raises(TypeError):
        TeacherSampler(eng, 4, sampler='FlowEulerODE', h=1.0)
    assert type(TeacherSampler(eng, 4).scheduler) is FlowEulerODEScheduler and TeacherSampler(eng, 4).sampler == 'FlowEulerODE'
    s = TeacherSampler(eng, 4, sampler='FlowSDE', h=2.0, shift=3.2)
    assert type(s.scheduler) is FlowSDEScheduler and s.scheduler.config.h == 2.0 and s.sampler == 'FlowSDE'
    assert TeacherSampler(eng, 4, sampler='FlowSDE').scheduler.config.h == 1.0
    sig, active = s.schedule(4, 4)
    assert sig.numel() == 5 and active == [False] * 4
    with pytest.raises(ValueError):                                        # step_noise of the wrong shape is refused before anything runs
        s(dict(hp=4, wp=4), torch.zeros(1, 16, 64), step_noise=torch.zeros(3, 1, 16, 64))


def test_cabi_argument_checks_without_a_device():
    """Null pointers, n % 64 != 0 and misaligned operands are refused with AFX_E_INVALID before any launch; an empty batch is a no-op."""
    from arcflow_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    p = [C.c_void_p(4096 * k) for k in range(1, 12)]
    step = lib.afx_teacher_sde_step

    def args(**over):
        a = dict(x=p[0], pos=p[1], neg=p[2], noise=p[3], sigma=p[4], sigma_to=p[5], m=p[6], c_noise=p[7], coef=p[8], scale=4.0,
                 x_out=p[9], x_out_bf16=p[10], batch=1, n=64, max_blocks=0, stream=None)
        a.update(over)
        return list(a.values())
    assert step(*args(x=None)) == -1
    assert b'null argument to afx_teacher_sde_step' in lib.afx_last_error()
    for missing in ('pos', 'sigma', 'sigma_to', 'm', 'c_noise', 'x_out', 'x_out_bf16'):           # neg, noise and coef are optional
        assert step(*args(**{missing: None})) == -1, missing
        assert b'afx_teacher_sde_step' in lib.afx_last_error()
    for n in (100, 0, 8, 63, 65, 64 * 5 + 8, -64):
        assert step(*args(n=n)) == -1, n
        assert b'afx_teacher_sde_step' in lib.afx_last_error() and b'multiple of 64' in lib.afx_last_error()
    assert step(*args(noise=C.c_void_p(4096 * 4 + 4))) == -1                                       # noise not 16-byte aligned
    assert b'afx_teacher_sde_step' in lib.afx_last_error() and b'16-byte aligned' in lib.afx_last_error()
    assert step(*args(x=C.c_void_p(4096 + 4))) == -1 and step(*args(neg=C.c_void_p(4096 * 3 + 8))) == -1
    assert step(*args(batch=-1)) == -1 and step(*args(max_blocks=-1)) == -1
    assert step(*args(batch=0)) == 0                                                               # an empty batch launches nothing
    assert step(*args(batch=0, neg=None, noise=None, coef=None)) == 0


def test_ops_refuse_cpu_tensors():
    from arcflow_amd import _lib, ops
    x = torch.zeros(1, 1, 64)
    one = torch.ones(1)
    with pytest.raises(_lib.ArcflowHipError):
        ops.teacher_sde_step(x, x.bfloat16(), None, x, one, one, one, one)
