"""The UniPC multistep teacher sampler without a device: ``FlowUniPCScheduler`` (arcflow_amd/schedule.py) against the loop-form fp64
reference tests/unipc_ref.py, its sigma tables against the reference's own ``FlowAdapterScheduler`` (fixture G14,
tests/golden/make_golden_flow_adapter.py), the name handling (``'UniPC'`` / ``'FlowAdapter'`` / ``allow_adapter``) and the C-ABI refusals of
``afx_teacher_unipc_step`` (they return before any launch).

What is and is not pinned.  The adapter's own part -- timesteps, sigmas, the clamp to 1 - eps, the keywords it builds its base scheduler
with -- is pinned by G14, produced by executing the reference class.  The multistep arithmetic is diffusers' ``UniPCMultistepScheduler``
as recalled; tests/unipc_ref.py writes it in the scheduler's loop form and the tests below hold the flattened weights, the last step,
exactness on a constant clean-sample prediction and the convergence order against that: self-consistency and the mathematics of the
solver, not parity with diffusers.
"""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from tests import unipc_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ORDERS, TYPES = (1, 2, 3), ('bh1', 'bh2')


def _scheduler(n, **kw):
    from arcflow_amd import FlowUniPCScheduler
    sch = FlowUniPCScheduler(1000, **kw)
    sch.set_timesteps(n)
    return sch


def _tables(sch):
    return sch.sigmas.double().numpy(), sch.base_sigmas.double().numpy()


def apply_coefficients(sch, model, x, begin=0):
    """The roll from FlowUniPCScheduler.coefficients alone, in fp64: what ``step()`` and the fused kernel evaluate in fp32.
    -> (x_end, every step's result, every step's m_t)."""
    st = sch.sigmas.double().numpy()
    x = np.asarray(x, dtype=np.float64)
    hist, last, traj, mts = [], None, [], []
    for i in range(begin, sch.num_inference_steps):
        co = sch.coefficients(i, begin)
        m_t = x - co.sigma * model(x, st[i], i)
        if co.corrector is None:
            x_c = x
        else:
            cl, cm, *ch = co.corrector
            x_c = cl * last + cm * m_t + sum(ch[k] * hist[-(k + 1)] for k in range(co.corrector_order))
        px, pm, *ph = co.predictor
        x = px * x_c + pm * m_t + sum(ph[k] * hist[-(k + 1)] for k in range(co.predictor_order - 1))
        hist, last = (hist + [m_t])[-sch.config.solver_order:], x_c
        traj.append(x)
        mts.append(m_t)
    return x, traj, mts


def _nonlinear(x, s, i):
    """A velocity field that is neither linear nor local, so that every history term matters."""
    return 0.7 * np.tanh(x) - 0.3 * s + 0.1 * np.roll(x, 1)


@pytest.fixture(scope='module')
def start():
    return np.random.default_rng(0).standard_normal(256)


@pytest.mark.parametrize('shift', [1.0, 3.2])
@pytest.mark.parametrize('n', [1, 2, 3, 5, 8])
@pytest.mark.parametrize('solver_type', TYPES)
@pytest.mark.parametrize('order', ORDERS)
def test_flattened_coefficients_reproduce_the_loop_reference(start, order, solver_type, n, shift):
    """1e-12 relative (of the largest state) on every step's result; n < order runs the warm-up and lower_order_final paths together."""
    sch = _scheduler(n, solver_order=order, solver_type=solver_type, shift=shift)
    st, sg = _tables(sch)
    ref, ref_traj = R.sample(_nonlinear, start, st, sg, order, solver_type, trajectory=True)
    got, traj, _ = apply_coefficients(sch, _nonlinear, start)
    assert len(traj) == len(ref_traj) == n
    for i, (a, b) in enumerate(zip(traj, ref_traj)):
        rel = np.abs(a - b).max() / np.abs(b).max()
        assert rel <= 1e-12, (i, rel)
    # the orders the two walked through: warm-up 1, 2, .. solver_order, then down again to 1 on the last step
    want = [min(order, n - i, i + 1) for i in range(n)]
    assert [sch.coefficients(i).predictor_order for i in range(n)] == want
    assert [sch.coefficients(i).corrector_order for i in range(n)] == [0] + want[:-1]
    assert sch.coefficients(0).corrector is None and all(sch.coefficients(i).corrector is not None for i in range(1, n))


@pytest.mark.parametrize('solver_type', TYPES)
@pytest.mark.parametrize('order', ORDERS)
def test_a_suffix_roll_starts_on_an_empty_history(start, order, solver_type):
    """strength < 1: the roll over steps begin .. n - 1 has no corrector and order 1 at ``begin`` -- the reference loop started there."""
    sch = _scheduler(7, solver_order=order, solver_type=solver_type, shift=3.2)
    st, sg = _tables(sch)
    for begin in (1, 3, 6):
        ref = R.sample(_nonlinear, start, st, sg, order, solver_type, begin=begin)
        got, traj, _ = apply_coefficients(sch, _nonlinear, start, begin=begin)
        assert len(traj) == 7 - begin and np.abs(got - ref).max() / np.abs(ref).max() <= 1e-12
        assert sch.coefficients(begin, begin).corrector is None and sch.coefficients(begin, begin).predictor_order == 1


@pytest.mark.parametrize('shift', [1.0, 3.2])
@pytest.mark.parametrize('n', [1, 2, 3, 5, 8])
@pytest.mark.parametrize('solver_type', TYPES)
@pytest.mark.parametrize('order', ORDERS)
def test_last_step_lands_on_the_clean_prediction_and_nothing_is_nan(start, order, solver_type, n, shift):
    sch = _scheduler(n, solver_order=order, solver_type=solver_type, shift=shift)
    for i in range(n):
        co = sch.coefficients(i)
        row = co.row()
        assert len(row) == 10 and all(np.isfinite(v) for v in row), (i, row)
        assert 0.0 < co.sigma <= 1 - 1e-4
    assert sch.coefficients(n - 1).predictor == (0.0, 1.0, 0.0, 0.0)
    got, traj, mts = apply_coefficients(sch, _nonlinear, start)
    assert np.array_equal(got, mts[-1])                        # bit for bit: 0 x_c + 1 m_t
    # and through step() in fp32: the last prev_sample is x - sigma u of the last call, bit for bit
    x = torch.from_numpy(start).float()
    for i, (t, s) in enumerate(zip(sch.timesteps, sch.sigmas)):
        u = torch.from_numpy(_nonlinear(x.double().numpy(), float(s), i)).float()
        m_t = x - torch.tensor(sch.coefficients(i).sigma, dtype=torch.float32) * u
        x = sch.step(u, t, x).prev_sample
    assert torch.equal(x, m_t) and torch.isfinite(x).all()


@pytest.mark.parametrize('shift', [1.0, 3.2])
@pytest.mark.parametrize('solver_type', TYPES)
@pytest.mark.parametrize('order', ORDERS)
def test_constant_clean_prediction_is_integrated_exactly(start, order, solver_type, shift):
    """u = (x - c) / sigma (the solver's sigma): m_t = c on every step, and every order then moves x along the straight line
    x_i = alpha_i c + s_i e with e = (x_0 - alpha_0 c) / s_0 fixed -- on every step, not only at the end (where x = m_t = c)."""
    c = 1.3
    for n in (1, 2, 3, 5, 8):
        sch = _scheduler(n, solver_order=order, solver_type=solver_type, shift=shift)
        st, sg = _tables(sch)

        def model(x, s, i):
            return (x - c) / sg[i]
        e = (start - (1 - sg[0]) * c) / sg[0]
        for roll in (R.sample(model, start, st, sg, order, solver_type, trajectory=True)[1], apply_coefficients(sch, model, start)[1]):
            for i, x in enumerate(roll):
                want = (1 - sg[i + 1]) * c + sg[i + 1] * e
                assert np.abs(x - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (n, i)
            assert np.abs(roll[-1] - c).max() <= 1e-12


MU, SD = 0.7, 1.0


def _gaussian_flow(x, s, i):
    """Data N(MU, SD^2) per element, x_s = (1 - s) x0 + s eps: u = (x - E[x0 | x]) / s, whose ODE ends on MU + SD eps."""
    a = 1.0 - s
    e0 = MU + a * SD * SD / (a * a * SD * SD + s * s) * (x - a * MU)
    return (x - e0) / s


@pytest.fixture(scope='module')
def convergence(start):
    """max |x_end - exact| of the fp64 loop reference and of Euler on the unshifted schedule, computed once: {n: {'euler' | (order, type): err}}."""
    exact = MU + SD * start
    table = {}
    for n in (8, 16, 32, 64):
        st, sg = _tables(_scheduler(n, shift=1.0))
        row = {'euler': np.abs(R.euler(_gaussian_flow, start, st) - exact).max()}
        for order in ORDERS:
            for solver_type in TYPES:
                row[(order, solver_type)] = np.abs(R.sample(_gaussian_flow, start, st, sg, order, solver_type) - exact).max()
        table[n] = row
        print(f'n={n}: euler {row["euler"]:.2e}  ' + '  '.join(f'o{o} {t} {row[(o, t)]:.2e}' for o in ORDERS for t in TYPES))
    return table


def test_order_one_error_at_least_thirds_with_each_doubling(convergence):
    for n in (8, 16, 32):
        ratio = convergence[n][(1, 'bh2')] / convergence[2 * n][(1, 'bh2')]
        print(f'order-1 bh2: err({n}) / err({2 * n}) = {ratio:.2f}')
        assert ratio >= 3.0, (n, ratio)


def test_every_variant_beats_euler_at_the_same_number_of_steps(convergence):
    for n in (16, 32, 64):
        for key, err in convergence[n].items():
            if key != 'euler':
                assert err < convergence[n]['euler'], (n, key, err, convergence[n]['euler'])


def test_flattened_rolls_converge_like_the_reference(start, convergence):
    """The scheduler's own weights on the same problem: the reference's error, to 1e-12 of the state."""
    exact = MU + SD * start
    for n in (16, 64):
        for order in ORDERS:
            sch = _scheduler(n, solver_order=order, shift=1.0)
            err = np.abs(apply_coefficients(sch, _gaussian_flow, start)[0] - exact).max()
            assert abs(err - convergence[n][(order, 'bh2')]) <= 1e-11, (n, order)


# ------------------------------------------------------------------------------------------------ tables (fixture G14)
TABLES = [dict(num_steps=4, shift=1.0), dict(num_steps=7, shift=3.2), dict(num_steps=5, use_dynamic_shifting=True, seq_len=1024),
          dict(num_steps=6, shift=3.2, terminal_sigma=0.02), dict(num_steps=40, shift=12.0, eps=5e-3)]


def test_tables_are_the_reference_adapters():
    from arcflow_amd import FlowEulerODEScheduler, FlowUniPCScheduler
    g14 = np.load(os.path.join(GOLDEN, 'g14_flow_adapter_tables.npz'))
    for k, c in enumerate(TABLES):
        kw = {a: v for a, v in c.items() if a not in ('num_steps', 'seq_len')}
        sch = FlowUniPCScheduler(1000, **kw)
        ts = sch.set_timesteps(c['num_steps'], seq_len=c.get('seq_len'))
        assert float(g14[f'tab{k}_eps']) == sch.config.eps
        assert torch.equal(ts, torch.from_numpy(g14[f'tab{k}_timesteps'])) and torch.equal(sch.timesteps, ts), k
        assert torch.equal(sch.sigmas, torch.from_numpy(g14[f'tab{k}_sigmas'])), k
        assert torch.equal(sch.base_sigmas, torch.from_numpy(g14[f'tab{k}_base_sigmas'])), k
        assert sch.base_sigmas.dtype == torch.float32 and float(sch.base_sigmas.max()) == float(np.float32(1 - sch.config.eps))
        # the same formula as the Euler scheduler's tables
        eu = FlowEulerODEScheduler(1000, **{a: v for a, v in kw.items() if a != 'eps'})
        eu.set_timesteps(c['num_steps'], seq_len=c.get('seq_len'))
        assert torch.equal(eu.sigmas, sch.sigmas) and torch.equal(eu.timesteps, sch.timesteps)
    # what the adapter asks of its base scheduler: the defaults FlowUniPCScheduler is written for
    assert sorted(g14['base_kwargs'].tolist()) == ['final_sigmas_type=zero', 'lower_order_final=True', 'num_train_timesteps=1000',
                                                   'prediction_type=flow_prediction', 'use_flow_sigmas=True']
    # sigmas that coincide after the clamp (table 4: three entries at 1 - eps) cannot be stepped between: refused, not a NaN
    with pytest.raises(ValueError, match='decreasing'):
        sch.coefficients(1)


def test_scheduler_constructor_and_state():
    from arcflow_amd import FlowEulerODEScheduler, FlowUniPCScheduler
    assert FlowUniPCScheduler._DEFAULTS == dict(FlowEulerODEScheduler._DEFAULTS, solver_order=2, solver_type='bh2', eps=1e-4)
    for bad in (dict(solver_order=0), dict(solver_order=4), dict(solver_order=2.5), dict(solver_order=True), dict(solver_type='bh3'),
                dict(solver_type='logrho'), dict(eps=0.0)):
        with pytest.raises(ValueError):
            FlowUniPCScheduler(1000, **bad)
    with pytest.raises(TypeError):
        FlowUniPCScheduler(1000, h=1.0)
    sch = FlowUniPCScheduler.from_config(dict(shift=3.2, solver_order=3, base_image_seq_len=256))
    assert sch.config.solver_order == 3 and sch.config.shift == 3.2
    sch.set_timesteps(4)
    x = torch.randn(2, 8, generator=torch.Generator().manual_seed(0))
    with pytest.raises(NotImplementedError):
        sch.step(x, sch.timesteps[0], x, prediction_type='x0')
    a = [x]
    for t in sch.timesteps:
        a.append(sch.step(0.3 * a[-1] - 0.2, t, a[-1]).prev_sample)
    assert sch.lower_order_nums == 3 and len(sch.model_outputs) == 3 and sch.this_order == 1 and sch.step_index == 4
    sch.set_timesteps(4)                                       # resets the multistep state: the same roll again, bit for bit
    assert sch.lower_order_nums == 0 and sch.model_outputs == [] and sch.last_sample is None and sch.this_order is None
    b = [x]
    for t in sch.timesteps:
        b.append(sch.step(0.3 * b[-1] - 0.2, t, b[-1]).prev_sample)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    # step() is the flattened form in fp32: within fp32 rounding of the fp64 loop reference
    st, sg = _tables(sch)
    ref = R.sample(lambda v, s, i: 0.3 * v - 0.2, x.double().numpy(), st, sg, 3, 'bh2')
    assert np.abs(b[-1].double().numpy() - ref).max() <= 1e-5
    # a roll begun in the middle (set_begin_index): the history is empty there
    sch.set_timesteps(4)
    sch.set_begin_index(2)
    y = sch.step(0.3 * x - 0.2, sch.timesteps[2], x).prev_sample
    ref = R.sample(lambda v, s, i: 0.3 * v - 0.2, x.double().numpy(), st, sg, 3, 'bh2', begin=2, trajectory=True)[1][0]
    assert np.abs(y.double().numpy() - ref).max() <= 1e-5


# ------------------------------------------------------------------------------------------------ names
TS = types.SimpleNamespace(shift=3.2, use_dynamic_shifting=False, base_seq_len=256, max_seq_len=4096, base_logshift=0.5, max_logshift=1.15)
SHIFT = dict(shift=3.2, use_dynamic_shifting=False, base_seq_len=256, max_seq_len=4096, base_logshift=0.5, max_logshift=1.15)


def test_allow_adapter_maps_the_reference_name():
    from arcflow_amd import FlowUniPCScheduler, TeacherSampler, sampler_kwargs_from_test_cfg
    cfg = dict(sampler='FlowAdapter', sampler_kwargs=dict(base_scheduler='UniPCMultistep', solver_order=3, solver_type='bh1', eps=1e-3), num_timesteps=12)
    # the default refuses it exactly as before
    with pytest.raises(ValueError, match='FlowAdapter'):
        sampler_kwargs_from_test_cfg(cfg, TS)
    with pytest.raises(ValueError, match='FlowAdapter'):
        sampler_kwargs_from_test_cfg(cfg, TS, allow_adapter=False)
    kw = sampler_kwargs_from_test_cfg(cfg, TS, allow_adapter=True)
    assert kw == dict(sampler='UniPC', solver_order=3, solver_type='bh1', eps=1e-3, num_steps=12, num_train_timesteps=1000, orthogonal_guidance=False, **SHIFT)
    assert cfg['sampler_kwargs']['base_scheduler'] == 'UniPCMultistep'                # the caller's dict is left alone
    s = TeacherSampler(types.SimpleNamespace(teacher_head=True), guidance_scale=4.0, **kw)
    assert type(s.scheduler) is FlowUniPCScheduler and s.sampler == 'UniPC' and s.num_steps == 12
    assert (s.scheduler.config.solver_order, s.scheduler.config.solver_type, s.scheduler.config.eps, s.scheduler.config.shift) == (3, 'bh1', 1e-3, 3.2)
    # base_scheduler absent: the adapter's default, UniPCMultistep, at diffusers' defaults
    kw = sampler_kwargs_from_test_cfg(dict(sampler='FlowAdapter', shift=2.0), TS, allow_adapter=True)
    assert kw['sampler'] == 'UniPC' and kw['shift'] == 2.0 and 'solver_order' not in kw and 'base_scheduler' not in kw
    assert TeacherSampler(types.SimpleNamespace(teacher_head=True), **kw).scheduler.config.solver_order == 2
    # every other family the adapter wraps is refused by name
    for base in ('DPMSolverMultistep', 'DPMSolverSinglestep', 'DEISMultistep', 'SASolver', 'EulerDiscrete', 'EulerAncestralDiscrete'):
        with pytest.raises(ValueError, match=base):
            sampler_kwargs_from_test_cfg(dict(sampler='FlowAdapter', sampler_kwargs=dict(base_scheduler=base)), TS, allow_adapter=True)
    with pytest.raises(TypeError):                             # a diffusers keyword this solver does not take
        sampler_kwargs_from_test_cfg(dict(sampler='FlowAdapter', sampler_kwargs=dict(predict_x0=False)), TS, allow_adapter=True)
    # the other names do not change with the flag
    for flag in (False, True):
        assert sampler_kwargs_from_test_cfg(dict(sampler='FlowSDE', sampler_kwargs=dict(h=2.0)), TS, allow_adapter=flag)['sampler'] == 'FlowSDE'
        assert sampler_kwargs_from_test_cfg({}, TS, allow_adapter=flag)['sampler'] == 'FlowEulerODE'
        with pytest.raises(ValueError):
            sampler_kwargs_from_test_cfg(dict(sampler='FlowMatchEulerDiscrete'), TS, allow_adapter=flag)


def test_sampler_names_and_the_mask_refusal():
    from arcflow_amd import FlowUniPCScheduler, TeacherSampler
    from arcflow_amd.teacher import SAMPLERS
    eng = types.SimpleNamespace(teacher_head=True)
    assert SAMPLERS['UniPC'] is FlowUniPCScheduler and 'FlowAdapter' not in SAMPLERS
    with pytest.raises(ValueError, match='FlowAdapter.*UniPC'):          # still refused; the message says where to go
        TeacherSampler(eng, 4, sampler='FlowAdapter')
    s = TeacherSampler(eng, 4, sampler='UniPC', solver_order=3, solver_type='bh1', shift=3.2)
    assert type(s.scheduler) is FlowUniPCScheduler and s.scheduler.config.solver_order == 3 and s.scheduler.config.solver_type == 'bh1'
    assert TeacherSampler(eng, 4, sampler='UniPC').scheduler.config.solver_order == 2
    with pytest.raises(ValueError):
        TeacherSampler(eng, 4, sampler='UniPC', solver_order=4)
    with pytest.raises(TypeError):
        TeacherSampler(eng, 4, sampler='FlowEulerODE', solver_order=2)       # the solver's keywords belong to UniPC
    sig, active = s.schedule(4, 4)
    assert sig.numel() == 5 and float(sig[0]) == 1.0 and active == [False] * 4     # the denoiser still sees the unclamped sigma
    cond, z = dict(hp=4, wp=4), torch.zeros(1, 16, 64)
    with pytest.raises(ValueError, match='mask.*UniPC'):                  # refused before anything runs
        s(cond, z, x0=z, mask=torch.ones(1, 16, 4), strength=0.5)
    with pytest.raises(ValueError, match='mask.*UniPC'):
        s(cond, z, mask=torch.ones(1, 16, 4))


# ------------------------------------------------------------------------------------------------ C ABI
def test_cabi_refusals_without_a_device():
    """NULL required operands, n not a positive multiple of 64, misaligned pointers and overlapping outputs are refused with AFX_E_INVALID by
    entry name before any launch (that the three documented aliases are accepted is shown on the device, tests/test_hip_teacher_unipc_step_fp64.py)."""
    from arcflow_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    step = lib.afx_teacher_unipc_step
    p = {k: C.c_void_p(0x100000 * (i + 1)) for i, k in enumerate(
        ('x', 'pos', 'neg', 'w', 'last', 'h1', 'h2', 'h3', 'coef', 'x_out', 'x_out_bf16', 'last_out', 'hist_out'))}

    def args(**over):
        a = dict(x=p['x'], pos=p['pos'], neg=p['neg'], w=p['w'], last=p['last'], h1=p['h1'], h2=p['h2'], h3=p['h3'], coef=p['coef'], scale=4.0,
                 x_out=p['x_out'], x_out_bf16=p['x_out_bf16'], last_out=p['last_out'], hist_out=p['hist_out'], batch=0, n=64, max_blocks=0, stream=None)
        a.update(over)
        return list(a.values())

    def refused(*words, **over):
        assert step(*args(**over)) == -1, over
        msg = lib.afx_last_error()
        assert b'afx_teacher_unipc_step' in msg and all(w in msg for w in words), (over, msg)
    assert step(*args()) == 0                                              # an empty batch launches nothing
    assert step(*args(neg=None, last=None, h1=None, h2=None, h3=None, coef=None)) == 0
    for missing in ('x', 'pos', 'w', 'x_out', 'x_out_bf16', 'last_out', 'hist_out'):
        refused(b'null argument', **{missing: None})
    refused(b'needs h1', h1=None)                                          # a corrector without its m[-1]
    refused(b'needs h1', last=None, h1=None, h3=None)                      # h2 without h1
    refused(b'h3 needs h2', h2=None)
    for n in (100, 0, 8, 63, 65, 64 * 5 + 8, -64):
        refused(b'multiple of 64', n=n)
    refused(batch=-1)
    refused(max_blocks=-1)
    for name in ('x', 'pos', 'neg', 'last', 'h1', 'h2', 'h3', 'x_out', 'x_out_bf16', 'last_out', 'hist_out'):
        refused(b'16-byte aligned', **{name: C.c_void_p(p[name].value + 8)})
    # overlaps (batch 2, n 64: 512 B of fp32, 256 B of bf16 per operand)
    live = dict(batch=2, n=64)
    for out, inp in (('x_out', 'last'), ('x_out', 'h1'), ('x_out', 'pos'), ('x_out', 'w'), ('x_out_bf16', 'x'), ('x_out_bf16', 'neg'), ('last_out', 'x'),
                     ('last_out', 'h2'), ('last_out', 'coef'), ('hist_out', 'x'), ('hist_out', 'last'), ('hist_out', 'pos'), ('x_out', 'hist_out'),
                     ('last_out', 'x_out'), ('hist_out', 'last_out'), ('x_out_bf16', 'hist_out')):
        refused(b'overlaps', **live, **{out: p[inp]})
    for out, inp in (('x_out', 'x'), ('last_out', 'last'), ('hist_out', 'h1')):          # a partial overlap with the permitted alias is still one
        refused(b'overlaps', **live, **{out: C.c_void_p(p[inp].value + 256)})


def test_ops_refuse_cpu_tensors_and_wrong_operands():
    from arcflow_amd import _lib, ops
    x = torch.zeros(1, 1, 64)
    w = torch.zeros(10, 1)
    with pytest.raises(_lib.ArcflowHipError):
        ops.teacher_unipc_step(x, x.bfloat16(), None, w, None, [], x.clone(), x.clone())
    with pytest.raises(ValueError, match='at most three'):
        ops.teacher_unipc_step(x, x.bfloat16(), None, w, None, [x, x, x, x], x.clone(), x.clone())
