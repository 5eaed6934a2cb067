"""Teacher sampling on the CPU: ``FlowEulerODEScheduler`` and the restated sampling loop (tests/teacher_sampler_ref.py) against
fixture G12 (tests/golden/g12_teacher_sampler.npz: the reference's own scheduler and ``GaussianFlow.forward_test`` executed on a
closed-form stub denoiser, tests/golden/make_golden_teacher_sampler.py), and the argument checks of the two new C-ABI entry
points, which return before any launch.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import teacher_sampler_ref as TS

TOL = 2e-6
TABLES = [dict(num_steps=4, shift=1.0), dict(num_steps=7, shift=3.2), dict(num_steps=5, use_dynamic_shifting=True, seq_len=1024),
          dict(num_steps=6, shift=3.2, terminal_sigma=0.02)]


@pytest.fixture(scope='module')
def g12(golden):
    return golden('g12_teacher_sampler')


def _stub(x, sigma, negative):
    """The closed-form denoiser fixture G12 was generated with (t / 1000 = sigma)."""
    if negative:
        return 0.25 * x - 0.5 * sigma + 0.04 * torch.roll(x, 1, dims=-2) + 0.1
    return 0.3 * x - 0.7 * sigma + 0.05 * torch.roll(x, 1, dims=-1)


@pytest.mark.parametrize('i', range(len(TABLES)))
def test_scheduler_tables_match_reference(g12, i):
    from arcflow_amd import FlowEulerODEScheduler
    c = dict(TABLES[i])
    n, seq_len = c.pop('num_steps'), c.pop('seq_len', None)
    sch = FlowEulerODEScheduler(1000, **c)
    ts = sch.set_timesteps(n, seq_len=seq_len)
    assert sch.sigmas.dtype == torch.float32 and sch.sigmas.numel() == n + 1 and float(sch.sigmas[-1]) == 0.0
    ref_s, ref_t = g12[f'tab{i}_sigmas'], g12[f'tab{i}_timesteps']
    print(f'table {i}: max |d sigma| {np.abs(sch.sigmas.numpy() - ref_s).max():.3e}  max |d t| / 1000 {np.abs(ts.numpy() - ref_t).max() / 1000:.3e}')
    assert np.abs(sch.sigmas.numpy() - ref_s).max() <= TOL
    assert np.abs(ts.numpy() - ref_t).max() <= TOL * 1000          # timesteps = sigma * 1000: the same relative bound
    if i == 0:          # shift 1: the table IS the linspace grid, which must be bit-exact
        assert np.array_equal(sch.sigmas.numpy()[:-1], np.linspace(1, 0, n, dtype=np.float32, endpoint=False))
        assert np.array_equal(sch.sigmas.numpy(), ref_s)
    # the helper's own grid is pinned by the same tables
    hs, ht = TS.euler_sigmas(n, seq_len=seq_len, **c)
    assert np.abs(hs.numpy() - ref_s).max() <= TOL and np.abs(ht.numpy() - ref_t).max() <= TOL * 1000


def test_scheduler_from_config_and_errors():
    from arcflow_amd import FlowEulerODEScheduler
    sch = FlowEulerODEScheduler.from_config(dict(num_train_timesteps=1000, shift=3.0, base_shift=0.5, _class_name='x'), shift=3.2)
    assert sch.config.shift == 3.2 and sch.config.terminal_sigma is None and len(sch) == 1000
    assert sch.get_shift(seq_len=4096) == 3.2                         # static shift: seq_len is ignored
    dyn = FlowEulerODEScheduler(use_dynamic_shifting=True)
    assert abs(dyn.get_shift(seq_len=256) - np.exp(0.5)) < 1e-12 and abs(dyn.get_shift(seq_len=4096) - np.exp(1.15)) < 1e-12
    with pytest.raises(TypeError):
        FlowEulerODEScheduler(flow_shift=3.0)
    sch.set_timesteps(3)
    with pytest.raises(ValueError):
        sch.step(torch.zeros(2), 0, torch.zeros(2))
    with pytest.raises(NotImplementedError):
        sch.step(torch.zeros(2), sch.timesteps[0], torch.zeros(2), prediction_type='x0')


def test_scheduler_step_matches_reference(g12):
    from arcflow_amd import FlowEulerODEScheduler
    sch = FlowEulerODEScheduler(1000, shift=3.2)
    sch.set_timesteps(7)
    x = torch.from_numpy(g12['step_sample'])
    worst = 0.0
    for t, u, ref in zip(sch.timesteps, torch.from_numpy(g12['step_model_output']), torch.from_numpy(g12['step_prev_sample'])):
        x = sch.step(u, t, x, return_dict=False)[0]
        worst = max(worst, (x - ref).abs().max().item())
        assert x.dtype == torch.float32
    print(f'step: max |d prev_sample| {worst:.3e}')
    assert worst <= TOL
    assert sch.step_index == 7


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('tag', ['plain', 'ortho', 'interval'])
def test_restated_loop_matches_forward_test(g12, tag, dtype):
    noise = torch.from_numpy(g12['roll_noise'])
    sigmas, _ = TS.euler_sigmas(5, shift=float(g12['roll_shift']))
    trace = {}
    x = TS.sample(_stub, noise, sigmas, guidance_scale=float(g12['roll_scale']),
                  guidance_interval=g12['roll_interval'].tolist() if tag == 'interval' else None,
                  orthogonal=tag == 'ortho', dtype=dtype, trace=trace)
    ref = torch.from_numpy(g12[f'roll_{tag}_x_t']).double()
    got = torch.stack(trace['x_t']).double()
    assert got.shape == ref.shape and torch.equal(got[-1], x.double())
    excess = ((got - ref).abs() / (1 + ref.abs())).max().item()
    print(f'{tag} {dtype}: max |d x_t| / (1 + |ref|) {excess:.3e}')
    assert excess <= TOL
    # the loop skipped the negative forward on exactly the steps the reference ran without the stacked batch
    assert trace['active'] == g12[f'roll_{tag}_active'].tolist()
    assert trace['negative_calls'] == int(g12[f'roll_{tag}_active'].sum())
    if tag == 'interval':
        assert trace['active'] == [True, True, True, False, False]


def test_orthogonal_bias_is_orthogonal_and_clamped():
    g = torch.Generator().manual_seed(3)
    pos, neg = torch.randn(2, 16, 64, generator=g).double(), torch.randn(2, 16, 64, generator=g).double()
    bias = TS.guidance_bias(pos, neg, 4.0, orthogonal=True)
    assert (bias * pos).flatten(1).sum(1).abs().max().item() < 1e-9
    pos[1] = 0                                   # the 1e-6 clamp: no division by zero, the bias of that sample is the plain one
    bias = TS.guidance_bias(pos, neg, 4.0, orthogonal=True)
    assert torch.isfinite(bias).all() and torch.equal(bias[1], (pos[1] - neg[1]) * 3.0)


def test_cabi_argument_checks_without_a_device():
    """Null pointers, n % 64 != 0 and misaligned operands are refused with AFX_E_INVALID before any launch."""
    from arcflow_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    p = [C.c_void_p(4096 * k) for k in range(1, 9)]
    step = lib.afx_teacher_euler_step
    assert step(None, None, None, None, None, None, 4.0, None, None, 1, 64, 0, None) == -1
    assert b'afx_teacher_euler_step' in lib.afx_last_error()
    for missing in (0, 1, 3, 4, 7, 8):           # x, pos, sigma, sigma_to, x_out, x_out_bf16 (neg and coef are optional)
        a = [p[0], p[1], p[2], p[3], p[4], p[5], 4.0, p[6], p[7], 1, 64, 0, None]
        a[missing] = None
        assert step(*a) == -1, missing
    for n in (0, 8, 63, 65, 64 * 5 + 8, -64):
        assert step(p[0], p[1], p[2], p[3], p[4], p[5], 4.0, p[6], p[7], 1, n, 0, None) == -1, n
    assert b'multiple of 64' in lib.afx_last_error()
    assert step(C.c_void_p(4096 + 4), p[1], p[2], p[3], p[4], p[5], 4.0, p[6], p[7], 1, 64, 0, None) == -1      # x not 16-byte aligned
    assert step(p[0], p[1], C.c_void_p(8192 + 8), p[3], p[4], p[5], 4.0, p[6], p[7], 1, 64, 0, None) == -1      # neg not 16-byte aligned
    assert step(p[0], p[1], p[2], p[3], p[4], p[5], 4.0, p[6], p[7], -1, 64, 0, None) == -1
    assert step(p[0], p[1], p[2], p[3], p[4], p[5], 4.0, p[6], p[7], 1, 64, -1, None) == -1
    assert step(p[0], p[1], None, p[3], p[4], None, 4.0, p[6], p[7], 0, 64, 0, None) == 0                         # an empty batch launches nothing
    coef = lib.afx_cfg_ortho_coef
    assert lib.afx_cfg_ortho_ws_bytes(3, 320) == 3 * 16                      # one work-group per sample: one (sum bias pos, sum pos pos) pair
    assert lib.afx_cfg_ortho_ws_bytes(2, 64 * 1031) == 2 * 9 * 16            # ceil(65984 / 8192) = 9 work-groups per sample
    assert lib.afx_cfg_ortho_ws_bytes(1, 64 * 8192 * 2) == 64 * 16           # capped at 64
    assert lib.afx_cfg_ortho_ws_bytes(1, 100) == -1 and lib.afx_cfg_ortho_ws_bytes(-1, 64) == -1
    assert coef(None, None, 4.0, None, None, 0, 1, 64, None) == -1
    for missing in (0, 1, 3, 4):
        a = [p[0], p[1], 4.0, p[2], p[3], 16, 1, 64, None]
        a[missing] = None
        assert coef(*a) == -1, missing
    assert coef(p[0], p[1], 4.0, p[2], p[3], 16, 1, 100, None) == -1
    assert coef(p[0], p[1], 4.0, p[2], p[3], 8, 1, 64, None) == -1           # workspace too small
    assert b'workspace' in lib.afx_last_error()
    assert coef(p[0], p[1], 4.0, p[2], C.c_void_p(4096 + 4), 16, 1, 64, None) == -1
    assert coef(p[0], p[1], 4.0, p[2], p[3], 0, 0, 64, None) == 0


def test_ops_refuse_cpu_tensors():
    from arcflow_amd import _lib, ops
    x = torch.zeros(1, 1, 64)
    with pytest.raises(_lib.ArcflowHipError):
        ops.teacher_euler_step(x, x.bfloat16(), None, torch.ones(1), torch.zeros(1))
    with pytest.raises(_lib.ArcflowHipError):
        ops.cfg_ortho_coef(x.bfloat16(), x.bfloat16(), 4.0)
