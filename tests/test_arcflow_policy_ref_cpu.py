"""The fp64 reference of the ArcFlow policy kernels (tests/arcflow_policy_ref.py) checked on the CPU, so that the GPU test built on it
(tests/test_hip_arcflow_policy_fp64.py) means something:

  * its forward agrees with the fp32 oracle (oracle/arcflow_ref.py) to fp32 accuracy at the shipped mixture shape;
  * its analytic gradients equal torch fp64 autograd of its own forward;
  * every mutation moves it by more than twice the bound on >= 1 % of the elements of every output the mutation targets, in every case the
    GPU test runs (the condition under which "the kernel's output rejects the mutation" cannot pass by the mutation being too small to see);
  * no gamma d_step lies where the fp32 and the fp64 clamp decisions could differ.
"""
import pytest
import torch

import arcflow_policy_ref as R

NAMES = ('d_means', 'd_logw', 'd_logg')


@pytest.mark.parametrize('B,N', [(2, 5), (3, 43)])
def test_forward_agrees_with_the_fp32_oracle(B, N):
    """momentum_step_packed (scalar sigmas: sample by sample) and policy_velocity (latent layout: through unpack_mixture / pack_latents) in
    fp32 differ from the fp64 reference by their own fp32 roundings, which the kernel's bound covers with a factor 2 to spare."""
    from oracle import arcflow_ref as O
    K, ch, pp = 16, 64, 4
    for name in ('scalar', 'per_sample', 'scalar_src_eq_start'):
        c = R.make_case(B, N, K, ch, pp, False, name)
        ref, bound = R.forward(c, 'step')
        sig = c['sig']
        for b in range(B):
            o = O.momentum_step_packed(c['x'][b:b + 1], c['means'][b:b + 1], c['logw'][b:b + 1], c['logg'][b:b + 1],
                                       float(sig[b, 0]), float(sig[b, 1]), float(sig[b, 2]), eps=R.EPS)
            err = (o.double() - ref[b:b + 1]).abs()
            assert (err <= 2 * bound[b:b + 1]).all(), (name, b, (err / bound[b:b + 1]).max().item())
        ref, bound = R.forward(c, 'velocity')
        ml, lwl, lgl = O.unpack_mixture(c['means'], c['logw'], c['logg'], 1, N)
        o = O.pack_latents(O.policy_velocity(ml, lwl, lgl, sig[:, 0], sig[:, 1]))
        err = (o.double() - ref).abs()
        assert (err <= 2 * bound).all(), (name, (err / bound).max().item())


def test_dphi_budget_does_not_follow_the_cancellation():
    """The phi' budget is the closed form's own worst case from |z| = 1 on, where nothing cancels (small, falling for z > 0, growing as
    XM |z| for z < 0), and stays at its |z| = 1 value below, where the closed form's grows as 4 / |z|."""
    z = torch.tensor([1e-4, 1e-3, 1e-2, 0.1, 0.5, 1.0], dtype=torch.float64)
    for sign in (1.0, -1.0):
        budget, closed = R.c_dphi(sign * z), R.kappa(sign * z)
        assert (budget - 2 * z <= R.kappa(sign * 1.0) + 1e-9).all() and budget[-1] - 2 == R.kappa(sign * 1.0)
        assert closed[0] > 1000 * budget[0] and closed[2] > 10 * budget[2]
        big = torch.linspace(1.0, 8.0, 701, dtype=torch.float64)
        assert (R.c_dphi(sign * big) <= R.kappa(sign * 1.0) + (R.XM + 2) * big).all()
        print(f'sign {sign:+.0f}: phi\' budget at |z| <= 1: {R.kappa(sign * 1.0).item():.1f} u + 2 |z|; closed form at |z| = 1e-4, 1e-3, 1e-2, 0.1: '
              + ', '.join(f'{k:.0f}' for k in closed[:4].tolist()) + ' u')


def test_fp64_dphi_series_and_closed_form_meet():
    z = torch.tensor([0.4999999, 0.5, -0.4999999, -0.5, 0.3, -0.3], dtype=torch.float64)
    closed = (torch.exp(z) - torch.expm1(z) / z) / z
    assert ((R.dphi64(z) - closed).abs() <= 1e-14 * closed.abs()).all()
    assert abs(R.dphi64(torch.tensor([1e-9], dtype=torch.float64)).item() - 0.5) < 1e-9


@pytest.mark.parametrize('K,ch,pp', R.BWD_SHAPES)
@pytest.mark.parametrize('B,N', R.TOKENS)
def test_analytic_gradients_equal_fp64_autograd(B, N, K, ch, pp):
    """Normalised by each output's largest magnitude.  Autograd differentiates expm1(z) / z as e^z / z - expm1(z) / z^2, which cancels in
    fp64 the way the kernel's closed form does in fp32: 1e-16 * 4 / |z| = 4e-12 relative on phi' at the planted |z| = 1.1 eps; hence 5e-12
    and not 1e-13."""
    worst = 0.0
    for tag, mode, c in R.cases_bwd(B, N, K, ch, pp):
        (outs, _), auto = R.backward(c, mode), R.forward_autograd_grads(c, mode)
        for name, a, b in zip(NAMES, outs, auto):
            assert torch.isfinite(a).all(), (tag, name)
            scale = a.abs().max().item()
            rel = (a - b).abs().max().item() / scale if scale > 0 else (a - b).abs().max().item()
            worst = max(worst, rel)
            assert rel <= 5e-12, (tag, name, rel)
    print(f'B={B} N={N} K={K} ch={ch} pp={pp}: analytic vs fp64 autograd, worst normalised difference {worst:.2e}')


def _check_mutations(tag, c, mode, kind, base, bound):
    for mut, targets in R.mutations_for(c, mode, kind).items():
        if kind == 'fwd':
            moved = {'out': R.forward(c, mode, mut)[0]}
        else:
            moved = dict(zip(NAMES, R.backward(c, mode, mut)[0]))
        for t in targets:
            frac = R.moved_fraction(moved[t], base[t], bound[t], 2.0)
            assert frac >= 0.01, (tag, mut, t, frac)


@pytest.mark.parametrize('K,ch,pp', R.STEP_SHAPES)
@pytest.mark.parametrize('B,N', R.TOKENS)
def test_forward_mutations_move_the_reference(B, N, K, ch, pp):
    n = 0
    for tag, mode, c in R.cases_fwd(B, N, K, ch, pp):
        m = 'velocity' if mode == 'velocity' else 'step'
        ref, bound = R.forward(c, m)
        assert torch.isfinite(ref).all() and torch.isfinite(bound).all() and (bound >= 0).all(), tag
        _check_mutations(tag, c, m, 'fwd', {'out': ref}, {'out': bound})
        n += len(R.mutations_for(c, m, 'fwd'))
    assert n > 0


@pytest.mark.parametrize('K,ch,pp', R.BWD_SHAPES)
@pytest.mark.parametrize('B,N', R.TOKENS)
def test_backward_mutations_move_the_reference(B, N, K, ch, pp):
    for tag, mode, c in R.cases_bwd(B, N, K, ch, pp):
        outs, bounds = R.backward(c, mode)
        for o, b in zip(outs, bounds):
            assert torch.isfinite(o).all() and torch.isfinite(b).all() and (b >= 0).all(), tag
        _check_mutations(tag, c, mode, 'bwd', dict(zip(NAMES, outs)), dict(zip(NAMES, bounds)))


def test_mutation_lists_leave_out_what_cannot_act():
    """The explicit exclusions: B = 1 for the neighbour mutations, K <= 2 for the gate off-by-one, pp = 1 and pp = ch for the sub-pixel
    index, d_step = 0 for everything but e_0 = 1; and every mutation is exercised somewhere."""
    seen = set()
    for B, N in R.TOKENS:
        for K, ch, pp in R.STEP_SHAPES:
            for tag, mode, c in R.cases_fwd(B, N, K, ch, pp):
                m = R.mutations_for(c, 'velocity' if mode == 'velocity' else 'step', 'fwd')
                seen |= set(m)
                assert not (B == 1 and {'nb_sigma', 'nb_drop'} & set(m)) and not (K <= 2 and 'gate_off_by_one' in m), tag
                assert not (pp == 1 and 'q_div' in m), tag
                if c['sigma_name'] == 'zero_step' and mode != 'velocity':
                    assert set(m) == {'e0_one'}, (tag, m)
        for K, ch, pp in R.BWD_SHAPES:
            for tag, mode, c in R.cases_bwd(B, N, K, ch, pp):
                m = R.mutations_for(c, mode, 'bwd')
                seen |= set(m)
                assert not (B == 1 and {'nb_sigma', 'nb_gscale'} & set(m)) and not (pp == ch and 'q_div' in m), tag
    assert seen == set(R.MUTATIONS), set(R.MUTATIONS) - seen


def test_no_gate_sits_on_the_clamp_edge():
    planted = 0
    for B, N in R.TOKENS:
        for shapes, cases in ((R.STEP_SHAPES, R.cases_fwd), (R.BWD_SHAPES, R.cases_bwd)):
            for K, ch, pp in shapes:
                for tag, mode, c in cases(B, N, K, ch, pp):
                    assert R.z_is_clear_of_eps(c), tag
                    z = R.z_of(c).abs() / R.EPS
                    planted += int(((z > 0.85) & (z < 1.15)).sum())
    assert planted > 100                                    # the planted 0.9 eps and 1.1 eps are there


def test_head_grad_mutation_moves_the_reference():
    for K, ch, lw, ldy in R.HEAD_SHAPES:
        for rows in R.HEAD_ROWS:
            c = R.make_head_case(rows, K, ch, lw, ldy)
            ref, bound = R.head_logw_ref(c)
            assert R.moved_fraction(R.head_logw_ref(c, 'sum_over_q')[0], ref, bound, 2.0) >= 0.01
