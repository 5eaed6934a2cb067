"""The fp64 reference, bounds and acceptance rules of tests/optimizer_ref.py, checked on the CPU before any kernel is held to them:
the reference equals torch.optim.AdamW in float64; correct fp32 arithmetic (the restatement oracle/adamw8bit_ref.py and a plain fp32
evaluation of the other formulas) passes every criterion of test_hip_optimizer_fp64.py on that test's own inputs and seeds with no
exception; and each of a list of plausible wrong kernels is rejected by the same criteria on the same inputs."""
import numpy as np
import pytest
import torch

import optimizer_ref as O
from arcflow_amd.ops import dynamic_map
from oracle import adamw8bit_ref as R

Q1, Q2 = dynamic_map(True), dynamic_map(False)
H = O.ADAMW8_HYPER


def _t(x):
    return torch.tensor(O.f32(x), dtype=torch.float32)


# ---- fp32 evaluations, right and wrong ------------------------------------------------------------------------------------------------
def fp32_adamw(p, g, m, v, lr, step, betas, eps, wd, gscale, variant=None):
    """One AdamW step in fp32 torch arithmetic, the formulas as written; `variant` plants one error."""
    b1, b2 = O.f32(betas[0]), O.f32(betas[1])
    t = step + {'bias_step_minus_1': -1, 'bias_step_plus_1': 1}.get(variant, 0)
    bc1, bc2 = torch.tensor(1.0 - b1 ** t, dtype=torch.float32), torch.tensor(1.0 - b2 ** t, dtype=torch.float32)
    gi = g * _t(gscale)
    if variant == 'l2_weight_decay':
        gi = gi + _t(wd) * p
    m1 = _t(b1) * m + (1 - _t(b1)) * gi
    gsq = g * g * _t(gscale) if variant == 'gscale_not_squared' else gi * gi
    v1 = _t(b2) * v + (1 - _t(b2)) * gsq
    den = (v1 / bc2 + _t(eps)).sqrt() if variant == 'eps_inside_sqrt' else (v1 / bc2).sqrt() + _t(eps)
    p1 = p if variant == 'l2_weight_decay' else p * (1 - _t(lr) * _t(wd))
    return p1 - _t(lr) * (m1 / bc1) / den, m1, v1


def _quantize(x, qmap, group=O.BLOCK, upper=False):
    """Block-wise codes + absmax.  group = 64: every wave normalises by its own maximum and the block stores wave 0's (the four-wave fold
    left out); upper: the upper neighbour of the nearest code is stored, for every element not already at 255."""
    n = x.numel()
    nb = (n + O.BLOCK - 1) // O.BLOCK
    pad = torch.zeros(nb * O.BLOCK)
    pad[:n] = x
    am = pad.view(-1, group).abs().amax(1)
    rep = am.repeat_interleave(group)
    normed = torch.where(rep > 0, pad / rep.clamp(min=1e-45), torch.zeros_like(pad))
    idx = torch.searchsorted(qmap, normed.contiguous()).clamp(max=255)
    lower = (idx - 1).clamp(min=0)
    codes = torch.where((idx > 0) & ((normed - qmap[lower]) <= (qmap[idx] - normed)), lower, idx)
    if upper:
        codes = (codes + 1).clamp(max=255)
    return codes[:n].to(torch.uint8), am.view(nb, -1)[:, 0].contiguous()


def fp32_adamw8bit(p, g, c1, c2, a1, a2, lr, step, betas, eps, wd, gscale, variant=None):
    m0, v0 = R.dequantize_blockwise(c1, a1, Q1), R.dequantize_blockwise(c2, a2, Q2)
    p1, m1, v1 = fp32_adamw(p, g, m0, v0, lr, step, betas, eps, wd, gscale, variant)
    group = 64 if variant == 'absmax_over_64' else O.BLOCK
    n1, s1 = _quantize(m1, Q1, group, variant == 'upper_code')
    n2, s2 = _quantize(v1, Q2, group, variant == 'upper_code')
    if variant == 'param_from_requantised':
        bc1, bc2 = (torch.tensor(bc, dtype=torch.float32) for bc in O.bias_corrections(betas, step))
        mq, vq = R.dequantize_blockwise(n1, s1, Q1), R.dequantize_blockwise(n2, s2, Q2)
        p1 = p * (1 - _t(lr) * _t(wd)) - _t(lr) * (mq / bc1) / ((vq / bc2).sqrt() + _t(eps))
    return p1, n1, n2, s1, s2


def _run8(n, kind, stepper):
    """Four steps of `stepper` from the zero state through every criterion; the state continues from the stepper's own output.
    -> worst ratios."""
    p, grads, expect = O.adamw8bit_case(n, kind)
    nb = (n + O.BLOCK - 1) // O.BLOCK
    c1 = c2 = torch.zeros(n, dtype=torch.uint8)
    a1 = a2 = torch.zeros(nb)
    worst = {}
    for t in range(4):
        got = stepper(p, grads[t], c1, c2, a1, a2, t + 1)
        r = O.check_adamw8bit_step(p, grads[t], c1, c2, a1, a2, Q1, Q2, got, step=t + 1, expect=expect[t], what=f'{kind} n={n}', **H)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
        p, c1, c2, a1, a2 = got
    return worst


# ---- the reference itself -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wd,gscale', [(0.0, 1.0), (0.01, 1.0), (0.01, 0.5)])
def test_adamw_ref_equals_torch_adamw_in_float64(wd, gscale):
    gen = torch.Generator().manual_seed(3)
    n, lr, betas, eps = 1000, O.f32(1e-3), (O.f32(0.9), O.f32(0.95)), O.f32(1e-8)
    p = torch.randn(n, generator=gen, dtype=torch.float64)
    pr = torch.nn.Parameter(p.clone())
    opt = torch.optim.AdamW([pr], lr=lr, betas=betas, eps=eps, weight_decay=O.f32(wd))
    m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(1, 6):
        g = torch.randn(n, generator=gen, dtype=torch.float64) * torch.logspace(-4, 0, n, dtype=torch.float64)
        pr.grad = g * O.f32(gscale)
        opt.step()
        p, m, v = O.adamw_ref(p, g, m, v, lr, step, betas, eps, wd, gscale)
        st = opt.state[pr]
        for name, a, b in (('p', p, pr.data), ('m', m, st['exp_avg']), ('v', v, st['exp_avg_sq'])):
            assert bool(((a - b).abs() <= 1e-12 * b.abs()).all()), (name, step, ((a - b).abs() / b.abs()).max().item())


def test_bias_correction_term():
    """The cancellation term of the host's fp32 1 - powf(beta, t): largest at t = 1, gone once beta^t underflows; and numpy's fp32 evaluation
    lies inside it at every step the tests use."""
    for beta, amp in ((0.9, 9.0), (0.95, 19.0)):
        assert O.bias_correction_err(beta, 1) / O.U == pytest.approx(2 * amp + 1, rel=1e-5)
        errs = [O.bias_correction_err(beta, t) for t in (1, 2, 3, 4, 100000)]
        assert errs == sorted(errs, reverse=True) and errs[-1] == 0.0
        assert O.bias_corrections((beta, beta), 100000) == (1.0, 1.0)
        for t in (1, 2, 3, 4, 100000):
            bc32 = float(np.float32(1.0) - np.power(np.float32(beta), np.float32(t), dtype=np.float32))
            bc = O.bias_corrections((beta, beta), t)[0]
            assert abs(bc32 - bc) <= O.bias_correction_err(beta, t) * bc


def test_code_book_facts():
    s, u = dynamic_map(True), dynamic_map(False)
    assert float(s[0]) == pytest.approx(-0.99297, abs=1e-5) and not bool((s == -1.0).any())
    assert s[127] == 0.0 and u[0] == 0.0 and s[255] == 1.0 and u[255] == 1.0
    # the smallest non-zero codes: what 'dynamic_range' relies on for its zero codes
    assert float(s[128]) == pytest.approx(5.5e-7, rel=1e-5) and float(u[1]) == pytest.approx(3.25e-7, rel=1e-5)


def test_code_is_nearest_rule():
    x = torch.tensor([0.0, 0.5, -1.0, 1.0, 0.30], dtype=torch.float64)
    near = torch.tensor([127, 0, 0, 255, 0])
    near[1] = int((Q1.double() - 0.5).abs().argmin())
    near[4] = int((Q1.double() - 0.30).abs().argmin())
    zero = torch.zeros(5, dtype=torch.float64)
    assert bool(O.code_is_nearest(near, x, zero, Q1)[0].all())
    # the neighbour of the nearest code fails with err_x = 0 and passes once err_x covers half the difference of the two distances
    up = (near + 1).clamp(max=255)
    ok = O.code_is_nearest(up, x, zero, Q1)[0]
    assert ok.tolist() == [False, False, False, True, False]
    excess = (Q1.double()[up] - x).abs() - (Q1.double()[near] - x).abs()
    assert bool(O.code_is_nearest(up, x, excess / 2 * (1 + 1e-9), Q1)[0].all())
    assert not bool(O.code_is_nearest(up, x, excess / 2 * (1 - 1e-9), Q1)[0][[0, 1, 2, 4]].any())


# ---- correct fp32 arithmetic passes, with no exception --------------------------------------------------------------------------------
@pytest.mark.parametrize('n,kind', O.adamw8bit_cases())
def test_fp32_restatement_passes_every_8bit_criterion(n, kind):
    hy = (O.f32(H['lr']), (O.f32(H['betas'][0]), O.f32(H['betas'][1])), O.f32(H['eps']), O.f32(H['wd']), O.f32(H['gscale']))

    def oracle(p, g, c1, c2, a1, a2, step):
        return R.adamw8bit_step(p, g, c1, c2, a1, a2, Q1, Q2, hy[0], step, hy[1], hy[2], hy[3], hy[4])
    worst = _run8(n, kind, oracle)
    print(f'restatement n={n} {kind}: worst ratios', {k: round(v, 3) for k, v in worst.items()})
    # ... and so does this file's own fp32 evaluation, which the wrong variants are planted in (it squares g' before the product with 1 - b2:
    # another order of the same six roundings)
    _run8(n, kind, lambda p, g, c1, c2, a1, a2, step: fp32_adamw8bit(p, g, c1, c2, a1, a2, step=step, **H))


@pytest.mark.parametrize('n', O.ADAMW_N)
@pytest.mark.parametrize('wd,gscale', O.ADAMW_WD_GSCALE)
def test_fp32_adamw_passes_every_criterion(n, wd, gscale):
    p, m, v, grads, zero = O.adamw_case(n)
    for t, step in enumerate(O.ADAMW_STEPS):
        got = fp32_adamw(p, grads[t], m, v, 1e-3, step, (0.9, 0.95), 1e-8, wd, gscale)
        O.check_adamw_step(p, grads[t], m, v, *got, 1e-3, step, wd=wd, gscale=gscale, zero=zero)
        p, m, v = got


# ---- wrong kernels are rejected -------------------------------------------------------------------------------------------------------
ADAMW_VARIANTS = ['bias_step_minus_1', 'bias_step_plus_1', 'l2_weight_decay', 'eps_inside_sqrt', 'gscale_not_squared']


@pytest.mark.parametrize('variant', ADAMW_VARIANTS)
def test_wrong_adamw_is_rejected(variant):
    p, m, v, grads, zero = O.adamw_case(4133)
    with pytest.raises(AssertionError):
        got = fp32_adamw(p, grads[1], m, v, 1e-3, 2, (0.9, 0.95), 1e-8, 0.01, 0.5, variant)
        O.check_adamw_step(p, grads[1], m, v, *got, 1e-3, 2, wd=0.01, gscale=0.5, zero=zero)


@pytest.mark.parametrize('n', [257, 4096])
@pytest.mark.parametrize('variant', ADAMW_VARIANTS + ['absmax_over_64', 'upper_code', 'param_from_requantised'])
def test_wrong_adamw8bit_is_rejected(n, variant):
    for kind in ('logspace', 'placed_max'):
        with pytest.raises(AssertionError):
            _run8(n, kind, lambda p, g, c1, c2, a1, a2, step: fp32_adamw8bit(p, g, c1, c2, a1, a2, step=step, variant=variant, **H))


def test_upper_code_is_rejected_at_every_element_below_255():
    """Not just somewhere: every element whose nearest code is not 255 fails code_is_nearest when its upper neighbour is stored."""
    p, grads, _ = O.adamw8bit_case(4096, 'logspace')
    z8, za = torch.zeros(4096, dtype=torch.uint8), torch.zeros(16)
    good = fp32_adamw8bit(p, grads[0], z8, z8, za, za, step=1, **H)
    r = O.adamw8bit_ref(p, grads[0], z8, z8, za, za, Q1, Q2, step=1, **H)
    em, ev = O.moment_bounds(r['m0'], r['v0'], grads[0], H['betas'], H['gscale'], deq=1)
    for codes, x, e, am, q in ((good[1], r['x1'], em, r['amax1'], Q1), (good[2], r['x2'], ev, r['amax2'], Q2)):
        ex = O.norm_bound(x, e, am, O._block_max(e), q) * O.U
        below = codes < 255
        ok = O.code_is_nearest((codes.long() + 1).clamp(max=255), x, ex, q)[0]
        assert not bool(ok[below].any()) and bool(ok[~below].all())


def _roll_inputs():
    gen = torch.Generator().manual_seed(11)
    a, b = torch.randn(4, 257, 64, generator=gen), torch.randn(4, 257, 64, generator=gen) + 1.0
    return a, b


def test_ema_euler_cfg_fp32_pass_and_wrong_variants_fail():
    a, b = _roll_inputs()
    for beta in O.EMA_BETAS:
        O.within(b + (a - b) * _t(beta), O.ema_ref(a, b, beta), O.ema_bound(a, b, beta), f'ema beta={beta}')
    with pytest.raises(AssertionError):       # beta and 1 - beta swapped
        O.within(b + (a - b) * (1 - _t(0.93)), O.ema_ref(a, b, 0.93), O.ema_bound(a, b, 0.93), 'ema swapped')
    sa, sb = O.EULER_SIGMAS
    out = a + b * (sb - sa)[:, None, None]
    O.within(out, O.euler_ref(a, b, sa, sb), O.euler_bound(a, b, sa, sb), 'euler')
    with pytest.raises(AssertionError):       # the per-sample sigmas in reversed sample order
        O.within(out, O.euler_ref(a, b, sa.flip(0), sb.flip(0)), O.euler_bound(a, b, sa, sb), 'euler flipped')
    for scale in O.CFG_SCALES:
        out = a + (a - b) * (_t(scale) - 1)
        O.within(out, O.cfg_ref(a, b, scale), O.cfg_bound(a, b, scale), f'cfg scale={scale}')
        if scale != 1:                        # cfg_combine has one scale for all samples: the reversed sample order is that of the negative branch
            with pytest.raises(AssertionError):
                O.within(out, O.cfg_ref(a, b.flip(0), scale), O.cfg_bound(a, b, scale), 'cfg flipped')
