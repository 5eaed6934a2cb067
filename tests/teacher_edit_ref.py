"""References of teacher image editing (``afx_teacher_edit_step`` / ``afx_teacher_sde_edit_step``, test helper, not a test module): an fp64
statement of the fused step written out in one piece, the composition it is defined by (the step of tests/teacher_sampler_ref.py /
tests/sde_sampler_ref.py followed by the blend of tests/edit_ref.py), the per-element bound, the inputs the kernel test runs on, and MUTANTS --
deliberately wrong references which the comparison of tests/test_hip_teacher_edit_step_fp64.py must reject on those inputs
(tests/test_teacher_edit_cpu.py checks without a GPU that each moves the reference by more than twice the bound on at least 1 % of the elements).

The fused step, per element e of token tok of sample b (packed channel e = c*4 + ph*2 + pw, so the latent pixel of the patch is e & 3):

    u     = pos [+ (pos - neg)(scale - 1)] [- coef[b] pos]
    x'    = x + u (sigma_to - sigma)                                                               Euler
    x'    = (1 - sigma_to)(x - sigma u) + sigma_to (m (x + (1 - sigma) u) + c_noise z)             FlowSDE, z the step's draw
    known = (1 - sigma_to) x0 + sigma_to noise0            (no noise term when noise0 is NULL)
    out   = mk x' + (1 - mk) known,    mk = mask[b, tok, e & 3]

The semantics are this project's own (after diffusers' img2img / inpaint pipelines as recalled); no golden fixture pins them.

Bound against fp64 from the same inputs.  The kernel computes x' exactly as the plain step kernels do, so x' is within the step tests' bounds
of its exact value (tests/test_hip_teacher_step_fp64.py: (7 | 9) eps (|x| + |dt| U) =: E_ode, the 9 with the orthogonal term;
tests/test_hip_teacher_sde_step_fp64.py: (16 | 18) eps M =: E_sde), with

    U = |pos| + |scale - 1| (|pos| + |neg|) + |coef pos|,        X_ode = |x| + |dt| U,
    X_sde = M = (1 - sigma_to)(|x| + sigma U) + sigma_to (m (|x| + (1 - sigma) U) + c_noise |z|)

bounding |x'| itself.  The blend then rounds om = fl(1 - sigma_to), p = fl(om x0), known = fl(sigma_to noise0 + p) (one fma), q = fl(1 - mk),
r = fl(q known), out = fl(mk x' + r) (one fma): six roundings, each of relative size eps = 2^-24 on a term whose magnitude, carried to the
output, is at most X + |x0| + |noise0| because mk and sigma_to are in [0, 1] -- tests/edit_ref.py's bound with the step's X in the place of |x|:
<= 6 eps (X + |x0| + |noise0|) to first order, 8 eps with room for the second-order terms (and for |fl(x')| exceeding X by a rounding).  The
step's own error reaches the output through the factor mk <= 1.  Together

    |err| <= E_step + 8 * 2^-24 * (X + |x0| + |noise0|).
"""
import functools

import numpy as np
import torch

EPS = 2.0 ** -24
SCALE = 4.0                                                   # scale - 1 is exact
STEPS = [(1.0, 2), (2.0, 3), ('inf', 4)]                      # (h, step index of the 7-step shift-3.2 schedule) of samples 0, 1, 2: all interior
MUTANTS = ('known_at_sigma', 'swap_m', 'subpixel_shift', 'sde_draw_as_noise0')          # the last one exists with FlowSDE only
MASKS = ('random', 'zeros', 'ones', 'checker')


@functools.lru_cache(maxsize=None)
def coefficients():
    """[4, 3] fp32: rows sigma, sigma_to, m, c_noise of FlowSDEScheduler; one column per sample (the Euler step uses the first two rows)."""
    from arcflow_amd import FlowSDEScheduler
    cols = []
    for h, i in STEPS:
        sch = FlowSDEScheduler(1000, h=h, shift=3.2)
        sch.set_timesteps(7)
        cols.append(torch.stack(sch.coefficients(i)))
    co = torch.stack(cols, 1)
    assert (co[0] < 1).all() and (co[1] > 0).all() and (co[0] != co[1]).all()
    return co


def make_mask(kind, B, n_tok, g):
    """[B, n_tok, 4] fp32: 'random' in [0, 1] (differs across sub-pixels, tokens and samples), 'zeros', 'ones', or 'checker': exact 0 / 1
    alternating over the four patch positions, the pattern inverted on every other token."""
    if kind == 'random':
        return torch.rand(B, n_tok, 4, generator=g)
    if kind == 'zeros':
        return torch.zeros(B, n_tok, 4)
    if kind == 'ones':
        return torch.ones(B, n_tok, 4)
    assert kind == 'checker'
    base = torch.tensor([0.0, 1.0, 1.0, 0.0])
    odd = (torch.arange(n_tok) % 2 == 1)[None, :, None]
    return torch.where(odd, 1.0 - base, base).expand(B, n_tok, 4).contiguous()


@functools.lru_cache(maxsize=None)
def make_case(B, n_tok):
    """Inputs (CPU) of one shape, computed once and shared by every test on it: x, z, x0, noise0 [B, n_tok, 64] fp32, pos / neg bf16 (drawn as
    the step tests draw them), per-sample sigma, sigma_to, m, c_noise, coef, and the four masks."""
    g = torch.Generator().manual_seed(500 + 31 * B + n_tok)
    shape = (B, n_tok, 64)
    x = torch.randn(shape, generator=g)
    pos = torch.randn(shape, generator=g).bfloat16()
    neg = (0.6 * pos.float() + 0.8 * torch.randn(shape, generator=g)).bfloat16()
    z = torch.randn(shape, generator=g)
    x0 = torch.randn(shape, generator=g) * 0.8
    noise0 = torch.randn(shape, generator=g)
    co = coefficients()[:, :B].contiguous()
    p, q = pos.double().flatten(1), neg.double().flatten(1)
    coef = (((p - q) * (SCALE - 1) * p).sum(1) / (p * p).sum(1).clamp(min=p.shape[1] * 1e-6)).float()
    c = dict(x=x, pos=pos, neg=neg, z=z, x0=x0, noise0=noise0, sigma=co[0].clone(), sigma_to=co[1].clone(), m=co[2].clone(),
             c_noise=co[3].clone(), coef=coef)
    for kind in MASKS:
        c['mask_' + kind] = make_mask(kind, B, n_tok, g)
    return c


def _scalars(c):
    return (c[k].double()[:, None, None] for k in ('sigma', 'sigma_to', 'm', 'c_noise', 'coef'))


def velocity(c, use_neg, use_coef):
    """fp64 guided velocity from the bf16 pos / neg and the fp32 coef."""
    p, q = c['pos'].double(), c['neg'].double()
    cf = c['coef'].double()[:, None, None]
    u = p.clone()
    if use_neg:
        u = p + (p - q) * (SCALE - 1)
    if use_coef:
        u = u - cf * p
    return u


def fused_ref(c, sde, use_neg, use_coef, mask, use_noise0=True, use_z=True, mutate=None):
    """fp64 fused step, written out in one piece -> [B, n_tok, 64] float64.  mask [B, n_tok, 4] or None (out = x')."""
    x, z, x0, n0 = c['x'].double(), c['z'].double(), c['x0'].double(), c['noise0'].double()
    sig, sig_to, m, cn, _ = _scalars(c)
    u = velocity(c, use_neg, use_coef)
    if sde:
        draw = z if use_z else torch.zeros_like(z)
        xp = (1 - sig_to) * (x - sig * u) + sig_to * (m * (x + (1 - sig) * u) + cn * draw)
    else:
        xp = x + u * (sig_to - sig)
    if mask is None:
        return xp
    at = sig if mutate == 'known_at_sigma' else sig_to
    known = (1 - at) * x0
    if use_noise0:
        known = known + at * (z if mutate == 'sde_draw_as_noise0' else n0)
    e = torch.arange(64)
    mk = mask.double()[:, :, (e >> 4) if mutate == 'subpixel_shift' else (e & 3)]
    if mutate == 'swap_m':
        mk = 1 - mk
    return mk * xp + (1 - mk) * known


def composed_ref(c, sde, use_neg, use_coef, mask, use_noise0=True, use_z=True):
    """The definition by composition: the step of the existing step references, then tests/edit_ref.py's blend of its result."""
    import edit_ref as ER
    from tests import sde_sampler_ref as SR
    from tests import teacher_sampler_ref as TS
    x, z = c['x'].double(), c['z'].double()
    sig, sig_to, m, cn, _ = _scalars(c)
    u = velocity(c, use_neg, use_coef)
    xp = SR.sde_step(x, u, sig, sig_to, m, cn, z if use_z else torch.zeros_like(z)) if sde else TS.euler_step(x, u, sig, sig_to)
    if mask is None:
        return xp
    out = ER.blend_ref(xp.numpy(), c['x0'].numpy(), c['noise0'].numpy(), mask.numpy(), c['sigma_to'].numpy(), noise_is_null=not use_noise0)
    return torch.from_numpy(out)


def bound(c, sde, use_neg, use_coef, use_noise0=True, use_z=True):
    """The per-element bound of the module docstring -> [B, n_tok, 64] float64."""
    x, z, p, q = c['x'].double().abs(), c['z'].double().abs(), c['pos'].double().abs(), c['neg'].double().abs()
    s, s_to, m, cn, cf = _scalars(c)
    U = p + ((SCALE - 1) * (p + q) if use_neg else 0) + ((cf.abs() * p) if use_coef else 0)
    if sde:
        X = (1 - s_to) * (x + s * U) + s_to * (m * (x + (1 - s) * U) + (cn * z if use_z else 0))
        E = (18 if use_coef else 16) * EPS * X
    else:
        X = x + (s_to - s).abs() * U
        E = (9 if use_coef else 7) * EPS * X
    return E + 8 * EPS * (X + c['x0'].double().abs() + (c['noise0'].double().abs() if use_noise0 else 0))


def mutants(sde, use_noise0, use_z=True):
    """The mutants that exist for a variant: the SDE draw can stand in for noise0 only where both are read."""
    return [m for m in MUTANTS if m != 'sde_draw_as_noise0' or (sde and use_noise0 and use_z)]


def bf16_rne(x32: torch.Tensor) -> torch.Tensor:
    """int16 bit pattern of the round-to-nearest-even bf16 of fp32 values (tests/edit_ref.py's integer statement of it)."""
    import edit_ref as ER
    return torch.from_numpy(ER.bf16_bits(x32.numpy()).view(np.int16)).view(x32.shape)
