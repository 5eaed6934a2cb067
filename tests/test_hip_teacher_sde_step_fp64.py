"""``afx_teacher_sde_step`` (true-CFG combine + FlowSDEScheduler.step + bf16 copy, one launch) against fp64, element by element, modelled on
tests/test_hip_teacher_step_fp64.py (same shapes, same inputs, plus the step's draw z ~ N(0, 1) in fp32).

Coefficients.  Every sample gets its own (sigma, sigma_to, m, c_noise) from a real schedule (FlowSDEScheduler, 7 steps, shift 3.2): sample 0
an interior step at h = 1, sample 1 an interior step at h = 2, sample 2 an interior step at h = 'inf' (m = 0, c_noise = 1).

Bound.  The fp64 reference is evaluated from the SAME inputs (bf16 pos / neg, fp32 x, z, sigma, sigma_to, m, c_noise, coef; scale = 4 so that
scale - 1 is exact).  With eps = 2^-24 (half an ulp, fp32 round-to-nearest), U the ODE test's bound on |u|,

    U = |pos| + |scale - 1| (|pos| + |neg|) + |coef pos|,
    M = (1 - sigma_to) (|x| + sigma U) + sigma_to (m (|x| + (1 - sigma) U) + c_noise |z|),

the kernel forms u with the ODE kernel's three roundings (d = fl(pos - neg), b = fl(d (scale - 1)), u = fl(pos + b)) and then computes
    a = fl(1 - sigma),  a' = fl(1 - sigma_to),  s = fl(sigma u),  x0 = fl(x - s),  t = fl(a u),  e = fl(x + t),  p = fl(m e),  q = fl(c_noise z),
    r = fl(p + q),  v = fl(a' x0),  w = fl(sigma_to r),  x' = fl(v + w):
twelve more.  Each perturbs x' by at most eps times the magnitude of the term it rounds, carried to the output through the factors that follow
it, and every such product is one of the summands of M or a part of one:
    the three of u: eps U ((1 - sigma_to) sigma + sigma_to m (1 - sigma));   a: eps (1 - sigma) U m sigma_to;   a': eps (1 - sigma_to) |x0|;
    s, x0: eps (1 - sigma_to) (|x| + sigma U);   t, e, p: eps sigma_to m (|x| + (1 - sigma) U);   q: eps sigma_to c_noise |z|;
    r, w: eps sigma_to (m |e| + c_noise |z|);   v: eps (1 - sigma_to) |x0|;   x': eps |x'| <= eps M.
So |err| <= 15 eps M to first order; one more unit covers the second-order terms: |err| <= 16 * 2^-24 * M.  The orthogonal path adds
c = fl(coef pos) and u' = fl(u - c), two more roundings of terms U already carries: |err| <= 18 * 2^-24 * M.  (Where hipcc contracts a
multiply-add into an fma, a rounding disappears; without neg the kernel skips d, b and u; without noise q and r: the bounds stay upper bounds.)

The bf16 output must be bit-equal to round-to-nearest-even of the kernel's own fp32 output.

h = 0.  With m = 1, c_noise = 0 the step is the Euler step in real arithmetic, so the kernel's output and afx_teacher_euler_step's on the same
inputs differ by at most the sum of the two kernels' bounds (16 / 18 eps M here, 7 / 9 eps M_ode there).

Every mutated reference (m and c_noise swapped, sigma for sigma_to in the outer blend, the neighbour sample's coefficients, the noise term
dropped, alpha for sigma in x0) must fail the same check on at least 1 % of the elements; that each moves the fp64 reference by more than
twice the bound on at least 1 % of the elements is asserted on the CPU side first (test_mutations_move_the_reference_cpu_side needs no
device), so the GPU assertion cannot pass by a mutation being too small to see.
"""
import functools

import pytest
import torch

EPS = 2.0 ** -24
SCALE = 4.0
GUARD = 64            # sentinel elements in front of and behind every output (keeps 16-byte alignment for fp32 and bf16)
SHAPES = [(3, 64 * 5), (1, 64), (2, 64 * 1031)]       # small with per-sample coefficients; a single chunk row; ragged, several blocks
VARIANTS = [(False, False), (True, False), (True, True)]          # (neg, coef): no neg, neg, neg + coef
STEPS = [(1.0, 2), (2.0, 3), ('inf', 4)]              # (h, step index of the 7-step shift-3.2 schedule) of samples 0, 1, 2: all interior


@functools.lru_cache(maxsize=None)
def _coefficients():
    """[4, 3] fp32: rows sigma, sigma_to, m, c_noise; one column per sample."""
    from arcflow_amd import FlowSDEScheduler
    cols = []
    for h, i in STEPS:
        sch = FlowSDEScheduler(1000, h=h, shift=3.2)
        sch.set_timesteps(7)
        cols.append(torch.stack(sch.coefficients(i)))
    co = torch.stack(cols, 1)
    assert (co[0] < 1).all() and (co[1] > 0).all() and co[2, 2] == 0 and co[3, 2] == 1 and (co[2, :2] > 0).all() and (co[3, :2] > 0).all()
    return co


@functools.lru_cache(maxsize=None)
def _case(B, n):
    """Inputs (CPU) of one shape, computed once and shared by every test on that shape (x, pos, neg, coef as the ODE step's test draws them)."""
    g = torch.Generator().manual_seed(100 + B * 7 + n)
    x = torch.randn(B, n, generator=g)
    pos = torch.randn(B, n, generator=g).bfloat16()
    neg = (0.6 * pos.float() + 0.8 * torch.randn(B, n, generator=g)).bfloat16()        # comparable magnitude, correlated like two prompts
    z = torch.randn(B, n, generator=g)
    co = _coefficients()[:, :B].contiguous()
    p, q = pos.double(), neg.double()
    coef = (((p - q) * (SCALE - 1) * p).sum(1) / (p * p).sum(1).clamp(min=n * 1e-6)).float()
    return dict(x=x, pos=pos, neg=neg, z=z, sigma=co[0].clone(), sigma_to=co[1].clone(), m=co[2].clone(), c_noise=co[3].clone(), coef=coef)


def _ref(c, use_neg, use_coef, use_noise, mutate=None, ode=False):
    """fp64 step from the case's inputs -> (reference, bound per element).  ode: m = 1, c_noise = 0 (the h = 0 coefficients)."""
    x, p, q, z = c['x'].double(), c['pos'].double(), c['neg'].double(), c['z'].double()
    sig, sig_to, m, cn, cf = (c[k].double()[:, None] for k in ('sigma', 'sigma_to', 'm', 'c_noise', 'coef'))
    if ode:
        m, cn = torch.ones_like(m), torch.zeros_like(cn)
    if not use_noise:
        z = torch.zeros_like(z)
    M_m, M_cn = m, cn
    if mutate == 'swap_m_c':
        m, cn = cn, m
    if mutate == 'neighbour':
        sig, sig_to, m, cn = (t.roll(1, 0) for t in (sig, sig_to, m, cn))
    if mutate == 'no_noise':
        z = torch.zeros_like(z)
    sm1 = SCALE - 1
    u = p.clone()
    if use_neg:
        u = p + (p - q) * sm1
    if use_coef:
        u = u - cf * p
    x0 = x - ((1 - sig) if mutate == 'alpha_x0' else sig) * u
    e = x + (1 - sig) * u
    outer = sig if mutate == 'sigma_outer' else sig_to
    ref = (1 - outer) * x0 + outer * (m * e + cn * z)
    s, s_to = c['sigma'].double()[:, None], c['sigma_to'].double()[:, None]
    U = p.abs() + (sm1 * (p.abs() + q.abs()) if use_neg else 0) + ((cf * p).abs() if use_coef else 0)
    M = (1 - s_to) * (x.abs() + s * U) + s_to * (M_m * (x.abs() + (1 - s) * U) + M_cn * z.abs())
    return ref, (18 if use_coef else 16) * EPS * M


def _mutations(B, use_noise):
    m = ['swap_m_c', 'sigma_outer', 'alpha_x0']
    if B > 1:
        m.append('neighbour')
    if use_noise:
        m.append('no_noise')
    return m


def _guarded(numel, dtype, sentinel):
    buf = torch.full((numel + 2 * GUARD,), sentinel, dtype=dtype, device='cuda')
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(buf, numel, sentinel):
    return bool((buf[:GUARD] == sentinel).all() and (buf[GUARD + numel:] == sentinel).all())


@pytest.mark.parametrize('use_noise', [True, False], ids=['noise', 'nonoise'])
@pytest.mark.parametrize('use_neg,use_coef', VARIANTS, ids=['nocfg', 'cfg', 'ortho'])
@pytest.mark.parametrize('B,n', SHAPES)
def test_mutations_move_the_reference_cpu_side(B, n, use_neg, use_coef, use_noise):
    """No device: every mutation moves the fp64 reference by more than twice the bound on >= 1 % of the elements (the condition under which
    the GPU test's mutation check means something)."""
    c = _case(B, n)
    ref, bound = _ref(c, use_neg, use_coef, use_noise)
    assert torch.isfinite(ref).all() and (bound > 0).all()
    for mut in _mutations(B, use_noise):
        frac = ((_ref(c, use_neg, use_coef, use_noise, mut)[0] - ref).abs() > 2 * bound).double().mean().item()
        print(f'B={B} n={n} neg={use_neg} coef={use_coef} noise={use_noise} mutation {mut}: moves {100 * frac:.1f} % of the elements by > 2 x bound')
        assert frac >= 0.01, (mut, frac)


@pytest.mark.gpu
@pytest.mark.parametrize('use_noise', [True, False], ids=['noise', 'nonoise'])
@pytest.mark.parametrize('use_neg,use_coef', VARIANTS, ids=['nocfg', 'cfg', 'ortho'])
@pytest.mark.parametrize('B,n', SHAPES)
def test_sde_step_within_fp32_rounding_of_fp64(B, n, use_neg, use_coef, use_noise):
    from arcflow_amd import ops
    c = _case(B, n)
    ref, bound = _ref(c, use_neg, use_coef, use_noise)
    muts = {mut: _ref(c, use_neg, use_coef, use_noise, mut)[0] for mut in _mutations(B, use_noise)}
    for mut, r in muts.items():          # the CPU-side condition again, on the spot
        assert ((r - ref).abs() > 2 * bound).double().mean().item() >= 0.01, mut
    x, pos, neg = c['x'].cuda(), c['pos'].cuda(), c['neg'].cuda() if use_neg else None
    z = c['z'].cuda() if use_noise else None
    sig, sig_to, m, cn = c['sigma'].cuda(), c['sigma_to'].cuda(), c['m'].cuda(), c['c_noise'].cuda()
    coef = c['coef'].cuda() if use_coef else None
    # out of place at the default grid, out of place on a capped grid (several grid-stride passes at the ragged shape: 65 blocks of work on 24),
    # in place, and seven more out-of-place runs -- all into guarded buffers
    runs = {}
    for tag, max_blocks, inplace in [('oop', 0, False), ('oop_capped', 24, False), ('inplace', 0, True)] + [(f'again{k}', 0, False) for k in range(7)]:
        fbuf, fout = _guarded(B * n, torch.float32, -768.0)
        hbuf, hout = _guarded(B * n, torch.bfloat16, -768.0)
        fout, hout = fout.view(B, n), hout.view(B, n)
        if inplace:
            fout.copy_(x)
        o, o16 = ops.teacher_sde_step(fout if inplace else x, pos, neg, z, sig, sig_to, m, cn, SCALE, coef, out=fout, out_bf16=hout, max_blocks=max_blocks)
        torch.cuda.synchronize()
        assert o.data_ptr() == fout.data_ptr() and o16.data_ptr() == hout.data_ptr()
        assert _guards_intact(fbuf, B * n, -768.0) and _guards_intact(hbuf, B * n, -768.0), tag
        runs[tag] = (fout.cpu(), hout.cpu())
    assert torch.equal(x.cpu(), c['x'])                                    # the out-of-place runs left x alone
    if use_noise:
        assert torch.equal(z.cpu(), c['z'])
    got, got16 = runs['oop']
    for tag, (f, h16) in runs.items():                                     # capped grid, in place and eight runs in all: bit-identical
        assert torch.equal(f.view(torch.int32), got.view(torch.int32)) and torch.equal(h16.view(torch.int16), got16.view(torch.int16)), tag
    err = (got.double() - ref).abs()
    print(f'B={B} n={n} neg={use_neg} coef={use_coef} noise={use_noise}: max err / bound {(err / bound).max().item():.3f}  (max |err| {err.max().item():.3e})')
    assert torch.isfinite(got).all()
    assert (err <= bound).all(), (err / bound).max().item()
    assert torch.equal(got16.view(torch.int16), got.bfloat16().view(torch.int16))          # bf16 copy = RNE of the kernel's own fp32 output
    for mut, r in muts.items():
        frac = ((got.double() - r).abs() > bound).double().mean().item()
        assert frac >= 0.01, (mut, frac)


@pytest.mark.gpu
@pytest.mark.parametrize('use_neg,use_coef', VARIANTS, ids=['nocfg', 'cfg', 'ortho'])
@pytest.mark.parametrize('B,n', SHAPES)
def test_h0_coefficients_agree_with_the_euler_step(B, n, use_neg, use_coef):
    from arcflow_amd import ops
    c = _case(B, n)
    x, pos, neg = c['x'].cuda(), c['pos'].cuda(), c['neg'].cuda() if use_neg else None
    sig, sig_to = c['sigma'].cuda(), c['sigma_to'].cuda()
    coef = c['coef'].cuda() if use_coef else None
    one, zero = torch.ones(B, device='cuda'), torch.zeros(B, device='cuda')
    ode, ode16 = ops.teacher_euler_step(x, pos, neg, sig, sig_to, SCALE, coef)
    ref, bound = _ref(c, use_neg, use_coef, False, ode=True)
    # the ODE kernel's own bound (tests/test_hip_teacher_step_fp64.py): (7 | 9) eps (|x| + |dt| U)
    p, q, cf = c['pos'].double(), c['neg'].double(), c['coef'].double()[:, None]
    U = p.abs() + ((SCALE - 1) * (p.abs() + q.abs()) if use_neg else 0) + ((cf * p).abs() if use_coef else 0)
    dt = (c['sigma_to'].double() - c['sigma'].double())[:, None]
    ode_bound = (9 if use_coef else 7) * EPS * (c['x'].double().abs() + dt.abs() * U)
    for tag, z in (('noise', c['z'].cuda()), ('nonoise', None)):          # c_noise = 0: the draw, read or not, does not matter
        sde, sde16 = ops.teacher_sde_step(x, pos, neg, z, sig, sig_to, one, zero, SCALE, coef)
        torch.cuda.synchronize()
        diff = (sde.double() - ode.double()).abs().cpu()
        print(f'B={B} n={n} neg={use_neg} coef={use_coef} {tag}: h = 0 vs Euler max diff / (sum of bounds) {(diff / (bound + ode_bound)).max().item():.3f}')
        assert (diff <= bound + ode_bound).all()
        assert ((sde.double().cpu() - ref).abs() <= bound).all()
    assert ((ode.double().cpu() - ref).abs() <= ode_bound).all()             # (the two forms share their exact value)


@pytest.mark.gpu
def test_without_output_buffers_allocates_and_refuses_wrong_operands():
    from arcflow_amd import _lib, ops
    c = _case(3, 320)
    ref, bound = _ref(c, True, False, True)
    d = {k: v.cuda() for k, v in c.items()}
    o, o16 = ops.teacher_sde_step(d['x'], d['pos'], d['neg'], d['z'], d['sigma'], d['sigma_to'], d['m'], d['c_noise'], SCALE)
    assert ((o.cpu().double() - ref).abs() <= bound).all() and o16.dtype == torch.bfloat16 and o16.shape == o.shape
    with pytest.raises(ValueError):         # a bf16 draw is not this kernel's operand
        ops.teacher_sde_step(d['x'], d['pos'], None, d['z'].bfloat16(), d['sigma'], d['sigma_to'], d['m'], d['c_noise'])
    with pytest.raises(ValueError):         # per-sample coefficients: [B]
        ops.teacher_sde_step(d['x'], d['pos'], None, d['z'], d['sigma'], d['sigma_to'], d['m'][:2], d['c_noise'])
    with pytest.raises(_lib.ArcflowHipError):         # n % 64 != 0
        one = torch.ones(1, device='cuda')
        ops.teacher_sde_step(torch.zeros(1, 72, device='cuda'), torch.zeros(1, 72, device='cuda', dtype=torch.bfloat16), None, None, one, one, one, one)
