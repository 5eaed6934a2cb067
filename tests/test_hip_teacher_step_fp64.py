"""The two kernels of teacher sampling against fp64, element by element: ``afx_teacher_euler_step`` (true-CFG combine + Euler step +
bf16 copy, one launch) and ``afx_cfg_ortho_coef`` (the per-sample projection coefficient of orthogonal guidance).

Bound of the step.  The fp64 reference is evaluated from the SAME inputs (bf16 pos / neg, fp32 x, sigma, sigma_to, coef, scale = 4
so that scale - 1 is exact).  With eps = 2^-24 (half an ulp, fp32 round-to-nearest) and, per element,

    M = |x| + |dt| (|pos| + |scale - 1| (|pos| + |neg|) + |coef pos|),        dt = sigma_to - sigma,

the kernel computes  dt = fl(sigma_to - sigma),  d = fl(pos - neg),  b = fl(d (scale - 1)),  u = fl(pos + b),  w = fl(u dt),
x' = fl(x + w): six roundings.  Each perturbs x' by at most eps times the magnitude of the term it rounds, carried to the output:
    dt: eps |dt| |u|;   d: eps |pos - neg| |scale - 1| |dt|;   b: eps |b| |dt|;   u: eps |u| |dt|;   w: eps |u dt|;   x': eps |x + u dt|
and every one of these is <= eps M, because |u| <= |pos| + |scale - 1| (|pos| + |neg|) + |coef pos| and |pos - neg| <= |pos| + |neg|.
So |err| <= 6 eps M to first order; one more unit covers the second-order terms: |err| <= 7 * 2^-24 * M.  (Where hipcc contracts
a multiply-add into an fma, a rounding disappears; the bound stays an upper bound.)  The orthogonal path adds c = fl(coef pos) and
u' = fl(u - c), two more roundings of terms that M already carries: |err| <= 9 * 2^-24 * M.  Without neg the kernel skips d, b and
u, so the same bounds hold with room to spare.

The bf16 output must be bit-equal to round-to-nearest-even of the kernel's own fp32 output.

Bound of the coefficient.  Against coef64 = sum(bias pos) / max(sum pos^2, n 1e-6) in fp64 from the same inputs: the kernel rounds
bias twice in fp32 (d and b above; relative error <= 2 eps per term of the numerator), multiplies and accumulates exactly enough in
fp64 (a product of two fp32 values is exact, the fp64 sums add ~n 2^-53), and rounds the quotient to fp32 once (<= eps |coef|
<= eps sum|bias pos| / den):  |d coef| <= 3 * 2^-24 * sum|bias pos| / max(sum pos^2, n 1e-6).

Every mutated reference (pos / neg swapped, the neighbour sample's sigma, scale for scale - 1, orthogonal term dropped) must fail the
same check on at least 1 % of the elements; that each moves the fp64 reference by more than twice the bound on at least 1 % of the
elements is asserted on the CPU side first, so the GPU assertion cannot pass by a mutation being too small to see.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
SCALE = 4.0
GUARD = 64            # sentinel elements in front of and behind every output (keeps 16-byte alignment for fp32, bf16 and fp64)
SHAPES = [(3, 64 * 5), (1, 64), (2, 64 * 1031)]       # small with per-sample sigmas; a single chunk row; ragged, several blocks


@functools.lru_cache(maxsize=None)
def _case(B, n):
    """Inputs (CPU) and fp64 references of one shape, computed once and shared by every test on that shape."""
    g = torch.Generator().manual_seed(100 + B * 7 + n)
    x = torch.randn(B, n, generator=g)
    pos = torch.randn(B, n, generator=g).bfloat16()
    neg = (0.6 * pos.float() + 0.8 * torch.randn(B, n, generator=g)).bfloat16()        # comparable magnitude, correlated like two prompts
    sigma = torch.tensor([0.95, 0.62, 0.30][:B])
    sigma_to = torch.tensor([0.80, 0.55, 0.05][:B])                                    # |dt| = 0.15, 0.07, 0.25: all >= 0.05, all different
    p, q = pos.double(), neg.double()
    bias32 = ((pos.float() - neg.float()) * (SCALE - 1)).double()                      # the kernels' fp32 bias (for the coefficient's exact sums)
    bias = (p - q) * (SCALE - 1)
    den = (p * p).sum(1).clamp(min=n * 1e-6)
    coef64 = (bias * p).sum(1) / den
    coef_bound = 3 * EPS * (bias * p).abs().sum(1) / den
    coef = coef64.float()                                                              # what the step kernel is handed in the coef variants
    return dict(x=x, pos=pos, neg=neg, sigma=sigma, sigma_to=sigma_to, coef=coef, coef64=coef64, coef_bound=coef_bound, bias32=bias32)


def _ref(c, use_neg, use_coef, mutate=None):
    """fp64 step from the case's inputs -> (reference, bound per element)."""
    x, p, q = c['x'].double(), c['pos'].double(), c['neg'].double()
    sig, sig_to, cf = c['sigma'].double()[:, None], c['sigma_to'].double()[:, None], c['coef'].double()[:, None]
    sm1 = SCALE - 1
    if mutate == 'swap':
        p, q = q, p
    if mutate == 'sigma':
        sig, sig_to = sig.roll(1, 0), sig_to.roll(1, 0)
    if mutate == 'scale':
        sm1 = SCALE
    u = p.clone()
    if use_neg:
        u = p + (p - q) * sm1
    if use_coef and mutate != 'no_ortho':
        u = u - cf * p
    dt = sig_to - sig
    ref = x + u * dt
    M = x.abs() + dt.abs() * (p.abs() + (abs(sm1) * (p.abs() + q.abs()) if use_neg else 0) + ((cf * p).abs() if use_coef else 0))
    return ref, (9 if use_coef else 7) * EPS * M


def _mutations(B, use_neg, use_coef):
    m = []
    if use_neg:
        m += ['swap', 'scale']
    if B > 1:
        m.append('sigma')
    if use_coef:
        m.append('no_ortho')
    return m


def _guarded(numel, dtype, sentinel):
    buf = torch.full((numel + 2 * GUARD,), sentinel, dtype=dtype, device='cuda')
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(buf, numel, sentinel):
    return bool((buf[:GUARD] == sentinel).all() and (buf[GUARD + numel:] == sentinel).all())


@pytest.mark.parametrize('use_coef', [False, True], ids=['plain', 'ortho'])
@pytest.mark.parametrize('use_neg', [True, False], ids=['cfg', 'nocfg'])
@pytest.mark.parametrize('B,n', SHAPES)
def test_step_within_fp32_rounding_of_fp64(B, n, use_neg, use_coef):
    from arcflow_amd import ops
    c = _case(B, n)
    ref, bound = _ref(c, use_neg, use_coef)
    # CPU side first: every mutation moves the reference by more than twice the bound on >= 1 % of the elements
    muts = {m: _ref(c, use_neg, use_coef, m)[0] for m in _mutations(B, use_neg, use_coef)}
    for m, r in muts.items():
        frac = ((r - ref).abs() > 2 * bound).double().mean().item()
        print(f'B={B} n={n} neg={use_neg} coef={use_coef} mutation {m}: moves {100 * frac:.1f} % of the elements by > 2 x bound')
        assert frac >= 0.01, (m, frac)
    x, pos, neg = c['x'].cuda(), c['pos'].cuda(), c['neg'].cuda() if use_neg else None
    sig, sig_to = c['sigma'].cuda(), c['sigma_to'].cuda()
    coef = c['coef'].cuda() if use_coef else None
    # out of place at the default grid, out of place on a capped grid (several grid-stride passes at the ragged shape: 65 blocks of work on 24),
    # and in place -- all into guarded buffers
    runs = {}
    for tag, max_blocks, inplace in (('oop', 0, False), ('oop_capped', 24, False), ('inplace', 0, True)):
        fbuf, fout = _guarded(B * n, torch.float32, -768.0)
        hbuf, hout = _guarded(B * n, torch.bfloat16, -768.0)
        fout, hout = fout.view(B, n), hout.view(B, n)
        if inplace:
            fout.copy_(x)
        o, o16 = ops.teacher_euler_step(fout if inplace else x, pos, neg, sig, sig_to, SCALE, coef, out=fout, out_bf16=hout, max_blocks=max_blocks)
        torch.cuda.synchronize()
        assert o.data_ptr() == fout.data_ptr() and o16.data_ptr() == hout.data_ptr()
        assert _guards_intact(fbuf, B * n, -768.0) and _guards_intact(hbuf, B * n, -768.0), tag
        runs[tag] = (fout.cpu(), hout.cpu())
    assert torch.equal(x.cpu(), c['x'])                                    # the out-of-place runs left x alone
    got, got16 = runs['oop']
    for tag in ('oop_capped', 'inplace'):
        assert torch.equal(runs[tag][0], got) and torch.equal(runs[tag][1], got16), tag
    err = (got.double() - ref).abs()
    print(f'B={B} n={n} neg={use_neg} coef={use_coef}: max err / bound {(err / bound).max().item():.3f}  (max |err| {err.max().item():.3e})')
    assert torch.isfinite(got).all()
    assert (err <= bound).all(), (err / bound).max().item()
    assert torch.equal(got16.view(torch.int16), got.bfloat16().view(torch.int16))          # bf16 copy = RNE of the kernel's own fp32 output
    for m, r in muts.items():
        frac = ((got.double() - r).abs() > bound).double().mean().item()
        assert frac >= 0.01, (m, frac)


def test_step_without_output_buffers_allocates_and_matches():
    from arcflow_amd import ops
    c = _case(3, 320)
    ref, bound = _ref(c, True, False)
    o, o16 = ops.teacher_euler_step(c['x'].cuda(), c['pos'].cuda(), c['neg'].cuda(), c['sigma'].cuda(), c['sigma_to'].cuda(), SCALE)
    assert ((o.cpu().double() - ref).abs() <= bound).all() and o16.dtype == torch.bfloat16 and o16.shape == o.shape
    with pytest.raises(ValueError):         # fp32 velocities are the composed path's operands, not this kernel's
        ops.teacher_euler_step(c['x'].cuda(), c['pos'].cuda().float(), None, c['sigma'].cuda(), c['sigma_to'].cuda())
    from arcflow_amd import _lib
    with pytest.raises(_lib.ArcflowHipError):         # n % 64 != 0
        ops.teacher_euler_step(torch.zeros(1, 72, device='cuda'), torch.zeros(1, 72, device='cuda', dtype=torch.bfloat16), None,
                               torch.ones(1, device='cuda'), torch.zeros(1, device='cuda'))


@pytest.mark.parametrize('B,n', [(3, 320), (2, 64 * 1031)], ids=['one_partial', 'nine_partials_ragged'])
def test_ortho_coef_against_fp64_and_reproducible(B, n):
    from arcflow_amd import _lib, ops
    c = _case(B, n)
    need = _lib.load().afx_cfg_ortho_ws_bytes(B, n)
    parts = need // (16 * B)
    assert parts == (1 if n == 320 else 9)
    pos, neg = c['pos'].cuda(), c['neg'].cuda()
    results, scratches = [], []
    for _ in range(8):
        wbuf, ws = _guarded(need // 8, torch.float64, -768.0)
        cbuf, out = _guarded(B, torch.float32, -768.0)
        r = ops.cfg_ortho_coef(pos, neg, SCALE, out=out, ws=ws)
        torch.cuda.synchronize()
        assert r.data_ptr() == out.data_ptr()
        assert _guards_intact(wbuf, need // 8, -768.0) and _guards_intact(cbuf, B, -768.0)
        results.append(out.cpu().clone())
        scratches.append(ws.cpu().clone())
    for r, s in zip(results[1:], scratches[1:]):
        assert torch.equal(r.view(torch.int32), results[0].view(torch.int32)) and torch.equal(s.view(torch.int64), scratches[0].view(torch.int64))
    got = results[0].double()
    err = (got - c['coef64']).abs()
    print(f'B={B} n={n}: coef {got.tolist()}  |d coef| / bound {(err / c["coef_bound"]).max().item():.3f}')
    assert (err <= c['coef_bound']).all(), (err / c['coef_bound']).tolist()
    # the slots hold the exact partial sums: added up they are the fp64 sums of the kernels' own fp32 bias, to fp64 rounding
    s = scratches[0].view(B, parts, 2).sum(1)
    p = c['pos'].double()
    assert torch.allclose(s[:, 0], (c['bias32'] * p).sum(1), rtol=1e-10, atol=0) and torch.allclose(s[:, 1], (p * p).sum(1), rtol=1e-10, atol=0)
    # a mutated reference (pos / neg swapped) is far outside the bound
    q = c['neg'].double()
    swapped = ((q - p) * (SCALE - 1) * q).sum(1) / (q * q).sum(1)
    assert ((got - swapped).abs() > c['coef_bound']).all()


def test_ortho_clamp_all_zero_pos_gives_zero_coef_and_finite_step():
    from arcflow_amd import ops
    c = _case(3, 320)
    pos = c['pos'].clone()
    pos[1] = 0
    pos_d, neg_d = pos.cuda(), c['neg'].cuda()
    coef = ops.cfg_ortho_coef(pos_d, neg_d, SCALE)
    assert coef[1].item() == 0.0 and torch.isfinite(coef).all() and coef[0].item() != 0.0
    x = c['x'].cuda()
    o, o16 = ops.teacher_euler_step(x, pos_d, neg_d, c['sigma'].cuda(), c['sigma_to'].cuda(), SCALE, coef)
    assert torch.isfinite(o).all() and torch.isfinite(o16.float()).all()
    # sample 1: pos = 0, so u = -(scale - 1) neg exactly as without the orthogonal term
    dt = (c['sigma_to'][1] - c['sigma'][1]).double()
    ref = c['x'][1].double() - (SCALE - 1) * c['neg'][1].double() * dt
    assert ((o[1].cpu().double() - ref).abs() <= 7 * EPS * (c['x'][1].abs().double() + dt.abs() * (SCALE - 1) * c['neg'][1].abs().double())).all()
