"""``afx_sample_score`` -- the per-sample agreement sums of training-time evaluation, sum (a-b)^2, sum a^2, sum b^2, sum a b -- against
torch fp64 on the CPU from the same inputs, for fp32 and bf16 operands, with and without the image-range transform.

Reference.  The four sums in torch fp64 on the CPU.  With transform 1 the transform is applied in fp32 exactly as specified,
``(v.float() / 2 + 0.5).clamp(0, 1)`` (v / 2 is exact, the addition rounds once: the same fp32 value the kernel forms, with or without a
contracted multiply-add), then widened.

Bound per sum:  |kernel - reference| <= 2 n 2^-53 sum|term|,  u = 2^-53 the fp64 unit roundoff, n the elements per sample.
  * The kernel's terms: x, y are fp32 (or bf16) values widened exactly.  x x, y y and x y have at most 48 significant bits: exact.
    d = fl(x - y) rounds once, fl(d d) once more: relative error <= 2 u + u^2 per term of S_dd.  (A contracted fma drops a rounding.)
  * The kernel's summation: every lane adds its terms in order, 64 lanes are added by a shuffle tree, 4 waves and then the <= 64 slots in
    index order.  Whatever the order, a sum of n terms by n - 1 additions has error <= (n - 1) u sum|term| to first order (each term
    passes through at most n - 1 additions); the kernel's tree is much shallower than that.
  * The reference's own error: torch's fp64 sum is pairwise / vectorised, error <= (log2 n + c) u sum|term| with a small constant c, and its
    terms carry the same <= 2 u.
  Together <= (n - 1 + 2) u + (log2 n + c + 2) u <= 2 n u for every n >= 64 (n = 64: 65 + 8 + c <= 128 for c <= 55).  The constant of
  the issue, 2 n 2^-53 -- recursive summation (n - 1) u plus one rounding per product or square -- therefore covers this summation order.

Also asserted: eight runs bit-identical (sums and workspace slots); guard elements around ``out`` and ``ws`` untouched; a == b gives
S_dd == 0 exactly and S_aa == S_bb == S_ab bit for bit; mutated references (the neighbouring sample's operand, transform dropped,
clamp dropped, a + b for a - b) each miss the bound on every sample in at least one sum, after the CPU side has shown that each moves the
reference by more than twice the bound on every sample.  The entry has no launch cap (the partition is a function of n alone), so
there is no second grid to compare against.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GUARD = 64
SHAPES = [(3, 320), (1, 64), (2, 64 * 1031), (1, 8192 * 64 + 64)]      # one slot; one row of lanes; 9 slots, ragged; past the 64-slot cap
PARTS = {320: 1, 64: 1, 64 * 1031: 9, 8192 * 64 + 64: 64}
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16}


def _unit_range(v, clamp=True):
    t = v.float() / 2 + 0.5
    return t.clamp(0, 1) if clamp else t


def _sums(x, y, plus=False):
    """x, y [B, n] fp64 -> (sums [B, 4], sum|term| [B, 4])"""
    d = x + y if plus else x - y
    terms = [d * d, x * x, y * y, x * y]
    return torch.stack([t.sum(1) for t in terms], 1), torch.stack([t.abs().sum(1) for t in terms], 1)


@functools.lru_cache(maxsize=None)
def _case(B, n, dname, transform):
    """Inputs (CPU, the operand dtype) and the fp64 reference of one case, computed once."""
    g = torch.Generator().manual_seed(7 + B * 13 + n + 1000 * transform)
    scale = 2.0 if transform else 1.0          # the transform clamps v <= -1 and v >= 1
    b = torch.randn(B, n, generator=g) * scale
    a = 0.8 * b + 0.6 * scale * torch.randn(B, n, generator=g) + 0.05          # correlated like a student and its teacher, small offset
    if transform:      # a narrow (std 0.4: inside) and a wide (std 3: 37 % past either end) population: ~15 % clamp at each end, ~70 % do not
        narrow = torch.rand(B, n, generator=g) < 0.6
        a = torch.where(narrow, a * 0.2, a * 1.5)
        b = torch.where(narrow, b * 0.2, b * 1.5)
    a, b = a.to(DTYPES[dname]), b.to(DTYPES[dname])
    if transform:
        for v in (a, b):
            t = _unit_range(v, clamp=False)
            lo, hi = (t <= 0).float().mean().item(), (t >= 1).float().mean().item()
            assert lo >= 0.10 and hi >= 0.10 and 1 - lo - hi >= 0.50, (lo, hi)
    x = (_unit_range(a) if transform else a).double()
    y = (_unit_range(b) if transform else b).double()
    ref, mag = _sums(x, y)
    return dict(a=a, b=b, ref=ref, bound=2 * n * U * mag)


def _mutations(c, B, transform):
    """name -> mutated fp64 reference [B, 4]"""
    a, b = c['a'], c['b']
    f = (lambda v: _unit_range(v).double()) if transform else (lambda v: v.double())
    m = {'plus': _sums(f(a), f(b), plus=True)[0]}
    if B > 1:
        m['neighbour'] = _sums(f(a), f(b.roll(1, 0)))[0]
    if transform:
        m['no_transform'] = _sums(a.double(), b.double())[0]
        m['no_clamp'] = _sums(_unit_range(a, False).double(), _unit_range(b, False).double())[0]
    return m


def _guarded(numel, sentinel=-768.0):
    buf = torch.full((numel + 2 * GUARD,), sentinel, dtype=torch.float64, device='cuda')
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(buf, numel, sentinel=-768.0):
    return bool((buf[:GUARD] == sentinel).all() and (buf[GUARD + numel:] == sentinel).all())


@pytest.mark.parametrize('transform', [0, 1], ids=['latent', 'image'])
@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
@pytest.mark.parametrize('B,n', SHAPES)
def test_sums_within_fp64_bound_reproducible_and_guarded(B, n, dname, transform):
    from arcflow_amd import _lib, ops
    c = _case(B, n, dname, transform)
    ref, bound = c['ref'], c['bound']
    muts = _mutations(c, B, transform)
    for name, r in muts.items():           # CPU side first: every mutation moves some sum of EVERY sample by more than twice the bound
        moved = ((r - ref).abs() > 2 * bound).any(1)
        print(f'B={B} n={n} {dname} transform={transform} mutation {name}: max move / bound {((r - ref).abs() / bound).max().item():.3e}')
        assert moved.all(), (name, ((r - ref).abs() / bound).tolist())
    need = _lib.load().afx_sample_score_ws_bytes(B, n)
    assert need == B * PARTS[n] * 32
    a, b = c['a'].cuda(), c['b'].cuda()
    outs, slots = [], []
    for _ in range(8):
        wbuf, ws = _guarded(need // 8)
        obuf, out = _guarded(B * 4)
        r = ops.sample_score(a, b, transform=bool(transform), out=out.view(B, 4), ws=ws)
        torch.cuda.synchronize()
        assert r.data_ptr() == out.data_ptr() and r.shape == (B, 4) and r.dtype == torch.float64
        assert _guards_intact(wbuf, need // 8) and _guards_intact(obuf, B * 4)
        outs.append(out.cpu().clone().view(B, 4))
        slots.append(ws.cpu().clone())
    for o, s in zip(outs[1:], slots[1:]):
        assert torch.equal(o.view(torch.int64), outs[0].view(torch.int64)) and torch.equal(s.view(torch.int64), slots[0].view(torch.int64))
    got = outs[0]
    assert torch.equal(a.cpu(), c['a']) and torch.equal(b.cpu(), c['b'])          # the operands are read only
    err = (got - ref).abs()
    print(f'B={B} n={n} {dname} transform={transform}: max err / bound {(err / bound).max().item():.3e}  sums[0] {got[0].tolist()}')
    assert torch.isfinite(got).all()
    assert (err <= bound).all(), (err / bound).tolist()
    # the slots hold the partial sums: added in index order they ARE the result, bit for bit
    s = slots[0].view(B, PARTS[n], 4)
    acc = torch.zeros(B, 4, dtype=torch.float64)
    for w in range(PARTS[n]):
        acc = acc + s[:, w]
    assert torch.equal(acc.view(torch.int64), got.view(torch.int64))
    for name, r in muts.items():           # the kernel is outside every mutated reference's bound, on every sample
        missed = ((got - r).abs() > bound).any(1)
        assert missed.all(), (name, ((got - r).abs() / bound).tolist())


@pytest.mark.parametrize('transform', [0, 1], ids=['latent', 'image'])
@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
def test_equal_operands_give_exact_zero_distance(dname, transform):
    from arcflow_amd import ops
    for B, n in ((3, 320), (2, 64 * 1031)):
        a = _case(B, n, dname, transform)['a'].cuda()
        for other in (a, a.clone()):            # the same buffer, and an equal copy
            got = ops.sample_score(a, other, transform=bool(transform)).cpu()
            assert (got[:, 0] == 0).all()
            assert torch.equal(got[:, 1].view(torch.int64), got[:, 2].view(torch.int64)) and torch.equal(got[:, 1].view(torch.int64), got[:, 3].view(torch.int64))
            assert (got[:, 1] > 0).all()


def test_wrapper_allocates_and_refuses_wrong_operands():
    from arcflow_amd import _lib, ops
    c = _case(3, 320, 'bf16', 0)
    a, b = c['a'].cuda(), c['b'].cuda()
    got = ops.sample_score(a.view(3, 5, 64), b.view(3, 5, 64)).cpu()            # [B, ...]: every other dimension is the sample
    assert ((got - c['ref']).abs() <= c['bound']).all()
    assert ops.sample_score_ws(3, 320).numel() == 3 * 4 and ops.sample_score_ws(3, 320).dtype == torch.float64
    with pytest.raises(ValueError):
        ops.sample_score(a, b.float())                       # mixed dtypes
    with pytest.raises(ValueError):
        ops.sample_score(a.half(), b.half())                 # neither fp32 nor bf16
    with pytest.raises(ValueError):
        ops.sample_score(a.t(), b.t())                       # not contiguous
    with pytest.raises(_lib.ArcflowHipError):
        ops.sample_score(a[:, :72].contiguous(), b[:, :72].contiguous())          # n % 64 != 0
    with pytest.raises(_lib.ArcflowHipError):
        ops.sample_score(a, b, ws=torch.empty(3, dtype=torch.float64, device='cuda'))       # short workspace
    with pytest.raises(_lib.ArcflowHipError):
        ops.sample_score(a.cpu(), b.cpu())
