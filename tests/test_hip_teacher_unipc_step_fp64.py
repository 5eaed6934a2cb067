"""``afx_teacher_unipc_step`` (true-CFG combine + one UniPC predictor-corrector step + bf16 copy + the solver's state, one launch) against
fp64, element by element, modelled on tests/test_hip_teacher_sde_step_fp64.py.

Coefficients.  Every sample gets its own row of ten fp32 weights from a real schedule (FlowUniPCScheduler, 7 steps): sample b takes the
pattern's step at shift 3.2 - 0.4 b (sample 1 with solver_type 'bh1'), so neighbouring samples differ in every weight.  The operand
patterns are the ones a roll produces -- first step (no corrector), corrector with m[-1] alone / with one / with two history terms,
predictor orders 1, 2, 3 -- and NULL operands are exactly the ones the step's orders do not reach.

Bound.  The fp64 reference is evaluated from the SAME inputs (bf16 pos / neg, fp32 x, last, h1..h3, the fp32 weights, coef; scale = 4 so
that scale - 1 is exact).  eps = 2^-24 (half an ulp, fp32 round-to-nearest); U bounds |u| as in the sibling tests,

    U   = |pos| + |scale - 1| (|pos| + |neg|) + |coef pos|,
    M_m = |x| + s U                                                  (the terms of m_t = x - s u)
    S_c = |c_last last| + sum_k |c_k h_k| + |c_mt| M_m                 (the terms of x_c; S_c = |x| without a corrector, x_c = x exactly)
    S_p = |p_xc| S_c + sum_k |p_k h_k| + |p_mt| M_m                    (the terms of x_next)

m_t: the kernel forms u with three roundings (d = fl(pos - neg), b = fl(d (scale - 1)), u = fl(pos + b)), each at most eps U, carried by
the factor s: 3 eps s U; the fma rounds once, eps |m_t| <= eps M_m.  |err(m_t)| <= 4 eps M_m, one more unit for the second-order terms:
5 eps M_m (7 with the two roundings of the orthogonal term, c = fl(coef pos), u' = fl(u - c)).
x_c: a chain of at most five multiply-adds, one rounding each of a partial sum bounded by S_c: 5 eps S_c; m_t enters with |c_mt| and its
own 4 (6) eps M_m, and |c_mt| M_m is a summand of S_c: 4 (6) eps S_c.  |err(x_c)| <= 9 eps S_c, one more for second order: 10 eps S_c (12).
x_next: a chain of at most four multiply-adds: 4 eps S_p; x_c enters with |p_xc| and its 9 (11) eps S_c, m_t with |p_mt| and its 4 (6) eps
M_m; |p_xc| S_c and |p_mt| M_m are DIFFERENT summands of S_p, so together at most 9 (11) eps S_p.  |err(x_next)| <= 13 eps S_p, one more
for second order: 14 eps S_p (16).  (Where a NULL operand drops a multiply-add a rounding disappears; without neg the kernel skips d, b
and u: the bounds stay upper bounds.)  Nothing here was tuned to the kernel: the integers count its roundings.
The bf16 output must be bit-equal to round-to-nearest-even of the kernel's own fp32 x_next (so it is within half a bf16 ulp of it).

Every mutated reference (the corrector's and the predictor's weight rows swapped, h1 and h2 swapped, the neighbour sample's weights,
alpha for s in m_t, the corrector skipped) must fail the same check on at least 1 % of the elements of the output it touches; that each
moves the fp64 reference by more than twice the bound there is asserted first, so the check cannot pass by a mutation being too small.
"""
import functools

import pytest
import torch

EPS = 2.0 ** -24
SCALE = 4.0
GUARD = 64            # sentinel elements in front of and behind every output (keeps 16-byte alignment for fp32 and bf16)
SENTINEL = -768.0
SHAPES = [(1, 64, 0), (3, 64 * 5, 0), (2, 64 * 33, 1)]            # (B, n, max_blocks): the smallest legal shape; per-sample weights; the grid-stride loop (9 passes of one block)
VARIANTS = [(False, False), (True, False), (True, True)]          # (neg, coef): no neg, neg, neg + coef
# name -> (solver_order, step of the 7-step schedule for sample 0, number of history operands handed over)
PATTERNS = {
    'first': (3, 0, 0),             # no corrector, predictor order 1: last and every h NULL
    'c1_p2': (3, 1, 1),             # corrector order 1 (m[-1] alone: no D term), predictor order 2
    'c2_p3': (3, 2, 2),             # corrector order 2 (one D term), predictor order 3
    'c3_p3': (3, 3, 3),             # corrector order 3 (two D terms), predictor order 3
    'c1_p1': (1, 2, 1),             # solver_order 1: corrector order 1, predictor order 1, the ring has ONE slot (hist_out == h1)
    'c2_p2': (2, 3, 2),             # the default order past the warm-up: 20 B read, 14 B written per element
}


@functools.lru_cache(maxsize=None)
def _weights(pattern, B):
    """-> ([10, B] fp32: column b is the row of the pattern's step at shift 3.2 - 0.4 b, 'bh1' for sample 1; (corrector order, predictor order))."""
    from arcflow_amd import FlowUniPCScheduler
    order, step, n_hist = PATTERNS[pattern]
    cols, want = [], None
    for b in range(B):
        sch = FlowUniPCScheduler(1000, solver_order=order, solver_type='bh2' if b != 1 else 'bh1', shift=3.2 - 0.4 * b)
        sch.set_timesteps(7)
        co = sch.coefficients(step)
        want = want or (co.corrector_order, co.predictor_order)
        assert (co.corrector_order, co.predictor_order) == want and max(co.corrector_order, co.predictor_order - 1) == n_hist
        cols.append(torch.tensor(co.row(), dtype=torch.float64).float())
    w = torch.stack(cols, 1).contiguous()
    assert torch.isfinite(w).all() and (w[0] > 0).all() and (w[0] < 1).all()
    return w, want


@functools.lru_cache(maxsize=None)
def _case(B, n):
    """Inputs (CPU) of one shape, computed once and shared by every test on that shape."""
    g = torch.Generator().manual_seed(300 + B * 7 + n)
    x = torch.randn(B, n, generator=g)
    pos = torch.randn(B, n, generator=g).bfloat16()
    neg = (0.6 * pos.float() + 0.8 * torch.randn(B, n, generator=g)).bfloat16()
    last = x + 0.05 * torch.randn(B, n, generator=g)              # the state a roll carries: near x, and near one another
    h = [torch.randn(B, n, generator=g) * 0.8 + 0.1 * k for k in range(3)]
    p, q = pos.double(), neg.double()
    coef = (((p - q) * (SCALE - 1) * p).sum(1) / (p * p).sum(1).clamp(min=n * 1e-6)).float()
    return dict(x=x, pos=pos, neg=neg, last=last, h=h, coef=coef)


def _ref(c, w, n_hist, has_last, use_neg, use_coef, mutate=None):
    """fp64 step -> ((m_t, x_c, x_next), (bound m_t, bound x_c, bound x_next)); the bounds always from the unmutated operands."""
    x, p, q, last = c['x'].double(), c['pos'].double(), c['neg'].double(), c['last'].double()
    h = [t.double() for t in c['h'][:n_hist]]
    cf = c['coef'].double()[:, None]
    W = w.double()
    Wb = W
    if mutate == 'neighbour':
        W = W.roll(1, 1)
    if mutate == 'swap_rows':
        W = W.clone()
        W[[1, 2, 3, 6, 7, 8]] = W[[6, 7, 8, 1, 2, 3]]
    hm = list(h)
    if mutate == 'swap_h':
        hm[0], hm[1] = hm[1], hm[0]
    sm1 = SCALE - 1
    u = p.clone()
    if use_neg:
        u = p + (p - q) * sm1
    if use_coef:
        u = u - cf * p
    r = lambda W_, k: W_[k][:, None]                                # noqa: E731
    s = r(W, 0)
    m_t = x - ((1 - s) if mutate == 'alpha' else s) * u
    if has_last and mutate != 'no_corrector':
        x_c = r(W, 1) * last + sum(r(W, 3 + k) * hm[k] for k in range(n_hist)) + r(W, 2) * m_t
    else:
        x_c = x
    x_n = r(W, 6) * x_c + sum(r(W, 8 + k) * hm[k] for k in range(min(n_hist, 2))) + r(W, 7) * m_t
    U = p.abs() + (sm1 * (p.abs() + q.abs()) if use_neg else 0) + ((cf * p).abs() if use_coef else 0)
    M_m = x.abs() + r(Wb, 0) * U
    if has_last:
        S_c = (r(Wb, 1) * last).abs() + sum((r(Wb, 3 + k) * h[k]).abs() for k in range(n_hist)) + r(Wb, 2).abs() * M_m
    else:
        S_c = x.abs()
    S_p = r(Wb, 6).abs() * S_c + sum((r(Wb, 8 + k) * h[k]).abs() for k in range(min(n_hist, 2))) + r(Wb, 7).abs() * M_m
    k_m, k_c, k_p = (7, 12, 16) if use_coef else (5, 10, 14)
    return (m_t, x_c, x_n), (k_m * EPS * M_m, (k_c * EPS * S_c) if has_last else torch.zeros_like(S_c), k_p * EPS * S_p)


def _mutations(B, n_hist, has_last):
    """name -> index of the output it must move (0 m_t, 1 x_c, 2 x_next)."""
    m = {'alpha': 0}
    if has_last:
        m.update(swap_rows=2, no_corrector=1)
    if n_hist >= 2:
        m['swap_h'] = 1
    if B > 1:
        m['neighbour'] = 2
    return m


def _guarded(numel, dtype):
    buf = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=dtype, device='cuda')
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(buf, numel):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[GUARD + numel:] == SENTINEL).all())


def _run(ops, c, w, n_hist, has_last, use_neg, use_coef, max_blocks, alias=()):
    """One launch into guarded buffers -> dict of CPU outputs.  alias: any of 'x' (x_out == x), 'last' (last_out == last), 'hist' (hist_out ==
    the oldest history operand): the aliased input is first copied into the guarded output buffer."""
    B, n = c['x'].shape
    bufs = {k: _guarded(B * n, torch.bfloat16 if k == 'x16' else torch.float32) for k in ('x', 'x16', 'last', 'hist')}
    view = {k: v[1].view(B, n) for k, v in bufs.items()}
    x, last = c['x'].cuda(), c['last'].cuda() if has_last else None
    hist = [t.cuda() for t in c['h'][:n_hist]]
    if 'x' in alias:
        view['x'].copy_(x)
        x = view['x']
    if 'last' in alias:
        view['last'].copy_(last)
        last = view['last']
    if 'hist' in alias:
        view['hist'].copy_(hist[-1])
        hist[-1] = view['hist']
    o, o16 = ops.teacher_unipc_step(x, c['pos'].cuda(), c['neg'].cuda() if use_neg else None, w.cuda(), last, hist, view['last'], view['hist'], SCALE,
                                    c['coef'].cuda() if use_coef else None, out=view['x'], out_bf16=view['x16'], max_blocks=max_blocks)
    torch.cuda.synchronize()
    assert o.data_ptr() == view['x'].data_ptr() and o16.data_ptr() == view['x16'].data_ptr()
    for k, (buf, _) in bufs.items():
        assert _guards_intact(buf, B * n), k
    if 'x' not in alias:
        assert torch.equal(x.cpu(), c['x'])                               # an out-of-place run leaves its inputs alone
    if has_last and 'last' not in alias:
        assert torch.equal(last.cpu(), c['last'])
    for k, t in enumerate(hist):
        if not ('hist' in alias and k == n_hist - 1):
            assert torch.equal(t.cpu(), c['h'][k])
    return {k: v.cpu() for k, v in view.items()}


@pytest.mark.gpu
@pytest.mark.parametrize('use_neg,use_coef', VARIANTS, ids=['nocfg', 'cfg', 'ortho'])
@pytest.mark.parametrize('pattern', list(PATTERNS))
@pytest.mark.parametrize('B,n,max_blocks', SHAPES)
def test_unipc_step_within_fp32_rounding_of_fp64(B, n, max_blocks, pattern, use_neg, use_coef):
    from arcflow_amd import ops
    c = _case(B, n)
    w, (oc, op) = _weights(pattern, B)
    n_hist, has_last = PATTERNS[pattern][2], oc > 0
    refs, bounds = _ref(c, w, n_hist, has_last, use_neg, use_coef)
    muts = {}
    for mut, which in _mutations(B, n_hist, has_last).items():            # the condition under which the mutation check means something
        r = _ref(c, w, n_hist, has_last, use_neg, use_coef, mut)[0][which]
        assert ((r - refs[which]).abs() > 2 * bounds[which]).double().mean().item() >= 0.01, mut
        muts[mut] = (which, r)
    got = _run(ops, c, w, n_hist, has_last, use_neg, use_coef, max_blocks)
    # the aliases a roll uses: in place, the state buffer in place, the history ring's oldest slot overwritten -- alone and all at once; and the
    # other grid (one block walking the tensor / the default): all bit-identical
    others = {'x_inplace': dict(alias=('x',)), 'other_grid': dict(max_blocks=0 if max_blocks else 1)}
    if has_last:
        others['last_inplace'] = dict(alias=('last',))
    if n_hist:
        others['ring'] = dict(alias=('hist',))
        others['all'] = dict(alias=('x', 'hist') + (('last',) if has_last else ()))
    for tag, kw in others.items():
        again = _run(ops, c, w, n_hist, has_last, use_neg, use_coef, kw.get('max_blocks', max_blocks), kw.get('alias', ()))
        for k in got:
            assert torch.equal(again[k].view(torch.int16 if k == 'x16' else torch.int32), got[k].view(torch.int16 if k == 'x16' else torch.int32)), (tag, k)
    for name, key, ref, bound in (('m_t', 'hist', refs[0], bounds[0]), ('x_c', 'last', refs[1], bounds[1]), ('x_next', 'x', refs[2], bounds[2])):
        err = (got[key].double() - ref).abs()
        ratio = (err / bound.clamp(min=1e-300)).max().item() if (bound > 0).any() else err.max().item()
        print(f'B={B} n={n} {pattern} neg={use_neg} coef={use_coef} {name}: max err / bound {ratio:.3f}  (max |err| {err.max().item():.3e})')
        assert torch.isfinite(got[key]).all()
        assert (err <= bound).all(), (name, ratio)
    if not has_last:
        assert torch.equal(got['last'], c['x'])                           # no corrector: x_c is x, bit for bit
    assert torch.equal(got['x16'].view(torch.int16), got['x'].bfloat16().view(torch.int16))          # bf16 copy = RNE of the kernel's own fp32 output
    out_of = ('hist', 'last', 'x')
    for mut, (which, r) in muts.items():
        frac = ((got[out_of[which]].double() - r).abs() > bounds[which]).double().mean().item()
        assert frac >= 0.01, (mut, frac)


@pytest.mark.gpu
@pytest.mark.parametrize('use_neg,use_coef', VARIANTS, ids=['nocfg', 'cfg', 'ortho'])
@pytest.mark.parametrize('B,n,max_blocks', SHAPES)
def test_final_step_lands_on_the_clean_prediction_bit_for_bit(B, n, max_blocks, use_neg, use_coef):
    """The weights of the step onto sigma 0 (p_xc = 0, p_mt = 1, p_1 = p_2 = 0), with the corrector of order 2 that precedes it at solver_order
    3: x_next and the history slot hold the same bits, and the bf16 copy is their rounding."""
    from arcflow_amd import FlowUniPCScheduler, ops
    sch = FlowUniPCScheduler(1000, solver_order=3, shift=3.2)
    sch.set_timesteps(7)
    co = sch.coefficients(6)
    assert co.predictor == (0.0, 1.0, 0.0, 0.0) and co.corrector_order == 2 and co.predictor_order == 1
    w = torch.tensor(co.row(), dtype=torch.float64).float()[:, None].expand(-1, B).contiguous()
    c = _case(B, n)
    got = _run(ops, c, w, 2, True, use_neg, use_coef, max_blocks)
    assert torch.equal(got['x'].view(torch.int32), got['hist'].view(torch.int32)) and torch.isfinite(got['x']).all()
    assert torch.equal(got['x16'].view(torch.int16), got['hist'].bfloat16().view(torch.int16))
    refs, bounds = _ref(c, w, 2, True, use_neg, use_coef)
    assert ((got['x'].double() - refs[0]).abs() <= bounds[0]).all() and ((got['last'].double() - refs[1]).abs() <= bounds[1]).all()
    # a single-step schedule: no corrector either, the whole step is x - s u
    one = FlowUniPCScheduler(1000, solver_order=3)
    one.set_timesteps(1)
    w1 = torch.tensor(one.coefficients(0).row(), dtype=torch.float64).float()[:, None].expand(-1, B).contiguous()
    got = _run(ops, c, w1, 0, False, use_neg, use_coef, max_blocks)
    assert torch.equal(got['x'].view(torch.int32), got['hist'].view(torch.int32)) and torch.equal(got['last'], c['x'])


@pytest.mark.gpu
def test_without_output_buffers_allocates_and_refuses_wrong_operands():
    from arcflow_amd import _lib, ops
    c = _case(3, 320)
    w, _ = _weights('c2_p2', 3)
    refs, bounds = _ref(c, w, 2, True, True, False)
    d = {k: (v.cuda() if isinstance(v, torch.Tensor) else [t.cuda() for t in v]) for k, v in c.items()}
    lo, ho = torch.empty_like(d['x']), torch.empty_like(d['x'])
    o, o16 = ops.teacher_unipc_step(d['x'], d['pos'], d['neg'], w.cuda(), d['last'], d['h'][:2], lo, ho, SCALE)
    assert ((o.cpu().double() - refs[2]).abs() <= bounds[2]).all() and o16.dtype == torch.bfloat16 and o16.shape == o.shape
    assert ((lo.cpu().double() - refs[1]).abs() <= bounds[1]).all() and ((ho.cpu().double() - refs[0]).abs() <= bounds[0]).all()
    ok = (d['x'], d['pos'], d['neg'], w.cuda(), d['last'], d['h'][:2], lo, ho)

    def call(**over):
        names = ('x', 'pos', 'neg', 'w', 'last', 'hist', 'last_out', 'hist_out')
        a = dict(zip(names, ok))
        out = over.pop('out', None)
        a.update(over)
        return ops.teacher_unipc_step(*[a[k] for k in names], SCALE, out=out)
    with pytest.raises(ValueError):         # the weights are [10, B] fp32
        call(w=w.cuda()[:9].contiguous())
    with pytest.raises(ValueError):
        call(w=w.cuda().double())
    with pytest.raises(ValueError):         # a bf16 history is not this kernel's operand
        call(hist=[d['h'][0].bfloat16()])
    with pytest.raises(ValueError):
        call(last_out=lo[:2])
    # refusals of the entry itself: overlapping outputs (by entry name), a corrector without m[-1], n % 64 != 0
    for over in (dict(last_out=d['x']), dict(hist_out=d['last']), dict(out=d['h'][0]), dict(out=lo), dict(hist_out=lo)):
        with pytest.raises(_lib.ArcflowHipError, match='afx_teacher_unipc_step.*overlaps'):
            call(**over)
    with pytest.raises(_lib.ArcflowHipError, match='needs h1'):
        call(hist=[])
    with pytest.raises(_lib.ArcflowHipError, match='multiple of 64'):
        z = torch.zeros(1, 72, device='cuda')
        ops.teacher_unipc_step(z, z.bfloat16(), None, torch.zeros(10, 1, device='cuda'), None, [], z.clone(), z.clone())
    assert torch.equal(d['x'].cpu(), c['x']) and torch.equal(d['last'].cpu(), c['last'])           # nothing was launched by the refused calls
