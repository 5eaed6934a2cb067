"""adamw_kernel, adamw8bit_kernel, ema_kernel, euler_kernel and cfg_kernel (afx_train.hip) per element against the fp64 reference of
tests/optimizer_ref.py, with its derived bounds (counts of fp32 roundings times u = 2^-24; test_optimizer_ref_cpu.py shows that correct fp32
arithmetic passes them on these very inputs and that a list of wrong kernels does not).  Every buffer a kernel writes is a view inside a
larger buffer of sentinels that must come back bit-identical; parameter and gradient views start at element offsets 0, 1 and 3 (not 16-byte
aligned, like the trainer's slices of its flat buffers).  Each assertion message and each printed line carries the worst err / bound seen."""
import pytest
import torch

import optimizer_ref as O

pytestmark = pytest.mark.gpu

PAD = 64
OFFSETS = (0, 1, 3)


@pytest.fixture(scope='module')
def ops():
    from arcflow_amd import ops as _ops
    return _ops


class Guarded:
    """A contiguous view of n values at element offset `off` inside a sentinel-filled GPU buffer with PAD values behind it."""

    def __init__(self, src, off, sentinel):
        n = src.numel()
        self.buf = torch.full((off + n + PAD,), sentinel, dtype=src.dtype, device='cuda')
        self.view = self.buf[off:off + n]
        self.view.copy_(src.flatten())
        self.off, self.n, self.sentinel = off, n, sentinel

    def intact(self, what):
        """Everything outside the view still holds the sentinel, bit for bit."""
        b = self.buf
        assert bool((b[:self.off] == self.sentinel).all()) and bool((b[self.off + self.n:] == self.sentinel).all()), \
            f'{what}: a write landed outside the view'


def _merge(worst, r):
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)


def _show(what, worst):
    print(f'{what}: worst err / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))


# ---- adamw_step ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wd,gscale', O.ADAMW_WD_GSCALE)
@pytest.mark.parametrize('i,n', list(enumerate(O.ADAMW_N)))
def test_adamw_step(ops, i, n, wd, gscale):
    p0, m0, v0, grads, zero = O.adamw_case(n)
    off = OFFSETS[i % 3]
    p, m, v = Guarded(p0, off, 7.0), Guarded(m0, off, -3.0), Guarded(v0, off, 5.0)
    worst = {}
    for t, step in enumerate(O.ADAMW_STEPS):
        g = Guarded(grads[t], off, 9.0)
        before = (p.view.cpu(), m.view.cpu(), v.view.cpu())                  # the kernel's own previous fp32 state: errors do not compound
        ops.adamw_step(p.view, g.view, m.view, v.view, 1e-3, step, betas=(0.9, 0.95), eps=1e-8, weight_decay=wd, grad_scale=gscale)
        torch.cuda.synchronize()
        for b in (p, m, v, g):
            b.intact(f'adamw_step n={n} step {step}')
        assert torch.equal(g.view.cpu(), grads[t])
        _merge(worst, O.check_adamw_step(before[0], grads[t], before[1], before[2], p.view, m.view, v.view, 1e-3, step, wd=wd, gscale=gscale,
                                         zero=zero, what=f'adamw_step n={n} wd={wd} gscale={gscale}'))
    _show(f'adamw_step n={n} wd={wd} gscale={gscale}', worst)


def test_adamw_step_of_nothing(ops):
    bufs = [Guarded(torch.zeros(0), 3, s) for s in (7.0, 9.0, -3.0, 5.0)]
    ops.adamw_step(*(b.view for b in bufs), 1e-3, 1)
    ops.ema_lerp(bufs[0].view, bufs[1].view, 0.5)
    torch.cuda.synchronize()
    for b in bufs:
        b.intact('n = 0')


# ---- adamw8bit_step -----------------------------------------------------------------------------------------------------------------------
def _state(ops, n):
    """An AdamW8bitState whose four arrays are guarded views at offset 0 (as the class allocates them), sentinels 0xA5 / 77.0."""
    st = ops.AdamW8bitState(n, 'cuda')
    guards = dict(state1=Guarded(st.state1, 0, 0xA5), state2=Guarded(st.state2, 0, 0xA5), absmax1=Guarded(st.absmax1, 0, 77.0),
                  absmax2=Guarded(st.absmax2, 0, 77.0))
    for k, gd in guards.items():
        setattr(st, k, gd.view)
    return st, guards


def _snapshot(st):
    return tuple(getattr(st, k).cpu() for k in ('state1', 'state2', 'absmax1', 'absmax2'))


def _step8(ops, p, g, st, step):
    h = O.ADAMW8_HYPER
    ops.adamw8bit_step(p.view, g.view, st, h['lr'], step, betas=h['betas'], eps=h['eps'], weight_decay=h['wd'], grad_scale=h['gscale'])
    torch.cuda.synchronize()


@pytest.mark.parametrize('i,n,kind', [(i, n, k) for i, (n, k) in enumerate(O.adamw8bit_cases())])
def test_adamw8bit_step(ops, i, n, kind):
    p0, grads, expect = O.adamw8bit_case(n, kind)
    off = OFFSETS[i % 3]
    p = Guarded(p0, off, 7.0)
    st, guards = _state(ops, n)
    q1, q2 = st.qmap1.cpu(), st.qmap2.cpu()
    what = f'adamw8bit_step n={n} {kind}'
    worst = {}
    for t in range(4):
        g = Guarded(grads[t], off, 9.0)
        p_before, before = p.view.cpu(), _snapshot(st)                        # the reference starts from the kernel's own codes and absmax
        if t == 3 and kind == 'logspace':                                     # the same step twice from the same state: bit-identical
            p2 = Guarded(p_before, off, 7.0)
            st2, _ = _state(ops, n)
            for k, b in zip(('state1', 'state2', 'absmax1', 'absmax2'), before):
                getattr(st2, k).copy_(b)
            _step8(ops, p2, g, st2, t + 1)
        _step8(ops, p, g, st, t + 1)
        for b in (p, g, *guards.values()):
            b.intact(f'{what} step {t + 1}')
        assert torch.equal(g.view.cpu(), grads[t])
        after = _snapshot(st)
        if t == 3 and kind == 'logspace':
            assert torch.equal(p.view, p2.view) and all(torch.equal(a, b) for a, b in zip(after, _snapshot(st2))), f'{what}: two runs differ'
        _merge(worst, O.check_adamw8bit_step(p_before, grads[t], *before, q1, q2, (p.view.cpu(), *after), step=t + 1, expect=expect[t],
                                             what=what, **O.ADAMW8_HYPER))
        # moments() is the fp32 product qmap[code] * absmax, bit for bit
        m, v = st.moments()
        rep = lambda a: a.repeat_interleave(256)[:n]                           # noqa: E731
        assert torch.equal(m.cpu(), q1[after[0].long()] * rep(after[2])) and torch.equal(v.cpu(), q2[after[1].long()] * rep(after[3])), \
            f'{what}: moments() is not qmap[code] * absmax'
        if 'neg_extreme' in expect[t] and expect[t]['neg_extreme'].numel():
            # the signed book has no -1: a negative extreme comes back as qmap1[0] * absmax = -0.99297 absmax
            i_neg = expect[t]['neg_extreme']
            assert torch.equal(m.cpu()[i_neg], q1[0] * after[2][i_neg // 256]) and float(q1[0]) == pytest.approx(-0.99297, abs=1e-5)
    _show(what, worst)


# ---- ema_lerp -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i,n', list(enumerate(O.EMA_N)))
def test_ema_lerp(ops, i, n):
    ema0, net0 = O.ema_case(n)
    worst = {}
    for j, beta in enumerate(O.EMA_BETAS):
        off = OFFSETS[(i + j) % 3]
        ema, net = Guarded(ema0, off, 7.0), Guarded(net0, off, 9.0)
        ops.ema_lerp(ema.view, net.view, beta)
        torch.cuda.synchronize()
        ema.intact(f'ema_lerp n={n} beta={beta}')
        net.intact(f'ema_lerp n={n} beta={beta}')
        out = ema.view.cpu()
        assert torch.equal(net.view.cpu(), net0)
        worst[f'beta={beta}'] = O.within(out, O.ema_ref(ema0, net0, beta), O.ema_bound(ema0, net0, beta), f'ema_lerp n={n} beta={beta}')
        same = ema0 == net0
        assert torch.equal(out[same].view(torch.int32), net0[same].view(torch.int32)), f'ema == net must stay, beta={beta}'
        if beta == 0.0:                                                       # the trainer's first lerp
            assert torch.equal(out.view(torch.int32), net0.view(torch.int32))
        if beta in (0.93, 0.9999) and n > 1:                                    # teeth: beta and 1 - beta swapped (0.5 is its own swap)
            with pytest.raises(AssertionError):
                O.within(out, O.ema_ref(ema0, net0, 1.0 - beta), O.ema_bound(ema0, net0, beta), 'swapped')
    _show(f'ema_lerp n={n}', worst)


# ---- euler_roll, cfg_combine --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', O.ROLL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_euler_roll(ops, shape):
    xa, u = O.roll_case(shape)
    sa, sb = O.EULER_SIGMAS
    out = ops.euler_roll(xa.cuda(), u.cuda(), sa.cuda(), sb.cuda()).cpu()
    bound = O.euler_bound(xa, u, sa, sb)
    worst = O.within(out, O.euler_ref(xa, u, sa, sb), bound, f'euler_roll {shape}')
    assert torch.equal(out[1].view(torch.int32), xa[1].view(torch.int32)), 'sigma_a == sigma_b must return x_a'
    with pytest.raises(AssertionError):                                       # teeth: the sigmas in reversed sample order
        O.within(out, O.euler_ref(xa, u, sa.flip(0), sb.flip(0)), bound, 'flipped')
    # a one-element sigma is expanded over the batch by the wrapper
    one_a, one_b = torch.tensor([0.8]), torch.tensor(0.3)
    out1 = ops.euler_roll(xa.cuda(), u.cuda(), one_a.cuda(), one_b.cuda()).cpu()
    w1 = O.within(out1, O.euler_ref(xa, u, one_a, one_b), O.euler_bound(xa, u, one_a, one_b), f'euler_roll {shape} one sigma')
    _show(f'euler_roll {shape}', dict(per_sample=worst, one_sigma=w1))


@pytest.mark.parametrize('shape', O.ROLL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_cfg_combine(ops, shape):
    pos, neg = O.roll_case(shape)
    worst = {}
    for scale in O.CFG_SCALES:
        out = ops.cfg_combine(pos.cuda(), neg.cuda(), scale).cpu()
        bound = O.cfg_bound(pos, neg, scale)
        worst[f'scale={scale}'] = O.within(out, O.cfg_ref(pos, neg, scale), bound, f'cfg_combine {shape} scale={scale}')
        if scale == 1.0:
            assert torch.equal(out.view(torch.int32), pos.view(torch.int32)), 'scale = 1 must return pos'
        else:                       # teeth: one scale serves all samples, so the reversed sample order is that of the negative branch
            with pytest.raises(AssertionError):
                O.within(out, O.cfg_ref(pos, neg.flip(0), scale), bound, 'flipped')
    _show(f'cfg_combine {shape}', worst)
