"""The ArcFlow policy step, its dropout and velocity forms, their backward and ``head_grad`` against fp64, element by element.

Reference, per-element bounds (derived in its docstring), mutations and the case lists live in tests/arcflow_policy_ref.py; that the reference is
right and that every mutation is large enough to see is checked without a device in tests/test_arcflow_policy_ref_cpu.py.  Here every case runs

  * the generic ``arcflow_step_kernel`` (any K <= 32, the c += 64 loop at ch = 128, pp = 1 / 3 / 16), the K = 16 / ch = 64 / pp = 4 fast kernel at
    one, two and four tokens per wave (AFX_STEP_TPW is read once per process: 2 and 4 each run in one fresh child process), and
    ``arcflow_bwd_kernel`` at ch < 64 (inactive lanes in the shuffles), pp = 1 / 16 / 64, K = 2 ... 32, fp32 and bf16 mixtures;
  * at 1, 10 and 129 tokens: a single wave, a sample boundary inside a 4-wave block with a short last block, and an odd count that spills one
    token into a new block;
  * with gates planted at gamma d_step = {0, +-0.5, +-0.9, +-1.1, +-2, +-10, +-100, +-1000} eps and gamma = +-8.

Checks: |got - ref| <= bound on every element and all finite; every applicable mutation rejected on >= 1 % of the elements of the outputs it
targets; two runs bit-identical; outputs written through ``out=`` / ``grads=`` sit between intact sentinel guards; a step with d_step = 0 returns x
bit for bit; a sample with gscale = 0 gets exactly zero gradients.  A fully dropped sample is out of scope for ``arcflow_step_dropout``: the
trainer's mask never produces one.

Shapes the backward does not take ((16, 128, 4): ch > 64; (5, 12, 3): pp no power of two) and K = 1 are refused by the C entry points' own
argument checks (afx_arcflow_backward: ``ch > 64 || (pp & (pp - 1)) || 64 % pp``; every entry point: ``!logg`` -- an empty logg tensor has a null
data pointer) before anything is launched; the tests assert the Python exception.

Measured on an MI355X, max err / bound over all cases: step / dropout / velocity 0.94 (TPW = 2 and 4: 0.77); d_means 1.00, d_logw 0.98,
d_logg 1.00 (the values next to 1 are the accumulate form, whose bound is dominated by the one rounding of old + gradient); head_grad logw
columns 0.99 (a bf16 store half an ulp off at the bottom of a binade).  Fresh d_logg by |gamma d_step| band, worst case of all shapes:
    closed-form phi' (e^z - phi) / z everywhere:   < eps 0.15,   eps..10 eps 445,    10..100 eps 56,    >= 100 eps 6.7
    series below |z| = 1 (arcflow_bwd_kernel now):  < eps 0.15,   eps..10 eps 0.12,   10..100 eps 0.16,  >= 100 eps 0.20
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

import arcflow_policy_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
SENT = -768.0
NAMES = ('d_means', 'd_logw', 'd_logg')
BANDS = [('<eps', 0.0, 1.0), ('eps..10eps', 1.0, 10.0), ('10..100eps', 10.0, 100.0), ('>=100eps', 100.0, float('inf'))]


def _guarded(shape, fill=None):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.float32, device='cuda')
    view = buf[GUARD:GUARD + n].view(*shape)
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENT).all() and (buf[-GUARD:] == SENT).all())


def _ratio(err, bound):
    """max err / bound, with 0 / 0 = 0 and x / 0 = inf."""
    r = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    return r.max().item() if r.numel() else 0.0


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sig_args(c, n):
    """The case's sigmas the way the case passes them: python floats, or per-sample [B] tensors."""
    sig = c['sig']
    if c.get('vec'):
        return [sig[:, i].cuda() for i in range(n)]
    assert bool((sig == sig[:1]).all())
    return [float(sig[0, i]) for i in range(n)]


def _run_fwd(ops, c, mode, dev):
    """One launch -> (output on the CPU, guard buffer or None)."""
    if mode == 'step':
        buf, view = _guarded(tuple(c['x'].shape))
        out = ops.arcflow_step(dev['x'], dev['means'], dev['logw'], dev['logg'], *_sig_args(c, 3), out=view)
        assert out.data_ptr() == view.data_ptr()
        return out, buf
    if mode == 'dropout':
        s = c['sig']
        return ops.arcflow_step_dropout(dev['x'], dev['means'], dev['logw'], dev['logg'], s[:, 0].cuda(), s[:, 1].cuda(), s[:, 2].cuda(),
                                        c['drop'].cuda()), None
    return ops.arcflow_velocity(dev['means'], dev['logw'], dev['logg'], *_sig_args(c, 2)), None


def _check_fwd(tag, c, mode, got, again=None):
    m = 'velocity' if mode == 'velocity' else 'step'
    ref, bound = R.forward(c, m)
    assert torch.isfinite(got).all(), tag
    if again is not None:
        assert torch.equal(_bits(got), _bits(again)), tag
    err = (got.double() - ref).abs()
    ratio = _ratio(err, bound)
    print(f'{tag}: max err / bound {ratio:.3f}')
    assert (err <= bound).all(), (tag, ratio)
    if c['sigma_name'] == 'zero_step' and mode != 'velocity':
        assert torch.equal(_bits(got), _bits(c['x'])), tag               # d_step = 0: x, bit for bit
    for mut in R.mutations_for(c, m, 'fwd'):
        mref = R.forward(c, m, mut)[0]
        assert R.moved_fraction(mref, ref, bound, 2.0) >= 0.01, (tag, mut)        # the CPU-side condition again, on the spot
        frac = R.moved_fraction(got.double(), mref, bound)
        assert frac >= 0.01, (tag, mut, frac)
    return ratio


def _dev(c):
    return {k: c[k].cuda() for k in ('x', 'means', 'logw', 'logg', 'g')}


@pytest.mark.parametrize('K,ch,pp', R.STEP_SHAPES)
@pytest.mark.parametrize('B,N', R.TOKENS)
def test_step_dropout_velocity_within_fp32_rounding_of_fp64(B, N, K, ch, pp):
    from arcflow_amd import ops
    worst = 0.0
    for tag, mode, c in R.cases_fwd(B, N, K, ch, pp):
        dev = _dev(c)
        out1, buf1 = _run_fwd(ops, c, mode, dev)
        out2, buf2 = _run_fwd(ops, c, mode, dev)
        torch.cuda.synchronize()
        for buf in (buf1, buf2):
            assert buf is None or _guards_intact(buf), tag
        assert torch.equal(dev['x'].cpu(), c['x']), tag                     # the input is left alone
        worst = max(worst, _check_fwd(tag, c, mode, out1.cpu(), out2.cpu()))
    print(f'B={B} N={N} K={K} ch={ch} pp={pp}: worst max err / bound over the forward cases {worst:.3f}')


def _run_bwd(ops, c, mode, dev, old=None):
    s = c['sig']
    s_end = s[:, 1] if mode == 'velocity' else s[:, 2]
    grads, bufs = None, []
    if old is not None:
        pairs = [_guarded(tuple(o.shape), o.cuda()) for o in old]
        bufs, grads = [p[0] for p in pairs], tuple(p[1] for p in pairs)
    out = ops.arcflow_backward(dev['g'], dev['means'], dev['logw'], dev['logg'], s[:, 0].cuda(), s[:, 1].cuda(), s_end.cuda(),
                               gscale=c['gscale'].cuda(), velocity=mode == 'velocity', grads=grads)
    if grads is not None:
        assert all(o.data_ptr() == g.data_ptr() for o, g in zip(out, grads))
    return out, bufs


def _band_ratios(c, mode, err, bound):
    """max err / bound of d_logg per band of |gamma d_step| / eps (step mode)."""
    if mode != 'step' or err.numel() == 0:
        return {}
    z = R.z_of(c).abs() / R.EPS
    out = {}
    for name, lo, hi in BANDS:
        sel = (z >= lo) & (z < hi)
        if sel.any():
            out[name] = _ratio(err[sel], bound[sel])
    return out


@pytest.mark.parametrize('K,ch,pp', R.BWD_SHAPES)
@pytest.mark.parametrize('B,N', R.TOKENS)
def test_backward_within_fp32_rounding_of_fp64(B, N, K, ch, pp):
    from arcflow_amd import ops
    worst = dict.fromkeys(NAMES, 0.0)
    bands = {}
    failures = []
    for tag, mode, c in R.cases_bwd(B, N, K, ch, pp):
        dev = _dev(c)
        refs, bounds = R.backward(c, mode)
        gen = torch.Generator().manual_seed(K * 1000 + ch * 10 + pp + B)
        old = tuple(torch.randn(r.shape, generator=gen) for r in refs)
        arefs, abounds = R.backward(c, mode, old=old)
        fresh1, _ = _run_bwd(ops, c, mode, dev)
        fresh2, _ = _run_bwd(ops, c, mode, dev)
        acc, bufs = _run_bwd(ops, c, mode, dev, old=old)
        torch.cuda.synchronize()
        assert all(_guards_intact(b) for b in bufs), tag
        muts = R.mutations_for(c, mode, 'bwd')
        mrefs = {mut: dict(zip(NAMES, R.backward(c, mode, mut)[0])) for mut in muts}
        zero_gs = (c['gscale'] == 0).nonzero().flatten().tolist()
        for i, name in enumerate(NAMES):
            got, again, gacc = fresh1[i].cpu(), fresh2[i].cpu(), acc[i].cpu()
            assert torch.isfinite(got).all() and torch.isfinite(gacc).all(), (tag, name)
            assert torch.equal(_bits(got), _bits(again)), (tag, name)                      # no atomics: bit-identical
            for b in zero_gs:
                assert bool((got[b] == 0).all()), (tag, name, 'gscale = 0')
                assert torch.equal(_bits(gacc[b]), _bits(old[i][b])), (tag, name, 'gscale = 0, accumulate')
            err, aerr = (got.double() - refs[i]).abs(), (gacc.double() - arefs[i]).abs()
            ratio, aratio = _ratio(err, bounds[i]), _ratio(aerr, abounds[i])
            worst[name] = max(worst[name], ratio, aratio)
            line = f'{tag} {name}: max err / bound fresh {ratio:.3f} accumulate {aratio:.3f}'
            if name == 'd_logg':
                br = _band_ratios(c, mode, err, bounds[i])
                for k, v in br.items():
                    bands[k] = max(bands.get(k, 0.0), v)
                line += '   by |z| band: ' + ', '.join(f'{k} {v:.3f}' for k, v in br.items())
            print(line)
            if not ((err <= bounds[i]).all() and (aerr <= abounds[i]).all()):
                failures.append((tag, name, ratio, aratio))
            for mut, targets in muts.items():
                if name in targets:
                    assert R.moved_fraction(mrefs[mut][name], refs[i], bounds[i], 2.0) >= 0.01, (tag, mut, name)
                    frac = R.moved_fraction(got.double(), mrefs[mut][name], bounds[i])
                    assert frac >= 0.01, (tag, mut, name, frac)
    print(f'B={B} N={N} K={K} ch={ch} pp={pp}: worst max err / bound ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items())
          + '   d_logg by |z| band: ' + ', '.join(f'{k} {v:.3f}' for k, v in bands.items()))
    assert not failures, failures[:8]


@pytest.mark.parametrize('K,ch,pp', R.BWD_REFUSED)
def test_backward_refuses_the_shapes_it_does_not_take(K, ch, pp):
    """afx_arcflow_backward returns AFX_E_INVALID on ch > 64 and on a pp that is no power of two dividing 64, before its launch."""
    from arcflow_amd import _lib, ops
    c = R.make_case(2, 5, K, ch, pp, False, 'scalar')
    dev = _dev(c)
    for mode in ('step', 'velocity'):
        with pytest.raises(_lib.ArcflowHipError):
            _run_bwd(ops, c, mode, dev)
    torch.cuda.synchronize()


def test_k1_is_refused_before_launch():
    """K = 1 has an empty logg, whose data pointer is null; every entry point checks ``!logg`` first and returns AFX_E_INVALID (the kernels
    would never read it, but the contract is pinned as it is: one component is refused, not computed)."""
    from arcflow_amd import _lib, ops
    c = R.make_case(2, 5, 1, 16, 4, False, 'scalar')
    dev = _dev(c)
    assert c['logg'].numel() == 0 and dev['logg'].data_ptr() == 0 and dev['logg'].bfloat16().contiguous().data_ptr() == 0
    c['vec'] = False
    with pytest.raises(_lib.ArcflowHipError):
        ops.arcflow_step(dev['x'], dev['means'], dev['logw'], dev['logg'], 1.0, 0.9, 0.4)
    with pytest.raises(_lib.ArcflowHipError):
        ops.arcflow_velocity(dev['means'], dev['logw'], dev['logg'], 1.0, 0.9)
    with pytest.raises(_lib.ArcflowHipError):
        _run_fwd(ops, dict(c, drop=torch.zeros(2, 1, dtype=torch.bool)), 'dropout', dev)
    with pytest.raises(_lib.ArcflowHipError):
        _run_bwd(ops, c, 'step', dev)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------------
# AFX_STEP_TPW = 2 and 4: one fresh child process each
_TPW_CHILD = r'''
import os, sys, torch
sys.path.insert(0, os.getcwd())
from arcflow_amd import ops
cases = torch.load(sys.argv[1])
outs = []
for c in cases:
    d = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    s = d['sig']
    if c['mode'] == 'step':
        a = [s[:, i] for i in range(3)] if c['vec'] else [float(c['sig'][0, i]) for i in range(3)]
        o = ops.arcflow_step(d['x'], d['means'], d['logw'], d['logg'], *a)
    elif c['mode'] == 'dropout':
        o = ops.arcflow_step_dropout(d['x'], d['means'], d['logw'], d['logg'], s[:, 0], s[:, 1], s[:, 2], d['drop'])
    else:
        a = [s[:, i] for i in range(2)] if c['vec'] else [float(c['sig'][0, i]) for i in range(2)]
        o = ops.arcflow_velocity(d['means'], d['logw'], d['logg'], *a)
    outs.append(o.cpu())
torch.cuda.synchronize()
torch.save(outs, sys.argv[2])
print('TPW_CHILD_OK', os.environ['AFX_STEP_TPW'], len(outs))
'''


@functools.lru_cache(maxsize=None)
def _tpw_cases():
    out = []
    for B, N in [(2, 5), (3, 43)]:
        out += list(R.cases_fwd(B, N, 16, 64, 4))
    return out


@pytest.mark.parametrize('tpw', [2, 4])
def test_two_and_four_tokens_per_wave(tpw, tmp_path):
    """The TPW = 2 / 4 instantiations of the fast kernel (tail-token clamping, a per-token sample index inside one wave): within the same
    fp64 bound, and within twice the bound of this process's TPW = 1 result."""
    from arcflow_amd import ops
    assert os.environ.get('AFX_STEP_TPW') in (None, '1'), 'this process must run the default TPW = 1'
    cases = _tpw_cases()
    payload = []
    for tag, mode, c in cases:
        keys = ['x', 'means', 'logw', 'logg', 'sig'] + (['drop'] if mode == 'dropout' else [])
        payload.append(dict({k: c[k] for k in keys}, mode=mode, vec=bool(c.get('vec'))))
    torch.save(payload, tmp_path / 'in.pt')
    script = tmp_path / 'tpw_child.py'
    script.write_text(_TPW_CHILD)
    r = subprocess.run([sys.executable, str(script), str(tmp_path / 'in.pt'), str(tmp_path / 'out.pt')], cwd=ROOT,
                       env=dict(os.environ, AFX_STEP_TPW=str(tpw)), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f'TPW_CHILD_OK {tpw} {len(cases)}' in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    outs = torch.load(tmp_path / 'out.pt')
    worst = 0.0
    for (tag, mode, c), got in zip(cases, outs):
        worst = max(worst, _check_fwd(f'TPW={tpw} {tag}', c, mode, got))
        one = _run_fwd(ops, c, mode, _dev(c))[0].cpu()
        _, bound = R.forward(c, 'velocity' if mode == 'velocity' else 'step')
        assert ((got.double() - one.double()).abs() <= 2 * bound).all(), (tag, 'vs TPW = 1')
    print(f'TPW={tpw}: worst max err / bound {worst:.3f} over {len(cases)} cases')


# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,ch,lw,ldy', R.HEAD_SHAPES)
@pytest.mark.parametrize('rows', R.HEAD_ROWS)
def test_head_grad_row(rows, K, ch, lw, ldy):
    """Means, gate and pad columns bit-equal to RNE-bf16 of the fp32 inputs (zero for the pad); logw columns within half a bf16 ulp plus the
    fp32 terms of d_lw - exp(logw_out) sum_k d_lw in fp64 from the same bf16 logw_out; the sum-over-q mutation rejected."""
    from arcflow_amd import ops
    c = R.make_head_case(rows, K, ch, lw, ldy)
    args = [c[k].cuda() for k in ('d_means', 'd_logw', 'd_logg', 'logw_out')]
    dy = ops.head_grad(*args, ldy)
    dy2 = ops.head_grad(*args, ldy)
    torch.cuda.synchronize()
    dy, dy2 = dy.cpu(), dy2.cpu()
    assert dy.shape == (rows, ldy) and torch.equal(dy.view(torch.int16), dy2.view(torch.int16))
    nm, nw, ng = K * ch, K * lw, (K - 1) * lw
    bits = lambda t: t.contiguous().view(torch.int16)
    assert torch.equal(bits(dy[:, :nm]), bits(c['d_means'].reshape(rows, nm).bfloat16()))
    assert torch.equal(bits(dy[:, nm + nw:nm + nw + ng]), bits(c['d_logg'].reshape(rows, ng).bfloat16()))
    assert bool((bits(dy[:, nm + nw + ng:]) == 0).all())
    got = dy[:, nm:nm + nw].reshape(rows, K, lw).double()
    ref, bound = R.head_logw_ref(c)
    err = (got - ref).abs()
    print(f'head_grad rows={rows} K={K} ch={ch} lw={lw} ldy={ldy}: logw columns max err / bound {_ratio(err, bound):.3f}')
    assert torch.isfinite(got).all() and (err <= bound).all(), _ratio(err, bound)
    mref = R.head_logw_ref(c, 'sum_over_q')[0]
    assert R.moved_fraction(mref, ref, bound, 2.0) >= 0.01 and R.moved_fraction(got, mref, bound) >= 0.01
