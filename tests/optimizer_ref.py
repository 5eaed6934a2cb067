"""fp64 reference, derived fp32 error bounds, acceptance rules and input sets of the optimizer and roll-out kernel tests
(test_optimizer_ref_cpu.py, test_hip_optimizer_fp64.py): adamw_kernel, adamw8bit_kernel, ema_kernel, euler_kernel, cfg_kernel of afx_train.hip.

CPU, torch and numpy only.  The references are written from the formulas

    g' = g gscale,  m' = b1 m + (1 - b1) g',  v' = b2 v + (1 - b2) g'^2,
    p' = p (1 - lr wd) - lr (m' / (1 - b1^t)) / (sqrt(v' / (1 - b2^t)) + eps)                       (decoupled weight decay)
    ema' = net + (ema - net) beta,   x_b = x_a + u (sigma_b - sigma_a),   cfg = pos + (pos - neg) (scale - 1)

in float64, from scalars rounded to float32 first (the C ABI takes `float`).

Error model.  u = 2^-24 is the unit roundoff of fp32: every fp32 operation (add, multiply, divide, sqrt -- the build keeps division and
square root correctly rounded) returns exact (1 + d), |d| <= u.  k roundings that act on one term compound to gamma(k) = k u / (1 - k u).
A contracted multiply-add rounds once where the separate operations round twice, so a count made for separate operations holds under either
contraction.  A result below the smallest normal number, 2^-126, is either rounded to a subnormal (absolute error 2^-150) or flushed to zero
(absolute error below 2^-126): every operation whose exact result is not zero adds TINY = 2^-126 to its absolute bound, an operation on
exact zeros adds nothing (0 x, 0 + 0 and 0 / x are exact).  No constant in this file comes from a kernel's output.  All bounds are returned
in units of u: a test asserts |out - ref| <= bound_u * U."""
import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
BLOCK = 256
# glibc documents powf within 1 ulp; one ulp of a value is at most 2 u of it
POWF_ULP = 1.0


def f32(x) -> float:
    """A python scalar as the C ABI's `float` receives it."""
    return float(np.float32(x))


def gamma(k):
    return k * U / (1.0 - k * U)


def _d(t):
    return t.detach().cpu().double()


def _rep(a, n):
    return a.repeat_interleave(BLOCK)[:n]


def bias_corrections(betas, step):
    """(1 - b1^t, 1 - b2^t) in fp64 from the float32-rounded betas."""
    return 1.0 - f32(betas[0]) ** step, 1.0 - f32(betas[1]) ** step


def bias_correction_err(beta, step) -> float:
    """Relative error (absolute number, not in u) of the host's fp32 `1.0f - powf(beta, (float)step)` against 1 - beta^t.
    powf returns beta^t (1 + e), |e| <= 2 u POWF_ULP (+ TINY where it underflows); the subtraction from 1 keeps that absolute error and adds one
    rounding of the difference: |bc32 - bc| <= 2 u POWF_ULP beta^t + TINY + u bc, relative to bc:
        2 POWF_ULP u beta^t / (1 - beta^t)  +  u  (+ TINY / bc)
    the cancellation term is largest at t = 1 (beta / (1 - beta): 9 for 0.9, 19 for 0.95) and vanishes once beta^t underflows to 0, where both
    the fp32 and the fp64 correction are exactly 1."""
    pw = f32(beta) ** step
    if pw == 0.0:
        return 0.0
    bc = 1.0 - pw
    return 2.0 * POWF_ULP * U * pw / bc + U + TINY / bc


# ---------------------------------------------------------------------------------------------------------------------------------------------
# references
def _hyper(lr, betas, eps, wd, gscale):
    return f32(lr), f32(betas[0]), f32(betas[1]), f32(eps), f32(wd), f32(gscale)


def _recurrence(p, g, m, v, lr, step, betas, eps, wd, gscale):
    lr, b1, b2, eps, wd, gs = _hyper(lr, betas, eps, wd, gscale)
    bc1, bc2 = bias_corrections(betas, step)
    gi = g * gs
    m1 = b1 * m + (1.0 - b1) * gi
    v1 = b2 * v + (1.0 - b2) * gi * gi
    p1 = p * (1.0 - lr * wd) - lr * (m1 / bc1) / ((v1 / bc2).sqrt() + eps)
    return p1, m1, v1


def adamw_ref(p, g, m, v, lr, step, betas=(0.9, 0.95), eps=1e-8, wd=0.0, gscale=1.0):
    """One AdamW step in fp64 -> (p', m', v')."""
    return _recurrence(_d(p), _d(g), _d(m), _d(v), lr, step, betas, eps, wd, gscale)


def dequant_ref(codes, absmax, qmap):
    """Block-wise dequantisation in fp64: qmap[code] * absmax[block]."""
    codes = codes.detach().cpu()
    return _d(qmap)[codes.long()] * _rep(_d(absmax), codes.numel())


def _block_max(x):
    n = x.numel()
    nb = (n + BLOCK - 1) // BLOCK
    pad = torch.zeros(nb * BLOCK, dtype=torch.float64)
    pad[:n] = x
    return pad.view(nb, BLOCK).amax(1)


def adamw8bit_ref(p, g, codes1, codes2, absmax1, absmax2, qmap1, qmap2, lr, step, betas=(0.9, 0.95), eps=1e-8, wd=0.0, gscale=1.0):
    """One block-wise 8-bit AdamW step in fp64 from the stored codes and absmax.  -> dict: p, m, v (the UNquantised new moments, which update p),
    m0, v0 (the dequantised old moments), amax1 = max |m'| and amax2 = max v' per block of 256, x1 = m' / amax1 and x2 = v' / amax2 (0 in a
    block whose maximum is 0)."""
    m0, v0 = dequant_ref(codes1, absmax1, qmap1), dequant_ref(codes2, absmax2, qmap2)
    p1, m1, v1 = _recurrence(_d(p), _d(g), m0, v0, lr, step, betas, eps, wd, gscale)
    n = p1.numel()
    a1, a2 = _block_max(m1.abs()), _block_max(v1)
    r1, r2 = _rep(a1, n), _rep(a2, n)
    x1 = torch.where(r1 > 0, m1 / r1.clamp_min(1e-300), torch.zeros_like(m1))
    x2 = torch.where(r2 > 0, v1 / r2.clamp_min(1e-300), torch.zeros_like(v1))
    return dict(p=p1, m=m1, v=v1, m0=m0, v0=v0, amax1=a1, amax2=a2, x1=x1, x2=x2)


def ema_ref(ema, net, beta):
    return _d(net) + (_d(ema) - _d(net)) * f32(beta)


def _per_sample(s, like):
    s = _d(s).flatten()
    return s.expand(like.shape[0]).reshape(-1, *([1] * (like.dim() - 1)))


def euler_ref(x_a, u, sigma_a, sigma_b):
    x_a, u = _d(x_a), _d(u)
    return x_a + u * (_per_sample(sigma_b, x_a) - _per_sample(sigma_a, x_a))


def cfg_ref(pos, neg, scale):
    return _d(pos) + (_d(pos) - _d(neg)) * (f32(scale) - 1.0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# bounds.  Internally absolute; the public functions return them in units of u.
def _nz(*xs):
    """TINY where any of the exact magnitudes is not zero (an operation on exact zeros cannot underflow)."""
    s = sum(x.abs() if torch.is_tensor(x) else abs(x) for x in xs)
    return TINY * (s > 0).double()


def moment_bounds(m0, v0, g, betas, gscale, deq: int = 0):
    """-> (bound of m', bound of v') per element in units of u: |m'_kernel - m'_64| <= bound * U.  m0, v0: the old moments in fp64 (for the 8-bit
    state: the fp64 dequantisation).  deq = 1 adds the rounding of the dequantising product.  The counts:
    m': (2 + deq) on |b1 m0| + 4 on |(1 - b1) g gscale|;  v': (2 + deq) on |b2 v0| + 6 on |(1 - b2) (g gscale)^2|;  + TINY per non-zero operation."""
    b1, b2, gs = f32(betas[0]), f32(betas[1]), f32(gscale)
    m0, v0, g = _d(m0), _d(v0), _d(g)
    #   m': A = b1 m0: [deq] dequantising product, product b1 * m0, the sum                      -> 2 + deq roundings
    #       B = (1 - b1) g gs: 1 - b1, g * gs, their product, the sum                            -> 4 roundings
    a, b = (b1 * m0).abs(), ((1.0 - b1) * g * gs).abs()
    em = gamma(2 + deq) * a + gamma(4) * b + (3 + deq) * _nz(a, b)
    #   v': A = b2 v0: as above                                                                  -> 2 + deq roundings
    #       B = (1 - b2) g'^2: 1 - b2, g' twice (it enters squared), two products, the sum       -> 6 roundings
    a, b = (b2 * v0).abs(), ((1.0 - b2) * (g * gs) ** 2).abs()
    ev = gamma(2 + deq) * a + gamma(6) * b + (4 + deq) * _nz(a, b)
    return em / U, ev / U


def _div_err(a, da, b, db):
    """fl(a' / b') against a / b for |a' - a| <= da, |b' - b| <= db < b, b > 0:
    |a'/b' - a/b| <= da / (b - db) + |a| db / (b (b - db)) = (|a| + da) / (b - db) - |a| / b, then one rounding of the quotient."""
    hi = (a.abs() + da) / (b - db)
    return hi - a.abs() / b + U * hi + _nz(a, da)


def param_bound(p, m1, v1, em_u, ev_u, lr, step, betas, eps, wd):
    """-> bound of p' per element in units of u, from the fp64 p, m', v' and the moment bounds (in u).  The kernel evaluates

        p' = fl( fl(p * fl(1 - fl(lr wd)))  -  fl( fl(lr * fl(m' / bc1)) / fl(fl(sqrt(fl(v' / bc2))) + eps) ) )

    and each step below carries the absolute error of its operands and adds its own rounding (first-order counts, where nothing cancels):
        decay term  |p (1 - lr wd)|:  lr * wd, 1 - (..), the product, the final subtraction                                   4
        update term |lr m^ / den|:    error of m' + error of bc1 + 3 (m' / bc1, lr * (..), the quotient) + the final sub.     m' + bc1 + 4
                                      through den = sqrt(v^) + eps:  (error of v' + error of bc2 + 1) / 2 + 1 (sqrt), weighted by
                                      sqrt(v^) / den, + 1 (the sum)                                                           <= v'/2 + bc2/2 + 2.5
    bc1, bc2: bias_correction_err.  The square root is not Lipschitz at 0, so its operand's error is carried exactly, as
    sqrt(x) - sqrt(max(x - dx, 0)) (>= sqrt(x + dx) - sqrt(x), since sqrt is concave), not linearised."""
    lr, b1, b2, eps, wd, _ = _hyper(lr, betas, eps, wd, 1.0)
    bc1, bc2 = bias_corrections(betas, step)
    e1, e2 = bias_correction_err(betas[0], step), bias_correction_err(betas[1], step)
    p, m1, v1 = _d(p), _d(m1), _d(v1)
    em, ev = em_u * U, ev_u * U
    one = torch.ones_like(p)
    mh, dmh = m1 / bc1, _div_err(m1, em, bc1 * one, bc1 * e1 * one)                  # m^ = m' / bc1
    t = lr * mh
    dt = lr * dmh + U * lr * (mh.abs() + dmh) + _nz(t, dmh)                         # lr * m^ (lr is exact)
    vh, dvh = v1 / bc2, _div_err(v1, ev, bc2 * one, bc2 * e2 * one)                  # v^ = v' / bc2
    s = vh.sqrt()
    ds = s - (vh - dvh).clamp_min(0).sqrt() + U * (vh + dvh).sqrt()                 # sqrt(v^)
    den = s + eps
    dden = ds + U * (den + ds)                                                      # + eps  (ds <= s, so den - dden >= eps (1 - u) - u s ... > 0)
    x = t / den
    dx = _div_err(t, dt, den, dden)                                                 # the update term
    decay = 1.0 - lr * wd
    ddecay = U * (lr * wd) + U * abs(decay) if wd != 0.0 else 0.0                   # fl(1 - fl(lr wd)); 1 - 0 is exact
    pd = p * decay
    dpd = p.abs() * ddecay + U * p.abs() * (abs(decay) + ddecay) + _nz(pd)           # p * decay
    out = pd - x
    return (dpd + dx + U * (out.abs() + dpd + dx)) / U                              # the final subtraction


def adamw_bounds(p, g, m, v, lr, step, betas=(0.9, 0.95), eps=1e-8, wd=0.0, gscale=1.0):
    """-> (p', m', v') bounds in u of one fp32-state AdamW step from the fp32 state p, g, m, v."""
    _, m1, v1 = adamw_ref(p, g, m, v, lr, step, betas, eps, wd, gscale)
    em, ev = moment_bounds(m, v, g, betas, gscale, deq=0)
    return param_bound(p, m1, v1, em, ev, lr, step, betas, eps, wd), em, ev


def norm_bound(x, e_u, amax, da_u, qmap):
    """Bound (in u) of the kernel's fp32 normalised value fl(m'_k / a_k) around x = m' / amax, where |m'_k - m'| <= e, |a_k - amax| <= da:
    the quotient's operand errors and its rounding (_div_err), plus half a rounding of the distance between the two codes that bracket x:
    nearest_code compares fl(x - q[lo-1]) <= fl(q[lo] - x), two subtractions with one rounding each of results that sum to the cell width,
    which moves the decision point by at most u width / 2.  Infinite where da >= amax > 0 (the block maximum is itself inside the noise);
    a block with amax = 0 holds exact zeros and the kernel normalises them to exactly 0."""
    q = _d(qmap)
    n = x.numel()
    a, da, e = _rep(amax, n), _rep(da_u, n) * U, e_u * U
    ok = a > da
    safe_a = torch.where(ok, a, torch.ones_like(a))
    err = torch.where(ok, _div_err(x * safe_a, e, safe_a, torch.where(ok, da, torch.zeros_like(da))), torch.full_like(a, float('inf')))
    err = torch.where(a == 0, torch.zeros_like(a), err)
    idx = torch.searchsorted(q, x.contiguous()).clamp(max=255)
    width = q[idx] - q[(idx - 1).clamp(min=0)]
    return (err + 0.5 * U * width) / U


def code_is_nearest(code, x64, err_x, qmap):
    """The acceptance rule of a stored code: |qmap[code] - x64| <= min_j |qmap[j] - x64| + 2 err_x, per element (err_x absolute).  The kernel
    takes the code nearest to ITS normalised value x_k, |x_k - x64| <= err_x: |q[c] - x64| <= |q[c] - x_k| + err_x <= |q[j] - x_k| + err_x
    <= |q[j] - x64| + 2 err_x for every j.  -> (bool per element, (|q[c] - x64| - min_j) / (2 err_x) per element)."""
    q = _d(qmap)
    code = code.detach().cpu().long()
    d = (q[code] - x64).abs()
    idx = torch.searchsorted(q, x64.contiguous()).clamp(max=255)
    dmin = torch.minimum((q[idx] - x64).abs(), (q[(idx - 1).clamp(min=0)] - x64).abs())
    excess = d - dmin
    ratio = torch.where(excess <= 0, torch.zeros_like(d), excess / (2 * err_x))
    return d <= dmin + 2 * err_x, ratio


def ema_bound(ema, net, beta):
    """fl(net + fl(fl(ema - net) * beta)): the difference and the product round the term |(ema - net) beta| twice, the sum rounds the result once."""
    d = ((_d(ema) - _d(net)) * f32(beta)).abs()
    return (gamma(2) * d + U * (ema_ref(ema, net, beta).abs() + gamma(2) * d) + 2 * _nz(d)) / U


def euler_bound(x_a, u, sigma_a, sigma_b):
    """fl(x_a + fl(u * fl(sigma_b - sigma_a))): two roundings of |u (sigma_b - sigma_a)|, one of the result."""
    d = (euler_ref(x_a, u, sigma_a, sigma_b) - _d(x_a)).abs()
    return (gamma(2) * d + U * (euler_ref(x_a, u, sigma_a, sigma_b).abs() + gamma(2) * d) + 2 * _nz(d)) / U


def cfg_bound(pos, neg, scale):
    """fl(pos + fl(fl(pos - neg) * fl(scale - 1))): three roundings of |(pos - neg) (scale - 1)|, one of the result."""
    d = (cfg_ref(pos, neg, scale) - _d(pos)).abs()
    return (gamma(3) * d + U * (cfg_ref(pos, neg, scale).abs() + gamma(3) * d) + 2 * _nz(d)) / U


# ---------------------------------------------------------------------------------------------------------------------------------------------
# checks shared by the CPU tests (on fp32 restatements and wrong variants) and the GPU tests (on the kernels).  Each returns the worst
# err / bound it saw and raises AssertionError with that figure.
def within(got, ref, bound_u, what):
    """|got - ref| <= bound_u * U for every element (a NaN fails).  -> worst err / bound."""
    got = _d(got)
    err = (got - ref).abs()
    bound = bound_u * U
    ok = err <= bound
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if not bool(ok.all()):
        i = int((~ok).flatten().nonzero()[0])
        raise AssertionError(f'{what}: {int((~ok).sum())} of {ok.numel()} elements beyond the bound, worst err / bound {worst:.3f}; first at {i}: '
                             f'got {got.flatten()[i].item()!r} ref {ref.flatten()[i].item()!r} bound {bound.flatten()[i].item():.3e}')
    return worst


def exact_decay(p, lr, wd):
    """p (1 - lr wd) as fp32 evaluates it, each operation rounded once: what a zero gradient on zero moments must leave, bit for bit."""
    decay = np.float32(1.0) - np.float32(lr) * np.float32(wd)
    return torch.from_numpy(p.detach().cpu().numpy() * decay)


def check_adamw_step(p, g, m, v, got_p, got_m, got_v, lr, step, betas=(0.9, 0.95), eps=1e-8, wd=0.0, gscale=1.0, zero=None, what='adamw'):
    """p, m, v of one fp32-state step per element against adamw_ref started from (p, g, m, v).  zero: elements with g = m = v = 0, which must
    keep m' = v' = 0 and p' = p (1 - lr wd) exactly.  -> dict of worst err / bound."""
    rp, rm, rv = adamw_ref(p, g, m, v, lr, step, betas, eps, wd, gscale)
    bp, bm, bv = adamw_bounds(p, g, m, v, lr, step, betas, eps, wd, gscale)
    out = dict(p=within(got_p, rp, bp, f'{what} p step {step}'), m=within(got_m, rm, bm, f'{what} m step {step}'),
               v=within(got_v, rv, bv, f'{what} v step {step}'))
    if zero is not None and bool(zero.any()):
        gm, gv, gp = got_m.cpu()[zero], got_v.cpu()[zero], got_p.cpu()[zero]
        assert bool((gm == 0).all()) and bool((gv == 0).all()), f'{what} step {step}: zero moments with a zero gradient did not stay zero'
        assert torch.equal(gp, exact_decay(p.cpu()[zero], lr, wd)), f'{what} step {step}: p\' != p (1 - lr wd) where g = m = v = 0'
    return out


def check_adamw8bit_step(p, g, c1, c2, a1, a2, q1, q2, got, lr, step, betas=(0.9, 0.95), eps=1e-8, wd=0.0, gscale=1.0, expect=None,
                         what='adamw8bit'):
    """One block-wise 8-bit step against adamw8bit_ref started from the given codes and absmax.  got = (p', codes1', codes2', absmax1', absmax2').
    Criteria: p' within the AdamW bound from the unquantised fp64 moments; absmax' within the moment bound (its block maximum) of the fp64 block
    maxima; every code passes code_is_nearest with norm_bound; nothing non-finite.  expect (dict, all optional) adds the input set's own:
      zero_blocks [ids]: absmax exactly 0, codes 127 / 0, p' = p (1 - lr wd) exactly;   pos_extreme / neg_extreme [element ids]: codes 255 / 255
      resp. 0 / 255;   small [mask]: codes 127 / 0;   zero_grad True: absmax2' = b2 absmax2 and absmax1' = b1 max|q1[code]| absmax1 (= b1 absmax1
      where the block holds code 255) within the roundings of those products.
    -> dict of worst ratios: p, absmax1, absmax2, code1, code2."""
    gp, gc1, gc2, ga1, ga2 = (t.detach().cpu() for t in got)
    n = gp.numel()
    w = f'{what} step {step}'
    for name, t in (('p', gp), ('absmax1', ga1), ('absmax2', ga2)):
        assert bool(torch.isfinite(t).all()), f'{w}: non-finite {name}'
    r = adamw8bit_ref(p, g, c1, c2, a1, a2, q1, q2, lr, step, betas, eps, wd, gscale)
    em, ev = moment_bounds(r['m0'], r['v0'], g, betas, gscale, deq=1)
    out = dict(p=within(gp, r['p'], param_bound(p, r['m'], r['v'], em, ev, lr, step, betas, eps, wd), f'{w} p'))
    da1, da2 = _block_max(em), _block_max(ev)
    out['absmax1'] = within(ga1, r['amax1'], da1, f'{w} absmax1')
    out['absmax2'] = within(ga2, r['amax2'], da2, f'{w} absmax2')
    for k, codes, x, e, am, da, q in (('code1', gc1, r['x1'], em, r['amax1'], da1, q1), ('code2', gc2, r['x2'], ev, r['amax2'], da2, q2)):
        ex = norm_bound(x, e, am, da, q) * U
        ok, ratio = code_is_nearest(codes, x, ex, q)
        worst = float(ratio.max())
        if not bool(ok.all()):
            i = int((~ok).nonzero()[0])
            raise AssertionError(f'{w} {k}: {int((~ok).sum())} of {n} codes are not the nearest, worst excess / (2 err_x) {worst:.3f}; first at {i}: '
                                 f'code {int(codes[i])} x {x[i].item()!r} err_x {ex[i].item():.3e}')
        out[k] = worst
    ex = expect or {}
    if 'zero_blocks' in ex:
        for b in ex['zero_blocks']:
            sl = slice(b * BLOCK, min((b + 1) * BLOCK, n))
            assert ga1[b] == 0 and ga2[b] == 0, f'{w}: absmax of the all-zero block {b} is {ga1[b].item()}, {ga2[b].item()}'
            assert bool((gc1[sl] == 127).all()) and bool((gc2[sl] == 0).all()), f'{w}: codes of the all-zero block {b} are not the zero codes'
            assert torch.equal(gp[sl], exact_decay(p.cpu()[sl], lr, wd)), f'{w}: p\' != p (1 - lr wd) in the all-zero block {b}'
    if 'pos_extreme' in ex:
        i = ex['pos_extreme']
        assert bool((gc1[i] == 255).all()) and bool((gc2[i] == 255).all()), f'{w}: a positive block extreme is not at code 255 in both books'
    if 'neg_extreme' in ex:
        i = ex['neg_extreme']
        assert bool((gc1[i] == 0).all()) and bool((gc2[i] == 255).all()), f'{w}: a negative block extreme is not at code 0 (signed) / 255 (unsigned)'
    if 'small' in ex:
        i = ex['small']
        assert bool((gc1[i] == 127).all()) and bool((gc2[i] == 0).all()), f'{w}: an element 1e-8 of its block maximum is not at the zero code'
    if ex.get('zero_grad'):
        b1, b2 = f32(betas[0]), f32(betas[1])
        # v: the unsigned book's block maximum sits at code 255 = 1.0: 1.0 * absmax2 is exact, b2 * (..) rounds once, + 0 is exact
        out['zg_absmax2'] = within(ga2, b2 * _d(a2), torch.ones_like(_d(a2)) * b2 * _d(a2) / U * gamma(1), f'{w} absmax2 = b2 absmax2')
        # m: the same where the block holds code 255; a block whose extreme was negative holds code 0 = -0.99297 instead, and its
        # maximum is b1 max|q1[code]| absmax1 after two roundings (the dequantising product, then b1 * (..))
        qa = _block_max(_d(q1)[c1.detach().cpu().long()].abs())
        has1 = qa == 1.0
        ref = b1 * qa * _d(a1)
        out['zg_absmax1'] = within(ga1, ref, torch.where(has1, gamma(1) * ref, gamma(2) * ref) / U, f'{w} absmax1 = b1 max|q| absmax1')
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# input sets of the 8-bit tests: CPU fp32 tensors from fixed seeds, the same for the CPU restatement and the kernel
ADAMW8_N = (256, 257, 511, 4096, 256 * 1031 + 77)
ADAMW8_KINDS = ('logspace', 'zero_block', 'placed_max', 'dynamic_range', 'zero_grad_step')
ADAMW8_HYPER = dict(lr=1e-3, betas=(0.9, 0.95), eps=1e-8, wd=0.01, gscale=0.5)
PLACED_LANES = (0, 63, 64, 127, 128, 255)


def adamw8bit_cases():
    """(n, kind) of every 8-bit case: the all-zero block needs a block on either side, so 3 blocks at least."""
    return [(n, k) for n in ADAMW8_N for k in ADAMW8_KINDS if not (k == 'zero_block' and n < 3 * BLOCK)]


def adamw8bit_case(n, kind):
    """-> (p [n], grads: 4 x [n], expect: 4 x dict) for steps 1..4 from the zero state an AdamW8bitState starts in."""
    gen = torch.Generator().manual_seed(1000 * ADAMW8_KINDS.index(kind) + n % 1000)
    nb = (n + BLOCK - 1) // BLOCK
    p = torch.randn(n, generator=gen)
    ordinary = lambda: torch.randn(n, generator=gen) * torch.logspace(-3, 0, n)        # noqa: E731
    grads, expect = [ordinary() for _ in range(4)], [{} for _ in range(4)]
    if kind == 'zero_block':
        # block 1 sees no gradient in steps 1 and 2 (zero state, zero gradient), then comes back to life in steps 3 and 4
        for t in (0, 1):
            grads[t][BLOCK:2 * BLOCK] = 0.0
            expect[t]['zero_blocks'] = [1]
    elif kind == 'placed_max':
        # block k: the extreme at lane PLACED_LANES[k % 6], positive for even k // 6 and negative for odd; in a partial last block at the last
        # valid lane.  The extreme's gradient is 10 x the largest of the rest, with the same sign in every step, so it stays the extreme of m and v.
        lane = torch.tensor([PLACED_LANES[k % 6] for k in range(nb)])
        if n % BLOCK:
            lane[-1] = n % BLOCK - 1
        idx = torch.arange(nb) * BLOCK + lane
        sign = torch.where((torch.arange(nb) // 6) % 2 == 0, 1.0, -1.0)
        if nb > 1 and nb < 12:
            sign = torch.where(torch.arange(nb) % 2 == 0, 1.0, -1.0)                 # few blocks: alternate, so both signs occur
        for t in range(4):
            s = (1.0, 0.6, 1.7, 0.9)[t]
            grads[t] = (torch.rand(n, generator=gen) * 2 - 1) * s
            grads[t][idx] = 10.0 * s * sign
            expect[t] = dict(pos_extreme=idx[sign > 0], neg_extreme=idx[sign < 0])
    elif kind == 'dynamic_range':
        # block 0 spans 1 .. 1e-9 with one sign pattern in every step (no cancellation between steps): elements at <= 1e-8 of the maximum are
        # below half the smallest non-zero code of either book (2.75e-7 signed, 1.6e-7 unsigned, and v goes with the square)
        mag = torch.logspace(0, -9, BLOCK)[torch.randperm(BLOCK, generator=gen)]
        sgn = torch.where(torch.rand(BLOCK, generator=gen) < 0.5, -1.0, 1.0)
        small = torch.zeros(n, dtype=torch.bool)
        small[:BLOCK] = mag <= 1e-8
        for t in range(4):
            grads[t][:BLOCK] = mag * sgn * (1.0, 0.7, 1.3, 0.9)[t]
            expect[t]['small'] = small
    elif kind == 'zero_grad_step':
        grads[2] = torch.zeros(n)
        expect[2]['zero_grad'] = True
    return p, grads, expect


# ... and of the fp32-state AdamW, EMA, Euler-roll and CFG tests
ADAMW_N = (1, 255, 256, 257, 4133, 256 * 1031 + 77)
ADAMW_STEPS = (1, 2, 3, 100000)                 # at the last both bias corrections are exactly 1
ADAMW_WD_GSCALE = ((0.0, 1.0), (0.01, 0.5))
EMA_N = (1, 257, 256 * 1031 + 77)
EMA_BETAS = (0.0, 0.5, 0.93, 0.9999, 1.0)
EULER_SIGMAS = (torch.tensor([0.9, 0.5, 0.25, 1.0]), torch.tensor([0.7, 0.5, 0.0, 0.03]))      # (sigma_a, sigma_b); sample 1: sigma_a == sigma_b
CFG_SCALES = (1.0, 4.0, 0.0)
ROLL_SHAPES = ((4, 257, 64), (4, 262144))


def adamw_case(n):
    """-> (p, m, v, grads: 4 x [n], zero mask): zero moments (as the trainer starts), gradients randn * logspace(-6, 0), a run of 17 elements
    with g = 0 in every step (so g = m = v = 0 there throughout) and a run of 17 with |g| = 1e-20, where g * g underflows."""
    gen = torch.Generator().manual_seed(7000 + n % 1000)
    p = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * torch.logspace(-6, 0, n) for _ in ADAMW_STEPS]
    zero = torch.zeros(n, dtype=torch.bool)
    if n >= 255:
        zero[n // 4:n // 4 + 17] = True
        for g in grads:
            g[zero] = 0.0
            g[n // 2:n // 2 + 17] = torch.where(torch.rand(17, generator=gen) < 0.5, -1e-20, 1e-20)
    return p, torch.zeros(n), torch.zeros(n), grads, zero


def ema_case(n):
    """-> (ema, net): randn pairs; a run with ema == net (the result is net exactly) and a run with |ema - net| ~ 1e-6 |net|."""
    gen = torch.Generator().manual_seed(8000 + n % 1000)
    ema, net = torch.randn(n, generator=gen), torch.randn(n, generator=gen) + 0.5
    if n >= 255:
        ema[10:40] = net[10:40]
        ema[60:120] = net[60:120] * (1 + 1e-6 * torch.randn(60, generator=gen))
    return ema, net


def roll_case(shape):
    gen = torch.Generator().manual_seed(9000 + len(shape))
    return torch.randn(shape, generator=gen), torch.randn(shape, generator=gen) + 1.0
