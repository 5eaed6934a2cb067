"""fp64 reference, per-element error bounds and mutated references of the ArcFlow policy kernels (no device code in this module).

The kernels (``arcflow_step_kernel``, ``arcflow_step_k16_kernel<., TPW>``, ``arcflow_bwd_kernel``) evaluate, per token and packed channel c with
sub-pixel q = c % pp,

    w_k = softmax_k(logw[k, q])   (dropped components at -inf),      D[c] = sum_k w_k m[k, c] e_k,
    step:      e_0 = d_step,  e_k = exp(g_k d_past) d_step phi(g_k d_step),      x_end = x - D
    velocity:  e_0 = 1,       e_k = exp(g_k d_past),                             u = D
    d_past = s_src - s_start,  d_step = s_start - s_end,  phi(z) = expm1(z_s) / z_s,  z_s = sgn(z) max(|z|, eps),  sgn(0) = +1,

and the gradients of  sum_c gD[c] D[c],  gD = gscale[b] g[c]:

    d_means[k, c] = gD w_k e_k,          r_k[q] = sum_{c: c % pp = q} gD m[k, c],      a_k = e_k r_k,      s = sum_j w_j a_j,
    d_logw[k, q]  = w_k (a_k - s),       d_logg[k-1, q] = w_k e'_k r_k,
    step:  e'_k = d_past e_k + exp(g_k d_past) d_step^2 phi'(g_k d_step)      velocity:  e'_k = d_past e_k,
    phi'(z) = (e^z - phi(z)) / z outside the clamp and phi' = 0 inside it (|z| < eps: z_s does not move with z there; the kernel's convention
    and torch autograd's through the clamp).

Everything here is torch fp64 on the CPU, evaluated from the SAME inputs the kernel gets: the fp32 or bf16 mixture tensors (logw and logg already
rounded the way ``ops._mix_dtype`` rounds them), fp32 x, g, gscale and sigmas, and the fp32 value of eps.  fp64 phi' switches to its series
sum_n z^n / (n! (n + 2)) below |z| = 0.5, where the closed form would lose 1e-16 * 4 / |z| itself.

Error bounds
------------
u = 2^-24 (half an ulp of fp32 round-to-nearest).  Every rounding of the kernel perturbs the output by at most u times the MAGNITUDE of the value
it rounds, carried to the output through the factors that follow.  In units of u, per component k and sub-pixel q (R_* are relative):

  softmax   l_k = fl(logw_k - max): u |logw_k - max|, which the exponential turns into a relative error A_k = |logw_k - max| (argument
            conditioning), then expf: XE.  den = sum of K positive terms, in sequence: K - 1, and it inherits the weighted errors of its terms,
            Asoft + XE with Asoft = sum_j w_j A_j.  1 / den: 1.  p_k * inv: 1.
                R_w(k) = A_k + Asoft + 2 XE + K + 1          (w_k = 0, a component at -inf, is exact: A_k := 0 there)
  decay     d_past = fl(s_src - s_start): 1, g d_past: 1, both act on the argument: 2 |g_k d_past|; expf: XE.
                R_dec(k) = 2 |g_k d_past| + XE
  phi       z = fl(g fl(d_step)): 2 relative on z, and |z phi'(z) / phi(z)| <= |z| (phi' / phi lies in (0, 1)): 2 |z| outside the clamp, 0 inside it
            (z_s = +-eps exactly; the sign of fl(z) is the sign of z).  expm1f: XM.  The division: 1.
                R_phi(k) = 2 |z| [unclamped] + XM + 1
  e_k       step: e_0 = fl(d_step): 1;   e_k = dec * d_step * phi: R_dec + R_phi + 1 (d_step) + 2 (products).   velocity: e_0: 0;  e_k: R_dec.
  D         t_k = w_k e_k m[k, c] costs two more products: R_w + R_e + 2.  The K terms are summed in sequence (or in a tree of depth <= 5 in
            the K = 16 kernel): (K - 1) S with S = sum_k |t_k|;  x - D: |x| + S.  One more S covers the second-order terms:
                |err x_end| <= u [ sum_k |t_k| (R_w + R_e + 2) + (K + 1) S + |x| ]        (velocity: without the |x| + S of the subtraction)
  gD        fl(gscale g): 1.
  d_means   one product of five factors:  |err| <= u |gD w_k e_k| (1 + R_w + R_e + 2 + 1)      (the last 1: second order)
  r_k       products gD m: 1 + 1 (gD); xor-shuffle tree of depth L = log2(64 / pp): L.  With Rabs_k = sum_{c in q} |gD m[k, c]|:
                |err r_k| <= u (2 + L) Rabs_k,       Aabs_k = |e_k| Rabs_k,       |err a_k| <= u C_a(k) Aabs_k,   C_a = 2 + L + R_e + 1
  s         products w_j a_j: R_w + 1, summed in sequence: K - 1.  Sabs = sum_j w_j Aabs_j:
                |err s| <= u sum_j w_j Aabs_j (C_a(j) + R_w(j) + K)
  d_logw    w_k (a_k - s): the subtraction rounds |a_k - s| <= Aabs_k + Sabs, the product 1, w_k brings R_w:
                |err| <= u w_k [ Aabs_k C_a(k) + sum_j w_j Aabs_j (C_a(j) + R_w(j) + K) + (Aabs_k + Sabs) (R_w(k) + 3) ]
            -- built from sum_j |w_j a_j| + |a_k|, never from a_k - s itself.
  d_logg    e'_k = fl(T1 + T2),  T1 = d_past e_k: 1 (d_past) + R_e + 1;  T2 = dec d_step phi' d_step: R_dec + 2 (d_step twice) + 3 (products) + C_dphi;
            the sum: 1.  Then w_k e'_k r_k: R_w + 2 products + the (2 + L) of r_k, all on (|T1| + |T2|) Rabs_k, one more for second order:
                |err| <= u w_k Rabs_k [ |T1| (R_e + 2) + |T2| (R_dec + 5 + C_dphi) + (|T1| + |T2|) (R_w + L + 6) ]
  phi'      C_dphi is the budget of a phi' that is accurate to a few u RELATIVE.  Its argument conditioning is 2 |z| (phi'' / phi' lies in (0, 1)
            like phi' / phi).  The closed form (em1 + 1 - phi) / z_s rounds em1 (XM |em1|), e^z = fl(em1 + 1) (e^z), phi (XM + 1) phi, the
            difference and the quotient (2):   kappa(z) = (XM |em1| + e^z + (XM + 1) phi) / |e^z - phi| + 2.
            For |z| >= 1 nothing cancels and kappa is small (25 at z = 1 and 31 at z = -1 with XM = 5.3, falling for z > 0; for z < 0 it grows again
            as XM |z|, because em1 -> -1 carries an absolute error XM u into e^z - phi -> 1 / |z|: a conditioning of the same kind as 2 |z|).
                C_dphi(z) = kappa(sgn(z) max(|z|, 1)) + 2 |z|
            Below |z| = 1 it is frozen at its |z| = 1 value.  Towards z = 0 the closed form's kappa grows as 4 / |z| -- the cancellation of two
            numbers near 1 -- and the bound does NOT follow it: a phi' that loses u / |z| fails this bound, as it should.
  accumulate (grads=...): fl(old + v) adds u (|old| + |v|), |v| taken as the magnitude sums above.

Where hipcc contracts a multiply-add into an fma a rounding disappears; the K = 16 forward kernel sums in trees and divides once where the generic
one multiplies by a reciprocal: the bounds stay upper bounds for all three kernels.

Device math functions.  The HIP math-function accuracy table is not part of the ROCm installation this suite is developed on, so expf, expm1f and
logf were measured once on an MI355X (hipcc -O3, the project's flags, 2^23 arguments per range against fp64): see ULP_MEASURED below.  The
allowance is twice the measured maximum; 1 ulp is at most 2 u relative, so XE = 2 * ULP_ALLOW['expf'], XM = 2 * ULP_ALLOW['expm1f'].  (logf is
used by the head split only and enters no bound here; its figure is recorded for completeness.)

Mutations.  ``MUTATIONS`` names one realistic slip each; ``mutations_for`` lists, for a case, the ones that can act on it and the outputs they
target, and says why the others are left out.
"""
import math

import torch

U = 2.0 ** -24
EPS = float(torch.tensor(1e-4, dtype=torch.float32))          # the kernels' fp32 eps (python's 1e-4 after ctypes' c_float)

# measured maximum ulp error (MI355X, hipcc -O3, 2^23 arguments per range): expf 0.8452 on [-40, 0] and 0.8576 on [-10, 10]; expm1f 1.3365 on
# +[5e-5, 10] and 0.8808 on -[5e-5, 10] (log-spaced); logf 2.3006 on [1, 64] and 2.1439 on [1e-6, 1] (log-spaced)
ULP_MEASURED = {'expf': 0.8576, 'expm1f': 1.3365, 'logf': 2.3006}
ULP_ALLOW = {k: 2.0 * v for k, v in ULP_MEASURED.items()}
XE = 2.0 * ULP_ALLOW['expf']
XM = 2.0 * ULP_ALLOW['expm1f']

MUTATIONS = ('swap_past_step', 'q_div', 'gate_off_by_one', 'nb_sigma', 'nb_drop', 'unsigned_clamp', 'e0_one', 'no_w_factor', 'nb_gscale')


def kappa(z):
    """Worst-case relative error (in u) of the closed form (em1 + 1 - phi) / z evaluated in fp32 with an XM-accurate expm1f (fp64 tensor or
    float in, fp64 tensor out)."""
    z = torch.as_tensor(z, dtype=torch.float64)
    em1 = torch.expm1(z)
    phi = em1 / z
    return (XM * em1.abs() + torch.exp(z) + (XM + 1) * phi) / (torch.exp(z) - phi).abs() + 2.0


def c_dphi(z: torch.Tensor) -> torch.Tensor:
    """The relative error budget of phi' in u (see the module docstring): the closed form's where |z| >= 1, frozen at |z| = 1 below."""
    sgn = torch.where(z < 0, -1.0, 1.0)
    return kappa(sgn * z.abs().clamp(min=1.0)) + 2 * z.abs()


def dphi64(zs: torch.Tensor) -> torch.Tensor:
    """phi'(z) in fp64: series below |z| = 0.5 (24 terms: 0.5^24 / 24! is far below 1e-16), closed form above."""
    small = zs.abs() < 0.5
    zz = torch.where(small, zs, torch.zeros_like(zs))
    ser = torch.zeros_like(zs)
    for n in range(23, -1, -1):
        ser = ser * zz + 1.0 / (math.factorial(n) * (n + 2))
    zl = torch.where(small, torch.ones_like(zs), zs)
    closed = (torch.exp(zl) - torch.expm1(zl) / zl) / zl
    return torch.where(small, ser, closed)


def qmap(ch: int, pp: int, mutate=None) -> torch.Tensor:
    c = torch.arange(ch)
    return c // (ch // pp) if mutate == 'q_div' else c % pp


def _terms(c, mode, mutate=None, autograd=False):
    """Everything both directions share, in fp64.  c: dict(means, logw, logg, sig [B, 3] fp32, drop [B, K] bool or None).  mode 'step' |
    'velocity' (velocity ignores sig[:, 2]: the kernel is called with s_end = s_start, d_step = 0, and never reads it)."""
    m, lw, gam = c['means'].double(), c['logw'].double(), c['logg'].double()
    if autograd:
        m, lw, gam = (t.clone().requires_grad_(True) for t in (m, lw, gam))
    leaves = (m, lw, gam)
    B, N, K, ch = m.shape
    pp = lw.shape[-1]
    sig = c['sig'].double()
    if mutate == 'nb_sigma':
        sig = sig.roll(1, 0)
    d_past = (sig[:, 0] - sig[:, 1]).reshape(B, 1, 1, 1)
    d_step = (sig[:, 1] - sig[:, 2]).reshape(B, 1, 1, 1) if mode == 'step' else torch.zeros(B, 1, 1, 1, dtype=torch.float64)
    if mutate == 'swap_past_step':
        d_past, d_step = d_step, d_past
    drop = c.get('drop')
    if drop is not None:
        if mutate == 'nb_drop':
            drop = drop.roll(1, 0)
        lw = lw.masked_fill(drop.reshape(B, 1, K, 1), float('-inf'))
    mx = lw.detach().amax(dim=2, keepdim=True)
    w = torch.softmax(lw, dim=2)
    if mutate == 'gate_off_by_one':
        gam = gam.roll(1, 2)
    dec = torch.exp(gam * d_past)
    z = gam * d_step
    clamped = z.detach().abs() < EPS
    sgn = torch.where(z.detach() < 0, -1.0, 1.0)
    if mutate == 'unsigned_clamp':
        zs, dsgn = z.abs().clamp(min=EPS), sgn                    # d z_s / d z = sgn(z) there
    else:
        zs, dsgn = sgn * z.abs().clamp(min=EPS), 1.0
    one = torch.ones(B, N, 1, pp, dtype=torch.float64)
    if mode == 'step':
        phi = torch.expm1(zs) / zs
        dphi = torch.where(clamped, torch.zeros_like(zs), dphi64(zs.detach()) * dsgn)
        e0 = one if mutate == 'e0_one' else d_step * one
        ek = dec * d_step * phi
        T1, T2 = d_past * ek, dec * d_step * d_step * dphi
    else:
        e0, ek = one, dec
        T1, T2 = d_past * ek, torch.zeros_like(ek)
    e = torch.cat([e0, ek], dim=2)
    zero = torch.zeros_like(one)
    # relative error budgets (units of u) -- from the UNMUTATED magnitudes of this evaluation (the bound is only used with mutate=None)
    wd, zd = w.detach(), z.detach()
    A = torch.where(wd > 0, (lw.detach() - mx).abs(), torch.zeros_like(wd))
    A = torch.where(torch.isfinite(A), A, torch.zeros_like(A))
    Rw = A + (wd * A).sum(2, keepdim=True) + 2 * XE + K + 1
    Rdec = 2 * (gam.detach() * d_past).abs() + XE
    if mode == 'step':
        Rphi = torch.where(clamped, torch.zeros_like(zd), 2 * zd.abs()) + XM + 1
        Re = torch.cat([one, Rdec + Rphi + 3], dim=2)
    else:
        Re = torch.cat([zero, Rdec], dim=2)
    Cdphi = c_dphi(zd)
    return dict(m=m, w=w, e=e, T1=torch.cat([zero, T1], 2), T2=torch.cat([zero, T2], 2), Rw=Rw, Re=Re, Rdec=torch.cat([zero, Rdec], 2),
                Cdphi=torch.cat([zero, Cdphi], 2), z=zd, clamped=clamped, leaves=leaves, B=B, N=N, K=K, ch=ch, pp=pp)


def forward(c, mode, mutate=None):
    """-> (x_end [step] or u [velocity], bound), both [B, N, ch] fp64."""
    t = _terms(c, mode, mutate)
    q = qmap(t['ch'], t['pp'], mutate)
    K = t['K']
    T = t['w'][..., q] * t['e'][..., q] * t['m']
    D = T.sum(2)
    S = T.abs().sum(2)
    bound = (T.abs() * (t['Rw'] + t['Re'] + 2)[..., q]).sum(2) + K * S
    if mode == 'velocity':
        return D, U * bound
    x = c['x'].double()
    return x - D, U * (bound + S + x.abs())


def forward_autograd_grads(c, mode):
    """torch fp64 autograd of sum gD D through the fp64 forward -> (d_means, d_logw, d_logg)."""
    t = _terms(c, mode, autograd=True)
    q = qmap(t['ch'], t['pp'])
    D = (t['w'][..., q] * t['e'][..., q] * t['m']).sum(2)
    (_gD(c) * D).sum().backward()
    return tuple(leaf.grad for leaf in t['leaves'])


def _gD(c, mutate=None):
    B = c['g'].shape[0]
    gs = c.get('gscale')
    gs = torch.ones(B, dtype=torch.float64) if gs is None else gs.double()
    if mutate == 'nb_gscale':
        gs = gs.roll(1, 0)
    return gs.reshape(B, 1, 1) * c['g'].double()


def backward(c, mode, mutate=None, old=None):
    """Analytic fp64 gradients -> ((d_means, d_logw, d_logg), (their bounds)).  old = (o_means, o_logw, o_logg): the accumulate form
    (reference old + gradient, bound + u (|old| + |gradient's magnitude|))."""
    t = _terms(c, mode, mutate)
    K, ch, pp = t['K'], t['ch'], t['pp']
    q = qmap(ch, pp, mutate)
    Q = torch.zeros(ch, pp, dtype=torch.float64)
    Q[torch.arange(ch), q] = 1.0
    L = math.log2(64 // pp) if 64 % pp == 0 else 6.0
    gD = _gD(c, mutate)[:, :, None, :]
    w, e, m, Rw, Re = t['w'], t['e'], t['m'], t['Rw'], t['Re']
    d_means = gD * w[..., q] * e[..., q]
    b_means = d_means.abs() * (Rw + Re + 4)[..., q]
    r = (gD * m) @ Q
    Rabs = (gD * m).abs() @ Q
    a = e * r
    s = (w * a).sum(2, keepdim=True)
    d_logw = (a - s) if mutate == 'no_w_factor' else w * (a - s)
    Aabs = e.abs() * Rabs
    Ca = Re + L + 3
    Sabs = (w * Aabs).sum(2, keepdim=True)
    m_logw = w * (Aabs + Sabs)
    b_logw = w * (Aabs * Ca + (w * Aabs * (Ca + Rw + K)).sum(2, keepdim=True) + (Aabs + Sabs) * (Rw + 3))
    de = t['T1'] + t['T2']
    T1, T2 = t['T1'].abs(), t['T2'].abs()
    d_logg = (w * de * r)[:, :, 1:]
    m_logg = (w * Rabs * (T1 + T2))[:, :, 1:]
    b_logg = (w * Rabs * (T1 * (Re + 2) + T2 * (t['Rdec'] + 5 + t['Cdphi']) + (T1 + T2) * (Rw + L + 6)))[:, :, 1:]
    outs, bounds, mags = [d_means, d_logw, d_logg], [b_means, b_logw, b_logg], [d_means.abs(), m_logw, m_logg]
    if old is not None:
        for i in range(3):
            o = old[i].double()
            outs[i] = o + outs[i]
            bounds[i] = bounds[i] + o.abs() + mags[i]
    return tuple(outs), tuple(U * b for b in bounds)


def z_of(c):
    """gamma * d_step in fp64 (step mode) -> [B, N, K-1, pp]."""
    sig = c['sig'].double()
    return c['logg'].double() * (sig[:, 1] - sig[:, 2]).reshape(-1, 1, 1, 1)


def mutations_for(c, mode, kind):
    """{mutation: targeted outputs} for the mutations that CAN act on case c.  kind 'fwd' (targets ('out',)) or 'bwd' (targets among
    'd_means', 'd_logw', 'd_logg').  Left out, and why:
      swap_past_step    where d_past = d_step for every sample (then nothing changes), and in velocity mode where d_past = 0 (both are 0);
      q_div             where c // (ch / pp) = c % pp for every channel: pp = 1 and pp = ch; a dropout step whose samples all keep component 0 only;
      gate_off_by_one   K <= 2 (no second gate to read instead), and where the gates do not matter (d_past = d_step = 0; velocity: d_past = 0);
      nb_sigma          B = 1, or every sample has the same (d_past, d_step) (scalar sigmas), or velocity with equal d_past;
      nb_drop           no drop mask, B = 1, d_step = 0;
      unsigned_clamp    velocity mode (no phi), d_step = 0, a dropout step whose samples all keep component 0 only;
      e0_one            velocity mode (e_0 = 1 is right there); never targets d_logg, which e_0 does not enter;
      no_w_factor       forward (there is no a_k - s); backward with every gradient zero (step mode at d_step = 0);
      nb_gscale         forward, B = 1, or equal gscale entries;
      (any, on d_logg)  velocity mode at d_past = 0 for every sample: e'_k = d_past e_k makes d_logg identically zero.
    A step at d_step = 0 returns x bit for bit, so only e0_one can act on it."""
    B, N, K, ch = c['means'].shape
    pp = c['logw'].shape[-1]
    sig = c['sig'].double()
    d_past = sig[:, 0] - sig[:, 1]
    d_step = sig[:, 1] - sig[:, 2] if mode == 'step' else torch.zeros(B, dtype=torch.float64)
    all_out = ('out',) if kind == 'fwd' else ('d_means', 'd_logw', 'd_logg')
    live = bool((d_step != 0).any()) if mode == 'step' else True
    gates_matter = K >= 2 and (bool((d_past != 0).any()) or (mode == 'step' and live))
    out = {}
    if K >= 2 and live and bool((d_past != d_step).any()) and (mode == 'step' or bool((d_past != 0).any())):
        out['swap_past_step'] = all_out
    drop = c.get('drop')
    q_seen = True                    # a sample whose only live component is k = 0 has w = 1 and no gate: no sub-pixel index enters
    if drop is not None:
        q_seen = any(not bool(drop[b, 1:].all()) for b in range(B))
    if live and q_seen and bool((qmap(ch, pp) != qmap(ch, pp, 'q_div')).any()):
        out['q_div'] = all_out
    if K >= 3 and live and gates_matter:
        out['gate_off_by_one'] = all_out
    dd = torch.stack([d_past, d_step], 1)
    if B > 1 and live and bool((dd != dd.roll(1, 0)).any()) and (mode == 'step' or (K >= 2 and bool((d_past != d_past.roll(1, 0)).any()))):
        out['nb_sigma'] = all_out
    if kind == 'fwd' and drop is not None and B > 1 and live and bool((drop != drop.roll(1, 0)).any()):
        out['nb_drop'] = all_out
    if mode == 'step' and live and K >= 2 and q_seen:
        out['unsigned_clamp'] = all_out
    if mode == 'step':
        out['e0_one'] = ('out',) if kind == 'fwd' else ('d_means', 'd_logw')
    if kind == 'bwd' and live and K >= 2:
        out['no_w_factor'] = ('d_logw',)
    gs = c.get('gscale')
    if kind == 'bwd' and B > 1 and gs is not None and bool((gs != gs.roll(1, 0)).any()) and (live or mode == 'velocity'):
        out['nb_gscale'] = all_out if live else ('d_means', 'd_logw')
    if kind == 'bwd' and mode == 'velocity' and not bool((d_past != 0).any()):        # e'_k = d_past e_k: d_logg is identically 0 there
        out = {k: tuple(t for t in v if t != 'd_logg') for k, v in out.items()}
    return out


# --------------------------------------------------------------------------------------------------------------------------------------
# the cases: token counts, mixture shapes, sigmas, inputs (shared by the CPU and the GPU test files)
TOKENS = [(1, 1), (2, 5), (3, 43)]
STEP_SHAPES = [(16, 64, 4), (2, 16, 4), (8, 64, 1), (32, 64, 4), (16, 128, 4), (16, 64, 16), (16, 32, 4), (5, 12, 3)]
VELOCITY_SHAPES = STEP_SHAPES                                        # the velocity is the same launch: it takes (5, 12, 3) as the step does
BWD_SHAPES = [s for s in STEP_SHAPES if s not in ((16, 128, 4), (5, 12, 3))] + [(4, 64, 64)]
BWD_REFUSED = [(16, 128, 4), (5, 12, 3)]
# (name, s_src, s_start, s_end, pass per-sample vectors?); the per-sample case lists up to three samples
SIGMAS = [('scalar_src_eq_start', (1.0,) * 3, (1.0,) * 3, (0.7619,) * 3, False),
          ('scalar', (1.0,) * 3, (0.9,) * 3, (0.4,) * 3, False),
          ('per_sample', (1.0, 0.8, 0.9), (0.9, 0.55, 0.7), (0.4, 0.1, 0.0), True),
          ('vector_equal', (1.0,) * 3, (0.9,) * 3, (0.4,) * 3, True),
          ('zero_step', (0.5,) * 3, (0.5,) * 3, (0.5,) * 3, False)]
PLANTS = [0.0, 0.5, -0.5, 0.9, -0.9, 1.1, -1.1, 2.0, -2.0, 10.0, -10.0, 100.0, -100.0, 1000.0, -1000.0]      # gamma d_step, in units of eps
BIG_GATES = [8.0, -8.0]


def sigma_tensor(name, B):
    _, a, b, e, _ = next(s for s in SIGMAS if s[0] == name)
    return torch.tensor([a[:B], b[:B], e[:B]], dtype=torch.float32).T.contiguous()


def drop_mask(B, K):
    """Sample 0 untouched, sample 1 with K - 1 components dropped (K // 2 survives), sample 2 with two dropped; B = 1: its only sample has
    components dropped (two, or one at K = 2).  A fully dropped sample is out of scope: the trainer's mask never produces one."""
    d = torch.zeros(B, K, dtype=torch.bool)
    if B == 1:                        # component 0 stays: it is the one e_0 belongs to
        d[0, 1 % K] = True
        if K > 2:
            d[0, K - 1] = True
        return d
    d[1] = True
    d[1, K // 2] = False
    if B > 2:
        d[2, 1 % K] = True
        if K > 2:
            d[2, K - 2] = True
    return d


def make_case(B, N, K, ch, pp, bf16, sigma_name, seed_extra=0, neg_inf=True):
    """Inputs of one case on the CPU: means / logw / logg in the mixture dtype (fp32, or bf16 with logw and logg rounded as ops._mix_dtype
    does), fp32 x, g, gscale, sig.  Gates are N(0, 1) with planted entries at gamma d_step = PLANTS * eps (of the sample's own d_step) and
    gamma = +-8; logw is a log-softmax of N(0, 2^2) draws with about 4 % of the entries at -inf (never a whole row; none with neg_inf=False:
    the dropout step's logw is a finite log-softmax, and a -inf under the one surviving component would drop the whole sample)."""
    gen = torch.Generator().manual_seed(7919 * B + 104729 * N + 31 * K + 7 * ch + pp + 1000003 * seed_extra)
    dt = torch.bfloat16 if bf16 else torch.float32
    sig = sigma_tensor(sigma_name, B)
    x = torch.randn(B, N, ch, generator=gen)
    means = torch.randn(B, N, K, ch, generator=gen)
    raw = 2.0 * torch.randn(B, N, K, pp, generator=gen)
    kill = torch.rand(B, N, K, pp, generator=gen) < 0.04
    keep = torch.randint(0, K, (B, N, 1, pp), generator=gen)
    kill.scatter_(2, keep, torch.zeros_like(keep, dtype=torch.bool))
    if not neg_inf:
        kill[:] = False
    logw = torch.log_softmax(raw.masked_fill(kill, float('-inf')), dim=2)
    logg = torch.randn(B, N, K - 1, pp, generator=gen)
    d_step = (sig[:, 1].double() - sig[:, 2].double())
    per = N * (K - 1) * pp
    plants = [('z', p) for p in PLANTS] + [('g', v) for v in BIG_GATES]
    n_plant = min(len(plants) * 2, per // 2)
    for b in range(B):
        pos = torch.randperm(per, generator=gen)[:n_plant]
        flat = logg[b].reshape(-1)
        for i, p in enumerate(pos.tolist()):
            kind, v = plants[(i + b + N + K) % len(plants)]
            if kind == 'g':
                flat[p] = v
            elif d_step[b] != 0:
                flat[p] = v * EPS / d_step[b].item()
    g = torch.randn(B, N, ch, generator=gen)
    gscale = torch.tensor([[-1.3], [0.0, -1.3], [0.7, 0.0, -1.3]][B - 1], dtype=torch.float32)
    return dict(x=x, means=means.to(dt), logw=logw.to(dt), logg=logg.to(dt), sig=sig, g=g, gscale=gscale, drop=None, bf16=bf16,
                sigma_name=sigma_name)


def z_is_clear_of_eps(c) -> bool:
    """No |gamma d_step|, drawn or planted, within 2^-18 relative of eps: there the clamp decision of fp32 fl(gamma d_step) and of fp64 can
    differ, and phi' is discontinuous.  (The planted 0.9 eps and 1.1 eps are 10 % away by construction; the bf16 rounding of gamma moves
    them by at most 2^-9 relative.)"""
    return bool(((z_of(c).abs() / EPS - 1).abs() > 2.0 ** -18).all())


# --------------------------------------------------------------------------------------------------------------------------------------
# head_grad
HEAD_SHAPES = [(16, 64, 4, 1152), (8, 16, 2, 192)]
HEAD_ROWS = [1, 3, 257]


def make_head_case(rows, K, ch, lw, ldy):
    gen = torch.Generator().manual_seed(rows * 131 + K * 17 + ch + lw)
    d_means = torch.randn(1, rows, K, ch, generator=gen)
    d_logw = torch.randn(1, rows, K, lw, generator=gen)
    d_logg = torch.randn(1, rows, K - 1, lw, generator=gen)
    logw_out = torch.log_softmax(2.0 * torch.randn(1, rows, K, lw, generator=gen), dim=2).bfloat16()
    return dict(d_means=d_means, d_logw=d_logw, d_logg=d_logg, logw_out=logw_out, ldy=ldy)


def head_logw_ref(c, mutate=None):
    """fp64  d_lw - exp(logw_out) sum_k d_lw  from the same bf16 logw_out -> (value, bound) [rows, K, lw].
    Roundings: the K-term sum in sequence ((K - 1) u sum_k |d_lw|), expf (XE u, its argument is exact), the product p s (1), the subtraction
    (|d_lw| + |p s|), one unit for second order, and the bf16 store: half a bf16 ulp, at most 2^-8 relative (bf16 keeps 8 significant bits), of the value's magnitude (taken with
    the fp32 error on top, as the store rounds the fp32 result, not the exact one).  mutate 'sum_over_q': the sum runs over the sub-pixels."""
    d, p = c['d_logw'][0].double(), torch.exp(c['logw_out'][0].double())
    K = d.shape[1]
    s = d.sum(2, keepdim=True) if mutate == 'sum_over_q' else d.sum(1, keepdim=True)
    sabs = d.abs().sum(1, keepdim=True)
    ref = d - p * s
    f32 = U * (p * sabs * (K - 1 + XE + 1 + 1) + d.abs() + p * sabs)
    return ref, f32 + 2.0 ** -8 * (ref.abs() + f32)


# --------------------------------------------------------------------------------------------------------------------------------------
# case lists of the two test files
def cases_fwd(B, N, K, ch, pp, sigma_names=None):
    """(tag, mode, case): mode 'step' | 'dropout' | 'velocity'."""
    for bf16 in (False, True):
        for name, _, _, _, vec in SIGMAS:
            if sigma_names is not None and name not in sigma_names:
                continue
            c = make_case(B, N, K, ch, pp, bf16, name)
            c['vec'] = vec
            tag = f'B{B} N{N} K{K} ch{ch} pp{pp} {"bf16" if bf16 else "fp32"} {name}'
            yield tag + ' step', 'step', c
            if name in ('scalar', 'per_sample', 'zero_step'):
                yield tag + ' dropout', 'dropout', dict(make_case(B, N, K, ch, pp, bf16, name, seed_extra=2, neg_inf=False), drop=drop_mask(B, K), vec=True)
            if (K, ch, pp) in VELOCITY_SHAPES:
                yield tag + ' velocity', 'velocity', c


def cases_bwd(B, N, K, ch, pp):
    """(tag, mode, case): mode 'step' | 'velocity'."""
    for bf16 in (False, True):
        for name, _, _, _, _ in SIGMAS:
            if name == 'vector_equal':          # the backward wrapper always passes per-sample vectors: same call as 'scalar'
                continue
            c = make_case(B, N, K, ch, pp, bf16, name, seed_extra=1)
            tag = f'B{B} N{N} K{K} ch{ch} pp{pp} {"bf16" if bf16 else "fp32"} {name}'
            yield tag + ' step', 'step', c
            if name in ('scalar', 'per_sample', 'zero_step'):
                yield tag + ' velocity', 'velocity', c


def moved_fraction(a, b, bound, factor=1.0):
    return ((a - b).abs() > factor * bound).double().mean().item()
