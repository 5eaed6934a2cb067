"""fp64 references of ``afx_lora_row_gain`` and ``afx_lora_fold_rows`` (include/arcflow_hip.h) with per-element bounds, derived by counting
roundings the way tests/lora_fold_ref.py does.  u = 2^-24, gamma(n) = n u / (1 - n u) >= (1 + u)^n - 1.

1. The row gain.   g[o] = m[o] / sqrt( sum_i v[o, i]^2 ),  v = w + s B A.

   The kernel forms v as the fold forms its fp32 sum for ONE adapter: ``lora_fold_ref.fold_reference`` gives v in fp64 and
   E_v = (r + 4) u (|w| + |s| sum_r |B||A|), the error of the device's fp32 v in any summation order (its R + 2 J + 2 with J = 1).  So the device
   squares some v' with |v'| in [max(|v| - E_v, 0), |v| + E_v].
   The sum of squares is accumulated in fp32 (chosen: fp32 fused multiply-adds, 8 columns per thread tile after tile, then 8 partial sums per
   row in column order).  All terms are >= 0, and a term passes through at most I roundings in ANY summation tree over I leaves (I - 1 additions,
   one more if the square is rounded by itself), so the computed sum lies in  [ (1 - gamma(I)) sum v'^2, (1 + gamma(I)) sum v'^2 ].
   One rounding for the square root and one for the division, both correctly rounded on the device (``__fsqrt_rn``, ``__fdiv_rn``): a factor
   within (1 -+ u) each.  Together, for the norm n:
       n_lo = sqrt( (1 - gamma(I)) sum max(|v| - E_v, 0)^2 ) (1 - u),     n_hi = sqrt( (1 + gamma(I)) sum (|v| + E_v)^2 ) (1 + u)
   and the device gain lies between m / n_hi and m / n_lo, widened by one relative u (outwards).  No first-order shortcut is taken: the
   interval is evaluated as written, in fp64.  A row with sum v^2 == 0 has gain exactly 0 (documented deviation from peft, which divides by 0).
   m is taken as given (the tests pass fp32 values, which is what the kernel receives).

2. The fold with row gains.   t[o, i] = c[o] w[o, i] + sum_j g_j[o] s_j P_j[o, i],   P_j = B_j A_j,   c = 1 + sum_{j with gain} (g_j - 1),
   g_j = 1 for an adapter without gains.  The gains are INPUTS here (fp32 values, widened exactly).  The device commits
     * r_j - 1 additions for P_j, each a relative u on a partial sum no larger than sum_r |B_j||A_j|                 (as lora_fold_ref)
     * for an adapter with gains one multiplication g_j s_j                                                            (1 per such adapter)
     * one fused multiply-add of (g_j s_j) P_j into the running total per adapter                                      (J)
     * c: per adapter with gains one subtraction g_j - 1 and one addition, on values bounded by 1 + sum |g_j - 1|       (2 per such adapter)
     * one fused multiply-add c w + total                                                                              (1)
   every one of them on a quantity bounded by  mag = (1 + sum_j |g_j - 1|) |w| + sum_j |g_j s_j| sum_r |B_j||A_j|.  With JD adapters with gains that is
   R + J + 3 JD + 1 roundings to first order; J + 1 more cover the second-order terms as in lora_fold_ref:

       E = (R + 2 J + 3 JD + 2) u mag.           Without gains (JD = 0, every g = 1) this IS lora_fold_ref's t and E.

   The criterion is lora_fold_ref's: a device value d passes iff rne_bf16(t - E) <= d <= rne_bf16(t + E).

3. Chained (device gains into the device fold).  t is linear in each g_j with slope v_j = w + s_j P_j, so gains anywhere within
   [g_j - rad_j, g_j + rad_j] (rad_j = the larger distance from the fp64 gain to the interval of 1.) move t by at most sum_j rad_j |v_j|; the fold's
   own error is bounded with |g_j| + rad_j and |g_j - 1| + rad_j in mag:

       E_chain = (R + 2 J + 3 JD + 2) u mag(|g| + rad) + sum_j rad_j |w + s_j P_j|."""
import torch

import lora_fold_ref as LR

U32 = LR.U32


def gamma(n: int) -> float:
    return n * U32 / (1.0 - n * U32)


def gain_reference(base, A, B, s, m):
    """base [O, I], A [r, I], B [O, r] bf16 (CPU), s a python float, m [O] (fp32 or fp64) -> (g, g_lo, g_hi) fp64 [O]."""
    v, Ev = LR.fold_reference(base, [A], [B], [s])
    I = base.shape[1]
    m = m.double().cpu()
    n2 = (v * v).sum(1)
    lo2 = ((v.abs() - Ev).clamp(min=0) ** 2).sum(1) * (1.0 - gamma(I))
    hi2 = ((v.abs() + Ev) ** 2).sum(1) * (1.0 + gamma(I))
    n_lo, n_hi = lo2.sqrt() * (1.0 - U32), hi2.sqrt() * (1.0 + U32)
    zero = n2 == 0
    safe = lambda n: torch.where(n == 0, torch.full_like(n, 1e-300), n)            # noqa: E731  (m / 1e-300: beyond any fp32 gain)
    g = torch.where(zero, torch.zeros_like(m), m / safe(n2.sqrt()))
    a, b = m / safe(n_hi), m / safe(n_lo)
    lo, hi = torch.minimum(a, b), torch.maximum(a, b)
    lo, hi = lo - lo.abs() * U32, hi + hi.abs() * U32
    z = torch.zeros_like(m)
    return g, torch.where(zero, z, lo), torch.where(zero, z, hi)


def failing_gain(dev, lo, hi) -> torch.Tensor:
    d = dev.double().cpu()
    return (d < lo) | (d > hi) | ~torch.isfinite(d)


def check_gain(dev, lo, hi, what='') -> None:
    bad = failing_gain(dev, lo, hi)
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} row gains outside their interval; first: row {i} device {dev[i].item()!r} '
                             f'interval [{lo[i].item()!r}, {hi[i].item()!r}]')


def fold_rows_reference(base, A=(), B=(), scales=(), gains=None, radius=None):
    """As ``lora_fold_ref.fold_reference`` with gains[j] = None or [O] values (taken as exact) and, for the chained bound, radius[j] = None or [O]
    -> (t fp64 [O, I], E fp64 [O, I])."""
    J = len(A)
    gains = [None] * J if gains is None else list(gains)
    radius = [None] * J if radius is None else list(radius)
    w = base.double().cpu()
    t = w.clone()                                   # (c = 1 so far: without gains the sums below are fold_reference's, bit for bit)
    mag = w.abs()
    drift = torch.zeros_like(w)
    c = torch.ones(w.shape[0], dtype=torch.float64)
    c_abs = torch.ones(w.shape[0], dtype=torch.float64)
    R = JD = 0
    for a, b, s, g, rad in zip(A, B, scales, gains, radius):
        s = LR.f32(s)
        ad, bd = a.double().cpu(), b.double().cpu()
        P, Pabs = bd @ ad, bd.abs() @ ad.abs()
        R += a.shape[0]
        if g is None:
            t += s * P
            mag += abs(s) * Pabs
            continue
        JD += 1
        g = g.double().cpu()
        rad = torch.zeros_like(g) if rad is None else rad.double().cpu()
        t += (g * s)[:, None] * P
        mag += ((g.abs() + rad) * abs(s))[:, None] * Pabs
        c += g - 1.0
        c_abs += (g - 1.0).abs() + rad
        drift += rad[:, None] * (w + s * P).abs()
    t += (c - 1.0)[:, None] * w
    mag += (c_abs - 1.0)[:, None] * w.abs()
    return t, (R + 2 * J + 3 * JD + 2) * U32 * mag + drift
