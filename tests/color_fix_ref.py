"""numpy fp64 reference of afx_color_fix (include/arcflow_hip.h), shared by tests/test_color_fix_ref_cpu.py and
tests/test_hip_color_fix_fp64.py.  Both rules are applied to the fp32 inputs exactly as the header states them, in fp64, and come with a
per-element bound E on what the fp32 kernel may differ by.  On the parent commit the entry, ``ops.color_fix`` and the pipelines'
``color_fix=`` do not exist: every test that uses this file fails there.

The bounds come from the roundings the header counts, with u = 2^-24 (fp32, round to nearest) and v = 2^-53 (fp64).  No constant is fitted.

wavelet.  s' = fma(2, s, -1) rounds once (only with src01): |err| <= u |s'|.  d = s' - e rounds once: <= u |d|.  With M0 = max |d| over
    the case, P = u (max |s'| [src01] + M0) bounds the error of every d.  A pass forms t = lo + hi (<= u |t| <= 2 u M, scaled by 0.25:
    0.5 u M) and q = fma(0.5, mid, 0.25 t) (<= u |q| <= u M): 1.5 u M of new error, while the errors of its inputs pass through a convex
    combination (weights 1/4, 1/2, 1/4: gain <= 1).  Every value of the chain is a convex combination of values of d with at most twenty
    roundings on the way, so M = (M0 + P) (1 + u)^20 bounds them all.  Ten passes: the error of L is <= P + 15 u M.  out = e + L rounds
    once, on a value within that error of r:   E = (P + 15 u M) (1 + u) + u |r| + 32 * 2^-149  (the last term: one unit of underflow per
    operation).  At these inputs M0 < 3.2, so E is about 17 u 3.2 + u |r| = 3.4e-6, far below the 2^-16 that a wrong tap moves.

adain.  Per plane of n elements, x widened exactly to fp64 (the source after its s' rounding, which the reference models as an
    error of u |s'| per element: it moves mu_s by <= u mean|s'| =: Ms and sumsq / n by <= 2 u mean(s'^2) (1 + u) =: Qs).
    A sum of n fp64 terms in any order errs by <= n v sum|x|:  dS = n v sum|x|,  dQ = n v sum x^2.
      dmu  = dS / n + v |mu| (+ Ms)
      dvar = dQ / n (+ Qs) + 2 |mu| dmu + dmu^2 + 4 v (sumsq / n + mu^2)          (quotient, product, difference)
      dsd  = dvar / (2 sd_lo) + 2 v sd,   sd_lo = sqrt(max(var - dvar, 0) + 1e-5)  (the add, the square root)
      drat = rat (dsd_s / sd_s + dsd_e / sd_e,lo + v) G        with G = 1 + 2^-10 for the products of these small terms
      da   = drat + u (|rat| + drat)                                               (a rounds once to fp32)
      db64 = dmu_s + |rat| dmu_e + |mu_e| drat + drat dmu_e + 2 v (|mu_s| + |rat mu_e|)
      db   = db64 + u (|b| + db64)                                                 (b rounds once to fp32)
    out = fma(a, e, b) rounds once on a value within da |e| + db of r:   E = (da |e| + db) (1 + u) + u |r| + 2^-149.
    stats: (dmu_e, dvar_e, dmu_s, dvar_s) as above bound the four fp64 numbers."""
import numpy as np

U = 2.0 ** -24
V = 2.0 ** -53
DILATIONS = (1, 2, 4, 8, 16)
EPS = 1e-5

# name, batch, source batch, C, H, W, bf16 edit
CASES = [
    ('clamp_both_sides', 1, 1, 1, 16, 24, False),          # every level clamps on both sides
    ('one_row', 1, 1, 3, 1, 70, False),
    ('one_column', 1, 1, 3, 70, 1, False),
    ('tiles_and_broadcast', 2, 1, 3, 80, 144, False),     # several 64 x 64 tiles on both axes, interior pixels with the whole 63-pixel footprint
    ('odd_bf16', 2, 2, 3, 67, 129, True),                 # sizes that are no multiple of anything
    ('thin_66000_rows', 1, 1, 1, 66000, 16, False),       # more rows than a grid axis holds (65535)
]


def bf16_round(x: np.ndarray) -> np.ndarray:
    """fp32 values rounded to bf16 (ties to even), as fp32."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7fff + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).reshape(x.shape)


def make_case(case, seed=0):
    """-> (e fp32 [B, C, H, W] in [-1.2, 1.2) -- bf16-representable values when the case says so --, s fp32 [Bs, C, H, W] in [0, 1), bf16)"""
    name, B, Bs, C, H, W, bf16 = case
    rng = np.random.default_rng(1000 * seed + sum(map(ord, name)))
    e = rng.uniform(-1.2, 1.2, (B, C, H, W)).astype(np.float32)
    s = rng.uniform(0.0, 1.0, (Bs, C, H, W)).astype(np.float32)
    s = np.minimum(s, np.float32(1.0) - np.float32(2.0 ** -24))
    return (bf16_round(e) if bf16 else e), s, bf16


def _source(s, src01):
    s = s.astype(np.float64)
    return 2.0 * s - 1.0 if src01 else s


def _shift(p, r, axis, zero_pad):
    """(p at index - r, p at index + r) along ``axis``: indices clamped into the image, or zeros outside it."""
    n = p.shape[axis]
    i = np.arange(n)
    lo, hi = np.take(p, np.clip(i - r, 0, n - 1), axis), np.take(p, np.clip(i + r, 0, n - 1), axis)
    if zero_pad:
        shape = [1] * p.ndim
        shape[axis] = n
        lo = lo * (i - r >= 0).reshape(shape)
        hi = hi * (i + r <= n - 1).reshape(shape)
    return lo, hi


def low_band(p, dilations=DILATIONS, zero_pad=False):
    """The separable [1, 2, 1] / 4 blur at each dilation in turn, horizontal then vertical, replicate borders; fp64."""
    for r in dilations:
        lo, hi = _shift(p, r, 3, zero_pad)
        p = 0.5 * p + 0.25 * (lo + hi)
        lo, hi = _shift(p, r, 2, zero_pad)
        p = 0.5 * p + 0.25 * (lo + hi)
    return p


def wavelet_ref(e, s, src01=True, mutate=None):
    """-> (r, E) fp64 [B, C, H, W]"""
    e64 = e.astype(np.float64)
    s1 = np.broadcast_to(_source(s, src01 and mutate != 'src01_ignored'), e64.shape)
    d = e64 - s1 if mutate == 'e_minus_s' else s1 - e64
    if mutate == 'dilations_12345':
        L = low_band(d, (1, 2, 3, 4, 5))
    elif mutate == 'zero_pad':
        L = low_band(d, zero_pad=True)
    elif mutate == 'four_levels':
        L = low_band(d, DILATIONS[:4])
    elif mutate == 'low_of_e_kept':
        L = low_band(s1)
    else:
        assert mutate in (None, 'e_minus_s', 'src01_ignored'), mutate
        L = low_band(d)
    r = e64 + L
    M0 = np.abs(d).max()
    P = U * ((np.abs(s1).max() if src01 else 0.0) + M0)
    M = (M0 + P) * (1 + U) ** 20
    E = (P + 15 * U * M) * (1 + U) + U * np.abs(r) + 32 * 2.0 ** -149
    return r, E


def wavelet_two_decompositions(e, s, src01=True):
    """StableSR's form: high(e) + low(s') from two decompositions, fp64."""
    e64 = e.astype(np.float64)
    return (e64 - low_band(e64)) + low_band(np.broadcast_to(_source(s, src01), e64.shape))


def _moments(x, extra_mu=0.0, extra_q=0.0, unbiased=False):
    """-> (mu, var, dmu, dvar) per plane [B, C] of x fp64 [B, C, H, W]"""
    n = x.shape[2] * x.shape[3]
    S, Q, A = x.sum((2, 3)), (x * x).sum((2, 3)), np.abs(x).sum((2, 3))
    mu = S / n
    var = Q / n - mu * mu
    if unbiased:
        var = var * n / max(n - 1, 1)
    dmu = V * A + V * np.abs(mu) + extra_mu
    dvar = V * Q + extra_q + 2 * np.abs(mu) * dmu + dmu * dmu + 4 * V * (Q / n + mu * mu)
    return mu, var, dmu, dvar


def adain_ref(e, s, src01=True, mutate=None):
    """-> (r, E, stats, stats_E, a): r, E fp64 [B, C, H, W]; stats, stats_E [B, C, 4] = (mu_e, var_e, mu_s, var_s) and their bounds; a [B, C]"""
    assert mutate in (None, 'unbiased', 'no_eps', 'wrong_channel', 'src01_ignored'), mutate
    e64 = e.astype(np.float64)
    B = e64.shape[0]
    s1 = _source(s, src01 and mutate != 'src01_ignored')
    unb = mutate == 'unbiased'
    eps = 0.0 if mutate == 'no_eps' else EPS
    mu_e, var_e, dmu_e, dvar_e = _moments(e64, unbiased=unb)
    ms = U * np.abs(s1).mean((2, 3)) if src01 else 0.0
    qs = 2 * U * (s1 * s1).mean((2, 3)) * (1 + U) if src01 else 0.0
    mu_s, var_s, dmu_s, dvar_s = (np.broadcast_to(t, (B,) + t.shape[1:]) for t in _moments(s1, ms, qs, unbiased=unb))
    with np.errstate(all='ignore'):
        sd_e, sd_s = np.sqrt(var_e + eps), np.sqrt(var_s + eps)
        lo_e, lo_s = np.sqrt(np.maximum(var_e - dvar_e, 0) + eps), np.sqrt(np.maximum(var_s - dvar_s, 0) + eps)
        dsd_e, dsd_s = dvar_e / (2 * lo_e) + 2 * V * sd_e, dvar_s / (2 * lo_s) + 2 * V * sd_s
        rat = sd_s / sd_e
        b = mu_s - rat * mu_e
        drat = rat * (dsd_s / sd_s + dsd_e / lo_e + V) * (1 + 2.0 ** -10)
        da = drat + U * (np.abs(rat) + drat)
        db64 = dmu_s + np.abs(rat) * dmu_e + np.abs(mu_e) * drat + drat * dmu_e + 2 * V * (np.abs(mu_s) + np.abs(rat * mu_e))
        db = db64 + U * (np.abs(b) + db64)
        if mutate == 'wrong_channel':
            rat, b = np.roll(rat, 1, 1), np.roll(b, 1, 1)
        r = rat[:, :, None, None] * e64 + b[:, :, None, None]
        E = (da[:, :, None, None] * np.abs(e64) + db[:, :, None, None]) * (1 + U) + U * np.abs(r) + 2.0 ** -149
    stats = np.stack([mu_e, var_e, mu_s, var_s], -1)
    stats_E = np.stack([dmu_e, dvar_e, dmu_s, dvar_s], -1)
    return r, E, stats, stats_E, rat
