"""The SSIM that ``afx_image_ssim`` computes (Wang et al. 2004, the common "Gaussian, valid" form) in torch fp64 on the CPU, seven mutated
references, an a-priori error bound and the inputs of the tests that use them (tests/test_ssim_ref_cpu.py, tests/test_hip_image_ssim_fp64.py,
tests/test_evaluate_ssim_gpu.py).

Definition.  a, b [B, C, H, W]; with ``transform`` both are first mapped to clamp(v / 2 + 0.5, 0, 1) in fp32; then everything is fp64.
g[i] = exp(-(i - 5)^2 / (2 1.5^2)), i = 0..10, normalised to sum 1; the 2-D window is g g^T, applied as two 1-D ``conv2d`` passes without
padding, so only the (H - 10)(W - 10) windows inside the image exist.  Per window, with E[.] the weighted mean:
    mu_a = E[a], mu_b = E[b], s_aa = E[a^2] - mu_a^2, s_bb = E[b^2] - mu_b^2, s_ab = E[a b] - mu_a mu_b            (biased)
    ssim = (2 mu_a mu_b + c1)(2 s_ab + c2) / ((mu_a^2 + mu_b^2 + c1)(s_aa + s_bb + c2)),   c1 = (0.01 L)^2, c2 = (0.03 L)^2, L = data_range.
The per-sample result is the mean over channels and windows.

The bound (``Reference.bound``) is derived in the docstring of tests/test_hip_image_ssim_fp64.py; it is a function of the inputs alone.
"""
import functools
from typing import Dict, NamedTuple

import torch
import torch.nn.functional as F

U = 2.0 ** -53
TAPS = 11
MUTANTS = ('sigma_1p4', 'taps_9', 'k2_0p02', 'same_padding', 'unbiased', 'no_transform', 'unnormalised')
PARTNERS = ('noisy', 'zero', 'saturated')
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16}


def unit_range(v: torch.Tensor) -> torch.Tensor:
    """The image range in fp32, exactly as the kernels form it (v / 2 is exact, the addition rounds once)."""
    return (v.float() / 2 + 0.5).clamp(0, 1)


def window(taps: int = TAPS, sigma: float = 1.5, normalise: bool = True) -> torch.Tensor:
    i = torch.arange(taps, dtype=torch.float64)
    g = torch.exp(-(i - (taps - 1) / 2) ** 2 / (2 * sigma ** 2))
    return g / g.sum() if normalise else g


def _smooth(x: torch.Tensor, g: torch.Tensor, same: bool) -> torch.Tensor:
    """x [B, C, H, W] fp64 -> the separable window g g^T applied per plane: a horizontal, then a vertical 1-D conv2d."""
    C, k = x.shape[1], g.numel()
    p = (k - 1) // 2 if same else 0
    x = F.conv2d(x, g.view(1, 1, 1, k).repeat(C, 1, 1, 1), padding=(0, p), groups=C)
    return F.conv2d(x, g.view(1, 1, k, 1).repeat(C, 1, 1, 1), padding=(p, 0), groups=C)


def moments(a, b, transform, *, sigma=1.5, taps=TAPS, same=False, normalise=True):
    """-> (mu_a, mu_b, E[a^2], E[a b], E[b^2]) per window, fp64 [B, C, h, w]"""
    x = (unit_range(a) if transform else a).double()
    y = (unit_range(b) if transform else b).double()
    g = window(taps, sigma, normalise)
    return tuple(_smooth(t, g, same) for t in (x, y, x * x, x * y, y * y))


def ssim_map(a, b, transform=False, data_range=1.0, *, k2=0.03, unbiased=False, **kw) -> torch.Tensor:
    """SSIM per window, fp64 [B, C, h, w] (h = H - 10, w = W - 10 for the definition; the keywords select a mutation)."""
    mu_a, mu_b, e_aa, e_ab, e_bb = moments(a, b, transform, **kw)
    c1, c2 = (0.01 * data_range) ** 2, (k2 * data_range) ** 2
    s_aa, s_ab, s_bb = e_aa - mu_a * mu_a, e_ab - mu_a * mu_b, e_bb - mu_b * mu_b
    if unbiased:
        n = float(kw.get('taps', TAPS)) ** 2
        s_aa, s_ab, s_bb = s_aa * (n / (n - 1)), s_ab * (n / (n - 1)), s_bb * (n / (n - 1))
    return (2 * mu_a * mu_b + c1) * (2 * s_ab + c2) / ((mu_a * mu_a + mu_b * mu_b + c1) * (s_aa + s_bb + c2))


def ssim_mean(a, b, transform=False, data_range=1.0, **kw) -> torch.Tensor:
    """Mean SSIM per sample, fp64 [B]."""
    return ssim_map(a, b, transform, data_range, **kw).flatten(1).mean(1)


def ssim_bound(a, b, transform=False, data_range=1.0) -> torch.Tensor:
    """|kernel mean - reference mean| <= this, per sample, fp64 [B]:
        mean over the windows of 2 u (346 S / B1 + 521 S / B2 + 21)  +  2 N u,
    S = E[a^2] + E[b^2], B1 = mu_a^2 + mu_b^2 + c1, B2 = s_aa + s_bb + c2 of the window, N = C (H - 10)(W - 10), u = 2^-53."""
    mu_a, mu_b, e_aa, e_ab, e_bb = moments(a, b, transform)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    S = e_aa + e_bb
    B1 = mu_a * mu_a + mu_b * mu_b + c1
    B2 = (e_aa - mu_a * mu_a) + (e_bb - mu_b * mu_b) + c2
    per_window = 2 * U * (346 * S / B1 + 521 * S / B2 + 21)
    return per_window.flatten(1).mean(1) + 2 * per_window[0].numel() * U


def mutants(a, b, transform=False, data_range=1.0) -> Dict[str, torch.Tensor]:
    """name -> mean SSIM per sample of a reference that is wrong in one way.  'no_transform' exists only where a transform is asked for."""
    m = dict(sigma_1p4=ssim_mean(a, b, transform, data_range, sigma=1.4),
             taps_9=ssim_mean(a, b, transform, data_range, taps=9),
             k2_0p02=ssim_mean(a, b, transform, data_range, k2=0.02),
             same_padding=ssim_mean(a, b, transform, data_range, same=True),
             unbiased=ssim_mean(a, b, transform, data_range, unbiased=True),
             unnormalised=ssim_mean(a, b, transform, data_range, normalise=False))
    if transform:
        m['no_transform'] = ssim_mean(a, b, False, data_range)
    return m


def make_inputs(B: int, C: int, H: int, W: int, dname: str, partner: str, transform: bool):
    """a: smooth noise, a 5 x 5 box blur of randn (standard deviation 0.2) times a scale.  With the transform the scale is 2.8: standard
    deviation 0.56, 6 % or more of the values lie past +-1, where the transform clamps.  Without it nothing clamps and the scale is 0.6
    (values within about +-0.5 for data_range 2.0): at 2.8 the local variances are so far above c2 that sigma 1.4, the 9-tap window and
    the unbiased moments move the mean by less than 1e-5 -- measured on the CPU, tests/test_ssim_ref_cpu.py holds the choice to that.
    b: a + 0.15 data ranges of white noise | zeros | 4 a (mostly saturated under the transform).  The noise is 0.3 randn on the raw values
    in both modes: the transform halves it to 0.15 of its range [0, 1], and transform 0 is scored with data_range 2.0.  (At 0.15 randn on
    the raw values the unbiased-moments mutant moves the transformed mean by 4e-6 to 8e-6 only.)  Both in the operand dtype, on the CPU."""
    g = torch.Generator().manual_seed(1000 * H + 10 * W + B + C + 100000 * PARTNERS.index(partner))
    a = F.avg_pool2d(torch.randn(B, C, H + 4, W + 4, generator=g), 5, stride=1) * (2.8 if transform else 0.6)
    if partner == 'noisy':
        b = a + 0.3 * torch.randn(B, C, H, W, generator=g)
    elif partner == 'zero':
        b = torch.zeros_like(a)
    else:
        b = 4 * a
    return a.to(DTYPES[dname]).contiguous(), b.to(DTYPES[dname]).contiguous()


class Reference(NamedTuple):
    a: torch.Tensor            # operands, CPU, the operand dtype
    b: torch.Tensor
    transform: bool
    data_range: float
    mean: torch.Tensor         # fp64 [B]
    bound: torch.Tensor        # fp64 [B]
    mutants: Dict[str, torch.Tensor]


@functools.lru_cache(maxsize=None)
def case(shape, dname: str, transform: bool, partner: str) -> Reference:
    """One case of the kernel test, computed once and shared: transform 0 is scored with data_range 2.0, transform 1 with 1.0."""
    a, b = make_inputs(*shape, dname, partner, bool(transform))
    L = 1.0 if transform else 2.0
    if transform:
        assert ((unit_range(a) == 0) | (unit_range(a) == 1)).double().mean().item() > 0.05          # the clamp is exercised
    return Reference(a, b, bool(transform), L, ssim_mean(a, b, transform, L), ssim_bound(a, b, transform, L), mutants(a, b, transform, L))
