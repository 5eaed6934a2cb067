"""The two masked scores of training-time evaluation -- ``afx_sample_score_masked`` and ``afx_image_ssim_masked`` -- restated in torch fp64 on
the CPU, with the mutated references their kernel tests must reject (tests/test_masked_score_ref_cpu.py,
tests/test_hip_sample_score_masked_fp64.py, tests/test_hip_image_ssim_masked_fp64.py).

Masked sums.  a, b [B, n] viewed as [B, G, P, R]; mask [Bm, P, Q], Bm in {1, B}, Q | R; element (s, g, p, r) takes w = m[s, p, r % Q].
    out[s, 0] = (sum w, sum w d^2, sum w a^2, sum w b^2, sum w a b)  with d = a - b,        out[s, 1] the same with w -> 1 - w,
after the optional image-range transform of both operands in fp32 (``ssim_ref.unit_range``).  Packed latents [B, N, 64] with the
[B, N, 4] operand of ``afx_edit_blend``: G = 1, P = N, R = 64, Q = 4 -- channel e = c 4 + ph 2 + pw of a token reads m[token, ph 2 + pw]
(afx_edit.hip: ``mask[b, tok, e & 3]``).  Images [B, C, H, W] with a [Bm, 1, H, W] mask: G = C, P = H W, R = Q = 1.

Masked SSIM.  ``ssim_ref.ssim_map`` per window; the weight of a window is the mask [Bm, 1, H, W] through the same two 11-tap passes (the
Gaussian-weighted mean over the window's own support), clamped to [0, 1].  out[s] = (sum w ssim, sum w, sum (1 - w) ssim, sum (1 - w))
over channels and windows.
"""
import torch

import ssim_ref as SR

U = 2.0 ** -53


def weights(mask: torch.Tensor, B: int, G: int, P: int, R: int, *, swap_hw: bool = False, ignore_batch: bool = False) -> torch.Tensor:
    """mask [Bm, P, Q] -> the weight of every element, fp64 [B, G P R].  Mutations: ``swap_hw`` reads m[p, pw 2 + ph] for Q = 4 (the 2 x 2
    patch transposed); ``ignore_batch`` reads sample 0's mask for every sample."""
    Bm, Pm, Q = mask.shape
    assert Pm == P and R % Q == 0 and Bm in (1, B)
    m = mask.double()
    if ignore_batch:
        m = m[:1]
    q = torch.arange(R) % Q
    if swap_hw:
        assert Q == 4
        q = (q & 1) * 2 + (q >> 1)
    w = m[:, :, q]                                          # [Bm, P, R]
    return w[:, None].expand(B, G, P, R).reshape(B, G * P * R)


def masked_sums(a, b, mask, view, transform=False, *, swap_regions=False, **mut):
    """a, b [B, ...] (fp32 or bf16, CPU), mask [Bm, P, Q] fp32, view = (G, P, R) -> (sums [B, 2, 5], sum|term| [B, 2, 5]), fp64."""
    B = a.shape[0]
    G, P, R = view
    x = (SR.unit_range(a) if transform else a).double().reshape(B, -1)
    y = (SR.unit_range(b) if transform else b).double().reshape(B, -1)
    assert x.shape[1] == G * P * R
    w = weights(mask, B, G, P, R, **mut)
    d = x - y
    sums, mags = [], []
    for ww in ((1.0 - w, w) if swap_regions else (w, 1.0 - w)):
        terms = [ww, ww * d * d, ww * x * x, ww * y * y, ww * x * y]
        sums.append(torch.stack([t.sum(1) for t in terms], 1))
        mags.append(torch.stack([t.abs().sum(1) for t in terms], 1))
    return torch.stack(sums, 1), torch.stack(mags, 1)


def view_of(a, mask):
    """(G, P, R) and the mask as [Bm, P, Q] for packed tokens + [Bm, N, 4], or images + [Bm, 1, H, W]."""
    if a.dim() == 3:
        return (1, a.shape[1], a.shape[2]), mask
    return (a.shape[1], a.shape[2] * a.shape[3], 1), mask.reshape(mask.shape[0], -1, 1)


def window_weights(mask, *, centre=False, transpose=False):
    """mask [Bm, 1, H, W] -> the weight of every window, fp64 [Bm, 1, H - 10, W - 10].  Mutations: ``centre`` takes the mask value at the
    window's centre instead of the Gaussian mean; ``transpose`` reads the mask's memory as [W, H] and transposes it (m[x H + y] for
    m[y W + x]: the transposed mask where it is square)."""
    m = mask.double()
    if transpose:
        m = m.reshape(m.shape[0], 1, m.shape[3], m.shape[2]).transpose(2, 3)
    if centre:
        return m[:, :, 5:-5, 5:-5].clamp(0, 1)
    return SR._smooth(m, SR.window(), False).clamp(0, 1)


def masked_ssim_sums(a, b, mask, transform=False, data_range=1.0, **mut):
    """-> [B, 4] fp64: (sum w ssim, sum w, sum (1 - w) ssim, sum (1 - w)) over channels and windows."""
    s = SR.ssim_map(a, b, transform, data_range)                      # [B, C, h, w]
    w = window_weights(mask, **mut).expand(s.shape[0], s.shape[1], -1, -1)
    k = 1.0 - w
    return torch.stack([(w * s).flatten(1).sum(1), w.flatten(1).sum(1), (k * s).flatten(1).sum(1), k.flatten(1).sum(1)], 1)


def masked_ssim_means(a, b, mask, transform=False, data_range=1.0, **mut):
    """-> (repaint mean, keep mean), fp64 [B] each."""
    s = masked_ssim_sums(a, b, mask, transform, data_range, **mut)
    return s[:, 0] / s[:, 1], s[:, 2] / s[:, 3]


def masked_ssim_bound(a, b, mask, transform=False, data_range=1.0):
    """|kernel mean - reference mean| <= this, per sample and region, fp64 [B, 2]: the bound of tests/test_hip_image_ssim_fp64.py with the
    window weights carried through (derived in tests/test_hip_image_ssim_masked_fp64.py):
        sum_i w_i e_i / sum_i w_i  +  2 N u  +  700 u,      e_i = 2 u (346 S / B1 + 521 S / B2 + 21) of window i, N = C (H - 10)(W - 10)."""
    mu_a, mu_b, e_aa, e_ab, e_bb = SR.moments(a, b, transform)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    S = e_aa + e_bb
    B1 = mu_a * mu_a + mu_b * mu_b + c1
    B2 = (e_aa - mu_a * mu_a) + (e_bb - mu_b * mu_b) + c2
    e = 2 * U * (346 * S / B1 + 521 * S / B2 + 21)
    w = window_weights(mask).expand_as(e)
    n_win = e[0].numel()
    out = [(ww * e).flatten(1).sum(1) / ww.flatten(1).sum(1) + 2 * n_win * U + 700 * U for ww in (w, 1.0 - w)]
    return torch.stack(out, 1)


def random_mask(shape, seed):
    """Fractional, non-symmetric weights in [0, 1]: uniform noise times a ramp that differs along every axis, with exact 0 and 1 entries."""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(shape, generator=g)
    ramp = torch.ones(shape)
    for ax, n in enumerate(shape):
        r = torch.linspace(0.3 + 0.1 * ax, 1.0, n).view([n if i == ax else 1 for i in range(len(shape))])
        ramp = ramp * r
    m = (m * ramp).float()
    flat = m.view(-1)
    flat[::7] = 0.0
    flat[3::11] = 1.0
    return m.contiguous()
