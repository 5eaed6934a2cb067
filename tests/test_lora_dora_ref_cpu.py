"""The fp64 references of the DoRA kernels (tests/lora_dora_ref.py) on their own: what they must reduce to.  Self-checks of the test-side
reference, with no product code in them."""
import torch

import lora_dora_ref as DR
import lora_fold_ref as LR


def _operands(O, I, ranks, seed=0):
    g = torch.Generator().manual_seed(seed)
    base = (torch.randn(O, I, generator=g) * 0.02).bfloat16()
    A = [(torch.randn(r, I, generator=g) * 0.1).bfloat16() for r in ranks]
    B = [(torch.randn(O, r, generator=g) * 0.1).bfloat16() for r in ranks]
    mags = [(torch.rand(O, generator=g) + 0.1).float() for _ in ranks]
    return base, A, B, mags


def test_no_gains_is_the_plain_fold_reference():
    base, A, B, _ = _operands(64, 128, (4, 16))
    for gains in (None, [None, None]):
        t, E = DR.fold_rows_reference(base, A, B, (1.0, -0.3), gains)
        t0, E0 = LR.fold_reference(base, A, B, (1.0, -0.3))
        assert torch.equal(t, t0) and torch.equal(E, E0)
    t, E = DR.fold_rows_reference(base)
    assert torch.equal(t, base.double()) and torch.equal(E, LR.fold_reference(base)[1])


def test_zero_b_with_the_rows_own_norm_returns_the_base():
    base, A, B, _ = _operands(64, 128, (8,))
    B0 = torch.zeros_like(B[0])
    m = base.double().norm(dim=1)                                       # fp64: the gain is 1 to fp64 roundoff (two ways of summing the squares)
    g, lo, hi = DR.gain_reference(base, A[0], B0, 0.7, m)
    eps = 2.0 ** -52
    assert bool(((g - 1).abs() <= 8 * eps).all()) and bool((lo < 1).all()) and bool((hi > 1).all())
    # width: gamma(I = 128) halved by the root on either side, E_v = (r + 4) u |w| with r = 8 on either side, root and division
    assert bool(((hi - lo) < (128 + 2 * 12 + 8) * 2.0 ** -24).all()) and bool(((hi - lo) > 128 * 2.0 ** -24).all())
    t, _ = DR.fold_rows_reference(base, A, [B0], (0.7,), [g])
    assert bool(((t - base.double()).abs() <= 8 * eps * base.double().abs()).all())
    t1, _ = DR.fold_rows_reference(base, A, [B0], (0.7,), [torch.ones(64, dtype=torch.float64)])
    assert torch.equal(t1, base.double())                               # and with the gain exactly 1, exactly the base
    # a row of zeros: gain 0 with an empty interval around it, and the folded row is 0
    base[5] = 0
    g, lo, hi = DR.gain_reference(base, A[0], B0, 0.7, torch.ones(64))
    assert g[5] == 0 and lo[5] == 0 and hi[5] == 0 and bool((g[:5] > 0).all())
    assert not DR.failing_gain(g.float(), lo, hi).any()
    bad = g.float().clone()
    bad[3] *= 1 + 2.0 ** -12
    assert DR.failing_gain(bad, lo, hi).nonzero().flatten().tolist() == [3]


def test_one_dora_adapter_is_the_rescaled_sum():
    base, A, B, mags = _operands(128, 64, (16,), seed=1)
    s = -0.3
    g, lo, hi = DR.gain_reference(base, A[0], B[0], s, mags[0])
    assert bool((lo <= g).all()) and bool((g <= hi).all())
    t, E = DR.fold_rows_reference(base, A, B, (s,), [g])
    v = base.double() + LR.f32(s) * (B[0].double() @ A[0].double())
    want = mags[0].double()[:, None] * v / v.norm(dim=1, keepdim=True)
    assert torch.allclose(t, want, rtol=1e-12, atol=1e-15)
    assert torch.allclose(t.norm(dim=1), mags[0].double(), rtol=1e-12)       # what DoRA is for: the rows have the magnitudes' lengths
    assert bool((E > 0).all())


def test_several_adapters_add_their_deltas():
    base, A, B, mags = _operands(64, 192, (16, 4, 130), seed=2)
    scales = (1.0, -0.3, 0.5)
    w = base.double()
    P = [LR.f32(s) * (b.double() @ a.double()) for a, b, s in zip(A, B, scales)]
    g0 = DR.gain_reference(base, A[0], B[0], scales[0], mags[0])[0]
    g2 = DR.gain_reference(base, A[2], B[2], scales[2], mags[2])[0]
    t, E = DR.fold_rows_reference(base, A, B, scales, [g0, None, g2])
    delta = lambda g, p: (g - 1)[:, None] * w + g[:, None] * p       # noqa: E731
    want = w + delta(g0, P[0]) + P[1] + delta(g2, P[2])
    assert torch.allclose(t, want, rtol=1e-12, atol=1e-15)
    # the chained bound contains the plain one and grows with the radius
    rad = [torch.full_like(g0, 1e-6), None, torch.full_like(g2, 1e-6)]
    t2, E2 = DR.fold_rows_reference(base, A, B, scales, [g0, None, g2], rad)
    assert torch.equal(t2, t) and bool((E2 > E).all())
    # a gain on the other adapter is another matrix
    t3, _ = DR.fold_rows_reference(base, A, B, scales, [None, g0, g2])
    assert not torch.allclose(t3, t, rtol=1e-3)
