"""tests/lycoris_fold_ref.py against itself and against torch, on the CPU: the LoKr index rule is ``torch.kron`` (row slices by ``row0`` included),
the LoHa target is the product of two explicit matmuls, an all-LoRA term list gives lora_dora_ref's t and E, an fp32 emulation of the kernel's order
stays inside [rne(t - E), rne(t + E)] -- and the mutated references the GPU test relies on do leave it.  On the parent commit the reference module
does not exist."""
import pytest
import torch

import lora_dora_ref as DR
import lora_fold_ref as LR
import lycoris_fold_ref as YR


def _base(O, I, g):
    return (torch.randn(O, I, generator=g) * 0.02).bfloat16()


@pytest.mark.parametrize('a,b,c,d', [(3, 5, 64, 64), (2, 10, 96, 32), (192, 320, 1, 1), (1, 1, 192, 320), (6, 4, 32, 80), (4, 64, 48, 5)])
def test_lokr_index_rule_is_torch_kron(a, b, c, d):
    g = torch.Generator().manual_seed(a * c + b)
    w1, w2 = torch.randn(a, b, generator=g), torch.randn(c, d, generator=g)
    full = torch.kron(w1.double(), w2.double())
    D, Dabs, n = YR.lokr_delta(w1, w2, 0, a * c)
    assert torch.equal(D, full) and torch.equal(Dabs, full.abs()) and n == 1
    for row0, O in ((0, 64), (64, 64), (a * c - 64, 64), (37, a * c - 37)):
        assert torch.equal(YR.lokr_delta(w1, w2, row0, O)[0], full[row0:row0 + O]), (row0, O)
    if a * c > 64:
        assert not torch.equal(YR.lokr_delta(w1, w2, 64, 64, 'lokr_ignore_row0')[0], full[64:128])
    if a > 1 and c > 1:
        assert not torch.equal(YR.lokr_delta(w1, w2, 0, a * c, 'lokr_swap_index')[0], full)


def test_loha_target_is_the_product_of_two_matmuls():
    g = torch.Generator().manual_seed(1)
    O, I = 64, 128
    term = YR.loha_operands(O, I, 5, 33, g)
    D, Dabs, n = YR.loha_delta(term['w1_a'], term['w1_b'], term['w2_a'], term['w2_b'])
    P1 = sum(term['w1_a'].double()[:, k:k + 1] * term['w1_b'].double()[k:k + 1] for k in range(5))
    P2 = sum(term['w2_a'].double()[:, k:k + 1] * term['w2_b'].double()[k:k + 1] for k in range(33))
    assert torch.allclose(D, P1 * P2, rtol=1e-13, atol=0) and n == 38 and bool((Dabs >= D.abs()).all())
    assert 0.3 < D.std().item() / 0.02 < 3.0                                       # the delta is of the size of a weight
    base = _base(O, I, g)
    t, E = YR.terms_reference(base, [dict(term, scale=-0.3)])
    assert torch.allclose(t, base.double() + LR.f32(-0.3) * P1 * P2, rtol=1e-12, atol=1e-18)
    assert torch.equal(E, (38 + 2 + 2) * YR.U32 * (base.double().abs() + abs(LR.f32(-0.3)) * Dabs))


def test_lora_terms_alone_are_the_dora_reference():
    g = torch.Generator().manual_seed(2)
    O, I = 128, 64
    base = _base(O, I, g)
    A = [(torch.randn(r, I, generator=g) * 0.05).bfloat16() for r in (4, 16)]
    B = [(torch.randn(O, r, generator=g) * 0.05).bfloat16() for r in (4, 16)]
    gain = (torch.rand(O, generator=g) + 0.5).float()
    for gains in ([None, None], [gain, None]):
        terms = [dict(kind='lora', A=a, B=b, scale=s, row_gain=gn) for a, b, s, gn in zip(A, B, (0.75, -0.3), gains)]
        t, E = YR.terms_reference(base, terms)
        t0, E0 = DR.fold_rows_reference(base, A, B, (0.75, -0.3), gains)
        assert torch.equal(t, t0) and torch.equal(E, E0)
    t1, E1 = LR.fold_reference(base, A, B, (0.75, -0.3))
    t, E = YR.terms_reference(base, [dict(kind='lora', A=a, B=b, scale=s) for a, b, s in zip(A, B, (0.75, -0.3))])
    assert torch.equal(t, t1) and torch.equal(E, E1)


def _mixed(O, I, g, row0=64):
    gain = (torch.rand(O, generator=g) * 0.4 + 0.8).float()
    return [dict(kind='lora', A=(torch.randn(16, I, generator=g) * 0.05).bfloat16(), B=(torch.randn(O, 16, generator=g) * 0.05).bfloat16(), scale=1.0),
            dict(YR.loha_operands(O, I, 8, 33, g), scale=0.7),
            dict(YR.lokr_operands((O + row0 + 95) // 96, I // 32, 96, 32, g), scale=-0.3, row0=row0),
            dict(kind='lora', A=(torch.randn(4, I, generator=g) * 0.05).bfloat16(), B=(torch.randn(O, 4, generator=g) * 0.05).bfloat16(), scale=0.5,
                 row_gain=gain),
            dict(YR.loha_operands(O, I, 130, 1, g), scale=1.0)]


def test_fp32_emulation_stays_inside_the_interval():
    g = torch.Generator().manual_seed(3)
    for O, I in ((64, 64), (192, 320)):
        base = _base(O, I, g)
        terms = _mixed(O, I, g)
        for sub in ([terms[1]], [terms[2]], [terms[4]], terms):
            t, E = YR.terms_reference(base, sub)
            dev = YR.emulate_fp32(base, sub)
            LR.check_fold(dev, t, E, f'{O}x{I} {[x["kind"] for x in sub]}')
            assert bool((dev != base).float().mean() > 0.9)                        # the terms do move the weights
        assert (E / t.abs().clamp(min=2.0 ** -126)).median().item() < 2.0 ** -12                   # E is far below half a bf16 ulp (2^-9 relative) as a rule


def test_mutated_references_leave_the_interval():
    g = torch.Generator().manual_seed(4)
    O, I = 192, 320
    base = _base(O, I, g)
    loha = [dict(YR.loha_operands(O, I, 8, 33, g), scale=0.7)]
    lokr = [dict(YR.lokr_operands(16, I // 32, 16, 32, g), scale=-0.3, row0=64)]
    for terms, mutations in ((loha, ('loha_bf16_products', 'loha_add')), (lokr, ('lokr_swap_index', 'lokr_ignore_row0'))):
        dev = YR.emulate_fp32(base, terms)
        LR.check_fold(dev, *YR.terms_reference(base, terms), 'un-mutated')
        for m in mutations:
            assert LR.failing(dev, *YR.terms_reference(base, terms, mutate=m)).any(), m
