"""``afx_lora_fold_terms`` alone against the fp64 reference of tests/lycoris_fold_ref.py, per element, no element left out.

Criterion (derived in lycoris_fold_ref.py): a device value passes iff rne_bf16(t - E) <= d <= rne_bf16(t + E), E = (N + 2 J + 3 JD + 2) 2^-24 mag, N the
roundings inside the terms (r per LoRA term, r1 + r2 per LoHa term, 1 per LoKr term).

Frames and canaries are those of tests/test_hip_lora_fold_fp64.py (its helpers are imported): every case folds into rows 64 .. 64 + O of a taller
dst from rows 64 .. 64 + O of a taller base, the (192, 320) case with leading dimensions above I; rows outside the slice and columns past I keep
their canary bits, base is unchanged.  Shapes (64, 64), (192, 320), (320, 192): one tile, 3 x 5 and 5 x 3 tiles.

LoHa: ranks 1, 8, 33 and 130 (a partial MFMA K-step, the unaligned-row path, several steps with a ragged tail), unequal ranks in the two pairs,
scales 1, -0.3 and 0.  LoKr: c and d in {64, 96, 32, 1} and c = O; c = 96 and 48 do not divide 64, so a tile straddles rows of w1; row0 = 0 and 64
with the slice inside a taller virtual delta.  The operands are sized so that |s D| is of the size of the weights (standard deviation 0.02):
``test_deltas_are_of_the_size_of_the_weights`` holds the cases to that, since a delta below half an ulp of the base would show nothing.

Mixed: one 8-term call with all three kinds and a LoRA term with row gains.  Equivalence: a call with LoRA terms alone, with and without gains, is
bit-identical to ``ops.lora_fold``; J = 0 copies and keeps -0; eight runs are bit-identical.  Five mutated references must FAIL the check.
On the parent commit every test here fails: ``ops.lora_fold_terms`` does not exist."""
import pytest
import torch

import lora_fold_ref as LR
import lycoris_fold_ref as YR
from test_hip_lora_fold_fp64 import R0, SHAPES, _assert_frame_intact, _bits, _frames, _operands

pytestmark = pytest.mark.gpu

LOHA = {                                                         # (r1, r2), scale
    'r1': ((1, 1), 1.0),
    'r8': ((8, 8), -0.3),
    'r33': ((33, 33), 1.0),
    'r130': ((130, 130), -0.3),
    'r8_33': ((8, 33), 1.0),
    'r130_1': ((130, 1), 0.7),
    'r16_s0': ((16, 16), 0.0),
}
LOKR = {                                                         # c, d, row0, scale; w1 has ceil((row0 + O) / c) rows
    'c64_d64': (64, 64, 0, 1.0),
    'c96_d32_row64': (96, 32, 64, -0.3),                         # a tile of 64 rows straddles rows of w1; the virtual delta is taller than row0 + O
    'c32_d1': (32, 1, 0, 1.0),
    'c1_d64_row64': (1, 64, 64, 0.7),
    'c48_d96_row64': (48, 96, 64, 1.0),                          # d = 96 divides I = 192 only: the other shapes run the (320, 192) case
    'cO_d32': ('O', 32, 0, -0.3),                                # c = the full O: w1 has one row
    'cO64_d1_row64': ('O+64', 1, 64, 1.0),                       # one row of w1, the slice starting at row 64 of it
}


def _to_cuda(term):
    return {k: v.cuda() if isinstance(v, torch.Tensor) else v for k, v in term.items()}


def _fold_terms(base, terms, O, I, ldd, ldb):
    from arcflow_amd import ops
    dst_full, base_full = _frames(base, O, I, ldd, ldb)
    before = _bits(base_full)
    out = ops.lora_fold_terms(base_full[R0:R0 + O, :I], dst_full[R0:R0 + O, :I], [_to_cuda(t) for t in terms])
    torch.cuda.synchronize()
    _assert_frame_intact(dst_full, base_full, before, O, I)
    return out.cpu()


def _base(O, I, seed):
    return _operands(O, I, (), seed)[0]


def _loha_case(O, I, name):
    (r1, r2), s = LOHA[name]
    g = torch.Generator().manual_seed(1000 + O + I + r1 + 3 * r2)
    return _base(O, I, O + r1), [dict(YR.loha_operands(O, I, r1, r2, g), scale=s)]


def _lokr_case(O, I, name):
    c, d, row0, s = LOKR[name]
    c = O if c == 'O' else O + 64 if c == 'O+64' else c
    if I % d:
        return None
    g = torch.Generator().manual_seed(2000 + O + I + c + d)
    return _base(O, I, O + c), [dict(YR.lokr_operands(-(-(row0 + O) // c), I // d, c, d, g), scale=s, row0=row0)]


def _mixed_case(O, I):
    """Eight terms: 3 LoRA (one with row gains), 3 LoHa, 2 LoKr."""
    g = torch.Generator().manual_seed(77 + O)
    base, A, B = _operands(O, I, (16, 4, 130), seed=O + I)
    gain = (torch.rand(O, generator=g) * 0.4 + 0.8).float()
    terms = [dict(kind='lora', A=A[0], B=B[0], scale=1.0),
             dict(YR.loha_operands(O, I, 8, 33, g), scale=0.7),
             dict(YR.lokr_operands(-(-(O + 64) // 96), I // 32, 96, 32, g), scale=-0.3, row0=64),
             dict(kind='lora', A=A[1], B=B[1], scale=0.5, row_gain=gain),
             dict(YR.loha_operands(O, I, 130, 1, g), scale=1.0),
             dict(YR.lokr_operands(1, I // 64, O, 64, g), scale=0.5),
             dict(kind='lora', A=A[2], B=B[2], scale=-1.25),
             dict(YR.loha_operands(O, I, 1, 1, g), scale=-0.3)]
    return base, terms


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('name', list(LOHA))
def test_loha_vs_fp64(shape, name):
    O, I, ldd, ldb = shape
    base, terms = _loha_case(O, I, name)
    dev = _fold_terms(base, terms, O, I, ldd, ldb)
    share = LR.check_fold(dev, *YR.terms_reference(base, terms), f'LoHa {name} {O}x{I}')
    print(f'LoHa {name} {O}x{I}: share of elements equal to rne(t) {share:.6f}')
    if terms[0]['scale'] == 0.0:
        assert torch.equal(dev.float(), base.float())                    # scale 0: the values of the base (0 * finite = 0)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('name', list(LOKR))
def test_lokr_vs_fp64(shape, name):
    O, I, ldd, ldb = shape
    case = _lokr_case(O, I, name)
    if case is None:
        assert name == 'c48_d96_row64' and I != 192                     # the one factorisation that only fits I = 192
        case = _lokr_case(320, 192, name)
        O, I, ldd, ldb = SHAPES[2]
    base, terms = case
    dev = _fold_terms(base, terms, O, I, ldd, ldb)
    share = LR.check_fold(dev, *YR.terms_reference(base, terms), f'LoKr {name} {O}x{I}')
    print(f'LoKr {name} {O}x{I}: share of elements equal to rne(t) {share:.6f}')


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_mixed_eight_terms_vs_fp64(shape):
    O, I, ldd, ldb = shape
    base, terms = _mixed_case(O, I)
    assert len(terms) == 8 and {t['kind'] for t in terms} == {'lora', 'loha', 'lokr'}
    dev = _fold_terms(base, terms, O, I, ldd, ldb)
    LR.check_fold(dev, *YR.terms_reference(base, terms), f'mixed {O}x{I}')


def test_deltas_are_of_the_size_of_the_weights():
    """No GPU work: every case above adds a delta whose standard deviation is within a factor 10 of the weights' 0.02 (scale 0 aside; a w1 of
    four elements makes the sample's spread wide), so the
    interval check is sensitive to it: the fp64 target differs from the base's bf16 value nearly everywhere."""
    for O, I, _, _ in SHAPES:
        cases = [(n, _loha_case(O, I, n)) for n in LOHA] + [(n, _lokr_case(O, I, n)) for n in LOKR]
        for name, case in cases:
            if case is None or case[1][0]['scale'] == 0.0:
                continue
            base, terms = case
            t, _ = YR.terms_reference(base, terms)
            ratio = (t - base.double()).std().item() / 0.02
            assert 0.1 < ratio < 10.0, (name, O, I, ratio)
            assert (LR.rne_bf16(t) != base.double()).double().mean().item() > 0.9, (name, O, I)


def test_lora_terms_alone_are_lora_fold_bit_for_bit():
    from arcflow_amd import ops
    O, I, ldd, ldb = SHAPES[1]
    ranks, scales = (16, 16, 130), (1.0, 0.0, -1.25)
    base, A, B = _operands(O, I, ranks, seed=21)
    g = torch.Generator().manual_seed(22)
    for gains in (None, [None, (torch.rand(O, generator=g) + 0.5).float(), (torch.rand(O, generator=g) + 0.5).float()]):
        terms = [dict(kind='lora', A=a, B=b, scale=s, row_gain=None if gains is None else gn)
                 for a, b, s, gn in zip(A, B, scales, gains or [None] * 3)]
        dev = _fold_terms(base, terms, O, I, ldd, ldb)
        want = torch.empty(O, I, dtype=torch.bfloat16, device='cuda')
        ops.lora_fold(base.cuda(), want, [a.cuda() for a in A], [b.cuda() for b in B], scales,
                      row_gains=None if gains is None else [None if gn is None else gn.cuda() for gn in gains])
        torch.cuda.synchronize()
        assert torch.equal(_bits(dev), _bits(want)), 'with gains' if gains else 'without gains'
        LR.check_fold(dev, *YR.terms_reference(base, terms), 'LoRA terms')


def test_no_terms_copy_and_keep_negative_zero():
    O, I, ldd, ldb = SHAPES[1]
    base = _base(O, I, 23)
    base[::3, ::5] = -0.0
    dev = _fold_terms(base, [], O, I, ldd, ldb)
    assert torch.equal(_bits(dev), _bits(base)) and bool((_bits(dev) == -32768).any())          # 0x8000: -0 stays -0


def test_fold_terms_is_bit_reproducible():
    O, I, ldd, ldb = SHAPES[2]
    base, terms = _mixed_case(O, I)
    runs = [_bits(_fold_terms(base, terms, O, I, ldd, ldb)) for _ in range(8)]
    assert all(torch.equal(r, runs[0]) for r in runs[1:])


def test_mutated_references_fail_the_check():
    O, I, ldd, ldb = SHAPES[1]
    base, terms = _loha_case(O, I, 'r8_33')
    dev = _fold_terms(base, terms, O, I, ldd, ldb)
    t, E = YR.terms_reference(base, terms)
    LR.check_fold(dev, t, E, 'un-mutated LoHa')
    # 1. each LoHa product rounded to bf16 before the multiply (the fp64 reference confirms first that this moves at least one element)
    t_mut, E_mut = YR.terms_reference(base, terms, mutate='loha_bf16_products')
    assert (LR.rne_bf16(t_mut) != LR.rne_bf16(t)).any(), 'the extra roundings move no element: the case shows nothing'
    assert LR.failing(dev, t_mut, E_mut).any()
    # 2. the LoHa products added instead of multiplied
    assert LR.failing(dev, *YR.terms_reference(base, terms, mutate='loha_add')).any()
    # 5. the scale rounded into a bf16 operand: s = 0.7 makes w1_a * s inexact in bf16
    term = dict(terms[0], scale=0.7)
    dev = _fold_terms(base, [term], O, I, ldd, ldb)
    t, E = YR.terms_reference(base, [term])
    LR.check_fold(dev, t, E, 'un-mutated LoHa, s = 0.7')
    mut = dict(term, w1_a=(term['w1_a'].float() * 0.7).bfloat16(), scale=1.0)
    t_mut, E_mut = YR.terms_reference(base, [mut])
    assert (LR.rne_bf16(t_mut) != LR.rne_bf16(t)).any()
    assert LR.failing(dev, t_mut, E_mut).any()
    # 3. o / c and o % c exchanged in the LoKr index: a = c = 20, rows 64 .. 384 of 400
    O, I, ldd, ldb = SHAPES[2]
    g = torch.Generator().manual_seed(31)
    base = _base(O, I, 24)
    terms = [dict(YR.lokr_operands(20, 6, 20, 32, g), scale=1.0, row0=64)]
    dev = _fold_terms(base, terms, O, I, ldd, ldb)
    LR.check_fold(dev, *YR.terms_reference(base, terms), 'un-mutated LoKr')
    assert LR.failing(dev, *YR.terms_reference(base, terms, mutate='lokr_swap_index')).any()
    # 4. row0 ignored
    assert LR.failing(dev, *YR.terms_reference(base, terms, mutate='lokr_ignore_row0')).any()
