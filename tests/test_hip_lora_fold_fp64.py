"""``afx_lora_fold`` alone against the fp64 reference of tests/lora_fold_ref.py, per element, no element left out.

Criterion (derived in lora_fold_ref.py): a device value passes iff rne_bf16(t - E) <= d <= rne_bf16(t + E) with t the fp64 value of
base + sum_j s_j B_j A_j and E = (R + 2 J + 2) 2^-24 (|w| + sum_j |s_j| sum_r |B_j||A_j|), the fp32 accumulation error of any summation order.

Shapes: (64, 64) is one tile, (192, 320) and (320, 192) give ragged tile counts in both directions (3 x 5 and 5 x 3 tiles of 64 x 64, more than
one work-group each way).  Every case folds into rows 64 .. 64 + O of a taller dst from rows 64 .. 64 + O of a taller base; the (192, 320) case
has leading dimensions above I (384 for dst, 448 for base).  Ranks 1, 4, 8, 16, 64, 130 and 256 cover a single partial MFMA K-step, the
unaligned-row path of B (r % 8 != 0), exact multiples of the 32-rank step and several steps with a ragged tail.  Weights N(0, 0.02^2), A and B
N(0, 0.05^2); one case with rows of the base and of every B scaled by 150, the heavy-tailed rows tests/test_full_depth_parity.py injects
(``_inject_outliers``: a handful of output rows two orders of magnitude above the rest).

Around every result: the rows of dst outside the slice and the columns past I keep their canary bits, base is unchanged.  Eight runs are
bit-identical.  Four mutated references must FAIL the same check, so the check is known to see them: a scale on the wrong adapter, A transposed
within a square adapter, alpha / r dropped, and B * s rounded to bf16 before the product (what weights._merge_one does; the fp64 reference
confirms first that this second rounding moves at least one element to another bf16 value)."""
import ctypes as C

import pytest
import torch

import lora_fold_ref as LR

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64, 64, 64), (192, 320, 384, 448), (320, 192, 192, 192)]         # O, I, ld_dst, ld_base
ADAPTERS = {                                                                    # ranks, scales (0, negative, 1 and magnitude 8 all occur)
    'j0': ((), ()),
    'j1_r1': ((1,), (1.0,)),
    'j1_r64': ((64,), (-8.0,)),
    'j2_r4_256': ((4, 256), (0.75, -0.3)),
    'j3_r16_16_130': ((16, 16, 130), (1.0, 0.0, -1.25)),
    'j8_r8': ((8,) * 8, (1.0, -1.0, 0.5, 8.0, 0.0, -0.25, 2.0, 0.125)),
}
CANARY = 0x7B5A                 # bf16 bits of a finite value (about 1.1e36) that no result here comes near
R0 = 64


def _operands(O, I, ranks, seed, ab_std=0.05, heavy=False):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(O, I, generator=g) * 0.02
    A = [torch.randn(r, I, generator=g) * ab_std for r in ranks]
    B = [torch.randn(O, r, generator=g) * ab_std for r in ranks]
    if heavy:
        rows = [7, 41, O // 2 + 3, O - 1]
        base[rows] *= 150.0
        for b in B:
            b[rows] *= 150.0
    return base.bfloat16(), [a.bfloat16() for a in A], [b.bfloat16() for b in B]


def _frames(base, O, I, ldd, ldb):
    """-> (dst_full [O + 128, ldd] of canaries, base_full [O + 128, ldb] of canaries with base in rows R0 .. R0 + O, columns < I), on the GPU."""
    dst_full = torch.full((O + 128, ldd), CANARY, dtype=torch.int16).view(torch.bfloat16).cuda()
    base_full = torch.full((O + 128, ldb), CANARY, dtype=torch.int16).view(torch.bfloat16)
    base_full[R0:R0 + O, :I] = base
    return dst_full, base_full.cuda()


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _assert_frame_intact(dst_full, base_full, base_before, O, I):
    d = _bits(dst_full)
    assert bool((d[:R0] == CANARY).all()) and bool((d[R0 + O:] == CANARY).all()), 'rows of dst outside the slice were written'
    assert bool((d[R0:R0 + O, I:] == CANARY).all()), 'columns of dst past I were written'
    assert torch.equal(_bits(base_full), base_before), 'base was written'


def _fold(base, A, B, scales, O, I, ldd, ldb):
    from arcflow_amd import ops
    dst_full, base_full = _frames(base, O, I, ldd, ldb)
    before = _bits(base_full)
    out = ops.lora_fold(base_full[R0:R0 + O, :I], dst_full[R0:R0 + O, :I], [a.cuda() for a in A], [b.cuda() for b in B], scales)
    torch.cuda.synchronize()
    _assert_frame_intact(dst_full, base_full, before, O, I)
    return out.cpu()


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('adapters', list(ADAPTERS))
def test_fold_vs_fp64(shape, adapters):
    O, I, ldd, ldb = shape
    ranks, scales = ADAPTERS[adapters]
    base, A, B = _operands(O, I, ranks, seed=O + I + len(ranks))
    dev = _fold(base, A, B, scales, O, I, ldd, ldb)
    t, E = LR.fold_reference(base, A, B, scales)
    share = LR.check_fold(dev, t, E, f'{adapters} {O}x{I}')
    print(f'{adapters} {O}x{I}: share of elements equal to rne(t) {share:.6f}')
    if not ranks:
        assert torch.equal(_bits(dev), _bits(base))                      # J == 0: a plain copy, bit for bit


def test_fold_heavy_tailed_rows():
    O, I, ldd, ldb = SHAPES[1]
    ranks, scales = ADAPTERS['j3_r16_16_130']
    base, A, B = _operands(O, I, ranks, seed=5, heavy=True)
    assert base.float().abs().max() > 50 * base.float().abs().median()
    t, E = LR.fold_reference(base, A, B, scales)
    LR.check_fold(_fold(base, A, B, scales, O, I, ldd, ldb), t, E, 'heavy-tailed')


def test_fold_is_bit_reproducible():
    O, I, ldd, ldb = SHAPES[2]
    ranks, scales = ADAPTERS['j3_r16_16_130']
    base, A, B = _operands(O, I, ranks, seed=6)
    runs = [_bits(_fold(base, A, B, scales, O, I, ldd, ldb)) for _ in range(8)]
    assert all(torch.equal(r, runs[0]) for r in runs[1:])


def test_mutated_references_fail_the_check():
    O, I, ldd, ldb = SHAPES[1]
    # 1. a scale applied to the wrong adapter
    ranks, scales = ADAPTERS['j2_r4_256']
    base, A, B = _operands(O, I, ranks, seed=7)
    dev = _fold(base, A, B, scales, O, I, ldd, ldb)
    LR.check_fold(dev, *LR.fold_reference(base, A, B, scales), 'un-mutated')
    assert LR.failing(dev, *LR.fold_reference(base, A, B, scales[::-1])).any()
    # 2. A transposed within a square adapter (r == I == 64)
    base, A, B = _operands(64, 64, (64,), seed=8)
    dev = _fold(base, A, B, (1.0,), 64, 64, 64, 64)
    LR.check_fold(dev, *LR.fold_reference(base, A, B, (1.0,)), 'un-mutated')
    assert LR.failing(dev, *LR.fold_reference(base, [A[0].t().contiguous()], B, (1.0,))).any()
    # 3. alpha / r dropped: the device folds with weight * alpha / r = 0.8 * 8 / 16, the mutated reference with the weight alone
    base, A, B = _operands(O, I, (16,), seed=9)
    dev = _fold(base, A, B, (0.8 * 8 / 16,), O, I, ldd, ldb)
    LR.check_fold(dev, *LR.fold_reference(base, A, B, (0.8 * 8 / 16,)), 'un-mutated')
    assert LR.failing(dev, *LR.fold_reference(base, A, B, (0.8,))).any()
    # 4. the scaled B rounded to bf16 first (weights._merge_one): s = 0.7 makes B * s inexact in bf16; larger A / B so that the delta carries the sum
    s = 0.7
    base, A, B = _operands(O, I, (64,), seed=10, ab_std=0.1)
    dev = _fold(base, A, B, (s,), O, I, ldd, ldb)
    t, E = LR.fold_reference(base, A, B, (s,))
    LR.check_fold(dev, t, E, 'un-mutated')
    b_rounded = (B[0].float() * s).bfloat16()
    t_mut, E_mut = LR.fold_reference(base, A, [b_rounded], (1.0,))
    moved = LR.rne_bf16(t_mut) != LR.rne_bf16(t)
    assert moved.any(), 'the second rounding moves no element: the case shows nothing'
    bad = LR.failing(dev, t_mut, E_mut)
    print(f'operand rounding: {int(moved.sum())} of {moved.numel()} elements round elsewhere, {int(bad.sum())} fail the check')
    assert bad.any()


def test_guards_leave_dst_untouched():
    from arcflow_amd import _lib
    lib = _lib.load()
    O, I = 128, 128
    base, A, B = _operands(O, I, (4, 16), seed=11)
    dst_full, base_full = _frames(base, O, I, I, I)
    Ad, Bd = [a.cuda() for a in A], [b.cuda() for b in B]
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    stream = vp(torch.cuda.current_stream().cuda_stream)
    bp, dp = base_full[R0:].data_ptr(), dst_full[R0:].data_ptr()

    def call(base=bp, ldb=I, dst=dp, ldd=I, O=O, I=I, J=2, A=(Ad[0].data_ptr(), Ad[1].data_ptr()), B=(Bd[0].data_ptr(), Bd[1].data_ptr()),
             ranks=(4, 16), scales=(1.0, 0.5)):
        n = max(len(A), 1)
        return lib.afx_lora_fold(vp(base) if base else None, ldb, vp(dst) if dst else None, ldd, O, I, J, (vp * n)(*A), (vp * n)(*B),
                                 (i32 * n)(*ranks), (f32 * n)(*scales), stream)
    for kw in (dict(base=0), dict(dst=0), dict(A=(Ad[0].data_ptr(), 0)), dict(B=(0, Bd[1].data_ptr())),
               dict(J=9, A=(Ad[0].data_ptr(),) * 9, B=(Bd[0].data_ptr(),) * 9, ranks=(4,) * 9, scales=(1.0,) * 9),
               dict(ranks=(4, 0)), dict(O=96), dict(I=96), dict(ldb=64), dict(ldd=120),
               dict(base=dp + 64 * I * 2),                                          # base starts inside dst
               dict(dst=bp)):                                                       # dst is base: dst_full is not what would be written, base is
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((_bits(dst_full) == CANARY).all())
    want = torch.full((O + 128, I), CANARY, dtype=torch.int16)
    want[R0:R0 + O] = _bits(base)
    assert torch.equal(_bits(base_full), want)
    assert call() == 0                                                              # the same arguments un-mutated do run
    torch.cuda.synchronize()
    LR.check_fold(dst_full[R0:R0 + O].cpu(), *LR.fold_reference(base, A, B, (1.0, 0.5)), 'after the guards')
