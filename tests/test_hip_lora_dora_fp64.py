"""``afx_lora_row_gain`` and ``afx_lora_fold_rows`` (DoRA adapters) against the fp64 references of tests/lora_dora_ref.py: every row gain inside
its interval, every folded element inside [rne(t - E), rne(t + E)], nothing left out.  The bounds are derived in lora_dora_ref.py by counting
roundings; none of them comes from what the kernels return.

Shapes, frames and operands are those of tests/test_hip_lora_fold_fp64.py: (64, 64) is one tile, (192, 320) with leading dimensions 384 / 448 and
(320, 192) give ragged tile counts both ways; every slice sits at row 64 of a taller frame of canaries, and the gains are written into a framed
vector too.  Ranks 1, 8 and 130 (a partial MFMA K-step, the unaligned rows of B, several steps with a ragged tail), scales 1, -0.3 and 0.  The
magnitudes are the rows' own norms times 0.8 .. 1.2 (gains near 1, as a trained DoRA has), one of them negative and one 0.

The two kernels are judged apart (the fold is fed the fp32-rounded REFERENCE gains) and then chained (device gains into the device fold,
against the composed bound).  Without gains the fold is bit-identical to ``ops.lora_fold``.  Eight runs of each kernel are bit-identical.  Five
mutated references must FAIL the same checks.  On the parent commit every test here fails: ``ops.lora_row_gain`` does not exist."""
import pytest
import torch

import lora_dora_ref as DR
import lora_fold_ref as LR
from test_hip_lora_fold_fp64 import CANARY, R0, SHAPES, _assert_frame_intact, _bits, _frames, _operands

pytestmark = pytest.mark.gpu

F32_CANARY = 1.5e30
SETS = {                                               # ranks, scales, which adapters carry a magnitude
    'dora': ((16,), (0.8,), (0,)),
    'dora_plain': ((16, 4), (1.0, -0.3), (0,)),
    'dora2_plain': ((16, 4, 130), (1.0, 0.0, -0.3), (0, 1)),
    'j8_dora3': ((8,) * 8, (1.0, -1.0, 0.5, 8.0, 0.0, -0.25, 2.0, 0.125), (1, 4, 6)),
}


def _magnitudes(base, n, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        m = (base.double().norm(dim=1) * (0.8 + 0.4 * torch.rand(base.shape[0], generator=g).double())).float()
        m[3], m[17] = -m[3], 0.0
        out.append(m)
    return out


def _gain(base, A, B, s, m, O, I, ldb):
    from arcflow_amd import ops
    _, base_full = _frames(base, O, I, I, ldb)
    before = _bits(base_full)
    out_full = torch.full((O + 128,), F32_CANARY, dtype=torch.float32).cuda()
    a, b, md = A.cuda(), B.cuda(), m.cuda()
    out = ops.lora_row_gain(base_full[R0:R0 + O, :I], a, b, s, md, out=out_full[R0:R0 + O])
    torch.cuda.synchronize()
    full = out_full.cpu()
    assert bool((full[:R0] == F32_CANARY).all()) and bool((full[R0 + O:] == F32_CANARY).all()), 'gains outside the slice were written'
    assert torch.equal(_bits(base_full), before), 'base was written'
    assert torch.equal(a.cpu(), A) and torch.equal(b.cpu(), B) and torch.equal(md.cpu(), m)
    return out.cpu()


def _fold_rows(base, A, B, scales, gains, O, I, ldd, ldb):
    from arcflow_amd import ops
    dst_full, base_full = _frames(base, O, I, ldd, ldb)
    before = _bits(base_full)
    kw = {} if isinstance(gains, str) else dict(row_gains=[None if g is None else g.cuda() for g in gains])      # 'plain': the call without row_gains
    out = ops.lora_fold(base_full[R0:R0 + O, :I], dst_full[R0:R0 + O, :I], [a.cuda() for a in A], [b.cuda() for b in B], scales, **kw)
    torch.cuda.synchronize()
    _assert_frame_intact(dst_full, base_full, before, O, I)
    return out.cpu()


def _reference_gains(base, A, B, scales, mags, dora):
    """-> per adapter None or (g, lo, hi) fp64, each with the adapter's own scale."""
    return [DR.gain_reference(base, A[j], B[j], scales[j], mags[j]) if j in dora else None for j in range(len(A))]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('rank', [1, 8, 130])
def test_gain_vs_fp64(shape, rank):
    O, I, _, ldb = shape
    base, A, B = _operands(O, I, (rank,), seed=O + I + rank)
    m = _magnitudes(base, 1, seed=rank)[0]
    for s in (1.0, -0.3, 0.0):
        g, lo, hi = DR.gain_reference(base, A[0], B[0], s, m)
        dev = _gain(base, A[0], B[0], s, m, O, I, ldb)
        DR.check_gain(dev, lo, hi, f'r{rank} s{s} {O}x{I}')
        assert dev[17] == 0 and dev[3] < 0
        print(f'r{rank} s{s} {O}x{I}: largest |device - fp64| / interval half-width {((dev.double() - g).abs() / ((hi - lo) / 2).clamp(min=1e-300)).max():.3f}')


def test_gain_heavy_tailed_rows_and_a_row_of_zeros():
    O, I, _, ldb = SHAPES[1]
    base, A, B = _operands(O, I, (130,), seed=5, heavy=True)
    assert base.float().abs().max() > 50 * base.float().abs().median()
    base[9], B[0][9] = 0, 0                                                       # w and B A are 0 along row 9: the sum of squares is 0
    m = _magnitudes(base, 1, seed=5)[0]
    m[9] = 1.0
    g, lo, hi = DR.gain_reference(base, A[0], B[0], -0.3, m)
    assert g[9] == 0 and lo[9] == 0 and hi[9] == 0
    dev = _gain(base, A[0], B[0], -0.3, m, O, I, ldb)
    DR.check_gain(dev, lo, hi, 'heavy-tailed')
    assert dev[9] == 0 and torch.isfinite(dev).all()                              # gain 0, where peft divides by zero


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('adapters', list(SETS))
def test_fold_rows_vs_fp64(shape, adapters):
    O, I, ldd, ldb = shape
    ranks, scales, dora = SETS[adapters]
    base, A, B = _operands(O, I, ranks, seed=O + I + len(ranks))
    mags = _magnitudes(base, len(ranks), seed=len(ranks))
    ref = _reference_gains(base, A, B, scales, mags, dora)
    gains = [None if r is None else r[0].float() for r in ref]                    # the fp32-rounded reference gains: the fold is judged on its own
    t, E = DR.fold_rows_reference(base, A, B, scales, gains)
    dev = _fold_rows(base, A, B, scales, gains, O, I, ldd, ldb)
    share = LR.check_fold(dev, t, E, f'{adapters} {O}x{I}')
    print(f'{adapters} {O}x{I}: share of elements equal to rne(t) {share:.6f}')


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_device_gains_into_device_fold(shape):
    O, I, ldd, ldb = shape
    ranks, scales, dora = SETS['dora2_plain']
    base, A, B = _operands(O, I, ranks, seed=O + 3 * I, heavy=(O == 192))
    mags = _magnitudes(base, len(ranks), seed=7)
    ref = _reference_gains(base, A, B, scales, mags, dora)
    dev_gains = [None if r is None else _gain(base, A[j], B[j], scales[j], mags[j], O, I, ldb) for j, r in enumerate(ref)]
    for j, r in enumerate(ref):
        if r is not None:
            DR.check_gain(dev_gains[j], r[1], r[2], f'adapter {j}')
    radius = [None if r is None else torch.maximum(r[2] - r[0], r[0] - r[1]) for r in ref]
    t, E = DR.fold_rows_reference(base, A, B, scales, [None if r is None else r[0] for r in ref], radius)
    LR.check_fold(_fold_rows(base, A, B, scales, dev_gains, O, I, ldd, ldb), t, E, f'chained {O}x{I}')


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_without_gains_the_bits_of_lora_fold(shape):
    O, I, ldd, ldb = shape
    for ranks, scales in (((), ()), ((1,), (1.0,)), ((16, 16, 130), (1.0, 0.0, -1.25)), ((8,) * 8, (1.0, -1.0, 0.5, 8.0, 0.0, -0.25, 2.0, 0.125))):
        base, A, B = _operands(O, I, ranks, seed=O + I + len(ranks))
        base[0, :8] = torch.tensor([0.0, -0.0] * 4).bfloat16()
        plain = _bits(_fold_rows(base, A, B, scales, 'plain', O, I, ldd, ldb))
        assert torch.equal(_bits(_fold_rows(base, A, B, scales, [None] * len(ranks), O, I, ldd, ldb)), plain), ranks


def test_both_kernels_are_bit_reproducible():
    O, I, ldd, ldb = SHAPES[2]
    ranks, scales, dora = SETS['dora2_plain']
    base, A, B = _operands(O, I, ranks, seed=6)
    mags = _magnitudes(base, len(ranks), seed=6)
    runs = [_gain(base, A[0], B[0], scales[0], mags[0], O, I, ldb) for _ in range(8)]
    assert all(torch.equal(r.view(torch.int32), runs[0].view(torch.int32)) for r in runs[1:])
    gains = [runs[0], _gain(base, A[1], B[1], scales[1], mags[1], O, I, ldb), None]
    folds = [_bits(_fold_rows(base, A, B, scales, gains, O, I, ldd, ldb)) for _ in range(8)]
    assert all(torch.equal(f, folds[0]) for f in folds[1:])


def test_mutated_references_fail_the_checks():
    # ---- the gain
    s = -0.3
    base, A, B = _operands(64, 64, (8,), seed=8, ab_std=0.1)
    m = _magnitudes(base, 1, seed=8)[0]
    dev = _gain(base, A[0], B[0], s, m, 64, 64, 64)
    g, lo, hi = DR.gain_reference(base, A[0], B[0], s, m)
    DR.check_gain(dev, lo, hi, 'un-mutated')
    mutants = {
        # 1. the norm taken down the columns: (w + s B A)^T = w^T + s A^T B^T
        'columns': DR.gain_reference(base.t().contiguous(), B[0].t().contiguous(), A[0].t().contiguous(), s, m),
        # 2. the gain taken from W without s B A
        'base only': DR.gain_reference(base, A[0], B[0], 0.0, m),
        # 5. s left out of the norm
        'no scale': DR.gain_reference(base, A[0], B[0], 1.0, m),
    }
    for name, (gm, lom, him) in mutants.items():
        assert bool(((gm - g).abs() > (hi - lo)).any()), f'{name}: the mutation moves no gain out of its interval, the case shows nothing'
        bad = DR.failing_gain(dev, lom, him)
        print(f'gain, {name}: {int(bad.sum())} of {bad.numel()} rows fail')
        assert bad.any(), name
    # ---- the fold
    O, I, ldd, ldb = SHAPES[1]
    ranks, scales, dora = (16, 4), (1.0, -0.3), (0,)
    base, A, B = _operands(O, I, ranks, seed=9)
    mags = _magnitudes(base, 2, seed=9)
    g0 = DR.gain_reference(base, A[0], B[0], scales[0], mags[0])[0].float()
    dev = _fold_rows(base, A, B, scales, [g0, None], O, I, ldd, ldb)
    t, E = DR.fold_rows_reference(base, A, B, scales, [g0, None])
    LR.check_fold(dev, t, E, 'un-mutated')
    # 3. the (g - 1) W term dropped: t - (c - 1) w with c - 1 = g - 1
    t_mut = t - (g0.double() - 1.0)[:, None] * base.double()
    # 4. the magnitude applied to the other adapter
    t_swap, E_swap = DR.fold_rows_reference(base, A, B, scales, [None, g0])
    for name, tm, Em in (('base term dropped', t_mut, E), ('gain on the other adapter', t_swap, E_swap)):
        moved = LR.rne_bf16(tm) != LR.rne_bf16(t)
        assert moved.any(), f'{name}: the mutation moves no element, the case shows nothing'
        bad = LR.failing(dev, tm, Em)
        print(f'fold, {name}: {int(moved.sum())} of {moved.numel()} elements round elsewhere, {int(bad.sum())} fail the check')
        assert bad.any(), name
