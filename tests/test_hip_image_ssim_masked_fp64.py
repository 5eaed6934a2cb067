"""``afx_image_ssim_masked`` -- ``afx_image_ssim``'s window SSIM with every window weighted by the Gaussian mean of an edit's mask over the
window's own support: per sample (sum w ssim, sum w, sum (1 - w) ssim, sum (1 - w)) -- against the torch fp64 restatement of
tests/masked_score_ref.py on the CPU from the same inputs: fp32 and bf16 operands, transform 0 (data_range 2.0) and transform 1.

Shapes [B, C, H, W] (a work-group is a tile of 32 x 16 windows of one plane): [2, 3, 11, 11] one window; [2, 3, 12, 43] 2 x 33 windows,
crossing the 32-window tile edge; [2, 3, 27, 12] 17 x 2 windows, crossing the 16-window tile edge.  The mask is [2, 1, H, W] (one per
sample) and [1, 1, H, W] (shared): random, fractional, non-symmetric, with exact zeros and ones.

Bound on |kernel mean - reference mean| per sample and region (``masked_score_ref.masked_ssim_bound``): that of
tests/test_hip_image_ssim_fp64.py, whose per-window term e_i = 2 u (346 S / B1 + 521 S / B2 + 21) and summation term 2 N u are taken
over as they are; the mean there is unweighted, here window i enters with weight w_i on both sides:
  * sum_i w_i e_i / sum_i w_i in place of the plain mean of e_i (every ssim_i within e_i, |ssim_i| <= 1);
  * numerator and denominator are sums of N non-negative terms: N u each, 2 N u on the quotient (as there);
  * the weight itself: the mask is non-negative, so its two 11-tap passes have no cancellation and w_i has the relative error of a moment
    there, <= 86 u on either side; the quotient sum w s / sum w moves by at most 2 max|delta_i| max|s_i - mean| <= 4 x 86 u per side, and
    the clamp and 1 - w add one rounding each: 700 u covers both sides.
The bound stays below 1e-7 on every case (asserted), the level above which the order of operations would be wrong.

Also asserted: a == b gives sum w ssim == sum w and sum (1 - w) ssim == sum (1 - w) bit for bit; m = 0 gives both repaint sums exactly 0 and
the kept pair (sum ssim, window count) of ``ops.image_ssim``; m = 1 gives a repaint mean within the bound of ``ops.image_ssim``'s mean; two
calls are bit-identical, slots included, and the slots added in the order the header states are the result; mutated references (the
weight taken at the window's centre, the mask read transposed) are missed by more than 1000 bounds, in the repaint mean or in the repaint
weight sum (one window per plane: the mean cannot see the weight, the weight sum does); guard elements around ``out`` and ``ws``
stay untouched; refused calls leave ``out`` as it was.
"""
import functools

import pytest
import torch

import masked_score_ref as MR
import ssim_ref as SR

pytestmark = pytest.mark.gpu

GUARD = 64
SHAPES = [(2, 3, 11, 11), (2, 3, 12, 43), (2, 3, 27, 12)]
TILES = {(11, 11): 1, (12, 43): 2, (27, 12): 2}          # ceil((H - 10) / 16) ceil((W - 10) / 32)


@functools.lru_cache(maxsize=None)
def _case(shape, dname, transform, mask_batch):
    B, C, H, W = shape
    a, b = SR.make_inputs(*shape, dname, 'noisy', bool(transform))
    L = 1.0 if transform else 2.0
    mask = MR.random_mask((mask_batch, 1, H, W), 17 + H + 3 * W + mask_batch)
    sums = MR.masked_ssim_sums(a, b, mask, bool(transform), L)
    means = torch.stack([sums[:, 0] / sums[:, 1], sums[:, 2] / sums[:, 3]], 1)
    muts = {'centre_weight': MR.masked_ssim_sums(a, b, mask, bool(transform), L, centre=True)}
    if (H, W) != (11, 11):          # one window: the Gaussian window is symmetric, the transposed mask has the same mean
        muts['mask_transposed'] = MR.masked_ssim_sums(a, b, mask, bool(transform), L, transpose=True)
    return dict(a=a, b=b, mask=mask, L=L, sums=sums, means=means, bound=MR.masked_ssim_bound(a, b, mask, bool(transform), L), muts=muts,
                plain=SR.ssim_mean(a, b, bool(transform), L), plain_bound=SR.ssim_bound(a, b, bool(transform), L))


def _guarded(numel, sentinel=-768.0):
    buf = torch.full((numel + 2 * GUARD,), sentinel, dtype=torch.float64, device='cuda')
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(buf, numel, sentinel=-768.0):
    return bool((buf[:GUARD] == sentinel).all() and (buf[GUARD + numel:] == sentinel).all())


def _ordered_sum(slots):
    """slots [B, parts] fp64 (CPU) -> the second launch's sum: lane l adds slots l, l + 64, ... in index order, then the xor shuffle tree."""
    B, parts = slots.shape
    pad = torch.zeros(B, (parts + 63) // 64 * 64, dtype=torch.float64)
    pad[:, :parts] = slots
    lanes = torch.zeros(B, 64, dtype=torch.float64)
    for row in pad.view(B, -1, 64).unbind(1):
        lanes = lanes + row
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, idx ^ o]
    return lanes[:, 0]


def _means(out):
    return torch.stack([out[:, 0] / out[:, 1], out[:, 2] / out[:, 3]], 1)


def _away(sums, mutant, bound, n_win, factor):
    """Per sample: is ``sums`` [B, 4] more than ``factor`` bounds away from ``mutant`` [B, 4], in the repaint mean or in the repaint weight
    sum?  (With one window per plane the mean does not see the weight at all: sum w s / sum w = s.  The weight sum does.)"""
    mean_off = (_means(sums)[:, 0] - _means(mutant)[:, 0]).abs() > factor * bound[:, 0]
    weight_off = (sums[:, 1] - mutant[:, 1]).abs() > factor * (2 * n_win + 700) * MR.U * n_win
    return mean_off | weight_off


@pytest.mark.parametrize('mask_batch', [2, 1], ids=['per_sample', 'shared'])
@pytest.mark.parametrize('transform', [0, 1], ids=['asis_L2', 'image'])
@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_masked_ssim_within_fp64_bound_reproducible_and_guarded(shape, dname, transform, mask_batch):
    from arcflow_amd import _lib, ops
    B, C, H, W = shape
    c = _case(shape, dname, transform, mask_batch)
    bound = c['bound']
    n_win = C * (H - 10) * (W - 10)
    for name, m in c['muts'].items():          # CPU side first: every mutation moves the reference of every sample by more than 2000 bounds
        assert _away(c['sums'], m, bound, n_win, 2000).all(), (name, m.tolist(), c['sums'].tolist())
    parts = C * TILES[(H, W)]
    need = _lib.load().afx_image_ssim_masked_ws_bytes(B, C, H, W)
    assert need == B * parts * 32
    a, b, mask = c['a'].cuda(), c['b'].cuda(), c['mask'].cuda()
    outs, slots = [], []
    for _ in range(2):
        wbuf, ws = _guarded(need // 8)
        obuf, out = _guarded(B * 4)
        r = ops.image_ssim_masked(a, b, mask, transform=bool(transform), data_range=c['L'], out=out.view(B, 4), ws=ws)
        torch.cuda.synchronize()
        assert r.data_ptr() == out.data_ptr() and r.shape == (B, 4) and r.dtype == torch.float64
        assert _guards_intact(wbuf, need // 8) and _guards_intact(obuf, B * 4)
        outs.append(out.cpu().clone().view(B, 4))
        slots.append(ws.cpu().clone())
    assert torch.equal(outs[1].view(torch.int64), outs[0].view(torch.int64)) and torch.equal(slots[1].view(torch.int64), slots[0].view(torch.int64))
    assert torch.equal(a.cpu(), c['a']) and torch.equal(b.cpu(), c['b']) and torch.equal(mask.cpu(), c['mask'])          # the operands are read only
    s = slots[0].view(B, parts, 4)
    for k in range(4):
        assert torch.equal(_ordered_sum(s[:, :, k].contiguous()).view(torch.int64), outs[0][:, k].contiguous().view(torch.int64)), k
    got = _means(outs[0])
    err = (got - c['means']).abs()
    wsum_err = (outs[0][:, [1, 3]] - c['sums'][:, [1, 3]]).abs()
    print(f'{shape} {dname} transform={transform} mask_batch={mask_batch}: repaint / keep mean ssim {got.tolist()}  max err {err.max().item():.3e}  '
          f'bound {bound.max().item():.3e}  err / bound {(err / bound).max().item():.3e}  weight sums {outs[0][:, [1, 3]].tolist()}')
    assert torch.isfinite(got).all() and bound.max().item() < 1e-7
    assert (err <= bound).all(), (err / bound).tolist()
    assert (wsum_err <= (2 * n_win + 700) * MR.U * n_win).all()                        # the two weight sums, N terms in [0, 1] each
    assert ((outs[0][:, 1] + outs[0][:, 3] - n_win).abs() <= (2 * n_win + 700) * MR.U * n_win).all()
    for name, m in c['muts'].items():          # the kernel is more than 1000 bounds away from every mutated reference, on every sample
        assert _away(outs[0], m, bound, n_win, 1000).all(), (name, m.tolist(), outs[0].tolist())


@pytest.mark.parametrize('transform', [0, 1], ids=['asis_L2', 'image'])
@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
def test_equal_operands_zero_mask_and_unit_mask(dname, transform):
    from arcflow_amd import ops
    for shape in SHAPES:
        B, C, H, W = shape
        c = _case(shape, dname, transform, 2)
        a, b, mask = c['a'].cuda(), c['b'].cuda(), c['mask'].cuda()
        n_win = C * (H - 10) * (W - 10)
        for other in (a, a.clone()):            # a == b: every window is exactly 1.0, so the weighted sums ARE the weight sums
            same = ops.image_ssim_masked(a, other, mask, transform=bool(transform), data_range=c['L']).cpu()
            assert torch.equal(same[:, 0].contiguous().view(torch.int64), same[:, 1].contiguous().view(torch.int64)), (shape, same.tolist())
            assert torch.equal(same[:, 2].contiguous().view(torch.int64), same[:, 3].contiguous().view(torch.int64)) and (same[:, 1] > 0).all()
        plain = ops.image_ssim(a, b, transform=bool(transform), data_range=c['L']).cpu()
        zero = ops.image_ssim_masked(a, b, torch.zeros_like(mask), transform=bool(transform), data_range=c['L']).cpu()
        assert (zero[:, 0] == 0).all() and (zero[:, 1] == 0).all() and (zero[:, 3] == n_win).all()
        assert torch.equal(zero[:, 2].contiguous().view(torch.int64), plain.view(torch.int64))          # weight 1.0 on every window: the unmasked sum itself
        one = ops.image_ssim_masked(a, b, torch.ones(1, 1, H, W, device='cuda'), transform=bool(transform), data_range=c['L']).cpu()
        assert ((one[:, 0] / one[:, 1] - plain / n_win).abs() <= c['plain_bound']).all(), (shape, (one[:, 0] / one[:, 1] - plain / n_win).tolist())
        assert ((one[:, 0] / one[:, 1] - c['plain']).abs() <= c['plain_bound']).all()


def test_wrapper_allocates_reuses_and_refuses_wrong_operands():
    from arcflow_amd import _lib, ops
    shape = (2, 3, 12, 43)
    c = _case(shape, 'bf16', 1, 2)
    a, b, mask = c['a'].cuda(), c['b'].cuda(), c['mask'].cuda()
    got = ops.image_ssim_masked(a, b, mask, transform=True).cpu()            # data_range defaults to 1.0
    assert ((_means(got) - c['means']).abs() <= c['bound']).all()
    ws = ops.image_ssim_masked_ws(*shape)
    assert ws.numel() == 2 * 3 * 2 * 4 and ws.dtype == torch.float64 and ws.is_cuda
    out = torch.empty(2, 4, dtype=torch.float64, device='cuda')
    assert torch.equal(ops.image_ssim_masked(a, b, mask, transform=True, out=out, ws=ws).cpu(), got)
    shared = ops.image_ssim_masked(a, b, mask[:1].contiguous(), transform=True).cpu()
    assert torch.equal(shared[0], got[0]) and not torch.equal(shared[1], got[1])
    with pytest.raises(ValueError):
        ops.image_ssim_masked(a, b.float(), mask)                              # mixed dtypes
    with pytest.raises(ValueError):
        ops.image_ssim_masked(a.half(), b.half(), mask)                        # neither fp32 nor bf16
    with pytest.raises(ValueError):
        ops.image_ssim_masked(a, b, mask.bfloat16())                           # the mask is fp32
    with pytest.raises(ValueError):
        ops.image_ssim_masked(a, b, mask[:, :, :, :42].contiguous())           # another size
    with pytest.raises(ValueError):
        ops.image_ssim_masked(a, b, mask.expand(2, 3, 12, 43).contiguous())    # one plane, not one per channel
    with pytest.raises(ValueError):
        ops.image_ssim_masked(a[0], b[0], mask[0])                             # rank 3
    with pytest.raises(_lib.ArcflowHipError, match='mask_batch'):
        ops.image_ssim_masked(torch.cat([a, a[:1]]), torch.cat([b, b[:1]]), mask)
    with pytest.raises(_lib.ArcflowHipError):
        ops.image_ssim_masked(a.cpu(), b.cpu(), mask.cpu())                    # no CPU path
    with pytest.raises(_lib.ArcflowHipError, match='workspace'):
        ops.image_ssim_masked(a, b, mask, ws=torch.empty(47, dtype=torch.float64, device='cuda'))
    with pytest.raises(_lib.ArcflowHipError, match='11'):
        ops.image_ssim_masked(a[:, :, :10].contiguous(), b[:, :, :10].contiguous(), mask[:, :, :10].contiguous())


def test_every_guard_returns_its_error_without_launching():
    """Real device buffers with watched contents: a refused call leaves ``out`` and ``ws`` as they were (nothing was launched)."""
    from arcflow_amd import _lib, ops
    lib = _lib.load()
    B, C, H, W = 2, 3, 12, 43
    a = torch.zeros(B, C, H, W, device='cuda')
    mask = torch.ones(B, 1, H, W, device='cuda')
    out = torch.full((B, 4), -3.0, dtype=torch.float64, device='cuda')
    ws = torch.full((B * C * 2 * 4,), -5.0, dtype=torch.float64, device='cuda')
    P = lambda t, off=0: t.data_ptr() + off          # noqa: E731
    ok = dict(a=P(a), b=P(a), mask=P(mask), dtype=_lib.AFX_DT_F32, transform=0, data_range=1.0, out=P(out), ws=P(ws), ws_bytes=B * C * 2 * 32, batch=B,
              mask_batch=B, C=C, H=H, W=W)
    defects = [dict(a=None), dict(b=None), dict(mask=None), dict(out=None), dict(ws=None), dict(ws=P(ws, 4)), dict(out=P(out, 4)), dict(a=P(a, 2)),
               dict(mask=P(mask, 2)), dict(ws_bytes=B * C * 2 * 32 - 1), dict(H=10), dict(W=10), dict(dtype=_lib.AFX_DT_FP8), dict(dtype=0),
               dict(transform=2), dict(batch=0), dict(C=0), dict(mask_batch=3), dict(mask_batch=0), dict(data_range=0.0)]
    for d in defects:
        k = dict(ok, **d)
        rc = lib.afx_image_ssim_masked(k['a'], k['b'], k['mask'], k['dtype'], k['transform'], k['data_range'], k['out'], k['ws'], k['ws_bytes'],
                                       k['batch'], k['mask_batch'], k['C'], k['H'], k['W'], None)
        assert rc == _lib.AFX_E_INVALID and b'afx_image_ssim_masked' in lib.afx_last_error(), (d, rc, lib.afx_last_error())
    torch.cuda.synchronize()
    assert (out == -3.0).all() and (ws == -5.0).all()
    got = ops.image_ssim_masked(a, a, mask).cpu()          # and the good call runs: every window is 1.0
    assert torch.equal(got[:, 0], got[:, 1]) and ((got[:, 1] - C * 2 * 33).abs() < 1e-9).all()
