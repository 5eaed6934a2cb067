"""``afx_sample_score_masked`` -- the agreement sums of training-time evaluation weighted by an edit's mask, a repainted (w = m) and a kept
(w = 1 - m) set of (sum w, sum w d^2, sum w a^2, sum w b^2, sum w a b) per sample -- against the torch fp64 restatement of
tests/masked_score_ref.py on the CPU from the same inputs: fp32 and bf16 operands, with and without the image-range transform.

Shapes.  Packed latents [B, N, 64] with the [B, N, 4] mask of ``afx_edit_blend``: N = 4 (one partial round of lanes), N = 130
(n = 8320: two work-groups, the second nearly empty), N = 257 (n = 16448: three work-groups of 8192-element shares, ragged).  Images
[2, 3, 64, 43] with a [1, 1, 64, 43] mask shared by the batch (n = 8256, two work-groups; odd width, so a 16-byte unit straddles rows and
channels).  The issue names [2, 3, 12, 43] for the image case, but 3 x 12 x 43 = 1548 is no multiple of 64, which the same issue makes
the entry refuse (asserted below, and in tests/test_masked_score_cabi_cpu.py): the height is raised to the next value that gives a
multiple of 64 with the same channels and width.

Bound per sum, the one of tests/test_hip_sample_score_fp64.py:  |kernel - reference| <= 2 n 2^-53 sum|term|,  u = 2^-53.
  The derivation there charges (n - 1) u to the kernel's summation, (log2 n + c) u to torch's and 2 u per term to either side.  The weight
  adds roundings to a term, none to the summation: the kernel forms fl(w d) and feeds it to a fused multiply-add (with fl(x - y): <= 3 u;
  the other sums take exact products into a fused multiply-add: 0), 1 - w rounds once more: <= 4 u; the reference forms fl(fl(w d) d) from
  fl(x - y) and fl(1 - w): <= 5 u.  Together (n - 1 + 4) u + (log2 n + c + 5) u <= 2 n u for every n >= 64 (n = 64: 67 + 11 + c <= 128
  for c <= 50).  The constant stands as it is.

Also asserted: m = 1 everywhere gives region 0's last four sums equal to ``ops.sample_score`` bit for bit, sum w = n and region 1 exactly 0;
two calls are bit-identical, slots included, and the slots added in index order are the result; mutated references (the 2 x 2 patch index
transposed in the ``% 4`` map, the regions swapped, the mask's batch index ignored) each miss the bound, after the CPU side has shown that
each moves the reference by more than twice the bound; guard elements around ``out`` and ``ws`` stay untouched; refused calls leave ``out``
as it was.
"""
import functools

import pytest
import torch

import masked_score_ref as MR

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GUARD = 64
#        operands           mask            work-groups per sample
CASES = {'N4': ((2, 4, 64), (2, 4, 4), 1), 'N130': ((2, 130, 64), (2, 130, 4), 2), 'N257': ((2, 257, 64), (2, 257, 4), 3),
         'image': ((2, 3, 64, 43), (1, 1, 64, 43), 2)}
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16}


@functools.lru_cache(maxsize=None)
def _case(name, dname, transform):
    """Inputs (CPU, the operand dtype), the fp64 reference and the mutated references of one case, computed once."""
    shape, mshape, parts = CASES[name]
    g = torch.Generator().manual_seed(11 + len(name) + 1000 * transform + sum(shape))
    scale = 2.0 if transform else 1.0
    b = torch.randn(shape, generator=g) * scale
    a = 0.8 * b + 0.6 * scale * torch.randn(shape, generator=g) + 0.05
    a, b = a.to(DTYPES[dname]).contiguous(), b.to(DTYPES[dname]).contiguous()
    mask = MR.random_mask(mshape, 5 + sum(mshape))
    assert 0 < (mask == 0).float().mean() < 0.5 and 0 < (mask == 1).float().mean() < 0.5 and ((mask > 0) & (mask < 1)).float().mean() > 0.5
    view, m3 = MR.view_of(a, mask)
    n = a[0].numel()
    ref, mag = MR.masked_sums(a, b, m3, view, bool(transform))
    muts = {'regions_swapped': MR.masked_sums(a, b, m3, view, bool(transform), swap_regions=True)[0]}
    if mshape[-1] == 4 and len(mshape) == 3:
        muts['ph_pw_swapped'] = MR.masked_sums(a, b, m3, view, bool(transform), swap_hw=True)[0]
    if mshape[0] > 1:
        muts['mask_batch_ignored'] = MR.masked_sums(a, b, m3, view, bool(transform), ignore_batch=True)[0]
    return dict(a=a, b=b, mask=mask, ref=ref, bound=2 * n * U * mag, muts=muts, n=n, parts=parts)


def _guarded(numel, sentinel=-768.0):
    buf = torch.full((numel + 2 * GUARD,), sentinel, dtype=torch.float64, device='cuda')
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(buf, numel, sentinel=-768.0):
    return bool((buf[:GUARD] == sentinel).all() and (buf[GUARD + numel:] == sentinel).all())


def _rows(name):
    """The samples a mutation must move: all of them, but sample 0 reads its own mask when the batch index is ignored."""
    return slice(1, None) if name == 'mask_batch_ignored' else slice(None)


@pytest.mark.parametrize('transform', [0, 1], ids=['latent', 'image'])
@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
@pytest.mark.parametrize('name', list(CASES))
def test_masked_sums_within_fp64_bound_reproducible_and_guarded(name, dname, transform):
    from arcflow_amd import _lib, ops
    c = _case(name, dname, transform)
    ref, bound, n, parts = c['ref'], c['bound'], c['n'], c['parts']
    B = ref.shape[0]
    for mut, r in c['muts'].items():           # CPU side first: every mutation moves some sum of every sample it can move by more than twice the bound
        moved = ((r - ref).abs() > 2 * bound).flatten(1).any(1)[_rows(mut)]
        print(f'{name} {dname} transform={transform} mutation {mut}: max move / bound {((r - ref).abs() / bound.clamp(min=1e-300)).max().item():.3e}')
        assert moved.all() and moved.numel() > 0, (mut, moved.tolist())
    need = _lib.load().afx_sample_score_masked_ws_bytes(B, n)
    assert need == B * parts * 80
    a, b, mask = c['a'].cuda(), c['b'].cuda(), c['mask'].cuda()
    outs, slots = [], []
    for _ in range(2):
        wbuf, ws = _guarded(need // 8)
        obuf, out = _guarded(B * 10)
        r = ops.sample_score_masked(a, b, mask, transform=bool(transform), out=out.view(B, 2, 5), ws=ws)
        torch.cuda.synchronize()
        assert r.data_ptr() == out.data_ptr() and r.shape == (B, 2, 5) and r.dtype == torch.float64
        assert _guards_intact(wbuf, need // 8) and _guards_intact(obuf, B * 10)
        outs.append(out.cpu().clone().view(B, 2, 5))
        slots.append(ws.cpu().clone())
    assert torch.equal(outs[1].view(torch.int64), outs[0].view(torch.int64)) and torch.equal(slots[1].view(torch.int64), slots[0].view(torch.int64))
    assert torch.equal(a.cpu(), c['a']) and torch.equal(b.cpu(), c['b']) and torch.equal(mask.cpu(), c['mask'])          # the operands are read only
    got = outs[0]
    err = (got - ref).abs()
    print(f'{name} {dname} transform={transform}: max err / bound {(err / bound).max().item():.3e}  sums[0] {got[0].tolist()}')
    assert torch.isfinite(got).all()
    assert (err <= bound).all(), (err / bound).tolist()
    s = slots[0].view(B, parts, 10)          # the slots hold the partial sums: added in index order they ARE the result, bit for bit
    acc = torch.zeros(B, 10, dtype=torch.float64)
    for w in range(parts):
        acc = acc + s[:, w]
    assert torch.equal(acc.view(torch.int64), got.view(B, 10).view(torch.int64))
    for mut, r in c['muts'].items():           # the kernel is outside every mutated reference's bound
        missed = ((got - r).abs() > bound).flatten(1).any(1)[_rows(mut)]
        assert missed.all(), (mut, ((got - r).abs() / bound.clamp(min=1e-300)).tolist())


@pytest.mark.parametrize('transform', [0, 1], ids=['latent', 'image'])
@pytest.mark.parametrize('dname', ['fp32', 'bf16'])
@pytest.mark.parametrize('name', list(CASES))
def test_a_mask_of_ones_is_the_unmasked_kernel_bit_for_bit(name, dname, transform):
    from arcflow_amd import ops
    c = _case(name, dname, transform)
    a, b = c['a'].cuda(), c['b'].cuda()
    ones = torch.ones(CASES[name][1], device='cuda')
    got = ops.sample_score_masked(a, b, ones, transform=bool(transform)).cpu()
    plain = ops.sample_score(a, b, transform=bool(transform)).cpu()
    assert torch.equal(got[:, 0, 1:].contiguous().view(torch.int64), plain.view(torch.int64))
    assert (got[:, 0, 0] == float(c['n'])).all() and (got[:, 1] == 0).all()
    zeros = ops.sample_score_masked(a, b, torch.zeros_like(ones), transform=bool(transform)).cpu()
    assert (zeros[:, 0] == 0).all() and torch.equal(zeros[:, 1, 1:].contiguous().view(torch.int64), plain.view(torch.int64)) and (zeros[:, 1, 0] == float(c['n'])).all()


def test_wrapper_allocates_broadcasts_and_refuses_wrong_operands():
    from arcflow_amd import _lib, ops
    c = _case('N130', 'bf16', 0)
    a, b, mask = c['a'].cuda(), c['b'].cuda(), c['mask'].cuda()
    assert ops.sample_score_masked_ws(2, 8320).numel() == 2 * 2 * 10 and ops.sample_score_masked_ws(2, 8320).dtype == torch.float64
    both = ops.sample_score_masked(a, b, mask).cpu()
    shared = ops.sample_score_masked(a, b, mask[:1].contiguous()).cpu()          # a mask batch of 1 is every sample's mask
    assert torch.equal(shared[0], both[0]) and not torch.equal(shared[1], both[1])
    assert torch.equal(shared[1], ops.sample_score_masked(a[1:].contiguous(), b[1:].contiguous(), mask[:1].contiguous()).cpu()[0])
    with pytest.raises(ValueError):
        ops.sample_score_masked(a, b.float(), mask)                       # mixed dtypes
    with pytest.raises(ValueError):
        ops.sample_score_masked(a.half(), b.half(), mask)                 # neither fp32 nor bf16
    with pytest.raises(ValueError):
        ops.sample_score_masked(a, b, mask.double())                      # the mask is fp32
    with pytest.raises(ValueError):
        ops.sample_score_masked(a, b, mask[:, :129].contiguous())         # another token count
    with pytest.raises(ValueError):
        ops.sample_score_masked(a, b, torch.ones(2, 130, 3, device='cuda'))          # Q = 3 does not divide 64
    with pytest.raises(_lib.ArcflowHipError, match='mask_batch'):
        ops.sample_score_masked(torch.cat([a, a[:1]]), torch.cat([b, b[:1]]), mask)          # 2 masks for 3 samples
    with pytest.raises(_lib.ArcflowHipError, match='multiple of 64'):
        ops.sample_score_masked(torch.zeros(2, 3, 12, 43, device='cuda'), torch.zeros(2, 3, 12, 43, device='cuda'), torch.ones(1, 1, 12, 43, device='cuda'))
    with pytest.raises(_lib.ArcflowHipError, match='workspace'):
        ops.sample_score_masked(a, b, mask, ws=torch.empty(39, dtype=torch.float64, device='cuda'))
    with pytest.raises(_lib.ArcflowHipError):
        ops.sample_score_masked(a.cpu(), b.cpu(), mask.cpu())


def test_every_guard_returns_its_error_without_launching():
    """Real device buffers with watched contents: a refused call leaves ``out`` and ``ws`` as they were (nothing was launched)."""
    from arcflow_amd import _lib, ops
    lib = _lib.load()
    B, N = 2, 130
    a = torch.zeros(B, N, 64, device='cuda')
    mask = torch.ones(B, N, 4, device='cuda')
    out = torch.full((B, 2, 5), -3.0, dtype=torch.float64, device='cuda')
    ws = torch.full((B * 2 * 10,), -5.0, dtype=torch.float64, device='cuda')
    P = lambda t, off=0: t.data_ptr() + off          # noqa: E731
    ok = dict(a=P(a), b=P(a), mask=P(mask), dtype=_lib.AFX_DT_F32, transform=0, out=P(out), ws=P(ws), ws_bytes=B * 2 * 80, batch=B, mask_batch=B,
              G=1, P=N, R=64, Q=4)
    defects = [dict(a=None), dict(b=None), dict(mask=None), dict(out=None), dict(ws=None), dict(dtype=_lib.AFX_DT_FP8), dict(dtype=0), dict(transform=2),
               dict(P=3, R=32), dict(Q=3), dict(Q=0), dict(mask_batch=3), dict(mask_batch=0), dict(ws_bytes=B * 2 * 80 - 1), dict(a=P(a, 8)),
               dict(mask=P(mask, 2)), dict(out=P(out, 4)), dict(ws=P(ws, 4)), dict(batch=-1), dict(G=1 << 20, P=1 << 10)]
    for d in defects:
        k = dict(ok, **d)
        rc = lib.afx_sample_score_masked(k['a'], k['b'], k['mask'], k['dtype'], k['transform'], k['out'], k['ws'], k['ws_bytes'], k['batch'],
                                         k['mask_batch'], k['G'], k['P'], k['R'], k['Q'], None)
        assert rc == _lib.AFX_E_INVALID and b'afx_sample_score_masked' in lib.afx_last_error(), (d, rc, lib.afx_last_error())
    torch.cuda.synchronize()
    assert (out == -3.0).all() and (ws == -5.0).all()
    got = ops.sample_score_masked(a, a, mask).cpu()          # and the good call runs
    assert (got[:, 0, 0] == N * 64).all() and (got[:, :, 1:] == 0).all() and (got[:, 1, 0] == 0).all()
