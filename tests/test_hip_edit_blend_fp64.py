"""``afx_edit_blend`` (the blend of image-to-image and inpainting) against fp64, element by element, on the inputs of tests/edit_ref.py:
B = 2 samples x 15 tokens x 64 channels (960 elements per sample, 240 chunks of 8: one work-group walks them in a single pass, so
``max_blocks=1`` and the default grid are both one block here -- the capped run is repeated on 3 x 175 tokens, 4200 chunks, where one block
of 256 lanes takes 17 passes), per-sample sigmas, a soft mask that differs across the four sub-pixels and across the samples.

Bound (derived in tests/edit_ref.py from six fp32 roundings; not measured): |err| <= 8 * 2^-24 * (|x| + |x0| + |noise|) per element.
The exactness cases are bit-equalities: a binary mask returns x where m = 1 and the no-mask call's ``known`` where m = 0, sigma_to = 1
returns noise, sigma_to = 0 without noise returns x0, and mask = NULL with x = NULL equals an all-zero mask.  The bf16 copy is the
round-to-nearest-even of the returned fp32 bit for bit, on inputs that include fp32 values exactly halfway between two bf16 neighbours
(routed through m = 1).  Outputs are written into guarded buffers; in place (x_out is x) equals out of place; inputs are left alone.
Every mutant of tests/edit_ref.py must fail the comparison that the kernel passes."""
import functools

import numpy as np
import pytest
import torch

import edit_ref as ER

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = -768.0


@functools.lru_cache(maxsize=None)
def _case():
    c = ER.make_case()
    dev = {k: torch.from_numpy(v).cuda() for k, v in c.items()}
    return c, dev


def _guarded(shape, dtype):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device='cuda')
    return buf, buf[GUARD:GUARD + n].view(shape)


def _intact(buf):
    return bool((buf[:GUARD] == SENT).all() and (buf[-GUARD:] == SENT).all())


def _run(x, x0, noise, mask, sigma_to, max_blocks=0, inplace=False, bf16=True):
    """One guarded launch -> (fp32 numpy, bf16 bits numpy or None)."""
    from arcflow_amd import ops
    fbuf, fout = _guarded(x0.shape, torch.float32)
    hbuf, hout = _guarded(x0.shape, torch.bfloat16)
    keep = [None if t is None else t.clone() for t in (x, x0, noise, mask, sigma_to)]
    if inplace:
        fout.copy_(x)
        x = fout
    o, o16 = ops.edit_blend(x, x0, noise, mask, sigma_to, out=fout, out_bf16=hout if bf16 else False, max_blocks=max_blocks)
    torch.cuda.synchronize()
    assert o.data_ptr() == fout.data_ptr() and (o16 is None if not bf16 else o16.data_ptr() == hout.data_ptr())
    assert _intact(fbuf) and _intact(hbuf)
    if not bf16:
        assert bool((hout == SENT).all())
    for t, k in zip((None if inplace else x, x0, noise, mask, sigma_to), keep):
        assert t is None or torch.equal(t, k)                                          # the inputs are left alone
    return fout.cpu().numpy().copy(), (hout.cpu().view(torch.int16).numpy().view(np.uint16).copy() if bf16 else None)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize('max_blocks', [1, 0], ids=['one_block', 'default_grid'])
def test_soft_mask_within_fp32_rounding_of_fp64_and_mutants_rejected(max_blocks):
    c, d = _case()
    bound = ER.blend_bound(c['x'], c['x0'], c['noise'])
    ref = ER.blend_ref(c['x'], c['x0'], c['noise'], c['mask'], c['sigma_to'])
    got, got16 = _run(d['x'], d['x0'], d['noise'], d['mask'], d['sigma_to'], max_blocks)
    err = np.abs(got.astype(np.float64) - ref)
    print(f'max_blocks={max_blocks}: max err / bound {(err / bound).max():.3f}  (max |err| {err.max():.3e})')
    assert np.isfinite(got).all() and (err <= bound).all(), (err / bound).max()
    assert np.array_equal(got16, ER.bf16_bits(got))                                    # bf16 copy = RNE of the kernel's own fp32
    assert not np.array_equal(got16, ER.bf16_bits(got, trunc=True))
    # the ties: token 0 of sample 0 has m = 1, so x comes back bit for bit and its bf16 copy rounds to even
    assert np.array_equal(_bits(got[0, 0]), _bits(c['x'][0, 0]))
    assert np.array_equal(got16[0, 0, :8], ER.bf16_bits(ER.tie_values()))
    assert (got16[0, 0, :8] != ER.bf16_bits(ER.tie_values(), trunc=True)).tolist() == [False, True, False, True, True, False, True, False]
    # in place, and without the bf16 copy: the same fp32
    again, again16 = _run(d['x'], d['x0'], d['noise'], d['mask'], d['sigma_to'], max_blocks, inplace=True)
    assert np.array_equal(_bits(again), _bits(got)) and np.array_equal(again16, got16)
    assert np.array_equal(_bits(_run(d['x'], d['x0'], d['noise'], d['mask'], d['sigma_to'], max_blocks, bf16=False)[0]), _bits(got))
    # the call without noise (sigma_to left at 0.7 / 0.35, so the missing term is visible) and the mutants
    ref_nn = ER.blend_ref(c['x'], c['x0'], c['noise'], c['mask'], c['sigma_to'], noise_is_null=True)
    got_nn, _ = _run(d['x'], d['x0'], None, d['mask'], d['sigma_to'], max_blocks)
    assert (np.abs(got_nn.astype(np.float64) - ref_nn) <= bound).all()
    for m in ER.MUTANTS:
        null = m == 'keep_noise'
        wrong = ER.blend_ref(c['x'], c['x0'], c['noise'], c['mask'], c['sigma_to'], mutate=m, noise_is_null=null)
        frac = (np.abs((got_nn if null else got).astype(np.float64) - wrong) > bound).mean()
        assert frac >= 0.01, (m, frac)


def test_capped_grid_walks_many_passes():
    """3 x 175 tokens = 4200 chunks on ONE block of 256 lanes: 17 grid-stride passes, the last one ragged; equal to the default grid."""
    g = np.random.default_rng(5)
    shape = (3, 175, 64)
    x, x0, noise = (torch.from_numpy(g.standard_normal(shape).astype(np.float32)).cuda() for _ in range(3))
    mask = torch.from_numpy(g.random((3, 175, 4)).astype(np.float32)).cuda()
    sig = torch.tensor([0.9, 0.5, 0.1], device='cuda')
    one, one16 = _run(x, x0, noise, mask, sig, max_blocks=1)
    full, full16 = _run(x, x0, noise, mask, sig, max_blocks=0)
    assert np.array_equal(_bits(one), _bits(full)) and np.array_equal(one16, full16)
    ref = ER.blend_ref(x.cpu().numpy(), x0.cpu().numpy(), noise.cpu().numpy(), mask.cpu().numpy(), sig.cpu().numpy())
    assert (np.abs(one.astype(np.float64) - ref) <= ER.blend_bound(x.cpu().numpy(), x0.cpu().numpy(), noise.cpu().numpy())).all()
    wrong = ER.blend_ref(x.cpu().numpy(), x0.cpu().numpy(), noise.cpu().numpy(), mask.cpu().numpy(), sig.cpu().numpy(), mutate='sigma0')
    assert (np.abs(one.astype(np.float64) - wrong) > ER.blend_bound(x.cpu().numpy(), x0.cpu().numpy(), noise.cpu().numpy())).mean() > 0.3


@pytest.mark.parametrize('max_blocks', [1, 0], ids=['one_block', 'default_grid'])
def test_exactness_cases_are_bit_exact(max_blocks):
    c, d = _case()
    known, known16 = _run(None, d['x0'], d['noise'], None, d['sigma_to'], max_blocks)               # mask = NULL, x = NULL
    assert (np.abs(known.astype(np.float64) - ER.blend_ref(None, c['x0'], c['noise'], None, c['sigma_to'])) <= ER.blend_bound(None, c['x0'], c['noise'])).all()
    zero, zero16 = _run(d['x'], d['x0'], d['noise'], torch.zeros_like(d['mask']), d['sigma_to'], max_blocks)
    assert np.array_equal(_bits(zero), _bits(known)) and np.array_equal(zero16, known16)
    # binary mask, different per sub-pixel and per sample
    g = np.random.default_rng(11)
    binary = (g.random(c['mask'].shape) > 0.5).astype(np.float32)
    assert 0.3 < binary.mean() < 0.7 and not np.array_equal(binary[0], binary[1]) and (binary.min(-1) != binary.max(-1)).any()
    got, got16 = _run(d['x'], d['x0'], d['noise'], torch.from_numpy(binary).cuda(), d['sigma_to'], max_blocks)
    sel = binary[:, :, np.arange(64) & 3] == 1.0
    assert np.array_equal(_bits(got)[sel], _bits(c['x'])[sel]) and np.array_equal(_bits(got)[~sel], _bits(known)[~sel])
    assert np.array_equal(got16, ER.bf16_bits(got))
    # sigma_to = 1 returns the noise, sigma_to = 0 without noise returns x0
    ones, zeros = torch.ones(ER.B, device='cuda'), torch.zeros(ER.B, device='cuda')
    assert np.array_equal(_bits(_run(None, d['x0'], d['noise'], None, ones, max_blocks)[0]), _bits(c['noise']))
    assert np.array_equal(_bits(_run(None, d['x0'], None, None, zeros, max_blocks)[0]), _bits(c['x0']))
    # ... and under a mask: the last step of an inpainting call keeps x0 exactly where m = 0
    last, _ = _run(d['x'], d['x0'], None, torch.from_numpy(binary).cuda(), zeros, max_blocks)
    assert np.array_equal(_bits(last)[~sel], _bits(c['x0'])[~sel]) and np.array_equal(_bits(last)[sel], _bits(c['x'])[sel])


def test_wrapper_allocates_and_refuses_wrong_operands():
    from arcflow_amd import _lib, ops
    c, d = _case()
    o, o16 = ops.edit_blend(d['x'], d['x0'], d['noise'], d['mask'], d['sigma_to'])
    ref = ER.blend_ref(c['x'], c['x0'], c['noise'], c['mask'], c['sigma_to'])
    assert (np.abs(o.cpu().numpy().astype(np.float64) - ref) <= ER.blend_bound(c['x'], c['x0'], c['noise'])).all()
    assert o16.dtype == torch.bfloat16 and o16.shape == o.shape and torch.equal(o16, o.bfloat16())
    with pytest.raises(ValueError):
        ops.edit_blend(d['x'], d['x0'].bfloat16(), d['noise'], d['mask'], d['sigma_to'])            # no cast
    with pytest.raises(ValueError):
        ops.edit_blend(d['x'], d['x0'], d['noise'], d['mask'][:, :, :1].expand(-1, -1, 4), d['sigma_to'])      # no copy of a strided mask
    with pytest.raises(ValueError):
        ops.edit_blend(None, d['x0'], d['noise'], d['mask'], d['sigma_to'])                       # x is required with a mask
    with pytest.raises(_lib.ArcflowHipError):
        ops.edit_blend(None, d['x0'][:, :, :32].contiguous(), None, None, d['sigma_to'])          # ch = 32
    with pytest.raises(_lib.ArcflowHipError):
        ops.edit_blend(d['x'], d['x0'], d['noise'], d['mask'], d['sigma_to'], out=d['x0'])         # the output over an input
