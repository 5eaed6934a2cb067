"""afx_image_paste per byte against the fp64 reference of tests/image_paste_ref.py, which consumes the same fp32 tables.

A byte q of the result is admissible iff rne(255 clamp(r - E)) <= q <= rne(255 clamp(r + E)) with the reference's value r and bound E (derived
in the reference's docstring from the resampling bound, its propagation through 0.5 v + 0.5 and the blend, and the blend's own fp32
roundings; no constant is fitted).  tests/test_image_paste_cpu.py shows, on these very inputs, that at most 1 % of the elements admit two
bytes and none three, and that each of the seven mutants is disjoint from the truth somewhere.  EVERY byte must be admissible; outside the
window, and for an all-zero mask, the result must be the source bit for bit.

Inputs (image_paste_ref.inputs): B = 2, sources uniform over all 256 byte values, img uniform in [-1.2, 1.2] so the clamp acts, masks with
exact 0 and 1 regions and a ramp between.  Cases (image_paste_ref.CASES): up, down and mixed windows, a source wider than a work-group
(two, the second partly filled), windows on the borders, a 1 x 1 window, and 66000 rows of dst, more than the grid's 65535, whose window
lies in the rows the row loop's second trip takes."""
import ctypes as C

import numpy as np
import pytest
import torch

import image_paste_ref as P

pytestmark = pytest.mark.gpu


def _tables(case):
    _, window, (h, w) = P.CASES[case]
    return P.tables(h, w, window, 'lanczos3'), P.tables(h, w, window, 'triangle')


def _run(case, img, mask, src):
    from arcflow_amd import ops
    _, window, _ = P.CASES[case]
    out = ops.image_paste(torch.from_numpy(img).cuda(), None if mask is None else torch.from_numpy(mask).cuda(), torch.from_numpy(src).cuda(), window)
    torch.cuda.synchronize()
    return out.cpu().numpy()


_cache = {}


def _case(case):
    """(inputs, the kernel's bytes, (r, E)) of a case with its mask: computed once, shared by the tests, never modified."""
    if case not in _cache:
        img, mask, src = P.inputs(case)
        got = _run(case, img, mask, src)
        itab, mtab = _tables(case)
        _, window, _ = P.CASES[case]
        r, E = P.paste(img, mask, src, window, *itab, *mtab)
        for a in (img, mask, src, got, r, E):
            a.setflags(write=False)
        _cache[case] = ((img, mask, src), got, (r, E))
    return _cache[case]


def _check(got, r, E, what):
    lo, hi = P.admissible(r, E)
    bad = (got < lo) | (got > hi)
    two = float((hi > lo).mean())
    print(f'{what}: {int(bad.sum())} of {bad.size} bytes inadmissible; {100 * two:.3f} % of the elements admit two bytes; max 255 E = {255 * E.max():.2e}')
    assert got.dtype == np.uint8 and got.shape == r.shape
    assert not bad.any(), what


@pytest.mark.parametrize('case', list(P.CASES))
def test_every_byte_is_admissible(case):
    (img, mask, src), got, (r, E) = _case(case)
    _check(got, r, E, f'{case} masked')
    _, (x0, y0, x1, y1), _ = P.CASES[case]
    outside = np.ones(src.shape, dtype=bool)
    outside[:, y0:y1, x0:x1] = False
    assert np.array_equal(got[outside], src[outside])                                  # outside the window: the source, bit for bit
    inside = got[:, y0:y1, x0:x1]
    if case != 'one_pixel':
        assert (inside != src[:, y0:y1, x0:x1]).any()                                  # ... and something was pasted


@pytest.mark.parametrize('case', ['mixed', 'down', 'two_groups', 'one_pixel'])
def test_unmasked_and_shared_mask(case):
    img, mask, src = P.inputs(case)
    itab, mtab = _tables(case)
    _, window, _ = P.CASES[case]
    _check(_run(case, img, None, src), *P.paste(img, None, src, window, *itab), f'{case} mask=None')
    one = np.ascontiguousarray(mask[1:])                                               # a batch of 1 is shared by both images
    _check(_run(case, img, one, src), *P.paste(img, one, src, window, *itab, *mtab), f'{case} shared mask')


def test_zero_mask_and_nan_image_return_the_source():
    for case in ('mixed', 'border', 'two_groups'):
        img, mask, src = P.inputs(case)
        got = _run(case, np.full_like(img, np.nan), np.zeros_like(mask), src)
        assert np.array_equal(got, src), case


def test_all_byte_values_pass_an_identity_window_bit_exactly():
    """mask = None, the window = the whole 16 x 16 source = the call's size, img = 2 b / 255 - 1 (fp32) over all 256 values: dst == b."""
    from arcflow_amd import ops
    b = torch.stack([torch.arange(256), torch.arange(255, -1, -1), (torch.arange(256) * 7) % 256]).view(1, 3, 16, 16)
    img = (b.float() * 2.0 / 255.0 - 1.0).contiguous()
    src = torch.full((1, 16, 16, 3), 99, dtype=torch.uint8)
    got = ops.image_paste(img.cuda(), None, src.cuda(), (0, 0, 16, 16)).cpu()
    assert torch.equal(got, b.permute(0, 2, 3, 1).to(torch.uint8))
    ones = torch.ones(1, 1, 16, 16)                                                     # ... and the same through an all-ones mask
    assert torch.equal(ops.image_paste(img.cuda(), ones.cuda(), src.cuda(), (0, 0, 16, 16)).cpu(), got)


def _raw(lib, img, mask, src, dst, ws, window, itab, mtab):
    from arcflow_amd import _lib
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    B, _, h, w = img.shape
    H, W = src.shape[1:3]
    x0, y0, x1, y1 = window
    tabs = [a for tab in itab + mtab for a in (p(tab[0]), p(tab[1]), p(tab[2]), tab[2].shape[1])]
    _lib.check(lib.afx_image_paste(p(img), p(mask), mask.shape[0], p(src), p(dst), B, h, w, H, W, x0, y0, x1, y1, x1 - x0, y1 - y0, *tabs,
                                   p(ws), ws.numel() * 4, None))
    torch.cuda.synchronize()


def test_guard_bands_inputs_and_determinism():
    from arcflow_amd import _lib, ops
    lib = _lib.load()
    case = 'mixed'
    (H, W), window, (h, w) = P.CASES[case]
    (img, mask, src), first, _ = _case(case)
    img, mask, src = (torch.from_numpy(a.copy()).cuda() for a in (img, mask, src))
    x0, y0, x1, y1 = window
    itab = [tuple(t.cuda() for t in ops.resample_tables(n, m, 'lanczos3')) for n, m in ((w, x1 - x0), (h, y1 - y0))]
    mtab = [tuple(t.cuda() for t in ops.resample_tables(n, m, 'triangle')) for n, m in ((w, x1 - x0), (h, y1 - y0))]
    operands = [img, mask, src] + [t for tab in itab + mtab for t in tab]
    keep = [t.clone() for t in operands]
    G, n = 4096, 2 * H * W * 3
    nws = lib.afx_image_paste_ws_bytes(2, 2, h, x1 - x0) // 4
    assert nws == (3 * 2 + 2) * h * (x1 - x0)
    outs = []
    for _ in range(2):
        buf = torch.full((G + n + G,), 0xA5, dtype=torch.uint8, device='cuda')
        wbuf = torch.full((G + nws + G,), float('nan'), device='cuda')                 # the workspace starts as NaN: nothing stale can be read as data
        wbuf[:G], wbuf[G + nws:] = -9.0, -9.0
        _raw(lib, img, mask, src, buf[G:G + n], wbuf[G:G + nws], window, itab, mtab)
        assert (buf[:G] == 0xA5).all() and (buf[G + n:] == 0xA5).all() and (wbuf[:G] == -9).all() and (wbuf[G + nws:] == -9).all()
        assert torch.isfinite(wbuf[G:G + nws]).all()                                   # every workspace element was written
        outs.append(buf[G:G + n].clone().view(2, H, W, 3))
    assert torch.equal(outs[0], outs[1]) and np.array_equal(outs[0].cpu().numpy(), first)
    for a, b in zip(keep, operands):
        assert torch.equal(a, b)
    # every byte of dst is written: two different fills give the same result
    buf = torch.zeros(n, dtype=torch.uint8, device='cuda')
    _raw(lib, img, mask, src, buf, torch.full((nws,), float('nan'), device='cuda'), window, itab, mtab)
    assert torch.equal(buf.view(2, H, W, 3), outs[0])
    out = torch.empty(2, H, W, 3, dtype=torch.uint8, device='cuda')
    assert ops.image_paste(img, mask, src, window, out=out) is out and torch.equal(out, outs[0])


@pytest.mark.parametrize('mutant', P.MUTANTS)
def test_mutated_references_are_rejected(mutant):
    """The kernel's bytes are admissible under the true reference (test_every_byte_is_admissible) and must NOT be under a mutated one."""
    rejected = {}
    for case in ('mixed', 'up4', 'down', 'two_groups', 'border'):
        (H, W), (x0, y0, x1, y1), (h, w) = P.CASES[case]
        if (mutant == 'swap' and h != w) or (mutant == 'shift' and (x1 == W or y1 == H)):
            continue
        (img, mask, src), got, (r, E) = _case(case)
        itab, mtab = _tables(case)
        if mutant == 'trunc':
            lo, hi = P.admissible(r, E, trunc=True)
        else:
            lo, hi = P.admissible(*P.paste(img, mask, src, (x0, y0, x1, y1), *itab, *mtab, mutant=mutant))
        rejected[case] = float(((got < lo) | (got > hi)).mean())
    print(mutant, {k: f'{100 * v:.1f} %' for k, v in rejected.items()})
    assert rejected and min(rejected.values()) > 0.0, mutant


def test_wrapper_argument_errors():
    from arcflow_amd import ops
    img, src = torch.zeros(1, 3, 8, 8, device='cuda'), torch.zeros(1, 16, 16, 3, dtype=torch.uint8, device='cuda')
    mask = torch.zeros(1, 1, 8, 8, device='cuda')
    for bad in (img[0], img.double(), img.half(), img[:, :2], img.permute(0, 1, 3, 2)[..., ::2], torch.zeros(1, 3, 0, 8, device='cuda')):
        with pytest.raises(ValueError, match='img'):
            ops.image_paste(bad, None, src, (0, 0, 8, 8))
    for bad in (src[0], src.float(), src.permute(0, 3, 1, 2), src.expand(2, -1, -1, -1), src[:, ::2]):
        with pytest.raises(ValueError, match='src_u8'):
            ops.image_paste(img, None, bad, (0, 0, 8, 8))
    for bad in (mask[0], mask.double(), torch.zeros(1, 1, 8, 9, device='cuda'), torch.zeros(3, 1, 8, 8, device='cuda'), torch.zeros(1, 3, 8, 8, device='cuda')):
        with pytest.raises(ValueError, match='mask'):
            ops.image_paste(img, bad, src, (0, 0, 8, 8))
    for bad in ((0, 0, 17, 8), (-1, 0, 8, 8), (4, 4, 4, 8), (0, 9, 8, 8), (0.5, 0, 8, 8)):
        with pytest.raises(ValueError, match='window'):
            ops.image_paste(img, None, src, bad)
    with pytest.raises(ValueError, match='out'):
        ops.image_paste(img, None, src, (0, 0, 8, 8), out=torch.zeros(1, 16, 16, 3, device='cuda'))
