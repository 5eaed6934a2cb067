"""afx_tiles_cut against torch slicing (bit equality) and afx_tiles_merge per byte against the fp64 reference of tests/tiles_ref.py, which
consumes the same fp32 tables (``schedule.tile_plan``).

A byte q of the merge is admissible iff rne(255 clamp(r - E)) <= q <= rne(255 clamp(r + E)) with the reference's value r and bound E (derived
in the reference's docstring from the fp32 roundings of the formula; no constant is fitted).  tests/test_tiles_ref_cpu.py shows, on these
very inputs, that at most 1 % of the elements admit two bytes and none three, and that each of six mutants leaves the admissible set.
EVERY byte must be admissible.  Inputs (tiles_ref.inputs): tiles uniform in [-1.2, 1.2) so the clamp acts.  Cases (tiles_ref.CASES):
2 x 2 and 3 x 4 tiles (a three-tile overlap), non-square tiles, one tile, overlap 0, a canvas wider than one work-group's strip, and
66000 rows, more than the grid's 65535.  Exact properties: a pixel in one tile is rint(255 clamp(fma(0.5, v, 0.5))), a cut-then-merge round
trip of a uint8 photo returns its bytes, two runs give equal bits, guard bytes stay.  On the parent commit every test here fails:
``ops.tiles_cut`` and ``ops.tiles_merge`` do not exist."""
import ctypes as C

import numpy as np
import pytest
import torch

import tiles_ref as T

pytestmark = pytest.mark.gpu

_cache = {}


def _case(case):
    """(plan, tiles, the kernel's bytes, (r, E)) of a case: computed once, shared by the tests, never modified."""
    if case not in _cache:
        from arcflow_amd import ops
        plan, tiles = T.plan_of(case), T.inputs(case)
        got = ops.tiles_merge(torch.from_numpy(tiles).cuda(), plan)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        r, E = T.merge(tiles, plan)
        for a in (tiles, got, r, E):
            a.setflags(write=False)
        _cache[case] = (plan, tiles, got, (r, E))
    return _cache[case]


@pytest.mark.parametrize('case', list(T.CASES))
def test_cut_is_torch_slicing(case):
    from arcflow_amd import ops
    plan = T.plan_of(case)
    g = torch.Generator().manual_seed(5)
    canvas = torch.randn(3, plan.H, plan.W, generator=g)
    canvas.view(torch.int32)[0, 0, :4] = torch.tensor([0x7fc00001, -2147483647, 1, -2147483648], dtype=torch.int32)      # NaN payload, -denormal, denormal, -0: bits pass
    dev = canvas.cuda()
    got = ops.tiles_cut(dev, plan)
    want = torch.stack([dev[:, y:y + plan.th, x:x + plan.tw] for y in plan.oy.tolist() for x in plan.ox.tolist()])
    assert got.shape == (plan.T, 3, plan.th, plan.tw) and got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32))
    assert torch.equal(ops.tiles_cut(dev[None], plan).view(torch.int32), got.view(torch.int32))             # [1, 3, H, W] is taken too
    assert torch.equal(dev.cpu().view(torch.int32), canvas.view(torch.int32))


def test_cut_aligned_and_unaligned_sources_agree():
    """W = 64 with origins 0 and 32 takes the 16-byte loads on every row; the same canvas one float further into its allocation takes the 4-byte ones."""
    from arcflow_amd import ops, schedule
    plan = schedule.tile_plan(48, 64, 32, 0)
    assert plan.ox.tolist() == [0, 32] and plan.oy.tolist() == [0, 16]
    buf = torch.randn(1 + 3 * 48 * 64, device='cuda')
    shifted = buf[1:].view(3, 48, 64)
    aligned = shifted.clone()
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
    a, b = ops.tiles_cut(aligned, plan), ops.tiles_cut(shifted, plan)
    assert torch.equal(a, b) and torch.equal(a[3], aligned[:, 16:48, 32:64])


@pytest.mark.parametrize('case', list(T.CASES))
def test_every_byte_is_admissible(case):
    plan, tiles, got, (r, E) = _case(case)
    lo, hi = T.admissible(r, E)
    bad = (got < lo) | (got > hi)
    print(f'{case}: {int(bad.sum())} of {bad.size} bytes inadmissible; {100 * float((hi > lo).mean()):.4f} % of the elements admit two bytes; '
          f'max 255 E = {255 * E.max():.2e}')
    assert got.dtype == np.uint8 and got.shape == (plan.H, plan.W, 3)
    assert not bad.any(), case
    assert got.min() == 0 and got.max() == 255


@pytest.mark.parametrize('case', ['two_by_two', 'three_by_four', 'one_tile', 'no_overlap', 'many_rows'])
def test_a_pixel_in_one_tile_is_that_tile_exactly(case):
    """Where both counts are 1 the weights are exactly 1.0f: the byte is rint(255 clamp(fma(0.5, v, 0.5))) in fp32, bit for bit."""
    plan, tiles, got, _ = _case(case)
    (sy, cy, _), (sx, cx, _) = plan.y, plan.x
    one = (cy == 1)[:, None] & (cx == 1)[None, :]
    assert one.any()
    Y, X = np.nonzero(one)
    iy, ix = sy[Y], sx[X]
    v = tiles[iy * plan.kx + ix, :, Y - plan.oy[iy], X - plan.ox[ix]]                    # [n, 3] fp32
    p = (v.astype(np.float64) * 0.5 + 0.5).astype(np.float32)                           # one rounding, as the fma (0.5 v is exact)
    want = np.rint(np.float32(255.0) * np.clip(p, np.float32(0), np.float32(1))).astype(np.uint8)
    assert np.array_equal(got[Y, X], want)


@pytest.mark.parametrize('case', ['two_by_two', 'three_by_four', 'non_square', 'two_groups'])
def test_cut_then_merge_returns_the_photo(case):
    from arcflow_amd import ops
    plan = T.plan_of(case)
    g = torch.Generator().manual_seed(7)
    photo = torch.randint(0, 256, (plan.H, plan.W, 3), generator=g, dtype=torch.uint8)
    photo[0, :256 if plan.W >= 256 else plan.W, 0] = torch.arange(256, dtype=torch.uint8)[:plan.W]       # (every value where the row is long enough)
    canvas = (photo.cuda().permute(2, 0, 1).float() * 2.0 / 255.0 - 1.0).contiguous()
    back = ops.tiles_merge(ops.tiles_cut(canvas, plan), plan)
    assert torch.equal(back.cpu(), photo)


def test_all_byte_values_round_trip_through_an_overlap():
    from arcflow_amd import ops, schedule
    plan = schedule.tile_plan(48, 48, 32, 16)                                           # tiles at 0 and 16 on both axes: the centre lies in four
    b = (torch.arange(48 * 48 * 3) % 256).to(torch.uint8).view(48, 48, 3)
    canvas = (b.cuda().permute(2, 0, 1).float() * 2.0 / 255.0 - 1.0).contiguous()
    assert torch.equal(ops.tiles_merge(ops.tiles_cut(canvas, plan), plan).cpu(), b)


def _raw_merge(lib, stack, plan, dev, out, **over):
    """The C entry itself on the device plan ``dev`` = ops._device_plan(...); ``over`` replaces named arguments."""
    p = lambda t: None if t is None else (t if isinstance(t, int) else C.c_void_p(t.data_ptr()))
    _, oy, ox, ytab, xtab = dev
    a = dict(tiles=stack, T=plan.T, th=plan.th, tw=plan.tw, oy=oy, ky=plan.ky, ox=ox, kx=plan.kx, y_start=ytab[0], y_count=ytab[1], y_w=ytab[2],
             y_taps=ytab[2].shape[1], x_start=xtab[0], x_count=xtab[1], x_w=xtab[2], x_taps=xtab[2].shape[1], dst=out, H=plan.H, W=plan.W)
    a.update(over)
    ptrs = ('tiles', 'oy', 'ox', 'y_start', 'y_count', 'y_w', 'x_start', 'x_count', 'x_w', 'dst')
    return lib.afx_tiles_merge(*[p(a[k]) if k in ptrs else a[k] for k in a], None)


def test_guard_bytes_determinism_and_operands():
    from arcflow_amd import _lib, ops
    lib = _lib.load()
    case = 'three_by_four'
    plan, tiles, first, _ = _case(case)
    tiles = torch.from_numpy(tiles.copy()).cuda()
    dev = ops._device_plan(plan.H, plan.W, plan.tile, plan.overlap, str(tiles.device))
    operands = [tiles, dev[1], dev[2], *dev[3], *dev[4]]
    keep = [t.clone() for t in operands]
    G, n = 4096, plan.H * plan.W * 3
    outs = []
    for fill in (0xA5, 0x00):                                                           # every byte of dst is written: two fills, one result
        buf = torch.full((G + n + G,), fill, dtype=torch.uint8, device='cuda')
        _lib.check(_raw_merge(lib, tiles, plan, dev, buf[G:G + n]))
        torch.cuda.synchronize()
        assert (buf[:G] == fill).all() and (buf[G + n:] == fill).all()
        outs.append(buf[G:G + n].clone().view(plan.H, plan.W, 3))
    assert torch.equal(outs[0], outs[1]) and np.array_equal(outs[0].cpu().numpy(), first)
    for a, b in zip(keep, operands):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    out = torch.empty(plan.H, plan.W, 3, dtype=torch.uint8, device='cuda')
    assert ops.tiles_merge(tiles, plan, out=out) is out and torch.equal(out, outs[0])
    # the cut: guard floats around the stack stay
    canvas = torch.randn(3, plan.H, plan.W, device='cuda')
    nt = plan.T * 3 * plan.th * plan.tw
    fbuf = torch.full((G + nt + G,), -9.0, device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(lib.afx_tiles_cut(p(canvas), plan.H, plan.W, p(dev[1]), plan.ky, p(dev[2]), plan.kx, plan.th, plan.tw, p(fbuf[G:]), None))
    torch.cuda.synchronize()
    assert (fbuf[:G] == -9).all() and (fbuf[G + nt:] == -9).all()
    assert torch.equal(fbuf[G:G + nt].view(plan.T, 3, plan.th, plan.tw), ops.tiles_cut(canvas, plan))


def test_bad_arguments_are_refused():
    from arcflow_amd import _lib, ops, schedule
    lib = _lib.load()
    plan = T.plan_of('two_by_two')
    tiles = torch.zeros(plan.T, 3, plan.th, plan.tw, device='cuda')
    dev = ops._device_plan(plan.H, plan.W, plan.tile, plan.overlap, str(tiles.device))
    dst = torch.full((plan.H, plan.W, 3), 7, dtype=torch.uint8, device='cuda')
    assert _raw_merge(lib, tiles, plan, dev, dst) == _lib.AFX_OK
    bad = [dict(tiles=None), dict(dst=None), dict(oy=None), dict(x_w=None), dict(y_count=None),
           dict(tiles=tiles.data_ptr() + 2), dict(y_w=dev[3][2].data_ptr() + 1), dict(ox=dev[2].data_ptr() + 2),
           dict(T=plan.T + 1), dict(T=plan.T - 1), dict(ky=plan.ky + 1), dict(y_taps=5), dict(x_taps=0), dict(x_taps=_lib.AFX_TILE_MAX_TAPS + 1),
           dict(H=0), dict(W=0), dict(th=0), dict(tw=-16), dict(kx=0), dict(th=24), dict(th=plan.H + 8), dict(tw=64), dict(dst=tiles)]
    dst.fill_(7)
    for over in bad:
        assert _raw_merge(lib, tiles, plan, dev, dst, **over) == _lib.AFX_E_INVALID, over
        assert b'afx_tiles_merge' in lib.afx_last_error(), over
    torch.cuda.synchronize()
    assert (dst == 7).all()                                                             # refused before any launch
    p = lambda t: None if t is None else (t if isinstance(t, int) else C.c_void_p(t.data_ptr()))
    canvas = torch.zeros(3, plan.H, plan.W, device='cuda')
    cut = lambda **o: lib.afx_tiles_cut(*[p(v) if k in ('canvas', 'oy', 'ox', 'tiles') else v for k, v in dict(
        dict(canvas=canvas, H=plan.H, W=plan.W, oy=dev[1], ky=plan.ky, ox=dev[2], kx=plan.kx, th=plan.th, tw=plan.tw, tiles=tiles), **o).items()], None)
    assert cut() == _lib.AFX_OK
    for over in (dict(canvas=None), dict(tiles=None), dict(oy=None), dict(ox=None), dict(tiles=tiles.data_ptr() + 4), dict(canvas=canvas.data_ptr() + 2),
                 dict(H=0), dict(ky=0), dict(th=20), dict(tw=plan.W + 8), dict(th=plan.H + 8), dict(tiles=canvas)):
        assert cut(**over) == _lib.AFX_E_INVALID and b'afx_tiles_cut' in lib.afx_last_error(), over
    # the wrappers
    for badt in (tiles[0], tiles.double(), tiles[:, :2], tiles[:3], tiles.cpu()):
        with pytest.raises((ValueError, _lib.ArcflowHipError), match='tiles'):
            ops.tiles_merge(badt, plan)
    with pytest.raises(ValueError, match='out'):
        ops.tiles_merge(tiles, plan, out=torch.zeros(plan.H, plan.W, 3, device='cuda'))
    with pytest.raises(ValueError, match='plan'):
        ops.tiles_merge(tiles, (plan.H, plan.W))
    for badc in (canvas[:2], canvas.double(), canvas[:, :, :-1], canvas.permute(0, 2, 1)):
        with pytest.raises(ValueError, match='canvas'):
            ops.tiles_cut(badc, plan)
