"""afx_image_resample per element against the fp64 reference of tests/image_resample_ref.py, which consumes the same fp32 tables.

Bound, per element (derived in the reference's docstring):  2^-24 (taps_h + taps_v + 4) sum_v |w_v| sum_h |w_h| |x|  -- the rounding of two
fp32 dot products plus the uint8 conversion and the clamp.  No element is excluded anywhere: where the weighted magnitude is 0 the kernel
must return exactly the reference's value.

Inputs: uint8 sources are uniform draws over all 256 values; fp32 sources are uniform in [-0.2, 1.2], so the clamp acts on them (and on
Lanczos' overshoot).  Every output width is no multiple of the 256-lane work-group; one case is wider than a work-group (two blocks, the
second partly filled) and two cases have more than 65535 rows (the row-stride loop of either pass)."""
import ctypes as C

import numpy as np
import pytest
import torch

import image_resample_ref as R

pytestmark = pytest.mark.gpu

# (H_in, W_in), (H_out, W_out), box (left, upper, right, lower)
CASES = {
    'mixed': ((37, 53), (48, 32), None),
    'down6': ((100, 70), (16, 16), None),
    'up5': ((16, 16), (80, 48), None),
    'tiny_source': ((5, 7), (32, 16), None),                 # the source is smaller than the support
    'three_wide': ((200, 3), (16, 48), None),
    'box': ((37, 53), (24, 40), (3.25, 1.5, 47.75, 30.125)),
    'two_blocks': ((8, 700), (12, 300), None),              # W_out = 256 + 44
    'square_box': ((40, 40), (24, 24), (2.5, 0.0, 37.5, 40.0)),       # same sizes on both axes, different tables: the swap mutant
}


def _source(form, channels, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    if form == 'u8':
        return torch.randint(0, 256, (2, h, w, channels), generator=g, dtype=torch.uint8)
    return torch.rand(2, channels, h, w, generator=g) * 1.4 - 0.2


def _tables(case, name, **mutant):
    from arcflow_amd import ops
    (hi, wi), (ho, wo), box = CASES[case]
    bw, bh = (None, None) if box is None else ((box[0], box[2]), (box[1], box[3]))
    if mutant:
        return R.rule_table(hi, ho, name, bh, **mutant), R.rule_table(wi, wo, name, bw, **mutant)
    return tuple(t.numpy() for t in ops.resample_tables(hi, ho, name, bh)), tuple(t.numpy() for t in ops.resample_tables(wi, wo, name, bw))


def _run(case, src, name, clamp=True):
    from arcflow_amd import ops
    _, (ho, wo), box = CASES[case]
    out = ops.image_resample(src.cuda(), ho, wo, name, box, clamp)
    torch.cuda.synchronize()
    return out.cpu().double().numpy()


def _check(got, ref, bound, what):
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if (bound > 0).any() else 0.0
    print(f'{what}: max err {err.max():.3e}, max err / bound {ratio:.3f}, elements with bound 0: {(bound == 0).sum()}')
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert (err <= bound).all(), what


@pytest.fixture(scope='module')
def down6():
    """The 100 x 70 -> 16 x 16 Lanczos-3 result on the uint8 source: computed once, shared by the mutant tests, never modified."""
    src = _source('u8', 3, 100, 70, seed=11)
    got = _run('down6', src, 'lanczos3')
    got.setflags(write=False)
    return src.numpy(), got


@pytest.mark.parametrize('form,channels', [('u8', 3), ('u8', 1), ('f32', 3), ('f32', 1)])
@pytest.mark.parametrize('case', list(CASES))
def test_kernel_against_fp64(case, form, channels):
    (hi, wi), (ho, wo), _ = CASES[case]
    src = _source(form, channels, hi, wi, seed=len(case) + channels)
    for name in ('lanczos3', 'triangle'):
        tab_h, tab_w = _tables(case, name)
        for clamp in (True, False):
            ref, bound = R.resample(src.numpy(), tab_h, tab_w, clamp)
            _check(_run(case, src, name, clamp), ref, bound, f'{case} {form} C={channels} {name} clamp={clamp}')
        if form == 'f32' and name == 'lanczos3' and case in ('mixed', 'up5'):
            unclamped = R.resample(src.numpy(), tab_h, tab_w, False)[0]
            assert unclamped.min() < 0.0 and unclamped.max() > 1.0                    # the clamp had something to do


@pytest.mark.parametrize('which', ['h_rows', 'v_rows'])
def test_more_rows_than_the_grid(which):
    """More than 65535 rows in one pass: the rows past the grid's y extent are taken by the row-stride loop.  h_rows: 2 x 3 planes of 11000
    source rows (66000 rows in the horizontal pass); the box keeps the LAST 100 rows of every plane, so plane 5's (rows 65900 .. 65999) are
    computed by the loop's second trip.  v_rows: 2 x 3 planes of 11000 output rows."""
    from arcflow_amd import ops
    g = torch.Generator().manual_seed(3)
    if which == 'h_rows':
        src = torch.rand(2, 3, 11000, 5, generator=g)
        box, (ho, wo), name = (0.0, 10900.0, 5.0, 11000.0), (8, 6), 'lanczos3'
    else:
        src = torch.rand(2, 3, 64, 5, generator=g)
        box, (ho, wo), name = None, (11000, 6), 'triangle'
    hi, wi = src.shape[2:]
    tab_h = tuple(t.numpy() for t in ops.resample_tables(hi, ho, name, None if box is None else (box[1], box[3])))
    tab_w = tuple(t.numpy() for t in ops.resample_tables(wi, wo, name, None if box is None else (box[0], box[2])))
    got = ops.image_resample(src.cuda(), ho, wo, name, box).cpu().double().numpy()
    ref, bound = R.resample(src.numpy(), tab_h, tab_w, True)
    _check(got, ref, bound, which)
    assert np.abs(ref[1, 2]).min() > 0                                                # the last plane is not trivially zero


def test_all_uint8_values_pass_an_identity_table_bit_exactly():
    from arcflow_amd import ops
    want = np.arange(256, dtype=np.float32) / 255                                     # numpy's float32 x / 255: what edit_inputs.images01 returns today
    for channels in (1, 3):
        src = torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1).expand(1, 16, 16, channels).contiguous()
        for name in ('lanczos3', 'triangle'):
            for clamp in (True, False):
                out = ops.image_resample(src.cuda(), 16, 16, name, None, clamp).cpu().numpy()
                assert out.shape == (1, channels, 16, 16)
                for c in range(channels):
                    assert np.array_equal(out[0, c].reshape(256).view(np.int32), want.view(np.int32)), (channels, name, clamp)
    x = (torch.rand(2, 3, 16, 48, generator=torch.Generator().manual_seed(1)) - 0.5) * 1e3            # fp32 through the identity, unclamped
    assert torch.equal(ops.image_resample(x.cuda(), 16, 48, clamp=False).cpu().view(torch.int32), x.view(torch.int32))


@pytest.mark.parametrize('sigma', [0.5, 2.0, 7.0])
def test_mask_feather(sigma):
    from arcflow_amd import ops
    mask = torch.zeros(2, 1, 48, 32)
    mask[0, 0, 10:30, 8:20] = 1.0                                                     # a hard rectangle
    mask[1, 0, :, :5] = 1.0                                                           # a band on the border: the clipped, renormalised windows
    mask[1, 0, 40:, 20:] = torch.rand(8, 12, generator=torch.Generator().manual_seed(2))            # soft values
    got = ops.mask_feather(mask.cuda(), sigma).cpu()
    tab_h, tab_w = (tuple(t.numpy() for t in ops.gaussian_tables(n, sigma)) for n in (48, 32))
    ref, bound = R.resample(mask.numpy(), tab_h, tab_w, True)
    _check(got.double().numpy(), ref, bound, f'feather sigma {sigma}')
    r = int(np.ceil(3 * sigma))
    far = torch.ones(48, 32, dtype=torch.bool)
    far[max(0, 10 - r):30 + r, max(0, 8 - r):20 + r] = False
    assert (got[0, 0][far] == 0).all()                                                # farther than ceil(3 sigma) from the mask: exactly 0
    assert got.min() >= 0 and got.max() <= 1 and abs(float(got[1, 0, 20, 0]) - ref[1, 0, 20, 0]) <= 1e-6
    assert ref[1, 0, 20, 0] > 0.4                                                     # the border is renormalised, not darkened by padding


def _raw(lib, src, tabs, dst, ws, shape, clamp=1):
    from arcflow_amd import _lib
    B, Cn, H, W, HO, WO = shape
    (hs, hc, hw), (vs, vc, vw) = tabs
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(lib.afx_image_resample(p(src), int(src.dtype == torch.uint8), B, Cn, H, W, p(hs), p(hc), p(hw), hw.shape[1], p(vs), p(vc), p(vw),
                                      vw.shape[1], p(dst), HO, WO, clamp, p(ws), ws.numel() * 4, None))
    torch.cuda.synchronize()


@pytest.mark.parametrize('form', ['u8', 'f32'])
def test_guard_bands_inputs_and_determinism(form):
    from arcflow_amd import _lib, ops
    lib = _lib.load()
    (hi, wi), (ho, wo), _ = CASES['mixed']
    src = _source(form, 3, hi, wi, seed=7).cuda()
    tabs = [tuple(t.cuda() for t in ops.resample_tables(n_in, n_out)) for n_in, n_out in ((wi, wo), (hi, ho))]
    keep = [src.clone()] + [t.clone() for tab in tabs for t in tab]
    G, n, nws = 4096, 2 * 3 * ho * wo, 2 * 3 * hi * wo
    assert lib.afx_image_resample_ws_bytes(2, 3, hi, wo) == 4 * nws
    outs = []
    for _ in range(2):
        buf = torch.full((G + n + G,), -7.0, device='cuda')
        wbuf = torch.full((G + nws + G,), -9.0, device='cuda')
        _raw(lib, src, tabs, buf[G:G + n], wbuf[G:G + nws], (2, 3, hi, wi, ho, wo))
        assert (buf[:G] == -7).all() and (buf[G + n:] == -7).all() and (wbuf[:G] == -9).all() and (wbuf[G + nws:] == -9).all()
        assert (buf[G:G + n] >= 0).all() and (wbuf[G:G + nws] != -9).all()          # ... and everything inside was written
        outs.append(buf[G:G + n].clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    for a, b in zip(keep, [src] + [t for tab in tabs for t in tab]):
        assert torch.equal(a, b)
    assert torch.equal(outs[0].view(2, 3, ho, wo), ops.image_resample(src, ho, wo))


def test_mutated_references_are_rejected(down6):
    """The kernel's result must MISS the bound against each wrong reference, and meet it against the right one with no element excluded."""
    src, got = down6
    tab_h, tab_w = _tables('down6', 'lanczos3')
    ref, bound = R.resample(src, tab_h, tab_w, True)
    _check(got, ref, bound, 'down6 unmutated')
    for what, mutant in (('window off by one', dict(shift=1)), ('no normalisation', dict(normalise=False)), ('fs = 1 on a downscale', dict(fs_one=True))):
        mh, mw = _tables('down6', 'lanczos3', **mutant)
        for th, tw, axis in ((mh, tab_w, 'H'), (tab_h, mw, 'W')):                     # the mutation on one axis alone is already caught
            mref, mbound = R.resample(src, th, tw, True)
            frac = float((np.abs(got - mref) > mbound).mean())
            print(f'{what} on {axis}: {100 * frac:.1f} % of the elements miss the bound')
            assert frac > 0.5, (what, axis)


def test_swapped_tables_are_rejected():
    (hi, wi), _, _ = CASES['square_box']
    src = _source('u8', 3, hi, wi, seed=13)
    got = _run('square_box', src, 'lanczos3')
    tab_h, tab_w = _tables('square_box', 'lanczos3')
    ref, bound = R.resample(src.numpy(), tab_h, tab_w, True)
    _check(got, ref, bound, 'square_box unmutated')
    mref, mbound = R.resample(src.numpy(), tab_w, tab_h, True)
    frac = float((np.abs(got - mref) > mbound).mean())
    print(f'horizontal and vertical tables swapped: {100 * frac:.1f} % of the elements miss the bound')
    assert frac > 0.5


def test_wrapper_argument_errors():
    """The ValueErrors of ops.image_resample / ops.mask_feather that sit behind the device check."""
    from arcflow_amd import ops
    ok = torch.zeros(1, 3, 8, 8, device='cuda')
    for bad in (ok[0], ok.double(), ok.half(), torch.zeros(8, 8, dtype=torch.uint8, device='cuda'), ok[None]):
        with pytest.raises(ValueError, match=r'need uint8 \[B, H, W, C\] or float32 \[B, C, H, W\]'):
            ops.image_resample(bad, 4, 4)
    for bad in (torch.zeros(1, 2, 8, 8, device='cuda'), torch.zeros(1, 8, 8, 4, dtype=torch.uint8, device='cuda'), torch.zeros(1, 3, 0, 8, device='cuda'),
                torch.zeros(0, 8, 8, 3, dtype=torch.uint8, device='cuda')):
        with pytest.raises(ValueError, match='1 or 3 channels and a non-empty image'):
            ops.image_resample(bad, 4, 4)
    for bad in (torch.zeros(1, 8, 8, 1, dtype=torch.uint8, device='cuda'), ok.double()):
        with pytest.raises(ValueError, match=r'mask: need float32'):
            ops.mask_feather(bad, 1.0)
    with pytest.raises(ValueError, match='mask: need uint8'):                           # the shared shape check, under the mask's name
        ops.mask_feather(ok[0, 0], 1.0)
    with pytest.raises(ValueError, match='1 or 3 channels'):
        ops.mask_feather(torch.zeros(1, 2, 8, 8, device='cuda'), 1.0)
    with pytest.raises(ValueError, match='sigma'):
        ops.mask_feather(ok, 1e-200)
    # a non-contiguous source is taken as it is given
    x = torch.rand(1, 3, 8, 16, device='cuda')
    assert torch.equal(ops.image_resample(x[..., ::2], 4, 4), ops.image_resample(x[..., ::2].contiguous(), 4, 4))
