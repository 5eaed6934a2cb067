"""Image resampling without a GPU: the tables of ``afx_resample_table`` / ``ops.resample_tables`` against an independent statement of the
rule (tests/image_resample_ref.py), the fp64 reference against Pillow, the argument guards of the C ABI (refused before any launch) and the
pipelines' new ``resize`` / ``mask_blur`` arguments on a pipeline without an engine."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import image_resample_ref as R

# (H_in, W_in) -> (H_out, W_out): up and down on either axis, a 6x downscale, a 5x upscale, a source smaller than the filter's support, a 3-pixel axis
SHAPES = [((37, 53), (48, 32)), ((100, 70), (16, 16)), ((16, 16), (80, 48)), ((5, 7), (32, 16)), ((200, 3), (16, 48))]
BOX_CASE = ((37, 53), (24, 40), (3.25, 1.5, 47.75, 30.125))          # (left, upper, right, lower), fractional
FILTERS = ['lanczos3', 'triangle']


def _axes():
    for (hi, wi), (ho, wo) in SHAPES:
        yield hi, ho, None
        yield wi, wo, None
    (hi, wi), (ho, wo), (l, u, r, b) = BOX_CASE
    yield hi, ho, (u, b)
    yield wi, wo, (l, r)


@pytest.mark.parametrize('name', FILTERS)
def test_tables_follow_the_rule(name):
    """start and count exactly; the weights to 2^-24 absolute: every |w| <= 1, so the one fp32 rounding is <= 2^-25 and the rest is the
    difference of two fp64 evaluations."""
    from arcflow_amd import ops
    for n_in, n_out, box in _axes():
        start, count, w = ops.resample_tables(n_in, n_out, name, box)
        rs, rc, rw = R.rule_table(n_in, n_out, name, box)
        assert w.dtype == torch.float32 and start.dtype == count.dtype == torch.int32 and w.shape == (n_out, int(rc.max())), (n_in, n_out)
        assert np.array_equal(start.numpy(), rs) and np.array_equal(count.numpy(), rc), (n_in, n_out, box)
        assert np.abs(w.double().numpy() - rw).max() <= 2.0 ** -24, (n_in, n_out, box)
        assert (start >= 0).all() and (start + count <= n_in).all() and (count >= 1).all()
        assert np.abs(w.double().sum(1).numpy() - 1.0).max() <= 1e-6


def test_same_size_tables_are_the_identity():
    from arcflow_amd import ops
    for name in FILTERS:
        for n in (1, 2, 16, 37):
            start, count, w = ops.resample_tables(n, n, name)
            m = R.dense((start.numpy(), count.numpy(), w.numpy()), n)
            assert np.array_equal(m, np.eye(n)), (name, n)
            assert ((w == 0) | (w == 1)).all()


@pytest.mark.parametrize('name,pil_name', [('lanczos3', 'LANCZOS'), ('triangle', 'BILINEAR')])
def test_reference_matches_pillow(name, pil_name):
    """The fp64 reference on ops.resample_tables against Pillow's mode 'F' resize, inputs in [0, 1].

    Tolerance: the larger of the difference measured when the rule was pinned, 8.8e-8 (with the draws of this test: at most 1.42e-7, Lanczos-3
    16 x 16 -> 80 x 48), and 4 * 2^-24 * max|x| per pass (two passes: 4.8e-7).  The factor 4: Pillow accumulates a pass in double and stores it as fp32, half an ulp of a value |v| <= sum|w| max|x| < 2 max|x|,
    i.e. at most 2 * 2^-24 max|x|; the tables here carry fp32 weights where Pillow's are doubles, at most 2^-24 sum|w| max|x| < 2 * 2^-24 max|x|
    more.  (The first pass's error also goes through the second pass's weights, sum|w| <= 1.3 for Lanczos-3; typical differences are far below
    the worst case, and the measured ones are printed.)"""
    from PIL import Image
    from arcflow_amd import ops
    rng = np.random.default_rng(5)
    cases = [(s, o, None) for s, o in SHAPES] + [BOX_CASE]
    for (hi, wi), (ho, wo), box in cases:
        x = rng.random((hi, wi), dtype=np.float32)
        bw, bh = ((0.0, float(wi)), (0.0, float(hi))) if box is None else ((box[0], box[2]), (box[1], box[3]))
        tab_w = tuple(t.numpy() for t in ops.resample_tables(wi, wo, name, bw))
        tab_h = tuple(t.numpy() for t in ops.resample_tables(hi, ho, name, bh))
        ref, _ = R.resample(x[None, None], tab_h, tab_w, clamp=False)
        pil = np.asarray(Image.fromarray(x, mode='F').resize((wo, ho), getattr(Image, pil_name), box=box), dtype=np.float64)
        diff = np.abs(ref[0, 0] - pil).max()
        tol = max(8.8e-8, 2 * 4 * 2.0 ** -24 * float(x.max()))
        print(f'{name} {hi}x{wi} -> {ho}x{wo} box {box}: max |ref - Pillow| = {diff:.3e} (tol {tol:.3e})')
        assert pil.shape == (ho, wo) and diff <= tol, (hi, wi, ho, wo, box)


def test_gaussian_tables():
    from arcflow_amd import ops
    for n, sigma in ((48, 0.5), (48, 2.0), (32, 7.0), (5, 7.0)):
        start, count, w = ops.gaussian_tables(n, sigma)
        rs, rc, rw = R.gaussian_rule(n, sigma)
        r = int(np.ceil(3 * sigma))
        assert np.array_equal(start.numpy(), rs) and np.array_equal(count.numpy(), rc) and np.abs(w.double().numpy() - rw).max() <= 2.0 ** -24
        assert np.abs(w.double().sum(1).numpy() - 1.0).max() <= 1e-6                   # every window is renormalised, also the clipped ones
        for i in range(n):
            assert int(start[i]) == max(0, i - r) and int(start[i] + count[i]) == min(n, i + r + 1)         # clipped at the borders, nothing padded
            if r <= i < n - r:                                                          # interior: the full symmetric window
                row = w[i, :2 * r + 1]
                assert int(count[i]) == 2 * r + 1 and torch.equal(row, row.flip(0)) and row.argmax() == r
        if n > 2 * r:
            assert float(w[0, 0]) > float(w[r, r])                                      # a border pixel's own weight grows: fewer taps share the 1
    for bad in (0.0, -1.0, float('inf'), float('nan'), 1e-200):                        # 1e-200: its square underflows, exp(-0 / 0) would be NaN
        with pytest.raises(ValueError, match='sigma'):
            ops.gaussian_tables(16, bad)
    start, count, w = ops.gaussian_tables(16, 1e-100)                                   # tiny but squarable: the identity, and finite
    assert torch.equal(w[torch.arange(16), torch.arange(16) - start], torch.ones(16)) and w.sum() == 16 and torch.isfinite(w).all()


def test_tap_cap_and_table_guards():
    from arcflow_amd import _lib, ops
    lib = _lib.load()
    cap = _lib.AFX_RESAMPLE_MAX_TAPS
    start, count, w = ops.resample_tables(1600, 100, 'lanczos3')                       # 16x down: within the cap
    assert 90 <= w.shape[1] <= 98 <= cap
    with pytest.raises(ValueError, match='AFX_RESAMPLE_MAX_TAPS'):
        ops.resample_tables(4000, 100, 'lanczos3')                                      # 40x down: 240 taps
    with pytest.raises(ValueError, match='AFX_RESAMPLE_MAX_TAPS'):
        ops.gaussian_tables(512, 40.0)                                                  # 241 taps
    with pytest.raises(ValueError, match='filter'):
        ops.resample_tables(16, 16, 'bicubic')
    with pytest.raises(ValueError, match='filter'):
        ops.image_resample(torch.zeros(1, 3, 4, 4), 4, 4, filter='nearest')
    f = lib.afx_resample_table
    s, c, wt = (np.zeros(8, np.int32), np.zeros(8, np.int32), np.zeros((8, 6), np.float32))
    ptr = [C.c_void_p(a.ctypes.data) for a in (s, c, wt)]
    assert f(16, 8, _lib.AFX_FILTER_LANCZOS3, 0.0, 16.0, 0.0, None, None, None, cap) == 12          # the query form
    assert f(16, 8, _lib.AFX_FILTER_LANCZOS3, 0.0, 16.0, 0.0, *ptr, 6) == _lib.AFX_E_INVALID and b'max_taps' in lib.afx_last_error()
    assert not wt.any()                                                                 # refused before anything was written
    assert f(4000, 100, _lib.AFX_FILTER_LANCZOS3, 0.0, 4000.0, 0.0, None, None, None, 1 << 20) == _lib.AFX_E_UNSUPPORTED
    assert f(16, 8, _lib.AFX_FILTER_LANCZOS3, 0.0, 16.0, 0.0, ptr[0], None, ptr[2], cap) == _lib.AFX_E_INVALID
    for args in ((0, 8, 0, 0.0, 16.0), (16, 0, 0, 0.0, 16.0), (16, 8, 7, 0.0, 16.0), (16, 8, 0, -1.0, 16.0), (16, 8, 0, 4.0, 4.0), (16, 8, 0, 0.0, 16.5),
                 (16, 8, 0, float('nan'), 16.0), (16, 8, _lib.AFX_FILTER_GAUSSIAN, 0.0, 16.0)):
        assert f(*args, 0.0, None, None, None, cap) == _lib.AFX_E_INVALID, args
    assert f(16, 8, 0, 0.0, 16.0, 0.0, None, None, None, 0) == _lib.AFX_E_INVALID


def test_image_resample_abi_guards():
    """AFX_E_INVALID / AFX_E_WORKSPACE before any launch: the pointers are never dereferenced, so plain integers stand in for device memory."""
    from arcflow_amd import _lib
    lib = _lib.load()
    f = lib.afx_image_resample
    MB = 1 << 20
    B, Cn, H, W, HO, WO, TH, TV = 2, 3, 20, 30, 8, 12, 6, 5
    src, hs, hc, hw, vs, vc, vw, dst, ws = [C.c_void_p(MB * k) for k in range(1, 10)]
    need = lib.afx_image_resample_ws_bytes(B, Cn, H, WO)
    assert need == 4 * B * Cn * H * WO
    names = ['src', 'src_u8', 'batch', 'C', 'H_in', 'W_in', 'h_start', 'h_count', 'h_w', 'h_taps', 'v_start', 'v_count', 'v_w', 'v_taps', 'dst',
             'H_out', 'W_out', 'clamp', 'ws', 'ws_bytes', 'stream']
    good = [src, 0, B, Cn, H, W, hs, hc, hw, TH, vs, vc, vw, TV, dst, HO, WO, 1, ws, need, None]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return f(*a)
    for name in ('src', 'dst', 'h_start', 'h_count', 'h_w', 'v_start', 'v_count', 'v_w'):
        assert call(**{name: None}) == _lib.AFX_E_INVALID and b'null' in lib.afx_last_error(), name
    for bad in (0, 2, 4, -1):
        assert call(C=bad) == _lib.AFX_E_INVALID and b'C must be 1 or 3' in lib.afx_last_error()
    for name in ('batch', 'H_in', 'W_in', 'H_out', 'W_out'):                            # empty shapes
        assert call(**{name: 0}) == _lib.AFX_E_INVALID, name
    for name in ('h_taps', 'v_taps'):
        assert call(**{name: 0}) == _lib.AFX_E_INVALID and call(**{name: _lib.AFX_RESAMPLE_MAX_TAPS + 1}) == _lib.AFX_E_INVALID, name
    for name in ('src', 'dst', 'ws', 'h_start', 'h_count', 'h_w', 'v_start', 'v_count', 'v_w'):
        base = good[names.index(name)].value
        assert call(**{name: C.c_void_p(base + 2)}) == _lib.AFX_E_INVALID and b'aligned' in lib.afx_last_error(), name
    assert call(ws=None) == _lib.AFX_E_WORKSPACE and call(ws_bytes=need - 4) == _lib.AFX_E_WORKSPACE and b'workspace' in lib.afx_last_error()
    dbytes, sbytes = 4 * B * Cn * HO * WO, 4 * B * Cn * H * W
    for name, nbytes in (('src', sbytes), ('h_start', 4 * WO), ('h_count', 4 * WO), ('h_w', 4 * WO * TH), ('v_start', 4 * HO), ('v_count', 4 * HO),
                         ('v_w', 4 * HO * TV), ('ws', need)):
        base = good[names.index(name)].value
        assert call(dst=C.c_void_p(base)) == _lib.AFX_E_INVALID and b'overlaps' in lib.afx_last_error(), name       # exact aliasing
        assert call(dst=C.c_void_p(base + nbytes - 4)) == _lib.AFX_E_INVALID, name                                  # dst starts in its last element
        assert call(dst=C.c_void_p(base - dbytes + 4)) == _lib.AFX_E_INVALID, name                                  # dst ends in its first element
        if name != 'ws':
            assert call(ws=C.c_void_p(base), ws_bytes=need) == _lib.AFX_E_INVALID, name
    for bad in ((0, 3, 4, 4), (1, 2, 4, 4), (1, 3, 0, 4), (1, 3, 4, 0)):
        assert lib.afx_image_resample_ws_bytes(*bad) == _lib.AFX_E_INVALID


# ------------------------------------------------------------------------------------------------ the pipelines' arguments
def _pipe(family='flux'):
    from arcflow_amd.pipelines import ArcFluxPipeline, ArcQwenImagePipeline
    return ArcFluxPipeline() if family == 'flux' else ArcQwenImagePipeline()         # no engine, no VAE: the guards come first


def test_default_size_rounding_and_crop_box():
    from arcflow_amd.pipelines.edit_inputs import crop_box, default_side
    for n, want in ((1, 16), (7, 16), (8, 16), (16, 16), (23, 16), (24, 32), (39, 32), (40, 48), (56, 64), (57, 64), (3000, 3008), (4000, 4000)):
        assert default_side(n) == want, n
    assert crop_box(40, 56, 32, 32) == (8.0, 0.0, 48.0, 40.0)                    # wider source: centred columns
    assert crop_box(56, 40, 32, 32) == (0.0, 8.0, 40.0, 48.0)                    # taller source: centred rows
    assert crop_box(30, 100, 32, 16) == (42.5, 0.0, 57.5, 30.0)                  # fractional
    assert crop_box(100, 30, 16, 32) == (0.0, 42.5, 30.0, 57.5)
    assert crop_box(60, 80, 24, 32) == (0.0, 0.0, 80.0, 60.0)                    # the target aspect already: the whole image
    for sh, sw, h, w in ((37, 53, 48, 32), (3000, 4000, 1024, 1024), (5, 7, 32, 16)):
        l, u, r, b = crop_box(sh, sw, h, w)
        assert 0 <= l < r <= sw and 0 <= u < b <= sh and abs((r - l) * h - (b - u) * w) < 1e-9 * sw * h          # inside, the call's aspect ...
        assert abs((l + r) / 2 - sw / 2) < 1e-9 and abs((u + b) / 2 - sh / 2) < 1e-9 and (r - l == sw or b - u == sh)       # ... centred, largest


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_new_argument_errors(family):
    pipe = _pipe(family)
    kw = dict(prompt_embeds=torch.zeros(1, 4, 8), output_type='latent')
    img, lat = torch.rand(1, 3, 32, 48), torch.zeros(1, 6, 64)
    for call in (pipe, pipe.sample_teacher):
        with pytest.raises(ValueError, match='resizes nothing'):                        # resize=None: the size mismatch reads as before
            call(image=img, height=64, width=48, **kw)
        with pytest.raises(ValueError, match='resizes nothing'):
            call(image=img, height=64, width=48, resize=None, mask_blur=0.0, **kw)
        with pytest.raises(ValueError, match='`resize`'):
            call(image=img, resize='fit', **kw)
        for bad in (np.zeros((4, 4), np.uint8), np.zeros((2, 4, 4, 2), np.uint8), np.zeros((4, 4, 3, 1, 1), np.uint8)):
            with pytest.raises(ValueError, match='cannot read uint8'):                  # a uint8 array that is no [B, H, W, 3]
                call(image=bad, resize='stretch', **kw)
        with pytest.raises(ValueError, match='cannot read uint8'):
            call(image_latents=lat, mask_image=np.zeros((1, 4, 4, 3), np.uint8), height=32, width=48, resize='stretch', **kw)
        with pytest.raises(ValueError, match='a torch tensor must be floating point'):
            call(image=torch.zeros(1, 3, 32, 48, dtype=torch.uint8), resize='stretch', **kw)
        with pytest.raises(ValueError, match='nothing to resize'):
            call(image_latents=lat, height=32, width=48, resize='stretch', **kw)
        with pytest.raises(ValueError, match='divisible by 16'):
            call(image=img, height=40, width=48, resize='stretch', **kw)
        for bad in (-1.0, float('inf'), float('nan')):
            with pytest.raises(ValueError, match='mask_blur'):
                call(image=img, mask_image=torch.ones(1, 1, 32, 48), mask_blur=bad, **kw)
        with pytest.raises(ValueError, match='`mask_blur` needs a `mask_image`'):
            call(image=img, mask_blur=2.0, **kw)
        with pytest.raises(ValueError, match='need `image`'):
            call(resize='crop', height=32, width=32, **kw)
        with pytest.raises(ValueError, match='need `image`'):
            call(mask_blur=1.0, height=32, width=32, **kw)
        params = inspect.signature(call).parameters
        assert params['resize'].kind is params['mask_blur'].kind is inspect.Parameter.KEYWORD_ONLY
        assert params['resize'].default is None and params['mask_blur'].default == 0.0
