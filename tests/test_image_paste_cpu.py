"""Pasting an edit back into its photo, without a GPU: the window rule of ``schedule.mask_crop_window`` against hand-computed cases, the fp64
reference (tests/image_paste_ref.py) against Pillow, that reference's seven mutants and its admissible sets at the shapes of the kernel
test, the argument guards of afx_mask_bbox / afx_image_paste (refused before any launch) and the refusals of the pipelines'
``padding_mask_crop`` keyword on a pipeline without an engine."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import image_paste_ref as P


# ------------------------------------------------------------------------------------------------ the window rule
# (bbox, src_h, src_w, height, width, pad) -> window, each worked out by hand from the rule in the docstring
WINDOWS = [
    (((0, 0, 6, 8), 40, 56, 32, 32, 4), (0, 0, 12, 12)),              # top-left corner: padded to (0, 0, 10, 12), widened by 2, pushed inside
    (((50, 0, 56, 8), 40, 56, 32, 32, 4), (44, 0, 56, 12)),           # top-right: the widening is shifted left
    (((0, 32, 6, 40), 40, 56, 32, 32, 4), (0, 28, 12, 40)),           # bottom-left
    (((50, 32, 56, 40), 40, 56, 32, 32, 4), (44, 28, 56, 40)),        # bottom-right
    (((10, 10, 16, 18), 40, 56, 32, 32, 0), (9, 10, 17, 18)),         # pad = 0: 6 x 8 -> 8 x 8, one column on either side
    (((10, 10, 16, 18), 40, 56, 32, 32, 100), (0, 0, 56, 40)),        # a pad larger than the image: the whole image (and no room for the aspect)
    (((10, 10, 40, 16), 40, 56, 32, 32, 0), (10, 0, 40, 30)),         # wider than the call: 30 x 6 -> 30 x 30, 12 rows up would cross the top
    (((20, 2, 24, 38), 40, 56, 32, 32, 0), (4, 2, 40, 38)),           # taller than the call: 4 x 36 -> 36 x 36
    (((10, 10, 16, 18), 40, 56, 32, 48, 2), (4, 8, 22, 20)),          # a 3 : 2 call: padded 10 x 12 -> ceil(12 * 48 / 32) = 18 wide
    (((40, 2, 60, 8), 10, 100, 32, 32, 0), (40, 0, 60, 10)),          # an image too small for the aspect: 20 wide wants 20 rows, has 10
    (((5, 7, 6, 8), 40, 56, 32, 32, 0), (5, 7, 6, 8)),                # a 1 x 1 box, square call: itself
    (((5, 7, 6, 8), 40, 56, 16, 32, 0), (5, 7, 7, 8)),                # a 1 x 1 box, 2 : 1 call: two columns, (2 - 1) // 2 = 0 to the left
]


@pytest.mark.parametrize('args,want', WINDOWS)
def test_window_rule_by_hand(args, want):
    from arcflow_amd.schedule import mask_crop_window
    assert mask_crop_window(*args) == want


def test_window_rule_properties_and_errors():
    from arcflow_amd.schedule import mask_crop_window
    rng = np.random.default_rng(7)
    cut = 0
    for _ in range(2000):
        H, W = (int(v) for v in rng.integers(1, 200, 2))
        height, width = (16 * int(v) for v in rng.integers(1, 9, 2))
        x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
        x1, y1 = int(rng.integers(x0 + 1, W + 1)), int(rng.integers(y0 + 1, H + 1))
        pad = int(rng.integers(0, 40))
        a0, b0, a1, b1 = mask_crop_window((x0, y0, x1, y1), H, W, height, width, pad)
        assert 0 <= a0 < a1 <= W and 0 <= b0 < b1 <= H                                                           # inside the image
        assert a0 <= max(x0 - pad, 0) and b0 <= max(y0 - pad, 0) and a1 >= min(x1 + pad, W) and b1 >= min(y1 + pad, H)          # holds the padded box
        ww, wh = a1 - a0, b1 - b0
        exact = 0 <= ww * height - wh * width < height or 0 <= wh * width - ww * height < width                # one side is the ceil of the other's share
        assert exact or ww == W or wh == H
        cut += not exact
    assert 0 < cut < 2000                                                                                       # both kinds occurred
    for empty in ((56, 40, 0, 0), (5, 5, 5, 9), (5, 5, 9, 5)):
        with pytest.raises(ValueError, match='no pixel'):
            mask_crop_window(empty, 40, 56, 32, 32, 4)
    for bad in (((0, 0, 57, 8), 40, 56, 32, 32, 0), ((-1, 0, 5, 8), 40, 56, 32, 32, 0), ((0, 0, 5, 8), 40, 56, 32, 32, -1), ((0, 0, 5, 8), 40, 56, 0, 32, 0)):
        with pytest.raises(ValueError, match='need pad'):
            mask_crop_window(*bad)


# ------------------------------------------------------------------------------------------------ the reference
def _reference(case, masked=True, mutant=None, seed=0):
    _, window, (h, w) = P.CASES[case]
    img, mask, src = P.inputs(case, seed)
    itab = P.tables(h, w, window, 'lanczos3')
    mtab = P.tables(h, w, window, 'triangle')
    return P.paste(img, mask if masked else None, src, window, *itab, *mtab, mutant=mutant)


@pytest.fixture(scope='module')
def truth():
    """(r, E) of every case of the kernel test, with its mask: computed once, shared, never modified."""
    out = {case: _reference(case) for case in P.CASES}
    for r, E in out.values():
        r.setflags(write=False)
        E.setflags(write=False)
    return out


def test_reference_matches_pillow():
    """The reference's bytes rne(255 clamp(r)) against Pillow: ``resize`` of the 8-bit edit (LANCZOS) and of the 8-bit mask (BILINEAR) to
    the window, ``paste`` of both into the photo and an empty mask, ``Image.composite``.  Both start from the same 8-bit edit e (img =
    2 e / 255 - 1) and 8-bit mask.  Pillow rounds the horizontal pass, the vertical pass, the resized mask and the composite to 8 bits, so
    the two differ by rounding only: every byte within 1.  The share of bytes that differ at all is capped at a quarter: outside the
    window and where the mask is 0 both hold the photo's byte; where m = 1 Pillow's byte is the rounding of the vertical pass over
    horizontally ROUNDED values, an error of about 0.29 sqrt(sum w^2) ~ 0.2 byte rms in front of the final rounding, which flips it for
    about E|e| ~ 0.18 of the bytes; the ramp adds the mask's and the composite's roundings on a small part of the window.  Measured here:
    7.6 % / 1.2 % / 0 % of the bytes differ (all by exactly 1) for the three windows.  The inputs are smooth (products of sinusoids, a
    ramp), as decoded images are: Pillow's 8-bit intermediate is the difference under test, not Lanczos' response to noise."""
    from PIL import Image
    yy, xx = np.mgrid[0:32, 0:48].astype(np.float64)
    edit = np.stack([127.5 + 100 * np.sin(yy / 7 + c) * np.cos(xx / 9 - c) for c in range(3)], -1).round().astype(np.uint8)
    mbyte = np.clip((xx - 12) * 16, 0, 255).round().astype(np.uint8)              # 0 on the left, 255 on the right, a 16-pixel ramp
    sy, sx = np.mgrid[0:60, 0:80].astype(np.float64)
    photo = np.stack([127.5 + 90 * np.cos(sy / 11 - c) * np.sin(sx / 13 + 2 * c) for c in range(3)], -1).round().astype(np.uint8)
    img = (edit.astype(np.float32).transpose(2, 0, 1)[None] * np.float32(2.0) / np.float32(255.0) - np.float32(1.0)).astype(np.float32)
    mask = (mbyte.astype(np.float32) / np.float32(255.0))[None, None]
    for window in ((10, 6, 70, 46), (30, 20, 54, 36), (16, 14, 64, 46)):           # 1.25x up, 2x down, the edit's own size
        x0, y0, x1, y1 = window
        r, _ = P.paste(img, mask, photo[None], window, *P.tables(32, 48, window, 'lanczos3'), *P.tables(32, 48, window, 'triangle'))
        ref = np.rint(255.0 * np.clip(r[0], 0.0, 1.0)).astype(np.int64)
        src = Image.fromarray(photo)
        pasted, full = src.copy(), Image.new('L', src.size, 0)
        pasted.paste(Image.fromarray(edit).resize((x1 - x0, y1 - y0), Image.LANCZOS), (x0, y0))
        full.paste(Image.fromarray(mbyte).resize((x1 - x0, y1 - y0), Image.BILINEAR), (x0, y0))
        pil = np.asarray(Image.composite(pasted, src, full), dtype=np.int64)
        diff = np.abs(ref - pil)
        share = float((diff > 0).mean())
        print(f'window {window}: {100 * share:.2f} % of the bytes differ from Pillow, max {diff.max()}')
        assert diff.max() <= 1 and share <= 0.25, window
        outside = np.ones(photo.shape[:2], dtype=bool)
        outside[y0:y1, x0:x1] = False
        assert np.array_equal(ref[outside], photo[outside].astype(np.int64))         # outside the window: the photo


def test_reference_exact_regions(truth):
    """Where the resampled mask is exactly 0 the reference is the source byte, and E there is a few ulp: the only admissible byte is the source's."""
    for case, (r, E) in truth.items():
        _, (x0, y0, x1, y1), (h, w) = P.CASES[case]
        _, _, src = P.inputs(case)
        lo, hi = P.admissible(r, E)
        outside = np.ones(r.shape, dtype=bool)
        outside[:, y0:y1, x0:x1] = False
        assert (E[outside] == 0).all() and np.array_equal(lo[outside], src[outside]) and np.array_equal(hi[outside], src[outside]), case


@pytest.mark.parametrize('mutant', P.MUTANTS)
def test_mutants_are_separable(truth, mutant):
    """At the kernel test's shapes each mutant's admissible bytes are disjoint from the true ones at some element: no output passes both."""
    hits = {}
    for case, (r, E) in truth.items():
        (H, W), (x0, y0, x1, y1), (h, w) = P.CASES[case]
        if (mutant == 'swap' and h != w) or (mutant == 'shift' and (x1 == W or y1 == H)):
            continue
        lo, hi = P.admissible(r, E)
        if mutant == 'trunc':
            mlo, mhi = P.admissible(r, E, trunc=True)
        else:
            mlo, mhi = P.admissible(*_reference(case, mutant=mutant))
        hits[case] = int(((mhi < lo) | (mlo > hi)).sum())
    print(mutant, hits)
    assert hits and max(hits.values()) > 0
    assert sum(v > 0 for v in hits.values()) >= min(3, len(hits))                      # ... and not at one lucky element of one case


def test_admissible_sets_are_narrow(truth):
    """The interval cannot hide a wrong kernel: in every case of the kernel test at most 1 % of the elements admit two bytes and none
    admits three.  (By estimate 255 E is about 6e-4, so about 0.1 % should; the shares are printed.)"""
    for case, (r, E) in truth.items():
        lo, hi = P.admissible(r, E)
        n = hi - lo + 1
        print(f'{case}: {100 * float((n == 2).mean()):.3f} % of the elements admit two bytes, max 255 E = {255 * E.max():.2e}')
        assert n.min() >= 1 and n.max() <= 2 and float((n == 2).mean()) <= 0.01, case
    for case in ('mixed', 'two_groups'):                                               # the unmasked form of the same inputs
        r, E = _reference(case, masked=False)
        n = np.subtract(*P.admissible(r, E)[::-1]) + 1
        assert n.min() >= 1 and n.max() <= 2 and float((n == 2).mean()) <= 0.01, case


# ------------------------------------------------------------------------------------------------ the C ABI's guards
def test_mask_bbox_abi_guards():
    """AFX_E_INVALID before any launch: the pointers are never dereferenced, so plain integers stand in for device memory."""
    from arcflow_amd import _lib
    lib = _lib.load()
    f = lib.afx_mask_bbox
    MB = 1 << 20
    mask, bbox = C.c_void_p(MB), C.c_void_p(2 * MB)
    assert f(None, 0, 2, 8, 8, bbox, None) == _lib.AFX_E_INVALID and b'null' in lib.afx_last_error()
    assert f(mask, 0, 2, 8, 8, None, None) == _lib.AFX_E_INVALID
    for bad in ((0, 8, 8), (2, 0, 8), (2, 8, 0), (-1, 8, 8), (65536, 8, 8)):
        assert f(mask, 0, *bad, bbox, None) == _lib.AFX_E_INVALID, bad
    assert f(C.c_void_p(MB + 2), 0, 2, 8, 8, bbox, None) == _lib.AFX_E_INVALID and b'aligned' in lib.afx_last_error()
    assert f(mask, 1, 2, 8, 8, C.c_void_p(2 * MB + 2), None) == _lib.AFX_E_INVALID and b'aligned' in lib.afx_last_error()
    assert f(mask, 0, 2, 8, 8, C.c_void_p(MB + 4 * 2 * 64 - 4), None) == _lib.AFX_E_INVALID and b'overlaps' in lib.afx_last_error()
    assert f(mask, 1, 2, 8, 8, C.c_void_p(MB - 32 + 4), None) == _lib.AFX_E_INVALID and b'overlaps' in lib.afx_last_error()


def test_image_paste_abi_guards():
    from arcflow_amd import _lib
    lib = _lib.load()
    f = lib.afx_image_paste
    MB = 1 << 20
    B, h, w, H, W, TI, TM = 2, 16, 24, 40, 56, 6, 2
    win = (5, 3, 45, 30)
    ww, wh = win[2] - win[0], win[3] - win[1]
    names = ['img', 'mask', 'mask_batch', 'src', 'dst', 'batch', 'h', 'w', 'H', 'W', 'x0', 'y0', 'x1', 'y1', 'n_out_w', 'n_out_h',
             'ih_start', 'ih_count', 'ih_w', 'ih_taps', 'iv_start', 'iv_count', 'iv_w', 'iv_taps',
             'mh_start', 'mh_count', 'mh_w', 'mh_taps', 'mv_start', 'mv_count', 'mv_w', 'mv_taps', 'ws', 'ws_bytes', 'stream']
    assert len(_lib.PROTOTYPES['afx_image_paste'][1]) == len(names)
    ptr = {n: C.c_void_p(MB * (k + 1)) for k, n in enumerate(n for n in names if n in ('img', 'mask', 'src', 'dst', 'ws') or (n[:2] in ('ih', 'iv', 'mh', 'mv') and not n.endswith('_taps')))}
    need = lib.afx_image_paste_ws_bytes(B, B, h, ww)
    assert need == 4 * (3 * B + B) * h * ww and lib.afx_image_paste_ws_bytes(B, 0, h, ww) == 4 * 3 * B * h * ww
    assert lib.afx_image_paste_ws_bytes(B, 1, h, ww) == 4 * (3 * B + 1) * h * ww
    for bad in ((0, 0, h, ww), (B, -1, h, ww), (4, 2, h, ww), (B, 0, 0, ww), (B, 0, h, 0)):
        assert lib.afx_image_paste_ws_bytes(*bad) == _lib.AFX_E_INVALID, bad
    good = dict(ptr, mask_batch=B, batch=B, h=h, w=w, H=H, W=W, x0=win[0], y0=win[1], x1=win[2], y1=win[3], n_out_w=ww, n_out_h=wh, ih_taps=TI,
                iv_taps=TI, mh_taps=TM, mv_taps=TM, ws_bytes=need, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return f(*[a[n] for n in names])
    # nothing is launched for the good arguments either: this test never calls them.  Every refusal names its reason.
    for name in ('img', 'src', 'dst', 'ih_start', 'ih_count', 'ih_w', 'iv_start', 'iv_count', 'iv_w', 'mh_start', 'mh_count', 'mh_w', 'mv_start',
                 'mv_count', 'mv_w'):
        assert call(**{name: None}) == _lib.AFX_E_INVALID and b'null' in lib.afx_last_error(), name
    for name in ('batch', 'h', 'w', 'H', 'W'):
        assert call(**{name: 0}) == _lib.AFX_E_INVALID, name
    for mb in (0, 3, -1):
        assert call(mask_batch=mb) == _lib.AFX_E_INVALID and b'mask_batch' in lib.afx_last_error(), mb
    assert call(mask=None, mask_batch=1) == _lib.AFX_E_INVALID and b'mask_batch' in lib.afx_last_error()
    for bad in (dict(x0=-1, n_out_w=ww + 1), dict(y0=-1, n_out_h=wh + 1), dict(x1=W + 1, n_out_w=ww + 12), dict(y1=H + 1, n_out_h=wh + 11),
                dict(x1=win[0], n_out_w=0), dict(y1=win[1] - 1, n_out_h=-1)):
        assert call(**bad) == _lib.AFX_E_INVALID and b'inside' in lib.afx_last_error(), bad              # a window not inside the source, or empty
    for bad in (dict(n_out_w=ww - 1), dict(n_out_h=wh + 1), dict(x0=win[0] + 1), dict(y1=win[3] - 1)):
        assert call(**bad) == _lib.AFX_E_INVALID and b'the tables are for' in lib.afx_last_error(), bad       # the window against the tables' n_out
    for name in ('ih_taps', 'iv_taps', 'mh_taps', 'mv_taps'):
        assert call(**{name: 0}) == _lib.AFX_E_INVALID and call(**{name: _lib.AFX_RESAMPLE_MAX_TAPS + 1}) == _lib.AFX_E_INVALID, name
    for name in ptr:
        if name not in ('src', 'dst'):
            assert call(**{name: C.c_void_p(ptr[name].value + 2)}) == _lib.AFX_E_INVALID and b'aligned' in lib.afx_last_error(), name
    assert call(ws=None) == _lib.AFX_E_WORKSPACE and call(ws_bytes=need - 4) == _lib.AFX_E_WORKSPACE and b'workspace' in lib.afx_last_error()
    sbytes = B * H * W * 3
    sizes = dict(img=4 * B * 3 * h * w, mask=4 * B * h * w, src=sbytes, ws=need, ih_start=4 * ww, ih_count=4 * ww, ih_w=4 * ww * TI, iv_start=4 * wh,
                 iv_count=4 * wh, iv_w=4 * wh * TI, mh_start=4 * ww, mh_count=4 * ww, mh_w=4 * ww * TM, mv_start=4 * wh, mv_count=4 * wh, mv_w=4 * wh * TM)
    for name, nbytes in sizes.items():
        base = ptr[name].value
        for at in (base, base + nbytes - 4, base - sbytes + 4):                          # aliased, dst starts in its last element, ends in its first
            assert call(dst=C.c_void_p(at)) == _lib.AFX_E_INVALID and b'overlaps' in lib.afx_last_error(), name
        if name != 'ws':
            assert call(ws=C.c_void_p(base)) == _lib.AFX_E_INVALID and b'overlaps' in lib.afx_last_error(), name
            assert call(ws=C.c_void_p(base - need + 4)) == _lib.AFX_E_INVALID, name


def test_ops_wrappers_refuse_before_the_device():
    """A CPU tensor never reaches the library (the product has no CPU path)."""
    from arcflow_amd import _lib, ops
    with pytest.raises(_lib.ArcflowHipError, match='GPU tensors only'):
        ops.mask_bbox(torch.zeros(1, 1, 4, 4))
    with pytest.raises(_lib.ArcflowHipError, match='GPU tensors only'):
        ops.image_paste(torch.zeros(1, 3, 4, 4), None, torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (0, 0, 4, 4))


# ------------------------------------------------------------------------------------------------ the pipelines' keyword
def _pipe(family):
    from arcflow_amd.pipelines import ArcFluxPipeline, ArcQwenImagePipeline
    return ArcFluxPipeline() if family == 'flux' else ArcQwenImagePipeline()           # no engine, no VAE: the guards come first


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_keyword_refusals(family):
    from PIL import Image
    pipe = _pipe(family)
    kw = dict(prompt_embeds=torch.zeros(1, 4, 8), height=32, width=32)
    photo = np.zeros((40, 56, 3), np.uint8)
    mask = np.zeros((40, 56), np.uint8)
    for call in (pipe, pipe.sample_teacher):
        params = inspect.signature(call).parameters
        assert params['padding_mask_crop'].kind is inspect.Parameter.KEYWORD_ONLY and params['padding_mask_crop'].default is None
        for resize in ('stretch', 'crop'):
            with pytest.raises(ValueError, match='`padding_mask_crop` and `resize` exclude'):
                call(image=photo, mask_image=mask, resize=resize, padding_mask_crop=4, **kw)
        with pytest.raises(ValueError, match='not `image_latents`'):
            call(image_latents=torch.zeros(1, 4, 64), mask_image=mask, padding_mask_crop=4, **kw)
        for img in (photo.astype(np.float32) / 255, torch.rand(1, 3, 40, 56), photo.astype(np.float64), torch.zeros(1, 3, 40, 56, dtype=torch.uint8)):
            with pytest.raises(ValueError, match='needs 8-bit pixels'):                 # a float image: the promise is the source's own bytes
                call(image=img, mask_image=mask, padding_mask_crop=4, **kw)
        for img in (photo, Image.fromarray(photo), [Image.fromarray(photo)]):
            with pytest.raises(ValueError, match='needs `image` and `mask_image`'):    # no mask
                call(image=img, padding_mask_crop=4, **kw)
        with pytest.raises(ValueError, match='needs `image` and `mask_image`'):
            call(mask_image=mask, padding_mask_crop=4, **kw)
        with pytest.raises(ValueError, match="not 'latent'"):
            call(image=photo, mask_image=mask, padding_mask_crop=4, output_type='latent', **kw)
        for bad in (-1, 2.5, '4', True):
            with pytest.raises(ValueError, match='an integer >= 0'):
                call(image=photo, mask_image=mask, padding_mask_crop=bad, **kw)
        with pytest.raises(ValueError, match='divisible by 16'):
            call(image=photo, mask_image=mask, padding_mask_crop=4, **dict(kw, height=40))
