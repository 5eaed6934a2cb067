"""afx_mask_bbox against numpy, integer equality: bbox[b] = (x0, y0, x1, y1), the half-open bounding box of the pixels with m > 0; an image
without one gives (W, H, 0, 0).  Both forms of the mask (uint8 [B, H, W, 1], fp32 [B, 1, H, W]); NaN and negative values are not > 0,
positive denormals and +inf are; widths below and above a work-group; 700 x 700 = 490000 pixels, more than the 1024 work-groups of 256
lanes that one image gets, so the grid-stride loop takes a second trip."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _want(mask):
    """mask: numpy [B, H, W], any dtype."""
    out = []
    for m in mask:
        on = m > 0                                                                     # False for NaN
        ys, xs = np.nonzero(on)
        out.append((m.shape[1], m.shape[0], 0, 0) if len(ys) == 0 else (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1))
    return np.array(out, dtype=np.int32)


def _got(mask, form):
    from arcflow_amd import ops
    t = torch.from_numpy(np.ascontiguousarray(mask))
    t = t.to(torch.uint8)[..., None] if form == 'u8' else t.to(torch.float32)[:, None]
    a = ops.mask_bbox(t.contiguous().cuda())
    b = ops.mask_bbox(t.contiguous().cuda())
    torch.cuda.synchronize()
    assert a.dtype == torch.int32 and a.shape == (mask.shape[0], 4) and a.is_cuda and torch.equal(a, b)          # two runs are equal
    return a.cpu().numpy()


@pytest.mark.parametrize('form', ['u8', 'f32'])
@pytest.mark.parametrize('H,W', [(7, 5), (40, 300), (700, 700)])
def test_pixels_boxes_full_and_empty(form, H, W):
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)]
    mask = np.zeros((len(spots) + 4, H, W), dtype=np.float32)
    for i, (y, x) in enumerate(spots):                                                 # one pixel at each corner and in the middle
        mask[i, y, x] = 1.0
    mask[5] = 1.0                                                                       # full; mask[6] stays empty
    mask[7, H // 3:H // 3 + 3, 1:4] = 0.5 if form == 'f32' else 200                    # two different boxes in one batch
    mask[8, H - 2:, W // 2:] = 1.0
    mask[8, 1, 0] = 1.0
    want = _want(mask)
    assert tuple(want[6]) == (W, H, 0, 0) and tuple(want[5]) == (0, 0, W, H) and tuple(want[4]) == (W // 2, H // 2, W // 2 + 1, H // 2 + 1)
    assert np.array_equal(_got(mask, form), want)
    rng = np.random.default_rng(H + W)
    sparse = (rng.random((2, H, W)) < 3.0 / (H * W)).astype(np.float32)               # a few random pixels
    assert np.array_equal(_got(sparse, form), _want(sparse))


def test_nan_negative_denormal_and_inf():
    H, W = 9, 300
    mask = np.zeros((5, H, W), dtype=np.float32)
    mask[0] = np.nan                                                                    # NaN everywhere: empty
    mask[1] = -1.0                                                                      # negative (and -0.0, -inf, a negative NaN pattern): empty
    mask[1, 0, :3] = (-0.0, -np.inf, np.float32(np.nan) * -1)
    mask[2] = np.nan
    mask[2, 4, 257] = np.float32(1e-45)                                                # the smallest positive denormal among NaN
    mask[3, 2, 7] = np.inf
    mask[3, 6, 299] = np.float32(1.17e-38)                                             # a denormal just below the normal range
    mask[3, 0, 0] = -np.float32(1e-45)
    mask[4, 8, 0] = np.finfo(np.float32).tiny
    assert mask[2, 4, 257] > 0 and mask[3, 6, 299] < np.finfo(np.float32).tiny
    want = np.array([(W, H, 0, 0), (W, H, 0, 0), (257, 4, 258, 5), (7, 2, 300, 7), (0, 8, 1, 9)], dtype=np.int32)
    assert np.array_equal(_want(mask), want)
    assert np.array_equal(_got(mask, 'f32'), want)


def test_wrapper_argument_errors():
    from arcflow_amd import ops
    ok = torch.zeros(2, 1, 8, 8, device='cuda')
    for bad in (ok[0], ok.double(), ok.half(), torch.zeros(2, 3, 8, 8, device='cuda'), torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device='cuda'),
                torch.zeros(2, 1, 8, 8, dtype=torch.uint8, device='cuda'), ok[..., ::2], torch.zeros(0, 1, 8, 8, device='cuda')):
        with pytest.raises(ValueError, match='mask: need'):
            ops.mask_bbox(bad)
