"""``padding_mask_crop=`` of both pipelines, on the tiny synthetic engines and VAEs of tests/test_edit_resize_gpu.py (its ``Setup``, imported),
at a 32 x 32 call on a 40 x 56 uint8 photo with a 6 x 8 mask rectangle and ``padding_mask_crop=4``: the window is
(16, 9, 32, 25) (the box (20, 14, 28, 20) padded to 16 x 14 and heightened to 16 x 16), so the edit is pasted back 2x down.  Every check
is a bit-equality.  On the parent commit every call here fails (``padding_mask_crop`` is an unknown keyword, ``ops.image_paste`` and
``ops.mask_bbox`` do not exist)."""
import numpy as np
import pytest
import torch

from test_edit_resize_gpu import HP, SIZE, WP, Setup

pytestmark = pytest.mark.gpu

PAD = 4
WINDOW = (16, 9, 32, 25)


@pytest.fixture(scope='module', params=['flux', 'qwen'])
def S(request):
    s = Setup(request.param)
    s.mask = np.zeros((40, 56), dtype=np.uint8)
    s.mask[14:20, 20:28] = 255                                                          # 6 rows x 8 columns
    return s


def _pieces(S):
    """The call's pieces by hand: the window, the resampled image and mask as the edit sees them."""
    from arcflow_amd import ops
    from arcflow_amd.schedule import mask_crop_window
    photo = torch.from_numpy(S.photo)[None].cuda()
    m8 = torch.from_numpy(S.mask)[None, ..., None].cuda()
    box = ops.mask_bbox(m8).cpu()
    assert box.tolist() == [[20, 14, 28, 20]]
    window = mask_crop_window(box[0].tolist(), 40, 56, SIZE, SIZE, PAD)
    assert window == WINDOW
    fbox = tuple(float(v) for v in window)
    img = ops.image_resample(photo, SIZE, SIZE, 'lanczos3', fbox)
    mask = ops.image_resample(m8, SIZE, SIZE, 'triangle', fbox)
    return photo, window, img, mask


def test_result_is_the_photo_with_the_edit_pasted_in(S):
    from arcflow_amd import ops
    photo, window, img, mask = _pieces(S)
    x0, y0, x1, y1 = window
    got = S.call(output_type='pt', image=S.photo, mask_image=S.mask, padding_mask_crop=PAD, height=SIZE, width=SIZE)
    assert got.dtype == torch.uint8 and got.shape == (1, 40, 56, 3)                    # the photo's size and dtype
    src = torch.from_numpy(S.photo)[None]
    outside = torch.ones(1, 40, 56, dtype=torch.bool)
    outside[:, y0:y1, x0:x1] = False
    assert torch.equal(got[outside], src[outside])                                      # every byte outside the window is the photo's
    small = ops.image_resample(mask, y1 - y0, x1 - x0, 'triangle').cpu()[0, 0]         # the mask as the paste resamples it
    kept = torch.zeros(1, 40, 56, dtype=torch.bool)
    kept[0, y0:y1, x0:x1] = small == 0
    assert kept.any() and (small > 0).any() and torch.equal(got[kept], src[kept])      # ... and inside it where the mask is 0
    assert not torch.equal(got, src)
    # the whole result: ops.image_paste by hand on the decoded edit of the same call made from its pieces
    decoded = S.call(output_type='pt', image=img.cpu(), mask_image=mask.cpu(), composite=False)
    assert decoded.shape == (1, 3, SIZE, SIZE)
    want = ops.image_paste(decoded.float().cuda().contiguous(), mask, photo, window).cpu()
    assert torch.equal(got, want)
    # composite=False: the paste without a mask
    plain = S.call(output_type='pt', image=S.photo, mask_image=S.mask, padding_mask_crop=PAD, height=SIZE, width=SIZE, composite=False)
    assert torch.equal(plain, ops.image_paste(decoded.float().cuda().contiguous(), None, photo, window).cpu())
    assert torch.equal(plain[outside], src[outside]) and not torch.equal(plain, got)
    again = S.call(output_type='pt', image=S.photo, mask_image=S.mask, padding_mask_crop=PAD, height=SIZE, width=SIZE)
    assert torch.equal(again, got)


def test_output_types_and_input_forms(S):
    from PIL import Image
    kw = dict(mask_image=S.mask, padding_mask_crop=PAD, height=SIZE, width=SIZE)
    pt = S.call(output_type='pt', image=S.photo, **kw)
    arr = S.call(output_type='np', image=S.photo, **kw)
    assert isinstance(arr, np.ndarray) and arr.dtype == np.float32 and arr.shape == (1, 40, 56, 3)
    assert np.array_equal(arr, pt.numpy().astype(np.float32) / np.float32(255.0))
    pil = S.call(output_type='pil', image=Image.fromarray(S.photo), mask_image=Image.fromarray(S.mask), padding_mask_crop=PAD, height=SIZE, width=SIZE)
    assert len(pil) == 1 and pil[0].size == (56, 40) and np.array_equal(np.asarray(pil[0]), pt[0].numpy())
    soft = S.call(output_type='pt', image=S.photo, mask_blur=1.0, **kw)                 # mask_blur feathers the call-size mask as before
    assert soft.shape == pt.shape and not torch.equal(soft, pt)
    with pytest.raises(ValueError, match='no pixel'):
        S.call(output_type='pt', image=S.photo, mask_image=np.zeros((40, 56), np.uint8), padding_mask_crop=PAD, height=SIZE, width=SIZE)
    with pytest.raises(ValueError, match="the mask has the image's size"):
        S.call(output_type='pt', image=S.photo, mask_image=np.zeros((40, 40), np.uint8), padding_mask_crop=PAD, height=SIZE, width=SIZE)


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_sample_teacher_returns_the_photos_size(family, tmp_path):
    from tests.test_teacher_edit_gpu import _pipeline
    pipe, kw = _pipeline(family, str(tmp_path / 'snap'))
    g = torch.Generator().manual_seed(4)
    photo = torch.randint(0, 256, (40, 56, 3), generator=g, dtype=torch.uint8).numpy()
    noise = torch.randn(2, HP * WP, 64, generator=g)
    mask = np.zeros((40, 56), dtype=np.uint8)
    mask[14:20, 20:28] = 255
    kw.update(num_inference_steps=3, strength=0.6, height=SIZE, width=SIZE)
    out = pipe.sample_teacher(image=photo, mask_image=mask, padding_mask_crop=PAD, latents=noise.clone(), output_type='pt', **kw).images.cpu()
    assert out.dtype == torch.uint8 and out.shape == (2, 40, 56, 3)                    # two prompts, one photo: the photo is shared
    x0, y0, x1, y1 = WINDOW
    outside = torch.ones(2, 40, 56, dtype=torch.bool)
    outside[:, y0:y1, x0:x1] = False
    src = torch.from_numpy(photo)[None].expand(2, -1, -1, -1)
    assert torch.equal(out[outside], src[outside]) and not torch.equal(out, src)
