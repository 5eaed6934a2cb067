"""The seams of ``arcflow_amd/pipelines/edit_inputs.py`` that no other CPU test crosses: which fields of ``EditRequest`` each of the three
ways in (as given, resized, cropped to the mask) fills, and ``bytes_output``.  The resized and cropped ways end in device kernels, so here
``ops.image_resample`` / ``ops.mask_bbox`` are stood in for by host functions of the same shapes: the test is about the request, not the pixels."""
import numpy as np
import pytest
import torch

H, W = 32, 48


@pytest.fixture
def EI(monkeypatch):
    from arcflow_amd.pipelines import edit_inputs

    def image_resample(src, height, width, filt='lanczos3', box=None, clamp=False):
        B, C = (src.shape[0], src.shape[3]) if src.dtype == torch.uint8 else src.shape[:2]
        return torch.full((B, C, height, width), 0.5)

    def mask_bbox(mask):
        return torch.tensor([[20, 14, 28, 20]] * mask.shape[0], dtype=torch.int32)
    monkeypatch.setattr(edit_inputs.ops, 'image_resample', image_resample)
    monkeypatch.setattr(edit_inputs.ops, 'mask_bbox', mask_bbox)
    return edit_inputs


def _populated(edit):
    return {k for k, v in vars(edit).items() if v is not None}


def test_edit_request_fields_of_the_three_branches(EI):
    g = torch.Generator().manual_seed(0)
    img, mask, lat = torch.rand(1, 3, H, W, generator=g), torch.ones(1, 1, H, W), torch.zeros(1, 6, 64)
    photo = torch.randint(0, 256, (40, 56, 3), generator=g, dtype=torch.uint8).numpy()
    pmask = np.zeros((40, 56), dtype=np.uint8)
    pmask[14:20, 20:28] = 255

    def call(image=None, image_latents=None, mask_image=None, strength=0.5, height=None, width=None, resize=None, mask_blur=0.0,
             padding_mask_crop=None, output_type='pt', color_fix=None):
        return EI.edit_inputs(image, image_latents, mask_image, strength, height, width, resize, mask_blur, padding_mask_crop, output_type,
                              color_fix, 'cpu', 1024)
    # as given
    edit, h, w = call(image=img, color_fix='wavelet')
    assert isinstance(edit, EI.EditRequest) and (h, w) == (H, W)
    assert _populated(edit) == {'image', 'strength', 'color_fix'} and edit.color_fix == 'wavelet' and edit.strength == 0.5
    assert torch.equal(edit.image, img)
    edit, h, w = call(image=img, mask_image=mask)
    assert _populated(edit) == {'image', 'mask', 'strength'} and torch.equal(edit.mask, mask)
    edit, h, w = call(image_latents=lat, mask_image=mask)
    assert _populated(edit) == {'image_latents', 'mask', 'strength'} and edit.image_latents is lat and (h, w) == (H, W)
    # resized: the size defaults to the photo's sides rounded to multiples of 16
    edit, h, w = call(image=photo, resize='stretch', color_fix='adain')
    assert (h, w) == (48, 64) and _populated(edit) == {'image', 'strength', 'color_fix'} and edit.color_fix == 'adain'
    assert edit.image.shape == (1, 3, 48, 64)
    edit, h, w = call(image=photo, mask_image=pmask, resize='crop', height=H, width=W)
    assert _populated(edit) == {'image', 'mask', 'strength'} and edit.image.shape == (1, 3, H, W) and edit.mask.shape == (1, 1, H, W)
    # cropped to the mask: the only way that sets ``paste`` -- the photo's own bytes and the window
    edit, h, w = call(image=photo, mask_image=pmask, padding_mask_crop=4, height=32, width=32)
    assert (h, w) == (32, 32) and _populated(edit) == {'image', 'mask', 'strength', 'paste'}
    src, window = edit.paste
    assert src.dtype == torch.uint8 and np.array_equal(src.numpy(), photo[None]) and window == (16, 9, 32, 25)
    assert edit.image.shape == (1, 3, 32, 32) and edit.mask.shape == (1, 1, 32, 32)
    for e in (call(image=img)[0], call(image=photo, resize='stretch')[0]):
        assert e.paste is None and e.color_fix is None and e.x0 is None and e.mask_tokens is None
    # text-to-image: no request
    assert call(height=None, width=512) == (None, None, 512)


def test_bytes_output():
    from PIL import Image
    from arcflow_amd.pipelines.edit_inputs import bytes_output
    out = torch.randint(0, 256, (2, 16, 24, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    assert bytes_output(out, 'pt') is out
    arr = bytes_output(out, 'np')
    assert isinstance(arr, np.ndarray) and arr.dtype == np.float32 and arr.shape == (2, 16, 24, 3)
    assert np.array_equal(arr, out.numpy().astype(np.float32) / np.float32(255))
    pil = bytes_output(out, 'pil')
    assert len(pil) == 2 and all(isinstance(im, Image.Image) and im.size == (24, 16) and im.mode == 'RGB' for im in pil)
    assert np.array_equal(np.stack([np.asarray(im) for im in pil]), out.numpy())
