"""Host-side half of image editing, shared by both pipelines: plain functions that read ``image`` / ``mask_image`` in
every accepted form, check the edit keywords and build the ``EditRequest`` that travels through the loop to ``_output``; and
``bytes_output``.  Nothing here holds a pipeline: what a function needs of one (``device``, the default size) is an argument."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Optional, Tuple

import numpy as np
import torch

from .. import ops
from ..schedule import mask_crop_window


@dataclass
class EditRequest:
    """The edit arguments of one call.  ``image`` / ``mask``: fp32 [B, C, H, W] in [0, 1] at the call's size; ``image_latents``: packed.
    ``paste``, set by ``padding_mask_crop`` alone: (the photo's bytes on the GPU, uint8 [B, H, W, 3]; the window (x0, y0, x1, y1)).
    ``x0`` [B, N, 64] and ``mask_tokens`` [B, N, 4] are filled in by ``_edit_prepare`` once the batch is known."""
    image: Optional[torch.Tensor]
    image_latents: Optional[torch.Tensor]
    mask: Optional[torch.Tensor]
    strength: float
    color_fix: Optional[str] = None
    paste: Optional[Tuple[torch.Tensor, Tuple[int, int, int, int]]] = None
    x0: Optional[torch.Tensor] = None
    mask_tokens: Optional[torch.Tensor] = None


# checks ----------------------------------------------------------------------------------------------
def check_strength(strength) -> None:
    if not 0.0 < float(strength) <= 1.0:
        raise ValueError(f'`strength` must be in (0, 1], got {strength}')


def check_color_fix(color_fix, image, mask_image, padding_mask_crop, output_type) -> None:
    """What ``color_fix`` refuses, before anything runs."""
    if color_fix is None:
        return
    if color_fix not in ('adain', 'wavelet'):
        raise ValueError(f"`color_fix`: None, 'adain' or 'wavelet', got {color_fix!r}")
    if image is None:
        raise ValueError('`color_fix` needs `image`: text-to-image and `image_latents` have no pixels to match the result to')
    if mask_image is not None or padding_mask_crop is not None:
        raise ValueError('`color_fix` does not go with `mask_image` (or `padding_mask_crop`): matching a repaint\'s colours to what it '
                         'replaces undoes the inpainting')
    if output_type == 'latent':
        raise ValueError("`color_fix` works on decoded pixels: output_type 'pil', 'np' or 'pt', not 'latent'")


def resolve_size(height, width, default: int, detail: str = ''):
    """-> (height, width) of a call: ``default`` for a side not given, both multiples of 16.  ``detail`` is what the site adds to the
    error ('{height}' / '{width}' are filled in)."""
    height, width = height or default, width or default
    if height % 16 or width % 16:
        raise ValueError('`height` and `width` have to be divisible by 16' + detail.format(height=height, width=width))
    return height, width


def default_side(n: int) -> int:
    """The call's side for a source side of ``n`` pixels under ``resize``: the nearest multiple of 16 (ties up), at least 16."""
    return max(16, 16 * ((int(n) + 8) // 16))


def crop_box(src_h: int, src_w: int, height: int, width: int):
    """(left, upper, right, lower) of the largest centred window of a ``src_h`` x ``src_w`` image with the aspect ratio ``width`` :
    ``height``, in source pixels; fractional.  An image that already has that ratio gives the whole image."""
    if src_w * height > src_h * width:                  # the source is wider: full height, centred columns
        cw = src_h * width / height
        return ((src_w - cw) / 2, 0.0, (src_w + cw) / 2, float(src_h))
    if src_w * height < src_h * width:
        ch = src_w * height / width
        return (0.0, (src_h - ch) / 2, float(src_w), (src_h + ch) / 2)
    return (0.0, 0.0, float(src_w), float(src_h))


# reading images and masks ----------------------------------------------------------------------------
def images01(image, name='image', channels=3) -> torch.Tensor:
    """A torch [B, C, H, W] / [C, H, W], numpy [B, H, W, C] / [H, W, C], PIL image or list of PIL images in [0, 1] (PIL: 8 bit) ->
    fp32 [B, C, H, W] in [0, 1].  With channels = 1 (a mask) the channel axis may be missing: [B, H, W] / [H, W]."""
    def pil(im):
        return torch.from_numpy(np.asarray(im.convert('RGB' if channels == 3 else 'L'), dtype=np.float32) / 255.0)
    if isinstance(image, (list, tuple)):
        t = torch.stack([pil(im) for im in image])
        t = t[:, None] if channels == 1 else t.permute(0, 3, 1, 2)
    elif isinstance(image, torch.Tensor):
        t = image
        if channels == 1:
            t = t[None, None] if t.dim() == 2 else (t[:, None] if t.dim() == 3 and t.shape[0] != 1 else t)
        if t.dim() == 3:
            t = t[None]
    elif isinstance(image, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(image))
        if channels == 1:
            t = t[None, None] if t.dim() == 2 else (t[:, None] if t.dim() == 3 else t.permute(0, 3, 1, 2))
        else:
            t = (t[None] if t.dim() == 3 else t).permute(0, 3, 1, 2)
    elif hasattr(image, 'convert'):
        t = pil(image)
        t = t[None, None] if channels == 1 else t.permute(2, 0, 1)[None]
    else:
        raise ValueError(f'`{name}`: a torch tensor, a numpy array, a PIL image or a list of PIL images, got {type(image).__name__}')
    if t.dim() != 4 or t.shape[1] != channels:
        raise ValueError(f'`{name}`: cannot read {tuple(t.shape)} as [B, {channels}, H, W]')
    return t.to(torch.float32)


def resize_source(image, name, channels, device) -> torch.Tensor:
    """``image`` on the GPU as ops.image_resample reads it: PIL images and uint8 numpy arrays as uint8 [B, H, W, C] (read as x / 255, 3 B per
    pixel over the bus), everything else as ``images01`` gives it, fp32 [B, C, H, W].  NOTE the one difference to ``resize=None``: there
    ``images01`` takes a uint8 numpy array as values already in [0, 1], undivided; here it is 8-bit pixels.  A uint8 torch tensor raises."""
    mode = 'RGB' if channels == 3 else 'L'
    if isinstance(image, (list, tuple)) and len(image) and all(hasattr(im, 'convert') for im in image):
        arr = np.stack([np.array(im.convert(mode), dtype=np.uint8) for im in image])
        arr = arr[..., None] if channels == 1 else arr
    elif hasattr(image, 'convert'):
        arr = np.array(image.convert(mode), dtype=np.uint8)[None]
        arr = arr[..., None] if channels == 1 else arr
    elif isinstance(image, np.ndarray) and image.dtype == np.uint8:
        arr = image
        if channels == 1:
            arr = arr[None, ..., None] if arr.ndim == 2 else (arr[..., None] if arr.ndim == 3 else arr)
        elif arr.ndim == 3:
            arr = arr[None]
        if arr.ndim != 4 or arr.shape[3] != channels:
            raise ValueError(f'`{name}`: cannot read uint8 {tuple(image.shape)} as [B, H, W, {channels}]')
    elif isinstance(image, torch.Tensor) and image.dtype == torch.uint8:
        # [B, C, H, W] bytes read undivided (as resize=None reads them) would saturate in the clamp, and a byte tensor's layout is ambiguous
        raise ValueError(f'`{name}`: with `resize`, pass 8-bit pixels as a PIL image or a uint8 numpy array [B, H, W, {channels}] (read as x / 255); '
                         f'a torch tensor must be floating point in [0, 1], got uint8 {tuple(image.shape)}')
    else:
        return images01(image, name, channels).to(device).contiguous()
    return torch.from_numpy(np.ascontiguousarray(arr)).to(device)


def photo_bytes(image, name: str, why: str) -> np.ndarray:
    """One photo given as 8-bit pixels -- a PIL image (or a list of one) or a uint8 numpy array [H, W, 3] / [1, H, W, 3] -- as uint8
    [1, H, W, 3] on the host; anything else, or a batch other than 1, raises (``why``: what the caller needs the bytes for)."""
    if isinstance(image, (list, tuple)) and len(image) and all(hasattr(im, 'convert') for im in image):
        arr = np.stack([np.array(im.convert('RGB'), dtype=np.uint8) for im in image])
    elif hasattr(image, 'convert'):
        arr = np.array(image.convert('RGB'), dtype=np.uint8)[None]
    elif isinstance(image, np.ndarray) and image.dtype == np.uint8:
        arr = image[None] if image.ndim == 3 else image
        if arr.ndim != 4 or arr.shape[3] != 3 or min(arr.shape) < 1:
            raise ValueError(f'`{name}`: cannot read uint8 {tuple(image.shape)} as [H, W, 3]')
    else:
        raise ValueError(f'`{name}` needs 8-bit pixels, a PIL image or a uint8 numpy array [H, W, 3]: {why}; got {type(image).__name__}'
                         + (f' {image.dtype}' if hasattr(image, 'dtype') else ''))
    if arr.shape[0] != 1:
        raise ValueError(f'`{name}`: one picture, got a batch of {arr.shape[0]}')
    return np.ascontiguousarray(arr)


# the three ways in -----------------------------------------------------------------------------------
def inputs_as_given(image, mask_image, height, width, default_size):
    """``resize=None``: -> (img, mask, height, width) on the host; every input must have the call's size."""
    img = None if image is None else images01(image)
    mask = None if mask_image is None else images01(mask_image, 'mask_image', 1)
    for t in (img, mask):
        if t is not None:
            height, width = height or t.shape[2], width or t.shape[3]
    height, width = resolve_size(height, width, default_size, ', got {height} x {width} (an edit resizes nothing)')
    for t, name in ((img, 'image'), (mask, 'mask_image')):
        if t is not None and tuple(t.shape[2:]) != (height, width):
            raise ValueError(f'`{name}` is {t.shape[2]} x {t.shape[3]}, the call is {height} x {width}: an edit resizes nothing')
    return img, mask, height, width


def inputs_resized(image, image_latents, mask_image, height, width, resize, device):
    """``resize='stretch' | 'crop'``: -> (img, mask, height, width) with img / mask fp32 [B, C, height, width] on the GPU, the image resampled
    with Lanczos-3, the mask with the triangle filter; ``height`` / ``width`` default to the source's sides rounded to multiples of 16."""
    if resize not in ('stretch', 'crop'):
        raise ValueError(f"`resize`: None, 'stretch' or 'crop', got {resize!r}")
    if image_latents is not None and mask_image is None:
        raise ValueError('`resize` with `image_latents` and no `mask_image` has nothing to resize: latents are not resampled')
    if (height and height % 16) or (width and width % 16):
        raise ValueError(f'`height` and `width` have to be divisible by 16, got {height} x {width}')
    srcs = [None if image is None else resize_source(image, 'image', 3, device),
            None if mask_image is None else resize_source(mask_image, 'mask_image', 1, device)]
    sizes = [None if t is None else ((t.shape[1], t.shape[2]) if t.dtype == torch.uint8 else (t.shape[2], t.shape[3])) for t in srcs]
    for hw in sizes:
        if hw is not None:
            height, width = height or default_side(hw[0]), width or default_side(hw[1])
    out = []
    for t, hw, filt in zip(srcs, sizes, ('lanczos3', 'triangle')):
        box = None if t is None or resize == 'stretch' else crop_box(hw[0], hw[1], height, width)
        out.append(None if t is None else ops.image_resample(t, height, width, filt, box, clamp=True))
    return out[0], out[1], height, width


def inputs_cropped(image, image_latents, mask_image, strength, height, width, resize, mask_blur, padding_mask_crop, output_type, device,
                   default_size):
    """``padding_mask_crop``: the edit runs at the call's size on a window around the mask of an 8-bit photo of any size and ``_output``
    pastes it back (ops.image_paste).  -> (edit, height, width); ``edit.paste`` holds the photo's bytes on the GPU and the window."""
    pad = padding_mask_crop
    if isinstance(pad, bool) or not isinstance(pad, (int, np.integer)) or pad < 0:
        raise ValueError(f'`padding_mask_crop`: None or an integer >= 0 (pixels of the source around the mask), got {pad!r}')
    if resize is not None:
        raise ValueError('`padding_mask_crop` and `resize` exclude each other: the crop to the mask is the resize')
    if image_latents is not None:
        raise ValueError('`padding_mask_crop` takes `image`, not `image_latents`: the result is pasted into the image\'s own pixels')
    if image is None or mask_image is None:
        raise ValueError('`padding_mask_crop` needs `image` and `mask_image`')
    if output_type == 'latent':
        raise ValueError("`padding_mask_crop` returns the image at its own size: output_type 'pil', 'np' or 'pt', not 'latent'")
    pils = isinstance(image, (list, tuple)) and len(image) and all(hasattr(im, 'convert') for im in image)
    if not (pils or hasattr(image, 'convert') or (isinstance(image, np.ndarray) and image.dtype == np.uint8)):
        raise ValueError('`padding_mask_crop` needs 8-bit pixels, a PIL image (or a list) or a uint8 numpy array [B, H, W, 3]: the result '
                         f'keeps the image\'s own bytes; got {type(image).__name__}' + (f' {image.dtype}' if hasattr(image, 'dtype') else ''))
    check_strength(strength)
    height, width = resolve_size(height, width, default_size, ', got {height} x {width}')
    src = resize_source(image, 'image', 3, device)
    msrc = resize_source(mask_image, 'mask_image', 1, device)
    H, W = src.shape[1:3]
    mhw = tuple(msrc.shape[1:3]) if msrc.dtype == torch.uint8 else tuple(msrc.shape[2:])
    if mhw != (H, W):
        raise ValueError(f'`mask_image` is {mhw[0]} x {mhw[1]}, `image` is {H} x {W}: with `padding_mask_crop` the mask has the image\'s size')
    box = ops.mask_bbox(msrc).cpu()                     # 16 B per image: the one host round trip of the way in
    union = (int(box[:, 0].min()), int(box[:, 1].min()), int(box[:, 2].max()), int(box[:, 3].max()))
    window = mask_crop_window(union, H, W, height, width, int(pad))
    fbox = tuple(float(v) for v in window)
    img = ops.image_resample(src, height, width, 'lanczos3', fbox, clamp=True)
    mask = ops.image_resample(msrc, height, width, 'triangle', fbox, clamp=True)
    if mask_blur:
        mask = ops.mask_feather(mask, mask_blur)
    return EditRequest(img, None, mask, float(strength), paste=(src, window)), height, width


def edit_inputs(image, image_latents, mask_image, strength, height, width, resize, mask_blur, padding_mask_crop, output_type, color_fix,
                device, default_size):
    """The edit keywords of a call -> (edit, height, width), ``edit`` None on the text-to-image path; ``height`` / ``width`` come from the
    inputs when not given.  ``mask_blur`` feathers the image-resolution mask after any resize; ``color_fix`` is checked first."""
    check_color_fix(color_fix, image, mask_image, padding_mask_crop, output_type)
    mask_blur = float(mask_blur)
    if not 0.0 <= mask_blur < float('inf'):
        raise ValueError(f'`mask_blur` must be a finite sigma >= 0, got {mask_blur}')
    if padding_mask_crop is not None:
        return inputs_cropped(image, image_latents, mask_image, strength, height, width, resize, mask_blur, padding_mask_crop, output_type,
                              device, default_size)
    if image is None and image_latents is None:
        if mask_image is not None:
            raise ValueError('`mask_image` needs `image` or `image_latents`')
        if resize is not None or mask_blur:
            raise ValueError('`resize` and `mask_blur` need `image` (or `image_latents` with a `mask_image`)')
        return None, height, width
    if image is not None and image_latents is not None:
        raise ValueError('Cannot forward both `image` and `image_latents`.')
    check_strength(strength)
    if mask_blur and mask_image is None:
        raise ValueError('`mask_blur` needs a `mask_image`')
    if resize is not None:
        img, mask, height, width = inputs_resized(image, image_latents, mask_image, height, width, resize, device)
    else:
        img, mask, height, width = inputs_as_given(image, mask_image, height, width, default_size)
    if mask_blur:
        mask = ops.mask_feather(mask.to(device), mask_blur)
    if image_latents is not None and (image_latents.dim() != 3 or tuple(image_latents.shape[1:]) != ((height // 16) * (width // 16), 64)):
        raise ValueError(f'`image_latents`: need packed [B, {(height // 16) * (width // 16)}, 64] for {height} x {width}, '
                         f'got {tuple(image_latents.shape)}')
    return EditRequest(img, image_latents, mask, float(strength), color_fix=color_fix), height, width


# results ---------------------------------------------------------------------------------------------
def bytes_output(out: torch.Tensor, output_type) -> Any:
    """Result bytes, uint8 [B, H, W, 3] -> what the call returns: 'pt' the tensor itself, 'np' bytes / 255 as float32 [B, H, W, 3],
    anything else ('pil') images of the bytes."""
    if output_type == 'pt':
        return out
    arr = out.cpu().numpy()
    if output_type == 'np':
        return arr.astype(np.float32) / np.float32(255.0)
    from PIL import Image          # needed by 'pil' results alone
    return [Image.fromarray(x) for x in arr]
