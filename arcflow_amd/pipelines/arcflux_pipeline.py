"""ArcFluxPipeline -- drop-in for ``lakonlab.pipelines.arcflux_pipeline.ArcFluxPipeline``
(reference arcflux_pipeline.py:73-542): same constructor extras (``policy_type``, ``policy_kwargs``),
same ``__call__`` keywords and defaults, ``.images`` result, ``load_arcflow_adapter``.

What runs where: the denoising loop (arcflux_pipeline.py:457-510) is two C-ABI calls per step --
``afx_mmdit_forward`` and ``afx_arcflow_step`` -- on latents that never leave the packed token layout.
Prompt encoding and VAE decode are the rows SURVEY 8f marks "next": pass ``prompt_embeds`` /
``pooled_prompt_embeds`` (or attach HF text encoders) and use ``output_type='latent'`` unless a decoder
module is attached as ``pipe.vae``.

Beyond the reference: ``__call__`` of both pipelines takes the keyword-only ``image`` / ``image_latents``, ``strength``, ``mask_image`` and
``composite`` (image-to-image and inpainting); one more C-ABI call, ``afx_edit_blend``, forms the noised start and, with a
mask, follows every step.  Without them the call is the text-to-image path unchanged.  ``enhance(photo, prompt, scale=, tile=, overlap=,
strength=)`` of both pipelines reworks a photo of any size through that call on overlapping tiles.
"""
from __future__ import annotations

import glob
import json
import os
from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Optional, Union

import torch

from .. import ops
from ..engine import MMDiTEngine
from ..schedule import FlowMatchEulerDiscreteScheduler, calculate_shift, edit_raw_timesteps, mask_crop_window, mask_to_tokens, retrieve_raw_timesteps
from .arcflow_loader import ArcFlowLoaderMixin

POLICY_CLASSES = ('ArcFlow',)


@dataclass
class FluxPipelineOutput:
    images: Any


def load_transformer_dir(path: str):
    """Read ``<path>/config.json`` + every ``*.safetensors`` shard of a diffusers transformer folder."""
    from safetensors import safe_open
    with open(os.path.join(path, 'config.json')) as f:
        cfg = json.load(f)
    sd: Dict[str, torch.Tensor] = {}
    files = sorted(glob.glob(os.path.join(path, '*.safetensors')))
    if not files:
        raise EnvironmentError(f'no safetensors weights under {path}')
    for fn in files:
        with safe_open(fn, framework='pt', device='cpu') as f:
            for k in f.keys():
                sd[k] = f.get_tensor(k)
    return cfg, sd


class _PipelineBase(ArcFlowLoaderMixin):
    _family = 'flux'
    _output_class = FluxPipelineOutput
    vae_scale_factor = 8
    default_sample_size = 128

    def __init__(self, scheduler=None, vae=None, text_encoder=None, tokenizer=None, transformer=None,
                 policy_type: str = 'ArcFlow', policy_kwargs: Optional[Dict[str, Any]] = None):
        assert policy_type in POLICY_CLASSES, \
            f'Invalid policy: {policy_type}. Supported policies are {list(POLICY_CLASSES)}.'
        self.policy_type = policy_type
        self.policy_kwargs = policy_kwargs or {}
        self.scheduler = scheduler or FlowMatchEulerDiscreteScheduler(shift=3.0, use_dynamic_shifting=True)
        self.vae, self.text_encoder, self.tokenizer = vae, text_encoder, tokenizer
        self.transformer = transformer
        self._base_state_dict: Dict[str, torch.Tensor] = {}
        self._transformer_config: Dict[str, Any] = {}
        self._device = torch.device('cuda')
        self._interrupt = False
        self._num_timesteps = 0
        self._current_timestep = None

    # diffusers-style plumbing -------------------------------------------------------------------
    def to(self, device=None, *a, **k):
        if device is not None and torch.device(device).type != 'cuda':
            raise RuntimeError('arcflow_amd pipelines run on the GPU only (no CPU fallback)')
        return self

    def enable_model_cpu_offload(self, *a, **k):      # 288 GB HBM: nothing to offload
        return self

    def maybe_free_model_hooks(self):
        pass

    @property
    def interrupt(self):
        return self._interrupt

    @property
    def num_timesteps(self):
        return self._num_timesteps

    @property
    def _execution_device(self):
        return self._device

    def _retrieve_timesteps(self, raw, device, image_seq_len):
        mu = calculate_shift(image_seq_len, self.scheduler.config.get('base_image_seq_len', 256),
                             self.scheduler.config.get('max_image_seq_len', 4096),
                             self.scheduler.config.get('base_shift', 0.5), self.scheduler.config.get('max_shift', 1.15))
        self.scheduler.set_timesteps(sigmas=raw, device=device, mu=mu)
        return self.scheduler.timesteps

    def _prepare_latents(self, batch, height, width, generator, latents):
        hp, wp = int(height) // (self.vae_scale_factor * 2), int(width) // (self.vae_scale_factor * 2)
        if latents is not None:
            return latents.to(self._device, torch.float32), hp, wp
        shape = (batch, 16, 2 * hp, 2 * wp)
        if isinstance(generator, list):
            noise = torch.cat([torch.randn((1,) + shape[1:], generator=g, device=g.device if hasattr(g, 'device') else 'cpu',
                                           dtype=torch.float32).to(self._device) for g in generator])
        else:
            gdev = generator.device if generator is not None else self._device
            noise = torch.randn(shape, generator=generator, device=gdev, dtype=torch.float32).to(self._device)
        # FLUX packing: [B,16,2hp,2wp] -> [B, hp*wp, 64], channel = c*4 + ph*2 + pw (arcflux_pipeline.py:162-175)
        packed = noise.view(batch, 16, hp, 2, wp, 2).permute(0, 2, 4, 1, 3, 5).reshape(batch, hp * wp, 64)
        return packed.contiguous(), hp, wp

    # image editing: image-to-image and inpainting ---------------------------------------------------------
    @staticmethod
    def _images01(image, name='image', channels=3) -> torch.Tensor:
        """A torch [B, C, H, W] / [C, H, W], numpy [B, H, W, C] / [H, W, C], PIL image or list of PIL images in [0, 1] (PIL: 8 bit) ->
        fp32 [B, C, H, W] in [0, 1].  With channels = 1 (a mask) the channel axis may be missing: [B, H, W] / [H, W]."""
        import numpy as np

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

    @staticmethod
    def _default_side(n: int) -> int:
        """The call's side for a source side of ``n`` pixels under ``resize``: the nearest multiple of 16 (ties up), at least 16."""
        return max(16, 16 * ((int(n) + 8) // 16))

    @staticmethod
    def _crop_box(src_h: int, src_w: int, height: int, width: int):
        """(left, upper, right, lower) of the largest centred window of a ``src_h`` x ``src_w`` image with the aspect ratio ``width`` :
        ``height``, in source pixels; fractional.  An image that already has that ratio gives the whole image."""
        if src_w * height > src_h * width:                  # the source is wider: full height, centred columns
            cw = src_h * width / height
            return ((src_w - cw) / 2, 0.0, (src_w + cw) / 2, float(src_h))
        if src_w * height < src_h * width:
            ch = src_w * height / width
            return (0.0, (src_h - ch) / 2, float(src_w), (src_h + ch) / 2)
        return (0.0, 0.0, float(src_w), float(src_h))

    def _resize_source(self, image, name, channels) -> torch.Tensor:
        """``image`` on the GPU as ops.image_resample reads it: PIL images and uint8 numpy arrays as uint8 [B, H, W, C] (read as x / 255, 3 B per
        pixel over the bus), everything else as ``_images01`` gives it, fp32 [B, C, H, W].  NOTE the one difference to ``resize=None``: there
        ``_images01`` takes a uint8 numpy array as values already in [0, 1], undivided; here it is 8-bit pixels.  A uint8 torch tensor raises."""
        import numpy as np
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
            return self._images01(image, name, channels).to(self._device).contiguous()
        return torch.from_numpy(np.ascontiguousarray(arr)).to(self._device)

    def _edit_inputs_resized(self, image, image_latents, mask_image, height, width, resize):
        """The ``resize`` branch of ``_edit_inputs``: -> (img, mask, height, width) with img / mask fp32 [B, C, height, width] on the GPU."""
        if resize not in ('stretch', 'crop'):
            raise ValueError(f"`resize`: None, 'stretch' or 'crop', got {resize!r}")
        if image_latents is not None and mask_image is None:
            raise ValueError('`resize` with `image_latents` and no `mask_image` has nothing to resize: latents are not resampled')
        if (height and height % 16) or (width and width % 16):
            raise ValueError(f'`height` and `width` have to be divisible by 16, got {height} x {width}')
        srcs = [None if image is None else self._resize_source(image, 'image', 3),
                None if mask_image is None else self._resize_source(mask_image, 'mask_image', 1)]
        sizes = [None if t is None else ((t.shape[1], t.shape[2]) if t.dtype == torch.uint8 else (t.shape[2], t.shape[3])) for t in srcs]
        for hw in sizes:
            if hw is not None:
                height, width = height or self._default_side(hw[0]), width or self._default_side(hw[1])
        out = []
        for t, hw, filt in zip(srcs, sizes, ('lanczos3', 'triangle')):
            box = None if t is None or resize == 'stretch' else self._crop_box(hw[0], hw[1], height, width)
            out.append(None if t is None else ops.image_resample(t, height, width, filt, box, clamp=True))
        return out[0], out[1], height, width

    def _edit_inputs_cropped(self, image, image_latents, mask_image, strength, height, width, resize, mask_blur, padding_mask_crop, output_type):
        """The ``padding_mask_crop`` branch of ``_edit_inputs``: the edit runs at the call's size on a window around the mask of an 8-bit
        photo of any size and ``_finish`` pastes it back (ops.image_paste).  -> (edit, height, width); ``edit['paste']`` holds the photo's
        bytes on the GPU (uint8 [B, H, W, 3]) and the window (x0, y0, x1, y1)."""
        import numpy as np
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
        if not 0.0 < float(strength) <= 1.0:
            raise ValueError(f'`strength` must be in (0, 1], got {strength}')
        height = height or self.default_sample_size * self.vae_scale_factor
        width = width or self.default_sample_size * self.vae_scale_factor
        if height % 16 or width % 16:
            raise ValueError(f'`height` and `width` have to be divisible by 16, got {height} x {width}')
        src = self._resize_source(image, 'image', 3)
        msrc = self._resize_source(mask_image, 'mask_image', 1)
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
        return dict(image=img, image_latents=None, mask=mask, strength=float(strength), paste=dict(source=src, window=window)), height, width

    @staticmethod
    def _check_color_fix(color_fix, image, mask_image, padding_mask_crop, output_type) -> None:
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

    def _edit_inputs(self, image, image_latents, mask_image, strength, height, width, resize=None, mask_blur=0.0, padding_mask_crop=None,
                     output_type=None, color_fix=None):
        """Host-side half of the edit arguments: -> (edit, height, width), ``edit`` None on the text-to-image path.  Normalises ``image`` and
        ``mask_image`` to fp32 [B, C, H, W], takes ``height`` / ``width`` from them when not given.  ``resize`` None: nothing is resized, an
        input of another size raises.  'stretch' / 'crop': both are resampled to the call's size on the GPU (ops.image_resample: the image
        with Lanczos-3, the mask with the triangle filter, soft values kept), 'crop' from the largest centred window of the call's aspect
        ratio; ``height`` / ``width`` then default to the source's sides rounded to multiples of 16.  ``mask_blur`` > 0: the
        image-resolution mask is feathered by a Gaussian of that sigma in output pixels (ops.mask_feather) after any resize.
        ``padding_mask_crop`` (an integer; with it ``output_type`` is checked too): ``_edit_inputs_cropped``.  ``color_fix`` is checked
        first (``_check_color_fix``) and kept in ``edit['color_fix']`` for ``_output``."""
        self._check_color_fix(color_fix, image, mask_image, padding_mask_crop, output_type)
        mask_blur = float(mask_blur)
        if not 0.0 <= mask_blur < float('inf'):
            raise ValueError(f'`mask_blur` must be a finite sigma >= 0, got {mask_blur}')
        if padding_mask_crop is not None:
            return self._edit_inputs_cropped(image, image_latents, mask_image, strength, height, width, resize, mask_blur, padding_mask_crop,
                                             output_type)
        if image is None and image_latents is None:
            if mask_image is not None:
                raise ValueError('`mask_image` needs `image` or `image_latents`')
            if resize is not None or mask_blur:
                raise ValueError('`resize` and `mask_blur` need `image` (or `image_latents` with a `mask_image`)')
            return None, height, width
        if image is not None and image_latents is not None:
            raise ValueError('Cannot forward both `image` and `image_latents`.')
        if not 0.0 < float(strength) <= 1.0:
            raise ValueError(f'`strength` must be in (0, 1], got {strength}')
        if mask_blur and mask_image is None:
            raise ValueError('`mask_blur` needs a `mask_image`')
        if resize is not None:
            img, mask, height, width = self._edit_inputs_resized(image, image_latents, mask_image, height, width, resize)
        else:
            img, mask, height, width = self._edit_inputs_as_given(image, mask_image, height, width)
        if mask_blur:
            mask = ops.mask_feather(mask.to(self._device), mask_blur)
        if image_latents is not None and (image_latents.dim() != 3 or tuple(image_latents.shape[1:]) != ((height // 16) * (width // 16), 64)):
            raise ValueError(f'`image_latents`: need packed [B, {(height // 16) * (width // 16)}, 64] for {height} x {width}, '
                             f'got {tuple(image_latents.shape)}')
        return dict(image=img, image_latents=image_latents, mask=mask, strength=float(strength), color_fix=color_fix), height, width

    def _edit_inputs_as_given(self, image, mask_image, height, width):
        """The ``resize=None`` branch of ``_edit_inputs``: -> (img, mask, height, width); every input must have the call's size."""
        img = None if image is None else self._images01(image)
        mask = None if mask_image is None else self._images01(mask_image, 'mask_image', 1)
        for t in (img, mask):
            if t is not None:
                height, width = height or t.shape[2], width or t.shape[3]
        height = height or self.default_sample_size * self.vae_scale_factor
        width = width or self.default_sample_size * self.vae_scale_factor
        if height % 16 or width % 16:
            raise ValueError(f'`height` and `width` have to be divisible by 16, got {height} x {width} (an edit resizes nothing)')
        for t, name in ((img, 'image'), (mask, 'mask_image')):
            if t is not None and tuple(t.shape[2:]) != (height, width):
                raise ValueError(f'`{name}` is {t.shape[2]} x {t.shape[3]}, the call is {height} x {width}: an edit resizes nothing')
        return img, mask, height, width

    def _edit_prepare(self, edit, B, hp, wp):
        """Device-side half: batch checks, the encode of ``image`` (posterior mode, packed), the mask per latent pixel."""
        device = self._device
        for name in ('image', 'image_latents', 'mask'):
            t = edit[name]
            if t is not None and t.shape[0] not in (1, B):
                raise ValueError(f'`{"mask_image" if name == "mask" else name}` has batch {t.shape[0]}, the call has {B} (a batch of 1 broadcasts)')
        if edit['image'] is not None:
            encoder = getattr(self.vae, 'encoder', None)
            if encoder is None:
                raise RuntimeError('`image=` needs a VAE encoder (pipe.vae.encoder: a snapshot with encoder.* weights); without one pass '
                                   '`image_latents=`, the packed latents of the image')
            x0 = encoder.encode_images01(edit['image'], sample=False, packed=True)
        else:
            x0 = edit['image_latents'].to(device, torch.float32)
        edit['x0'] = x0.expand(B, -1, -1).contiguous()
        if edit['mask'] is not None:
            edit['mask_tokens'] = mask_to_tokens(edit['mask'].to(device), hp, wp).expand(B, -1, -1).contiguous()
        return edit

    def _composite(self, image, edit, composite, padding_mask_crop=None):
        """Paste the original pixels back outside the mask: m decoded + (1 - m) original, in the decoder's range [-1, 1] and dtype.  With
        ``padding_mask_crop`` nothing happens here: the blend is part of the paste into the photo (``_paste``)."""
        if not composite or edit is None or edit['image'] is None or edit['mask'] is None or padding_mask_crop is not None:
            return image
        m = edit['mask'].to(image.device, torch.float32)
        orig = (edit['image'].to(image.device) * 2 - 1).to(image.dtype).to(torch.float32)
        return (m * image.to(torch.float32) + (1 - m) * orig).to(image.dtype)

    def _denoise_edit(self, noise, edit, num_inference_steps, total_substeps, timestep_ratio, fwd, callback_on_step_end,
                      callback_on_step_end_tensor_inputs, prompt_embeds, prepare=None):
        """``_denoise`` from a noised image: ``num_inference_steps`` student steps over the raw time [strength, 0], started on
        (1 - sigma) x0 + sigma noise; with a mask, after every step the unmasked latent pixels are put back on the source's own
        trajectory at the sigma the step landed on, with the same noise every time (afx_edit_blend: blend + the next forward's bf16 copy)."""
        device = self._device
        x0, mask = edit['x0'], edit.get('mask_tokens')
        B = x0.shape[0]
        if tuple(noise.shape) != tuple(x0.shape):
            raise ValueError(f'`latents` (the start noise) is {tuple(noise.shape)}, the image latents are {tuple(x0.shape)}')
        noise = noise.contiguous()
        raw, per_step, total = edit_raw_timesteps(num_inference_steps, total_substeps, timestep_ratio, edit['strength'])
        timesteps = self._retrieve_timesteps(raw, device, x0.shape[1])
        assert len(timesteps) == total
        self._num_timesteps = total
        self.scheduler.set_begin_index(0)
        ntt = self.scheduler.config.num_train_timesteps
        ts_host = timesteps.float().cpu().tolist()
        starts = [sum(per_step[:i]) for i in range(num_inference_steps)]
        prepared = bool(prepare([ts_host[j] / 1000.0 for j in starts])) if prepare is not None and not self.interrupt else False
        latents, lat16 = ops.edit_blend(None, x0, noise, None, torch.full((B,), ts_host[0] / ntt, device=device, dtype=torch.float32))
        tid = 0
        for i in range(num_inference_steps):
            if self.interrupt:
                continue
            t_src = ts_host[tid]
            sigma_src = t_src / ntt
            self._current_timestep = t_src
            out = fwd(lat16 if lat16 is not None else latents.to(torch.bfloat16), torch.full((B,), t_src / 1000.0, device=device),
                      prompt_embeds, i if prepared else None)
            tid += per_step[i]
            sigma_end = (ts_host[tid] / ntt) if tid < len(ts_host) else 0.0
            latents = ops.arcflow_step(latents, out.means, out.logweights, out.loggammas, sigma_src, sigma_src, sigma_end, eps=1e-4)
            lat16 = None
            if mask is not None:
                latents, lat16 = ops.edit_blend(latents, x0, noise if sigma_end > 0.0 else None, mask,
                                                torch.full((B,), sigma_end, device=device, dtype=torch.float32), out=latents, out_bf16=lat16)
            if callback_on_step_end is not None:
                local = dict(latents=latents, prompt_embeds=prompt_embeds)
                cb = callback_on_step_end(self, i, torch.tensor(t_src, device=device),
                                          {k: local[k] for k in callback_on_step_end_tensor_inputs})
                latents, lat16 = cb.pop('latents', latents), None          # the callback may have changed them: the kernel's bf16 copy is dropped
                prompt_embeds = cb.pop('prompt_embeds', prompt_embeds)
        self._current_timestep = None
        return latents

    def _denoise(self, latents, hp, wp, num_inference_steps, total_substeps, timestep_ratio, fwd,
                 callback_on_step_end, callback_on_step_end_tensor_inputs, prompt_embeds, prepare=None, edit=None):
        if edit is not None:
            return self._denoise_edit(latents, edit, num_inference_steps, total_substeps, timestep_ratio, fwd, callback_on_step_end,
                                      callback_on_step_end_tensor_inputs, prompt_embeds, prepare)
        device = self._device
        raw, per_step, total = retrieve_raw_timesteps(num_inference_steps, total_substeps, timestep_ratio)
        timesteps = self._retrieve_timesteps(raw, device, latents.shape[1])
        assert len(timesteps) == total
        self._num_timesteps = total
        self.scheduler.set_begin_index(0)
        ntt = self.scheduler.config.num_train_timesteps
        ts_host = timesteps.float().cpu().tolist()          # 128 floats, once per call
        # every step's source timestep is known here: the AdaLN modulation vectors of ALL steps (functions of t, guidance and the
        # pooled text only) come out of one pass over the stacked modulation matrix instead of one pass per transformer call
        starts = [sum(per_step[:i]) for i in range(num_inference_steps)]
        prepared = bool(prepare([ts_host[j] / 1000.0 for j in starts])) if prepare is not None and not self.interrupt else False
        tid = 0
        for i in range(num_inference_steps):
            if self.interrupt:
                continue
            t_src = ts_host[tid]
            sigma_src = t_src / ntt
            self._current_timestep = t_src
            out = fwd(latents.to(torch.bfloat16), torch.full((latents.shape[0],), t_src / 1000.0, device=device), prompt_embeds,
                      i if prepared else None)
            tid += per_step[i]
            sigma_end = (ts_host[tid] / ntt) if tid < len(ts_host) else 0.0
            latents = ops.arcflow_step(latents, out.means, out.logweights, out.loggammas,
                                       sigma_src, sigma_src, sigma_end, eps=1e-4)
            if callback_on_step_end is not None:
                local = dict(latents=latents, prompt_embeds=prompt_embeds)
                cb = callback_on_step_end(self, i, torch.tensor(t_src, device=device),
                                          {k: local[k] for k in callback_on_step_end_tensor_inputs})
                latents = cb.pop('latents', latents)
                # the reference also takes back a modified conditioning (arcflux_pipeline.py:519 pops "prompt_embeds")
                prompt_embeds = cb.pop('prompt_embeds', prompt_embeds)
        self._current_timestep = None
        return latents

    # teacher sampling ------------------------------------------------------------------------------
    def _teacher_engine(self) -> MMDiTEngine:
        """The ``teacher_head=True`` engine of the plain snapshot: the pipeline's own transformer until an adapter is loaded,
        afterwards a second engine built once from the kept base weights."""
        if self.transformer is not None and self.transformer.teacher_head:
            return self.transformer
        if getattr(self, '_teacher', None) is None:
            if 'proj_out.weight' not in self._base_state_dict:
                raise RuntimeError('sample_teacher() needs the plain snapshot\'s velocity head: this pipeline holds an ArcFlow student only and '
                                   'no base `proj_out` was kept (build it with from_pretrained(<plain snapshot>), or from a state dict that '
                                   'contains proj_out.weight / proj_out.bias)')
            self._teacher = self._build_engine(teacher_head=True)
            self._teacher.load_state_dict(self._base_state_dict)
        return self._teacher

    def _euler_scheduler_kwargs(self) -> Dict[str, Any]:
        """The pipeline scheduler's shift settings in FlowEulerODEScheduler's names (diffusers counts ``image_seq_len`` in tokens)."""
        c = self.scheduler.config
        return dict(num_train_timesteps=c.get('num_train_timesteps', 1000), shift=c.get('shift', 1.0),
                    use_dynamic_shifting=bool(c.get('use_dynamic_shifting', False)), base_seq_len=c.get('base_image_seq_len', 256),
                    max_seq_len=c.get('max_image_seq_len', 4096), base_logshift=c.get('base_shift', 0.5), max_logshift=c.get('max_shift', 1.15),
                    terminal_sigma=c.get('shift_terminal') or None)

    def _sample_teacher(self, cond, batch, height, width, num_inference_steps, guidance_scale, true_cfg_scale, generator, latents,
                        guidance_interval, orthogonal_guidance, sampler='FlowEulerODE', h=None, edit=None, solver_order=None, solver_type=None):
        """-> (latents, hp, wp, edit).  ``edit`` (from ``_edit_inputs``; None: from pure noise) is prepared as ``__call__`` prepares it and
        reaches TeacherSampler as ``x0`` / ``mask`` / ``strength``; ``latents`` / ``generator`` give the start noise either way."""
        from ..teacher import TeacherSampler
        engine = self._teacher_engine()
        latents, hp, wp = self._prepare_latents(batch, height, width, generator, latents)
        cond = dict(cond, hp=hp, wp=wp)
        kw = {}
        if edit is not None:
            edit = self._edit_prepare(edit, batch, hp, wp)
            if tuple(latents.shape) != tuple(edit['x0'].shape):
                raise ValueError(f'`latents` (the start noise) is {tuple(latents.shape)}, the image latents are {tuple(edit["x0"].shape)}')
            kw = dict(x0=edit['x0'], mask=edit.get('mask_tokens'), strength=edit['strength'])
        solver = {k: v for k, v in dict(h=h, solver_order=solver_order, solver_type=solver_type).items() if v is not None}       # the scheduler refuses a keyword that is not its own
        sampler = TeacherSampler(engine, num_inference_steps, guidance_scale=true_cfg_scale, distilled_guidance=guidance_scale,
                                 guidance_interval=guidance_interval, orthogonal_guidance=orthogonal_guidance, tokens_as_seq_len=True,
                                 sampler=sampler, **solver, **self._euler_scheduler_kwargs())
        self._num_timesteps = num_inference_steps
        return sampler(cond, latents, generator=generator, **kw), hp, wp, edit          # (the generator's stream continues from the start noise into FlowSDE's step draws)

    def _unpack(self, latents, hp, wp):
        b = latents.shape[0]
        return latents.view(b, hp, wp, 16, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(b, 16, 2 * hp, 2 * wp)

    def _postprocess(self, image, output_type):
        if output_type == 'pt':
            return image
        img = (image.float() / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).cpu().numpy()
        if output_type == 'np':
            return img
        from PIL import Image
        return [Image.fromarray((x * 255).round().astype('uint8')) for x in img]

    def _paste(self, image, edit, composite) -> torch.Tensor:
        """The decoded edit [B, 3, h, w] in [-1, 1] back into the photo it was cut from -> uint8 [B, H, W, 3] on the GPU (ops.image_paste):
        the window takes the edit resampled to its size, blended with the photo by the call's mask (``composite`` off: the whole window is
        the edit); every other byte is the photo's own."""
        paste = edit['paste']
        src = paste['source']
        if src.shape[0] != image.shape[0]:
            if src.shape[0] != 1:
                raise ValueError(f'`image` has batch {src.shape[0]}, the call has {image.shape[0]} (a batch of 1 broadcasts)')
            src = src.expand(image.shape[0], -1, -1, -1).contiguous()
        return ops.image_paste(image.to(torch.float32).contiguous(), edit['mask'] if composite else None, src, paste['window'])

    def _output(self, image, edit, composite, output_type, padding_mask_crop=None):
        """The decoded image -> what the call returns.  With ``padding_mask_crop``: the photo's size, from the bytes of ``_paste`` ('pt': the
        uint8 [B, H, W, 3] device tensor, 'np': bytes / 255 as float32 [B, H, W, 3], 'pil': images of the bytes).  With ``color_fix`` the
        decoded image is first matched to the call's ``image`` (ops.color_fix) and is float32 from there on."""
        if padding_mask_crop is None:
            if edit is not None and edit.get('color_fix') is not None:
                if image.dtype not in (torch.float32, torch.bfloat16):
                    image = image.to(torch.float32)
                image = ops.color_fix(image.contiguous(), edit['image'].to(image.device, torch.float32).contiguous(), edit['color_fix'])
            return self._postprocess(self._composite(image, edit, composite), output_type)
        out = self._paste(image, edit, composite)
        if output_type == 'pt':
            return out
        arr = out.cpu().numpy()
        if output_type == 'np':
            import numpy as np
            return arr.astype(np.float32) / np.float32(255.0)
        from PIL import Image
        return [Image.fromarray(x) for x in arr]

    # tiled image-to-image: a photo of any size reworked at its own (or a larger) size -------------------------
    def _enhance_conditioning(self, prompt, **conditioning) -> Dict[str, Any]:
        """The family's half of ``enhance``: encode the prompt once -> the conditioning keywords of ``__call__`` for a batch of 1."""
        raise NotImplementedError

    @torch.inference_mode()
    def enhance(self, image, prompt: Union[str, List[str]] = None, *, scale: float = 1.0, tile: int = 1024, overlap: int = 128,
                strength: float = 0.3, tile_batch: int = 4, num_inference_steps: int = 2, timestep_ratio: float = 1.0,
                total_substeps: int = 128, generator: Optional[torch.Generator] = None, latents: Optional[torch.Tensor] = None,
                output_type: Optional[str] = 'pil', return_dict: bool = True, color_fix: Optional[str] = None, **conditioning):
        """Rework one photo of any size at its own size, or ``scale`` times it (the "tile upscale / detail pass"): the photo is resampled
        to the canvas H' = round(H scale), W' = round(W scale) with Lanczos-3 (``ops.image_resample``; at scale 1 the source's values
        exactly), the canvas is cut into overlapping tiles of at most ``tile`` pixels a side (``schedule.tile_plan``: sides multiples of
        16, neighbours sharing at least ``overlap`` pixels; ``ops.tiles_cut``), the tiles go in order, ``tile_batch`` at a time, through
        this pipeline's own image-to-image call at ``strength`` -- ``self(image=tiles, strength=..., latents=noise, output_type='pt', ...)``,
        so the result is by construction the merge of ordinary calls --, and the decoded tiles are cross-faded into bytes with one rounding
        (``ops.tiles_merge``).  Both sides of the canvas must be at least 16 pixels.

        ``image``: one picture in any form ``resize=`` takes (a PIL image, a uint8 numpy array [H, W, 3], a float tensor [3, H, W] in
        [0, 1]); a batch other than 1 raises.  The prompt is encoded once; the conditioning keywords are the family's, as on ``__call__``
        (FLUX: ``prompt_embeds``, ``pooled_prompt_embeds``, ``guidance_scale``, ``max_sequence_length``; Qwen-Image: ``prompt_embeds``,
        ``prompt_embeds_mask``, ``max_sequence_length``).  The tiles' start noise is ``latents`` [T, (th / 16) (tw / 16), 64] if given, else
        one draw of that shape from ``generator``.  The result has the canvas' size, as with ``padding_mask_crop``: 'pt' the uint8
        [1, H', W', 3] device tensor, 'np' bytes / 255 as float32, 'pil' images of the bytes; 'latent' raises.

        ``color_fix`` ('adain' or 'wavelet'; None: off) is handed to that call: every decoded tile is matched to the canvas tile it was cut
        from (``ops.color_fix``) before the merge, so a tile cannot drift in colour or brightness on its own.

        Out of scope: the teacher (``sample_teacher``), masks, one noise field shared by overlapping tiles (every tile has its own), lists
        of photos, and equal bits for different ``tile_batch`` values (a batched forward is not promised to equal single ones)."""
        from ..schedule import tile_plan
        if output_type == 'latent':
            raise ValueError("`enhance` returns the image at the canvas' size: output_type 'pil', 'np' or 'pt', not 'latent'")
        self._check_color_fix(color_fix, image, None, None, output_type)
        if isinstance(tile_batch, bool) or int(tile_batch) != tile_batch or tile_batch < 1:
            raise ValueError(f'`tile_batch`: an integer >= 1, got {tile_batch!r}')
        if not 0.0 < float(strength) <= 1.0:
            raise ValueError(f'`strength` must be in (0, 1], got {strength}')
        if not 0.0 < float(scale) < float('inf'):
            raise ValueError(f'`scale` must be positive and finite, got {scale}')
        src = self._resize_source(image, 'image', 3)
        B, H, W = (src.shape[0], src.shape[1], src.shape[2]) if src.dtype == torch.uint8 else (src.shape[0], src.shape[2], src.shape[3])
        if B != 1:
            raise ValueError(f'`image`: `enhance` takes one picture, got a batch of {B}')
        Hc, Wc = round(H * float(scale)), round(W * float(scale))
        if min(Hc, Wc) < 16:
            raise ValueError(f'the canvas is {Hc} x {Wc} ({H} x {W} at scale {scale}): both sides must be at least 16 pixels')
        plan = tile_plan(Hc, Wc, tile, overlap)
        T, hp, wp = plan.T, plan.th // 16, plan.tw // 16
        if latents is not None and tuple(latents.shape) != (T, hp * wp, 64):
            raise ValueError(f'`latents` (the tiles\' start noise): need [{T}, {hp * wp}, 64] for {T} tiles of {plan.th} x {plan.tw}, '
                             f'got {tuple(latents.shape)}')
        cond = self._enhance_conditioning(prompt, **conditioning)
        noise, _, _ = self._prepare_latents(T, plan.th, plan.tw, generator, latents)
        tiles = ops.tiles_cut(ops.image_resample(src, Hc, Wc, 'lanczos3', clamp=True), plan)
        decoded = torch.empty_like(tiles)
        for i in range(0, T, int(tile_batch)):
            n = min(int(tile_batch), T - i)
            decoded[i:i + n] = self(image=tiles[i:i + n], strength=strength, latents=noise[i:i + n], num_images_per_prompt=n,
                                    num_inference_steps=num_inference_steps, timestep_ratio=timestep_ratio, total_substeps=total_substeps,
                                    output_type='pt', color_fix=color_fix, **cond).images
        out = ops.tiles_merge(decoded, plan)[None]
        if output_type != 'pt':
            arr = out.cpu().numpy()
            if output_type == 'np':
                import numpy as np
                out = arr.astype(np.float32) / np.float32(255.0)
            else:
                from PIL import Image
                out = [Image.fromarray(x) for x in arr]
        return self._output_class(images=out) if return_dict else (out,)


class ArcFluxPipeline(_PipelineBase):
    r"""Policy-based FLUX pipeline, 2-NFE capable (reference arcflux_pipeline.py:73)."""
    _family = 'flux'

    def __init__(self, scheduler=None, vae=None, text_encoder=None, tokenizer=None, text_encoder_2=None,
                 tokenizer_2=None, transformer=None, image_encoder=None, feature_extractor=None,
                 policy_type: str = 'ArcFlow', policy_kwargs: Optional[Dict[str, Any]] = None):
        super().__init__(scheduler, vae, text_encoder, tokenizer, transformer, policy_type, policy_kwargs)
        self.text_encoder_2, self.tokenizer_2 = text_encoder_2, tokenizer_2

    # construction -----------------------------------------------------------------------------------
    def _build_engine(self, num_gaussians=16, logweights_channels=4, teacher_head=False) -> MMDiTEngine:
        c = self._transformer_config
        return MMDiTEngine('flux', c.get('num_layers', 19), c.get('num_single_layers', 38),
                           heads=c.get('num_attention_heads', 24), head_dim=c.get('attention_head_dim', 128),
                           in_channels=c.get('in_channels', 64), joint_dim=c.get('joint_attention_dim', 4096),
                           pooled_dim=c.get('pooled_projection_dim', 768), guidance_embeds=c.get('guidance_embeds', True),
                           num_gaussians=num_gaussians, logweights_channels=logweights_channels,
                           teacher_head=teacher_head, axes_dims=tuple(c.get('axes_dims_rope', (16, 56, 56))))

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, torch_dtype=torch.bfloat16, **kwargs):
        """Local diffusers snapshot (``transformer/``, ``scheduler/`` ...).  No network in this build."""
        if torch_dtype not in (torch.bfloat16, None):
            raise ValueError('the MI355X engine computes in bf16')
        root = pretrained_model_name_or_path
        if not os.path.isdir(os.path.join(root, 'transformer')):
            raise EnvironmentError(f'{root}/transformer not found: pass a local FLUX.1-dev snapshot directory')
        cfg, sd = load_transformer_dir(os.path.join(root, 'transformer'))
        sched_cfg = {}
        sp = os.path.join(root, 'scheduler', 'scheduler_config.json')
        if os.path.exists(sp):
            sched_cfg = json.load(open(sp))
        pipe = cls(scheduler=FlowMatchEulerDiscreteScheduler.from_config(sched_cfg))
        pipe._transformer_config, pipe._base_state_dict = cfg, sd
        if os.path.isdir(os.path.join(root, 'vae')):          # AutoencoderKL decoder on the HIP engine
            from ..vae import AutoencoderKLDecoder
            vcfg, vsd = load_transformer_dir(os.path.join(root, 'vae'))
            pipe.vae = AutoencoderKLDecoder(vsd, tuple(vcfg.get('block_out_channels', (128, 256, 512, 512))),
                                            vcfg.get('norm_num_groups', 32), vcfg.get('layers_per_block', 2),
                                            vcfg.get('scaling_factor', 0.3611), vcfg.get('shift_factor', 0.1159))
            if any(k.startswith('encoder.') for k in vsd):     # full VAE snapshot: pipe.vae.encode(...) as on the reference's PretrainedVAE
                from ..vae import AutoencoderKLEncoder
                pipe.vae.encoder = AutoencoderKLEncoder(vsd, tuple(vcfg.get('block_out_channels', (128, 256, 512, 512))),
                                                        vcfg.get('norm_num_groups', 32), vcfg.get('layers_per_block', 2),
                                                        vcfg.get('scaling_factor', 0.3611), vcfg.get('shift_factor', 0.1159))
        if os.path.isdir(os.path.join(root, 'text_encoder')) and os.path.isdir(os.path.join(root, 'text_encoder_2')):
            from ..text_encoders import load_clip_text_encoder, load_t5_encoder       # prompt encoders on the HIP engine
            pipe.text_encoder = load_clip_text_encoder(os.path.join(root, 'text_encoder'))
            pipe.text_encoder_2 = load_t5_encoder(os.path.join(root, 'text_encoder_2'))
            from transformers import AutoTokenizer                                      # tokenisation is host-side plumbing
            pipe.tokenizer = AutoTokenizer.from_pretrained(os.path.join(root, 'tokenizer'))
            pipe.tokenizer_2 = AutoTokenizer.from_pretrained(os.path.join(root, 'tokenizer_2'))
        if 'proj_out.weight' in sd:          # plain FLUX: usable as the teacher until an adapter is loaded
            pipe.transformer = pipe._build_engine(teacher_head=True)
            pipe.transformer.load_state_dict(sd)
        return pipe

    @classmethod
    def from_state_dict(cls, transformer_config: Dict[str, Any], state_dict: Dict[str, torch.Tensor],
                        scheduler=None, student: bool = True, **kw):
        """Build from an in-memory diffusers-keyed state dict (tests, synthetic weights)."""
        pipe = cls(scheduler=scheduler, **kw)
        pipe._transformer_config, pipe._base_state_dict = dict(transformer_config), state_dict
        pipe.transformer = pipe._build_engine(transformer_config.get('num_gaussians', 16),
                                              transformer_config.get('logweights_channels', 4), teacher_head=not student)
        pipe.transformer.load_state_dict(state_dict)
        return pipe

    # prompt encoding (text encoders are a "next" row) -------------------------------------
    def encode_prompt(self, prompt, prompt_2, prompt_embeds, pooled_prompt_embeds, device, num_images_per_prompt,
                      max_sequence_length):
        if prompt_embeds is None:
            if self.text_encoder is None or self.text_encoder_2 is None:
                raise RuntimeError('no text encoders attached: pass prompt_embeds and pooled_prompt_embeds')
            prompt = [prompt] if isinstance(prompt, str) else prompt
            prompt_2 = prompt if prompt_2 is None else ([prompt_2] if isinstance(prompt_2, str) else prompt_2)
            from ..text_encoders import CLIPTextEncoder, T5Encoder
            with torch.no_grad():      # diffusers FluxPipeline._get_clip_prompt_embeds / _get_t5_prompt_embeds: no attention masks
                ids = self.tokenizer(prompt, padding='max_length', max_length=77, truncation=True, return_tensors='pt').input_ids
                if isinstance(self.text_encoder, CLIPTextEncoder):
                    pooled_prompt_embeds = self.text_encoder(ids)[1]
                else:
                    pooled_prompt_embeds = self.text_encoder(ids.to(self.text_encoder.device)).pooler_output
                ids2 = self.tokenizer_2(prompt_2, padding='max_length', max_length=max_sequence_length, truncation=True,
                                        return_tensors='pt').input_ids
                if isinstance(self.text_encoder_2, T5Encoder):
                    prompt_embeds = self.text_encoder_2(ids2)
                else:
                    prompt_embeds = self.text_encoder_2(ids2.to(self.text_encoder_2.device))[0]
        prompt_embeds = prompt_embeds.to(device, torch.bfloat16).repeat_interleave(num_images_per_prompt, dim=0)
        pooled_prompt_embeds = pooled_prompt_embeds.to(device, torch.bfloat16).repeat_interleave(num_images_per_prompt, dim=0)
        return prompt_embeds, pooled_prompt_embeds

    def check_inputs(self, prompt, height, width, prompt_embeds, pooled_prompt_embeds, max_sequence_length):
        if height % (self.vae_scale_factor * 2) != 0 or width % (self.vae_scale_factor * 2) != 0:
            raise ValueError(f'`height` and `width` have to be divisible by {self.vae_scale_factor * 2}')
        if prompt is not None and prompt_embeds is not None:
            raise ValueError('Cannot forward both `prompt` and `prompt_embeds`.')
        if prompt is None and prompt_embeds is None:
            raise ValueError('Provide either `prompt` or `prompt_embeds`.')
        if prompt_embeds is not None and pooled_prompt_embeds is None:
            raise ValueError('If `prompt_embeds` are provided, `pooled_prompt_embeds` also have to be passed.')
        if max_sequence_length is not None and max_sequence_length > 512:
            raise ValueError(f'`max_sequence_length` cannot be greater than 512 but is {max_sequence_length}')

    def _enhance_conditioning(self, prompt, prompt_embeds=None, pooled_prompt_embeds=None, guidance_scale: float = 3.5,
                              max_sequence_length: int = 512) -> Dict[str, Any]:
        self.check_inputs(prompt, 16, 16, prompt_embeds, pooled_prompt_embeds, max_sequence_length)
        if (prompt_embeds.shape[0] if prompt is None else (1 if isinstance(prompt, str) else len(prompt))) != 1:
            raise ValueError('`enhance` takes one prompt (the tiles share it)')
        pe, pooled = self.encode_prompt(prompt, None, prompt_embeds, pooled_prompt_embeds, self._execution_device, 1, max_sequence_length)
        return dict(prompt_embeds=pe, pooled_prompt_embeds=pooled, guidance_scale=guidance_scale, max_sequence_length=max_sequence_length)

    @torch.inference_mode()
    def __call__(self, prompt: Union[str, List[str]] = None, prompt_2: Optional[Union[str, List[str]]] = None,
                 height: Optional[int] = None, width: Optional[int] = None, num_inference_steps: int = 4,
                 total_substeps: int = 128, timestep_ratio: float = 0.5, temperature: Union[float, str] = 'auto',
                 guidance_scale: float = 3.5, num_images_per_prompt: Optional[int] = 1,
                 generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None,
                 latents: Optional[torch.FloatTensor] = None, prompt_embeds: Optional[torch.FloatTensor] = None,
                 pooled_prompt_embeds: Optional[torch.FloatTensor] = None, ip_adapter_image=None,
                 ip_adapter_image_embeds=None, output_type: Optional[str] = 'pil', return_dict: bool = True,
                 joint_attention_kwargs: Optional[Dict[str, Any]] = None,
                 callback_on_step_end: Optional[Callable[[int, int, Dict], None]] = None,
                 callback_on_step_end_tensor_inputs: List[str] = ['latents'], max_sequence_length: int = 512, *,
                 image=None, image_latents: Optional[torch.Tensor] = None, strength: float = 1.0, mask_image=None,
                 composite: bool = True, resize: Optional[str] = None, mask_blur: float = 0.0, padding_mask_crop: Optional[int] = None,
                 color_fix: Optional[str] = None):
        """Text-to-image by default.  ``image`` (or its packed latents ``image_latents``) starts the sampler from the image noised to
        ``strength`` in (0, 1] instead of from pure noise (image-to-image); ``mask_image`` (1 = repaint) keeps the unmasked region on the
        image's own trajectory (inpainting) and, with ``composite``, pastes the original pixels back there after decoding.  ``height`` /
        ``width`` default to the image's size.  ``resize`` None: nothing is resized and an input of another size raises; 'stretch' / 'crop':
        ``image`` (Lanczos-3) and ``mask_image`` (triangle filter, soft values kept) are resampled to the call's size on the GPU, 'crop' from
        the largest centred window of the call's aspect ratio, PIL and uint8 numpy inputs uploaded as uint8; ``height`` / ``width`` then
        default to the image's sides rounded to multiples of 16.  With ``resize`` a uint8 numpy array is 8-bit pixels, read as x / 255
        (with ``resize=None`` it is taken, as before, as values already in [0, 1]); a uint8 torch tensor raises with ``resize``.  ``mask_blur``: sigma in output pixels of a Gaussian feather of the mask
        (0 = none), which feeds the latent blend and the composite alike.  ``latents`` / ``generator`` give the start noise as before.
        ``padding_mask_crop`` (an integer number of source pixels; needs ``image`` as 8-bit pixels -- PIL or a uint8 numpy array -- and a
        ``mask_image`` of the image's size, of ANY size; not with ``resize`` or ``image_latents``): the edit runs at the call's size
        (``height`` / ``width``, default 1024) on a window around the mask's bounding box, padded by that many pixels and grown to the call's
        aspect ratio (``schedule.mask_crop_window``), and the result is the image at ITS OWN size: the window holds the edit, resampled back
        and blended by the mask (``composite=False``: unblended), every other byte is the image's own (``ops.image_paste``).  'pil' comes
        from those bytes, 'np' is bytes / 255 as float32 [B, H, W, 3], 'pt' the uint8 [B, H, W, 3] device tensor; 'latent' raises.
        diffusers' ``padding_mask_crop`` + ``apply_overlay`` as recalled; parity unpinned.
        ``color_fix`` ('adain' or 'wavelet'; None: off, and every result as before): the decoded image is matched to ``image`` before
        anything else is done with it (``ops.color_fix``: 'wavelet' swaps the edit's low band for the image's, 'adain' gives it the image's
        per-channel mean and deviation), so an image-to-image call keeps the image's colours and lighting.  With it 'pt' returns float32
        whatever the decoder's dtype.  It needs ``image`` and goes with neither ``mask_image``, ``padding_mask_crop`` nor 'latent'
        (DESIGN.md 6.3.4)."""
        edit, height, width = self._edit_inputs(image, image_latents, mask_image, strength, height, width, resize, mask_blur, padding_mask_crop,
                                                output_type, color_fix)
        height = height or self.default_sample_size * self.vae_scale_factor
        width = width or self.default_sample_size * self.vae_scale_factor
        self.check_inputs(prompt, height, width, prompt_embeds, pooled_prompt_embeds, max_sequence_length)
        if ip_adapter_image is not None or ip_adapter_image_embeds is not None:
            raise NotImplementedError('IP-Adapter inputs are outside the ArcFlow hot path')
        self._apply_lora_scale(float((joint_attention_kwargs or {}).get('scale', 1.0)))      # arcflux.py:147-154: scale_lora_layers around the forward
        if self.transformer is None or self.transformer.teacher_head:
            raise RuntimeError('load_arcflow_adapter() must be called before sampling (the plain FLUX head '
                               'predicts a single velocity, not an ArcFlow policy)')
        self._guidance_scale, self._interrupt = guidance_scale, False
        if prompt is not None and isinstance(prompt, str):
            batch_size = 1
        elif prompt is not None:
            batch_size = len(prompt)
        else:
            batch_size = prompt_embeds.shape[0]
        device = self._execution_device
        prompt_embeds, pooled = self.encode_prompt(prompt, prompt_2, prompt_embeds, pooled_prompt_embeds, device,
                                                   num_images_per_prompt, max_sequence_length)
        B = batch_size * num_images_per_prompt
        latents, hp, wp = self._prepare_latents(B, height, width, generator, latents)
        if edit is not None:
            edit = self._edit_prepare(edit, B, hp, wp)
        guidance = torch.full((B,), guidance_scale, device=device, dtype=torch.float32) \
            if self.transformer.guidance_embeds else None

        def fwd(x, t, pe, prepared_step=None):
            return self.transformer(x, t, pe.to(device, torch.bfloat16), pooled, guidance, hp, wp, prepared_step=prepared_step)

        def prepare(sigmas):
            return self.transformer.prepare_steps(sigmas, pooled, guidance, B, hp * wp, prompt_embeds.shape[1])
        latents = self._denoise(latents, hp, wp, num_inference_steps, total_substeps, timestep_ratio, fwd,
                                callback_on_step_end, callback_on_step_end_tensor_inputs, prompt_embeds, prepare, edit=edit)
        return self._finish(latents, hp, wp, output_type, return_dict, edit, composite, padding_mask_crop)

    def _finish(self, latents, hp, wp, output_type, return_dict, edit=None, composite=True, padding_mask_crop=None):
        """Packed latents -> the call's result: decode through the attached VAE unless ``output_type='latent'``.  An inpainting call
        (``edit`` with an image and a mask) gets the original pixels pasted back outside the mask unless ``composite`` is off."""
        if output_type == 'latent':
            image = latents
        else:
            if self.vae is None:
                raise RuntimeError("no VAE decoder attached: use output_type='latent' or set pipe.vae")
            from ..vae import AutoencoderKLDecoder
            if isinstance(self.vae, AutoencoderKLDecoder):      # HIP decoder: un-scaling + unpack fused into its first kernel
                image = self.vae.decode_packed(latents, hp, wp)
            else:                                               # any module with the diffusers AutoencoderKL interface
                lat = self._unpack(latents, hp, wp)
                lat = lat / self.vae.config.scaling_factor + self.vae.config.shift_factor
                image = self.vae.decode(lat.to(next(self.vae.parameters()).dtype), return_dict=False)[0]
            image = self._output(image, edit, composite, output_type, padding_mask_crop)
        self.maybe_free_model_hooks()
        if not return_dict:
            return (image,)
        return FluxPipelineOutput(images=image)

    @torch.inference_mode()
    def sample_teacher(self, prompt: Union[str, List[str]] = None, negative_prompt: Union[str, List[str]] = None,
                       height: Optional[int] = None, width: Optional[int] = None, num_inference_steps: int = 28,
                       guidance_scale: float = 3.5, true_cfg_scale: float = 1.0,
                       generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None,
                       latents: Optional[torch.FloatTensor] = None, prompt_embeds: Optional[torch.FloatTensor] = None,
                       pooled_prompt_embeds: Optional[torch.FloatTensor] = None, negative_prompt_embeds: Optional[torch.FloatTensor] = None,
                       negative_pooled_prompt_embeds: Optional[torch.FloatTensor] = None, output_type: Optional[str] = 'pil',
                       return_dict: bool = True, guidance_interval=None, orthogonal_guidance: bool = False,
                       num_images_per_prompt: int = 1, max_sequence_length: int = 512, sampler: str = 'FlowEulerODE',
                       h: Optional[Union[float, str]] = None, *, image=None, image_latents: Optional[torch.Tensor] = None,
                       strength: float = 1.0, mask_image=None, composite: bool = True, solver_order: Optional[int] = None,
                       solver_type: Optional[str] = None, resize: Optional[str] = None, mask_blur: float = 0.0,
                       padding_mask_crop: Optional[int] = None, color_fix: Optional[str] = None):
        """Sample the TEACHER (plain FLUX.1-dev): ``num_inference_steps`` Euler ODE steps (FlowEulerODEScheduler on this pipeline's
        shift settings), ``guidance_scale`` = the distilled guidance embedding, ``true_cfg_scale`` > 1 = true classifier-free
        guidance against ``negative_prompt`` / ``negative_prompt_embeds`` (a second forward per step; ``guidance_interval`` in
        t = 1000 sigma limits it, ``orthogonal_guidance`` projects it).  ``sampler='FlowSDE'`` takes the stochastic steps of
        FlowSDEScheduler instead, with noise strength ``h`` (a float, default 1.0, or 'inf'); their draws come from ``generator``
        after the start noise.  ``sampler='UniPC'`` takes the multistep predictor-corrector steps of FlowUniPCScheduler
        (``solver_order`` 1 / 2 (default) / 3, ``solver_type`` 'bh1' / 'bh2'; no ``mask_image`` with it).  Works before
        ``load_arcflow_adapter()`` on the pipeline's own engine; afterwards a teacher engine is built once from the kept base weights, which holds a SECOND copy of the
        transformer on the GPU (FLUX.1-dev: about 24 GB in bf16) next to the student.  Style LoRAs (``load_lora_weights``) and the
        adapter weights of ``set_adapters`` do not apply: the teacher is the plain model.  Decoding is ``__call__``'s.

        ``image`` / ``image_latents``, ``strength``, ``mask_image`` and ``composite`` are ``__call__``'s, validated and prepared by the
        same code: the teacher's image-to-image and inpainting, the many-step reference for the student's edits.  Unlike the student
        (which takes all its steps over [strength, 0]) the teacher walks a SUFFIX of its ``num_inference_steps`` schedule: t_start =
        int(max(n - min(n strength, n), 0)), start on the image noised to sigmas[t_start], steps t_start .. n - 1 run
        (``schedule.truncate_by_strength``); with a mask every step also puts the unmasked latent pixels back on the image's own
        trajectory with the start noise (fused into the step kernel, ``afx_teacher_edit_step``).  These follow diffusers' img2img /
        inpaint pipelines as recalled; the reference has no image-conditioned sampling and nothing pins them.  ``resize``
        and ``mask_blur`` are ``__call__``'s too: the device resize of ``image`` / ``mask_image`` and the Gaussian feather of the mask, and so
        is ``padding_mask_crop``: the edit of a window around the mask, pasted back into the image at its own size, and ``color_fix``:
        the decoded image matched to ``image`` ('pt' is float32 then)."""
        edit, height, width = self._edit_inputs(image, image_latents, mask_image, strength, height, width, resize, mask_blur, padding_mask_crop,
                                                output_type, color_fix)
        height = height or self.default_sample_size * self.vae_scale_factor
        width = width or self.default_sample_size * self.vae_scale_factor
        self.check_inputs(prompt, height, width, prompt_embeds, pooled_prompt_embeds, max_sequence_length)
        device = self._execution_device
        pe, pooled = self.encode_prompt(prompt, None, prompt_embeds, pooled_prompt_embeds, device, num_images_per_prompt, max_sequence_length)
        cond = dict(prompt_embeds=pe, pooled=pooled)
        if true_cfg_scale > 1.0:
            if negative_prompt is None and negative_prompt_embeds is None:
                raise ValueError('true_cfg_scale > 1 needs `negative_prompt` or `negative_prompt_embeds` (+ `negative_pooled_prompt_embeds`)')
            if negative_prompt_embeds is not None and negative_pooled_prompt_embeds is None:
                raise ValueError('If `negative_prompt_embeds` are provided, `negative_pooled_prompt_embeds` also have to be passed.')
            if negative_prompt_embeds is None and isinstance(negative_prompt, str):
                negative_prompt = [negative_prompt] * (pe.shape[0] // num_images_per_prompt)
            ne, npooled = self.encode_prompt(negative_prompt if negative_prompt_embeds is None else None, None, negative_prompt_embeds,
                                             negative_pooled_prompt_embeds, device, num_images_per_prompt, max_sequence_length)
            if ne.shape[0] != pe.shape[0]:
                raise ValueError(f'{ne.shape[0]} negative prompts for {pe.shape[0]} prompts')
            cond.update(negative_prompt_embeds=ne, negative_pooled=npooled)
        out, hp, wp, edit = self._sample_teacher(cond, pe.shape[0], height, width, num_inference_steps, guidance_scale, true_cfg_scale,
                                                 generator, latents, guidance_interval, orthogonal_guidance, sampler, h, edit, solver_order, solver_type)
        return self._finish(out, hp, wp, output_type, return_dict, edit, composite, padding_mask_crop)
