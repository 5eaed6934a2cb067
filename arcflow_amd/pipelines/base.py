"""``ArcFlowPipelineBase``, what ``ArcFluxPipeline`` and ``ArcQwenImagePipeline`` share: the diffusers-style plumbing, the start noise,
the one student loop (``_denoise``: two C-ABI calls per step, ``afx_mmdit_forward`` and ``afx_arcflow_step``, on latents that never leave
the packed token layout), the teacher sampling, the way out (``_finish``: the family's ``_decode``, then ``_output``), ``enhance`` and ``outpaint``."""
from __future__ import annotations

import glob
import json
import os
from typing import Any, Dict, List, Optional, Union

import torch

from .. import ops
from ..engine import MMDiTEngine
from ..schedule import FlowMatchEulerDiscreteScheduler, calculate_shift, edit_raw_timesteps, mask_to_tokens, retrieve_raw_timesteps
from . import edit_inputs
from .arcflow_loader import ArcFlowLoaderMixin

POLICY_CLASSES = ('ArcFlow',)


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


def load_scheduler_config(root: str) -> Dict[str, Any]:
    """``<root>/scheduler/scheduler_config.json`` of a diffusers snapshot; {} without one."""
    sp = os.path.join(root, 'scheduler', 'scheduler_config.json')
    if not os.path.exists(sp):
        return {}
    with open(sp) as f:
        return json.load(f)


class ArcFlowPipelineBase(ArcFlowLoaderMixin):
    _family = None              # 'flux' / 'qwen'
    _output_class = None        # the family's result dataclass, ``images``
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

    def _unpack(self, latents, hp, wp):
        b = latents.shape[0]
        return latents.view(b, hp, wp, 16, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(b, 16, 2 * hp, 2 * wp)

    # image editing: image-to-image and inpainting ---------------------------------------------------------
    def _edit_inputs(self, image, image_latents, mask_image, strength, height, width, resize=None, mask_blur=0.0, padding_mask_crop=None,
                     output_type=None, color_fix=None):
        """Host-side half of the edit arguments: -> (EditRequest, height, width), the request None on the text-to-image path."""
        return edit_inputs.edit_inputs(image, image_latents, mask_image, strength, height, width, resize, mask_blur, padding_mask_crop, output_type,
                              color_fix, self._device, self.default_sample_size * self.vae_scale_factor)

    def _edit_prepare(self, edit, B, hp, wp):
        """Device-side half: batch checks, the encode of ``image`` (posterior mode, packed), the mask per latent pixel."""
        device = self._device
        for name, t in (('image', edit.image), ('image_latents', edit.image_latents), ('mask_image', edit.mask)):
            if t is not None and t.shape[0] not in (1, B):
                raise ValueError(f'`{name}` has batch {t.shape[0]}, the call has {B} (a batch of 1 broadcasts)')
        if edit.image is not None:
            encoder = getattr(self.vae, 'encoder', None)
            if encoder is None:
                raise RuntimeError('`image=` needs a VAE encoder (pipe.vae.encoder: a snapshot with encoder.* weights); without one pass '
                                   '`image_latents=`, the packed latents of the image')
            x0 = encoder.encode_images01(edit.image, sample=False, packed=True)
        else:
            x0 = edit.image_latents.to(device, torch.float32)
        edit.x0 = x0.expand(B, -1, -1).contiguous()
        if edit.mask is not None:
            edit.mask_tokens = mask_to_tokens(edit.mask.to(device), hp, wp).expand(B, -1, -1).contiguous()
        return edit

    @staticmethod
    def _check_start_noise(noise, edit):
        if tuple(noise.shape) != tuple(edit.x0.shape):
            raise ValueError(f'`latents` (the start noise) is {tuple(noise.shape)}, the image latents are {tuple(edit.x0.shape)}')

    def _denoise(self, latents, hp, wp, num_inference_steps, total_substeps, timestep_ratio, fwd,
                 callback_on_step_end, callback_on_step_end_tensor_inputs, prompt_embeds, prepare=None, edit=None):
        """The student loop, from the noise ``latents`` over the raw time [1, 0]; with ``edit`` (prepared by ``_edit_prepare``) over
        [strength, 0], started on (1 - sigma) x0 + sigma noise and, with a mask, blended back onto the source's trajectory after every step
        (afx_edit_blend).  ``lat16``, that kernel's bf16 copy of ``latents``, feeds the next forward; a step without a mask and a callback drop it."""
        device = self._device
        B = latents.shape[0]
        mask = None
        if edit is None:
            raw, per_step, total = retrieve_raw_timesteps(num_inference_steps, total_substeps, timestep_ratio)
        else:
            self._check_start_noise(latents, edit)
            x0, mask, noise = edit.x0, edit.mask_tokens, latents.contiguous()
            raw, per_step, total = edit_raw_timesteps(num_inference_steps, total_substeps, timestep_ratio, edit.strength)
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
        lat16 = None
        if edit is not None:
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
                                                torch.full((B,), sigma_end, device=device, dtype=torch.float32), out=latents)
            if callback_on_step_end is not None:
                local = dict(latents=latents, prompt_embeds=prompt_embeds)
                cb = callback_on_step_end(self, i, torch.tensor(t_src, device=device),
                                          {k: local[k] for k in callback_on_step_end_tensor_inputs})
                latents, lat16 = cb.pop('latents', latents), None          # the callback may have changed them
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
            self._check_start_noise(latents, edit)
            kw = dict(x0=edit.x0, mask=edit.mask_tokens, strength=edit.strength)
        solver = {k: v for k, v in dict(h=h, solver_order=solver_order, solver_type=solver_type).items() if v is not None}       # the scheduler refuses a keyword that is not its own
        sampler = TeacherSampler(engine, num_inference_steps, guidance_scale=true_cfg_scale, distilled_guidance=guidance_scale,
                                 guidance_interval=guidance_interval, orthogonal_guidance=orthogonal_guidance, tokens_as_seq_len=True,
                                 sampler=sampler, **solver, **self._euler_scheduler_kwargs())
        self._num_timesteps = num_inference_steps
        return sampler(cond, latents, generator=generator, **kw), hp, wp, edit          # (the generator's stream continues from the start noise into FlowSDE's step draws)

    # the way out: packed latents -> the call's result ----------------------------------------------------
    def _decode(self, latents, hp, wp) -> torch.Tensor:
        """The family's VAE decode of packed latents -> the image [B, 3, 16 hp, 16 wp] in [-1, 1], in the decoder's dtype."""
        raise NotImplementedError

    def _finish(self, latents, hp, wp, output_type, return_dict, edit=None, composite=True):
        """Packed latents -> the call's result: decode through the attached VAE unless ``output_type='latent'``.  An inpainting call
        (``edit`` with an image and a mask) gets the original pixels pasted back outside the mask unless ``composite`` is off."""
        if output_type == 'latent':
            image = latents
        else:
            if self.vae is None:
                raise RuntimeError("no VAE decoder attached: use output_type='latent' or set pipe.vae")
            image = self._output(self._decode(latents, hp, wp), edit, composite, output_type)
        self.maybe_free_model_hooks()
        return self._output_class(images=image) if return_dict else (image,)

    def _output(self, image, edit, composite, output_type):
        """The decoded image -> what the call returns.  With ``padding_mask_crop`` (``edit.paste``): the photo's size, from the bytes of
        ``_paste``.  With ``color_fix`` the decoded image is first matched to the call's ``image`` and is float32 from there on."""
        if edit is not None and edit.paste is not None:
            return edit_inputs.bytes_output(self._paste(image, edit, composite), output_type)
        if edit is not None and edit.color_fix is not None:
            if image.dtype not in (torch.float32, torch.bfloat16):
                image = image.to(torch.float32)
            image = ops.color_fix(image.contiguous(), edit.image.to(image.device, torch.float32).contiguous(), edit.color_fix)
        return self._postprocess(self._composite(image, edit, composite), output_type)

    def _composite(self, image, edit, composite):
        """Paste the original pixels back outside the mask: m decoded + (1 - m) original, in the decoder's range [-1, 1] and dtype."""
        if not composite or edit is None or edit.image is None or edit.mask is None:
            return image
        m = edit.mask.to(image.device, torch.float32)
        orig = (edit.image.to(image.device) * 2 - 1).to(image.dtype).to(torch.float32)
        return (m * image.to(torch.float32) + (1 - m) * orig).to(image.dtype)

    def _paste(self, image, edit, composite) -> torch.Tensor:
        """The decoded edit [B, 3, h, w] in [-1, 1] back into the photo it was cut from -> uint8 [B, H, W, 3] on the GPU (ops.image_paste):
        the window takes the edit resampled to its size, blended with the photo by the call's mask (``composite`` off: the whole window is
        the edit); every other byte is the photo's own."""
        src, window = edit.paste
        if src.shape[0] != image.shape[0]:
            if src.shape[0] != 1:
                raise ValueError(f'`image` has batch {src.shape[0]}, the call has {image.shape[0]} (a batch of 1 broadcasts)')
            src = src.expand(image.shape[0], -1, -1, -1).contiguous()
        return ops.image_paste(image.to(torch.float32).contiguous(), edit.mask if composite else None, src, window)

    def _postprocess(self, image, output_type):
        if output_type == 'pt':
            return image
        img = (image.float() / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).cpu().numpy()
        if output_type == 'np':
            return img
        from PIL import Image
        return [Image.fromarray(x) for x in (img * 255).round().astype('uint8')]

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
        edit_inputs.check_color_fix(color_fix, image, None, None, output_type)
        if isinstance(tile_batch, bool) or int(tile_batch) != tile_batch or tile_batch < 1:
            raise ValueError(f'`tile_batch`: an integer >= 1, got {tile_batch!r}')
        edit_inputs.check_strength(strength)
        if not 0.0 < float(scale) < float('inf'):
            raise ValueError(f'`scale` must be positive and finite, got {scale}')
        src = edit_inputs.resize_source(image, 'image', 3, self._device)
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
        out = edit_inputs.bytes_output(ops.tiles_merge(decoded, plan)[None], output_type)
        return self._output_class(images=out) if return_dict else (out,)

    # outpainting: the photo on a larger canvas, the new pixels painted window by window ------------------------
    @torch.inference_mode()
    def outpaint(self, image, prompt: Union[str, List[str]] = None, *, left: int = 0, right: int = 0, top: int = 0, bottom: int = 0,
                 tile: int = 1024, overlap: int = 256, blend: int = 32, fill: str = 'reflect', strength: float = 1.0,
                 num_inference_steps: int = 2, timestep_ratio: float = 1.0, total_substeps: int = 128,
                 generator: Optional[torch.Generator] = None, latents: Optional[torch.Tensor] = None, output_type: Optional[str] = 'pil',
                 return_dict: bool = True, **conditioning):
        """Make one photo larger by ``left``, ``right``, ``top``, ``bottom`` pixels and paint what lies beyond its borders.  The photo is
        laid on the extended canvas, the new pixels filled from it (``fill``: 'reflect' mirrors the photo, 'edge' repeats its border;
        ``ops.canvas_extend``, which also gives the mask state M: 1 on the new pixels, a ramp over ``blend`` pixels inside every extended
        side).  ``schedule.outpaint_plan`` lays windows of at most ``tile`` pixels a side over the new area -- the left and right bands
        first, then the top and bottom bands with the corners, each window ``overlap`` pixels over what is already known -- and every
        window, in order, is one ordinary inpainting call of this pipeline at the window's size,
        ``self(image=window of the canvas, mask_image=window of M, strength=..., latents=noise[k], composite=False, output_type='pt')``,
        whose result ``ops.image_paste`` blends into the canvas by that same mask (once: hence ``composite=False``; where M is 0 the
        canvas keeps its bytes) and ``ops.canvas_mark`` then marks as painted, leaving a ramp of ``blend`` pixels inside the window's inner
        sides for the next window to cross-fade over.  A window sees what the windows before it painted: they run one per call, in the
        plan's order, and cannot be batched.

        ``image``: one photo as 8-bit pixels, a PIL image or a uint8 numpy array [H, W, 3] (the result keeps the photo's bytes); a batch
        other than 1 raises.  The prompt is encoded once; the conditioning keywords are the family's, as on ``enhance``.  ``strength`` is
        the inpainting call's (1: the new pixels start from pure noise, the fill only steers through the unmasked context).  The windows'
        start noise is ``latents`` [T, (wh / 16) (ww / 16), 64] for the plan's T windows of wh x ww, else one draw of that shape from
        ``generator``.  The result has the canvas' size, (H + top + bottom) x (W + left + right): 'pt' the uint8 [1, Hc, Wc, 3] device
        tensor, 'np' bytes / 255 as float32, 'pil' images of the bytes; 'latent' raises.  With ``blend=0`` every byte of the photo is kept;
        otherwise every byte deeper than ``blend`` pixels inside its extended sides.  What is refused (``schedule.outpaint_plan``'s rules
        among it) is refused before anything runs.

        Out of scope: the teacher (``sample_teacher``), batches of windows, windows of differing sizes, other fills, ``color_fix`` (it
        refuses masks), lists of photos."""
        from ..schedule import outpaint_plan
        if output_type == 'latent':
            raise ValueError("`outpaint` returns the image at the canvas' size: output_type 'pil', 'np' or 'pt', not 'latent'")
        if fill not in ops.CANVAS_FILLS:
            raise ValueError(f"`fill`: 'edge' or 'reflect', got {fill!r}")
        photo = edit_inputs.photo_bytes(image, 'image', 'the result keeps the photo\'s own bytes')
        edit_inputs.check_strength(strength)
        H, W = photo.shape[1:3]
        plan = outpaint_plan(H, W, left, top, right, bottom, tile, overlap, blend)
        T, hp, wp = len(plan.windows), plan.wh // 16, plan.ww // 16
        if latents is not None and tuple(latents.shape) != (T, hp * wp, 64):
            raise ValueError(f'`latents` (the windows\' start noise): need [{T}, {hp * wp}, 64] for {T} windows of {plan.wh} x {plan.ww}, '
                             f'got {tuple(latents.shape)}')
        cond = self._enhance_conditioning(prompt, **conditioning)
        noise, _, _ = self._prepare_latents(T, plan.wh, plan.ww, generator, latents)
        src = edit_inputs.resize_source(photo, 'image', 3, self._device)
        canvas, M = ops.canvas_extend(src, plan.photo[0], plan.photo[1], plan.Wc - plan.photo[2], plan.Hc - plan.photo[3], fill, blend)
        other = torch.empty_like(canvas)
        for k, window in enumerate(plan.windows):
            x0, y0, x1, y1 = window
            # the window as the call reads it, float(byte) / 255 exactly: a same-size resample of the window's rows is the identity
            win = ops.image_resample(canvas[:, y0:y1], plan.wh, plan.ww, 'lanczos3', (float(x0), 0.0, float(x1), float(plan.wh)), clamp=True)
            mwin = M[:, :, y0:y1, x0:x1].contiguous()
            out = self(image=win, mask_image=mwin, strength=strength, latents=noise[k:k + 1], num_images_per_prompt=1, composite=False,
                       num_inference_steps=num_inference_steps, timestep_ratio=timestep_ratio, total_substeps=total_substeps,
                       output_type='pt', **cond).images
            canvas, other = ops.image_paste(out.to(torch.float32).contiguous(), mwin, canvas, window, out=other), canvas
            ops.canvas_mark(M, window, blend)
        out = edit_inputs.bytes_output(canvas, output_type)
        return self._output_class(images=out) if return_dict else (out,)
