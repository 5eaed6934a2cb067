"""ArcFluxPipeline -- drop-in for ``lakonlab.pipelines.arcflux_pipeline.ArcFluxPipeline``
(reference arcflux_pipeline.py:73-542): same constructor extras (``policy_type``, ``policy_kwargs``),
same ``__call__`` keywords and defaults, ``.images`` result, ``load_arcflow_adapter``.

This file holds what is FLUX's: the constructor, the engine, ``from_pretrained``, prompt encoding (CLIP pooled + T5), ``__call__``,
``sample_teacher`` and the AutoencoderKL decode.  The denoising loop (reference arcflux_pipeline.py:457-510), the way from latents to
the result and ``enhance`` are ``base.py``'s, shared with Qwen-Image.  Prompt encoding and VAE decode are the rows SURVEY 8f marks
"next": pass ``prompt_embeds`` / ``pooled_prompt_embeds`` (or attach HF text encoders) and use ``output_type='latent'`` unless a
decoder module is attached as ``pipe.vae``.

Beyond the reference: ``__call__`` of both pipelines takes the keyword-only ``image`` / ``image_latents``, ``strength``, ``mask_image`` and
``composite`` (image-to-image and inpainting; read by ``edit_inputs.py``).  Without them the call is the text-to-image
path unchanged.  ``enhance(photo, prompt, scale=, tile=, overlap=, strength=)`` of both pipelines reworks a photo of any size through that
call on overlapping tiles.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Optional, Union

import torch

from ..engine import MMDiTEngine
from ..schedule import FlowMatchEulerDiscreteScheduler
from .base import POLICY_CLASSES, ArcFlowPipelineBase, load_scheduler_config, load_transformer_dir  # noqa: F401  (both names are imported from here)
from .edit_inputs import resolve_size


@dataclass
class FluxPipelineOutput:
    images: Any


class ArcFluxPipeline(ArcFlowPipelineBase):
    r"""Policy-based FLUX pipeline, 2-NFE capable (reference arcflux_pipeline.py:73)."""
    _family = 'flux'
    _output_class = FluxPipelineOutput

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
        pipe = cls(scheduler=FlowMatchEulerDiscreteScheduler.from_config(load_scheduler_config(root)))
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
        height, width = resolve_size(height, width, self.default_sample_size * self.vae_scale_factor)
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
        return self._finish(latents, hp, wp, output_type, return_dict, edit, composite)

    def _decode(self, latents, hp, wp) -> torch.Tensor:
        """AutoencoderKL: packed latents -> the image [B, 3, 16 hp, 16 wp] in [-1, 1]."""
        from ..vae import AutoencoderKLDecoder
        if isinstance(self.vae, AutoencoderKLDecoder):      # HIP decoder: un-scaling + unpack fused into its first kernel
            return self.vae.decode_packed(latents, hp, wp)
        lat = self._unpack(latents, hp, wp)                 # any module with the diffusers AutoencoderKL interface
        lat = lat / self.vae.config.scaling_factor + self.vae.config.shift_factor
        return self.vae.decode(lat.to(next(self.vae.parameters()).dtype), return_dict=False)[0]

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
        height, width = resolve_size(height, width, self.default_sample_size * self.vae_scale_factor)
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
        return self._finish(out, hp, wp, output_type, return_dict, edit, composite)
