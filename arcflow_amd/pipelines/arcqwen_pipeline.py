"""ArcQwenImagePipeline -- drop-in for ``lakonlab.pipelines.arcqwen_pipeline.ArcQwenImagePipeline``
(reference arcqwen_pipeline.py:65-489).  Differences from the FLUX pipeline that the reference has too:
no pooled/guidance inputs, variable text length (``prompt_embeds_mask``; only the real tokens enter the
transformer, arcqwen_pipeline.py:393 / arcqwen.py:325-330), QwenEmbedRope tables, per-channel latent
de-normalisation before the (3-D, T=1) VAE."""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Any, Callable, Dict, List, Optional, Union

import torch

from ..engine import MMDiTEngine
from ..schedule import FlowMatchEulerDiscreteScheduler
from .base import ArcFlowPipelineBase, load_scheduler_config, load_transformer_dir
from .edit_inputs import resolve_size


@dataclass
class QwenImagePipelineOutput:
    images: Any


class ArcQwenImagePipeline(ArcFlowPipelineBase):
    _family = 'qwen'
    _output_class = QwenImagePipelineOutput

    def __init__(self, scheduler=None, vae=None, text_encoder=None, tokenizer=None, transformer=None,
                 policy_type: str = 'ArcFlow', policy_kwargs: Optional[Dict[str, Any]] = None):
        super().__init__(scheduler, vae, text_encoder, tokenizer, transformer, policy_type, policy_kwargs)

    def _build_engine(self, num_gaussians=16, logweights_channels=4, teacher_head=False) -> MMDiTEngine:
        c = self._transformer_config
        return MMDiTEngine('qwen', c.get('num_layers', 60), 0, heads=c.get('num_attention_heads', 24),
                           head_dim=c.get('attention_head_dim', 128), in_channels=c.get('in_channels', 64),
                           joint_dim=c.get('joint_attention_dim', 3584), num_gaussians=num_gaussians,
                           logweights_channels=logweights_channels, teacher_head=teacher_head,
                           axes_dims=tuple(c.get('axes_dims_rope', (16, 56, 56))))

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, torch_dtype=torch.bfloat16, **kwargs):
        root = pretrained_model_name_or_path
        if not os.path.isdir(os.path.join(root, 'transformer')):
            raise EnvironmentError(f'{root}/transformer not found: pass a local Qwen-Image snapshot directory')
        cfg, sd = load_transformer_dir(os.path.join(root, 'transformer'))
        pipe = cls(scheduler=FlowMatchEulerDiscreteScheduler.from_config(load_scheduler_config(root)))
        pipe._transformer_config, pipe._base_state_dict = cfg, sd
        if os.path.isdir(os.path.join(root, 'vae')):          # AutoencoderKLQwenImage decoder on the HIP engine
            from ..vae import AutoencoderKLQwenImageDecoder
            vcfg, vsd = load_transformer_dir(os.path.join(root, 'vae'))
            pipe.vae = AutoencoderKLQwenImageDecoder(vsd, vcfg['latents_mean'], vcfg['latents_std'],
                                                     tuple(vcfg.get('dim_mult', (1, 2, 4, 4))), vcfg.get('num_res_blocks', 2),
                                                     vcfg.get('z_dim', 16))
            if any(k.startswith('encoder.') for k in vsd):     # full VAE snapshot: pipe.vae.encode(...) as on the reference's PretrainedVAEQwenImage
                from ..vae import AutoencoderKLQwenImageEncoder
                pipe.vae.encoder = AutoencoderKLQwenImageEncoder(vsd, vcfg['latents_mean'], vcfg['latents_std'], vcfg.get('base_dim'),
                                                                 tuple(vcfg.get('dim_mult', (1, 2, 4, 4))), vcfg.get('num_res_blocks', 2),
                                                                 tuple(vcfg.get('temperal_downsample', (False, True, True))), vcfg.get('z_dim', 16))
        if os.path.isdir(os.path.join(root, 'text_encoder')) and os.path.isdir(os.path.join(root, 'tokenizer')):
            from ..text_encoders import load_qwen25_text_encoder
            pipe.text_encoder = load_qwen25_text_encoder(os.path.join(root, 'text_encoder'))
            from transformers import AutoTokenizer
            pipe.tokenizer = AutoTokenizer.from_pretrained(os.path.join(root, 'tokenizer'))
        if 'proj_out.weight' in sd:
            pipe.transformer = pipe._build_engine(teacher_head=True)
            pipe.transformer.load_state_dict(sd)
        return pipe

    # diffusers QwenImagePipeline prompt template (the reference inherits encode_prompt from it: arcqwen_pipeline.py:65,346)
    prompt_template_encode = ('<|im_start|>system\nDescribe the image by detailing the color, shape, size, texture, quantity, text, '
                              'spatial relationships of the objects and background:<|im_end|>\n<|im_start|>user\n{}<|im_end|>\n'
                              '<|im_start|>assistant\n')
    prompt_template_encode_start_idx = 34
    tokenizer_max_length = 1024

    def encode_prompt(self, prompt, max_sequence_length: int = 1024):
        """-> (prompt_embeds [B, T, D] zero padded, prompt_embeds_mask [B, T]): wrap in the template, run the language model,
        keep the valid tokens and drop the template's first ``prompt_template_encode_start_idx`` of them."""
        if self.text_encoder is None or self.tokenizer is None:
            raise RuntimeError('no text encoder attached: pass prompt_embeds (+ prompt_embeds_mask)')
        prompt = [prompt] if isinstance(prompt, str) else prompt
        drop = self.prompt_template_encode_start_idx
        tok = self.tokenizer([self.prompt_template_encode.format(e) for e in prompt], max_length=self.tokenizer_max_length + drop,
                             padding=True, truncation=True, return_tensors='pt')
        from ..text_encoders import Qwen25TextEncoder
        if isinstance(self.text_encoder, Qwen25TextEncoder):
            hidden = self.text_encoder(tok.input_ids, tok.attention_mask)
        else:
            hidden = self.text_encoder(input_ids=tok.input_ids.to(self.text_encoder.device), attention_mask=tok.attention_mask.to(self.text_encoder.device),
                                       output_hidden_states=True).hidden_states[-1]
        mask = tok.attention_mask.to(hidden.device).bool()
        rows = [hidden[b][mask[b]][drop:] for b in range(hidden.shape[0])]
        T = max(r.shape[0] for r in rows)
        embeds = torch.stack([torch.cat([r, r.new_zeros(T - r.shape[0], r.shape[1])]) for r in rows])
        emask = torch.stack([torch.cat([torch.ones(r.shape[0], dtype=torch.long), torch.zeros(T - r.shape[0], dtype=torch.long)]) for r in rows])
        return embeds[:, :max_sequence_length], emask[:, :max_sequence_length].to(hidden.device)

    def _enhance_conditioning(self, prompt, prompt_embeds=None, prompt_embeds_mask=None, max_sequence_length: int = 512) -> Dict[str, Any]:
        if prompt is not None and prompt_embeds is not None:
            raise ValueError('Cannot forward both `prompt` and `prompt_embeds`.')
        if prompt_embeds is None:
            if prompt is None:
                raise ValueError('Provide either `prompt` or `prompt_embeds`.')
            prompt_embeds, prompt_embeds_mask = self.encode_prompt(prompt, max_sequence_length=max_sequence_length)
        if prompt_embeds.shape[0] != 1:
            raise ValueError('`enhance` takes one prompt (the tiles share it)')
        return dict(prompt_embeds=prompt_embeds, prompt_embeds_mask=prompt_embeds_mask, max_sequence_length=max_sequence_length)

    @torch.inference_mode()
    def __call__(self, prompt: Union[str, List[str]] = None, height: Optional[int] = None, width: Optional[int] = None,
                 num_inference_steps: int = 4, total_substeps: int = 128, timestep_ratio: float = 0.5,
                 temperature: Union[float, str] = 'auto', num_images_per_prompt: int = 1,
                 generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None,
                 latents: Optional[torch.Tensor] = None, prompt_embeds: Optional[torch.Tensor] = None,
                 prompt_embeds_mask: Optional[torch.Tensor] = None, output_type: Optional[str] = 'pil',
                 return_dict: bool = True, attention_kwargs: Optional[Dict[str, Any]] = None,
                 callback_on_step_end: Optional[Callable[[int, int, Dict], None]] = None,
                 callback_on_step_end_tensor_inputs: List[str] = ['latents'], max_sequence_length: int = 512, *,
                 image=None, image_latents: Optional[torch.Tensor] = None, strength: float = 1.0, mask_image=None,
                 composite: bool = True, resize: Optional[str] = None, mask_blur: float = 0.0, padding_mask_crop: Optional[int] = None,
                 color_fix: Optional[str] = None):
        """Text-to-image by default; ``image`` / ``image_latents``, ``strength``, ``mask_image``, ``composite``, ``resize`` and ``mask_blur``
        as on ``ArcFluxPipeline.__call__`` (image-to-image and inpainting; ``resize='stretch'|'crop'`` resamples inputs of any size on the GPU,
        ``mask_blur`` feathers the mask), and ``padding_mask_crop`` as there: the edit runs on a window around the mask of an 8-bit image of any size
        and is pasted back into it at the image's own size.  ``color_fix`` ('adain' or 'wavelet') as there too: the decoded image is matched
        to ``image`` (``ops.color_fix``), and 'pt' is float32 then."""
        edit, height, width = self._edit_inputs(image, image_latents, mask_image, strength, height, width, resize, mask_blur, padding_mask_crop,
                                                output_type, color_fix)
        height, width = resolve_size(height, width, self.default_sample_size * self.vae_scale_factor)
        if prompt is not None and prompt_embeds is not None:
            raise ValueError('Cannot forward both `prompt` and `prompt_embeds`.')
        if prompt_embeds is None:
            if prompt is None:
                raise ValueError('Provide either `prompt` or `prompt_embeds`.')
            prompt_embeds, prompt_embeds_mask = self.encode_prompt(prompt, max_sequence_length=max_sequence_length)
        self._apply_lora_scale(float((attention_kwargs or {}).get('scale', 1.0)))      # arcflux.py:147-154: scale_lora_layers around the forward
        if self.transformer is None or self.transformer.teacher_head:
            raise RuntimeError('load_arcflow_adapter() must be called before sampling')
        self._interrupt = False
        device = self._execution_device
        prompt_embeds = prompt_embeds.to(device, torch.bfloat16).repeat_interleave(num_images_per_prompt, dim=0)
        if prompt_embeds_mask is not None:
            lens = prompt_embeds_mask.sum(dim=1).tolist()          # the reference's host sync (arcqwen_pipeline.py:393)
            prompt_embeds = prompt_embeds[:, :int(max(lens))]
        B = prompt_embeds.shape[0]
        latents, hp, wp = self._prepare_latents(B, height, width, generator, latents)
        if edit is not None:
            edit = self._edit_prepare(edit, B, hp, wp)

        def fwd(x, t, pe, prepared_step=None):
            return self.transformer(x, t, pe.to(device, torch.bfloat16), None, None, hp, wp, prepared_step=prepared_step)

        def prepare(sigmas):
            return self.transformer.prepare_steps(sigmas, None, None, B, hp * wp, prompt_embeds.shape[1])
        latents = self._denoise(latents, hp, wp, num_inference_steps, total_substeps, timestep_ratio, fwd,
                                callback_on_step_end, callback_on_step_end_tensor_inputs, prompt_embeds, prepare, edit=edit)
        return self._finish(latents, hp, wp, output_type, return_dict, edit, composite)

    def _decode(self, latents, hp, wp) -> torch.Tensor:
        """AutoencoderKLQwenImage (3-D, T = 1): packed latents -> the image [B, 3, 16 hp, 16 wp] in [-1, 1]."""
        from ..vae import AutoencoderKLQwenImageDecoder
        if isinstance(self.vae, AutoencoderKLQwenImageDecoder):   # HIP decoder: un-normalisation + unpack fused into its first kernel
            return self.vae.decode_packed(latents, hp, wp)
        device = self._execution_device                           # any module with the diffusers AutoencoderKLQwenImage interface
        lat = self._unpack(latents, hp, wp)[:, :, None]
        mean = torch.tensor(self.vae.config.latents_mean, device=device).view(1, -1, 1, 1, 1)
        std = torch.tensor(self.vae.config.latents_std, device=device).view(1, -1, 1, 1, 1)
        return self.vae.decode((lat * std + mean).to(next(self.vae.parameters()).dtype), return_dict=False)[0][:, :, 0]

    def _teacher_text(self, prompt, embeds, mask, num_images_per_prompt, max_sequence_length):
        """-> [B, T_real, D] bf16 on the device: only the real tokens enter the transformer, as in ``__call__``."""
        if embeds is None:
            embeds, mask = self.encode_prompt(prompt, max_sequence_length=max_sequence_length)
        embeds = embeds.to(self._execution_device, torch.bfloat16).repeat_interleave(num_images_per_prompt, dim=0)
        if mask is not None:
            embeds = embeds[:, :int(max(mask.sum(dim=1).tolist()))]
        return embeds

    @torch.inference_mode()
    def sample_teacher(self, prompt: Union[str, List[str]] = None, negative_prompt: Union[str, List[str]] = None,
                       height: Optional[int] = None, width: Optional[int] = None, num_inference_steps: int = 50,
                       guidance_scale: Optional[float] = None, true_cfg_scale: float = 4.0,
                       generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None,
                       latents: Optional[torch.Tensor] = None, prompt_embeds: Optional[torch.Tensor] = None,
                       prompt_embeds_mask: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                       negative_prompt_embeds_mask: Optional[torch.Tensor] = None, output_type: Optional[str] = 'pil',
                       return_dict: bool = True, guidance_interval=None, orthogonal_guidance: bool = False,
                       num_images_per_prompt: int = 1, max_sequence_length: int = 512, sampler: str = 'FlowEulerODE',
                       h: Optional[Union[float, str]] = None, *, image=None, image_latents: Optional[torch.Tensor] = None,
                       strength: float = 1.0, mask_image=None, composite: bool = True, solver_order: Optional[int] = None,
                       solver_type: Optional[str] = None, resize: Optional[str] = None, mask_blur: float = 0.0,
                       padding_mask_crop: Optional[int] = None, color_fix: Optional[str] = None):
        """Sample the TEACHER (plain Qwen-Image): ``num_inference_steps`` Euler ODE steps (FlowEulerODEScheduler on this pipeline's
        shift settings) with true classifier-free guidance ``true_cfg_scale`` against ``negative_prompt`` /
        ``negative_prompt_embeds`` (+ masks) when it is > 1; ``guidance_scale`` is accepted for signature parity and unused
        (Qwen-Image has no guidance embedding).  ``sampler='FlowSDE'`` takes the stochastic steps of FlowSDEScheduler instead, with
        noise strength ``h`` (a float, default 1.0, or 'inf'); their draws come from ``generator`` after the start noise.
        ``sampler='UniPC'`` takes the multistep steps of FlowUniPCScheduler (``solver_order``, ``solver_type``; no ``mask_image`` with it).  Works before ``load_arcflow_adapter()`` on the pipeline's own engine; afterwards a
        teacher engine is built once from the kept base weights, which holds a SECOND copy of the transformer on the GPU
        (Qwen-Image: about 41 GB in bf16) next to the student.  Style LoRAs (``load_lora_weights``) and the adapter weights of
        ``set_adapters`` do not apply: the teacher is the plain model.  Decoding is ``__call__``'s.  ``image`` / ``image_latents``,
        ``strength``, ``mask_image`` and ``composite``: the teacher's image-to-image and inpainting, as on
        ``ArcFluxPipeline.sample_teacher`` (a suffix of the schedule chosen by ``strength``; unpinned semantics); ``resize`` and
        ``mask_blur``, ``padding_mask_crop`` and ``color_fix`` as on ``ArcFluxPipeline.__call__``."""
        edit, height, width = self._edit_inputs(image, image_latents, mask_image, strength, height, width, resize, mask_blur, padding_mask_crop,
                                                output_type, color_fix)
        height, width = resolve_size(height, width, self.default_sample_size * self.vae_scale_factor)
        if prompt is not None and prompt_embeds is not None:
            raise ValueError('Cannot forward both `prompt` and `prompt_embeds`.')
        if prompt is None and prompt_embeds is None:
            raise ValueError('Provide either `prompt` or `prompt_embeds`.')
        pe = self._teacher_text(prompt, prompt_embeds, prompt_embeds_mask, num_images_per_prompt, max_sequence_length)
        cond = dict(prompt_embeds=pe)
        if true_cfg_scale > 1.0:
            if negative_prompt is None and negative_prompt_embeds is None:
                raise ValueError('true_cfg_scale > 1 needs `negative_prompt` or `negative_prompt_embeds`')
            if negative_prompt_embeds is None and isinstance(negative_prompt, str):
                negative_prompt = [negative_prompt] * (pe.shape[0] // num_images_per_prompt)
            ne = self._teacher_text(negative_prompt, negative_prompt_embeds, negative_prompt_embeds_mask, num_images_per_prompt,
                                    max_sequence_length)
            if ne.shape[0] != pe.shape[0]:
                raise ValueError(f'{ne.shape[0]} negative prompts for {pe.shape[0]} prompts')
            cond['negative_prompt_embeds'] = ne
        out, hp, wp, edit = self._sample_teacher(cond, pe.shape[0], height, width, num_inference_steps, None, true_cfg_scale, generator,
                                                 latents, guidance_interval, orthogonal_guidance, sampler, h, edit, solver_order, solver_type)
        return self._finish(out, hp, wp, output_type, return_dict, edit, composite)
