"""Training-time evaluation: does the few-step student, started from the same noise, land where the frozen teacher's many-step ODE lands?

The reference answers this with ``eval_interval`` / ``test_cfg`` / ``val_step`` (lakonlab/models/latent_diffusion_text_image.py:108-170,
``ArcFlowImitationBase.forward_test``, arcflow.py:211-271), which saves decoded images for metrics computed elsewhere.  Here the two
sample sets are scored against each other on the device: ``Evaluator`` holds a fixed set of conditions, one fixed start noise per
condition (a private generator: the training draws are untouched) and -- the teacher being frozen and the noise fixed -- the teacher's
latents for that noise, computed on the first call and kept.  Every later evaluation costs the student's ``nfe`` forwards and one
scoring pass.

What is scored: the packed latents (what the distillation loss acts on; no decoder needed) and, with a VAE decoder, the decoded images
in the [0, 1] range of the reference's ``val_step``.  The per-sample sums come from ONE kernel, ``afx_sample_score`` (fp64
accumulation, fixed partition, ordered second pass: bit-reproducible); ``metrics_from_sums`` turns them into numbers on the host.
MSE and PSNR are per-pixel; the decoded images are also scored structurally, by ``afx_image_ssim`` (the 11 x 11 Gaussian-window SSIM
in fp64, the same reduction scheme) and ``ssim_from_sums``.
The student's sampling semantics are the pipelines' ``__call__`` (``ArcFlowDistiller.sample_student``); ``temperature`` plays no part.
"""
from __future__ import annotations

import contextlib
import math
from typing import Any, Dict, List, Optional, Sequence

import torch

from .. import ops

LATENT_KEYS = ('latent_mse', 'latent_rel_l2', 'latent_cosine')
IMAGE_KEYS = ('image_psnr', 'image_mse', 'image_ssim')
SSIM_WINDOW = 11          # the taps of afx_image_ssim's Gaussian window: the smallest image side it scores


def metrics_from_sums(sums, n: int, data_range: Optional[float] = None) -> Dict[str, torch.Tensor]:
    """sums [B, 4] = (S_dd, S_aa, S_bb, S_ab) per sample -- sum (a-b)^2, sum a^2, sum b^2, sum a b over n elements, b the teacher --
    -> fp64 CPU tensors [B]:
        mse    = S_dd / n
        rel_l2 = sqrt(S_dd / max(S_bb, 1e-30))
        cosine = S_ab / sqrt(max(S_aa S_bb, 1e-60))
        psnr   = 10 log10(data_range^2 / max(mse, 1e-30))        only with ``data_range`` (1.0 for images in [0, 1])
    The floors keep every result finite for b = 0 and a = b (psnr is capped at 10 log10(data_range^2) + 300 dB)."""
    s = torch.as_tensor(sums).detach().to('cpu', torch.float64).reshape(-1, 4)
    dd, aa, bb, ab = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    mse = dd / float(n)
    out = dict(mse=mse, rel_l2=torch.sqrt(dd / bb.clamp(min=1e-30)), cosine=ab / torch.sqrt((aa * bb).clamp(min=1e-60)))
    if data_range is not None:
        out['psnr'] = 10.0 * torch.log10(float(data_range) ** 2 / mse.clamp(min=1e-30))
    return out


def ssim_from_sums(sums, channels: int, height: int, width: int) -> torch.Tensor:
    """sums [B] = afx_image_ssim's per-sample sum of the window ratios over ``channels`` planes of ``height`` x ``width`` -> the mean SSIM
    per sample, fp64 CPU [B]: sums / (channels (height - 10)(width - 10)), the number of windows that lie inside the image."""
    if channels < 1 or height < SSIM_WINDOW or width < SSIM_WINDOW:
        raise ValueError(f'ssim_from_sums: no {SSIM_WINDOW} x {SSIM_WINDOW} window fits {channels} x {height} x {width}')
    s = torch.as_tensor(sums).detach().to('cpu', torch.float64).reshape(-1)
    return s / float(channels * (height - SSIM_WINDOW + 1) * (width - SSIM_WINDOW + 1))


class Evaluator:
    """``evaluate() -> dict``: per-sample lists ``latent_mse``, ``latent_rel_l2``, ``latent_cosine`` (+ ``image_psnr``, ``image_mse`` with a
    ``vae``, + ``image_ssim`` where the decoded images are [B, C, H, W] with H, W >= 11), their means as ``<key>_mean``, ``iteration`` and
    ``seconds`` (HIP events around the call).

    distiller: an ArcFlowDistiller.  conds: a list of per-batch condition dicts as ``train_step`` takes them.  seed: condition i draws its
    start noise from ``torch.Generator(device).manual_seed(seed + i)``, once.  teacher_steps / teacher_kwargs: ``sample_teacher``'s
    ``num_steps`` and further keywords.  nfe / timestep_ratio: ``sample_student``'s (None: the training values).  use_ema: score the EMA
    weights (one exchange around the whole evaluation).  vae: a decoder with ``decode_packed(latents, hp, wp)``."""

    def __init__(self, distiller, conds: Sequence[Dict[str, Any]], *, seed: int = 0, teacher_steps: int = 28,
                 teacher_kwargs: Optional[Dict[str, Any]] = None, nfe: Optional[int] = None, timestep_ratio: Optional[float] = None,
                 use_ema: bool = True, vae=None):
        if len(conds) == 0:
            raise ValueError('Evaluator needs at least one condition batch')
        self.distiller, self.conds = distiller, list(conds)
        self.seed, self.teacher_steps, self.teacher_kwargs = int(seed), int(teacher_steps), dict(teacher_kwargs or {})
        self.nfe, self.timestep_ratio, self.use_ema, self.vae = nfe, timestep_ratio, bool(use_ema), vae
        dev = distiller.device
        self.noise: List[torch.Tensor] = []
        for i, c in enumerate(self.conds):
            g = torch.Generator(device=dev).manual_seed(self.seed + i)
            self.noise.append(torch.randn(c['prompt_embeds'].shape[0], c['hp'] * c['wp'], distiller.C, device=dev, generator=g))
        self.teacher_latents: List[Optional[torch.Tensor]] = [None] * len(self.conds)
        self.teacher_images: List[Optional[torch.Tensor]] = [None] * len(self.conds)

    def _teacher(self, i: int):
        """Teacher latents (and decoded images) of condition i for its fixed noise: computed once, then read."""
        if self.teacher_latents[i] is None:
            c = self.conds[i]
            self.teacher_latents[i] = self.distiller.sample_teacher(c, self.noise[i], num_steps=self.teacher_steps, **self.teacher_kwargs)
            if self.vae is not None:
                self.teacher_images[i] = self.vae.decode_packed(self.teacher_latents[i], c['hp'], c['wp']).contiguous()
        return self.teacher_latents[i], self.teacher_images[i]

    @torch.no_grad()
    def evaluate(self) -> Dict[str, Any]:
        d = self.distiller
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        lat_sums, img_sums = [], []            # (sums [B, 4] on the device, elements per sample) per condition
        ssim_sums = []                         # (sums [B] on the device, C, H, W) per condition -- only where a window fits the decoded images
        with d.ema_weights() if self.use_ema else contextlib.nullcontext():
            for i, c in enumerate(self.conds):
                t_lat, t_img = self._teacher(i)
                s_lat = d.sample_student(c, self.noise[i], self.nfe, self.timestep_ratio)
                lat_sums.append((ops.sample_score(s_lat, t_lat), s_lat[0].numel()))                 # a = student, b = teacher
                if self.vae is not None:
                    s_img = self.vae.decode_packed(s_lat, c['hp'], c['wp']).contiguous()
                    img_sums.append((ops.sample_score(s_img, t_img, transform=True), s_img[0].numel()))
                    if s_img.dim() == 4 and min(s_img.shape[2:]) >= SSIM_WINDOW:
                        ssim_sums.append((ops.image_ssim(s_img, t_img, transform=True, data_range=1.0), *s_img.shape[1:]))
        end.record()
        end.synchronize()
        out: Dict[str, Any] = dict(iteration=int(d.iteration))
        lat = [metrics_from_sums(s, n) for s, n in lat_sums]
        for key in LATENT_KEYS:
            out[key] = [v for m in lat for v in m[key[len('latent_'):]].tolist()]
        if self.vae is not None:
            img = [metrics_from_sums(s, n, data_range=1.0) for s, n in img_sums]
            for key in ('image_psnr', 'image_mse'):
                out[key] = [v for m in img for v in m[key[len('image_'):]].tolist()]
            if len(ssim_sums) == len(self.conds):          # every condition's images took a window (a stand-in decoder of another shape: no key)
                out['image_ssim'] = [v for s, ch, h, w in ssim_sums for v in ssim_from_sums(s, ch, h, w).tolist()]
        for key in [k for k in out if k != 'iteration']:
            out[key + '_mean'] = math.fsum(out[key]) / len(out[key])
        out['seconds'] = start.elapsed_time(end) / 1000.0
        return out
