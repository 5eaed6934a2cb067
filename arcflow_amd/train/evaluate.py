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


def masked_metrics_from_sums(sums, data_range: Optional[float] = None) -> List[Dict[str, torch.Tensor]]:
    """sums [B, 2, 5] = afx_sample_score_masked's (S_w, S_dd, S_aa, S_bb, S_ab) per sample and region -- the weighted sums, region 0
    repainted (weight m), region 1 kept (weight 1 - m), b the teacher -- -> [repainted, kept], each a dict of fp64 CPU tensors [B]:
        weight = S_w
        mse    = S_dd / max(S_w, 1e-300)
        rel_l2, cosine as ``metrics_from_sums`` (the weights cancel)
        psnr   = 10 log10(data_range^2 / max(mse, 1e-30))        only with ``data_range``
    A region of weight 0 (a mask that is 0 or 1 everywhere) has no elements: every metric of it is NaN, its weight 0."""
    s = torch.as_tensor(sums).detach().to('cpu', torch.float64).reshape(-1, 2, 5)
    nan = torch.full((s.shape[0],), float('nan'), dtype=torch.float64)
    out = []
    for g in range(2):
        w, dd, aa, bb, ab = (s[:, g, k] for k in range(5))
        empty = w <= 0
        mse = dd / w.clamp(min=1e-300)
        m = dict(weight=w, mse=mse, rel_l2=torch.sqrt(dd / bb.clamp(min=1e-30)), cosine=ab / torch.sqrt((aa * bb).clamp(min=1e-60)))
        if data_range is not None:
            m['psnr'] = 10.0 * torch.log10(float(data_range) ** 2 / mse.clamp(min=1e-30))
        out.append({k: (v if k == 'weight' else torch.where(empty, nan, v)) for k, v in m.items()})
    return out


def masked_ssim_from_sums(sums):
    """sums [B, 4] = afx_image_ssim_masked's (sum w ssim, sum w, sum (1 - w) ssim, sum (1 - w)) -> (ssim_repaint, ssim_keep), the weighted
    mean SSIM of either region per sample, fp64 CPU [B]: S / max(S_w, 1e-300), NaN for a region whose weight is 0."""
    s = torch.as_tensor(sums).detach().to('cpu', torch.float64).reshape(-1, 4)
    nan = torch.full((s.shape[0],), float('nan'), dtype=torch.float64)
    return tuple(torch.where(s[:, k + 1] <= 0, nan, s[:, k] / s[:, k + 1].clamp(min=1e-300)) for k in (0, 2))


def edit_mask(kind: str, batch: int, hp: int, wp: int, device='cpu') -> torch.Tensor:
    """The named masks of ``eval_cfg['edit_mask']``, image resolution [batch, 1, 16 hp, 16 wp] fp32, 1 = repaint: 'box' the centred
    rectangle of half the side, 'left' the left half."""
    H, W = 16 * hp, 16 * wp
    m = torch.zeros(batch, 1, H, W, dtype=torch.float32, device=device)
    if kind == 'box':
        m[:, :, H // 4:H // 4 + H // 2, W // 4:W // 4 + W // 2] = 1.0
    elif kind == 'left':
        m[:, :, :, :W // 2] = 1.0
    else:
        raise ValueError(f"edit_mask: 'box' or 'left', got {kind!r}")
    return m


EDIT_LATENT_KEYS = ('edit_latent_mse', 'edit_latent_rel_l2', 'edit_latent_cosine', 'edit_keep_latent_mse')
EDIT_IMAGE_KEYS = ('edit_image_psnr', 'edit_image_mse', 'edit_keep_image_psnr')
EDIT_SSIM_KEYS = ('edit_image_ssim', 'edit_keep_image_ssim')


class Evaluator:
    """``evaluate() -> dict``: per-sample lists ``latent_mse``, ``latent_rel_l2``, ``latent_cosine`` (+ ``image_psnr``, ``image_mse`` with a
    ``vae``, + ``image_ssim`` where the decoded images are [B, C, H, W] with H, W >= 11), their means as ``<key>_mean``, ``iteration`` and
    ``seconds`` (HIP events around the call).

    edits: score an edit of every condition as well -- None (nothing more is computed or returned), a dict ``mask=`` (image resolution
    [B or 1, 1, 16 hp, 16 wp] in [0, 1], or 'box' / 'left': ``edit_mask``), ``strength=`` in (0, 1] and optionally ``x0=`` (packed source
    latents [B, N, 64]; default: the teacher's own cached text-to-image latents of that condition, so no image is needed), or a list of one
    such dict per condition.  Student (``sample_student(x0=, mask=, strength=)``) and teacher (``sample_teacher(x0=, mask=, strength=)``,
    computed once and kept) start from a second fixed noise, ``manual_seed(seed + 7919 + i)``.  Added keys, weighted by the mask
    (``afx_sample_score_masked`` / ``afx_image_ssim_masked``; the token mask ``mask_to_tokens(mask, 'max')`` weights the latents, the image
    mask the images): ``edit_latent_mse`` / ``_rel_l2`` / ``_cosine`` (repainted region), ``edit_keep_latent_mse`` (kept region: exactly 0
    for a binary mask, both samplers re-impose the source at sigma 0), with a ``vae`` ``edit_image_psnr``, ``edit_image_mse``,
    ``edit_keep_image_psnr`` and, where a window fits, ``edit_image_ssim``, ``edit_keep_image_ssim``.

    distiller: an ArcFlowDistiller.  conds: a list of per-batch condition dicts as ``train_step`` takes them.  seed: condition i draws its
    start noise from ``torch.Generator(device).manual_seed(seed + i)``, once.  teacher_steps / teacher_kwargs: ``sample_teacher``'s
    ``num_steps`` and further keywords.  nfe / timestep_ratio: ``sample_student``'s (None: the training values).  use_ema: score the EMA
    weights (one exchange around the whole evaluation).  vae: a decoder with ``decode_packed(latents, hp, wp)``."""

    def __init__(self, distiller, conds: Sequence[Dict[str, Any]], *, seed: int = 0, teacher_steps: int = 28,
                 teacher_kwargs: Optional[Dict[str, Any]] = None, nfe: Optional[int] = None, timestep_ratio: Optional[float] = None,
                 use_ema: bool = True, vae=None, edits=None):
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
        self.edits = self._read_edits(edits)
        self.edit_noise: List[torch.Tensor] = []
        if self.edits is not None:
            for i, c in enumerate(self.conds):          # a second private generator: the plain start noise above is what it was
                g = torch.Generator(device=dev).manual_seed(self.seed + 7919 + i)
                self.edit_noise.append(torch.randn(c['prompt_embeds'].shape[0], c['hp'] * c['wp'], distiller.C, device=dev, generator=g))
        self.teacher_edit_latents: List[Optional[torch.Tensor]] = [None] * len(self.conds)
        self.teacher_edit_images: List[Optional[torch.Tensor]] = [None] * len(self.conds)

    def _read_edits(self, edits):
        """``edits`` -> None, or per condition dict(mask [B or 1, 1, 16 hp, 16 wp] fp32 on the device, tokens [B or 1, N, 4], strength, x0 or None)."""
        from ..schedule import mask_to_tokens
        if edits is None:
            return None
        if isinstance(edits, (str, dict)):
            edits = [edits] * len(self.conds)
        if len(edits) != len(self.conds):
            raise ValueError(f'edits: one dict per condition, got {len(edits)} for {len(self.conds)} conditions')
        dev, out = self.distiller.device, []
        for c, e in zip(self.conds, edits):
            e = dict(mask=e) if isinstance(e, str) else dict(e)
            unknown = set(e) - {'mask', 'strength', 'x0'}
            if unknown or 'mask' not in e:
                raise ValueError(f"edits: a dict of mask=, strength= and optionally x0=; got keys {sorted(e)}")
            B, hp, wp = c['prompt_embeds'].shape[0], c['hp'], c['wp']
            mask = edit_mask(e['mask'], 1, hp, wp) if isinstance(e['mask'], str) else e['mask']
            if mask.dim() != 4 or mask.shape[0] not in (1, B) or tuple(mask.shape[1:]) != (1, 16 * hp, 16 * wp):
                raise ValueError(f'edits: mask must be [{B} or 1, 1, {16 * hp}, {16 * wp}], got {tuple(mask.shape)}')
            mask = mask.to(dev, torch.float32).contiguous()
            if not bool(((mask >= 0) & (mask <= 1)).all()):
                raise ValueError('edits: mask values must lie in [0, 1]')
            strength = float(e.get('strength', 0.8))
            if not 0.0 < strength <= 1.0:
                raise ValueError(f'edits: strength must be in (0, 1], got {strength}')
            x0 = e.get('x0')
            if x0 is not None:
                if tuple(x0.shape) != (B, hp * wp, self.distiller.C):
                    raise ValueError(f'edits: x0 must be packed latents [{B}, {hp * wp}, {self.distiller.C}], got {tuple(x0.shape)}')
                x0 = x0.to(dev, torch.float32).contiguous()
            out.append(dict(mask=mask, tokens=mask_to_tokens(mask, hp, wp, 'max'), strength=strength, x0=x0))
        return out

    def _teacher_edit(self, i: int):
        """(source latents, teacher's edited latents, their decoded images) of condition i for its fixed edit noise: the teacher's edit is
        computed once, then read.  The source defaults to the teacher's own cached text-to-image latents of the condition."""
        c, e = self.conds[i], self.edits[i]
        x0 = e['x0'] if e['x0'] is not None else self._teacher(i)[0]
        if self.teacher_edit_latents[i] is None:
            B = x0.shape[0]
            self.teacher_edit_latents[i] = self.distiller.sample_teacher(c, self.edit_noise[i], num_steps=self.teacher_steps, x0=x0,
                                                                         mask=e['tokens'].expand(B, -1, -1).contiguous(),
                                                                         strength=e['strength'], **self.teacher_kwargs)
            if self.vae is not None:
                self.teacher_edit_images[i] = self.vae.decode_packed(self.teacher_edit_latents[i], c['hp'], c['wp']).contiguous()
        return x0, self.teacher_edit_latents[i], self.teacher_edit_images[i]

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
        edit_lat, edit_img, edit_ssim = [], [], []          # masked sums [B, 2, 5], [B, 2, 5], [B, 4] on the device per condition (edits only)
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
                if self.edits is not None:
                    e = self.edits[i]
                    x0, te_lat, te_img = self._teacher_edit(i)
                    se_lat = d.sample_student(c, self.edit_noise[i], self.nfe, self.timestep_ratio, x0=x0, mask=e['tokens'], strength=e['strength'])
                    edit_lat.append(ops.sample_score_masked(se_lat, te_lat, e['tokens']))
                    if self.vae is not None:
                        se_img = self.vae.decode_packed(se_lat, c['hp'], c['wp']).contiguous()
                        if se_img.dim() != 4 or tuple(se_img.shape[2:]) != tuple(e['mask'].shape[2:]):
                            raise ValueError(f"edits: the decoded images are {tuple(se_img.shape)}, the mask is {tuple(e['mask'].shape)}: "
                                             'the image metrics of an edit need images at the mask\'s resolution')
                        edit_img.append(ops.sample_score_masked(se_img, te_img, e['mask'], transform=True))
                        if min(se_img.shape[2:]) >= SSIM_WINDOW:
                            edit_ssim.append(ops.image_ssim_masked(se_img, te_img, e['mask'], transform=True, data_range=1.0))
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
        if self.edits is not None:
            cat = lambda ms, g, name: [v for m in ms for v in m[g][name].tolist()]          # noqa: E731
            lat = [masked_metrics_from_sums(s) for s in edit_lat]
            out['edit_latent_mse'], out['edit_latent_rel_l2'] = cat(lat, 0, 'mse'), cat(lat, 0, 'rel_l2')
            out['edit_latent_cosine'], out['edit_keep_latent_mse'] = cat(lat, 0, 'cosine'), cat(lat, 1, 'mse')
            if self.vae is not None:
                img = [masked_metrics_from_sums(s, data_range=1.0) for s in edit_img]
                out['edit_image_psnr'], out['edit_image_mse'] = cat(img, 0, 'psnr'), cat(img, 0, 'mse')
                out['edit_keep_image_psnr'] = cat(img, 1, 'psnr')
                if len(edit_ssim) == len(self.conds):
                    pairs = [masked_ssim_from_sums(s) for s in edit_ssim]
                    out['edit_image_ssim'] = [v for p in pairs for v in p[0].tolist()]
                    out['edit_keep_image_ssim'] = [v for p in pairs for v in p[1].tolist()]
        for key in [k for k in out if k != 'iteration']:
            out[key + '_mean'] = math.fsum(out[key]) / len(out[key])
        out['seconds'] = start.elapsed_time(end) / 1000.0
        return out
