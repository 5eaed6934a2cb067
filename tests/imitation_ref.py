"""CPU restatement of one data-mode distillation step (test helper, not a test module): the reference's
``ArcFlowImitation.forward_train`` (lakonlab/models/diffusions/arcflow.py:304-335) put together from ``oracle.arcflow_ref``.

    sample_t (arcflow.py:277-302)  ->  forward diffusion (gaussian_flow.py:83-88)  ->  the student's mixture at (x_t, sigma)
    ->  per sample: ``R.segment_distill`` with that sample's segment size  ->  mean of the per-sample losses

``R.segment_distill`` takes one float segment, so a batch whose samples sit on different segments is evaluated one sample at a
time; the flow loss is a mean over the samples of per-sample means (``R.flow_mse_loss``), so the mean of the per-sample losses IS
the batch loss of the reference's stacked call (no segment weight: arcflow.py:331).

Parity status: PINNED by tests/golden/g10_imitation_sample_t.npz and g11_imitation_step.npz (tests/test_imitation_cpu.py).
"""
from __future__ import annotations

import contextlib
from typing import Callable, Dict, List, Optional

import torch

from oracle import arcflow_ref as R

Tensor = torch.Tensor


def sample_t(u: Tensor, nfe: int, timestep_ratio: float = 1.0, shift: float = 3.2, eps: float = 1e-4):
    """u [B] uniforms -> (raw_t_src, sigma_t_src, segment_size, source index), all [B] (arcflow.py:277-302; the sampler's draw
    is raw_t = 1 - rand, sampler.py:68).  Index 1 is the final segment (scaled by ``timestep_ratio``), index nfe starts at 1."""
    ratio = max(timestep_ratio, eps)
    base = 1 / (nfe - (1 - ratio))
    raw_t = (1 - u).clamp(min=eps)
    idx = torch.ceil(raw_t / base + (1 - ratio)).clamp(min=1, max=nfe)
    raw_src = ((idx - (1 - ratio)) * base).clamp(min=eps, max=1)
    seg = torch.where(idx == 1, torch.tensor(ratio * base, dtype=raw_src.dtype), torch.tensor(base, dtype=raw_src.dtype))
    return raw_src, R.shift_sigma(raw_src, shift), seg, idx.long()


def forward_diffuse(x0: Tensor, noise: Tensor, sigma: Tensor) -> Tensor:
    """x_t = x0 (1 - sigma_b) + noise sigma_b   (gaussian_flow.py:83-88), x0 / noise [B, ...], sigma [B]."""
    s = sigma.reshape(-1, *([1] * (x0.dim() - 1))).to(x0.dtype)
    return x0 * (1 - s) + noise * s


@contextlib.contextmanager
def _tap(name: str, sink: List[Tensor]):
    """Record what ``R.<name>`` returns while the block runs (the per-state predicted velocities of segment_distill)."""
    orig = getattr(R, name)

    def wrapped(*a, **kw):
        out = orig(*a, **kw)
        sink.append(out.detach().clone())
        return out
    setattr(R, name, wrapped)
    try:
        yield
    finally:
        setattr(R, name, orig)


def imitation_step(teacher: Callable, policy: Callable, x0: Tensor, noise: Tensor, u: Tensor, teacher_ratio: float,
                   u_drop: Tensor, u_student: Tensor, u_teacher: Tensor, nfe: int, timestep_ratio: float = 1.0,
                   gm_dropout: float = 0.1, shift: float = 3.2, eps: float = 1e-4, total_substeps: int = 128,
                   window_substeps: int = 3, loss_scale: float = 30.0, trace: Optional[Dict[str, object]] = None) -> Tensor:
    """One data-mode step on latents x0 [B,C,H,W] with noise of the same shape.

    policy(x_t [B,C,H,W], sigma [B]) -> (means [B,K,C,H,W], logw [B,K,1,H,W], logg [B,K-1,1,H,W])  (differentiable)
    teacher(x_a [1,C,H,W], t [1], b) -> velocity of sample b
    u_drop [B,K,1,1,1], u_student [B,n], u_teacher [B,n-1]: the uniforms of piid_segment_momentum in the reference's draw order.
    trace (optional dict) receives x_t_src, raw_t_src, sigma_t_src, segment_size and per sample lists x_t_a / tgt_u / pred_u.
    Returns the loss (mean of the per-sample segment losses)."""
    B = x0.shape[0]
    raw_src, sigma_src, seg, _ = sample_t(u, nfe, timestep_ratio, shift, eps)
    x_t = forward_diffuse(x0, noise, sigma_src)
    means, logw, logg = policy(x_t, sigma_src)
    mask = R.gm_dropout_mask(u_drop, gm_dropout) if gm_dropout > 0 else None
    if trace is not None:
        trace.update(x_t_src=x_t.detach().clone(), raw_t_src=raw_src, sigma_t_src=sigma_src, segment_size=seg,
                     x_t_a=[], tgt_u=[], pred_u=[])
    losses = []
    for b in range(B):
        sl = slice(b, b + 1)
        xa, tg, pr = [], [], []

        def teacher_b(x_a, t, b=b, xa=xa, tg=tg):
            out = teacher(x_a, t, b)
            xa.append(x_a.detach().clone())
            tg.append(out.detach().clone())
            return out
        with _tap('mean_velocity', pr):
            loss_b, _, _ = R.segment_distill(teacher_b, x_t[sl], means[sl], logw[sl], logg[sl], raw_src[sl], teacher_ratio,
                                             float(seg[b]), u_student[sl], u_teacher[sl],
                                             drop_mask=None if mask is None else mask[sl], total_substeps=total_substeps,
                                             window_substeps=window_substeps, shift=shift, eps=eps, loss_scale=loss_scale)
        losses.append(loss_b)
        if trace is not None:
            trace['x_t_a'].append(torch.cat(xa))        # [n, C, H, W] of sample b
            trace['tgt_u'].append(torch.cat(tg))
            trace['pred_u'].append(torch.cat(pr))
    return torch.stack(losses).mean()
