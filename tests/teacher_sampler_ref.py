"""CPU restatement of the teacher's sampling loop (test helper, not a test module): the reference's ``GaussianFlow.forward_test``
(lakonlab/models/diffusions/gaussian_flow.py:149-222) with its default ``FlowEulerODE`` sampler
(schedulers/flow_euler_ode.py:76-91,141-150) and ``guidance_jit`` (gaussian_flow.py:18-26), in fp32 (the reference's arithmetic)
or fp64 (the error-free evaluation of the same formulas).

    sigma grid (euler_sigmas)  ->  per step: positive forward, negative forward when guidance is active at t = sigma * num_timesteps
    ->  bias = (pos - neg)(scale - 1) [- orthogonal projection on pos]  ->  x <- x + (pos + bias)(sigma_next - sigma)

The reference stacks [negative; positive] into one 2B forward; here ``denoise(x, sigma, negative)`` is called once per half
(per-sample results are the same).  Layout-free: the orthogonal means run over every dimension but the first, which is the same
element set for [B, C, H, W] latents and [B, N, C] packed tokens.

Parity status: PINNED by tests/golden/g12_teacher_sampler.npz (tests/test_teacher_sampler_cpu.py).
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

Tensor = torch.Tensor


def euler_sigmas(num_steps: int, shift: float = 1.0, use_dynamic_shifting: bool = False, seq_len: Optional[int] = None,
                 base_seq_len: int = 256, max_seq_len: int = 4096, base_logshift: float = 0.5, max_logshift: float = 1.15,
                 terminal_sigma: Optional[float] = None, num_train_timesteps: int = 1000):
    """-> (sigmas [num_steps + 1] fp32 with the trailing 0, timesteps [num_steps] fp32)   (flow_euler_ode.py:58-91)."""
    s = torch.from_numpy(np.linspace(1, 0, num_steps, dtype=np.float32, endpoint=False))
    if use_dynamic_shifting and seq_len is not None:
        m = (max_logshift - base_logshift) / (max_seq_len - base_seq_len)
        shift = np.exp((seq_len - base_seq_len) * m + base_logshift)
    s = shift * s / (1 + (shift - 1) * s)
    if terminal_sigma is not None:
        om = 1 - s
        s = 1 - (om * (1 - terminal_sigma) / om[-1])
    return torch.cat([s, torch.zeros(1)]), s * num_train_timesteps


def guidance_bias(pos: Tensor, neg: Tensor, scale: float, orthogonal: bool = False) -> Tensor:
    """guidance_jit (gaussian_flow.py:18-26) in the dtype of its inputs."""
    bias = (pos - neg) * (scale - 1)
    if orthogonal:
        dim = list(range(1, pos.dim()))
        bias = bias - (bias * pos).mean(dim=dim, keepdim=True) / (pos * pos).mean(dim=dim, keepdim=True).clamp(min=1e-6) * pos
    return bias


def guidance_active(t: float, interval: Optional[Sequence[float]], num_timesteps: int = 1000) -> bool:
    """interval in t = sigma * num_timesteps units, both ends inclusive (gaussian_flow.py:180,200)."""
    lo, hi = (0, num_timesteps) if interval is None else interval
    return bool(lo <= t <= hi)


def euler_step(x: Tensor, u: Tensor, sigma: Tensor, sigma_to: Tensor) -> Tensor:
    """FlowEulerODEScheduler.step, prediction_type 'u' (flow_euler_ode.py:141-150)."""
    return x + u * (sigma_to - sigma)


def sample(denoise: Callable[[Tensor, float, bool], Tensor], noise: Tensor, sigmas: Tensor, guidance_scale: float = 1.0,
           guidance_interval: Optional[Sequence[float]] = None, orthogonal: bool = False, dtype=torch.float32,
           num_timesteps: int = 1000, trace: Optional[Dict[str, List]] = None) -> Tensor:
    """The loop of forward_test.  denoise(x_t, sigma, negative) -> velocity of the positive / negative conditioning.
    sigmas [n + 1] (euler_sigmas); dtype float32 (the reference) or float64.  trace (optional dict) receives ``x_t`` (the state
    after every step), ``active`` (whether guidance ran on the step) and ``negative_calls``."""
    x = noise.to(dtype)
    sig = sigmas.to(dtype)
    t_all = sigmas[:-1].float() * num_timesteps
    use_guidance = guidance_scale > 1.0
    if trace is not None:
        trace.update(x_t=[], active=[], negative_calls=0)
    for i in range(sigmas.numel() - 1):
        s = float(sigmas[i])
        active = use_guidance and guidance_active(float(t_all[i]), guidance_interval, num_timesteps)
        pos = denoise(x, s, False).to(dtype)
        u = pos
        if active:
            neg = denoise(x, s, True).to(dtype)
            u = pos + guidance_bias(pos, neg, guidance_scale, orthogonal)
        x = euler_step(x, u, sig[i], sig[i + 1])
        if trace is not None:
            trace['x_t'].append(x.clone())
            trace['active'].append(bool(active))
            trace['negative_calls'] += int(active)
    return x


def qwen_teacher_forward(D, w, cfg, hidden, ctx, timestep, hp, wp):
    """Plain Qwen-Image (teacher) forward on ``oracle.dit_ref`` (module ``D``): the oracle has the ArcFlow forward only, so the
    single ``proj_out`` head is evaluated as the first component of the means head of a weight set whose ``proj_out_means`` rows
    0..C-1 are ``proj_out`` (same trunk, same norm_out, same linear: oracle/dit_ref.py arc_heads)."""
    C = cfg.in_channels
    w2 = dict(w)
    for suf in ('weight', 'bias'):
        full = w['proj_out_means.' + suf].clone()
        full[:C] = w['proj_out.' + suf].to(full.dtype)
        w2['proj_out_means.' + suf] = full
    means, _, _ = D.qwen_forward(w2, cfg, hidden, ctx, timestep, hp, wp)
    return means[:, :, 0, :]
