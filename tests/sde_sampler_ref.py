"""CPU restatement of the teacher's STOCHASTIC sampling loop (test helper, not a test module): the reference's
``GaussianFlow.forward_test`` (lakonlab/models/diffusions/gaussian_flow.py:149-222) with ``sampler='FlowSDE'``
(schedulers/flow_sde.py:143-166), in fp32 (the reference's arithmetic) or fp64 (the error-free evaluation of the same formulas).
The grid, the guidance bias and the interval rule are tests/teacher_sampler_ref.py's (the two schedulers share their tables).

    per step:  u as in the ODE loop  ->  x0 = x - sigma u,  eps = x + (1 - sigma) u
               m = 0 (h = 'inf') | 1 (h = 0) | (sigma_to (1 - sigma) / max(sigma (1 - sigma_to), 1e-6)) ^ (h^2)
               x <- (1 - sigma_to) x0 + sigma_to (m eps + sqrt(max(1 - m^2, 0)) z_i),      z_i the step's N(0, 1) draw

``m`` is always evaluated in fp32 from the fp32 table, as the scheduler does (its sigmas are fp32 whatever the latents are); the fp64
loop then uses that fp32 value exactly -- the same per-step scalars the fused kernel is handed.

Parity status: PINNED by tests/golden/g13_sde_sampler.npz (tests/test_sde_sampler_cpu.py).
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import torch

from tests import teacher_sampler_ref as TS

Tensor = torch.Tensor


def sde_coefficients(sigma: Tensor, sigma_to: Tensor, h: Union[float, str]) -> Tuple[Tensor, Tensor]:
    """-> (m, sqrt(max(1 - m^2, 0))) in the dtype of sigma (flow_sde.py:157-166)."""
    if h == 'inf':
        m = torch.zeros_like(sigma)
    elif h == 0.0:
        m = torch.ones_like(sigma)
    else:
        assert h > 0.0
        m = (sigma_to * (1 - sigma) / (sigma * (1 - sigma_to)).clamp(min=1e-6)) ** (h * h)
    return m, (1 - m.square()).clamp(min=0).sqrt()


def sde_step(x: Tensor, u: Tensor, sigma: Tensor, sigma_to: Tensor, m: Tensor, c_noise: Tensor, z: Tensor) -> Tensor:
    """FlowSDEScheduler.step, prediction_type 'u' (flow_sde.py:143-166), in the dtype of x."""
    alpha, alpha_to = 1 - sigma, 1 - sigma_to
    x0 = x - sigma * u
    eps = x + alpha * u
    return alpha_to * x0 + sigma_to * (m * eps + c_noise * z)


def sample(denoise: Callable[[Tensor, float, bool], Tensor], noise: Tensor, sigmas: Tensor, step_noise: Tensor, h: Union[float, str] = 1.0,
           guidance_scale: float = 1.0, guidance_interval: Optional[Sequence[float]] = None, orthogonal: bool = False,
           dtype=torch.float32, num_timesteps: int = 1000, trace: Optional[Dict[str, List]] = None) -> Tensor:
    """The loop of forward_test with the FlowSDE sampler.  denoise(x_t, sigma, negative) -> velocity; sigmas [n + 1] fp32
    (teacher_sampler_ref.euler_sigmas); step_noise [n, ...] the per-step draws; dtype float32 (the reference) or float64.
    trace (optional dict) receives ``x_t`` (the state after every step), ``m`` and ``c_noise`` (fp32 scalars per step)."""
    x = noise.to(dtype)
    sig = sigmas.to(dtype)
    t_all = sigmas[:-1].float() * num_timesteps
    use_guidance = guidance_scale > 1.0
    if trace is not None:
        trace.update(x_t=[], m=[], c_noise=[])
    for i in range(sigmas.numel() - 1):
        s = float(sigmas[i])
        active = use_guidance and TS.guidance_active(float(t_all[i]), guidance_interval, num_timesteps)
        pos = denoise(x, s, False).to(dtype)
        u = pos
        if active:
            neg = denoise(x, s, True).to(dtype)
            u = pos + TS.guidance_bias(pos, neg, guidance_scale, orthogonal)
        m, c = sde_coefficients(sigmas[i].float(), sigmas[i + 1].float(), h)
        x = sde_step(x, u, sig[i], sig[i + 1], m.to(dtype), c.to(dtype), step_noise[i].to(dtype))
        if trace is not None:
            trace['x_t'].append(x.clone())
            trace['m'].append(m)
            trace['c_noise'].append(c)
    return x
