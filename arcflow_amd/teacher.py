"""Teacher sampling: the Euler ODE loop with true classifier-free guidance that the reference runs in
``GaussianFlow.forward_test`` (lakonlab/models/diffusions/gaussian_flow.py:149-222) with its ``FlowEulerODEScheduler``
(schedulers/flow_euler_ode.py) -- what the student is judged against, and a source of latents for the data mode.

Per step: the positive teacher forward, the negative one when guidance is active on that step, the projection coefficient of
orthogonal guidance (``afx_cfg_ortho_coef``, orthogonal only) and ONE step kernel (``afx_teacher_euler_step``) that combines the
two bf16 velocities, advances the fp32 latents in place and writes the bf16 copy the next forward reads.  No torch arithmetic
runs inside the loop; the latents never leave the packed token layout.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence

import torch

from . import ops
from .engine import MMDiTEngine
from .schedule import FlowEulerODEScheduler


class TeacherSampler:
    """``sampler(cond, noise) -> latents``: noise / latents [B, N, C] fp32 packed tokens.

    engine: a ``teacher_head=True`` MMDiTEngine.
    cond: ``prompt_embeds`` [B, T, joint] (+ ``pooled`` for FLUX), ``hp``, ``wp``, and for true CFG ``negative_prompt_embeds``
    (+ ``negative_pooled``) -- the dict ``ArcFlowDistiller.train_step`` takes.
    guidance_scale: true CFG, active only when > 1.0 (the reference's ``use_guidance``); distilled_guidance: the value of the
    FLUX guidance embedding (ignored by engines without one); guidance_interval: [lo, hi] in t = sigma * num_train_timesteps,
    both inclusive -- outside it the negative forward is skipped; orthogonal_guidance: remove from the guidance term its projection
    on the positive velocity (guidance_jit).  scheduler_kwargs go to FlowEulerODEScheduler (shift, use_dynamic_shifting,
    terminal_sigma ...); its ``seq_len`` is the number of latent pixels 4 hp wp, as the reference counts it
    (gaussian_flow.py:186 on [B, C, H, W] latents), or with ``tokens_as_seq_len`` the number of tokens hp wp, which is what a
    diffusers scheduler config's ``base_image_seq_len`` / ``max_image_seq_len`` are written for (the pipelines pass it).
    prepare_steps=False evaluates the modulation vectors per forward (the plain path; same numbers)."""

    def __init__(self, engine: MMDiTEngine, num_steps: int = 28, guidance_scale: float = 1.0, distilled_guidance: Optional[float] = None,
                 guidance_interval: Optional[Sequence[float]] = None, orthogonal_guidance: bool = False,
                 num_train_timesteps: int = 1000, prepare_steps: bool = True, tokens_as_seq_len: bool = False, **scheduler_kwargs: Any):
        if not engine.teacher_head:
            raise ValueError('TeacherSampler needs a teacher_head=True engine (a single velocity, not an ArcFlow policy)')
        if num_steps < 1:
            raise ValueError('num_steps must be >= 1')
        self.engine, self.num_steps = engine, int(num_steps)
        self.guidance_scale, self.distilled_guidance = float(guidance_scale), distilled_guidance
        self.guidance_interval = None if guidance_interval is None else (float(guidance_interval[0]), float(guidance_interval[1]))
        self.orthogonal_guidance = bool(orthogonal_guidance)
        self.prepare_steps = bool(prepare_steps)
        self.tokens_as_seq_len = bool(tokens_as_seq_len)
        self.scheduler = FlowEulerODEScheduler(num_train_timesteps, **scheduler_kwargs)

    # ------------------------------------------------------------------ schedule
    def schedule(self, hp: int, wp: int):
        """-> (sigmas [num_steps + 1] fp32 with the trailing 0, active [num_steps] bools: true CFG runs on that step)."""
        sch = self.scheduler
        sch.set_timesteps(self.num_steps, seq_len=hp * wp * (1 if self.tokens_as_seq_len else 4))
        lo, hi = (0.0, float(sch.config.num_train_timesteps)) if self.guidance_interval is None else self.guidance_interval
        use = self.guidance_scale > 1.0
        active = [bool(use and lo <= t <= hi) for t in sch.timesteps.tolist()]
        return sch.sigmas.clone(), active

    # ------------------------------------------------------------------ one step
    def step(self, x: torch.Tensor, x_bf16: torch.Tensor, cond: Dict[str, Any], sigma: torch.Tensor, sigma_to: torch.Tensor,
             active: bool, prepared_step: Optional[int] = None, scratch: Optional[dict] = None) -> None:
        """Advance x (fp32, in place) and x_bf16 (its rounding, in place) from sigma [B] to sigma_to [B]."""
        eng = self.engine
        B = x.shape[0]
        s = scratch if scratch is not None else {}
        g = s.get('guidance')
        if g is None and eng.guidance_embeds and self.distilled_guidance is not None:
            g = s['guidance'] = torch.full((B,), float(self.distilled_guidance), dtype=torch.float32, device=x.device)
        pooled, npooled = cond.get('pooled'), cond.get('negative_pooled')
        pos = eng.forward(x_bf16, sigma, cond['prompt_embeds'], pooled, g, cond['hp'], cond['wp'], prepared_step=prepared_step)
        neg = coef = None
        if active:
            # the negative pass may reuse the prepared vectors when the conditioning does not see the prompt (Qwen-Image: timestep only)
            neg_prep = prepared_step if pooled is None and npooled is None else None
            neg = eng.forward(x_bf16, sigma, cond['negative_prompt_embeds'], npooled, g, cond['hp'], cond['wp'], prepared_step=neg_prep)
            if self.orthogonal_guidance:
                if 'coef' not in s:
                    s['coef'] = torch.empty(B, dtype=torch.float32, device=x.device)
                    s['ws'] = ops.cfg_ortho_ws(B, x[0].numel(), x.device)
                coef = ops.cfg_ortho_coef(pos, neg, self.guidance_scale, out=s['coef'], ws=s['ws'])
        ops.teacher_euler_step(x, pos, neg, sigma, sigma_to, self.guidance_scale, coef, out=x, out_bf16=x_bf16)

    # ------------------------------------------------------------------ the loop
    def _roll(self, cond: Dict[str, Any], noise: torch.Tensor) -> torch.Tensor:
        eng = self.engine
        B, N, _ = noise.shape
        hp, wp = cond['hp'], cond['wp']
        dev = eng.device
        # conditioning on the device in the engine's dtype once, so that no cast runs per forward
        cond = {k: (v.to(dev, torch.bfloat16).contiguous() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in cond.items()}
        sigmas, active = self.schedule(hp, wp)
        sig = sigmas[:, None].expand(-1, B).contiguous().to(dev)             # [num_steps + 1, B]: row i is the per-sample sigma of step i
        x = noise.to(dev, torch.float32).clone().contiguous()
        xb = x.to(torch.bfloat16)
        T = cond['prompt_embeds'].shape[1]
        if any(active):
            T = max(T, cond['negative_prompt_embeds'].shape[1])
        eng._workspace(B, N, T)           # sized for both prompts up front: a workspace that grows mid-loop would drop the prepared steps
        chunk = min(max(8 // B, 1), self.num_steps) if self.prepare_steps else 0
        scratch: dict = {}
        g = None
        if eng.guidance_embeds and self.distilled_guidance is not None:
            g = scratch['guidance'] = torch.full((B,), float(self.distilled_guidance), dtype=torch.float32, device=dev)
        prepared = False
        for i in range(self.num_steps):
            if chunk > 1 and i % chunk == 0:
                prepared = eng.prepare_steps(sig[i:min(i + chunk, self.num_steps)], cond.get('pooled'), g, B, N, T)
            self.step(x, xb, cond, sig[i], sig[i + 1], active[i], (i % chunk) if (chunk > 1 and prepared) else None, scratch)
        return x

    @torch.no_grad()
    def __call__(self, cond: Dict[str, Any], noise: torch.Tensor) -> torch.Tensor:
        if noise.dim() != 3:
            raise ValueError(f'noise: need packed tokens [B, N, C], got {tuple(noise.shape)}')
        if noise.shape[1] != cond['hp'] * cond['wp']:
            raise ValueError(f'noise has {noise.shape[1]} tokens but cond says {cond["hp"]} x {cond["wp"]}')
        if self.guidance_scale > 1.0 and 'negative_prompt_embeds' not in cond:
            raise ValueError('guidance_scale > 1 (true CFG) needs cond["negative_prompt_embeds"]')
        B = noise.shape[0]
        if B <= 4:
            return self._roll(cond, noise)
        # the engine's prepared steps hold at most 4 samples: larger batches run as micro-batches of 4 (per-sample results are the same)
        outs: List[torch.Tensor] = []
        for a in range(0, B, 4):
            mb = {k: (v[a:a + 4] if isinstance(v, torch.Tensor) and v.dim() > 0 and v.shape[0] == B else v) for k, v in cond.items()}
            outs.append(self._roll(mb, noise[a:a + 4]))
        return torch.cat(outs)
