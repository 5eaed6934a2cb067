"""Teacher sampling: the loop with true classifier-free guidance that the reference runs in ``GaussianFlow.forward_test``
(lakonlab/models/diffusions/gaussian_flow.py:149-222) with one of its own schedulers, chosen by name as ``test_cfg['sampler']`` does:
``FlowEulerODEScheduler`` (schedulers/flow_euler_ode.py, the default), the stochastic ``FlowSDEScheduler`` (schedulers/flow_sde.py) or,
as ``'UniPC'``, the multistep solver behind ``FlowAdapterScheduler`` (schedulers/flow_adapter.py on its default base scheduler;
``schedule.FlowUniPCScheduler``) -- what the student is judged against, and a source of latents for the data mode.

Per step: the positive teacher forward, the negative one when guidance is active on that step, the projection coefficient of
orthogonal guidance (``afx_cfg_ortho_coef``, orthogonal only) and ONE step kernel (``afx_teacher_euler_step`` /
``afx_teacher_sde_step`` / ``afx_teacher_unipc_step``) that combines the two bf16 velocities, advances the fp32 latents in place and writes the bf16 copy the next
forward reads.  No torch arithmetic runs inside the loop -- with FlowSDE, nothing but the step's N(0, 1) draw, which stays torch's so
that a ``torch.Generator`` reproduces a run; the latents never leave the packed token layout.

Image editing (``x0=``, ``mask=``, ``strength=``): the same loop over a suffix of the schedule, started on the source
latents noised to the suffix's first sigma (``afx_edit_blend``); with a mask the step kernel is ``afx_teacher_edit_step`` /
``afx_teacher_sde_edit_step``, which also puts the kept region back on the source's own trajectory at the sigma the step lands on --
still one launch per step.  The reference has no image-conditioned sampling: these semantics follow the image-to-image / inpainting
pipelines of diffusers as recalled and are not pinned by a fixture.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence

import torch

from . import ops
from .engine import MMDiTEngine
from .schedule import FlowEulerODEScheduler, FlowSDEScheduler, FlowUniPCScheduler, truncate_by_strength

SAMPLERS = {'FlowEulerODE': FlowEulerODEScheduler, 'FlowSDE': FlowSDEScheduler, 'UniPC': FlowUniPCScheduler}


class TeacherSampler:
    """``sampler(cond, noise, generator=None, step_noise=None, x0=None, mask=None, strength=1.0) -> latents``: noise / latents
    [B, N, C] fp32 packed tokens.

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
    prepare_steps=False evaluates the modulation vectors per forward (the plain path; same numbers).
    sampler: 'FlowEulerODE' (the default) or 'FlowSDE', the scheduler class as the reference's ``test_cfg['sampler']`` names it;
    FlowSDE's ``h`` (a float or 'inf') travels in scheduler_kwargs.  With FlowSDE every step takes a fresh N(0, 1) draw of the latents'
    shape: from ``generator`` (one torch.randn per step, also on the steps whose draw is not read, so that the generator advances as in
    the reference), or from ``step_noise`` [num_steps, B, N, C].  With FlowEulerODE and UniPC both are accepted and ignored.
    'UniPC': the predictor-corrector multistep solver of FlowUniPCScheduler (``solver_order`` 1 / 2 (default) / 3, ``solver_type`` 'bh1' /
    'bh2', ``eps`` in scheduler_kwargs), one forward (pair) per step like the others; the step kernel afx_teacher_unipc_step also keeps
    the solver's state -- the corrected sample and a ring of ``solver_order`` past clean-sample predictions, allocated once per roll.

    Editing.  ``x0`` [B, N, 64] fp32, the packed latents of a source image, starts the roll from the image instead of from noise:
    with ``sigmas`` the full schedule of ``num_steps`` = n steps, ``schedule.truncate_by_strength`` gives t_start = int(max(n -
    min(n strength, n), 0)); the roll starts on (1 - s) x0 + s noise, s = sigmas[t_start] (at s = 1 that is ``noise`` itself), and runs
    the steps t_start .. n - 1.  ``strength`` in (0, 1]; 1.0 runs all n steps.  ``mask`` [B, N, 4] fp32 in [0, 1] (one value per latent
    pixel of the 2 x 2 patch, ``schedule.mask_to_tokens``; 1 = repaint, 0 = keep) needs ``x0``: after every step sigma -> sigma_to the
    kept region is set to (1 - sigma_to) x0 + sigma_to noise with the START noise (never a FlowSDE draw), so after the last step
    (sigma_to = 0) it is x0 bit for bit.  With FlowSDE one draw is made for every step that RUNS and none for the skipped ones: a
    generator advances n - t_start times, and ``step_noise`` is [n - t_start, B, N, C].  Guidance interval, orthogonal guidance, the
    prepared-step chunks and the micro-batches work as without an edit.  With UniPC a ``strength`` < 1 roll starts its suffix on an
    empty history (first order, then warming up), and ``mask`` is refused: re-imposing the kept region after a step would invalidate the
    history the next step extrapolates from, so inpainting stays with FlowEulerODE and FlowSDE."""

    def __init__(self, engine: MMDiTEngine, num_steps: int = 28, guidance_scale: float = 1.0, distilled_guidance: Optional[float] = None,
                 guidance_interval: Optional[Sequence[float]] = None, orthogonal_guidance: bool = False,
                 num_train_timesteps: int = 1000, prepare_steps: bool = True, tokens_as_seq_len: bool = False, sampler: str = 'FlowEulerODE',
                 **scheduler_kwargs: Any):
        if not engine.teacher_head:
            raise ValueError('TeacherSampler needs a teacher_head=True engine (a single velocity, not an ArcFlow policy)')
        if num_steps < 1:
            raise ValueError('num_steps must be >= 1')
        if sampler not in SAMPLERS:
            hint = " (the adapter's default base scheduler, UniPCMultistep, is sampler='UniPC' here)" if sampler == 'FlowAdapter' else ''
            raise ValueError(f'sampler: one of {sorted(SAMPLERS)}, got {sampler!r}{hint}')
        self.engine, self.num_steps = engine, int(num_steps)
        self.guidance_scale, self.distilled_guidance = float(guidance_scale), distilled_guidance
        self.guidance_interval = None if guidance_interval is None else (float(guidance_interval[0]), float(guidance_interval[1]))
        self.orthogonal_guidance = bool(orthogonal_guidance)
        self.prepare_steps = bool(prepare_steps)
        self.tokens_as_seq_len = bool(tokens_as_seq_len)
        self.sampler = sampler
        self.scheduler = SAMPLERS[sampler](num_train_timesteps, **scheduler_kwargs)

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
             active: bool, prepared_step: Optional[int] = None, scratch: Optional[dict] = None, m: Optional[torch.Tensor] = None,
             c_noise: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None, x0: Optional[torch.Tensor] = None,
             noise0: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, unipc: Optional[Dict[str, Any]] = None) -> None:
        """Advance x (fp32, in place) and x_bf16 (its rounding, in place) from sigma [B] to sigma_to [B].  FlowSDE: m, c_noise [B]
        (FlowSDEScheduler.coefficients) and the step's draw ``noise`` like x (None: no noise term on this step).  Inpainting: with
        ``mask`` [B, N, 4] the fused edit step re-imposes (1 - sigma_to) x0 + sigma_to noise0 where the mask is 0 (``noise0`` None on
        the step landing on sigma_to = 0); without a mask the plain step runs.  UniPC: ``unipc`` = the step's operands for
        ops.teacher_unipc_step (w, last, hist, last_out, hist_out); sigma_to is not read (the weights carry it)."""
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
        if self.sampler == 'UniPC':
            if unipc is None:
                raise ValueError('a UniPC step needs its weights and state buffers (FlowUniPCScheduler.coefficients)')
            if mask is not None:
                raise ValueError("mask: not with sampler='UniPC' (inpainting stays with FlowEulerODE and FlowSDE)")
            ops.teacher_unipc_step(x, pos, neg, unipc['w'], unipc['last'], unipc['hist'], unipc['last_out'], unipc['hist_out'],
                                   self.guidance_scale, coef, out=x, out_bf16=x_bf16)
        elif self.sampler == 'FlowSDE':
            if m is None or c_noise is None:
                raise ValueError('a FlowSDE step needs m and c_noise (FlowSDEScheduler.coefficients)')
            if mask is not None:
                ops.teacher_sde_edit_step(x, pos, neg, noise, sigma, sigma_to, m, c_noise, x0, noise0, mask, self.guidance_scale, coef,
                                          out=x, out_bf16=x_bf16)
            else:
                ops.teacher_sde_step(x, pos, neg, noise, sigma, sigma_to, m, c_noise, self.guidance_scale, coef, out=x, out_bf16=x_bf16)
        elif mask is not None:
            ops.teacher_edit_step(x, pos, neg, sigma, sigma_to, x0, noise0, mask, self.guidance_scale, coef, out=x, out_bf16=x_bf16)
        else:
            ops.teacher_euler_step(x, pos, neg, sigma, sigma_to, self.guidance_scale, coef, out=x, out_bf16=x_bf16)

    # ------------------------------------------------------------------ the draws of the stochastic sampler
    def _draw(self, shape, generator) -> torch.Tensor:
        """One step's N(0, 1) draw [B, N, C] fp32 on the engine's device.  A generator draws on its own device (a CPU generator gives
        the CPU stream); a list of generators draws one sample each."""
        dev = self.engine.device
        if isinstance(generator, (list, tuple)):
            if len(generator) != shape[0]:
                raise ValueError(f'{len(generator)} generators for a batch of {shape[0]}')
            return torch.cat([torch.randn((1,) + tuple(shape[1:]), device=g.device, dtype=torch.float32, generator=g).to(dev) for g in generator])
        gdev = generator.device if generator is not None else dev
        return torch.randn(tuple(shape), device=gdev, dtype=torch.float32, generator=generator).to(dev)

    # ------------------------------------------------------------------ the loop
    def _roll(self, cond: Dict[str, Any], noise: torch.Tensor, generator=None, step_noise: Optional[torch.Tensor] = None,
              x0: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, t_start: int = 0) -> torch.Tensor:
        eng = self.engine
        B, N, _ = noise.shape
        hp, wp = cond['hp'], cond['wp']
        dev = eng.device
        # conditioning on the device in the engine's dtype once, so that no cast runs per forward
        cond = {k: (v.to(dev, torch.bfloat16).contiguous() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in cond.items()}
        sigmas, active = self.schedule(hp, wp)
        sig = sigmas[:, None].expand(-1, B).contiguous().to(dev)             # [num_steps + 1, B]: row i is the per-sample sigma of step i
        sde = self.sampler == 'FlowSDE'
        if sde:
            # the scheduler's per-step scalars, once: rows [num_steps, B] of m and c_noise, and whether the step's draw is read at all
            co = torch.stack([torch.stack(self.scheduler.coefficients(i)) for i in range(self.num_steps)])           # [num_steps, 4]
            m_rows = co[:, 2, None].expand(-1, B).contiguous().to(dev)
            c_rows = co[:, 3, None].expand(-1, B).contiguous().to(dev)
            reads_noise = ((co[:, 1] * co[:, 3]) != 0).tolist()               # sigma_to c_noise = 0 (always so on the final step): the kernel gets no noise
            if step_noise is not None:
                step_noise = step_noise.to(dev, torch.float32).contiguous()
        multistep = self.sampler == 'UniPC'
        if multistep:
            # the solver's per-step weights, once (the history is empty at t_start): rows [num_steps, 10, B]
            so = self.scheduler.config.solver_order
            steps = {i: self.scheduler.coefficients(i, t_start) for i in range(t_start, self.num_steps)}
            rows = torch.tensor([steps[i].row() if i in steps else [0.0] * 10 for i in range(self.num_steps)], dtype=torch.float64)
            w_rows = rows.to(torch.float32)[:, :, None].expand(-1, -1, B).contiguous().to(dev)
        if x0 is None:
            x = noise.to(dev, torch.float32).clone().contiguous()
            xb = x.to(torch.bfloat16)
        else:
            # the source noised to the first sigma that runs (at sigma = 1: the noise itself, bit for bit) and its bf16 copy, one launch
            noise = noise.to(dev, torch.float32).contiguous()
            x0 = x0.to(dev, torch.float32).contiguous()
            mask = None if mask is None else mask.to(dev, torch.float32).contiguous()
            x, xb = ops.edit_blend(None, x0, noise, None, sig[t_start].clone())      # (a row of sig need not be 16-byte aligned)
            lands_on_zero = (sigmas[1:] == 0).tolist()                       # the step whose sigma_to is 0 reads no start noise
        T = cond['prompt_embeds'].shape[1]
        if any(active):
            T = max(T, cond['negative_prompt_embeds'].shape[1])
        eng._workspace(B, N, T)           # sized for both prompts up front: a workspace that grows mid-loop would drop the prepared steps
        chunk = min(max(8 // B, 1), self.num_steps - t_start) if self.prepare_steps else 0
        scratch: dict = {}
        g = None
        if eng.guidance_embeds and self.distilled_guidance is not None:
            g = scratch['guidance'] = torch.full((B,), float(self.distilled_guidance), dtype=torch.float32, device=dev)
        if multistep:
            last_sample = torch.empty_like(x)
            ring = [torch.empty_like(x) for _ in range(so)]                   # slot j % so receives the clean-sample prediction of the j-th step that runs
        prepared = False
        for i in range(t_start, self.num_steps):
            j = i - t_start                                                   # the steps that run are counted from the first one that does
            if chunk > 1 and j % chunk == 0:
                prepared = eng.prepare_steps(sig[i:min(i + chunk, self.num_steps)], cond.get('pooled'), g, B, N, T)
            prep = (j % chunk) if (chunk > 1 and prepared) else None
            edit = {} if mask is None else dict(x0=x0, noise0=None if lands_on_zero[i] else noise, mask=mask)
            if multistep:
                # m[-k] lives in slot (j - k) % so; only the terms the step's orders reach are handed over (the oldest may be the slot written)
                reach = max(steps[i].corrector_order, steps[i].predictor_order - 1)
                ms = dict(w=w_rows[i], last=last_sample if j > 0 else None, hist=[ring[(j - k) % so] for k in range(1, reach + 1)],
                          last_out=last_sample, hist_out=ring[j % so])
                self.step(x, xb, cond, sig[i], sig[i + 1], active[i], prep, scratch, unipc=ms)
            elif sde:
                z = step_noise[j] if step_noise is not None else self._draw(x.shape, generator)
                self.step(x, xb, cond, sig[i], sig[i + 1], active[i], prep, scratch, m_rows[i], c_rows[i], z if reads_noise[i] else None, **edit)
            else:
                self.step(x, xb, cond, sig[i], sig[i + 1], active[i], prep, scratch, **edit)
        return x

    @torch.no_grad()
    def __call__(self, cond: Dict[str, Any], noise: torch.Tensor, generator=None, step_noise: Optional[torch.Tensor] = None,
                 x0: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, strength: float = 1.0) -> torch.Tensor:
        if noise.dim() != 3:
            raise ValueError(f'noise: need packed tokens [B, N, C], got {tuple(noise.shape)}')
        if noise.shape[1] != cond['hp'] * cond['wp']:
            raise ValueError(f'noise has {noise.shape[1]} tokens but cond says {cond["hp"]} x {cond["wp"]}')
        if self.guidance_scale > 1.0 and 'negative_prompt_embeds' not in cond:
            raise ValueError('guidance_scale > 1 (true CFG) needs cond["negative_prompt_embeds"]')
        B = noise.shape[0]
        t_start = 0
        if mask is not None and self.sampler == 'UniPC':
            raise ValueError("mask: not with sampler='UniPC' -- re-imposing the kept region after each step invalidates the multistep history; "
                             "inpaint with sampler='FlowEulerODE' or 'FlowSDE'")
        if x0 is None:
            if mask is not None:
                raise ValueError('mask needs x0 (the packed latents of the image whose unmasked region is kept)')
            if float(strength) != 1.0:
                raise ValueError('strength needs x0 (without a source image the roll starts from pure noise)')
        else:
            if tuple(x0.shape) != tuple(noise.shape) or noise.shape[2] != 64:
                raise ValueError(f'x0: need packed source latents like noise, [B, N, 64]; got {tuple(x0.shape)} for noise {tuple(noise.shape)}')
            if mask is not None and tuple(mask.shape) != (B, noise.shape[1], 4):
                raise ValueError(f'mask: need [B, N, 4] = {(B, noise.shape[1], 4)} (schedule.mask_to_tokens), got {tuple(mask.shape)}')
            t_start = truncate_by_strength(self.schedule(cond['hp'], cond['wp'])[0], strength)[0]
        n_run = self.num_steps - t_start
        if self.sampler != 'FlowSDE':
            generator = step_noise = None
        elif step_noise is not None:
            if tuple(step_noise.shape) != (n_run,) + tuple(noise.shape):
                raise ValueError(f'step_noise: need [steps that run, B, N, C] = {(n_run,) + tuple(noise.shape)}, got {tuple(step_noise.shape)}')
        elif B > 4:
            # the whole batch's draws first, step by step as a single roll would make them: the result does not depend on the micro-batch split
            step_noise = torch.stack([self._draw(noise.shape, generator) for _ in range(n_run)])
        if B <= 4:
            return self._roll(cond, noise, generator, step_noise, x0, mask, t_start)
        # the engine's prepared steps hold at most 4 samples: larger batches run as micro-batches of 4 (per-sample results are the same)
        outs: List[torch.Tensor] = []
        for a in range(0, B, 4):
            mb = {k: (v[a:a + 4] if isinstance(v, torch.Tensor) and v.dim() > 0 and v.shape[0] == B else v) for k, v in cond.items()}
            outs.append(self._roll(mb, noise[a:a + 4], None, None if step_noise is None else step_noise[:, a:a + 4],
                                   None if x0 is None else x0[a:a + 4], None if mask is None else mask[a:a + 4], t_start))
        return torch.cat(outs)


_SHIFT_KEYS = ('shift', 'use_dynamic_shifting', 'base_seq_len', 'max_seq_len', 'base_logshift', 'max_logshift')
# ContinuousTimeStepSampler's own defaults (lakonlab/models/diffusions/sampler.py:11-22), for a config dict that leaves a key out
_TIMESTEP_SAMPLER_DEFAULTS = dict(shift=1.0, use_dynamic_shifting=False, base_seq_len=256, max_seq_len=4096, base_logshift=0.5, max_logshift=1.15)


_ADAPTER_BASE = 'UniPCMultistep'          # FlowAdapterScheduler's default base_scheduler, the one built here (sampler='UniPC')


def sampler_kwargs_from_test_cfg(test_cfg: Optional[Dict[str, Any]] = None, timestep_sampler: Any = None, num_timesteps: int = 1000,
                                 allow_adapter: bool = False) -> Dict[str, Any]:
    """A reference ``test_cfg`` (what ``GaussianFlow.forward_test`` reads, gaussian_flow.py:157-181) -> the keyword arguments of
    ``TeacherSampler(engine, **kwargs)``.

    ``sampler`` (default 'FlowEulerODE') picks the scheduler; ``sampler_kwargs`` go to it (FlowSDE's ``h``); the shift family
    (shift, use_dynamic_shifting, base_seq_len, max_seq_len, base_logshift, max_logshift) that ``sampler_kwargs`` leaves out is
    taken from ``test_cfg`` itself and otherwise from ``timestep_sampler`` -- the model's training timestep sampler, as an object
    with these attributes or as its config dict (a key it leaves out has ContinuousTimeStepSampler's default) -- exactly as
    gaussian_flow.py:167-171 fills them.  ``num_timesteps`` of the test_cfg is the number of sampling steps (default: the model's
    ``num_timesteps``, the argument here, which is also the scheduler's ``num_train_timesteps``).  A sampler this project does
    not have (any diffusers scheduler) raises ValueError, and so does 'FlowAdapter' unless ``allow_adapter``: then a test_cfg with
    sampler 'FlowAdapter' whose ``sampler_kwargs['base_scheduler']`` is 'UniPCMultistep' or absent (the adapter's default) maps to
    ``sampler='UniPC'`` with its solver_order, solver_type, eps and the shift family; any other base_scheduler (the DPM-Solver, DEIS, SA and
    Euler families) raises ValueError naming it."""
    cfg = dict(test_cfg or {})
    name = cfg.get('sampler', 'FlowEulerODE')
    kw = dict(cfg.get('sampler_kwargs') or {})
    if name == 'FlowAdapter' and allow_adapter:
        base = kw.pop('base_scheduler', _ADAPTER_BASE)
        if base != _ADAPTER_BASE:
            raise ValueError(f'test_cfg sampler FlowAdapter with base_scheduler {base!r}: only {_ADAPTER_BASE!r} (the default) is built here')
        name = 'UniPC'
    elif name not in SAMPLERS:
        raise ValueError(f"test_cfg sampler {name!r} is not available here: one of {sorted(SAMPLERS)}, or FlowAdapter on its "
                         f"{_ADAPTER_BASE} base scheduler with allow_adapter=True (TeacherSampler's sampler='UniPC'); the other diffusers schedulers are not built")
    unknown = set(kw) - set(SAMPLERS[name]._DEFAULTS)
    if unknown:
        raise TypeError(f'{name}Scheduler takes no {sorted(unknown)}')
    for key in _SHIFT_KEYS:
        if key in kw:
            continue
        if key in cfg:
            kw[key] = cfg[key]
        elif isinstance(timestep_sampler, dict):
            kw[key] = timestep_sampler.get(key, _TIMESTEP_SAMPLER_DEFAULTS[key])
        elif timestep_sampler is not None:
            kw[key] = getattr(timestep_sampler, key)
        else:
            kw[key] = _TIMESTEP_SAMPLER_DEFAULTS[key]
    kw.update(sampler=name, num_steps=int(cfg.get('num_timesteps', num_timesteps)), num_train_timesteps=int(num_timesteps),
              orthogonal_guidance=bool(cfg.get('orthogonal_guidance', False)))
    if cfg.get('guidance_interval') is not None:
        kw['guidance_interval'] = [float(v) for v in cfg['guidance_interval']]
    return kw
