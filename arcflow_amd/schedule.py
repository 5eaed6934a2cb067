"""Time grid of the ArcFlow sampler and the flow-matching scheduler object the reference's entry
scripts configure (inference_flux.py:14-15: ``FlowMatchEulerDiscreteScheduler.from_config(
pipe.scheduler.config, shift=3.2, shift_terminal=None, use_dynamic_shifting=False)``), and the
``FlowEulerODEScheduler`` of the reference's own teacher sampling (GaussianFlow.forward_test).

Host-side float arithmetic only (128 numbers per image) -- nothing here runs on the GPU.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch


def retrieve_raw_timesteps(num_inference_steps: int, total_substeps: int, timestep_ratio: float
                           ) -> Tuple[List[float], List[int], int]:
    """Raw sub-step times, sub-steps per inference step and their total
    (same contract as lakonlab/pipelines/arcflux_pipeline.py:34-70)."""
    if num_inference_steps < 1:
        raise ValueError('num_inference_steps must be >= 1')
    seg = 1.0 / (num_inference_steps - 1 + timestep_ratio)
    times: List[float] = []
    per_step: List[int] = []
    upper = 1.0
    for i in range(num_inference_steps):
        size = seg * timestep_ratio if i == num_inference_steps - 1 else seg
        n = max(round(size * total_substeps), 1)
        per_step.append(n)
        times += np.linspace(upper, upper - size, n, endpoint=False).clip(min=0.0).tolist()
        upper -= size
    return times, per_step, sum(per_step)


def edit_raw_timesteps(num_inference_steps: int, total_substeps: int, timestep_ratio: float, strength: float
                       ) -> Tuple[List[float], List[int], int]:
    """The raw grid of an edit (``image=`` / ``strength=`` on the pipelines): ``retrieve_raw_timesteps`` with every time multiplied by
    ``strength`` in (0, 1].  The edit takes ``num_inference_steps`` full student steps over the raw time [strength, 0]; it does not walk a
    truncated prefix of the text-to-image grid, which at 2 NFE could only express strength 0.5 or 1.  strength == 1.0 returns the lists of
    ``retrieve_raw_timesteps`` themselves."""
    strength = float(strength)
    if not 0.0 < strength <= 1.0:
        raise ValueError(f'strength must be in (0, 1], got {strength}')
    times, per_step, total = retrieve_raw_timesteps(num_inference_steps, total_substeps, timestep_ratio)
    if strength != 1.0:
        times = [strength * t for t in times]
    return times, per_step, total


def truncate_by_strength(sigmas: torch.Tensor, strength: float) -> Tuple[int, torch.Tensor]:
    """The schedule of a many-step edit (``sample_teacher(image=..., strength=...)``, TeacherSampler with ``x0``): a suffix of the
    sampler's FULL schedule ``sigmas`` [n + 1] (trailing 0; shift / dynamic shifting already applied for all n steps), as the
    image-to-image pipelines of diffusers truncate theirs (as recalled; unpinned):

        init = min(n * strength, n),   t_start = int(max(n - init, 0)),   steps t_start .. n - 1 run

    -> (t_start, sigmas[t_start:]): the edit starts from the source noised to ``sigmas[t_start]``.  ``strength`` must lie in (0, 1];
    1.0 keeps all n steps, and a strength so small that no step is left raises like one outside the interval."""
    strength = float(strength)
    if not 0.0 < strength <= 1.0:
        raise ValueError(f'strength must be in (0, 1], got {strength}')
    n = int(sigmas.numel()) - 1
    if n < 1:
        raise ValueError('sigmas: need at least one step (two entries)')
    t_start = int(max(n - min(n * strength, n), 0))
    if t_start >= n:
        raise ValueError(f'strength {strength} leaves none of the {n} steps to run')
    return t_start, sigmas[t_start:]


def mask_to_tokens(mask: torch.Tensor, hp: int, wp: int, reduce: str = 'max') -> torch.Tensor:
    """An image-resolution mask [B, 1, H, W] or [B, H, W] with H = 16 hp, W = 16 wp -> [B, hp*wp, 4] fp32, the operand of
    ``ops.edit_blend``: latent pixel (2r + ph, 2c + pw) of token r*wp + c, at index ph*2 + pw, takes the max (``reduce='max'``: any
    repainted pixel repaints its latent pixel, a binary mask stays binary) or the mean (``'mean'``) of its 8 x 8 pixel block.  Once per
    call, on whatever device the mask lives: plain torch."""
    if reduce not in ('max', 'mean'):
        raise ValueError(f"reduce: 'max' or 'mean', got {reduce!r}")
    if mask.dim() == 4 and mask.shape[1] == 1:
        mask = mask[:, 0]
    if mask.dim() != 3 or tuple(mask.shape[1:]) != (16 * hp, 16 * wp):
        raise ValueError(f'mask: need [B, 1, {16 * hp}, {16 * wp}] or [B, {16 * hp}, {16 * wp}], got {tuple(mask.shape)}')
    blocks = mask.to(torch.float32).reshape(mask.shape[0], hp, 2, 8, wp, 2, 8)          # [B, r, ph, i, c, pw, j]
    red = blocks.amax(dim=(3, 6)) if reduce == 'max' else blocks.mean(dim=(3, 6))      # [B, r, ph, c, pw]
    return red.permute(0, 1, 3, 2, 4).reshape(mask.shape[0], hp * wp, 4).contiguous()


def student_sigmas(num_inference_steps: int, total_substeps: int = 128, timestep_ratio: float = 1.0, shift: float = 3.2,
                   num_train_timesteps: int = 1000) -> List[float]:
    """sigma at the start of every student step plus the terminal 0, as the pipelines' ``__call__`` walks them: the raw sub-step grid
    (retrieve_raw_timesteps) through the static shift of FlowMatchEulerDiscreteScheduler in fp32, every step reading the first
    sub-step of its segment as ``timestep / num_train_timesteps``.  For samplers outside the pipelines (ArcFlowDistiller.sample_student)."""
    raw, per_step, total = retrieve_raw_timesteps(num_inference_steps, total_substeps, timestep_ratio)
    sch = FlowMatchEulerDiscreteScheduler(num_train_timesteps=num_train_timesteps, shift=shift, use_dynamic_shifting=False)
    ts = sch.set_timesteps(sigmas=raw).float().tolist()
    out, tid = [], 0
    for n in per_step:
        out.append(ts[tid] / num_train_timesteps)
        tid += n
    assert tid == total == len(ts)
    return out + [0.0]


class _Config(dict):
    """dict with attribute access, like diffusers' FrozenDict configs."""
    __getattr__ = dict.get

    def get(self, k, default=None):          # noqa: D401 - keep dict.get semantics
        return super().get(k, default)


class FlowMatchEulerDiscreteScheduler:
    """The subset of diffusers' scheduler the ArcFlow pipelines touch: config, from_config(),
    set_begin_index(), set_timesteps(sigmas=..., mu=...), .timesteps / .sigmas.

    sigma' = shift * s / (1 + (shift-1) s) for the static shift; with use_dynamic_shifting the
    exponential time shift exp(mu) / (exp(mu) + (1/s - 1)) of the stock FLUX pipeline.
    """
    _DEFAULTS = dict(num_train_timesteps=1000, shift=1.0, use_dynamic_shifting=False, base_shift=0.5,
                     max_shift=1.15, base_image_seq_len=256, max_image_seq_len=4096, shift_terminal=None)

    def __init__(self, **kwargs: Any):
        cfg = dict(self._DEFAULTS)
        cfg.update(kwargs)
        self.config = _Config(cfg)
        self.timesteps: Optional[torch.Tensor] = None
        self.sigmas: Optional[torch.Tensor] = None
        self._begin_index = None

    @classmethod
    def from_config(cls, config: Optional[Dict[str, Any]] = None, **overrides: Any):
        cfg = dict(config or {})
        cfg.update(overrides)
        cfg = {k: v for k, v in cfg.items() if not k.startswith('_')}
        return cls(**cfg)

    def set_begin_index(self, begin_index: int = 0):
        self._begin_index = begin_index

    def set_timesteps(self, num_inference_steps: Optional[int] = None, device=None,
                      sigmas: Optional[List[float]] = None, mu: Optional[float] = None):
        if sigmas is None:
            n = num_inference_steps
            sigmas = np.linspace(1.0, 1.0 / self.config.num_train_timesteps, n)
        s = np.asarray(sigmas, dtype=np.float32)
        if self.config.use_dynamic_shifting:
            if mu is None:
                raise ValueError('mu is required with use_dynamic_shifting')
            s = (math.exp(mu) / (math.exp(mu) + (1.0 / s - 1.0))).astype(np.float32)
        else:
            sh = np.float32(self.config.shift)
            s = (sh * s / (np.float32(1) + (sh - np.float32(1)) * s)).astype(np.float32)
        if self.config.shift_terminal:
            one_minus = 1 - s
            s = (1 - one_minus / (one_minus[-1] / (1 - self.config.shift_terminal))).astype(np.float32)
        sig = torch.from_numpy(s)
        self.timesteps = (sig * self.config.num_train_timesteps).to(device)
        self.sigmas = torch.cat([sig, torch.zeros(1)]).to(device)
        return self.timesteps


def calculate_shift(image_seq_len, base_seq_len=256, max_seq_len=4096, base_shift=0.5, max_shift=1.15):
    m = (max_shift - base_shift) / (max_seq_len - base_seq_len)
    return image_seq_len * m + (base_shift - m * base_seq_len)


class _FlowSchedulerTables:
    """What the reference's own flow schedulers share (schedulers/flow_euler_ode.py:20-118 and schedulers/flow_sde.py:21-111 are the
    same text up to ``step()``): ``config``, ``from_config()``, ``get_shift()``, ``stretch_to_terminal()``, ``set_timesteps(n, seq_len=...)``
    and the step index.  A subclass sets ``_DEFAULTS`` and adds ``step()``.

    Grid: n points of linspace(1, 0, endpoint=False), warped by sigma' = s sigma / (1 + (s - 1) sigma) with the static ``shift`` or,
    with ``use_dynamic_shifting``, s = exp(logshift) interpolated linearly in ``seq_len`` between (base_seq_len, base_logshift)
    and (max_seq_len, max_logshift); optionally stretched so that the last sigma is ``terminal_sigma``; a trailing 0 is appended to
    ``sigmas`` (the last step lands on the clean sample)."""
    order = 1
    _DEFAULTS: Dict[str, Any] = {}

    def __init__(self, num_train_timesteps: int = 1000, **kwargs: Any):
        cfg = dict(self._DEFAULTS)
        cfg['num_train_timesteps'] = num_train_timesteps
        unknown = set(kwargs) - set(cfg)
        if unknown:
            raise TypeError(f'{type(self).__name__} got unexpected arguments {sorted(unknown)}')
        cfg.update(kwargs)
        self.config = _Config(cfg)
        shift = self.config.shift
        sigmas = torch.from_numpy(1 - np.linspace(0, 1, num_train_timesteps, dtype=np.float32, endpoint=False))
        self.sigmas = shift * sigmas / (1 + (shift - 1) * sigmas)
        self.timesteps = self.sigmas * num_train_timesteps
        self._step_index = None
        self._begin_index = None
        self.sigma_min = self.sigmas[-1].item()
        self.sigma_max = self.sigmas[0].item()

    @classmethod
    def from_config(cls, config: Optional[Dict[str, Any]] = None, **overrides: Any):
        cfg = dict(config or {})
        cfg.update(overrides)
        cfg = {k: v for k, v in cfg.items() if k in cls._DEFAULTS}       # a foreign scheduler's config: only the shared keys apply
        return cls(**cfg)

    @property
    def step_index(self):
        return self._step_index

    @property
    def begin_index(self):
        return self._begin_index

    def set_begin_index(self, begin_index: int = 0):
        self._begin_index = begin_index

    def get_shift(self, seq_len=None):
        c = self.config
        if c.use_dynamic_shifting and seq_len is not None:
            m = (c.max_logshift - c.base_logshift) / (c.max_seq_len - c.base_seq_len)
            logshift = (seq_len - c.base_seq_len) * m + c.base_logshift
            return torch.exp(logshift) if isinstance(logshift, torch.Tensor) else np.exp(logshift)
        return c.shift

    def stretch_to_terminal(self, sigma: torch.Tensor) -> torch.Tensor:
        one_minus_sigma = 1 - sigma
        return 1 - (one_minus_sigma * (1 - self.config.terminal_sigma) / one_minus_sigma[-1])

    def set_timesteps(self, num_inference_steps: int, seq_len=None, device=None):
        self.num_inference_steps = num_inference_steps
        sigmas = torch.from_numpy(np.linspace(1, 0, num_inference_steps, dtype=np.float32, endpoint=False))
        shift = self.get_shift(seq_len=seq_len)
        sigmas = shift * sigmas / (1 + (shift - 1) * sigmas)
        if self.config.terminal_sigma is not None:
            sigmas = self.stretch_to_terminal(sigmas)
        self.timesteps = (sigmas * self.config.num_train_timesteps).to(device)
        self.sigmas = torch.cat([sigmas, torch.zeros(1)])
        self._step_index = None
        self._begin_index = None
        return self.timesteps

    def index_for_timestep(self, timestep, schedule_timesteps=None):
        ts = self.timesteps if schedule_timesteps is None else schedule_timesteps
        indices = (ts == timestep).nonzero()
        return indices[1 if len(indices) > 1 else 0].item()

    def _begin_step(self, timestep, prediction_type: str) -> int:
        """The checks both ``step()``s open with; -> the index of the step about to be taken."""
        if prediction_type != 'u':
            raise NotImplementedError(f"{type(self).__name__}.step: only prediction_type='u' (the teacher predicts a velocity)")
        if isinstance(timestep, int) or (isinstance(timestep, torch.Tensor) and not timestep.is_floating_point()):
            raise ValueError('pass one of scheduler.timesteps as the timestep, not an integer index')
        if self._step_index is None:
            if self._begin_index is None:
                t = timestep.to(self.timesteps.device) if isinstance(timestep, torch.Tensor) else timestep
                self._step_index = self.index_for_timestep(t)
            else:
                self._step_index = self._begin_index
        return self._step_index

    def __len__(self):
        return self.config.num_train_timesteps


class FlowEulerODEScheduler(_FlowSchedulerTables):
    """The reference's own Euler ODE scheduler (lakonlab/models/diffusions/schedulers/flow_euler_ode.py:20-164), the default
    ``sampler`` of ``GaussianFlow.forward_test``, without diffusers: ``config``, ``from_config()``, ``get_shift()``,
    ``stretch_to_terminal()``, ``set_timesteps(n, seq_len=...)`` and ``step()`` for ``prediction_type='u'``.  Same fp32 operations in the
    same order as the reference (tests/golden/g12_teacher_sampler.npz)."""
    _DEFAULTS = dict(num_train_timesteps=1000, shift=1.0, use_dynamic_shifting=False, base_seq_len=256, max_seq_len=4096,
                     base_logshift=0.5, max_logshift=1.15, terminal_sigma=None)

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator=None, return_dict: bool = True,
             prediction_type: str = 'u'):
        """prev_sample = sample + model_output (sigma_next - sigma) in fp32, cast back to model_output's dtype."""
        i = self._begin_step(timestep, prediction_type)
        ori_dtype = model_output.dtype
        sigma = self.sigmas[i]
        sigma_to = self.sigmas[i + 1]
        dt = (sigma_to - sigma).to(sample.device)
        prev_sample = (sample.to(torch.float32) + model_output.to(torch.float32) * dt).to(ori_dtype)
        self._step_index += 1
        if not return_dict:
            return (prev_sample,)
        return _Config(prev_sample=prev_sample)


class FlowSDEScheduler(_FlowSchedulerTables):
    """The reference's stochastic scheduler (lakonlab/models/diffusions/schedulers/flow_sde.py:21-180; ``sampler='FlowSDE'`` in a
    ``test_cfg``) without diffusers: the tables of FlowEulerODEScheduler, and a ``step()`` that re-injects fresh noise with a strength
    set by ``h`` -- a float, or the string ``'inf'``.  With x0 = x - sigma u and eps = x + (1 - sigma) u the predictions of the clean
    sample and of the noise,

        prev = (1 - sigma_to) x0 + sigma_to (m eps + sqrt(max(1 - m^2, 0)) z),      z ~ N(0, 1) fresh per step,
        m = (sigma_to (1 - sigma) / max(sigma (1 - sigma_to), 1e-6)) ^ (h^2)

    h = 0 gives m = 1: the ODE step (algebraically x + u (sigma_to - sigma)); h = 'inf' gives m = 0: the predicted clean sample is
    re-noised completely.  Same fp32 operations in the same order as the reference (tests/golden/g13_sde_sampler.npz)."""
    _DEFAULTS = dict(FlowEulerODEScheduler._DEFAULTS, h=1.0)

    def __init__(self, num_train_timesteps: int = 1000, **kwargs: Any):
        super().__init__(num_train_timesteps, **kwargs)
        h = self.config.h
        if isinstance(h, str) and h != 'inf':
            raise ValueError(f"h: a float or the string 'inf', got {h!r}")

    def coefficients(self, i: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """-> (sigma, sigma_to, m, c_noise) of step i as fp32 scalars, c_noise = sqrt(max(1 - m^2, 0)): what ``step()`` mixes with,
        and what the fused step kernel (afx_teacher_sde_step) is handed.  Needs ``set_timesteps()``."""
        sigma, sigma_to = self.sigmas[i], self.sigmas[i + 1]
        alpha, alpha_to = 1 - sigma, 1 - sigma_to
        h = self.config.h
        if h == 'inf':
            m = torch.zeros_like(sigma)
        elif h == 0.0:
            m = torch.ones_like(sigma)
        else:
            if not h > 0.0:
                raise ValueError(f'h must be >= 0 (or the string \'inf\'), got {h!r}')
            m = (sigma_to * alpha / (sigma * alpha_to).clamp(min=1e-6)) ** (h * h)
        return sigma, sigma_to, m, (1 - m.square()).clamp(min=0).sqrt()

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator=None, return_dict: bool = True,
             prediction_type: str = 'u', noise: Optional[torch.Tensor] = None):
        """One stochastic step in fp32, cast back to model_output's dtype.  noise: the step's N(0, 1) draw (default: torch.randn of
        model_output's shape on its device from ``generator``)."""
        i = self._begin_step(timestep, prediction_type)
        ori_dtype = model_output.dtype
        sample = sample.to(torch.float32)
        model_output = model_output.to(torch.float32)
        sigma, sigma_to, m, c_noise = self.coefficients(i)
        alpha, alpha_to = 1 - sigma, 1 - sigma_to
        x0 = sample - sigma * model_output
        epsilon = sample + alpha * model_output
        if noise is None:
            noise = torch.randn(model_output.shape, generator=generator, device=model_output.device, dtype=torch.float32)
        prev_sample = (alpha_to * x0 + sigma_to * (m * epsilon + c_noise * noise)).to(ori_dtype)
        self._step_index += 1
        if not return_dict:
            return (prev_sample,)
        return _Config(prev_sample=prev_sample)
