#!/usr/bin/env python3
"""Generate the golden vectors of teacher sampling by EXECUTING the reference's own functions.

Companion of make_golden.py / make_golden_imitation.py (same rules: build container only, the reference is parsed in place,
nothing of it is copied, only inputs + outputs are written).  Executed (paths under /root/reference/lakonlab):
  models/diffusions/schedulers/flow_euler_ode.py : FlowEulerODEScheduler (whole class; diffusers is absent, so ``ConfigMixin``,
                                                   ``SchedulerMixin`` and ``register_to_config`` are stubs that keep the
                                                   constructor arguments as ``self.config``)
  models/diffusions/gaussian_flow.py             : GaussianFlow.forward_test, guidance_jit (decorator stripped)

Fixture g12_teacher_sampler.npz:
  tab{i}_sigmas / tab{i}_timesteps : the scheduler's tables for (num_steps, shift, use_dynamic_shifting + seq_len, terminal_sigma) in
                                     {(4, 1.0, off, None), (7, 3.2, off, None), (5, -, on with seq_len 1024, None), (6, 3.2, off, 0.02)}
  step_*                           : FlowEulerODEScheduler.step over the 7-step table (sample, model outputs, every prev_sample)
  roll_{plain,ortho,interval}_x_t  : every intermediate x_t of a 5-step forward_test at latent [2, 16, 4, 4], guidance 4.0, shift 3.2,
                                     closed-form stub denoiser (below): orthogonal off / on, and orthogonal off with
                                     guidance_interval [700, 1000] (guidance off on the last two steps); *_active: the steps on
                                     which the reference ran the stacked [negative; positive] forward

Usage:  python tests/golden/make_golden_teacher_sampler.py
"""
import functools
import inspect
import os
import sys
import types
from copy import deepcopy
from typing import Optional, Tuple, Union

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

REF = MG.REF
TABLES = [dict(num_steps=4, shift=1.0), dict(num_steps=7, shift=3.2), dict(num_steps=5, use_dynamic_shifting=True, seq_len=1024),
          dict(num_steps=6, shift=3.2, terminal_sigma=0.02)]
ROLL_STEPS, ROLL_SHIFT, ROLL_SCALE, ROLL_INTERVAL = 5, 3.2, 4.0, [700, 1000]


def register_to_config(init):
    """diffusers' decorator, reduced to what the scheduler reads back: the constructor arguments as ``self.config.<name>``."""
    @functools.wraps(init)
    def wrapper(self, *a, **kw):
        bound = inspect.signature(init).bind(self, *a, **kw)
        bound.apply_defaults()
        self.config = types.SimpleNamespace(**{k: v for k, v in bound.arguments.items() if k != 'self'})
        init(self, *a, **kw)
    return wrapper


def load_scheduler():
    ns = dict(torch=torch, np=np, Optional=Optional, Tuple=Tuple, Union=Union, register_to_config=register_to_config,
              ConfigMixin=type('ConfigMixin', (), {}), SchedulerMixin=type('SchedulerMixin', (), {}),
              FlowEulerODESchedulerOutput=dict)
    return MG.grab_class(REF + '/models/diffusions/schedulers/flow_euler_ode.py', 'FlowEulerODEScheduler', ns)


def stub_velocity(x, t, negative):
    """Closed-form stand-in for the denoiser (t in [0, 1000]); the two conditionings differ in every term."""
    s = t / 1000.0
    if negative:
        return 0.25 * x - 0.5 * s + 0.04 * torch.roll(x, 1, dims=-2) + 0.1
    return 0.3 * x - 0.7 * s + 0.05 * torch.roll(x, 1, dims=-1)


def build_flow(Scheduler):
    ns = dict(torch=torch, deepcopy=deepcopy, inspect=inspect, sys=sys, mmcv=None,
              diffusers=types.SimpleNamespace(schedulers=types.SimpleNamespace()),
              schedulers=types.SimpleNamespace(FlowEulerODEScheduler=Scheduler))
    MG.grab(REF + '/models/diffusions/gaussian_flow.py', ['guidance_jit'], ns=ns)
    MG.grab(REF + '/models/diffusions/gaussian_flow.py', ['forward_test'], cls='GaussianFlow', ns=ns)
    flow = MG.Obj()
    flow.num_timesteps = 1000
    flow.timestep_sampler = types.SimpleNamespace(shift=ROLL_SHIFT, use_dynamic_shifting=False, base_seq_len=256, max_seq_len=4096,
                                                  base_logshift=0.5, max_logshift=1.15)
    flow.forward_test = types.MethodType(ns['forward_test'], flow)
    return flow


def golden_tables(Scheduler, out):
    for i, c in enumerate(TABLES):
        kw = {k: v for k, v in c.items() if k not in ('num_steps', 'seq_len')}
        sch = Scheduler(1000, **kw)
        sch.set_timesteps(c['num_steps'], seq_len=c.get('seq_len'))
        assert sch.sigmas.numel() == c['num_steps'] + 1 and float(sch.sigmas[-1]) == 0.0
        out[f'tab{i}_sigmas'], out[f'tab{i}_timesteps'] = sch.sigmas.clone(), sch.timesteps.clone()
        if i == 1:
            gen = torch.Generator().manual_seed(1207)
            x = torch.randn(2, 16, 4, 4, generator=gen)
            us = torch.randn(c['num_steps'], 2, 16, 4, 4, generator=gen)
            prev = []
            out['step_sample'], out['step_model_output'] = x.clone(), us
            for t, u in zip(sch.timesteps, us):
                x = sch.step(u, t, x, return_dict=False)[0]
                prev.append(x.clone())
            out['step_prev_sample'] = torch.stack(prev)


def golden_rolls(flow, out):
    gen = torch.Generator().manual_seed(1208)
    noise = torch.randn(2, 16, 4, 4, generator=gen)
    out['roll_noise'] = noise
    out['roll_scale'], out['roll_shift'], out['roll_interval'] = np.float32(ROLL_SCALE), np.float32(ROLL_SHIFT), np.float32(ROLL_INTERVAL)
    B = noise.size(0)
    for tag, cfg in (('plain', dict(orthogonal_guidance=False)), ('ortho', dict(orthogonal_guidance=True)),
                     ('interval', dict(orthogonal_guidance=False, guidance_interval=ROLL_INTERVAL))):
        seen, active = [], []

        def pred(x_t, t, **kw):
            stacked = x_t.size(0) == 2 * B
            active.append(stacked)
            seen.append(x_t[-B:].clone())
            pos = stub_velocity(x_t[-B:], t, False)
            return torch.cat([stub_velocity(x_t[:B], t, True), pos]) if stacked else pos
        flow.pred = pred
        flow.test_cfg = dict(sampler='FlowEulerODE', num_timesteps=ROLL_STEPS, **cfg)
        x_end = flow.forward_test(noise=noise, guidance_scale=ROLL_SCALE)
        assert len(seen) == ROLL_STEPS and torch.equal(seen[0], noise)
        out[f'roll_{tag}_x_t'] = torch.stack(seen[1:] + [x_end])
        out[f'roll_{tag}_active'] = np.asarray(active)
    assert out['roll_plain_active'].all() and out['roll_ortho_active'].all()
    assert out['roll_interval_active'].tolist() == [True, True, True, False, False]


def main():
    torch.set_num_threads(4)
    Scheduler = load_scheduler()
    out = {}
    golden_tables(Scheduler, out)
    golden_rolls(build_flow(Scheduler), out)
    MG.save('g12_teacher_sampler', **out)


if __name__ == '__main__':
    main()
