#!/usr/bin/env python3
"""Generate the golden vectors of STOCHASTIC teacher sampling by EXECUTING the reference's own functions.

Companion of make_golden_teacher_sampler.py (same rules: build container only, the reference is parsed in place, nothing of it is
copied, only inputs + outputs are written; its ``register_to_config`` / mixin stubs, its stub denoiser and its ``build_flow`` are
reused).  Executed (paths under /root/reference/lakonlab):
  models/diffusions/schedulers/flow_sde.py : FlowSDEScheduler (whole class).  ``randn_tensor`` (diffusers is absent) is a stub that
                                             draws with ``torch.randn`` from a seeded CPU generator and RECORDS every draw, so the
                                             fixture holds the noise the reference used
  models/diffusions/gaussian_flow.py       : GaussianFlow.forward_test, guidance_jit (decorator stripped)

Fixture g13_sde_sampler.npz:
  tab_sigmas / tab_timesteps       : the scheduler's tables for 7 steps at shift 3.2 (the ODE scheduler's, G12 tab1)
  step_sample / step_model_output  : the inputs of the step() runs, latent [2, 16, 4, 4] (drawn as G12's)
  step_noise                       : the 7 recorded draws (the recording generator is reseeded per h: every h sees the same noise)
  step_{tag}_prev_sample           : FlowSDEScheduler.step over the 7-step table, tag in h0, h0p5, h1, h2, hinf  (h = 0.0, 0.5, 1.0, 2.0, 'inf')
  step_{tag}_m / step_{tag}_c      : the ``m`` the reference's step() held when it returned (read from its frame) and
                                     sqrt(clamp(1 - m^2, 0)) evaluated from that tensor with the reference's expression -- every step,
                                     the first (sigma = 1: m = 0) and the last (sigma_to = 0: m = 0) included
  roll_noise / roll_draws          : start noise (seed 1208, G12's) and the 5 recorded per-step draws (the same for every roll)
  roll_{h1_plain,h1_ortho,h0}_x_t  : every intermediate x_t of a 5-step forward_test with sampler 'FlowSDE' at guidance 4.0, shift 3.2,
                                     stub denoiser of fixture G12: h = 1.0 orthogonal off / on, and h = 0.0

Usage:  python tests/golden/make_golden_sde_sampler.py
"""
import os
import sys
from typing import Optional, Tuple, Union

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402
import make_golden_teacher_sampler as TG  # noqa: E402

REF = MG.REF
HS = [('h0', 0.0), ('h0p5', 0.5), ('h1', 1.0), ('h2', 2.0), ('hinf', 'inf')]
STEP_TABLE = dict(num_steps=7, shift=3.2)
ROLLS = [('h1_plain', 1.0, False), ('h1_ortho', 1.0, True), ('h0', 0.0, False)]


class Recorder:
    """The stand-in for diffusers' ``randn_tensor``: seeded CPU draws, every one kept."""

    def __init__(self):
        self.gen = torch.Generator()
        self.draws = []

    def reseed(self, seed):
        self.gen.manual_seed(seed)
        self.draws = []

    def __call__(self, shape, generator=None, device=None, dtype=None, layout=None):
        z = torch.randn(tuple(shape), generator=self.gen, dtype=dtype or torch.float32)
        self.draws.append(z.clone())
        return z


def load_scheduler(recorder):
    ns = dict(torch=torch, np=np, Optional=Optional, Tuple=Tuple, Union=Union, register_to_config=TG.register_to_config,
              ConfigMixin=type('ConfigMixin', (), {}), SchedulerMixin=type('SchedulerMixin', (), {}),
              FlowSDESchedulerOutput=dict, randn_tensor=recorder)
    return MG.grab_class(REF + '/models/diffusions/schedulers/flow_sde.py', 'FlowSDEScheduler', ns)


def step_recording_m(sch, u, t, x):
    """sch.step(...) -> (prev_sample, the ``m`` in the frame of the reference's step() when it returned)."""
    seen = {}

    def prof(frame, event, arg):
        if event == 'return' and frame.f_code.co_name == 'step' and 'm' in frame.f_locals:
            seen['m'] = frame.f_locals['m'].clone()
    sys.setprofile(prof)
    try:
        prev = sch.step(u, t, x, return_dict=False)[0]
    finally:
        sys.setprofile(None)
    return prev, seen['m']


def golden_steps(Scheduler, rec, out):
    gen = torch.Generator().manual_seed(1207)           # G12's step inputs
    x0 = torch.randn(2, 16, 4, 4, generator=gen)
    us = torch.randn(STEP_TABLE['num_steps'], 2, 16, 4, 4, generator=gen)
    out['step_sample'], out['step_model_output'] = x0.clone(), us
    for tag, h in HS:
        sch = Scheduler(1000, h=h, shift=STEP_TABLE['shift'])
        sch.set_timesteps(STEP_TABLE['num_steps'])
        assert sch.sigmas.numel() == STEP_TABLE['num_steps'] + 1 and float(sch.sigmas[-1]) == 0.0
        out['tab_sigmas'], out['tab_timesteps'] = sch.sigmas.clone(), sch.timesteps.clone()
        rec.reseed(1307)
        x, prev, ms = x0.clone(), [], []
        for t, u in zip(sch.timesteps, us):
            x, m = step_recording_m(sch, u, t, x)
            prev.append(x.clone())
            ms.append(m)
        m = torch.stack(ms)
        out[f'step_{tag}_prev_sample'] = torch.stack(prev)
        out[f'step_{tag}_m'], out[f'step_{tag}_c'] = m, (1 - m.square()).clamp(min=0).sqrt()
        noise = torch.stack(rec.draws)
        assert noise.shape == us.shape
        if 'step_noise' in out:
            assert torch.equal(out['step_noise'], noise)
        out['step_noise'] = noise
        assert float(m[0]) == 0.0 or h == 0.0            # sigma = 1: alpha = 0
        assert float(m[-1]) == 0.0 or h == 0.0           # sigma_to = 0
    assert (out['step_h0_m'] == 1).all() and (out['step_hinf_m'] == 0).all()


def golden_rolls(Scheduler, rec, out):
    flow = TG.build_flow(TG.load_scheduler())
    flow.forward_test.__func__.__globals__['schedulers'].FlowSDEScheduler = Scheduler
    gen = torch.Generator().manual_seed(1208)            # G12's start noise
    noise = torch.randn(2, 16, 4, 4, generator=gen)
    out['roll_noise'] = noise
    out['roll_scale'], out['roll_shift'] = np.float32(TG.ROLL_SCALE), np.float32(TG.ROLL_SHIFT)
    B = noise.size(0)
    for tag, h, orthogonal in ROLLS:
        seen = []

        def pred(x_t, t, **kw):
            assert x_t.size(0) == 2 * B                  # guidance is active on every step
            seen.append(x_t[-B:].clone())
            return torch.cat([TG.stub_velocity(x_t[:B], t, True), TG.stub_velocity(x_t[-B:], t, False)])
        flow.pred = pred
        flow.test_cfg = dict(sampler='FlowSDE', sampler_kwargs=dict(h=h), num_timesteps=TG.ROLL_STEPS, orthogonal_guidance=orthogonal)
        rec.reseed(1308)
        x_end = flow.forward_test(noise=noise, guidance_scale=TG.ROLL_SCALE)
        assert len(seen) == TG.ROLL_STEPS and torch.equal(seen[0], noise) and len(rec.draws) == TG.ROLL_STEPS
        out[f'roll_{tag}_x_t'] = torch.stack(seen[1:] + [x_end])
        draws = torch.stack(rec.draws)
        if 'roll_draws' in out:
            assert torch.equal(out['roll_draws'], draws)
        out['roll_draws'] = draws
    assert not torch.equal(out['roll_h1_plain_x_t'], out['roll_h0_x_t'])


def main():
    torch.set_num_threads(4)
    rec = Recorder()
    Scheduler = load_scheduler(rec)
    out = {}
    golden_steps(Scheduler, rec, out)
    golden_rolls(Scheduler, rec, out)
    MG.save('g13_sde_sampler', **out)


if __name__ == '__main__':
    main()
