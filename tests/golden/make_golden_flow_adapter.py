#!/usr/bin/env python3
"""Generate the golden sigma tables of the adapter scheduler by EXECUTING the reference's own class.

Companion of make_golden_teacher_sampler.py (same rules: build container only, the reference is parsed in place, nothing of it is
copied, only inputs + outputs are written; its ``register_to_config`` / mixin stubs are reused).  Executed (path under
/root/reference/lakonlab):
  models/diffusions/schedulers/flow_adapter.py : FlowAdapterScheduler.__init__ / get_shift / stretch_to_terminal / set_timesteps with the
                                                 default base_scheduler 'UniPCMultistep'

diffusers is absent, so ``diffusers.schedulers.UniPCMultistepScheduler`` is a stub that records its constructor keywords and whose
``set_timesteps`` does nothing: the adapter overwrites the base scheduler's ``timesteps`` and ``sigmas`` right after calling it
(flow_adapter.py:136-149), and those two tables are all this fixture pins.  The multistep arithmetic itself is diffusers' and is NOT
executed here: nothing pins it (DESIGN.md 6.1 "Multistep sampling").

Fixture g14_flow_adapter_tables.npz, for each table k of TABLES (static shift 1.0 and 3.2, dynamic shift at seq_len 1024, shift 3.2 with
terminal_sigma 0.02, and 40 steps at shift 12 with eps 5e-3, where three sigmas exceed 1 - eps):
  tab{k}_timesteps / tab{k}_sigmas : the adapter's own tables (sigmas with the trailing 0)
  tab{k}_base_sigmas               : what the base scheduler is handed, sigmas.clamp(max=1 - eps)
  tab{k}_eps                       : the eps of the clamp
  base_kwargs                      : the keywords the adapter built the base scheduler with (names = values as text)

Usage:  python tests/golden/make_golden_flow_adapter.py
"""
import inspect
import os
import sys
import types
from dataclasses import dataclass
from typing import Optional, Tuple, Union

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402
import make_golden_teacher_sampler as TG  # noqa: E402

REF = MG.REF
TABLES = TG.TABLES + [dict(num_steps=40, shift=12.0, eps=5e-3)]


class UniPCMultistepScheduler:
    """The stand-in for diffusers' class: the keywords the adapter reads from its signature, nothing computed."""
    seen = None

    def __init__(self, num_train_timesteps=1000, prediction_type='epsilon', use_flow_sigmas=False, final_sigmas_type='zero',
                 lower_order_final=True, **kwargs):
        type(self).seen = dict(num_train_timesteps=num_train_timesteps, prediction_type=prediction_type, use_flow_sigmas=use_flow_sigmas,
                               final_sigmas_type=final_sigmas_type, lower_order_final=lower_order_final, **kwargs)

    def set_timesteps(self, num_inference_steps, device=None):
        self.num_inference_steps = num_inference_steps


def load_scheduler():
    diffusers = types.SimpleNamespace(schedulers=types.SimpleNamespace(UniPCMultistepScheduler=UniPCMultistepScheduler))
    ns = dict(torch=torch, np=np, inspect=inspect, diffusers=diffusers, dataclass=dataclass, Optional=Optional, Tuple=Tuple, Union=Union,
              register_to_config=TG.register_to_config, ConfigMixin=type('ConfigMixin', (), {}), SchedulerMixin=type('SchedulerMixin', (), {}),
              FlowWrapperSchedulerOutput=dict)
    cls = MG.grab_class(REF + '/models/diffusions/schedulers/flow_adapter.py', 'FlowAdapterScheduler', ns)
    cls.__init__ = TG.register_to_config(cls.__init__)          # (grab_class strips decorators; the class reads self.config.eps)
    return cls


def main():
    torch.set_num_threads(4)
    Scheduler = load_scheduler()
    out = {}
    for k, c in enumerate(TABLES):
        kw = {a: v for a, v in c.items() if a not in ('num_steps', 'seq_len')}
        sch = Scheduler(1000, **kw)
        assert sch.config.base_scheduler == 'UniPCMultistep'
        sch.set_timesteps(c['num_steps'], seq_len=c.get('seq_len'))
        assert sch.sigmas.numel() == c['num_steps'] + 1 and float(sch.sigmas[-1]) == 0.0
        assert torch.equal(sch.base_scheduler.timesteps, sch.timesteps) and bool((sch.scales == 1).all())
        out[f'tab{k}_timesteps'], out[f'tab{k}_sigmas'] = sch.timesteps.clone(), sch.sigmas.clone()
        out[f'tab{k}_base_sigmas'] = sch.base_scheduler.sigmas.clone()
        out[f'tab{k}_eps'] = np.float64(sch.config.eps)
    assert int((out['tab4_base_sigmas'] != out['tab4_sigmas']).sum()) >= 2           # the clamp bites past the first entry there
    out['base_kwargs'] = np.array(sorted(f'{a}={v}' for a, v in UniPCMultistepScheduler.seen.items()))
    MG.save('g14_flow_adapter_tables', **out)


if __name__ == '__main__':
    main()
