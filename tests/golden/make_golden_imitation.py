#!/usr/bin/env python3
"""Generate the golden vectors of the data-based trainer (``ArcFlowImitation``) by EXECUTING the reference's own functions.

Companion of make_golden.py (same rules: build container only, the reference is parsed in place, nothing of it is copied,
only inputs + outputs are written).  Functions executed (paths under /root/reference/lakonlab):
  models/diffusions/arcflow.py       : ArcFlowImitation.sample_t, ArcFlowImitationBase.{piid_segment_momentum (with a TENSOR
                                       segment_size), momentum_integration, policy_average_u_momentum, get_shape_info}
  models/diffusions/gaussian_flow.py : GaussianFlow.sample_forward_diffusion
  models/diffusions/sampler.py       : ContinuousTimeStepSampler (its ``torch.rand`` is fed the recorded uniforms)
  models/diffusions/policies/*.py    : ArcFlowPolicy

Fixtures:
  g10_imitation_sample_t.npz : uniforms u -> (raw_t_src, sigma_t_src, segment_size) for (nfe, timestep_ratio) in
                               {(2, 1.0), (3, 0.5), (4, 0.25)}, shift 3.2; u covers every source index and both clamps
  g11_imitation_step.npz     : one forward_train-equivalent pass, latent [3, 16, 4, 4], K = 16, nfe 3, timestep_ratio 0.5, the three
                               samples on three source indices (two segment sizes), closed-form stub teacher as G7's; also the
                               (raw_t_start, raw_t_end) of every mean-velocity call, which set the conditioning of pred_u

Usage:  python tests/golden/make_golden_imitation.py
"""
import contextlib
import math
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG  # noqa: E402

REF = MG.REF
CASES = [(2, 1.0), (3, 0.5), (4, 0.25)]
SHIFT = 3.2


class FedRandom:
    """Stands in for the ``torch`` module inside the reference's sampler: ``rand`` hands out the recorded uniforms, everything
    else is torch's."""

    def __init__(self):
        self.queue = []

    def rand(self, size, **kw):
        u = self.queue.pop(0)
        assert tuple(u.shape) == tuple(size), (u.shape, size)
        return u.clone()

    def __getattr__(self, name):
        return getattr(torch, name)


def build():
    ArcFlowPolicy = MG.load_policy()
    base_ns = {'torch': torch, 'np': np, 'math': math}
    fed = FedRandom()
    samp_ns = dict(base_ns)
    samp_ns['torch'] = fed
    Sampler = MG.grab_class(REF + '/models/diffusions/sampler.py', 'ContinuousTimeStepSampler', samp_ns)
    trn = dict(base_ns)
    trn['ArcFlowPolicy'] = ArcFlowPolicy
    trn['module_eval'] = lambda m: contextlib.nullcontext()
    MG.grab(REF + '/models/diffusions/arcflow.py',
            ['momentum_integration', 'policy_average_u_momentum', 'piid_segment_momentum', 'get_shape_info'],
            cls='ArcFlowImitationBase', ns=trn)
    imi = MG.grab(REF + '/models/diffusions/arcflow.py', ['sample_t'], cls='ArcFlowImitation', ns=dict(base_ns))
    gf = MG.grab(REF + '/models/diffusions/gaussian_flow.py', ['sample_forward_diffusion'], cls='GaussianFlow', ns=dict(base_ns))
    dif = MG.Obj()
    dif.timestep_sampler = Sampler(num_timesteps=1, shift=SHIFT)
    dif.num_timesteps = 1
    dif.momentum_integration = types.MethodType(trn['momentum_integration'], dif)
    dif.policy_average_u_momentum = types.MethodType(trn['policy_average_u_momentum'], dif)
    dif.get_shape_info = trn['get_shape_info']
    dif.sample_t = types.MethodType(imi['sample_t'], dif)
    dif.sample_forward_diffusion = types.MethodType(gf['sample_forward_diffusion'], dif)
    dif.piid = types.MethodType(trn['piid_segment_momentum'], dif)
    return dif, fed, ArcFlowPolicy


def golden_sample_t(dif, fed):
    # raw_t = 1 - u: u = 0 -> raw_t = 1 (upper clamp of raw_t_src), u > 1 - eps -> raw_t < eps (lower clamp), the rest walks every segment
    u = torch.cat([torch.tensor([0.0, 0.99995, 0.999999, 1 - 1e-4, 0.5]), torch.linspace(0.01, 0.99, 27)]).float()
    out = dict(u=u, shift=np.float32(SHIFT), eps=np.float32(1e-4))
    for nfe, ratio in CASES:
        dif.train_cfg = dict(eps=1e-4, nfe=nfe, timestep_ratio=ratio)
        fed.queue.append(u)
        raw, sigma, t_src, seg = dif.sample_t(u.numel(), 4)
        tag = f'n{nfe}_r{str(ratio).replace(".", "p")}'
        seg = torch.as_tensor(seg, dtype=torch.float32).expand(u.numel())
        idx = torch.round((raw / seg.max()) + (1 - ratio))            # bookkeeping only: which source index each u landed on
        assert set(idx.long().tolist()) == set(range(1, nfe + 1)), (tag, sorted(set(idx.long().tolist())))
        out[tag + '_raw_t_src'] = raw
        out[tag + '_sigma_t_src'] = sigma.flatten()
        out[tag + '_segment_size'] = seg
    MG.save('g10_imitation_sample_t', **out)


def golden_step(dif, fed, ArcFlowPolicy):
    gen = torch.Generator().manual_seed(2711)
    b, k, c, h, w = 3, 16, 16, 4, 4
    nfe, ratio, teacher_ratio = 3, 0.5, 0.6
    means, logw, logg = MG.rand_mixture(gen, b, k, c, h, w)
    x0 = torch.randn(b, c, h, w, generator=gen)
    noise = torch.randn(b, c, h, w, generator=gen)
    u = torch.tensor([0.9, 0.5, 0.1])                                    # raw_t 0.1 / 0.5 / 0.9 -> source index 1 / 2 / 3
    dif.train_cfg = dict(eps=1e-4, nfe=nfe, timestep_ratio=ratio, total_substeps=128, num_intermediate_states=4,
                         window_substeps=3, gm_dropout=0.1)
    captured, x_a_all = {}, []

    def flow_loss(kw):
        captured.update({k2: v.detach().clone() for k2, v in kw.items()})
        return ((kw['u_t_pred'] - kw['u_t']) ** 2).flatten(1).mean(dim=1).mul(0.5 * 30.0).mean()

    def teacher(return_u=True, x_t=None, t=None, **kw):
        x_a_all.append(x_t.detach().clone())
        return 0.3 * x_t - 0.7 * t.reshape(-1, 1, 1, 1) + 0.05 * torch.roll(x_t, 1, dims=-1)

    windows = []                                  # (raw_t_start, raw_t_end) as piid_segment_momentum hands them to the mean-velocity call
    inner = dif.policy_average_u_momentum

    def recording(sigma_t_src, x_t_start, sigma_t_start, raw_t_start, raw_t_end, *a, **kw):
        windows.append((raw_t_start.clone(), raw_t_end.clone()))
        return inner(sigma_t_src, x_t_start, sigma_t_start, raw_t_start, raw_t_end, *a, **kw)

    dif.policy_average_u_momentum = recording
    dif.flow_loss = flow_loss
    fed.queue.append(u)
    raw_src, sigma_src, t_src, seg = dif.sample_t(b, 4)
    assert len(set(raw_src.tolist())) == 3 and len(set(seg.tolist())) == 2
    x_t_src, _, _ = dif.sample_forward_diffusion(x0, t_src, noise)
    pol = ArcFlowPolicy(dict(means=means, logweights=logw.clone(), loggammas=logg), x_t_src, sigma_src)
    seed = 14
    torch.manual_seed(seed)
    loss, x_dst, raw_dst = dif.piid(teacher, pol, x_t_src, raw_src, sigma_src, teacher_ratio, seg, dict())
    assert x_dst is None
    dif.policy_average_u_momentum = inner
    torch.manual_seed(seed)
    u_drop = torch.rand(b, k, 1, 1, 1)
    u_stu = torch.rand(b, 4)
    u_tea = torch.rand(b, 3)
    MG.save('g11_imitation_step', means=means, logw=logw, logg=logg, x0=x0, noise=noise, u=u, nfe=np.int64(nfe),
            timestep_ratio=np.float32(ratio), teacher_ratio=np.float32(teacher_ratio), u_drop=u_drop, u_student=u_stu, u_teacher=u_tea,
            raw_t_src=raw_src, sigma_t_src=sigma_src.flatten(), segment_size=seg, x_t_src=x_t_src, x_t_a=torch.stack(x_a_all),
            pred_u=captured['u_t_pred'], tgt_u=captured['u_t'], timesteps=captured['timesteps'], loss=loss, raw_t_dst=raw_dst,
            raw_t_a=torch.stack([a for a, _ in windows]), raw_t_e=torch.stack([e for _, e in windows]))


def main():
    torch.set_num_threads(4)
    dif, fed, ArcFlowPolicy = build()
    golden_sample_t(dif, fed)
    golden_step(dif, fed, ArcFlowPolicy)


if __name__ == '__main__':
    main()
