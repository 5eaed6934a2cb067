#!/usr/bin/env python3
"""Teacher sampling on one MI355X, synthetic FLUX weights at full depth, 1024^2 (4096 image + 512 text tokens):

  * the fused step (afx_cfg_ortho_coef when orthogonal + afx_teacher_euler_step) against the composed one (bf16 cast of x,
    .float() of both velocities, ops.cfg_combine, ops.euler_roll), interleaved in every round;
  * a 28-step teacher image without CFG and with true CFG 4.0 (TeacherSampler).

HIP events, 3 warm-up rounds, the median of 11 rounds; one JSON line per measurement (also written to ``--out``).

``--edit`` measures teacher image editing instead: the fused edit step (afx_teacher_edit_step / afx_teacher_sde_edit_step)
against the two launches it replaces (afx_teacher_euler_step / afx_teacher_sde_step, then afx_edit_blend in place), at B = 1 and 4,
interleaved in every round, at least 21 rounds, with the bytes per element and the GB/s of each; and a 28-step inpainting roll
(TeacherSampler with x0 and a mask) beside the plain roll.

``--sampler UniPC`` measures the multistep sampler instead (DESIGN.md 6.1 "Multistep sampling"): the fused UniPC step
(afx_teacher_unipc_step at order 2 past the warm-up: 34 B per element, in place, history ring rotated) beside the Euler step (14 B) at B = 1 and 4,
interleaved in every round, with the GB/s of each; and a ``--steps`` UniPC teacher image beside the Euler one.

    python tools/teacher_sampler_bench.py --out profiles/teacher_sampler_bench.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def edit_bench(args, emit):
    """The fused edit step against step + afx_edit_blend, and an inpainting roll against the plain one."""
    from arcflow_amd import MMDiTEngine, TeacherSampler, ops
    from arcflow_amd.weights import random_packed
    dev = 'cuda'
    g = torch.Generator(device=dev).manual_seed(0)
    N, C, T = 4096, 64, 512
    rounds = max(args.rounds, 21)
    # bytes per element: x 4 + pos 2 + neg 2 (+ z 4) read, x' 4 + bf16 2 written by the step; x' 4 + x0 4 + noise0 4 + mask 0.25 read, 4 + 2 written by the blend
    nbytes = dict(euler_fused=22.25, euler_composed=14 + 18.25, sde_fused=26.25, sde_composed=18 + 18.25)
    for B in (1, 4):
        x = torch.randn(B, N, C, generator=g, device=dev)
        pos = torch.randn(B, N, C, generator=g, device=dev).bfloat16()
        neg = torch.randn(B, N, C, generator=g, device=dev).bfloat16()
        z, x0, n0 = (torch.randn(B, N, C, generator=g, device=dev) for _ in range(3))
        mask = torch.rand(B, N, 4, generator=g, device=dev)
        sig, sig_to = torch.full((B,), 0.7, device=dev), torch.full((B,), 0.65, device=dev)
        m, cn = torch.full((B,), 0.8, device=dev), torch.full((B,), 0.6, device=dev)
        xo, xb = torch.empty_like(x), torch.empty(B, N, C, dtype=torch.bfloat16, device=dev)

        def euler_fused():
            ops.teacher_edit_step(x, pos, neg, sig, sig_to, x0, n0, mask, 4.0, None, out=xo, out_bf16=xb)

        def euler_composed():
            ops.teacher_euler_step(x, pos, neg, sig, sig_to, 4.0, None, out=xo, out_bf16=xb)
            ops.edit_blend(xo, x0, n0, mask, sig_to, out=xo, out_bf16=xb)

        def sde_fused():
            ops.teacher_sde_edit_step(x, pos, neg, z, sig, sig_to, m, cn, x0, n0, mask, 4.0, None, out=xo, out_bf16=xb)

        def sde_composed():
            ops.teacher_sde_step(x, pos, neg, z, sig, sig_to, m, cn, 4.0, None, out=xo, out_bf16=xb)
            ops.edit_blend(xo, x0, n0, mask, sig_to, out=xo, out_bf16=xb)

        variants = dict(euler_fused=euler_fused, euler_composed=euler_composed, sde_fused=sde_fused, sde_composed=sde_composed)
        samples = {k: [] for k in variants}
        for r in range(args.warmup + rounds):
            for k, fn in variants.items():                 # interleaved: every round times every variant
                t = timed(fn, 50)
                if r >= args.warmup:
                    samples[k].append(t)
        for k, v in samples.items():
            med = statistics.median(v)
            emit(dict(what='teacher_edit_step', variant=k, shape=[B, N, C], us_median=1e3 * med, us_min=1e3 * min(v), us_max=1e3 * max(v),
                      bytes_per_element=nbytes[k], gb_per_s=nbytes[k] * B * N * C / (med * 1e-3) / 1e9, rounds=len(v), reps_per_round=50))
    if args.skip_image:
        return
    B = 1
    eng = MMDiTEngine('flux', 19, 38, teacher_head=True)
    eng.bind_packed(random_packed('flux', 19, 38, dev, teacher=True))
    cond = dict(prompt_embeds=(torch.randn(B, T, 4096, generator=g, device=dev) * 0.5).bfloat16(),
                pooled=(torch.randn(B, 768, generator=g, device=dev) * 0.5).bfloat16(), hp=64, wp=64)
    noise, x0 = torch.randn(B, N, C, generator=g, device=dev), torch.randn(B, N, C, generator=g, device=dev)
    mask = (torch.rand(B, N, 4, generator=g, device=dev) > 0.5).float()
    s = TeacherSampler(eng, args.steps, guidance_scale=1.0, distilled_guidance=3.5, shift=3.2)
    runs = dict(plain=lambda: s(cond, noise), inpaint=lambda: s(cond, noise, x0=x0, mask=mask, strength=1.0))
    samples = {k: [] for k in runs}
    for r in range(1 + 5):
        for k, fn in runs.items():
            t = timed(fn, 1)
            if r >= 1:
                samples[k].append(t)
    for k, v in samples.items():
        emit(dict(what='teacher_image_1024', variant=k, steps=args.steps, ms_median=statistics.median(v), ms_min=min(v), ms_max=max(v), rounds=len(v)))


def unipc_bench(args, emit):
    """The fused UniPC step beside the Euler step, and a UniPC roll beside the Euler roll."""
    from arcflow_amd import FlowUniPCScheduler, MMDiTEngine, TeacherSampler, ops
    from arcflow_amd.weights import random_packed
    dev = 'cuda'
    g = torch.Generator(device=dev).manual_seed(0)
    N, C, T = 4096, 64, 512
    rounds = max(args.rounds, 21)
    sch = FlowUniPCScheduler(1000, shift=3.2, solver_order=args.solver_order)
    sch.set_timesteps(args.steps)
    i = min(args.steps // 2, args.steps - 2)                     # a step past the warm-up and before the order drops again
    co = sch.coefficients(i)
    reach = max(co.corrector_order, co.predictor_order - 1)
    nbytes = dict(euler=14.0, unipc=4 + 2 + 2 + 4 + 4 * reach + 4 + 2 + 4 + 4)
    for B in (1, 4):
        x = torch.randn(B, N, C, generator=g, device=dev)
        pos = torch.randn(B, N, C, generator=g, device=dev).bfloat16()
        neg = torch.randn(B, N, C, generator=g, device=dev).bfloat16()
        last = torch.randn(B, N, C, generator=g, device=dev)
        ring = [torch.randn(B, N, C, generator=g, device=dev) for _ in range(max(reach, 1))]
        w = torch.tensor(co.row(), dtype=torch.float64).float()[:, None].expand(-1, B).contiguous().to(dev)
        sig, sig_to = torch.full((B,), 0.7, device=dev), torch.full((B,), 0.65, device=dev)
        xo, xb = torch.empty_like(x), torch.empty(B, N, C, dtype=torch.bfloat16, device=dev)

        def euler():
            ops.teacher_euler_step(x, pos, neg, sig, sig_to, 4.0, None, out=xo, out_bf16=xb)

        def unipc():                                               # as the roll calls it: the state in place, the oldest slot overwritten
            ops.teacher_unipc_step(x, pos, neg, w, last, ring[:reach], last, ring[reach - 1], 4.0, None, out=xo, out_bf16=xb)

        variants = dict(euler=euler, unipc=unipc)
        samples = {k: [] for k in variants}
        for r in range(args.warmup + rounds):
            for k, fn in variants.items():                 # interleaved: every round times every variant
                t = timed(fn, 50)
                if r >= args.warmup:
                    samples[k].append(t)
        for k, v in samples.items():
            med = statistics.median(v)
            emit(dict(what='teacher_unipc_step', variant=k, shape=[B, N, C], solver_order=args.solver_order, us_median=1e3 * med, us_min=1e3 * min(v),
                      us_max=1e3 * max(v), bytes_per_element=nbytes[k], gb_per_s=nbytes[k] * B * N * C / (med * 1e-3) / 1e9, rounds=len(v), reps_per_round=50))
    if args.skip_image:
        return
    B = 1
    eng = MMDiTEngine('flux', 19, 38, teacher_head=True)
    eng.bind_packed(random_packed('flux', 19, 38, dev, teacher=True))
    cond = dict(prompt_embeds=(torch.randn(B, T, 4096, generator=g, device=dev) * 0.5).bfloat16(),
                pooled=(torch.randn(B, 768, generator=g, device=dev) * 0.5).bfloat16(), hp=64, wp=64)
    noise = torch.randn(B, N, C, generator=g, device=dev)
    runs = dict(euler=TeacherSampler(eng, args.steps, guidance_scale=1.0, distilled_guidance=3.5, shift=3.2),
                unipc=TeacherSampler(eng, args.steps, guidance_scale=1.0, distilled_guidance=3.5, shift=3.2, sampler='UniPC', solver_order=args.solver_order))
    samples = {k: [] for k in runs}
    for r in range(1 + 5):
        for k, s in runs.items():
            t = timed(lambda: s(cond, noise), 1)
            if r >= 1:
                samples[k].append(t)
    for k, v in samples.items():
        emit(dict(what='teacher_image_1024', variant=k, steps=args.steps, ms_median=statistics.median(v), ms_min=min(v), ms_max=max(v), rounds=len(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--steps', type=int, default=28)
    ap.add_argument('--skip-image', action='store_true')
    ap.add_argument('--edit', action='store_true', help='measure the fused edit step against the two-launch composition, and an inpainting roll')
    ap.add_argument('--sampler', choices=['FlowEulerODE', 'UniPC'], default='FlowEulerODE', help='UniPC: measure the multistep step and roll beside the Euler ones')
    ap.add_argument('--solver-order', type=int, choices=[1, 2, 3], default=2)
    args = ap.parse_args()
    from arcflow_amd import MMDiTEngine, TeacherSampler, ops
    from arcflow_amd.weights import random_packed
    dev = 'cuda'
    g = torch.Generator(device=dev).manual_seed(0)
    B, N, C, T = 1, 4096, 64, 512
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    if args.edit or args.sampler == 'UniPC':
        (edit_bench if args.edit else unipc_bench)(args, emit)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                for rec in lines:
                    f.write(json.dumps(rec) + '\n')
        return

    # ---- the step alone --------------------------------------------------------------------------------------------------
    x = torch.randn(B, N, C, generator=g, device=dev)
    pos = torch.randn(B, N, C, generator=g, device=dev).bfloat16()
    neg = torch.randn(B, N, C, generator=g, device=dev).bfloat16()
    sig, sig_to = torch.full((B,), 0.7, device=dev), torch.full((B,), 0.65, device=dev)
    xo, xb = torch.empty_like(x), torch.empty(B, N, C, dtype=torch.bfloat16, device=dev)
    coef, ws = torch.empty(B, device=dev), ops.cfg_ortho_ws(B, N * C, dev)

    def fused():
        ops.teacher_euler_step(x, pos, neg, sig, sig_to, 4.0, None, out=xo, out_bf16=xb)

    def fused_ortho():
        ops.cfg_ortho_coef(pos, neg, 4.0, out=coef, ws=ws)
        ops.teacher_euler_step(x, pos, neg, sig, sig_to, 4.0, coef, out=xo, out_bf16=xb)

    def composed():
        ops.euler_roll(x, ops.cfg_combine(pos.float(), neg.float(), 4.0), sig, sig_to).to(torch.bfloat16)

    variants = dict(fused=fused, fused_orthogonal=fused_ortho, composed=composed)
    samples = {k: [] for k in variants}
    for r in range(args.warmup + args.rounds):
        for k, fn in variants.items():                 # interleaved: every round times every variant
            t = timed(fn, 50)
            if r >= args.warmup:
                samples[k].append(t)
    for k, v in samples.items():
        emit(dict(what='teacher_step', variant=k, shape=[B, N, C], us_median=1e3 * statistics.median(v), us_min=1e3 * min(v), us_max=1e3 * max(v),
                  rounds=len(v), reps_per_round=50))

    # ---- a whole teacher image ---------------------------------------------------------------------------------------------
    if not args.skip_image:
        eng = MMDiTEngine('flux', 19, 38, teacher_head=True)
        eng.bind_packed(random_packed('flux', 19, 38, dev, teacher=True))
        cond = dict(prompt_embeds=(torch.randn(B, T, 4096, generator=g, device=dev) * 0.5).bfloat16(),
                    negative_prompt_embeds=(torch.randn(B, T, 4096, generator=g, device=dev) * 0.5).bfloat16(),
                    pooled=(torch.randn(B, 768, generator=g, device=dev) * 0.5).bfloat16(),
                    negative_pooled=(torch.randn(B, 768, generator=g, device=dev) * 0.5).bfloat16(), hp=64, wp=64)
        noise = torch.randn(B, N, C, generator=g, device=dev)
        runs = dict(no_cfg=TeacherSampler(eng, args.steps, guidance_scale=1.0, distilled_guidance=3.5, shift=3.2),
                    true_cfg_4=TeacherSampler(eng, args.steps, guidance_scale=4.0, distilled_guidance=3.5, shift=3.2))
        samples = {k: [] for k in runs}
        for r in range(args.warmup + args.rounds):
            for k, s in runs.items():
                t = timed(lambda: s(cond, noise), 1)
                if r >= args.warmup:
                    samples[k].append(t)
        for k, v in samples.items():
            emit(dict(what='teacher_image_1024', variant=k, steps=args.steps, ms_median=statistics.median(v), ms_min=min(v), ms_max=max(v), rounds=len(v),
                      forwards=args.steps * (2 if k == 'true_cfg_4' else 1)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
