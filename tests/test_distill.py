"""Distillation step: (GPU) one full iteration of the HIP path against torch autograd on the CPU oracle, same
draws; (CPU, gloo world_size 2) the data-parallel gradient exchange."""
import os

import pytest
import torch


def _setup():
    from arcflow_amd.weights import init_arcflow_heads_from_teacher
    from oracle import dit_ref as D
    cfg = D.FluxCfg(num_layers=1, num_single_layers=1, heads=2, joint_dim=128, pooled_dim=64)
    w = D.make_flux_weights(cfg, seed=7, teacher_head=True)
    for k in [k for k in w if k.startswith('proj_out_')]:
        del w[k]
    w = init_arcflow_heads_from_teacher(w, generator=torch.Generator().manual_seed(1))
    # non-trivial log-weights / rates so every gradient path is exercised
    g = torch.Generator().manual_seed(2)
    w['proj_out_logweights.weight'] = (torch.randn(64, 256, generator=g) * 0.05).bfloat16()
    w['proj_out_loggamma.weight'] = (torch.randn(60, 256, generator=g) * 0.05).bfloat16()
    return cfg, w


@pytest.mark.gpu
def test_train_step_matches_cpu_autograd():
    from arcflow_amd.train import ArcFlowDistiller, DistillConfig
    from oracle import arcflow_ref as R
    from oracle import dit_ref as D
    cfg, w = _setup()
    B, hp, wp, T = 2, 8, 8, 12
    N = hp * wp
    g = torch.Generator().manual_seed(3)
    pe = (torch.randn(B, T, 128, generator=g) * 0.5).bfloat16()
    pooled = (torch.randn(B, 64, generator=g) * 0.5).bfloat16()
    x0 = torch.randn(B, N, 64, generator=g)
    draws = [(torch.rand(B, 16, generator=g), torch.rand(B, 4, generator=g), torch.rand(B, 3, generator=g)) for _ in range(2)]
    dc = DistillConfig(num_decay_iters=4, warmup_iters=0, grad_clip_begin_iter=0, ema_start_iter=0)
    dist = ArcFlowDistiller('flux', dict(num_double=1, num_single=1, heads=2, joint_dim=128, pooled_dim=64), w, dc)
    dist.iteration = 1                       # teacher_ratio = 0.75: both student and teacher intervals active
    p_before = dist.params.clone()
    cond = dict(prompt_embeds=pe.cuda(), pooled=pooled.cuda(), hp=hp, wp=wp)
    info = dist.train_step(cond, B, x_init=x0.cuda(), draws=draws)
    torch.cuda.synchronize()

    # ---- CPU reference: fp32 oracle forward, autograd through policy math + heads + norm_out -------------------
    names = ['proj_out_means', 'proj_out_logweights', 'proj_out_loggamma', 'norm_out.linear']
    wt = {k: v.float() for k, v in w.items()}
    leaves = {}
    for nm in names:
        for s in ('.weight', '.bias'):
            leaves[nm + s] = wt[nm + s].clone().requires_grad_(True)
    ws = dict(wt)
    ws.update(leaves)
    w_teacher = dict(wt)
    gd = torch.full((B,), 3.5)

    def teacher(x_lat, t):
        with torch.no_grad():
            xt = R.pack_latents(x_lat)
            u = D.flux_teacher_forward(w_teacher, cfg, xt.bfloat16().float(), pe.float(), pooled.float(), t, gd, hp, wp)
            return R.unpack_latents(u.bfloat16().float(), hp, wp)       # the engine returns bf16

    x, raw = x0.clone(), torch.ones(B)
    total = 0
    for step in range(2):
        sig = R.shift_sigma(raw)
        m, lw, lg = D.flux_forward(ws, cfg, x.bfloat16().float(), pe.float(), pooled.float(), sig, gd, hp, wp)
        # the engine hands bf16 outputs to the policy math: round with a straight-through gradient
        rnd = lambda t: t + (t.bfloat16().float() - t).detach()   # noqa: E731
        ml, lwl, lgl = R.unpack_mixture(rnd(m), rnd(lw), rnd(lg), hp, wp)
        u_drop, u_stu, u_tea = draws[step]
        mask = R.gm_dropout_mask(u_drop.reshape(B, 16, 1, 1, 1), 0.1)
        loss, x_dst, raw = R.segment_distill(teacher, R.unpack_latents(x, hp, wp), ml, lwl, lgl, raw, 0.75, 0.5,
                                             u_stu, u_tea, drop_mask=mask)
        total = total + loss * 0.5
        x = R.pack_latents(x_dst.detach())
    total.backward()

    assert abs(info['loss'] - total.item()) < 2e-2 * abs(total.item()) + 1e-4, (info['loss'], total.item())
    rel = ((dist.last_x.cpu() - x).norm() / x.norm()).item()
    assert rel < 2e-2, rel
    got = dist.trainable_state_dict()
    # gradient check through the applied AdamW update is indirect; compare the raw summed gradient buffers instead
    gsum = dist.grads[0]
    K, C, L, Dm = 16, 64, 4, 256
    hw = gsum[:1152 * Dm].view(1152, Dm).cpu()
    hb = gsum[1152 * Dm:1152 * Dm + 1152].cpu()
    ref_hw = torch.cat([leaves['proj_out_means.weight'].grad, leaves['proj_out_logweights.weight'].grad,
                        leaves['proj_out_loggamma.weight'].grad])
    ref_hb = torch.cat([leaves['proj_out_means.bias'].grad, leaves['proj_out_logweights.bias'].grad,
                        leaves['proj_out_loggamma.bias'].grad])

    def rel_l2(a, b):
        return ((a - b).norm() / b.norm().clamp(min=1e-12)).item()
    assert rel_l2(hw[:1148], ref_hw) < 5e-2, rel_l2(hw[:1148], ref_hw)
    assert rel_l2(hb[:1148], ref_hb) < 5e-2, rel_l2(hb[:1148], ref_hb)
    off = 1152 * Dm + 1152
    nw = gsum[off:off + 2 * Dm * Dm].view(2 * Dm, Dm).cpu()
    nb = gsum[off + 2 * Dm * Dm:].cpu()
    assert rel_l2(nw, leaves['norm_out.linear.weight'].grad) < 5e-2
    assert rel_l2(nb, leaves['norm_out.linear.bias'].grad) < 5e-2
    # optimizer moved every trainable tensor and the EMA followed (start_iter 0 -> lerp with beta(t=2))
    assert info['grad_norm'] > 0 and not info['skipped']
    assert (dist.params - p_before).abs().max().item() > 0
    assert set(got) == {n + s for n in names for s in ('.weight', '.bias')}
    # a non-finite gradient skips the update (base.py:91-95)
    p_now = dist.params.clone()
    info = dist.train_step(cond, B, x_init=torch.full((B, N, 64), float('nan'), device='cuda'), draws=draws)
    assert info['skipped'] and torch.equal(dist.params, p_now)


@pytest.mark.gpu
def test_teacher_fp8_step_tracks_bf16_step_and_oracle():
    """BASELINE.json configs[4] ("fp8 MFMA fwd + bf16 grads"): DistillConfig.teacher_fp8 runs the frozen teacher's block linears on
    the e4m3 MFMA (row-wise scales); student forward, gradients and optimizer stay bf16 / fp32.  Stated tolerance: the teacher
    targets move by fp8 quantisation noise only -- loss within 5 %, every gradient block within 0.25 rel-L2 of the bf16-teacher
    step on the same draws, and the loss within 6 % of autograd through the fp32 CPU oracle."""
    from arcflow_amd.train import ArcFlowDistiller, DistillConfig
    from oracle import arcflow_ref as R
    from oracle import dit_ref as D
    cfg, w = _setup()
    B, hp, wp, T = 2, 8, 8, 12
    N = hp * wp
    g = torch.Generator().manual_seed(3)
    pe = (torch.randn(B, T, 128, generator=g) * 0.5).bfloat16()
    pooled = (torch.randn(B, 64, generator=g) * 0.5).bfloat16()
    x0 = torch.randn(B, N, 64, generator=g)
    draws = [(torch.rand(B, 16, generator=g), torch.rand(B, 4, generator=g), torch.rand(B, 3, generator=g)) for _ in range(2)]
    cond = dict(prompt_embeds=pe.cuda(), pooled=pooled.cuda(), hp=hp, wp=wp)
    res = {}
    for fp8 in (False, True):
        dc = DistillConfig(num_decay_iters=4, warmup_iters=0, grad_clip_begin_iter=10 ** 9, ema_start_iter=0, teacher_fp8=fp8)
        d = ArcFlowDistiller('flux', dict(num_double=1, num_single=1, heads=2, joint_dim=128, pooled_dim=64), w, dc)
        assert d.teacher._weights.get('d0.img_qkv.weight_q') is not None if fp8 else True       # the quantised copies exist
        d.iteration = 1
        info = d.train_step(cond, B, x_init=x0.cuda(), draws=draws)
        res[fp8] = (info, d.grad.clone(), d.last_x.clone())
    (i16, g16, x16), (i8, g8, x8) = res[False], res[True]
    assert not i8['skipped'] and i8['loss'] != i16['loss']                          # the fp8 teacher really ran
    assert abs(i8['loss'] - i16['loss']) < 5e-2 * abs(i16['loss']), (i8['loss'], i16['loss'])
    assert ((g8 - g16).norm() / g16.norm()).item() < 0.25
    assert ((x8 - x16).norm() / x16.norm()).item() < 3e-2
    # ---- fp32 CPU oracle (same chain as test_train_step_matches_cpu_autograd, loss only) -----------------------------------
    wt = {k: v.float() for k, v in w.items()}
    gd = torch.full((B,), 3.5)

    def teacher(x_lat, t):
        u = D.flux_teacher_forward(wt, cfg, R.pack_latents(x_lat).bfloat16().float(), pe.float(), pooled.float(), t, gd, hp, wp)
        return R.unpack_latents(u.bfloat16().float(), hp, wp)
    with torch.no_grad():
        x, raw, total = x0.clone(), torch.ones(B), 0.0
        for step in range(2):
            m, lw, lg = D.flux_forward(wt, cfg, x.bfloat16().float(), pe.float(), pooled.float(), R.shift_sigma(raw), gd, hp, wp)
            ml, lwl, lgl = R.unpack_mixture(m.bfloat16().float(), lw.bfloat16().float(), lg.bfloat16().float(), hp, wp)
            u_drop, u_stu, u_tea = draws[step]
            mask = R.gm_dropout_mask(u_drop.reshape(B, 16, 1, 1, 1), 0.1)
            loss, x_dst, raw = R.segment_distill(teacher, R.unpack_latents(x, hp, wp), ml, lwl, lgl, raw, 0.75, 0.5, u_stu, u_tea, drop_mask=mask)
            total += float(loss) * 0.5
            x = R.pack_latents(x_dst)
    assert abs(i8['loss'] - total) < 6e-2 * abs(total), (i8['loss'], total)


def _dp_worker(rank, world, port, tmp):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from arcflow_amd.train.reducer import GradReducer
    red = GradReducer()
    assert red.world == world
    g = torch.Generator().manual_seed(100 + rank)
    buf = torch.randn(5000, generator=g)                # ONE flat gradient buffer, exchanged in slices as they become final
    local = buf.clone()
    slices = [(3000, 4200), (1800, 3000), (700, 1800)]  # "blocks" in reverse, the way the last backward releases them
    for a, b in slices:
        red.launch(buf[a:b])
    red.launch(buf[:700])                               # the rest: heads ...
    red.launch(buf[4200:])                              # ... and the embedder pair
    assert red.bytes_launched == buf.numel() * 4        # every byte exactly once per iteration
    scale = red.finish()
    assert scale == 1.0 / world and red.bytes_launched == 0
    # construction-time state sync (DDP's _sync_module_states): ranks start from different values, a mismatch is detected, the
    # broadcast makes them rank 0's
    state = torch.randn(1000, generator=torch.Generator().manual_seed(7 + rank))
    mine = state.clone()
    caught = False
    try:
        red.check_consistent(state)
    except RuntimeError as e:
        caught = 'disagree' in str(e)
    red.broadcast_(state)
    red.check_consistent(state)
    # a NaN on ONE rank: both ranks must raise the "non-finite" error (not "disagree"), and neither may hang in the collectives
    poisoned = state.clone()
    if rank == 1:
        poisoned[17] = float('nan')
    nonfinite = False
    try:
        red.check_consistent(poisoned)
    except RuntimeError as e:
        nonfinite = 'non-finite' in str(e)
    assert nonfinite
    torch.save(dict(local=local, reduced=buf, mx=red.all_reduce_max(float(rank + 1), 'cpu'), caught=caught, state=state, mine=mine),
               os.path.join(tmp, f'r{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


def test_grad_reducer_gloo_world2(tmp_path):
    import torch.multiprocessing as mp
    port = 29500 + os.getpid() % 2000
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(tmp_path, f'r{i}.pt')) for i in range(2))
    expect = r0['local'] + r1['local']
    assert torch.allclose(r0['reduced'], expect) and torch.allclose(r1['reduced'], expect)
    assert r0['mx'] == 2.0 and r1['mx'] == 2.0
    # DDP-style state sync: the mismatch was detected on both ranks, then everybody holds rank 0's values
    assert r0['caught'] and r1['caught'] and not torch.equal(r0['mine'], r1['mine'])
    assert torch.equal(r0['state'], r0['mine']) and torch.equal(r1['state'], r0['mine'])
    red_single = __import__('arcflow_amd.train.reducer', fromlist=['GradReducer']).GradReducer()
    assert red_single.world == 1 and red_single.finish() == 1.0


def test_block_slices_cover_the_lora_region_once():
    """The per-block gradient slices the distiller hands to the reducer are contiguous, disjoint, block-major, and together
    with 'the rest' cover the flat buffer exactly once (pure index arithmetic: no GPU)."""
    from arcflow_amd.train.trunk import lora_targets
    for family, nd, ns in (('flux', 3, 5), ('qwen', 4, 0)):
        D, r, base = 256, 16, 1000
        off, spans = base, {}
        for name, key, row0, out_f, in_f in lora_targets(family, nd, ns, D):
            n = r * in_f + out_f * r
            blk = key.split('.')[0]
            a, b = spans.get(blk, (off, off))
            assert b == off or blk not in spans, 'a block\'s adapters must be contiguous in the flat buffer'
            spans[blk] = (min(a, off), off + n)
            off += n
        blocks = [f'd{i}' for i in range(nd)] + [f's{i}' for i in range(ns)]
        pos = base
        for blk in blocks:
            a, b = spans[blk]
            assert a == pos and b > a
            pos = b
        assert spans['temb'][0] == pos and spans['temb'][1] == off      # the embedder pair closes the buffer


def _dp_train_worker(rank, world, port, tmp):
    """Rank ``rank`` of a 2-process data-parallel step: sample ``rank`` of the 2-sample batch, both ranks on cuda:0
    (gloo; the reducer stages device buffers through the host because RCCL refuses two ranks on one device)."""
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from arcflow_amd.train import ArcFlowDistiller
    st = torch.load(os.path.join(tmp, 'setup.pt'), weights_only=False)
    # every rank draws its adapter initialisation from a DIFFERENT seed: the construction-time broadcast (sync_module_states,
    # DDP's _sync_module_states) must leave all of them with rank 0's trainables
    dd = ArcFlowDistiller('flux', dict(num_double=1, num_single=1, heads=2, joint_dim=128, pooled_dim=64), st['w'], st['dc'],
                          init_seed=1234 + 17 * rank)
    assert dd.reducer.world == world and dd.reducer.rank == rank
    torch.save(dd.params.cpu(), os.path.join(tmp, f'init{rank}.pt'))
    for sp in dd.trunk.specs:
        dd.trunk.B(sp).copy_(st['B'][sp.name].cuda())
    dd.trunk.refresh()
    dd.iteration = 1
    sl = slice(rank, rank + 1)
    cond = dict(prompt_embeds=st['pe'][sl].cuda(), pooled=st['pooled'][sl].cuda(), hp=8, wp=8)
    draws = [tuple(d[sl] for d in step) for step in st['draws']]
    info = dd.train_step(cond, 1, x_init=st['x0'][sl].cuda(), draws=draws)
    torch.cuda.synchronize()
    torch.save(dict(grad=dd.grad.cpu(), params=dd.params.cpu(), info=info), os.path.join(tmp, f'dp{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_two_rank_train_step_equals_single_process_batch(tmp_path):
    """Reference semantics (ddp_wrapper.py:19-25, base_diffusion.py:59-60): the batch is sharded over the ranks, gradients
    are averaged.  Two processes with one sample each (fixed draws) must reproduce the single-process 2-sample iteration:
    same exchanged gradient (x 1/world), same parameters after AdamW."""
    import torch.multiprocessing as mp
    from arcflow_amd.train import ArcFlowDistiller, DistillConfig
    cfg, w = _setup()
    B, hp, wp, T, r = 2, 8, 8, 64, 64
    g = torch.Generator().manual_seed(15)
    pe = (torch.randn(B, T, 128, generator=g) * 0.5).bfloat16()
    pooled = (torch.randn(B, 64, generator=g) * 0.5).bfloat16()
    x0 = torch.randn(B, hp * wp, 64, generator=g)
    draws = [(torch.rand(B, 16, generator=g), torch.rand(B, 4, generator=g), torch.rand(B, 3, generator=g)) for _ in range(2)]
    dc = DistillConfig(num_decay_iters=4, warmup_iters=0, grad_clip_begin_iter=10 ** 9, ema_start_iter=0, lora_rank=r)
    single = ArcFlowDistiller('flux', dict(num_double=1, num_single=1, heads=2, joint_dim=128, pooled_dim=64), w, dc)
    Bm = {sp.name: (torch.randn(sp.out_f, r, generator=g) * 0.02) for sp in single.trunk.specs}
    for sp in single.trunk.specs:
        single.trunk.B(sp).copy_(Bm[sp.name].cuda())
    single.trunk.refresh()
    single.iteration = 1
    info = single.train_step(dict(prompt_embeds=pe.cuda(), pooled=pooled.cuda(), hp=hp, wp=wp), B, x_init=x0.cuda(), draws=draws)
    torch.cuda.synchronize()
    torch.save(dict(w=w, dc=dc, B=Bm, pe=pe, pooled=pooled, x0=x0, draws=draws), os.path.join(tmp_path, 'setup.pt'))
    port = 29500 + (os.getpid() + 7) % 2000
    mp.spawn(_dp_train_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(tmp_path, f'dp{i}.pt'), weights_only=False) for i in range(2))
    assert torch.equal(r0['grad'], r1['grad']) and torch.equal(r0['params'], r1['params'])      # ranks stay in lock-step
    i0, i1 = (torch.load(os.path.join(tmp_path, f'init{i}.pt')) for i in range(2))
    assert torch.equal(i0, i1)                                   # rank 1 drew seed 1251 and was overwritten with rank 0's (seed 1234) state
    ref_g, ref_p = single.grad.cpu(), single.params.cpu()
    got_g = r0['grad'] * 0.5                                    # the exchanged SUM x 1/world
    rel = ((got_g - ref_g).norm() / ref_g.norm()).item()
    assert rel < 1e-4, rel
    assert ref_g.abs().max().item() > 0
    assert ((r0['params'] - ref_p).abs().max() / ref_p.abs().max()).item() < 1e-5
    assert abs(r0['info']['grad_norm'] - info['grad_norm']) < 1e-3 * info['grad_norm']
    # the loss is each rank's local mean: their average is the single-process loss
    assert abs(0.5 * (r0['info']['loss'] + r1['info']['loss']) - info['loss']) < 1e-3 * abs(info['loss'])


@pytest.mark.gpu
@pytest.mark.parametrize('B', [1, 2, 4])
def test_teacher_modulation_prepared_per_chunk_equals_per_forward(B, monkeypatch):
    """The teacher's timesteps of a segment are known before its roll-out: their AdaLN modulation vectors come out of one pass over the stacked modulation matrix
    per chunk of states (8 / B states) instead of one pass per teacher forward.  Same kernels, same numbers (the engine-level test pins bit-identity: test_hip_engine.py): the
    iteration equals ARCFLOW_TRAIN_PREP_MOD=0 (B = 4: chunks of 2 states, B = 2: one chunk of 4, B = 1: one chunk of 4 of the 8 rows)."""
    from arcflow_amd.train import ArcFlowDistiller, DistillConfig
    cfg, w = _setup()
    hp, wp, T = 8, 8, 12
    g = torch.Generator().manual_seed(41 + B)
    pe = (torch.randn(B, T, 128, generator=g) * 0.5).bfloat16().cuda()
    pooled = (torch.randn(B, 64, generator=g) * 0.5).bfloat16().cuda()
    x0 = torch.randn(B, hp * wp, 64, generator=g).cuda()
    draws = [(torch.rand(B, 16, generator=g), torch.rand(B, 4, generator=g), torch.rand(B, 3, generator=g)) for _ in range(2)]
    dc = DistillConfig(num_decay_iters=4, warmup_iters=0, grad_clip_begin_iter=10 ** 9, ema_start_iter=0)
    eng = dict(num_double=1, num_single=1, heads=2, joint_dim=128, pooled_dim=64)
    res = []
    for mode in ('1', '0'):
        monkeypatch.setenv('ARCFLOW_TRAIN_PREP_MOD', mode)
        d = ArcFlowDistiller('flux', eng, w, dc)
        d.iteration = 1
        calls = []
        orig = d.teacher.prepare_steps
        d.teacher.prepare_steps = lambda *a, **k: calls.append(1) or orig(*a, **k)
        info = d.train_step(dict(prompt_embeds=pe, pooled=pooled, hp=hp, wp=wp), B, x_init=x0, draws=draws)
        torch.cuda.synchronize()
        res.append((info['loss'], d.grad.clone(), d.params.clone(), len(calls)))
    assert res[0][3] == (4 if B == 4 else 2) and res[1][3] == 0          # two segments x (4 states / chunk) passes, none with the switch off
    # (the loss scalar and two of the gradient reductions are summed with float atomics: equal up to their order, run to run as well)
    assert abs(res[0][0] - res[1][0]) < 1e-6 * abs(res[1][0])
    assert ((res[0][1] - res[1][1]).norm() / res[1][1].norm()).item() < 1e-6
    assert ((res[0][2] - res[1][2]).norm() / res[1][2].norm()).item() < 1e-7


@pytest.mark.gpu
def test_micro_batched_step_equals_one_batch():
    """more than 4 samples per GPU run as micro-batches of <= 4 and must give the gradient of the whole
    batch (mean over ALL samples), not of the last chunk."""
    from arcflow_amd.train import ArcFlowDistiller, DistillConfig
    cfg, w = _setup()
    B, hp, wp, T = 6, 8, 8, 12
    g = torch.Generator().manual_seed(33)
    pe = (torch.randn(B, T, 128, generator=g) * 0.5).bfloat16().cuda()
    pooled = (torch.randn(B, 64, generator=g) * 0.5).bfloat16().cuda()
    x0 = torch.randn(B, hp * wp, 64, generator=g).cuda()
    draws = [(torch.rand(B, 16, generator=g), torch.rand(B, 4, generator=g), torch.rand(B, 3, generator=g)) for _ in range(2)]
    dc = DistillConfig(num_decay_iters=4, warmup_iters=0, grad_clip_begin_iter=10 ** 9, ema_start_iter=0)
    eng = dict(num_double=1, num_single=1, heads=2, joint_dim=128, pooled_dim=64)
    big = ArcFlowDistiller('flux', eng, w, dc)
    big.iteration = 1
    info = big.train_step(dict(prompt_embeds=pe, pooled=pooled, hp=hp, wp=wp), B, x_init=x0, draws=draws)
    # reference: the same six samples as two independent 3-sample steps, gradients combined as (3 g_a + 3 g_b) / 6
    acc, loss = torch.zeros_like(big.grad), 0.0
    for a, b in ((0, 3), (3, 6)):
        d = ArcFlowDistiller('flux', eng, w, dc)
        d.iteration = 1
        i2 = d.train_step(dict(prompt_embeds=pe[a:b], pooled=pooled[a:b], hp=hp, wp=wp), b - a, x_init=x0[a:b],
                          draws=[tuple(t[a:b] for t in step) for step in draws])
        acc += d.grad * 0.5
        loss += 0.5 * i2['loss']
    rel = ((big.grad - acc).norm() / acc.norm()).item()
    assert rel < 2e-3, rel          # chunk boundaries differ (4+2 vs 3+3): bf16 GEMM tiles see different row groupings
    assert abs(info['loss'] - loss) < 1e-3 * abs(loss)
    assert big.last_x.shape == (B, hp * wp, 64)


@pytest.mark.gpu
def test_lora_trunk_backward_matches_cpu_autograd():
    """LoRA adapter gradients through the whole trunk (block recompute, flash-attention backward, dgrad GEMMs,
    LN / RoPE / GELU backward) against autograd through the fp32 oracle with W' = W + B A."""
    from arcflow_amd.train import ArcFlowDistiller, DistillConfig
    from arcflow_amd.train.trunk import lora_targets
    from oracle import arcflow_ref as R
    from oracle import dit_ref as D
    cfg, w = _setup()
    B, hp, wp, T, r = 2, 8, 8, 64, 64
    N = hp * wp
    g = torch.Generator().manual_seed(5)
    pe = (torch.randn(B, T, 128, generator=g) * 0.5).bfloat16()
    pooled = (torch.randn(B, 64, generator=g) * 0.5).bfloat16()
    x0 = torch.randn(B, N, 64, generator=g)
    draws = [(torch.rand(B, 16, generator=g), torch.rand(B, 4, generator=g), torch.rand(B, 3, generator=g)) for _ in range(2)]
    dc = DistillConfig(num_decay_iters=4, warmup_iters=0, grad_clip_begin_iter=10 ** 9, ema_start_iter=0, lora_rank=r)
    dist = ArcFlowDistiller('flux', dict(num_double=1, num_single=1, heads=2, joint_dim=128, pooled_dim=64), w, dc)
    tr = dist.trunk
    # non-zero B so that dA is exercised; keep a host copy of A, B for the oracle
    AB = {}
    for sp in tr.specs:
        tr.B(sp).copy_((torch.randn(sp.out_f, r, generator=g) * 0.02).cuda())
        AB[sp.name] = (tr.A(sp).cpu().clone(), tr.B(sp).cpu().clone())
    tr.refresh()
    dist.iteration = 1
    cond = dict(prompt_embeds=pe.cuda(), pooled=pooled.cuda(), hp=hp, wp=wp)
    info = dist.train_step(cond, B, x_init=x0.cuda(), draws=draws)
    torch.cuda.synchronize()
    gsum = dist.grads[0]

    # ---- oracle -------------------------------------------------------------------------------------------------
    wt = {k: v.float() for k, v in w.items()}
    leaves = {}
    ws = dict(wt)
    rnd = lambda t: t + (t.bfloat16().float() - t).detach()   # noqa: E731
    for sp in tr.specs:
        a = AB[sp.name][0].bfloat16().float().requires_grad_(True)       # the kernels consume bf16 working copies
        b = AB[sp.name][1].bfloat16().float().requires_grad_(True)
        leaves[sp.name] = (a, b)
        ws[sp.name + '.weight'] = rnd(wt[sp.name + '.weight'] + b @ a)
    gd = torch.full((B,), 3.5)

    def teacher(x_lat, t):
        with torch.no_grad():
            u = D.flux_teacher_forward(wt, cfg, R.pack_latents(x_lat).bfloat16().float(), pe.float(), pooled.float(), t, gd, hp, wp)
            return R.unpack_latents(u.bfloat16().float(), hp, wp)
    x, raw = x0.clone(), torch.ones(B)
    total = 0
    for step in range(2):
        m, lw, lg = D.flux_forward(ws, cfg, x.bfloat16().float(), pe.float(), pooled.float(), R.shift_sigma(raw), gd, hp, wp)
        ml, lwl, lgl = R.unpack_mixture(rnd(m), rnd(lw), rnd(lg), hp, wp)
        u_drop, u_stu, u_tea = draws[step]
        mask = R.gm_dropout_mask(u_drop.reshape(B, 16, 1, 1, 1), 0.1)
        loss, x_dst, raw = R.segment_distill(teacher, R.unpack_latents(x, hp, wp), ml, lwl, lgl, raw, 0.75, 0.5, u_stu, u_tea, drop_mask=mask)
        total = total + loss * 0.5
        x = R.pack_latents(x_dst.detach())
    total.backward()
    assert abs(info['loss'] - total.item()) < 3e-2 * abs(total.item()) + 1e-4, (info['loss'], total.item())

    def rel_l2(a, b):
        return ((a - b).norm() / b.norm().clamp(min=1e-12)).item()
    worst = 0.0
    for sp in tr.specs:
        ga, gb = tr.A(sp, gsum).cpu(), tr.B(sp, gsum).cpu()
        ra, rb = leaves[sp.name][0].grad, leaves[sp.name][1].grad
        ea, eb = rel_l2(ga, ra), rel_l2(gb, rb)
        worst = max(worst, ea, eb)
        assert ea < 8e-2 and eb < 8e-2, (sp.name, ea, eb)
    assert len(tr.specs) == len(lora_targets('flux', 1, 1, 256)) == 8        # 6 block linears + the timestep-embedder pair
    # the step changed the adapters and re-merged the student's weights
    sp = tr.specs[0]
    assert (tr.A(sp).cpu() - AB[sp.name][0]).abs().max().item() > 0
    merged = tr.merged_state()[sp.name].float().cpu()
    ref = (w[sp.name + '.weight'].float() + tr.B(sp).cpu().bfloat16().float() @ tr.A(sp).cpu().bfloat16().float())
    assert rel_l2(merged, ref) < 4e-3


@pytest.mark.gpu
def test_qwen_distill_step_with_true_cfg_teacher():
    """Qwen-Image family: 2 double blocks, LoRA on img_mlp (all) + txt_mlp (all but the last block), teacher with
    true classifier-free guidance (negative prompt, scale 4: configs/qwen/arcqwen_2nfe_k16.py:100) vs CPU autograd."""
    from arcflow_amd.train import ArcFlowDistiller, DistillConfig
    from arcflow_amd.weights import init_arcflow_heads_from_teacher
    from oracle import arcflow_ref as R
    from oracle import dit_ref as D
    cfg = D.QwenCfg(num_layers=2, heads=2, joint_dim=192)
    w = D.make_qwen_weights(cfg, seed=11)
    g = torch.Generator().manual_seed(12)
    w['proj_out.weight'] = (torch.randn(64, 256, generator=g) * 0.05).bfloat16()
    w['proj_out.bias'] = (torch.randn(64, generator=g) * 0.02).bfloat16()
    B, hp, wp, T, r = 1, 8, 8, 64, 64
    N = hp * wp
    pe = (torch.randn(B, T, 192, generator=g) * 0.5).bfloat16()
    ne = (torch.randn(B, T, 192, generator=g) * 0.5).bfloat16()
    x0 = torch.randn(B, N, 64, generator=g)
    draws = [(torch.rand(B, 16, generator=g), torch.rand(B, 4, generator=g), torch.rand(B, 3, generator=g)) for _ in range(2)]
    dc = DistillConfig(num_decay_iters=4, warmup_iters=0, grad_clip_begin_iter=10 ** 9, ema_start_iter=0, lora_rank=r,
                       teacher_guidance_scale=4.0)
    dist = ArcFlowDistiller('qwen', dict(num_double=2, heads=2, joint_dim=192), w, dc)
    tr = dist.trunk
    assert len(tr.specs) == 8                       # 2 x img_mlp pairs + 1 x txt_mlp pair + the timestep-embedder pair
    AB = {}
    for sp in tr.specs:
        tr.B(sp).copy_((torch.randn(sp.out_f, r, generator=g) * 0.02).cuda())
        AB[sp.name] = (tr.A(sp).cpu().clone(), tr.B(sp).cpu().clone())
    tr.refresh()
    dist.iteration = 2
    cond = dict(prompt_embeds=pe.cuda(), negative_prompt_embeds=ne.cuda(), hp=hp, wp=wp)
    info = dist.train_step(cond, B, x_init=x0.cuda(), draws=draws)
    gsum = dist.grads[0]
    wt = {k: v.float() for k, v in w.items()}
    ws = dict(wt)
    rnd = lambda t: t + (t.bfloat16().float() - t).detach()   # noqa: E731
    leaves = {}
    for sp in tr.specs:
        a = AB[sp.name][0].bfloat16().float().requires_grad_(True)
        b = AB[sp.name][1].bfloat16().float().requires_grad_(True)
        leaves[sp.name] = (a, b)
        ws[sp.name + '.weight'] = rnd(wt[sp.name + '.weight'] + b @ a)

    def qwen_teacher_u(ctx, x_tok, t):
        # plain Qwen-Image forward: same trunk, single proj_out head (diffusers/qwen.py:107-139)
        saved = {k: wt[k] for k in ('proj_out_means.weight', 'proj_out_means.bias')}
        wv = dict(wt)
        wv['proj_out_means.weight'] = torch.cat([wt['proj_out.weight']] + [torch.zeros(64, 256)] * 15)
        wv['proj_out_means.bias'] = torch.cat([wt['proj_out.bias']] + [torch.zeros(64)] * 15)
        m, _, _ = D.qwen_forward(wv, cfg, x_tok, ctx, t, hp, wp)
        return m[:, :, 0]

    def teacher(x_lat, t):
        with torch.no_grad():
            xt = R.pack_latents(x_lat).bfloat16().float()
            pos = qwen_teacher_u(pe.float(), xt, t).bfloat16().float()
            neg = qwen_teacher_u(ne.float(), xt, t).bfloat16().float()
            return R.unpack_latents(pos + R.cfg_bias(pos, neg, 4.0), hp, wp)
    x, raw, total = x0.clone(), torch.ones(B), 0
    for step in range(2):
        m, lw, lg = D.qwen_forward(ws, cfg, x.bfloat16().float(), pe.float(), R.shift_sigma(raw), hp, wp)
        ml, lwl, lgl = R.unpack_mixture(rnd(m), rnd(lw), rnd(lg), hp, wp)
        u_drop, u_stu, u_tea = draws[step]
        mask = R.gm_dropout_mask(u_drop.reshape(B, 16, 1, 1, 1), 0.1)
        loss, x_dst, raw = R.segment_distill(teacher, R.unpack_latents(x, hp, wp), ml, lwl, lgl, raw, 0.5, 0.5, u_stu, u_tea, drop_mask=mask)
        total = total + loss * 0.5
        x = R.pack_latents(x_dst.detach())
    total.backward()
    assert abs(info['loss'] - total.item()) < 3e-2 * abs(total.item()) + 1e-4, (info['loss'], total.item())
    for sp in tr.specs:
        for got, ref in ((tr.A(sp, gsum).cpu(), leaves[sp.name][0].grad), (tr.B(sp, gsum).cpu(), leaves[sp.name][1].grad)):
            e = ((got - ref).norm() / ref.norm().clamp(min=1e-12)).item()
            assert e < 8e-2, (sp.name, e)


@pytest.mark.gpu
def test_qwen_fp8_teacher_true_cfg_step_is_baseline_configs4():
    """BASELINE.json configs[4] in its stated combination: Qwen-Image family x true-CFG teacher (negative prompt, scale 4.0:
    configs/qwen/arcqwen_2nfe_k16.py:100) x ``teacher_fp8`` (both teacher forwards of every state on the e4m3 MFMA; student forward,
    gradients and optimizer bf16 / fp32).  Stated tolerance: against the bf16-teacher step on the same draws the loss moves by < 6 %
    and the flat gradient by < 0.3 rel-L2 (CFG amplifies the teacher's quantisation noise by the guidance scale); against the fp32
    CPU oracle chain (LoRA folded in, same draws) the loss is within 8 %."""
    from arcflow_amd.train import ArcFlowDistiller, DistillConfig
    from oracle import arcflow_ref as R
    from oracle import dit_ref as D
    cfg = D.QwenCfg(num_layers=2, heads=2, joint_dim=192)
    w = D.make_qwen_weights(cfg, seed=21)
    g = torch.Generator().manual_seed(22)
    w['proj_out.weight'] = (torch.randn(64, 256, generator=g) * 0.05).bfloat16()
    w['proj_out.bias'] = (torch.randn(64, generator=g) * 0.02).bfloat16()
    B, hp, wp, T, r = 1, 8, 8, 64, 64
    pe = (torch.randn(B, T, 192, generator=g) * 0.5).bfloat16()
    ne = (torch.randn(B, T, 192, generator=g) * 0.5).bfloat16()
    x0 = torch.randn(B, hp * wp, 64, generator=g)
    draws = [(torch.rand(B, 16, generator=g), torch.rand(B, 4, generator=g), torch.rand(B, 3, generator=g)) for _ in range(2)]
    cond = dict(prompt_embeds=pe.cuda(), negative_prompt_embeds=ne.cuda(), hp=hp, wp=wp)
    Bs, res = None, {}
    for fp8 in (False, True):
        dc = DistillConfig(num_decay_iters=4, warmup_iters=0, grad_clip_begin_iter=10 ** 9, ema_start_iter=0, lora_rank=r,
                           teacher_guidance_scale=4.0, teacher_fp8=fp8)
        dist = ArcFlowDistiller('qwen', dict(num_double=2, heads=2, joint_dim=192), w, dc)
        tr = dist.trunk
        if Bs is None:
            Bs = {sp.name: (torch.randn(sp.out_f, r, generator=g) * 0.02) for sp in tr.specs}
        AB = {}
        for sp in tr.specs:
            tr.B(sp).copy_(Bs[sp.name].cuda())
            AB[sp.name] = (tr.A(sp).cpu().clone(), tr.B(sp).cpu().clone())
        tr.refresh()
        if fp8:
            assert dist.teacher._weights.get('d0.img_qkv.weight_q') is not None
        dist.iteration = 2
        info = dist.train_step(cond, B, x_init=x0.cuda(), draws=draws)
        res[fp8] = (info, dist.grads[0].clone(), dist.last_x.clone(), AB)
    (i16, g16, x16, AB), (i8, g8, x8, _) = res[False], res[True]
    assert not i8['skipped'] and i8['loss'] != i16['loss']                  # the fp8 teacher really ran
    assert abs(i8['loss'] - i16['loss']) < 6e-2 * abs(i16['loss']), (i8['loss'], i16['loss'])
    assert ((g8 - g16).norm() / g16.norm()).item() < 0.3
    assert ((x8 - x16).norm() / x16.norm()).item() < 4e-2
    # ---- fp32 CPU oracle, loss only ----------------------------------------------------------------------------------------
    wt = {k: v.float() for k, v in w.items()}
    ws = dict(wt)
    for name, (a, b) in AB.items():
        ws[name + '.weight'] = (wt[name + '.weight'] + b.bfloat16().float() @ a.bfloat16().float()).bfloat16().float()

    def teacher_u(ctx, x_tok, t):
        wv = dict(wt)
        wv['proj_out_means.weight'] = torch.cat([wt['proj_out.weight']] + [torch.zeros(64, 256)] * 15)
        wv['proj_out_means.bias'] = torch.cat([wt['proj_out.bias']] + [torch.zeros(64)] * 15)
        return D.qwen_forward(wv, cfg, x_tok, ctx, t, hp, wp)[0][:, :, 0]

    def teacher(x_lat, t):
        xt = R.pack_latents(x_lat).bfloat16().float()
        pos, neg = teacher_u(pe.float(), xt, t).bfloat16().float(), teacher_u(ne.float(), xt, t).bfloat16().float()
        return R.unpack_latents(pos + R.cfg_bias(pos, neg, 4.0), hp, wp)
    with torch.no_grad():
        x, raw, total = x0.clone(), torch.ones(B), 0.0
        for step in range(2):
            m, lw, lg = D.qwen_forward(ws, cfg, x.bfloat16().float(), pe.float(), R.shift_sigma(raw), hp, wp)
            ml, lwl, lgl = R.unpack_mixture(m.bfloat16().float(), lw.bfloat16().float(), lg.bfloat16().float(), hp, wp)
            u_drop, u_stu, u_tea = draws[step]
            mask = R.gm_dropout_mask(u_drop.reshape(B, 16, 1, 1, 1), 0.1)
            loss, x_dst, raw = R.segment_distill(teacher, R.unpack_latents(x, hp, wp), ml, lwl, lgl, raw, 0.5, 0.5, u_stu, u_tea, drop_mask=mask)
            total += float(loss) * 0.5
            x = R.pack_latents(x_dst)
    assert abs(i16['loss'] - total) < 3e-2 * abs(total) + 1e-4, (i16['loss'], total)
    assert abs(i8['loss'] - total) < 8e-2 * abs(total), (i8['loss'], total)


@pytest.mark.gpu
def test_lora_dropout_masks_and_kernel_modes():
    from arcflow_amd import ops
    g = torch.Generator().manual_seed(0)
    x = torch.randn(300, 256, generator=g).bfloat16().cuda()
    p, seed = 0.25, 1234567
    keep_scale = ops.lora_dropout(torch.ones_like(x), p, seed, row0=40, mode=1).float()
    vals = set(keep_scale.unique().tolist())
    assert vals == {0.0, float(torch.tensor(1 / (1 - p)).bfloat16())}
    frac = (keep_scale == 0).float().mean().item()
    assert abs(frac - p) < 0.01                                        # drop rate
    # the mask depends on (seed, global row, col) only: a row-shifted call sees the shifted mask
    part = ops.lora_dropout(torch.ones(100, 256, dtype=torch.bfloat16, device='cuda'), p, seed, row0=140, mode=1).float()
    assert torch.equal(part, keep_scale[100:200])
    assert not torch.equal(ops.lora_dropout(torch.ones_like(x), p, seed + 1, row0=40, mode=1).float(), keep_scale)
    d0 = ops.lora_dropout(x, p, seed, row0=40, mode=0).float()
    d1 = ops.lora_dropout(x, p, seed, row0=40, mode=1).float()
    exact = (keep_scale > 0).float() / (1 - p)                          # the read-back value is bf16-rounded
    assert torch.allclose(d1, (x.float() * exact).bfloat16().float()) and torch.allclose(d1 - d0, x.float(), atol=2e-2, rtol=2e-2)
    acc = x.clone()
    ops.lora_dropout(x, p, seed, row0=40, mode=2, out=acc)
    assert torch.allclose(acc.float(), (x.float() + d0).bfloat16().float(), atol=2e-2, rtol=2e-2)


@pytest.mark.gpu
def test_lora_dropout_train_step_matches_cpu_autograd():
    """peft lora_dropout on the adapters' input: staged student forward (engine conditioning -> trunk blocks with the
    B A (x . delta) correction -> engine head), recompute and backward, against autograd through the fp32 oracle with the
    LoRA branch applied to the SAME dropped inputs (masks read back from the kernel)."""
    from arcflow_amd import ops
    from arcflow_amd.train import ArcFlowDistiller, DistillConfig
    from oracle import arcflow_ref as R
    from oracle import dit_ref as D
    cfg, w = _setup()
    B, hp, wp, T, r, pdrop = 2, 8, 8, 64, 64, 0.25
    N, S = hp * wp, hp * wp + T
    g = torch.Generator().manual_seed(6)
    pe = (torch.randn(B, T, 128, generator=g) * 0.5).bfloat16()
    pooled = (torch.randn(B, 64, generator=g) * 0.5).bfloat16()
    x0 = torch.randn(B, N, 64, generator=g)
    draws = [(torch.rand(B, 16, generator=g), torch.rand(B, 4, generator=g), torch.rand(B, 3, generator=g)) for _ in range(2)]
    dc = DistillConfig(num_decay_iters=4, warmup_iters=0, grad_clip_begin_iter=10 ** 9, ema_start_iter=0, lora_rank=r, lora_dropout=pdrop)
    dist = ArcFlowDistiller('flux', dict(num_double=1, num_single=1, heads=2, joint_dim=128, pooled_dim=64), w, dc)
    tr = dist.trunk
    AB = {}
    for sp in tr.specs:
        tr.B(sp).copy_((torch.randn(sp.out_f, r, generator=g) * 0.05).cuda())       # a LoRA branch big enough to matter
        AB[sp.name] = (tr.A(sp).cpu().clone(), tr.B(sp).cpu().clone())
    tr.refresh()
    dist.iteration = 1
    seeds = [dist.dropout_seed(0), dist.dropout_seed(1)]
    cond = dict(prompt_embeds=pe.cuda(), pooled=pooled.cuda(), hp=hp, wp=wp)
    info = dist.train_step(cond, B, x_init=x0.cuda(), draws=draws)
    torch.cuda.synchronize()
    gsum = dist.grads[0]

    wt = {k: v.float() for k, v in w.items()}
    leaves = {sp.name: (AB[sp.name][0].bfloat16().float().requires_grad_(True), AB[sp.name][1].bfloat16().float().requires_grad_(True))
              for sp in tr.specs}
    gd = torch.full((B,), 3.5)

    def student_weights(step):
        ws = dict(wt)
        tr.seed = seeds[step]
        for sp in tr.specs:
            rows = B if 'time_text_embed' in sp.name else B * S        # the embedder's rows are the samples
            ks = ops.lora_dropout(torch.ones(rows, sp.in_f, dtype=torch.bfloat16, device='cuda'), pdrop, tr._site_seed(sp), 0, mode=1)
            ks = (ks.float().cpu() > 0).float() / (1 - pdrop)
            ks = ks if rows == B else ks.view(B, S, sp.in_f)
            if 'time_text_embed' in sp.name:
                pass
            elif 'ff_context' in sp.name:
                ks = ks[:, :T]
            elif 'transformer_blocks' in sp.name and 'single' not in sp.name:
                ks = ks[:, T:]
            ws[sp.name + '.lora'] = (leaves[sp.name][0], leaves[sp.name][1], ks)
        return ws

    def teacher(x_lat, t):
        with torch.no_grad():
            u = D.flux_teacher_forward(wt, cfg, R.pack_latents(x_lat).bfloat16().float(), pe.float(), pooled.float(), t, gd, hp, wp)
            return R.unpack_latents(u.bfloat16().float(), hp, wp)
    rnd = lambda t: t + (t.bfloat16().float() - t).detach()   # noqa: E731
    x, raw = x0.clone(), torch.ones(B)
    total = 0
    for step in range(2):
        m, lw, lg = D.flux_forward(student_weights(step), cfg, x.bfloat16().float(), pe.float(), pooled.float(), R.shift_sigma(raw), gd, hp, wp)
        ml, lwl, lgl = R.unpack_mixture(rnd(m), rnd(lw), rnd(lg), hp, wp)
        u_drop, u_stu, u_tea = draws[step]
        mask = R.gm_dropout_mask(u_drop.reshape(B, 16, 1, 1, 1), 0.1)
        loss, x_dst, raw = R.segment_distill(teacher, R.unpack_latents(x, hp, wp), ml, lwl, lgl, raw, 0.75, 0.5, u_stu, u_tea, drop_mask=mask)
        total = total + loss * 0.5
        x = R.pack_latents(x_dst.detach())
    total.backward()
    assert abs(info['loss'] - total.item()) < 3e-2 * abs(total.item()) + 1e-4, (info['loss'], total.item())
    for sp in tr.specs:
        ga, gb = tr.A(sp, gsum).cpu(), tr.B(sp, gsum).cpu()
        ra, rb = leaves[sp.name][0].grad, leaves[sp.name][1].grad
        ea = ((ga - ra).norm() / ra.norm()).item()
        eb = ((gb - rb).norm() / rb.norm()).item()
        assert ea < 8e-2 and eb < 8e-2, (sp.name, ea, eb)
    # and dropout really changed the result: the same step without it gives a different loss
    dist2 = ArcFlowDistiller('flux', dict(num_double=1, num_single=1, heads=2, joint_dim=128, pooled_dim=64), w,
                             DistillConfig(num_decay_iters=4, warmup_iters=0, grad_clip_begin_iter=10 ** 9, ema_start_iter=0, lora_rank=r))
    for sp in dist2.trunk.specs:
        dist2.trunk.A(sp).copy_(AB[sp.name][0].cuda())
        dist2.trunk.B(sp).copy_(AB[sp.name][1].cuda())
    dist2.trunk.refresh()
    dist2.iteration = 1
    info2 = dist2.train_step(cond, B, x_init=x0.cuda(), draws=draws)
    assert abs(info2['loss'] - info['loss']) > 1e-4 * abs(info['loss'])


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_student_fp8_forward_bf16_grads_step(family):
    """BASELINE.json configs[4] "fp8 MFMA fwd + bf16 grads" on the STUDENT: ``DistillConfig.student_fp8`` runs the block linears of the
    student forward and of the backward's recompute as e4m3 x e4m3 GEMMs (activations quantised per token, merged weights W + B A per
    output row, re-quantised after every optimizer step); dgrad and the LoRA gradients stay bf16 on the bf16 weights.  flux: with LoRA
    dropout (the reference config); qwen: together with the true-CFG fp8 teacher (configs[4] with every forward on fp8).
    Stated tolerance against the all-bf16 step on the same draws: loss within 8 %, flat gradient within 0.35 rel-L2 and cosine > 0.94
    (each e4m3 GEMM carries ~4e-2 of noise, which the K = 16 mixture heads and the CFG scale amplify), next state within 5e-2."""
    from arcflow_amd.train import ArcFlowDistiller, DistillConfig
    from oracle import dit_ref as D
    g = torch.Generator().manual_seed(31)
    r = 64
    if family == 'flux':
        cfg, w = _setup()
        B, hp, wp, T = 2, 8, 8, 64
        pe = (torch.randn(B, T, 128, generator=g) * 0.5).bfloat16()
        pooled = (torch.randn(B, 64, generator=g) * 0.5).bfloat16()
        cond = dict(prompt_embeds=pe.cuda(), pooled=pooled.cuda(), hp=hp, wp=wp)
        arch = dict(num_double=1, num_single=1, heads=2, joint_dim=128, pooled_dim=64)
        extra = dict(lora_dropout=0.05)
    else:
        cfg = D.QwenCfg(num_layers=2, heads=2, joint_dim=192)
        w = D.make_qwen_weights(cfg, seed=21)
        w['proj_out.weight'] = (torch.randn(64, 256, generator=g) * 0.05).bfloat16()
        w['proj_out.bias'] = (torch.randn(64, generator=g) * 0.02).bfloat16()
        B, hp, wp, T = 1, 8, 8, 64
        pe = (torch.randn(B, T, 192, generator=g) * 0.5).bfloat16()
        ne = (torch.randn(B, T, 192, generator=g) * 0.5).bfloat16()
        cond = dict(prompt_embeds=pe.cuda(), negative_prompt_embeds=ne.cuda(), hp=hp, wp=wp)
        arch = dict(num_double=2, heads=2, joint_dim=192)
        extra = dict(teacher_guidance_scale=4.0, teacher_fp8=True)
    x0 = torch.randn(B, hp * wp, 64, generator=g)
    draws = [(torch.rand(B, 16, generator=g), torch.rand(B, 4, generator=g), torch.rand(B, 3, generator=g)) for _ in range(2)]
    Bs, res = None, {}
    for fp8 in (False, True):
        dc = DistillConfig(num_decay_iters=4, warmup_iters=0, grad_clip_begin_iter=10 ** 9, ema_start_iter=0, lora_rank=r, student_fp8=fp8, **extra)
        dist = ArcFlowDistiller(family, arch, w, dc)
        tr = dist.trunk
        assert tr.fp8 == fp8
        if Bs is None:
            Bs = {sp.name: (torch.randn(sp.out_f, r, generator=g) * 0.02) for sp in tr.specs}
        for sp in tr.specs:
            tr.B(sp).copy_(Bs[sp.name].cuda())
        tr.refresh()
        if fp8:     # every block linear's FROZEN weight is quantised once (the LoRA branch stays a bf16 rank-r product); shared with the fp8 teacher when it has them
            key = tr.specs[0].packed_key
            q, sc = tr.wq[key]
            wm = tr.packed[key + '.weight'].float()
            deq = _e4m3_to_float(q) * sc[:, None]
            assert ((deq - wm).norm() / wm.norm()).item() < 4e-2
            if family == 'qwen':
                assert tr.wq['d0.img_qkv'][0].data_ptr() == dist.teacher._weights['d0.img_qkv.weight_q'].data_ptr()
        dist.iteration = 2
        info = dist.train_step(cond, B, x_init=x0.cuda(), draws=draws)
        assert not info['skipped']
        res[fp8] = (info['loss'], dist.grads[0].clone(), dist.last_x.clone())
        # an optimizer step leaves the quantised frozen weights alone
        if fp8:
            q2, sc2 = tr.wq[key]
            wm2 = tr.packed[key + '.weight'].float()
            assert ((_e4m3_to_float(q2) * sc2[:, None] - wm2).norm() / wm2.norm()).item() < 4e-2
    (l16, g16, x16), (l8, g8, x8) = res[False], res[True]
    assert l8 != l16                                                     # the fp8 path really ran
    assert abs(l8 - l16) < 8e-2 * abs(l16), (l8, l16)
    rel = ((g8 - g16).norm() / g16.norm()).item()
    cos = (torch.dot(g8, g16) / (g8.norm() * g16.norm())).item()
    assert rel < 0.35 and cos > 0.94, (rel, cos)
    assert ((x8 - x16).norm() / x16.norm()).item() < 5e-2


def _e4m3_to_float(q):
    """OCP e4m3 (uint8) -> fp32 (bias 7, no infinities, 0x7f / 0xff = NaN)."""
    q = q.to(torch.int32)
    s = torch.where((q & 0x80) != 0, -1.0, 1.0)
    e = (q >> 3) & 0xF
    m = (q & 7).float()
    v = torch.where(e == 0, m / 8.0 * 2.0 ** -6, (1.0 + m / 8.0) * torch.pow(2.0, (e - 7).float()))
    return (s * v).to(torch.float32)


_RCCL_ONE_RANK = r'''
import os, sys, torch
sys.path.insert(0, os.getcwd())
import torch.distributed as dist
os.environ['MASTER_ADDR'] = '127.0.0.1'
os.environ.setdefault('MASTER_PORT', '29731')
os.environ['ARCFLOW_DP_FORCE_COLLECTIVES'] = '1'
torch.cuda.set_device(0)
dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
from tests.test_distill import _setup
from arcflow_amd.train import ArcFlowDistiller, DistillConfig
cfg, w = _setup()
B, hp, wp, T = 2, 8, 8, 64
g = torch.Generator().manual_seed(3)
pe = (torch.randn(B, T, 128, generator=g) * 0.5).bfloat16()
pooled = (torch.randn(B, 64, generator=g) * 0.5).bfloat16()
x0 = torch.randn(B, hp * wp, 64, generator=g)
draws = [(torch.rand(B, 16, generator=g), torch.rand(B, 4, generator=g), torch.rand(B, 3, generator=g)) for _ in range(2)]
cond = dict(prompt_embeds=pe.cuda(), pooled=pooled.cuda(), hp=hp, wp=wp)
out = {}
for force in ('1', '0'):
    os.environ['ARCFLOW_DP_FORCE_COLLECTIVES'] = force
    dc = DistillConfig(num_decay_iters=4, warmup_iters=0, grad_clip_begin_iter=10 ** 9, ema_start_iter=0, lora_rank=64)
    d = ArcFlowDistiller('flux', dict(num_double=1, num_single=1, heads=2, joint_dim=128, pooled_dim=64), w, dc)
    assert d.reducer.backend == 'nccl' and d.reducer._skip_single == (force == '0')
    d.iteration = 1
    info = d.train_step(cond, B, x_init=x0.cuda(), draws=draws)
    torch.cuda.synchronize()
    d.reducer.check_consistent(d.params)
    out[force] = (info['loss'], d.params.clone(), info['allreduce_bytes'] if 'allreduce_bytes' in info else None, info.get('allreduce_exposed_ms'))
dp = (out['1'][1] - out['0'][1]).abs().max().item()
# (not bit-identical: the loss and the column sums are accumulated with float atomics, 1e-8 run to run)
assert abs(out['1'][0] - out['0'][0]) <= 1e-6 * abs(out['0'][0]) and dp <= 1e-6, ('a one-rank SUM all-reduce must change nothing', out['1'][0], out['0'][0], dp)
print('RCCL_ONE_RANK_OK', out['1'][0], out['1'][2], out['1'][3])
dist.destroy_process_group()
'''


@pytest.mark.gpu
def test_rccl_branch_of_the_exchange_executes_on_one_rank(tmp_path):
    """The 'nccl' (= RCCL) branch of GradReducer -- async all-reduce handles on device tensors, the compute stream's wait, the exposed-time
    events, the construction broadcast and the checksum all-reduces -- has only ever run as 'gloo' in the tests (two ranks cannot share one
    GPU under RCCL).  A one-rank nccl group with ARCFLOW_DP_FORCE_COLLECTIVES=1 executes every one of those calls on this single-GPU box;
    a one-rank SUM changes nothing, so the step must equal the run that skips the collectives (to the 1e-8 of the float atomics)."""
    import subprocess
    import sys
    script = tmp_path / 'rccl_one_rank.py'
    script.write_text(_RCCL_ONE_RANK)
    env = dict(os.environ, MASTER_PORT=str(29500 + os.getpid() % 400))
    r = subprocess.run([sys.executable, str(script)], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'RCCL_ONE_RANK_OK' in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


_RCCL_FULL_SIZE = r'''
import os, sys, torch
sys.path.insert(0, os.getcwd())
import torch.distributed as dist
os.environ['MASTER_ADDR'] = '127.0.0.1'
os.environ.setdefault('MASTER_PORT', '29733')
os.environ['ARCFLOW_DP_FORCE_COLLECTIVES'] = '1'
torch.cuda.set_device(0)
dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))
from arcflow_amd.train.trunk import lora_targets
from arcflow_amd.train.reducer import GradReducer
# the FLUX-12B trainable set exactly as ArcFlowDistiller lays it out (distill.py: [head.weight | head.bias | norm_out.weight | norm_out.bias | adapters, block-major])
D, nd, ns, r, head_n = 3072, 19, 38, 256, 1152
base = head_n * D + head_n + 2 * D * D + 2 * D
spans, off = {}, base
for name, key, row0, out_f, in_f in lora_targets('flux', nd, ns, D):
    blk = key.split('.')[0]
    a, b = spans.get(blk, (off, off))
    spans[blk] = (min(a, off), off + r * in_f + out_f * r)
    off += r * in_f + out_f * r
n = off
assert n == 652_418_176, n        # 652.4 M fp32 parameters (DESIGN section 6)
grad = torch.ones(n, dtype=torch.float32, device='cuda')
red = GradReducer()
assert red.backend == 'nccl' and not red._skip_single
# one iteration's exchange: the blocks' slices in backward order (single blocks first, then double), then everything else as one message
launched = []
busy = torch.randn(8192, 8192, device='cuda')
for blk in [f's{i}' for i in reversed(range(ns))] + [f'd{i}' for i in reversed(range(nd))]:
    a, b = spans[blk]
    red.launch(grad[a:b]); launched.append((a, b))
    busy = busy @ busy * 1e-4                      # the remaining blocks' backward the exchange hides under
pos, rest = 0, 0
for a, b in sorted(launched):
    if a > pos:
        red.launch(grad[pos:a]); rest += 1
    pos = max(pos, b)
if pos < n:
    red.launch(grad[pos:]); rest += 1
msgs = len(launched) + rest
assert len(launched) == nd + ns == 57 and rest >= 1
assert red.bytes_launched == 4 * n, (red.bytes_launched, 4 * n)          # every byte of the trainable set exactly once
sizes_mb = sorted((b - a) * 4 / 2**20 for a, b in launched)
inv = red.finish()
ms = red.exposed_ms()
torch.cuda.synchronize()
assert inv == 1.0 and ms >= 0.0 and red.last_exposed_ms == ms
assert bool((grad == 1.0).all())                                          # a one-rank SUM changes nothing
print('RCCL_FULL_SIZE_OK', n, msgs, f'{4 * n / 2**30:.2f} GiB', f'block slices {sizes_mb[0]:.0f}-{sizes_mb[-1]:.0f} MiB', f'exposed {ms:.2f} ms')
dist.destroy_process_group()
'''


@pytest.mark.gpu
def test_rccl_exchange_at_the_production_slice_sizes_on_one_rank(tmp_path):
    """no multi-GPU node has been available, so the first 8-GPU line must explain itself.  The RCCL branch of the reducer with
    the REAL message sizes of a FLUX-12B iteration -- 57 per-block adapter slices in backward order + the rest (heads, norm_out, timestep-embedder
    pair) as one message, 2.4 GiB of fp32 gradients -- on a one-rank nccl group: every byte launched exactly once
    (bytes_launched == 4 x trainable parameters), async handles waited on the compute stream, an exposed-time event pair produced."""
    import subprocess
    import sys
    script = tmp_path / 'rccl_full_size.py'
    script.write_text(_RCCL_FULL_SIZE)
    env = dict(os.environ, MASTER_PORT=str(29900 + os.getpid() % 90))
    r = subprocess.run([sys.executable, str(script)], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'RCCL_FULL_SIZE_OK' in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    print(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_unmerged_trunk_forward_matches_merged_engine():
    """the reference keeps LoRA un-fused at inference (base GEMM + two rank-r GEMMs per adapted linear); the
    inference engine folds W + B A once.  The training trunk evaluates the un-fused form (y = [x | x A^T] [W | B]^T), so the two can be
    compared on one device with the live adapters: deviation of the folded forward from the un-fused one, and of both from the fp32
    oracle with the LoRA branch evaluated separately (peft's op order)."""
    from arcflow_amd.train import ArcFlowDistiller, DistillConfig
    from oracle import dit_ref as D
    cfg, w = _setup()
    B, hp, wp, T, r = 2, 8, 8, 64, 64
    g = torch.Generator().manual_seed(77)
    pe = (torch.randn(B, T, 128, generator=g) * 0.5).bfloat16()
    pooled = (torch.randn(B, 64, generator=g) * 0.5).bfloat16()
    x = torch.randn(B, hp * wp, 64, generator=g)
    dc = DistillConfig(num_decay_iters=4, warmup_iters=0, grad_clip_begin_iter=10 ** 9, ema_start_iter=0, lora_rank=r)
    d = ArcFlowDistiller('flux', dict(num_double=1, num_single=1, heads=2, joint_dim=128, pooled_dim=64), w, dc)
    tr = d.trunk
    for sp in tr.specs:                                   # adapters of the size a trained checkpoint has, not the B = 0 initialisation
        tr.B(sp).copy_((torch.randn(sp.out_f, r, generator=g) * 0.05).cuda())
    tr.refresh()
    cond = dict(prompt_embeds=pe.cuda(), pooled=pooled.cuda(), hp=hp, wp=wp)
    sigma = torch.tensor([0.7619, 0.7619], device='cuda')
    un, _ = d.student_forward_unmerged(x.cuda(), sigma, cond, 0.0, 0)
    un = [t.float().cpu() for t in (un.means, un.logweights, un.loggammas)]
    tr.bind_merged()
    mg = d.student.forward(x.cuda().bfloat16(), sigma, cond['prompt_embeds'], cond['pooled'], torch.full((B,), 3.5, device='cuda'), hp, wp)
    mg = [t.float().cpu() for t in (mg.means, mg.logweights, mg.loggammas)]
    # fp32 oracle, LoRA as a separate branch (dit_ref.lin's '.lora' entry = peft's forward)
    wl = {k: v.float() for k, v in w.items()}
    for sp in tr.specs:
        wl[sp.name + '.lora'] = (tr.A(sp).cpu().bfloat16().float(), tr.B(sp).cpu().bfloat16().float(), 1.0)
    ref = D.flux_forward(wl, cfg, x.bfloat16().float(), pe.float(), pooled.float(), sigma.cpu(), torch.full((B,), 3.5), hp, wp)
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()          # noqa: E731
    dev_means, dev_logg = rel(mg[0], un[0]), rel(mg[2], un[2])
    assert dev_means < 1.5e-2 and dev_logg < 1.5e-2, (dev_means, dev_logg)           # folded vs un-fused: bf16 rounding of W + B A
    for got in (un, mg):
        assert rel(got[0], ref[0]) < 2.5e-2 and rel(got[2], ref[2]) < 2.5e-2 and (got[1] - ref[1]).abs().max().item() < 0.1
    # a forward of the student ENGINE must never silently run the un-adapted trunk.  Changing the adapters marks the bound weights stale,
    # and student_forward() re-merges before it runs; the engine evaluated WITHOUT the re-merge is the stale W + B_old A.
    assert not tr._merged_dirty
    for sp in tr.specs:
        tr.B(sp).mul_(-1.0)
    tr.refresh()
    assert tr._merged_dirty
    stale = d.student.forward(x.cuda().bfloat16(), sigma, cond['prompt_embeds'], cond['pooled'], torch.full((B,), 3.5, device='cuda'), hp, wp).means.float().cpu()
    fresh = d.student_forward(x.cuda(), sigma, cond).means.float().cpu()
    assert not tr._merged_dirty
    un2, _ = d.student_forward_unmerged(x.cuda(), sigma, cond, 0.0, 0)
    assert rel(fresh, un2.means.float().cpu()) < 1.5e-2
    assert rel(stale, un2.means.float().cpu()) > 5e-2        # what the unguarded call would have returned


@pytest.mark.gpu
@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_kept_forward_outputs_equal_recompute(family):
    """The backward reads the training forward's GEMM / attention outputs back from the stash (288 GB HBM) instead of recomputing every block
    from its checkpoint as the reference does (arcflux.py:181-189).  Same kernels, same operands: loss, roll-out and every gradient of an iteration
    must be IDENTICAL to the recompute path's (`trunk.use_stash = False`, ARCFLOW_TRAIN_RECOMPUTE=1).  All three levels run: the stash with the
    adapters' dropped inputs, the stash without them (`trunk.keep_xd = False`: the fall-back when HBM is short) and recompute."""
    from arcflow_amd.train import ArcFlowDistiller, DistillConfig
    from oracle import dit_ref as D
    g = torch.Generator().manual_seed(41)
    r = 64
    if family == 'flux':
        cfg, w = _setup()
        B, hp, wp, T = 2, 8, 8, 64
        cond = dict(prompt_embeds=(torch.randn(B, T, 128, generator=g) * 0.5).bfloat16().cuda(),
                    pooled=(torch.randn(B, 64, generator=g) * 0.5).bfloat16().cuda(), hp=hp, wp=wp)
        arch, extra = dict(num_double=1, num_single=1, heads=2, joint_dim=128, pooled_dim=64), dict(lora_dropout=0.05)
    else:
        cfg = D.QwenCfg(num_layers=2, heads=2, joint_dim=192)
        w = D.make_qwen_weights(cfg, seed=21)
        w['proj_out.weight'] = (torch.randn(64, 256, generator=g) * 0.05).bfloat16()
        w['proj_out.bias'] = (torch.randn(64, generator=g) * 0.02).bfloat16()
        B, hp, wp, T = 1, 8, 8, 45                       # ragged joint length: 64 + 45 tokens
        cond = dict(prompt_embeds=(torch.randn(B, T, 192, generator=g) * 0.5).bfloat16().cuda(),
                    negative_prompt_embeds=(torch.randn(B, T, 192, generator=g) * 0.5).bfloat16().cuda(), hp=hp, wp=wp)
        arch, extra = dict(num_double=2, heads=2, joint_dim=192), dict(teacher_guidance_scale=4.0, lora_dropout=0.05)
    x0 = torch.randn(B, hp * wp, 64, generator=g)
    draws = [(torch.rand(B, 16, generator=g), torch.rand(B, 4, generator=g), torch.rand(B, 3, generator=g)) for _ in range(2)]
    Bs, res = None, {}
    for level in ('full', 'outputs', 'recompute'):
        stash = level != 'recompute'
        dc = DistillConfig(num_decay_iters=4, warmup_iters=0, grad_clip_begin_iter=10 ** 9, ema_start_iter=0, lora_rank=r, **extra)
        dist = ArcFlowDistiller(family, arch, w, dc)
        tr = dist.trunk
        tr.use_stash = stash
        if level == 'outputs':
            tr.keep_xd = False
        if Bs is None:
            Bs = {sp.name: (torch.randn(sp.out_f, r, generator=g) * 0.02) for sp in tr.specs}
        for sp in tr.specs:
            tr.B(sp).copy_(Bs[sp.name].cuda())
        tr.refresh()
        dist.iteration = 2
        info = dist.train_step(cond, B, x_init=x0.cuda(), draws=draws)
        assert (tr.stash is not None) == stash
        if stash:       # the allocation and the byte count come from one table
            assert tr.stash.keep_xd == (level == 'full')
            assert sum(t.numel() * t.element_size() for t in tr.stash.buf.values()) == tr.stash_bytes(tr.stash.rows)
        res[level] = (info['loss'], dist.grads[0].clone(), dist.last_x.clone(), dist.params.clone())
    # outputs only vs full: the same kernels on the same stored values (the dropout mask is a pure function of (seed, site, row, column), X1 / Pre
    # come from the stash) -- only the order of the float atomics may differ, the bound of test_text_side_stream_equals_one_stream.
    # Measured on the code before the block walk was split by mode: 1.8e-9 (flux) and 3.3e-10 (qwen), beside 1.9e-9 / 3.5e-10 between two full-level runs.
    (lf, gf, _, _), (lm, gm, _, _) = res['full'], res['outputs']
    rel_levels = ((gm - gf).norm() / gf.norm()).item()
    print('outputs-only stash vs full stash: gradient rel-L2', rel_levels, 'loss', lm, lf)
    assert abs(lm - lf) < 1e-5 * abs(lf) and rel_levels < 1e-6, (lm, lf, rel_levels)
    for kept in ('full', 'outputs'):
        _check_kept_against_recompute(res[kept], res['recompute'])


def _check_kept_against_recompute(kept, recomputed):
    (l1, g1, x1, p1), (l0, g0, x0_, p0) = kept, recomputed
    # the FORWARD is the same code in both modes: loss and roll-out agree to the order of the loss kernel's float atomics
    assert abs(l1 - l0) < 1e-5 * abs(l0) and ((x1 - x0_).norm() / x0_.norm()).item() < 1e-6
    assert g0.abs().max().item() > 0
    # the BACKWARD differs by design in one rounding: the recompute path forms X1 = X + gate . (O W^T) in the GEMM epilogue (fp32, one rounding),
    # the training forward rounds the branch output to bf16 first (it is kept for the gate gradient) -- the stash hands the backward the values the
    # forward really produced, the recompute path a bf16-ulp-different copy.  Gradients agree to that level.
    rel = ((g1 - g0).norm() / g0.norm()).item()
    print('stash vs recompute: gradient rel-L2', rel)
    assert rel < 5e-3, rel
    assert ((p1 - p0).abs().max() / p0.abs().max()).item() < 1e-3          # (AdamW turns a sign flip of a near-zero gradient into a 2 lr step)


@pytest.mark.gpu
def test_text_side_stream_equals_one_stream():
    """The text stream of a double block runs on a side HIP stream beside the image stream (train/trunk.py `_streams`) and the adapters'
    weight-gradient products on a third one (`_adapted_backward`).  Same iteration
    with and without it, while a third stream keeps the chip busy (the interleaving that exposed a scratch tensor shared by the two
    streams when this was built): gradients agree to the order of the float atomics."""
    from arcflow_amd.train import ArcFlowDistiller, DistillConfig
    cfg, w = _setup()
    B, hp, wp, T, r = 2, 8, 8, 64, 64
    g = torch.Generator().manual_seed(15)
    pe = (torch.randn(B, T, 128, generator=g) * 0.5).bfloat16().cuda()
    pooled = (torch.randn(B, 64, generator=g) * 0.5).bfloat16().cuda()
    x0 = torch.randn(B, hp * wp, 64, generator=g).cuda()
    draws = [(torch.rand(B, 16, generator=g), torch.rand(B, 4, generator=g), torch.rand(B, 3, generator=g)) for _ in range(2)]
    dc = DistillConfig(num_decay_iters=4, warmup_iters=0, grad_clip_begin_iter=10 ** 9, ema_start_iter=0, lora_rank=r)
    Bm = {}
    noise_stream, junk = torch.cuda.Stream(), torch.randn(1 << 22, device='cuda')

    def run(side):
        d = ArcFlowDistiller('flux', dict(num_double=1, num_single=1, heads=2, joint_dim=128, pooled_dim=64), w, dc)
        for sp in d.trunk.specs:
            if sp.name not in Bm:
                Bm[sp.name] = (torch.randn(sp.out_f, r, generator=g) * 0.02).cuda()
            d.trunk.B(sp).copy_(Bm[sp.name])
        d.trunk.refresh()
        assert d.trunk.side is not None and d.trunk.aux is not None         # the defaults
        if not side:
            d.trunk.side = d.trunk.aux = None
        d.iteration = 1
        with torch.cuda.stream(noise_stream):
            for _ in range(200):
                junk.mul_(1.0001)
        info = d.train_step(dict(prompt_embeds=pe, pooled=pooled, hp=hp, wp=wp), B, x_init=x0, draws=draws)
        torch.cuda.synchronize()
        return d.grad.clone(), info['loss']

    ref, loss_ref = run(False)
    assert ref.abs().max().item() > 0
    for _ in range(4):
        got, loss = run(True)
        assert ((got - ref).norm() / ref.norm()).item() < 1e-6
        assert abs(loss - loss_ref) <= 1e-6 * abs(loss_ref)
