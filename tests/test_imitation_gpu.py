"""Data-based distillation (``ArcFlowImitation``) on the GPU: the patchify + pack + forward-diffusion kernel against fp64 per
element, its argument checks, and the data-mode ``train_step`` against CPU autograd (tests/imitation_ref.py), against the
data-free path it shares its segment code with, and across micro-batches."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(3, 16, 16, 16), (2, 16, 6, 10), (1, 16, 128, 128)]      # square / hp != wp with 15 tokens (no multiple of a wave) / 1024^2
GUARD = 4                                                          # sentinel token rows in front of and behind both outputs
SENTINEL = -768.0                                                  # exact in bf16 too


def _sigma_sets(B):
    """Per-sample sigmas that include 1 (pure noise), warp(eps) (the lower clamp of sample_t) and an interior value."""
    from oracle import arcflow_ref as R
    vals = [1.0, float(R.shift_sigma(torch.tensor(1e-4))), 0.37]
    return [torch.tensor([vals[(r + i) % 3] for i in range(B)], dtype=torch.float32) for r in range(3 if B < 3 else 1)]


def _launch(x0, noise, sigma, want_bf16=True):
    """The C entry on guarded buffers -> (rc, xt fp32 [B,N,64], xt bf16 or None, guards untouched)."""
    from arcflow_amd import _lib
    lib = _lib.load()
    B, Cc, H, W = x0.shape
    N = (H // 2) * (W // 2)
    f32 = torch.full((B * N + 2 * GUARD, 64), SENTINEL, device='cuda')
    b16 = torch.full((B * N + 2 * GUARD, 64), SENTINEL, device='cuda', dtype=torch.bfloat16)
    p = lambda t: C.c_void_p(t.data_ptr())         # noqa: E731
    rc = lib.afx_forward_diffuse_pack(p(x0), p(noise), p(sigma), p(f32[GUARD:]), p(b16[GUARD:]) if want_bf16 else None,
                                      B, Cc, H, W, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    guards_ok = all(bool((t[:GUARD] == SENTINEL).all()) and bool((t[-GUARD:] == SENTINEL).all()) for t in (f32, b16))
    if not want_bf16:
        guards_ok = guards_ok and bool((b16 == SENTINEL).all())
    return rc, f32[GUARD:-GUARD].view(B, N, 64), (b16[GUARD:-GUARD].view(B, N, 64) if want_bf16 else None), guards_ok


def _within(got, x0d_tok, noise_d, sigma):
    """|got - ref| <= 4 x 2^-24 x (|x0 (1 - sigma)| + |noise sigma|): four half-ulp fp32 roundings (1 - sigma, two products, one sum),
    doubled to allow either FMA contraction.  -> (all inside, worst err / bound)."""
    s = sigma.double().reshape(-1, 1, 1)
    a, b = x0d_tok * (1 - s), noise_d * s
    bound = 4 * 2.0 ** -24 * (a.abs() + b.abs())
    err = (got.double() - (a + b)).abs()
    return bool((err <= bound).all()), (err / bound.clamp(min=1e-300)).max().item()


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_forward_diffuse_pack_against_fp64(shape):
    from arcflow_amd import ops
    from oracle import arcflow_ref as R
    B, Cc, H, W = shape
    hp, wp = H // 2, W // 2
    g = torch.Generator().manual_seed(H * 1000 + W)
    x0 = torch.randn(B, Cc, H, W, generator=g) * 1.7
    noise = torch.randn(B, hp * wp, 4 * Cc, generator=g)
    x0d_tok = R.pack_latents(R.patchify(x0.double()), patch=1)
    assert torch.equal(x0d_tok, R.pack_latents(x0.double()))           # one-pixel tokens of the folded latent = the engine's 2x2 pack
    x0g, ng = x0.cuda(), noise.cuda()
    for sigma in _sigma_sets(B):
        rc, xt, xt16, guards = _launch(x0g, ng, sigma.cuda())
        assert rc == 0 and guards
        ok, worst = _within(xt.cpu(), x0d_tok, noise.double(), sigma)
        print(shape, sigma.tolist(), 'worst err / bound', worst)
        assert ok, worst
        assert torch.equal(xt16.view(torch.int16), xt.bfloat16().view(torch.int16))
        # the same check must tell a transposed grid and a neighbour's sigma apart
        if bool((sigma != 1).any()):               # (at sigma = 1 the latent has no weight: nothing to tell apart)
            assert not _within(xt.cpu(), R.pack_latents(x0.double().transpose(2, 3).contiguous()), noise.double(), sigma)[0]
        if B > 1:
            assert not _within(xt.cpu(), x0d_tok, noise.double(), sigma.roll(1))[0]
    # sigma = 0: the layout alone, exactly; without the bf16 output nothing is written there
    rc, xt, none16, guards = _launch(x0g, ng, torch.zeros(B, device='cuda'), want_bf16=False)
    assert rc == 0 and guards and none16 is None
    assert torch.equal(xt.cpu(), R.pack_latents(R.patchify(x0), patch=1))
    # the Python op: same numbers, optional bf16, GPU tensors only
    sigma = _sigma_sets(B)[0]
    y, y16 = ops.forward_diffuse_pack(x0g, ng, sigma.cuda())
    assert torch.equal(y, _launch(x0g, ng, sigma.cuda())[1]) and torch.equal(y16, y.bfloat16())
    assert ops.forward_diffuse_pack(x0g, ng, sigma.cuda(), want_bf16=False)[1] is None
    with pytest.raises(Exception, match='GPU tensors only'):
        ops.forward_diffuse_pack(x0, noise, sigma)


def test_forward_diffuse_pack_refuses_bad_arguments():
    from arcflow_amd import _lib
    lib = _lib.load()
    x0 = torch.randn(2, 16, 6, 10, device='cuda')
    noise = torch.randn(2, 15, 64, device='cuda')
    sigma = torch.tensor([0.3, 0.8], device='cuda')
    out = torch.full((2, 15, 64), SENTINEL, device='cuda')
    out16 = torch.full((2, 15, 64), SENTINEL, device='cuda', dtype=torch.bfloat16)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())        # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(a=x0, n=noise, s=sigma, o=out, o16=out16, dims=(2, 16, 6, 10)):
        return lib.afx_forward_diffuse_pack(p(a), p(n), p(s), p(o), p(o16), *dims, st)
    for kw in (dict(dims=(2, 16, 5, 10)), dict(dims=(2, 16, 6, 9)), dict(dims=(2, 8, 6, 10)), dict(dims=(2, 32, 6, 10)),
               dict(a=None), dict(n=None), dict(s=None), dict(o=None)):
        assert call(**kw) != 0, kw
        assert b'afx_forward_diffuse_pack' in lib.afx_last_error()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((out16 == SENTINEL).all())          # a refused call writes nothing
    assert call(o16=None) == 0 and call() == 0                                         # the bf16 output is optional
    torch.cuda.synchronize()
    assert torch.equal(out16, out.bfloat16()) and bool((out != SENTINEL).all())
    from arcflow_amd import ops
    with pytest.raises(ValueError):
        ops.forward_diffuse_pack(torch.randn(2, 16, 5, 10, device='cuda'), noise, sigma)
    with pytest.raises(ValueError):
        ops.forward_diffuse_pack(x0, noise.view(2, 64, 15), sigma)


def _toy():
    from arcflow_amd.weights import init_arcflow_heads_from_teacher
    from oracle import dit_ref as D
    cfg = D.FluxCfg(num_layers=1, num_single_layers=1, heads=2, joint_dim=128, pooled_dim=64)
    w = D.make_flux_weights(cfg, seed=7, teacher_head=True)
    for k in [k for k in w if k.startswith('proj_out_')]:
        del w[k]
    w = init_arcflow_heads_from_teacher(w, generator=torch.Generator().manual_seed(1))
    g = torch.Generator().manual_seed(2)          # non-trivial log-weights / rates so every gradient path is exercised
    w['proj_out_logweights.weight'] = (torch.randn(64, 256, generator=g) * 0.05).bfloat16()
    w['proj_out_loggamma.weight'] = (torch.randn(60, 256, generator=g) * 0.05).bfloat16()
    return cfg, w


ENG = dict(num_double=1, num_single=1, heads=2, joint_dim=128, pooled_dim=64)


def _inputs(B, hp, wp, T, seed):
    g = torch.Generator().manual_seed(seed)
    pe = (torch.randn(B, T, 128, generator=g) * 0.5).bfloat16()
    pooled = (torch.randn(B, 64, generator=g) * 0.5).bfloat16()
    x0 = torch.randn(B, 16, 2 * hp, 2 * wp, generator=g)
    noise = torch.randn(B, hp * wp, 64, generator=g)
    draws = [(torch.rand(B, 16, generator=g), torch.rand(B, 4, generator=g), torch.rand(B, 3, generator=g))]
    return pe, pooled, x0, noise, draws


def rel_l2(a, b):
    return ((a - b).norm() / b.norm().clamp(min=1e-12)).item()


def test_data_mode_step_matches_cpu_autograd():
    """Three samples on three different source indices (nfe 3, timestep_ratio 0.5: two segment sizes, a different sigma per sample in
    ONE student forward) against autograd through the CPU restatement; bounds of test_distill.py::test_train_step_matches_cpu_autograd."""
    from arcflow_amd.train import ArcFlowDistiller, DistillConfig
    from oracle import arcflow_ref as R
    from oracle import dit_ref as D
    from tests import imitation_ref as IR
    cfg, w = _toy()
    B, hp, wp, T = 3, 8, 8, 12
    pe, pooled, x0, noise, draws = _inputs(B, hp, wp, T, seed=5)
    u = torch.tensor([0.9, 0.5, 0.1])
    assert IR.sample_t(u, 3, 0.5)[3].tolist() == [1, 2, 3]
    dc = DistillConfig(mode='data', nfe=3, timestep_ratio=0.5, num_decay_iters=4, warmup_iters=0, grad_clip_begin_iter=0, ema_start_iter=0)
    dist = ArcFlowDistiller('flux', ENG, w, dc)
    dist.iteration = 1                       # teacher_ratio = 0.75: both student and teacher intervals active
    p_before = dist.params.clone()
    cond = dict(prompt_embeds=pe.cuda(), pooled=pooled.cuda(), hp=hp, wp=wp)
    info = dist.train_step(cond, B, x0=x0.cuda(), t_draws=u, noise=noise.cuda(), draws=draws)
    torch.cuda.synchronize()

    names = ['proj_out_means', 'proj_out_logweights', 'proj_out_loggamma', 'norm_out.linear']
    wt = {k: v.float() for k, v in w.items()}
    leaves = {nm + s: wt[nm + s].clone().requires_grad_(True) for nm in names for s in ('.weight', '.bias')}
    ws = dict(wt)
    ws.update(leaves)
    gd = torch.full((B,), 3.5)
    rnd = lambda t: t + (t.bfloat16().float() - t).detach()   # noqa: E731  (the engine hands bf16 outputs to the policy math)

    def teacher(x_lat, t, b):
        with torch.no_grad():
            u_ = D.flux_teacher_forward(wt, cfg, R.pack_latents(x_lat).bfloat16().float(), pe[b:b + 1].float(), pooled[b:b + 1].float(),
                                        t, gd[:1], hp, wp)
            return R.unpack_latents(u_.bfloat16().float(), hp, wp)

    def policy(x_t, sigma):
        m, lw, lg = D.flux_forward(ws, cfg, R.pack_latents(x_t).bfloat16().float(), pe.float(), pooled.float(), sigma, gd, hp, wp)
        return R.unpack_mixture(rnd(m), rnd(lw), rnd(lg), hp, wp)

    trace = {}
    u_drop, u_stu, u_tea = draws[0]
    loss = IR.imitation_step(teacher, policy, x0, R.unpack_latents(noise, hp, wp), u, 0.75, u_drop.reshape(B, 16, 1, 1, 1), u_stu, u_tea,
                             nfe=3, timestep_ratio=0.5, trace=trace)
    loss.backward()
    print('loss', info['loss'], loss.item())
    assert abs(info['loss'] - loss.item()) < 2e-2 * abs(loss.item()) + 1e-4, (info['loss'], loss.item())
    x_t = R.pack_latents(trace['x_t_src'])
    assert rel_l2(dist.last_x.cpu(), x_t) < 1e-6                     # the start state: x0 noised to each sample's own segment start
    gsum = dist.grads[0]
    Dm = 256
    hw = gsum[:1152 * Dm].view(1152, Dm).cpu()
    hb = gsum[1152 * Dm:1152 * Dm + 1152].cpu()
    ref_hw = torch.cat([leaves[n + '.weight'].grad for n in names[:3]])
    ref_hb = torch.cat([leaves[n + '.bias'].grad for n in names[:3]])
    off = 1152 * Dm + 1152
    nw = gsum[off:off + 2 * Dm * Dm].view(2 * Dm, Dm).cpu()
    nb = gsum[off + 2 * Dm * Dm:].cpu()
    rels = dict(head_w=rel_l2(hw[:1148], ref_hw), head_b=rel_l2(hb[:1148], ref_hb),
                norm_out_w=rel_l2(nw, leaves['norm_out.linear.weight'].grad), norm_out_b=rel_l2(nb, leaves['norm_out.linear.bias'].grad))
    print(rels)
    assert all(v < 5e-2 for v in rels.values()), rels
    assert info['grad_norm'] > 0 and not info['skipped'] and (dist.params - p_before).abs().max().item() > 0


def test_data_mode_at_pure_noise_equals_the_data_free_first_segment_with_lora():
    """nfe 2, timestep_ratio 1 and t_draws = 0 put every sample on raw_t_src = 1: x_t is the noise, and the data-mode gradient is the
    data-free first segment's on the same noise and draws without its segment weight of 0.5.  Kept-against-recompute figure: 3e-5."""
    from arcflow_amd.train import ArcFlowDistiller, DistillConfig
    cfg, w = _toy()
    B, hp, wp, T, r = 2, 8, 8, 64, 64
    pe, pooled, x0, noise, draws = _inputs(B, hp, wp, T, seed=9)
    cond = dict(prompt_embeds=pe.cuda(), pooled=pooled.cuda(), hp=hp, wp=wp)
    g = torch.Generator().manual_seed(10)
    res, Bs = {}, None
    for mode in ('data', 'data_free'):
        dc = DistillConfig(mode=mode, num_decay_iters=4, warmup_iters=0, grad_clip_begin_iter=10 ** 9, ema_start_iter=0, lora_rank=r, lora_dropout=0.0)
        d = ArcFlowDistiller('flux', ENG, w, dc)
        tr = d.trunk
        if Bs is None:
            Bs = {sp.name: (torch.randn(sp.out_f, r, generator=g) * 0.02) for sp in tr.specs}
        for sp in tr.specs:
            tr.B(sp).copy_(Bs[sp.name].cuda())
        tr.refresh()
        d.iteration = 2                      # teacher_ratio 0.5
        if mode == 'data':
            info = d.train_step(cond, B, x0=x0.cuda(), t_draws=torch.zeros(B), noise=noise.cuda(), draws=draws)
            assert torch.equal(d.last_x, noise.cuda())
            res[mode] = (info['loss'], d.grad.clone())
        else:
            d._launched = []
            d._segment(0, noise.cuda(), torch.ones(B, device='cuda'), cond, 0.5, 0.5, None, draws[0], batch_total=B)
            torch.cuda.synchronize()
            res[mode] = (float(d._loss_acc), d.grad.clone())
    (l_data, g_data), (l_free, g_free) = res['data'], res['data_free']
    assert g_free.abs().max().item() > 0 and g_free[d._off[4]:].abs().max().item() > 0        # the adapters' part is live
    rel = rel_l2(g_data, g_free / 0.5)
    print('data mode vs data-free segment / 0.5: gradient rel-L2', rel, 'loss', l_data, l_free / 0.5)
    assert rel <= 3e-5, rel
    assert abs(l_data - l_free / 0.5) <= 1e-5 * abs(l_data)


def test_float_segment_path_is_unchanged_by_the_tensor_path():
    """A data-free step with its scalar segments against the same step with every segment handed over as a [B] tensor of that value."""
    from arcflow_amd.train import ArcFlowDistiller, DistillConfig
    cfg, w = _toy()
    B, hp, wp, T = 2, 8, 8, 12
    g = torch.Generator().manual_seed(3)
    cond = dict(prompt_embeds=(torch.randn(B, T, 128, generator=g) * 0.5).bfloat16().cuda(),
                pooled=(torch.randn(B, 64, generator=g) * 0.5).bfloat16().cuda(), hp=hp, wp=wp)
    x_init = torch.randn(B, hp * wp, 64, generator=g).cuda()
    draws = [(torch.rand(B, 16, generator=g), torch.rand(B, 4, generator=g), torch.rand(B, 3, generator=g)) for _ in range(2)]
    res = []
    for routed in (False, True):
        d = ArcFlowDistiller('flux', ENG, w, DistillConfig(num_decay_iters=4, warmup_iters=0, grad_clip_begin_iter=10 ** 9, ema_start_iter=0))
        d.iteration = 1
        if routed:
            inner, seen = d._segment, []

            def as_tensor(step_id, x_src, raw_src, cc, ratio, segment, *a, inner=inner, seen=seen, **kw):
                seen.append(segment)
                return inner(step_id, x_src, raw_src, cc, ratio, torch.full((x_src.shape[0],), segment), *a, loss_weight=segment, **kw)
            d._segment = as_tensor
        info = d.train_step(cond, B, x_init=x_init, draws=draws)
        if routed:
            assert seen == [0.5, 0.5]
        res.append((info['loss'], d.last_x.clone(), d.grad.clone()))
    (l0, x0_, g0), (l1, x1, g1) = res
    assert torch.equal(x0_, x1)
    assert abs(l0 - l1) <= 1e-5 * abs(l0), (l0, l1)
    rel = rel_l2(g1, g0)
    print('tensor-segment path vs float path: gradient rel-L2', rel)
    assert rel <= 3e-5, rel          # the loss kernel's float atomics order the sum differently from run to run


def test_data_mode_micro_batches_sum_to_the_batch():
    """batch 6 = micro-batches of 4 + 2: the step equals those two micro-batches run as separate steps on the same draws, combined as
    (4 g_a + 2 g_b) / 6.  Bounds of test_distill.py::test_micro_batched_step_equals_one_batch."""
    from arcflow_amd.train import ArcFlowDistiller, DistillConfig
    cfg, w = _toy()
    B, hp, wp, T = 6, 8, 8, 12
    pe, pooled, x0, noise, draws = _inputs(B, hp, wp, T, seed=33)
    pe, pooled, x0, noise = pe.cuda(), pooled.cuda(), x0.cuda(), noise.cuda()
    u = torch.tensor([0.9, 0.5, 0.1, 0.3, 0.75, 0.0])
    dc = DistillConfig(mode='data', nfe=3, timestep_ratio=0.5, num_decay_iters=4, warmup_iters=0, grad_clip_begin_iter=10 ** 9, ema_start_iter=0)
    big = ArcFlowDistiller('flux', ENG, w, dc)
    big.iteration = 1
    info = big.train_step(dict(prompt_embeds=pe, pooled=pooled, hp=hp, wp=wp), B, x0=x0, t_draws=u, noise=noise, draws=draws)
    acc, loss = torch.zeros_like(big.grad), 0.0
    for a, b in ((0, 4), (4, 6)):
        d = ArcFlowDistiller('flux', ENG, w, dc)
        d.iteration = 1
        i2 = d.train_step(dict(prompt_embeds=pe[a:b], pooled=pooled[a:b], hp=hp, wp=wp), b - a, x0=x0[a:b], t_draws=u[a:b],
                          noise=noise[a:b], draws=[tuple(t[a:b] for t in draws[0])])
        acc += d.grad * ((b - a) / B)
        loss += i2['loss'] * ((b - a) / B)
        assert torch.equal(d.last_x, big.last_x[a:b])
    rel = rel_l2(big.grad, acc)
    print('batch 6 vs 4 + 2 separate steps: gradient rel-L2', rel)
    assert rel < 2e-3, rel
    assert abs(info['loss'] - loss) < 1e-3 * abs(loss)
    assert big.last_x.shape == (B, hp * wp, 64)
