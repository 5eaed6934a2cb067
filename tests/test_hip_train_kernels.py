"""GPU parity of the distillation-step kernels against torch autograd on the CPU oracle."""
import numpy as np
import pytest
import torch
from bf16_parity import U32, check_bf16 as _check_bf16

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from arcflow_amd import ops as _ops
    return _ops


def close(a, b, rtol=2e-5, atol=2e-5):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err = (a - b).abs().max().item()
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f'max abs err {err}, ref scale {b.abs().max().item()}'


def _mix(seed=0, B=2, N=24, K=16, ch=64, pp=4):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, ch, generator=g)
    m = torch.randn(B, N, K, ch, generator=g)
    lw = torch.log_softmax(torch.randn(B, N, K, pp, generator=g) * 1.5, dim=2)
    lg = torch.randn(B, N, K - 1, pp, generator=g)
    lg[0, 0] = 0.0
    lg[0, 1] = 3e-5
    lg[1, 2] = -3e-5
    up = torch.randn(B, N, ch, generator=g)
    return x, m, lw, lg, up


def test_arcflow_backward_step_and_velocity(ops):
    from oracle import arcflow_ref as R
    x, m, lw, lg, up = _mix()
    B = x.shape[0]
    s_src = torch.tensor([1.0, 0.8])
    s_a = torch.tensor([0.9, 0.55])
    s_b = torch.tensor([0.4, 0.1])
    gs = torch.tensor([0.7, -1.3])
    mr, lwr, lgr = (t.clone().requires_grad_(True) for t in (m, lw, lg))
    tot = 0
    for b in range(B):
        xe = R.momentum_step_packed(x[b:b + 1], mr[b:b + 1], lwr[b:b + 1], lgr[b:b + 1], float(s_src[b]), float(s_a[b]), float(s_b[b]))
        disp = x[b:b + 1] - xe
        tot = tot + (disp * up[b:b + 1]).sum() * gs[b]
    tot.backward()
    dm, dw, dg = ops.arcflow_backward(up.cuda(), m.cuda(), lw.cuda(), lg.cuda(), s_src.cuda(), s_a.cuda(), s_b.cuda(), gscale=gs.cuda())
    close(dm, mr.grad)
    close(dw, lwr.grad, atol=2e-4)
    close(dg, lgr.grad, atol=2e-4)
    # velocity form + accumulation into the same buffers
    mr2, lwr2, lgr2 = (t.clone().requires_grad_(True) for t in (m, lw, lg))
    hp, wp = 4, 6
    ml, lwl, lgl = R.unpack_mixture(mr2, lwr2, lgr2, hp, wp)
    u = R.pack_latents(R.policy_velocity(ml, lwl, lgl, s_src, s_a))
    (u * up).sum().backward()
    ops.arcflow_backward(up.cuda(), m.cuda(), lw.cuda(), lg.cuda(), s_src.cuda(), s_a.cuda(), s_a.cuda(), velocity=True, grads=(dm, dw, dg))
    close(dm, mr.grad + mr2.grad)
    close(dw, lwr.grad + lwr2.grad, atol=2e-4)
    close(dg, lgr.grad + lgr2.grad, atol=2e-4)


def test_step_dropout_euler_cfg_mse(ops):
    from oracle import arcflow_ref as R
    x, m, lw, lg, up = _mix(1)
    B, N, K = x.shape[0], x.shape[1], m.shape[2]
    drop = torch.zeros(B, K, dtype=torch.bool)
    drop[0, 3] = drop[0, 7] = drop[1, 0] = True
    s_src, s_a, s_b = torch.tensor([1.0, 0.7]), torch.tensor([0.95, 0.7]), torch.tensor([0.5, 0.2])
    out = ops.arcflow_step_dropout(x.cuda(), m.cuda(), lw.cuda(), lg.cuda(), s_src.cuda(), s_a.cuda(), s_b.cuda(), drop.cuda())
    lwm = lw.masked_fill(drop[:, None, :, None], float('-inf'))
    for b in range(B):
        ref = R.momentum_step_packed(x[b:b + 1], m[b:b + 1], lwm[b:b + 1], lg[b:b + 1], float(s_src[b]), float(s_a[b]), float(s_b[b]))
        close(out[b:b + 1], ref)
    close(ops.euler_roll(x.cuda(), up.cuda(), s_a.cuda(), s_b.cuda()), x + up * (s_b - s_a).reshape(B, 1, 1))
    close(ops.cfg_combine(x.cuda(), up.cuda(), 4.0), x + R.cfg_bias(x, up, 4.0))
    loss = torch.zeros(1, device='cuda')
    coef = 30.0 / x[0].numel() / B * 0.5
    g = ops.mse_loss(x.cuda(), up.cuda(), coef, loss)
    ref_loss = R.flow_mse_loss(x.reshape(B, -1), up.reshape(B, -1)) * 0.5        # x segment size 0.5
    close(loss[0], ref_loss, rtol=1e-5)
    close(g, coef * (x - up))


def test_head_grad_and_weight_grads(ops):
    g = torch.Generator().manual_seed(3)
    B, N, K, ch, lw_ch, D = 2, 96, 16, 64, 4, 256
    M = B * N
    xn = torch.randn(M, D, generator=g).bfloat16()
    w = (torch.randn(1152, D, generator=g) * 0.05).bfloat16()
    w[1148:] = 0
    wr = w.float().clone().requires_grad_(True)
    y = xn.float() @ wr.T
    means = y[:, :1024].reshape(B, N, K, ch)
    logw = y[:, 1024:1088].reshape(B, N, K, lw_ch).log_softmax(dim=2)
    logg = y[:, 1088:1148].reshape(B, N, K - 1, lw_ch)
    dm = torch.randn(B, N, K, ch, generator=g)
    dw = torch.randn(B, N, K, lw_ch, generator=g)
    dg = torch.randn(B, N, K - 1, lw_ch, generator=g)
    ((means * dm).sum() + (logw * dw).sum() + (logg * dg).sum()).backward()
    dy = ops.head_grad(dm.cuda(), dw.cuda(), dg.cuda(), logw.detach().bfloat16().cuda(), 1152)
    # reference dY from autograd: recompute via y.grad is not retained, so rebuild analytically
    yl = y.detach().clone().requires_grad_(True)
    ml = yl[:, :1024].reshape(B, N, K, ch)
    ll = yl[:, 1024:1088].reshape(B, N, K, lw_ch).log_softmax(dim=2)
    gl = yl[:, 1088:1148].reshape(B, N, K - 1, lw_ch)
    ((ml * dm).sum() + (ll * dw).sum() + (gl * dg).sum()).backward()
    close(dy.float()[:, :1148], yl.grad[:, :1148], rtol=1e-2, atol=2e-2)      # bf16 rows
    assert dy[:, 1148:].abs().max().item() == 0
    # dW = dY^T X through the transposed-operand GEMM with fp32 output
    dyt, xt = ops.transpose(dy), ops.transpose(xn.cuda())
    assert torch.equal(dyt.cpu(), dy.cpu().T) and torch.equal(xt.cpu(), xn.T)
    Mp = (M + 63) // 64 * 64
    assert Mp == M
    dW = ops.linear_f32out(dyt, xt)
    ref = dy.float().cpu().T @ xn.float()
    close(dW, ref, rtol=1e-4, atol=1e-3)
    dW2 = ops.linear_f32out(dyt, xt, out=dW.clone(), accumulate=True)
    close(dW2, 2 * ref, rtol=1e-4, atol=2e-3)
    rel = ((dW[:1148].cpu() - wr.grad[:1148]).norm() / wr.grad[:1148].norm()).item()
    assert rel < 5e-3, rel                                                       # vs autograd (dY rounded to bf16)
    db = ops.colsum(dy, torch.zeros(1152, device='cuda'))
    close(db, dy.float().cpu().sum(0), rtol=1e-5, atol=1e-3)


def test_normout_backward_and_outer(ops):
    g = torch.Generator().manual_seed(4)
    B, N, D = 2, 64, 512
    x = (torch.randn(B * N, D, generator=g) * 2 + 0.5).bfloat16()
    dxn = torch.randn(B * N, D, generator=g).bfloat16()
    sc = torch.randn(B, D, generator=g).requires_grad_(True)
    sh = torch.randn(B, D, generator=g).requires_grad_(True)
    xn = torch.nn.functional.layer_norm(x.float(), (D,), eps=1e-6).reshape(B, N, D) * (1 + sc[:, None]) + sh[:, None]
    (xn * dxn.float().reshape(B, N, D)).sum().backward()
    dmod = ops.normout_backward(x.cuda(), dxn.cuda(), torch.zeros(B, 2, D, device='cuda'), N)
    close(dmod[:, 0], sc.grad, rtol=1e-4, atol=1e-3)
    close(dmod[:, 1], sh.grad, rtol=1e-4, atol=1e-3)
    semb = torch.randn(B, 128, generator=g)
    dflat = dmod.reshape(B, 2 * D)
    dW = ops.outer_accum(dflat, semb.cuda(), torch.ones(2 * D, 128, device='cuda'))
    close(dW, 1 + dflat.cpu().T @ semb, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize('B,N,D', [(1, 4608, 3072), (2, 516, 3072), (3, 100, 1024), (1, 504, 3072), (1, 512, 3072), (2, 4095, 3072),
                                   (4, 4096, 3072)])
def test_normout_backward_training_shapes(ops, B, N, D):
    """The two-stage version (per-wave partial sums, then a fold over the waves of a batch entry) at the training shapes: many waves per
    batch entry (split fold), a row count that forces fewer rows per wave (516 = 4 x 129), accumulation INTO a non-zero result.
    504 / 512 rows per batch entry sit either side of the 1 -> 8 split switch (63 / 64 waves of 8 rows), 4095 is odd (1 row per wave),
    4 x 4096 is the B = 4 distillation step.  Column-dependent offsets of x give every column of d_scale a non-zero mean, dxn has mean 1;
    both are column views of wider rows.  Besides the old tolerance: the summation-order bound and the dropped-wave check (see below)."""
    g = _gen(B * N)
    R = B * N
    off = torch.nn.functional.pad(torch.randn(D, generator=g, device='cuda') * 2 + 0.5, (0, 64))
    x = (torch.randn(R, D + 64, generator=g, device='cuda') * 2 + off).bfloat16()[:, :D]
    dxn = (torch.randn(R, D + 32, generator=g, device='cuda') * 0.5 + 1.0).bfloat16()[:, 32:]
    y, rstd = _ln64(x)
    dd = dxn.double()
    t_sc, t_sh = (dd * y).reshape(B, N, D), dd.reshape(B, N, D)
    dsc, dsh = t_sc.sum(1), t_sh.sum(1)
    start = torch.full((B, 2, D), 0.5, device='cuda')
    dmod = ops.normout_backward(x, dxn, start.clone(), N)
    close(dmod[:, 0] - 0.5, dsc.float(), rtol=2e-4, atol=2e-2)
    close(dmod[:, 1] - 0.5, dsh.float(), rtol=2e-4, atol=2e-2)
    rpw = 8                                                              # rows per wave, as afx_normout_backward picks it
    while N % rpw:
        rpw //= 2
    wpb = N // rpw
    splits = 8 if wpb >= 64 else 1
    depth = rpw + (wpb + splits - 1) // splits + splits + 3            # rows per wave, waves per split, split atomics, start + pair folds
    # LN(x) carries the fp32 error of its row statistics: (D / 64 serial + 6 wave levels + 4) u relative to |y| + |x| rstd
    mag_sc = (dd.abs() * (y.abs() + x.double().abs() * rstd)).reshape(B, N, D).sum(1) + 0.5
    _check_sum(dmod[:, 0], 0.5 + dsc, mag_sc, depth + D // 64 + 10, 0.5 + dsc - t_sc[:, N - rpw:].sum(1), f'd_scale {B}x{N}')
    _check_sum(dmod[:, 1], 0.5 + dsh, t_sh.abs().sum(1) + 0.5, depth, 0.5 + dsh - t_sh[:, N - rpw:].sum(1), f'd_shift {B}x{N}')


def test_adamw_ema_sumsq_cast(ops):
    g = torch.Generator().manual_seed(5)
    n = 100003
    p0 = torch.randn(n, generator=g)
    pr = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([pr], lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.01)
    p = p0.clone().cuda()
    m, v = torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
    for step in range(1, 4):
        gr = torch.randn(n, generator=g)
        pr.grad = gr.clone() * 0.5
        opt.step()
        ops.adamw_step(p, gr.cuda(), m, v, 1e-3, step, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.01, grad_scale=0.5)
    close(p, pr.data, rtol=1e-5, atol=1e-6)
    ema = torch.randn(n, generator=g)
    e = ema.clone().cuda()
    ops.ema_lerp(e, p, 0.93)
    close(e, p.cpu() + (ema - p.cpu()) * 0.93)
    acc = ops.sumsq(p, torch.zeros(1, device='cuda'))
    close(acc[0], (p.cpu().double() ** 2).sum().float(), rtol=1e-4, atol=1e-2)
    close(ops.cast_bf16(p).float(), p.cpu().bfloat16().float(), rtol=0, atol=0)


@pytest.mark.parametrize('B,S,H', [(1, 64, 1), (2, 200, 2), (1, 333, 3), (1, 1024, 2), (2, 128, 1), (1, 97, 9), (1, 1500, 2), (1, 4608, 1)])
def test_attention_backward(ops, B, S, H):
    g = torch.Generator().manual_seed(S + 1)
    q, k, v, do = (torch.randn(B, S, H, 128, generator=g).bfloat16() for _ in range(4))
    qr, kr, vr = (t.float().clone().requires_grad_(True) for t in (q, k, v))
    ref = torch.nn.functional.scaled_dot_product_attention(qr.transpose(1, 2), kr.transpose(1, 2), vr.transpose(1, 2)).transpose(1, 2)
    (ref * do.float()).sum().backward()
    o, lse = ops.attention_fwd_lse(q.cuda(), k.cuda(), v.cuda())
    o_plain = ops.attention(q.cuda(), k.cuda(), v.cuda())
    assert torch.equal(o, o_plain)                                  # the LSE side output does not perturb O
    # lse is the log2-domain log-sum-exp of the scaled scores
    s = torch.einsum('bqhd,bkhd->bhqk', q.float(), k.float()) / 128 ** 0.5
    ref_lse = torch.logsumexp(s, dim=-1) / np.log(2.0)
    assert torch.allclose(lse[:, :, :S].cpu(), ref_lse, atol=2e-2)
    dq, dk, dv = ops.attention_bwd(q.cuda(), k.cuda(), v.cuda(), o.reshape(B, S, H, 128), do.cuda(), lse)

    def rel(a, b):
        return ((a.float().cpu() - b).norm() / b.norm()).item()
    assert rel(dv, vr.grad) < 1.5e-2, rel(dv, vr.grad)
    assert rel(dq, qr.grad) < 2e-2, rel(dq, qr.grad)
    assert rel(dk, kr.grad) < 2e-2, rel(dk, kr.grad)
    for t in (dq, dk, dv):
        assert torch.isfinite(t.float()).all()


@pytest.mark.parametrize('S,H', [(4608, 24), (4224, 24), (4133, 5)])
def test_attention_backward_generations_agree_at_the_production_shapes(ops, S, H):
    """FLUX (4096 + 512 tokens) and Qwen-Image (4096 + 128) shapes, 24 heads, and a ragged one: the generated streams (one launch / two launches / dK-dV only)
    against the round-4 kernels -- the same mathematics and the same bf16 rounding points (P and dS rounded to bf16 before the accumulating products), so the
    results differ by summation order only."""
    g = torch.Generator(device='cuda').manual_seed(S)
    q, k, v, do = (torch.randn(1, S, H, 128, generator=g, device='cuda').bfloat16() for _ in range(4))
    o, lse = ops.attention_fwd_lse(q, k, v)
    try:
        ops.set_attn_bwd_impl(2)
        ref = ops.attention_bwd(q, k, v, o.reshape(1, S, H, 128), do, lse)
        for impl in (3, 4, 1):
            ops.set_attn_bwd_impl(impl)
            got = ops.attention_bwd(q, k, v, o.reshape(1, S, H, 128), do, lse)
            for name, a, b in zip(('dq', 'dk', 'dv'), got, ref):
                assert torch.isfinite(a.float()).all()
                err = ((a.float() - b.float()).norm() / b.float().norm()).item()
                assert err < 6e-3, (impl, name, err)
    finally:
        ops.set_attn_bwd_impl(3)


def test_attention_backward_strided_views_and_determinism(ops):
    """The training trunk hands the backward row-strided views (q | k | v columns of one [rows, 3 H 128] stash, gradients into a second one); the generated
    kernels (afx_attn_bwd3.hip) read them through LDS-DMA with the caller's strides.  Same numbers as the contiguous call, bit for bit, and twice the same
    (no atomics anywhere in the backward)."""
    B, S, H = 2, 333, 2
    g = torch.Generator().manual_seed(11)
    q, k, v, do = (torch.randn(B, S, H, 128, generator=g).bfloat16().cuda() for _ in range(4))
    o, lse = ops.attention_fwd_lse(q, k, v)
    ref = ops.attention_bwd(q, k, v, o.reshape(B, S, H, 128), do, lse)
    D = H * 128
    stash = torch.zeros(B * S, 3 * D + 64, dtype=torch.bfloat16, device='cuda')
    stash[:, :D], stash[:, D:2 * D], stash[:, 2 * D:3 * D] = q.reshape(B * S, D), k.reshape(B * S, D), v.reshape(B * S, D)
    gbuf = torch.full((B * S, 3 * D), 7.0, dtype=torch.bfloat16, device='cuda')
    dov = torch.zeros(B * S, D + 8, dtype=torch.bfloat16, device='cuda')
    dov[:, :D] = do.reshape(B * S, D)
    for _ in range(2):
        ops.attention_bwd_2d(stash[:, :D], stash[:, D:2 * D], stash[:, 2 * D:3 * D], o.reshape(B * S, D), dov[:, :D], lse, gbuf[:, :D], gbuf[:, D:2 * D],
                             gbuf[:, 2 * D:], B, S, H)
        for i, r in enumerate(ref):
            assert torch.equal(gbuf[:, i * D:(i + 1) * D], r.reshape(B * S, D)), i


def test_elementwise_backward_kernels(ops):
    from oracle import dit_ref as D
    g = torch.Generator().manual_seed(9)
    B, S, Dm = 2, 37, 512
    x = (torch.randn(B * S, Dm, generator=g) * 1.5 + 0.2).bfloat16()
    dxn = torch.randn(B * S, Dm, generator=g).bfloat16()
    dres = torch.randn(B * S, Dm, generator=g).bfloat16()
    sc = torch.randn(B, Dm, generator=g)
    xr = x.float().clone().requires_grad_(True)
    xn = torch.nn.functional.layer_norm(xr, (Dm,), eps=1e-6).reshape(B, S, Dm) * (1 + sc[:, None])
    (xn * dxn.float().reshape(B, S, Dm)).sum().backward()
    out = ops.ln_modulate_backward(x.cuda(), dxn.cuda(), sc.cuda(), S, dres=dres.cuda())
    ref = xr.grad + dres.float()
    assert ((out.float().cpu() - ref).norm() / ref.norm()).item() < 6e-3
    # RMSNorm + RoPE out-of-place forward == in-place kernel, backward vs autograd
    hp, wp, T, H = 4, 5, 6, 2
    S2 = T + hp * wp
    q = torch.randn(B, S2, H * 128, generator=g).bfloat16()
    dy = torch.randn(B, S2, H * 128, generator=g).bfloat16()
    wt, wi = 1 + 0.1 * torch.randn(128, generator=g), 1 + 0.1 * torch.randn(128, generator=g)
    cos, sin = D.flux_rope_tables(hp, wp, T)
    y = ops.qk_norm_rope(q.cuda(), wt.cuda(), wi.cuda(), cos.cuda(), sin.cuda(), T)
    y_ip = ops.qk_norm_rope_(q.cuda().reshape(B, S2, H, 128).clone(), wt.cuda(), wi.cuda(), cos.cuda(), sin.cuda(), T)
    assert torch.equal(y.reshape(B, S2, H, 128), y_ip)
    qr = q.float().clone().requires_grad_(True)
    q4 = qr.reshape(B, S2, H, 128)
    yr = torch.cat([D.apply_rope(D.rms_norm(q4[:, :T], wt), cos[:T], sin[:T]),
                    D.apply_rope(D.rms_norm(q4[:, T:], wi), cos[T:], sin[T:])], dim=1)
    (yr * dy.float().reshape(B, S2, H, 128)).sum().backward()
    dq = ops.qk_norm_rope(q.cuda(), wt.cuda(), wi.cuda(), cos.cuda(), sin.cuda(), T, dy=dy.cuda())
    assert ((dq.float().cpu() - qr.grad).norm() / qr.grad.norm()).item() < 6e-3
    # GELU forward / backward, add_scale
    pre = (torch.randn(50, 256, generator=g) * 2).bfloat16()
    dh = torch.randn(50, 256, generator=g).bfloat16()
    pr = pre.float().clone().requires_grad_(True)
    hr = torch.nn.functional.gelu(pr, approximate='tanh')
    (hr * dh.float()).sum().backward()
    assert ((ops.gelu(pre.cuda()).float().cpu() - hr.detach()).abs().max().item()) < 2e-2
    dpre = ops.gelu(pre.cuda(), dh=dh.cuda())
    assert ((dpre.float().cpu() - pr.grad).norm() / pr.grad.norm()).item() < 6e-3
    gate = torch.randn(2, 256, generator=g)
    out = ops.add_scale(pre.cuda(), dh.cuda(), gate.cuda(), rows_per_batch=25)
    ref = (pre.float() + dh.float()) * gate.repeat_interleave(25, 0)
    assert ((out.float().cpu() - ref).norm() / ref.norm()).item() < 6e-3


# ------------------------------------------------------------------------------------------ TN product (LoRA weight gradients, afx_tn.hip)
@pytest.mark.parametrize('M,N1,N2', [(4608, 3072, 256), (4096, 256, 3072), (512, 12288, 256), (77, 256, 1024), (130, 64, 192), (4608, 256, 15360),
                                     (64, 128, 128), (1, 8, 8), (333, 200, 72)])
def test_linear_tn_f32out_matches_transposed_products(ops, M, N1, N2):
    """C (+)= X^T Y straight from token-major operands (ds_read_b64_tr_b16 fragments) against fp32 math and against the round-4 path (two explicit
    transposes + the NT kernel): the LoRA shapes (dB [out, 256] over 4608 / 512 tokens, dA [256, in]), ragged token counts (the last K-step's rows
    past M are zeroed in LDS), widths below / off the 128-column tile, strided views (a column range of a wider buffer) and the accumulate mode.
    The inputs are NOT symmetric: a swapped operand or a transposed output would show."""
    g = torch.Generator(device='cuda').manual_seed(M + 3 * N1 + 7 * N2)
    xw = torch.randn(M, N1 + 64, generator=g, device='cuda').bfloat16()
    yw = (torch.randn(M, N2 + 8, generator=g, device='cuda') * 0.5 + 0.1).bfloat16()
    x, y = xw[:, 32:32 + N1], yw[:, 8:8 + N2]                                  # views: row stride != width, 16-byte aligned starts
    ref = x.float().t() @ y.float()
    out = ops.linear_tn_f32out(x, y)
    scale = ref.abs().max().item() + 1e-6
    assert (out - ref).abs().max().item() <= 2e-5 * scale * max(1.0, (M / 64) ** 0.5), ((out - ref).abs().max().item(), scale)
    c0 = torch.randn(N1, N2 + 4, generator=g, device='cuda')
    c = c0.clone()
    ops.linear_tn_f32out(x, y, out=c[:, :N2], accumulate=True)
    assert torch.equal(c[:, N2:], c0[:, N2:])                                   # nothing written past the columns
    assert (c[:, :N2] - (c0[:, :N2] + ref)).abs().max().item() <= 3e-5 * (scale + c0.abs().max().item()) * max(1.0, (M / 64) ** 0.5)
    if True:                                                                   # the round-4 formulation: same products, fp32 accumulation in another order
        old = ops.linear_f32out(ops.transpose(x.contiguous(), 64), ops.transpose(y.contiguous(), 64))
        assert (out - old).abs().max().item() <= 2e-5 * scale * (M / 64) ** 0.5
    # deterministic: a second launch is bit-identical (also with the token loop split over work-groups: partial tiles added in a fixed order)
    assert torch.equal(out, ops.linear_tn_f32out(x, y))
    from arcflow_amd import _lib
    nws = _lib.load().afx_linear_tn_ws_bytes(M, N1, N2)
    if (M, N1, N2) in ((4608, 3072, 256), (4096, 256, 3072), (4608, 256, 15360)):
        assert nws > 0 and nws % (4 * N1 * N2) == 0 and nws // (4 * N1 * N2) >= 2         # the LoRA gradient shapes take the split
    if M <= 130:
        assert nws == 0                                                                    # too few K-steps to cut


@pytest.mark.parametrize('M,N,K,p', [(4608, 3072, 256, 0.05), (512, 12288, 256, 0.05), (130, 192, 64, 0.3), (4096, 15360, 256, 0.0)])
def test_linear_dropres_matches_product_then_masked_add(ops, M, N, K, p):
    """dx = dx0 + ((dy B) A) . keep/(1-p) in the GEMM's epilogue against the round-4 formulation (product to memory as bf16, then lora_dropout mode 3):
    the SAME mask bits (dropped positions keep the residual bit for bit), kept positions equal up to the bf16 rounding of the product that no longer happens;
    in place over the residual; every tile shape the launcher picks for these sizes."""
    g = torch.Generator(device='cuda').manual_seed(M + N)
    a = torch.randn(M, K, generator=g, device='cuda').bfloat16()
    w = (torch.randn(N, K, generator=g, device='cuda') * 0.1).bfloat16()
    res = torch.randn(M, N, generator=g, device='cuda').bfloat16()
    seed, row0 = 0x1234567, 4608
    old = res.clone()
    ops.lora_dropout(ops.linear(a, w), p, seed, row0, mode=3, out=old)
    new = res.clone()
    ops.linear_dropres(a, w, new, p, seed, row0, out=new)
    prod = a.float() @ w.float().t()
    keep = ops.lora_dropout(torch.ones(M, N, device='cuda', dtype=torch.bfloat16), p, seed, row0, mode=1) > 0
    ref = res.float() + torch.where(keep, prod / (1.0 - p), torch.zeros_like(prod))
    assert torch.equal(new[~keep], res[~keep])                                 # dropped: the residual, untouched
    assert abs(float((~keep).float().mean()) - p) < 0.01
    scale = ref.abs().max().item()
    assert (new.float() - ref).abs().max().item() <= 2 ** -8 * scale           # one bf16 rounding of the sum
    assert (new.float() - ref).abs().max().item() <= (old.float() - ref).abs().max().item() + 1e-6
    # under a kernel choice without the fused epilogue (A/B runs, parity tests: set_gemm_mode(2) = the 8-phase kernel) the call falls back to product + mask-and-add
    # instead of failing -- the round-4 formulation's bits exactly
    from arcflow_amd import _lib
    try:
        ops.set_gemm_mode(2)
        assert _lib.load().afx_gemm_dropres_available() == 0
        fb = res.clone()
        ops.linear_dropres(a, w, fb, p, seed, row0, out=fb)
        old2 = res.clone()
        ops.lora_dropout(ops.linear(a, w), p, seed, row0, mode=3, out=old2)
        assert torch.equal(fb, old2)
    finally:
        ops.set_gemm_mode(3)
    assert _lib.load().afx_gemm_dropres_available() == 1


def test_linear_dropres_and_lora_dropout_draw_the_same_mask_across_the_row_wrap(ops):
    """The GEMM's masked residual add and lora_dropout_kernel hash (seed, row0 + row, col) with one function: the elements linear_dropres leaves equal to
    the residual are exactly the ones lora_dropout(mode=1) zeroes -- two index sets, no tolerance -- with row0 = 2^31 - 3, so that the global row
    passes 2^31 inside the matrix (the row hash keeps the low 32 bits of a 64-bit product).  Every product is >= 64 * 0.25 = 16 against residuals
    of order 1: no product is an exact zero and no kept sum rounds back to its residual."""
    M, N, K, p, seed, row0 = 256, 256, 64, 0.25, 0x1234567, 2 ** 31 - 3
    g = torch.Generator(device='cuda').manual_seed(7)
    a = (torch.rand(M, K, generator=g, device='cuda') + 0.5).bfloat16()
    w = (torch.rand(N, K, generator=g, device='cuda') + 0.5).bfloat16()
    res = torch.randn(M, N, generator=g, device='cuda').bfloat16()
    new = res.clone()
    ops.linear_dropres(a, w, new, p, seed, row0, out=new)
    dropped = ops.lora_dropout(torch.ones(M, N, device='cuda', dtype=torch.bfloat16), p, seed, row0, mode=1) == 0
    assert torch.equal(new == res, dropped)
    assert abs(float(dropped.float().mean()) - p) < 0.01


# ------------------------------------------------------------------------------------------ full-width parity against fp64
# The distillation backward at the production shapes (D = 3072, H = 24, MLP 12288; 4608 = 4096 + 512 FLUX rows, 4224 = 4096 + 128 Qwen rows,
# and a ragged 4133), against a plain fp64 torch reference built from the same bf16 / fp32 inputs.  How tight each check is:
#   * bf16 outputs of element-wise kernels: every element within one bf16 ulp of the fp64 value (plus, where said, the fp32 evaluation error
#     of a formula that cancels), and >= 99 % of them equal to the fp64 value rounded to nearest even.  A systematic relative error e moves
#     about e / 5.4e-3 of the elements across a rounding boundary (5.4e-3 = the mean bf16 ulp / |x|), so e = 3e-3 fails the second check
#     with ~55 % and e = 1e-4 with ~2 %.
#   * row-normalising kernels: one bf16 ulp plus fp32 eps x D x the row's scale, and >= 98 % rounded like the reference (e = 1e-3 fails it).
#   * fp32 reductions: |out - ref| <= depth * 2^-24 * sum |terms| per output, depth = the longest chain of fp32 roundings an output goes
#     through (serial adds per thread + atomic adds + the starting value + product / statistics roundings) -- the classical worst-case bound
#     of recursive summation.  Inputs have non-zero mean, and every such test also shows that the bound is not vacuous: the same comparison
#     against the reference with one kernel-sized row slab left out fails.
def _check_sum(out, ref, mag, depth, ref_drop, what=''):
    """fp32 reduction: |out - ref| <= depth u mag everywhere; and the same comparison against ref_drop (one slab left out) fails."""
    bound = depth * U32 * mag
    err = (out.double() - ref).abs()
    assert bool((err <= bound).all()), f'{what}: max err / bound {(err / bound).max().item():.3f} (depth {depth})'
    assert bool(((out.double() - ref_drop).abs() > bound).any()), f'{what}: the bound cannot tell a dropped slab'


def _guarded(shape, dtype, sentinel, dev='cuda'):
    return torch.full(shape, sentinel, dtype=dtype, device=dev)


def _unchanged_outside(buf, sentinel, rows, cols, what=''):
    """Everything of buf outside [rows, cols] still holds the sentinel (bit for bit)."""
    mask = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    mask[rows, cols] = False
    assert bool((buf[mask] == sentinel).all()), f'{what}: a write landed outside the view'


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


@pytest.mark.parametrize('R,C', [(4608, 3072), (4224, 3072), (4133, 1152)])
def test_coldot_colsum_full_width(ops, R, C):
    """coldot (32-row slabs x 2048-column blocks: 2 column blocks at 3072) and colsum (256 x 256 tiles; 1152 = 4.5 tiles) over row-sliced
    operands wider than they are (the ybuf slices of trunk.py), into a slice of a larger fp32 buffer that starts non-zero."""
    g = _gen(R + C)
    abuf = (torch.randn(R, C + 96, generator=g, device='cuda') * 0.5 + 1.0).bfloat16()
    bbuf = (torch.randn(R + 9, 2 * C, generator=g, device='cuda') * 0.5 + 0.75).bfloat16()
    a, b = abuf[:, 32:32 + C], bbuf[9:, C:]
    assert a.stride(0) > C and b.stride(0) > C
    ad, bd = a.double(), b.double()
    for name, fn, terms, slab in (('coldot', lambda o: ops.coldot(a, b, o), ad * bd, 32), ('colsum', lambda o: ops.colsum(a, o), ad, 256)):
        acc0 = torch.randn(3 * C, generator=g, device='cuda')
        acc = acc0.clone()
        fn(acc[C:2 * C])
        assert torch.equal(acc[:C], acc0[:C]) and torch.equal(acc[2 * C:], acc0[2 * C:]), f'{name}: wrote outside its slice'
        start = acc0[C:2 * C].double()
        ref = start + terms.sum(0)
        mag = start.abs() + terms.abs().sum(0)
        depth = slab + (R + slab - 1) // slab + 2          # serial rows per thread, one atomic per slab, the start value, the product
        _check_sum(acc[C:2 * C], ref, mag, depth, ref - terms[:slab].sum(0), f'{name} {R}x{C}')


@pytest.mark.parametrize('B,N,K', [(1, 4133, 2056), (2, 1553, 3072), (3, 4096, 2056), (4, 8203, 3072)])
def test_gemv_t_shapes(ops, B, N, K):
    """out[b, k] += sum_n x[b, n] W[n, k]: B = 1..4 partial rows, K = 3072 (2 column blocks of 2048, the second partial) and 2056 (a
    second block of ONE 8-column chunk), N not a multiple of the 512-row slab; x a row-strided view."""
    g = _gen(B * N + K)
    xbuf = torch.rand(B, N + 40, generator=g, device='cuda') + 0.5
    x = xbuf[:, 8:8 + N]
    W = (torch.rand(N, K, generator=g, device='cuda') + 0.5).bfloat16()
    acc0 = torch.rand(B, K, generator=g, device='cuda')
    out = ops.gemv_t(x, W, acc0.clone())
    ref = acc0.double() + x.double() @ W.double()             # all terms positive: sum |terms| = ref
    depth = 512 + (N + 511) // 512 + 2
    _check_sum(out, ref, ref, depth, ref - x[:, :512].double() @ W[:512].double(), f'gemv_t {B}x{N}x{K}')


def test_gemv_t_flux_n_mod(ops):
    """The FLUX modulation matrix: N = n_mod = 344 x 3072 = 1 056 768 rows (2064 row slabs of 512), K = 3072, B = 4.  W (6.5 GB) is built on
    the device and the fp64 reference is computed there in row chunks; everything is freed before the test returns."""
    B, N, K, ch = 4, 344 * 3072, 3072, 32768
    g = _gen(344)
    W = torch.empty(N, K, dtype=torch.bfloat16, device='cuda')
    for i in range(0, N, ch):
        W[i:i + ch] = (torch.rand(min(ch, N - i), K, generator=g, device='cuda') + 0.5).bfloat16()
    x = torch.rand(B, N, generator=g, device='cuda') + 0.5
    acc0 = torch.rand(B, K, generator=g, device='cuda')
    out = ops.gemv_t(x, W, acc0.clone())
    ref = acc0.double()
    for i in range(0, N, ch):
        ref = ref + x[:, i:i + ch].double() @ W[i:i + ch].double()
    drop = x[:, N - 512:].double() @ W[N - 512:].double()
    del W
    torch.cuda.empty_cache()
    _check_sum(out, ref, ref, 512 + N // 512 + 2, ref - drop, 'gemv_t n_mod')


def _ln64(x):
    xd = x.double()
    mu = xd.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((xd - mu) ** 2).mean(-1, keepdim=True) + 1e-6)
    return (xd - mu) * rstd, rstd


@pytest.mark.parametrize('R', [4608, 512, 4133])
def test_normout_backward_split_into_slices(ops, R):
    """The trunk's form (trunk.py _dmod_ln): one batch entry, d_scale and d_shift written into two D-slices of the sample's larger
    modulation-gradient vector (start non-zero, the other slices untouched)."""
    D = 3072
    g = _gen(R + 7)
    x = (torch.randn(R, 3 * D, generator=g, device='cuda') * 1.5 + 0.3).bfloat16()[:, D:2 * D]
    dxn = (torch.randn(R, D, generator=g, device='cuda') * 0.5 + 1.0).bfloat16()
    buf0 = torch.randn(6 * D, generator=g, device='cuda')
    buf = buf0.clone()
    ops.normout_backward_split(x, dxn, buf[4 * D:5 * D], buf[3 * D:4 * D])
    for lo, hi in ((0, 3 * D), (5 * D, 6 * D)):
        assert torch.equal(buf[lo:hi], buf0[lo:hi])
    y, rstd = _ln64(x)
    dd = dxn.double()
    rpw = 8
    while R % rpw:
        rpw //= 2
    wpb = R // rpw
    splits = 8 if wpb >= 64 else 1
    depth = rpw + (wpb + splits - 1) // splits + splits + 3
    ref_sc = buf0[4 * D:5 * D].double() + (dd * y).sum(0)
    ref_sh = buf0[3 * D:4 * D].double() + dd.sum(0)
    mag_sc = (dd.abs() * (y.abs() + x.double().abs() * rstd)).sum(0) + buf0[4 * D:5 * D].double().abs()
    _check_sum(buf[4 * D:5 * D], ref_sc, mag_sc, depth + D // 64 + 10, ref_sc - (dd * y)[:rpw].sum(0), 'split d_scale')
    _check_sum(buf[3 * D:4 * D], ref_sh, dd.abs().sum(0) + buf0[3 * D:4 * D].double().abs(), depth, ref_sh - dd[:rpw].sum(0), 'split d_shift')


@pytest.mark.parametrize('B,Kd', [(1, 3072), (3, 3072), (8, 3072), (4, 1), (8, 1)])
def test_outer_accum_full_width(ops, B, Kd):
    """dW[j, k] += sum_b dmod[b, j] x[b, k] at J = 6144 (2 D), B up to 8, Kd = D and 1 (the bias column)."""
    J = 6144
    g = _gen(B * 100 + Kd)
    dmod = torch.randn(B, J, generator=g, device='cuda') + 0.5
    x = torch.randn(B, Kd, generator=g, device='cuda') + 0.5
    dW0 = torch.randn(J, Kd, generator=g, device='cuda')
    dW = ops.outer_accum(dmod, x, dW0.clone())
    terms = dmod.double()[:, :, None] * x.double()[:, None, :]
    ref = dW0.double() + terms.sum(0)
    # B serial products (each rounded) and adds, then the add into dW; the "slab" here is one batch row
    _check_sum(dW, ref, dW0.double().abs() + terms.abs().sum(0), 2 * B + 2, ref - terms[B - 1], f'outer_accum B={B} Kd={Kd}')


def _strided_bf16(R, C, g, scale=1.0, shift=0.0, pad=64):
    buf = (torch.randn(R, C + pad, generator=g, device='cuda') * scale + shift).bfloat16()
    return buf[:, pad // 2:pad // 2 + C]


@pytest.mark.parametrize('rows_per_batch,B,with_dres', [(0, 1, True), (0, 1, False), (2304, 2, True), (2066, 2, False)])
def test_ln_modulate_backward_full_width(ops, rows_per_batch, B, with_dres):
    """D = 3072: 384 column chunks, six per lane.  Strided x / dxn / dres / out views, per-batch scale rows read with a row stride > D."""
    D = 3072
    R = rows_per_batch * B if rows_per_batch else 4608
    g = _gen(R + B + int(with_dres))
    x = _strided_bf16(R, D, g, 1.5, 0.3)
    dxn = _strided_bf16(R, D, g, 1.0, 0.1)
    dres = _strided_bf16(R, D, g) if with_dres else None
    scbuf = torch.randn(B, 3 * D, generator=g, device='cuda') * 0.3
    sc = scbuf[:, D:2 * D]
    obuf = _guarded((R, D + 64), torch.bfloat16, 7.0)
    out = ops.ln_modulate_backward(x, dxn, sc if B > 1 else sc[0], rows_per_batch, dres=dres, out=obuf[:, 16:16 + D])
    _unchanged_outside(obuf, 7.0, slice(None), slice(16, 16 + D), 'ln_modulate_backward')
    y, rstd = _ln64(x)
    scr = sc.double().repeat_interleave(R // B, 0)
    gq = dxn.double() * (1 + scr)
    mg, mgy = gq.mean(-1, keepdim=True), (gq * y).mean(-1, keepdim=True)
    ref = rstd * (gq - mg - y * mgy)
    row_scale = (rstd * (gq.abs() + mg.abs() + (y * mgy).abs())).amax(-1, keepdim=True)
    if dres is not None:
        ref = ref + dres.double()
        row_scale = row_scale + dres.double().abs().amax(-1, keepdim=True)
    _check_bf16(out, ref, floor=U32 * D * row_scale, min_equal=0.98, what=f'ln_modulate_backward rpb={rows_per_batch}')


def _rope_tables(kind):
    from oracle import dit_ref as Dr
    if kind == 'flux':
        return (*Dr.flux_rope_tables(64, 64, 512), 512)
    img, txt = Dr.qwen_rope_angles(64, 64, 128)
    ang = torch.cat([txt, img])
    return torch.cos(ang).float(), torch.sin(ang).float(), 128


def _qk_ref(x, w_t, w_i, cos, sin, T, dy=None):
    """fp64 per-head RMSNorm (eps 1e-6) + pair RoPE on [B, S, H, 128], or its backward with dy.  Returns (value, per-head scale)."""
    xd = x.double()
    S = xd.shape[1]
    w = torch.where((torch.arange(S, device=x.device) < T)[:, None], w_t.double()[None], w_i.double()[None])[None, :, None]
    rstd = 1.0 / torch.sqrt((xd * xd).mean(-1, keepdim=True) + 1e-6)
    c, s = cos.double()[None, :, None], sin.double()[None, :, None]
    if dy is None:
        n = xd * rstd * w
        a, b = n[..., 0::2], n[..., 1::2]
        out = torch.stack([a * c - b * s, a * s + b * c], -1).flatten(-2)
        return out, n.abs().amax(-1, keepdim=True) * 2
    d = dy.double()
    d0, d1 = d[..., 0::2], d[..., 1::2]
    z = torch.stack([d0 * c + d1 * s, -d0 * s + d1 * c], -1).flatten(-2)
    gg = z * w
    xh = xd * rstd
    dot = (gg * xh).mean(-1, keepdim=True)
    return rstd * (gg - xh * dot), (rstd * (gg.abs() + (xh * dot).abs())).amax(-1, keepdim=True)


@pytest.mark.parametrize('B,kind,width', [(1, 'flux', 9216), (2, 'flux', 9216), (1, 'qwen', 21504), (2, 'qwen', 9216)])
def test_qk_norm_rope_full_width(ops, B, kind, width):
    """H = 24 heads of 128, FLUX (512 text rows) and Qwen (128) tables; with B = 2 the text / image boundary repeats inside one call.  The
    input is the q (or k) column range of a wider qkv row (row stride 9216, 21504 for the single-stream blocks), the output a column range of
    a wider gradient row (trunk.py: dQKVp[:, :D]), the backward's dy a strided view as well."""
    H, D = 24, 3072
    cos, sin, T = _rope_tables(kind)
    S = cos.shape[0]
    cos, sin = cos.cuda(), sin.cuda()
    g = _gen(B * S + width)
    qkv = (torch.randn(B, S, width, generator=g, device='cuda') * 1.3 + 0.2).bfloat16()
    x = qkv[:, :, D:2 * D]
    w_t = 1 + 0.2 * torch.randn(128, generator=g, device='cuda')
    w_i = 1 + 0.2 * torch.randn(128, generator=g, device='cuda')
    dybuf = torch.randn(B, S, 2 * D, generator=g, device='cuda').bfloat16()
    dy = dybuf[:, :, D:]
    for back in (False, True):
        obuf = _guarded((B * S, 3 * D), torch.bfloat16, -3.0)
        out = ops.qk_norm_rope(x, w_t, w_i, cos, sin, T, out=obuf[:, :D], dy=dy if back else None)
        _unchanged_outside(obuf, -3.0, slice(None), slice(0, D), 'qk_norm_rope')
        ref, scale = _qk_ref(x.reshape(B, S, H, 128), w_t, w_i, cos, sin, T, dy.reshape(B, S, H, 128) if back else None)
        _check_bf16(out.reshape(B, S, H, 128), ref, floor=U32 * 128 * scale, min_equal=0.98, what=f'qk_norm_rope {kind} B={B} backward={back}')
    # the direct ABI call of trunk._rope (B = 1 per call, raw pointers) gives the same bits as the wrapper
    if B == 1:
        from arcflow_amd import _lib
        from arcflow_amd.ops import _p, _s
        y2 = torch.empty(S, D, dtype=torch.bfloat16, device='cuda')
        x2 = x.view(S, D)
        _lib.check(_lib.load().afx_qk_norm_rope_oop_bf16(_p(x2), x2.stride(0), _p(y2), y2.stride(0), _p(dy.view(S, D)), dy.stride(1), _p(w_t),
                                                          _p(w_i), _p(cos), _p(sin), 1, S, T, H, 1, _s()))
        assert torch.equal(y2, out.view(S, D))


def _gelu64(x):
    """gelu_tanh and its derivative in fp64, in the sigmoid form: 0.5 (1 + tanh u) = sigmoid(2u), 1 - tanh^2 u = 4 sigmoid(2u) sigmoid(-2u).
    (1 + tanh u itself cancels in fp64 for x < -5: the reference would be off by tens of percent in the tail.)"""
    x = x.double()
    k = (2.0 / np.pi) ** 0.5
    u = k * (x + 0.044715 * x ** 3)
    s, sm = torch.sigmoid(2 * u), torch.sigmoid(-2 * u)
    du = k * (1 + 3 * 0.044715 * x * x)
    return x * s, s + 2 * x * s * sm * du, u, du


def test_gelu_full_width(ops):
    """gelu_tanh forward and backward at 12288 columns through the column-offset views of trunk.py (gelu(Mp, out=G[:, D:]),
    gelu(Mp, dh=dG[:, D:], out=dFp[:, 3 D:])): inputs up to |x| = 9.5 and +10, exact zeros, and a band around x = -0.75 where gelu' crosses 0."""
    D, F, R = 3072, 12288, 512
    g = _gen(12288)
    Mbuf = (torch.randn(R, 7 * D, generator=g, device='cuda') * 3).clamp(-9.5, 10.0)
    Mbuf[:64, 3 * D:] = torch.rand(64, F, generator=g, device='cuda') * 0.3 - 0.9          # -0.9 .. -0.6
    Mbuf[64:72, 3 * D:] = 0.0
    Mbuf[72, 3 * D:3 * D + 4] = torch.tensor([10.0, -9.5, 9.5, -9.0], device='cuda')
    Mp = Mbuf.bfloat16()[:, 3 * D:]
    dG = (torch.randn(R, 5 * D, generator=g, device='cuda') + 0.25).bfloat16()[:, D:]
    h_ref, d_ref, u, du = _gelu64(Mp)
    Gbuf = _guarded((R, 5 * D), torch.bfloat16, 5.0)
    ops.gelu(Mp, out=Gbuf[:, D:])
    _unchanged_outside(Gbuf, 5.0, slice(None), slice(D, None), 'gelu forward')
    # forward: x sigmoid(2u) from exp2 + rcp; both within a few fp32 ulp -> covered by one bf16 ulp
    _check_bf16(Gbuf[:, D:], h_ref, what='gelu forward')
    dFp = _guarded((R, 7 * D), torch.bfloat16, 5.0)
    ops.gelu(Mp, dh=dG, out=dFp[:, 3 * D:])
    _unchanged_outside(dFp, 5.0, slice(None), slice(3 * D, None), 'gelu backward')
    # backward: the fp32 tanh form with __expf sums terms of size 1 and |x du| that cancel at gelu' = 0; each carries a few fp32 ulp, scaled
    # by (1 + |u|) through exp's argument -> floor 16 u |dh| (1 + |u|) (1 + |x du|)  (2.5e-6 |dh| at x = -0.75)
    dh = dG.double()
    floor = 16 * U32 * dh.abs() * (1 + u.abs()) * (1 + (Mp.double() * du).abs())
    _check_bf16(dFp[:, 3 * D:], dh * d_ref, floor=floor, what='gelu backward')


def test_add_scale_gate_residual_strided(ops):
    """add_scale: a alone, a + b, a per-batch gate [2, C] (rows_per_batch, gate rows read with a stride > C); gate_residual: res + gate y.
    All operands and outputs are column views of wider rows, the outputs' neighbours hold a sentinel."""
    R, C = 4608, 3072
    g = _gen(77)
    a = _strided_bf16(R, C, g, 1.0, 0.2)
    b = _strided_bf16(R, C, g, 2.0, -0.1)
    gbuf = torch.randn(2, 2 * C, generator=g, device='cuda')
    gate2 = gbuf[:, C:]
    ad, bd = a.double(), b.double()
    cases = (('a', dict(), ad, 0.0),
             ('a+b', dict(b=b), ad + bd, 0.0),
             ('a*gate', dict(gate=gate2[0]), ad * gate2[0].double(), 0.0),
             ('(a+b)*gate[batch]', dict(b=b, gate=gate2, rows_per_batch=R // 2), (ad + bd) * gate2.double().repeat_interleave(R // 2, 0),
              2 * U32 * (ad.abs() + bd.abs()) * gate2.double().abs().repeat_interleave(R // 2, 0)))
    for name, kw, ref, floor in cases:
        obuf = _guarded((R, C + 48), torch.bfloat16, 9.0)
        ops.add_scale(a, out=obuf[:, 40:40 + C], **kw)
        _unchanged_outside(obuf, 9.0, slice(None), slice(40, 40 + C), name)
        # a + b is exact in fp32 unless it cancels; the floor covers the one rounding of the gated sum in that case
        _check_bf16(obuf[:, 40:40 + C], ref, floor=floor, what=f'add_scale {name}')
    y = _strided_bf16(R, C, g, 1.0, 0.5)
    res = _strided_bf16(R, C, g, 1.0, -0.3)
    gate = torch.randn(C, generator=g, device='cuda')
    obuf = _guarded((R, C + 48), torch.bfloat16, 9.0)
    ops.gate_residual(y, gate, res, out=obuf[:, 8:8 + C])
    _unchanged_outside(obuf, 9.0, slice(None), slice(8, 8 + C), 'gate_residual')
    ref = res.double() + gate.double() * y.double()
    # res + fma-free gate * y: two fp32 roundings of terms of size |res| + |gate y| (where the sum cancels)
    _check_bf16(obuf[:, 8:8 + C], ref, floor=2 * U32 * (res.double().abs() + (gate.double() * y.double()).abs()), what='gate_residual')


def test_axpby_rows_per_sample(ops):
    """alpha[s] a + beta[s] b with B = 4 samples of 4096 x 64 values: each sample takes its own scalars."""
    g = _gen(4096)
    a = torch.randn(4, 4096, 64, generator=g, device='cuda')
    b = torch.randn(4, 4096, 64, generator=g, device='cuda') + 1.0
    al = torch.tensor([0.5, -2.0, 3.25, 1e-3], device='cuda')
    be = torch.tensor([1.5, 0.25, -1.0, 7.0], device='cuda')
    out = ops.axpby_rows(a, al, b, be)
    ta, tb = al.double()[:, None, None] * a.double(), be.double()[:, None, None] * b.double()
    # two products and one add, each rounded once in fp32
    assert bool(((out.double() - (ta + tb)).abs() <= 2 * U32 * (ta.abs() + tb.abs()) + 1e-300).all())
    wrong = al.double().flip(0)[:, None, None] * a.double() + tb            # a swapped sample order would not pass
    assert not bool(((out.double() - wrong).abs() <= 2 * U32 * (ta.abs() + tb.abs())).all())


def test_mse_sumsq_grid_stride(ops):
    """mse_loss over B x 4096 x 64 = 4 x 262144 values plus a ragged tail, sumsq over n = 3 x 2048 x 256 + 12345: the grid-stride loops
    run several times per thread; both accumulate into a non-zero start.  A single NaN / inf in the LAST element reaches sumsq's result
    (the distillation step skips on a non-finite gradient norm)."""
    grid = 2048 * 256
    g = _gen(5)
    n = 3 * grid + 12345
    p = torch.randn(n, generator=g, device='cuda') + 0.5
    t = torch.randn(n, generator=g, device='cuda') * 0.5
    sweeps = (n + grid - 1) // grid
    depth = sweeps + 6 + 2 + 2048 + 2          # serial per thread, wave levels, 4 waves, one atomic per block, start, square
    tail = slice(3 * grid, n)                 # the last sweep: only the loop's last trip covers it
    # sumsq
    x64 = p.double()
    acc = ops.sumsq(p, torch.full((1,), 3.0, device='cuda'))
    ref = 3.0 + (x64 * x64).sum()
    _check_sum(acc[0], ref, ref, depth, ref - (x64[tail] ** 2).sum(), 'sumsq')
    for bad in (float('nan'), float('inf'), float('-inf')):
        q = p.clone()
        q[-1] = bad
        v = ops.sumsq(q, torch.zeros(1, device='cuda'))[0].item()
        assert (np.isnan(v) if np.isnan(bad) else v == float('inf')), (bad, v)
    # mse_loss: loss += coef / 2 sum (p - t)^2, grad = coef (p - t)
    for shape in ((4, 4096, 64), (n,)):
        m = int(np.prod(shape))
        pp, tt = p[:m].reshape(shape), t[:m].reshape(shape)
        coef = 30.0 / m
        loss = torch.full((1,), 0.125, device='cuda')
        grad = ops.mse_loss(pp, tt, coef, loss)
        d = (pp.double() - tt.double()).flatten()
        sw = (m + grid - 1) // grid
        ref = 0.125 + 0.5 * coef * (d * d).sum()
        last = slice((sw - 1) * grid, m)
        _check_sum(loss[0], ref, ref, sw + 6 + 2 + 2048 + 4, ref - 0.5 * coef * (d[last] ** 2).sum(), f'mse {shape}')
        # grad: the fp32 difference (exact-ish: one rounding) times coef (one rounding)
        assert bool(((grad.double().flatten() - coef * d).abs() <= 2 * U32 * coef * d.abs() + 1e-300).all()), f'mse grad {shape}'


def test_cast_bf16_round_to_nearest_even(ops):
    """fp32 -> bf16 over an odd n above one grid, bit-identical to torch's round-to-nearest-even: exact ties (both parities), values just
    either side of a tie, the fp32 -> bf16 overflow edge, +-inf, NaN, fp32 and bf16 subnormals, signed zeros."""
    g = _gen(6)
    n = 2 * 2048 * 256 + 4133
    bits = torch.randint(0, 2 ** 32, (n,), generator=g, device='cuda', dtype=torch.int64)
    special = torch.tensor([0x3f808000, 0x3f818000, 0x3f808001, 0x3f807fff, 0xbf808000, 0xbf818000,     # ties to even (down / up), either side
                            0x7f7fffff, 0x7f7f8000, 0x7f7f7fff, 0xff7fffff,                              # rounds to inf / max bf16
                            0x7f800000, 0xff800000, 0x7fc00000, 0x7f800001, 0xffc00001,                  # inf, NaN (quiet / signalling)
                            0x00000001, 0x00008000, 0x00018000, 0x007fffff, 0x80008000, 0x00400000,      # subnormals, incl. ties
                            0x00000000, 0x80000000], device='cuda', dtype=torch.int64)
    bits[:special.numel()] = special
    bits[-special.numel():] = special
    x = (bits - (bits >= 2 ** 31).long() * 2 ** 32).int().view(torch.float32)
    y = ops.cast_bf16(x)
    ref = x.bfloat16()
    finite = ~torch.isnan(x)
    assert torch.equal(y[finite].view(torch.int16), ref[finite].view(torch.int16))
    assert bool(torch.isnan(y[~finite].float()).all())


def test_wrappers_reject_bad_operands_before_launch(ops):
    """The wrappers pass base pointers and row strides only: a transposed view, a wrong dtype, operands of different shapes, a strided or
    short accumulator, or a multi-row gate / scale without a matching rows_per_batch must raise -- before any kernel runs (the sentinel
    outputs and accumulators stay as they were).  So must the in-place adamw_step, adamw8bit_step, ema_lerp and cast_bf16 for an operand
    that is not on the GPU, not of the kernel's dtype, not contiguous or not of the call's length, an AdamW8bitState whose arrays do not
    match n and ceil(n / 256), a code book that is not 256 float32 entries, or a step below 1."""
    R, C = 256, 512
    g = _gen(1)
    a = torch.randn(R, C, generator=g, device='cuda').bfloat16()
    b = torch.randn(R, C, generator=g, device='cuda').bfloat16()
    acc = torch.full((2 * C,), 4.0, device='cuda')
    out = torch.full((R, C), 4.0, dtype=torch.bfloat16, device='cuda')
    gate2 = torch.randn(2, C, generator=g, device='cuda')
    w = torch.randn(C, 128, generator=g, device='cuda').bfloat16()
    x32 = torch.randn(2, C, generator=g, device='cuda')
    cos = torch.zeros(R, 64, device='cuda')
    cases = {
        'coldot transposed a': lambda: ops.coldot(a.t().contiguous().t(), b, acc[:C]),
        'coldot rows differ': lambda: ops.coldot(a, b[1:], acc[:C]),
        'coldot strided accumulator': lambda: ops.coldot(a, b, acc[::2]),
        'coldot short accumulator': lambda: ops.coldot(a, b, acc[:C - 8]),
        'colsum fp32 x': lambda: ops.colsum(a.float(), acc[:C]),
        'gemv_t bf16 x': lambda: ops.gemv_t(x32.bfloat16(), w, acc[:256].view(2, 128)),
        'gemv_t N differs': lambda: ops.gemv_t(x32[:, 1:], w, acc[:256].view(2, 128)),
        'gemv_t transposed w': lambda: ops.gemv_t(x32[:, :128], w.t(), acc[:C * 2].view(2, C)),
        'normout dmod shape': lambda: ops.normout_backward(a, b, acc[:2 * C].view(1, C, 2), R),
        'normout rows_per_batch': lambda: ops.normout_backward(a, b, acc[:2 * C].view(1, 2, C), R - 1),
        'normout_split dxn fp32': lambda: ops.normout_backward_split(a, b.float(), acc[:C], acc[C:]),
        'outer_accum batch differs': lambda: ops.outer_accum(x32, x32[:1, :128], acc[:C * 2].view(C, 2)),
        'outer_accum dW shape': lambda: ops.outer_accum(x32, x32[:, :1], acc[:C].view(1, C)),
        'gate_residual res shape': lambda: ops.gate_residual(a, gate2[0], b[:, :C - 8], out=out),
        'gate_residual [B, C] gate': lambda: ops.gate_residual(a, gate2, b, out=out),
        'add_scale [B, C] gate without rows_per_batch': lambda: ops.add_scale(a, gate=gate2, out=out),
        'add_scale rows != rows_per_batch x gate rows': lambda: ops.add_scale(a, gate=gate2, rows_per_batch=R // 2 + 1, out=out),
        'add_scale transposed b': lambda: ops.add_scale(a[:, :R], b[:R, :R].t(), out=out[:, :R]),
        'ln_modulate_backward [B, D] scale without rows_per_batch': lambda: ops.ln_modulate_backward(a, b, gate2, out=out),
        'ln_modulate_backward dres rows': lambda: ops.ln_modulate_backward(a, b, gate2[0], dres=b[1:], out=out[1:]),
        'gelu transposed out': lambda: ops.gelu(a[:, :R], out=out[:, :R].t()),
        'gelu dh dtype': lambda: ops.gelu(a, dh=b.float(), out=out),
        'qk_norm_rope bf16 cos': lambda: ops.qk_norm_rope(a.view(1, R, C)[..., :256], gate2[0, :128], gate2[1, :128], cos.bfloat16(), cos, 8,
                                                          out=out[:, :256]),
        'qk_norm_rope short out': lambda: ops.qk_norm_rope(a.view(1, R, C)[..., :256], gate2[0, :128], gate2[1, :128], cos, cos, 8,
                                                           out=out[1:, :256]),
        'sumsq strided x': lambda: ops.sumsq(x32.t(), acc[:1]),
    }
    # the in-place optimizer / EMA / cast wrappers: raw pointers and a length, so every operand must be a contiguous GPU tensor of the
    # kernel's dtype and of that length -- and never a converted copy, which would take the update and be dropped
    n8 = 512
    pw, mw, vw, gw = acc[:256], acc[256:512], acc[512:768], x32[0, :256]
    st_ok = ops.AdamW8bitState(n8, 'cuda')

    def st8(**kw):
        st = ops.AdamW8bitState(n8, 'cuda')
        for k, val in kw.items():
            setattr(st, k, val(getattr(st, k)))
        return st
    cases.update({
        'adamw_step cpu grad': lambda: ops.adamw_step(pw, gw.cpu(), mw, vw, 1e-3, 1),
        'adamw_step cpu param': lambda: ops.adamw_step(pw.cpu(), gw, mw, vw, 1e-3, 1),
        'adamw_step bf16 param': lambda: ops.adamw_step(out[0, :256], gw, mw, vw, 1e-3, 1),
        'adamw_step bf16 grad': lambda: ops.adamw_step(pw, gw.bfloat16(), mw, vw, 1e-3, 1),
        'adamw_step strided param': lambda: ops.adamw_step(acc[:512:2], gw, mw, vw, 1e-3, 1),
        'adamw_step strided grad': lambda: ops.adamw_step(pw, x32[0, ::2], mw, vw, 1e-3, 1),
        'adamw_step grad length': lambda: ops.adamw_step(pw, gw[:255], mw, vw, 1e-3, 1),
        'adamw_step short exp_avg': lambda: ops.adamw_step(pw, gw, mw[:255], vw, 1e-3, 1),
        'adamw_step long exp_avg_sq': lambda: ops.adamw_step(pw, gw, mw, acc[512:769], 1e-3, 1),
        'adamw_step step 0': lambda: ops.adamw_step(pw, gw, mw, vw, 1e-3, 0),
        'adamw8bit_step cpu param': lambda: ops.adamw8bit_step(acc[:n8].cpu(), x32[0], st_ok, 1e-3, 1),
        'adamw8bit_step bf16 param': lambda: ops.adamw8bit_step(out[0], x32[0], st_ok, 1e-3, 1),
        'adamw8bit_step strided param': lambda: ops.adamw8bit_step(acc[::2], x32[0], st_ok, 1e-3, 1),
        'adamw8bit_step grad length': lambda: ops.adamw8bit_step(acc[:n8], x32[0, 1:], st_ok, 1e-3, 1),
        'adamw8bit_step state of another n': lambda: ops.adamw8bit_step(acc[:n8 - 1], x32[0, 1:], st_ok, 1e-3, 1),
        'adamw8bit_step short codes': lambda: ops.adamw8bit_step(acc[:n8], x32[0], st8(state2=lambda t: t[:-1]), 1e-3, 1),
        'adamw8bit_step float codes': lambda: ops.adamw8bit_step(acc[:n8], x32[0], st8(state1=lambda t: t.float()), 1e-3, 1),
        'adamw8bit_step short absmax': lambda: ops.adamw8bit_step(acc[:n8], x32[0], st8(absmax1=lambda t: t[:-1]), 1e-3, 1),
        'adamw8bit_step cpu absmax': lambda: ops.adamw8bit_step(acc[:n8], x32[0], st8(absmax2=lambda t: t.cpu()), 1e-3, 1),
        'adamw8bit_step code book of 255': lambda: ops.adamw8bit_step(acc[:n8], x32[0], st8(qmap1=lambda t: t[1:]), 1e-3, 1),
        'adamw8bit_step fp64 code book': lambda: ops.adamw8bit_step(acc[:n8], x32[0], st8(qmap2=lambda t: t.double()), 1e-3, 1),
        'adamw8bit_step step 0': lambda: ops.adamw8bit_step(acc[:n8], x32[0], st_ok, 1e-3, 0),
        'ema_lerp cpu net': lambda: ops.ema_lerp(pw, gw.cpu(), 0.5),
        'ema_lerp cpu ema': lambda: ops.ema_lerp(pw.cpu(), gw, 0.5),
        'ema_lerp bf16 ema': lambda: ops.ema_lerp(out[0, :256], gw, 0.5),
        'ema_lerp strided ema': lambda: ops.ema_lerp(acc[:512:2], gw, 0.5),
        'ema_lerp net length': lambda: ops.ema_lerp(pw, gw[1:], 0.5),
        'cast_bf16 out size': lambda: ops.cast_bf16(x32[0], out=out[0, 1:]),
        'cast_bf16 fp32 out': lambda: ops.cast_bf16(x32[0], out=acc[:C]),
        'cast_bf16 cpu out': lambda: ops.cast_bf16(x32[0], out=out[0].cpu()),
        'cast_bf16 strided out': lambda: ops.cast_bf16(x32[0, :256], out=out[0, ::2]),
        'cast_bf16 bf16 x': lambda: ops.cast_bf16(a[0], out=out[0]),
        'cast_bf16 strided x': lambda: ops.cast_bf16(x32[0, ::2], out=out[0, :256]),
        'cast_bf16 cpu x': lambda: ops.cast_bf16(x32[0].cpu(), out=out[0]),
    })
    for name, call in cases.items():
        with pytest.raises(ValueError):
            call()
        torch.cuda.synchronize()
        assert bool((acc == 4.0).all()) and bool((out == 4.0).all()), f'{name}: something ran before the error'
        assert not bool(st_ok.state1.any()) and not bool(st_ok.state2.any()) and not bool(st_ok.absmax1.any()) and not bool(st_ok.absmax2.any()), \
            f'{name}: the 8-bit state was touched before the error'
