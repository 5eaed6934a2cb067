"""The timestep-embedder LoRA pair of the training trunk (LoraTrunk.temb_forward / temb_backward: gemv, transposed gemv and rank-B
outer-product kernels) at D = 3072 against fp64 autograd: sincos(1000 sigma) -> Linear -> SiLU -> Linear with the branch B A dropout(.)
on both linears, the masks read back from the device as the trunk draws them (`_keep_scale`).  The whole-step tests see this pair only
through one rel-L2 per tensor at D = 256 (test_distill.py, < 8e-2).

Judged: the output per element (error over the RMS of the sample's row), dA1, dB1, dA2, dB2 per row and per column (rel-L2).  Everything
on this path is fp32 arithmetic on bf16 weights, so the yardstick here is an FP32 torch evaluation of the same formula on the device --
not the eager-bf16 evaluation of the block tests: in every group the trunk's worst value is at most 1.5 x the fp32 evaluation's worst.
A column of dA whose input the mask dropped in every sample is exactly zero in the reference; there the trunk's must be exactly zero
too, and the column has no quotient.

Cases: both families (FLUX rounds 1000 t to bf16 a second time), B in {1, 4}, p in {0, 0.05}.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

D_MODEL, RANK, BAR, SEED = 3072, 256, 1.5, 7654321
SIGMAS = [0.7619, 1.0, 0.3, 0.05]
_DISTS = {}


def _dist(family):
    if family not in _DISTS:
        from arcflow_amd.train import ArcFlowDistiller, DistillConfig
        from oracle import dit_ref
        if family == 'flux':
            cfg = dit_ref.FluxCfg(num_layers=1, num_single_layers=1)
            w = dit_ref.make_flux_weights(cfg, seed=51, teacher_head=True, device='cuda')
            arch = dict(num_double=1, num_single=1)
        else:
            cfg = dit_ref.QwenCfg(num_layers=1)
            w = dit_ref.make_qwen_weights(cfg, seed=52, device='cuda')
            w['proj_out.weight'] = torch.zeros(64, D_MODEL, dtype=torch.bfloat16, device='cuda')
            w['proj_out.bias'] = torch.zeros(64, dtype=torch.bfloat16, device='cuda')
            arch = dict(num_double=1, joint_dim=cfg.joint_dim)
        dc = DistillConfig(num_decay_iters=4, warmup_iters=0, grad_clip_begin_iter=10 ** 9, ema_start_iter=0, lora_rank=RANK, lora_dropout=0.05)
        dist = ArcFlowDistiller(family, arch, w, dc)
        tr = dist.trunk
        g = torch.Generator(device='cuda').manual_seed(53)
        for sp in tr.specs:
            tr.B(sp).copy_(torch.randn(sp.out_f, RANK, generator=g, device='cuda') * 0.02)
        tr.refresh()
        _DISTS[family] = dist
    return _DISTS[family]


def _reference(tr, sigma, dtemb, k1, k2, dt):
    """(y, dA1, dB1, dA2, dB2) by autograd in dtype dt, following temb_forward's docstring."""
    sp1, sp2 = tr._spec('temb.t.l1'), tr._spec('temb.t.l2')
    t = sigma.float().bfloat16().float() * 1000.0                 # the reference's explicit casts of the timestep (dit_ref.cond_cast)
    if tr.family == 'flux':
        t = t.bfloat16().float()
    freqs = torch.exp(-math.log(10000.0) * torch.arange(128, dtype=dt, device='cuda') / 128.0)
    ang = t.to(dt)[:, None] * freqs[None]
    s = torch.cat([ang.cos(), ang.sin()], dim=1)
    W1, W2 = tr.base['temb.t.l1'].to(dt), tr.base['temb.t.l2'].to(dt)
    b1, b2 = tr.packed['temb.t.l1.bias'].to(dt), tr.packed['temb.t.l2.bias'].to(dt)
    A1, B1, A2, B2 = (x.to(dt).clone().requires_grad_(True) for x in (tr.a16[sp1.name], tr.b16[sp1.name], tr.a16[sp2.name], tr.b16[sp2.name]))
    sd = s if k1 is None else s * k1.to(dt)
    u = s @ W1.T + b1 + (sd @ A1.T) @ B1.T
    h = torch.nn.functional.silu(u)
    hd = h if k2 is None else h * k2.to(dt)
    y = h @ W2.T + b2 + (hd @ A2.T) @ B2.T
    g = torch.autograd.grad((y * dtemb.to(dt)).sum(), [A1, B1, A2, B2])
    return dict(y=y.detach().double(), dA1=g[0].double(), dB1=g[1].double(), dA2=g[2].double(), dB2=g[3].double())


def _errors(got, ref, exact_zero_of=None):
    e = {}
    err = (got['y'].double() - ref['y']).abs()
    rms = ref['y'].pow(2).mean(dim=1).sqrt()
    assert bool((rms > 0).all())
    for b in range(err.shape[0]):
        e[f'y sample {b}'] = err[b] / rms[b]
    for k in ('dA1', 'dB1', 'dA2', 'dB2'):
        d = got[k].double() - ref[k]
        for axis, dim in (('rows', 1), ('cols', 0)):
            den = ref[k].norm(dim=dim)
            live = den > 0
            assert live.any()
            if not live.all():                # masked in every sample: exact zeros on both sides
                assert k in ('dA1', 'dA2') and axis == 'cols', (k, axis)
                assert not got[k].double().index_select(1, (~live).nonzero().flatten()).any(), k
            e[f'{k} {axis}'] = d.norm(dim=dim)[live] / den[live]
    return e


@pytest.mark.parametrize('p', [0.0, 0.05])
@pytest.mark.parametrize('B', [1, 4])
@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_temb_pair_forward_and_backward_vs_fp64(family, B, p):
    dist = _dist(family)
    tr = dist.trunk
    sp1, sp2 = tr._spec('temb.t.l1'), tr._spec('temb.t.l2')
    tr.p_drop, tr.seed = p, SEED
    g = torch.Generator(device='cuda').manual_seed(60 + B)
    sigma = torch.tensor(SIGMAS[:B], device='cuda')
    dtemb = torch.randn(B, D_MODEL, generator=g, device='cuda')
    y = tr.temb_forward(sigma)
    grads = torch.zeros_like(dist.grad)
    tr.temb_backward(dtemb, grads)
    torch.cuda.synchronize()
    got = dict(y=y, dA1=tr.A(sp1, grads), dB1=tr.B(sp1, grads), dA2=tr.A(sp2, grads), dB2=tr.B(sp2, grads))
    assert not grads[:sp1.off_a].any() and not grads[sp2.off_b + sp2.out_f * RANK:].any()       # nothing but the pair
    k1, k2 = tr._keep_scale(sp1, B, 256), tr._keep_scale(sp2, B, D_MODEL)
    assert (k1 is None) == (p == 0.0)
    if p > 0:
        assert 0 < (k2 == 0).float().mean().item() < 3 * p
    ref = _reference(tr, sigma, dtemb, k1, k2, torch.float64)
    f32 = _reference(tr, sigma, dtemb, k1, k2, torch.float32)
    if family == 'flux':                      # the second rounding is not a no-op for these timesteps
        assert (sigma.bfloat16().float() * 1000).bfloat16().float().ne(sigma.bfloat16().float() * 1000).any()
    hip, base = _errors(got, ref), _errors(f32, ref)
    bad, ratios = [], {}
    for grp, h in hip.items():
        hmax, emax = h.max().item(), base[grp].max().item()
        ratios[grp] = hmax / emax
        if not hmax <= BAR * emax:
            bad.append(f'{grp} {int(h.argmax())}: error {hmax:.3e} > {BAR} x {emax:.3e}, the largest of the fp32 evaluation in this group')
    print(f'{family} B={B} p={p}: hip max / fp32 max ' + ' '.join(f'{k.replace(" ", "/")}={v:.2f}' for k, v in ratios.items()))
    assert not bad, f'{family} B={B} p={p}: ' + '; '.join(bad)
