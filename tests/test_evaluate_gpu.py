"""Training-time evaluation on the GPU: ``ArcFlowDistiller.sample_student`` / ``ema_weights`` and ``Evaluator`` on the tiny engines of
tests/test_distill.py (1 double + 1 single FLUX block, D = 256, an 8 x 8 token grid, 12 text tokens), and tools/train.py --eval-interval.

Bars.  ``sample_student`` is held to the project's bar (tests/test_full_depth_parity.py): rel-L2 of the HIP latents
against the fp32 oracle (oracle/dit_ref.py forward + oracle/arcflow_ref.py analytic step on the grid of arcflow_ref.inference_sigmas)
<= 1.5 x the eager-bf16 oracle's + 2e-3, both measured here.  ``ema_weights`` and the repeated evaluation are bit-equalities.  The
Evaluator's numbers are compared with ``metrics_from_sums`` of fp64 CPU sums of the same latents: every kernel sum is within
2 n 2^-53 sum|term| of the CPU sum (tests/test_hip_sample_score_fp64.py), i.e. within a relative 2 n 2^-53 kappa with
kappa = sum|term| / |sum| (1 for the three sums of squares, >= 1 for S_ab); a metric is a quotient / square root of two sums, so its
relative error is at most the sum of theirs plus a few fp64 roundings of the host formulas: rtol = (kappa_ab + 3) 2 n 2^-53 + 8 * 2^-53.

Measured on the MI355X (rel-L2 against the fp32 oracle, hip / eager-bf16): recorded in DESIGN.md section 6.2.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = WP = 8
N = HP * WP
T = 12
FACTOR, FLOOR = 1.5, 2e-3
ENG = dict(num_double=1, num_single=1, heads=2, joint_dim=128, pooled_dim=64)
U = 2.0 ** -53


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp(min=1e-12)).item()


def _weights():
    from arcflow_amd.weights import init_arcflow_heads_from_teacher
    from oracle import dit_ref as D
    cfg = D.FluxCfg(num_layers=1, num_single_layers=1, heads=2, joint_dim=128, pooled_dim=64)
    w = D.make_flux_weights(cfg, seed=7, teacher_head=True)
    for k in [k for k in w if k.startswith('proj_out_')]:
        del w[k]
    w = init_arcflow_heads_from_teacher(w, generator=torch.Generator().manual_seed(1))       # the student's means start on the teacher's velocity
    g = torch.Generator().manual_seed(2)
    w['proj_out_logweights.weight'] = (torch.randn(64, 256, generator=g) * 0.05).bfloat16()
    w['proj_out_loggamma.weight'] = (torch.randn(60, 256, generator=g) * 0.05).bfloat16()
    return cfg, w


def _cond(B, seed=3):
    g = torch.Generator().manual_seed(seed)
    return dict(prompt_embeds=(torch.randn(B, T, 128, generator=g) * 0.5).bfloat16().cuda(),
                pooled=(torch.randn(B, 64, generator=g) * 0.5).bfloat16().cuda(), hp=HP, wp=WP)


def _noise(B, seed=4):
    return torch.randn(B, N, 64, generator=torch.Generator().manual_seed(seed))


def _distiller(lora_rank=0, steps=0):
    """A tiny distiller, optionally ``steps`` training steps in.  EMA from iteration 0 with gamma 1 (beta = (1 - 1/t)^2: 0, 0.25, 0.44), so that
    after three steps it differs from the live weights by far more than a bf16 rounding; lr 5e-4 without warm-up moves every weight by
    ~1.5e-3 (several per cent of its size)."""
    from arcflow_amd.train import ArcFlowDistiller, DistillConfig
    cfg, w = _weights()
    dc = DistillConfig(num_decay_iters=4, warmup_iters=0, grad_clip_begin_iter=10 ** 9, ema_start_iter=0, ema_gamma=1.0, lora_rank=lora_rank, lr=5e-4)
    d = ArcFlowDistiller('flux', dict(ENG), w, dc)
    rng = torch.Generator(device='cuda').manual_seed(11)
    cond = _cond(2)
    for _ in range(steps):
        assert not d.train_step(cond, 2, rng=rng)['skipped']
    return d


@pytest.fixture(scope='module')
def dists():
    cache = {}

    def get(lora_rank, steps):
        if (lora_rank, steps) not in cache:
            cache[(lora_rank, steps)] = _distiller(lora_rank, steps)
        return cache[(lora_rank, steps)]
    return get


def _oracle_weights(d, ema=False):
    """The oracle's fp32 weights of the distiller's CURRENT student: trainable_state_dict() + the trunk's merged_state()."""
    _, w = _weights()
    wt = {k: v.float() for k, v in w.items()}
    wt.update({k: v.float().cpu() for k, v in d.trainable_state_dict(ema=ema).items()})
    if d.trunk is not None:
        assert not ema
        for name, m in d.trunk.merged_state().items():
            wt[name + '.weight'] = m.float().cpu()
    return wt


def _oracle_roll(wt, cond, noise, nfe, ratio, guidance=3.5):
    """-> (fp32 oracle latents, eager-bf16 oracle latents) of the student's nfe-step roll."""
    from oracle import arcflow_ref as R
    from oracle import dit_ref as D
    cfg, _ = _weights()
    pe, pooled = cond['prompt_embeds'].float().cpu(), cond['pooled'].float().cpu()
    B = noise.shape[0]
    sig, _ = R.inference_sigmas(nfe, 128, ratio, 3.2)

    def roll():
        x = noise.clone()
        for i in range(nfe):
            m, lw, lg = D.flux_forward(wt, cfg, x.bfloat16().float(), pe, pooled, torch.full((B,), sig[i]), torch.full((B,), guidance), HP, WP)
            x = R.momentum_step_packed(x, m, lw, lg, sig[i], sig[i], sig[i + 1])
        return x
    with torch.no_grad():
        ref = roll()
        with D.eager_bf16():
            eager = roll()
    return ref, eager


def _assert_bar(tag, hip, ref, eager):
    e_hip, e_eager = rel_l2(hip, ref), rel_l2(eager, ref)
    print(f'{tag}: student latents rel-L2 vs fp32 oracle: hip {e_hip:.3e}  eager-bf16 {e_eager:.3e}')
    assert hip.dtype == torch.float32 and tuple(hip.shape) == tuple(ref.shape) and torch.isfinite(hip).all()
    assert e_hip <= FACTOR * e_eager + FLOOR, (e_hip, e_eager)


@pytest.mark.parametrize('ratio', [1.0, 0.5])
@pytest.mark.parametrize('nfe', [1, 2])
def test_sample_student_against_fp32_and_eager_bf16_oracles(dists, nfe, ratio):
    d = dists(0, 0)
    cond, noise = _cond(2), _noise(2)
    hip = d.sample_student(cond, noise.cuda(), nfe=nfe, timestep_ratio=ratio)
    ref, eager = _oracle_roll(_oracle_weights(d), cond, noise, nfe, ratio)
    _assert_bar(f'nfe={nfe} timestep_ratio={ratio}', hip, ref, eager)
    if nfe == 2 and ratio == 1.0:          # the defaults are the training values
        assert torch.equal(d.sample_student(cond, noise.cuda()), hip)
    with pytest.raises(ValueError):
        d.sample_student(cond, noise[:, :32].cuda())


@pytest.mark.parametrize('lora_rank', [0, 8])
def test_sample_student_after_training_matches_oracle_on_current_weights(dists, lora_rank):
    d = dists(lora_rank, 3)
    assert d.iteration == 3 and (lora_rank == 0) == (d.trunk is None)
    cond, noise = _cond(2, seed=21), _noise(2, seed=22)
    hip = d.sample_student(cond, noise.cuda())
    ref, eager = _oracle_roll(_oracle_weights(d), cond, noise, 2, 1.0)
    _assert_bar(f'lora_rank={lora_rank} after 3 steps', hip, ref, eager)
    stale, _ = _oracle_roll({k: v.float() for k, v in _weights()[1].items()}, cond, noise, 2, 1.0)
    print(f'lora_rank={lora_rank}: the initial weights are {rel_l2(stale, ref):.3e} away')
    assert rel_l2(hip, ref) < rel_l2(hip, stale)                       # ... and it IS the trained student that was sampled
    # B = 5 runs as micro-batches of 4 + 1 with the same per-sample numbers
    cond5, noise5 = _cond(5, seed=23), _noise(5, seed=24).cuda()
    take = lambda c, a, b: {k: (v[a:b] if isinstance(v, torch.Tensor) else v) for k, v in c.items()}      # noqa: E731
    out5 = d.sample_student(cond5, noise5)
    assert torch.equal(out5, torch.cat([d.sample_student(take(cond5, 0, 4), noise5[:4]), d.sample_student(take(cond5, 4, 5), noise5[4:])]))


def _state(d):
    s = dict(params=d.params.clone(), ema=d.ema.clone(), w_head=d.w_head.clone(), b_head=d.b_head.clone(), w_no=d.w_no.clone(), b_no=d.b_no.clone(),
             iteration=d.iteration, opt_steps=d.opt_steps)
    if d.exp_avg is not None:
        s.update(exp_avg=d.exp_avg.clone(), exp_avg_sq=d.exp_avg_sq.clone())
    if d.trunk is not None:
        for name in ('a16', 'b16', 'at16', 'bt16', 'a16p', 'at16p', 'wcat', 'wtcat'):
            for k, v in getattr(d.trunk, name).items():
                s[f'trunk.{name}.{k}'] = v.clone()
    return s


def _assert_state_equal(d, before):
    now = _state(d)
    assert set(now) == set(before)
    for k, v in before.items():
        assert torch.equal(now[k], v) if torch.is_tensor(v) else now[k] == v, k


@pytest.mark.parametrize('lora_rank', [0, 8])
def test_ema_weights_exchange_restores_every_buffer_bit_for_bit(dists, lora_rank):
    d = dists(lora_rank, 3)
    assert not torch.equal(d.params, d.ema)
    cond, noise = _cond(2, seed=31), _noise(2, seed=32).cuda()
    live = d.sample_student(cond, noise)
    x, sig = noise, torch.full((2,), 0.7, device='cuda')
    fwd_before = d.student_forward(x, sig, cond).means.clone()
    before = _state(d)
    with d.ema_weights() as inside:
        assert inside is d and torch.equal(d.params, before['ema']) and torch.equal(d.ema, before['params'])
        assert not torch.equal(d.w_head, before['w_head'])
        in_ctx = d.sample_student(cond, noise)
    _assert_state_equal(d, before)
    with pytest.raises(RuntimeError, match='boom'):
        with d.ema_weights():
            raise RuntimeError('boom')
    _assert_state_equal(d, before)
    assert torch.equal(d.student_forward(x, sig, cond).means, fwd_before)           # with LoRA: the merged weights were rebuilt to the same bits
    assert torch.equal(d.sample_student(cond, noise), live)
    via_flag = d.sample_student(cond, noise, ema=True)
    _assert_state_equal(d, before)
    assert torch.equal(via_flag, in_ctx) and not torch.equal(via_flag, live)
    # a second distiller with the EMA state loaded as its live parameters samples the same bits
    other = _distiller(lora_rank, 0)
    other.params.copy_(d.ema)
    other._sync_working_copies()
    if other.trunk is not None:
        other.trunk.refresh()
    assert torch.equal(other.sample_student(cond, noise), via_flag)
    if lora_rank == 0:          # and the oracle on the EMA state dict agrees
        ref, eager = _oracle_roll(_oracle_weights(d, ema=True), cond, noise.cpu(), 2, 1.0)
        _assert_bar('ema weights', via_flag, ref, eager)


def _cpu_metrics(student, teacher):
    from arcflow_amd.train.evaluate import metrics_from_sums
    a, b = student.double().cpu().flatten(1), teacher.double().cpu().flatten(1)
    sums = torch.stack([((a - b) ** 2).sum(1), (a * a).sum(1), (b * b).sum(1), (a * b).sum(1)], 1)
    kappa = ((a * b).abs().sum(1) / (a * b).sum(1).abs()).max().item()
    return metrics_from_sums(sums, a.shape[1]), kappa


def test_evaluator_scores_caches_the_teacher_and_leaves_the_generators_alone(dists):
    from arcflow_amd.train import Evaluator
    d = dists(0, 3)
    conds = [_cond(2, seed=41), _cond(1, seed=42)]
    rng = torch.Generator(device='cuda').manual_seed(5)
    torch.rand(3, device='cuda', generator=rng)
    g_cpu, g_cuda, g_rng = torch.get_rng_state(), torch.cuda.get_rng_state(), rng.get_state()
    calls = []
    real = d.teacher.forward

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    d.teacher.forward = counting
    try:
        ev = Evaluator(d, conds, seed=9, teacher_steps=4)
        before = _state(d)
        first = ev.evaluate()
        n_first = len(calls)
        second = ev.evaluate()
        n_second = len(calls) - n_first
    finally:
        del d.teacher.forward
    assert n_first == 2 * 4 and n_second == 0                          # 2 conditions x 4 teacher steps (no true CFG), then the kept latents
    _assert_state_equal(d, before)
    assert torch.equal(torch.get_rng_state(), g_cpu) and torch.equal(torch.cuda.get_rng_state(), g_cuda) and torch.equal(rng.get_state(), g_rng)
    strip = lambda r: {k: v for k, v in r.items() if k != 'seconds'}       # noqa: E731
    assert strip(first) == strip(second)                                # bit-identical: python floats compare exactly
    assert first['seconds'] > 0 and second['seconds'] > 0 and first['iteration'] == 3
    keys = ('latent_mse', 'latent_rel_l2', 'latent_cosine')
    assert set(first) == {'iteration', 'seconds'} | set(keys) | {k + '_mean' for k in keys}             # no vae: no image metrics
    assert all(len(first[k]) == 3 and all(v == v and abs(v) != float('inf') for v in first[k]) for k in keys)
    # the noise is the private generator's, per condition
    for i, c in enumerate(conds):
        want = torch.randn(c['prompt_embeds'].shape[0], N, 64, device='cuda', generator=torch.Generator(device='cuda').manual_seed(9 + i))
        assert torch.equal(ev.noise[i], want)
    # the numbers: metrics_from_sums of fp64 CPU sums of the same latents (a = the EMA student, b = the teacher), within the kernel bound
    got = {k: [] for k in keys}
    rtol = 0.0
    for i, c in enumerate(conds):
        stu = d.sample_student(c, ev.noise[i], ema=True)
        tea = d.sample_teacher(c, ev.noise[i], num_steps=4)
        assert torch.equal(tea, ev.teacher_latents[i])
        m, kappa = _cpu_metrics(stu, tea)
        rtol = max(rtol, (kappa + 3) * 2 * N * 64 * U + 8 * U)
        for k in keys:
            got[k] += m[k[len('latent_'):]].tolist()
    for k in keys:
        worst = max(abs(x - y) / abs(y) for x, y in zip(first[k], got[k]))
        print(f'{k}: {first[k]}  max rel diff to the CPU {worst:.3e} (rtol {rtol:.3e})')
        assert worst <= rtol, (k, worst, rtol)
        assert abs(first[k + '_mean'] - sum(got[k]) / 3) <= rtol * abs(first[k + '_mean']) + 4 * U * abs(first[k + '_mean'])
    # use_ema=False scores the live weights: different numbers
    live = Evaluator(d, conds, seed=9, teacher_steps=4, use_ema=False).evaluate()
    assert live['latent_rel_l2'] != first['latent_rel_l2']


def test_evaluator_orientation_teacher_like_heads_score_better_than_random_heads(dists):
    """Sign and orientation: the fresh student's means are copies of the teacher's velocity head, so its samples must be closer to the
    teacher's than those of a student whose heads are re-randomised -- in rel-L2 relative to the TEACHER (b)."""
    from arcflow_amd.train import Evaluator
    d = dists(0, 0)
    conds = [_cond(2, seed=51)]
    good = Evaluator(d, conds, seed=1, teacher_steps=8, use_ema=False).evaluate()
    keep = d.params.clone()
    try:
        g = torch.Generator().manual_seed(52)
        rows = d.K * d.C + d.K * d.L + (d.K - 1) * d.L                  # means | logweights | loggamma rows (the rest of head_n is padding)
        d._view(d.params, 0).view(d.head_n, d.D)[:rows].copy_((torch.randn(rows, d.D, generator=g) * 0.05).cuda())
        d._sync_working_copies()
        ev = Evaluator(d, conds, seed=1, teacher_steps=8, use_ema=False)
        bad = ev.evaluate()
        stu, tea = d.sample_student(conds[0], ev.noise[0]), ev.teacher_latents[0]
    finally:
        d.params.copy_(keep)
        d._sync_working_copies()
    print(f'latent_rel_l2: teacher-copied heads {good["latent_rel_l2"]}  random heads {bad["latent_rel_l2"]}')
    assert all(x < y for x, y in zip(good['latent_rel_l2'], bad['latent_rel_l2']))
    assert good['latent_cosine_mean'] > bad['latent_cosine_mean']
    # relative to the teacher's norm, not the student's
    to_teacher = [rel_l2(stu[i], tea[i]) for i in range(2)]
    to_student = [rel_l2(tea[i], stu[i]) for i in range(2)]
    assert all(abs(x - y) <= 1e-9 * y for x, y in zip(bad['latent_rel_l2'], to_teacher))
    assert any(abs(x - y) > 1e-5 * y for x, y in zip(bad['latent_rel_l2'], to_student))          # (the two norms differ, if not by much: |stu| ~ |tea|)


def test_evaluator_image_metrics_through_the_vae_path(dists):
    """With a decoder the images are scored through transform=1.  A stand-in decoder (a fixed reshape of the packed latents to bf16
    [B, 1, hp*wp, 64], scaled) keeps the test on the Evaluator's plumbing; the VAE kernels have their own tests."""
    from arcflow_amd.train import Evaluator
    from arcflow_amd.train.evaluate import metrics_from_sums

    class Decoder:
        def decode_packed(self, latents, hp, wp):
            return (latents * 1.5).to(torch.bfloat16).view(latents.shape[0], 1, hp * wp, 64)
    d = dists(0, 3)
    conds = [_cond(2, seed=61)]
    ev = Evaluator(d, conds, seed=2, teacher_steps=4, vae=Decoder())
    res = ev.evaluate()
    assert len(res['image_psnr']) == 2 and len(res['image_mse']) == 2 and 'image_psnr_mean' in res and 'latent_mse_mean' in res
    f = lambda v: ((v * 1.5).to(torch.bfloat16).float() / 2 + 0.5).clamp(0, 1).double().cpu().flatten(1)      # noqa: E731
    a, b = f(d.sample_student(conds[0], ev.noise[0], ema=True)), f(ev.teacher_latents[0])
    assert ((a == 0) | (a == 1)).double().mean().item() > 0.05                # the clamp is exercised
    sums = torch.stack([((a - b) ** 2).sum(1), (a * a).sum(1), (b * b).sum(1), (a * b).sum(1)], 1)
    want = metrics_from_sums(sums, N * 64, data_range=1.0)
    rtol = 4 * 2 * N * 64 * U + 8 * U                                         # [0, 1] values: every sum has kappa = 1
    assert all(abs(x - y) <= rtol * abs(y) for x, y in zip(res['image_mse'], want['mse'].tolist()))
    assert all(abs(x - y) <= 10 * rtol for x, y in zip(res['image_psnr'], want['psnr'].tolist()))        # psnr = -10 log10(mse): an absolute (10 / ln 10) rtol
    assert all(0 < v < 100 for v in res['image_psnr'])


def test_train_cli_writes_eval_lines_and_leaves_a_run_without_the_flag_alone(tmp_path):
    """tools/train.py --synthetic --iters 4 --eval-interval 2: three lines in eval.jsonl (iterations 0, 2, 4), finite metrics; without the
    flag no such file.  The evaluation draws nothing from the training generator and restores every buffer bit for bit, so both runs train
    on the same draws from the same weights.  The losses are compared to 1e-5 relative on the first iteration (the loss is accumulated in
    fp32 with atomics: the order of the additions is not fixed, a few 2^-24 relative) and to 1e-3 on the later ones (the adapters' modulation
    gradients are summed with float atomics too, and the 8-bit optimizer state quantises what they feed): two runs of the SAME command line
    are not bit-identical either."""
    from tests.test_train_frontend import _TINY_CFG
    cfgp = tmp_path / 'tiny.py'
    cfgp.write_text(_TINY_CFG + "eval_interval = 2\ntest_cfg = dict(nfe=2, timestep_ratio=1.0, total_substeps=128)\n")
    base = [sys.executable, os.path.join(ROOT, 'tools', 'train.py'), str(cfgp), '--synthetic', '--latent-tokens', '8', '8', '--iters', '4']
    runs = {}
    for tag, extra in (('eval', ['--eval-interval', '2', '--eval-teacher-steps', '4']), ('plain', [])):
        work = tmp_path / tag
        r = subprocess.run(base + ['--work-dir', str(work)] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        logs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{')]
        assert [l['iter'] for l in logs] == [1, 2, 3, 4]
        runs[tag] = (work, logs, r.stdout)
    work, logs, out = runs['eval']
    lines = [json.loads(l) for l in open(work / 'eval.jsonl')]
    assert [l['iteration'] for l in lines] == [0, 2, 4]
    for l in lines:
        assert len(l['latent_rel_l2']) == 2 and l['seconds'] > 0                        # samples_per_gpu = 2, one batch
        for k in ('latent_mse', 'latent_rel_l2', 'latent_cosine'):
            assert all(v == v and abs(v) != float('inf') for v in l[k] + [l[k + '_mean']]), (k, l)
    assert out.count('[eval] iter') == 3
    assert lines[0]['latent_rel_l2'] != lines[2]['latent_rel_l2']                        # training moved the (EMA) student
    pwork, plogs, pout = runs['plain']
    assert not (pwork / 'eval.jsonl').exists() and '[eval]' not in pout
    assert abs(plogs[0]['loss'] - logs[0]['loss']) <= 1e-5 * abs(plogs[0]['loss']) + 1e-6, (plogs[0], logs[0])          # (+ the 6 printed decimals)
    for a, b in zip(plogs[1:], logs[1:]):
        assert abs(a['loss'] - b['loss']) <= 1e-3 * abs(a['loss']) + 1e-6, (a, b)
