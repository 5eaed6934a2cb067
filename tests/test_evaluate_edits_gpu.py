"""Scoring edits in training-time evaluation, on the tiny distiller of tests/test_evaluate_gpu.py (its builders are imported, not copied):
``ArcFlowDistiller.sample_student(x0=, mask=, strength=)``, ``Evaluator(edits=...)`` and ``tools/train.py --eval-edits``.

The sampler's properties are bit-equalities (the blend kernel returns x for m = 1, the source for m = 0 and the noise at sigma 1 bit for
bit).  The Evaluator's edit numbers are compared with ``masked_metrics_from_sums`` of fp64 CPU sums of the same latents: every kernel sum
is within 2 n 2^-53 sum|term| of the CPU sum (tests/test_hip_sample_score_masked_fp64.py), a metric is a quotient / square root of two
sums, so rtol = (kappa_ab + 3) 2 n 2^-53 + 8 * 2^-53 as in tests/test_evaluate_gpu.py.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests.test_evaluate_gpu import HP, N, ROOT, U, WP, _assert_state_equal, _cond, _distiller, _noise, _state

pytestmark = pytest.mark.gpu

EDIT_LATENT = ('edit_latent_mse', 'edit_latent_rel_l2', 'edit_latent_cosine', 'edit_keep_latent_mse')
EDIT_IMAGE = ('edit_image_psnr', 'edit_image_mse', 'edit_keep_image_psnr', 'edit_image_ssim', 'edit_keep_image_ssim')


@pytest.fixture(scope='module')
def dist():
    return _distiller(0, 3)


def _token_mask(B, seed):
    from arcflow_amd.schedule import mask_to_tokens
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(B, 1, 16 * HP, 16 * WP, generator=g) < 0.02).float()          # sparse pixels: about 72 % of the latent pixels repaint under 'max'
    tok = mask_to_tokens(m, HP, WP, 'max')
    assert 0.2 < tok.mean().item() < 0.9
    return tok.cuda()


def test_sample_student_edit_reduces_to_the_plain_sampler_and_to_the_source(dist):
    d = dist
    cond, noise = _cond(2, seed=71), _noise(2, seed=72).cuda()
    x0 = (_noise(2, seed=73) * 0.8).cuda()
    plain = d.sample_student(cond, noise)
    assert torch.equal(d.sample_student(cond, noise, x0=x0, strength=1.0), plain)          # sigma_0 = 1: the start IS the noise, the grid the plain one
    img2img = d.sample_student(cond, noise, x0=x0, strength=0.7)
    assert not torch.equal(img2img, plain) and torch.isfinite(img2img).all()
    ones, zeros = torch.ones(2, N, 4, device='cuda'), torch.zeros(1, N, 4, device='cuda')
    assert torch.equal(d.sample_student(cond, noise, x0=x0, mask=ones, strength=0.7), img2img)          # everything repaints: no mask
    assert torch.equal(d.sample_student(cond, noise, x0=x0, mask=zeros, strength=0.7), x0)              # nothing repaints: the source, re-imposed at sigma 0
    tok = _token_mask(2, 74)
    part = d.sample_student(cond, noise, x0=x0, mask=tok, strength=0.7)
    w = tok[:, :, None, :].expand(2, N, 16, 4).reshape(2, N, 64)                                         # element e of a token reads m[token, e & 3]
    assert torch.equal(part[w == 0], x0[w == 0]) and not torch.equal(part[w == 1], x0[w == 1])
    on_ema = d.sample_student(cond, noise, x0=x0, mask=tok, strength=0.7, ema=True)
    with d.ema_weights():
        assert torch.equal(d.sample_student(cond, noise, 2, 1.0, False, x0, tok, 0.7), on_ema)          # positionally, after `ema`
    assert not torch.equal(on_ema, part) and torch.equal(on_ema[w == 0], x0[w == 0])
    with pytest.raises(ValueError, match='x0'):
        d.sample_student(cond, noise, mask=tok)
    with pytest.raises(ValueError, match='strength'):
        d.sample_student(cond, noise, strength=0.5)
    with pytest.raises(ValueError):
        d.sample_student(cond, noise, x0=x0, strength=0.0)
    with pytest.raises(ValueError):
        d.sample_student(cond, noise, x0=x0[:, :32], strength=0.5)
    # B = 5 runs as micro-batches of 4 + 1 with the same per-sample numbers, the mask sliced or shared
    cond5, noise5, x5, tok5 = _cond(5, seed=75), _noise(5, seed=76).cuda(), (_noise(5, seed=77) * 0.8).cuda(), _token_mask(5, 78)
    take = lambda c, a, b: {k: (v[a:b] if isinstance(v, torch.Tensor) else v) for k, v in c.items()}      # noqa: E731
    out5 = d.sample_student(cond5, noise5, x0=x5, mask=tok5, strength=0.6)
    assert torch.equal(out5, torch.cat([d.sample_student(take(cond5, 0, 4), noise5[:4], x0=x5[:4], mask=tok5[:4], strength=0.6),
                                        d.sample_student(take(cond5, 4, 5), noise5[4:], x0=x5[4:], mask=tok5[4:], strength=0.6)]))
    assert torch.equal(d.sample_student(cond5, noise5, x0=x5, mask=tok5[:1], strength=0.6)[4],
                       d.sample_student(take(cond5, 4, 5), noise5[4:], x0=x5[4:], mask=tok5[:1], strength=0.6)[0])


class _Decoder:
    """A stand-in decoder at the mask's resolution: the packed latents as a 64 x 64 plane, every value repeated 2 x 2, scaled, bf16."""
    def decode_packed(self, latents, hp, wp):
        img = (latents * 1.5).to(torch.bfloat16).view(latents.shape[0], 1, hp * wp, 64)
        return img.repeat_interleave(16 * hp // (hp * wp), 2).repeat_interleave(16 * wp // 64, 3)


def _strip(r):
    return {k: v for k, v in r.items() if k != 'seconds'}


def test_evaluator_without_edits_is_what_it_was(dist):
    from arcflow_amd.train import Evaluator
    conds = [_cond(2, seed=81)]
    base = Evaluator(dist, conds, seed=9, teacher_steps=4, vae=_Decoder()).evaluate()
    none = Evaluator(dist, conds, seed=9, teacher_steps=4, vae=_Decoder(), edits=None).evaluate()
    assert _strip(base) == _strip(none) and not any(k.startswith('edit_') for k in none)
    assert set(base) == {'iteration', 'seconds'} | {k + s for k in ('latent_mse', 'latent_rel_l2', 'latent_cosine', 'image_psnr', 'image_mse', 'image_ssim')
                                                    for s in ('', '_mean')}


def test_evaluator_scores_the_box_edit_caches_the_teacher_and_leaves_the_state_alone(dist):
    from arcflow_amd.schedule import mask_to_tokens
    from arcflow_amd.train import Evaluator
    from arcflow_amd.train.evaluate import edit_mask, masked_metrics_from_sums
    d = dist
    conds = [_cond(2, seed=91), _cond(1, seed=92)]
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
        ev = Evaluator(d, conds, seed=9, teacher_steps=4, edits=dict(mask='box', strength=0.8))
        before = _state(d)
        first = ev.evaluate()
        n_first = len(calls)
        second = ev.evaluate()
        n_second = len(calls) - n_first
    finally:
        del d.teacher.forward
    # 2 conditions x (4 plain teacher steps + the 4 steps a strength of 0.8 leaves of them: int(4 - 3.2) = 0 are cut), then the kept latents
    assert n_first == 2 * (4 + 4) and n_second == 0
    _assert_state_equal(d, before)                                      # params, ema, the moments and the working copies, bit for bit
    assert torch.equal(torch.get_rng_state(), g_cpu) and torch.equal(torch.cuda.get_rng_state(), g_cuda) and torch.equal(rng.get_state(), g_rng)
    assert _strip(first) == _strip(second)
    plain = Evaluator(d, conds, seed=9, teacher_steps=4).evaluate()
    assert {k: v for k, v in _strip(first).items() if not k.startswith('edit_')} == _strip(plain)          # the plain keys and values are untouched
    assert set(first) - set(plain) == {k + s for k in EDIT_LATENT for s in ('', '_mean')}                  # no vae: no image keys
    assert all(len(first[k]) == 3 and all(v == v and abs(v) != float('inf') for v in first[k]) for k in EDIT_LATENT)
    assert first['edit_keep_latent_mse'] == [0.0, 0.0, 0.0] and all(v > 0 for v in first['edit_latent_mse'])          # both samplers re-impose x0 at sigma 0
    # the edit noise is the second private generator's, the source the teacher's own text-to-image latents, the token mask the box's
    got = {k: [] for k in EDIT_LATENT}
    rtol = 0.0
    for i, c in enumerate(conds):
        B = c['prompt_embeds'].shape[0]
        want = torch.randn(B, N, 64, device='cuda', generator=torch.Generator(device='cuda').manual_seed(9 + 7919 + i))
        assert torch.equal(ev.edit_noise[i], want) and not torch.equal(ev.edit_noise[i], ev.noise[i])
        tok = mask_to_tokens(edit_mask('box', 1, HP, WP), HP, WP, 'max').cuda()
        assert torch.equal(ev.edits[i]['tokens'], tok) and tok.mean().item() == 0.25
        x0 = ev.teacher_latents[i]
        tea = d.sample_teacher(c, want, num_steps=4, x0=x0, mask=tok.expand(B, -1, -1).contiguous(), strength=0.8)
        assert torch.equal(tea, ev.teacher_edit_latents[i])
        stu = d.sample_student(c, want, x0=x0, mask=tok, strength=0.8, ema=True)
        a, b = stu.double().cpu().flatten(1), tea.double().cpu().flatten(1)
        w = tok.cpu().double()[:, :, None, :].expand(1, N, 16, 4).reshape(1, N * 64)
        sums = torch.stack([torch.stack([ww.expand_as(a).sum(1), (ww * (a - b) ** 2).sum(1), (ww * a * a).sum(1), (ww * b * b).sum(1), (ww * a * b).sum(1)], 1)
                            for ww in (w, 1 - w)], 1)
        kappa = ((w * a * b).abs().sum(1) / (w * a * b).sum(1).abs()).max().item()
        rtol = max(rtol, (kappa + 3) * 2 * N * 64 * U + 8 * U)
        rep, keep = masked_metrics_from_sums(sums)
        for k, v in zip(EDIT_LATENT, (rep['mse'], rep['rel_l2'], rep['cosine'], keep['mse'])):
            got[k] += v.tolist()
    for k in EDIT_LATENT:
        worst = max(abs(x - y) / max(abs(y), 1e-300) for x, y in zip(first[k], got[k]) if y != 0 or x != 0) if any(got[k]) else 0.0
        print(f'{k}: {first[k]}  max rel diff to the CPU {worst:.3e} (rtol {rtol:.3e})')
        assert worst <= rtol, (k, worst, rtol)


def test_evaluator_edit_image_metrics_through_the_vae_path(dist):
    from arcflow_amd.train import Evaluator
    conds = [_cond(2, seed=95)]
    mask = torch.zeros(1, 1, 16 * HP, 16 * WP)
    mask[:, :, 20:90, 30:100] = 1.0
    mask[:, :, 40:60, 50:70] = 0.5                                     # a fractional patch: weights need not be binary
    ev = Evaluator(dist, conds, seed=2, teacher_steps=4, vae=_Decoder(), edits=[dict(mask=mask, strength=0.6, x0=(_noise(2, seed=96) * 0.8))])
    res = ev.evaluate()
    for k in EDIT_LATENT + EDIT_IMAGE:
        assert len(res[k]) == 2 and all(v == v and abs(v) != float('inf') for v in res[k]) and k + '_mean' in res, (k, res.get(k))
    assert all(0 < v < 100 for v in res['edit_image_psnr']) and all(-1 <= v <= 1 for v in res['edit_image_ssim'] + res['edit_keep_image_ssim'])
    assert all(v > 0 for v in res['edit_image_mse']) and res['edit_image_ssim'] != res['image_ssim']
    assert _strip(ev.evaluate()) == _strip(res)
    with pytest.raises(ValueError, match='mask'):
        Evaluator(dist, conds, edits=dict(mask=mask[:, :, :64], strength=0.6))
    with pytest.raises(ValueError, match='strength'):
        Evaluator(dist, conds, edits=dict(mask=mask, strength=0.0))
    with pytest.raises(ValueError, match='one dict per condition'):
        Evaluator(dist, conds, edits=[dict(mask='box'), dict(mask='left')])


def test_train_cli_writes_the_edit_keys_and_refuses_the_flag_without_evaluation(tmp_path):
    from tests.test_train_frontend import _TINY_CFG
    cfgp = tmp_path / 'tiny.py'
    cfgp.write_text(_TINY_CFG + "test_cfg = dict(nfe=2, timestep_ratio=1.0, total_substeps=128)\n")
    base = [sys.executable, os.path.join(ROOT, 'tools', 'train.py'), str(cfgp), '--synthetic', '--latent-tokens', '8', '8', '--iters', '2']
    work = tmp_path / 'edits'
    r = subprocess.run(base + ['--work-dir', str(work), '--eval-interval', '1', '--eval-teacher-steps', '4', '--eval-edits', 'box', '--eval-edit-strength', '0.7'],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in open(work / 'eval.jsonl')]
    assert [l['iteration'] for l in lines] == [0, 1, 2]
    for l in lines:
        for k in EDIT_LATENT:
            assert len(l[k]) == 2 and all(v == v and abs(v) != float('inf') for v in l[k] + [l[k + '_mean']]), (k, l)
        assert l['edit_keep_latent_mse'] == [0.0, 0.0] and 'latent_rel_l2' in l
    assert r.stdout.count('[eval] iter') == 3 and r.stdout.count('"edit_latent_rel_l2_mean"') == 3
    for flags in (['--eval-edits', 'box'], ['--eval-edit-strength', '0.5']):          # refused while the arguments are read, like --vae-dir
        bad = subprocess.run(base + ['--work-dir', str(tmp_path / 'refused')] + flags, capture_output=True, text=True, timeout=600)
        assert bad.returncode != 0 and 'eval-interval' in bad.stderr and not (tmp_path / 'refused' / 'eval.jsonl').exists(), (flags, bad.stderr[-500:])
