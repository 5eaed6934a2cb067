"""``image_ssim`` in training-time evaluation, on the tiny engines and the 8 x 8 token grid of tests/test_evaluate_gpu.py (whose helpers
build them), and ``tools/train.py --vae-dir``.

The stand-in decoder of that file -- the packed latents, scaled, as bf16 [B, 1, 64, 64] -- is an image a window fits, so the Evaluator
reports ``image_ssim`` for it: the mean of afx_image_ssim's per-sample sum over the 54 x 54 windows, held to the fp64 CPU reference of
tests/ssim_ref.py within its bound (derived in tests/test_hip_image_ssim_fp64.py; the division by the window count on the host adds one
rounding of a value <= 1: 2^-53).  Every other key must be what an Evaluator without SSIM returned: ``metrics_from_sums`` of
``ops.sample_score`` of the same latents and images, bit for bit.  A decoder whose output takes no window ([B, 1, 4, 1024]) keeps working
and reports no ``image_ssim``.
"""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import ssim_ref as SR
import test_evaluate_gpu as EG

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


class Decoder:
    """tests/test_evaluate_gpu.py's stand-in: a fixed reshape of the packed latents to bf16 [B, 1, hp * wp, 64], scaled."""
    shape = (1, EG.N, 64)

    def decode_packed(self, latents, hp, wp):
        return (latents * 1.5).to(torch.bfloat16).view(latents.shape[0], *self.shape)


class WideDecoder(Decoder):
    shape = (1, 4, 1024)          # four rows: no 11 x 11 window fits


@pytest.fixture(scope='module')
def dist():
    return EG._distiller(0, 0)


def _expected(d, ev, conds, decoder):
    """What the Evaluator must report, from the same latents: the sample_score keys bit for bit, and the CPU SSIM with its bound."""
    from arcflow_amd import ops
    from arcflow_amd.train.evaluate import metrics_from_sums
    want = {k: [] for k in ('latent_mse', 'latent_rel_l2', 'latent_cosine', 'image_psnr', 'image_mse')}
    ssim, bound = [], []
    for i, c in enumerate(conds):
        stu, tea = d.sample_student(c, ev.noise[i]), ev.teacher_latents[i]
        m = metrics_from_sums(ops.sample_score(stu, tea), stu[0].numel())
        for k in ('mse', 'rel_l2', 'cosine'):
            want['latent_' + k] += m[k].tolist()
        a, b = decoder.decode_packed(stu, c['hp'], c['wp']).contiguous(), decoder.decode_packed(tea, c['hp'], c['wp']).contiguous()
        m = metrics_from_sums(ops.sample_score(a, b, transform=True), a[0].numel(), data_range=1.0)
        want['image_psnr'] += m['psnr'].tolist()
        want['image_mse'] += m['mse'].tolist()
        if a.shape[2] >= 11:
            ssim += SR.ssim_mean(a.cpu(), b.cpu(), True, 1.0).tolist()
            bound += (SR.ssim_bound(a.cpu(), b.cpu(), True, 1.0) + U).tolist()
            assert ((SR.unit_range(a) == 0) | (SR.unit_range(a) == 1)).double().mean().item() > 0.05          # the clamp is exercised
    return want, ssim, bound


def test_evaluator_reports_image_ssim_and_leaves_the_other_keys_alone(dist):
    from arcflow_amd.train import Evaluator
    d = dist
    conds = [EG._cond(2, seed=61), EG._cond(1, seed=62)]
    ev = Evaluator(d, conds, seed=2, teacher_steps=4, use_ema=False, vae=Decoder())
    res = ev.evaluate()
    want, ssim, bound = _expected(d, ev, conds, Decoder())
    keys = ('latent_mse', 'latent_rel_l2', 'latent_cosine', 'image_psnr', 'image_mse', 'image_ssim')
    assert set(res) == {'iteration', 'seconds'} | set(keys) | {k + '_mean' for k in keys}
    for k, v in want.items():
        assert res[k] == v, k                                   # python floats: bit for bit
        assert res[k + '_mean'] == math.fsum(v) / 3
    assert len(res['image_ssim']) == 3
    for got, ref, bnd in zip(res['image_ssim'], ssim, bound):
        print(f'image_ssim {got!r}  CPU fp64 {ref!r}  |diff| {abs(got - ref):.3e}  bound {bnd:.3e}')
        assert 0 < got <= 1 and abs(got - ref) <= bnd
    assert abs(res['image_ssim_mean'] - sum(ssim) / 3) <= max(bound) + 4 * U
    again = ev.evaluate()
    assert again['image_ssim'] == res['image_ssim']           # bit-reproducible, teacher images kept


def test_image_ssim_orientation_teacher_like_heads_score_higher_than_random_heads(dist):
    """The fresh student's means are copies of the teacher's velocity head: its decoded samples must be structurally closer to the teacher's
    than those of a student whose heads are re-randomised."""
    from arcflow_amd.train import Evaluator
    d = dist
    conds = [EG._cond(2, seed=51)]
    good = Evaluator(d, conds, seed=1, teacher_steps=8, use_ema=False, vae=Decoder()).evaluate()
    keep = d.params.clone()
    try:
        g = torch.Generator().manual_seed(52)
        rows = d.K * d.C + d.K * d.L + (d.K - 1) * d.L
        d._view(d.params, 0).view(d.head_n, d.D)[:rows].copy_((torch.randn(rows, d.D, generator=g) * 0.05).cuda())
        d._sync_working_copies()
        bad = Evaluator(d, conds, seed=1, teacher_steps=8, use_ema=False, vae=Decoder()).evaluate()
    finally:
        d.params.copy_(keep)
        d._sync_working_copies()
    print(f'image_ssim: teacher-copied heads {good["image_ssim"]}  random heads {bad["image_ssim"]}')
    assert all(0 < y < x <= 1 for x, y in zip(good['image_ssim'], bad['image_ssim']))
    assert good['image_ssim_mean'] > bad['image_ssim_mean']


def test_decoder_of_another_shape_reports_no_image_ssim(dist):
    from arcflow_amd.train import Evaluator
    d = dist
    conds = [EG._cond(2, seed=61)]
    ev = Evaluator(d, conds, seed=2, teacher_steps=4, use_ema=False, vae=WideDecoder())
    res = ev.evaluate()
    want, ssim, _ = _expected(d, ev, conds, WideDecoder())
    keys = ('latent_mse', 'latent_rel_l2', 'latent_cosine', 'image_psnr', 'image_mse')
    assert ssim == [] and set(res) == {'iteration', 'seconds'} | set(keys) | {k + '_mean' for k in keys}
    for k, v in want.items():
        assert res[k] == v, k


def test_edit_tool_scores_two_written_images():
    """tools/edit_image.py score_images: PSNR and SSIM of two PIL images on their 8-bit values / 255, against the CPU reference."""
    import importlib.util
    import numpy as np
    from PIL import Image
    spec = importlib.util.spec_from_file_location('edit_image_tool', os.path.join(ROOT, 'tools', 'edit_image.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    g = torch.Generator().manual_seed(71)
    base = torch.nn.functional.avg_pool2d(torch.rand(1, 3, 36, 52, generator=g), 5, stride=1)[0]          # [3, 32, 48], smooth
    other = (base + 0.05 * torch.randn(3, 32, 48, generator=g)).clamp(0, 1)
    to_u8 = lambda t: (t * 255).round().to(torch.uint8)          # noqa: E731
    a8, b8 = to_u8(base), to_u8(other)
    got = tool.score_images(Image.fromarray(a8.permute(1, 2, 0).numpy()), Image.fromarray(b8.permute(1, 2, 0).numpy()))
    a, b = (torch.from_numpy(np.asarray(t, dtype=np.float32) / 255.0)[None] for t in (a8.numpy(), b8.numpy()))
    ref, bound = SR.ssim_mean(a, b, False, 1.0), SR.ssim_bound(a, b, False, 1.0) + U
    mse = ((a.double() - b.double()) ** 2).mean().item()
    assert set(got) == {'image_psnr', 'image_ssim'} and len(got['image_ssim']) == 1
    assert abs(got['image_ssim'][0] - ref.item()) <= bound.item() and 0 < got['image_ssim'][0] < 1
    assert abs(got['image_psnr'][0] + 10 * math.log10(mse)) <= 1e-9
    same = tool.score_images(Image.fromarray(a8.permute(1, 2, 0).numpy()), Image.fromarray(a8.permute(1, 2, 0).numpy()))
    assert same['image_ssim'] == [1.0]


def _write_vae_dir(path):
    """A FLUX vae/ directory at the widths tests/test_vae_encoder.py decodes with (64, 128, 128, 128; 16 groups), seeded random weights."""
    from safetensors.torch import save_file
    from oracle import vae_ref as V
    chans = (64, 128, 128, 128)
    os.makedirs(path)
    with open(os.path.join(path, 'config.json'), 'w') as f:
        json.dump(dict(block_out_channels=list(chans), norm_num_groups=16, layers_per_block=2, scaling_factor=0.3611, shift_factor=0.1159), f)
    save_file({k: v.contiguous() for k, v in V.make_decoder_weights(chans, seed=4).items()}, os.path.join(path, 'diffusion_pytorch_model.safetensors'))


def test_train_cli_vae_dir_writes_the_image_means(tmp_path):
    """tools/train.py --synthetic --iters 2 --eval-interval 2 --vae-dir <dir>: eval.jsonl carries image_ssim_mean and image_psnr_mean (decoded
    [2, 3, 128, 128] images); the same command without --vae-dir carries neither; --vae-dir without --eval-interval is refused."""
    cfgp = tmp_path / 'tiny.py'
    cfgp.write_text(_tiny_cfg())
    vae_dir = str(tmp_path / 'vae')
    _write_vae_dir(vae_dir)
    base = [sys.executable, os.path.join(ROOT, 'tools', 'train.py'), str(cfgp), '--synthetic', '--latent-tokens', '8', '8', '--iters', '2']
    ev = ['--eval-interval', '2', '--eval-teacher-steps', '4']
    r = subprocess.run(base + ['--work-dir', str(tmp_path / 'refused'), '--vae-dir', vae_dir], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and '--eval-interval' in r.stderr and not (tmp_path / 'refused' / 'eval.jsonl').exists()
    for tag, extra in (('vae', ['--vae-dir', vae_dir]), ('plain', [])):
        work = tmp_path / tag
        r = subprocess.run(base + ev + ['--work-dir', str(work)] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [json.loads(l) for l in open(work / 'eval.jsonl')]
        assert [l['iteration'] for l in lines] == [0, 2]
        shown = [l for l in r.stdout.splitlines() if l.startswith('[eval] iter')]
        assert len(shown) == 2
        for l, s in zip(lines, shown):
            assert all(v == v and abs(v) != float('inf') for v in l['latent_rel_l2'])
            if tag == 'vae':
                assert len(l['image_ssim']) == 2 and all(0 < v <= 1 for v in l['image_ssim'])
                assert 0 < l['image_ssim_mean'] <= 1 and 0 < l['image_psnr_mean'] < 400 and l['image_mse_mean'] >= 0
                assert '"image_ssim_mean"' in s and '"image_psnr_mean"' in s
            else:
                assert not any(k.startswith('image_') for k in l) and 'image_' not in s


def _tiny_cfg():
    from tests.test_train_frontend import _TINY_CFG
    return _TINY_CFG + "eval_interval = 2\ntest_cfg = dict(nfe=2, timestep_ratio=1.0, total_substeps=128)\n"
