"""Training-time evaluation on the CPU: ``metrics_from_sums`` against direct torch fp64 formulas, the argument checks of the
``afx_sample_score`` C-ABI entry (they return before any launch), the config keys ``eval_interval`` / ``test_cfg`` / ``eval_cfg`` and
the front-end's flags (evaluation is off without ``--eval-interval``), and the student's sigma grid against the oracle's.  No GPU."""
import ctypes as C
import json
import math
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sums(a, b):
    a, b = a.double(), b.double()
    return torch.stack([((a - b) ** 2).sum(1), (a * a).sum(1), (b * b).sum(1), (a * b).sum(1)], 1)


def test_metrics_from_sums_match_direct_formulas():
    from arcflow_amd.train.evaluate import metrics_from_sums
    g = torch.Generator().manual_seed(0)
    B, n = 5, 192
    b = torch.rand(B, n, generator=g, dtype=torch.float64)
    a = (b + 0.1 * torch.randn(B, n, generator=g, dtype=torch.float64)).clamp(0, 1)
    m = metrics_from_sums(_sums(a, b), n, data_range=1.0)
    mse = ((a - b) ** 2).mean(1)
    assert all(v.dtype == torch.float64 and v.shape == (B,) and v.device.type == 'cpu' for v in m.values())
    assert torch.allclose(m['mse'], mse, rtol=1e-13, atol=0)
    assert torch.allclose(m['rel_l2'], (a - b).norm(dim=1) / b.norm(dim=1), rtol=1e-13, atol=0)
    assert torch.allclose(m['cosine'], torch.nn.functional.cosine_similarity(a, b, dim=1), rtol=1e-13, atol=0)
    assert torch.allclose(m['psnr'], 10 * torch.log10(1.0 / mse), rtol=1e-13, atol=0)
    assert torch.allclose(metrics_from_sums(_sums(a, b), n, data_range=255.0)['psnr'], 10 * torch.log10(255.0 ** 2 / mse), rtol=1e-13, atol=0)
    assert 'psnr' not in metrics_from_sums(_sums(a, b), n)                       # only with a data range
    assert set(metrics_from_sums(_sums(a, b).tolist(), n)) == {'mse', 'rel_l2', 'cosine'}        # a list of lists is fine too
    # the teacher is b: rel_l2 is relative to IT
    swapped = metrics_from_sums(_sums(b, a), n)
    assert torch.allclose(swapped['rel_l2'], (a - b).norm(dim=1) / a.norm(dim=1), rtol=1e-13, atol=0) and not torch.allclose(swapped['rel_l2'], m['rel_l2'])


def test_metrics_from_sums_floors_keep_degenerate_cases_finite():
    from arcflow_amd.train.evaluate import metrics_from_sums
    g = torch.Generator().manual_seed(1)
    a = torch.randn(3, 64, generator=g, dtype=torch.float64)
    same = metrics_from_sums(_sums(a, a), 64, data_range=1.0)                   # a = b
    assert (same['mse'] == 0).all() and (same['rel_l2'] == 0).all()
    assert torch.allclose(same['cosine'], torch.ones(3, dtype=torch.float64), rtol=1e-14, atol=0)
    assert torch.allclose(same['psnr'], torch.full((3,), 300.0, dtype=torch.float64), rtol=1e-14, atol=0)     # capped by the 1e-30 floor
    zero = metrics_from_sums(_sums(a, torch.zeros_like(a)), 64, data_range=1.0)          # b = 0: S_bb = S_ab = 0
    assert all(torch.isfinite(v).all() for v in zero.values())
    assert (zero['cosine'] == 0).all() and torch.allclose(zero['rel_l2'], a.norm(dim=1) / math.sqrt(1e-30), rtol=1e-13, atol=0)
    both = metrics_from_sums(torch.zeros(2, 4), 64, data_range=1.0)                      # a = b = 0
    assert all(torch.isfinite(v).all() for v in both.values()) and (both['rel_l2'] == 0).all() and (both['cosine'] == 0).all()


def test_cabi_argument_checks_without_a_device():
    """Null pointers, n % 64 != 0, misaligned operands, a short workspace and a bad dtype / transform are refused before any launch,
    and afx_last_error() names the entry."""
    from arcflow_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    p = [C.c_void_p(4096 * k) for k in range(1, 5)]
    score, BF16, F32 = lib.afx_sample_score, _lib.AFX_DT_BF16, _lib.AFX_DT_F32

    def refused(*args):
        rc = score(*args)
        return rc < 0 and b'afx_sample_score' in lib.afx_last_error()
    assert lib.afx_sample_score_ws_bytes(3, 320) == 3 * 32                      # one work-group per sample, 4 doubles
    assert lib.afx_sample_score_ws_bytes(2, 64 * 1031) == 2 * 9 * 32            # ceil(65984 / 8192) = 9
    assert lib.afx_sample_score_ws_bytes(1, 8192 * 64 + 64) == 64 * 32          # capped at 64
    assert lib.afx_sample_score_ws_bytes(1, 100) == -1 and b'afx_sample_score_ws_bytes' in lib.afx_last_error()
    assert lib.afx_sample_score_ws_bytes(-1, 64) == -1
    assert refused(None, None, BF16, 0, None, None, 0, 1, 64, None)
    for missing in (0, 1, 4, 5):                                                # a, b, out, ws
        a = [p[0], p[1], BF16, 0, p[2], p[3], 32, 1, 64, None]
        a[missing] = None
        assert refused(*a), missing
    for n in (0, 8, 63, 65, 64 * 5 + 8, -64):
        assert refused(p[0], p[1], F32, 0, p[2], p[3], 1 << 20, 1, n, None), n
    assert b'multiple of 64' in lib.afx_last_error()
    assert refused(C.c_void_p(4096 + 8), p[1], F32, 0, p[2], p[3], 32, 1, 64, None)         # a not 16-byte aligned
    assert refused(p[0], C.c_void_p(8192 + 2), BF16, 0, p[2], p[3], 32, 1, 64, None)        # b not 16-byte aligned
    assert refused(p[0], p[1], BF16, 0, C.c_void_p(12288 + 4), p[3], 32, 1, 64, None)       # out not 8-byte aligned
    assert refused(p[0], p[1], BF16, 0, p[2], C.c_void_p(16384 + 4), 32, 1, 64, None)       # ws not 8-byte aligned
    assert refused(p[0], p[1], BF16, 0, p[2], p[3], 24, 1, 64, None) and b'workspace' in lib.afx_last_error()
    assert refused(p[0], p[1], BF16, 0, p[2], p[3], 2 * 9 * 32 - 8, 2, 64 * 1031, None)
    assert refused(p[0], p[1], _lib.AFX_DT_FP8, 0, p[2], p[3], 32, 1, 64, None)
    assert refused(p[0], p[1], 0, 0, p[2], p[3], 32, 1, 64, None)
    assert refused(p[0], p[1], BF16, 2, p[2], p[3], 32, 1, 64, None)
    assert refused(p[0], p[1], BF16, 0, p[2], p[3], 32, -1, 64, None)
    assert score(p[0], p[1], BF16, 1, p[2], p[3], 0, 0, 64, None) == 0                       # an empty batch launches nothing


def test_ops_refuse_cpu_tensors():
    from arcflow_amd import _lib, ops
    x = torch.zeros(1, 64)
    with pytest.raises(_lib.ArcflowHipError):
        ops.sample_score(x, x)
    with pytest.raises(_lib.ArcflowHipError):
        ops.sample_score(x.bfloat16(), x.bfloat16(), transform=True)


def _golden_config(name):
    """One reference experiment config as the config reader merged it (fixture G10)."""
    def dec(v):
        if isinstance(v, dict):
            return tuple(dec(x) for x in v['__tuple__']) if set(v) == {'__tuple__'} else {k: dec(x) for k, x in v.items()}
        if isinstance(v, list):
            return [dec(x) for x in v]
        return v
    with open(os.path.join(ROOT, 'tests', 'golden', 'g10_configs.json')) as f:
        return dec(json.load(f)[name])


def test_config_carries_eval_keys():
    from arcflow_amd.train import config as CFG
    cfg = _golden_config('flux/arcflux_2nfe_k16.py')
    run = CFG.distill_setup(cfg)[3]
    assert run['eval_interval'] == 500
    assert run['test_cfg'] == dict(nfe=2, timestep_ratio=1.0, distilled_guidance_scale=3.5)
    assert run['eval_cfg'] == dict(num_batches=1, seed=0, teacher_steps=28, use_ema=True) == CFG.EVAL_CFG_DEFAULTS      # no eval_cfg: the defaults
    q = CFG.distill_setup(_golden_config('qwen/arcqwen_2nfe_k16.py'))[3]
    assert q['eval_interval'] == 400 and q['test_cfg'] == dict(nfe=2, timestep_ratio=1.0, distilled_guidance_scale=None)
    over = CFG.distill_setup(CFG.apply_options(cfg, {'eval_cfg': dict(num_batches=3, use_ema=False), 'eval_interval': 50}))[3]
    assert over['eval_cfg'] == dict(num_batches=3, seed=0, teacher_steps=28, use_ema=False) and over['eval_interval'] == 50
    with pytest.raises(ValueError, match='eval_cfg'):
        CFG.distill_setup(CFG.apply_options(cfg, {'eval_cfg': dict(batches=3)}))
    bare = {k: v for k, v in cfg.items() if k not in ('eval_interval', 'test_cfg')}
    r = CFG.distill_setup(bare)[3]
    assert r['eval_interval'] is None and r['test_cfg'] == dict(nfe=None, timestep_ratio=None, distilled_guidance_scale=None)
    # the example config shows the keys and reads back
    ex = CFG.distill_setup(CFG.load_config(os.path.join(ROOT, 'examples', 'flux_distill_2nfe.py')))[3]
    assert ex['eval_interval'] == 500 and ex['eval_cfg'] == CFG.EVAL_CFG_DEFAULTS and ex['test_cfg']['nfe'] == 2


def test_train_cli_leaves_evaluation_off_without_the_flag():
    from tools import train as T
    run = dict(eval_interval=500)
    args = T.parse_args(['cfg.py', '--synthetic'])
    assert args.eval_interval is None and args.eval_batches is None and args.eval_teacher_steps is None
    assert T.eval_interval(args, run) == 0                                      # off, whatever the config says
    assert T.eval_interval(T.parse_args(['cfg.py', '--eval-interval', '2']), run) == 2
    assert T.eval_interval(T.parse_args(['cfg.py', '--eval-interval', 'config']), run) == 500
    assert T.eval_interval(T.parse_args(['cfg.py', '--eval-interval', '0']), run) == 0
    a = T.parse_args(['cfg.py', '--eval-interval', '2', '--eval-batches', '3', '--eval-teacher-steps', '4'])
    assert (a.eval_batches, a.eval_teacher_steps) == (3, 4)
    with pytest.raises(SystemExit):
        T.eval_interval(T.parse_args(['cfg.py', '--eval-interval', 'config']), dict(eval_interval=None))
    with pytest.raises(SystemExit):
        T.eval_interval(T.parse_args(['cfg.py', '--eval-interval', 'often']), run)


@pytest.mark.parametrize('nfe,ratio', [(1, 1.0), (2, 1.0), (2, 0.5), (4, 0.5)])
def test_student_sigmas_are_the_pipelines_grid(nfe, ratio):
    """schedule.student_sigmas against the oracle's restatement of the pipelines' grid (oracle/arcflow_ref.inference_sigmas): the same raw
    grid and fp32 shift; the pipelines read sigma back as (sigma * 1000) / 1000, one fp32 rounding away."""
    from arcflow_amd.schedule import student_sigmas
    from oracle import arcflow_ref as R
    got = student_sigmas(nfe, 128, ratio, 3.2)
    ref, _ = R.inference_sigmas(nfe, 128, ratio, 3.2)
    assert len(got) == nfe + 1 and got[-1] == 0.0 and abs(got[0] - 1.0) < 1e-6
    assert all(x > y for x, y in zip(got, got[1:]))
    assert max(abs(x - y) for x, y in zip(got, ref)) <= 2.0 ** -23
