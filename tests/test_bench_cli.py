"""bench.py's launcher contract (CPU): `--gpus N` never silently degrades to one GPU (VERDICT r01 "What's missing" 1)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_single_gpu_runs_in_process():
    import bench
    args = bench.parse_args(['--steps', '3'])
    assert args.gpus == 1 and args.steps == 3 and args.warmup == 2
    assert bench.launcher_cmd(args, ['--steps', '3'], environ={}, device_count=1) is None


def test_multi_gpu_self_launch_command():
    import bench
    argv = ['--gpus', '4', '--steps', '7', '--warmup', '1', '--model', 'qwen']
    args = bench.parse_args(argv)
    cmd = bench.launcher_cmd(args, argv, environ={}, device_count=8)
    assert cmd[:3] == [sys.executable, '-m', 'torch.distributed.run']
    assert '--nnodes=1' in cmd
    assert cmd[cmd.index('--nproc-per-node') + 1] == '4'
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1'
    i = cmd.index(os.path.join(ROOT, 'bench.py'))
    assert cmd[i + 1:] == argv                      # every flag is forwarded to the ranks


def test_multi_gpu_request_on_a_small_box_fails_loudly():
    import bench
    argv = ['--gpus', '2']
    with pytest.raises(SystemExit) as e:
        bench.launcher_cmd(bench.parse_args(argv), argv, environ={}, device_count=1)
    assert '--gpus 2' in str(e.value) and '1 GPU' in str(e.value)


def test_rank_of_a_torchrun_launch_runs_in_process_and_checks_world_size():
    import bench
    argv = ['--gpus', '8']
    assert bench.launcher_cmd(bench.parse_args(argv), argv, environ={'WORLD_SIZE': '8', 'RANK': '3'}, device_count=8) is None
    with pytest.raises(SystemExit):
        bench.launcher_cmd(bench.parse_args(argv), argv, environ={'WORLD_SIZE': '2', 'RANK': '0'}, device_count=8)
    with pytest.raises(SystemExit):      # the driver's bare `python bench.py` under a stale WORLD_SIZE
        bench.launcher_cmd(bench.parse_args([]), [], environ={'WORLD_SIZE': '4'}, device_count=8)


def test_train_mode_defaults():
    import bench
    a = bench.parse_args(['--train', '--model', 'qwen'])
    assert a.train and a.steps == 2 and a.warmup == 1 and a.batch is None


def test_plain_run_is_the_headline_and_full_is_opt_in():
    import bench
    a = bench.parse_args(['--steps', '4', '--warmup', '1'])
    assert not a.full and a.dump_outputs is None and a.steps == 4 and a.warmup == 1
    a = bench.parse_args(['--full', '--dump-outputs', 'out'])
    assert a.full and a.dump_outputs == 'out'
    for bad in (['--steps', '0'], ['--warmup', '-1'], ['--e2e', '--dump-outputs', 'out']):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_dump_outputs_float_npy_and_seeded_sample(tmp_path):
    import numpy as np
    import torch
    import bench
    big = torch.arange(bench.DUMP_MAX_ELEMS + 1000, dtype=torch.float32)
    s1, s2 = bench._seeded_sample(big), bench._seeded_sample(big.clone())
    assert s1.numel() == bench.DUMP_MAX_ELEMS and torch.equal(s1, s2)          # the same elements in every run
    assert bool((s1[1:] >= s1[:-1]).all())
    small = torch.randn(3, 5)
    assert torch.equal(bench._seeded_sample(small), small.reshape(-1))
    bench.dump_outputs(str(tmp_path / 'd'), {'lat': small.bfloat16(), 'loss': torch.tensor([0.5], dtype=torch.float64)})
    lat, loss = np.load(tmp_path / 'd' / 'lat.npy'), np.load(tmp_path / 'd' / 'loss.npy')
    assert lat.dtype == np.float32 and lat.shape == (3, 5) and np.allclose(lat, small.bfloat16().float().numpy())
    assert loss.dtype == np.float64 and loss.tolist() == [0.5]


@pytest.mark.gpu
def test_plain_run_line_and_dumped_latents(tmp_path):
    """A plain `bench.py` run prints the headline alone and --dump-outputs writes the last timed image's latents."""
    import json
    import subprocess
    import numpy as np
    out = tmp_path / 'dump'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--dump-outputs', str(out)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1
    ln = lines[0]
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in ln, k
    assert ln['steps'] == 2 and ln['warmup'] == 1 and ln['value'] > 0 and ln['ms_per_step'] > 0
    assert not {'roofline', 'roofline_step', 'cpu_baseline', 'qwen', 'e2e'} & set(ln)
    lat = np.load(out / 'latents.npy')
    assert lat.dtype == np.float32 and lat.shape == (1, 4096, 64) and np.isfinite(lat).all()
