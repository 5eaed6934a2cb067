"""The GEMM's kernel choice (arcflow_amd/csrc/afx_gemm_plan.h plan_gemm) without a GPU: tests/gemm_plan_check.hip builds batches with fake pointers, plans
them for 256 CUs under explicit settings and prints one line per case; the expectations below are worked out by hand from the rules (tile counts =
ceil(M / tm) * ceil(N / tn) summed over the problems, cost = rounds of 256 tiles x tile area x the shape's factor)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lines(tmp_path_factory):
    from arcflow_amd import build
    exe = str(tmp_path_factory.mktemp('gemm_plan') / 'gemm_plan_check')
    subprocess.run([build._hipcc(), '-std=c++17', '-O1', '-Wall', '--offload-arch=gfx950', '-I', build.CSRC,
                    os.path.join(ROOT, 'tests', 'gemm_plan_check.hip'), '-o', exe], check=True)
    out = subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout
    got = dict(l.split(': ', 1) for l in out.splitlines())
    assert len(got) == len(out.splitlines())          # every case has a name of its own
    return got


def plan(family, shape, total, group_m=6, persist=0, grid=None):
    return f'ok {family} {shape} total={total} group_m={group_m} persist={persist} grid={total if grid is None else grid}'


EXPECT = {
    # bf16, tile shape picked per launch: 4096 + 512 rows are 16 + 2 row tiles of 256
    'flux_n3072': plan('v3', '256x224', 252) + ' tiles 16x14*1@0 tiles 2x14*1@224',      # one round either way: 224 x 1.03 < 256
    'flux_n3072_f32': plan('v3', '256x256', 216),                                        # fp32 output: no 256x224
    'flux_n12288': plan('v3', '256x224', 990),                                           # 18 x 55 tiles, 4 rounds like 256x256's 864
    'lora_n256': plan('v3', '128x128', 72, group_m=8),                                   # 18 tiles of 256x256 for 256 CUs
    # fused q / k epilogue: 256x256 or 224x256 only
    'qk_qwen': plan('v3', '224x256', 720),                                               # 20 x 36 tiles: 3 rounds like the 612 of 256x256
    'qk_flux': plan('v3', '256x256', 648),                                               # 224x256: 22 x 36 = 792 tiles = 4 rounds
    'qk_flux_tile6': plan('v3', '224x256', 792),
    'qk_flux_tile2': plan('v3', '256x256', 648),                                         # any other forced shape: 256x256
    'qk_qwen_impl2': 'invalid',
    'qk_flux_impl2': 'invalid',
    'qk_no_table': 'invalid',
    # forced shapes, forced super-row height, forced 8-phase kernel
    'tile1': plan('v3', '256x256', 216),
    'tile2': plan('v3', '288x192', 272, group_m=5),
    'tile3': plan('v3', '320x192', 240, group_m=4),
    'tile4': plan('v3', '128x128', 864, group_m=8),
    'tile5': plan('v3', '256x224', 252),
    'tile6': plan('v3', '224x256', 264),
    'tile5_f32': plan('v3', '256x256', 192),
    'group_m9': plan('v3', '256x224', 252, group_m=9),
    'group_m9_conv': plan('v3conv', '256x128', 5, group_m=9),
    'group_m9_8phase': plan('8phase', '256x256', 216, group_m=9),
    'impl2': plan('8phase', '256x256', 216),
    # what the one-wave-per-SIMD kernel does not take goes to the 8-phase kernel
    'pre': plan('8phase', '256x256', 216),
    'splitk4': plan('8phase', '256x256', 48) + ' tiles 1x12*4@0',
    'splitk_ignored': plan('v3', '128x128', 48, group_m=8) + ' tiles 2x24*1@0',
    'k32': plan('8phase', '256x256', 4),
    'f32_gelu': plan('8phase', '256x256', 4),
    # convolutions: 34 x 34 padded grid = 1156 rows = 5 row tiles
    'conv_n128': plan('v3conv', '256x128', 5),
    'conv_n256': plan('v3conv', '256x256', 5),
    'conv_tile1': plan('8phase', '256x256', 5),
    'conv_impl2': plan('8phase', '256x256', 5),
    'conv_mixed': plan('8phase', '256x256', 10),
    # fp8: the one-wave-per-SIMD kernel from half a round (128) of 256x256 tiles on
    'fp8_120': plan('8phase+fp8', '256x256', 120),
    'fp8_128': plan('v3f8', '224x256', 160),                                             # 128 tiles of 256x256 = 160 of 224x256, one round either way
    'fp8_qwen': plan('v3f8', '224x256', 240),
    'fp8_tile1': plan('v3f8', '256x256', 204),
    'fp8_tile2': plan('v3f8', '224x256', 240),
    'fp8_min0': plan('v3f8', '224x256', 36),
    'fp8_v3_off': plan('8phase+fp8', '256x256', 192),
    'fp8_v3_off_mx': 'invalid',
    'fp8_impl2': plan('8phase+fp8', '256x256', 192),
    'mx': plan('v3f8+mx', '224x256', 36),                                                # block scales: this kernel whatever the tile count
    'mx_k3200': 'invalid',
    'mx_mixed': 'invalid',
    'c8_gelu': plan('v3f8', '224x256', 144),
    'c8_gate_res': 'invalid',
    'c8_impl2': 'invalid',
    'fp8_qk': plan('v3f8+mx', '256x256', 612),                                           # the fused q / k epilogue keeps 256x256
    # validation
    'drop': plan('v3', '288x192', 256, group_m=5),                                       # 16 x 16 tiles fill one round exactly
    'drop_gate': 'invalid',
    'drop_impl2': 'invalid',
    'drop_k32': 'invalid',
    'perm16_n4600': 'invalid',
    'perm16_n4608': plan('v3', '224x256', 252),
    'perm16_impl2': 'invalid',
    'empty': 'empty',
    'empty_qk': 'empty',
    'empty_conv': 'empty',
    'empty_8phase': 'empty',
    # the persistent walk
    'persist0': plan('v3', '256x224', 990),
    'persist1': plan('v3', '256x224', 990, persist=1, grid=256),
    'persist2': plan('v3', '256x224', 990, persist=2, grid=256),
    'persist3': plan('v3', '256x224', 990),                                              # no such walk: the plain launch
    'persist1_one_round': plan('v3', '256x224', 252),                                    # not more tiles than work-group slots
    'persist1_cus250': plan('v3', '256x224', 990),                                       # slots no multiple of the 8 XCDs
    'persist1_conv': plan('v3conv', '256x128', 1033),
    'persist1_fp8': plan('v3f8', '224x256', 1008),
    'persist1_8phase': plan('8phase', '256x256', 864),
    'persist1_128x128': plan('v3', '128x128', 864, group_m=8, persist=1, grid=512),      # two work-groups per CU
    'persist2_128x128_one_round': plan('v3', '128x128', 72, group_m=8),
    'pred qk_fusion qk_fuse=0': 'available=0',
    'pred fp8_mx_ok fp8_v3=0': 'available=0',
}
# the predicates under (impl, tile): (3, 0), (3, 1), (2, 0) -- and the planner agrees with each
for _mode, _qk, _drop, _conv, _mx in (('(3,0)', 1, 1, 1, 1), ('(3,1)', 1, 1, 0, 1), ('(2,0)', 0, 0, 0, 0)):
    EXPECT[f'pred qk_fusion {_mode}'] = f'available={_qk} planned={_qk}'
    EXPECT[f'pred dropres {_mode}'] = f'available={_drop} planned={_drop}'
    EXPECT[f'pred conv_stats {_mode}'] = f'available={_conv} planned={_conv}'
    EXPECT[f'pred fp8_mx_ok {_mode} K=3072'] = f'available={_mx} planned={_mx}'
    EXPECT[f'pred fp8_mx_ok {_mode} K=3200'] = 'available=0 planned=0'                   # K % 512
    EXPECT[f'pred fp8_mx_ok {_mode} K=256'] = 'available=0 planned=0'                    # K < 512


def test_gemm_plan(lines):
    assert lines == EXPECT
