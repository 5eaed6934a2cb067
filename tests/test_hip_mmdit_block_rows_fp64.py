"""Every MMDiT block of the engine per row and per column against the fp64 block, at the released width (D = 3072, 24 heads; FLUX joint
4096 / pooled 768, Qwen-Image joint 3584): the WIRING of the kernels into a block -- which rows of the joint [text T | image N] matrix
belong to which problem of a grouped launch, which sample's gate / scale / shift slice a row reads, where the k | v | q | mlp column ranges
start, which of the three operand paths a shape takes -- and the packing of the diffusers-named weights (load_state_dict, ModLayout; two
blocks of each kind, so the block stride counts).  The kernels themselves have per-element tests; a whole-matrix rel-L2 (test_hip_engine,
test_production_shape) hides a fault in one row (tests/mmdit_block_ref.py).

Per case: one forward with a checkpoint buffer, so block k's input is ck[k] and its output ck[k + 1] (x_tokens for the last block).  Every
block is judged from its OWN input -- nothing compounds; the conditioning chain enters through the exported temb only -- against
  * y64      the fp64 block (mmdit_block_ref.block64) of the engine's input, on the device;
  * y_eager  oracle/dit_ref.py's block under eager_bf16() (how the reference itself runs) from the same input,
with the project's standing bar (test_full_depth_parity.py) on row and column maxima: in every (sample, stream) group the
engine's worst row / column is no worse than 1.5 x the eager evaluation's worst.  Measured ratios and the detected single-row scaling:
DESIGN.md section 2 (printed here with -s).

Shapes: the smallest that reach each path and boundary (S = N + T rows per sample):
  flux B 1, 16 x 16, T 77, S 333   BASELINE.json configs[0]: QK_EPI, a ragged last tile in both streams
  flux B 2, 12 x 16, T 64, S 256   VT_PROJ (T % 16 == 0, S % 64 == 0: vt_proj_shape_ok): 6 problems per sample in the double blocks; k, q, mlp
                                   and one V^T per sample in the single blocks
  flux B 4,  8 x 14, T 16, S 128   the largest micro-batch: stream_gemm fills all 8 problem slots, the single blocks' VT_PROJ runs at B + 3 = 7
  flux B 2, 16 x 16, T 77          the 8-phase GEMM (set_gemm_mode(2)): no q / k epilogue, so KV_PREP
  qwen B 2, 16 x 16, T 77          QK_EPI
  qwen B 1,  8 x 14, T 16          VT_PROJ
Which path the forward takes is asserted through afx_qkv_operands: the forward picks the first of VT_PROJ, QK_EPI, KV_PREP that can run
(qkv_path() in afx_engine.hip; bf16 linears, AFX_VT_FUSE_OFF unset), and the library refuses a forced path that cannot run on the shape or
with the GEMM kernel in use -- the first forced path it accepts on the engine's own weights is the forward's.
"""
import re

import pytest
import torch

import mmdit_block_ref as R

pytestmark = pytest.mark.gpu

D_MODEL, HEADS = 3072, 24
BAR = 1.5
T_VALUES = [1.0, 0.7619, 0.3, 0.05]           # one per sample: every sample has its own modulation vectors

# (family, B, hp, wp, T, GEMM mode, path of the double blocks, path of the single blocks)
CASES = [
    ('flux', 1, 16, 16, 77, (3, 0), 'qk_epi', 'qk_epi'),
    ('flux', 2, 12, 16, 64, (3, 0), 'vt_proj', 'vt_proj'),
    ('flux', 4, 8, 14, 16, (3, 0), 'vt_proj', 'vt_proj'),
    ('flux', 2, 16, 16, 77, (2, 0), 'kv_prep', 'kv_prep'),
    ('qwen', 2, 16, 16, 77, (3, 0), 'qk_epi', None),
    ('qwen', 1, 8, 14, 16, (3, 0), 'vt_proj', None),
]
TEETH_CASES = [CASES[1], CASES[4]]            # two samples each: the sample-boundary and other-gate faults need a second one

_MODELS, _RUNS = {}, {}


def _model(family):
    """(cfg, diffusers-named weights on the device, engine loaded through load_state_dict): drawn once per module."""
    if family not in _MODELS:
        from arcflow_amd import MMDiTEngine
        from oracle import dit_ref
        if family == 'flux':
            cfg = dit_ref.FluxCfg(num_layers=2, num_single_layers=2)
            w = dit_ref.make_flux_weights(cfg, seed=21, device='cuda')
            eng = MMDiTEngine('flux', 2, 2)
        else:
            cfg = dit_ref.QwenCfg(num_layers=2)
            w = dit_ref.make_qwen_weights(cfg, seed=22, device='cuda')
            eng = MMDiTEngine('qwen', 2, 0, joint_dim=cfg.joint_dim)
        assert cfg.dim == D_MODEL and cfg.heads == HEADS and cfg.joint_dim == (4096 if family == 'flux' else 3584)
        eng.load_state_dict(w)
        _MODELS[family] = (cfg, w, eng)
    return _MODELS[family]


def _blocks(family):
    """(kind, state-dict prefix) of the engine's blocks in checkpoint order."""
    if family == 'qwen':
        return [('qwen', f'transformer_blocks.{i}.') for i in range(2)]
    return [('flux_double', f'transformer_blocks.{i}.') for i in range(2)] + [('flux_single', f'single_transformer_blocks.{i}.') for i in range(2)]


def _forward_path(eng, single, a, B, N, T, cos, sin):
    """The first of the three operand paths afx_qkv_operands accepts for this shape under the GEMM mode in force (module docstring)."""
    from arcflow_amd import _lib, ops
    W = eng._weights
    if single:
        args = ('single', a, W['s0.fused.weight'], W['s0.fused.bias'], W['s0.qknorm'])
    else:
        args = ('double', a, (W['d0.img_qkv.weight'], W['d0.txt_qkv.weight']), (W['d0.img_qkv.bias'], W['d0.txt_qkv.bias']), W['d0.qknorm'])
    for path in ('vt_proj', 'qk_epi', 'kv_prep'):
        try:
            ops.qkv_operands(*args, cos, sin, B, N, T, path=path)
            return path
        except _lib.ArcflowHipError:
            continue
    return None


def _run(case):
    """One forward of the case and, per block, its input, the engine's output, the fp64 block and the errors of both evaluations.
    Computed once per case and left unchanged."""
    if case in _RUNS:
        return _RUNS[case]
    from arcflow_amd import ops
    from oracle import dit_ref
    family, B, hp, wp, T, mode, dpath, spath = case
    cfg, w, eng = _model(family)
    N, S = hp * wp, hp * wp + T
    g = torch.Generator(device='cuda').manual_seed(1000 * B + T + mode[0])
    hid = torch.randn(B, N, 64, generator=g, device='cuda').bfloat16()
    ctx = (torch.randn(B, T, cfg.joint_dim, generator=g, device='cuda') * 0.5).bfloat16()
    t = torch.tensor(T_VALUES[:B], device='cuda')
    pooled = gd = None
    if family == 'flux':
        pooled = (torch.randn(B, cfg.pooled_dim, generator=g, device='cuda') * 0.5).bfloat16()
        gd = torch.full((B,), 3.5, device='cuda')
    blocks = _blocks(family)
    ck = torch.zeros(len(blocks), B * S, D_MODEL, dtype=torch.bfloat16, device='cuda')
    x_last = torch.empty(B * S, D_MODEL, dtype=torch.bfloat16, device='cuda')
    temb = torch.empty(B, D_MODEL, device='cuda')
    try:
        ops.set_gemm_mode(*mode)
        eng.set_checkpoint_buffer(ck)
        eng(hid, t, ctx, pooled, gd, hp, wp)
        eng.export('x_tokens', x_last, B, N, T)
        eng.export('temb', temb, B, N, T)
        torch.cuda.synchronize()
        cos, sin = eng.rope_tables(hp, wp, T)
        paths = (_forward_path(eng, False, ck[0], B, N, T, cos, sin), _forward_path(eng, True, ck[0], B, N, T, cos, sin) if spath else None)
        torch.cuda.synchronize()
    finally:
        eng.set_checkpoint_buffer(None)
        ops.set_gemm_mode(3, 0)
    assert torch.isfinite(temb).all() and torch.isfinite(x_last.float()).all()
    if B > 1:                                 # every sample has its own conditioning
        assert (temb[0] - temb[1]).abs().max().item() > 1e-2
    recs = []
    for k, (kind, p) in enumerate(blocks):
        x_in = ck[k].view(B, S, D_MODEL)
        x_out = (ck[k + 1] if k + 1 < len(blocks) else x_last).view(B, S, D_MODEL)
        tables = R.rope_tables(kind, hp, wp, T, 'cuda')
        y64 = R.block64(kind, w, p, HEADS, x_in, temb, T, tables)
        with dit_ref.eager_bf16():
            y_eager = R.oracle_block(kind, w, p, HEADS, x_in, temb, T, tables)
        recs.append(dict(kind=kind, p=p, x_in=x_in, x_out=x_out, y64=y64, tables=tables, temb=temb,
                         hip=R.block_row_col_errors(x_in, x_out, y64, T), eager=R.block_row_col_errors(x_in, y_eager, y64, T),
                         whole_hip=R.whole_rel_l2(x_out, y64), whole_eager=R.whole_rel_l2(y_eager, y64)))
    _RUNS[case] = (paths, recs)
    return _RUNS[case]


def _name(case):
    family, B, hp, wp, T, mode = case[:6]
    return f'{family} B={B} {hp}x{wp} T={T} gemm={mode[0]}'


@pytest.mark.parametrize('case', CASES, ids=_name)
def test_blocks_per_row_and_column_vs_fp64(case):
    (dpath, spath), recs = _run(case)
    assert (dpath, spath) == case[6:], f'{_name(case)}: the forward takes {dpath} / {spath}, the case is meant for {case[6:]}'
    failures = []
    for k, r in enumerate(recs):
        what = f'{_name(case)} block {k} ({r["p"][:-1]}, {dpath if r["kind"] != "flux_single" else spath})'
        assert torch.isfinite(r['hip']['rows']).all() and torch.isfinite(r['eager']['rows']).all(), what
        try:
            ratios = R.assert_rows_cols(r['hip'], r['eager'], BAR, what)
            print(f'{what}: whole-matrix rel-L2 hip {r["whole_hip"]:.2e} eager {r["whole_eager"]:.2e}; hip max / eager max '
                  f'{R.format_ratios(ratios)}; worst {max(ratios.values()):.2f}')
        except AssertionError as e:           # (every block of the case is reported before the test fails)
            print(f'FAIL {e}')
            failures.append(str(e))
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('case', TEETH_CASES, ids=_name)
def test_planted_faults_fail_the_check_on_the_engines_output(case):
    """The planted faults of test_mmdit_block_ref_cpu.py on a copy of the ENGINE's output, the second block of each kind: each is scaled to at
    most 6e-3 of the whole matrix (plant_fault), and the check fails on it and names its row or column.  Reported: the smallest single-row
    scaling 1 + eps of an increment (last text row and first image row of sample 0) the check detects."""
    family, B, hp, wp, T = case[:5]
    _, w, _ = _model(family)
    S = hp * wp + T
    _, recs = _run(case)
    for k, r in enumerate(recs):
        if not r['p'].endswith('.1.'):
            continue
        what = f'{_name(case)} block {k} ({r["p"][:-1]})'
        other = R.block64(r['kind'], w, r['p'], HEADS, r['x_in'], r['temb'], T, r['tables'], gate_rows=R.other_gate_rows(B, S, 'cuda'))
        for fault in R.FAULTS:
            faulty, where, alpha = R.plant_fault(fault, r['x_in'], r['x_out'], r['y64'], T, other)
            whole = R.whole_rel_l2(faulty, r['y64'])
            with pytest.raises(AssertionError) as ei:
                R.assert_rows_cols(R.block_row_col_errors(r['x_in'], faulty, r['y64'], T), r['eager'], BAR, what)
            assert re.search(R.fault_message(where), str(ei.value)), (fault, where, str(ei.value))
            print(f'{what} {fault}: alpha {alpha:.3f}, whole-matrix rel-L2 {r["whole_hip"]:.2e} -> {whole:.2e} (bound {R.OLD_BOUND}), caught at {where}')
        eps = [R.smallest_detected_scaling(r['x_in'], r['x_out'], r['y64'], r['eager'], T, 0, row, BAR) for row in (T - 1, T)]
        print(f'{what}: smallest detected single-row scaling eps: text row {T - 1}: {eps[0]}, image row {T}: {eps[1]}')
        assert all(e is not None for e in eps), eps          # (None: not even a row that is 50 % wrong would be seen)
