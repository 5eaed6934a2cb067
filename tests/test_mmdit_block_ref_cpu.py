"""tests/mmdit_block_ref.py without a kernel, at a toy width (2 heads, D = 256, B = 2, 13 text rows): (1) the fp64 blocks against
oracle/dit_ref.py's fp32 blocks per element; (2) the statistic and the assertion on dit_ref's own bf16 evaluation, which stands in for the
engine here; (3) every planted fault stays below the whole-matrix bound of the block tests and fails the row / column check, which names
the row or column it was planted in."""
import re

import pytest
import torch

import mmdit_block_ref as R
from oracle import dit_ref

HEADS, B, HP, WP, T = 2, 2, 6, 10, 13          # S = 73: neither stream a multiple of 16
BAR = 1.5


def _case(kind):
    """(w, prefix, x_in [B, S, D] bf16 values, temb [B, D], tables): the block's input and conditioning come out of dit_ref's own embedders,
    one timestep per sample."""
    g = torch.Generator().manual_seed(11 + R.KINDS.index(kind))
    t = torch.tensor([1.0, 0.3])
    N = HP * WP
    hid = torch.randn(B, N, 64, generator=g).bfloat16().float()
    if kind == 'qwen':
        cfg = dit_ref.QwenCfg(num_layers=1, heads=HEADS, joint_dim=192)
        w = dit_ref.make_qwen_weights(cfg, seed=2)
        ctx = (torch.randn(B, T, cfg.joint_dim, generator=g) * 0.5).bfloat16().float()
        img, txt = dit_ref.lin(w, 'img_in', hid), dit_ref.lin(w, 'txt_in', dit_ref.rms_norm(ctx, w['txt_norm.weight']))
        temb = dit_ref.mlp_embed(w, 'time_text_embed.timestep_embedder', dit_ref.sincos_embedding(dit_ref.cond_cast(t), scale=1000.0))
        p = 'transformer_blocks.0.'
    else:
        nd, ns = (1, 0) if kind == 'flux_double' else (0, 1)
        cfg = dit_ref.FluxCfg(num_layers=nd, num_single_layers=ns, heads=HEADS, joint_dim=128, pooled_dim=64)
        w = dit_ref.make_flux_weights(cfg, seed=2)
        ctx = (torch.randn(B, T, cfg.joint_dim, generator=g) * 0.5).bfloat16().float()
        pooled = (torch.randn(B, cfg.pooled_dim, generator=g) * 0.5).bfloat16().float()
        img, txt = dit_ref.lin(w, 'x_embedder', hid), dit_ref.lin(w, 'context_embedder', ctx)
        temb = dit_ref.flux_temb(w, cfg, t, torch.full((B,), 3.5), pooled)
        p = 'transformer_blocks.0.' if nd else 'single_transformer_blocks.0.'
    x_in = torch.cat([txt, img], dim=1).bfloat16().float()
    return w, p, x_in, temb, R.rope_tables(kind, HP, WP, T)


_CACHE = {}


def _evaluated(kind):
    """... with the fp64 block, the fp32 and the eager-bf16 oracle blocks and the eager errors: computed once, never modified."""
    if kind not in _CACHE:
        w, p, x_in, temb, tables = _case(kind)
        y64 = R.block64(kind, w, p, HEADS, x_in, temb, T, tables)
        y32 = R.oracle_block(kind, w, p, HEADS, x_in, temb, T, tables)
        with dit_ref.eager_bf16():
            y_eager = R.oracle_block(kind, w, p, HEADS, x_in, temb, T, tables)
        _CACHE[kind] = dict(w=w, p=p, x_in=x_in, temb=temb, tables=tables, y64=y64, y32=y32, y_eager=y_eager,
                            eager=R.block_row_col_errors(x_in, y_eager, y64, T))
    return _CACHE[kind]


@pytest.mark.parametrize('kind', R.KINDS)
def test_fp64_blocks_match_the_fp32_oracle_per_element(kind):
    """The bound: the longest fp32 sum of a block at this width is proj_out's / the mlp down-projection's, K <= 5 D = 1280 terms, and an
    output passes through a chain of six such linears (modulation, q/k/v, out, mlp up, mlp down) plus LayerNorm and softmax sums of
    <= 256 terms: 6 x 1280 u of the output's magnitude, u = 2^-24 (4.6e-4 relative).  A transcription error in the fp64 block -- a swapped
    chunk, the other stream's norm weight, shift and scale exchanged -- moves elements by 1e-1 and more."""
    c = _evaluated(kind)
    assert c['y64'].dtype == torch.float64 and c['y64'].shape == c['x_in'].shape
    bound = 6 * 1280 * 2.0 ** -24 * c['y64'].abs().amax(dim=-1, keepdim=True)
    err = (c['y32'].double() - c['y64']).abs()
    assert bool((err <= bound).all()), (kind, (err / bound).max().item())
    # and the block does something on every row: the statistic divides by the increment's norm, which has to stand clear of the bf16
    # spacing of the row itself (2^-8 relative) for the quotient to measure the block and not the rounding of x
    inc = (c['y64'] - c['x_in'].double()).norm(dim=2) / c['x_in'].double().norm(dim=2)
    assert inc.min().item() > 4 * 2.0 ** -8, inc.min().item()


@pytest.mark.parametrize('kind', R.KINDS)
def test_eager_bf16_oracle_passes_the_check_against_itself(kind):
    c = _evaluated(kind)
    e = c['eager']
    S = HP * WP + T
    assert e['rows'].shape == (B, S) and e['cols'].shape == (B, 2, HEADS * 128)
    # by hand, one row and one column
    err, inc = c['y_eager'].double() - c['y64'], c['y64'] - c['x_in'].double()
    assert e['rows'][1, T].item() == pytest.approx((err[1, T].norm() / inc[1, T].norm()).item(), rel=1e-12)
    assert e['cols'][1, 0, 7].item() == pytest.approx((err[1, :T, 7].norm() / inc[1, :T, 7].norm()).item(), rel=1e-12)
    assert e['cols'][0, 1, 9].item() == pytest.approx((err[0, T:, 9].norm() / inc[0, T:, 9].norm()).item(), rel=1e-12)
    ratios = R.assert_rows_cols(e, e, BAR, kind)
    assert len(ratios) == B * 2 * 2 and all(v == 1.0 for v in ratios.values())
    # bf16 rounding noise, not zero and not large: the eager evaluation is a meaningful yardstick for the rows.  (Columns: at this width the
    # image rows' increment is 5 % of x, and in its quietest columns it lies below the bf16 spacing of x -- their error is the increment
    # itself, a quotient of about 1; the median column is at the rows' level.)
    assert 1e-3 < e['rows'].max().item() < 0.2 and 1e-3 < e['cols'].median().item() < 0.2
    # the fp32 oracle is far inside the bar; the bar is not vacuous the other way round either
    R.assert_rows_cols(R.block_row_col_errors(c['x_in'], c['y32'], c['y64'], T), e, 0.01, kind)
    with pytest.raises(AssertionError):
        R.assert_rows_cols(e, R.block_row_col_errors(c['x_in'], c['y32'], c['y64'], T), BAR, kind)


@pytest.mark.parametrize('fault', R.FAULTS)
@pytest.mark.parametrize('kind', R.KINDS)
def test_planted_fault_passes_the_whole_matrix_bound_and_fails_the_check(kind, fault):
    """The gap in numbers: the faulty output is within OLD_BOUND of the fp64 block over the whole token matrix, and the row / column
    check fails on it, naming the planted row or column."""
    c = _evaluated(kind)
    S = HP * WP + T
    other = None
    if fault == 'row_other_gate':
        other = R.block64(kind, c['w'], c['p'], HEADS, c['x_in'], c['temb'], T, c['tables'], gate_rows=R.other_gate_rows(B, S))
        changed = ((other - c['y64']).abs().amax(dim=2) > 0)
        assert changed.sum().item() == 1 and bool(changed[1, 0])          # the gate is row-local: no other row moves
    clean = R.whole_rel_l2(c['y_eager'], c['y64'])
    faulty, where, alpha = R.plant_fault(fault, c['x_in'], c['y_eager'], c['y64'], T, other)
    whole = R.whole_rel_l2(faulty, c['y64'])
    print(f'{kind} {fault}: alpha {alpha:.3f}, whole-matrix rel-L2 {clean:.2e} -> {whole:.2e} (bound {R.OLD_BOUND})')
    assert 0 < alpha <= 1 and clean < whole < R.OLD_BOUND
    with pytest.raises(AssertionError) as ei:
        R.assert_rows_cols(R.block_row_col_errors(c['x_in'], faulty, c['y64'], T), c['eager'], BAR, f'{kind} {fault}')
    assert re.search(R.fault_message(where), str(ei.value)), (where, str(ei.value))
    e = R.block_row_col_errors(c['x_in'], faulty, c['y64'], T)
    if where[1] is not None:                 # a row fault: the planted row is the worst of its group
        group = slice(0, T) if where[2] == 'text' else slice(T, S)
        assert int(e['rows'][where[1], group].argmax()) + group.start == where[3]
    else:                                    # the column fault: the planted column is the worst of every group
        assert bool((e['cols'].argmax(dim=2) == where[3]).all())


def test_smallest_detected_scaling_is_monotone_and_small():
    """A single row's increment scaled by 1 + eps: detected down to an eps of the order of the eager evaluation's own worst row."""
    c = _evaluated('flux_double')
    eps = R.smallest_detected_scaling(c['x_in'], c['y_eager'], c['y64'], c['eager'], T, 0, T - 1, BAR)
    worst = c['eager']['rows'][0, :T].max().item()
    assert eps is not None and eps <= 4 * BAR * worst, (eps, worst)
    # the undetected side: half of it passes
    R.assert_rows_cols(R.block_row_col_errors(c['x_in'], R.scale_row(c['x_in'], c['y_eager'], 0, T - 1, eps / 2), c['y64'], T), c['eager'], BAR)
