"""tests/lora_block_grad_ref.py without a kernel, at a toy width (2 heads, D = 256, rank 16, 13 text + 24 image rows, one sample): (1) the
fp64 gradients of a block -- with the '.lora' branch of lin64, the modulation handed in as the bias of a zeroed modulation linear, the
slice order of the engine -- against fp32 autograd through oracle/dit_ref.py's own block per element; (2) the statistic on dit_ref's
eager-bf16 evaluation, every reference denominator > 0; (3) every planted fault stays within 5e-2 of each whole tensor (the train-step
tests assert 8e-2) and fails the check, which names the tensor and the row, column or slice it was planted in."""
import re

import pytest
import torch

import lora_block_grad_ref as G
import mmdit_block_ref as R
from oracle import dit_ref

HEADS, HP, WP, T, RANK, P_DROP = 2, 4, 6, 13, 16, 0.05
N, S, D = HP * WP, HP * WP + T, HEADS * 128
BAR = 1.5
CASES = [('flux_double', True), ('flux_single', True), ('qwen', True), ('qwen', False)]       # (kind, the txt MLP is adapted)
_IDS = ['flux_double', 'flux_single', 'qwen', 'qwen_txt_unadapted']
_CACHE = {}


def _masks(g, ads):
    ks = {}
    for n, s in ads:
        rows = G.stream_rows(s, T, S)
        in_f = {'.net.0.proj': D, '.net.2': 4 * D, 'proj_mlp': D, 'proj_out': 5 * D}[[k for k in ('.net.0.proj', '.net.2', 'proj_mlp', 'proj_out') if n.endswith(k)][0]]
        ks[n] = (torch.rand(rows.stop - rows.start, in_f, generator=g) >= P_DROP).float() / (1 - P_DROP)
    return ks


def _case(kind, txt_adapted):
    """Everything of one case, computed once and never modified: weights, leaves, the three evaluations, the eager errors."""
    key = (kind, txt_adapted)
    if key in _CACHE:
        return _CACHE[key]
    g = torch.Generator().manual_seed(31 + 7 * G.R.KINDS.index(kind) + int(txt_adapted))
    if kind == 'qwen':
        w = dit_ref.make_qwen_weights(dit_ref.QwenCfg(num_layers=1, heads=HEADS, joint_dim=192), seed=3)
        p = 'transformer_blocks.0.'
    else:
        nd, ns = (1, 0) if kind == 'flux_double' else (0, 1)
        w = dit_ref.make_flux_weights(dit_ref.FluxCfg(num_layers=nd, num_single_layers=ns, heads=HEADS, joint_dim=128, pooled_dim=64), seed=3)
        p = 'transformer_blocks.0.' if nd else 'single_transformer_blocks.0.'
    # the block's linears at the gain they have at the released width (std 0.02 sqrt(3072 / D)): with the generator's 0.02 the branches of a
    # D = 256 block are a third as strong, the increment of dX sinks below the bf16 spacing of dX itself and the statistic measures that rounding
    for k in [k for k in w if k.startswith(p) and k.endswith('.weight') and w[k].dim() == 2 and not any(m in k for m in G.MOD_LINEARS[kind])]:
        w[k] = (w[k].float() * (3072 / D) ** 0.5).bfloat16()
    X = torch.randn(S, D, generator=g).bfloat16().float()
    mod = torch.randn(G.mod_size(kind, D), generator=g) * 0.3
    cot = torch.randn(S, D, generator=g).bfloat16().float()                 # dense
    ads = G.block_adapters(kind, p, txt_adapted)
    ks = _masks(g, ads)
    lora = {}
    for n, _ in ads:
        out_f, in_f = w[n + '.weight'].shape
        lora[n] = ((torch.randn(RANK, in_f, generator=g) / RANK).bfloat16().float(), (torch.randn(out_f, RANK, generator=g) * 0.02).bfloat16().float(), ks[n])
    tables = R.rope_tables(kind, HP, WP, T)
    blocks = [(kind, p, 0)]
    taps = []
    g64 = G.evaluate('fp64', blocks, w, HEADS, X, mod, lora, T, tables, cot, taps=taps)
    g32 = G.evaluate('fp32', blocks, w, HEADS, X, mod, lora, T, tables, cot)
    ge = G.evaluate('eager', blocks, w, HEADS, X, mod, lora, T, tables, cot)
    slices = [(nm, i * D, (i + 1) * D) for i, nm in enumerate(G.slice_names(kind))]
    c = dict(kind=kind, p=p, w=w, X=X, mod=mod, cot=cot, ads=ads, lora=lora, tables=tables, blocks=blocks, taps=taps, g64=g64, g32=g32, ge=ge,
             slices=slices, eager=G.grad_errors(ge, g64, cot, T, slices), gen=g, txt_adapted=txt_adapted)
    _CACHE[key] = c
    return c


def _tensors(gs):
    yield 'dX', gs['dX']
    yield 'dmod', gs['dmod']
    for k in ('dA', 'dB'):
        for n, t in gs[k].items():
            yield f'{k} {n}', t


@pytest.mark.parametrize('kind,txt_adapted', CASES, ids=_IDS)
def test_fp64_gradients_match_fp32_autograd_through_the_oracle(kind, txt_adapted):
    """The bound: forward and backward pass through a chain of about twelve linears whose longest fp32 sum has K <= 5 D = 1280 terms:
    12 x 1280 u of the tensor's magnitude, u = 2^-24 (9e-4 relative).  A transcription error -- the LoRA branch on the un-dropped input, a
    modulation slice in another order, the bias trick reaching the wrong linear -- moves a gradient by 1e-1 and more."""
    c = _case(kind, txt_adapted)
    assert len(c['ads']) == (2 if kind == 'flux_single' else 4 if txt_adapted else 2)
    assert (c['g64']['out'] - c['g32']['out']).abs().max().item() <= 12 * 1280 * 2.0 ** -24 * c['g64']['out'].abs().max().item()
    for (name, t64), (_, t32) in zip(_tensors(c['g64']), _tensors(c['g32'])):
        assert t64.dtype == torch.float64 and t64.shape == t32.shape
        err, bound = (t32 - t64).abs().max().item(), 12 * 1280 * 2.0 ** -24 * t64.abs().max().item()
        assert err <= bound, (kind, name, err / bound)
    # every leaf matters: the modulation and the adapters reach the output, and a mask is not the identity
    assert all(t.abs().max().item() > 0 for _, t in _tensors(c['g64']))
    assert all(0 < (k == 0).float().mean().item() < 3 * P_DROP for _, _, k in c['lora'].values())
    # the LoRA branch is dropped-input: the same evaluation with keep_scale = 1 is another function
    plain = {n: (a, b, 1.0) for n, (a, b, _) in c['lora'].items()}
    g1 = G.evaluate('fp64', c['blocks'], c['w'], HEADS, c['X'], c['mod'], plain, T, c['tables'], c['cot'])
    n0 = c['ads'][0][0]
    assert R.whole_rel_l2(g1['dA'][n0], c['g64']['dA'][n0]) > 1e-2


@pytest.mark.parametrize('kind,txt_adapted', CASES, ids=_IDS)
def test_eager_bf16_evaluation_is_a_finite_nonzero_yardstick(kind, txt_adapted):
    """The reference denominators (asserted > 0 inside grad_errors) come from the fp64 evaluation alone: dXo is dense and p = 0.05.  The
    eager evaluation's own worst errors are finite and non-zero in every group, it passes the check against itself, and the fp32
    evaluation is far inside it."""
    c = _case(kind, txt_adapted)
    e = c['eager']
    n_groups = 1 + 2 + 4 * len(c['ads'])
    assert len(e) == n_groups
    assert e['dmod rel-L2'].numel() == (3 if kind == 'flux_single' else 12)
    for grp, v in e.items():
        vals = torch.cat([v['rows'].flatten(), v['cols'].flatten()]) if grp == 'dX' else v
        assert torch.isfinite(vals).all() and 0 < vals.max().item() < 0.5, (grp, vals.max().item())
    n0 = c['ads'][0][0]
    assert e[f'dA {n0} rows'].numel() == RANK and e[f'dA {n0} cols'].numel() == D and e[f'dB {n0} rows'].numel() == 4 * D
    print(kind, 'worst errors of the eager evaluation: dX increment row', e['dX']['rows'].max().item(),
          'dA row', max(v.max().item() for k, v in e.items() if k.startswith('dA') and k.endswith('rows')),
          'dB row', max(v.max().item() for k, v in e.items() if k.startswith('dB') and k.endswith('rows')),
          'dmod slice', e['dmod rel-L2'].max().item())
    ratios = G.assert_grads(e, e, BAR, c['slices'], kind)
    assert all(v == 1.0 for v in ratios.values())
    e32 = G.grad_errors(c['g32'], c['g64'], c['cot'], T, c['slices'])
    G.assert_grads(e32, e, 0.01, c['slices'], kind)
    with pytest.raises(AssertionError):
        G.assert_grads(e, e32, BAR, c['slices'], kind)


# (a single block has one stream and one scale, a double block one d_shift per stream: each fault where it can be planted)
_FAULT_CASES = [(k, t, f) for (k, t) in CASES for f in G.FAULTS if G.fault_applies(f, k, t)]


def test_every_fault_is_planted_somewhere():
    assert {f for _, _, f in _FAULT_CASES} == set(G.FAULTS) and len(_FAULT_CASES) == 5 + 3 + 5 + 4


@pytest.mark.parametrize('kind,txt_adapted,fault', _FAULT_CASES, ids=[f'{_IDS[CASES.index((k, t))]}-{f}' for k, t, f in _FAULT_CASES])
def test_planted_fault_stays_inside_the_whole_tensor_bound_and_fails_the_check(kind, txt_adapted, fault):
    c = _case(kind, txt_adapted)
    wrong = None
    if fault == 'txt_mask_row0':
        n = [x for x, s in c['ads'] if s == 'txt'][0]
        other = dict(c['lora'])
        a, b, k = other[n]
        k2 = (torch.rand(k.shape, generator=torch.Generator().manual_seed(99)) >= P_DROP).float() / (1 - P_DROP)
        assert 0 < (k2 != k).float().mean().item() < 3 * P_DROP
        other[n] = (a, b, k2)
        gw = G.evaluate('fp64', c['blocks'], c['w'], HEADS, c['X'], c['mod'], other, T, c['tables'], c['cot'])
        differs = ((k2 != k).sum(0) > 0)                     # the fault is limited to the columns in which some row's keep flag differs
        assert differs.any() and not differs.all()
        wrong = (torch.where(differs[None], gw['dA'][n], c['g64']['dA'][n]), gw['dX'])
    faulty, where, alphas = G.plant_fault(fault, kind, c['p'], c['g64'], c['X'], c['mod'], c['cot'], T, c['taps'], wrong, txt_adapted)
    whole = G.whole_rel_l2(faulty, c['g64'])
    print(kind, fault, 'alpha', alphas, 'whole-tensor rel-L2', {k: f'{v:.2e}' for k, v in whole.items() if v > 0})
    assert all(0 < a <= 1 for a in alphas.values())
    assert 0 < max(whole.values()) <= G.FAULT_BUDGET * (1 + 1e-9), whole
    with pytest.raises(AssertionError) as ei:
        G.assert_grads(G.grad_errors(faulty, c['g64'], c['cot'], T, c['slices']), c['eager'], BAR, c['slices'], f'{kind} {fault}')
    assert re.search(where, str(ei.value)), (where, str(ei.value))


def test_smallest_detected_row_scaling_of_the_dx_increment():
    c = _case('flux_double', True)
    for row in (T - 1, T):
        eps = G.smallest_detected_scaling(c['ge'], c['g64'], c['eager'], c['cot'], T, row, BAR)
        stream = slice(0, T) if row < T else slice(T, S)
        worst = c['eager']['dX']['rows'][0, stream].max().item()
        print(f'smallest detected scaling of dX increment row {row}: eps = {eps}; the eager evaluation\'s worst row of that stream {worst:.2e}')
        assert eps is not None and eps <= 4 * BAR * worst, (eps, worst)
