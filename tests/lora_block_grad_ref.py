"""The LoRA trunk's block BACKWARD against autograd: the gradient of one MMDiT block (or of the whole chain of blocks behind norm_out's
modulate) from the block's own input, for ONE sample, evaluated (1) in fp64 (mmdit_block_ref.block64 with the '.lora' branch of lin64), and
(2) the way the reference itself runs it (oracle/dit_ref.py under eager_bf16(): every op output AND, through autograd, every gradient at the
same points rounded to bf16), plus the per-row / per-column / per-slice statistic, the one assertion built on it and the planted faults of
its teeth checks -- shared by test_lora_block_grad_ref_cpu.py (the helper alone) and test_hip_lora_trunk_backward_fp64.py (the trunk at the
released width).  The backward twin of mmdit_block_ref.py: a whole-tensor rel-L2 per adapter (test_distill.py, < 8e-2) cannot see one row
of dB lost at a row0 boundary, a mask regenerated at the wrong global row for one stream, a d_gate read from the other branch's output or
one row of dX taking the other stream's scale.

Leaves: the block input X [S, D] (text rows first), the modulation vector `mod` (12 D per double block: shift, scale, gate, x 2, image then
text; 3 D per single block; the engine's order) and A [r, in] / B [out, r] of every adapter.  The modulation becomes a leaf WITHOUT a
change to the oracle: in a copy of the weight dict the block's modulation linears get a zero weight and the sample's slice of `mod` as
bias, so with one sample the linear's output IS the bias.  Dropout masks are inputs (keep_scale = keep / (1 - p), [rows of the adapter's
stream, in]).  Loss: (block(X) . dXo).sum() for a given dXo -- or, with `final`, (modulate(X_out[image rows], scale, shift) . dxn).sum()
with norm_out's (scale, shift) = mod[final : final + 2 D], scale first.

Statistic (grad_errors): dX by mmdit_block_ref.block_row_col_errors on the gradient's increment dX - dXo (rows and columns per stream,
never pooled); dmod per D-slice, the slice's rel-L2 and its largest element error over the slice's RMS; dA and dB the rel-L2 of every row
and of every column.  Every denominator comes from the fp64 reference and is asserted > 0; no row, column or slice is left out.
Assertion (assert_grads): in every group the worst value of the evaluation under test is at most bar x the worst of the eager-bf16
evaluation in that group (maxima, as assert_rows_cols); a failure names the tensor and its row, column or slice.
"""
import contextlib

import torch

import mmdit_block_ref as R
from oracle import dit_ref

FAULT_BUDGET = 5e-2       # whole-tensor rel-L2 a planted fault is scaled to: below the 8e-2 of test_lora_trunk_backward_matches_cpu_autograd

MOD_LINEARS = {'flux_double': ('norm1.linear', 'norm1_context.linear'), 'flux_single': ('norm.linear',), 'qwen': ('img_mod.1', 'txt_mod.1')}
_SLICES6 = ('shift1', 'scale1', 'gate1', 'shift2', 'scale2', 'gate2')


def mod_size(kind, D):
    return 3 * D if kind == 'flux_single' else 12 * D


def slice_names(kind):
    if kind == 'flux_single':
        return ['shift', 'scale', 'gate']
    return [f'{s} {c}' for s in ('img', 'txt') for c in _SLICES6]


def block_adapters(kind, p, txt_adapted=True):
    """((diffusers name of the adapted linear, stream), ...) of block `p` in the trunk's order (lora_targets): stream 'img' / 'txt' -- the
    image / text rows of the joint matrix -- or 'all' (single block)."""
    if kind == 'flux_single':
        return [(p + 'proj_mlp', 'all'), (p + 'proj_out', 'all')]
    ffs = (('img', 'ff'), ('txt', 'ff_context')) if kind == 'flux_double' else (('img', 'img_mlp'), ('txt', 'txt_mlp'))
    return [(p + ff + nm, s) for s, ff in ffs if s == 'img' or txt_adapted for nm in ('.net.0.proj', '.net.2')]


def stream_rows(stream, T, S):
    return {'img': slice(T, S), 'txt': slice(0, T), 'all': slice(0, S)}[stream]


def _with_leaves(w, blocks, mod, lora):
    """A copy of the weight dict `w` whose modulation linears of `blocks` ((kind, prefix, offset into mod), ...) return the slices of
    `mod`, and whose adapted linears carry their '.lora' entry."""
    ww = dict(w)
    for kind, p, m0 in blocks:
        for nm in MOD_LINEARS[kind]:
            n = w[p + nm + '.weight'].shape[0]
            ww[p + nm + '.weight'] = torch.zeros_like(w[p + nm + '.weight'])
            ww[p + nm + '.bias'] = mod[m0:m0 + n]
            m0 += n
    for name, abk in lora.items():
        ww[name + '.lora'] = abk
    return ww


@contextlib.contextmanager
def _tap_modulate(taps):
    """Every modulate64 call of the fp64 blocks records (input, scale, output); the output keeps its gradient.  (The planted faults are
    built from these: the gradient at a norm's output, the residual stream between the two halves of a block.)"""
    orig = R.modulate64

    def tapped(x, scale, shift):
        y = orig(x, scale, shift)
        taps.append((x, scale, y))
        return y
    R.modulate64 = tapped
    try:
        yield
    finally:
        R.modulate64 = orig


def evaluate(mode, blocks, w, heads, X, mod, lora, T, tables, cot, final=None, taps=None, round_dx=True):
    """Gradients of the chain `blocks` ((kind, prefix, offset of the block's slice in mod), ...) from its input X [S, D], one sample.
    mode: 'fp64', 'fp32' (dit_ref's own blocks) or 'eager' (the same under eager_bf16()).  lora: {linear name: (A, B, keep_scale)}.
    cot: dXo [S, D], or with final = offset of norm_out's (scale, shift) in mod the gradient dxn [N, D] at norm_out's output.
    round_dx (mode 'eager' only): dX is rounded to bf16, as the reference's own chain rounds it -- the gradient reaches the block in front
    through the `_r` of that block's last gated_add, whose backward casts it to bf16 -- and as the trunk hands dX from block to block (a
    bf16 [S, D] buffer by design); evaluated as a leaf's gradient the block would otherwise be spared the one rounding every block's dX has.
    Returns {'dX' [S, D], 'dmod' like mod, 'dA': {name: [r, in]}, 'dB': {name: [out, r]}, 'out': the chain's output [S, D]} in fp64."""
    dt = torch.float64 if mode == 'fp64' else torch.float32
    D = X.shape[1]
    Xl = X.to(dt)[None].clone().requires_grad_(True)
    ml = mod.to(dt).clone().requires_grad_(True)
    ll = {n: (a.to(dt).clone().requires_grad_(True), b.to(dt).clone().requires_grad_(True), k if not torch.is_tensor(k) else k.to(dt))
          for n, (a, b, k) in lora.items()}
    ww = _with_leaves(w, blocks, ml, ll)
    temb = torch.zeros(1, D, dtype=dt, device=X.device)
    ctx = dit_ref.eager_bf16() if mode == 'eager' else contextlib.nullcontext()
    tap = _tap_modulate(taps) if (taps is not None and mode == 'fp64') else contextlib.nullcontext()
    with ctx, tap:
        y = Xl
        for kind, p, _ in blocks:
            y = R.block64(kind, ww, p, heads, y, temb, T, tables) if mode == 'fp64' else R.oracle_block(kind, ww, p, heads, y, temb, T, tables)
        out = y
        if final is not None:
            sc, sh = ml[final:final + D][None], ml[final + D:final + 2 * D][None]
            y = R.modulate64(y[:, T:], sc, sh) if mode == 'fp64' else dit_ref.modulate(y[:, T:], sc, sh)
        loss = (y[0] * cot.to(dt)).sum()
    names = list(ll)
    leaves = [Xl, ml] + [ll[n][0] for n in names] + [ll[n][1] for n in names]
    tapped = [t[2] for t in taps] if (taps is not None and mode == 'fp64') else []
    g = torch.autograd.grad(loss, leaves + tapped)
    if tapped:                                    # (x, scale, d loss / d output) of every modulate call
        taps[:] = [(x.detach()[0], s.detach()[0], gi[0]) for (x, s, _), gi in zip(taps, g[len(leaves):])]
    k = len(names)
    if mode == 'eager' and round_dx:
        g = (g[0].bfloat16().float(),) + tuple(g[1:])
    return {'dX': g[0][0].double(), 'dmod': g[1].double(), 'dA': {n: g[2 + i].double() for i, n in enumerate(names)},
            'dB': {n: g[2 + k + i].double() for i, n in enumerate(names)}, 'out': out.detach()[0].double()}


# ------------------------------------------------------------------------------------------------ the statistic and the assertion
def _rel(err, ref, dim):
    den = ref.norm(dim=dim)
    assert bool((den > 0).all()), 'a reference denominator is zero'
    return err.norm(dim=dim) / den


def grad_errors(got, ref, cot, T, slices, with_dx=True, zero_slices_exact=False):
    """Errors of the gradient set `got` against the fp64 set `ref` (the dicts of evaluate; got may hold the trunk's tensors in any dtype).
    slices: ((name, a, b), ...) of dmod.  Returns {group: values}; group 'dX' holds block_row_col_errors of the increment.
    zero_slices_exact: a dmod slice that is exactly zero in the reference has to be exactly zero in `got` and has no quotient (value 0)."""
    e = {}
    if with_dx:
        inc = ref['dX'] - cot.double()
        assert bool((inc.norm(dim=1) > 0).all()) and bool((inc[:T].norm(dim=0) > 0).all()) and bool((inc[T:].norm(dim=0) > 0).all())
        e['dX'] = R.block_row_col_errors(cot[None], got['dX'][None], ref['dX'][None], T)
    gm, rm = got['dmod'].double(), ref['dmod'].double()
    l2, mx = [], []
    for nm, a, b in slices:
        den = rm[a:b].norm()
        if zero_slices_exact and den.item() == 0:         # (the chain: the last double block's text MLP half does not reach the image rows)
            assert not gm[a:b].any(), f'dmod slice {nm} is exactly zero in the reference and is not in the evaluation under test'
            l2.append(den)
            mx.append(den)
            continue
        assert den.item() > 0, 'a dmod slice of the reference is zero'
        l2.append((gm[a:b] - rm[a:b]).norm() / den)
        mx.append((gm[a:b] - rm[a:b]).abs().max() / (den / (b - a) ** 0.5))
    e['dmod rel-L2'] = torch.stack(l2)
    e['dmod max/rms'] = torch.stack(mx)
    for k in ('dA', 'dB'):
        for n, r in ref[k].items():
            err = got[k][n].double() - r
            e[f'{k} {n} rows'] = _rel(err, r, 1)
            e[f'{k} {n} cols'] = _rel(err, r, 0)
    return e


def _label(group, i, slices):
    if group.startswith('dmod'):
        return f'{group} slice {slices[i][0]}'
    return f'{group[:-5]} {"row" if group.endswith("rows") else "column"} {i}'


def assert_grads(hip, eager, bar, slices, what=''):
    """In every group (dX rows / columns per stream; the dmod slices, both statistics; every adapter's dA and dB, rows and columns): the
    largest error of `hip` is at most bar x the largest of `eager`.  Returns {group: hip max / eager max}; a failure names the tensor and
    the row, column or slice."""
    ratios, bad = {}, []
    assert set(hip) == set(eager)
    for group, h in hip.items():
        if group == 'dX':
            try:
                ratios.update({f'dX {s} {a}': v for (_, s, a), v in R.assert_rows_cols(h, eager[group], bar, 'dX').items()})
            except AssertionError as ex:
                bad.append(str(ex).replace('sample 0 ', 'dX '))
            continue
        hmax, emax = h.max().item(), eager[group].max().item()
        ratios[group] = hmax / emax if emax > 0 else float('inf')
        if not hmax <= bar * emax:
            i = int(torch.nan_to_num(h, nan=float('inf')).argmax())
            bad.append(f'{_label(group, i, slices)}: error {h[i].item():.3e} > {bar} x {emax:.3e}, the largest of the eager-bf16 evaluation '
                       f'over the {h.numel()} of this group')
    if bad:
        raise AssertionError(f'{what}: ' + '; '.join(bad))
    return ratios


def format_ratios(ratios):
    """The worst ratio per tensor kind (dX rows / cols per stream, dmod, dA, dB): one line."""
    worst = {}
    for g, v in ratios.items():
        k = g if g.startswith('dX') or g.startswith('dmod') else g.split()[0] + ' ' + g.split()[-1]
        worst[k] = max(worst.get(k, 0.0), v)
    return ' '.join(f'{k.replace(" ", "/")}={v:.2f}' for k, v in worst.items())


def whole_rel_l2(got, ref):
    """The old statistic: one rel-L2 per tensor."""
    out = {'dmod': R.whole_rel_l2(got['dmod'], ref['dmod'])}
    if 'dX' in got:
        out['dX'] = R.whole_rel_l2(got['dX'], ref['dX'])
    for k in ('dA', 'dB'):
        for n in ref[k]:
            out[f'{k} {n}'] = R.whole_rel_l2(got[k][n], ref[k][n])
    return out


# ------------------------------------------------------------------------------------------------ planted faults
FAULTS = ('dx_row_other_scale', 'db_first_row_zero', 'da_col_neighbour', 'txt_mask_row0', 'dgate2_attn_branch', 'dshift_txt_missing')


def _copy(g):
    return {'dX': g['dX'].double().clone(), 'dmod': g['dmod'].double().clone(), 'dA': {n: t.double().clone() for n, t in g['dA'].items()},
            'dB': {n: t.double().clone() for n, t in g['dB'].items()}}


def _scaled(d, ref, budget):
    return min(1.0, budget * ref.norm().item() / d.norm().item())


def _ln_vjp(x_row, g_row):
    """LN^T g at x: the pull-back of layer_norm64 for one row."""
    x = x_row.clone().requires_grad_(True)
    return torch.autograd.grad((R.layer_norm64(x) * g_row).sum(), x)[0]


def fault_applies(fault, kind, txt_adapted=True):
    if fault in ('dx_row_other_scale', 'dgate2_attn_branch'):
        return kind != 'flux_single'
    if fault == 'txt_mask_row0':
        return kind != 'flux_single' and txt_adapted
    if fault == 'dshift_txt_missing':
        return kind == 'flux_single'
    return True


def plant_fault(fault, kind, p, g64, X, mod, cot, T, taps, wrong_mask=None, txt_adapted=True, budget=FAULT_BUDGET, base=None):
    """A copy of the fp64 gradient set g64 of ONE block (mod = its own 12 D / 3 D) with one wiring fault, and the regular expression the
    failure message of assert_grads has to match.  taps: what evaluate(..., taps=[]) recorded.  Every fault is the difference d between
    the faulty and the right tensor scaled by alpha = min(1, budget ||tensor|| / ||d||): the tensor's whole rel-L2 stays <= budget.

      dx_row_other_scale   the last text row of dX takes the norm1 increment computed with the IMAGE stream's scale1 (double blocks);
      db_first_row_zero    the first row of the first adapter's dB (proj_mlp / mlp1: the row0 boundary of the packed weight) is zero;
      da_col_neighbour     the quietest column of the second adapter's (mlp2 / proj_out) dA takes its neighbour's values;
      txt_mask_row0        the text stream's mlp1 mask is drawn at another row offset: `wrong_mask` = (dA of that adapter, dX) of an
                           evaluation with that mask, the caller having limited dA to the columns where a row's keep flag differs; of dX
                           only the text rows are taken;
      dgate2_attn_branch   d_gate2 of the text stream is sum_rows dXo . y1 (the attention branch output) where y2 (the MLP branch) is meant;
      dshift_txt_missing   the text rows' contribution is missing from one element of d_shift (single block: one joint stream).
    Returns (faulty set, regex, {tensor: alpha})."""
    S, D = X.shape
    f = _copy(g64 if base is None else base)         # (base: the set the fault is planted into, e.g. the trunk's own output)
    ads = block_adapters(kind, p, txt_adapted)
    alphas = {}
    if fault == 'dx_row_other_scale':
        # taps of a double block: 0 img norm1, 1 txt norm1, 2 img norm2, 3 txt norm2
        (_, sc_i, _), (x_t, sc_t, gy_t) = taps[0], taps[1]
        d = torch.zeros_like(f['dX'])
        d[T - 1] = _ln_vjp(x_t[T - 1], gy_t[T - 1] * (1 + sc_i)) - _ln_vjp(x_t[T - 1], gy_t[T - 1] * (1 + sc_t))
        alphas['dX'] = a = _scaled(d, g64['dX'], budget)
        f['dX'] += a * d
        where = rf'dX text row {T - 1}:'
    elif fault == 'db_first_row_zero':
        n = ads[0][0]
        d = torch.zeros_like(f['dB'][n])
        d[0] = -f['dB'][n][0]
        alphas[f'dB {n}'] = a = _scaled(d, g64['dB'][n], budget)
        f['dB'][n] += a * d
        where = rf'dB {n} row 0:'
    elif fault == 'da_col_neighbour':
        n = ads[1][0]
        t = f['dA'][n]
        c = int(t.norm(dim=0).argmin())
        d = torch.zeros_like(t)
        d[:, c] = t[:, c + 1 if c + 1 < t.shape[1] else c - 1] - t[:, c]
        alphas[f'dA {n}'] = a = _scaled(d, t, budget)
        f['dA'][n] += a * d
        where = rf'dA {n} column {c}:'
    elif fault == 'txt_mask_row0':
        n = [x for x, s in ads if s == 'txt'][0]
        dA_w, dX_w = wrong_mask
        d = dA_w - g64['dA'][n]
        alphas[f'dA {n}'] = a = _scaled(d, g64['dA'][n], budget)
        f['dA'][n] += a * d
        dx = torch.zeros_like(f['dX'])
        dx[:T] = (dX_w - g64['dX'])[:T]
        alphas['dX'] = a = _scaled(dx, g64['dX'], budget)
        f['dX'] += a * dx
        where = rf'dA {n} column \d+:'
    elif fault == 'dgate2_attn_branch':
        x_t, x1_t = taps[1][0], taps[3][0]                       # the text stream's input and its residual stream after the attention half
        g1 = mod[8 * D:9 * D].double()                           # txt gate1
        y1 = (x1_t - x_t) / g1
        d = torch.zeros_like(f['dmod'])
        d[11 * D:12 * D] = (cot.double()[:T] * y1).sum(0) - g64['dmod'][11 * D:12 * D]
        alphas['dmod'] = a = _scaled(d, g64['dmod'], budget)
        f['dmod'] += a * d
        where = r'dmod [\w/-]+ slice txt gate2:'
    elif fault == 'dshift_txt_missing':
        gy = taps[0][2]                                          # d loss / d Xn of the joint stream
        c = int(gy[:T].sum(0).abs().argmax())
        d = torch.zeros_like(f['dmod'])
        d[c] = -gy[:T, c].sum()
        alphas['dmod'] = a = _scaled(d, g64['dmod'], budget)
        f['dmod'] += a * d
        where = r'dmod max/rms slice shift:'
    else:
        raise ValueError(fault)
    return f, where, alphas


def smallest_detected_scaling(got, ref, eager_err, cot, T, row, bar):
    """The smallest eps = 2^-k down to which a scaling (1 + eps) of row `row` of got's dX increment fails the dX part of the check."""
    return R.smallest_detected_scaling(cot[None], got['dX'][None], ref['dX'][None], eager_err['dX'], T, 0, row, bar)
