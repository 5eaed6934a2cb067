"""fp64 restatement of the three MMDiT blocks of oracle/dit_ref.py on the engine's joint layout, the per-row / per-column statistic of a
block's increment, the one assertion built on it and the planted faults of its teeth checks -- shared by test_mmdit_block_ref_cpu.py (the
helper alone), test_hip_mmdit_block_rows_fp64.py (the engine's blocks at the released width) and test_production_shape.py.

Why rows and columns.  The block tests assert one rel-L2 over the whole token matrix (< 1e-2).  One row of R that is completely wrong
contributes sqrt(1 / R) of its own relative error to that number (1.5e-2 at R = 4173, 0.8e-2 when the row is 50 % wrong): a grouped launch
that hands one row the neighbouring problem's gate, or an epilogue that writes a ragged last tile twice, stays below the bound.  Here every
row and every column of the block's INCREMENT x_out - x_in is measured on its own against the fp64 block evaluated from the same input,
and the worst of them is held against the worst row / column of the reference's own bf16 evaluation (dit_ref under eager_bf16()).

The fp64 blocks read the diffusers-named state dict (the `w` of dit_ref and of MMDiTEngine.load_state_dict), take the block input as
[B, T + N, D] (text rows first), temb [B, D] and the oracle's rotary tables, and follow dit_ref line by line with every tensor in double:
no bf16 rounding anywhere, weights cast to double (dit_ref.lin casts them to fp32).  `gate_rows` [B, S] names, per row, the sample whose
GATE vectors the row takes (default: its own) -- the "other sample's gate" fault is that argument and nothing else.
"""
import torch
import torch.nn.functional as F

from oracle import dit_ref

OLD_BOUND = 1e-2          # the whole-matrix bound of the block tests (test_production_shape.TOL_BLOCK, test_hip_engine)
FAULT_BUDGET = 6e-3       # whole-matrix rel-L2 a planted fault is scaled to: sqrt(6e-3^2 + e^2) < 1e-2 for every e < 8e-3


# ------------------------------------------------------------------------------------------------ fp64 primitives
def lin64(w, name, x):
    """nn.Linear in fp64; with ``w[name + '.lora'] = (A [r, in], B [out, r], keep_scale)`` also the peft LoRA branch of dit_ref.lin:
    y = W x + b + B A (x . keep_scale)."""
    b = w.get(name + '.bias')
    y = F.linear(x, w[name + '.weight'].double(), None if b is None else b.double())
    if name + '.lora' in w:
        a_, b_, keep_scale = w[name + '.lora']
        ks = keep_scale.double() if torch.is_tensor(keep_scale) else keep_scale
        y = y + F.linear(F.linear(x * ks, a_.double()), b_.double())
    return y


def layer_norm64(x):
    c = x - x.mean(-1, keepdim=True)
    return c / torch.sqrt((c * c).mean(-1, keepdim=True) + dit_ref.LN_EPS)


def modulate64(x, scale, shift):
    return layer_norm64(x) * (1 + scale[:, None]) + shift[:, None]


def rms_norm64(x, weight):
    return x / torch.sqrt((x * x).mean(-1, keepdim=True) + 1e-6) * weight.double()


def gelu_tanh64(x):
    return F.gelu(x, approximate='tanh')


def apply_rope64(x, cos, sin):
    xe, xo = x[..., 0::2], x[..., 1::2]
    c, s = cos.double()[None, :, None, :], sin.double()[None, :, None, :]
    return torch.stack([xe * c - xo * s, xe * s + xo * c], dim=-1).flatten(-2)


def attention64(q, k, v):
    """q, k, v [B, S, H, 128] -> [B, S, H * 128]: softmax(q k^T / sqrt(d)) v, head group by head group (<= 1 GB of fp64 scores at a time)."""
    qt, kt, vt = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
    o = torch.empty_like(qt)
    hs = max(1, (1 << 27) // (q.shape[0] * q.shape[1] * k.shape[1]))
    for h0 in range(0, qt.shape[1], hs):
        p = torch.softmax(torch.matmul(qt[:, h0:h0 + hs], kt[:, h0:h0 + hs].transpose(-1, -2)) * (q.shape[-1] ** -0.5), dim=-1)
        o[:, h0:h0 + hs] = torch.matmul(p, vt[:, h0:h0 + hs])
    return o.transpose(1, 2).flatten(2)


def _heads(x, h):
    return x.unflatten(-1, (h, -1))


def _gate(gate, rows):
    """gate [B, D] -> per-row [B, R, D]: row (b, r) takes the vector of sample rows[b, r] (None: its own)."""
    return gate[:, None] if rows is None else gate[rows]


def _qkv64(w, p, names, norms, x, h):
    q = rms_norm64(_heads(lin64(w, p + names[0], x), h), w[p + norms[0]])
    k = rms_norm64(_heads(lin64(w, p + names[1], x), h), w[p + norms[1]])
    return q, k, _heads(lin64(w, p + names[2], x), h)


_IMG_QKV, _TXT_QKV = ('attn.to_q', 'attn.to_k', 'attn.to_v'), ('attn.add_q_proj', 'attn.add_k_proj', 'attn.add_v_proj')
_IMG_NORM, _TXT_NORM = ('attn.norm_q.weight', 'attn.norm_k.weight'), ('attn.norm_added_q.weight', 'attn.norm_added_k.weight')


# ------------------------------------------------------------------------------------------------ the three blocks
def flux_double_block64(w, p, heads, x, temb, T, cos, sin, gate_rows=None):
    """dit_ref.flux_double_block on the joint layout: x [B, T + N, D] -> [B, T + N, D]."""
    x, temb = x.double(), temb.double()
    txt, img = x[:, :T], x[:, T:]
    gr_t, gr_i = (None, None) if gate_rows is None else (gate_rows[:, :T], gate_rows[:, T:])
    e = F.silu(temb)
    i_sh1, i_sc1, i_g1, i_sh2, i_sc2, i_g2 = lin64(w, p + 'norm1.linear', e).chunk(6, dim=1)
    t_sh1, t_sc1, t_g1, t_sh2, t_sc2, t_g2 = lin64(w, p + 'norm1_context.linear', e).chunk(6, dim=1)
    q, k, v = _qkv64(w, p, _IMG_QKV, _IMG_NORM, modulate64(img, i_sc1, i_sh1), heads)
    qt, kt, vt = _qkv64(w, p, _TXT_QKV, _TXT_NORM, modulate64(txt, t_sc1, t_sh1), heads)
    q = apply_rope64(torch.cat([qt, q], dim=1), cos, sin)
    k = apply_rope64(torch.cat([kt, k], dim=1), cos, sin)
    o = attention64(q, k, torch.cat([vt, v], dim=1))
    img = img + _gate(i_g1, gr_i) * lin64(w, p + 'attn.to_out.0', o[:, T:])
    txt = txt + _gate(t_g1, gr_t) * lin64(w, p + 'attn.to_add_out', o[:, :T])
    img = img + _gate(i_g2, gr_i) * lin64(w, p + 'ff.net.2', gelu_tanh64(lin64(w, p + 'ff.net.0.proj', modulate64(img, i_sc2, i_sh2))))
    txt = txt + _gate(t_g2, gr_t) * lin64(w, p + 'ff_context.net.2',
                                          gelu_tanh64(lin64(w, p + 'ff_context.net.0.proj', modulate64(txt, t_sc2, t_sh2))))
    return torch.cat([txt, img], dim=1)


def flux_single_block64(w, p, heads, x, temb, cos, sin, gate_rows=None):
    """dit_ref.flux_single_block: x [B, S, D] -> [B, S, D]."""
    x, temb = x.double(), temb.double()
    sh, sc, g = lin64(w, p + 'norm.linear', F.silu(temb)).chunk(3, dim=1)
    xn = modulate64(x, sc, sh)
    mlp = gelu_tanh64(lin64(w, p + 'proj_mlp', xn))
    q, k, v = _qkv64(w, p, _IMG_QKV, _IMG_NORM, xn, heads)
    o = attention64(apply_rope64(q, cos, sin), apply_rope64(k, cos, sin), v)
    return x + _gate(g, gate_rows) * lin64(w, p + 'proj_out', torch.cat([o, mlp], dim=2))


def qwen_block64(w, p, heads, x, temb, T, rope_img, rope_txt, gate_rows=None):
    """dit_ref.qwen_block on the joint layout: x [B, T + N, D] -> [B, T + N, D]."""
    x, temb = x.double(), temb.double()
    txt, img = x[:, :T], x[:, T:]
    gr_t, gr_i = (None, None) if gate_rows is None else (gate_rows[:, :T], gate_rows[:, T:])
    e = F.silu(temb)
    im1, im2 = lin64(w, p + 'img_mod.1', e).chunk(2, dim=-1)
    tm1, tm2 = lin64(w, p + 'txt_mod.1', e).chunk(2, dim=-1)

    def mod3(x_, mod):
        sh, sc, g = mod.chunk(3, dim=-1)
        return modulate64(x_, sc, sh), g
    xi, gi1 = mod3(img, im1)
    xt, gt1 = mod3(txt, tm1)
    q, k, v = _qkv64(w, p, _IMG_QKV, _IMG_NORM, xi, heads)
    qt, kt, vt = _qkv64(w, p, _TXT_QKV, _TXT_NORM, xt, heads)
    q, k = apply_rope64(q, *rope_img), apply_rope64(k, *rope_img)
    qt, kt = apply_rope64(qt, *rope_txt), apply_rope64(kt, *rope_txt)
    o = attention64(torch.cat([qt, q], 1), torch.cat([kt, k], 1), torch.cat([vt, v], 1))
    img = img + _gate(gi1, gr_i) * lin64(w, p + 'attn.to_out.0', o[:, T:])
    txt = txt + _gate(gt1, gr_t) * lin64(w, p + 'attn.to_add_out', o[:, :T])
    xi, gi2 = mod3(img, im2)
    img = img + _gate(gi2, gr_i) * lin64(w, p + 'img_mlp.net.2', gelu_tanh64(lin64(w, p + 'img_mlp.net.0.proj', xi)))
    xt, gt2 = mod3(txt, tm2)
    txt = txt + _gate(gt2, gr_t) * lin64(w, p + 'txt_mlp.net.2', gelu_tanh64(lin64(w, p + 'txt_mlp.net.0.proj', xt)))
    return torch.cat([txt, img], dim=1)


# ------------------------------------------------------------------------------------------------ one interface over both evaluations
KINDS = ('flux_double', 'flux_single', 'qwen')


def rope_tables(kind, hp, wp, T, device='cpu'):
    """The oracle's tables as dit_ref.flux_forward / qwen_forward build them: FLUX (cos, sin) [S, 64] rounded to bf16; Qwen
    ((cos, sin) of the image rows, (cos, sin) of the text rows) in fp32."""
    if kind == 'qwen':
        ia, ta = (t.to(device) for t in dit_ref.qwen_rope_angles(hp, wp, T))
        return (torch.cos(ia), torch.sin(ia)), (torch.cos(ta), torch.sin(ta))
    return tuple(t.to(device) for t in dit_ref.flux_rope_tables(hp, wp, T))


def block64(kind, w, p, heads, x, temb, T, tables, gate_rows=None):
    """The fp64 block `kind` with prefix p (e.g. 'transformer_blocks.1.') on x [B, T + N, D]."""
    if kind == 'flux_double':
        return flux_double_block64(w, p, heads, x, temb, T, *tables, gate_rows=gate_rows)
    if kind == 'flux_single':
        return flux_single_block64(w, p, heads, x, temb, *tables, gate_rows=gate_rows)
    return qwen_block64(w, p, heads, x, temb, T, *tables, gate_rows=gate_rows)


def oracle_block(kind, w, p, heads, x, temb, T, tables):
    """dit_ref's own block on the joint layout, in the mode in force (fp32, or every op output rounded to bf16 under eager_bf16())."""
    x, temb = x.float(), temb.float()
    if kind == 'flux_single':
        return dit_ref.flux_single_block(w, p, dit_ref.FluxCfg(heads=heads), x, temb, *tables)
    if kind == 'flux_double':
        txt, img = dit_ref.flux_double_block(w, p, dit_ref.FluxCfg(heads=heads), x[:, T:], x[:, :T], temb, *tables)
    else:
        txt, img = dit_ref.qwen_block(w, p, dit_ref.QwenCfg(heads=heads), x[:, T:], x[:, :T], temb, *tables)
    return torch.cat([txt, img], dim=1)


# ------------------------------------------------------------------------------------------------ the statistic and the assertion
STREAMS = ('text', 'image')


def whole_rel_l2(out, ref):
    """The block tests' statistic: one rel-L2 over the whole token matrix."""
    out, ref = out.double(), ref.double()
    return ((out - ref).norm() / ref.norm()).item()


def block_row_col_errors(x_in, x_out, y_ref, T):
    """Relative L2 error of the block's increment, [B, S, D] tensors: 'rows' [B, S], ||(x_out - y_ref)[r]|| / ||(y_ref - x_in)[r]||, and
    'cols' [B, 2, D], the same per column over the text rows (index 0) and over the image rows (index 1) of each sample -- the two
    streams' increments differ in size, so they are never pooled."""
    x_in, x_out, y_ref = x_in.double(), x_out.double(), y_ref.double()
    err, inc = x_out - y_ref, y_ref - x_in
    rows = err.norm(dim=2) / inc.norm(dim=2)
    cols = torch.stack([err[:, a:b].norm(dim=1) / inc[:, a:b].norm(dim=1) for a, b in ((0, T), (T, x_in.shape[1]))], dim=1)
    return {'rows': rows, 'cols': cols, 'T': T}


def _groups(e):
    """((sample, stream name, rows [n], first row, cols [D]), ...) of one block_row_col_errors result."""
    T, S = e['T'], e['rows'].shape[1]
    for b in range(e['rows'].shape[0]):
        for s, (a, z) in enumerate(((0, T), (T, S))):
            yield b, STREAMS[s], e['rows'][b, a:z], a, e['cols'][b, s]


_AXIS = {'rows': 'row', 'cols': 'column'}


def assert_rows_cols(hip, eager, bar, what=''):
    """In every (sample, stream) group: the largest row error of `hip` is at most bar x the largest row error of `eager`, and the same
    for columns.  Maxima only: a row's error is a sum over D terms of rounding noise, so row against row would be needlessly flaky.
    Returns {(sample, stream, 'rows' | 'cols'): hip max / eager max}; a failure names the worst row (joint row of its sample) or column,
    its value and the group's eager maximum."""
    ratios, bad = {}, []
    for (b, stream, hr, r0, hc), (_, _, er, _, ec) in zip(_groups(hip), _groups(eager)):
        for axis, h, e, off in (('rows', hr, er, r0), ('cols', hc, ec, 0)):
            hmax, emax = h.max().item(), e.max().item()
            ratios[(b, stream, axis)] = hmax / emax
            if not hmax <= bar * emax:           # (also fails on a NaN)
                i = int(torch.nan_to_num(h, nan=float('inf')).argmax())
                bad.append(f'sample {b} {stream} {_AXIS[axis]} {i + off}: increment error {h[i].item():.3e} > {bar} x {emax:.3e}, the largest '
                           f'of the eager-bf16 evaluation over the {h.numel()} {stream} {axis} of this sample')
    if bad:
        raise AssertionError(f'{what}: ' + '; '.join(bad))
    return ratios


def format_ratios(ratios):
    return ' '.join(f'b{b}/{s[:3]}/{a}={v:.2f}' for (b, s, a), v in sorted(ratios.items()))


# ------------------------------------------------------------------------------------------------ planted faults
FAULTS = ('row_stream_boundary', 'row_sample_boundary', 'row_other_gate', 'col_neighbour', 'head_band')


def plant_fault(name, x_in, x_out, y_ref, T, y_ref_other_gate=None, budget=FAULT_BUDGET):
    """A copy of x_out [B, S, D] (fp64) with one wiring fault, and where the check has to find it.

      row_stream_boundary  the last text row of sample 0 takes the increment of the first image row (row T - 1 <- row T);
      row_sample_boundary  the last row of sample 0 takes the increment of the first row of sample 1 (the next row of the flat matrix);
      row_other_gate       the first row of sample 1 is computed with sample 0's gate: y_ref_other_gate - y_ref on that row,
                           y_ref_other_gate = block64(..., gate_rows=other_gate_rows(B, S));
      col_neighbour        the column c whose increment is the smallest over all rows -- where a norm over the whole matrix sees least --
                           takes, in every row, the increment of column c + 1 (c - 1 when c is the last);
      head_band            the first 128-column band of sample 0's first image row takes the increment of the next band.

    The fault is the difference d between the faulty and the right increment, scaled by alpha = min(1, budget ||y_ref|| / ||d||): its
    whole-matrix rel-L2 is at most `budget`, so the whole-matrix bound OLD_BOUND cannot see it on top of any output within 8e-3.
    Returns (faulty x_out, (axis, sample, stream, index) as assert_rows_cols names it, alpha)."""
    x_in, x_out, y_ref = x_in.double(), x_out.double(), y_ref.double()
    B, S, D = x_out.shape
    inc = x_out - x_in
    d = torch.zeros_like(x_out)
    if name == 'row_stream_boundary':
        d[0, T - 1] = inc[0, T] - inc[0, T - 1]
        where = ('row', 0, 'text', T - 1)
    elif name == 'row_sample_boundary':
        d[0, S - 1] = inc[1, 0] - inc[0, S - 1]
        where = ('row', 0, 'image', S - 1)
    elif name == 'row_other_gate':
        d[1, 0] = (y_ref_other_gate.double() - y_ref)[1, 0]
        where = ('row', 1, 'text', 0)
    elif name == 'col_neighbour':
        c = int((y_ref - x_in).flatten(0, 1).norm(dim=0).argmin())
        d[:, :, c] = inc[:, :, c + 1 if c + 1 < D else c - 1] - inc[:, :, c]
        where = ('column', None, None, c)
    elif name == 'head_band':
        d[0, T, :128] = inc[0, T, 128:256] - inc[0, T, :128]
        where = ('row', 0, 'image', T)
    else:
        raise ValueError(name)
    alpha = min(1.0, budget * y_ref.norm().item() / d.norm().item())
    return x_out + alpha * d, where, alpha


def other_gate_rows(B, S, device='cpu'):
    """gate_rows of the row_other_gate fault: every row its own sample's gate, but the first row of sample 1 takes sample 0's."""
    rows = torch.arange(B, device=device)[:, None].expand(B, S).clone()
    rows[1, 0] = 0
    return rows


def fault_message(where):
    """The regular expression the failure message of assert_rows_cols must match for a fault planted at `where`."""
    axis, b, stream, i = where
    return rf'sample \d+ \w+ column {i}:' if b is None else rf'sample {b} {stream} row {i}:'


def scale_row(x_in, x_out, b, r, eps):
    """x_out with the increment of row (b, r) scaled by 1 + eps."""
    out = x_out.double().clone()
    out[b, r] = x_in.double()[b, r] + (1 + eps) * (out[b, r] - x_in.double()[b, r])
    return out


def smallest_detected_scaling(x_in, x_out, y_ref, eager, T, b, r, bar):
    """The smallest eps = 2^-k, k = 1 .. 12, down to which EVERY single-row scaling (1 + eps) of row (b, r)'s increment fails the check
    (None: not even 2^-1 does)."""
    found = None
    for k in range(1, 13):
        eps = 2.0 ** -k
        try:
            assert_rows_cols(block_row_col_errors(x_in, scale_row(x_in, x_out, b, r, eps), y_ref, T), eager, bar)
        except AssertionError:
            found = eps
            continue
        break
    return found
