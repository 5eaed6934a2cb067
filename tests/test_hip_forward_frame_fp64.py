"""fp64 parity, per element, of the frame around the MMDiT blocks at the released widths (D = 3072, H = 24, joint_dim 4096 / 3584, K = 16
gaussians, head_n = 1152): the plain AdaLN / RMS rows (afx_norm_modulate_bf16), the embedders through stage 1, and norm_out, the head GEMM
and head_split_kernel through afx_mmdit_import_tokens and stage 2, with the exports the distillation step builds on.

References, bounds (each derived in tests/forward_frame_ref.py from the operation: chain depth x 2^-24 x magnitude, plus one bf16 ulp),
inputs and the assertion itself (frame_check) live in forward_frame_ref.py; test_forward_frame_ref_cpu.py validates them against the oracle
and shows on these inputs that the fp64 reference meets every share and that each mutated reference below fails.  Every teeth check here
runs the kernel's output through the SAME frame_check against the mutated reference and must see it fail.

Engines: one double (and, FLUX, one single) block -- the smallest at which norm_out's modulation rows do not start at column 0 of the stacked
tensor -- with every block weight behind one shared zero buffer and the q / k norm weights behind one buffer of ones; the conditioning
weights, embedders and head are random.  Each check prints its worst err / tol.
"""
import pytest
import torch

import forward_frame_ref as R
from bf16_parity import proj64

pytestmark = pytest.mark.gpu

D = R.D
SENT = -7.75                         # guard-band sentinel (bf16-exact)
DEV = 'cuda'


@pytest.fixture(scope='module')
def ops():
    from arcflow_amd import ops as _ops
    return _ops


def _check(out, ref, bound, what, **kw):
    worst = R.frame_check(out, ref, bound, what, **kw)
    print(f'{what}: worst err / tol {worst:.3f}')
    return worst


def _fails(out, ref, bound, **kw):
    with pytest.raises(AssertionError, match='beyond'):
        R.frame_check(out, ref, bound, 'mutated reference', **kw)


def _unchanged(buf, inner, what):
    mask = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    mask[inner] = False
    assert bool((buf[mask] == SENT).all()), f'{what}: a write landed in the guard band'


# ------------------------------------------------------------------------------------------------ plain AdaLN and RMS rows
@pytest.mark.parametrize('rows,rpb,Dm', R.NORM_CASES)
def test_plain_adaln_and_rms_rows_vs_fp64(ops, rows, rpb, Dm):
    """ops.norm_modulate as the single blocks and norm_out call it: x a column view of a wider buffer, the output a view of a wider buffer
    filled with a sentinel (guard bands untouched), scale / shift column slices of one stacked [B, 5 D] fp32 tensor (ldmod = 5 D).
      D = 3072, rows >= 1024 -> norm_modulate_rows_kernel<6, 2, 0>: (2050, 1025) a sample boundary inside a wave's pair of rows,
        (2049, 683) an odd tail (the last wave holds one row), (1024, 1024) the smallest launch that kernel takes;
      (1023, 341) one row below the switch: norm_modulate_kernel, three samples;
      37 rows, two samples, norm_modulate_kernel in LN and in RMS mode (weight vector, shift None): D = 4096 all 8 chunks of every lane,
        3584 (Qwen's txt_norm) 448 chunks, the last round of lanes half empty, 264 = 33 chunks: lanes 0..32 one chunk, the others none.
    Row 5 holds an outlier of 40.0, row 9 one constant value: its variance is 0, the output must be the shift (bound 0 on that row: the
    cancellation is exact, forward_frame_ref docstring).  Bound elsewhere: one bf16 ulp + 2^-24 D row_scale; >= 99 % equal to RNE(ref).
    Teeth: the reference with sample index (row + 1) // rows_per_batch fails the same check (not at B = 1, where it is the true one)."""
    x, mod, w = R.norm_inputs(rows, rpb, Dm, DEV)
    sc, sh = mod[:, R.SC_COL * Dm:(R.SC_COL + 1) * Dm], mod[:, R.SH_COL * Dm:(R.SH_COL + 1) * Dm]
    assert sc.stride(0) == R.N_MOD * Dm and x.stride(0) == Dm + 64
    inner = (slice(1, 1 + rows), slice(24, 24 + Dm))
    what = f'plain AdaLN rows={rows} rpb={rpb} D={Dm}'
    obuf = torch.full((rows + 2, Dm + 64), SENT, dtype=torch.bfloat16, device=DEV)
    ops.norm_modulate(x, sc, sh, rows_per_batch=rpb, out=obuf[inner])
    _unchanged(obuf, inner, what)
    ref, bound = R.norm_case64(x, mod, rpb)
    _check(obuf[inner], ref, bound, what)
    if mod.shape[0] > 1:
        _fails(obuf[inner], *R.norm_case64(x, mod, rpb, shifted=True))
    if rows < 1023:
        obuf.fill_(SENT)
        ops.norm_modulate(x, w, None, rms=True, out=obuf[inner])
        _unchanged(obuf, inner, what + ' rms')
        _check(obuf[inner], *R.rms64(x, w), what + ' rms')


# ------------------------------------------------------------------------------------------------ engines
def _engine(family, teacher=False, seed=0):
    """(engine, packed): random conditioning weights (scale in^-0.5, bias 0.1), zero block weights, q / k norm weights of ones; the embedders
    and the head are zero until a test binds its own."""
    from arcflow_amd import MMDiTEngine
    flux = family == 'flux'
    nd, ns, J = 1, (1 if flux else 0), (4096 if flux else 3584)
    eng = MMDiTEngine(family, nd, ns, joint_dim=J, teacher_head=teacher)
    g = torch.Generator(device=DEV).manual_seed(77 + seed)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, generator=g, device=DEV) * sc).bfloat16()     # noqa: E731
    cond = {'temb.t.l1': (D, 256), 'temb.t.l2': (D, D), 'mod': (eng.n_mod, D)}
    if flux:
        cond.update({'temb.g.l1': (D, 256), 'temb.g.l2': (D, D), 'temb.p.l1': (D, 768), 'temb.p.l2': (D, D)})
    packed = {}
    for n, (o, i) in cond.items():
        packed[n + '.weight'], packed[n + '.bias'] = rnd(o, i, sc=i ** -0.5), rnd(o, sc=0.1)
    trunk = {'x_in': (D, 64), 'ctx_in': (D, J), 'head': (eng.head_n, D)}
    for i in range(nd):
        for s in ('img', 'txt'):
            trunk.update({f'd{i}.{s}_qkv': (3 * D, D), f'd{i}.{s}_out': (D, D), f'd{i}.{s}_mlp1': (4 * D, D), f'd{i}.{s}_mlp2': (D, 4 * D)})
    for i in range(ns):
        trunk.update({f's{i}.fused': (7 * D, D), f's{i}.out': (D, 5 * D)})
    zero = torch.zeros(7 * D * D, dtype=torch.bfloat16, device=DEV)
    for n, (o, i) in trunk.items():
        packed[n + '.weight'], packed[n + '.bias'] = zero[:o * i].view(o, i), zero[:o]
    ones = torch.ones(4 * 128, device=DEV)
    for i in range(nd):
        packed[f'd{i}.qknorm'] = ones.view(4, 128)
    for i in range(ns):
        packed[f's{i}.qknorm'] = ones[:256].view(2, 128)
    if not flux:
        packed['txt_norm.weight'] = torch.ones(J, device=DEV)
    eng.bind_packed(packed)
    return eng, packed


def _cond_args(family, B):
    """timestep, pooled, guidance of a staged call: the two samples differ"""
    t = torch.tensor([0.7619, 0.05], device=DEV)[:B]
    if family != 'flux':
        return t, None, None
    g = torch.Generator(device=DEV).manual_seed(5)
    return t, torch.randn(B, 768, generator=g, device=DEV).bfloat16(), torch.tensor([3.5, 1.25], device=DEV)[:B]


# ------------------------------------------------------------------------------------------------ embedders through stage 1
@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_embedders_stage1_vs_fp64(family):
    """stage 1, then export('x_tokens'): all B (T + N) rows of the joint token matrix -- x_in (K = 64) on the image rows, ctx_in (K = 4096 /
    3584; Qwen: behind RMSNorm with a random weight, the normed row stored as bf16) on the text rows, rows [text T | image N] per sample.
    FLUX B = 2, T = 77, N = 16; Qwen B = 2, T = 20, N = 16.  Bound: one bf16 ulp + proj64's summation bound; on Qwen's text rows also one
    bf16 ulp (+ the RMS bound) of every operand element through |W| -- the stored normed operand may sit one ulp from RNE of the exact one, so
    those rows take no part in the 99 % RNE share.  Teeth: the reference with each sample's text and image blocks swapped fails."""
    B, T, N, J = R.EMBED_SHAPES[family]
    inp = R.embed_inputs(family, DEV)
    eng, _ = _engine(family)
    bind = {'x_in.weight': inp['x_in'][0], 'x_in.bias': inp['x_in'][1], 'ctx_in.weight': inp['ctx_in'][0], 'ctx_in.bias': inp['ctx_in'][1]}
    if family == 'qwen':
        bind['txt_norm.weight'] = inp['txt_norm']
    eng.bind_packed(bind)
    t, pooled, gd = _cond_args(family, B)
    eng(inp['x'], t, inp['ctx'], pooled, gd, 4, 4, stage=1)
    xt = torch.full((B * (T + N) + 1, D), SENT, dtype=torch.bfloat16, device=DEV)
    eng.export('x_tokens', xt, B, N, T)
    torch.cuda.synchronize()
    assert bool((xt[-1] == SENT).all()), 'export wrote past B (T + N) rows'
    xt = xt[:-1]
    args = (inp['x'], inp['ctx'], inp['x_in'], inp['ctx_in'], inp['txt_norm'])
    ref, bound, is_txt = R.embed64(*args)
    _check(xt, ref, bound, f'{family} x_tokens', share=~is_txt if family == 'qwen' else None)
    if family == 'qwen':
        _check(xt[is_txt], ref[is_txt], bound[is_txt], 'qwen x_tokens text rows (bound only)', min_equal=None)
    _fails(xt, *R.embed64(*args, swapped=True)[:2], min_equal=None)


# ------------------------------------------------------------------------------------------------ norm_out, head, head split through stage 2
def _staged_head(eng, inp, N, teacher=False):
    """stage 1 (real conditioning: mod_final populated, different per sample), import the token matrix, stage 2.  Returns the outputs and
    the exports."""
    B, T = R.HEAD_B, R.HEAD_T
    hp, wp = R.HEAD_N_IMG[N]
    g = torch.Generator(device=DEV).manual_seed(N)
    x = torch.randn(B, N, 64, generator=g, device=DEV).bfloat16()
    ctx = torch.randn(B, T, 4096, generator=g, device=DEV).bfloat16()
    t, pooled, gd = _cond_args('flux', B)
    call = (x, t, ctx, pooled, gd, hp, wp)
    eng(*call, stage=1)
    eng.import_tokens(inp['tokens'], B, N, T)
    out = eng(*call, stage=2)
    ex = {'x_final': torch.empty(B * N, D, dtype=torch.bfloat16, device=DEV), 'head_in': torch.empty(B * N, D, dtype=torch.bfloat16, device=DEV),
          'mod_final': torch.empty(B, 2 * D, device=DEV), 'mod_all': torch.empty(B, eng.n_mod, device=DEV)}
    for name, dst in ex.items():
        eng.export(name, dst, B, N, T)
    torch.cuda.synchronize()
    return out, ex


@pytest.mark.parametrize('N', sorted(R.HEAD_N_IMG))
def test_norm_out_head_and_split_stage2_vs_fp64(N):
    """FLUX, B = 2, T = 77; N = 1025 (25 x 41) sends each sample's norm_out launch through the rows kernel with an odd tail, N = 256 through
    the one-row kernel.  The imported token matrix is random (x 1.5 + 0.3) with every text row 300.0: a norm_out that starts T rows early
    reads constant rows.
      x_final / mod_final: bit for bit the image rows of the imported matrix / the last 2 D columns of mod_all.
      head_in: norm_out64 of the imported image rows with the EXPORTED (scale | shift): bound and share of the plain AdaLN test.
      means, logg: the head GEMM on the exported head_in (proj64, K = 3072), columns [0, 1024) and [1088, 1148).  Teeth: logg read lw = 4
        columns further on.
      logw, random head: log_softmax over k of the bf16-rounded fp64 logits at column 1024 + 4 k + p; bound 2 max_k (ulp_bf16 + GEMM bound)
        + the fp32 evaluation term E (forward_frame_ref docstring); no RNE share (the input perturbation is of the order of an output ulp).
      logw, exact logits: the head rebound with zero weight rows under the logits and a bias of 64 different bf16-exact values, one of them
        20 above the rest: every token's logits are exactly the bias; bound one bf16 ulp + E, >= 99 % equal to RNE(ref) -- over the 63 of
        64 entries whose value exceeds E: the dominant entry's output (~ -1e-8) lies below the fp32 resolution of lse = 23.875 and is held
        by E alone.  Teeth: the softmax over p at fixed k (the transposed layout) fails."""
    B, T = R.HEAD_B, R.HEAD_T
    inp = R.head_inputs(N, device=DEV)
    eng, _ = _engine('flux')
    eng.bind_packed({'head.weight': inp['head'][0], 'head.bias': inp['head'][1]})
    out, ex = _staged_head(eng, inp, N)
    ximg = R.image_rows(inp['tokens'], B, N, T)
    assert torch.equal(ex['x_final'], ximg), 'x_final is not the image rows of the imported token matrix'
    assert torch.equal(ex['mod_final'], ex['mod_all'][:, -2 * D:]), 'mod_final is not the fin slices of mod_all'
    assert not torch.equal(ex['mod_final'][0], ex['mod_final'][1])
    hin, hb = R.norm_out64(ximg, ex['mod_final'], N)
    _check(ex['head_in'], hin, hb, f'N={N} head_in')
    y, e = proj64(ex['head_in'], *inp['head'])
    means, logw, logg, wb = R.head_split64(y, e)
    lg = slice(R.NM + R.NW, R.NM + R.NW + R.NG)
    _check(out.means.view(B * N, R.NM), means, e[:, :R.NM], f'N={N} means')
    _check(out.loggammas.view(B * N, R.NG), logg, e[:, lg], f'N={N} logg')
    _fails(out.loggammas.view(B * N, R.NG), R.head_split64(y, logg_shift=R.LW)[2], e[:, lg.start + R.LW:lg.stop + R.LW])
    _check(out.logweights.view(B * N, R.NW), logw, wb, f'N={N} logw (random head)', min_equal=None)
    # the second binding: exact logits
    eng.bind_packed({'head.weight': inp['head_exact'][0], 'head.bias': inp['head_exact'][1]})
    out, ex2 = _staged_head(eng, inp, N)
    assert torch.equal(ex2['head_in'], ex['head_in'])
    lx, xb = R.head_split64(proj64(ex2['head_in'], *inp['head_exact'])[0])[1::2]
    big = R.big_logit_mask(B * N, DEV)
    _check(out.logweights.view(B * N, R.NW), lx, xb, f'N={N} logw (exact logits)', share=~big)
    _fails(out.logweights.view(B * N, R.NW), *R.head_split64(proj64(ex2['head_in'], *inp['head_exact'])[0], over='p')[1::2], share=~big)


def test_teacher_head_stage2_vs_fp64():
    """teacher_head=True, N = 256: the head GEMM (head_n = 64) writes the velocity [B N, 64] straight into the output; same GEMM bound."""
    B, T, N = R.HEAD_B, R.HEAD_T, 256
    inp = R.head_inputs(N, teacher=True, device=DEV)
    eng, _ = _engine('flux', teacher=True)
    assert eng.head_n == R.CH
    eng.bind_packed({'head.weight': inp['head'][0], 'head.bias': inp['head'][1]})
    v, ex = _staged_head(eng, inp, N, teacher=True)
    assert v.shape == (B, N, R.CH)
    hin, hb = R.norm_out64(R.image_rows(inp['tokens'], B, N, T), ex['mod_final'], N)
    _check(ex['head_in'], hin, hb, 'teacher head_in')
    _check(v.view(B * N, R.CH), *proj64(ex['head_in'], *inp['head']), 'teacher velocity')
