"""The fp64 references of tests/forward_frame_ref.py without a kernel: (1) against oracle/dit_ref.py -- the embedders, norm_out and the three
heads of the reference forward -- at a toy width; (2) on the very inputs of test_hip_forward_frame_fp64.py: the reference rounded to bf16
passes the shared assertion with every share at 1.0, the bound exceeds the reference's magnitude on fewer than 1 % of the elements (the two
stated exceptions below), and every mutated reference of the teeth checks fails that same assertion."""
import pytest
import torch
import torch.nn.functional as F

import forward_frame_ref as R
from bf16_parity import proj64
from oracle import dit_ref

ATOL = 2e-5        # the oracle runs in fp32: sums of <= 128 terms of magnitude ~1 (128 u ~ 8e-6)


def _rne(ref):
    return ref.float().bfloat16()


def _fails(out, ref, bound, **kw):
    with pytest.raises(AssertionError, match='beyond'):
        R.frame_check(out, ref, bound, 'mutated', **kw)


# ------------------------------------------------------------------------------------------------ (1) against the oracle, toy width
@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_embed64_matches_the_oracle(family):
    g = torch.Generator().manual_seed(3)
    B, T, N, C, J, Dm = 2, 5, 4, 64, 128, 256
    rnd = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).bfloat16()     # noqa: E731
    x, ctx = rnd(B, N, C), rnd(B, T, J)
    xi, ci = ('x_embedder', 'context_embedder') if family == 'flux' else ('img_in', 'txt_in')
    w = {xi + '.weight': rnd(Dm, C, sc=C ** -0.5), xi + '.bias': rnd(Dm, sc=0.1), ci + '.weight': rnd(Dm, J, sc=J ** -0.5),
         ci + '.bias': rnd(Dm, sc=0.1)}
    wn = None
    img = dit_ref.lin(w, xi, x.float())
    if family == 'flux':
        txt = dit_ref.lin(w, ci, ctx.float())
    else:
        wn = w['txt_norm.weight'] = 1 + 0.3 * torch.randn(J, generator=g)
        normed = dit_ref.rms_norm(ctx.float(), wn)
        txt = dit_ref.lin(w, ci, normed)
        txt_rounded = dit_ref.lin(w, ci, normed.bfloat16().float())
    args = (x, ctx, (w[xi + '.weight'], w[xi + '.bias']), (w[ci + '.weight'], w[ci + '.bias']), wn)
    ref, bound, is_txt = R.embed64(*args, round_normed=False)
    want = torch.cat([txt, img], 1).reshape(B * (T + N), Dm).double()
    assert (ref - want).abs().max().item() <= ATOL
    assert is_txt.tolist() == ([True] * T + [False] * N) * B
    if family == 'qwen':
        # the bf16-rounded operand: the fp32 oracle's row may round to the neighbour of RNE(fp64 row) -- exactly what the bound allows
        ref_r, bound_r, _ = R.embed64(*args)
        want_r = torch.cat([txt_rounded, img], 1).reshape(B * (T + N), Dm).double()
        assert bool(((ref_r - want_r).abs() <= bound_r + ATOL).all())
        assert (ref_r - want_r)[~is_txt].abs().max().item() <= ATOL
        assert (ref_r - ref)[is_txt].abs().max().item() > 1e-4          # the rounding is there


def test_norm_out64_and_head_split64_match_the_oracle():
    g = torch.Generator().manual_seed(4)
    B, N, Dm = 2, 6, 128
    K, ch, lw = R.K_G, R.CH, R.LW
    rnd = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc     # noqa: E731
    w = {}
    for name, o in (('norm_out.linear', 2 * Dm), ('proj_out_means', K * ch), ('proj_out_logweights', K * lw), ('proj_out_loggamma', (K - 1) * lw)):
        w[name + '.weight'], w[name + '.bias'] = rnd(o, Dm, sc=Dm ** -0.5), rnd(o, sc=0.3)
    temb, x = rnd(B, Dm), rnd(B, N, Dm, sc=1.5) + 0.3
    means, logw, logg = dit_ref.arc_heads(w, temb, x, K, ch, lw)
    mod_final = dit_ref.lin(w, 'norm_out.linear', F.silu(temb))                     # (scale | shift): the oracle chunks scale first
    hin, _ = R.norm_out64(x.reshape(B * N, Dm), mod_final, N)
    sc, sh = mod_final.chunk(2, dim=1)
    assert (hin - dit_ref.modulate(x, sc, sh).reshape(B * N, Dm).double()).abs().max().item() <= ATOL
    names = ('proj_out_means', 'proj_out_logweights', 'proj_out_loggamma')
    head, _ = proj64(hin, torch.cat([w[n + '.weight'] for n in names]), torch.cat([w[n + '.bias'] for n in names]))
    m64, w64, g64, _ = R.head_split64(head, round_first=False)
    for got, want in ((m64, means), (w64, logw), (g64, logg)):
        assert (got - want.reshape(B * N, -1).double()).abs().max().item() <= ATOL
    # the kernel's reading: the logits rounded to bf16 first
    assert torch.equal(R.head_split64(head)[1], R.head_split64(head.float().bfloat16().double(), round_first=False)[1])


# ------------------------------------------------------------------------------------------------ (2) the kernel test's own inputs
@pytest.mark.parametrize('rows,rpb,Dm', R.NORM_CASES)
def test_norm_cases_reference_conditions_and_teeth(rows, rpb, Dm):
    x, mod, w = R.norm_inputs(rows, rpb, Dm)
    ref, bound = R.norm_case64(x, mod, rpb)
    assert R.frame_check(_rne(ref), ref, bound, 'LN') <= 0.5
    assert R.vacuous_share(ref, bound) < 0.01
    # the constant row: bound 0, the output is the shift
    assert float(bound[R.CONST_ROW].max()) == 0.0 and bool((bound[R.CONST_ROW + 1] > 0).all())
    assert torch.equal(ref[R.CONST_ROW], mod[0, R.SH_COL * Dm:(R.SH_COL + 1) * Dm].double())
    if mod.shape[0] > 1:                 # (one sample: the shifted index is the true one)
        _fails(_rne(ref), *R.norm_case64(x, mod, rpb, shifted=True))
    if rows < 1023:
        ref, bound = R.rms64(x, w)
        assert R.frame_check(_rne(ref), ref, bound, 'RMS') <= 0.5
        assert R.vacuous_share(ref, bound) < 0.01


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_embed_reference_conditions_and_teeth(family):
    inp = R.embed_inputs(family)
    args = (inp['x'], inp['ctx'], inp['x_in'], inp['ctx_in'], inp['txt_norm'])
    ref, bound, is_txt = R.embed64(*args)
    assert R.frame_check(_rne(ref), ref, bound, family, share=~is_txt if family == 'qwen' else None) <= 0.5
    # Qwen's text rows carry one bf16 ulp of every operand element through |W| (a worst case over 3584 terms): a sizeable share of their
    # elements lies below that bound, which is why they also take no part in the RNE share; every other row is held to < 1 %
    rows = ~is_txt if family == 'qwen' else torch.ones_like(is_txt)
    assert R.vacuous_share(ref[rows], bound[rows]) < 0.01
    _fails(_rne(ref), *R.embed64(*args, swapped=True)[:2], min_equal=None)


@pytest.mark.parametrize('N', sorted(R.HEAD_N_IMG))
def test_head_reference_conditions_and_teeth(N):
    B, T = R.HEAD_B, R.HEAD_T
    inp = R.head_inputs(N)
    ximg = R.image_rows(inp['tokens'], B, N, T)
    assert bool((inp['tokens'].view(B, T + N, -1)[:, :T] == R.TEXT_FILL).all())
    hin, hb = R.norm_out64(ximg, inp['mod_final'], N)
    assert R.frame_check(_rne(hin), hin, hb, 'head_in') <= 0.5
    assert R.vacuous_share(hin, hb) < 0.01
    # an image-row offset error of T rows reads the text fill: constant rows, whose LN output is the shift alone
    off = inp['tokens'].view(B, T + N, -1)[:, :N].reshape(B * N, -1)
    _fails(_rne(hin), *R.norm_out64(off, inp['mod_final'], N))
    head_in = _rne(hin)
    y, e = proj64(head_in, *inp['head'])
    means, logw, logg, wb = R.head_split64(y, e)
    for name, ref, bnd in (('means', means, e[:, :R.NM]), ('logg', logg, e[:, R.NM + R.NW:R.NM + R.NW + R.NG])):
        assert R.frame_check(_rne(ref), ref, bnd, name) <= 0.5
        assert R.vacuous_share(ref, bnd) < 0.01
    _fails(_rne(logg), R.head_split64(y, logg_shift=R.LW)[2], e[:, R.NM + R.NW + R.LW:R.NM + R.NW + R.LW + R.NG])
    assert R.frame_check(_rne(logw), logw, wb, 'logw', min_equal=None) <= 0.5
    assert R.vacuous_share(logw, wb) < 0.01
    # exact logits: every token's logits are the bias
    yx, _ = proj64(head_in, *inp['head_exact'])
    table = R.exact_logit_table().flatten()
    assert torch.equal(yx[:, R.NM:R.NM + R.NW], table.expand(B * N, R.NW))
    _, lx, _, xb = R.head_split64(yx)
    big = R.big_logit_mask(B * N)
    assert R.frame_check(_rne(lx), lx, xb, 'logw exact', share=~big) <= 0.5
    assert torch.equal(xb > lx.abs(), big)             # the dominant entry alone (1 of 64) lies below the fp32 resolution of lse
    _fails(_rne(lx), *R.head_split64(yx, over='p')[1::2], share=~big)


def test_teacher_head_reference_conditions():
    B, T, N = R.HEAD_B, R.HEAD_T, 256
    inp = R.head_inputs(N, teacher=True)
    hin, _ = R.norm_out64(R.image_rows(inp['tokens'], B, N, T), inp['mod_final'], N)
    v, e = proj64(_rne(hin), *inp['head'])
    assert v.shape == (B * N, R.CH)
    assert R.frame_check(_rne(v), v, e, 'velocity') <= 0.5
    assert R.vacuous_share(v, e) < 0.01
