"""``afx_teacher_edit_step`` / ``afx_teacher_sde_edit_step`` (CFG combine + Euler / FlowSDE step + the inpainting blend at the sigma the step
lands on + bf16 copy, one launch) against fp64, element by element, on the inputs of tests/teacher_edit_ref.py.

Bound (derived in tests/teacher_edit_ref.py, not fitted to the kernel): the plain step tests' bound on x' plus the blend's six fp32 roundings,

    |err| <= E_step + 8 * 2^-24 * (X + |x0| + |noise0|),
    E_step = (7 | 9) eps X_ode (Euler; the 9 with the orthogonal term)  or  (16 | 18) eps X_sde (FlowSDE),

X the step tests' bound on |x'| itself.  The bf16 output must be bit-equal to round-to-nearest-even of the kernel's own fp32 output.

Bit-exact.  The fused step is DEFINED as the plain step entry followed by ``afx_edit_blend`` on its result: both outputs of the fused launch
must equal that composition's bit for bit, for every case; ``mask = NULL`` must equal the plain step entry; a zero mask with
``sigma_to = 0`` must return ``x0``.

Cases: Euler and FlowSDE; no neg / neg / neg + orthogonal coef; noise0 given and NULL; B = 1 and 3; 1, 3, 64, 257 tokens; the grid capped at one
work-group (24 grid-stride passes at the largest shape) and the default; masks random in [0, 1], all 0, all 1 and a 0 / 1 checkerboard over the
four patch positions; NaN guard rows around every output.  On the random mask every mutant of tests/teacher_edit_ref.py (known at sigma instead
of sigma_to, m and 1 - m swapped, mask index e >> 4, the SDE draw used as noise0) must fail the same check on at least 1 % of the elements;
tests/test_teacher_edit_cpu.py shows that each moves the reference by more than twice the bound on those inputs.
"""
import pytest
import torch

import teacher_edit_ref as TE

pytestmark = pytest.mark.gpu

GUARD = 64            # NaN sentinel elements in front of and behind every output (keeps 16-byte alignment for fp32 and bf16)
SHAPES = [(B, n_tok) for B in (1, 3) for n_tok in (1, 3, 64, 257)]
VARIANTS = [(False, False), (True, False), (True, True)]          # (neg, coef)


def _guarded(shape, dtype):
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((numel + 2 * GUARD,), float('nan'), dtype=dtype, device='cuda')
    return buf, buf[GUARD:GUARD + numel].view(shape)


def _guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _device(c):
    return {k: v.cuda() for k, v in c.items()}


def _plain(ops, d, sde, neg, coef, z, sig_to=None):
    """The existing step entry -> (x', its bf16 copy)."""
    sig_to = d['sigma_to'] if sig_to is None else sig_to
    if sde:
        return ops.teacher_sde_step(d['x'], d['pos'], neg, z, d['sigma'], sig_to, d['m'], d['c_noise'], TE.SCALE, coef)
    return ops.teacher_euler_step(d['x'], d['pos'], neg, d['sigma'], sig_to, TE.SCALE, coef)


def _fused(ops, d, sde, neg, coef, z, noise0, mask, sig_to=None, **kw):
    sig_to = d['sigma_to'] if sig_to is None else sig_to
    if sde:
        return ops.teacher_sde_edit_step(d['x'], d['pos'], neg, z, d['sigma'], sig_to, d['m'], d['c_noise'], d['x0'], noise0, mask, TE.SCALE, coef, **kw)
    return ops.teacher_edit_step(d['x'], d['pos'], neg, d['sigma'], sig_to, d['x0'], noise0, mask, TE.SCALE, coef, **kw)


@pytest.mark.parametrize('sde', [False, True], ids=['euler', 'sde'])
@pytest.mark.parametrize('use_neg,use_coef', VARIANTS, ids=['nocfg', 'cfg', 'ortho'])
@pytest.mark.parametrize('B,n_tok', SHAPES)
def test_edit_step_against_fp64_and_the_two_launch_composition(B, n_tok, use_neg, use_coef, sde):
    from arcflow_amd import ops
    c = TE.make_case(B, n_tok)
    d = _device(c)
    shape = (B, n_tok, 64)
    neg, coef, z = d['neg'] if use_neg else None, d['coef'] if use_coef else None, d['z'] if sde else None
    xp, xp16 = _plain(ops, d, sde, neg, coef, z)
    worst = 0.0
    for kind in TE.MASKS:
        mask = d['mask_' + kind]
        for use_noise0 in (True, False):
            noise0 = d['noise0'] if use_noise0 else None
            ref = TE.fused_ref(c, sde, use_neg, use_coef, c['mask_' + kind], use_noise0)
            bnd = TE.bound(c, sde, use_neg, use_coef, use_noise0)
            comp, comp16 = ops.edit_blend(xp, d['x0'], noise0, mask, d['sigma_to'])                 # the second launch of the composition
            runs = {}
            for tag, max_blocks, inplace in (('default', 0, False), ('one_block', 1, False), ('inplace', 0, True)):
                fbuf, fout = _guarded(shape, torch.float32)
                hbuf, hout = _guarded(shape, torch.bfloat16)
                dd = d
                if inplace:
                    fout.copy_(d['x'])
                    dd = dict(d, x=fout)
                o, o16 = _fused(ops, dd, sde, neg, coef, z, noise0, mask, out=fout, out_bf16=hout, max_blocks=max_blocks)
                torch.cuda.synchronize()
                assert o.data_ptr() == fout.data_ptr() and o16.data_ptr() == hout.data_ptr()
                assert _guards_intact(fbuf) and _guards_intact(hbuf), (kind, use_noise0, tag)
                runs[tag] = (fout.clone(), hout.clone())
            got, got16 = runs['default']
            for tag, (f, h16) in runs.items():                     # one work-group, in place: the same bits; and the definition by composition
                assert torch.equal(_bits(f), _bits(got)) and torch.equal(_bits(h16), _bits(got16)), (kind, use_noise0, tag)
            assert torch.equal(_bits(got), _bits(comp)) and torch.equal(_bits(got16), _bits(comp16)), (kind, use_noise0)
            got, got16 = got.cpu(), got16.cpu()
            err = (got.double() - ref).abs()
            ratio = (err / bnd).max().item()
            worst = max(worst, ratio)
            print(f'B={B} n_tok={n_tok} sde={sde} neg={use_neg} coef={use_coef} mask={kind} noise0={use_noise0}: max err / bound {ratio:.3f}')
            assert torch.isfinite(got).all()
            assert (err <= bnd).all(), (kind, use_noise0, ratio)
            assert torch.equal(_bits(got16), TE.bf16_rne(got)) and torch.equal(_bits(got16), _bits(got.bfloat16()))      # bf16 copy = RNE of the fp32 output
            if kind == 'ones':                                     # m = 1: today's step, bitwise
                assert torch.equal(_bits(got), _bits(xp.cpu())) and torch.equal(_bits(got16), _bits(xp16.cpu()))
            if kind == 'zeros':                                    # m = 0: known, bitwise -- the blend with no mask at all
                known, known16 = ops.edit_blend(None, d['x0'], noise0, None, d['sigma_to'])
                assert torch.equal(_bits(got), _bits(known.cpu())) and torch.equal(_bits(got16), _bits(known16.cpu()))
            if kind == 'random':
                for mut in TE.mutants(sde, use_noise0):
                    r = TE.fused_ref(c, sde, use_neg, use_coef, c['mask_random'], use_noise0, mutate=mut)
                    assert ((r - ref).abs() > 2 * bnd).double().mean().item() >= 0.01, mut       # the CPU-side condition again, on the spot
                    frac = ((got.double() - r).abs() > bnd).double().mean().item()
                    assert frac >= 0.01, (mut, use_noise0, frac)
    for k in ('x', 'x0', 'noise0', 'z', 'mask_random'):            # the out-of-place runs left their operands alone
        assert torch.equal(d[k].cpu(), c[k]), k
    print(f'B={B} n_tok={n_tok} sde={sde} neg={use_neg} coef={use_coef}: worst max err / bound {worst:.3f}')


@pytest.mark.parametrize('sde', [False, True], ids=['euler', 'sde'])
@pytest.mark.parametrize('use_neg,use_coef', VARIANTS, ids=['nocfg', 'cfg', 'ortho'])
@pytest.mark.parametrize('B,n_tok', SHAPES)
def test_null_mask_is_the_plain_step_and_the_last_step_returns_x0(B, n_tok, use_neg, use_coef, sde):
    from arcflow_amd import ops
    c = TE.make_case(B, n_tok)
    d = _device(c)
    neg, coef, z = d['neg'] if use_neg else None, d['coef'] if use_coef else None, d['z'] if sde else None
    xp, xp16 = _plain(ops, d, sde, neg, coef, z)
    for noise0 in (d['noise0'], None):
        for max_blocks in (0, 1):
            o, o16 = _fused(ops, d, sde, neg, coef, z, noise0, None, max_blocks=max_blocks)
            assert torch.equal(_bits(o), _bits(xp)) and torch.equal(_bits(o16), _bits(xp16))
    # the last step of a sampler: sigma_to = 0, no start noise.  Kept elements are x0 bit for bit, repainted ones the plain step's
    zero = torch.zeros(B, device='cuda')
    last, last16 = _plain(ops, d, sde, neg, coef, None, sig_to=zero)
    o, o16 = _fused(ops, d, sde, neg, coef, None, None, d['mask_zeros'], sig_to=zero)
    assert torch.equal(_bits(o), _bits(d['x0'])) and torch.equal(_bits(o16), _bits(d['x0'].bfloat16()))
    o, o16 = _fused(ops, d, sde, neg, coef, None, None, d['mask_checker'], sig_to=zero)
    keep = (d['mask_checker'] == 0)[:, :, torch.arange(64, device='cuda') & 3]
    assert torch.equal(_bits(o[keep]), _bits(d['x0'][keep])) and torch.equal(_bits(o[~keep]), _bits(last[~keep]))
    assert torch.equal(_bits(o16), _bits(o.bfloat16())) and torch.equal(_bits(o16[~keep]), _bits(last16[~keep]))


def test_wrappers_allocate_and_refuse_wrong_operands():
    from arcflow_amd import _lib, ops
    c = TE.make_case(3, 3)
    d = _device(c)
    o, o16 = ops.teacher_edit_step(d['x'], d['pos'], d['neg'], d['sigma'], d['sigma_to'], d['x0'], d['noise0'], d['mask_random'], TE.SCALE)
    ref, bnd = TE.fused_ref(c, False, True, False, c['mask_random']), TE.bound(c, False, True, False)
    assert ((o.cpu().double() - ref).abs() <= bnd).all() and o16.dtype == torch.bfloat16 and o16.shape == o.shape
    with pytest.raises(ValueError):         # the mask is [B, N, 4], one value per latent pixel of the patch
        ops.teacher_edit_step(d['x'], d['pos'], None, d['sigma'], d['sigma_to'], d['x0'], None, d['mask_random'][:, :, :1].contiguous())
    with pytest.raises(ValueError):         # a bf16 source is not this kernel's operand
        ops.teacher_edit_step(d['x'], d['pos'], None, d['sigma'], d['sigma_to'], d['x0'].bfloat16(), None, d['mask_random'])
    with pytest.raises(ValueError):         # per-sample coefficients: [B]
        ops.teacher_sde_edit_step(d['x'], d['pos'], None, d['z'], d['sigma'], d['sigma_to'], d['m'][:2], d['c_noise'], d['x0'], None, d['mask_random'])
    with pytest.raises(_lib.ArcflowHipError):         # x_out over x0
        ops.teacher_edit_step(d['x'], d['pos'], None, d['sigma'], d['sigma_to'], d['x0'], None, d['mask_random'], out=d['x0'])
    with pytest.raises(_lib.ArcflowHipError):         # 32 channels per token
        x = torch.zeros(1, 4, 32, device='cuda')
        ops.teacher_edit_step(x, x.bfloat16(), None, torch.ones(1, device='cuda'), torch.ones(1, device='cuda'), x.clone(), None,
                              torch.ones(1, 4, 4, device='cuda'))
