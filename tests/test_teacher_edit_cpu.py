"""Teacher image editing without a GPU: the truncation of the schedule by ``strength``, the fp64 reference of the fused step against the
composition that defines it, the strength of the mutants of tests/teacher_edit_ref.py, the argument guards of ``afx_teacher_edit_step`` /
``afx_teacher_sde_edit_step`` (refused before any launch, as tests/test_cabi_cpu.py calls the library without a device) and the argument
errors of ``sample_teacher`` on pipelines without an engine."""
import ctypes as C

import numpy as np
import pytest
import torch

import teacher_edit_ref as TE

SHAPES = [(1, 1), (3, 3), (1, 64), (3, 257)]
VARIANTS = [(False, False), (True, False), (True, True)]          # (neg, coef)


# ------------------------------------------------------------------------------------------------ truncation by strength
@pytest.mark.parametrize('n,strength,t_start', [(4, 1.0, 0), (4, 0.5, 2), (4, 0.3, 2), (28, 0.6, 11), (50, 0.02, 49)])
def test_truncation_table(n, strength, t_start):
    from arcflow_amd.schedule import FlowEulerODEScheduler, truncate_by_strength
    assert t_start == int(max(n - min(n * strength, n), 0))                       # the rule as the issue states it, on the table's own rows
    for kw, seq_len in ((dict(shift=3.2), None), (dict(use_dynamic_shifting=True), 1024), (dict(use_dynamic_shifting=True, terminal_sigma=0.02), 4096)):
        sch = FlowEulerODEScheduler(1000, **kw)
        sch.set_timesteps(n, seq_len=seq_len)
        full = sch.sigmas.clone()
        got, sub = truncate_by_strength(full, strength)
        assert got == t_start and sub.numel() == n - t_start + 1
        assert sub[0] == full[t_start] and torch.equal(sub, full[t_start:]) and sub[-1] == 0      # a suffix of the FULL schedule, shifted for all n
        assert torch.equal(sch.sigmas, full)                                      # pure: the scheduler's table is left alone
    if strength == 1.0:
        assert torch.equal(sub, full)


def test_truncation_refuses_bad_strengths():
    from arcflow_amd.schedule import truncate_by_strength
    sig = torch.linspace(1, 0, 5)
    for bad in (0, 0.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match='strength'):
            truncate_by_strength(sig, bad)
    with pytest.raises(ValueError, match='none of the 4 steps'):                  # n - n strength rounds to n: zero steps would run
        truncate_by_strength(sig, 1e-20)
    assert truncate_by_strength(sig, 1e-3)[0] == 3                                # ... while any strength that leaves a step runs the last one


# ------------------------------------------------------------------------------------------------ the reference and its mutants
@pytest.mark.parametrize('sde', [False, True], ids=['euler', 'sde'])
@pytest.mark.parametrize('use_neg,use_coef', VARIANTS, ids=['nocfg', 'cfg', 'ortho'])
@pytest.mark.parametrize('B,n_tok', SHAPES)
def test_fused_reference_is_the_composition(B, n_tok, use_neg, use_coef, sde):
    c = TE.make_case(B, n_tok)
    for kind in TE.MASKS + (None,):
        mask = None if kind is None else c['mask_' + kind]
        for use_noise0 in (True, False):
            ref = TE.fused_ref(c, sde, use_neg, use_coef, mask, use_noise0)
            comp = TE.composed_ref(c, sde, use_neg, use_coef, mask, use_noise0)
            scale = TE.bound(c, sde, use_neg, use_coef, use_noise0) / TE.EPS      # the magnitudes the bound is made of
            assert torch.isfinite(ref).all() and ((ref - comp).abs() <= 2.0 ** -48 * scale).all(), (kind, use_noise0)
    # the consequences the semantics promise, in exact arithmetic: m = 1 is the plain step, m = 0 is known
    plain = TE.fused_ref(c, sde, use_neg, use_coef, None)
    assert torch.equal(TE.fused_ref(c, sde, use_neg, use_coef, c['mask_ones']), plain)
    s_to = c['sigma_to'].double()[:, None, None]
    known = (1 - s_to) * c['x0'].double() + s_to * c['noise0'].double()
    assert torch.equal(TE.fused_ref(c, sde, use_neg, use_coef, c['mask_zeros']), known)


@pytest.mark.parametrize('sde', [False, True], ids=['euler', 'sde'])
@pytest.mark.parametrize('use_neg,use_coef', VARIANTS, ids=['nocfg', 'cfg', 'ortho'])
@pytest.mark.parametrize('B,n_tok', SHAPES)
def test_every_mutant_moves_the_reference_beyond_the_bound(B, n_tok, use_neg, use_coef, sde):
    """On the random mask (the only one on which all of them can show) every mutant moves the reference by more than twice the bound on at
    least 1 % of the elements: the condition under which the GPU test's rejection means something."""
    c = TE.make_case(B, n_tok)
    mask = c['mask_random']
    for use_noise0 in (True, False):
        ref, bnd = TE.fused_ref(c, sde, use_neg, use_coef, mask, use_noise0), TE.bound(c, sde, use_neg, use_coef, use_noise0)
        assert (bnd > 0).all()
        muts = TE.mutants(sde, use_noise0)
        assert ('sde_draw_as_noise0' in muts) == (sde and use_noise0) and len(muts) >= 3
        for mut in muts:
            frac = ((TE.fused_ref(c, sde, use_neg, use_coef, mask, use_noise0, mutate=mut) - ref).abs() > 2 * bnd).double().mean().item()
            print(f'B={B} n_tok={n_tok} sde={sde} neg={use_neg} coef={use_coef} noise0={use_noise0} mutant {mut}: moves {100 * frac:.1f} % by > 2 x bound')
            assert frac >= 0.01, (mut, frac)


def test_bf16_rne_helper_is_torchs_rounding():
    v = torch.cat([TE.make_case(3, 3)['x'].flatten(), torch.from_numpy(__import__('edit_ref').tie_values())])
    assert torch.equal(TE.bf16_rne(v), v.bfloat16().view(torch.int16))


# ------------------------------------------------------------------------------------------------ the C ABI's guards
def _aligned(nbytes, fill):
    """A host buffer of ``nbytes`` at a 16-byte aligned address, filled with ``fill``: stands in for an output that must stay untouched."""
    raw = np.full(nbytes + 16, fill, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw, raw[off:off + nbytes]


@pytest.mark.parametrize('sde', [False, True], ids=['euler', 'sde'])
def test_edit_step_argument_guards_no_gpu(sde):
    """AFX_E_INVALID before any launch: no pointer is dereferenced, so plain integers stand in for device memory; the two outputs are real
    host buffers so that 'untouched' can be seen."""
    from arcflow_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    name = b'afx_teacher_sde_edit_step' if sde else b'afx_teacher_edit_step'
    f = getattr(lib, name.decode())
    B, N = 2, 15
    nbytes = B * N * 64 * 4
    raw_o, out = _aligned(nbytes, 0xA5)
    raw_h, out16 = _aligned(nbytes // 2, 0x5A)
    MB = 1 << 20
    ptr = {k: C.c_void_p(MB * (i + 1)) for i, k in enumerate(('x', 'pos', 'neg', 'noise', 'sigma', 'sigma_to', 'm', 'c_noise', 'coef', 'x0', 'noise0', 'mask'))}
    ptr.update(x_out=C.c_void_p(out.ctypes.data), x_out_bf16=C.c_void_p(out16.ctypes.data))
    order = ('x', 'pos', 'neg') + (('noise',) if sde else ()) + ('sigma', 'sigma_to') + (('m', 'c_noise') if sde else ()) + \
        ('coef', 'scale', 'x0', 'noise0', 'mask', 'x_out', 'x_out_bf16', 'batch', 'n_tok', 'ch', 'max_blocks', 'stream')
    good = dict(ptr, scale=4.0, batch=B, n_tok=N, ch=64, max_blocks=0, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return f(*[a[k] for k in order])

    def refused(what, **kw):
        assert call(**kw) == _lib.AFX_E_INVALID, kw
        err = lib.afx_last_error()
        assert name in err and what in err, (kw, err)
    required = ('x', 'pos', 'sigma', 'sigma_to', 'x0', 'x_out', 'x_out_bf16') + (('m', 'c_noise') if sde else ())
    for k in required:
        refused(b'null argument', **{k: None})
    refused(b'64', ch=32)
    for kw in (dict(n_tok=0), dict(batch=0), dict(max_blocks=-1)):
        refused(b'bad argument', **kw)
    for k in ('x', 'pos', 'neg', 'x0', 'noise0', 'mask', 'x_out', 'x_out_bf16') + (('noise',) if sde else ()):
        refused(b'aligned', **{k: C.c_void_p(good[k].value + 4)})
    # an output over an operand: partial overlaps from either side and exact aliasing; only x_out == x is allowed
    for k in ('x', 'x0', 'noise0', 'pos', 'neg', 'mask', 'coef') + (('noise',) if sde else ()):
        base = good[k].value
        refused(b'x_out overlaps', x_out=C.c_void_p(base + 64 if k not in ('coef',) else base))
        refused(b'x_out overlaps', x_out=C.c_void_p(base - nbytes + 16))
        if k != 'x':
            refused(b'x_out overlaps', x_out=C.c_void_p(base))
        refused(b'x_out_bf16 overlaps', x_out_bf16=C.c_void_p(base))
        refused(b'x_out_bf16 overlaps', x_out_bf16=C.c_void_p(base - nbytes // 2 + 16))
    refused(b'x_out overlaps', x_out_bf16=C.c_void_p(out.ctypes.data + 128))
    refused(b'x_out overlaps', x_out=ptr['x'], x_out_bf16=C.c_void_p(ptr['x'].value + nbytes - 16))
    # with mask = NULL the same guards answer under the same name (the call would go on to the plain step entry)
    refused(b'null argument', mask=None, x0=None)
    refused(b'64', mask=None, ch=32)
    assert (out == 0xA5).all() and (out16 == 0x5A).all() and (raw_o == 0xA5).all() and (raw_h == 0x5A).all()        # nothing was written


def test_ops_wrappers_refuse_cpu_tensors():
    from arcflow_amd import _lib, ops
    x, pos, one = torch.zeros(1, 4, 64), torch.zeros(1, 4, 64, dtype=torch.bfloat16), torch.ones(1)
    with pytest.raises(_lib.ArcflowHipError):
        ops.teacher_edit_step(x, pos, None, one, one, x, None, torch.ones(1, 4, 4))
    with pytest.raises(_lib.ArcflowHipError):
        ops.teacher_sde_edit_step(x, pos, None, None, one, one, one, one, x, None, torch.ones(1, 4, 4))


# ------------------------------------------------------------------------------------------------ sample_teacher's edit arguments
@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_sample_teacher_refuses_bad_edit_arguments_before_anything_runs(family):
    from arcflow_amd.pipelines import ArcFluxPipeline, ArcQwenImagePipeline
    pipe = ArcFluxPipeline() if family == 'flux' else ArcQwenImagePipeline()          # no engine, no VAE: the guards come first
    pe = torch.zeros(1, 4, 128)
    kw = dict(prompt_embeds=pe, pooled_prompt_embeds=torch.zeros(1, 64)) if family == 'flux' else dict(prompt_embeds=pe)
    img, lat, mask = torch.rand(1, 3, 32, 48), torch.zeros(1, 6, 64), torch.ones(1, 1, 32, 48)
    with pytest.raises(ValueError, match='mask_image'):
        pipe.sample_teacher(mask_image=mask, **kw)                                    # mask without an image
    with pytest.raises(ValueError, match='both'):
        pipe.sample_teacher(image=img, image_latents=lat, **kw)
    with pytest.raises(ValueError, match='resizes nothing'):
        pipe.sample_teacher(image=img, height=64, width=48, **kw)
    with pytest.raises(ValueError, match='image_latents'):
        pipe.sample_teacher(image_latents=lat, height=32, width=32, **kw)             # 6 tokens are not 32 x 32
    for bad in (0.0, 1.5, -0.1):
        with pytest.raises(ValueError, match='strength'):
            pipe.sample_teacher(image=img, strength=bad, **kw)
    with pytest.raises(TypeError):
        pipe.sample_teacher(None, None, None, None, 28, 3.5, 1.0, None, None, pe, None, None, None, 'pil', True, None, False, 1, 512, 'FlowEulerODE',
                            None, img)                                                # the edit keywords are keyword-only
