"""Image editing without a GPU: the edit time grid, the mask reduction, the argument guards of ``afx_edit_blend`` (refused before any
launch), the input normalisation and its errors on a pipeline without an engine, and the strength of the mutants of tests/edit_ref.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import edit_ref as ER


# ------------------------------------------------------------------------------------------------ schedule
@pytest.mark.parametrize('nfe,ratio', [(1, 1.0), (2, 1.0), (2, 0.5), (4, 0.5)])
def test_edit_raw_timesteps(nfe, ratio):
    from arcflow_amd.schedule import edit_raw_timesteps, retrieve_raw_timesteps
    times, per_step, total = retrieve_raw_timesteps(nfe, 128, ratio)
    assert edit_raw_timesteps(nfe, 128, ratio, 1.0) == (times, per_step, total)
    t6, p6, n6 = edit_raw_timesteps(nfe, 128, ratio, 0.6)
    assert t6 == [0.6 * t for t in times] and p6 == per_step and n6 == total
    for bad in (0, 1.5, -0.1):
        with pytest.raises(ValueError):
            edit_raw_timesteps(nfe, 128, ratio, bad)


@pytest.mark.parametrize('reduce', ['max', 'mean'])
def test_mask_to_tokens_matches_the_loops(reduce):
    from arcflow_amd.schedule import mask_to_tokens
    hp, wp, B = 3, 5, 2
    g = torch.Generator().manual_seed(1)
    mask = torch.rand(B, 16 * hp, 16 * wp, generator=g)
    mask[0, :24] = (mask[0, :24] > 0.97).float()                # a sparse binary part: single repainted pixels
    ref = ER.mask_to_tokens_loop(mask.numpy(), hp, wp, reduce)
    for m in (mask, mask[:, None]):
        got = mask_to_tokens(m, hp, wp, reduce)
        assert got.shape == (B, hp * wp, 4) and got.dtype == torch.float32 and got.is_contiguous()
        err = np.abs(got.double().numpy() - ref).max()
        assert err == 0.0 if reduce == 'max' else err <= 64 * 2.0 ** -24, err
    assert torch.equal(mask_to_tokens(mask, hp, wp), mask_to_tokens(mask, hp, wp, 'max'))            # the default
    binary = (mask > 0.5).float()
    assert set(mask_to_tokens(binary, hp, wp).unique().tolist()) <= {0.0, 1.0}
    with pytest.raises(ValueError):
        mask_to_tokens(mask, hp, wp + 1)
    with pytest.raises(ValueError):
        mask_to_tokens(mask, hp, wp, 'min')


# ------------------------------------------------------------------------------------------------ the C ABI's guards
def test_edit_blend_argument_guards_no_gpu():
    """AFX_E_INVALID before any launch: the pointers are never dereferenced, so plain integers stand in for device memory."""
    from arcflow_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    f = lib.afx_edit_blend
    MB = 1 << 20
    x, x0, nz, mk, sg, out, o16 = [C.c_void_p(MB * k) for k in range(1, 8)]
    good = [x, x0, nz, mk, sg, out, o16, 2, 15, 64, 0, None]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[dict(x=0, x0=1, noise=2, mask=3, sigma_to=4, x_out=5, x_out_bf16=6, batch=7, n_tok=8, ch=9, max_blocks=10)[k]] = v
        return f(*a)
    assert call(x0=None) == _lib.AFX_E_INVALID and b'afx_edit_blend' in lib.afx_last_error()
    assert call(x_out=None) == _lib.AFX_E_INVALID and call(sigma_to=None) == _lib.AFX_E_INVALID
    assert call(x=None) == _lib.AFX_E_INVALID                                  # x is required with a mask
    assert call(ch=32) == _lib.AFX_E_INVALID and b'64' in lib.afx_last_error()
    assert call(n_tok=0) == _lib.AFX_E_INVALID and call(batch=0) == _lib.AFX_E_INVALID and call(max_blocks=-1) == _lib.AFX_E_INVALID
    for name in ('x', 'x0', 'noise', 'mask', 'sigma_to', 'x_out', 'x_out_bf16'):
        base = good[dict(x=0, x0=1, noise=2, mask=3, sigma_to=4, x_out=5, x_out_bf16=6)[name]].value
        assert call(**{name: C.c_void_p(base + 4)}) == _lib.AFX_E_INVALID, name
        assert b'aligned' in lib.afx_last_error()
    # partial overlap of x_out with x, x0, noise and the bf16 copy; exact aliasing of x0 is refused too (only x_out == x is allowed)
    nbytes = 2 * 15 * 64 * 4
    for name in ('x', 'x0', 'noise'):
        base = good[dict(x=0, x0=1, noise=2)[name]].value
        assert call(x_out=C.c_void_p(base + 64)) == _lib.AFX_E_INVALID, name
        assert call(x_out=C.c_void_p(base - nbytes + 16)) == _lib.AFX_E_INVALID, name
        assert b'overlaps' in lib.afx_last_error()
    assert call(x_out=x0) == _lib.AFX_E_INVALID
    assert call(x_out_bf16=C.c_void_p(out.value + 128)) == _lib.AFX_E_INVALID
    assert call(x_out_bf16=C.c_void_p(x0.value + nbytes - 16)) == _lib.AFX_E_INVALID


def test_ops_edit_blend_refuses_cpu_tensors_and_wrong_layouts():
    from arcflow_amd import _lib, ops
    x0 = torch.zeros(1, 4, 64)
    with pytest.raises(_lib.ArcflowHipError):
        ops.edit_blend(None, x0, None, None, torch.zeros(1))


# ------------------------------------------------------------------------------------------------ the mutants are visible
def test_every_mutant_moves_the_reference_beyond_the_bound():
    c = ER.make_case()
    bound = ER.blend_bound(c['x'], c['x0'], c['noise'])
    ref = ER.blend_ref(c['x'], c['x0'], c['noise'], c['mask'], c['sigma_to'])
    ref_nn = ER.blend_ref(c['x'], c['x0'], c['noise'], c['mask'], c['sigma_to'], noise_is_null=True)
    assert np.abs(ref - ref_nn).max() > 0
    for m in ER.MUTANTS:
        null = m == 'keep_noise'
        base = ref_nn if null else ref
        moved = np.abs(ER.blend_ref(c['x'], c['x0'], c['noise'], c['mask'], c['sigma_to'], mutate=m, noise_is_null=null) - base) > 2 * bound
        assert moved.mean() >= 0.01, (m, moved.mean())
    # the truncated bf16 copy differs from the rounded one on about half of random values, and on the constructed ties that round up
    vals = np.concatenate([ref.astype(np.float32).ravel(), ER.tie_values()])
    rne, cut = ER.bf16_bits(vals), ER.bf16_bits(vals, trunc=True)
    assert 0.3 < (rne != cut).mean() < 0.7
    assert (rne[-8:] != cut[-8:]).tolist() == [False, True, False, True, True, False, True, False]
    assert np.array_equal(rne, torch.from_numpy(vals).bfloat16().view(torch.int16).numpy().view(np.uint16))      # RNE as torch rounds


# ------------------------------------------------------------------------------------------------ the pipelines' edit arguments
def _pipe(family='flux'):
    from arcflow_amd.pipelines import ArcFluxPipeline, ArcQwenImagePipeline
    return ArcFluxPipeline() if family == 'flux' else ArcQwenImagePipeline()         # no engine, no VAE: the guards come first


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_call_refuses_bad_edit_arguments_before_anything_runs(family):
    pipe = _pipe(family)
    pe = torch.zeros(1, 4, 128)
    kw = dict(prompt_embeds=pe, pooled_prompt_embeds=torch.zeros(1, 64)) if family == 'flux' else dict(prompt_embeds=pe)
    img, lat, mask = torch.rand(1, 3, 32, 48), torch.zeros(1, 6, 64), torch.ones(1, 1, 32, 48)
    with pytest.raises(ValueError, match='mask_image'):
        pipe(mask_image=mask, **kw)                                              # mask without an image
    with pytest.raises(ValueError, match='both'):
        pipe(image=img, image_latents=lat, **kw)
    with pytest.raises(ValueError, match='16'):
        pipe(image=torch.rand(1, 3, 40, 48), **kw)                               # not a multiple of 16
    with pytest.raises(ValueError, match='resizes nothing'):
        pipe(image=img, height=64, width=48, **kw)                               # size mismatch
    with pytest.raises(ValueError, match='resizes nothing'):
        pipe(image=img, mask_image=torch.ones(1, 1, 32, 32), **kw)
    with pytest.raises(ValueError, match='image_latents'):
        pipe(image_latents=lat, height=32, width=32, **kw)                       # 6 tokens are not 32 x 32
    for bad in (0.0, 1.5, -0.1):
        with pytest.raises(ValueError, match='strength'):
            pipe(image=img, strength=bad, **kw)


def test_edit_inputs_normalise_every_accepted_form():
    from PIL import Image
    pipe = _pipe()
    g = torch.Generator().manual_seed(0)
    u8 = (torch.rand(2, 32, 48, 3, generator=g) * 255).round().to(torch.uint8)
    want = u8.float().permute(0, 3, 1, 2) / 255
    pils = [Image.fromarray(a.numpy()) for a in u8]
    forms = {'torch4': want, 'torch3': want[0], 'numpy4': want.permute(0, 2, 3, 1).numpy(), 'numpy3': want[0].permute(1, 2, 0).numpy(),
             'pil': pils[0], 'pils': pils}
    for name, image in forms.items():
        edit, h, w = pipe._edit_inputs(image, None, None, 0.5, None, None)
        n = 2 if name in ('torch4', 'numpy4', 'pils') else 1
        assert (h, w) == (32, 48) and edit.image.dtype == torch.float32 and torch.equal(edit.image, want[:n]), name
        assert edit.strength == 0.5 and edit.mask is None
    m8 = (torch.rand(32, 48, generator=g) > 0.5).to(torch.uint8) * 255
    mwant = (m8.float() / 255)[None, None]
    for name, mask in {'torch2': mwant[0, 0], 'torch3': mwant[0], 'torch4': mwant, 'numpy2': mwant[0, 0].numpy(), 'numpy3': mwant[0].numpy(),
                       'pil': Image.fromarray(m8.numpy())}.items():
        edit, h, w = pipe._edit_inputs(want, None, mask, 1.0, None, None)
        assert torch.equal(edit.mask, mwant), name
    # the text-to-image path is untouched: no edit, the sizes as given
    assert pipe._edit_inputs(None, None, None, 1.0, None, 512) == (None, None, 512)
    # with latents only, the mask gives the size
    edit, h, w = pipe._edit_inputs(None, torch.zeros(1, 6, 64), mwant, 1.0, None, None)
    assert (h, w) == (32, 48) and edit.image is None


def test_edit_prepare_batch_mismatch_and_missing_encoder():
    pipe = _pipe()
    img = torch.rand(3, 3, 32, 48)
    edit, h, w = pipe._edit_inputs(img, None, None, 1.0, None, None)
    with pytest.raises(ValueError, match='batch 3'):
        pipe._edit_prepare(edit, 2, 2, 3)
    edit, h, w = pipe._edit_inputs(img[:1], None, torch.ones(3, 32, 48), 1.0, None, None)
    with pytest.raises(ValueError, match='mask_image'):
        pipe._edit_prepare(edit, 2, 2, 3)
    edit, h, w = pipe._edit_inputs(None, torch.zeros(3, 6, 64), None, 1.0, 32, 48)
    with pytest.raises(ValueError, match='image_latents'):
        pipe._edit_prepare(edit, 2, 2, 3)
    edit, h, w = pipe._edit_inputs(img, None, None, 1.0, None, None)
    with pytest.raises(RuntimeError, match='image_latents='):                    # no pipe.vae at all
        pipe._edit_prepare(edit, 3, 2, 3)
    pipe.vae = object()                                                           # a decoder without an encoder
    with pytest.raises(RuntimeError, match='image_latents='):
        pipe._edit_prepare(edit, 3, 2, 3)
