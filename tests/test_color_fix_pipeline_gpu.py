"""``color_fix=`` of both pipelines on the tiny synthetic engines and VAEs of tests/test_edit_resize_gpu.py (its ``Setup``): the 40 x 56
photo, tile 32, overlap 8, strength 0.6, 2 NFE.  Every check is a bit-equality: with ``color_fix`` a call returns ``ops.color_fix`` of what
it returns without, matched to the call's own ``image``; ``None`` changes nothing; ``enhance`` is ``ops.tiles_merge`` of per-tile calls
with the same argument.  On the parent commit every test here fails: ``color_fix`` is an unknown keyword and ``ops.color_fix`` does not
exist."""
import numpy as np
import pytest
import torch

from test_edit_resize_gpu import HP, SIZE, WP, Setup

pytestmark = pytest.mark.gpu

NFE, RATIO, STRENGTH = 2, 1.0, 0.6
MODES = ['adain', 'wavelet']


@pytest.fixture(scope='module', params=['flux', 'qwen'])
def S(request):
    from arcflow_amd import ops
    s = Setup(request.param)
    g = torch.Generator().manual_seed(21)
    s.tile_noise = torch.randn(4, HP * WP, 64, generator=g)
    s.image = ops.image_resample(torch.from_numpy(s.photo)[None].cuda(), SIZE, SIZE)            # fp32 [1, 3, 32, 32] in [0, 1]
    s.plain = s.call('pt', image=s.image)                                                       # the call without the argument, shared
    return s


def _bits(t):
    return t.contiguous().view(torch.int32)


def _cond(S):
    if S.family == 'flux':
        return dict(prompt_embeds=S.pe, pooled_prompt_embeds=S.pooled)
    return dict(prompt_embeds=S.pe, prompt_embeds_mask=torch.ones(1, 12, dtype=torch.long))


@pytest.mark.parametrize('mode', MODES)
def test_call_is_color_fix_of_the_plain_call(S, mode):
    from arcflow_amd import ops
    got = S.call('pt', image=S.image, color_fix=mode)
    assert got.dtype == torch.float32 and got.shape == (1, 3, SIZE, SIZE)                      # fp32 whatever the decoder's dtype
    want = ops.color_fix(S.plain.cuda(), S.image, mode).cpu()
    assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want))
    assert not torch.equal(got, S.plain.float())                                               # ... and it did something
    # 'np' and 'pil' come from the same values
    arr = S.call('np', image=S.image, color_fix=mode)
    assert np.array_equal(arr, (got / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).numpy())
    pil = S.call('pil', image=S.image, color_fix=mode)
    assert np.array_equal(np.asarray(pil[0]), (arr[0] * 255).round().astype('uint8'))


def test_none_changes_nothing(S):
    got = S.call('pt', image=S.image, color_fix=None)
    assert got.dtype == S.plain.dtype and torch.equal(got.float(), S.plain.float())
    assert torch.equal(_bits(got.float()), _bits(S.plain.float()))


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_sample_teacher_is_color_fix_of_the_plain_call(family, tmp_path):
    """On the teacher pipelines of tests/test_teacher_edit_gpu.py (synthetic snapshots, a batch of 2 with one shared source)."""
    from arcflow_amd import ops
    from tests.test_teacher_edit_gpu import _pipeline
    pipe, kw = _pipeline(family, str(tmp_path / 'snap'))
    g = torch.Generator().manual_seed(4)
    photo = torch.randint(0, 256, (40, 56, 3), generator=g, dtype=torch.uint8).numpy()
    noise = torch.randn(2, HP * WP, 64, generator=g)
    image = ops.image_resample(torch.from_numpy(photo)[None].cuda(), SIZE, SIZE)
    kw.update(num_inference_steps=3, output_type='pt', strength=STRENGTH, image=image)
    plain = pipe.sample_teacher(latents=noise.clone(), **kw).images
    assert plain.shape == (2, 3, SIZE, SIZE)
    for mode in MODES:
        got = pipe.sample_teacher(latents=noise.clone(), color_fix=mode, **kw).images
        torch.cuda.synchronize()
        assert got.dtype == torch.float32 and torch.isfinite(got).all()
        assert torch.equal(_bits(got), _bits(ops.color_fix(plain.contiguous(), image, mode))) and not torch.equal(got, plain.float())


@pytest.mark.parametrize('mode', MODES)
def test_enhance_is_the_merge_of_per_tile_calls_with_color_fix(S, mode):
    """The by-hand merge of tests/test_enhance_gpu.py::_by_hand, every tile call with ``color_fix``."""
    from arcflow_amd import ops, schedule
    plan = schedule.tile_plan(40, 56, SIZE, 8)
    assert plan.T == 4
    kw = dict(num_inference_steps=NFE, timestep_ratio=RATIO, **_cond(S))
    got = S.pipe.enhance(S.photo, tile=SIZE, overlap=8, strength=STRENGTH, latents=S.tile_noise.clone(), tile_batch=2, output_type='pt',
                         color_fix=mode, **kw).images
    tiles = ops.tiles_cut(ops.image_resample(torch.from_numpy(S.photo)[None].cuda(), 40, 56), plan)
    outs = []
    for i in range(0, plan.T, 2):
        out = S.pipe(image=tiles[i:i + 2], strength=STRENGTH, latents=S.tile_noise[i:i + 2].clone(), num_images_per_prompt=2, output_type='pt',
                     color_fix=mode, **kw).images
        assert out.dtype == torch.float32 and out.shape == (2, 3, plan.th, plan.tw)
        outs.append(out)
    want = ops.tiles_merge(torch.cat(outs).contiguous(), plan)[None]
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and got.shape == (1, 40, 56, 3) and torch.equal(got, want)
    plain = S.pipe.enhance(S.photo, tile=SIZE, overlap=8, strength=STRENGTH, latents=S.tile_noise.clone(), tile_batch=2, output_type='pt', **kw).images
    assert not torch.equal(got, plain)
    none = S.pipe.enhance(S.photo, tile=SIZE, overlap=8, strength=STRENGTH, latents=S.tile_noise.clone(), tile_batch=2, output_type='pt',
                          color_fix=None, **kw).images
    assert torch.equal(none, plain)
