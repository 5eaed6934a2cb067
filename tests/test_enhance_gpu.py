"""``pipe.enhance`` of both pipelines on the tiny synthetic engines and VAEs of tests/test_edit_resize_gpu.py (its ``Setup``): the 40 x 56
photo, tile 32, overlap 8 (2 x 2 tiles of a 2 x 2 token grid), strength 0.6, 2 NFE, ``prompt_embeds`` given.  Every check is a
bit-equality: the tiled result is by construction ``ops.tiles_merge`` of ordinary image-to-image calls on the tiles of ``ops.tiles_cut``.
On the parent commit every test here fails: ``pipe.enhance``, ``ops.tiles_cut`` and ``ops.tiles_merge`` do not exist."""
import numpy as np
import pytest
import torch

from test_edit_resize_gpu import HP, SIZE, WP, Setup

pytestmark = pytest.mark.gpu

NFE, RATIO, STRENGTH = 2, 1.0, 0.6


@pytest.fixture(scope='module', params=['flux', 'qwen'])
def S(request):
    s = Setup(request.param)
    g = torch.Generator().manual_seed(11)
    s.tile_noise = torch.randn(12, HP * WP, 64, generator=g)                            # 2 x 2 tiles at scale 1, 3 x 4 at scale 1.5
    return s


def _cond(S):
    if S.family == 'flux':
        return dict(prompt_embeds=S.pe, pooled_prompt_embeds=S.pooled)
    return dict(prompt_embeds=S.pe, prompt_embeds_mask=torch.ones(1, 12, dtype=torch.long))


def _enhance(S, image=None, output_type='pt', **kw):
    kw.setdefault('tile', SIZE)
    kw.setdefault('overlap', 8)
    kw.setdefault('strength', STRENGTH)
    out = S.pipe.enhance(S.photo if image is None else image, num_inference_steps=NFE, timestep_ratio=RATIO, output_type=output_type,
                         **_cond(S), **kw).images
    torch.cuda.synchronize()
    return out


def _by_hand(S, canvas, plan, noise, batch):
    """ops.tiles_merge of ordinary calls on the tiles of ``canvas`` [1, 3, H, W], ``batch`` tiles per call."""
    from arcflow_amd import ops
    tiles = ops.tiles_cut(canvas, plan)
    outs = []
    for i in range(0, plan.T, batch):
        out = S.pipe(image=tiles[i:i + batch], strength=STRENGTH, latents=noise[i:i + batch].clone(), num_images_per_prompt=len(tiles[i:i + batch]),
                     num_inference_steps=NFE, timestep_ratio=RATIO, output_type='pt', **_cond(S)).images
        assert out.shape == (len(tiles[i:i + batch]), 3, plan.th, plan.tw)
        outs.append(out.float())
    return ops.tiles_merge(torch.cat(outs).contiguous(), plan)[None]


@pytest.fixture(scope='module')
def base(S):
    """The 'pt' result at scale 1 with one tile per call: computed once, shared, never modified."""
    return _enhance(S, latents=S.tile_noise[:4].clone(), tile_batch=1)


def test_result_is_the_merge_of_per_tile_calls(S, base):
    from arcflow_amd import ops, schedule
    assert base.dtype == torch.uint8 and base.shape == (1, 40, 56, 3) and base.is_cuda
    plan = schedule.tile_plan(40, 56, SIZE, 8)
    assert (plan.T, plan.th, plan.tw) == (4, SIZE, SIZE)
    canvas = ops.image_resample(torch.from_numpy(S.photo)[None].cuda(), 40, 56)        # the same size: the photo's values / 255
    assert torch.equal(base, _by_hand(S, canvas, plan, S.tile_noise[:4], 1))
    assert not torch.equal(base.cpu(), torch.from_numpy(S.photo)[None])                # ... and it is an edit, not the photo
    assert torch.equal(_enhance(S, latents=S.tile_noise[:4].clone(), tile_batch=1), base)          # a repeated call is equal


def test_tile_batch_two_is_the_merge_of_two_batched_calls(S):
    from arcflow_amd import ops, schedule
    plan = schedule.tile_plan(40, 56, SIZE, 8)
    canvas = ops.image_resample(torch.from_numpy(S.photo)[None].cuda(), 40, 56)
    got = _enhance(S, latents=S.tile_noise[:4].clone(), tile_batch=2)
    assert torch.equal(got, _by_hand(S, canvas, plan, S.tile_noise[:4], 2))
    three = _enhance(S, latents=S.tile_noise[:4].clone(), tile_batch=3)                 # a last group that is not full: 3 + 1
    assert three.shape == got.shape and torch.equal(three, _by_hand(S, canvas, plan, S.tile_noise[:4], 3))


def test_scale_resamples_the_photo_first(S):
    from arcflow_amd import ops, schedule
    got = _enhance(S, scale=1.5, latents=S.tile_noise.clone(), tile_batch=4)
    assert got.dtype == torch.uint8 and got.shape == (1, 60, 84, 3)
    plan = schedule.tile_plan(60, 84, SIZE, 8)
    assert plan.T == 12
    canvas = ops.image_resample(torch.from_numpy(S.photo)[None].cuda(), 60, 84)
    assert torch.equal(got, _by_hand(S, canvas, plan, S.tile_noise, 4))


def test_a_larger_tile_takes_what_the_axes_hold(S):
    """tile = 64 on the 40 x 56 photo: 2 x 2 tiles of 32 x 48 pixels, a 2 x 3 token grid; the result has the photo's size."""
    from arcflow_amd import schedule
    plan = schedule.tile_plan(40, 56, 64, 8)
    assert (plan.T, plan.th, plan.tw) == (4, 32, 48)
    g = torch.Generator().manual_seed(12)
    noise = torch.randn(4, 2 * 3, 64, generator=g)
    got = _enhance(S, tile=64, latents=noise.clone())
    assert got.dtype == torch.uint8 and got.shape == (1, 40, 56, 3)
    with pytest.raises(ValueError, match='latents'):
        _enhance(S, tile=64, latents=S.tile_noise[:4].clone())                         # noise of the 2 x 2 grid
    # without latents the noise is one draw from the generator: the same seed, the same result
    a = _enhance(S, tile=64, generator=torch.Generator().manual_seed(3))
    assert torch.equal(a, _enhance(S, tile=64, generator=torch.Generator().manual_seed(3))) and not torch.equal(a, got)


def test_output_types_agree(S, base):
    from PIL import Image
    kw = dict(latents=S.tile_noise[:4].clone(), tile_batch=1)
    arr = _enhance(S, output_type='np', **kw)
    assert isinstance(arr, np.ndarray) and arr.dtype == np.float32 and arr.shape == (1, 40, 56, 3)
    assert np.array_equal(arr, base.cpu().numpy().astype(np.float32) / np.float32(255.0))
    pil = _enhance(S, output_type='pil', **kw)
    assert len(pil) == 1 and isinstance(pil[0], Image.Image) and pil[0].size == (56, 40)
    assert np.array_equal(np.asarray(pil[0]), base[0].cpu().numpy())
    tup = S.pipe.enhance(Image.fromarray(S.photo), num_inference_steps=NFE, timestep_ratio=RATIO, output_type='pt', return_dict=False, tile=SIZE,
                         overlap=8, strength=STRENGTH, **_cond(S), **kw)
    assert isinstance(tup, tuple) and len(tup) == 1 and torch.equal(tup[0], base)      # a PIL photo goes the same way


def test_refusals(S):
    kw = dict(latents=S.tile_noise[:4].clone())
    with pytest.raises(ValueError, match='latent'):
        _enhance(S, output_type='latent', **kw)
    with pytest.raises(ValueError, match='one picture'):
        _enhance(S, image=np.stack([S.photo, S.photo]), **kw)
    with pytest.raises(ValueError, match='overlap'):
        _enhance(S, overlap=SIZE // 2 + 1, **kw)
    with pytest.raises(ValueError, match='tile'):
        _enhance(S, tile=40, **kw)
    with pytest.raises(ValueError, match='16'):
        _enhance(S, image=S.photo[:12].copy(), **kw)                                    # a 12-pixel side
    with pytest.raises(ValueError, match='16'):
        _enhance(S, scale=0.25, **kw)                                                   # 10 x 14 after the scale
    with pytest.raises(ValueError, match='tile_batch'):
        _enhance(S, tile_batch=0, **kw)
    with pytest.raises(TypeError):
        _enhance(S, mask_image=torch.ones(1, 1, 40, 56), **kw)                          # masks are out of scope: not a keyword
