"""``pipe.outpaint`` of both pipelines on the tiny synthetic engines and VAEs of tests/test_edit_resize_gpu.py (its ``Setup``): the 40 x 56
photo extended 24 px to the right and 16 px down, tile 32, overlap 8, blend 4 (5 windows of a 2 x 2 token grid), 2 NFE, ``prompt_embeds``
given.  Every check is a bit-equality: the result is by construction a chain of ordinary inpainting calls, ``ops.image_paste`` and
``ops.canvas_mark`` over the windows of ``schedule.outpaint_plan``.  On the parent commit every test here fails: ``pipe.outpaint``,
``ops.canvas_extend``, ``ops.canvas_mark`` and ``schedule.outpaint_plan`` do not exist."""
import numpy as np
import pytest
import torch

from test_edit_resize_gpu import HP, SIZE, WP, Setup

pytestmark = pytest.mark.gpu

NFE, RATIO = 2, 1.0
GEOM = dict(right=24, bottom=16, tile=SIZE, overlap=8, blend=4)


@pytest.fixture(scope='module', params=['flux', 'qwen'])
def S(request):
    s = Setup(request.param)
    g = torch.Generator().manual_seed(13)
    s.win_noise = torch.randn(5, HP * WP, 64, generator=g)
    return s


def _cond(S):
    if S.family == 'flux':
        return dict(prompt_embeds=S.pe, pooled_prompt_embeds=S.pooled)
    return dict(prompt_embeds=S.pe, prompt_embeds_mask=torch.ones(1, 12, dtype=torch.long))


def _outpaint(S, image=None, output_type='pt', **kw):
    kw = dict(GEOM, **kw)
    out = S.pipe.outpaint(S.photo if image is None else image, num_inference_steps=NFE, timestep_ratio=RATIO, output_type=output_type,
                          **_cond(S), **kw).images
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope='module')
def base(S):
    """The 'pt' result of the geometry above with given noise, and the device mask state after the run: computed once, never modified."""
    from arcflow_amd import ops
    seen = []
    mark = ops.canvas_mark
    ops.canvas_mark = lambda mask, window, blend: seen.append(mask) or mark(mask, window, blend)
    try:
        out = _outpaint(S, latents=S.win_noise.clone())
    finally:
        ops.canvas_mark = mark
    assert len(seen) == 5 and all(m is seen[0] for m in seen)
    return out, seen[0]


def test_result_is_the_chain_of_per_window_calls(S, base):
    from arcflow_amd import ops, schedule
    out, M_end = base
    assert out.dtype == torch.uint8 and out.shape == (1, 56, 80, 3) and out.is_cuda
    plan = schedule.outpaint_plan(40, 56, 0, 0, 24, 16, tile=SIZE, overlap=8, blend=4)
    assert len(plan.windows) == 5 and (plan.wh, plan.ww) == (SIZE, SIZE)
    canvas, M = ops.canvas_extend(torch.from_numpy(S.photo)[None].cuda(), 0, 0, 24, 16, fill='reflect', blend=4)
    fill, M0 = canvas.clone(), M.clone()
    for k, (x0, y0, x1, y1) in enumerate(plan.windows):
        win = (canvas[0, y0:y1, x0:x1].cpu().numpy().astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)[None]       # byte / 255 exactly
        mwin = M[:, :, y0:y1, x0:x1].contiguous()
        edit = S.pipe(image=torch.from_numpy(np.ascontiguousarray(win)), mask_image=mwin.cpu(), strength=1.0, latents=S.win_noise[k:k + 1].clone(),
                      num_images_per_prompt=1, composite=False, num_inference_steps=NFE, timestep_ratio=RATIO, output_type='pt',
                      **_cond(S)).images
        assert edit.shape == (1, 3, SIZE, SIZE)
        canvas = ops.image_paste(edit.float().contiguous(), mwin, canvas, (x0, y0, x1, y1))
        ops.canvas_mark(M, (x0, y0, x1, y1), 4)
    assert torch.equal(out, canvas)
    assert (M == 0).all() and (M_end == 0).all() and M_end.shape == (1, 1, 56, 80)          # nothing is left to paint, on the device too
    # every photo byte whose canvas_extend mask is 0 is the photo's own
    keep = (M0[0, 0, :40, :56] == 0).cpu().numpy()
    assert keep.sum() == 36 * 52 and np.array_equal(out[0, :40, :56].cpu().numpy()[keep], S.photo[keep])
    # ... and every new pixel was painted: its bytes differ from the fill (3 random bytes of a decoder's output against the mirrored photo)
    new = np.ones((56, 80), dtype=bool)
    new[:40, :56] = False
    differs = (out[0] != fill[0]).any(dim=2).cpu().numpy()
    assert differs[new].mean() > 0.95
    assert torch.equal(_outpaint(S, latents=S.win_noise.clone()), out)                      # the same latents, the same bytes


def test_blend_zero_keeps_every_photo_byte(S):
    out = _outpaint(S, blend=0, latents=S.win_noise.clone())
    assert out.shape == (1, 56, 80, 3) and np.array_equal(out[0, :40, :56].cpu().numpy(), S.photo)
    edge = _outpaint(S, blend=0, fill='edge', latents=S.win_noise.clone())
    assert np.array_equal(edge[0, :40, :56].cpu().numpy(), S.photo) and not torch.equal(edge, out)       # the fill steers what is painted


def test_seeds_and_latents(S, base):
    a = _outpaint(S, generator=torch.Generator().manual_seed(3))
    assert torch.equal(a, _outpaint(S, generator=torch.Generator().manual_seed(3)))
    assert not torch.equal(a, _outpaint(S, generator=torch.Generator().manual_seed(4))) and not torch.equal(a, base[0])
    with pytest.raises(ValueError, match='latents'):
        _outpaint(S, latents=S.win_noise[:4].clone())
    with pytest.raises(ValueError, match='latents'):
        _outpaint(S, latents=torch.zeros(5, 6, 64))


def test_output_types_agree(S, base):
    from PIL import Image
    out = base[0]
    arr = _outpaint(S, output_type='np', latents=S.win_noise.clone())
    assert isinstance(arr, np.ndarray) and arr.dtype == np.float32 and arr.shape == (1, 56, 80, 3)
    assert np.array_equal(arr, out.cpu().numpy().astype(np.float32) / np.float32(255.0))
    pil = _outpaint(S, output_type='pil', latents=S.win_noise.clone())
    assert len(pil) == 1 and isinstance(pil[0], Image.Image) and pil[0].size == (80, 56)
    assert np.array_equal(np.asarray(pil[0]), out[0].cpu().numpy())
    tup = S.pipe.outpaint(Image.fromarray(S.photo), num_inference_steps=NFE, timestep_ratio=RATIO, output_type='pt', return_dict=False,
                          latents=S.win_noise.clone(), **GEOM, **_cond(S))
    assert isinstance(tup, tuple) and len(tup) == 1 and torch.equal(tup[0], out)           # a PIL photo goes the same way
