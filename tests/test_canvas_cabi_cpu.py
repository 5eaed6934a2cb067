"""The argument guards of afx_canvas_extend / afx_canvas_mark without a GPU: AFX_E_INVALID before any launch, so the pointers are never
dereferenced and plain integers stand in for device memory; the good arguments are never called.  Then the refusals of
``ops.canvas_extend`` / ``ops.canvas_mark`` and of both pipelines' ``outpaint``, which come before anything touches an engine, a VAE or the
GPU.  On the parent commit every test here fails: the header declares neither entry, and ``ops.canvas_*`` and ``pipe.outpaint`` do not exist."""
import ctypes as C

import numpy as np
import pytest
import torch

MB = 1 << 20
B, H, W, L, T, R, BT = 2, 40, 56, 16, 24, 8, 0
HC, WC = H + T + BT, W + L + R


def _caller(f, names, good):
    def call(**kw):
        a = dict(good, **kw)
        return f(*[a[n] for n in names])
    return call


def test_canvas_extend_abi_guards():
    from arcflow_amd import _lib
    lib = _lib.load()
    assert (_lib.AFX_FILL_EDGE, _lib.AFX_FILL_REFLECT) == (0, 1)
    names = ['src', 'batch', 'H', 'W', 'left', 'top', 'right', 'bottom', 'fill', 'blend', 'canvas', 'mask', 'stream']
    res, args = _lib.PROTOTYPES['afx_canvas_extend']
    assert res is C.c_int32 and len(args) == len(names)
    assert [a is C.c_void_p for a in args] == [n in ('src', 'canvas', 'mask', 'stream') for n in names]
    ptr = {n: C.c_void_p(MB * (k + 1)) for k, n in enumerate(('src', 'canvas', 'mask'))}
    call = _caller(lib.afx_canvas_extend, names, dict(ptr, batch=B, H=H, W=W, left=L, top=T, right=R, bottom=BT, fill=_lib.AFX_FILL_REFLECT,
                                                      blend=4, stream=None))
    for name in ptr:
        assert call(**{name: None}) == _lib.AFX_E_INVALID and b'null argument to afx_canvas_extend' in lib.afx_last_error(), name
    for name in ('batch', 'H', 'W'):
        assert call(**{name: 0}) == _lib.AFX_E_INVALID and call(**{name: -1}) == _lib.AFX_E_INVALID, name
    for bad in (2, -1, 7):
        assert call(fill=bad) == _lib.AFX_E_INVALID and b'unknown fill' in lib.afx_last_error(), bad
    for name in ('left', 'top', 'right', 'bottom'):
        assert call(**{name: -1}) == _lib.AFX_E_INVALID and b'extents' in lib.afx_last_error(), name
    assert call(left=0, top=0, right=0, bottom=0) == _lib.AFX_E_INVALID and b'extents' in lib.afx_last_error()
    assert call(blend=-1) == _lib.AFX_E_INVALID and b'blend' in lib.afx_last_error()
    for off in (1, 2, 3):
        assert call(mask=C.c_void_p(ptr['mask'].value + off)) == _lib.AFX_E_INVALID and b'4-byte aligned' in lib.afx_last_error(), off
    sbytes, cbytes, mbytes = B * H * W * 3, B * HC * WC * 3, HC * WC * 4
    for at in (ptr['src'].value + sbytes - 1, ptr['src'].value - cbytes + 1):             # canvas begins on src's last byte / ends on its first
        assert call(canvas=C.c_void_p(at)) == _lib.AFX_E_INVALID and b'overlaps' in lib.afx_last_error(), at
    for base, nbytes in ((ptr['src'].value, sbytes), (ptr['canvas'].value, cbytes)):      # mask on src, mask on canvas (4-byte aligned addresses)
        for at in (base + (nbytes - 1) // 4 * 4, base - mbytes + 4):
            assert call(mask=C.c_void_p(at)) == _lib.AFX_E_INVALID and b'overlaps' in lib.afx_last_error(), at
    # the grid limit: a canvas side past 2^31 - 1, and a pixel count past the 64-bit byte offsets
    big = 2 ** 30
    for bad in (dict(H=big, top=big, bottom=big), dict(W=big, left=big, right=big), dict(W=2 ** 31 - 1, left=1),
                dict(batch=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1, top=0, bottom=0, left=0, right=1)):
        assert call(**bad) == _lib.AFX_E_INVALID and b'index range' in lib.afx_last_error(), bad


def test_canvas_mark_abi_guards():
    from arcflow_amd import _lib
    lib = _lib.load()
    names = ['mask', 'Hc', 'Wc', 'x0', 'y0', 'x1', 'y1', 'blend', 'stream']
    res, args = _lib.PROTOTYPES['afx_canvas_mark']
    assert res is C.c_int32 and len(args) == len(names)
    mask = C.c_void_p(MB)
    call = _caller(lib.afx_canvas_mark, names, dict(mask=mask, Hc=48, Wc=80, x0=8, y0=4, x1=40, y1=36, blend=4, stream=None))
    assert call(mask=None) == _lib.AFX_E_INVALID and b'null argument to afx_canvas_mark' in lib.afx_last_error()
    for name in ('Hc', 'Wc'):
        assert call(**{name: 0}) == _lib.AFX_E_INVALID and call(**{name: -48}) == _lib.AFX_E_INVALID, name
    outside = (dict(x0=-1), dict(y0=-1), dict(x1=81), dict(y1=49), dict(Wc=39), dict(Hc=35), dict(x0=80, x1=112))
    empty = (dict(x1=8), dict(y1=4), dict(x0=40), dict(y0=36), dict(x0=41), dict(x1=0), dict(y1=-3))
    for bad in outside + empty:
        assert call(**bad) == _lib.AFX_E_INVALID and b'non-empty and inside' in lib.afx_last_error(), bad
    assert call(blend=-1) == _lib.AFX_E_INVALID and b'blend' in lib.afx_last_error()
    for off in (1, 2, 3):
        assert call(mask=C.c_void_p(MB + off)) == _lib.AFX_E_INVALID and b'4-byte aligned' in lib.afx_last_error(), off


def test_ops_refuse_cpu_tensors_and_wrong_layouts():
    from arcflow_amd import _lib, ops
    src = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(_lib.ArcflowHipError, match='GPU tensors only'):
        ops.canvas_extend(src, 1, 0, 0, 0)
    with pytest.raises(_lib.ArcflowHipError, match='GPU tensors only'):
        ops.canvas_mark(torch.ones(1, 1, 8, 8), (0, 0, 4, 4), 1)
    # the layout, the dtype and the integers are checked first, so a CPU tensor shows those refusals too
    u8 = lambda *shape: torch.zeros(*shape, dtype=torch.uint8)                                            # noqa: E731
    f32 = lambda *shape: torch.ones(*shape)                                                               # noqa: E731
    with pytest.raises(ValueError, match='fill'):
        ops.canvas_extend(src, 1, 0, 0, 0, fill='wrap')
    for bad in (u8(8, 8, 3), u8(1, 3, 8, 8), u8(1, 8, 8, 1), f32(1, 8, 8, 3), u8(1, 8, 16, 3)[:, :, ::2], u8(1, 8, 0, 3)):
        with pytest.raises(ValueError, match='src_u8'):
            ops.canvas_extend(bad, 1, 0, 0, 0)
    for ext in ((0, 0, 0, 0), (-1, 0, 0, 2), (1.5, 0, 0, 0), (True, 0, 0, 0)):
        with pytest.raises(ValueError, match='left|top|right|bottom'):
            ops.canvas_extend(src, *ext)
    with pytest.raises(ValueError, match='blend'):
        ops.canvas_extend(src, 1, 0, 0, 0, blend=-1)
    for bad in (f32(2, 1, 8, 8), f32(1, 3, 8, 8), f32(8), f32(1, 8, 8), u8(1, 1, 8, 8), f32(1, 1, 8, 16)[..., ::2], f32(8, 8).double()):
        with pytest.raises(ValueError, match='mask'):
            ops.canvas_mark(bad, (0, 0, 4, 4), 1)
    for win in ((0, 0, 9, 4), (4, 0, 4, 4), (-1, 0, 4, 4), (0, 0, 4, 9), (0, 5, 4, 5), (0.5, 0, 4, 4)):
        with pytest.raises(ValueError, match='window'):
            ops.canvas_mark(f32(1, 1, 8, 8), win, 1)
    with pytest.raises(ValueError, match='blend'):
        ops.canvas_mark(f32(8, 8), (0, 0, 4, 4), -2)


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_outpaint_refuses_before_anything_runs(family):
    """A pipeline without an engine, a VAE or text encoders: every refusal is raised on the host, before any of them is asked for."""
    from arcflow_amd.pipelines import ArcFluxPipeline, ArcQwenImagePipeline
    pipe = (ArcFluxPipeline if family == 'flux' else ArcQwenImagePipeline)()
    assert pipe.transformer is None and pipe.vae is None
    photo = np.zeros((40, 56, 3), dtype=np.uint8)
    kw = dict(right=24, bottom=16, tile=32, overlap=8, blend=4)
    with pytest.raises(ValueError, match='8-bit pixels'):
        pipe.outpaint(photo.astype(np.float32), **kw)
    with pytest.raises(ValueError, match='8-bit pixels'):
        pipe.outpaint(torch.zeros(1, 3, 40, 56), **kw)
    with pytest.raises(ValueError, match='batch of 2'):
        pipe.outpaint(np.stack([photo, photo]), **kw)
    with pytest.raises(ValueError, match='at least one > 0'):
        pipe.outpaint(photo, tile=32, overlap=8, blend=4)
    with pytest.raises(ValueError, match='blend'):
        pipe.outpaint(photo, **dict(kw, blend=5))
    with pytest.raises(ValueError, match='latent'):
        pipe.outpaint(photo, output_type='latent', **kw)
    with pytest.raises(ValueError, match='fill'):
        pipe.outpaint(photo, fill='wrap', **kw)
    with pytest.raises(ValueError, match='overlap'):
        pipe.outpaint(photo, **dict(kw, overlap=17))
    with pytest.raises(ValueError, match='strength'):
        pipe.outpaint(photo, strength=0.0, **kw)
    with pytest.raises(ValueError, match='latents'):
        pipe.outpaint(photo, latents=torch.zeros(4, 4, 64), **kw)                                         # the plan has 5 windows
