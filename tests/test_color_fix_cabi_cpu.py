"""The argument guards of afx_color_fix without a GPU: every refusal comes before the first launch, so the pointers are never dereferenced
and plain integers stand in for device memory; the good arguments are never called.  Then the pipelines' refusals of ``color_fix=``, which
come before anything runs (no engine, no VAE, no GPU).  On the parent commit every test here fails: the header does not declare the
entry, ``ops.color_fix`` does not exist and ``color_fix`` is an unknown keyword."""
import ctypes as C

import pytest
import torch

MB = 1 << 20
B, CH, H, W = 2, 3, 40, 56
NAMES = ['edit', 'dtype', 'src', 'src_batch', 'src01', 'mode', 'out', 'stats', 'ws', 'ws_bytes', 'batch', 'C', 'H', 'W', 'stream']
PTRS = ('edit', 'src', 'out', 'stats', 'ws')


def _call(lib, good):
    def call(**kw):
        a = dict(good, **kw)
        return lib.afx_color_fix(*[a[n] for n in NAMES])
    return call


def _good(_lib, mode):
    ptr = {n: C.c_void_p(16 * MB * (k + 1)) for k, n in enumerate(PTRS)}
    return dict(ptr, dtype=_lib.AFX_DT_F32, src_batch=B, src01=1, mode=mode, ws_bytes=8 * MB, batch=B, C=CH, H=H, W=W, stream=None)


def test_constants_and_ws_bytes():
    from arcflow_amd import _lib
    lib = _lib.load()
    assert (_lib.AFX_COLOR_ADAIN, _lib.AFX_COLOR_WAVELET, _lib.AFX_COLOR_WAVELET_LEVELS) == (0, 1, 2)
    assert len(_lib.PROTOTYPES['afx_color_fix'][1]) == len(NAMES)
    assert lib.afx_color_fix_ws_bytes(_lib.AFX_COLOR_WAVELET, B, CH, H, W) == 0                    # the fused pass needs none
    assert lib.afx_color_fix_ws_bytes(_lib.AFX_COLOR_WAVELET_LEVELS, B, CH, H, W) == 2 * 4 * B * CH * H * W
    parts = -(-H * W // 4096)
    assert lib.afx_color_fix_ws_bytes(_lib.AFX_COLOR_ADAIN, B, CH, H, W) == 8 * B * CH * (4 * parts + 1)
    assert lib.afx_color_fix_ws_bytes(_lib.AFX_COLOR_ADAIN, 1, 3, 1024, 1024) == 8 * 3 * (4 * 256 + 1)
    for bad in ((3, B, CH, H, W), (-1, B, CH, H, W), (0, 0, CH, H, W), (1, B, 0, H, W), (1, B, CH, 0, W), (2, B, CH, H, -1)):
        assert lib.afx_color_fix_ws_bytes(*bad) == _lib.AFX_E_INVALID, bad
    # the grid limit the header states: the work-groups of a launch stay below 2^31
    assert lib.afx_color_fix_ws_bytes(_lib.AFX_COLOR_WAVELET, 32768, 65535, 64, 64) == 0           # 2^31 - 32768 tiles
    assert lib.afx_color_fix_ws_bytes(_lib.AFX_COLOR_WAVELET, 32768, 65535, 65, 64) == _lib.AFX_E_INVALID
    assert b'work-groups' in lib.afx_last_error()
    assert lib.afx_color_fix_ws_bytes(_lib.AFX_COLOR_ADAIN, 32768, 65535, 64, 64) == _lib.AFX_E_INVALID
    assert lib.afx_color_fix_ws_bytes(_lib.AFX_COLOR_WAVELET, 65536, 65536, 1, 1) == _lib.AFX_E_INVALID      # batch C itself
    assert lib.afx_color_fix_ws_bytes(_lib.AFX_COLOR_WAVELET, 1, 1, 65536, 65536) == _lib.AFX_E_INVALID      # H W itself


@pytest.mark.parametrize('mode_name', ['AFX_COLOR_ADAIN', 'AFX_COLOR_WAVELET', 'AFX_COLOR_WAVELET_LEVELS'])
def test_color_fix_abi_guards(mode_name):
    from arcflow_amd import _lib
    lib = _lib.load()
    mode = getattr(_lib, mode_name)
    good = _good(_lib, mode)
    call = _call(lib, good)
    INV, WSE = _lib.AFX_E_INVALID, _lib.AFX_E_WORKSPACE
    needs_ws = mode != _lib.AFX_COLOR_WAVELET
    for name in ('edit', 'src', 'out'):
        assert call(**{name: None}) == INV and b'null argument to afx_color_fix' in lib.afx_last_error(), name
    for bad in (0, _lib.AFX_DT_FP8, 7):
        assert call(dtype=bad) == INV and b'dtype' in lib.afx_last_error(), bad
    for bad in (-1, 3, 17):
        assert call(mode=bad) == INV, bad
    for bad in (-1, 2):
        assert call(src01=bad) == INV and b'src01' in lib.afx_last_error(), bad
    for bad in (0, 3, B + 1, -1):
        assert call(src_batch=bad) == INV and b'src_batch' in lib.afx_last_error(), bad
    for name in ('batch', 'C', 'H', 'W'):
        for bad in (0, -4):
            assert call(**{name: bad}) == INV, (name, bad)
    # alignment: the edit to its element, src and out to 4 bytes, stats and ws to 8
    at = lambda n, off: C.c_void_p(good[n].value + off)          # noqa: E731
    assert call(edit=at('edit', 2)) == INV and b'aligned' in lib.afx_last_error()
    assert call(edit=at('edit', 1), dtype=_lib.AFX_DT_BF16) == INV and b'aligned' in lib.afx_last_error()
    for name, off in (('src', 2), ('out', 2), ('ws', 4)):
        assert call(**{name: at(name, off)}) == INV and b'aligned' in lib.afx_last_error(), name
    if mode == _lib.AFX_COLOR_ADAIN:
        assert call(stats=at('stats', 4)) == INV and b'aligned' in lib.afx_last_error()
    # overlaps: a written range begins on an operand's last byte / ends on its first (aligned, so the overlap is what refuses)
    ebytes = obytes = sbytes = 4 * B * CH * H * W
    need = lib.afx_color_fix_ws_bytes(mode, B, CH, H, W)
    written = [('out', obytes, 4)]
    if mode == _lib.AFX_COLOR_ADAIN:
        written.append(('stats', 32 * B * CH, 8))
    if needs_ws:
        written.append(('ws', need, 8))
    for wname, wbytes, al in written:
        for oname, nbytes in (('edit', ebytes), ('src', sbytes)):
            for addr in (good[oname].value + (nbytes - 1) // al * al, good[oname].value - wbytes + al):
                assert call(**{wname: C.c_void_p(addr)}) == INV and b'overlaps' in lib.afx_last_error(), (wname, oname)
        assert call(**{wname: good['edit']}) == INV and b'overlaps' in lib.afx_last_error(), wname          # in place
    for a, b, abytes in (('stats', 'out', 0), ('ws', 'out', 0), ('ws', 'stats', 0)):
        if (a == 'ws' and not needs_ws) or ('stats' in (a, b) and mode != _lib.AFX_COLOR_ADAIN):
            continue
        assert call(**{a: good[b]}) == INV and b'overlaps' in lib.afx_last_error(), (a, b)
    assert call(src_batch=1, out=C.c_void_p(good['src'].value + sbytes // 2 - 4)) == INV and b'overlaps' in lib.afx_last_error()
    # the workspace, where the mode needs one
    if needs_ws:
        assert call(ws=None) == WSE and b'workspace' in lib.afx_last_error()
        assert call(ws_bytes=need - 1) == WSE and call(ws_bytes=0) == WSE
    # the grid limit
    assert call(batch=32768, src_batch=1, C=65535, H=65, W=64) == INV


def test_ops_color_fix_refuses_cpu_tensors_and_wrong_layouts():
    from arcflow_amd import _lib, ops
    e, s = torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16)
    with pytest.raises(ValueError, match='mode'):
        ops.color_fix(e, s, mode='lab')
    with pytest.raises(_lib.ArcflowHipError, match='GPU tensors only'):
        ops.color_fix(e, s)
    with pytest.raises(ValueError, match='mode'):
        ops.color_fix_ws('histogram', 1, 3, 16, 16)


def _pipe(family):
    from arcflow_amd.pipelines import ArcFluxPipeline, ArcQwenImagePipeline
    return ArcFluxPipeline() if family == 'flux' else ArcQwenImagePipeline()         # no engine, no VAE: the guards come first


@pytest.mark.parametrize('family', ['flux', 'qwen'])
def test_pipelines_refuse_bad_color_fix_before_anything_runs(family):
    pipe = _pipe(family)
    pe = torch.zeros(1, 4, 128)
    kw = dict(prompt_embeds=pe, pooled_prompt_embeds=torch.zeros(1, 64)) if family == 'flux' else dict(prompt_embeds=pe)
    img, lat, mask = torch.rand(1, 3, 32, 48), torch.zeros(1, 6, 64), torch.ones(1, 1, 32, 48)
    for entry in (pipe, pipe.sample_teacher):
        with pytest.raises(ValueError, match="`color_fix`: None, 'adain' or 'wavelet'"):
            entry(image=img, color_fix='lab', **kw)
        with pytest.raises(ValueError, match='`color_fix` needs `image`'):
            entry(color_fix='wavelet', **kw)                                          # text-to-image
        with pytest.raises(ValueError, match='`color_fix` needs `image`'):
            entry(image_latents=lat, color_fix='adain', **kw)                         # latents only: no pixels to match
        with pytest.raises(ValueError, match='`color_fix` does not go with `mask_image`'):
            entry(image=img, mask_image=mask, color_fix='wavelet', **kw)
        with pytest.raises(ValueError, match='`color_fix` does not go with `mask_image`'):
            entry(image=img, mask_image=mask, padding_mask_crop=8, color_fix='wavelet', **kw)
        with pytest.raises(ValueError, match='`color_fix` works on decoded pixels'):
            entry(image=img, color_fix='adain', output_type='latent', **kw)
    with pytest.raises(ValueError, match='`color_fix`'):
        pipe.enhance(img[0], color_fix='lab', **kw)
    with pytest.raises(ValueError, match='latent'):
        pipe.enhance(img[0], color_fix='wavelet', output_type='latent', **kw)
