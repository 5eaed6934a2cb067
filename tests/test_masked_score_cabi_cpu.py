"""``afx_sample_score_masked`` and ``afx_image_ssim_masked`` refuse every bad argument on the host, before any launch, by their own name.
Fake but aligned pointers (a launch would fault, and there is no GPU here): every refusal is AFX_E_INVALID from the entry's checks.
"""
import ctypes as C

import pytest


@pytest.fixture(scope='module')
def lib():
    from arcflow_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def _p(off=0):
    return (1 << 24) + off


def test_both_entries_are_declared_in_the_header_and_exported(lib):
    from arcflow_amd import _lib
    for name in ('afx_sample_score_masked', 'afx_sample_score_masked_ws_bytes', 'afx_image_ssim_masked', 'afx_image_ssim_masked_ws_bytes'):
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    assert len(_lib.PROTOTYPES['afx_sample_score_masked'][1]) == 15 and len(_lib.PROTOTYPES['afx_image_ssim_masked'][1]) == 15


def test_sample_score_masked_refuses_bad_arguments_before_launch(lib):
    from arcflow_amd import _lib
    vp = C.c_void_p
    # [2, 130, 64] latents with a [2, 130, 4] mask: n = 8320, two work-groups per sample, 2 x 2 x 10 doubles of workspace
    ok = dict(a=_p(), b=_p(1 << 20), mask=_p(2 << 20), dtype=_lib.AFX_DT_F32, transform=0, out=_p(3 << 20), ws=_p(4 << 20), ws_bytes=320, batch=2,
              mask_batch=2, G=1, P=130, R=64, Q=4)
    assert lib.afx_sample_score_masked_ws_bytes(2, 8320) == 320 and lib.afx_sample_score_masked_ws_bytes(1, 64) == 80
    assert lib.afx_sample_score_masked_ws_bytes(3, 64 * 8192 + 64) == 3 * 64 * 80

    def call(**d):
        k = dict(ok, **d)
        ptr = lambda v: vp(v) if v else None      # noqa: E731
        return lib.afx_sample_score_masked(ptr(k['a']), ptr(k['b']), ptr(k['mask']), k['dtype'], k['transform'], ptr(k['out']), ptr(k['ws']), k['ws_bytes'],
                                           k['batch'], k['mask_batch'], k['G'], k['P'], k['R'], k['Q'], None)
    for d, msg in ((dict(a=0), b'null'), (dict(b=0), b'null'), (dict(mask=0), b'null'), (dict(out=0), b'null'), (dict(ws=0), b'null'),
                   (dict(dtype=_lib.AFX_DT_FP8), b'dtype'), (dict(dtype=0), b'dtype'), (dict(transform=2), b'transform'),
                   (dict(P=3, R=32), b'multiple of 64'), (dict(G=3, P=12 * 43, R=1, Q=1), b'multiple of 64'),          # n = 96, n = 1548
                   (dict(Q=3), b'must divide'), (dict(Q=128), b'must divide'), (dict(Q=0), b'>= 1'), (dict(R=0), b'>= 1'), (dict(G=0), b'>= 1'),
                   (dict(P=-1), b'>= 1'), (dict(mask_batch=3), b'mask_batch'), (dict(mask_batch=0), b'mask_batch'), (dict(batch=-1), b'batch'),
                   (dict(ws_bytes=319), b'workspace'), (dict(batch=3, mask_batch=1), b'workspace'),
                   (dict(G=1 << 20, P=1 << 10, R=64), b'2^31'), (dict(a=_p(8)), b'aligned'), (dict(mask=_p((2 << 20) + 2)), b'aligned'),
                   (dict(out=_p((3 << 20) + 4)), b'aligned'), (dict(ws=_p((4 << 20) + 4)), b'aligned')):
        assert call(**d) == _lib.AFX_E_INVALID, d
        err = lib.afx_last_error()
        assert b'afx_sample_score_masked' in err and msg in err, (d, err)
    assert lib.afx_sample_score_masked_ws_bytes(2, 72) < 0 and b'afx_sample_score_masked_ws_bytes' in lib.afx_last_error()
    assert call(batch=0, mask_batch=0) == 0                    # an empty batch: nothing to launch


def test_image_ssim_masked_refuses_bad_arguments_before_launch(lib):
    from arcflow_amd import _lib
    vp = C.c_void_p
    # [2, 3, 12, 43]: 1 x 2 tiles per plane, 2 x 3 x 2 slots of 4 doubles
    ok = dict(a=_p(), b=_p(1 << 20), mask=_p(2 << 20), dtype=_lib.AFX_DT_BF16, transform=1, data_range=1.0, out=_p(3 << 20), ws=_p(4 << 20),
              ws_bytes=384, batch=2, mask_batch=1, C=3, H=12, W=43)
    assert lib.afx_image_ssim_masked_ws_bytes(2, 3, 12, 43) == 384 == 4 * lib.afx_image_ssim_ws_bytes(2, 3, 12, 43)
    assert lib.afx_image_ssim_masked_ws_bytes(1, 1, 11, 11) == 32 and lib.afx_image_ssim_masked_ws_bytes(1, 3, 27, 12) == 3 * 2 * 32

    def call(**d):
        k = dict(ok, **d)
        ptr = lambda v: vp(v) if v else None      # noqa: E731
        return lib.afx_image_ssim_masked(ptr(k['a']), ptr(k['b']), ptr(k['mask']), k['dtype'], k['transform'], k['data_range'], ptr(k['out']),
                                         ptr(k['ws']), k['ws_bytes'], k['batch'], k['mask_batch'], k['C'], k['H'], k['W'], None)
    for d, msg in ((dict(a=0), b'null'), (dict(b=0), b'null'), (dict(mask=0), b'null'), (dict(out=0), b'null'), (dict(ws=0), b'null'),
                   (dict(dtype=_lib.AFX_DT_FP8), b'dtype'), (dict(dtype=0), b'dtype'), (dict(transform=-1), b'transform'),
                   (dict(data_range=0.0), b'data_range'), (dict(H=10), b'at least 11'), (dict(W=10), b'at least 11'),
                   (dict(mask_batch=3), b'mask_batch'), (dict(mask_batch=0), b'mask_batch'), (dict(batch=0, mask_batch=0), b'batch'), (dict(C=0), b'C >= 1'),
                   (dict(ws_bytes=383), b'workspace'), (dict(a=_p(1)), b'aligned'), (dict(mask=_p((2 << 20) + 2)), b'aligned'),
                   (dict(out=_p((3 << 20) + 4)), b'aligned')):
        assert call(**d) == _lib.AFX_E_INVALID, d
        err = lib.afx_last_error()
        assert b'afx_image_ssim_masked' in err and msg in err, (d, err)
    assert lib.afx_image_ssim_masked_ws_bytes(1, 3, 10, 64) < 0 and b'afx_image_ssim_masked_ws_bytes' in lib.afx_last_error()
