"""The CPU side of the SSIM feature: the fp64 reference of tests/ssim_ref.py against cases that can be worked out by hand, the separation of
its seven mutated versions on the inputs of the GPU test (tests/test_hip_image_ssim_fp64.py), ``ssim_from_sums`` and the argument guards of
``afx_image_ssim`` / ``afx_image_ssim_ws_bytes`` that need no device.  No GPU compute is launched here."""
import ctypes as C

import pytest
import torch

import ssim_ref as SR

SHAPES = [(2, 3, 11, 11), (2, 3, 16, 24), (1, 3, 45, 77), (2, 1, 64, 64), (1, 3, 128, 128)]          # the GPU test's


@pytest.fixture(scope='module')
def lib():
    from arcflow_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_window_is_the_normalised_gaussian():
    g = SR.window()
    assert g.dtype == torch.float64 and g.numel() == 11 and abs(g.sum().item() - 1) < 4 * SR.U
    assert torch.equal(g, g.flip(0)) and g.argmax().item() == 5
    assert abs((g[4] / g[5]).item() - 0.8007374029168081) < 1e-15          # exp(-1 / 4.5)
    assert abs((g[0] / g[5]).item() - 0.0038659201394728076) < 1e-17       # exp(-25 / 4.5)


@pytest.mark.parametrize('L', [1.0, 2.0, 255.0])
def test_constant_images_give_the_luminance_term(L):
    """a = p, b = q everywhere: every variance is 0 up to rounding, so ssim = (2 p q + c1) / (p^2 + q^2 + c1) at every window."""
    for p, q in ((0.25, 0.75), (0.0, 1.0), (0.5, 0.5), (1.0, 0.9)):
        a, b = torch.full((2, 3, 13, 17), p * L, dtype=torch.float64), torch.full((2, 3, 13, 17), q * L, dtype=torch.float64)
        m = SR.ssim_map(a, b, False, L)
        c1 = (0.01 * L) ** 2
        want = (2 * p * q * L * L + c1) / ((p * p + q * q) * L * L + c1)
        assert m.shape == (2, 3, 3, 7)
        assert (m - want).abs().max().item() < 1e-9          # the cancelled variances leave ~1e-16 L^2 against c2 = 9e-4 L^2
    # under the transform: raw -1 and 0 are 0 and 0.5
    m = SR.ssim_map(torch.full((1, 1, 11, 11), -1.0), torch.zeros(1, 1, 11, 11), True, 1.0)
    assert abs(m.item() - 1e-4 / (0.25 + 1e-4)) < 1e-9


def test_equal_images_give_one_and_the_arguments_commute():
    for shape in SHAPES[:4]:
        for transform in (False, True):
            c = SR.case(shape, 'fp32', transform, 'noisy')
            assert torch.equal(SR.ssim_map(c.a, c.a, transform, c.data_range), torch.ones(shape[0], shape[1], shape[2] - 10, shape[3] - 10, dtype=torch.float64))
            ab, ba = SR.ssim_mean(c.a, c.b, transform, c.data_range), SR.ssim_mean(c.b, c.a, transform, c.data_range)
            assert (ab - ba).abs().max().item() <= 2 * c.bound.max().item()
            assert ((c.mean > 0) & (c.mean < 1)).all()


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_every_mutant_moves_the_mean_by_more_than_1e_5(shape):
    """... on every sample of every case the GPU test runs, and by more than 1000 x the bound the kernel is held to there."""
    for dname in ('fp32', 'bf16'):
        for transform in (False, True):
            for partner in SR.PARTNERS:
                c = SR.case(shape, dname, transform, partner)
                assert set(c.mutants) == set(SR.MUTANTS) - (set() if transform else {'no_transform'})
                assert c.bound.max().item() < 1e-7
                for name, m in c.mutants.items():
                    sep = (m - c.mean).abs()
                    assert (sep > 1e-5).all() and (sep > 1000 * c.bound).all(), (shape, dname, transform, partner, name, sep.tolist())


def test_ssim_from_sums():
    from arcflow_amd.train.evaluate import IMAGE_KEYS, ssim_from_sums
    assert IMAGE_KEYS == ('image_psnr', 'image_mse', 'image_ssim')
    got = ssim_from_sums(torch.tensor([3.0 * 54 * 54, 1.5 * 54 * 54]), 3, 64, 64)
    assert got.dtype == torch.float64 and got.device.type == 'cpu' and got.tolist() == [1.0, 0.5]
    assert ssim_from_sums([7.0], 7, 11, 11).tolist() == [1.0]
    assert ssim_from_sums(torch.tensor([[12.0], [6.0]], dtype=torch.float32), 1, 12, 16).tolist() == [1.0, 0.5]
    for bad in ((3, 10, 64), (3, 64, 10), (0, 64, 64)):
        with pytest.raises(ValueError):
            ssim_from_sums([1.0], *bad)


def test_image_ssim_entry_points_validate_before_launch(lib):
    """Every guard of afx_image_ssim returns AFX_E_INVALID, and afx_last_error() names the entry, before anything touches the device (fake but
    aligned pointers: a launch would fault).  Each call carries exactly one defect."""
    from arcflow_amd import _lib
    p = lambda off=0: C.c_void_p(1 << 20 | off)         # noqa: E731
    wsb = lib.afx_image_ssim_ws_bytes
    assert wsb(2, 3, 11, 11) == 2 * 3 * 8 and wsb(2, 3, 16, 24) == 2 * 3 * 8 and wsb(1, 3, 45, 77) == 3 * 3 * 3 * 8
    assert wsb(2, 1, 64, 64) == 2 * 4 * 2 * 8 and wsb(1, 3, 128, 128) == 3 * 8 * 4 * 8 and wsb(1, 3, 1024, 1024) == 3 * 64 * 32 * 8
    assert wsb(1, 1, 26, 42) == 8 and wsb(1, 1, 27, 42) == 16 and wsb(1, 1, 26, 43) == 16          # 16 x 32 windows fill one tile
    for bad in ((0, 3, 11, 11), (1, 0, 11, 11), (1, 3, 10, 11), (1, 3, 11, 10), (-1, 3, 11, 11)):
        assert wsb(*bad) == _lib.AFX_E_INVALID and b'afx_image_ssim_ws_bytes' in lib.afx_last_error()
    ok = dict(a=p(), b=p(), dtype=_lib.AFX_DT_F32, transform=1, data_range=1.0, out=p(), ws=p(), ws_bytes=1 << 20, batch=2, C=3, H=45, W=77)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.afx_image_ssim(a['a'], a['b'], a['dtype'], a['transform'], a['data_range'], a['out'], a['ws'], a['ws_bytes'], a['batch'], a['C'],
                                  a['H'], a['W'], None)
    defects = dict(a=None, b=None, out=None, ws=None, dtype=_lib.AFX_DT_FP8, transform=2, data_range=0.0, batch=0, C=0, H=10, W=10,
                   ws_bytes=2 * 27 * 8 - 1)
    for name, value in defects.items():
        assert call(**{name: value}) == _lib.AFX_E_INVALID, name
        err = lib.afx_last_error()
        assert b'afx_image_ssim' in err and b'afx_image_ssim_' not in err.replace(b'afx_image_ssim_ws_bytes()', b''), (name, err)
    assert call(dtype=0) == -1 and call(transform=-1) == -1 and call(data_range=-1.0) == -1 and call(data_range=float('nan')) == -1
    assert call(batch=-1) == -1 and call(C=-3) == -1 and call(batch=65536) == -1
    assert call(ws=p(4)) == -1 and b'aligned' in lib.afx_last_error()
    assert call(out=p(4)) == -1 and call(a=p(2)) == -1 and call(b=p(1)) == -1
    assert call(dtype=_lib.AFX_DT_BF16, a=p(1)) == -1 and b'aligned' in lib.afx_last_error()
    assert call(ws_bytes=0) == -1 and b'workspace' in lib.afx_last_error()
