"""The argument guards of afx_lora_row_gain / afx_lora_fold_rows without a GPU: AFX_E_INVALID before any launch, so the pointers are never
dereferenced and plain integers stand in for device memory; the good arguments are never called.  Then the refusals of ``ops.lora_row_gain`` and
``ops.lora_fold(..., row_gains=...)`` that come before the library is asked.  On the parent commit every test here fails: the header declares
neither entry."""
import ctypes as C

import pytest
import torch

MB = 1 << 20
vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float


def p(off=0):
    return 16 * MB + off


def test_row_gain_abi_guards():
    from arcflow_amd import _lib
    lib = _lib.load()
    names = ['base', 'ld_base', 'O', 'I', 'A', 'B', 'r', 's', 'm', 'gain', 'stream']
    res, args = _lib.PROTOTYPES['afx_lora_row_gain']
    assert res is i32 and len(args) == len(names)
    assert [a is vp for a in args] == [n in ('base', 'A', 'B', 'm', 'gain', 'stream') for n in names] and args[7] is f32
    good = dict(base=p(), ld_base=256, O=128, I=256, A=p(MB), B=p(2 * MB), r=4, s=0.5, m=p(3 * MB), gain=p(4 * MB), stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.afx_lora_row_gain(*[vp(a[n]) if n in ('base', 'A', 'B', 'm', 'gain') and a[n] else a[n] for n in names])
    for name in ('base', 'A', 'B', 'm', 'gain'):
        assert call(**{name: None}) == _lib.AFX_E_INVALID and b'null' in lib.afx_last_error(), name
    for bad in (dict(O=96), dict(O=0), dict(O=-64), dict(I=96, ld_base=96), dict(I=0)):
        assert call(**bad) == _lib.AFX_E_INVALID and b'multiples of 64' in lib.afx_last_error(), bad
    assert call(ld_base=192) == _lib.AFX_E_INVALID and b'leading dimension' in lib.afx_last_error()
    for bad in (dict(ld_base=260), dict(base=p(8)), dict(A=p(MB + 8)), dict(B=p(2 * MB + 1)), dict(m=p(3 * MB + 2)), dict(gain=p(4 * MB + 1))):
        assert call(**bad) == _lib.AFX_E_INVALID and b'aligned' in lib.afx_last_error(), bad
    for bad in (0, -3):
        assert call(r=bad) == _lib.AFX_E_INVALID and b'rank' in lib.afx_last_error(), bad
    base_bytes, a_bytes, b_bytes = (127 * 256 + 256) * 2, 4 * 256 * 2, 128 * 4 * 2
    for at in (p(base_bytes - 4), p(-128 * 4 + 4), p(MB + a_bytes - 4), p(2 * MB + b_bytes - 4), p(3 * MB), p(3 * MB + 127 * 4)):
        assert call(gain=at) == _lib.AFX_E_INVALID and b'overlaps' in lib.afx_last_error(), at


def test_fold_rows_abi_guards():
    """afx_lora_fold's guards under the new name, plus the gain pointers'."""
    from arcflow_amd import _lib
    lib = _lib.load()
    res, args = _lib.PROTOTYPES['afx_lora_fold_rows']
    assert res is i32 and args == _lib.PROTOTYPES['afx_lora_fold'][1][:-1] + [vp, vp]

    def call(base=p(), ldb=256, dst=p(4 * MB), ldd=256, O=128, I=256, J=2, A=(p(MB), p(2 * MB)), B=(p(3 * MB), p(5 * MB)), ranks=(4, 16),
             scales=(1.0, 0.5), gains=(p(6 * MB), 0), null_arrays=False):
        n = max(len(A), 1)
        arr = lambda ty, v: None if null_arrays else (ty * n)(*v)      # noqa: E731
        return lib.afx_lora_fold_rows(vp(base) if base else None, ldb, vp(dst) if dst else None, ldd, O, I, J, arr(vp, A), arr(vp, B),
                                      arr(i32, ranks), arr(f32, scales), None if gains is None else (vp * n)(*[g or None for g in gains]), None)
    for kw, msg in ((dict(base=0), b'null'), (dict(dst=0), b'null'), (dict(null_arrays=True), b'null'), (dict(A=(p(MB), 0)), b'null'),
                    (dict(B=(0, p(5 * MB))), b'null'),
                    (dict(J=9, A=(p(),) * 9, B=(p(),) * 9, ranks=(4,) * 9, scales=(1.0,) * 9, gains=(0,) * 9), b'adapters'), (dict(J=-1), b'adapters'),
                    (dict(ranks=(4, 0)), b'rank'), (dict(ranks=(-3, 16)), b'rank'),
                    (dict(O=96), b'multiples of 64'), (dict(I=96, ldb=96, ldd=96), b'multiples of 64'), (dict(O=0), b'multiples of 64'),
                    (dict(ldb=192), b'leading dimension'), (dict(ldd=248), b'leading dimension'),
                    (dict(dst=p(64 * 256 * 2)), b'overlaps'), (dict(dst=p()), b'overlaps'), (dict(base=p(8)), b'aligned'),
                    (dict(dst=p(4 * MB + 8)), b'aligned'), (dict(ldd=260), b'aligned'), (dict(A=(p(MB + 8), p(2 * MB))), b'aligned'),
                    (dict(gains=(p(6 * MB + 2), 0)), b'4-byte aligned'), (dict(gains=(0, p(6 * MB + 1))), b'4-byte aligned'),
                    (dict(gains=(p(4 * MB + 64), 0)), b'overlaps the row gains'), (dict(gains=(0, p(4 * MB - 4))), b'overlaps the row gains'),
                    (dict(gains=(0, 0), dst=p()), b'overlaps'), (dict(gains=None, dst=p()), b'overlaps')):
        assert call(**kw) == _lib.AFX_E_INVALID, kw
        assert msg in lib.afx_last_error() and b'afx_lora_fold_rows' in lib.afx_last_error(), (kw, lib.afx_last_error())


def test_ops_refuse_before_the_library():
    from arcflow_amd import _lib, ops
    bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)      # noqa: E731
    with pytest.raises(_lib.ArcflowHipError, match='GPU tensors only'):
        ops.lora_row_gain(bf(64, 64), bf(4, 64), bf(64, 4), 1.0, torch.ones(64))
    with pytest.raises(_lib.ArcflowHipError, match='GPU tensors only'):
        ops.lora_fold(bf(64, 64), bf(64, 64), [bf(4, 64)], [bf(64, 4)], [1.0], row_gains=[torch.ones(64)])
