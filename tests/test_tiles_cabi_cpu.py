"""The argument guards of afx_tiles_cut / afx_tiles_merge without a GPU: AFX_E_INVALID before any launch, so the pointers are never
dereferenced and plain integers stand in for device memory; the good arguments are never called.  On the parent commit every test here
fails: the header declares neither entry."""
import ctypes as C

MB = 1 << 20
H, W, TH, TW, KY, KX, TY, TX = 40, 56, 32, 32, 2, 2, 2, 2


def _caller(f, names, good):
    def call(**kw):
        a = dict(good, **kw)
        return f(*[a[n] for n in names])
    return call


def test_tiles_merge_abi_guards():
    from arcflow_amd import _lib, schedule
    lib = _lib.load()
    assert _lib.AFX_TILE_MAX_TAPS == schedule.AFX_TILE_MAX_TAPS == 4
    names = ['tiles', 'T', 'th', 'tw', 'oy', 'ky', 'ox', 'kx', 'y_start', 'y_count', 'y_w', 'y_taps', 'x_start', 'x_count', 'x_w', 'x_taps',
             'dst', 'H', 'W', 'stream']
    assert len(_lib.PROTOTYPES['afx_tiles_merge'][1]) == len(names)
    ptrs = [n for n in names if n in ('tiles', 'oy', 'ox', 'dst') or n[2:] in ('start', 'count', 'w')]
    ptr = {n: C.c_void_p(MB * (k + 1)) for k, n in enumerate(ptrs)}
    call = _caller(lib.afx_tiles_merge, names, dict(ptr, T=KY * KX, th=TH, tw=TW, ky=KY, kx=KX, y_taps=TY, x_taps=TX, H=H, W=W, stream=None))
    for name in ptrs:
        assert call(**{name: None}) == _lib.AFX_E_INVALID and b'null argument to afx_tiles_merge' in lib.afx_last_error(), name
        if name != 'dst':
            assert call(**{name: C.c_void_p(ptr[name].value + 2)}) == _lib.AFX_E_INVALID and b'aligned' in lib.afx_last_error(), name
    for name in ('th', 'tw', 'ky', 'kx', 'H', 'W'):
        assert call(**{name: 0}) == _lib.AFX_E_INVALID and call(**{name: -16}) == _lib.AFX_E_INVALID, name
    for bad in (dict(th=24), dict(tw=40), dict(th=48), dict(tw=64)):                    # no multiple of 16, or larger than the canvas
        assert call(**bad) == _lib.AFX_E_INVALID and b'multiples of 16' in lib.afx_last_error(), bad
    for bad in (dict(T=3), dict(T=5), dict(ky=3), dict(kx=1), dict(T=0)):
        assert call(**bad) == _lib.AFX_E_INVALID and b'T = ' in lib.afx_last_error(), bad
    for name in ('y_taps', 'x_taps'):
        for bad in (0, -1, _lib.AFX_TILE_MAX_TAPS + 1):
            assert call(**{name: bad}) == _lib.AFX_E_INVALID and b'AFX_TILE_MAX_TAPS' in lib.afx_last_error(), (name, bad)
        assert call(**{name: _lib.AFX_TILE_MAX_TAPS, 'dst': None}) == _lib.AFX_E_INVALID and b'null' in lib.afx_last_error()
    sizes = dict(tiles=4 * KY * KX * 3 * TH * TW, oy=4 * KY, ox=4 * KX, y_start=4 * H, y_count=4 * H, y_w=4 * H * TY, x_start=4 * W, x_count=4 * W,
                 x_w=4 * W * TX)
    for name, nbytes in sizes.items():                                                   # dst begins on the operand's last byte / ends on its first
        for at in (ptr[name].value + nbytes - 1, ptr[name].value - H * W * 3 + 1):
            assert call(dst=C.c_void_p(at)) == _lib.AFX_E_INVALID and b'overlaps' in lib.afx_last_error(), name


def test_tiles_cut_abi_guards():
    from arcflow_amd import _lib
    lib = _lib.load()
    names = ['canvas', 'H', 'W', 'oy', 'ky', 'ox', 'kx', 'th', 'tw', 'tiles', 'stream']
    assert len(_lib.PROTOTYPES['afx_tiles_cut'][1]) == len(names)
    ptr = {n: C.c_void_p(MB * (k + 1)) for k, n in enumerate(('canvas', 'oy', 'ox', 'tiles'))}
    call = _caller(lib.afx_tiles_cut, names, dict(ptr, H=H, W=W, ky=KY, kx=KX, th=TH, tw=TW, stream=None))
    for name in ptr:
        assert call(**{name: None}) == _lib.AFX_E_INVALID and b'null argument to afx_tiles_cut' in lib.afx_last_error(), name
        assert call(**{name: C.c_void_p(ptr[name].value + 2)}) == _lib.AFX_E_INVALID and b'aligned' in lib.afx_last_error(), name
    for off in (4, 8, 12):                                                               # tiles is stored in 16-byte chunks
        assert call(tiles=C.c_void_p(ptr['tiles'].value + off)) == _lib.AFX_E_INVALID and b'16-byte' in lib.afx_last_error(), off
    for name in ('th', 'tw', 'ky', 'kx', 'H', 'W'):
        assert call(**{name: 0}) == _lib.AFX_E_INVALID, name
    for bad in (dict(th=24), dict(tw=40), dict(th=48), dict(tw=64)):
        assert call(**bad) == _lib.AFX_E_INVALID and b'multiples of 16' in lib.afx_last_error(), bad
    tbytes = 4 * KY * KX * 3 * TH * TW
    for name, nbytes in dict(canvas=4 * 3 * H * W, oy=4 * KY, ox=4 * KX).items():
        for at in (ptr[name].value + (nbytes - 1) // 16 * 16, ptr[name].value - tbytes + 16):        # (16-byte aligned: the overlap is what refuses)
            assert call(tiles=C.c_void_p(at)) == _lib.AFX_E_INVALID and b'overlaps' in lib.afx_last_error(), name
