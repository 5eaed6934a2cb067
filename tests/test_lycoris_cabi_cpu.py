"""The argument guards of afx_lora_fold_terms without a GPU, in the manner of tests/test_lora_dora_cabi_cpu.py: AFX_E_INVALID before any launch, so
the pointers are never dereferenced and plain integers stand in for device memory; the good arguments are never called.  Then the structure as
``_lib.parse_struct`` derives it from the header, and the refusals of ``ops.lora_fold_terms`` that come before the library is asked.  On the parent
commit every test here fails: the header declares neither the entry nor the structure."""
import ctypes as C

import pytest
import torch

MB = 1 << 20
vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float


def p(off=0):
    return 16 * MB + off


def test_struct_and_prototype_come_from_the_header():
    from arcflow_amd import _lib
    assert _lib.LoraTerm._fields_ == [('kind', i32), ('rank', i32), ('rank2', i32), ('scale', f32), ('down', vp), ('up', vp), ('down2', vp), ('up2', vp),
                                      ('row_gain', vp), ('w1', vp), ('w2', vp), ('ka', i32), ('kb', i32), ('kc', i32), ('kd', i32), ('row0', i64)]
    assert C.sizeof(_lib.LoraTerm) == 16 + 7 * 8 + 16 + 8                          # no padding: what the C compiler lays out
    assert (_lib.AFX_LORA_TERM_LORA, _lib.AFX_LORA_TERM_LOHA, _lib.AFX_LORA_TERM_LOKR) == (0, 1, 2)
    res, args = _lib.PROTOTYPES['afx_lora_fold_terms']
    assert res is i32 and args == _lib.PROTOTYPES['afx_lora_fold'][1][:7] + [vp, vp]


LORA = dict(kind=0, rank=4, scale=1.0, down=p(MB), up=p(2 * MB), row_gain=p(6 * MB))
LOHA = dict(kind=1, rank=4, rank2=33, scale=0.5, down=p(MB), up=p(2 * MB), down2=p(3 * MB), up2=p(5 * MB))
LOKR = dict(kind=2, scale=-0.3, w1=p(7 * MB), w2=p(8 * MB), ka=3, kb=4, kc=96, kd=64, row0=64)          # 288 virtual rows, 256 columns


def test_fold_terms_abi_guards():
    from arcflow_amd import _lib
    lib = _lib.load()

    def call(base=p(), ldb=256, dst=p(4 * MB), ldd=256, O=128, I=256, J=None, terms=(LORA, LOHA, LOKR), null_terms=False):
        arr = (_lib.LoraTerm * max(len(terms), 1))()
        for c, t in zip(arr, terms):
            for k, v in t.items():
                setattr(c, k, v)
        return lib.afx_lora_fold_terms(vp(base) if base else None, ldb, vp(dst) if dst else None, ldd, O, I, len(terms) if J is None else J,
                                       None if null_terms else C.cast(arr, vp), None)

    def one(term, **kw):
        return dict(terms=(dict(term, **kw),))
    cases = [(dict(base=0), b'null'), (dict(dst=0), b'null'), (dict(null_terms=True), b'null term array'),
             (dict(terms=(LORA,) * 9), b'terms (0 .. 8)'), (dict(J=-1), b'terms (0 .. 8)'),
             (dict(O=96), b'multiples of 64'), (dict(I=96, ldb=96, ldd=96), b'multiples of 64'), (dict(O=0), b'multiples of 64'),
             (dict(ldb=192), b'leading dimension'), (dict(ldd=248), b'leading dimension'),
             (dict(dst=p(64 * 256 * 2)), b'overlaps base'), (dict(dst=p()), b'overlaps base'), (dict(base=p(8)), b'aligned'),
             (dict(dst=p(4 * MB + 8)), b'aligned'), (dict(ldd=260), b'aligned'),
             # the kind
             (one(LORA, kind=3), b'unknown kind'), (one(LORA, kind=-1), b'unknown kind'),
             # a LoRA term
             (one(LORA, down=0), b'null'), (one(LORA, up=0), b'null'), (one(LORA, rank=0), b'rank'), (one(LORA, rank=-2), b'rank'),
             (one(LORA, down=p(MB + 8)), b'16-byte aligned'), (one(LORA, up=p(2 * MB + 1)), b'2-byte aligned'),
             (one(LORA, row_gain=p(6 * MB + 2)), b'4-byte aligned'), (one(LORA, row_gain=p(4 * MB + 64)), b'overlaps the row gains'),
             (one(LORA, row_gain=p(4 * MB - 4)), b'overlaps the row gains'),
             # a LoHa term
             (one(LOHA, down=0), b'null'), (one(LOHA, up=0), b'null'), (one(LOHA, down2=0), b'null'), (one(LOHA, up2=0), b'null'),
             (one(LOHA, rank=0), b'rank'), (one(LOHA, rank2=0), b'rank'), (one(LOHA, rank2=-1), b'rank'),
             (one(LOHA, down2=p(3 * MB + 8)), b'16-byte aligned'), (one(LOHA, up2=p(5 * MB + 1)), b'2-byte aligned'),
             (one(LOHA, row_gain=p(6 * MB)), b'no LoRA term'),
             # a LoKr term
             (one(LOKR, w1=0), b'null'), (one(LOKR, w2=0), b'null'), (one(LOKR, w1=p(7 * MB + 2)), b'4-byte aligned'),
             (one(LOKR, w2=p(8 * MB + 1)), b'4-byte aligned'), (one(LOKR, row_gain=p(6 * MB)), b'no LoRA term'),
             (one(LOKR, ka=0), b'all >= 1'), (one(LOKR, kb=0), b'all >= 1'), (one(LOKR, kc=-96), b'all >= 1'), (one(LOKR, kd=0), b'all >= 1'),
             (one(LOKR, kd=32), b'columns'), (one(LOKR, kb=5), b'columns'),
             (one(LOKR, row0=-64), b'row0'), (one(LOKR, row0=161), b'row0'), (one(LOKR, ka=1), b'row0'),
             (one(LOKR, ka=1 << 30, kc=1 << 30, row0=0), b'row0'),                    # 2^60 virtual rows: past the 32-bit row index
             # a fault in the last of three terms is found too
             (dict(terms=(LORA, LOHA, dict(LOKR, kd=32))), b'term 2')]
    for kw, msg in cases:
        assert call(**kw) == _lib.AFX_E_INVALID, kw
        assert msg in lib.afx_last_error() and b'afx_lora_fold_terms' in lib.afx_last_error(), (kw, lib.afx_last_error())


def test_ops_refuse_before_the_library():
    from arcflow_amd import _lib, ops
    bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)      # noqa: E731
    loha = dict(kind='loha', w1_a=bf(64, 4), w1_b=bf(4, 64), w2_a=bf(64, 2), w2_b=bf(2, 64), scale=1.0)
    with pytest.raises(_lib.ArcflowHipError, match='GPU tensors only'):
        ops.lora_fold_terms(bf(64, 64), bf(64, 64), [loha])
    with pytest.raises(_lib.ArcflowHipError, match='GPU tensors only'):
        ops.lora_fold_terms(bf(64, 64), bf(64, 64), [dict(kind='lokr', w1=torch.zeros(8, 8), w2=torch.zeros(8, 8), scale=1.0)])


def test_ops_refusals_name_the_operand(monkeypatch):
    """Shapes, dtypes and contiguity, with the device check out of the way: the refusals are raised before the library is asked (a call that got
    that far would raise ArcflowHipError for its CPU pointers' sake, or fault)."""
    from arcflow_amd import _lib, ops
    monkeypatch.setattr(ops, '_gpu', lambda *a, **k: None)
    monkeypatch.setattr(_lib, 'load', lambda: None)
    bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)      # noqa: E731
    z = lambda *s: torch.zeros(*s)                             # noqa: E731
    base, dst = bf(128, 256), bf(128, 256)
    lora = dict(kind='lora', A=bf(4, 256), B=bf(128, 4), scale=1.0)
    loha = dict(kind='loha', w1_a=bf(128, 4), w1_b=bf(4, 256), w2_a=bf(128, 2), w2_b=bf(2, 256), scale=1.0)
    lokr = dict(kind='lokr', w1=z(3, 4), w2=z(96, 64), scale=1.0, row0=64)
    for terms, msg in (([dict(lora, A=bf(4, 128))], r'term 0 needs contiguous A \[r, 256\] and B \[128, r\]'),
                       ([dict(lora, B=bf(128, 5))], 'term 0 needs contiguous A'),
                       ([dict(lora, A=z(4, 256))], r'terms\[0\] A: need a 2-D torch.bfloat16'),
                       ([dict(lora, row_gain=z(64))], r'terms\[0\] row_gain'),
                       ([lora, dict(loha, w2_a=bf(128, 3))], r'term 1 needs contiguous w2_b \[r, 256\] and w2_a \[128, r\]'),
                       ([dict(loha, w1_a=bf(4, 128).t())], r'terms\[0\] w1_a: need a 2-D torch.bfloat16 tensor with unit inner stride'),
                       ([dict(loha, w1_a=bf(128, 8)[:, :4])], 'term 0 needs contiguous w1_b'),
                       ([dict(loha, w1_b=z(4, 256))], r'terms\[0\] w1_b: need a 2-D torch.bfloat16'),
                       ([dict(loha, row_gain=z(128))], 'row gains belong to LoRA terms'),
                       ([dict(lokr, row_gain=z(128))], 'row gains belong to LoRA terms'),
                       ([dict(lokr, w1=bf(3, 4))], 'contiguous 2-D float32 w1'),
                       ([dict(lokr, w2=z(64, 96).t())], 'contiguous 2-D float32 w2'),
                       ([dict(lokr, w2=z(96, 32))], r'\[288, 128\]'),
                       ([dict(lokr, row0=192)], 'rows 192 .. 320'),
                       ([dict(lokr, row0=-1)], 'rows -1'),
                       ([dict(kind='locon', scale=1.0)], "kind 'locon'")):
        with pytest.raises(ValueError, match=msg):
            ops.lora_fold_terms(base, dst, terms)
    with pytest.raises(ValueError, match='lora_fold_terms dst'):
        ops.lora_fold_terms(base, bf(128, 128), [])
    with pytest.raises(ValueError, match='lora_fold_terms base'):
        ops.lora_fold_terms(z(128, 256), dst, [])
