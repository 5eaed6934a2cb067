"""CPU-side checks of the C-ABI boundary: the library builds/loads, exports every symbol that
include/arcflow_hip.h declares, validates arguments, and the host logic (schedule, rope tables,
weight packing) agrees with the oracle.  No GPU compute is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from arcflow_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


SYNTHETIC_HEADER = """
/* block comment with a call-like token afx_fake(int x); and a
 * second line: int afx_fake2(void); */
#ifndef SYN_H_
#define SYN_H_
#include <stdint.h>
extern "C" {
#define AFX_OK 0
#define AFX_E_BAD (-7)   /* trailing comment afx_fake( */
#define AFX_WIDE 64      // line comment afx_fake(
typedef struct afx_ctx afx_ctx;
typedef struct afx_pair {
  int32_t first;   /* a field comment */
  int64_t second;
  const float* third;
} afx_pair;
const char* afx_name(void);
// int afx_fake3(int a);
int afx_open(const afx_pair* desc, afx_ctx** out, const char* name);
int64_t afx_bytes(const afx_ctx* ctx, int32_t rows,
                  int64_t ld,   /* stride */
                  uint32_t seed, float p, double q, int n);
int afx_fold(const void* const* A, const float* const scales, const int32_t* ranks, const int64_t n, void* stream);
}
#endif
"""


def test_header_reader_on_synthetic_text():
    """The reader of arcflow_amd/_lib.py on a header written here: comments that look like calls, a prototype over several lines, (void),
    const char* as result and parameter, const-qualified pointers and scalars, a negative macro in parentheses, a struct."""
    from arcflow_amd import _lib
    vp, cp, i32, i64, u32, f32, f64 = C.c_void_p, C.c_char_p, C.c_int32, C.c_int64, C.c_uint32, C.c_float, C.c_double
    assert _lib.parse_prototypes(SYNTHETIC_HEADER) == {
        'afx_name': (cp, []),
        'afx_open': (i32, [vp, vp, cp]),
        'afx_bytes': (i64, [vp, i32, i64, u32, f32, f64, i32]),
        'afx_fold': (i32, [vp, vp, vp, i64, vp]),
    }
    assert list(_lib.parse_prototypes(SYNTHETIC_HEADER)) == ['afx_name', 'afx_open', 'afx_bytes', 'afx_fold']
    assert _lib.parse_struct(SYNTHETIC_HEADER, 'afx_pair') == [('first', i32), ('second', i64), ('third', vp)]
    assert _lib.parse_constants(SYNTHETIC_HEADER) == {'AFX_OK': 0, 'AFX_E_BAD': -7, 'AFX_WIDE': 64}
    # an unknown scalar type names the function it stands in
    for bad in ('int afx_odd(size_t n);', 'int afx_odd(unsigned int n);', 'size_t afx_odd(void);', 'int afx_ok(int a);\nint afx_odd(long n);'):
        with pytest.raises(ValueError, match='afx_o'):
            _lib.parse_prototypes(SYNTHETIC_HEADER + bad)
    # a declaration the pattern cannot take is caught by the count of "afx_*(" tokens, not skipped
    for bad in ('int afx_cb(void (*fn)(int), void* arg);', 'static inline int afx_inl(int a);', 'int afx_nosemi(int a)',
                '#define AFX_CALL(x) afx_name()'):
        with pytest.raises(ValueError, match='tokens'):
            _lib.parse_prototypes(SYNTHETIC_HEADER + bad)
    with pytest.raises(ValueError):
        _lib.parse_struct(SYNTHETIC_HEADER, 'afx_missing')
    with pytest.raises(ValueError, match='afx_pair'):
        _lib.parse_struct(SYNTHETIC_HEADER.replace('int64_t second', 'long second'), 'afx_pair')
    for bad in ('#define AFX_F 1.5', '#define AFX_M(x) 3', '#define AFX_S "s"', '#define AFX_OK 1'):
        with pytest.raises(ValueError):
            _lib.parse_constants(SYNTHETIC_HEADER + bad + '\n')


def _header_names():
    from arcflow_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'arcflow_hip.h')).read()
    names = set(re.findall(r'^(?:int|int64_t|const char\*)\s+(afx_[a-z0-9_]+)\s*\(', hdr, flags=re.M))
    return hdr, names, _lib


def test_header_reader_on_real_header():
    hdr, names, _lib = _header_names()
    protos = _lib.parse_prototypes(hdr)
    assert protos == _lib.PROTOTYPES and set(protos) == names and _lib.EXPORTS == sorted(names)
    assert len(protos) == len(re.findall(r'afx_\w+\s*\(', re.sub(r'/\*.*?\*/|//[^\n]*', ' ', hdr, flags=re.S))) >= 110
    for name, (restype, argtypes) in protos.items():
        assert restype in (C.c_int32, C.c_int64, C.c_char_p), name
        want = C.c_int64 if name.endswith('_ws_bytes') or name == 'afx_workspace_bytes' else \
            C.c_char_p if name in ('afx_last_error', 'afx_version') else C.c_int32
        assert restype is want, name
        assert all(t in (C.c_void_p, C.c_char_p, C.c_int32, C.c_int64, C.c_uint32, C.c_float, C.c_double) for t in argtypes), name
    assert protos['afx_linear_tn_ws_bytes'][0] is C.c_int64 and sum(n.endswith('_ws_bytes') for n in protos) >= 7
    assert protos['afx_bind_weight'] == (C.c_int32, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p])
    assert protos['afx_lora_dropout_bf16'][1][7:9] == [C.c_float, C.c_uint32]
    assert _lib.ModelDesc._fields_ == [(n, C.c_int32) for n in (
        'family', 'num_double', 'num_single', 'heads', 'head_dim', 'in_channels', 'joint_dim', 'pooled_dim', 'guidance_embeds',
        'num_gaussians', 'logweights_channels', 'head_mode')]
    assert C.sizeof(_lib.ModelDesc) == 48
    assert (_lib.AFX_DT_BF16, _lib.AFX_DT_F32, _lib.AFX_DT_FP8, _lib.AFX_BLOCK_DOUBLE, _lib.AFX_BLOCK_SINGLE) == (1, 2, 3, 0, 1)
    assert _lib.AFX_QKV_PATHS == {'auto': 0, 'vt_proj': 1, 'qk_epi': 2, 'kv_prep': 3}
    assert (_lib.AFX_OK, _lib.AFX_E_INVALID, _lib.AFX_E_MISSING, _lib.AFX_E_WORKSPACE, _lib.AFX_E_HIP, _lib.AFX_E_UNSUPPORTED) == (0, -1, -2, -3, -4, -5)
    from arcflow_amd.pipelines import arcflow_loader
    assert arcflow_loader.MAX_FOLD_ADAPTERS == _lib.AFX_LORA_MAX_ADAPTERS == 8


def test_loaded_functions_carry_the_header_types(lib):
    _, _, _lib = _header_names()
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_missing_header_raises_with_its_path(tmp_path):
    """The binding cannot be derived without the header: like a missing library, that is an ArcflowHipError naming the path."""
    _, _, _lib = _header_names()
    gone = str(tmp_path / 'include' / 'arcflow_hip.h')
    with pytest.raises(_lib.ArcflowHipError, match=re.escape(gone)):
        _lib.read_header(gone)
    assert _lib.read_header() == open(os.path.join(ROOT, 'include', 'arcflow_hip.h')).read()


def test_header_symbols_exported(lib):
    hdr, names, _lib = _header_names()
    assert len(names) >= 17
    for n in names:
        assert hasattr(lib, n), f'{n} declared in arcflow_hip.h but not exported'
    # the other direction, from the built library: its unmangled afx_* functions are the header's, plus the undeclared debug hooks
    import shutil
    from arcflow_amd import build
    rocm_bin = os.path.dirname(os.path.realpath(build._hipcc()))
    cands = [os.path.join(rocm_bin, '..', 'llvm', 'bin', 'llvm-nm'), os.path.join(rocm_bin, '..', 'lib', 'llvm', 'bin', 'llvm-nm'),
             shutil.which('llvm-nm'), shutil.which('nm')]
    nm = next((c for c in cands if c and os.path.exists(c)), None)
    if nm is None:
        pytest.skip('no llvm-nm / nm found to list the dynamic symbols of the built library')
    import subprocess
    out = subprocess.run([nm, '-D', '--defined-only', lib._name], capture_output=True, text=True, check=True).stdout
    syms = {f[2] for f in (line.split() for line in out.splitlines()) if len(f) == 3 and f[1] in 'TtWw' and f[2].startswith('afx_')}
    assert {s for s in syms if not s.startswith('afx_debug_')} == names, (sorted(syms - names), sorted(names - syms))


def test_argument_validation_no_gpu(lib):
    from arcflow_amd import _lib
    desc = _lib.ModelDesc(0, 1, 1, 2, 64, 64, 128, 64, 1, 16, 4, 0)      # head_dim != 128
    ctx = C.c_void_p()
    assert lib.afx_create(C.byref(desc), C.byref(ctx)) == -5
    assert b'head_dim' in lib.afx_last_error()
    desc = _lib.ModelDesc(0, 1, 1, 2, 128, 64, 128, 64, 1, 16, 4, 0)
    assert lib.afx_create(C.byref(desc), C.byref(ctx)) == 0
    assert lib.afx_finalize(ctx) == -2                                    # weights missing
    assert b'not bound' in lib.afx_last_error()
    assert lib.afx_workspace_bytes(ctx, 1, 64, 16) > 0
    assert lib.afx_workspace_bytes(ctx, 0, 64, 16) == -1
    assert lib.afx_mmdit_forward(ctx, None, None, None, None, None, None, None, 1, 4, 4, None, None, None, None) == -1
    assert lib.afx_linear_bf16(None, 8, None, 8, None, None, 8, 1, 8, 64, 0, 0, None, 0, 1, None, 0, None) == -1
    assert lib.afx_arcflow_step(None, None, None, None, 1, 1.0, 1.0, 0.5, None, 1e-4, None, 1, 1, 16, 64, 4, None) == -1
    # round-5 entry points: nulls, misaligned / non-multiple-of-8 widths are refused before any launch
    assert lib.afx_linear_tn_f32out(None, 8, None, 8, None, 8, 64, 8, 8, 0, None) == -1
    assert lib.afx_linear_tn_f32out(C.c_void_p(4096), 8, C.c_void_p(8192), 8, C.c_void_p(16384), 8, 64, 12, 8, 0, None) == -1      # N1 % 8
    assert lib.afx_linear_tn_f32out(C.c_void_p(4096 + 2), 8, C.c_void_p(8192), 8, C.c_void_p(16384), 8, 64, 8, 8, 0, None) == -1   # 16-byte alignment
    assert b'afx_linear_tn_f32out' in lib.afx_last_error()
    assert lib.afx_linear_bf16_dropres(None, 64, None, 64, None, 8, 1, 8, 64, None, 8, 0.05, 1, 0, None) == -1
    assert lib.afx_linear_bf16_dropres(C.c_void_p(4096), 64, C.c_void_p(8192), 64, C.c_void_p(16384), 8, 1, 8, 64, C.c_void_p(16384), 8, 1.5, 1, 0, None) == -1   # p >= 1
    assert lib.afx_normout_backward_split(None, 8, None, 8, None, None, 1, 8, None) == -1
    # round-6: the token-split TN product: workspace sizes are a host-side function of the shape; the _ws entry refuses a missing / misaligned workspace before any launch
    if os.environ.get('AFX_TN_SPLIT') is None:
        assert lib.afx_linear_tn_ws_bytes(4608, 3072, 256) == 9 * 3072 * 256 * 4          # 48 tiles -> 9 runs of 8 K-steps
        assert lib.afx_linear_tn_ws_bytes(4608, 12288, 256) == 2 * 12288 * 256 * 4
        assert lib.afx_linear_tn_ws_bytes(130, 64, 192) == 0 and lib.afx_linear_tn_ws_bytes(1, 8, 8) == 0
        assert lib.afx_linear_tn_f32out_ws(C.c_void_p(4096), 3072, C.c_void_p(8192), 256, C.c_void_p(16384), 256, 4608, 3072, 256, 0, None, None) == -1     # needs a workspace
        assert b'workspace' in lib.afx_last_error()
    assert lib.afx_linear_tn_ws_bytes(-1, 8, 8) == -1
    assert lib.afx_linear_tn_f32out_ws(None, 8, None, 8, None, 8, 64, 8, 8, 0, None, None) == -1
    assert lib.afx_linear_tn_f32out_ws(C.c_void_p(4096), 8, C.c_void_p(8192), 8, C.c_void_p(16384), 8, 64, 8, 8, 0, C.c_void_p(4096 + 4), None) == -1   # misaligned workspace
    # round-6: the capability query behind ops.linear_dropres' fallback follows the kernel choice (host-side state only)
    if os.environ.get('AFX_GEMM_IMPL', '3') == '3':
        assert lib.afx_gemm_dropres_available() == 1
        assert lib.afx_gemm_set_mode(2, 0) == 0 and lib.afx_gemm_dropres_available() == 0
        assert lib.afx_gemm_set_mode(3, 0) == 0 and lib.afx_gemm_dropres_available() == 1
        assert lib.afx_gemm_set_mode(1, 0) == 0 and lib.afx_gemm_dropres_available() == 1      # no kernel 1 any more: the default stays in force
        assert lib.afx_gemm_set_mode(3, 0) == 0
    assert lib.afx_destroy(ctx) == 0


def test_head_width_query(lib):
    """afx_head_width: K C + K L + (K - 1) L rounded up to 8 -- the N of the head GEMM (host-side, no GPU needed)."""
    from arcflow_amd import _lib
    desc = _lib.ModelDesc(0, 1, 1, 2, 128, 64, 128, 64, 1, 16, 4, 0)
    ctx = C.c_void_p()
    assert lib.afx_create(C.byref(desc), C.byref(ctx)) == 0
    try:
        assert lib.afx_head_width(ctx) == (16 * 64 + 16 * 4 + 15 * 4 + 7) // 8 * 8 == 1152
    finally:
        assert lib.afx_destroy(ctx) == 0
    desc = _lib.ModelDesc(0, 1, 1, 2, 128, 128, 128, 64, 1, 5, 3, 0)
    assert lib.afx_create(C.byref(desc), C.byref(ctx)) == 0
    try:
        assert lib.afx_head_width(ctx) == (5 * 128 + 5 * 3 + 4 * 3 + 7) // 8 * 8 == 672
    finally:
        assert lib.afx_destroy(ctx) == 0
    assert lib.afx_head_width(None) == -1


def test_fp8_tile_setter_clamps_to_per_launch_choice(lib):
    """afx_gemm_set_fp8_tile: 0 / 1 / 2 are taken as given, any other value selects 0 (picked per launch); host-side state only."""
    from arcflow_amd import ops
    try:
        for want, got in ((1, 1), (2, 2), (0, 0), (3, 0), (-1, 0), (2, 2), (7, 0), (1 << 20, 0)):
            assert lib.afx_gemm_set_fp8_tile(want) == got, want
        assert ops.set_fp8_tile(2) == 2 and ops.set_fp8_tile(5) == 0
    finally:
        lib.afx_gemm_set_fp8_tile(0)


def test_forward_operand_entry_points_validate_before_launch(lib):
    """afx_qkv_operands / afx_norm_modulate_joint_bf16 / afx_norm_modulate_mx8 refuse bad arguments with AFX_E_INVALID before anything
    touches the device (fake but aligned pointers: a launch would fault)."""
    p = lambda off=0: C.c_void_p(1 << 20 | off)         # noqa: E731
    D, H = 3072, 24
    qkv = lib.afx_qkv_operands
    ok = dict(A=p(), lda=D, wi=p(), bi=p(), wt=p(), bt=p(), qkn=p(), cos=p(), sin=p(), B=1, N=4096, T=512, H=H, path=0, F=p(), ldf=3 * D, Vt=p())

    def call(kind=0, **kw):
        a = dict(ok, **kw)
        return qkv(kind, a['A'], a['lda'], a['wi'], a['bi'], a['wt'], a['bt'], a['qkn'], a['cos'], a['sin'], a['B'], a['N'], a['T'], a['H'],
                   a['path'], a['F'], a['ldf'], a['Vt'], None)
    assert call(kind=2) == -1 and b'kind' in lib.afx_last_error()
    assert call(A=None) == -1 and b'null' in lib.afx_last_error()
    assert call(wt=None) == -1                                            # a double block needs the text weights
    assert call(bt=None) == -1                                            # ... and a bias for both streams or neither
    assert call(B=5) == -1 and call(B=0) == -1 and call(T=0) == -1 and call(path=4) == -1 and call(path=-1) == -1
    assert call(lda=D - 8) == -1 and call(ldf=3 * D - 8) == -1 and call(ldf=3 * D + 4) == -1
    assert call(kind=1, ldf=3 * D) == -1 and b'ldf' in lib.afx_last_error()       # a single block writes 7D columns
    assert call(A=p(8)) == -1 and call(Vt=p(2)) == -1 and call(qkn=p(4)) == -1 and b'aligned' in lib.afx_last_error()
    if os.environ.get('AFX_GEMM_IMPL', '3') == '3' and os.environ.get('AFX_QK_FUSE') is None:
        assert call(path=1, T=77) == -1 and b'% 16' in lib.afx_last_error()      # V^T from the projection: 16-key groups, no key padding
        assert call(path=1, N=4100, T=496) == -1                                  # S % 64 != 0
        assert lib.afx_gemm_set_mode(2, 0) == 0
        try:
            for path in (1, 2):
                assert call(path=path) == -1 and b'q / k epilogue' in lib.afx_last_error()
        finally:
            assert lib.afx_gemm_set_mode(3, 0) == 0
    # the AdaLN entry points
    nmj = lib.afx_norm_modulate_joint_bf16
    assert nmj(None, D, p(), D, 4608, D, p(), p(), p(), p(), 98304, 4608, 512, None) == -1
    assert nmj(p(), D, p(), D, 4608, D, p(), p(), p(), None, 98304, 4608, 512, None) == -1            # shift_txt missing
    assert nmj(p(), D, p(), D, 4608, D, p(), p(), None, None, 98304, 4608, 512, None) == -1            # n_txt without text vectors
    assert nmj(p(), D, p(), D, 4608, D, p(), p(), p(), p(), 98304, 4608, 4609, None) == -1             # n_txt > S
    assert nmj(p(), D, p(), D, 4608, D + 4, p(), p(), p(), p(), 98304, 4608, 512, None) == -1          # D % 8
    assert nmj(p(), D - 8, p(), D, 4608, D, p(), p(), p(), p(), 98304, 4608, 512, None) == -1          # ldx < D
    assert nmj(p(), D, p(), D, 4608, D, p(), p(), p(), p(), 98306, 4608, 512, None) == -1              # ldmod % 4
    assert nmj(p(), D, p(8), D, 4608, D, p(), p(), p(), p(), 98304, 4608, 512, None) == -1             # out misaligned
    assert b'afx_norm_modulate_joint_bf16' in lib.afx_last_error()
    mx8 = lib.afx_norm_modulate_mx8
    fused = C.c_int32(7)
    assert mx8(p(), D, p(), D, p(), 24, None, 4608, D, p(), p(), p(), p(), 98304, 4608, 512, None, None) == -1     # no fused flag
    assert mx8(p(), D, p(), D, None, 24, None, 4608, D, p(), p(), p(), p(), 98304, 4608, 512, C.byref(fused), None) == -1   # no scales
    assert mx8(p(), D, p(), D, p(), 20, None, 4608, D, p(), p(), p(), p(), 98304, 4608, 512, C.byref(fused), None) == -1   # ld_mx < D / 128
    assert mx8(p(), D, p(), D, p(), 26, None, 4608, D, p(), p(), p(), p(), 98304, 4608, 512, C.byref(fused), None) == -1   # ld_mx % 4
    assert mx8(p(), D, p(4), D, p(), 24, None, 4608, D, p(), p(), p(), p(), 98304, 4608, 512, C.byref(fused), None) == -1  # q8 alignment
    assert mx8(p(), D, p(), D, None, 0, p(2), 4608, D, p(), p(), p(), p(), 98304, 4608, 512, C.byref(fused), None) == -1   # rowscale alignment
    assert fused.value == 7 and b'afx_norm_modulate_mx8' in lib.afx_last_error()


def test_linear_entry_points_refuse_by_their_own_name(lib):
    """Each afx_linear_* GEMM entry and both afx_linear_tn_f32out* refuse a null operand, a K one element off its multiple (64 bf16, 128 fp8,
    512 block-scaled; the TN product has no K rule: its width N1, a multiple of 8, stands in) and a leading dimension one element off its
    multiple with AFX_E_INVALID, and afx_last_error() names the entry that was called.  Every call carries exactly one defect and fake but
    aligned pointers: validation returns before any launch."""
    from arcflow_amd import _lib
    p = lambda: C.c_void_p(1 << 20)         # noqa: E731
    M, N = 264, 136
    entries = {      # name -> (K, call(A, K, lda)); ldw stays at the good K
        'afx_linear_bf16': (128, lambda A, K, lda: lib.afx_linear_bf16(A, lda, p(), 128, p(), p(), N, M, N, K, 0, 0, None, 0, 1, None, 0, None)),
        'afx_linear_bf16_pre': (128, lambda A, K, lda: lib.afx_linear_bf16_pre(A, lda, p(), 128, p(), p(), N, M, N, K, 0, 0, None, 0, 1, None, 0,
                                                                                  p(), N, None)),
        'afx_linear_bf16_f32out': (128, lambda A, K, lda: lib.afx_linear_bf16_f32out(A, lda, p(), 128, p(), N, M, N, K, 0, None)),
        'afx_linear_bf16_splitk': (128, lambda A, K, lda: lib.afx_linear_bf16_splitk(A, lda, p(), 128, p(), p(), M, N, K, 0, None)),
        'afx_linear_bf16_dropres': (128, lambda A, K, lda: lib.afx_linear_bf16_dropres(A, lda, p(), 128, p(), N, M, N, K, p(), N, 0.05, 1, 0, None)),
        'afx_linear_fp8': (128, lambda A, K, lda: lib.afx_linear_fp8(A, lda, p(), p(), 128, p(), p(), p(), N, M, N, K, 0, 0, None, 0, 1, None, 0,
                                                                        None)),
        'afx_linear_fp8_mx': (512, lambda A, K, lda: lib.afx_linear_fp8_mx(A, lda, p(), 4, p(), p(), 512, p(), p(), p(), N, M, N, K, 0, 0, None, 0, 1,
                                                                              None, 0, None)),
        'afx_linear_fp8_to_mx8': (512, lambda A, K, lda: lib.afx_linear_fp8_to_mx8(A, lda, p(), 4, p(), p(), 512, p(), p(), p(), N, p(), N, p(), 4, 0,
                                                                                      M, N, K, 0, None)),
        'afx_linear_tn_f32out': (128, lambda X, N1, ldx: lib.afx_linear_tn_f32out(X, ldx, p(), N, p(), N, M, N1, N, 0, None)),
        'afx_linear_tn_f32out_ws': (128, lambda X, N1, ldx: lib.afx_linear_tn_f32out_ws(X, ldx, p(), N, p(), N, M, N1, N, 0, None, None)),
    }
    assert set(entries) == {n for n in _lib.PROTOTYPES if n.startswith('afx_linear_') and not n.endswith(('_ws_bytes', '_chunks'))}
    for name, (K, call) in entries.items():
        for defect, args in (('null operand', (None, K, K)), ('K + 1', (p(), K + 1, K + 8 if '_tn_' in name else K)), ('lda + 1', (p(), K, K + 1))):
            assert call(*args) == _lib.AFX_E_INVALID, (name, defect)
            assert name.encode() in lib.afx_last_error() and (name + '_').encode() not in lib.afx_last_error(), (name, defect, lib.afx_last_error())


def test_schedule_matches_oracle_and_golden(golden):
    from arcflow_amd.schedule import FlowMatchEulerDiscreteScheduler, retrieve_raw_timesteps
    from oracle import arcflow_ref as R
    g = golden('g1_time_grid')
    for nfe, ratio in [(2, 1.0), (4, 1.0), (4, 0.5), (1, 1.0), (3, 0.25), (8, 1.0)]:
        tag = f'n{nfe}_r{str(ratio).replace(".", "p")}'
        raw, counts, total = retrieve_raw_timesteps(nfe, 128, ratio)
        assert np.array_equal(np.asarray(raw), g[tag + '_raw'])
        assert counts == g[tag + '_counts'].tolist() and total == int(g[tag + '_total'])
    sch = FlowMatchEulerDiscreteScheduler.from_config(dict(num_train_timesteps=1000, use_dynamic_shifting=True),
                                                      shift=3.2, shift_terminal=None, use_dynamic_shifting=False)
    raw, counts, total = retrieve_raw_timesteps(2, 128, 1.0)
    ts = sch.set_timesteps(sigmas=raw, mu=1.15)
    assert len(ts) == 128
    sig, _ = R.inference_sigmas(2)
    assert abs(float(ts[0]) / 1000 - sig[0]) < 1e-7 and abs(float(ts[64]) / 1000 - sig[1]) < 1e-6


def test_rope_tables_match_oracle():
    from arcflow_amd import rope
    from oracle import dit_ref as D
    c, s = rope.flux_tables(5, 7, 9)
    oc, os_ = D.flux_rope_tables(5, 7, 9)
    assert torch.equal(c, oc) and torch.equal(s, os_)
    c, s = rope.qwen_tables(6, 4, 5)
    ia, ta = D.qwen_rope_angles(6, 4, 5)
    assert torch.allclose(c, torch.cat([torch.cos(ta), torch.cos(ia)]), atol=1e-6)


def test_weight_packing_and_lora_merge():
    from arcflow_amd.weights import merge_lora, pack_flux
    from oracle import dit_ref as D
    cfg = D.FluxCfg(num_layers=1, num_single_layers=1, heads=2, joint_dim=128, pooled_dim=64)
    w = D.make_flux_weights(cfg, 0)
    p = pack_flux(w, 1, 1, 'cpu')
    Dm = 256
    assert p['d0.img_qkv.weight'].shape == (3 * Dm, Dm)
    assert torch.equal(p['d0.img_qkv.weight'][2 * Dm:], w['transformer_blocks.0.attn.to_q.weight'])
    assert torch.equal(p['s0.fused.weight'][:Dm], w['single_transformer_blocks.0.attn.to_k.weight'])
    assert torch.equal(p['s0.fused.weight'][3 * Dm:], w['single_transformer_blocks.0.proj_mlp.weight'])
    assert p['mod.weight'].shape == (12 * Dm + 3 * Dm + 2 * Dm, Dm)
    assert p['head.weight'].shape == (1152, Dm) and p['head.weight'][1148:].abs().sum() == 0
    g = torch.Generator().manual_seed(0)
    a = torch.randn(8, Dm, generator=g).bfloat16()
    b = torch.randn(4 * Dm, 8, generator=g).bfloat16()
    name = 'transformer_blocks.0.ff.net.0.proj'
    merged = merge_lora(w, {name + '.lora_A.weight': a, name + '.lora_B.weight': b})
    ref = (w[name + '.weight'].float() + b.float() @ a.float()).bfloat16()
    assert torch.equal(merged[name + '.weight'], ref)
    assert merged['x_embedder.weight'] is w['x_embedder.weight']


def test_phase_weights_reproduce_conv_of_nearest_upsample():
    """arcflow_amd.vae.phase_weights (host logic of afx_upconv3x3_bf16): conv3x3(nearest-2x upsample(x)) == the four 2x2 phase convolutions on
    the low-resolution input, interleaved -- in fp32 torch on the CPU (the kernel side is tests/test_vae.py::test_upsample_folded_into_conv_vs_torch)."""
    import torch
    from arcflow_amd.vae import phase_weights
    g = torch.Generator().manual_seed(0)
    co, ci, H, W = 8, 64, 5, 6
    wt = (torch.randn(co, ci, 3, 3, generator=g) * 0.1).bfloat16()
    x = torch.randn(1, ci, H, W, generator=g)
    w9 = wt.permute(0, 2, 3, 1).reshape(co, 9 * ci).contiguous()
    w4 = phase_weights(w9, ci).float().reshape(4, co, 2, 2, ci)
    ref = torch.nn.functional.conv2d(torch.nn.functional.interpolate(x, scale_factor=2, mode='nearest'), wt.float(), padding=1)[0]
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1))[0]                          # zero border, like the padded grid
    out = torch.zeros(co, 2 * H, 2 * W)
    for py in (0, 1):
        for px in (0, 1):
            k = w4[2 * py + px].permute(0, 3, 1, 2)                           # [co, ci, 2, 2]
            # source rows {y - 1 + py, y + py} -> padded rows {y + py, y + py + 1}
            ph = torch.nn.functional.conv2d(xp[None, :, py:py + H + 1, px:px + W + 1], k)[0]
            out[:, py::2, px::2] = ph
    # the phase kernels are sums of bf16 taps rounded once more to bf16
    assert ((out - ref).norm() / ref.norm()).item() < 5e-3
