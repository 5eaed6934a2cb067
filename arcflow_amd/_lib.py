"""ctypes binding of libarcflow_hip.so, derived from include/arcflow_hip.h.

The header is the one written copy of the C ABI: the prototypes, ``afx_model_desc`` and the ``AFX_*`` constants below are read from its
text, so a function declared there is callable from Python with no edit here.  The reader takes the header's regular subset of C and
raises on anything else.

The product path has NO CPU fallback: if the shared library is missing or a call fails this
module raises.  Build it with ``python -m arcflow_amd.build`` (or ``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Dict, List, Optional, Tuple

from .build import HERE, lib_path

HEADER = os.path.join(HERE, '..', 'include', 'arcflow_hip.h')
_SCALARS = {'int': C.c_int32, 'int32_t': C.c_int32, 'int64_t': C.c_int64, 'uint32_t': C.c_uint32, 'float': C.c_float, 'double': C.c_double}


class ArcflowHipError(RuntimeError):
    pass


def _code(text: str) -> str:
    return re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)


def _ctype(decl: str, where: str, named: bool = True):
    """ctypes type of one parameter, field (``named``) or result: ``const char*`` -> c_char_p, any other pointer -> c_void_p, else a scalar."""
    words = decl.replace('*', ' * ').split()
    if '*' in words:
        return C.c_char_p if words[:words.index('*')] == ['const', 'char'] else C.c_void_p
    words = [w for w in words if w != 'const']
    if len(words) != 1 + named or words[0] not in _SCALARS:
        raise ValueError(f'{where}: cannot read the type of "{decl.strip()}"')
    return _SCALARS[words[0]]


def parse_prototypes(text: str) -> Dict[str, Tuple[type, List[type]]]:
    """name -> (restype, [argtypes]) of every ``afx_*`` function the header text declares."""
    code = _code(text)
    tokens = len(re.findall(r'afx_\w+\s*\(', code))
    code = re.sub(r'^[ \t]*#.*$', '', code, flags=re.M)           # the preprocessor lines hold no prototype
    protos = {}
    for res, name, params in re.findall(r'(?:^|[;{}])\s*((?:const\s+)?\w+\s*\*?)\s*\b(afx_\w+)\s*\(([^()]*)\)\s*(?=;)', code):
        args = [] if params.strip() == 'void' else [_ctype(p, name) for p in params.split(',')]
        protos[name] = (_ctype(res, name, named=False), args)
    if len(protos) != tokens:
        raise ValueError(f'read {len(protos)} prototypes, but the text has {tokens} "afx_*(" tokens')
    return protos


def parse_struct(text: str, name: str) -> List[Tuple[str, type]]:
    """The (field, type) list of ``typedef struct name { ... } name;`` in declaration order."""
    body = re.search(r'typedef\s+struct\s+%s\s*\{([^{}]*)\}\s*%s\s*;' % (name, name), _code(text))
    if body is None:
        raise ValueError(f'no typedef struct {name}')
    fields = [f for f in body.group(1).split(';') if f.strip()]
    return [(f.split()[-1], _ctype(f, name)) for f in fields]


def parse_constants(text: str) -> Dict[str, int]:
    """Every ``#define AFX_NAME <integer or (negative integer)>``."""
    code = _code(text)
    consts = {n: int(v.strip('()')) for n, v in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(AFX_\w+)[ \t]+(-?\d+|\(-?\d+\))[ \t]*$', code, flags=re.M)}
    if len(consts) != len(re.findall(r'#[ \t]*define[ \t]+AFX_', code)):
        raise ValueError('an AFX_* macro is not a plain integer (or is defined twice)')
    return consts


def read_header(path: str = HEADER) -> str:
    if not os.path.exists(path):
        raise ArcflowHipError(f'{path} not found: the ctypes binding of the HIP engine is derived from this header.')
    with open(path) as f:
        return f.read()


_text = read_header()
PROTOTYPES = parse_prototypes(_text)
CONSTANTS = parse_constants(_text)
EXPORTS = sorted(PROTOTYPES)
globals().update(CONSTANTS)           # AFX_DT_*, AFX_BLOCK_*, AFX_E_*, AFX_LORA_MAX_ADAPTERS, ... under the header's names
AFX_QKV_PATHS = {n[len('AFX_QKV_'):].lower(): v for n, v in CONSTANTS.items() if n.startswith('AFX_QKV_')}


class ModelDesc(C.Structure):
    _fields_ = parse_struct(_text, 'afx_model_desc')


class LoraTerm(C.Structure):
    _fields_ = parse_struct(_text, 'afx_lora_term')


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """dlopen the engine; raises ArcflowHipError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get('ARCFLOW_HIP_LIB', lib_path())
    if not os.path.exists(path):
        raise ArcflowHipError(
            f'{path} not found: the HIP engine is not built. Run `python -m arcflow_amd.build` '
            '(needs hipcc, cross-compiles for gfx950 without a GPU). There is no CPU fallback.')
    lib = C.CDLL(path)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        raise ArcflowHipError(f'libarcflow_hip error {rc}: {load().afx_last_error().decode()}')
