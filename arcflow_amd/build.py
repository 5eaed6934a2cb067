"""Build libarcflow_hip.so (the C-ABI engine, include/arcflow_hip.h) for gfx950 with hipcc.

In-tree build: the shared object lands in arcflow_amd/lib/ so that it travels with the source
snapshot to the GPU box.  hipcc cross-compiles without a GPU.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

from .isa_audit import RULES, audit

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIBDIR = os.path.join(HERE, 'lib')
LIBNAME = 'libarcflow_hip.so'
SOURCES = ['afx_gemm.hip', 'afx_attn.hip', 'afx_attn3.hip', 'afx_attn_bwd.hip', 'afx_attn_bwd3.hip', 'afx_elementwise.hip', 'afx_policy.hip', 'afx_train.hip', 'afx_sampler.hip', 'afx_score.hip', 'afx_edit.hip', 'afx_image.hip', 'afx_color.hip', 'afx_vae.hip', 'afx_text.hip', 'afx_tn.hip', 'afx_lora.hip', 'afx_ops_api.hip', 'afx_engine.hip']
HEADERS = ['afx_common.h', 'afx_kernels.h', 'afx_gemm_plan.h', 'afx_gemm_problem.h', 'afx_api_util.h', 'afx_reduce.h', 'afx_attn_bwd3_kernel.inc', os.path.join('..', '..', 'include', 'arcflow_hip.h')]
HEADERS += [os.path.join('gen', f) for f in sorted(os.listdir(os.path.join(CSRC, 'gen'))) if f.endswith('.inc')]


def lib_path() -> str:
    return os.path.join(LIBDIR, LIBNAME)


def _hipcc() -> str:
    for cand in (os.environ.get('HIPCC'), shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError('hipcc not found (set HIPCC or install ROCm under /opt/rocm)')


def needs_build() -> bool:
    out = lib_path()
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS]
    return any(os.path.getmtime(d) > t for d in deps)


def _obj(objdir: str, src: str) -> str:
    return os.path.join(objdir, src.replace('.hip', '.o'))


def _compile(hipcc: str, flags, src: str, objdir: str, keep_asm: bool = False, check_scratch: bool = True, verbose: bool = False):
    """Start hipcc on one source.  Returns finish(): it waits for hipcc and, where the source has rules in isa_audit.RULES, audits the saved ISA."""
    obj = _obj(objdir, src)
    cmd = [hipcc, *flags, '-c', os.path.join(CSRC, src), '-o', obj]
    if keep_asm or src in RULES:
        cmd.append('-save-temps=obj')       # keeps the .s next to the object
    if src in RULES and '-Wno-inline-asm' not in flags:
        cmd.append('-Wno-inline-asm')
    if verbose:
        print('[arcflow_amd.build]', ' '.join(cmd), flush=True)
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)

    def finish() -> None:
        log, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f'hipcc failed on {src} ({objdir}):\n{log}')
        if verbose and log.strip():
            print(log)
        if src in RULES:
            audit(obj[:-len('.o')] + '-hip-amdgcn-amd-amdhsa-gfx950.s', RULES[src], check_scratch)
    return finish


def _link(hipcc: str, objs, out: str, verbose: bool = False) -> str:
    cmd = [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', *objs, '-o', out]
    if verbose:
        print('[arcflow_amd.build]', ' '.join(cmd), flush=True)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f'link failed:\n{r.stdout}')
    return out


def build(force: bool = False, verbose: bool = True) -> str:
    """Compile every HIP source for gfx950 and link the shared library.  Returns its path."""
    out = lib_path()
    if not force and not needs_build():
        return out
    objdir = os.path.join(LIBDIR, 'obj')
    os.makedirs(objdir, exist_ok=True)
    hipcc = _hipcc()
    flags = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wall', '-Wno-unused-function']
    flags += os.environ.get('AFX_EXTRA_FLAGS', '').split()          # e.g. -DAFX_ATTN_TRACE for tools/attn_trace.py
    for finish in [_compile(hipcc, flags, src, objdir, verbose=verbose) for src in SOURCES]:       # all sources compile in parallel
        finish()
    return _link(hipcc, [_obj(objdir, src) for src in SOURCES], out, verbose)


def build_variant(name: str, extra_flags, sources) -> str:
    """lib/libarcflow_hip_<name>.so = the standard objects with `sources` recompiled under `extra_flags` (trace / A-B builds that
    travel next to the product library; select with ARCFLOW_HIP_LIB=<path>)."""
    build(verbose=False)
    vdir = os.path.join(LIBDIR, 'obj_' + name)
    os.makedirs(vdir, exist_ok=True)
    hipcc = _hipcc()
    flags = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-function', '-Wno-inline-asm', *extra_flags]
    objs = []
    for src in SOURCES:
        if src in sources:
            # check_scratch=False: trace builds add live values and are never the product, so the zero-scratch rule is not asked of them
            _compile(hipcc, flags, src, vdir, keep_asm=True, check_scratch=False)()
        objs.append(_obj(vdir if src in sources else os.path.join(LIBDIR, 'obj'), src))
    return _link(hipcc, objs, os.path.join(LIBDIR, f'libarcflow_hip_{name}.so'))


if __name__ == '__main__':
    if '--variant' in sys.argv:         # python -m arcflow_amd.build --variant trace -DAFX_ATTN_TRACE -- afx_attn3.hip
        i = sys.argv.index('--variant')
        j = sys.argv.index('--')
        print(build_variant(sys.argv[i + 1], sys.argv[i + 2:j], sys.argv[j + 1:]))
    else:
        print(build(force='--force' in sys.argv))
