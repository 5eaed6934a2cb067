#!/usr/bin/env python3
"""Time ``afx_lora_fold`` (the device fold behind ``load_lora_weights`` / ``set_adapters``) on synthetic weights -- no snapshot needed.

    python tools/lora_fold_bench.py [--double 19 --single 38] [--reps 3] [--iters 20] [--skip-parent]
    python tools/lora_fold_bench.py --lycoris [--parent-lib libarcflow_hip.so of the parent commit]

Prints
  * per FLUX matrix shape: the kernel's time (device events around --iters launches, after a warm-up) and GB/s over the 4 * O * I bytes it
    has to move (2 B read + 2 B written per element; the A / B panels are not counted), with one r = 256 and one r = 16 adapter;
  * the whole-model time of ONE weight change with an ArcFlow-sized adapter (r = 256) plus one style adapter (r = 16) on every attention
    and MLP linear of the FLUX trunk, every linear with its own base and live buffers (no reuse: a re-used 18 MB matrix would sit in the
    Infinity Cache);
  * beside it, interleaved on the same box, the path a scale change of the ArcFlow adapter alone takes without style LoRAs:
    ``weights.merge_lora`` + ``MMDiTEngine.load_state_dict``.  Here its state dict is already device-resident, so the 24 GB host-to-device
    upload the pipelines pay on that path (their base state dict lives on the host) is NOT in the number: it is a lower bound.
One JSON line at the end.  Nothing is asserted; there is no fallback without a GPU."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D = 3072
SHAPES = [('attn to_q/k/v/out', D, D), ('mlp up (ff.net.0 / proj_mlp)', 4 * D, D), ('mlp down (ff.net.2)', D, 4 * D),
          ('single proj_out', D, 5 * D), ('norm1.linear', 6 * D, D), ('norm.linear', 3 * D, D)]
RANKS = (256, 16)


def trunk_linears(n_double, n_single):
    """(module, O, I) of every attention / MLP linear of the FLUX trunk: what the released ArcFlow adapter adapts."""
    out = []
    for i in range(n_double):
        p = f'transformer_blocks.{i}.'
        out += [(p + 'attn.' + n, D, D) for n in ('to_q', 'to_k', 'to_v', 'add_q_proj', 'add_k_proj', 'add_v_proj', 'to_out.0', 'to_add_out')]
        for ff in ('ff', 'ff_context'):
            out += [(p + ff + '.net.0.proj', 4 * D, D), (p + ff + '.net.2', D, 4 * D)]
    for i in range(n_single):
        p = f'single_transformer_blocks.{i}.'
        out += [(p + 'attn.' + n, D, D) for n in ('to_q', 'to_k', 'to_v')] + [(p + 'proj_mlp', 4 * D, D), (p + 'proj_out', D, 5 * D)]
    return out


def main(argv=None):
    import torch
    from arcflow_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument('--double', type=int, default=19)
    ap.add_argument('--single', type=int, default=38)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--skip-parent', action='store_true')
    ap.add_argument('--dora', action='store_true', help='time afx_lora_row_gain and afx_lora_fold_rows per FLUX shape against the torch formulation, and stop')
    ap.add_argument('--lycoris', action='store_true', help='time afx_lora_fold_terms with a LoHa, a LoKr and a mixed term list per FLUX shape against '
                    'the torch formulation and the plain LoRA fold, and stop')
    ap.add_argument('--parent-lib', help='--lycoris: a libarcflow_hip.so built from the parent commit; its afx_lora_fold is timed beside this build\'s')
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('lora_fold_bench needs the GPU: a CPU run measures nothing')
    dev = 'cuda'
    g = torch.Generator(device=dev).manual_seed(0)

    def rnd(*shape, std=0.02):
        return (torch.randn(*shape, generator=g, device=dev) * std).to(torch.bfloat16)

    def adapters(O, I):
        return [rnd(r, I, std=0.05) for r in RANKS], [rnd(O, r, std=0.05) for r in RANKS]
    res = dict(device=torch.cuda.get_device_name(0), ranks=list(RANKS), shapes=[], double=a.double, single=a.single)
    if a.dora:
        return dora(a, ops, rnd, res)
    if a.lycoris:
        return lycoris(a, ops, rnd, res)
    # ---- per shape
    for name, O, I in SHAPES:
        base, dst = rnd(O, I), torch.empty(O, I, dtype=torch.bfloat16, device=dev)
        A, B = adapters(O, I)
        for _ in range(3):
            ops.lora_fold(base, dst, A, B, (1.0, 0.8))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            ops.lora_fold(base, dst, A, B, (1.0, 0.8))
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.iters
        gbs = 4.0 * O * I / (ms * 1e-3) / 1e9
        res['shapes'].append(dict(name=name, O=O, I=I, ms=ms, gb_per_s=gbs))
        print(f'{name:32s} [{O:6d}, {I:6d}]  {ms * 1e3:9.1f} us  {gbs:8.1f} GB/s over 4 O I bytes (matrix re-used: {4 * O * I / 2 ** 20:.0f} MiB)')
        del base, dst
    # ---- whole model: one weight change, r = 256 + r = 16 on every trunk linear
    lin = trunk_linears(a.double, a.single)
    bufs = [(rnd(O, I), torch.empty(O, I, dtype=torch.bfloat16, device=dev), *adapters(O, I)) for _, O, I in lin]
    total_bytes = sum(4.0 * O * I for _, O, I in lin)

    def new_path(s):
        t0 = time.perf_counter()
        for base, dst, A, B in bufs:
            ops.lora_fold(base, dst, A, B, (s, 0.8))
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    new_path(1.0)                                              # warm-up
    sd = lora = eng = None
    if not a.skip_parent:
        from arcflow_amd import MMDiTEngine
        from arcflow_amd.weights import expected_transformer_keys, merge_lora
        cfg = dict(num_layers=a.double, num_single_layers=a.single)
        sd = {k: rnd(*s) for k, s in expected_transformer_keys('flux', cfg, True).items()}
        lora = {}
        for m, O, I in lin:
            lora[m + '.lora_A.weight'], lora[m + '.lora_B.weight'] = rnd(RANKS[0], I, std=0.05), rnd(O, RANKS[0], std=0.05)
        eng = MMDiTEngine('flux', a.double, a.single)

        def parent_path(s):
            t0 = time.perf_counter()
            eng.load_state_dict(merge_lora(sd, lora, scale=s))
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        parent_path(1.0)                                       # warm-up
    new_s, par_s = [], []
    for k in range(a.reps):                                    # interleaved: other work shares the box
        new_s.append(new_path(0.9 - 0.1 * k))
        if not a.skip_parent:
            par_s.append(parent_path(0.9 - 0.1 * k))
    res.update(linears=len(lin), fold_bytes=total_bytes, fold_seconds=new_s, fold_gb_per_s=[total_bytes / t / 1e9 for t in new_s], parent_seconds=par_s)
    print(f'whole model, {len(lin)} linears, r = 256 + r = 16, {total_bytes / 1e9:.1f} GB to move: ' + ', '.join(f'{t * 1e3:.1f} ms' for t in new_s)
          + f'  ({min(total_bytes / t / 1e9 for t in new_s):.0f} .. {max(total_bytes / t / 1e9 for t in new_s):.0f} GB/s, host clock around a synchronise)')
    if par_s:
        print('merge_lora + load_state_dict, ArcFlow adapter alone, device-resident state dict (no upload): ' + ', '.join(f'{t * 1e3:.1f} ms' for t in par_s))
    print(json.dumps(res))


def dora(a, ops, rnd, res):
    """--dora: one DoRA adapter of rank 16 at scale 0.8 per FLUX shape.  The gain pass (``afx_lora_row_gain``: 2 O I bytes to read), the fold with
    its gains (``afx_lora_fold_rows``: 4 O I bytes) and, beside them, the torch formulation of the same result: ``W + s * B @ A`` in fp32,
    ``torch.linalg.norm(dim=1)``, scale by m / norm, cast to bf16.  Device events around --iters launches after a warm-up, the three
    alternating --reps times; the median is printed."""
    import statistics
    import torch
    r, s = RANKS[1], 0.8

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters
    for name, O, I in SHAPES:
        base, dst = rnd(O, I), torch.empty(O, I, dtype=torch.bfloat16, device='cuda')
        A, B = rnd(r, I, std=0.05), rnd(O, r, std=0.05)
        m = base.float().norm(dim=1).contiguous()
        gain = torch.empty(O, dtype=torch.float32, device='cuda')

        def torch_path():
            v = torch.addmm(base.float(), B.float(), A.float(), alpha=s)
            return (v * (m / torch.linalg.norm(v, dim=1))[:, None]).to(torch.bfloat16)
        paths = dict(gain=lambda: ops.lora_row_gain(base, A, B, s, m, out=gain), fold_rows=lambda: ops.lora_fold(base, dst, [A], [B], [s], row_gains=[gain]),
                     torch=torch_path)
        for fn in paths.values():
            for _ in range(3):
                fn()
        ms = {k: [] for k in paths}
        for _ in range(a.reps):
            for k, fn in paths.items():
                ms[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in ms.items()}
        row = dict(name=name, O=O, I=I, rank=r, gain_ms=ms['gain'], fold_rows_ms=ms['fold_rows'], torch_ms=ms['torch'],
                   gain_gb_per_s=2.0 * O * I / (med['gain'] * 1e-3) / 1e9, fold_rows_gb_per_s=4.0 * O * I / (med['fold_rows'] * 1e-3) / 1e9)
        res['shapes'].append(row)
        print(f'{name:32s} [{O:6d}, {I:6d}]  gain {med["gain"] * 1e3:8.1f} us {row["gain_gb_per_s"]:7.1f} GB/s over 2 O I bytes | fold_rows '
              f'{med["fold_rows"] * 1e3:8.1f} us {row["fold_rows_gb_per_s"]:7.1f} GB/s over 4 O I bytes | torch {med["torch"] * 1e3:8.1f} us')
        del base, dst
    print(json.dumps(res))


def kron_factors(n):
    """(m, n / m) with m the largest divisor of n not above sqrt(n): LyCORIS' default factorisation (factor = -1) as recalled."""
    m = int(n ** 0.5)
    while n % m:
        m -= 1
    return m, n // m


def lycoris(a, ops, rnd, res):
    """--lycoris: per FLUX shape, ``afx_lora_fold_terms`` with one LoHa adapter of rank 16, one LoKr adapter at LyCORIS' default factorisation (w2 dense:
    w1 [a, b] holds the smaller factors of O and I, w2 [c, d] the larger), and the mixed call (LoRA r = 256, LoHa and LoKr together), each beside the
    torch formulation of the same result (``torch.kron`` / ``matmul`` / ``mul`` / ``add`` in fp32, then a cast) and beside the plain LoRA fold (r = 256
    and r = 16) of this build and, with --parent-lib, of the parent commit's library.  Device events around --iters launches after a warm-up, the paths
    alternating --reps times; the median is printed, all repeats go into the JSON line.  The buffers are re-used, so a matrix that fits the Infinity
    Cache is not an HBM figure."""
    import ctypes as C
    import statistics
    import torch
    from arcflow_amd import _lib
    parent = None
    if a.parent_lib:
        parent = C.CDLL(a.parent_lib)
        parent.afx_lora_fold.restype, parent.afx_lora_fold.argtypes = _lib.PROTOTYPES['afx_lora_fold']
    s = 0.8

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters
    for name, O, I in SHAPES:
        base, dst = rnd(O, I), torch.empty(O, I, dtype=torch.bfloat16, device='cuda')
        A, B = [rnd(r, I, std=0.05) for r in RANKS], [rnd(O, r, std=0.05) for r in RANKS]
        loha = dict(kind='loha', w1_a=rnd(O, 16, std=0.2), w1_b=rnd(16, I, std=0.2), w2_a=rnd(O, 16, std=0.2), w2_b=rnd(16, I, std=0.2), scale=s)
        (ka, kc), (kb, kd) = kron_factors(O), kron_factors(I)
        lokr = dict(kind='lokr', w1=rnd(ka, kb, std=0.14).float(), w2=rnd(kc, kd, std=0.14).float(), scale=s)
        lora = dict(kind='lora', A=A[0], B=B[0], scale=1.0)
        pa, pb = (C.c_void_p * 2)(*[t.data_ptr() for t in A]), (C.c_void_p * 2)(*[t.data_ptr() for t in B])
        rk, sc = (C.c_int32 * 2)(*RANKS), (C.c_float * 2)(1.0, s)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def t_loha():
            return torch.addcmul(base.float(), loha['w1_a'].float() @ loha['w1_b'].float(), loha['w2_a'].float() @ loha['w2_b'].float(), value=s).to(torch.bfloat16)

        def t_lokr():
            return torch.add(base.float(), torch.kron(lokr['w1'], lokr['w2']), alpha=s).to(torch.bfloat16)

        def t_mixed():
            v = torch.addmm(base.float(), B[0].float(), A[0].float())
            v = torch.addcmul(v, loha['w1_a'].float() @ loha['w1_b'].float(), loha['w2_a'].float() @ loha['w2_b'].float(), value=s)
            return torch.add(v, torch.kron(lokr['w1'], lokr['w2']), alpha=s).to(torch.bfloat16)
        paths = dict(loha=lambda: ops.lora_fold_terms(base, dst, [loha]), torch_loha=t_loha, lokr=lambda: ops.lora_fold_terms(base, dst, [lokr]),
                     torch_lokr=t_lokr, mixed=lambda: ops.lora_fold_terms(base, dst, [lora, loha, lokr]), torch_mixed=t_mixed,
                     lora_fold=lambda: ops.lora_fold(base, dst, A, B, (1.0, s)))
        if parent is not None:
            paths['parent_lora_fold'] = lambda: parent.afx_lora_fold(C.c_void_p(base.data_ptr()), I, C.c_void_p(dst.data_ptr()), I, O, I, 2, pa, pb, rk, sc, stream)
        for fn in paths.values():
            for _ in range(3):
                fn()
        ms = {k: [] for k in paths}
        for _ in range(a.reps):
            for k, fn in paths.items():
                ms[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in ms.items()}
        res['shapes'].append(dict(name=name, O=O, I=I, lokr_factors=[ka, kb, kc, kd], ms=ms, gb_per_s={k: 4.0 * O * I / (v * 1e-3) / 1e9 for k, v in med.items()}))
        print(f'{name:32s} [{O:6d}, {I:6d}] kron [{ka}, {kb}] x [{kc}, {kd}]  ' + '  '.join(f'{k} {v * 1e3:.1f} us' for k, v in med.items()))
        del base, dst
    print(json.dumps(res))


if __name__ == '__main__':
    main()
