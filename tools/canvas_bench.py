#!/usr/bin/env python
"""Measure the two device passes of ``pipe.outpaint`` around the denoiser: ``ops.canvas_extend`` (afx_canvas_extend) and
``ops.canvas_mark`` (afx_canvas_mark), each against the same operation written in torch, on one machine, interleaved round by round.

The default is a 3000 x 4000 photo extended 512 px on every side (a 4024 x 5024 canvas) and a 1024 x 1024 window of that canvas.
  extend, device: the raw C-ABI call on preallocated buffers, one launch, canvas and mask together;
  extend, torch:  ``F.pad(mode='reflect' | 'replicate')`` on the bytes permuted to [B, 3, H, W] (as float: torch pads no integers with
                  these modes), back to uint8 [B, Hc, Wc, 3], plus the mask as ``1 - (min(index ramps) + 1) / (blend + 1)`` clamped at 0
                  inside the photo's rectangle and 1 outside -- the formulation a host-driven pipeline would use;
  mark, device:   the raw call, one launch, in place;
  mark, torch:    the slice update ``M[window] = torch.minimum(M[window], ramp)`` with the ramp plane precomputed.
Reported per pass: the device time by HIP events around ``--reps`` back-to-back calls, divided (after warm-up rounds; median, min and max
over the rounds), the algorithmic traffic -- the photo read once, the canvas and the mask written once for the extend; the window read
and written once for the mark -- and the GB/s over it as a share of the 6.29 TB/s a streaming kernel reaches on one MI355X; the torch time
the same way.  The two formulations are compared for equality.  Nothing is asserted on the time.

    python tools/canvas_bench.py [--src 3000 4000] [--extend 512] [--window 1024] [--blend 32] [--fill reflect] [--rounds 11] [--reps 10]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_GBPS = 6290.0            # what a streaming kernel reaches on one MI355X (8 TB/s peak)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--src', type=int, nargs=2, default=[3000, 4000], help='photo height width')
    ap.add_argument('--extend', type=int, default=512, help='pixels added on every side')
    ap.add_argument('--window', type=int, default=1024)
    ap.add_argument('--blend', type=int, default=32)
    ap.add_argument('--fill', choices=['reflect', 'edge'], default='reflect')
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args(argv)
    from arcflow_amd import _lib, ops
    H, W = args.src
    e, blend, win = args.extend, args.blend, args.window
    Hc, Wc = H + 2 * e, W + 2 * e
    g = torch.Generator(device='cuda').manual_seed(0)
    src = torch.randint(0, 256, (1, H, W, 3), generator=g, device='cuda', dtype=torch.uint8)
    canvas = torch.empty(1, Hc, Wc, 3, dtype=torch.uint8, device='cuda')
    mask = torch.empty(1, 1, Hc, Wc, dtype=torch.float32, device='cuda')
    window = (Wc - win - e // 2, e // 2, Wc - e // 2, e // 2 + win)            # an inner window: all four sides ramp
    state = torch.rand(1, 1, Hc, Wc, generator=g, device='cuda')
    M, M_torch = state.clone(), state.clone()
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fill = ops.CANVAS_FILLS[args.fill]

    def dev_extend():
        _lib.check(lib.afx_canvas_extend(p(src), 1, H, W, e, e, e, e, fill, blend, p(canvas), p(mask), stream))

    def dev_mark():
        _lib.check(lib.afx_canvas_mark(p(M), Hc, Wc, *window, blend, stream))

    iy, ix = torch.arange(H, device='cuda'), torch.arange(W, device='cuda')
    torch_out = [None, None]

    def torch_extend():
        padded = F.pad(src.permute(0, 3, 1, 2).float(), (e, e, e, e), mode='reflect' if args.fill == 'reflect' else 'replicate')
        torch_out[0] = padded.to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        d = torch.minimum(torch.minimum(iy, H - 1 - iy)[:, None], torch.minimum(ix, W - 1 - ix)[None, :])
        m = torch.ones(1, 1, Hc, Wc, device='cuda')
        m[0, 0, e:e + H, e:e + W] = (1.0 - (d + 1).float() / float(blend + 1)).clamp_(min=0.0)
        torch_out[1] = m

    x0, y0, x1, y1 = window
    jy, jx = torch.arange(win, device='cuda'), torch.arange(win, device='cuda')
    dwin = torch.minimum(torch.minimum(jy, win - 1 - jy)[:, None], torch.minimum(jx, win - 1 - jx)[None, :])
    ramp = (1.0 - (dwin + 1).float() / float(blend + 1)).clamp_(min=0.0)

    def torch_mark():
        M_torch[0, 0, y0:y1, x0:x1] = torch.minimum(M_torch[0, 0, y0:y1, x0:x1], ramp)

    def events(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    fns = dict(extend=dev_extend, extend_torch=torch_extend, mark=dev_mark, mark_torch=torch_mark)
    for _ in range(args.warmup):
        for fn in fns.values():
            events(fn, args.reps)
    ms = {k: [] for k in fns}
    for _ in range(args.rounds):                                     # interleaved
        for k, fn in fns.items():
            ms[k].append(events(fn, args.reps))
    dev_extend()
    torch_extend()
    torch.cuda.synchronize()
    same = dict(extend_canvas_equals_torch=bool(torch.equal(canvas, torch_out[0])),
                extend_mask_max_diff_to_torch=float((mask - torch_out[1]).abs().max()), mark_max_diff_to_torch=float((M - M_torch).abs().max()))
    traffic = dict(extend=H * W * 3 + Hc * Wc * 3 + Hc * Wc * 4, mark=2 * win * win * 4)
    res = dict(src=args.src, extend=e, canvas=[Hc, Wc], window=list(window), blend=blend, fill=args.fill, rounds=args.rounds, warmup=args.warmup,
               reps=args.reps, stream_gbps=STREAM_GBPS)
    for k in ('extend', 'mark'):
        m, t = statistics.median(ms[k]), statistics.median(ms[k + '_torch'])
        res.update({f'{k}_ms': round(m, 4), f'{k}_ms_min': round(min(ms[k]), 4), f'{k}_ms_max': round(max(ms[k]), 4),
                    f'{k}_traffic_mb': round(traffic[k] / 1e6, 1), f'{k}_gbps': round(traffic[k] / m / 1e6, 1),
                    f'{k}_stream_share': round(traffic[k] / m / 1e6 / STREAM_GBPS, 4), f'{k}_torch_ms': round(t, 4),
                    f'{k}_torch_ms_min': round(min(ms[k + '_torch']), 4), f'{k}_torch_ms_max': round(max(ms[k + '_torch']), 4),
                    f'{k}_speedup_vs_torch': round(t / m, 2)})
    res.update(same)
    print(json.dumps(res))
    return res


if __name__ == '__main__':
    main()
