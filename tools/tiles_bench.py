#!/usr/bin/env python
"""Measure the two device passes of ``pipe.enhance`` around the denoiser: ``ops.tiles_cut`` (afx_tiles_cut) and ``ops.tiles_merge``
(afx_tiles_merge), each against the same operation written in torch, on one machine, interleaved round by round.

The default is a 1.5x enhance of a 3000 x 4000 photo: a 4500 x 6000 canvas, 1024-pixel tiles, overlap 128 (5 x 7 = 35 tiles).
  merge, device: the raw C-ABI call on preallocated buffers, one launch;
  merge, torch:  an fp32 canvas [3, H, W] and a weight plane [H, W], per tile ``canvas[window] += w * (0.5 tile + 0.5)`` and
                 ``weight[window] += w`` with w the outer product of the tile's un-normalised ramps, then divide, clamp, x 255, round, to uint8
                 [H, W, 3] -- the formulation a host-driven pipeline would use (its rounding differs from the kernel's in the last place);
  cut, device:   the raw call, one launch;   cut, torch: ``torch.stack`` of the 35 slices.
Reported per pass: the device time by HIP events around ``--reps`` back-to-back calls, divided (after warm-up rounds; median, min and max
over the rounds), the algorithmic traffic -- every tile value read once and every output byte written once for the merge, the tiles read and
written for the cut -- and the GB/s over it as a share of the 6.29 TB/s a streaming kernel reaches on one MI355X; the torch time the same
way; how many bytes of the two merges differ.  Nothing is asserted on the time.

    python tools/tiles_bench.py [--src 3000 4000] [--scale 1.5] [--tile 1024] [--overlap 128] [--rounds 11] [--reps 10]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_GBPS = 6290.0            # what a streaming kernel reaches on one MI355X (8 TB/s peak)


def _ramp(L, t, o, i, k):
    """u_i(x) over tile i's span, fp32 [t]: the planner's un-normalised cross-fade weight."""
    x = np.arange(o, o + t)
    dl = x - o + 1 if i > 0 else np.full(t, np.inf)
    dr = o + t - x if i < k - 1 else np.full(t, np.inf)
    u = np.minimum(dl, dr)
    return np.where(np.isinf(u), 1.0, u).astype(np.float32)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--src', type=int, nargs=2, default=[3000, 4000], help='photo height width')
    ap.add_argument('--scale', type=float, default=1.5)
    ap.add_argument('--tile', type=int, default=1024)
    ap.add_argument('--overlap', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args(argv)
    from arcflow_amd import _lib, ops, schedule
    H, W = round(args.src[0] * args.scale), round(args.src[1] * args.scale)
    plan = schedule.tile_plan(H, W, args.tile, args.overlap)
    th, tw, T = plan.th, plan.tw, plan.T
    g = torch.Generator(device='cuda').manual_seed(0)
    canvas = torch.rand(3, H, W, generator=g, device='cuda')
    tiles = ops.tiles_cut(canvas, plan) * 2.0 - 1.0                      # consistent in the overlaps, in the decoder's range
    cut_out = torch.empty_like(tiles)
    dst = torch.empty(H, W, 3, dtype=torch.uint8, device='cuda')
    lib = _lib.load()
    _, oy, ox, ytab, xtab = ops._device_plan(plan.H, plan.W, plan.tile, plan.overlap, str(canvas.device))
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def dev_merge():
        _lib.check(lib.afx_tiles_merge(p(tiles), T, th, tw, p(oy), plan.ky, p(ox), plan.kx, p(ytab[0]), p(ytab[1]), p(ytab[2]), ytab[2].shape[1],
                                       p(xtab[0]), p(xtab[1]), p(xtab[2]), xtab[2].shape[1], p(dst), H, W, stream))

    def dev_cut():
        _lib.check(lib.afx_tiles_cut(p(canvas), H, W, p(oy), plan.ky, p(ox), plan.kx, th, tw, p(cut_out), stream))

    uy = [torch.from_numpy(_ramp(H, th, int(o), i, plan.ky)).cuda() for i, o in enumerate(plan.oy)]
    ux = [torch.from_numpy(_ramp(W, tw, int(o), i, plan.kx)).cuda() for i, o in enumerate(plan.ox)]
    win = [(int(y), int(x), uy[iy][:, None] * ux[ix][None, :]) for iy, y in enumerate(plan.oy) for ix, x in enumerate(plan.ox)]
    acc, wsum = torch.empty(3, H, W, device='cuda'), torch.empty(H, W, device='cuda')
    torch_out = [None]

    def torch_merge():
        acc.zero_()
        wsum.zero_()
        for i, (y, x, w) in enumerate(win):
            acc[:, y:y + th, x:x + tw] += w * (0.5 * tiles[i] + 0.5)
            wsum[y:y + th, x:x + tw] += w
        torch_out[0] = (acc / wsum).clamp_(0, 1).mul_(255).round_().to(torch.uint8).permute(1, 2, 0).contiguous()

    def torch_cut():
        torch_out[0] = torch.stack([canvas[:, y:y + th, x:x + tw] for y in plan.oy.tolist() for x in plan.ox.tolist()])

    def events(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    fns = dict(merge=dev_merge, merge_torch=torch_merge, cut=dev_cut, cut_torch=torch_cut)
    for _ in range(args.warmup):
        for fn in fns.values():
            events(fn, args.reps)
    ms = {k: [] for k in fns}
    for _ in range(args.rounds):                                     # interleaved
        for k, fn in fns.items():
            ms[k].append(events(fn, args.reps))
    torch_cut()
    assert torch.equal(cut_out, torch_out[0])
    torch_merge()
    diff = (dst.to(torch.int16) - torch_out[0].to(torch.int16)).abs()
    tile_bytes = T * 3 * th * tw * 4
    traffic = dict(merge=tile_bytes + H * W * 3, cut=2 * tile_bytes)
    res = dict(src=args.src, scale=args.scale, canvas=[H, W], tile=[th, tw], overlap=args.overlap, tiles=[plan.ky, plan.kx], rounds=args.rounds,
               warmup=args.warmup, reps=args.reps, stream_gbps=STREAM_GBPS)
    for k in ('merge', 'cut'):
        m, t = statistics.median(ms[k]), statistics.median(ms[k + '_torch'])
        res.update({f'{k}_ms': round(m, 4), f'{k}_ms_min': round(min(ms[k]), 4), f'{k}_ms_max': round(max(ms[k]), 4),
                    f'{k}_traffic_mb': round(traffic[k] / 1e6, 1), f'{k}_gbps': round(traffic[k] / m / 1e6, 1),
                    f'{k}_stream_share': round(traffic[k] / m / 1e6 / STREAM_GBPS, 4), f'{k}_torch_ms': round(t, 4),
                    f'{k}_torch_ms_min': round(min(ms[k + '_torch']), 4), f'{k}_torch_ms_max': round(max(ms[k + '_torch']), 4),
                    f'{k}_speedup_vs_torch': round(t / m, 2)})
    res.update(merge_bytes_differing_from_torch=round(float((diff > 0).float().mean()), 6), merge_max_byte_diff_to_torch=int(diff.max()))
    print(json.dumps(res))
    return res


if __name__ == '__main__':
    main()
