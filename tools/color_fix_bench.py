#!/usr/bin/env python
"""Measure ``ops.color_fix`` (afx_color_fix), the colour match of decoded tiles to the canvas tiles they were cut from, each mode against
the same operation written in torch, on one machine, interleaved round by round.

The default is one ``tile_batch`` of ``pipe.enhance``: 4 x 3 x 1024 x 1024 fp32 tiles in [-1, 1] and their sources in [0, 1].
  wavelet, fused:   the raw C-ABI call on preallocated buffers, one launch, all five levels of a tile in LDS;
  wavelet, levels:  AFX_COLOR_WAVELET_LEVELS, one launch per pass through two workspace planes (the same bits);
  wavelet, torch:   StableSR's form as a user would write it: five levels of ``F.pad(mode='replicate')`` + depthwise
                    ``F.conv2d(dilation=r)`` with the 3 x 3 kernel [1, 2, 1]^T [1, 2, 1] / 16 on BOTH images, out = e - low(e) + low(s');
  adain, device:    the raw call, three launches;   adain, torch: ``mean`` / ``var`` over (H, W) plus broadcast arithmetic.
Reported per pass: the device time by HIP events around ``--reps`` back-to-back calls, divided (after warm-up rounds; median, min and max
over the rounds); for the device passes the GB/s of the algorithmic traffic -- e and s read once, out written once, 37.7 MB per
3 x 1024 x 1024 fp32 image (the AdaIN pass reads e twice: 50.3 MB) -- as a share of the 6.29 TB/s a streaming kernel reaches on one MI355X;
how many elements differ from the torch form and by how much; and what the fix adds to an enhance of ``--tiles`` tiles beside the
cut + merge time given by ``--cut-merge-ms``.  Nothing is asserted on the time.

    python tools/color_fix_bench.py [--batch 4] [--size 1024 1024] [--tiles 35] [--rounds 11] [--reps 10]
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
    ap.add_argument('--batch', type=int, default=4, help='tiles per call (enhance: tile_batch)')
    ap.add_argument('--size', type=int, nargs=2, default=[1024, 1024], help='tile height width')
    ap.add_argument('--tiles', type=int, default=35, help='tiles of the enhance the share is given for')
    ap.add_argument('--cut-merge-ms', type=float, default=0.33, help='cut + merge time of that enhance (tools/tiles_bench.py)')
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args(argv)
    from arcflow_amd import _lib, ops
    B, (H, W), Cn = args.batch, args.size, 3
    g = torch.Generator(device='cuda').manual_seed(0)
    e = torch.rand(B, Cn, H, W, generator=g, device='cuda') * 2.4 - 1.2
    s = torch.rand(B, Cn, H, W, generator=g, device='cuda')
    out = {m: torch.empty_like(e) for m in ops.COLOR_FIX_MODES}
    ws = {m: ops.color_fix_ws(m, B, Cn, H, W) for m in ops.COLOR_FIX_MODES}
    lib = _lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())              # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def dev(mode):
        def fn():
            _lib.check(lib.afx_color_fix(p(e), _lib.AFX_DT_F32, p(s), B, 1, ops.COLOR_FIX_MODES[mode], p(out[mode]), None, p(ws[mode]),
                                         ws[mode].numel() * 8, B, Cn, H, W, stream))
        return fn

    k1 = torch.tensor([1.0, 2.0, 1.0], device='cuda')
    kern = (k1[:, None] * k1[None, :] / 16.0)[None, None].repeat(Cn, 1, 1, 1)
    torch_out = {}

    def low(x):
        for r in (1, 2, 4, 8, 16):
            x = F.conv2d(F.pad(x, (r, r, r, r), mode='replicate'), kern, groups=Cn, dilation=r)
        return x

    def torch_wavelet():
        torch_out['wavelet'] = (e - low(e)) + low(s * 2 - 1)

    def torch_adain():
        s1 = s * 2 - 1
        sd_e, sd_s = (e.var((2, 3), unbiased=False, keepdim=True) + 1e-5).sqrt(), (s1.var((2, 3), unbiased=False, keepdim=True) + 1e-5).sqrt()
        torch_out['adain'] = (e - e.mean((2, 3), keepdim=True)) / sd_e * sd_s + s1.mean((2, 3), keepdim=True)

    def events(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    fns = dict(wavelet=dev('wavelet'), wavelet_levels=dev('wavelet_levels'), wavelet_torch=torch_wavelet, adain=dev('adain'), adain_torch=torch_adain)
    for _ in range(args.warmup):
        for fn in fns.values():
            events(fn, args.reps)
    ms = {k: [] for k in fns}
    for _ in range(args.rounds):                                     # interleaved
        for k, fn in fns.items():
            ms[k].append(events(fn, args.reps))
    torch.cuda.synchronize()
    assert torch.equal(out['wavelet'].view(torch.int32), out['wavelet_levels'].view(torch.int32))          # the two forms: the same bits
    image_bytes = Cn * H * W * 4
    traffic = dict(wavelet=3 * image_bytes * B, wavelet_levels=3 * image_bytes * B, adain=4 * image_bytes * B)
    res = dict(batch=B, channels=Cn, size=[H, W], rounds=args.rounds, warmup=args.warmup, reps=args.reps, stream_gbps=STREAM_GBPS,
               device=torch.cuda.get_device_name(0))
    for k in fns:
        m = statistics.median(ms[k])
        res.update({f'{k}_ms': round(m, 4), f'{k}_ms_min': round(min(ms[k]), 4), f'{k}_ms_max': round(max(ms[k]), 4)})
        if k in traffic:
            res.update({f'{k}_traffic_mb': round(traffic[k] / 1e6, 1), f'{k}_gbps': round(traffic[k] / m / 1e6, 1),
                        f'{k}_stream_share': round(traffic[k] / m / 1e6 / STREAM_GBPS, 4)})
    for k in ('wavelet', 'adain'):
        d = (out[k] - torch_out[k]).abs()
        res.update({f'{k}_speedup_vs_torch': round(res[f'{k}_torch_ms'] / res[f'{k}_ms'], 2),
                    f'{k}_elements_differing_from_torch': round(float((d > 0).float().mean()), 6), f'{k}_max_abs_diff_to_torch': float(d.max())})
    res['wavelet_speedup_vs_levels'] = round(res['wavelet_levels_ms'] / res['wavelet_ms'], 2)
    calls = -(-args.tiles // B)
    for k in ('wavelet', 'adain'):
        res[f'{k}_ms_per_enhance_of_{args.tiles}_tiles'] = round(calls * res[f'{k}_ms'], 4)
    res['cut_merge_ms'] = args.cut_merge_ms
    print(json.dumps(res))
    return res


if __name__ == '__main__':
    main()
