#!/usr/bin/env python
"""Measure pasting an edit back into a photo: ``ops.image_paste`` (afx_image_paste) against the same operation in Pillow on the host.

A 1024 x 1024 edit (fp32 [1, 3, 1024, 1024] in [-1, 1]) and its mask are pasted into a window of a photo-sized uint8 image (default
3000 x 4000 x 3; the window is centred, ``--window`` pixels on a side), two ways, interleaved round by round on one machine:
  device: the raw C-ABI call on preallocated buffers (its launches: the horizontal taps of the image and of the mask, the paste);
  host:   Pillow ``resize`` of the 8-bit edit (LANCZOS) and of the 8-bit mask (BILINEAR) to the window, ``paste`` of both, ``Image.composite``.
Reported: the device time by HIP events around ``--reps`` back-to-back calls, divided (after warm-up rounds; median, min and max over the
rounds), beside the events around a single call (which include launch latency); the algorithmic traffic -- the photo read and the result
written (2 x 36 MB = 72 MB at the default size), the edit and the mask read, the workspace written and read -- and the GB/s over it, as a
share of the 6.29 TB/s a streaming kernel reaches on one MI355X; the host's wall time; how many bytes of the two results differ.  Nothing
is asserted on the time.

    python tools/image_paste_bench.py [--src 3000 4000] [--size 1024] [--window 1536] [--rounds 11] [--reps 20] [--no-mask]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_GBPS = 6290.0            # what a streaming kernel reaches on one MI355X (8 TB/s peak)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--src', type=int, nargs=2, default=[3000, 4000], help='photo height width')
    ap.add_argument('--size', type=int, default=1024, help='side of the edit')
    ap.add_argument('--window', type=int, default=1536, help='side of the centred window the edit is pasted into')
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--no-mask', action='store_true', help='mask = NULL: the whole window is the edit')
    args = ap.parse_args(argv)
    from PIL import Image
    from arcflow_amd import _lib, ops
    H, W = args.src
    S, Wn = args.size, min(args.window, H, W)
    x0, y0 = (W - Wn) // 2, (H - Wn) // 2
    window = (x0, y0, x0 + Wn, y0 + Wn)
    rng = np.random.default_rng(0)
    photo = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    edit8 = rng.integers(0, 256, (S, S, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:S, 0:S]
    mask8 = np.clip(255.0 * (1.25 - np.hypot(yy - S / 2, xx - S / 2) / (S / 2.5)), 0, 255).round().astype(np.uint8)       # a feathered disc
    src = torch.from_numpy(photo)[None].cuda()
    img = (torch.from_numpy(edit8).cuda().permute(2, 0, 1)[None].float() * 2.0 / 255.0 - 1.0).contiguous()
    mask = None if args.no_mask else (torch.from_numpy(mask8).cuda().float() / 255.0)[None, None].contiguous()
    dst = torch.empty_like(src)

    lib = _lib.load()
    dev = str(src.device)
    tabs = [ops._device_table(S, Wn, f, 0.0, float(S), 0.0, dev) for f in (_lib.AFX_FILTER_LANCZOS3,) * 2 + (_lib.AFX_FILTER_TRIANGLE,) * 2]
    if mask is None:
        tabs[2:] = [(None, None, None)] * 2
    mb = 0 if mask is None else 1
    need = lib.afx_image_paste_ws_bytes(1, mb, S, Wn)
    ws = torch.empty(need // 4, dtype=torch.float32, device='cuda')
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    targs = [a for t in tabs for a in (p(t[0]), p(t[1]), p(t[2]), 0 if t[2] is None else t[2].shape[1])]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw():
        _lib.check(lib.afx_image_paste(p(img), p(mask), mb, p(src), p(dst), 1, S, S, H, W, *window, Wn, Wn, *targs, p(ws), need, stream))

    def events(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            raw()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    pil_photo, pil_edit, pil_mask = Image.fromarray(photo), Image.fromarray(edit8), Image.fromarray(mask8)

    def host():
        pasted = pil_photo.copy()
        pasted.paste(pil_edit.resize((Wn, Wn), Image.LANCZOS), (x0, y0))
        if args.no_mask:
            return pasted
        full = Image.new('L', pil_photo.size, 0)
        full.paste(pil_mask.resize((Wn, Wn), Image.BILINEAR), (x0, y0))
        return Image.composite(pasted, pil_photo, full)

    for _ in range(args.warmup):
        events(args.reps)
    host()
    assert torch.equal(dst, ops.image_paste(img, mask, src, window))
    dev_ms, single_ms, host_ms = [], [], []
    for _ in range(args.rounds):                                    # interleaved
        dev_ms.append(events(args.reps))
        single_ms.append(events(1))
        t = time.perf_counter()
        out = host()
        host_ms.append((time.perf_counter() - t) * 1e3)
    diff = np.abs(dst[0].cpu().numpy().astype(np.int16) - np.asarray(out, dtype=np.int16))
    base = 2 * H * W * 3                                            # the photo read, the result written
    extra = 4 * (3 + mb) * S * S + 2 * need                         # the edit and the mask read, the workspace written and read
    ms = statistics.median(dev_ms)
    res = dict(src=[H, W], size=S, window=list(window), mask=not args.no_mask, rounds=args.rounds, warmup=args.warmup, reps=args.reps,
               paste_ms=round(ms, 4), paste_ms_min=round(min(dev_ms), 4), paste_ms_max=round(max(dev_ms), 4),
               single_call_events_ms=round(statistics.median(single_ms), 4), photo_mb=round(base / 1e6, 1), workspace_mb=round(need / 1e6, 1),
               traffic_mb=round((base + extra) / 1e6, 1), gbps=round((base + extra) / ms / 1e6, 1), stream_gbps=STREAM_GBPS,
               stream_share=round((base + extra) / ms / 1e6 / STREAM_GBPS, 4), pillow_ms=round(statistics.median(host_ms), 2),
               cpus_usable=len(os.sched_getaffinity(0)), bytes_differing_from_pillow=round(float((diff > 0).mean()), 5),
               max_byte_diff_to_pillow=int(diff.max()))
    print(json.dumps(res))
    return res


if __name__ == '__main__':
    main()
