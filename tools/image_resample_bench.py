#!/usr/bin/env python
"""Measure the device resize of the edit pipelines against the host path it replaces.

A photo-sized uint8 input (default 3000 x 4000 x 3) is resized to 1024 x 1024 two ways, interleaved round by round on one machine:
  device: the uint8 pixels are uploaded (3 B per pixel) and ``ops.image_resample`` (afx_image_resample, Lanczos-3, clamp) runs on the GPU;
  host:   Pillow ``Image.resize((1024, 1024), LANCZOS)`` on the CPU, ``x / 255`` in numpy, and the fp32 result is uploaded (12 B per output pixel).
Reported: the time of the kernel's two launches (HIP events around 20 back-to-back calls, divided; median over the rounds), its traffic and
achieved GB/s against the HBM roofline, beside the events around a single call (which include launch latency); the
wall time of either input path from the host array to a synchronised fp32 [1, 3, 1024, 1024] tensor on the GPU; and the wall time of
``pipe(image=..., resize='stretch')`` against the same pipeline fed the host-resized image (``resize=None``), on the reduced synthetic student
of tools/edit_image.py with a random-weight VAE encoder of the released FLUX width.  No threshold is set: the baseline is the Pillow path.

    python tools/image_resample_bench.py [--src 3000 4000] [--size 1024] [--rounds 11] [--no-pipe]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

HBM_ROOFLINE_GBPS = 6300.0          # achievable HBM3E rate of one MI355X (8 TB/s peak)


def _wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--src', type=int, nargs=2, default=[3000, 4000], help='source height width')
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--rounds', type=int, default=11)
    ap.add_argument('--no-pipe', action='store_true', help='skip the end-to-end pipeline calls')
    args = ap.parse_args(argv)
    from PIL import Image
    from arcflow_amd import ops
    H, W = args.src
    S = args.size
    photo = np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)
    pil = Image.fromarray(photo)
    dev = torch.from_numpy(photo)[None].cuda()

    def device_path():
        return ops.image_resample(torch.from_numpy(photo)[None].cuda(), S, S)

    def host_image():
        return torch.from_numpy(np.asarray(pil.resize((S, S), Image.LANCZOS), dtype=np.float32) / 255.0).permute(2, 0, 1)[None]

    def host_path():
        return host_image().cuda()
    for _ in range(3):
        ops.image_resample(dev, S, S)
        device_path()
    host_path()
    # the two kernels alone: HIP events around `reps` back-to-back raw C-ABI calls on preallocated buffers, divided by reps.  The host issues a
    # call (one ctypes call, two launches) faster than the GPU runs it, so after the first the queue never drains and launch latency
    # and host time are not part of the quotient; the events around ONE call are reported beside it (that figure includes both).
    import ctypes as C
    from arcflow_amd import _lib
    lib = _lib.load()
    filt = _lib.AFX_FILTER_LANCZOS3
    tw = ops._device_table(W, S, filt, 0.0, float(W), 0.0, 'cuda:0')
    th = ops._device_table(H, S, filt, 0.0, float(H), 0.0, 'cuda:0')
    need = lib.afx_image_resample_ws_bytes(1, 3, H, S)
    ws = torch.empty(need // 4, dtype=torch.float32, device='cuda')
    dst = torch.empty(1, 3, S, S, dtype=torch.float32, device='cuda')
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw():
        _lib.check(lib.afx_image_resample(p(dev), 1, 1, 3, H, W, p(tw[0]), p(tw[1]), p(tw[2]), tw[2].shape[1], p(th[0]), p(th[1]), p(th[2]),
                                          th[2].shape[1], p(dst), S, S, 1, p(ws), need, stream))
    reps = 20

    def events(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            raw()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n
    events(reps)
    assert torch.equal(dst, ops.image_resample(dev, S, S))
    kernel_ms = statistics.median(events(reps) for _ in range(args.rounds))
    single_ms = statistics.median(events(1) for _ in range(args.rounds))
    traffic = H * W * 3 + 2 * 4 * 3 * H * S + 4 * 3 * S * S         # source read, workspace written and read, result written
    t_dev, t_host = [], []
    for _ in range(args.rounds):                                    # interleaved
        t_dev.append(_wall(device_path))
        t_host.append(_wall(host_path))
    diff = (device_path().cpu() - host_image()).abs().max().item()
    res = dict(src=[H, W], size=S, rounds=args.rounds, cpus=os.cpu_count(), cpus_usable=len(os.sched_getaffinity(0)),
               kernel_ms=round(kernel_ms, 4), kernel_reps=reps, single_call_events_ms=round(single_ms, 4), traffic_mb=round(traffic / 1e6, 1), kernel_gbps=round(traffic / kernel_ms / 1e6, 1),
               hbm_roofline_gbps=HBM_ROOFLINE_GBPS, roofline_fraction=round(traffic / kernel_ms / 1e6 / HBM_ROOFLINE_GBPS, 3),
               input_device_ms=round(statistics.median(t_dev), 3), input_pillow_ms=round(statistics.median(t_host), 3),
               max_abs_diff_to_pillow_8bit=round(diff, 5))
    if not args.no_pipe:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import vae_encoder_ref as E
        from arcflow_amd import vae as VAE
        from edit_image import synthetic_pipeline
        pipe, cond = synthetic_pipeline('flux')
        chans = (128, 256, 512, 512)

        class _Vae:
            encoder = VAE.AutoencoderKLEncoder(E.make_encoder_weights(chans, seed=3), chans)
        pipe.vae = _Vae()
        kw = dict(num_inference_steps=2, timestep_ratio=1.0, output_type='latent', strength=0.8, **cond)

        def pipe_device():
            pipe(image=photo, resize='stretch', height=S, width=S, generator=torch.Generator().manual_seed(0), **kw)

        def pipe_host():
            pipe(image=host_image(), generator=torch.Generator().manual_seed(0), **kw)
        pipe_device()
        pipe_host()
        p_dev, p_host = [], []
        for _ in range(args.rounds):
            p_dev.append(_wall(pipe_device))
            p_host.append(_wall(pipe_host))
        res.update(pipe_device_ms=round(statistics.median(p_dev), 3), pipe_pillow_ms=round(statistics.median(p_host), 3),
                   pipe='reduced synthetic FLUX student (1 + 1 blocks, width 256), released-width random VAE encoder, 2 NFE, latent output')
    print(json.dumps(res))
    return res


if __name__ == '__main__':
    main()
