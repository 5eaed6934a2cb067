#!/usr/bin/env python3
"""1024^2 decode time of the two VAE decoders (random weights of the released shapes).

    python tools/vae_bench.py [both|flux|qwen]            decode times (wall clock, mean of 5)
    python tools/vae_bench.py [both|flux|qwen] --encode   1024^2 ENCODE: HIP-event time, warmed up, median of 21 interleaved rounds of
                                                          (HIP encoder | the same encoder in torch under bf16 autocast | this repo's decoder)
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arcflow_amd.vae import AutoencoderKLDecoder, AutoencoderKLQwenImageDecoder  # noqa: E402
from oracle import vae_qwen_ref, vae_ref  # noqa: E402   (weight generators only)


def timeit(fn, n=5):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def bench_encode(which, rounds=21):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
    import vae_encoder_ref as E                      # the torch restatement of the encoders (weight generators + the comparator graph)
    from arcflow_amd.vae import AutoencoderKLEncoder, AutoencoderKLQwenImageEncoder
    img = torch.rand(1, 3, 1024, 1024, device='cuda') * 2 - 1
    tok = torch.randn(1, 4096, 64, device='cuda')
    print(f'device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, rounds {rounds} (median), 3 warm-up rounds')

    def event_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def run(name, fns):
        for _ in range(3):
            for f in fns.values():
                f()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(rounds):                      # interleaved: clock / thermal drift hits every candidate alike
            for k, f in fns.items():
                t[k].append(event_ms(f))
        for k, v in t.items():
            v.sort()
            print(f'{name:5s} {k:34s} median {v[len(v) // 2]:8.2f} ms   min {v[0]:8.2f}   max {v[-1]:8.2f}')

    if which in ('both', 'flux'):
        chans = (128, 256, 512, 512)
        we = E.make_encoder_weights(chans, seed=0)
        enc = AutoencoderKLEncoder(we, chans)
        dec = AutoencoderKLDecoder(vae_ref.make_decoder_weights(chans, seed=0), chans)
        wd = {k: v.cuda().float() for k, v in we.items()}

        def torch_bf16():
            with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
                return E.flux_moments(wd, img, chans, 32)
        run('flux', {'HIP encode 1024^2': lambda: enc.encode(img, sample=False, packed=True),
                     'torch bf16-autocast encode 1024^2': torch_bf16,
                     'HIP decode 1024^2': lambda: dec.decode_packed(tok, 64, 64)})
        del enc, dec, wd
        torch.cuda.empty_cache()
    if which in ('both', 'qwen'):
        we = E.make_qwen_encoder_weights(dim=96, seed=0)
        enc = AutoencoderKLQwenImageEncoder(we, [0.0] * 16, [1.0] * 16)
        dec = AutoencoderKLQwenImageDecoder(vae_qwen_ref.make_decoder_weights(dim=96, seed=0), [0.0] * 16, [1.0] * 16)
        # the comparator gets the one-frame reduction for free: every 3x3x3 kernel cut to its last temporal tap, so conv3d sees no zero frames
        wd = {k: (v[:, :, -1:] if v.dim() == 5 and v.shape[2] == 3 else v).cuda().float().contiguous() for k, v in we.items() if 'time_conv' not in k}

        def torch_bf16_q():
            with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
                return E.qwen_moments(wd, img)
        run('qwen', {'HIP encode 1024^2': lambda: enc.encode(img, sample=False, packed=True),
                     'torch bf16-autocast encode 1024^2': torch_bf16_q,
                     'HIP decode 1024^2': lambda: dec.decode_packed(tok, 64, 64)})


args = [a for a in sys.argv[1:] if not a.startswith('--')]
which = args[0] if args else 'both'
if '--encode' in sys.argv[1:]:
    bench_encode(which)
    sys.exit(0)
tok = torch.randn(1, 4096, 64, device='cuda')
if which in ('both', 'flux'):
  flux = AutoencoderKLDecoder(vae_ref.make_decoder_weights((128, 256, 512, 512), seed=0), (128, 256, 512, 512))
  print(f'FLUX AutoencoderKL decoder        1024^2: {timeit(lambda: flux.decode_packed(tok, 64, 64)):.1f} ms')
if which in ('both', 'qwen'):
  qwen = AutoencoderKLQwenImageDecoder(vae_qwen_ref.make_decoder_weights(dim=96, seed=0), [0.0] * 16, [1.0] * 16)
  print(f'Qwen AutoencoderKLQwenImage decoder 1024^2: {timeit(lambda: qwen.decode_packed(tok, 64, 64)):.1f} ms')
