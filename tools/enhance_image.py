#!/usr/bin/env python3
"""Rework a photo of any size at its own size, or upscaled, with the ArcFlow student: ``pipe.enhance(image, prompt, scale=, tile=, overlap=,
strength=)`` of ArcFluxPipeline / ArcQwenImagePipeline.  The photo is resampled to ``--scale`` times its size (Lanczos-3 on the GPU), cut
into overlapping tiles of at most ``--tile`` pixels a side, every tile goes through low-strength image-to-image (``--strength``, ``--nfe``
student steps) and the decoded tiles are cross-faded back into one image without seams.

    python tools/enhance_image.py --family flux --snapshot /path/to/FLUX.1-dev --adapter /path/to/arcflow --image photo.jpg \\
        --prompt "a sharp photo" --scale 1.5 --strength 0.3 --out photo_x1.5.png

``--synthetic``: random-init weights of a reduced student and of a reduced VAE (encoder and decoder), random prompt embeddings and a random
photo of ``--size``: writes the result as an image, for trying the path end to end without a snapshot.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.edit_image import synthetic_pipeline          # noqa: E402


def _random_weights(shapes, seed: int):
    """A state dict of ``shapes``: norm scales 1, biases 0, every other weight N(0, 1 / fan_in)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in shapes.items():
        if name.endswith('.bias'):
            sd[name] = torch.zeros(shape)
        elif name.endswith('.gamma') or len(shape) == 1:
            sd[name] = torch.ones(shape)
        else:
            fan_in = 1
            for n in shape[1:]:
                fan_in *= n
            sd[name] = torch.randn(shape, generator=g) * fan_in ** -0.5
    return sd


def synthetic_vae(family: str, seed: int = 0):
    """A reduced random VAE of the family, decoder with ``.encoder`` attached, as ``from_pretrained`` attaches a snapshot's."""
    from arcflow_amd import vae as VAE
    if family == 'flux':
        from oracle import vae_ref
        chans = (64, 128, 128, 128)
        dec = VAE.AutoencoderKLDecoder(vae_ref.make_decoder_weights(chans, seed=seed), chans, norm_num_groups=16)
        dec.encoder = VAE.AutoencoderKLEncoder(_random_weights(VAE.kl_encoder_shapes(chans), seed + 1), chans, norm_num_groups=16)
    else:
        from oracle import vae_qwen_ref
        mean, std = [0.0] * 16, [1.0] * 16
        dec = VAE.AutoencoderKLQwenImageDecoder(vae_qwen_ref.make_decoder_weights(dim=32, seed=seed), mean, std)
        dec.encoder = VAE.AutoencoderKLQwenImageEncoder(_random_weights(VAE.qwen_encoder_shapes(dim=32), seed + 1), mean, std)
    return dec


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--family', choices=['flux', 'qwen'], required=True)
    ap.add_argument('--snapshot', help='local FLUX.1-dev / Qwen-Image snapshot (transformer/, vae/ with encoder weights, text encoders)')
    ap.add_argument('--adapter', help='ArcFlow adapter directory (load_arcflow_adapter)')
    ap.add_argument('--image', help='the photo to rework, of any size (both sides at least 16 pixels after --scale)')
    ap.add_argument('--prompt', default='')
    ap.add_argument('--strength', type=float, default=0.3, help='in (0, 1]: small values stay close to the photo')
    ap.add_argument('--nfe', type=int, default=2)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', required=True)
    ap.add_argument('--synthetic', action='store_true', help='reduced random-init student and VAE, random embeddings, a random photo')
    ap.add_argument('--size', type=int, nargs=2, default=[200, 296], help='--synthetic: height width of the random photo')
    ap.add_argument('--scale', type=float, default=1.0, help='the canvas is the photo resampled to this many times its size (Lanczos-3)')
    ap.add_argument('--tile', type=int, default=1024, help='the largest tile side, a multiple of 16 (the size the model works at)')
    ap.add_argument('--overlap', type=int, default=128, help='pixels neighbouring tiles share at least, cross-faded; at most tile // 2')
    ap.add_argument('--tile-batch', type=int, default=4, help='tiles per denoiser call')
    ap.add_argument('--color-fix', choices=['adain', 'wavelet'], help='match every decoded tile to the canvas tile it was cut from before the '
                    'merge: wavelet swaps the tile\'s low band for the canvas\', adain gives it the canvas\' per-channel mean and deviation')
    args = ap.parse_args(argv)
    kw = dict(scale=args.scale, tile=args.tile, overlap=args.overlap, strength=args.strength, tile_batch=args.tile_batch, color_fix=args.color_fix,
              num_inference_steps=args.nfe, timestep_ratio=1.0 if args.nfe == 2 else 0.5, generator=torch.Generator().manual_seed(args.seed))
    if args.synthetic:
        import numpy as np
        pipe, cond = synthetic_pipeline(args.family, seed=args.seed)
        pipe.vae = synthetic_vae(args.family, seed=args.seed)
        h, w = args.size
        photo = np.random.default_rng(args.seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
        if args.tile == 1024:
            kw.update(tile=64, overlap=min(args.overlap, 32))            # the reduced model's size
        out = pipe.enhance(photo, **cond, **kw).images[0]
    else:
        if not args.snapshot or not args.image or not args.adapter:
            raise SystemExit('--snapshot, --adapter and --image are required (or pass --synthetic)')
        from PIL import Image
        from arcflow_amd.pipelines import ArcFluxPipeline, ArcQwenImagePipeline
        pipe = (ArcFluxPipeline if args.family == 'flux' else ArcQwenImagePipeline).from_pretrained(args.snapshot)
        pipe.load_arcflow_adapter(args.adapter)
        out = pipe.enhance(Image.open(args.image), args.prompt, **kw).images[0]
    out.save(args.out)
    print(f'wrote {args.out} ({out.size[0]} x {out.size[1]})')
    return out


if __name__ == '__main__':
    main()
