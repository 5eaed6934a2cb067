#!/usr/bin/env python3
"""Make a photo larger and let the ArcFlow student paint what lies beyond its borders: ``pipe.outpaint(image, prompt, left=, right=, top=,
bottom=, tile=, overlap=, blend=, fill=, strength=)`` of ArcFluxPipeline / ArcQwenImagePipeline.  The photo is laid on the extended canvas,
the new pixels are filled from it (mirrored or the border repeated) and then repainted window by window, each window one inpainting call
that sees what the windows before it painted.

    python tools/outpaint_image.py --family flux --snapshot /path/to/FLUX.1-dev --adapter /path/to/arcflow --image photo.jpg \\
        --prompt "a wide landscape" --left 512 --right 512 --out photo_wide.png

``--synthetic``: random-init weights of a reduced student and of a reduced VAE (encoder and decoder), random prompt embeddings and a random
photo of ``--size``: writes the result as an image, for trying the path end to end without a snapshot.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.edit_image import synthetic_pipeline          # noqa: E402
from tools.enhance_image import synthetic_vae            # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--family', choices=['flux', 'qwen'], required=True)
    ap.add_argument('--snapshot', help='local FLUX.1-dev / Qwen-Image snapshot (transformer/, vae/ with encoder weights, text encoders)')
    ap.add_argument('--adapter', help='ArcFlow adapter directory (load_arcflow_adapter)')
    ap.add_argument('--image', help='the photo to extend, of any size')
    ap.add_argument('--prompt', default='')
    ap.add_argument('--left', type=int, default=0, help='pixels to add on the left')
    ap.add_argument('--right', type=int, default=0)
    ap.add_argument('--top', type=int, default=0)
    ap.add_argument('--bottom', type=int, default=0)
    ap.add_argument('--tile', type=int, default=1024, help='the largest window side, a multiple of 16 (the size the model works at)')
    ap.add_argument('--overlap', type=int, default=256, help='pixels a window reaches back into what is known; at most tile // 2')
    ap.add_argument('--blend', type=int, default=32, help='pixels of cross-fade inside the photo and between windows; at most overlap // 2')
    ap.add_argument('--fill', choices=['reflect', 'edge'], default='reflect', help='what the new pixels hold before they are painted')
    ap.add_argument('--strength', type=float, default=1.0, help='in (0, 1]: 1 paints the new pixels from pure noise')
    ap.add_argument('--nfe', type=int, default=2)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', required=True)
    ap.add_argument('--synthetic', action='store_true', help='reduced random-init student and VAE, random embeddings, a random photo')
    ap.add_argument('--size', type=int, nargs=2, default=[200, 296], help='--synthetic: height width of the random photo')
    args = ap.parse_args(argv)
    if not (args.left or args.right or args.top or args.bottom):
        raise SystemExit('give at least one of --left, --right, --top, --bottom')
    kw = dict(left=args.left, right=args.right, top=args.top, bottom=args.bottom, tile=args.tile, overlap=args.overlap, blend=args.blend,
              fill=args.fill, strength=args.strength, num_inference_steps=args.nfe, timestep_ratio=1.0 if args.nfe == 2 else 0.5,
              generator=torch.Generator().manual_seed(args.seed))
    if args.synthetic:
        import numpy as np
        pipe, cond = synthetic_pipeline(args.family, seed=args.seed)
        pipe.vae = synthetic_vae(args.family, seed=args.seed)
        h, w = args.size
        photo = np.random.default_rng(args.seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
        if args.tile == 1024:
            kw.update(tile=64, overlap=min(args.overlap, 32), blend=min(args.blend, 16))            # the reduced model's size
        out = pipe.outpaint(photo, **cond, **kw).images[0]
    else:
        if not args.snapshot or not args.image or not args.adapter:
            raise SystemExit('--snapshot, --adapter and --image are required (or pass --synthetic)')
        from PIL import Image
        from arcflow_amd.pipelines import ArcFluxPipeline, ArcQwenImagePipeline
        pipe = (ArcFluxPipeline if args.family == 'flux' else ArcQwenImagePipeline).from_pretrained(args.snapshot)
        pipe.load_arcflow_adapter(args.adapter)
        out = pipe.outpaint(Image.open(args.image), args.prompt, **kw).images[0]
    out.save(args.out)
    print(f'wrote {args.out} ({out.size[0]} x {out.size[1]})')
    return out


if __name__ == '__main__':
    main()
