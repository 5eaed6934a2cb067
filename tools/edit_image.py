#!/usr/bin/env python3
"""Edit an image with the ArcFlow student: image-to-image (``--image``, ``--strength``) and inpainting (``--mask``, white = repaint) through
``pipe(image=..., strength=..., mask_image=...)`` of ArcFluxPipeline / ArcQwenImagePipeline.  The image is encoded by the snapshot's VAE
encoder, noised to ``--strength``, denoised in ``--nfe`` student steps and decoded; with a mask the unmasked region stays on the image's
own trajectory and the original pixels are pasted back after decoding.  Nothing is resized: the image (and the mask) must be a multiple of
16 pixels on both sides.

    python tools/edit_image.py --family flux --snapshot /path/to/FLUX.1-dev --adapter /path/to/arcflow --image in.png --mask mask.png \\
        --prompt "a red door" --strength 0.8 --out out.png

``--synthetic``: random-init weights of a reduced architecture, random prompt embeddings and a random image in latent space
(``image_latents=``; no snapshot, no VAE): writes the edited packed latents to ``--out`` with torch.save, for trying the path end to end.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_pipeline(family: str, device='cuda', seed: int = 0):
    """A reduced student (1 + 1 FLUX blocks / 2 Qwen-Image blocks, width 256) with random weights -> (pipeline, conditioning keywords)."""
    from arcflow_amd import FlowMatchEulerDiscreteScheduler, MMDiTEngine
    from arcflow_amd.pipelines import ArcFluxPipeline, ArcQwenImagePipeline
    from arcflow_amd.weights import random_packed
    joint, pooled = (128, 64) if family == 'flux' else (192, 0)
    nd, ns = (1, 1) if family == 'flux' else (2, 0)
    eng = MMDiTEngine(family, nd, ns, heads=2, joint_dim=joint, pooled_dim=pooled or 768, device=device)
    eng.bind_packed(random_packed(family, nd, ns, device, heads=2, joint_dim=joint, pooled_dim=pooled or 768, seed=seed))
    pipe = (ArcFluxPipeline if family == 'flux' else ArcQwenImagePipeline)(scheduler=FlowMatchEulerDiscreteScheduler(shift=3.2))
    pipe.transformer = eng
    g = torch.Generator().manual_seed(seed + 1)
    cond = dict(prompt_embeds=(torch.randn(1, 8, joint, generator=g) * 0.5).bfloat16())
    if family == 'flux':
        cond['pooled_prompt_embeds'] = (torch.randn(1, pooled, generator=g) * 0.5).bfloat16()
    return pipe, cond


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--family', choices=['flux', 'qwen'], required=True)
    ap.add_argument('--snapshot', help='local FLUX.1-dev / Qwen-Image snapshot (transformer/, vae/ with encoder weights, text encoders)')
    ap.add_argument('--adapter', help='ArcFlow adapter directory (load_arcflow_adapter)')
    ap.add_argument('--image', help='the image to edit (sides multiples of 16)')
    ap.add_argument('--mask', help='inpainting mask, same size: white = repaint, black = keep')
    ap.add_argument('--prompt', default='')
    ap.add_argument('--strength', type=float, default=0.8, help='in (0, 1]: 1 starts from pure noise, small values stay close to the image')
    ap.add_argument('--nfe', type=int, default=2)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', required=True)
    ap.add_argument('--synthetic', action='store_true', help='reduced random-init student, random embeddings, a random image in latent space')
    ap.add_argument('--size', type=int, nargs=2, default=[256, 256], help='--synthetic: height width')
    args = ap.parse_args(argv)
    gen = torch.Generator().manual_seed(args.seed)
    kw = dict(strength=args.strength, num_inference_steps=args.nfe, timestep_ratio=1.0 if args.nfe == 2 else 0.5, generator=gen)
    if args.synthetic:
        pipe, cond = synthetic_pipeline(args.family, seed=args.seed)
        h, w = args.size
        g = torch.Generator().manual_seed(args.seed + 2)
        x0 = torch.randn(1, (h // 16) * (w // 16), 64, generator=g) * 0.8
        mask = None
        if args.mask:
            from PIL import Image
            mask = Image.open(args.mask)
        out = pipe(image_latents=x0, mask_image=mask, height=h, width=w, output_type='latent', **cond, **kw).images
        torch.save(out.cpu(), args.out)
        print(f'wrote edited latents {tuple(out.shape)} to {args.out}  (|out - source| rel-L2 {((out.cpu() - x0).norm() / x0.norm()).item():.3f})')
        return out
    if not args.snapshot or not args.image:
        raise SystemExit('--snapshot and --image are required (or pass --synthetic)')
    from PIL import Image
    from arcflow_amd.pipelines import ArcFluxPipeline, ArcQwenImagePipeline
    pipe = (ArcFluxPipeline if args.family == 'flux' else ArcQwenImagePipeline).from_pretrained(args.snapshot)
    if args.adapter:
        pipe.load_arcflow_adapter(args.adapter)
    image = Image.open(args.image)
    mask = Image.open(args.mask) if args.mask else None
    out = pipe(prompt=args.prompt, image=image, mask_image=mask, **kw).images[0]
    out.save(args.out)
    print(f'wrote {args.out} ({out.size[0]} x {out.size[1]})')
    return out


if __name__ == '__main__':
    main()
