#!/usr/bin/env python3
"""Encode a directory of images into the distillation cache (the sibling of tools/cache_prompts.py): every record of ``--cache-dir`` gets the
``latents`` (+ ``latent_size``) of the image with the same file stem, as the reference's ``ImagePrompt`` dataset reads them
(image_prompts.py:373-383), through the HIP VAE encoder.

    python tools/cache_latents.py --family flux --snapshot /path/to/FLUX.1-dev --images data/images --cache-dir data/preproc_flux

Images are cropped to multiples of 16 pixels.  ``--mode`` stores the posterior mean instead of a sample (seeded per item by ``--seed``).
"""
import argparse
import os
import pickle
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IMAGE_EXT = ('.png', '.jpg', '.jpeg', '.webp', '.bmp')


def load_image01(path: str) -> torch.Tensor:
    """-> [3, H, W] fp32 in [0, 1], cropped (top-left) to multiples of 16."""
    import numpy as np
    from PIL import Image
    a = np.asarray(Image.open(path).convert('RGB'), dtype=np.float32) / 255.0
    h, w = a.shape[0] // 16 * 16, a.shape[1] // 16 * 16
    if h == 0 or w == 0:
        raise ValueError(f'{path}: smaller than 16 x 16')
    return torch.from_numpy(np.ascontiguousarray(a[:h, :w])).permute(2, 0, 1).contiguous()


def read_record(path: str) -> dict:
    from arcflow_amd.train.data import _load_item
    return _load_item(path)


def write_record(path: str, item: dict) -> None:
    from arcflow_amd.train import zstd_io
    raw = pickle.dumps(item, protocol=pickle.HIGHEST_PROTOCOL)
    if path.endswith('.zst'):
        raw = zstd_io.compress(raw, level=3)
    tmp = f'{path}.tmp{os.getpid()}'
    with open(tmp, 'wb') as f:
        f.write(raw)
    os.replace(tmp, path)


def add_latents(encode, image_dir: str, cache_dir: str, sample: bool = True, seed: int = 0, dtype=torch.float16):
    """encode(images01 [1, 3, H, W], generator or None) -> latents [1, 16, H/8, W/8].  Returns the stems written; an image without a record raises."""
    records = {os.path.splitext(f)[0]: f for f in sorted(os.listdir(cache_dir)) if f.endswith(('.zst', '.pkl'))}
    done = []
    for fn in sorted(os.listdir(image_dir)):
        stem, ext = os.path.splitext(fn)
        if ext.lower() not in IMAGE_EXT:
            continue
        if stem not in records:
            raise KeyError(f'{fn}: no cache record {stem}.zst / {stem}.pkl under {cache_dir} (run tools/cache_prompts.py first)')
        path = os.path.join(cache_dir, records[stem])
        item = read_record(path)
        gen = torch.Generator().manual_seed(seed + len(done)) if sample else None
        lat = encode(load_image01(os.path.join(image_dir, fn))[None], gen)[0].to('cpu', dtype)
        item['latents'], item['latent_size'] = lat, tuple(lat.shape)
        item.pop('latents_scale', None)
        write_record(path, item)
        done.append(stem)
    return done


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--family', choices=['flux', 'qwen'], required=True)
    ap.add_argument('--snapshot', required=True, help='local model snapshot whose vae/ holds encoder.* weights')
    ap.add_argument('--images', required=True)
    ap.add_argument('--cache-dir', required=True)
    ap.add_argument('--mode', action='store_true', help='store the posterior mean, not a sample')
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    from arcflow_amd.pipelines.arcflux_pipeline import load_transformer_dir
    from arcflow_amd.vae import AutoencoderKLEncoder, AutoencoderKLQwenImageEncoder
    cfg, sd = load_transformer_dir(os.path.join(args.snapshot, 'vae'))
    if args.family == 'flux':
        enc = AutoencoderKLEncoder(sd, tuple(cfg.get('block_out_channels', (128, 256, 512, 512))), cfg.get('norm_num_groups', 32),
                                   cfg.get('layers_per_block', 2), cfg.get('scaling_factor', 0.3611), cfg.get('shift_factor', 0.1159))
    else:
        enc = AutoencoderKLQwenImageEncoder(sd, cfg['latents_mean'], cfg['latents_std'], cfg.get('base_dim'), tuple(cfg.get('dim_mult', (1, 2, 4, 4))),
                                            cfg.get('num_res_blocks', 2), tuple(cfg.get('temperal_downsample', (False, True, True))))
    done = add_latents(lambda im, g: enc.encode_images01(im, generator=g, sample=not args.mode), args.images, args.cache_dir,
                       sample=not args.mode, seed=args.seed)
    print(f'wrote latents into {len(done)} records of {args.cache_dir}')


if __name__ == '__main__':
    main()
