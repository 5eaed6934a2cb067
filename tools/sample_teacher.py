#!/usr/bin/env python3
"""Sample the TEACHER into the distillation cache: every record of ``--cache-dir`` (tools/cache_prompts.py, or written here from
``--prompts``) gets the ``latents`` (+ ``latent_size``) of a teacher sample for its prompt -- the third source of latents for the
data mode next to encoded images (tools/cache_latents.py) and the reference's own caches.  Euler ODE steps, or with
``--sampler FlowSDE --h <float | inf>`` the stochastic steps of FlowSDEScheduler (diverse latents for one prompt), with optional true
classifier-free guidance (arcflow_amd.teacher.TeacherSampler; GaussianFlow.forward_test in the reference).

    python tools/sample_teacher.py --family flux --snapshot /path/to/FLUX.1-dev --prompts prompts.txt --cache-dir data/teacher_flux
    python tools/train.py examples/flux_distill_data_2nfe.py --transformer-dir /path/to/FLUX.1-dev/transformer --data-dir data/teacher_flux

``--image`` (+ ``--mask``, white = repaint; ``--strength``) conditions every sample on one source image: the teacher's image-to-image /
inpainting (TeacherSampler ``x0`` / ``mask`` / ``strength``), so that edit-conditioned teacher latents can be cached too.  The image is
encoded by the snapshot's VAE encoder and must match every record's ``latent_size`` (8 pixels per latent pixel; nothing is resized).  A
``.pt`` file is read with torch.load instead: a tensor [16, H, W] (or [1, 16, H, W]) of latents for ``--image``, [H, W] in [0, 1] at
latent resolution for ``--mask`` -- which is all ``--synthetic`` can take, having no VAE.

``--synthetic``: random-init weights of a reduced architecture and random prompt embeddings (no snapshot, no text encoders): writes
``--count`` complete records, for trying the data path end to end.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cache_latents import read_record, write_record          # noqa: E402  (the cache writer is the image tool's)


def unpack(latents: torch.Tensor, hp: int, wp: int) -> torch.Tensor:
    """[B, hp wp, 64] packed tokens -> [B, 16, 2 hp, 2 wp] latents (channel = c*4 + ph*2 + pw)."""
    b = latents.shape[0]
    return latents.view(b, hp, wp, 16, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(b, 16, 2 * hp, 2 * wp)


def pack(latents: torch.Tensor) -> torch.Tensor:
    """[B, 16, 2 hp, 2 wp] latents -> [B, hp wp, 64] packed tokens: the inverse of ``unpack``."""
    b, c, h, w = latents.shape
    return latents.view(b, c, h // 2, 2, w // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(b, (h // 2) * (w // 2), c * 4).contiguous()


def load_edit(image: str, mask=None, encoder=None, device='cuda'):
    """``--image`` / ``--mask`` -> dict(x0 [1, N, 64] packed fp32 latents, mask [1, N, 4] or None, size (16, H, W)).  ``.pt`` files hold
    latent-space tensors; anything else is an image file, which needs ``encoder`` (pipe.vae.encoder)."""
    from arcflow_amd.schedule import mask_to_tokens
    if image.endswith('.pt'):
        lat = torch.load(image).to(torch.float32)
        lat = lat[None] if lat.dim() == 3 else lat
        if lat.dim() != 4 or lat.shape[1] != 16 or lat.shape[2] % 2 or lat.shape[3] % 2:
            raise SystemExit(f'--image {image}: need latents [16, H, W] with even H, W, got {tuple(lat.shape)}')
        x0 = pack(lat).to(device)
        _, _, h, w = lat.shape
    else:
        if encoder is None:
            raise SystemExit('--image needs a snapshot whose vae/ holds encoder weights (or a .pt file of latents)')
        from PIL import Image
        from arcflow_amd.pipelines.edit_inputs import images01
        img = images01(Image.open(image))
        if img.shape[2] % 16 or img.shape[3] % 16:
            raise SystemExit(f'--image {image}: sides must be multiples of 16, got {img.shape[2]} x {img.shape[3]}')
        x0 = encoder.encode_images01(img, sample=False, packed=True).to(torch.float32)
        h, w = img.shape[2] // 8, img.shape[3] // 8
    tokens = None
    if mask is not None:
        if mask.endswith('.pt'):
            m = torch.load(mask).to(torch.float32).reshape(1, h, w)
            tokens = m.view(1, h // 2, 2, w // 2, 2).permute(0, 1, 3, 2, 4).reshape(1, (h // 2) * (w // 2), 4).contiguous().to(device)
        else:
            from PIL import Image
            from arcflow_amd.pipelines.edit_inputs import images01
            m = images01(Image.open(mask), 'mask', 1)
            if tuple(m.shape[2:]) != (8 * h, 8 * w):
                raise SystemExit(f'--mask {mask} is {m.shape[2]} x {m.shape[3]}, the image is {8 * h} x {8 * w}')
            tokens = mask_to_tokens(m.to(device), h // 2, w // 2)
    return dict(x0=x0, mask=tokens, size=(16, h, w))


def add_teacher_latents(sampler, cache_dir: str, negative=None, seed: int = 0, dtype=torch.float16, device='cuda', edit=None,
                        strength: float = 1.0):
    """sampler(cond, noise [1, N, 64]) -> packed latents.  Every record of ``cache_dir`` is sampled at its own ``latent_size`` from
    noise seeded with ``seed + index`` (the same generator goes on to the step draws of a stochastic sampler) and rewritten with
    ``latents``.  negative: prompt_embed_kwargs of the negative prompt (true
    CFG).  edit (``load_edit``): every record is an edit of that one source image at ``strength``.  Returns {file name: the fp32 latents [16, H, W] before the cast to ``dtype``}."""
    from arcflow_amd.train import data
    ds = data.PromptEmbedCache(cache_dir)
    done = {}
    for i, fn in enumerate(ds.files):
        item = ds[i]
        if negative is not None:
            item['negative_prompt_embed_kwargs'] = negative
        cond = data.collate([item], device=device)
        _, h, w = item['latent_size']
        gen = torch.Generator().manual_seed(seed + i)
        noise = torch.randn(1, cond['hp'] * cond['wp'], 64, generator=gen).to(device)
        kw = {}
        if edit is not None:
            if tuple(edit['size']) != (16, h, w):
                raise SystemExit(f'{fn}: latent_size {tuple(item["latent_size"])} but --image gives {edit["size"]}')
            kw = dict(x0=edit['x0'], mask=edit['mask'], strength=strength)
        lat = unpack(sampler(cond, noise, generator=gen, **kw), cond['hp'], cond['wp'])[0].float().cpu()
        assert tuple(lat.shape) == (16, h, w)
        path = os.path.join(cache_dir, fn)
        rec = read_record(path)
        rec['latents'], rec['latent_size'] = lat.to(dtype), tuple(lat.shape)
        rec.pop('latents_scale', None)
        write_record(path, rec)
        done[fn] = lat
    return done


def write_synthetic_records(cache_dir: str, family: str, count: int, joint_dim: int, pooled_dim: int, latent_size, seed: int, text_len: int = 8):
    """``count`` records with random prompt embeddings in the cache layout (arcflow_amd/train/prompts.py write_cache)."""
    os.makedirs(cache_dir, exist_ok=True)
    g = torch.Generator().manual_seed(seed)
    for i in range(count):
        kw = dict(encoder_hidden_states=(torch.randn(text_len, joint_dim, generator=g) * 0.5).half())
        if family == 'flux':
            kw['pooled_projections'] = (torch.randn(pooled_dim, generator=g) * 0.5).half()
        else:
            kw['encoder_hidden_states_mask'] = torch.ones(text_len, dtype=torch.long)
        write_record(os.path.join(cache_dir, f'{i:08d}.pkl'), dict(prompt=f'synthetic {i}', prompt_embed_kwargs=kw, latent_size=tuple(latent_size)))


def synthetic_engine(family: str, device='cuda', seed: int = 0):
    """A reduced teacher (1 + 1 FLUX blocks / 2 Qwen-Image blocks, width 256) with random weights -> (engine, joint_dim, pooled_dim)."""
    from arcflow_amd import MMDiTEngine
    from arcflow_amd.weights import random_packed
    joint, pooled = (128, 64) if family == 'flux' else (192, 0)
    nd, ns = (1, 1) if family == 'flux' else (2, 0)
    eng = MMDiTEngine(family, nd, ns, heads=2, joint_dim=joint, pooled_dim=pooled or 768, teacher_head=True, device=device)
    eng.bind_packed(random_packed(family, nd, ns, device, heads=2, joint_dim=joint, pooled_dim=pooled or 768, seed=seed, teacher=True))
    return eng, joint, pooled


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--family', choices=['flux', 'qwen'], required=True)
    ap.add_argument('--cache-dir', required=True, help='prompt cache to add the latents to (created from --prompts / --synthetic when it does not exist)')
    ap.add_argument('--snapshot', help='local plain FLUX.1-dev / Qwen-Image snapshot (transformer/ with proj_out; text encoders for --prompts)')
    ap.add_argument('--prompts', help='text file, one prompt per line: encoded into --cache-dir first')
    ap.add_argument('--negative-prompt', default=None, help='negative prompt of true CFG (needs the snapshot\'s text encoders)')
    ap.add_argument('--negative-prompt-embeds', help='torch.load-able embeddings of the negative prompt (as tools/train.py takes them)')
    ap.add_argument('--synthetic', action='store_true', help='reduced random-init teacher and random prompt embeddings')
    ap.add_argument('--count', type=int, default=4, help='--synthetic: records to write')
    ap.add_argument('--latent-size', type=int, nargs=3, default=[16, 128, 128])
    ap.add_argument('--steps', type=int, default=28)
    ap.add_argument('--guidance-scale', type=float, default=3.5, help='distilled guidance embedding (FLUX)')
    ap.add_argument('--true-cfg-scale', type=float, default=1.0)
    ap.add_argument('--guidance-interval', type=float, nargs=2, default=None)
    ap.add_argument('--orthogonal-guidance', action='store_true')
    ap.add_argument('--shift', type=float, default=3.2)
    ap.add_argument('--sampler', choices=['FlowEulerODE', 'FlowSDE', 'UniPC'], default='FlowEulerODE')
    ap.add_argument('--solver-order', type=int, choices=[1, 2, 3], default=None, help='--sampler UniPC: order of the multistep solver (default 2)')
    ap.add_argument('--solver-type', choices=['bh1', 'bh2'], default=None, help='--sampler UniPC: the B(h) of the solver (default bh2)')
    ap.add_argument('--h', type=lambda v: v if v == 'inf' else float(v), default=None,
                    help='--sampler FlowSDE: noise strength, a float (0 = the ODE; default 1.0) or inf (re-noise the clean prediction completely)')
    ap.add_argument('--image', help='source image of an edit (sides multiples of 16), or a .pt file of its latents [16, H, W]')
    ap.add_argument('--mask', help='inpainting mask of --image: an image of its size (white = repaint), or a .pt file [H, W] in [0, 1] per latent pixel')
    ap.add_argument('--strength', type=float, default=1.0, help='--image: in (0, 1], the share of the --steps schedule that runs (1 = all of it)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--max-sequence-length', type=int, default=512)
    args = ap.parse_args(argv)
    from arcflow_amd import TeacherSampler
    from arcflow_amd.train import data
    dev = 'cuda'
    negative = None
    encoder = None
    if args.mask and not args.image:
        raise SystemExit('--mask needs --image')
    if args.mask and args.sampler == 'UniPC':
        raise SystemExit('--mask: not with --sampler UniPC (inpainting stays with FlowEulerODE and FlowSDE)')
    if args.synthetic:
        engine, joint, pooled = synthetic_engine(args.family, dev, args.seed)
        if not os.path.isdir(args.cache_dir) or not os.listdir(args.cache_dir):
            write_synthetic_records(args.cache_dir, args.family, args.count, joint, pooled, args.latent_size, args.seed)
        if args.true_cfg_scale > 1.0:
            g = torch.Generator().manual_seed(args.seed + 977)
            negative = dict(encoder_hidden_states=torch.randn(8, joint, generator=g) * 0.5)
            if pooled:
                negative['pooled_projections'] = torch.randn(pooled, generator=g) * 0.5
    else:
        if not args.snapshot:
            raise SystemExit('--snapshot is required (or pass --synthetic)')
        from arcflow_amd.pipelines import ArcFluxPipeline, ArcQwenImagePipeline
        pipe = (ArcFluxPipeline if args.family == 'flux' else ArcQwenImagePipeline).from_pretrained(args.snapshot)
        engine = pipe._teacher_engine()
        encoder = getattr(pipe.vae, 'encoder', None)
        if args.prompts:
            from arcflow_amd.train.prompts import PromptEncoder, write_cache
            enc = PromptEncoder(args.family, pipe, max_sequence_length=args.max_sequence_length)
            with open(args.prompts, encoding='utf-8') as f:
                write_cache(enc, [l.rstrip('\n') for l in f if l.strip()], args.cache_dir, tuple(args.latent_size))
            if args.negative_prompt is not None:
                e = enc.encode([args.negative_prompt])
                negative = {k: v[0].float().cpu() for k, v in e.items() if k != 'encoder_hidden_states_mask'}
                if 'encoder_hidden_states_mask' in e:
                    negative['encoder_hidden_states'] = negative['encoder_hidden_states'][e['encoder_hidden_states_mask'][0].bool().cpu()]
        if args.negative_prompt_embeds:
            negative = data.PromptEmbedCache(args.cache_dir, negative_prompt_embeds_path=args.negative_prompt_embeds).negative_prompt_embed_kwargs
    if args.true_cfg_scale > 1.0 and negative is None:
        raise SystemExit('--true-cfg-scale > 1 needs --negative-prompt (with --prompts) or --negative-prompt-embeds')
    sampler = TeacherSampler(engine, args.steps, guidance_scale=args.true_cfg_scale, distilled_guidance=args.guidance_scale,
                             guidance_interval=args.guidance_interval, orthogonal_guidance=args.orthogonal_guidance, shift=args.shift,
                             sampler=args.sampler,
                             **{k: v for k, v in dict(h=args.h, solver_order=args.solver_order, solver_type=args.solver_type).items() if v is not None})
    edit = load_edit(args.image, args.mask, encoder, dev) if args.image else None
    done = add_teacher_latents(sampler, args.cache_dir, negative, args.seed, device=dev, edit=edit, strength=args.strength)
    print(f'wrote teacher latents into {len(done)} records of {args.cache_dir}')
    return done


if __name__ == '__main__':
    main()
