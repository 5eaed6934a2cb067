#!/usr/bin/env python3
"""Edit an image with the ArcFlow student: image-to-image (``--image``, ``--strength``) and inpainting (``--mask``, white = repaint) through
``pipe(image=..., strength=..., mask_image=...)`` of ArcFluxPipeline / ArcQwenImagePipeline.  The image is encoded by the snapshot's VAE
encoder, noised to ``--strength``, denoised in ``--nfe`` student steps and decoded; with a mask the unmasked region stays on the image's
own trajectory and the original pixels are pasted back after decoding.  Nothing is resized: the image (and the mask) must be a multiple of
16 pixels on both sides -- unless ``--resize`` resamples them to the call's size, or ``--padding-mask-crop N`` edits a window around the mask of a
photo of any size and writes the photo at its own size, every kept pixel byte for byte.

    python tools/edit_image.py --family flux --snapshot /path/to/FLUX.1-dev --adapter /path/to/arcflow --image in.png --mask mask.png \\
        --prompt "a red door" --strength 0.8 --out out.png

``--teacher`` also (or, without ``--adapter``, only) produces the TEACHER's edit of the same source, noise and mask through
``pipe.sample_teacher(image=..., strength=..., mask_image=...)`` in ``--steps`` steps, written beside ``--out`` as ``<out>.teacher<ext>``;
with both, the latents of the two edits are scored against each other with ``afx_sample_score`` (student = a, teacher = b): mse, rel-L2 and
cosine per sample, and the two decoded edits as written (8 bits per channel, / 255) with ``afx_sample_score`` and ``afx_image_ssim``:
``image_psnr`` and ``image_ssim``, and with ``--mask`` the same two weighted by the mask, ``repaint_image_psnr`` and ``repaint_image_ssim``
(``afx_sample_score_masked``, ``afx_image_ssim_masked``).  The teacher walks the last ``strength`` share of its schedule, the student all its steps over [strength, 0]; both
start from the same noise draw (``--seed``).

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


def score_latents(student: torch.Tensor, teacher: torch.Tensor):
    """Packed latents [B, N, 64] of the two edits -> {'latent_mse' | 'latent_rel_l2' | 'latent_cosine': per-sample list} (afx_sample_score)."""
    from arcflow_amd import ops
    from arcflow_amd.train.evaluate import metrics_from_sums
    a, b = student.to('cuda', torch.float32).contiguous(), teacher.to('cuda', torch.float32).contiguous()
    m = metrics_from_sums(ops.sample_score(a, b), a[0].numel())
    return {'latent_' + k: m[k].tolist() for k in ('mse', 'rel_l2', 'cosine')}


def score_images(student, teacher, mask=None):
    """The two decoded edits as written (PIL images of one size, 8 bits per channel) -> {'image_psnr' | 'image_ssim': per-sample list} on
    their values / 255 (afx_sample_score, afx_image_ssim; data range 1).  With ``mask`` (a PIL image, white = repaint; the mask file as
    given, its grey values / 255, stretched to the edits' size when it differs -- not the pipeline's feathered copy) also
    'repaint_image_psnr' | 'repaint_image_ssim': the same two scores weighted by the mask (afx_sample_score_masked,
    afx_image_ssim_masked).  The whole-image scores are dominated by the kept region, which both edits paste back from the source."""
    import numpy as np
    from arcflow_amd import ops
    from arcflow_amd.train.evaluate import masked_metrics_from_sums, masked_ssim_from_sums, metrics_from_sums, ssim_from_sums

    def planes(im):
        return torch.from_numpy(np.asarray(im.convert('RGB'), dtype=np.float32) / 255.0).permute(2, 0, 1)[None].contiguous().cuda()
    a, b = planes(student), planes(teacher)
    m = metrics_from_sums(ops.sample_score(a, b), a[0].numel(), data_range=1.0)
    out = {'image_psnr': m['psnr'].tolist(), 'image_ssim': ssim_from_sums(ops.image_ssim(a, b), *a.shape[1:]).tolist()}
    if mask is not None:
        grey = mask.convert('L')
        if grey.size != student.size:
            grey = grey.resize(student.size, 2)          # 2 = bilinear
        w = torch.from_numpy(np.asarray(grey, dtype=np.float32) / 255.0)[None, None].contiguous().cuda()
        out['repaint_image_psnr'] = masked_metrics_from_sums(ops.sample_score_masked(a, b, w), data_range=1.0)[0]['psnr'].tolist()
        out['repaint_image_ssim'] = masked_ssim_from_sums(ops.image_ssim_masked(a, b, w))[0].tolist()
    return out


def _teacher_path(out: str) -> str:
    root, ext = os.path.splitext(out)
    return root + '.teacher' + ext


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--family', choices=['flux', 'qwen'], required=True)
    ap.add_argument('--snapshot', help='local FLUX.1-dev / Qwen-Image snapshot (transformer/, vae/ with encoder weights, text encoders)')
    ap.add_argument('--adapter', help='ArcFlow adapter directory (load_arcflow_adapter)')
    ap.add_argument('--image', help='the image to edit (sides multiples of 16, or any size with --resize)')
    ap.add_argument('--mask', help='inpainting mask, same size: white = repaint, black = keep')
    ap.add_argument('--prompt', default='')
    ap.add_argument('--strength', type=float, default=0.8, help='in (0, 1]: 1 starts from pure noise, small values stay close to the image')
    ap.add_argument('--nfe', type=int, default=2)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', required=True)
    ap.add_argument('--synthetic', action='store_true', help='reduced random-init student, random embeddings, a random image in latent space')
    ap.add_argument('--size', type=int, nargs=2, default=[256, 256], help='--synthetic: height width')
    ap.add_argument('--teacher', action='store_true', help='also write the teacher\'s edit (sample_teacher) and score the student\'s against it')
    ap.add_argument('--steps', type=int, default=28, help='--teacher: steps of the full schedule (the last `strength` share of them runs)')
    ap.add_argument('--true-cfg-scale', type=float, default=1.0, help='--teacher: true classifier-free guidance against --negative-prompt when > 1')
    ap.add_argument('--negative-prompt', default='')
    ap.add_argument('--resize', choices=['stretch', 'crop'], help='resample --image and --mask to the call\'s size on the GPU (Lanczos-3; the mask '
                    'with the triangle filter): stretch the whole image, or crop the largest centred window of the target aspect ratio.  Without it '
                    'the image must already have the size, a multiple of 16')
    ap.add_argument('--mask-blur', type=float, default=0.0, help='sigma in output pixels of a Gaussian feather of the mask (0 = none)')
    ap.add_argument('--height', type=int, help='with --resize: the output height (default: the image\'s, rounded to a multiple of 16)')
    ap.add_argument('--width', type=int, help='with --resize: the output width')
    ap.add_argument('--padding-mask-crop', type=int, metavar='N', help='inpaint a photo of any size at its own size: edit a window around the '
                    'mask\'s bounding box, padded by N source pixels, at --height x --width (default 1024 x 1024) and paste the result back; every '
                    'pixel outside the mask keeps the photo\'s own bytes.  Needs --mask; not with --resize')
    ap.add_argument('--color-fix', choices=['adain', 'wavelet'], help='image-to-image only: match the decoded edit to --image (wavelet: its low '
                    'band; adain: its per-channel mean and deviation).  Not with --mask or --synthetic')
    args = ap.parse_args(argv)
    if args.color_fix and (args.mask or args.synthetic):
        raise SystemExit('--color-fix matches pixels to --image: not with --mask (it would undo the inpainting) or --synthetic (latents only)')
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
        mkw = dict(resize=args.resize, mask_blur=args.mask_blur) if mask is not None else {}        # latents are not resampled: only a mask is
        out = pipe(image_latents=x0, mask_image=mask, height=h, width=w, output_type='latent', **cond, **kw, **mkw).images
        torch.save(out.cpu(), args.out)
        print(f'wrote edited latents {tuple(out.shape)} to {args.out}  (|out - source| rel-L2 {((out.cpu() - x0).norm() / x0.norm()).item():.3f})')
        if args.teacher:
            from arcflow_amd import MMDiTEngine
            from arcflow_amd.weights import random_packed
            eng = pipe.transformer
            nd, ns = (1, 1) if args.family == 'flux' else (2, 0)
            joint, pooled = (128, 64) if args.family == 'flux' else (192, 768)
            pipe._teacher = MMDiTEngine(args.family, nd, ns, heads=2, joint_dim=joint, pooled_dim=pooled, teacher_head=True, device=eng.device)
            pipe._teacher.bind_packed(random_packed(args.family, nd, ns, eng.device, heads=2, joint_dim=joint, pooled_dim=pooled, seed=args.seed,
                                                    teacher=True))
            tea = pipe.sample_teacher(image_latents=x0, mask_image=mask, height=h, width=w, output_type='latent', strength=args.strength,
                                      num_inference_steps=args.steps, true_cfg_scale=1.0, generator=torch.Generator().manual_seed(args.seed),
                                      **cond, **mkw).images
            torch.save(tea.cpu(), _teacher_path(args.out))
            scores = score_latents(out, tea)
            print(f'wrote the teacher\'s edit ({args.steps} steps) to {_teacher_path(args.out)}; student vs teacher: {scores}')
            return out, tea, scores
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
    student = pipe.transformer is not None and not pipe.transformer.teacher_head
    if not student and not args.teacher:
        raise SystemExit('no ArcFlow student loaded: pass --adapter, or --teacher for the base model\'s own edit')
    out = lat = None
    crop = args.padding_mask_crop
    if crop is not None and (mask is None or args.resize):
        raise SystemExit('--padding-mask-crop needs --mask and excludes --resize')
    if (args.height or args.width) and not args.resize and crop is None:
        raise SystemExit('--height / --width need --resize or --padding-mask-crop (without them the call has the image\'s size)')
    kw.update(resize=args.resize, mask_blur=args.mask_blur if mask is not None else 0.0, height=args.height, width=args.width)
    if crop is not None:
        kw.update(padding_mask_crop=crop)             # the result has the photo's size; there are no latents of that size to score
    if student:
        lat = None if crop is not None else pipe(prompt=args.prompt, image=image, mask_image=mask, output_type='latent', **kw).images
        out = pipe(prompt=args.prompt, image=image, mask_image=mask, color_fix=args.color_fix,
                   **dict(kw, generator=torch.Generator().manual_seed(args.seed))).images[0]
        out.save(args.out)
        print(f'wrote {args.out} ({out.size[0]} x {out.size[1]})')
    if args.teacher:
        tkw = dict(prompt=args.prompt, image=image, mask_image=mask, strength=args.strength, num_inference_steps=args.steps,
                   true_cfg_scale=args.true_cfg_scale, negative_prompt=args.negative_prompt if args.true_cfg_scale > 1.0 else None,
                   resize=kw['resize'], mask_blur=kw['mask_blur'], height=args.height, width=args.width, padding_mask_crop=crop)
        tlat = None if crop is not None else pipe.sample_teacher(output_type='latent', generator=torch.Generator().manual_seed(args.seed), **tkw).images
        tea = pipe.sample_teacher(generator=torch.Generator().manual_seed(args.seed), color_fix=args.color_fix, **tkw).images[0]
        tea.save(_teacher_path(args.out))
        print(f'wrote the teacher\'s edit ({args.steps} steps) to {_teacher_path(args.out)}')
        if student:
            print(f'student vs teacher: {dict(score_latents(lat, tlat) if crop is None else {}, **score_images(out, tea, mask))}')
        out = tea if out is None else out
    return out


if __name__ == '__main__':
    main()
