#!/usr/bin/env python3
"""Rewrite a community LoRA file (Kohya / ComfyUI key layout, with or without DoRA magnitudes) in the diffusers layout.

    python tools/convert_lora.py IN.safetensors OUT.safetensors --family flux|qwen [--transformer-config config.json] [--teacher]

OUT holds ``transformer.<module>.lora_A.weight`` / ``lora_B.weight`` / ``alpha`` per diffusers linear (fused qkv / linear1 tensors split by rows, each
part with its own copy of ``lora_A``) and ``transformer.<module>.lora_magnitude_vector`` where the file has a DoRA magnitude; text-encoder tensors
are left out.  LyCORIS LoHa / LoKr modules come out under the diffusers module name with LyCORIS' own tensor names
(``transformer.<module>.hada_w1_a`` ..., ``lokr_w1`` ...; the parts of a fused LoKr share both factors and carry ``lokr_row0``, their first row in the
fused delta) -- a layout this project's loader reads; other software may not.  ``--transformer-config`` is the transformer's ``config.json`` (default: the released FLUX.1-dev / Qwen-Image sizes); ``--teacher``
keeps ``final_layer.linear`` as ``proj_out``, which the ArcFlow student does not have.  ``load_lora_weights`` does the same conversion in memory
(``arcflow_amd/pipelines/lora_formats.py``, which also says what is not pinned: the BFL <-> diffusers table is restated from memory); this tool
is for handing the result to other software.  Runs on the CPU."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def convert_file(src: str, dst: str, family: str, config=None, student: bool = True):
    from safetensors import safe_open
    from safetensors.torch import save_file
    from arcflow_amd.pipelines.lora_formats import convert_community_lora
    with safe_open(src, framework='pt', device='cpu') as h:
        sd = {k: h.get_tensor(k) for k in h.keys()}
        meta = h.metadata() or {}
    out, mags, skipped = convert_community_lora(sd, family, config or {}, student=student)
    out = {k: v.clone().contiguous() for k, v in out.items()}                      # safetensors refuses tensors that share memory
    for m, v in mags.items():
        out[f'transformer.{m}.lora_magnitude_vector'] = v.contiguous()
    save_file(out, dst, metadata=meta)
    return out, skipped


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('src')
    ap.add_argument('dst')
    ap.add_argument('--family', required=True, choices=['flux', 'qwen'])
    ap.add_argument('--transformer-config')
    ap.add_argument('--teacher', action='store_true')
    a = ap.parse_args(argv)
    config = None
    if a.transformer_config:
        with open(a.transformer_config) as f:
            config = json.load(f)
    out, skipped = convert_file(a.src, a.dst, a.family, config, student=not a.teacher)
    n_mod = sum(k.endswith('.lora_A.weight') for k in out)
    n_mag = sum(k.endswith('.lora_magnitude_vector') for k in out)
    n_loha = sum(k.endswith('.hada_w1_a') for k in out)
    n_lokr = sum(k.endswith(('.lokr_w1', '.lokr_w1_a')) for k in out)
    print(f'{a.dst}: {n_mod} adapted linears, {n_mag} DoRA magnitudes, {n_loha} LoHa and {n_lokr} LoKr linears, {len(skipped)} tensors skipped')


if __name__ == '__main__':
    main()
