"""Community LoRA layouts -> the diffusers / peft layout ``arcflow_loader.parse_lora_state_dict`` accepts, on the host.

Three things arrive here (``needs_conversion`` decides; ``load_lora_weights`` and ``tools/convert_lora.py`` call ``convert_community_lora``):

* Kohya / ComfyUI files with BFL module names (FLUX only), underscored (``lora_unet_double_blocks_3_img_attn_qkv.lora_down.weight``) or dotted
  (``diffusion_model.double_blocks.3.img_attn.qkv.lora_A.weight``), whose fused tensors (qkv, ``linear1``) cover several diffusers linears;
* Kohya-style files with diffusers module names written with underscores (``lora_unet_transformer_blocks_0_attn_to_q``,
  ``lora_transformer_single_transformer_blocks_7_proj_mlp``), either family;
* DoRA magnitudes in any layout: ``<module>.dora_scale`` of shape [O], [O, 1] or [1, O], ``<module>.lora_magnitude_vector[.weight]``, and peft's
  form with an adapter name, ``<module>.lora_magnitude_vector.<adapter>.weight``.

A fused tensor becomes ONE ``lora_A`` shared by its parts plus row slices of ``lora_up`` (row-wise concatenated, the parts' ``B_m @ A`` are
``lora_up @ lora_down`` exactly); the module's ``alpha`` goes to every part and a fused magnitude is split by the same rows.  The slice sizes
come from ``weights.expected_transformer_keys``.  A ``lora_down`` of rank 3r with a block-diagonal ``lora_up`` (Kohya's ``split_qkv``) needs
no special case: the product is the same.  Underscored names are resolved by exact lookup in ``{name.replace('.', '_'): name}`` built from the
modules the transformer has, never by pattern: ``to_out_0`` / ``net_0_proj`` cannot be split into words any other way.

NOT PINNED: the BFL <-> diffusers correspondence below is diffusers' own conversion as recalled (the q, k, v, mlp order of the fused tensors,
the scale-before-shift swap of ``final_layer.adaLN_modulation.1``).  One refinement of the table this was built from: it names ``vector_in`` and
``guidance_in`` as wholes, here they are taken as BFL's two-layer MLPEmbedder like ``time_in``: ``vector_in.in_layer`` / ``.out_layer`` ->
``text_embedder.linear_1`` / ``linear_2``, the same for ``guidance_in``; a bare ``vector_in`` key resolves to nothing and raises.  No third-party library here can check it and no published checkpoint
has been loaded; the tests check this module against itself (products, row ranges, names) and nothing more.

Not supported, refused by name: LoHa (``hada_w*``), LoKr (``lokr_w*``), full differences (``diff`` / ``diff_b``) and convolution LoRAs
(4-D tensors, ``.lora_mid.``).  A magnitude taken over the input axis (LyCORIS ``[1, I]`` with I != O) does not have O elements and is refused."""
from __future__ import annotations

import warnings
from typing import Dict, List, Optional, Tuple

import torch

COMMUNITY_PREFIXES = ('lora_unet_', 'lora_transformer_', 'lora_te', 'diffusion_model.')
MAGNITUDE_SUFFIXES = ('.dora_scale', '.lora_magnitude_vector', '.lora_magnitude_vector.weight')
_SLOT = {'.lora_down.weight': 'A', '.lora_A.weight': 'A', '.lora_up.weight': 'B', '.lora_B.weight': 'B', '.alpha': 'alpha'}
_LYCORIS = 'LoHa (hada_w*), LoKr (lokr_w*), diff / diff_b and conv / .lora_mid. tensors are LyCORIS families that are not supported'


def _magnitude_stem(k: str) -> Optional[str]:
    """The module part of a magnitude key, or None: ``<module>.dora_scale``, ``<module>.lora_magnitude_vector[.weight]`` and peft's form with an
    adapter name, ``<module>.lora_magnitude_vector.<adapter>.weight`` (as ``lora_A.<adapter>.weight`` is accepted by the parser)."""
    for suf in MAGNITUDE_SUFFIXES:
        if k.endswith(suf):
            return k[:-len(suf)]
    stem, sep, tail = k.partition('.lora_magnitude_vector.')
    if sep and tail.endswith('.weight') and '.' not in tail[:-len('.weight')]:
        return stem
    return None


def needs_conversion(sd: Dict[str, torch.Tensor]) -> bool:
    return any(k.startswith(COMMUNITY_PREFIXES) or _magnitude_stem(k) is not None for k in sd)


def bfl_modules(cfg: Dict, student: bool = True) -> Dict[str, Tuple[Optional[List[str]], bool]]:
    """FLUX: BFL module name (dotted) -> (the diffusers modules its rows cover in order, swap the two row halves first); the modules are None
    for ``final_layer.linear`` of the student, which has no ``proj_out``."""
    t: Dict[str, Tuple[Optional[List[str]], bool]] = {}
    for n in range(cfg.get('num_layers', 19)):
        b, d = f'double_blocks.{n}.', f'transformer_blocks.{n}.'
        t[b + 'img_attn.qkv'] = ([d + 'attn.to_q', d + 'attn.to_k', d + 'attn.to_v'], False)
        t[b + 'txt_attn.qkv'] = ([d + 'attn.add_q_proj', d + 'attn.add_k_proj', d + 'attn.add_v_proj'], False)
        for src, dst in (('img_attn.proj', 'attn.to_out.0'), ('txt_attn.proj', 'attn.to_add_out'), ('img_mlp.0', 'ff.net.0.proj'),
                         ('img_mlp.2', 'ff.net.2'), ('txt_mlp.0', 'ff_context.net.0.proj'), ('txt_mlp.2', 'ff_context.net.2'),
                         ('img_mod.lin', 'norm1.linear'), ('txt_mod.lin', 'norm1_context.linear')):
            t[b + src] = ([d + dst], False)
    for n in range(cfg.get('num_single_layers', 38)):
        b, d = f'single_blocks.{n}.', f'single_transformer_blocks.{n}.'
        t[b + 'linear1'] = ([d + 'attn.to_q', d + 'attn.to_k', d + 'attn.to_v', d + 'proj_mlp'], False)
        t[b + 'linear2'] = ([d + 'proj_out'], False)
        t[b + 'modulation.lin'] = ([d + 'norm.linear'], False)
    e = 'time_text_embed.'
    for src, dst in (('img_in', 'x_embedder'), ('txt_in', 'context_embedder'), ('time_in.in_layer', e + 'timestep_embedder.linear_1'),
                     ('time_in.out_layer', e + 'timestep_embedder.linear_2'), ('vector_in.in_layer', e + 'text_embedder.linear_1'),
                     ('vector_in.out_layer', e + 'text_embedder.linear_2')):
        t[src] = ([dst], False)
    if cfg.get('guidance_embeds', True):
        t['guidance_in.in_layer'] = ([e + 'guidance_embedder.linear_1'], False)
        t['guidance_in.out_layer'] = ([e + 'guidance_embedder.linear_2'], False)
    t['final_layer.adaLN_modulation.1'] = (['norm_out.linear'], True)          # diffusers stores scale before shift there
    t['final_layer.linear'] = (None if student else ['proj_out'], False)
    return t


def _split_key(k: str):
    """-> (everything before the suffix, slot 'A' | 'B' | 'alpha' | 'm') or (k, None)."""
    if _magnitude_stem(k) is not None:
        return _magnitude_stem(k), 'm'
    for suf, slot in _SLOT.items():
        if k.endswith(suf):
            return k[:-len(suf)], slot
    return k, None


def _refuse_lycoris(k: str, v) -> None:
    tail = k.rsplit('.', 2)
    if ('hada_w' in k or 'lokr_w' in k or '.lora_mid.' in k or tail[-1] in ('diff', 'diff_b')
            or (k.endswith('.weight') and 'lora_' in k and getattr(v, 'dim', lambda: 2)() > 2)):
        raise ValueError(f'{k!r}: {_LYCORIS}')


def _magnitude(k: str, v: torch.Tensor) -> torch.Tensor:
    if not (v.dim() == 1 or (v.dim() == 2 and 1 in v.shape)):
        raise ValueError(f'{k!r}: a DoRA magnitude has shape [O], [O, 1] or [1, O], got {tuple(v.shape)}')
    return v.reshape(-1).float()


def convert_community_lora(sd: Dict[str, torch.Tensor], family: str, transformer_config: Dict, student: bool = True):
    """-> (state dict in the layout ``parse_lora_state_dict`` accepts, {diffusers module: fp32 [O] DoRA magnitude}, [skipped keys]).

    Keys already in the diffusers / peft layout pass through untouched (their magnitude keys move to the second result).  ``lora_te*`` keys
    and, for the student, ``final_layer.linear`` are skipped with ONE warning; a key that resolves to no linear of the transformer, and any
    LyCORIS tensor (module docstring), raises ValueError naming the key.  The BFL <-> diffusers table (``bfl_modules``) is diffusers'
    conversion as recalled: parity with diffusers is NOT pinned by anything in this repository."""
    from ..weights import expected_transformer_keys, packed_row_slices
    shapes = expected_transformer_keys(family, transformer_config, student)
    linears = list(packed_row_slices(family, transformer_config, student))
    dotted: Dict[str, Tuple[Optional[List[str]], bool]] = {n: ([n], False) for n in linears}
    if family == 'flux':
        dotted.update(bfl_modules(transformer_config, student))
    underscored = {n.replace('.', '_'): n for n in dotted}

    out: Dict[str, torch.Tensor] = {}
    mags: Dict[str, torch.Tensor] = {}
    skipped: List[str] = []
    fused: Dict[str, Dict] = {}                     # source module (dotted) -> its tensors, in arrival order
    n_te = n_head = 0
    for k, v in sd.items():
        _refuse_lycoris(k, v)
        if k.startswith('lora_te'):
            skipped.append(k)
            n_te += 1
            continue
        stem, slot = _split_key(k)
        if k.startswith(('lora_unet_', 'lora_transformer_')):
            token = stem[len('lora_unet_'):] if k.startswith('lora_unet_') else stem[len('lora_transformer_'):]
            name = underscored.get(token)
        elif k.startswith('diffusion_model.'):
            name = stem[len('diffusion_model.'):]
            name = name if name in dotted else None
        else:                                       # diffusers / peft layout: only the magnitudes are taken out
            if slot == 'm':
                mags[stem[len('transformer.'):] if stem.startswith('transformer.') else stem] = _magnitude(k, v)
            else:
                out[k] = v
            continue
        if slot is None:
            raise ValueError(f'{k!r} is not a LoRA key (expected <module>.lora_down/lora_up.weight, .lora_A/lora_B.weight, .alpha, .dora_scale '
                             f'or .lora_magnitude_vector[.weight])')
        if name is None:
            raise ValueError(f'{k!r}: the {family} transformer has no module for it (neither a BFL nor a diffusers module name)')
        if dotted[name][0] is None:
            skipped.append(k)
            n_head += 1
            continue
        entry = fused.setdefault(name, dict(A=None, B=None, alpha=None, m=None))
        if entry[slot] is not None:
            raise ValueError(f'{k!r}: a second {slot} tensor for module {name!r}')
        entry[slot] = _magnitude(k, v) if slot == 'm' else v

    for name, e in fused.items():
        parts, swap = dotted[name]
        if e['A'] is None or e['B'] is None:
            raise ValueError(f'LoRA module {name!r}: lora_down / lora_up pair is incomplete')
        sizes = [shapes[p + '.weight'][0] for p in parts]
        up, m = e['B'], e['m']
        if up.dim() != 2 or up.shape[0] != sum(sizes):
            raise ValueError(f'LoRA module {name!r}: lora_up {tuple(up.shape)} does not have the {sum(sizes)} rows of {parts}')
        if m is not None and m.numel() != sum(sizes):
            raise ValueError(f'LoRA module {name!r}: a DoRA magnitude of {m.numel()} elements for {sum(sizes)} output rows')
        if swap:
            h = sum(sizes) // 2
            up = torch.cat([up[h:], up[:h]])
            m = None if m is None else torch.cat([m[h:], m[:h]])
        r0 = 0
        for p, n in zip(parts, sizes):
            ka, kb = f'transformer.{p}.lora_A.weight', f'transformer.{p}.lora_B.weight'
            if ka in out or kb in out:
                raise ValueError(f'LoRA module {name!r}: {p!r} is adapted twice in this file')
            out[ka], out[kb] = e['A'], up[r0:r0 + n]
            if e['alpha'] is not None:
                out[f'transformer.{p}.alpha'] = e['alpha']
            if m is not None:
                mags[p] = m[r0:r0 + n].contiguous()
            r0 += n
    if skipped:
        parts = []
        if n_te:
            parts.append(f'{n_te} text-encoder LoRA tensors were skipped: only transformer LoRAs are applied.')
        if n_head:
            parts.append(f'{n_head} `final_layer.linear` tensors were skipped: the ArcFlow student has no `proj_out`.')
        warnings.warn('  '.join(parts))
    return out, mags, skipped
