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

LyCORIS LoHa and LoKr (under every module spelling above; their tensors carry no ``.weight`` suffix):

* LoHa, ``<module>.hada_w1_a`` [O, r1], ``hada_w1_b`` [r1, I], ``hada_w2_a`` [O, r2], ``hada_w2_b`` [r2, I]: delta = (w1_a w1_b) (*) (w2_a w2_b) element by
  element, factor ``alpha / r1`` (1 without ``alpha``).  A fused tensor shares ``w1_b`` / ``w2_b`` among its parts, which take row slices of ``w1_a`` /
  ``w2_a``: the element-wise product of row slices is the row slice of the element-wise product.  The swapped final modulation swaps their row halves.
* LoKr, ``<module>.lokr_w1`` [a, b] or ``lokr_w1_a`` [a, r] + ``lokr_w1_b`` [r, b], and the same for ``lokr_w2`` [c, d]: delta = kron(w1, w2), i.e.
  delta[p c + q, u d + v] = w1[p, u] w2[q, v], a c = O, b d = I.  Factor ``alpha / r`` with r the rank of a low-rank factor (w2's when both are
  low-rank), 1 with both factors dense or without ``alpha`` (``lycoris_factor``).  A Kronecker product cannot be split by rows in general, so a
  fused tensor hands BOTH factors to every part together with ``<module>.lokr_row0``, an integer scalar: the part's first row in the fused delta (0 when
  the key is absent).  On ``final_layer.adaLN_modulation.1`` (row halves swapped) a LoKr is refused.

They are emitted under the diffusers module name with LyCORIS' own tensor names plus ``alpha``; ``lycoris_entry`` groups them for
``parse_lora_state_dict``; one module holds one kind per file.  NOT PINNED either: these are LyCORIS' / ComfyUI's rules restated from memory --
neither library is installed here and no published LoHa / LoKr file was at hand.

Not supported, refused by key: Tucker / convolution tensors (``hada_t1``, ``hada_t2``, ``lokr_t2``, 4-D tensors, ``.lora_mid.``), full differences
(``diff`` / ``diff_b``), a DoRA magnitude on a LoHa / LoKr module.  A magnitude taken over the input axis (LyCORIS ``[1, I]`` with I != O) does not
have O elements and is refused."""
from __future__ import annotations

import warnings
from typing import Dict, List, Optional, Tuple

import torch

COMMUNITY_PREFIXES = ('lora_unet_', 'lora_transformer_', 'lora_te', 'diffusion_model.')
MAGNITUDE_SUFFIXES = ('.dora_scale', '.lora_magnitude_vector', '.lora_magnitude_vector.weight')
_SLOT = {'.lora_down.weight': 'A', '.lora_A.weight': 'A', '.lora_up.weight': 'B', '.lora_B.weight': 'B', '.alpha': 'alpha'}
_LYCORIS = 'Tucker (hada_t*, lokr_t2), diff / diff_b and conv / .lora_mid. / 4-D tensors are LyCORIS families that are not supported'
LOHA_SLOTS = ('hada_w1_a', 'hada_w1_b', 'hada_w2_a', 'hada_w2_b')
LOKR_SLOTS = ('lokr_w1', 'lokr_w1_a', 'lokr_w1_b', 'lokr_w2', 'lokr_w2_a', 'lokr_w2_b')
LOKR_ROW0 = 'lokr_row0'
_TUCKER = ('hada_t1', 'hada_t2', 'lokr_t2')


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


def lycoris_slot(k: str) -> Tuple[str, Optional[str]]:
    """-> (module part, LoHa / LoKr tensor name or 'lokr_row0') or (k, None)."""
    stem, _, tail = k.rpartition('.')
    return (stem, tail) if stem and tail in LOHA_SLOTS + LOKR_SLOTS + (LOKR_ROW0,) else (k, None)


def _refuse_lycoris(k: str, v) -> None:
    tail = k.rsplit('.', 2)
    dims = getattr(v, 'dim', lambda: 2)()
    if ('.lora_mid.' in k or tail[-1] in ('diff', 'diff_b') + _TUCKER or (k.endswith('.weight') and 'lora_' in k and dims > 2)
            or (lycoris_slot(k)[1] is not None and dims > 2)):
        raise ValueError(f'{k!r}: {_LYCORIS}')


def lycoris_entry(name: str, tensors: Dict[str, torch.Tensor], keys: Dict[str, str], alpha, row0=None) -> Dict:
    """The per-module entry of one LoHa or LoKr group: ``dict(kind='loha', w1_a, w1_b, w2_a, w2_b, alpha)`` or ``dict(kind='lokr', w1, w1_a, w1_b, w2,
    w2_a, w2_b, alpha, row0, sliced)`` (a LoKr factor is dense, ``w1``, or a pair, ``w1_a`` / ``w1_b``; the other form is None; ``sliced``: a row0 was
    given, so the module is a row slice of a taller delta).  `tensors` maps LyCORIS'
    tensor names to tensors, `keys` the same names to the keys they came under (for the messages).  An incomplete or mixed group raises ValueError
    naming the family and a key."""
    first = keys[next(iter(tensors))]
    loha, lokr = [s for s in tensors if s in LOHA_SLOTS], [s for s in tensors if s in LOKR_SLOTS]
    if loha and lokr:
        raise ValueError(f'{first!r}: module {name!r} has LoHa and LoKr tensors: one module holds one kind per file')
    for s, v in tensors.items():
        if v.dim() != 2 or 0 in v.shape:
            raise ValueError(f'{keys[s]!r}: a {"LoHa" if loha else "LoKr"} tensor is a non-empty matrix, got {tuple(v.shape)}')
    if loha:
        missing = [s for s in LOHA_SLOTS if s not in tensors]
        if missing:
            raise ValueError(f'{first!r}: LoHa module {name!r} is incomplete: no {", ".join(missing)}')
        if row0 is not None:
            raise ValueError(f'{first!r}: LoHa module {name!r} has a {LOKR_ROW0}, which belongs to LoKr modules')
        e = dict(kind='loha', alpha=alpha, **{s[len('hada_'):]: tensors[s] for s in LOHA_SLOTS})
        for n in ('w1', 'w2'):
            if e[n + '_a'].shape[1] != e[n + '_b'].shape[0]:
                raise ValueError(f'{keys["hada_" + n + "_a"]!r}: LoHa module {name!r}: hada_{n}_a {tuple(e[n + "_a"].shape)} and hada_{n}_b '
                                 f'{tuple(e[n + "_b"].shape)} share no rank')
        if e['w1_a'].shape[0] != e['w2_a'].shape[0] or e['w1_b'].shape[1] != e['w2_b'].shape[1]:
            raise ValueError(f'{first!r}: LoHa module {name!r}: the two products are {e["w1_a"].shape[0]} x {e["w1_b"].shape[1]} and '
                             f'{e["w2_a"].shape[0]} x {e["w2_b"].shape[1]}')
        return e
    e = dict(kind='lokr', alpha=alpha, row0=0 if row0 is None else int(row0), sliced=row0 is not None)
    for n in ('w1', 'w2'):
        dense, a, b = (tensors.get('lokr_' + n + suf) for suf in ('', '_a', '_b'))
        if (dense is None) == (a is None and b is None) or (a is None) != (b is None):
            raise ValueError(f'{first!r}: LoKr module {name!r} is incomplete: it needs lokr_{n}, or lokr_{n}_a and lokr_{n}_b, and has '
                             f'{sorted(s for s in tensors if s.startswith("lokr_" + n)) or "neither"}')
        if a is not None and a.shape[1] != b.shape[0]:
            raise ValueError(f'{keys["lokr_" + n + "_a"]!r}: LoKr module {name!r}: lokr_{n}_a {tuple(a.shape)} and lokr_{n}_b {tuple(b.shape)} share no rank')
        e.update({n: dense, n + '_a': a, n + '_b': b})
    return e


def lokr_shapes(e: Dict) -> Tuple[int, int, int, int]:
    """(a, b, c, d) of a LoKr entry: w1 is [a, b], w2 is [c, d], dense or as a pair."""
    dims = []
    for n in ('w1', 'w2'):
        dims += list(e[n].shape) if e[n] is not None else [e[n + '_a'].shape[0], e[n + '_b'].shape[1]]
    return tuple(dims)


def lycoris_factor(e: Dict) -> float:
    """alpha / r: LoHa, r = the rank of the first pair; LoKr, r = the rank of a low-rank factor (w2's when both are low-rank) and 1 with both factors
    dense.  1 without alpha.  LyCORIS' rule as recalled (module docstring)."""
    if e['alpha'] is None:
        return 1.0
    if e['kind'] == 'loha':
        return e['alpha'] / e['w1_b'].shape[0]
    if e['w2'] is None:
        return e['alpha'] / e['w2_b'].shape[0]
    return 1.0 if e['w1'] is not None else e['alpha'] / e['w1_b'].shape[0]


def _magnitude(k: str, v: torch.Tensor) -> torch.Tensor:
    if not (v.dim() == 1 or (v.dim() == 2 and 1 in v.shape)):
        raise ValueError(f'{k!r}: a DoRA magnitude has shape [O], [O, 1] or [1, O], got {tuple(v.shape)}')
    return v.reshape(-1).float()


def _convert_lycoris(name: str, e: Dict, parts: List[str], sizes: List[int], in_f: int, swap: bool, out: Dict, claim) -> None:
    """One LoHa / LoKr source module -> its parts' keys in `out` (module docstring: row slices of the ``_a`` tensors; both factors plus ``lokr_row0``)."""
    keys = e['keys']
    first = keys[next(iter(e['lyc']))]
    for slot in ('A', 'B'):
        if e[slot] is not None:
            raise ValueError(f'{keys[slot]!r}: module {name!r} has LoRA and LoHa / LoKr tensors: one module holds one kind per file')
    if e['m'] is not None:
        raise ValueError(f'{keys["m"]!r}: a DoRA magnitude on the LoHa / LoKr module {name!r} is not supported')
    if LOKR_ROW0 in e['lyc']:
        raise ValueError(f'{keys[LOKR_ROW0]!r}: {LOKR_ROW0} is written by the conversion, next to diffusers module names only')
    entry = lycoris_entry(name, e['lyc'], keys, e['alpha'])
    O = sum(sizes)
    if entry['kind'] == 'loha':
        for n in ('w1', 'w2'):
            if entry[n + '_a'].shape[0] != O or entry[n + '_b'].shape[1] != in_f:
                raise ValueError(f'{keys["hada_" + n + "_a"]!r}: LoHa module {name!r}: hada_{n}_a {tuple(entry[n + "_a"].shape)} / hada_{n}_b '
                                 f'{tuple(entry[n + "_b"].shape)} do not give the [{O}, {in_f}] of {parts}')
        ups = {n: entry[n + '_a'] for n in ('w1', 'w2')}
        if swap:
            ups = {n: torch.cat([u[O // 2:], u[:O // 2]]) for n, u in ups.items()}
    else:
        a, b, c, d = lokr_shapes(entry)
        if a * c != O or b * d != in_f:
            raise ValueError(f'{first!r}: LoKr module {name!r}: kron of w1 [{a}, {b}] and w2 [{c}, {d}] is [{a * c}, {b * d}] (a c x b d), not the '
                             f'[{O}, {in_f}] of {parts}')
        if swap:
            raise ValueError(f'{first!r}: a LoKr on {name!r} is not supported: diffusers keeps its two row halves in the other order and a Kronecker '
                             f'product cannot be reordered by rows')
    r0 = 0
    for p, n in zip(parts, sizes):
        claim(name, p)
        pre = f'transformer.{p}.'
        if entry['kind'] == 'loha':
            for f in ('w1', 'w2'):
                out[pre + f'hada_{f}_a'], out[pre + f'hada_{f}_b'] = ups[f][r0:r0 + n], entry[f + '_b']
        else:
            for slot in LOKR_SLOTS:
                if entry[slot[len('lokr_'):]] is not None:
                    out[pre + slot] = entry[slot[len('lokr_'):]]
            if len(parts) > 1:
                out[pre + LOKR_ROW0] = torch.tensor(r0, dtype=torch.int64)
        if e['alpha'] is not None:
            out[pre + 'alpha'] = e['alpha']
        r0 += n


def convert_community_lora(sd: Dict[str, torch.Tensor], family: str, transformer_config: Dict, student: bool = True):
    """-> (state dict in the layout ``parse_lora_state_dict`` accepts, {diffusers module: fp32 [O] DoRA magnitude}, [skipped keys]).

    Keys already in the diffusers / peft layout pass through untouched (their magnitude keys move to the second result).  ``lora_te*`` keys
    and, for the student, ``final_layer.linear`` are skipped with ONE warning; a key that resolves to no linear of the transformer, and any
    unsupported LyCORIS tensor (module docstring), raises ValueError naming the key.  LoHa / LoKr tensors come out under the diffusers module name
    with LyCORIS' tensor names (``transformer.<module>.hada_w1_a`` ..., ``lokr_w1`` ..., ``lokr_row0`` for the parts of a fused LoKr).  The BFL <-> diffusers table (``bfl_modules``) is diffusers'
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
    mag_keys: Dict[str, str] = {}                   # diffusers module -> the key its magnitude came under
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
        if slot is None:
            stem, slot = lycoris_slot(k)
        if k.startswith(('lora_unet_', 'lora_transformer_')):
            token = stem[len('lora_unet_'):] if k.startswith('lora_unet_') else stem[len('lora_transformer_'):]
            name = underscored.get(token)
        elif k.startswith('diffusion_model.'):
            name = stem[len('diffusion_model.'):]
            name = name if name in dotted else None
        else:                                       # diffusers / peft layout: only the magnitudes are taken out
            if slot == 'm':
                mod = stem[len('transformer.'):] if stem.startswith('transformer.') else stem
                mags[mod], mag_keys[mod] = _magnitude(k, v), k
            else:
                out[k] = v
            continue
        if slot is None:
            raise ValueError(f'{k!r} is not a LoRA key (expected <module>.lora_down/lora_up.weight, .lora_A/lora_B.weight, .alpha, .dora_scale, '
                             f'.lora_magnitude_vector[.weight], .hada_w1_a/_b, .hada_w2_a/_b or .lokr_w1/w2[_a/_b])')
        if name is None:
            raise ValueError(f'{k!r}: the {family} transformer has no module for it (neither a BFL nor a diffusers module name)')
        if dotted[name][0] is None:
            skipped.append(k)
            n_head += 1
            continue
        entry = fused.setdefault(name, dict(A=None, B=None, alpha=None, m=None, lyc={}, keys={}))
        if slot in LOHA_SLOTS + LOKR_SLOTS + (LOKR_ROW0,):
            if slot in entry['lyc']:
                raise ValueError(f'{k!r}: a second {slot} tensor for module {name!r}')
            entry['lyc'][slot] = v
        else:
            if entry[slot] is not None:
                raise ValueError(f'{k!r}: a second {slot} tensor for module {name!r}')
            entry[slot] = _magnitude(k, v) if slot == 'm' else v
        entry['keys'][slot] = k

    def claim(name, p):
        if any(f'transformer.{p}.{suf}' in out for suf in ('lora_A.weight', 'lora_B.weight') + LOHA_SLOTS + LOKR_SLOTS):
            raise ValueError(f'LoRA module {name!r}: {p!r} is adapted twice in this file')

    for name, e in fused.items():
        parts, swap = dotted[name]
        sizes = [shapes[p + '.weight'][0] for p in parts]
        in_f = shapes[parts[0] + '.weight'][1]
        if e['lyc']:
            _convert_lycoris(name, e, parts, sizes, in_f, swap, out, claim)
            continue
        if e['A'] is None or e['B'] is None:
            raise ValueError(f'LoRA module {name!r}: lora_down / lora_up pair is incomplete')
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
            claim(name, p)
            out[f'transformer.{p}.lora_A.weight'], out[f'transformer.{p}.lora_B.weight'] = e['A'], up[r0:r0 + n]
            if e['alpha'] is not None:
                out[f'transformer.{p}.alpha'] = e['alpha']
            if m is not None:
                mags[p] = m[r0:r0 + n].contiguous()
            r0 += n
    for mod, k in mag_keys.items():                 # diffusers-layout files: a magnitude beside LoHa / LoKr tensors of the same module
        if any(f'{pre}{mod}.{suf}' in out for pre in ('transformer.', '') for suf in LOHA_SLOTS + LOKR_SLOTS):
            raise ValueError(f'{k!r}: a DoRA magnitude on the LoHa / LoKr module {mod!r} is not supported')
    if skipped:
        parts = []
        if n_te:
            parts.append(f'{n_te} text-encoder LoRA tensors were skipped: only transformer LoRAs are applied.')
        if n_head:
            parts.append(f'{n_head} `final_layer.linear` tensors were skipped: the ArcFlow student has no `proj_out`.')
        warnings.warn('  '.join(parts))
    return out, mags, skipped
