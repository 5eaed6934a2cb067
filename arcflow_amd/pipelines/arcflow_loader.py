"""``load_arcflow_adapter()`` with the reference's contract
(lakonlab/pipelines/arcflow_loader.py:45-275): read ``config.json`` (``_class_name`` must be an ArcFlow
transformer), read ``diffusion_pytorch_model.safetensors`` (keys written by
export_arcflow_to_diffusers.py:100-127), overlay every non-LoRA key (three heads, ``norm_out``) on the
base transformer's weights, fold the LoRA pairs in, swap the pipeline's ``transformer`` for the ArcFlow
student and return ``f"{target_module_name}_arcflow"`` (or ``None`` + a warning without LoRA keys).

MI355X specifics: the student is a new ``MMDiTEngine`` with the 3-head velocity output; LoRA is merged
into the bf16 base weights at load (fp32 merge, one rounding) instead of running side GEMMs per call.
"""
from __future__ import annotations

import ctypes
import json
import os
import re
import warnings
from typing import Dict, List, Optional

import torch

from .._lib import AFX_LORA_MAX_ADAPTERS as MAX_FOLD_ADAPTERS       # adapters one afx_lora_fold launch sums

LOCAL_CLASS_MAPPING = {
    'ArcFluxTransformer2DModel': 'flux',
    'ArcQwenImageTransformer2DModel': 'qwen',
}
SAFETENSORS_WEIGHTS_NAME = 'diffusion_pytorch_model.safetensors'
_HF_KWARGS = ('cache_dir', 'force_download', 'proxies', 'token', 'local_files_only', 'revision', 'subfolder',
              'low_cpu_mem_usage', 'variant', 'use_safetensors', 'disable_mmap')


def _resolve_dir(path: str, subfolder: Optional[str]) -> str:
    d = os.path.join(path, subfolder) if subfolder else path
    if not os.path.isdir(d):
        raise EnvironmentError(
            f'{d} is not a local directory. This build has no network access: pass a local snapshot of the '
            f'adapter repository (the layout export_arcflow_to_diffusers.py writes).')
    return d


def read_adapter(path: str, subfolder: Optional[str] = None, variant: Optional[str] = None):
    """-> (config dict, state dict, safetensors metadata)."""
    from safetensors import safe_open
    d = _resolve_dir(path, subfolder)
    with open(os.path.join(d, 'config.json')) as f:
        config = json.load(f)
    name = SAFETENSORS_WEIGHTS_NAME if not variant else SAFETENSORS_WEIGHTS_NAME.replace('.safetensors', f'.{variant}.safetensors')
    sd: Dict[str, torch.Tensor] = {}
    with safe_open(os.path.join(d, name), framework='pt', device='cpu') as f:
        meta = f.metadata() or {}
        for k in f.keys():
            sd[k] = f.get_tensor(k)
    return config, sd, meta


LORA_WEIGHT_NAME = 'pytorch_lora_weights.safetensors'
_LORA_KEY = re.compile(r'^(?P<mod>.+)\.(?P<kind>lora_A|lora_B|lora_down|lora_up)(?:\.(?P<infix>[^.]+))?\.weight$')


def read_lora_file(path: str, weight_name: Optional[str] = None, subfolder: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """A local ``.safetensors`` file, or a directory (+ ``subfolder``) holding ``weight_name`` (default: diffusers'
    ``pytorch_lora_weights.safetensors``) -> state dict.  Never reaches the network."""
    from safetensors import safe_open
    f = path
    if os.path.isdir(path):
        f = os.path.join(_resolve_dir(path, subfolder), weight_name or LORA_WEIGHT_NAME)
    if not os.path.isfile(f):
        raise EnvironmentError(f'{f} is not a local file. This build has no network access: pass a local .safetensors file, or a '
                               f'directory and `weight_name`.')
    with safe_open(f, framework='pt', device='cpu') as h:
        return {k: h.get_tensor(k) for k in h.keys()}


def parse_lora_state_dict(sd: Dict[str, torch.Tensor], prefix: str = 'transformer'):
    """Group a diffusers / peft LoRA state dict by module -> ({module: dict(A=[r, in], B=[out, r], alpha=float or None)}, number of
    skipped ``text_encoder*`` keys).  Accepted per module, with or without the leading ``transformer.``:
    ``<module>.lora_A.weight`` / ``lora_B.weight`` (also with an adapter infix, ``lora_A.default.weight``), ``<module>.lora_down.weight``
    / ``lora_up.weight``, and an optional scalar ``<module>.alpha``.  Kohya / ComfyUI checkpoints (``lora_unet_*`` keys, fused qkv /
    linear1 tensors) are refused: convert them to the diffusers layout first.

    LyCORIS tensors under the same module names (``<module>.hada_w1_a`` / ``hada_w1_b`` / ``hada_w2_a`` / ``hada_w2_b``; ``<module>.lokr_w1`` or
    ``lokr_w1_a`` + ``lokr_w1_b``, the same for ``lokr_w2``, and the integer scalar ``<module>.lokr_row0`` the conversion writes for the parts of a
    fused tensor) become entries that carry their kind, ``dict(kind='loha' | 'lokr', ...)`` as ``lora_formats.lycoris_entry`` builds them; a LoRA
    entry has no ``kind``.  One module holds one kind per file; an incomplete group raises ValueError naming the family and a key."""
    from . import lora_formats as F
    mods: Dict[str, Dict] = {}
    lyc: Dict[str, Dict] = {}                       # module -> dict(t={LyCORIS tensor name: tensor}, keys={name: key}, row0=None or int)
    skipped = 0
    for k, v in sd.items():
        if k.startswith('lora_unet_') or k.startswith('lora_te'):
            raise ValueError(f'{k!r}: this is a Kohya / ComfyUI LoRA checkpoint (fused qkv / linear1 tensors under `lora_unet_*`), which '
                             f'is not supported: convert it to the diffusers layout (transformer.<module>.lora_A/lora_B.weight) first')
        if k.startswith('text_encoder'):
            skipped += 1
            continue
        k2 = k[len(prefix) + 1:] if k.startswith(prefix + '.') else k
        stem, slot = F.lycoris_slot(k2)
        if slot is not None:
            F._refuse_lycoris(k, v)
            group = lyc.setdefault(stem, dict(t={}, keys={}, row0=None))
            if slot == F.LOKR_ROW0:
                if v.numel() != 1 or v.is_floating_point():
                    raise ValueError(f'{k!r}: {F.LOKR_ROW0} is an integer scalar, got {tuple(v.shape)} {v.dtype}')
                group['row0'] = int(v)
            else:
                group['t'][slot] = v
            group['keys'][slot] = k
            continue
        if k2.rpartition('.')[2] in F._TUCKER + ('diff', 'diff_b'):
            F._refuse_lycoris(k, v)
        m = _LORA_KEY.match(k2)
        if m is not None:
            slot = 'A' if m.group('kind') in ('lora_A', 'lora_down') else 'B'
            entry = mods.setdefault(m.group('mod'), dict(A=None, B=None, alpha=None))
            if entry[slot] is not None:
                raise ValueError(f'{k!r}: a second {m.group("kind")} tensor for module {m.group("mod")!r}')
            entry[slot] = v
        elif k2.endswith('.alpha'):
            mods.setdefault(k2[:-len('.alpha')], dict(A=None, B=None, alpha=None))['alpha'] = float(v)
        else:
            raise ValueError(f'{k!r} is not a LoRA key (expected <module>.lora_A/lora_B[.<adapter>].weight, <module>.lora_down/lora_up.weight '
                             f'or <module>.alpha)')
    if skipped:
        warnings.warn(f'{skipped} text-encoder LoRA tensors were skipped: only transformer LoRAs are applied.')
    for name, group in lyc.items():
        first = group['keys'][next(iter(group['keys']))]
        e = mods.pop(name, dict(A=None, B=None, alpha=None))
        if e['A'] is not None or e['B'] is not None:
            raise ValueError(f'{first!r}: module {name!r} has LoRA and LoHa / LoKr tensors: one module holds one kind per file')
        if not group['t']:
            raise ValueError(f'{first!r}: LoKr module {name!r} is incomplete: a {F.LOKR_ROW0} without factors')
        mods[name] = F.lycoris_entry(name, group['t'], group['keys'], e['alpha'], group['row0'])
    for name, e in mods.items():
        if 'kind' not in e and (e['A'] is None or e['B'] is None):
            raise ValueError(f'LoRA module {name!r}: lora_A / lora_B (lora_down / lora_up) pair is incomplete')
    return mods, skipped


class ArcFlowLoaderMixin:
    """Adds ``load_arcflow_adapter`` and the diffusers LoRA surface (``load_lora_weights``, ``set_adapters``, ``delete_adapters``,
    ``unload_lora_weights``, ``get_active_adapters``, ``get_list_adapters``) to a pipeline that keeps ``self._base_state_dict``
    (diffusers keys) and ``self._transformer_config``."""

    def load_arcflow_adapter(self, pretrained_model_name_or_path: str, target_module_name: str = 'transformer',
                             adapter_name: Optional[str] = None, **kwargs) -> Optional[str]:
        unknown = set(kwargs) - set(_HF_KWARGS)
        if unknown:
            raise TypeError(f'load_arcflow_adapter() got unexpected keyword arguments {sorted(unknown)}')
        if getattr(self, '_style', None) is not None:
            raise RuntimeError('style LoRAs are loaded: call unload_lora_weights() before loading an ArcFlow adapter')
        subfolder = kwargs.get('subfolder')
        config, adapter_sd, meta = read_adapter(pretrained_model_name_or_path, subfolder, kwargs.get('variant'))
        cls_name = config.get('_class_name')
        if cls_name not in LOCAL_CLASS_MAPPING:
            raise ValueError(f"Can't find a model linked to {cls_name}.")
        family = LOCAL_CLASS_MAPPING[cls_name]
        if family != self._family:
            raise ValueError(f'{cls_name} adapter cannot be loaded into a {self._family} pipeline')
        base = dict(self._base_state_dict)
        lora: Dict[str, torch.Tensor] = {}
        prefix = target_module_name + '.'
        for k, v in adapter_sd.items():
            k2 = k[len(prefix):] if k.startswith(prefix) else k
            (lora if 'lora' in k2 else base)[k2] = v
        if len(lora) == 0:
            warnings.warn(f'No LoRA weights were found in {pretrained_model_name_or_path}.')
            return None
        if adapter_name is None:
            adapter_name = f'{target_module_name}_arcflow'
        from ..weights import merge_lora
        merged = merge_lora(base, lora, scale=1.0)
        student = self._build_engine(num_gaussians=config.get('num_gaussians', 16),
                                     logweights_channels=config.get('logweights_channels', 4), teacher_head=False)
        student.load_state_dict(merged)
        setattr(self, target_module_name, student)
        self.policy_config = json.loads(meta['policy_config']) if 'policy_config' in meta else {'type': 'ArcFlow'}
        self._adapters = getattr(self, '_adapters', []) + [adapter_name]
        # kept for a runtime LoRA scale (`joint_attention_kwargs={'scale': s}` / `set_adapters(..., adapter_weights=s)`): see _apply_lora_scale
        self._adapter_state = dict(target=target_module_name, base=base, lora=lora, merged_scale=1.0, weight=1.0)
        return adapter_name

    # ------------------------------------------------------------------ runtime LoRA scale
    def set_adapters(self, adapter_names, adapter_weights=None) -> None:
        """diffusers' `pipe.set_adapters(names, adapter_weights=w)` for the ArcFlow adapter (inference_flux.py:9 mentions it): the adapter's
        LoRA branch is weighted by w from now on.  With style LoRAs loaded (`load_lora_weights`) this is diffusers' full form: the listed
        adapters become active with `adapter_weights` (a float for all, a list, or None = 1.0), every adapter not listed becomes
        inactive, and the weights are folded on the device at the next call (see `load_lora_weights`).  Leaving the ArcFlow adapter out
        switches off its LoRA branch only -- its heads and `norm_out` stay, exactly as `adapter_weights=0` does."""
        names = [adapter_names] if isinstance(adapter_names, str) else list(adapter_names)
        known = getattr(self, '_adapters', [])
        for n in names:
            if n not in known:
                raise ValueError(f'adapter {n!r} is not loaded (loaded: {known})')
        if getattr(self, '_style', None) is not None:
            self._set_style_adapters(names, adapter_weights)
            return
        if adapter_weights is None:
            w = 1.0
        elif isinstance(adapter_weights, (int, float)):
            w = float(adapter_weights)
        else:
            w = float(list(adapter_weights)[0])
        self._adapter_state['weight'] = w
        self._apply_lora_scale(1.0)

    def _apply_lora_scale(self, call_scale: float) -> None:
        """The reference scales every LoRA layer by `joint_attention_kwargs['scale']` around the forward (`scale_lora_layers` /
        `unscale_lora_layers`, lakonlab/models/architecture/arcflow/arcflux.py:147-154, :251-252): y = W x + s (alpha / r) B A x.  Here the
        adapter is folded into the weights, so a different s means folding again: W + s B A from the kept base and LoRA tensors (one
        fp32-accumulating GEMM per adapted linear on the device + a re-pack, about a second for FLUX-12B), cached until s changes --
        a call with the same scale as the previous one costs nothing.  Deviation of the folded forward from the un-folded one:
        tests/test_distill.py::test_unmerged_trunk_forward_matches_merged_engine."""
        if getattr(self, '_style', None) is not None:
            self._fold_adapters(float(call_scale))
            return
        st = getattr(self, '_adapter_state', None)
        if st is None:
            if call_scale != 1.0:
                raise RuntimeError('a LoRA scale was passed but no ArcFlow adapter is loaded')
            return
        s = float(call_scale) * st['weight']
        if s == st['merged_scale']:
            return
        from ..weights import merge_lora
        getattr(self, st['target']).load_state_dict(merge_lora(st['base'], st['lora'], scale=s))
        st['merged_scale'] = s

    # ------------------------------------------------------------------ style LoRAs next to the ArcFlow adapter
    def _lora_engine(self):
        st = getattr(self, '_adapter_state', None)
        return getattr(self, st['target'] if st else 'transformer')

    def _arcflow_adapter_name(self) -> Optional[str]:
        return self._adapters[0] if getattr(self, '_adapter_state', None) is not None else None

    def load_lora_weights(self, pretrained_model_name_or_path_or_dict, weight_name: Optional[str] = None,
                          adapter_name: Optional[str] = None, subfolder: Optional[str] = None) -> str:
        """diffusers' `pipe.load_lora_weights(...)` for transformer (style) LoRAs, to be combined with the ArcFlow adapter through
        `set_adapters` as inference_flux.py:9 suggests.  Reads a local `.safetensors` file, a directory + `weight_name`
        (default `pytorch_lora_weights.safetensors`), or a state dict; never the network.  Keys: see `parse_lora_state_dict`
        (`text_encoder*` keys are skipped with one warning).  Kohya / ComfyUI checkpoints (`lora_unet_*`, `lora_transformer_*`,
        `diffusion_model.*` keys: BFL module names with fused qkv / linear1 tensors on FLUX, underscored diffusers names on either family)
        and DoRA magnitudes (`dora_scale`, `lora_magnitude_vector`) go through `lora_formats.convert_community_lora` first; its BFL <->
        diffusers table is diffusers' conversion as recalled and is not pinned against diffusers.  LoHa / LoKr / diff / conv tensors are
        refused by name.  A module the transformer does not have, or a shape that does not fit its linear, raises ValueError; so does a
        duplicate `adapter_name`.  The new adapter becomes active with weight 1.0; the other adapters keep their state.  Returns the
        adapter's name.

        DoRA: an adapter with a magnitude m on a linear contributes (g - 1) W_base + g s B A there, g[o] = m[o] / ||(W_base + s B A)[o, :]||
        with its own effective scale s -- peft's rule for several active adapters as recalled, not checked against peft.  `afx_lora_row_gain`
        computes g on the device whenever s changed (the vectors are cached per adapter and linear) and `afx_lora_fold_rows` folds with it:
        still one rounding.  An active DoRA adapter at weight 0 still applies its magnitude ((m / ||W_base|| - 1) W_base, as peft does); an
        adapter left out of `set_adapters` contributes nothing.  A row with ||.|| = 0 gets g = 0 where peft divides by zero.

        LyCORIS LoHa (`hada_w1_a/b`, `hada_w2_a/b`) and LoKr (`lokr_w1[_a/_b]`, `lokr_w2[_a/_b]`) files load under the same module spellings
        (`lora_formats`): a LoHa module contributes s (w1_a w1_b) (*) (w2_a w2_b), a LoKr module s kron(w1, w2), s = the effective scale below
        with factor `alpha / r` as `lora_formats.lycoris_factor` states it.  LoHa operands are kept as bf16, LoKr factors as dense fp32 (a low-rank
        factor is multiplied out once at load); a linear with such a term is folded by `afx_lora_fold_terms`, LoRA / DoRA / LoHa / LoKr terms
        of all active adapters together, still with one rounding.  The LyCORIS rules are restated from memory: not checked against LyCORIS or
        ComfyUI.  A DoRA magnitude on a LoHa / LoKr module, Tucker / convolution tensors and `diff` keys are refused.

        Every adapter's tensors are uploaded once as bf16: fp32 / fp16 files are rounded once here, as `weights._merge_one` does for the
        ArcFlow adapter.  Its factor is `alpha / r` per module (1 without `alpha`); the effective scale of adapter j is
        `call_scale * adapter_weights[j] * alpha_j / r_j`, with `call_scale` = `joint_attention_kwargs['scale']` (`attention_kwargs`
        on Qwen-Image) multiplying EVERY active adapter as the reference's `scale_lora_layers` does.

        Folding: W = bf16(W_base + sum_j s_j B_j A_j) per adapted linear by `afx_lora_fold` straight into the engine's live packed
        weights (same addresses, no re-bind, no host round trip, no re-pack), the scales applied in fp32 to fp32 sums and ONE rounding
        at the store.  W_base is the plain snapshot plus the ArcFlow adapter's non-LoRA keys.  Folds are lazy: nothing runs before the
        next `__call__`, only linears whose scale list changed are folded, and an unchanged state costs nothing.  Memory: while any
        style LoRA is loaded the pipeline keeps a device-resident bf16 copy of W_base for every linear that ANY loaded adapter (the
        ArcFlow one included) touches -- up to one more bf16 copy of the adapted matrices -- plus the small A / B tensors.
        `unload_lora_weights()` frees it.  Not supported together with the engine's fp8 linear mode (NotImplementedError): the
        quantised weight copies would have to be rebuilt after every fold.  `sample_teacher` is not affected by any of this."""
        eng = self._lora_engine()
        if eng is None or eng.teacher_head:
            raise RuntimeError('load_lora_weights() needs the ArcFlow student: call load_arcflow_adapter() first')
        if getattr(eng, 'fp8_linear', False):
            raise NotImplementedError('style LoRAs with the fp8 linear mode on are not supported (the quantised weights are not rebuilt '
                                      'after a fold): call enable_fp8(False) first')
        sd = pretrained_model_name_or_path_or_dict
        if not isinstance(sd, dict):
            sd = read_lora_file(sd, weight_name, subfolder)
        known = list(getattr(self, '_adapters', []))
        if adapter_name is None:
            n = 0
            while f'default_{n}' in known:
                n += 1
            adapter_name = f'default_{n}'
        if adapter_name in known:
            raise ValueError(f'adapter {adapter_name!r} is already loaded (loaded: {known})')
        from . import lora_formats
        magnitudes = {}
        if lora_formats.needs_conversion(sd):
            sd, magnitudes, _ = lora_formats.convert_community_lora(sd, self._family, self._transformer_config, student=True)
        mods, _ = parse_lora_state_dict(sd)
        if not mods:
            raise ValueError('no transformer LoRA weights were found')
        for m, v in magnitudes.items():
            if m not in mods:
                raise ValueError(f'adapter {adapter_name!r}: a DoRA magnitude for {m!r}, which has no lora_A / lora_B pair in this file')
            if 'kind' in mods[m]:
                raise ValueError(f'adapter {adapter_name!r}: a DoRA magnitude on the LoHa / LoKr module {m!r} is not supported')
            mods[m]['magnitude'] = v
        sty = getattr(self, '_style', None)
        fresh = sty is None
        if fresh:
            from ..weights import packed_row_slices
            sty = dict(slices=packed_row_slices(self._family, self._transformer_config, True, eng.num_gaussians, eng.logweights_channels),
                       loras={}, active={}, base={}, arc={}, folded={}, magnitude={}, gain={})
            arc = self._arcflow_adapter_name()
            if arc is not None:
                arc_mods, _ = parse_lora_state_dict(self._adapter_state['lora'])
                sty['arc'] = self._upload_adapter(sty, arc_mods, eng.device, 'the ArcFlow adapter')
                sty['active'][arc] = float(self._adapter_state['weight'])
        mag = {}
        new = self._upload_adapter(sty, mods, eng.device, f'adapter {adapter_name!r}', mag)
        base_sd = self._adapter_state['base'] if getattr(self, '_adapter_state', None) is not None else self._base_state_dict
        for m in list(sty['arc']) + list(new):
            if m not in sty['base']:
                w = base_sd.get(m + '.weight', base_sd.get(m + '.base_layer.weight'))
                sty['base'][m] = w.to(device=eng.device, dtype=torch.bfloat16).contiguous()
        sty['loras'][adapter_name] = new
        sty['magnitude'][adapter_name] = mag
        sty['active'][adapter_name] = 1.0
        self._style = sty
        self._adapters = known + [adapter_name]
        return adapter_name

    def _upload_adapter(self, sty, mods, device, what: str, magnitude: Optional[Dict] = None):
        """{module: dict(A, B, alpha)} -> {module: (A bf16 on the device, B bf16 on the device, alpha / r)}, checked against the linear it adapts.
        A module's DoRA magnitude (its 'magnitude' entry, [rows]) goes into `magnitude` as fp32 on the device.

        A LoHa entry becomes dict(kind='loha', w1_a, w1_b, w2_a, w2_b bf16 on the device, factor); a LoKr entry dict(kind='lokr', w1 [a, b], w2 [c, d]
        dense fp32 on the device, row0, factor), a low-rank factor multiplied out here, once, in fp32 (it is [c, d]-sized)."""
        from . import lora_formats as F
        out = {}
        for m, e in mods.items():
            if m not in sty['slices']:
                raise ValueError(f'{what}: the transformer has no linear {m!r}')
            _, _, rows, in_f = sty['slices'][m]
            if 'kind' in e:
                if rows % 64 or in_f % 64:
                    raise ValueError(f'{what}: {m!r} is a [{rows}, {in_f}] linear; adapters are folded on linears whose sizes are multiples of 64')
                if e['kind'] == 'loha':
                    for n in ('w1', 'w2'):
                        if e[n + '_a'].shape[0] != rows or e[n + '_b'].shape[1] != in_f:
                            raise ValueError(f'{what}: {m!r} is a [{rows}, {in_f}] linear, hada_{n}_a {tuple(e[n + "_a"].shape)} / hada_{n}_b '
                                             f'{tuple(e[n + "_b"].shape)} do not fit it')
                    out[m] = dict(kind='loha', factor=F.lycoris_factor(e),
                                  **{n: e[n].to(device=device, dtype=torch.bfloat16).contiguous() for n in ('w1_a', 'w1_b', 'w2_a', 'w2_b')})
                else:
                    a, b, c, d = F.lokr_shapes(e)
                    if b * d != in_f or e['row0'] < 0 or e['row0'] + rows > a * c or (not e['sliced'] and a * c != rows):
                        raise ValueError(f'{what}: {m!r} is a [{rows}, {in_f}] linear; kron of lokr_w1 [{a}, {b}] and lokr_w2 [{c}, {d}] is '
                                         f'[{a * c}, {b * d}] (a c x b d), which does not fit it at lokr_row0 = {e["row0"]}')
                    dense = {n: e[n].float() if e[n] is not None else e[n + '_a'].float() @ e[n + '_b'].float() for n in ('w1', 'w2')}
                    out[m] = dict(kind='lokr', factor=F.lycoris_factor(e), row0=e['row0'],
                                  **{n: w.to(device=device, dtype=torch.float32).contiguous() for n, w in dense.items()})
                continue
            a, b = e['A'], e['B']
            if a.dim() != 2 or b.dim() != 2 or a.shape[0] < 1 or a.shape[0] != b.shape[1] or a.shape[1] != in_f or b.shape[0] != rows:
                raise ValueError(f'{what}: {m!r} is a [{rows}, {in_f}] linear, lora_A {tuple(a.shape)} / lora_B {tuple(b.shape)} do not fit it')
            if rows % 64 or in_f % 64:
                raise ValueError(f'{what}: {m!r} is a [{rows}, {in_f}] linear; LoRAs are folded on linears whose sizes are multiples of 64')
            r = a.shape[0]
            out[m] = (a.to(device=device, dtype=torch.bfloat16).contiguous(), b.to(device=device, dtype=torch.bfloat16).contiguous(),
                      1.0 if e['alpha'] is None else e['alpha'] / r)
            if e.get('magnitude') is not None:
                if e['magnitude'].numel() != rows:
                    raise ValueError(f'{what}: {m!r} has {rows} output rows, its DoRA magnitude {e["magnitude"].numel()} elements')
                magnitude[m] = e['magnitude'].reshape(rows).to(device=device, dtype=torch.float32).contiguous()
        return out

    def _set_style_adapters(self, names: List[str], adapter_weights) -> None:
        if adapter_weights is None:
            ws = [1.0] * len(names)
        elif isinstance(adapter_weights, (int, float)):
            ws = [float(adapter_weights)] * len(names)
        else:
            ws = [1.0 if w is None else float(w) for w in adapter_weights]
            if len(ws) != len(names):
                raise ValueError(f'{len(names)} adapters but {len(ws)} adapter_weights')
        self._style['active'] = dict(zip(names, ws))
        arc = self._arcflow_adapter_name()
        if arc is not None:
            self._adapter_state['weight'] = self._style['active'].get(arc, 0.0)

    def get_active_adapters(self) -> List[str]:
        sty = getattr(self, '_style', None)
        if sty is None:
            return list(getattr(self, '_adapters', []))
        return [n for n in self._adapters if n in sty['active']]

    def get_list_adapters(self) -> Dict[str, List[str]]:
        names = list(getattr(self, '_adapters', []))
        return {'transformer': names} if names else {}

    def delete_adapters(self, adapter_names) -> None:
        """Remove style LoRAs.  The ArcFlow adapter cannot be deleted (the student's heads would be left without a trunk to match)."""
        names = [adapter_names] if isinstance(adapter_names, str) else list(adapter_names)
        known = getattr(self, '_adapters', [])
        for n in names:
            if n not in known:
                raise ValueError(f'adapter {n!r} is not loaded (loaded: {known})')
            if n == self._arcflow_adapter_name():
                raise ValueError(f'{n!r} is the ArcFlow adapter: it cannot be deleted (set_adapters without it switches its LoRA branch off)')
        sty = getattr(self, '_style', None)
        if sty is None:
            return
        for n in names:
            del sty['loras'][n]
            del sty['magnitude'][n]
            for key in [key for key in sty['gain'] if key[0] == n]:
                del sty['gain'][key]
            sty['active'].pop(n, None)
            self._adapters.remove(n)
        if not sty['loras']:
            self._restore_without_style()

    def unload_lora_weights(self) -> None:
        """Remove every style LoRA and free their device memory.  Deviation from diffusers: the ArcFlow adapter stays -- unloading it
        would leave a model with no usable head.  Afterwards the weights are the ones `load_arcflow_adapter` / `set_adapters` alone
        produce for the current ArcFlow weight, bit for bit (that path is run)."""
        sty = getattr(self, '_style', None)
        if sty is None:
            return
        for n in list(sty['loras']):
            self._adapters.remove(n)
        sty['loras'].clear()
        self._restore_without_style()

    def _restore_without_style(self) -> None:
        sty, self._style = self._style, None
        st = getattr(self, '_adapter_state', None)
        if st is not None:
            st['merged_scale'] = None            # whatever is folded now, the ArcFlow-only path below rebuilds the weights
            self._apply_lora_scale(1.0)
            return
        from .. import ops
        eng = self._lora_engine()
        for m, sig in sty['folded'].items():
            if sig:
                packed, r0, rows, _ = sty['slices'][m]
                ops.lora_fold(sty['base'][m], eng._weights[packed][r0:r0 + rows])

    def _fold_adapters(self, call_scale: float) -> None:
        """Bring the engine's packed weights to the active adapters at `call_scale`: one `afx_lora_fold` per linear whose list of
        (adapter, fp32 scale) differs from what is folded in now.  A linear with an active DoRA adapter is folded by `afx_lora_fold_rows`
        with that adapter's row gains, computed by `afx_lora_row_gain` when its scale is not the one the cached vector was made for.  A linear
        with an active LoHa / LoKr term goes through `afx_lora_fold_terms` with all its terms; every other linear takes the call it always took."""
        from .. import ops
        sty = self._style
        eng = self._lora_engine()
        if getattr(eng, 'fp8_linear', False):
            raise NotImplementedError('style LoRAs with the fp8 linear mode on are not supported (the quantised weights are not rebuilt '
                                      'after a fold): unload_lora_weights() or enable_fp8(False)')
        arc = self._arcflow_adapter_name()
        sources = ([(arc, sty['arc'])] if arc is not None else []) + list(sty['loras'].items())
        for m, base in sty['base'].items():
            A, B, S, sig = [], [], [], []
            for name, mods in sources:
                if name in sty['active'] and m in mods:
                    if isinstance(mods[m], dict):                                   # a LoHa / LoKr entry: the whole entry stands where A stands
                        a, b, factor = mods[m], None, mods[m]['factor']
                    else:
                        a, b, factor = mods[m]
                    s = ctypes.c_float(call_scale * sty['active'][name] * factor).value
                    if s != 0.0 or m in sty['magnitude'].get(name, ()):             # a DoRA adapter at scale 0 still applies its magnitude
                        A.append(a); B.append(b); S.append(s); sig.append((name, s))
            lycoris = any(isinstance(a, dict) for a in A)
            sig = tuple(sig)
            if sty['folded'].get(m, None if m in sty['arc'] else ()) == sig:        # (the ArcFlow-only path folded the arc linears so far)
                continue
            if len(A) > MAX_FOLD_ADAPTERS:
                raise ValueError(f'{len(A)} active adapters on {m!r}: at most {MAX_FOLD_ADAPTERS} can be folded into one linear')
            packed, r0, rows, _ = sty['slices'][m]
            gains = None
            if any(m in sty['magnitude'].get(name, ()) for name, _ in sig):
                gains = []
                for j, (name, s) in enumerate(sig):
                    mag = sty['magnitude'].get(name, {}).get(m)
                    if mag is None:
                        gains.append(None)
                        continue
                    cached = sty['gain'].get((name, m))
                    if cached is None or cached[0] != s:
                        cached = sty['gain'][(name, m)] = (s, ops.lora_row_gain(base, A[j], B[j], s, mag))
                    gains.append(cached[1])
            if not lycoris:                                                         # the call this linear always took
                ops.lora_fold(base, eng._weights[packed][r0:r0 + rows], A, B, S, row_gains=gains)
            else:
                terms = [dict(a, scale=s) if isinstance(a, dict) else dict(kind='lora', A=a, B=b, scale=s, row_gain=None if gains is None else gains[j])
                         for j, (a, b, s) in enumerate(zip(A, B, S))]
                ops.lora_fold_terms(base, eng._weights[packed][r0:r0 + rows], terms)
            sty['folded'][m] = sig
            for k in (packed + '_q', packed[:-len('weight')] + 'wscale'):      # quantised copies of an earlier enable_fp8(): stale now, a later
                eng._weights.pop(k, None)                                      # enable_fp8() quantises this matrix again
