"""Community LoRA layouts and DoRA through ``load_lora_weights`` on the GPU, on the tiny pipelines of tests/test_lora_adapters_gpu.py (its
``Setup``: D = 256, 2 heads, FLUX 1 double + 1 single block, Qwen-Image 1 layer, an ArcFlow adapter with a rank-8 LoRA).

* A Kohya-layout dict (FLUX: BFL names with fused qkv / linear1 and the swapped final modulation; Qwen-Image: underscored diffusers names) and
  the same adapter written by hand in the diffusers layout leave every packed weight bit-identical.
* A DoRA adapter beside the ArcFlow adapter (FLUX: a Kohya file with ``dora_scale`` on a fused qkv, sharing ``to_q`` with the ArcFlow LoRA;
  Qwen-Image: a peft file with ``lora_magnitude_vector``): every touched packed slice is held to the chained bound of tests/lora_dora_ref.py
  (device gains into the device fold), everything else to bit-equality with the packed base; at weight 0 the magnitude still applies; another
  weight refolds; left out of ``set_adapters`` it contributes nothing; ``delete_adapters`` / ``unload_lora_weights`` restore the earlier bits; one
  call returns finite latents that differ from the ones without it.
On the parent commit every test here fails: the loader refuses ``lora_unet_*`` keys and magnitudes."""
import pytest
import torch

import lora_dora_ref as DR
import lora_fold_ref as LR
from test_evaluate_gpu import FLOOR, rel_l2
from test_lora_adapters_gpu import Setup, _weights_equal

pytestmark = pytest.mark.gpu

ARC = 'transformer_arcflow'
D = 256
R, ALPHA = 4, 8.0


@pytest.fixture(scope='module', params=['flux', 'qwen'])
def S(request, tmp_path_factory):
    return Setup(request.param, str(tmp_path_factory.mktemp('community_' + request.param)))


def _pair(g, o, i, std=0.05):
    return (torch.randn(R, i, generator=g) * std).bfloat16(), (torch.randn(o, R, generator=g) * std).bfloat16()


def _two_layouts(S):
    """-> (community-layout dict, the same adapter in the diffusers layout, written out by hand)."""
    g = torch.Generator().manual_seed(31)
    kohya, diff = {}, {}

    def put(k, parts, down, up):
        kohya.update({k + '.lora_down.weight': down, k + '.lora_up.weight': up, k + '.alpha': torch.tensor(ALPHA)})
        for name, rows in parts:
            diff.update({f'transformer.{name}.lora_A.weight': down, f'transformer.{name}.lora_B.weight': rows, f'transformer.{name}.alpha': torch.tensor(ALPHA)})
    if S.family == 'flux':
        t, s = 'transformer_blocks.0.', 'single_transformer_blocks.0.'
        down, up = _pair(g, 3 * D, D)
        put('lora_unet_double_blocks_0_img_attn_qkv', [(t + 'attn.to_q', up[:D]), (t + 'attn.to_k', up[D:2 * D]), (t + 'attn.to_v', up[2 * D:])], down, up)
        down, up = _pair(g, 7 * D, D)
        put('lora_unet_single_blocks_0_linear1',
            [(s + 'attn.to_q', up[:D]), (s + 'attn.to_k', up[D:2 * D]), (s + 'attn.to_v', up[2 * D:3 * D]), (s + 'proj_mlp', up[3 * D:])], down, up)
        down, up = _pair(g, 2 * D, D)
        put('lora_unet_final_layer_adaLN_modulation_1', [('norm_out.linear', torch.cat([up[D:], up[:D]]))], down, up)
        down, up = _pair(g, D, 4 * D)
        put('lora_unet_double_blocks_0_txt_mlp_2', [(t + 'ff_context.net.2', up)], down, up)
        down, up = _pair(g, D, 64)
        put('lora_unet_img_in', [('x_embedder', up)], down, up)
    else:
        for name in ('transformer_blocks.0.attn.to_q', 'transformer_blocks.0.img_mod.1', 'transformer_blocks.0.txt_mlp.net.0.proj', 'img_in'):
            o, i = S.w[name + '.weight'].shape
            down, up = _pair(g, o, i)
            put(('lora_unet_', 'lora_transformer_')[len(kohya) // 3 % 2] + name.replace('.', '_'), [(name, up)], down, up)
    return kohya, diff


def test_community_layout_equals_the_hand_written_diffusers_layout(S):
    kohya, diff = _two_layouts(S)
    pipes = []
    for sd in (kohya, diff):
        pipe = S.with_arcflow()
        pipe.load_lora_weights(dict(sd), adapter_name='style')
        pipe.set_adapters([ARC, 'style'], [1.0, 0.7])
        S.run(pipe, 0.9)
        pipes.append(pipe)
    _weights_equal(*pipes)
    only = S.with_arcflow()
    changed = [k for k, v in pipes[0].transformer._weights.items() if not torch.equal(v, only.transformer._weights[k])]
    assert len(changed) >= 4, changed                                              # ... and the adapter did change the packed matrices


def _dora_adapter(S):
    """-> (state dict to load, {module: (A, B, alpha / r, magnitude fp32)}) of a DoRA adapter; 'transformer_blocks.0.attn.to_q' is shared with the ArcFlow LoRA."""
    g = torch.Generator().manual_seed(41)
    mods, sd = {}, {}

    def magnitude(name):
        w = S.base_sd[name + '.weight'].bfloat16().double()
        return (w.norm(dim=1) * (0.8 + 0.4 * torch.rand(w.shape[0], generator=g).double())).float()
    if S.family == 'flux':
        t = 'transformer_blocks.0.'
        down, up = _pair(g, 3 * D, D)
        m = torch.cat([magnitude(t + 'attn.' + n) for n in ('to_q', 'to_k', 'to_v')])
        k = 'lora_unet_double_blocks_0_img_attn_qkv'
        sd.update({k + '.lora_down.weight': down, k + '.lora_up.weight': up, k + '.alpha': torch.tensor(ALPHA), k + '.dora_scale': m[:, None]})
        for n, name in enumerate(('to_q', 'to_k', 'to_v')):
            mods[t + 'attn.' + name] = (down, up[n * D:(n + 1) * D], ALPHA / R, m[n * D:(n + 1) * D])
        down, up = _pair(g, D, 64)
        m = magnitude('x_embedder')
        sd.update({'lora_unet_img_in.lora_down.weight': down, 'lora_unet_img_in.lora_up.weight': up, 'lora_unet_img_in.dora_scale': m[None, :]})
        mods['x_embedder'] = (down, up, 1.0, m)
        down, up = _pair(g, 4 * D, D)                                              # one module without a magnitude: a plain LoRA in a DoRA file
        sd.update({'lora_unet_double_blocks_0_img_mlp_0.lora_down.weight': down, 'lora_unet_double_blocks_0_img_mlp_0.lora_up.weight': up})
        mods[t + 'ff.net.0.proj'] = (down, up, 1.0, None)
    else:
        for n, name in enumerate(('transformer_blocks.0.attn.to_q', 'img_in', 'transformer_blocks.0.txt_mod.1')):
            o, i = S.w[name + '.weight'].shape
            down, up = _pair(g, o, i)
            m = None if n == 2 else magnitude(name)
            sd.update({f'transformer.{name}.lora_A.weight': down, f'transformer.{name}.lora_B.weight': up})
            if m is not None:
                sd['transformer.' + name + ('.lora_magnitude_vector', '.lora_magnitude_vector.weight')[n]] = m
            mods[name] = (down, up, 1.0, m)
    return sd, mods


def _reference(S, mods, w_arc, w_dora, call_scale):
    """{module: (t, E)} with the chained bound; w_arc / w_dora None = the adapter is not active."""
    out = {}
    for name in sorted(set(S.arc) | set(mods)):
        base = S.base_sd[name + '.weight'].bfloat16()
        A, B, Sc, gains, radius = [], [], [], [], []
        if w_arc is not None and name in S.arc and call_scale * w_arc != 0.0:
            A.append(S.arc[name][0]); B.append(S.arc[name][1]); Sc.append(call_scale * w_arc); gains.append(None); radius.append(None)
        if w_dora is not None and name in mods:
            a, b, factor, m = mods[name]
            s = call_scale * w_dora * factor
            if m is not None or s != 0.0:
                A.append(a); B.append(b); Sc.append(s)
                if m is None:
                    gains.append(None); radius.append(None)
                else:
                    gq, lo, hi = DR.gain_reference(base, a, b, s, m)
                    gains.append(gq); radius.append(torch.maximum(hi - gq, gq - lo))
        out[name] = DR.fold_rows_reference(base, A, B, Sc, gains, radius)
    return out


def test_dora_beside_the_arcflow_adapter(S):
    sd, mods = _dora_adapter(S)
    pipe = S.with_arcflow()
    plain = S.run(pipe)
    only = S.with_arcflow()
    assert pipe.load_lora_weights(dict(sd), adapter_name='dora') == 'dora'
    assert set(pipe._style['magnitude']['dora']) == {n for n, e in mods.items() if e[3] is not None}
    pipe.set_adapters([ARC, 'dora'], [1.0, 0.7])
    out = S.run(pipe, 0.9)
    ref = _reference(S, mods, 1.0, 0.7, 0.9)
    S.check_packed(pipe, ref)
    assert torch.isfinite(out).all() and rel_l2(out, plain) > FLOOR                 # finite, and not the latents without the adapter
    # the rows do have the magnitudes' lengths where the DoRA adapter is alone on a linear (what DoRA is for): loose, bf16 rows
    from arcflow_amd.weights import packed_row_slices
    alone = next(n for n, e in mods.items() if e[3] is not None and n not in S.arc)
    pname, r0, rows, _ = packed_row_slices(S.family, S.tcfg, True)[alone]
    got = pipe.transformer._weights[pname][r0:r0 + rows].double().norm(dim=1).cpu()
    assert torch.allclose(got, mods[alone][3].double(), rtol=2.0 ** -7)
    # another weight refolds to the new reference; the same state again folds nothing
    pipe.set_adapters([ARC, 'dora'], [0.5, -0.4])
    S.run(pipe)
    S.check_packed(pipe, _reference(S, mods, 0.5, -0.4, 1.0))
    folded = dict(pipe._style['folded'])
    gains = {k: v[1].data_ptr() for k, v in pipe._style['gain'].items()}
    S.run(pipe)
    assert pipe._style['folded'] == folded and {k: v[1].data_ptr() for k, v in pipe._style['gain'].items()} == gains
    # at weight 0 an active DoRA adapter still applies its magnitude: (m / ||W|| - 1) W
    pipe.set_adapters([ARC, 'dora'], [1.0, 0.0])
    S.run(pipe)
    ref0 = _reference(S, mods, 1.0, 0.0, 1.0)
    S.check_packed(pipe, ref0)
    t_without, _ = LR.fold_reference(S.base_sd[alone + '.weight'].bfloat16())
    assert bool((LR.rne_bf16(ref0[alone][0]) != LR.rne_bf16(t_without)).any())
    # left out of set_adapters it contributes nothing: the ArcFlow adapter alone
    pipe.set_adapters([ARC])
    S.run(pipe)
    S.check_packed(pipe, _reference(S, mods, 1.0, None, 1.0))
    # removal restores the earlier bits, by either door
    pipe.set_adapters([ARC, 'dora'])
    S.run(pipe)
    pipe.delete_adapters('dora')
    assert pipe._style is None and pipe.get_list_adapters() == {'transformer': [ARC]}
    _weights_equal(pipe, only)
    pipe.load_lora_weights(dict(sd), adapter_name='dora')
    S.run(pipe, 0.8)
    S.check_packed(pipe, _reference(S, mods, 1.0, 1.0, 0.8))
    pipe.unload_lora_weights()
    _weights_equal(pipe, only)
    assert torch.equal(S.run(pipe), plain)
