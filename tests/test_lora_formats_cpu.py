"""``arcflow_amd.pipelines.lora_formats``: Kohya / ComfyUI layouts and DoRA magnitudes into the layout ``parse_lora_state_dict`` accepts.  The
BFL <-> diffusers table is restated here from the issue that asked for it (diffusers' conversion as recalled): this pins the module to that
table, not the table to diffusers.  On the parent commit the module does not exist."""
import warnings

import pytest
import torch

FLUX = dict(num_layers=1, num_single_layers=1, num_attention_heads=2, attention_head_dim=128, in_channels=64, joint_attention_dim=128,
            pooled_projection_dim=64, guidance_embeds=True)
QWEN = dict(num_layers=2, num_attention_heads=2, attention_head_dim=128, in_channels=64, joint_attention_dim=192)
T, S, E = 'transformer_blocks.0.', 'single_transformer_blocks.0.', 'time_text_embed.'
TABLE = {                                                        # BFL module -> diffusers modules, in row order
    'double_blocks.0.img_attn.qkv': [T + 'attn.to_q', T + 'attn.to_k', T + 'attn.to_v'],
    'double_blocks.0.txt_attn.qkv': [T + 'attn.add_q_proj', T + 'attn.add_k_proj', T + 'attn.add_v_proj'],
    'double_blocks.0.img_attn.proj': [T + 'attn.to_out.0'],
    'double_blocks.0.txt_attn.proj': [T + 'attn.to_add_out'],
    'double_blocks.0.img_mlp.0': [T + 'ff.net.0.proj'],
    'double_blocks.0.img_mlp.2': [T + 'ff.net.2'],
    'double_blocks.0.txt_mlp.0': [T + 'ff_context.net.0.proj'],
    'double_blocks.0.txt_mlp.2': [T + 'ff_context.net.2'],
    'double_blocks.0.img_mod.lin': [T + 'norm1.linear'],
    'double_blocks.0.txt_mod.lin': [T + 'norm1_context.linear'],
    'single_blocks.0.linear1': [S + 'attn.to_q', S + 'attn.to_k', S + 'attn.to_v', S + 'proj_mlp'],
    'single_blocks.0.linear2': [S + 'proj_out'],
    'single_blocks.0.modulation.lin': [S + 'norm.linear'],
    'img_in': ['x_embedder'],
    'txt_in': ['context_embedder'],
    'time_in.in_layer': [E + 'timestep_embedder.linear_1'],
    'time_in.out_layer': [E + 'timestep_embedder.linear_2'],
    'vector_in.in_layer': [E + 'text_embedder.linear_1'],
    'vector_in.out_layer': [E + 'text_embedder.linear_2'],
    'guidance_in.in_layer': [E + 'guidance_embedder.linear_1'],
    'guidance_in.out_layer': [E + 'guidance_embedder.linear_2'],
    'final_layer.adaLN_modulation.1': ['norm_out.linear'],
}
SWAPPED = 'final_layer.adaLN_modulation.1'
R = 4


def _shapes(family, cfg, student=True):
    from arcflow_amd.weights import expected_transformer_keys
    return expected_transformer_keys(family, cfg, student)


def _kohya(spelling, dora=False, seed=0):
    """Every row of TABLE once -> (state dict, {bfl: (down fp32, up fp32, alpha, magnitude or None)})."""
    shapes = _shapes('flux', FLUX)
    g = torch.Generator().manual_seed(seed)
    sd, src = {}, {}
    for n, (bfl, parts) in enumerate(TABLE.items()):
        o, i = sum(shapes[p + '.weight'][0] for p in parts), shapes[parts[0] + '.weight'][1]
        # small integers: every product and sum below is exact in fp64 in any order, so "equal" means equal on any machine
        down, up = torch.randint(-8, 9, (R, i), generator=g).float(), torch.randint(-8, 9, (o, R), generator=g).float()
        alpha = torch.tensor(float(n + 1))
        m = torch.rand(o, generator=g) + 0.5 if dora else None
        if spelling == 'underscored':
            k = 'lora_unet_' + bfl.replace('.', '_')
            sd.update({k + '.lora_down.weight': down, k + '.lora_up.weight': up, k + '.alpha': alpha})
        else:
            k = 'diffusion_model.' + bfl
            sd.update({k + '.lora_A.weight': down, k + '.lora_B.weight': up, k + '.alpha': alpha})
        if dora:
            sd[k + '.dora_scale'] = (m, m[:, None], m[None, :])[n % 3]            # [O], [O, 1], [1, O]
        src[bfl] = (down, up, alpha, m)
    return sd, src


@pytest.mark.parametrize('spelling', ['underscored', 'dotted'])
def test_bfl_names_cover_the_table(spelling):
    from arcflow_amd.pipelines.arcflow_loader import parse_lora_state_dict
    from arcflow_amd.pipelines.lora_formats import convert_community_lora, needs_conversion
    shapes = _shapes('flux', FLUX)
    sd, src = _kohya(spelling, dora=True)
    assert needs_conversion(sd)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        out, mags, skipped = convert_community_lora(sd, 'flux', FLUX, student=True)
    assert not rec and skipped == []
    mods, n_te = parse_lora_state_dict(out)                                        # the unchanged parser takes it
    assert n_te == 0 and set(mods) == {p for parts in TABLE.values() for p in parts} == set(mags)
    for bfl, parts in TABLE.items():
        down, up, alpha, m = src[bfl]
        if bfl == SWAPPED:                                                         # diffusers keeps scale before shift: the halves change places
            h = up.shape[0] // 2
            up, m = torch.cat([up[h:], up[:h]]), torch.cat([m[h:], m[:h]])
            assert torch.equal(mods['norm_out.linear']['B'][:h], src[bfl][1][h:]) and torch.equal(mods['norm_out.linear']['B'][h:], src[bfl][1][:h])
        got = torch.cat([mods[p]['B'].double() @ mods[p]['A'].double() for p in parts])
        assert torch.equal(got, up.double() @ down.double()), bfl                  # exactly: the same rows times the same matrix
        assert torch.equal(torch.cat([mags[p] for p in parts]), m), bfl
        for p in parts:
            assert tuple(mods[p]['B'].shape) == (shapes[p + '.weight'][0], R) and tuple(mods[p]['A'].shape) == (R, shapes[p + '.weight'][1]), p
            assert mods[p]['A'] is down and mods[p]['alpha'] == float(alpha), p    # one shared lora_A, alpha on every part
            assert mags[p].dtype == torch.float32 and mags[p].dim() == 1
    # linear1 is q, k, v of D rows each and then the 4 D rows of proj_mlp: sizes from the expected keys, not an equal split
    assert [mods[p]['B'].shape[0] for p in TABLE['single_blocks.0.linear1']] == [256, 256, 256, 1024]


def test_final_layer_linear_and_text_encoder_keys_are_skipped_with_one_warning():
    from arcflow_amd.pipelines.lora_formats import convert_community_lora
    sd, _ = _kohya('underscored')
    te = {'lora_te1_text_model_encoder_layers_0_self_attn_q_proj.lora_down.weight': torch.zeros(4, 8),
          'lora_te1_text_model_encoder_layers_0_self_attn_q_proj.lora_up.weight': torch.zeros(8, 4),
          'lora_te2_encoder_block_0_layer_0_SelfAttention_q.alpha': torch.tensor(4.0)}
    head = {'lora_unet_final_layer_linear.lora_down.weight': torch.zeros(4, 256), 'lora_unet_final_layer_linear.lora_up.weight': torch.zeros(64, 4)}
    want, _, _ = convert_community_lora(sd, 'flux', FLUX)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        out, _, skipped = convert_community_lora({**sd, **te, **head}, 'flux', FLUX, student=True)
    assert len(rec) == 1 and '3 text-encoder LoRA tensors were skipped' in str(rec[0].message) and 'final_layer.linear' in str(rec[0].message)
    assert sorted(skipped) == sorted(list(te) + list(head)) and set(out) == set(want)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        convert_community_lora({**sd, **te}, 'flux', FLUX)
    assert len(rec) == 1 and '3 text-encoder LoRA tensors were skipped' in str(rec[0].message) and 'final_layer' not in str(rec[0].message)
    with warnings.catch_warnings(record=True) as rec:                              # only the head: the warning speaks of the head alone
        warnings.simplefilter('always')
        convert_community_lora({**sd, **head}, 'flux', FLUX)
    assert len(rec) == 1 and str(rec[0].message).startswith('2 `final_layer.linear` tensors were skipped') and 'text-encoder' not in str(rec[0].message)
    # the teacher does have proj_out
    out, _, skipped = convert_community_lora(head, 'flux', FLUX, student=False)
    assert skipped == [] and set(out) == {'transformer.proj_out.lora_A.weight', 'transformer.proj_out.lora_B.weight'}


@pytest.mark.parametrize('family,cfg', [('flux', FLUX), ('qwen', QWEN)])
def test_underscored_diffusers_names_resolve(family, cfg):
    from arcflow_amd.pipelines.arcflow_loader import parse_lora_state_dict
    from arcflow_amd.pipelines.lora_formats import convert_community_lora
    from arcflow_amd.weights import packed_row_slices
    slices = packed_row_slices(family, cfg, True)
    sd, want = {}, {}
    for n, (name, (_, _, rows, in_f)) in enumerate(slices.items()):                # every linear the transformer has
        prefix = ('lora_unet_', 'lora_transformer_')[n % 2]
        k = prefix + name.replace('.', '_')
        sd[k + '.lora_down.weight'], sd[k + '.lora_up.weight'] = torch.full((2, in_f), float(n)), torch.full((rows, 2), float(n))
        want[name] = float(n)
    out, mags, skipped = convert_community_lora(sd, family, cfg)
    mods, _ = parse_lora_state_dict(out)
    assert not mags and not skipped and set(mods) == set(slices)
    for name, n in want.items():
        assert mods[name]['A'][0, 0] == n and mods[name]['B'][0, 0] == n and mods[name]['alpha'] is None, name
    if family == 'qwen':                                                           # ComfyUI's dotted spelling of diffusers names
        k = 'diffusion_model.transformer_blocks.1.attn.to_out.0'
        out, _, _ = convert_community_lora({k + '.lora_A.weight': torch.zeros(2, 256), k + '.lora_B.weight': torch.zeros(256, 2)}, family, cfg)
        assert set(out) == {'transformer.transformer_blocks.1.attn.to_out.0.lora_A.weight', 'transformer.transformer_blocks.1.attn.to_out.0.lora_B.weight'}
        with pytest.raises(ValueError, match='lora_unet_double_blocks_0_img_attn_qkv'):       # BFL names are FLUX's
            convert_community_lora({'lora_unet_double_blocks_0_img_attn_qkv.lora_down.weight': torch.zeros(2, 256)}, family, cfg)


def test_refusals_name_the_key():
    from arcflow_amd.pipelines.lora_formats import convert_community_lora
    z = torch.zeros(4, 4)
    for key, what in (('lora_unet_double_blocks_7_img_attn_qkv.lora_down.weight', 'no module'),          # the tiny model has one double block
                      ('lora_unet_double_blocks_0_img_attn_nope.lora_up.weight', 'no module'),
                      ('diffusion_model.double_blocks.0.img_attn.nope.lora_A.weight', 'no module'),
                      ('lora_unet_double_blocks_0_img_attn_qkv.weird', 'not a LoRA key'),
                      ('lora_unet_double_blocks_0_img_attn_qkv.hada_w1_a', 'LoHa'),
                      ('lora_unet_double_blocks_0_img_attn_qkv.lokr_w1', 'LoKr'),
                      ('lora_unet_double_blocks_0_img_attn_qkv.diff', 'diff'),
                      ('diffusion_model.double_blocks.0.img_attn.qkv.diff_b', 'diff'),
                      ('lora_unet_img_in.lora_mid.weight', 'lora_mid')):
        with pytest.raises(ValueError, match=what) as e:
            convert_community_lora({key: z}, 'flux', FLUX)
        assert key in str(e.value), key
    with pytest.raises(ValueError, match='LyCORIS') as e:                          # a convolution LoRA
        convert_community_lora({'lora_unet_img_in.lora_down.weight': torch.zeros(4, 64, 1, 1)}, 'flux', FLUX)
    assert 'lora_unet_img_in.lora_down.weight' in str(e.value)
    with pytest.raises(ValueError, match='incomplete'):
        convert_community_lora({'lora_unet_img_in.lora_down.weight': torch.zeros(4, 64)}, 'flux', FLUX)
    with pytest.raises(ValueError, match='768 rows'):                              # a fused tensor of the wrong height
        convert_community_lora({'lora_unet_double_blocks_0_img_attn_qkv.lora_down.weight': torch.zeros(4, 256),
                                'lora_unet_double_blocks_0_img_attn_qkv.lora_up.weight': torch.zeros(512, 4)}, 'flux', FLUX)
    with pytest.raises(ValueError, match=r'\[O\], \[O, 1\] or \[1, O\]'):
        convert_community_lora({'lora_unet_img_in.dora_scale': torch.zeros(2, 128)}, 'flux', FLUX)
    with pytest.raises(ValueError, match='256 output rows'):                       # a magnitude over the input axis: 64 elements for 256 rows
        convert_community_lora({'lora_unet_img_in.lora_down.weight': torch.zeros(4, 64), 'lora_unet_img_in.lora_up.weight': torch.zeros(256, 4),
                                'lora_unet_img_in.dora_scale': torch.zeros(1, 64)}, 'flux', FLUX)


def test_peft_magnitudes_leave_the_other_keys_alone():
    from arcflow_amd.pipelines.arcflow_loader import parse_lora_state_dict
    from arcflow_amd.pipelines.lora_formats import convert_community_lora, needs_conversion
    a, b, m = torch.randn(4, 64), torch.randn(256, 4), torch.rand(256) + 0.5
    for spelling in ('lora_magnitude_vector', 'lora_magnitude_vector.weight', 'lora_magnitude_vector.default.weight'):
        sd = {'transformer.x_embedder.lora_A.weight': a, 'transformer.x_embedder.lora_B.weight': b, f'transformer.x_embedder.{spelling}': m,
              'transformer_blocks.0.attn.to_q.lora_A.default.weight': torch.zeros(4, 256), 'transformer_blocks.0.attn.to_q.lora_B.default.weight': torch.zeros(256, 4)}
        assert needs_conversion(sd)
        out, mags, skipped = convert_community_lora(sd, 'flux', FLUX)
        assert set(mags) == {'x_embedder'} and torch.equal(mags['x_embedder'], m) and not skipped
        assert set(out) == set(sd) - {f'transformer.x_embedder.{spelling}'} and all(out[k] is sd[k] for k in out)
        assert set(parse_lora_state_dict(out)[0]) == {'x_embedder', 'transformer_blocks.0.attn.to_q'}
    assert not needs_conversion({'transformer.x_embedder.lora_A.weight': a, 'x_embedder.alpha': torch.tensor(1.0)})


def test_convert_tool_round_trip(tmp_path):
    """tools/convert_lora.py writes a file that reads back, through the same door, as what the in-memory conversion gives."""
    import json
    from safetensors.torch import load_file, save_file
    from arcflow_amd.pipelines.arcflow_loader import parse_lora_state_dict
    from arcflow_amd.pipelines.lora_formats import convert_community_lora
    from tools import convert_lora
    sd, _ = _kohya('underscored', dora=True)
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / 'kohya.safetensors'))
    (tmp_path / 'config.json').write_text(json.dumps(FLUX))
    convert_lora.main([str(tmp_path / 'kohya.safetensors'), str(tmp_path / 'out.safetensors'), '--family', 'flux', '--transformer-config',
                       str(tmp_path / 'config.json')])
    back = load_file(str(tmp_path / 'out.safetensors'))
    assert all(k.startswith('transformer.') for k in back) and sum(k.endswith('.lora_magnitude_vector') for k in back) == sum(len(p) for p in TABLE.values())
    want_sd, want_mags, _ = convert_community_lora(sd, 'flux', FLUX)
    got_sd, got_mags, _ = convert_community_lora(back, 'flux', FLUX)
    want, got = parse_lora_state_dict(want_sd)[0], parse_lora_state_dict(got_sd)[0]
    assert set(got) == set(want) and set(got_mags) == set(want_mags)
    for m in want:
        assert torch.equal(got[m]['A'], want[m]['A']) and torch.equal(got[m]['B'], want[m]['B']) and got[m]['alpha'] == want[m]['alpha'], m
        assert torch.equal(got_mags[m], want_mags[m]), m


def test_load_lora_weights_takes_the_community_layout():
    """The registry of tests/test_lora_adapters_cpu.py (device fold stubbed): a Kohya file lands as its diffusers modules, magnitudes beside them."""
    from test_lora_adapters_cpu import _pipe
    pipe, w, folds = _pipe()
    sd, src = _kohya('underscored', dora=True)
    keep = ('lora_unet_double_blocks_0_img_attn_qkv', 'lora_unet_single_blocks_0_linear1', 'lora_unet_img_in', 'lora_te1_x')
    sd = {k: v for k, v in sd.items() if k.startswith(keep)}
    sd['lora_te1_x.lora_down.weight'] = torch.zeros(4, 8)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        assert pipe.load_lora_weights(sd, adapter_name='kohya') == 'kohya'
    assert len(rec) == 1 and '1 text-encoder' in str(rec[0].message)
    mods = pipe._style['loras']['kohya']
    want = set(TABLE['double_blocks.0.img_attn.qkv'] + TABLE['single_blocks.0.linear1'] + ['x_embedder'])
    assert set(mods) == want == set(pipe._style['magnitude']['kohya'])
    down, up, alpha, m = src['double_blocks.0.img_attn.qkv']
    A, B, factor = mods['transformer_blocks.0.attn.to_k']
    assert torch.equal(A, down.bfloat16()) and torch.equal(B, up[256:512].bfloat16()) and factor == float(alpha) / R
    assert torch.equal(pipe._style['magnitude']['kohya']['transformer_blocks.0.attn.to_k'], m[256:512])
    assert pipe._style['magnitude']['kohya']['x_embedder'].dtype == torch.float32
    # a magnitude without its pair, and a magnitude of the wrong length, leave no trace
    with pytest.raises(ValueError, match='no lora_A / lora_B pair'):
        pipe.load_lora_weights({'transformer.x_embedder.lora_A.weight': torch.zeros(4, 64), 'transformer.x_embedder.lora_B.weight': torch.zeros(256, 4),
                                'transformer.context_embedder.lora_magnitude_vector': torch.ones(256)}, adapter_name='bad')
    with pytest.raises(ValueError, match='256 output rows'):
        pipe.load_lora_weights({'transformer.x_embedder.lora_A.weight': torch.zeros(4, 64), 'transformer.x_embedder.lora_B.weight': torch.zeros(256, 4),
                                'transformer.x_embedder.lora_magnitude_vector': torch.ones(64)}, adapter_name='bad')
    assert pipe.get_list_adapters() == {'transformer': ['transformer_arcflow', 'kohya']} and 'bad' not in pipe._style['magnitude']
    pipe.delete_adapters('kohya')
    assert pipe._style is None
