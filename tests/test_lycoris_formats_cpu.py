"""LyCORIS LoHa / LoKr tensors through ``lora_formats.convert_community_lora`` and ``parse_lora_state_dict``, on the tiny configs of
tests/test_lora_formats_cpu.py.  The rules (LoHa = (w1_a w1_b) (*) (w2_a w2_b), LoKr = kron(w1, w2), the alpha / rank factors) are restated here from
the issue that asked for them -- LyCORIS' arithmetic as recalled: this pins the module to those rules, not the rules to LyCORIS.  Small integers
make every product and sum exact in fp64, so "equal" means equal on any machine.  On the parent commit every test here fails: the keys are refused."""
import json
import warnings

import pytest
import torch

from test_lora_formats_cpu import FLUX, QWEN, SWAPPED, TABLE, _shapes

QKV, LIN1 = 'double_blocks.0.img_attn.qkv', 'single_blocks.0.linear1'


def _ints(g, *shape):
    return torch.randint(-4, 5, shape, generator=g).float()


def _loha(g, o, i, r1=2, r2=3):
    return {'hada_w1_a': _ints(g, o, r1), 'hada_w1_b': _ints(g, r1, i), 'hada_w2_a': _ints(g, o, r2), 'hada_w2_b': _ints(g, r2, i)}


def _lokr(g, o, i, c, d, low=()):
    """w1 [o / c, i / d], w2 [c, d]; the factors named in `low` as rank-2 pairs."""
    t = {}
    for n, (rows, cols) in (('lokr_w1', (o // c, i // d)), ('lokr_w2', (c, d))):
        if n[-2:] in low:
            t[n + '_a'], t[n + '_b'] = _ints(g, rows, 2), _ints(g, 2, cols)
        else:
            t[n] = _ints(g, rows, cols)
    return t


def _key(spelling, module, bfl=None):
    """A source key prefix for a diffusers `module` (or the BFL module `bfl`) in one of the accepted spellings."""
    name = bfl or module
    return {'unet': 'lora_unet_' + name.replace('.', '_'), 'transformer_': 'lora_transformer_' + name.replace('.', '_'),
            'dotted': 'diffusion_model.' + name, 'diffusers': 'transformer.' + name, 'bare': name}[spelling]


def _delta(e):
    """The fp64 delta of a parsed entry (all its rows: row0 is applied by the caller)."""
    if e['kind'] == 'loha':
        return (e['w1_a'].double() @ e['w1_b'].double()) * (e['w2_a'].double() @ e['w2_b'].double())
    w = [e[n].double() if e[n] is not None else e[n + '_a'].double() @ e[n + '_b'].double() for n in ('w1', 'w2')]
    return torch.kron(w[0], w[1])


def _convert(sd, family='flux', cfg=FLUX):
    from arcflow_amd.pipelines.arcflow_loader import parse_lora_state_dict
    from arcflow_amd.pipelines.lora_formats import convert_community_lora, needs_conversion
    if needs_conversion(sd):
        sd, mags, skipped = convert_community_lora(sd, family, cfg)
        assert not mags and not skipped
    return parse_lora_state_dict(sd)[0]


@pytest.mark.parametrize('kind', ['loha', 'lokr'])
def test_every_spelling_resolves_to_the_same_modules(kind):
    g = torch.Generator().manual_seed(1)
    mod = 'transformer_blocks.0.attn.to_out.0'                                     # BFL: double_blocks.0.img_attn.proj, [256, 256]
    t = _loha(g, 256, 256) if kind == 'loha' else _lokr(g, 256, 256, 16, 32, low=('w2',))
    got = []
    for spelling, bfl in (('unet', None), ('transformer_', None), ('dotted', None), ('diffusers', None), ('bare', None), ('unet', 'double_blocks.0.img_attn.proj'),
                          ('dotted', 'double_blocks.0.img_attn.proj')):
        k = _key(spelling, mod, bfl)
        mods = _convert({**{f'{k}.{n}': v for n, v in t.items()}, k + '.alpha': torch.tensor(4.0)})
        assert set(mods) == {mod}, (spelling, bfl)
        got.append(mods[mod])
    for e in got:
        assert e['kind'] == kind and e['alpha'] == 4.0
        assert torch.equal(_delta(e), _delta(got[0]))
        for n, v in t.items():
            assert torch.equal(e[n[len('hada_'):] if kind == 'loha' else n[len('lokr_'):]], v)
    if kind == 'lokr':
        assert got[0]['row0'] == 0 and got[0]['w2'] is None and got[0]['w1_a'] is None
    # Qwen-Image: underscored and dotted diffusers names
    qmod = 'transformer_blocks.1.attn.to_out.0'
    for spelling in ('unet', 'dotted', 'diffusers'):
        k = _key(spelling, qmod)
        assert set(_convert({f'{k}.{n}': v for n, v in t.items()}, 'qwen', QWEN)) == {qmod}


@pytest.mark.parametrize('bfl', [QKV, LIN1])
def test_fused_loha_parts_are_row_slices_of_the_fused_delta(bfl):
    g = torch.Generator().manual_seed(2)
    shapes = _shapes('flux', FLUX)
    parts = TABLE[bfl]
    sizes = [shapes[p + '.weight'][0] for p in parts]
    t = _loha(g, sum(sizes), 256)
    k = _key('unet', None, bfl)
    mods = _convert({**{f'{k}.{n}': v for n, v in t.items()}, k + '.alpha': torch.tensor(6.0)})
    assert set(mods) == set(parts)
    fused = (t['hada_w1_a'].double() @ t['hada_w1_b'].double()) * (t['hada_w2_a'].double() @ t['hada_w2_b'].double())
    r0 = 0
    for p, n in zip(parts, sizes):
        e = mods[p]
        assert e['kind'] == 'loha' and e['alpha'] == 6.0 and e['w1_b'] is t['hada_w1_b'] and e['w2_b'] is t['hada_w2_b']          # the _b tensors are shared
        assert torch.equal(e['w1_a'], t['hada_w1_a'][r0:r0 + n]) and torch.equal(e['w2_a'], t['hada_w2_a'][r0:r0 + n])
        assert torch.equal(_delta(e), fused[r0:r0 + n]), p                       # exactly
        r0 += n
    assert sizes == ([256, 256, 256, 1024] if bfl == LIN1 else [256, 256, 256])


@pytest.mark.parametrize('bfl,c,d,low', [(QKV, 32, 16, ()), (QKV, 48, 64, ('w1',)), (LIN1, 56, 8, ('w2',)), (LIN1, 64, 32, ('w1', 'w2'))])
def test_fused_lokr_parts_share_the_factors_and_carry_row0(bfl, c, d, low):
    from arcflow_amd.pipelines.lora_formats import convert_community_lora, lokr_shapes
    g = torch.Generator().manual_seed(3)
    shapes = _shapes('flux', FLUX)
    parts = TABLE[bfl]
    sizes = [shapes[p + '.weight'][0] for p in parts]
    O = sum(sizes)
    t = _lokr(g, O, 256, c, d, low)
    k = _key('dotted', None, bfl)
    out, _, _ = convert_community_lora({f'{k}.{n}': v for n, v in t.items()}, 'flux', FLUX)
    mods = _convert({f'{k}.{n}': v for n, v in t.items()})
    fused = None
    r0 = 0
    for p, n in zip(parts, sizes):
        e = mods[p]
        assert e['kind'] == 'lokr' and e['row0'] == r0 and e['alpha'] is None and lokr_shapes(e) == (O // c, 256 // d, c, d)
        row0 = out[f'transformer.{p}.lokr_row0']
        assert row0.dtype == torch.int64 and row0.dim() == 0 and int(row0) == r0  # an integer scalar next to the factors
        for name, v in t.items():
            assert e[name[len('lokr_'):]] is v                                    # both factors, whole, on every part
        fused = _delta(e) if fused is None else fused
        assert tuple(fused.shape) == (O, 256)
        # the part's delta by the index rule at row0 equals its rows of the fused delta, exactly
        w1, w2 = [e[f].double() if e[f] is not None else e[f + '_a'].double() @ e[f + '_b'].double() for f in ('w1', 'w2')]
        rows, cols = torch.arange(n) + r0, torch.arange(256)
        part = w1[(rows // c)[:, None], (cols // d)[None, :]] * w2[(rows % c)[:, None], (cols % d)[None, :]]
        assert torch.equal(part, fused[r0:r0 + n]), p
        r0 += n
    # an unfused module carries no row0 key and reads back as row0 = 0
    k = _key('unet', 'x_embedder')
    t1 = _lokr(g, 256, 64, 16, 8)
    out, _, _ = convert_community_lora({f'{k}.{n}': v for n, v in t1.items()}, 'flux', FLUX)
    assert set(out) == {'transformer.x_embedder.lokr_w1', 'transformer.x_embedder.lokr_w2'} and _convert(out)['x_embedder']['row0'] == 0


def test_factor_rules():
    from arcflow_amd.pipelines.lora_formats import lycoris_factor
    g = torch.Generator().manual_seed(4)
    k = _key('unet', 'x_embedder')

    def factor(t, alpha=6.0):
        sd = {f'{k}.{n}': v for n, v in t.items()}
        if alpha is not None:
            sd[k + '.alpha'] = torch.tensor(alpha)
        return lycoris_factor(_convert(sd)['x_embedder'])
    assert factor(_loha(g, 256, 64, r1=2, r2=3)) == 6.0 / 2                        # LoHa: alpha / r
    assert factor(_loha(g, 256, 64), alpha=None) == 1.0
    assert factor(_lokr(g, 256, 64, 16, 8)) == 1.0                                 # both factors dense: 1, whatever alpha says
    assert factor(_lokr(g, 256, 64, 16, 8, low=('w2',))) == 6.0 / 2                # the rank of the low-rank factor
    assert factor(_lokr(g, 256, 64, 16, 8, low=('w1',))) == 6.0 / 2
    t = _lokr(g, 256, 64, 16, 8, low=('w1',))
    t['lokr_w2_a'], t['lokr_w2_b'] = _ints(g, 16, 3), _ints(g, 3, 8)
    del t['lokr_w2']
    assert factor(t) == 6.0 / 3                                                    # both low-rank: w2's rank
    assert factor(_lokr(g, 256, 64, 16, 8, low=('w2',)), alpha=None) == 1.0


def test_adaln_half_swap():
    g = torch.Generator().manual_seed(5)
    k = _key('unet', None, SWAPPED)
    t = _loha(g, 512, 256)
    e = _convert({f'{k}.{n}': v for n, v in t.items()})['norm_out.linear']
    for n in ('w1', 'w2'):
        src = t[f'hada_{n}_a']
        assert torch.equal(e[n + '_a'][:256], src[256:]) and torch.equal(e[n + '_a'][256:], src[:256]) and e[n + '_b'] is t[f'hada_{n}_b']
    fused = (t['hada_w1_a'].double() @ t['hada_w1_b'].double()) * (t['hada_w2_a'].double() @ t['hada_w2_b'].double())
    assert torch.equal(_delta(e), torch.cat([fused[256:], fused[:256]]))
    with pytest.raises(ValueError, match='LoKr') as err:                           # a Kronecker product cannot be reordered by rows
        _convert({f'{k}.{n}': v for n, v in _lokr(g, 512, 256, 32, 16).items()})
    assert k + '.lokr_w1' in str(err.value)


def test_refusals_name_the_key():
    from arcflow_amd.pipelines.arcflow_loader import parse_lora_state_dict
    from arcflow_amd.pipelines.lora_formats import convert_community_lora
    g = torch.Generator().manual_seed(6)
    k = _key('unet', 'x_embedder')
    z = torch.zeros(4, 4)
    loha, lokr = _loha(g, 256, 64), _lokr(g, 256, 64, 16, 8)

    def sd_of(t, prefix=k, **extra):
        return {**{f'{prefix}.{n}': v for n, v in t.items()}, **{f'{prefix}.{n}': v for n, v in extra.items()}}
    cases = [(sd_of(loha, hada_t1=torch.zeros(2, 2, 1, 1)), k + '.hada_t1', 'Tucker'),
             (sd_of(loha, hada_t2=z), k + '.hada_t2', 'Tucker'),
             (sd_of(lokr, lokr_t2=z), k + '.lokr_t2', 'Tucker'),
             (sd_of(dict(loha, hada_w1_a=torch.zeros(256, 2, 1, 1))), k + '.hada_w1_a', '4-D'),
             (sd_of(loha, diff=z), k + '.diff', 'diff'),
             (sd_of(loha, diff_b=z), k + '.diff_b', 'diff'),
             (sd_of(loha, dora_scale=torch.ones(256)), k + '.dora_scale', 'magnitude on the LoHa / LoKr module'),
             (sd_of(lokr, dora_scale=torch.ones(256)), k + '.dora_scale', 'magnitude on the LoHa / LoKr module'),
             (sd_of(lokr, 'transformer.x_embedder', lora_magnitude_vector=torch.ones(256)), 'transformer.x_embedder.lora_magnitude_vector',
              'magnitude on the LoHa / LoKr module'),
             (sd_of(_lokr(g, 128, 64, 16, 8)), k + '.lokr_w1', r'\[128, 64\] \(a c x b d\)'),                        # a c != O
             (sd_of(_lokr(g, 256, 128, 16, 8)), k + '.lokr_w1', r'\[256, 128\] \(a c x b d\)'),                      # b d != I
             (sd_of(_loha(g, 128, 64)), k + '.hada_w1_a', 'do not give'),
             (sd_of({n: v for n, v in loha.items() if n != 'hada_w2_b'}), k + '.hada_w1_a', 'LoHa module .* is incomplete: no hada_w2_b'),
             (sd_of({'lokr_w1': lokr['lokr_w1']}), k + '.lokr_w1', 'LoKr module .* is incomplete'),
             (sd_of({'lokr_w1': lokr['lokr_w1'], 'lokr_w2_a': z}), k + '.lokr_w1', 'LoKr module .* is incomplete'),
             (sd_of(dict(lokr, lokr_w2_a=z, lokr_w2_b=z)), k + '.lokr_w1', 'LoKr module .* is incomplete'),        # dense and a pair at once
             (sd_of({**loha, 'lokr_w1': z}), k + '.hada_w1_a', 'one kind per file'),
             (sd_of(loha, **{'lora_down.weight': torch.zeros(2, 64)}), k + '.lora_down.weight', 'one kind per file'),
             (sd_of(lokr, lokr_row0=torch.tensor(0)), k + '.lokr_row0', 'written by the conversion'),
             (sd_of(dict(loha, hada_w1_b=torch.zeros(3, 64))), k + '.hada_w1_a', 'share no rank')]
    for sd, key, what in cases:
        with pytest.raises(ValueError, match=what) as err:
            convert_community_lora(sd, 'flux', FLUX)
        assert key in str(err.value), (key, str(err.value))
    # the parser's own refusals, on the diffusers layout
    d = 'transformer.x_embedder'
    for sd, key, what in [(sd_of({n: v for n, v in loha.items() if n != 'hada_w1_a'}, d), d + '.hada_w1_b', 'LoHa module .* is incomplete'),
                          (sd_of({'lokr_w2': lokr['lokr_w2']}, d), d + '.lokr_w2', 'LoKr module .* is incomplete'),
                          (sd_of({}, d, lokr_row0=torch.tensor(64)), d + '.lokr_row0', 'LoKr module .* is incomplete'),
                          (sd_of(loha, d, hada_t1=z), d + '.hada_t1', 'Tucker'),
                          (sd_of(lokr, d, diff=z), d + '.diff', 'diff'),
                          (sd_of(lokr, d, lokr_row0=torch.tensor(1.5)), d + '.lokr_row0', 'integer scalar'),
                          (sd_of(loha, d, lokr_row0=torch.tensor(64)), d + '.hada_w1_a', 'belongs to LoKr'),
                          (sd_of(loha, d, **{'lora_A.weight': torch.zeros(2, 64), 'lora_B.weight': torch.zeros(256, 2)}), d + '.hada_w1_a', 'one kind per file')]:
        with pytest.raises(ValueError, match=what) as err:
            parse_lora_state_dict(sd)
        assert key in str(err.value), (key, str(err.value))


def test_loader_checks_shapes_and_keeps_the_operand_formats():
    """The registry of tests/test_lora_adapters_cpu.py (device fold stubbed): LoHa operands stay bf16, LoKr factors become dense fp32 (a low-rank factor
    multiplied out once), every shape is checked against the linear, a magnitude on a LoHa / LoKr module is refused."""
    from test_lora_adapters_cpu import _pipe
    pipe, w, folds = _pipe()
    g = torch.Generator().manual_seed(7)
    k = _key('unet', None, QKV)
    lokr = _lokr(g, 768, 256, 48, 64, low=('w2',))
    sd = {**{f'{k}.{n}': v for n, v in lokr.items()}, k + '.alpha': torch.tensor(4.0),
          **{f'transformer.x_embedder.{n}': v for n, v in _loha(g, 256, 64, 2, 3).items()}, 'transformer.x_embedder.alpha': torch.tensor(3.0)}
    assert pipe.load_lora_weights(sd, adapter_name='lyco') == 'lyco' and not folds
    mods = pipe._style['loras']['lyco']
    assert set(mods) == set(TABLE[QKV]) | {'x_embedder'}
    e = mods['x_embedder']
    assert e['kind'] == 'loha' and e['factor'] == 3.0 / 2 and all(e[n].dtype == torch.bfloat16 for n in ('w1_a', 'w1_b', 'w2_a', 'w2_b'))
    assert tuple(e['w1_a'].shape) == (256, 2) and tuple(e['w2_b'].shape) == (3, 64)
    for n, p in enumerate(TABLE[QKV]):
        e = mods[p]
        assert e['kind'] == 'lokr' and e['row0'] == 256 * n and e['factor'] == 4.0 / 2
        assert e['w1'].dtype == e['w2'].dtype == torch.float32 and tuple(e['w1'].shape) == (16, 4) and tuple(e['w2'].shape) == (48, 64)
        assert torch.equal(e['w1'], lokr['lokr_w1']) and torch.equal(e['w2'], lokr['lokr_w2_a'] @ lokr['lokr_w2_b'])      # small integers: exact
    assert set(TABLE[QKV]) <= set(pipe._style['base'])
    d = 'transformer.transformer_blocks.0.attn.to_q.'
    for bad, what in (({d + n: v for n, v in _lokr(g, 512, 256, 32, 16).items()}, 'does not fit it'),                    # a c != O without a row0
                      ({**{d + n: v for n, v in _lokr(g, 512, 256, 32, 16).items()}, d + 'lokr_row0': torch.tensor(320)}, 'does not fit it'),
                      ({**{d + n: v for n, v in _lokr(g, 512, 256, 32, 16).items()}, d + 'lokr_row0': torch.tensor(-64)}, 'does not fit it'),
                      ({d + n: v for n, v in _lokr(g, 256, 128, 32, 16).items()}, 'does not fit it'),                    # b d != I
                      ({d + n: v for n, v in _loha(g, 256, 128).items()}, 'do not fit it'),
                      ({d + n: v for n, v in _loha(g, 128, 256).items()}, 'do not fit it'),
                      ({**{d + n: v for n, v in _loha(g, 256, 256).items()}, d + 'lora_magnitude_vector': torch.ones(256)}, 'magnitude on the LoHa / LoKr module'),
                      ({'transformer.transformer_blocks.7.attn.to_q.' + n: v for n, v in _loha(g, 256, 256).items()}, 'no linear')):
        with pytest.raises(ValueError, match=what):
            pipe.load_lora_weights(bad, adapter_name='bad')
    good = {**{d + n: v for n, v in _lokr(g, 512, 256, 32, 16).items()}, d + 'lokr_row0': torch.tensor(256)}           # rows 256 .. 512 of a taller delta
    assert pipe.load_lora_weights(good, adapter_name='tall') == 'tall'
    assert pipe.get_list_adapters() == {'transformer': ['transformer_arcflow', 'lyco', 'tall']}
    pipe.delete_adapters(['lyco', 'tall'])
    assert pipe._style is None


def test_convert_tool_round_trip(tmp_path):
    """tools/convert_lora.py writes a file that loads, through the same door, to the entries the in-memory conversion gives."""
    from safetensors.torch import load_file, save_file
    from arcflow_amd.pipelines.lora_formats import needs_conversion
    from tools import convert_lora
    g = torch.Generator().manual_seed(8)
    sd = {}
    for prefix, t in ((_key('unet', None, QKV), _lokr(g, 768, 256, 48, 64, low=('w1',))), (_key('unet', None, LIN1), _loha(g, 1792, 256)),
                      (_key('unet', None, SWAPPED), _loha(g, 512, 256)), (_key('dotted', 'x_embedder'), _lokr(g, 256, 64, 16, 8))):
        sd.update({f'{prefix}.{n}': v for n, v in t.items()})
        sd[prefix + '.alpha'] = torch.tensor(5.0)
    k = _key('unet', None, 'double_blocks.0.img_mlp.0')
    sd.update({k + '.lora_down.weight': _ints(g, 2, 256), k + '.lora_up.weight': _ints(g, 1024, 2)})               # a plain LoRA module in the same file
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / 'lyco.safetensors'))
    (tmp_path / 'config.json').write_text(json.dumps(FLUX))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        convert_lora.main([str(tmp_path / 'lyco.safetensors'), str(tmp_path / 'out.safetensors'), '--family', 'flux', '--transformer-config',
                           str(tmp_path / 'config.json')])
    back = load_file(str(tmp_path / 'out.safetensors'))
    assert all(key.startswith('transformer.') for key in back) and not needs_conversion(back)
    assert sum(key.endswith('.lokr_row0') for key in back) == 3 and back['transformer.transformer_blocks.0.attn.to_v.lokr_row0'].item() == 512
    want, got = _convert(sd), _convert(back)
    assert set(got) == set(want) == set(TABLE[QKV] + TABLE[LIN1] + ['norm_out.linear', 'x_embedder', 'transformer_blocks.0.ff.net.0.proj'])
    for m, e in want.items():
        assert set(got[m]) == set(e), m
        for n, v in e.items():
            assert torch.equal(got[m][n], v) if isinstance(v, torch.Tensor) else got[m][n] == v, (m, n)
