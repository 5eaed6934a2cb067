"""Style LoRAs next to the ArcFlow adapter, everything that needs no GPU: the map from diffusers modules to packed rows against the pack
functions, key parsing, the adapter registry of the pipelines (the device fold stubbed), the fp64 fold reference on its own
(tests/lora_fold_ref.py) and the argument checks of ``afx_lora_fold`` (they run on the host, before any launch)."""
import ctypes as C
import warnings

import pytest
import torch

import lora_fold_ref as LR

FLUX = dict(num_layers=1, num_single_layers=1, num_attention_heads=2, attention_head_dim=128, in_channels=64, joint_attention_dim=128,
            pooled_projection_dim=64, guidance_embeds=True)
QWEN = dict(num_layers=2, num_attention_heads=2, attention_head_dim=128, in_channels=64, joint_attention_dim=192)


def _iota_state_dict(family, cfg, student):
    """Every tensor of the expected layout filled with small integers (exact in bf16): row i of the n-th tensor holds (37 n + i) % 251 + column % 2, so
    a slice taken from the wrong tensor, or from the right one at the wrong row, differs."""
    from arcflow_amd.weights import expected_transformer_keys
    sd = {}
    for n, (k, shape) in enumerate(sorted(expected_transformer_keys(family, cfg, student).items())):
        rows = (torch.arange(shape[0]) + 37 * n) % 251
        sd[k] = rows.float() if len(shape) == 1 else rows.float()[:, None] + (torch.arange(shape[1]) % 2).float()[None]
    return sd


@pytest.mark.parametrize('family,cfg,student', [('flux', FLUX, True), ('flux', FLUX, False), ('flux', dict(FLUX, guidance_embeds=False), True),
                                                ('qwen', QWEN, True), ('qwen', QWEN, False)])
def test_row_slices_match_the_pack_functions(family, cfg, student):
    from arcflow_amd.weights import expected_transformer_keys, pack_flux, pack_qwen, packed_row_slices
    sd = _iota_state_dict(family, cfg, student)
    if family == 'flux':
        packed = pack_flux(sd, cfg['num_layers'], cfg['num_single_layers'], 'cpu', guidance=cfg['guidance_embeds'], teacher=not student)
    else:
        packed = pack_qwen(sd, cfg['num_layers'], 'cpu', teacher=not student)
    slices = packed_row_slices(family, cfg, student)
    linears = {k[:-len('.weight')] for k, s in expected_transformer_keys(family, cfg, student).items() if k.endswith('.weight') and len(s) == 2}
    assert set(slices) == linears                                                    # every linear the pack functions consume, nothing else
    covered = {}
    for m, (name, r0, rows, in_f) in slices.items():
        src = sd[m + '.weight']
        assert (rows, in_f) == tuple(src.shape), m
        assert torch.equal(packed[name][r0:r0 + rows], src.bfloat16()), m
        assert torch.equal(packed[name[:-len('weight')] + 'bias'][r0:r0 + rows], sd[m + '.bias'].bfloat16()), m      # the bias rows go with them
        covered.setdefault(name, []).append((r0, rows))
    for name, spans in covered.items():                                               # the slices tile each packed matrix, in order, without gaps
        end = 0
        for r0, rows in sorted(spans):
            assert r0 == end, name
            end = r0 + rows
        assert end == packed[name].shape[0] or (name == 'head.weight' and packed[name].shape[0] - end < 8), name
    assert set(covered) == {k for k, v in packed.items() if k.endswith('.weight') and v.dim() == 2 and v.dtype == torch.bfloat16}


def test_every_released_linear_meets_the_fold_contract():
    """afx_lora_fold takes O % 64 == 0 and I % 64 == 0: true of every linear of FLUX.1-dev and Qwen-Image (default configs) but the
    student's 60-row log-gamma head, which no LoRA adapts (it is a full weight of the ArcFlow adapter)."""
    from arcflow_amd.weights import packed_row_slices
    for family in ('flux', 'qwen'):
        for student in (True, False):
            odd = {m for m, (_, r0, rows, in_f) in packed_row_slices(family, {}, student).items() if rows % 64 or in_f % 64}
            assert odd == ({'proj_out_loggamma'} if student else set()), (family, student, odd)


def _lora(mod, r, o, i, seed, spelling='peft', prefix='transformer.', infix='', alpha=None):
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(r, i, generator=g) * 0.1, torch.randn(o, r, generator=g) * 0.1
    ka, kb = ('lora_A', 'lora_B') if spelling == 'peft' else ('lora_down', 'lora_up')
    sd = {f'{prefix}{mod}.{ka}{infix}.weight': a, f'{prefix}{mod}.{kb}{infix}.weight': b}
    if alpha is not None:
        sd[f'{prefix}{mod}.alpha'] = torch.tensor(float(alpha))
    return sd


def test_key_parsing():
    from arcflow_amd.pipelines.arcflow_loader import parse_lora_state_dict
    sd = {}
    sd.update(_lora('transformer_blocks.0.attn.to_q', 4, 256, 256, 1))
    sd.update(_lora('transformer_blocks.0.attn.to_k', 4, 256, 256, 2, infix='.default'))
    sd.update(_lora('transformer_blocks.0.attn.to_out.0', 4, 256, 256, 3, spelling='kohya-names', prefix='', alpha=2.0))
    sd.update(_lora('x_embedder', 16, 256, 64, 4, prefix=''))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        mods, skipped = parse_lora_state_dict(sd)
    assert skipped == 0 and not rec
    assert set(mods) == {'transformer_blocks.0.attn.to_q', 'transformer_blocks.0.attn.to_k', 'transformer_blocks.0.attn.to_out.0', 'x_embedder'}
    assert mods['transformer_blocks.0.attn.to_out.0']['alpha'] == 2.0 and mods['x_embedder']['alpha'] is None
    assert torch.equal(mods['transformer_blocks.0.attn.to_k']['A'], sd['transformer.transformer_blocks.0.attn.to_k.lora_A.default.weight'])
    assert torch.equal(mods['transformer_blocks.0.attn.to_out.0']['B'], sd['transformer_blocks.0.attn.to_out.0.lora_up.weight'])
    assert mods['x_embedder']['A'].shape == (16, 64) and mods['x_embedder']['B'].shape == (256, 16)
    # text-encoder keys: skipped, ONE warning that counts them
    te = dict(sd)
    te.update({'text_encoder.text_model.encoder.layers.0.self_attn.q_proj.lora_A.weight': torch.zeros(4, 8),
               'text_encoder.text_model.encoder.layers.0.self_attn.q_proj.lora_B.weight': torch.zeros(8, 4),
               'text_encoder_2.encoder.block.0.layer.0.SelfAttention.q.lora_A.weight': torch.zeros(4, 8)})
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        mods2, skipped = parse_lora_state_dict(te)
    assert skipped == 3 and set(mods2) == set(mods)
    assert len(rec) == 1 and '3 text-encoder' in str(rec[0].message)
    with pytest.raises(ValueError, match='Kohya / ComfyUI'):
        parse_lora_state_dict({'lora_unet_double_blocks_0_img_attn_qkv.lora_down.weight': torch.zeros(4, 8)})
    with pytest.raises(ValueError, match='incomplete'):
        parse_lora_state_dict({'transformer.x_embedder.lora_A.weight': torch.zeros(4, 64)})
    with pytest.raises(ValueError, match='not a LoRA key'):
        parse_lora_state_dict({'transformer.x_embedder.weight': torch.zeros(256, 64)})


class _StubEngine:
    """What the registry touches of an MMDiTEngine before a fold."""
    teacher_head, num_gaussians, logweights_channels, fp8_linear = False, 16, 4, False
    device = torch.device('cpu')

    def __init__(self):
        self.loaded = []

    def load_state_dict(self, sd):
        self.loaded.append(sd)


def _pipe(with_arcflow=True):
    from arcflow_amd.pipelines import ArcFluxPipeline
    from oracle import dit_ref as D
    w = D.make_flux_weights(D.FluxCfg(num_layers=1, num_single_layers=1, heads=2, joint_dim=128, pooled_dim=64), seed=9)
    pipe = ArcFluxPipeline()
    pipe._transformer_config, pipe._base_state_dict = dict(FLUX), w
    pipe.transformer = _StubEngine()
    folds = []
    pipe._fold_adapters = lambda scale: folds.append((scale, dict(pipe._style['active'])))      # the device fold, stubbed
    if with_arcflow:
        lora = _lora('single_transformer_blocks.0.proj_mlp', 8, 1024, 256, 5, prefix='')
        lora = {k: v.bfloat16() for k, v in lora.items()}
        pipe._adapters = ['transformer_arcflow']
        pipe._adapter_state = dict(target='transformer', base=dict(w), lora=lora, merged_scale=1.0, weight=1.0)
    return pipe, w, folds


def test_registry_semantics():
    pipe, w, folds = _pipe()
    arc = 'transformer_arcflow'
    assert pipe.get_list_adapters() == {'transformer': [arc]} and pipe.get_active_adapters() == [arc]
    a = _lora('transformer_blocks.0.attn.to_q', 4, 256, 256, 1, spelling='kohya-names', alpha=8.0)
    b = _lora('transformer_blocks.0.norm1.linear', 16, 1536, 256, 2)
    b.update(_lora('x_embedder', 16, 256, 64, 3))
    assert pipe.load_lora_weights(a, adapter_name='a') == 'a'
    assert pipe.load_lora_weights(b) == 'default_0'
    assert not folds and not pipe.transformer.loaded                               # lazy: nothing folded, nothing re-packed
    assert pipe.get_list_adapters() == {'transformer': [arc, 'a', 'default_0']}
    assert pipe.get_active_adapters() == [arc, 'a', 'default_0']                   # a loaded adapter is active with weight 1
    sty = pipe._style
    assert sty['active'] == {arc: 1.0, 'a': 1.0, 'default_0': 1.0}
    A, B, factor = sty['loras']['a']['transformer_blocks.0.attn.to_q']
    assert A.dtype == B.dtype == torch.bfloat16 and factor == 8.0 / 4                 # bf16 once at upload; alpha / r
    assert sty['loras']['default_0']['x_embedder'][2] == 1.0                         # no alpha: factor 1
    # the base copies: every linear any loaded adapter touches (the ArcFlow one included), as bf16 of the un-adapted weight
    assert set(sty['base']) == {'single_transformer_blocks.0.proj_mlp', 'transformer_blocks.0.attn.to_q', 'transformer_blocks.0.norm1.linear', 'x_embedder'}
    assert torch.equal(sty['base']['x_embedder'], w['x_embedder.weight'].bfloat16())
    with pytest.raises(ValueError, match='already loaded'):
        pipe.load_lora_weights(a, adapter_name='a')
    with pytest.raises(ValueError, match='already loaded'):
        pipe.load_lora_weights(a, adapter_name=arc)
    with pytest.raises(ValueError, match="no linear 'transformer_blocks.7.attn.to_q'"):
        pipe.load_lora_weights(_lora('transformer_blocks.7.attn.to_q', 4, 256, 256, 1), adapter_name='c')
    with pytest.raises(ValueError, match='do not fit'):
        pipe.load_lora_weights(_lora('transformer_blocks.0.attn.to_q', 4, 256, 128, 1), adapter_name='c')
    with pytest.raises(ValueError, match='do not fit'):
        pipe.load_lora_weights(_lora('transformer_blocks.0.attn.to_q', 4, 512, 256, 1), adapter_name='c')
    assert pipe.get_list_adapters() == {'transformer': [arc, 'a', 'default_0']}      # a refused load leaves no trace
    # set_adapters: float / list / None weights; adapters not listed become inactive
    pipe.set_adapters([arc, 'a'], adapter_weights=[1.0, 0.8])
    assert pipe.get_active_adapters() == [arc, 'a'] and pipe._style['active'] == {arc: 1.0, 'a': 0.8}
    pipe.set_adapters(['a', 'default_0'], 0.5)
    assert pipe._style['active'] == {'a': 0.5, 'default_0': 0.5} and pipe._adapter_state['weight'] == 0.0      # the ArcFlow LoRA branch is off
    pipe.set_adapters('default_0')
    assert pipe._style['active'] == {'default_0': 1.0} and pipe.get_active_adapters() == ['default_0']
    with pytest.raises(ValueError, match='not loaded'):
        pipe.set_adapters(['a', 'nope'])
    with pytest.raises(ValueError, match='adapter_weights'):
        pipe.set_adapters(['a', 'default_0'], [1.0])
    assert not folds                                                                 # still lazy
    pipe._apply_lora_scale(0.75)                                                     # what __call__ does with joint_attention_kwargs['scale']
    assert folds == [(0.75, {'default_0': 1.0})]
    # removal
    with pytest.raises(ValueError, match='ArcFlow adapter'):
        pipe.delete_adapters(arc)
    with pytest.raises(ValueError, match='not loaded'):
        pipe.delete_adapters('nope')
    pipe.set_adapters([arc, 'a', 'default_0'], [0.25, 1.0, 1.0])
    pipe.delete_adapters('a')
    assert pipe.get_list_adapters() == {'transformer': [arc, 'default_0']} and pipe._style is not None and not pipe.transformer.loaded
    pipe.unload_lora_weights()
    assert pipe._style is None and pipe.get_list_adapters() == {'transformer': [arc]} and pipe.get_active_adapters() == [arc]
    # ... the ArcFlow-only path rebuilt the weights for the current ArcFlow weight (0.25): merge_lora + load_state_dict, as before this feature
    from arcflow_amd.weights import merge_lora
    assert len(pipe.transformer.loaded) == 1 and pipe._adapter_state['merged_scale'] == 0.25
    want = merge_lora(pipe._adapter_state['base'], pipe._adapter_state['lora'], scale=0.25)
    got = pipe.transformer.loaded[0]
    assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
    with pytest.raises(ValueError, match='not loaded'):
        pipe.set_adapters('default_0')
    pipe.unload_lora_weights()                                                       # nothing loaded: a no-op
    assert len(pipe.transformer.loaded) == 1


def test_registry_guards():
    pipe, w, folds = _pipe(with_arcflow=False)
    assert pipe.get_list_adapters() == {} and pipe.get_active_adapters() == []
    pipe.transformer.teacher_head = True
    with pytest.raises(RuntimeError, match='load_arcflow_adapter'):
        pipe.load_lora_weights(_lora('x_embedder', 4, 256, 64, 1))
    pipe.transformer.teacher_head = False
    pipe.transformer.fp8_linear = True
    with pytest.raises(NotImplementedError, match='fp8'):
        pipe.load_lora_weights(_lora('x_embedder', 4, 256, 64, 1))
    pipe.transformer.fp8_linear = False
    with pytest.raises(EnvironmentError, match='no network'):
        pipe.load_lora_weights('someone/some-style-lora')
    with pytest.raises(ValueError, match='multiples of 64'):
        pipe.load_lora_weights(_lora('proj_out_loggamma', 4, 60, 256, 1))
    assert pipe.load_lora_weights(_lora('x_embedder', 4, 256, 64, 1), adapter_name='style') == 'style'      # a student without an ArcFlow LoRA
    assert pipe.get_active_adapters() == ['style']
    with pytest.raises(RuntimeError, match='unload_lora_weights'):
        pipe.load_arcflow_adapter('/nonexistent')


def test_load_from_file(tmp_path):
    from safetensors.torch import save_file
    pipe, w, folds = _pipe()
    sd = _lora('transformer_blocks.0.attn.to_q', 4, 256, 256, 1)
    save_file(sd, str(tmp_path / 'style.safetensors'))
    (tmp_path / 'sub').mkdir()
    save_file(sd, str(tmp_path / 'sub' / 'pytorch_lora_weights.safetensors'))
    assert pipe.load_lora_weights(str(tmp_path / 'style.safetensors'), adapter_name='file') == 'file'
    assert pipe.load_lora_weights(str(tmp_path), weight_name='style.safetensors', adapter_name='dir') == 'dir'
    assert pipe.load_lora_weights(str(tmp_path), subfolder='sub', adapter_name='sub') == 'sub'
    ref = pipe._style['loras']['file']['transformer_blocks.0.attn.to_q']
    for n in ('dir', 'sub'):
        got = pipe._style['loras'][n]['transformer_blocks.0.attn.to_q']
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    assert torch.equal(ref[0], sd['transformer.transformer_blocks.0.attn.to_q.lora_A.weight'].bfloat16())      # fp32 file: rounded once


# ---------------------------------------------------------------------------------------------------- the fp64 reference on its own
def _operands(O, I, ranks, seed=0):
    g = torch.Generator().manual_seed(seed)
    base = (torch.randn(O, I, generator=g) * 0.02).bfloat16()
    A = [(torch.randn(r, I, generator=g) * 0.1).bfloat16() for r in ranks]
    B = [(torch.randn(O, r, generator=g) * 0.1).bfloat16() for r in ranks]
    return base, A, B


def test_reference_properties():
    base, A, B = _operands(64, 128, (4, 16))
    t0, E0 = LR.fold_reference(base)
    assert torch.equal(t0, base.double()) and torch.equal(LR.rne_bf16(t0).bfloat16(), base)            # J == 0: the identity
    assert not LR.failing(base, t0, E0).any()
    t1, _ = LR.fold_reference(base, A, B, (1.0, 0.5))
    t2, _ = LR.fold_reference(base, A, B, (2.0, 1.0))
    t3, _ = LR.fold_reference(base, A, B, (3.0, 1.5))
    assert torch.allclose((t2 - t0), 2 * (t1 - t0), rtol=1e-12, atol=0) and torch.allclose(t3 - t2, t1 - t0, rtol=1e-10, atol=1e-18)      # linear in s
    tz, _ = LR.fold_reference(base, A, B, (0.0, 0.0))
    assert torch.equal(tz, t0)
    # E grows with R: the same products with more (zero-padded) ranks have the same t and mag, and a larger bound
    pad = lambda a, b, r: (torch.cat([a, a.new_zeros(r, a.shape[1])]), torch.cat([b, b.new_zeros(b.shape[0], r)], dim=1))      # noqa: E731
    a2, b2 = pad(A[0], B[0], 60)
    ts, Es = LR.fold_reference(base, [A[0]], [B[0]], (1.0,))
    tl, El = LR.fold_reference(base, [a2], [b2], (1.0,))
    assert torch.equal(ts, tl) and bool((El > Es).all())
    assert torch.allclose(El / Es, torch.full_like(El, (64 + 4) / (4 + 4)), rtol=1e-12)
    # the scale is taken as the fp32 value the kernel receives
    assert LR.f32(0.7) != 0.7 and LR.f32(0.5) == 0.5
    # rne_bf16 rounds fp64 directly and ties to even: 1 + 2^-8 is a tie between 1 and 1 + 2^-7
    x = torch.tensor([1 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -40, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 0.0, 2.0 ** -130], dtype=torch.float64)
    assert LR.rne_bf16(x).tolist() == [1.0, 1 + 2.0 ** -7, 1 + 2.0 ** -6, -1.0, 0.0, 2.0 ** -130]
    # the criterion: rne(t) passes, a tie inside the interval may go either way, the next value does not pass
    t = torch.tensor([[1 + 2.0 ** -8]], dtype=torch.float64)
    E = torch.tensor([[2.0 ** -20]], dtype=torch.float64)
    for v, ok in ((1.0, True), (1 + 2.0 ** -7, True), (1 + 2.0 ** -6, False), (1 - 2.0 ** -8, False)):
        assert bool(LR.failing(torch.tensor([[v]]).bfloat16(), t, E).any()) != ok, v
    with pytest.raises(AssertionError, match='1 of 1 elements'):
        LR.check_fold(torch.tensor([[1 + 2.0 ** -6]]).bfloat16(), t, E)


# ---------------------------------------------------------------------------------------------------- the ABI's argument checks (host side)
@pytest.fixture(scope='module')
def lib():
    from arcflow_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_lora_fold_refuses_bad_arguments_before_launch(lib):
    """Fake but aligned pointers (a launch would fault): every refusal is AFX_E_INVALID from the host-side checks."""
    p = lambda off=0: (1 << 24) + off         # noqa: E731
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float

    def call(base=p(), ldb=256, dst=p(1 << 22), ldd=256, O=128, I=256, J=2, A=(p(1 << 20), p(1 << 21)), B=(p(3 << 20), p(5 << 20)), ranks=(4, 16),
             scales=(1.0, 0.5), null_arrays=False):
        n = max(len(A), 1)
        arr = lambda ty, v: None if null_arrays else (ty * n)(*v)      # noqa: E731
        return lib.afx_lora_fold(vp(base) if base else None, ldb, vp(dst) if dst else None, ldd, O, I, J, arr(vp, A), arr(vp, B), arr(i32, ranks),
                                 arr(f32, scales), None)
    for kw, msg in ((dict(base=0), b'null'), (dict(dst=0), b'null'), (dict(null_arrays=True), b'null'), (dict(A=(p(1 << 20), 0)), b'null'),
                    (dict(B=(0, p(5 << 20))), b'null'),
                    (dict(J=9, A=(p(),) * 9, B=(p(),) * 9, ranks=(4,) * 9, scales=(1.0,) * 9), b'adapters'), (dict(J=-1), b'adapters'),
                    (dict(ranks=(4, 0)), b'rank'), (dict(ranks=(-3, 16)), b'rank'),
                    (dict(O=96), b'multiples of 64'), (dict(I=96, ldb=96, ldd=96), b'multiples of 64'), (dict(O=0), b'multiples of 64'),
                    (dict(ldb=192), b'leading dimension'), (dict(ldd=248), b'leading dimension'),
                    (dict(dst=p(64 * 256 * 2)), b'overlaps'), (dict(dst=p()), b'overlaps'), (dict(base=p(8)), b'aligned'),
                    (dict(dst=p((1 << 22) + 8)), b'aligned'), (dict(ldd=260), b'aligned'), (dict(A=(p((1 << 20) + 8), p(1 << 21))), b'aligned')):
        assert call(**kw) == -1, kw
        assert msg in lib.afx_last_error(), (kw, lib.afx_last_error())
    # a base that starts inside dst's last row is an overlap
    assert call(base=p(1 << 22) + (127 * 256 + 128) * 2) == -1 and b'overlaps' in lib.afx_last_error()
