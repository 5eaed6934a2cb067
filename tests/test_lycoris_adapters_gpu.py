"""LyCORIS LoHa / LoKr adapters through ``load_lora_weights`` / ``set_adapters`` on the GPU, on the tiny pipelines of tests/test_lora_adapters_gpu.py
(its ``Setup``: D = 256, 2 heads, FLUX 1 double + 1 single block, Qwen-Image 1 layer, an ArcFlow adapter with a rank-8 LoRA).

Three style adapters beside the ArcFlow adapter: 'loha' (FLUX: Kohya BFL spelling with a fused qkv, which shares ``to_q`` with the ArcFlow LoRA, plus the
image embedder; Qwen-Image: underscored diffusers names), 'lokr' (dense factors under diffusers names; c = 32 and 96, d = 16 and 64) and the plain LoRA
'a' of the Setup.  After the next call every adapted row slice of the live packed weights lies inside the interval of tests/lycoris_fold_ref.py built
from the HOST tensors, everything else equals the packed base bit for bit.  A changed weight refolds only the linears it touches; ``delete_adapters``
/ ``unload_lora_weights`` give back the ArcFlow-only weights bit for bit; a ninth term on one linear raises; with ``enable_fp8()`` on, loading raises.
On the parent commit every test here fails: the loader refuses ``hada_*`` / ``lokr_*`` keys."""
import pytest
import torch

import lycoris_fold_ref as YR
from test_evaluate_gpu import FLOOR, rel_l2
from test_lora_adapters_gpu import Setup, _weights_equal

pytestmark = pytest.mark.gpu

ARC = 'transformer_arcflow'
D = 256
ALPHA = 4.0


@pytest.fixture(scope='module', params=['flux', 'qwen'])
def S(request, tmp_path_factory):
    return Setup(request.param, str(tmp_path_factory.mktemp('lycoris_' + request.param)))


def _adapters(S):
    """-> (LoHa state dict, LoKr state dict, {module: term without scale} per adapter, factors): host tensors rounded as the loader rounds them."""
    g = torch.Generator().manual_seed(51)
    q = 'transformer_blocks.0.attn.to_q'
    loha_sd, lokr_sd, loha, lokr = {}, {}, {}, {}

    def put_loha(key, parts, o, i, r1=4, r2=6):
        t = YR.loha_operands(o, i, r1, r2, g)
        loha_sd.update({f'{key}.hada_{n}': t[n] for n in ('w1_a', 'w1_b', 'w2_a', 'w2_b')})
        loha_sd[key + '.alpha'] = torch.tensor(ALPHA)
        r0 = 0
        for p in parts:
            rows = S.w[p + '.weight'].shape[0]
            loha[p] = dict(t, w1_a=t['w1_a'][r0:r0 + rows], w2_a=t['w2_a'][r0:r0 + rows])
            r0 += rows
        return ALPHA / r1

    def put_lokr(p, c, d):
        o, i = S.w[p + '.weight'].shape
        t = YR.lokr_operands(o // c, i // d, c, d, g)
        lokr_sd.update({f'transformer.{p}.lokr_w1': t['w1'], f'transformer.{p}.lokr_w2': t['w2'], f'transformer.{p}.alpha': torch.tensor(ALPHA)})
        lokr[p] = dict(t, row0=0)
    if S.family == 'flux':
        t0 = 'transformer_blocks.0.attn.'
        f_loha = put_loha('lora_unet_double_blocks_0_img_attn_qkv', [t0 + 'to_q', t0 + 'to_k', t0 + 'to_v'], 3 * D, D)
        put_loha('lora_unet_img_in', ['x_embedder'], D, 64)
        put_lokr(q, 32, 16)
        put_lokr('transformer_blocks.0.ff.net.0.proj', 64, 64)
        put_lokr('single_transformer_blocks.0.proj_out', 32, 64)
    else:
        f_loha = put_loha('lora_unet_' + q.replace('.', '_'), [q], D, D)
        put_loha('lora_transformer_img_in', ['img_in'], *S.w['img_in.weight'].shape)
        put_lokr(q, 32, 16)
        put_lokr('transformer_blocks.0.img_mlp.net.2', 64, 64)
        put_lokr('transformer_blocks.0.txt_mod.1', 96, 64)
    return loha_sd, lokr_sd, dict(loha=loha, lokr=lokr), dict(loha=f_loha, lokr=1.0)           # both LoKr factors dense: factor 1 whatever alpha says


def _reference(S, terms, factors, active, call_scale):
    """active {'arc' | 'a' | 'loha' | 'lokr': weight} -> {module: (t, E)} over every linear any adapter touches."""
    out = {}
    for m in sorted(set(S.arc) | set(S.a) | set(terms['loha']) | set(terms['lokr'])):
        ts = []
        for name in ('arc', 'a'):
            if name in active and m in getattr(S, name) and call_scale * active[name] != 0.0:
                ts.append(dict(kind='lora', A=getattr(S, name)[m][0], B=getattr(S, name)[m][1], scale=call_scale * active[name] * S.factor[name]))
        for name in ('loha', 'lokr'):
            if name in active and m in terms[name] and call_scale * active[name] != 0.0:
                ts.append(dict(terms[name][m], scale=call_scale * active[name] * factors[name]))
        out[m] = YR.terms_reference(S.base_sd[m + '.weight'].bfloat16(), ts)
    return out


def _load(S, pipe, loha_sd, lokr_sd):
    assert pipe.load_lora_weights(dict(loha_sd), adapter_name='loha') == 'loha'
    assert pipe.load_lora_weights(dict(lokr_sd), adapter_name='lokr') == 'lokr'
    assert pipe.load_lora_weights(dict(S.sd_a), adapter_name='a') == 'a'


def test_loha_lokr_and_lora_beside_the_arcflow_adapter(S):
    loha_sd, lokr_sd, terms, factors = _adapters(S)
    pipe, only = S.with_arcflow(), S.with_arcflow()
    plain = S.run(pipe)
    _load(S, pipe, loha_sd, lokr_sd)
    sty = pipe._style
    assert set(sty['loras']['loha']) == set(terms['loha']) and set(sty['loras']['lokr']) == set(terms['lokr'])
    assert all(e['kind'] == 'loha' and e['w1_a'].dtype == torch.bfloat16 and e['factor'] == factors['loha'] for e in sty['loras']['loha'].values())
    assert all(e['kind'] == 'lokr' and e['w1'].dtype == e['w2'].dtype == torch.float32 and e['factor'] == 1.0 for e in sty['loras']['lokr'].values())
    assert not sty['folded']                                                        # lazy: nothing is folded before the next call
    pipe.set_adapters([ARC, 'loha', 'lokr', 'a'], [1.0, 0.7, -0.5, 0.6])
    out = S.run(pipe, 0.9)
    S.check_packed(pipe, _reference(S, terms, factors, dict(arc=1.0, loha=0.7, lokr=-0.5, a=0.6), 0.9))
    assert torch.isfinite(out).all() and rel_l2(out, plain) > FLOOR
    q = 'transformer_blocks.0.attn.to_q'
    assert [n for n, _ in sty['folded'][q]] == [ARC, 'loha', 'lokr', 'a']             # four kinds of adapter on one linear, in load order
    # a changed weight refolds only the linears it touches; the same state again folds nothing
    before = dict(sty['folded'])
    pipe.set_adapters([ARC, 'loha', 'lokr', 'a'], [1.0, 0.7, 0.25, 0.6])
    S.run(pipe, 0.9)
    changed = {m for m in sty['folded'] if sty['folded'][m] != before.get(m)}
    assert changed == set(terms['lokr'])
    S.check_packed(pipe, _reference(S, terms, factors, dict(arc=1.0, loha=0.7, lokr=0.25, a=0.6), 0.9))
    before = dict(sty['folded'])
    S.run(pipe, 0.9)
    assert sty['folded'] == before
    # left out of set_adapters an adapter contributes nothing
    pipe.set_adapters([ARC, 'lokr'], [0.5, 1.0])
    S.run(pipe)
    S.check_packed(pipe, _reference(S, terms, factors, dict(arc=0.5, lokr=1.0), 1.0))
    # removal restores the ArcFlow-only bits, by either door
    pipe.set_adapters([ARC, 'loha', 'lokr', 'a'])
    S.run(pipe)
    pipe.delete_adapters('loha')
    S.run(pipe)
    S.check_packed(pipe, _reference(S, terms, factors, dict(arc=1.0, lokr=1.0, a=1.0), 1.0))
    pipe.delete_adapters(['lokr', 'a'])
    assert pipe._style is None and pipe.get_list_adapters() == {'transformer': [ARC]}
    _weights_equal(pipe, only)
    _load(S, pipe, loha_sd, lokr_sd)
    S.run(pipe, 0.8)
    S.check_packed(pipe, _reference(S, terms, factors, dict(arc=1.0, loha=1.0, lokr=1.0, a=1.0), 0.8))
    pipe.unload_lora_weights()
    _weights_equal(pipe, only)
    assert torch.equal(S.run(pipe), plain)


def test_a_ninth_term_on_one_linear_raises(S):
    _, lokr_sd, _, _ = _adapters(S)
    pipe = S.with_arcflow()
    for n in range(8):                                                              # the ArcFlow adapter + 8 LoKr adapters on to_q
        pipe.load_lora_weights(dict(lokr_sd), adapter_name=f'k{n}')
    with pytest.raises(ValueError, match='9 active adapters'):
        S.run(pipe)
    pipe.set_adapters([ARC] + [f'k{n}' for n in range(7)])                          # eight terms fold
    assert torch.isfinite(S.run(pipe)).all()


def test_fp8_linear_mode_refuses(S):
    loha_sd, _, _, _ = _adapters(S)
    pipe = S.with_arcflow()
    pipe.transformer.enable_fp8()
    with pytest.raises(NotImplementedError, match='fp8'):
        pipe.load_lora_weights(dict(loha_sd), adapter_name='loha')
    pipe.transformer.enable_fp8(False)
    pipe.load_lora_weights(dict(loha_sd), adapter_name='loha')
    pipe.transformer.enable_fp8()
    with pytest.raises(NotImplementedError, match='fp8'):
        S.run(pipe)                                                                 # a fold is due: refused
