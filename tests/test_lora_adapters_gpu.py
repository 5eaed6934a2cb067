"""Style LoRAs next to the ArcFlow adapter on the GPU: ``load_lora_weights`` / ``set_adapters`` / ``delete_adapters`` /
``unload_lora_weights`` of both pipelines on the tiny engines of tests/test_distill.py (D = 256, 2 heads, FLUX 1 double + 1 single block,
Qwen-Image 1 layer, an 8 x 8 token grid).

Setup: an ArcFlow adapter (heads, norm_out, rank-8 LoRA) plus two style LoRAs -- 'a' of rank 4 in the lora_down / lora_up spelling with
alpha = 8 (alpha / r = 2), 'b' of rank 16 with the `.default` infix on a modulation linear, the image embedder and an MLP linear; 'a' and the
ArcFlow adapter share a linear, so do 'b' and the ArcFlow adapter.

Bars.  The packed weights are held to the per-element criterion of tests/lora_fold_ref.py against the fp64 fold of the HOST tensors placed
at their packed rows (everything outside the adapted rows must equal the packed base bit for bit).  Latents: a fresh pipeline built from the
fp64-merged state dict rounded once to bf16 differs from the folded one by weight rounding only -- at most a few elements on a tie inside
[t - E, t + E] -- which is below what tests/test_evaluate_gpu.py lets two roundings of the same network differ by: its FLOOR (2e-3 rel-L2, the
part of its bar that stands for rounding noise; its FACTOR multiplies an oracle distance that is not formed here).  Everything else is a
bit-equality."""
import json
import os

import pytest
import torch

import lora_fold_ref as LR
from test_evaluate_gpu import FLOOR, rel_l2

pytestmark = pytest.mark.gpu

WEIGHTS, CALL_SCALE = [1.0, 0.7, -0.5], 0.8


def _family(family):
    from oracle import dit_ref as D
    if family == 'flux':
        cfg = D.FluxCfg(num_layers=1, num_single_layers=1, heads=2, joint_dim=128, pooled_dim=64)
        w = D.make_flux_weights(cfg, seed=9, teacher_head=True)
        tcfg = dict(num_layers=1, num_single_layers=1, num_attention_heads=2, attention_head_dim=128, in_channels=64, joint_attention_dim=128,
                    pooled_projection_dim=64, guidance_embeds=True)
        mods = dict(arc=['single_transformer_blocks.0.proj_mlp', 'transformer_blocks.0.attn.to_q'],
                    a=['transformer_blocks.0.attn.to_q', 'transformer_blocks.0.ff_context.net.2'],
                    b=['transformer_blocks.0.norm1.linear', 'x_embedder', 'single_transformer_blocks.0.proj_mlp'])
        return cfg, w, tcfg, mods, 'ArcFluxTransformer2DModel'
    cfg = D.QwenCfg(num_layers=1, heads=2, joint_dim=192)
    w = D.make_qwen_weights(cfg, seed=5)
    tcfg = dict(num_layers=1, num_attention_heads=2, attention_head_dim=128, in_channels=64, joint_attention_dim=192)
    mods = dict(arc=['transformer_blocks.0.img_mlp.net.0.proj', 'transformer_blocks.0.attn.to_q'],
                a=['transformer_blocks.0.attn.to_q', 'transformer_blocks.0.txt_mlp.net.2'],
                b=['transformer_blocks.0.img_mod.1', 'img_in', 'transformer_blocks.0.img_mlp.net.0.proj'])
    return cfg, w, tcfg, mods, 'ArcQwenImageTransformer2DModel'


class Setup:
    def __init__(self, family, tmp):
        from safetensors.torch import save_file
        self.family = family
        self.cfg, self.w, self.tcfg, mods, cls_name = _family(family)
        g = torch.Generator().manual_seed(21)

        def pair(m, r, std):
            o, i = self.w[m + '.weight'].shape
            return (torch.randn(r, i, generator=g) * std).bfloat16(), (torch.randn(o, r, generator=g) * std).bfloat16()
        self.arc = {m: pair(m, 8, 0.05) for m in mods['arc']}
        self.a = {m: pair(m, 4, 0.05) for m in mods['a']}
        self.b = {m: pair(m, 16, 0.05) for m in mods['b']}
        self.factor = dict(arc=1.0, a=8.0 / 4, b=1.0)
        adapter = {k: v.clone() for k, v in self.w.items() if k.startswith('proj_out_') or k.startswith('norm_out')}
        adapter['norm_out.linear.bias'] = adapter['norm_out.linear.bias'] + 0.125
        self.overlay = dict(adapter)
        for m, (A, B) in self.arc.items():
            adapter[m + '.lora_A.weight'], adapter[m + '.lora_B.weight'] = A, B
        d = os.path.join(tmp, 'arcflow')
        os.makedirs(d, exist_ok=True)
        json.dump({'_class_name': cls_name, 'num_gaussians': 16, 'logweights_channels': 4}, open(os.path.join(d, 'config.json'), 'w'))
        save_file({k: v.contiguous() for k, v in adapter.items()}, os.path.join(d, 'diffusion_pytorch_model.safetensors'),
                  metadata={'policy_config': json.dumps({'type': 'ArcFlow'})})
        self.root = tmp
        self.sd_a, self.sd_b = {}, {}
        for m, (A, B) in self.a.items():
            self.sd_a.update({f'{m}.lora_down.weight': A, f'{m}.lora_up.weight': B, f'{m}.alpha': torch.tensor(8.0)})
        for m, (A, B) in self.b.items():
            self.sd_b.update({f'transformer.{m}.lora_A.default.weight': A, f'transformer.{m}.lora_B.default.weight': B})
        self.base_sd = dict(self.w)                       # W_base: the plain snapshot + the ArcFlow adapter's non-LoRA keys
        self.base_sd.update(self.overlay)
        gi = torch.Generator().manual_seed(3)
        jd = self.tcfg['joint_attention_dim']
        self.pe = (torch.randn(1, 12, jd, generator=gi) * 0.5).bfloat16()
        self.pooled = (torch.randn(1, 64, generator=gi) * 0.5).bfloat16()
        self.lat = torch.randn(1, 64, 64, generator=gi)

    def plain(self, sd=None, student=False):
        from arcflow_amd import FlowMatchEulerDiscreteScheduler
        from arcflow_amd.pipelines import ArcFluxPipeline, ArcQwenImagePipeline
        sch = FlowMatchEulerDiscreteScheduler(shift=3.2)
        if self.family == 'flux':
            w = self.w if sd is None else sd
            if not student:
                w = {k: v for k, v in w.items() if not k.startswith('proj_out_')}
            return ArcFluxPipeline.from_state_dict(self.tcfg, w, scheduler=sch, student=student).to('cuda')
        return ArcQwenImagePipeline.from_state_dict(self.tcfg, self.w if sd is None else sd, scheduler=sch)

    def with_arcflow(self):
        pipe = self.plain()
        assert pipe.load_arcflow_adapter(self.root, subfolder='arcflow') == 'transformer_arcflow'
        return pipe

    def run(self, pipe, scale=None):
        kw = {}
        if scale is not None:
            kw['joint_attention_kwargs' if self.family == 'flux' else 'attention_kwargs'] = {'scale': scale}
        if self.family == 'flux':
            out = pipe(prompt_embeds=self.pe, pooled_prompt_embeds=self.pooled, latents=self.lat.clone(), width=128, height=128, num_inference_steps=2,
                       timestep_ratio=1.0, output_type='latent', **kw).images
        else:
            out = pipe(prompt_embeds=self.pe, prompt_embeds_mask=torch.ones(1, 12, dtype=torch.long), latents=self.lat.clone(), width=128, height=128,
                       num_inference_steps=2, timestep_ratio=1.0, output_type='latent', return_dict=False, **kw)[0]
        torch.cuda.synchronize()
        return out.cpu()

    def reference(self, active, call_scale):
        """active {'arc' | 'a' | 'b': weight} -> {module: (t fp64, E fp64)} of every linear any of the three adapters touches."""
        out = {}
        for m in sorted(set(self.arc) | set(self.a) | set(self.b)):
            A, B, S = [], [], []
            for name in ('arc', 'a', 'b'):
                if name in active and m in getattr(self, name):
                    A.append(getattr(self, name)[m][0]); B.append(getattr(self, name)[m][1]); S.append(call_scale * active[name] * self.factor[name])
            out[m] = LR.fold_reference(self.base_sd[m + '.weight'].bfloat16(), A, B, S)
        return out

    def packed_base(self):
        from arcflow_amd.weights import pack_flux, pack_qwen
        if self.family == 'flux':
            return pack_flux(self.base_sd, 1, 1, 'cpu')
        return pack_qwen(self.base_sd, 1, 'cpu')

    def check_packed(self, pipe, ref):
        from arcflow_amd.weights import packed_row_slices
        slices = packed_row_slices(self.family, self.tcfg, True)
        want = self.packed_base()
        live = {k: v.cpu() for k, v in pipe.transformer._weights.items() if not k.endswith(('.weight_q', '.wscale'))}      # (fp8 copies: not packed weights)
        assert set(live) == set(want)
        for name, base in want.items():
            if not (name.endswith('.weight') and base.dim() == 2 and base.dtype == torch.bfloat16):
                assert torch.equal(live[name], base), name
                continue
            t, E = base.double(), torch.zeros(base.shape, dtype=torch.float64)          # E = 0 outside the adapted rows: bit-equality there
            for m, (tm, Em) in ref.items():
                pname, r0, rows, _ = slices[m]
                if pname == name:
                    t[r0:r0 + rows], E[r0:r0 + rows] = tm, Em
            LR.check_fold(live[name], t, E, name)


@pytest.fixture(scope='module', params=['flux', 'qwen'])
def S(request, tmp_path_factory):
    return Setup(request.param, str(tmp_path_factory.mktemp('lora_' + request.param)))


def _weights_equal(p1, p2):
    w1, w2 = p1.transformer._weights, p2.transformer._weights
    assert set(w1) == set(w2)
    for k in w1:
        assert torch.equal(w1[k], w2[k]), k


def _load_styles(S, pipe):
    assert pipe.load_lora_weights(S.sd_a, adapter_name='a') == 'a'
    assert pipe.load_lora_weights(S.sd_b, adapter_name='b') == 'b'


def test_weighted_adapters_fold_and_sample(S, monkeypatch):
    from arcflow_amd import ops
    arc = 'transformer_arcflow'
    pipe = S.with_arcflow()
    ptrs = {k: v.data_ptr() for k, v in pipe.transformer._weights.items()}
    _load_styles(S, pipe)
    pipe.set_adapters([arc, 'a', 'b'], WEIGHTS)
    calls = []
    real = ops.lora_fold
    monkeypatch.setattr(ops, 'lora_fold', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    out = S.run(pipe, CALL_SCALE)
    assert len(calls) == len(set(S.arc) | set(S.a) | set(S.b))                           # one launch per adapted linear
    assert {k: v.data_ptr() for k, v in pipe.transformer._weights.items()} == ptrs      # the live packed tensors, no re-bind
    ref = S.reference(dict(arc=WEIGHTS[0], a=WEIGHTS[1], b=WEIGHTS[2]), CALL_SCALE)
    S.check_packed(pipe, ref)
    # a second call with the same state folds nothing and returns the same latents; a changed scale folds again
    del calls[:]
    assert torch.equal(S.run(pipe, CALL_SCALE), out) and not calls
    S.run(pipe)
    assert len(calls) == len(ref)
    S.check_packed(pipe, S.reference(dict(arc=WEIGHTS[0], a=WEIGHTS[1], b=WEIGHTS[2]), 1.0))
    # the fresh pipeline of the fp64-merged, once-rounded state dict
    merged = dict(S.base_sd)
    for m, (t, _) in ref.items():
        merged[m + '.weight'] = LR.rne_bf16(t).bfloat16()
    fresh = S.plain(merged, student=True)
    want = S.run(fresh)
    err = rel_l2(out, want)
    print(f'{S.family}: folded vs fresh fp64-merged pipeline, latents rel-L2 {err:.3e}')
    assert torch.isfinite(out).all() and err <= FLOOR, err
    plain = S.run(S.with_arcflow())
    assert rel_l2(out, plain) > FLOOR                                                    # ... and the style LoRAs did change the network


def test_subset_equals_fresh_load_and_unload_restores(S):
    arc = 'transformer_arcflow'
    pipe = S.with_arcflow()
    _load_styles(S, pipe)
    pipe.set_adapters([arc, 'a', 'b'], WEIGHTS)
    S.run(pipe, CALL_SCALE)
    pipe.set_adapters([arc, 'a'])
    assert pipe.get_active_adapters() == [arc, 'a'] and pipe.get_list_adapters() == {'transformer': [arc, 'a', 'b']}
    out = S.run(pipe)
    two = S.with_arcflow()
    two.load_lora_weights(S.sd_a, adapter_name='a')
    two.set_adapters([arc, 'a'])
    assert torch.equal(S.run(two), out)
    _weights_equal(pipe, two)
    S.check_packed(pipe, S.reference(dict(arc=1.0, a=1.0), 1.0))
    # without the ArcFlow adapter in the list its LoRA branch is off, its heads and norm_out stay
    pipe.set_adapters(['b'], 0.5)
    S.run(pipe)
    S.check_packed(pipe, S.reference(dict(b=0.5), 1.0))
    pipe.set_adapters([arc, 'a', 'b'])
    # removal: back to what load_arcflow_adapter alone produces, bit for bit
    only = S.with_arcflow()
    pipe.delete_adapters('a')
    assert pipe.get_list_adapters() == {'transformer': [arc, 'b']}
    with pytest.raises(ValueError, match='ArcFlow adapter'):
        pipe.delete_adapters(arc)
    pipe.unload_lora_weights()
    assert pipe.get_list_adapters() == {'transformer': [arc]}
    _weights_equal(pipe, only)
    assert torch.equal(S.run(pipe), S.run(only))
    with pytest.raises(ValueError, match='not loaded'):
        pipe.set_adapters([arc, 'a'])


def test_reference_snippet_and_fp8_refusal(S, tmp_path):
    """inference_flux.py:9: `pipe.set_adapters([adapter_name, 'style'], adapter_weights=[1.0, 0.8])` after `pipe.load_lora_weights(...)` of a file;
    and the documented refusal of the fp8 linear mode."""
    from safetensors.torch import save_file
    pipe = S.plain()
    adapter_name = pipe.load_arcflow_adapter(S.root, subfolder='arcflow')
    save_file({k: v.contiguous() for k, v in S.sd_b.items()}, str(tmp_path / 'style.safetensors'))
    pipe.load_lora_weights(str(tmp_path / 'style.safetensors'), adapter_name='style')
    pipe.set_adapters([adapter_name, 'style'], adapter_weights=[1.0, 0.8])
    assert torch.isfinite(S.run(pipe)).all()
    S.check_packed(pipe, S.reference(dict(arc=1.0, b=0.8), 1.0))
    pipe.transformer.enable_fp8()
    with pytest.raises(NotImplementedError, match='fp8'):
        S.run(pipe, 0.5)                                                                  # a fold is due: refused
    with pytest.raises(NotImplementedError, match='fp8'):
        pipe.load_lora_weights(S.sd_a, adapter_name='a')
    pipe.transformer.enable_fp8(False)
    S.run(pipe, 0.5)                                                                      # bf16 linears again: the fold runs
    S.check_packed(pipe, S.reference(dict(arc=1.0, b=0.8), 0.5))
