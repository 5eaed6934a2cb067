"""Data-based distillation (``ArcFlowImitation``), the parts that need no GPU: segment sampling and the CPU restatement of
the step against the reference's recorded results (fixtures G10 / G11, tests/golden/make_golden_imitation.py), the
config-type mapping, the mode / argument checks of ``train_step`` and the latent feed through the dataset and collate."""
import json
import os
import pickle

import pytest
import torch

from arcflow_amd.train import config as CFG
from arcflow_amd.train import data as DATA
from arcflow_amd.train.distill import ArcFlowDistiller, DistillConfig, sample_t
from oracle import arcflow_ref as R
from tests import imitation_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(2, 1.0), (3, 0.5), (4, 0.25)]


def close(a, b, rtol=2e-6, atol=2e-6):          # the fp32 bound of tests/test_oracle_golden.py
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs().max().item()
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f'max abs err {err}'


@pytest.mark.parametrize('nfe,ratio', CASES)
def test_sample_t_matches_reference(golden, nfe, ratio):
    g = golden('g10_imitation_sample_t')
    tag = f'n{nfe}_r{str(ratio).replace(".", "p")}'
    u = torch.from_numpy(g['u'])
    ref_raw, ref_sigma, ref_seg = (torch.from_numpy(g[f'{tag}_{k}']) for k in ('raw_t_src', 'sigma_t_src', 'segment_size'))
    base = 1 / (nfe - 1 + ratio)
    ref_idx = torch.round(ref_raw.double() / base + (1 - ratio)).long()         # raw_t_src = (idx - (1 - ratio)) base
    # the fixture walks every source index and both clamps: raw_t below eps (u > 1 - eps) and raw_t = 1 (u = 0)
    assert set(ref_idx.tolist()) == set(range(1, nfe + 1))
    assert (1 - u < float(g['eps'])).any() and (u == 0).any() and (ref_raw == 1).any()
    raw, sigma, seg = sample_t(u, nfe, ratio, float(g['shift']), float(g['eps']))
    assert raw.shape == sigma.shape == seg.shape == u.shape and seg.dtype == torch.float32
    assert torch.equal(seg, ref_seg)
    assert torch.equal(torch.round(raw.double() / base + (1 - ratio)).long(), ref_idx)
    close(raw, ref_raw)
    close(sigma, ref_sigma)
    # the test helper's restatement (it also returns the index)
    raw2, sigma2, seg2, idx2 = IR.sample_t(u, nfe, ratio, float(g['shift']), float(g['eps']))
    assert torch.equal(idx2, ref_idx) and torch.equal(seg2, ref_seg)
    close(raw2, ref_raw)
    close(sigma2, ref_sigma)


def test_imitation_ref_matches_reference_step(golden):
    g = {k: torch.from_numpy(v) for k, v in golden('g11_imitation_step').items()}
    B, n = g['x0'].shape[0], g['u_student'].shape[1]

    def teacher(x_t, t, b):               # the closed-form stub of the fixture (per-sample terms only)
        return 0.3 * x_t - 0.7 * t.reshape(-1, 1, 1, 1) + 0.05 * torch.roll(x_t, 1, dims=-1)

    trace = {}
    loss = IR.imitation_step(teacher, lambda x_t, sigma: (g['means'], g['logw'], g['logg']), g['x0'], g['noise'], g['u'],
                             float(g['teacher_ratio']), g['u_drop'], g['u_student'], g['u_teacher'], int(g['nfe']),
                             float(g['timestep_ratio']), trace=trace)
    assert len(set(g['raw_t_src'].tolist())) == 3 and len(set(g['segment_size'].tolist())) == 2     # three source indices, two sizes
    assert torch.equal(trace['segment_size'], g['segment_size'])
    close(trace['raw_t_src'], g['raw_t_src'])
    close(trace['sigma_t_src'], g['sigma_t_src'])
    close(trace['x_t_src'], g['x_t_src'])
    # the reference stacks the states as [state][sample]; the helper walks [sample][state]
    shape = (n, B, *g['x0'].shape[1:])
    x_a, tgt, pred = (torch.stack(trace[k], dim=1) for k in ('x_t_a', 'tgt_u', 'pred_u'))
    close(x_a, g['x_t_a'])
    close(tgt, g['tgt_u'].reshape(shape))
    # pred_u = (x_a - x_e) / (sigma_a - sigma_e) is a quotient over a window of ~3/128 of raw time: x_e = x_a - displacement is rounded
    # to half an ulp of its own size in either implementation before the division, which the small denominator magnifies.  So on top
    # of the fp32 bound on the value itself: 2 x 2^-24 x (|x_a| + |x_a - x_e|) / (sigma_a - sigma_e), with the window ends as the
    # reference passed them (fixture raw_t_a / raw_t_e).  Roll-outs under two sub-steps use the local velocity: no quotient.
    ref = g['pred_u'].reshape(shape).double()
    den = (R.shift_sigma(g['raw_t_a']) - R.shift_sigma(g['raw_t_e'])).clamp(min=1e-4).double().reshape(n, B, 1, 1, 1)
    long = (torch.round((g['raw_t_a'] - g['raw_t_e']) * 128) >= 2).double().reshape(n, B, 1, 1, 1)
    assert long.sum() > 0
    tol = 2e-6 + 2e-6 * ref.abs() + long * 2.0 ** -23 * (g['x_t_a'].double().abs() + ref.abs() * den) / den
    err = (pred.double() - ref).abs()
    print('pred_u: max err', err.max().item(), 'max err / tol', (err / tol).max().item())
    assert (err <= tol).all(), (err / tol).max().item()
    close(loss, g['loss'])


def _golden_config(name):
    def dec(v):
        if isinstance(v, dict):
            return tuple(dec(x) for x in v['__tuple__']) if set(v) == {'__tuple__'} else {k: dec(x) for k, x in v.items()}
        if isinstance(v, list):
            return [dec(x) for x in v]
        return v
    with open(os.path.join(ROOT, 'tests', 'golden', 'g10_configs.json')) as f:
        return dec(json.load(f)[name])


def test_config_type_selects_the_mode():
    for name in ('flux/arcflux_2nfe_k16.py', 'qwen/arcqwen_2nfe_k16.py'):
        assert CFG.distill_setup(_golden_config(name))[2].mode == 'data_free'
    cfg = CFG.load_config(os.path.join(ROOT, 'examples', 'flux_distill_data_2nfe.py'))
    fam, eng, dc, run = CFG.distill_setup(cfg)
    assert (fam, dc.mode, dc.nfe, dc.lora_rank) == ('flux', 'data', 2, 256)
    assert CFG.distill_setup(CFG.load_config(os.path.join(ROOT, 'examples', 'flux_distill_2nfe.py')))[2].mode == 'data_free'
    cfg['model']['diffusion']['type'] = 'GaussianFlow'
    with pytest.raises(ValueError, match='GaussianFlow'):
        CFG.distill_setup(cfg)
    assert DistillConfig().mode == 'data_free'
    with pytest.raises(ValueError):
        DistillConfig(mode='latents')


def test_train_step_refuses_arguments_of_the_other_mode():
    """The checks run before anything touches the device: a bare object with the config is enough."""
    cond = dict(hp=4, wp=4)
    d = ArcFlowDistiller.__new__(ArcFlowDistiller)
    d.cfg = DistillConfig(mode='data_free')
    with pytest.raises(ValueError, match="mode 'data'"):
        d.train_step(cond, 2, x0=torch.zeros(2, 16, 8, 8))
    with pytest.raises(ValueError, match="mode 'data'"):
        d.train_step(cond, 2, t_draws=torch.zeros(2))
    d.cfg = DistillConfig(mode='data')
    with pytest.raises(ValueError, match='x0'):
        d.train_step(cond, 2)
    with pytest.raises(ValueError, match='x_init'):
        d.train_step(cond, 2, x0=torch.zeros(2, 16, 8, 8), x_init=torch.zeros(2, 16, 64))
    with pytest.raises(ValueError, match='x0 must be'):
        d.train_step(cond, 2, x0=torch.zeros(2, 16, 8, 12))        # does not match cond's hp / wp
    with pytest.raises(ValueError, match='x0 must be'):
        d.train_step(cond, 2, x0=torch.zeros(3, 16, 8, 8))         # does not match the batch


def test_cached_latents_reach_the_shape_train_step_takes(tmp_path):
    g = torch.Generator().manual_seed(0)
    lats = []
    for i in range(3):
        lat = torch.randn(16, 6, 10, generator=g).half()
        lats.append(lat)
        item = dict(prompt=f'p{i}', prompt_embed_kwargs=dict(encoder_hidden_states=torch.randn(5, 32, generator=g).half(),
                                                              pooled_projections=torch.randn(16, generator=g).half()),
                    latent_size=(16, 6, 10), latents=lat)
        if i == 1:
            item['latents'], item['latents_scale'] = (lat.float() / 0.5).half(), 0.5
        with open(tmp_path / f'{i:04d}.pkl', 'wb') as f:
            pickle.dump(item, f)
    ds = DATA.PromptEmbedCache(str(tmp_path), pad_seq_len=6, bucketize=True, load_latents=True)
    cond = DATA.collate([ds[i] for i in range(3)], device='cpu')
    x0 = cond.pop('latents')
    assert x0.dtype == torch.float32 and tuple(x0.shape) == (3, 16, 2 * cond['hp'], 2 * cond['wp']) == (3, 16, 6, 10)
    assert torch.equal(x0[0], lats[0].float()) and torch.equal(x0[2], lats[2].float())
    assert torch.allclose(x0[1], lats[1].float(), atol=2e-3)
    # train_step's own shape check ties x0 to cond's hp / wp: the transposed grid is refused
    d = ArcFlowDistiller.__new__(ArcFlowDistiller)
    d.cfg = DistillConfig(mode='data')
    with pytest.raises(ValueError, match='x0 must be'):
        d.train_step(dict(cond, hp=cond['wp'], wp=cond['hp']), 3, x0=x0)
    # without load_latents the batch is what it was; a record without latents fails with the dataset's message
    assert 'latents' not in DATA.collate([DATA.PromptEmbedCache(str(tmp_path), pad_seq_len=6)[0]], device='cpu')
    item = dict(prompt='q', prompt_embed_kwargs=dict(encoder_hidden_states=torch.randn(5, 32, generator=g).half()), latent_size=(16, 6, 10))
    with open(tmp_path / '0009.pkl', 'wb') as f:
        pickle.dump(item, f)
    with pytest.raises(KeyError, match='no latents'):
        DATA.PromptEmbedCache(str(tmp_path), load_latents=True)[3]

