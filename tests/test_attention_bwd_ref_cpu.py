"""The fp64 reference of the attention backward (attention_bwd_ref.py) held without a GPU: its formulas and log2-domain convention against torch.autograd,
its bound against an fp32 emulation of the kernels' rounding points, and the criterion that gives the GPU test (test_hip_attention_bwd_fp64.py) its teeth, on
the inputs that test uses."""
import pytest
import torch
from attention_bwd_ref import C32, LN2, SCALE32, attention_bwd_reference, exact_forward, teeth
from attention_inputs import TEETH_ALL, TEETH_DK, TEETH_DQ, TEETH_DV, TEETH_SHARE, case_inputs
from bf16_parity import check_bf16_bound


@pytest.mark.parametrize('S', [37, 70])
def test_reference_equals_autograd_of_fp64_attention(S):
    """With O and lse computed exactly in fp64, the reference's dQ / dK / dV are the gradients of sum(O dO) under torch.autograd, to 1e-12 relative.  The
    attention differentiated is the base-2 softmax of s c the kernels define (c = C32, an fp32 number); its chain rule carries c ln 2 where the kernels'
    epilogue carries SCALE, two separately rounded constants (ratio 1 + O(2^-24)), so autograd's dQ and dK are rescaled by SCALE / (c ln 2) -- explicitly."""
    B, H = 1, 2
    g = torch.Generator().manual_seed(S)
    q, k, v, do = (torch.randn(B, S, H, 128, generator=g, dtype=torch.float64) for _ in range(4))
    q, k = q * 0.7, k * 0.7
    o, lse = exact_forward(q, k, v)
    ref = attention_bwd_reference(q, k, v, o, do, lse)
    assert float((ref['rowsum'] - 1).abs().max()) < 1e-12
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    t = torch.einsum('bqhd,bkhd->bhqk', qa, ka) * C32
    oa = torch.einsum('bhqk,bkhd->bqhd', torch.softmax(t * LN2, dim=-1), va)
    assert float((oa.detach() - o).abs().max()) < 1e-12
    (oa * do).sum().backward()
    fix = SCALE32 / (C32 * LN2)
    for name, got, want in (('dq', ref['dq'], qa.grad * fix), ('dk', ref['dk'], ka.grad * fix), ('dv', ref['dv'], va.grad)):
        want = want.reshape(B * S, H * 128)
        err = float((got - want).abs().max() / want.abs().max())
        assert err < 1e-12, (name, err)
        assert bool((ref['b' + name[1]] > 0).all())


_TEETH = TEETH_ALL


@pytest.mark.parametrize('B,S,H,design', _TEETH, ids=[f'{b}x{s}x{h}' for b, s, h, _ in _TEETH])
def test_a_dropped_key_or_query_separates_the_references(B, S, H, design):
    """The teeth criterion, which involves no kernel: with the last real key (dQ) or the last real query (dK, dV) left out of the reference, the mutated and the
    true reference differ by more than twice the tolerance in some element of at least 90 % of the random-design heads' rows -- for dQ, dK and dV each on its
    own -- so that no output satisfies both.  The inputs are the GPU test's own (attention_inputs.case_inputs); O is the exact fp64 O rounded to bf16 and lse the
    exact one rounded to fp32, as a correct forward returns them.  Shares found:
      (1, 37, 4)   dQ 0.973   dK 0.919   dV 1.000
      (1, 65, 4)   dQ 0.938   dK 0.908   dV 1.000
      (1, 191, 9)  dQ 0.730   dK 0.754   dV 0.990
    dQ and dK miss the share at S = 191 (a key or a query is 1 / 191 of such a row and the bound does not shrink with S): their teeth are held at S = 37 and 65,
    dV's at S = 65 and 191 (attention_inputs.TEETH_*).  The dropped query puts a weight of 1.000 on its planted key in every planted-key head."""
    q, k, v, do = case_inputs(B, S, H, design, 'cpu')
    o, lse = exact_forward(q, k, v)
    _, _, _, shares, planted = teeth(q, k, v, o.bfloat16(), do, lse.float())
    print(f'teeth B={B} S={S} H={H} dO design {design}: shares {shares}, planted-key weight {planted.flatten().tolist()}')
    for name, where in (('dq', TEETH_DQ), ('dk', TEETH_DK), ('dv', TEETH_DV)):
        if (B, S, H, design) in where:
            assert shares[name] >= TEETH_SHARE, (name, shares)
    if (B, S, H, design) in TEETH_DV:
        # the dropped query's planted key: more than half of that query's weight, so its dV row moves by more than half of dO[last query]
        assert float(planted.min()) > 0.5, planted


def _emulate_fp32(q, k, v, o, do, lse):
    """The kernels' arithmetic in plain torch: fp32 everywhere, P and dS rounded to bf16 (nearest even) in front of the accumulating products, bf16 outputs."""
    B, S, H, _ = q.shape
    qf, kf, vf, of, dof = (t.float().permute(0, 2, 1, 3) for t in (q, k, v, o, do))
    P = torch.exp2((qf @ kf.transpose(-1, -2)) * C32 - lse[:, :, :S, None])
    dS = (P * (dof @ vf.transpose(-1, -2) - (dof * of).sum(-1, keepdim=True))).bfloat16().float()
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(B * S, H * 128).bfloat16()         # noqa: E731
    return {'dq': flat((dS @ kf) * SCALE32), 'dk': flat((dS.transpose(-1, -2) @ qf) * SCALE32), 'dv': flat(P.bfloat16().float().transpose(-1, -2) @ dof)}


@pytest.mark.parametrize('B,S,H,design', _TEETH, ids=[f'{b}x{s}x{h}' for b, s, h, _ in _TEETH])
def test_an_fp32_emulation_of_the_rounding_points_meets_the_bound(B, S, H, design):
    """The bound must admit a faithful implementation.  (With the bf16 roundings taken as 2^-9 of the value -- half an ulp at the TOP of a binade -- instead of
    the exact half ulp, this emulation exceeds the bound at each of these shapes: see (3) of the derivation.)"""
    q, k, v, do = case_inputs(B, S, H, design, 'cpu')
    o, lse = exact_forward(q, k, v)
    o, lse = o.bfloat16(), lse.float()
    ref = attention_bwd_reference(q, k, v, o, do, lse)
    for name, out in _emulate_fp32(q, k, v, o, do, lse).items():
        worst = check_bf16_bound(out, ref[name], ref['b' + name[1]], f'B={B} S={S} H={H} emulation: {name}')
        print(f'emulation B={B} S={S} H={H}: {name} worst err / tol {worst:.3f}')
