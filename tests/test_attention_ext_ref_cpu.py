"""The fp64 reference of the text-encoder (EXT) attention (attention_ext_ref.py) held without a GPU, on the inputs the GPU test (test_hip_attention_ext_fp64.py)
runs: (a) it equals a plain fp64 torch.softmax implementation, (b) each of the seven mutated references separates from it by more than twice the tolerance on
at least 0.9 of the rows the mutation is held on, (c) the reference rounded to bf16 and an fp32 emulation of the kernel's rounding points stay within the bound.

Shares of separated rows found here, per head design 0 (positive V) / 1 (planted key) / 2 (growing scores) / 3 (plain) over ALL rows of those heads -- the reason for
the rows attention_ext_ref.teeth_targets picks (on the picked rows every share printed by (b) is 1.000):
  causal_ge   1x65  h4 d64  'diag'  0.37 / 0.985 / 0.985 / 0.985     (row 0 is the missing 1 / 65);  plant 'rand' at 1x64: 0.42 / 0.36 / 0.98 / 0.98
  tile_short  1x128 h4 d64  'diag'  0.45 / 0.50 / 0.50 / 0.50        (rows 64 .. 127 are the affected half);  1x333: 0.31 / 0.42 / 0.42 / 0.42 (141 of 333 rows)
  bias_shift  1x65  h4 d64          1.00 / 0.09 / 1.00 / 1.00;       1x193: 1.00 / 0.14 / 1.00 / 1.00
  kv_mod      1x65  h8 kv2 d128     0.50 / 0.50                      (heads 0, 2, 5, 7 map alike under h % 2 and h // 4)
  drop_last   1x17  h4 d64 bias     0.53 / 0.06 / 1.00 / 1.00;       1x65: 0.08 / 0.015 / 1.00 / 1.00;   1x65 h4 d128: 0.12 / 0.015 / 1.00 / 1.00
              1x193 h4 d128         0.01 / 0.005 / 1.00 / 0.88       (design 3 falls under the share from S ~ 190 on: the tooth stays at 17 and 65)
  scale_128   1x65  h4 d64  causal  0.91 / 0.23 / 0.985 / 0.97;      1x193: 0.74 / 0.31 / 0.995 / 0.99
  vt_batch0   2x65                  0.50 on every design (all rows of b = 1);  3x65: 0.667"""
import pytest
import torch
from attention_ext_ref import (CASES, EDGE_S, MUTATIONS, TEETH, TEETH_SHARE, TOY, c32, ext_reference, find_case, mutations_of, separated_rows,
                               softmax_reference, teeth_targets)
from bf16_parity import check_bf16_bound

_TEETH_CASES = [c for c in CASES if mutations_of(c)]
_PAIRS = [(m, find_case(B, S, cfg)) for m in MUTATIONS for B, S, cfg in TEETH[m]]
_refs = {}


def _true(case):
    """Inputs and the true reference of a case, computed once for the tests of this file."""
    if case.id not in _refs:
        inp = case.inputs('cpu')
        _refs[case.id] = inp + ext_reference(inp[0], inp[1], inp[2], inp[3], case.scale, case.causal)
    return _refs[case.id]


def test_case_table_covers_what_the_issue_lists():
    keys = {c.key for c in CASES}
    assert len(keys) == len(CASES)
    for S in EDGE_S:
        for cfg in TOY:
            assert (1, S) + cfg in keys
    for key in [(1, 512, 64, 64, 64, False, True), (1, 77, 12, 12, 64, True, False)] + [(1, S, 28, 4, 128, True, False) for S in (40, 333, 1058)]:
        assert key in keys
    for B in (2, 3):
        for S in (65, 200):
            assert (B, S) + TOY[2] in keys and (B, S) + TOY[0] in keys
    for d in (64, 128):
        assert {c.layout for c in CASES if c.d == d} == {'packed', 'separate'}
        assert {c.plant for c in CASES if c.d == d and c.causal} == {'diag', 'rand'}
    for m in MUTATIONS:
        assert TEETH[m], m


@pytest.mark.parametrize('case', _TEETH_CASES, ids=[c.id for c in _TEETH_CASES])
def test_reference_equals_plain_softmax_and_admits_a_faithful_kernel(case):
    """(a) ext_reference = the plain fp64 softmax implementation to 1e-12;  (c) the reference rounded to bf16 is within the bound of itself everywhere, and so is
    an fp32 emulation of the kernel's rounding points (fp32 scores, one fp32 add of the table entry, fma(s, c, -m c), P rounded to bf16 in front of P.V, l from
    the unrounded P): the bound must admit a faithful implementation before a kernel is held to it."""
    q, k, v, bias, _, _, O, OB = _true(case)
    B, S, H, d = q.shape
    plain = softmax_reference(q, k, v, bias, case.scale, case.causal)
    assert float((O - plain).abs().max()) < 1e-12
    assert bool((OB > 0).all()) and bool(torch.isfinite(OB).all())
    check_bf16_bound(O.float().bfloat16(), O, OB, f'{case.id}: the reference rounded to bf16')
    group = H // k.shape[2]
    qf = q.float().permute(0, 2, 1, 3)
    kf, vf = (t.float().permute(0, 2, 1, 3).repeat_interleave(group, 1) for t in (k, v))
    s = qf @ kf.transpose(-1, -2)
    idx = torch.arange(S)
    if bias is not None:
        s = s + bias[:, (idx[None, :] - idx[:, None]) + S - 1]
    if case.causal:
        s = s.masked_fill(idx[None, :] > idx[:, None], float('-inf'))
    c = torch.tensor(c32(case.scale), dtype=torch.float32)
    m = s.amax(-1, keepdim=True)
    P = torch.exp2(torch.addcmul(-(m * c), s, c))
    o = ((P.bfloat16().float() @ vf) * (1.0 / P.sum(-1, keepdim=True))).permute(0, 2, 1, 3).reshape(B * S, H * d).bfloat16()
    worst = check_bf16_bound(o, O, OB, f'{case.id}: fp32 emulation')
    print(f'{case.id}: fp32 emulation worst err / tol {worst:.3f}')


@pytest.mark.parametrize('mutate,case', _PAIRS, ids=[f'{m}-{c.id}' for m, c in _PAIRS])
def test_each_mutation_separates_on_its_rows(mutate, case):
    """(b) On at least 0.9 of the rows the mutation is held on, some element has |O64 - O64_mut| > 2 (ulp + bound), with the larger tolerance of the two
    references: no output within the bound of the true reference is within the bound of the mutated one there."""
    q, k, v, bias, design, plant_key, O, OB = _true(case)
    B, S, H, d = q.shape
    Om, OBm = ext_reference(q, k, v, bias, case.scale, case.causal, mutate=mutate)
    sep = separated_rows(O, OB, Om, OBm, B, S, H, d)
    target = teeth_targets(case, mutate, design, plant_key)
    n = int(target.sum())
    assert n >= 1, 'no row to hold the mutation on'
    share = sep[target].double().mean().item()
    by_design = [round(sep[:, :, [h for h in range(H) if design[h] == des]].double().mean().item(), 3) if bool((design == des).any()) else None for des in range(4)]
    print(f'{mutate} {case.id}: {n} targeted rows, share {share:.3f}; all rows by design {by_design}')
    assert share >= TEETH_SHARE, (mutate, case.id, share)
