"""fp64 parity, per element, of the text-encoder attention: the EXT instantiations attention_kernel<64, true> / <128, true> of afx_attn.hip with
v_transpose_kernel<64 | 128> in front, through afx_attention_ext_bf16 (T5-XXL, CLIP-L, Qwen2.5).

The kernel computes, per query i of head h with KV head h // (H / Hkv) and c = fp32(fp32(scale) * fp32(log2 e)):
  s_j = q . k_j, an fp32 sum of exact bf16 products on v_mfma_f32_32x32x16_bf16 (HD / 16 steps);  s'_j = s_j + bias[h][j - i + S - 1], one fp32 add, only with a
  table;  keys j > i (causal) and j >= S removed;  a_j = fma(s'_j, c, -m c) with m the deferred running max (a_j <= 5);  P_j = exp2(a_j) in fp32, rounded to
  bf16 for P.V;  l = sum of the UNROUNDED P_j;  O = (sum_j bf16(P_j) v_j) * (1 / l), rounded to bf16.
The fp64 reference (attention_ext_ref.ext_reference) is the exact base-2 softmax of (q . k + bias) c over the same keys with the same fp32 c, O64 = Pn V.

The bound is the one derived in test_hip_attention_fp64.py, term by term, with u = 2^-24, W = sum_j Pn_j |v_j|, Wa = sum_j Pn_j (|a_j| + 5) |v_j| (fp64, per
element, over the keys the row keeps):

  |O - O64| <= ulp_bf16(O64) + (2^-8 + eps) W + 2 ln2 u Wa + 4 u |O64|
    2^-8       P rounded to bf16 before P.V.
    eps        2 (ln2 c ds + 4 u)  +  (D_l + D_pv + 4) u
      ds       max over the row's kept keys of (HD / 16 + 16) u sum_d |q_d k_jd| [+ u (|s_j| + |bias_j|) with a table]: HD / 16 MFMA steps + a serial chain over
               one instruction's 16 products -- depth 20 at head dim 64, 24 at 128 (the joint file takes 36, the larger of its two kernels) -- and the one fp32
               add of the table entry, whose rounding is u |s_j + bias_j| <= u (|s_j| + |bias_j|).  Times c ln 2 it is P's relative error, twice (numerator, l).
               c is the runtime fp32 product above: 1.0 * log2 e for T5, d^-0.5 * log2 e otherwise.
      4 u      v_exp_f32, 2 fp32 ulp allowed per instruction, as there.
      D_l      fp32 depth of l over the keys the row VISITS, n = i + 1 under the causal mask, S otherwise: ceil(n / 64) tile adds + 40 inside a tile.  A masked
               key adds exp2(-inf) = 0 exactly, and so does a whole tile right of the diagonal that the work-group still walks for its later rows.
      D_pv     fp32 depth of the P.V accumulator over the same keys: ceil(n / 16) MFMA steps + 32.
      + 4 u    the reciprocal and the multiply of the normalisation.
    2 ln2 u Wa the rounding of the exp2 argument (u |a_j| absolute; a_j <= |a64_j| + 5 by the deferred max).
  Terms of the joint derivation that do not carry over: the KV-split doubling of 2^-8 and its 2 ln2 E_lse + 16 u (the EXT launch has one pass over the keys, no
  bf16 partial rows), and the whole lse bound (the EXT launches pass lse = nullptr).  Nothing is added in their place and no number above was fitted to the
  kernel: test_attention_ext_ref_cpu.py shows on the CPU that an fp32 emulation of these rounding points stays at about half of the bound.

Inputs (attention_ext_ref.ext_inputs): the four head designs of attention_inputs.head_design_inputs at head dim 64 / 128 with separate H and Hkv -- the KV heads
carry different designs, so h % Hkv instead of h // group reads another design; planted keys on the diagonal or at a random j <= i under the causal mask; an
N(0, 1) bias table with one +-8 ramp head that fires the deferred rescale on its own; q, k at 0.35 where the scale is 1.
Every launch is watched: O is a column view inside a buffer of sentinels (border untouched), the V^T workspace is filled with 0xFF bytes (bf16 NaN) and has a
guard tail (a pad key that the transpose does not zero, or that is read unmasked, gives 0 x NaN = NaN in O), and q, k, v sit inside buffers whose other rows and
columns hold NaN (the kernel clamps ragged key and query rows to S - 1; a NaN in O is a read outside the operands).  Layouts: 'packed' rows q | k | v as the
encoders, 'separate' three buffers of three row strides with k and v at a column offset.
Teeth (attention_ext_ref.TEETH, proved separable without a device by test_attention_ext_ref_cpu.py): the output is rejected by each of seven mutated references
-- causal j >= i, tile skip one short, bias index + 1, KV head h % Hkv, last ragged key dropped, 128^-0.5 at head dim 64, V^T of batch 0 -- on every row where the
two references are more than twice the tolerance apart.
"""
import pytest
import torch
from attention_ext_ref import CASES, TEETH_SHARE, ext_reference, mutations_of, rejected_rows, separated_rows, teeth_targets
from bf16_parity import check_bf16_bound

pytestmark = pytest.mark.gpu

SENT = -7.75
AFX_E_INVALID = -1
NAN = float('nan')


@pytest.fixture(scope='module')
def lib():
    from arcflow_amd import _lib
    return _lib.load()


def _p(t):
    from arcflow_amd.text_encoders import _p as p
    return p(t)


def _s():
    from arcflow_amd.text_encoders import _s as s
    return s()


def _operands(q, k, v, layout):
    """q, k, v [B, S, heads, d] -> three 2-D views [B*S, heads*d] with their row strides, inside NaN-filled buffers with 8 NaN rows in front and behind."""
    B, S, H, d = q.shape
    R, Dq, Dk = B * S, H * d, k.shape[2] * d
    nanbuf = lambda w: torch.full((R + 16, w), NAN, dtype=torch.bfloat16, device='cuda')        # noqa: E731
    if layout == 'packed':
        buf = nanbuf(Dq + 2 * Dk)
        views = (buf[8:8 + R, :Dq], buf[8:8 + R, Dq:Dq + Dk], buf[8:8 + R, Dq + Dk:])
    else:
        views = (nanbuf(Dq + 8)[8:8 + R, :Dq], nanbuf(Dk + 24)[8:8 + R, 8:8 + Dk], nanbuf(Dk + 40)[8:8 + R, 16:16 + Dk])
        assert len({t.stride(0) for t in views}) == 3
    for dst, src, w in zip(views, (q, k, v), (Dq, Dk, Dk)):
        dst.copy_(src.reshape(R, w))
    return views


def _run(lib, case, q, k, v, bias):
    """One afx_attention_ext_bf16 call with every watch armed; returns O [B*S, H*d] bf16 (a view into the guarded buffer)."""
    from arcflow_amd import _lib
    B, S, H, Hkv, d = case.B, case.S, case.H, case.Hkv, case.d
    R, Dq = B * S, H * d
    qv, kv, vv = _operands(q, k, v, case.layout)
    obuf = torch.full((R + 16, Dq + 128), SENT, dtype=torch.bfloat16, device='cuda')
    o = obuf[8:8 + R, 64:64 + Dq]
    nws = lib.afx_attention_ext_ws_bytes(B, Hkv, S, d)
    assert nws == B * Hkv * d * (-(-S // 64) * 64) * 2
    ws = torch.full((nws + 256,), 0xFF, dtype=torch.uint8, device='cuda')
    _lib.check(lib.afx_attention_ext_bf16(_p(qv), qv.stride(0), _p(kv), kv.stride(0), _p(vv), vv.stride(0), _p(o), o.stride(0), _p(ws), B, H, Hkv, S, d,
                                          case.scale, int(case.causal), _p(bias), _s()))
    torch.cuda.synchronize()
    mask = torch.ones(obuf.shape, dtype=torch.bool, device='cuda')
    mask[8:8 + R, 64:64 + Dq] = False
    assert bool((obuf[mask] == SENT).all()), f'{case.id}: a write landed in the guard band of O'
    assert bool((ws[nws:] == 0xFF).all()), f'{case.id}: a write landed behind the V^T workspace'
    nan_rows = torch.isnan(o.float()).any(-1).nonzero().flatten().tolist()
    assert not nan_rows, f'{case.id}: NaN in O rows {nan_rows[:8]} (b = row // S, query = row % S): a pad key of the workspace or a row outside q / k / v was read'
    return o


@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_attention_ext_vs_fp64(lib, case):
    """Every output element of the case within the derived bound of the fp64 reference; then, at the cases that carry teeth, the same output rejected by each
    mutated reference on every targeted row where the two references are separated (and those are at least 0.9 of the targeted rows)."""
    B, S, H, d = case.B, case.S, case.H, case.d
    q, k, v, bias, design, plant_key = case.inputs('cuda')
    o = _run(lib, case, q, k, v, bias)
    O, OB = ext_reference(q, k, v, bias, case.scale, case.causal)
    worst = check_bf16_bound(o, O, OB, case.id)
    print(f'ext-attention {case.family} {case.id}: worst err / tol {worst:.3f}')
    for mutate in mutations_of(case):
        Om, OBm = ext_reference(q, k, v, bias, case.scale, case.causal, mutate=mutate)
        target = teeth_targets(case, mutate, design, plant_key)
        held = target & separated_rows(O, OB, Om, OBm, B, S, H, d)
        share = held.sum().item() / target.sum().item()
        assert share >= TEETH_SHARE, (mutate, case.id, share)
        missed = held & ~rejected_rows(o, Om, OBm, B, S, H, d)
        assert not bool(missed.any()), f'{case.id}: the output passes the reference mutated by {mutate} on rows (b, query, head) {missed.nonzero()[:8].tolist()}'
        with pytest.raises(AssertionError):
            check_bf16_bound(o, Om, OBm, f'{case.id} {mutate}')


def test_attention_ext_argument_guards(lib):
    """Every bad argument is refused on the host with the invalid-argument code, nothing is launched and the output keeps its sentinel.  The good call in front
    proves that the same arguments do run."""
    B, S, H, Hkv, d = 1, 17, 4, 4, 64
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(S, 3 * H * d, generator=g).bfloat16().cuda()
    Dq = H * d
    ws = torch.zeros(lib.afx_attention_ext_ws_bytes(2, Hkv, S, 128), dtype=torch.uint8, device='cuda')
    bias = torch.zeros(H, 2 * S - 1, device='cuda')
    o = torch.full((S, Dq), SENT, dtype=torch.bfloat16, device='cuda')
    ld = qkv.stride(0)
    good = dict(q=_p(qkv), ldq=ld, k=_p(qkv[:, Dq:]), ldk=ld, v=_p(qkv[:, 2 * Dq:]), ldv=ld, o=_p(o), ldo=Dq, ws=_p(ws), B=B, H=H, Hkv=Hkv, S=S, d=d,
                scale=0.125, causal=0, bias=_p(bias))

    def call(**change):
        a = dict(good, **change)
        rc = lib.afx_attention_ext_bf16(a['q'], a['ldq'], a['k'], a['ldk'], a['v'], a['ldv'], a['o'], a['ldo'], a['ws'], a['B'], a['H'], a['Hkv'], a['S'], a['d'],
                                        a['scale'], a['causal'], a['bias'], _s())
        torch.cuda.synchronize()
        return rc

    bad = [dict(Hkv=3), dict(H=6, Hkv=4), dict(d=96), dict(d=32), dict(d=0), dict(ldq=ld + 4), dict(ldk=ld + 1), dict(ldv=ld + 2), dict(ldo=Dq + 4),
           dict(scale=0.0), dict(scale=-0.125), dict(scale=NAN), dict(S=0), dict(S=-1), dict(B=0), dict(B=-1), dict(H=0, Hkv=0), dict(Hkv=0),
           dict(q=None), dict(k=None), dict(v=None), dict(o=None), dict(ws=None)]
    for change in bad:
        assert call(**change) == AFX_E_INVALID, f'{change} was not refused'
        assert b'afx_attention_ext_bf16' in lib.afx_last_error()
        assert bool((o == SENT).all()), f'{change}: refused, but the output was written'
    assert call() == 0
    assert not bool((o == SENT).any())
