"""fp64 parity of the joint attention forward (O and its log2-domain log-sum-exp) and of its block-scaled fp8 epilogue.

The kernels (afx_attn.hip, afx_attn3.hip) compute, per query row, with c = fp32(1/sqrt(128)) * fp32(log2 e) rounded to fp32:
  scores s_j = q . k_j, an fp32 MFMA sum of exact bf16 products;  a_j = fma(s_j, c, -m c) with m the running max (deferred: a_j <= 5);
  P_j = exp2(a_j) in fp32, rounded to bf16 for P.V;  l = sum of the UNROUNDED fp32 P_j;  O = (sum_j bf16(P_j) v_j) * (1 / l);  lse = m c + log2(l).
A KV-split row (impl 0) is first finished per key range as a normalised bf16 partial + fp32 lse_p; the long part starts from the partials merged
with exp2(lse_p - max) weights.  The fp64 reference is the exact base-2 softmax of s c (same fp32 c), O64 = Pn V with Pn = P / l, lse64 = log2 sum
exp2(s c).  With u = 2^-24 and W = sum_j Pn_j |v_j|, Wa = sum_j Pn_j (|a_j| + 5) |v_j| (fp64, per element):

  |O - O64| <= ulp_bf16(O64) + (2^-8 [+ 2^-8 split] + eps) W + 2 ln2 u Wa + 4 u |O64|
    2^-8       P rounded to bf16 before P.V (bf16 keeps 8 significant bits: relative error <= 2^-8; [split] once more for the bf16 partial rows)
    eps        2 (ln2 c ds + 4 u)  +  (D_l + D_pv + 4) u  [+ 2 ln2 E_lse + 16 u split]
      ds       score summation bound 36 u sum_d |q_d k_jd| (max over the row's keys): K = 128 in MFMA steps of 16 or 32 + a serial chain over one
               instruction (depth 128 / 16 + 16 <= 128 / 32 + 32 = 36); times c ln 2 it is P's relative error, twice (numerator and l).
      4 u      v_exp_f32: 2 fp32 ulp allowed per instruction (not measured here; the ISA documents 1 ulp); v_log_f32 / v_rcp_f32 likewise.
      D_l      fp32 depth of l: ceil(S / 64) tile adds + 40 inside a tile (16 pairs, the pair sum, the half-wave exchange).
      D_pv     fp32 depth of the P.V accumulator: ceil(S / 16) MFMA steps + 32.
      + 4 u    the reciprocal and the multiply of the normalisation.
    2 ln2 u Wa the rounding of the exp2 argument: u |a_j| absolute, P's relative error ln2 u |a_j| (a_j <= |a64_j| + 5: the deferred max).
  |lse - lse64| <= E_lse = c ds + (D_l + 8) u / ln2 + u sum_j Pn_j (|a_j| + 5) + 2 u |lse64| + 4 u (|log2 l| + 1)     (log2 units)
    the score error, l's summation and exp2 (relative -> / ln 2), the argument roundings, the final add, v_log_f32 (2 ulp of its result).
    KV split: 2 E_lse + 16 u / ln2 + 2 u |lse64| (the partials' own error enters through the merge weights, then the long part's).
At S = 4608 and the random heads below E_lse is about 2e-5 (4e-5 split); one missing key moves lse by about 1 / (S ln 2 e^0.07) = 3e-4.

Inputs: 4 head designs, each for a failure that plain randn inputs hide -- (0) V positive with a non-zero mean: W ~ |O| and the bound is relative;
(1) one planted dominant key per query at a permuted position: O ~ v_pi(i), any key or V^T addressing error is gross; (2) scores grown tile after
tile: the deferred rescale (RESCALE_LOG2) fires again and again; (3) plain random heads (q, k at 0.6: every key carries ~1/S of the row).
Teeth: with the last real key of a ragged S left out of the reference, the LSE bound fails on >= 99 % of the random heads' rows.
O is written over Q (attention_fwd_lse_2d, as the engine does) inside a buffer whose guard columns / rows hold a sentinel; the fp8 bytes and
scale bytes of attention_to_mx8 likewise (0xA5).
"""
import math

import numpy as np
import pytest
import torch
from attention_inputs import head_design_inputs as _inputs
from bf16_parity import U32, check_bf16_bound as _check_o, check_f32

pytestmark = pytest.mark.gpu

SENT = -7.75
C32 = float(np.float32(np.float32(0.08838834764831845) * np.float32(1.4426950408889634)))
LN2 = math.log(2.0)


@pytest.fixture(scope='module')
def ops():
    from arcflow_amd import ops as _ops
    return _ops


def _reference(q, k, v, split, drop_last=False):
    """fp64 O, its per-element bound (without the output ulp), lse and its per-row bound; a few heads at a time."""
    B, S, H, _ = q.shape
    O = torch.empty(B, S, H, 128, dtype=torch.float64, device='cuda')
    OB = torch.empty_like(O)
    L = torch.empty(B, H, S, dtype=torch.float64, device='cuda')
    LB = torch.empty_like(L)
    D_l, D_pv = -(-S // 64) + 40, -(-S // 16) + 32
    n = S - 1 if drop_last else S
    for b in range(B):
        for h0 in range(0, H, 4):
            hs = slice(h0, min(H, h0 + 4))
            qd, kd, vd = (t[b, :, hs].double().transpose(0, 1) for t in (q, k, v))        # [h, S, 128]
            kd, vd = kd[:, :n], vd[:, :n]
            s = (qd @ kd.transpose(1, 2)) * C32
            ds = 36 * U32 * (qd.abs() @ kd.abs().transpose(1, 2)).amax(-1)                # [h, S]
            m = s.amax(-1, keepdim=True)
            a = s - m
            P = torch.exp2(a)
            l = P.sum(-1, keepdim=True)
            Pn = P / l
            lse = (m + torch.log2(l))[..., 0]
            o = Pn @ vd
            W = Pn @ vd.abs()
            Wa = (Pn * (a.abs() + 5)) @ vd.abs()
            e_lse = C32 * ds + (D_l + 8) * U32 / LN2 + U32 * (Pn * (a.abs() + 5)).sum(-1) + 2 * U32 * lse.abs() \
                + 4 * U32 * (torch.log2(l[..., 0]).abs() + 1)
            eps = 2 * (LN2 * C32 * ds + 4 * U32) + (D_l + D_pv + 4) * U32
            rel = 2.0 ** -8
            if split:
                eps = eps + 2 * LN2 * e_lse + 16 * U32
                rel = 2 * rel
                e_lse = 2 * e_lse + 16 * U32 / LN2 + 2 * U32 * lse.abs()
            O[b, :, hs] = o.transpose(0, 1)
            OB[b, :, hs] = ((rel + eps[..., None]) * W + 2 * LN2 * U32 * Wa + 4 * U32 * o.abs()).transpose(0, 1)
            L[b, hs] = lse
            LB[b, hs] = e_lse
    return O.reshape(B * S, H * 128), OB.reshape(B * S, H * 128), L, LB


def _run(ops, q, k, v, impl):
    """attention_fwd_lse_2d with O over Q inside a guarded buffer: (O [B*S, H*128] bf16, lse [B, H, S_pad], buffer check)."""
    B, S, H, _ = q.shape
    buf = torch.full((B * S + 16, H * 128 + 128), SENT, dtype=torch.bfloat16, device='cuda')
    qo = buf[8:8 + B * S, 64:64 + H * 128]
    qo.copy_(q.reshape(B * S, H * 128))
    ops.set_attn_impl(impl)
    try:
        lse = ops.attention_fwd_lse_2d(qo, k.reshape(B * S, H * 128), v.reshape(B * S, H * 128), qo, B, S, H)
        torch.cuda.synchronize()
    finally:
        ops.set_attn_impl(0)
    mask = torch.ones(buf.shape, dtype=torch.bool, device='cuda')
    mask[8:8 + B * S, 64:64 + H * 128] = False
    assert bool((buf[mask] == SENT).all()), f'impl {impl}: a write landed in the guard band'
    assert bool(torch.isinf(lse[:, :, S:]).all()), f'impl {impl}: lse written past S'
    return qo, lse[:, :, :S]


SHAPES = [(1, 4608, 24), (1, 4224, 24), (1, 4173, 24), (3, 4608, 24), (2, 1101, 24), (1, 65, 4), (1, 191, 4), (1, 576, 9)]


@pytest.mark.parametrize('B,S,H', SHAPES, ids=[f'{b}x{s}x{h}' for b, s, h in SHAPES])
def test_attention_forward_vs_fp64(ops, B, S, H):
    """impl 0 (KV split + hand-over where the last round is under-filled), 1 (4-wave kernel), 3 (plain grid): O per element, lse per row."""
    q, k, v = _inputs(B, S, H, seed=B * 100000 + S * 10 + H)
    refs = {}
    for impl in (3, 1, 0):
        split = impl == 0
        if split not in refs:
            refs[split] = _reference(q, k, v, split)
        O, OB, L, LB = refs[split]
        o, lse = _run(ops, q, k, v, impl)
        what = f'B={B} S={S} H={H} impl={impl}'
        _check_o(o, O, OB, f'{what}: O')
        check_f32(lse, L, LB, what=f'{what}: lse')
        if S == 4173 and B == 1:
            # teeth: the last real key left out of the reference moves lse beyond the bound on the random heads' rows
            if ('drop', split) not in refs:
                refs[('drop', split)] = _reference(q, k, v, split, drop_last=True)[2]
            Ld = refs[('drop', split)]
            rnd = [h for h in range(H) if h % 4 == 3]
            fails = ((lse[:, rnd].double() - Ld[:, rnd]).abs() > LB[:, rnd]).double().mean().item()
            assert fails >= 0.99, f'{what}: the LSE bound misses a dropped key on {1 - fails:.4f} of the random rows'


def _mx_exp64(x):
    return (torch.ceil(torch.log2(x.clamp_min(1e-300) / 448.0)) + 127).clamp(1, 254).long()


def _e4m3_ord(codes):
    c = codes.long()
    mag = c & 0x7f
    return torch.where((c & 0x80) != 0, -mag, mag)


def _rne_e4m3_ord(x):
    return _e4m3_ord(x.clamp(-448, 448).float().to(torch.float8_e4m3fn).view(torch.uint8))


@pytest.mark.parametrize('B,S,H', [(1, 4608, 8), (2, 333, 4)])
def test_attention_to_mx8_vs_fp64(ops, B, S, H):
    """The fp8 epilogue (plain grid, fp32 O quantised per token and head): E8M0 = ceil(log2(blockmax64 / 448)) and e4m3 = RNE(O64 / 2^e), each exempt
    only where the O bound (without the bf16 ulp) straddles a power of two / an e4m3 midpoint -- then between the two candidates.  The positive-V
    and planted-key heads (bounds relative to |O|) carry the exempt-share limits; every head is held to the candidates."""
    q, k, v = _inputs(B, S, H, seed=S + H)
    O, OB, _, _ = _reference(q, k, v, split=False)
    R = B * S
    obuf = torch.full((R + 16, H * 128 + 128), 0xA5, dtype=torch.uint8, device='cuda')
    mbuf = torch.full((R + 16, H + 8 + (-H) % 4), 0xA5, dtype=torch.uint8, device='cuda')
    o8, mx = obuf[8:8 + R, 64:64 + H * 128], mbuf[8:8 + R, 4:4 + H]
    ops.attention_to_mx8(q, k, v, out=(o8, mx))
    torch.cuda.synchronize()
    for buf, c0, n in ((obuf, 64, H * 128), (mbuf, 4, H)):
        mask = torch.ones(buf.shape, dtype=torch.bool, device='cuda')
        mask[8:8 + R, c0:c0 + n] = False
        assert bool((buf[mask] == 0xA5).all()), 'attention mx8: a write landed in the guard band'
    blocks, fb = O.view(R, H, 128), OB.view(R, H, 128)
    bm = blocks.abs().amax(-1)
    slack = fb.amax(-1) + 2 * U32 * bm
    lo, hi, want = _mx_exp64((bm - slack).clamp_min(0)), _mx_exp64(bm + slack), _mx_exp64(bm)
    got = mx.long()
    assert bool(((got >= lo) & (got <= hi)).all()), 'attention mx8: an E8M0 byte outside its candidates'
    ex_b = lo != hi
    assert bool((got[~ex_b] == want[~ex_b]).all()), 'attention mx8: E8M0 bytes off ceil(log2(max / 448))'
    sc = torch.exp2(got.double() - 127)[..., None]
    clo, chi = _rne_e4m3_ord((blocks - fb) / sc), _rne_e4m3_ord((blocks + fb) / sc)
    gq = _e4m3_ord(o8).view(R, H, 128)
    assert bool(((gq >= clo) & (gq <= chi)).all()), f'attention mx8: {int(((gq < clo) | (gq > chi)).sum())} e4m3 codes outside their candidates'
    ex_c = clo != chi
    assert bool((gq[~ex_c] == clo[~ex_c]).all()), 'attention mx8: e4m3 codes off RNE(O64 / 2^e)'
    tight = [h for h in range(H) if h % 4 in (0, 1)]
    nb, nc = ex_b[:, tight].double().mean().item(), ex_c[:, tight].double().mean().item()
    print(f'attention mx8 B={B} S={S} H={H}: exempt scale bytes {ex_b.double().mean().item():.4f} (tight heads {nb:.4f}), '
          f'codes {ex_c.double().mean().item():.4f} (tight heads {nc:.4f})')
    assert nb <= 0.05 and nc <= 0.25, (nb, nc)
