"""fp64 reference of the joint attention backward with a per-element error bound read off the kernels (device-agnostic: no kernel is called here).

The operation (afx_attn_bwd.hip, afx_attn_bwd3.hip + afx_attn_bwd3_kernel.inc, tools/gen_attn_bwd3.py), with q, k, v, o, dO (bf16) and the forward's
row statistic L = lse (fp32, log2 domain) taken as EXACT inputs, c = fp32(fp32(1/sqrt(128)) * fp32(log2 e)) (C32) and SCALE = fp32(1/sqrt(128)):
  s = q . k      P = exp2(s c - L)      delta_q = sum_d dO O      dP = dO V^T      dS = P o (dP - delta)
  dV = P^T dO      dK = SCALE dS^T Q      dQ = SCALE dS K
The reference evaluates exactly this in fp64.  It is NOT softmax attention differentiated: P is whatever the given L makes it (sum_k P = 1 only as far as
L is the true log-sum-exp; `rowsum` is returned so that the caller can hold the convention), and delta comes from the given, bf16-rounded O.

The bound, with u = 2^-24 (fp32 unit roundoff; one fp32 ulp = 2 u) per pair (q, k) unless said otherwise:

 (1) P.  The score is an fp32 MFMA sum of exact bf16 products on v_mfma_f32_32x32x16_bf16: K = 128 in 8 steps plus a serial chain over one instruction's
     16 products, depth D_s = 128 / 16 + 16 = 24:  |s^ - s| <= ds = D_s u sum_d |q_d k_d|.  The exponent a = s c - L is one v_fma_f32 in the generated
     streams (u |a|); the round-4 kernels write `sa * C_LOG2 - L`, which may round the product first (u |s c|) -- both are allowed.  v_exp_f32: its
     accuracy cannot be derived here; 2 fp32 ulp = 4 u are ALLOWED, as the forward test allows them (the ISA documents 1 ulp).  Hence, relative to P,
         eP = expm1(ln2 (c ds + u |a| + u |s c|)) (1 + 4 u) + 4 u              |P32 - P| <= eP P
 (2) x = dP - delta.  delta: 8 serial products (exact in fp32: bf16 x bf16) and 4 shuffle adds, depth D_d = 12 over sum_d |dO_d O_d| (attn_delta_kernel,
     attn_bwd_stats_kernel).  The generated streams start the dP MFMA chain FROM -delta (depth D_s over sum_d |dO_d V_kd| + |delta|); the round-4 kernels
     start from 0 and subtract delta afterwards, one rounding more: depth D_x = D_s + 1 = 25 covers both.
         ex = D_x u (sum_d |dO_d V_kd| + |delta_q|) + D_d u sum_d |dO_d O_qd|   |x^ - x| <= ex
 (3) Rounding to bf16 (v_cvt_pk_bf16_f32, round to nearest even): half a bf16 ulp of the value rounded, h(y) = ulp_bf16(y) / 2.  dV's operand is P32 rounded;
     dS32 = fl(P32 x^) (one v_mul_f32, from the UNROUNDED P32) is rounded for dK and dQ.  h(y) lies between 2^-9 |y| (top of a binade) and 2^-8 |y| (bottom).
     The issue quotes 2^-9 |y|; that is the best case, not a bound: an fp32 emulation of the rounding points above in plain torch -- no kernel -- exceeds a bound
     built on 2^-9 at 8 of the 9 shapes of the GPU test (by up to 1.4 tol, where a few addends carry an element and their roundings fall alike), so the term is
     the exact half ulp, taken at the largest value the kernel can be rounding (h is monotone).  test_attention_bwd_ref_cpu.py keeps that emulation.
         EP  = eP P + h(P (1 + eP))                                               |bf16(P32) - P|  <= EP
         E32 = eP P (|x| + ex) + P ex + u (1 + eP) P (|x| + ex)                  |dS32 - dS|      <= E32
         EdS = E32 + h(|dS| + E32)                                               |bf16(dS32) - dS| <= EdS
 (4) The accumulating products: fp32 MFMA chains over the streamed index, S_pad / 16 steps + 16 inside an instruction, D_a = S_pad / 16 + 16
     (S_pad = S rounded up to 64; the padded rows contribute exact zeros: L = +inf, masked keys or zero K^T columns):
         bV = EP^T |dO| + D_a u (P + EP)^T |dO|
 (5) The epilogue multiplies dK and dQ by SCALE (the same fp32 constant as here) in fp32, one rounding more, D_a + 1:
         bK = SCALE (EdS^T |Q| + (D_a + 1) u (|dS| + EdS)^T |Q|)                  bQ = SCALE (EdS |K| + (D_a + 1) u (|dS| + EdS) |K|)
     The output's rounding to bf16 is the ulp_bf16(ref) of the check (bf16_parity.check_bf16_bound), not part of these bounds.
No constant is fitted to what a kernel returns.

Mutated references (the teeth of tests/test_hip_attention_bwd_fp64.py): drop_key = j leaves key j of every batch out of dQ, dK, dV; drop_query = i leaves
query i out.  L, O and delta stay as given -- a kernel that skips a key or a query does exactly that.
"""
import math

import numpy as np
import torch
from bf16_parity import U32, bf16_ulp

SCALE32 = float(np.float32(0.08838834764831845))
C32 = float(np.float32(np.float32(0.08838834764831845) * np.float32(1.4426950408889634)))
LN2 = math.log(2.0)
D_S, D_X, D_D = 128 // 16 + 16, 128 // 16 + 16 + 1, 8 + 4


def exact_forward(q, k, v):
    """O [B, S, H, 128] and lse [B, H, S] of the base-2 softmax of s c, in fp64 (what the forward kernel approximates)."""
    qd, kd, vd = (t.double().permute(0, 2, 1, 3) for t in (q, k, v))        # [B, H, S, 128]
    t = (qd @ kd.transpose(-1, -2)) * C32
    m = t.amax(-1, keepdim=True)
    P = torch.exp2(t - m)
    l = P.sum(-1, keepdim=True)
    return ((P / l) @ vd).permute(0, 2, 1, 3), (m + torch.log2(l))[..., 0]


def attention_bwd_reference(q, k, v, o, do, lse, drop_key=None, drop_query=None, heads=4):
    """q, k, v, o, do [B, S, H, 128]; lse [B, H, >= S].  Returns a dict of fp64 tensors: dq, dk, dv and their bounds bq, bk, bv [B * S, H * 128] (the bounds
    without the output's bf16 ulp), rowsum [B, H, S] = sum_k exp2(s c - L) over ALL keys.  A few heads at a time: the fp64 matrices are S x S per head."""
    B, S, H, _ = q.shape
    dev = q.device
    out = {n: torch.empty(B, S, H, 128, dtype=torch.float64, device=dev) for n in ('dq', 'dk', 'dv', 'bq', 'bk', 'bv')}
    out['rowsum'] = torch.empty(B, H, S, dtype=torch.float64, device=dev)
    D_a = -(-S // 64) * 64 // 16 + 16
    u = U32
    for b in range(B):
        for h0 in range(0, H, heads):
            hs = slice(h0, min(H, h0 + heads))
            qd, kd, vd, od, dod = (t[b, :, hs].double().transpose(0, 1) for t in (q, k, v, o, do))         # [h, S, 128]
            L = lse[b, hs, :S].double()[..., None]                                                          # [h, S, 1]
            sc = (qd @ kd.transpose(1, 2)) * C32
            a = sc - L
            P = torch.exp2(a)
            eP = torch.expm1(LN2 * (C32 * D_S * u * (qd.abs() @ kd.abs().transpose(1, 2)) + u * a.abs() + u * sc.abs())) * (1 + 4 * u) + 4 * u
            del sc, a
            out['rowsum'][b, hs] = P.sum(-1)
            if drop_key is not None:
                P[:, :, drop_key] = 0
            if drop_query is not None:
                P[:, drop_query, :] = 0
            delta = (dod * od).sum(-1, keepdim=True)
            x = dod @ vd.transpose(1, 2) - delta
            ex = D_X * u * (dod.abs() @ vd.abs().transpose(1, 2) + delta.abs()) + D_D * u * (dod.abs() * od.abs()).sum(-1, keepdim=True)
            dS = P * x
            EP = eP * P + 0.5 * bf16_ulp(P * (1 + eP))
            xa = x.abs() + ex
            E32 = eP * P * xa + P * ex + u * (1 + eP) * P * xa
            del x, xa, ex
            EdS = E32 + 0.5 * bf16_ulp(dS.abs() + E32)
            AdS = dS.abs() + EdS
            del E32
            res = {'dv': P.transpose(1, 2) @ dod,
                   'bv': EP.transpose(1, 2) @ dod.abs() + D_a * u * ((P + EP).transpose(1, 2) @ dod.abs()),
                   'dk': SCALE32 * (dS.transpose(1, 2) @ qd),
                   'bk': SCALE32 * (EdS.transpose(1, 2) @ qd.abs() + (D_a + 1) * u * (AdS.transpose(1, 2) @ qd.abs())),
                   'dq': SCALE32 * (dS @ kd),
                   'bq': SCALE32 * (EdS @ kd.abs() + (D_a + 1) * u * (AdS @ kd.abs()))}
            for n, t in res.items():
                out[n][b, :, hs] = t.transpose(0, 1)
    for n in ('dq', 'dk', 'dv', 'bq', 'bk', 'bv'):
        out[n] = out[n].reshape(B * S, H * 128)
    return out


def tolerance(ref, bound):
    return bf16_ulp(ref) + bound


def row_share(hit, B, S, H, heads):
    """hit [B * S, H * 128] bool -> the share of (row, head) pairs of `heads` with a hit in some element."""
    return hit.reshape(B * S, H, 128)[:, heads].any(-1).double().mean().item()


def separated(true, mut, n):
    """Elements where no output can satisfy both references: |true - mutated| > twice the (larger) tolerance."""
    tol = torch.maximum(tolerance(true['d' + n], true['b' + n]), tolerance(mut['d' + n], mut['b' + n]))
    return (true['d' + n] - mut['d' + n]).abs() > 2 * tol


def teeth(q, k, v, o, do, lse, true=None):
    """The true reference, the two mutated ones (last real key / last real query dropped) and the shares of the criterion: of the random-design heads' rows
    (h % 4 == 3), the share where the mutated and the true reference differ in some element by more than twice the tolerance -- dQ rows for the dropped key,
    dK rows and dV rows, each on their own, for the dropped query.  `planted` holds, per planted-key head (h % 4 == 1) and batch, the largest
    |dV - dV_mut| / |dO[last query]| over the head: the weight the dropped query puts on its planted key."""
    B, S, H, _ = q.shape
    if true is None:
        true = attention_bwd_reference(q, k, v, o, do, lse)
    mk = attention_bwd_reference(q, k, v, o, do, lse, drop_key=S - 1)
    mq = attention_bwd_reference(q, k, v, o, do, lse, drop_query=S - 1)
    rnd = [h for h in range(H) if h % 4 == 3]
    shares = {'dq': row_share(separated(true, mk, 'q'), B, S, H, rnd), 'dk': row_share(separated(true, mq, 'k'), B, S, H, rnd),
              'dv': row_share(separated(true, mq, 'v'), B, S, H, rnd)}
    moved = ((true['dv'] - mq['dv']).abs().view(B, S, H, 128) / do[:, S - 1:].double().abs().clamp_min(2.0 ** -126)).amin(-1).amax(1)        # [B, H]
    planted = moved[:, [h for h in range(H) if h % 4 == 1]]
    return true, mk, mq, shares, planted
