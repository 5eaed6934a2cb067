"""fp64 reference, per-element bound, inputs and case table of the text-encoder (EXT) attention: shared by test_hip_attention_ext_fp64.py (the kernel on
the device) and test_attention_ext_ref_cpu.py (the reference, the bound and the teeth criterion without a device).  The derivation of the bound is in the
docstring of test_hip_attention_ext_fp64.py."""
import math

import numpy as np
import torch
from bf16_parity import U32, bf16_ulp

LN2 = math.log(2.0)
LOG2E32 = np.float32(1.4426950408889634)
KVB, QB = 64, 128                      # keys per tile, queries per work-group (afx_attn.hip)
PLANT_NATS = 20.0                      # scaled score of a planted key, as in attention_inputs.head_design_inputs (1.77 * 128 / sqrt(128))


def c32(scale):
    """The kernel's exponent factor: fp32(fp32(scale) * fp32(log2 e))."""
    return float(np.float32(np.float32(scale) * LOG2E32))


def default_scale(d, use_bias):
    """T5 folds its scale into the weights (1.0, with the bias table); CLIP and Qwen2.5 use d^-0.5."""
    return 1.0 if use_bias else d ** -0.5


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------
def ext_inputs(B, S, H, Hkv, d, causal, use_bias, scale, seed, plant='diag'):
    """q [B, S, H, d], k, v [B, S, Hkv, d] bf16, bias [H, 2S-1] fp32 or None, design [H], plant_key [B, S, H] (the planted key of a row, -1: none) -- on the CPU generator whatever the device,
    so that the CPU test of the teeth sees the numbers the GPU test runs.  KV head g has design g % 4 of attention_inputs.head_design_inputs and the H / Hkv
    query heads of its group follow it, so a query head sent to another KV head meets another design:
      0  V positive with a non-zero mean;
      1  a planted dominant key per query (k = f q, f q.q scale = 20 nats; the query heads of a group share the planted direction and differ by 0.3 noise).
         Not causal: at a permuted position.  Causal: plant 'diag' on the diagonal (j = i), plant 'rand' at pi(i) for the queries with pi(i) <= i of a
         random permutation pi (a key can carry one query, so about half of the rows; the others stay unplanted);
      2  scores growing tile after tile by 32 nats over the row: the deferred rescale fires again and again;
      3  plain heads, q and k scaled by 0.6.
    With a bias table at scale 1 (T5) q and k are drawn at 0.35, so q.k stays in T5's range.  The table is N(0, 1); on the design-3 heads it is a ramp from -8
    to +8 over the 2S - 1 offsets plus N(0, 0.5), clamped to +-8: 8 nats = 11.5 in the exponent across one row, the deferred rescale fires from the bias alone."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)                     # noqa: E731
    group = H // Hkv
    sig = 0.35 if (use_bias and scale == 1.0) else 1.0
    q, k, v = rn(B, S, H, d) * sig, rn(B, S, Hkv, d) * sig, rn(B, S, Hkv, d)
    design = torch.tensor([(h // group) % 4 for h in range(H)])
    plant_key = torch.full((B, S, H), -1, dtype=torch.long)
    idx = torch.arange(S)
    for kv in range(Hkv):
        des, heads = kv % 4, range(kv * group, (kv + 1) * group)
        if des == 0:
            v[:, :, kv] = v[:, :, kv].abs() * 0.5 + 1.0
        elif des == 1:
            f = PLANT_NATS / (d * sig * sig * scale)
            qg = rn(B, S, d) * sig
            for h in heads:
                q[:, :, h] = qg + (0.3 * sig) * rn(B, S, d) if group > 1 else qg
            for b in range(B):
                pi = idx if (causal and plant == 'diag') else torch.randperm(S, generator=g)
                has = pi <= idx if causal else torch.ones(S, dtype=torch.bool)
                k[b, pi[has], kv] = qg[b, has] * f
                for h in heads:
                    plant_key[b, :, h] = torch.where(has, pi, -1)
        elif des == 2:
            base = rn(d)
            base = base / base.norm()
            a = 6.0 * sig
            for h in heads:
                q[:, :, h] += a * base
            k[:, :, kv] += (idx.float() / S * (32.0 / (a * scale)))[None, :, None] * base
        else:
            for h in heads:
                q[:, :, h] *= 0.6
            k[:, :, kv] *= 0.6
    bias = None
    if use_bias:
        bias = rn(H, 2 * S - 1)
        ramp = -8.0 + 16.0 * torch.arange(2 * S - 1).float() / max(1, 2 * S - 2)
        for h in range(H):
            if design[h] == 3:
                bias[h] = (ramp + 0.5 * rn(2 * S - 1)).clamp(-8.0, 8.0)
    return q.bfloat16(), k.bfloat16(), v.bfloat16(), bias, design, plant_key


# ---- reference --------------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ('causal_ge', 'tile_short', 'bias_shift', 'kv_mod', 'drop_last', 'scale_128', 'vt_batch0')


def _visible(S, causal, mutate, device):
    """[S queries, S keys] bool: the keys a query keeps.  The mutations that change the key set model (1) a causal mask that removes j >= i (row 0 keeps its
    only key), (2) a tile skip one tile short -- the last tile a 128-query block visits, min(S_pad / 64, 2 block + 2) - 1, is lost to its rows (a row left
    with no key keeps its keys) -- and (5) the last real key left out."""
    i = torch.arange(S, device=device)[:, None]
    j = torch.arange(S, device=device)[None, :]
    vis = (j <= i) if causal else torch.ones(S, S, dtype=torch.bool, device=device)
    if mutate == 'causal_ge':
        assert causal
        vis = (j < i) | ((i == 0) & (j == 0))
    elif mutate == 'tile_short':
        assert causal
        s_pad = -(-S // KVB) * KVB
        last = torch.minimum(torch.tensor(s_pad // KVB, device=device), 2 * (i // QB) + 2) - 1          # [S, 1]
        cut = vis & (j // KVB != last)
        vis = torch.where(cut.any(-1, keepdim=True), cut, vis)
    elif mutate == 'drop_last':
        vis = vis & (j < S - 1)
        vis[0, 0] = True                                                                                 # S = 1 / causal row 0: nothing else to keep
    return vis


def ext_reference(q, k, v, bias, scale, causal, mutate=None, heads_at_once=4):
    """fp64 O [B*S, H*d] of the exact base-2 softmax of (q.k + bias) c over the kept keys, c = c32(scale), and its per-element bound [B*S, H*d] without the
    output's bf16 ulp (see test_hip_attention_ext_fp64.py).  mutate: one of MUTATIONS, a reference with that feature subtly wrong."""
    assert mutate is None or mutate in MUTATIONS
    B, S, H, d = q.shape
    Hkv = k.shape[2]
    group = H // Hkv
    dev = q.device
    c = c32(128 ** -0.5) if mutate == 'scale_128' else c32(scale)       # 128^-0.5 at head dim 64
    if mutate == 'scale_128':
        assert d == 64 and scale == d ** -0.5
    vis = _visible(S, causal, mutate, dev)
    n_vis = vis.sum(-1).double()                                                        # keys a row visits
    D_l = torch.ceil(n_vis / KVB) + 40
    D_pv = torch.ceil(n_vis / 16) + 32
    depth = d // 16 + 16
    rel_idx = None
    if bias is not None:
        i = torch.arange(S, device=dev)
        rel_idx = i[None, :] - i[:, None] + S - 1
        bd = bias.double()
        if mutate == 'bias_shift':
            bd = torch.cat([bd[:, 1:], torch.zeros(H, 1, dtype=torch.float64, device=dev)], 1)          # j - i + S; the one entry past the table reads 0
    O = torch.empty(B, S, H, d, dtype=torch.float64, device=dev)
    OB = torch.empty_like(O)
    for b in range(B):
        for h0 in range(0, H, heads_at_once):
            hs = list(range(h0, min(H, h0 + heads_at_once)))
            kvh = [h % Hkv if mutate == 'kv_mod' else h // group for h in hs]
            qd = q[b][:, hs].double().transpose(0, 1)                                   # [h, S, d]
            kd = k[b][:, kvh].double().transpose(0, 1)
            vd = v[0 if mutate == 'vt_batch0' else b][:, kvh].double().transpose(0, 1)
            s = qd @ kd.transpose(1, 2)
            ds = depth * U32 * (qd.abs() @ kd.abs().transpose(1, 2))                    # per key: the fp32 MFMA sum of exact products
            if bias is not None:
                bb = bd[hs][:, rel_idx]                                                 # [h, S, S]
                ds = ds + U32 * (s.abs() + bb.abs())                                    # the one fp32 add of the table entry
                s = s + bb
            ds = ds.masked_fill(~vis, 0.0).amax(-1)                                     # [h, S]: max over the row's keys
            s = (s * c).masked_fill(~vis, float('-inf'))
            m = s.amax(-1, keepdim=True)
            a = s - m
            P = torch.exp2(a)
            Pn = P / P.sum(-1, keepdim=True)
            o = Pn @ vd
            W = Pn @ vd.abs()
            Wa = (Pn * (a.abs() + 5).masked_fill(~vis, 0.0)) @ vd.abs()
            eps = 2 * (LN2 * c * ds + 4 * U32) + (D_l + D_pv + 4) * U32
            O[b][:, hs] = o.transpose(0, 1)
            OB[b][:, hs] = ((2.0 ** -8 + eps[..., None]) * W + 2 * LN2 * U32 * Wa + 4 * U32 * o.abs()).transpose(0, 1)
    return O.reshape(B * S, H * d), OB.reshape(B * S, H * d)


def softmax_reference(q, k, v, bias, scale, causal):
    """The same operation written the plain way (natural-base torch.softmax of s c ln 2, repeat_interleave for the groups, masked_fill): what (a) of the CPU test
    holds ext_reference to."""
    B, S, H, d = q.shape
    group = H // k.shape[2]
    qd = q.double().permute(0, 2, 1, 3)
    kd = k.double().permute(0, 2, 1, 3).repeat_interleave(group, 1)
    vd = v.double().permute(0, 2, 1, 3).repeat_interleave(group, 1)
    s = qd @ kd.transpose(-1, -2)
    idx = torch.arange(S, device=q.device)
    if bias is not None:
        s = s + bias.double()[:, (idx[None, :] - idx[:, None]) + S - 1]
    s = s * (c32(scale) * LN2)
    if causal:
        s = s.masked_fill(idx[None, :] > idx[:, None], float('-inf'))
    return (torch.softmax(s, -1) @ vd).permute(0, 2, 1, 3).reshape(B * S, H * d)


def separated_rows(O, OB, Om, OBm, B, S, H, d):
    """[B, S, H] bool: rows where some element has |O - Om| > 2 max(ulp + bound of either reference) -- no output can be within the bound of both."""
    tol = torch.maximum(bf16_ulp(O) + OB, bf16_ulp(Om) + OBm)
    return ((O - Om).abs() > 2 * tol).view(B, S, H, d).any(-1)


def rejected_rows(out, Om, OBm, B, S, H, d):
    """[B, S, H] bool: rows of a bf16 output where some element is beyond the bound of the (mutated) reference."""
    return ((out.double() - Om).abs() > bf16_ulp(Om) + OBm).view(B, S, H, d).any(-1)


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """One launch: shape, features, the planted-key variant, and how q, k, v lie in memory ('packed' as the encoders, 'separate' three buffers of three strides)."""

    def __init__(self, B, S, H, Hkv, d, causal, use_bias, plant='diag', layout='packed', family='toy'):
        self.B, self.S, self.H, self.Hkv, self.d, self.causal, self.use_bias = B, S, H, Hkv, d, causal, use_bias
        self.plant, self.layout, self.family = plant, layout, family
        self.scale = default_scale(d, use_bias)

    @property
    def key(self):
        return (self.B, self.S, self.H, self.Hkv, self.d, self.causal, self.use_bias)

    @property
    def id(self):
        return (f'{self.family}-{self.B}x{self.S}-h{self.H}kv{self.Hkv}d{self.d}' + ('-causal' if self.causal else '') + ('-bias' if self.use_bias else '')
                + (f'-{self.plant}' if self.causal else '') + f'-{self.layout}')

    @property
    def seed(self):
        return self.B * 1000003 + self.S * 1009 + self.H * 31 + self.Hkv * 7 + self.d + 2 * int(self.causal) + int(self.use_bias)

    def inputs(self, device='cpu'):
        q, k, v, bias, design, plant_key = ext_inputs(self.B, self.S, self.H, self.Hkv, self.d, self.causal, self.use_bias, self.scale, self.seed, self.plant)
        mv = lambda t: None if t is None else t.to(device)              # noqa: E731
        return mv(q), mv(k), mv(v), mv(bias), design, mv(plant_key)


TOY = [(4, 4, 64, False, True), (4, 4, 64, True, False), (8, 2, 128, True, False), (4, 4, 128, False, False)]
EDGE_S = [1, 17, 63, 64, 65, 127, 128, 129, 193, 257, 333]
T5_XXL, CLIP_L, QWEN25 = (64, 64, 64, False, True), (12, 12, 64, True, False), (28, 4, 128, True, False)


def _cases():
    out = []
    for n, S in enumerate(EDGE_S):                     # planted variant and layout alternate along the list: every config meets both of each
        for m, cfg in enumerate(TOY):
            out.append(Case(1, S, *cfg, plant='diag' if n % 2 == 0 else 'rand', layout='packed' if (n + m) % 2 == 0 else 'separate'))
    out.append(Case(1, 512, *T5_XXL, layout='packed', family='t5'))
    out.append(Case(1, 77, *CLIP_L, plant='diag', layout='packed', family='clip'))
    out.append(Case(1, 40, *QWEN25, plant='rand', layout='packed', family='qwen'))
    out.append(Case(1, 333, *QWEN25, plant='diag', layout='separate', family='qwen'))
    out.append(Case(1, 1058, *QWEN25, plant='rand', layout='packed', family='qwen'))
    for n, (B, S) in enumerate([(2, 65), (3, 65), (2, 200), (3, 200)]):
        out.append(Case(B, S, 8, 2, 128, True, False, plant='diag', layout='packed' if n % 2 else 'separate', family='batch'))
        out.append(Case(B, S, 4, 4, 64, False, True, layout='separate' if n % 2 else 'packed', family='batch'))
    return out


CASES = _cases()


def find_case(B, S, cfg):
    hit = [c for c in CASES if c.key == (B, S) + tuple(cfg)]
    assert len(hit) == 1, (B, S, cfg)
    return hit[0]


# ---- teeth --------------------------------------------------------------------------------------------------------------------------------------------
# Per mutation, the cases that carry it and (teeth_targets) the rows it is held on: the rows where the feature decides the output.  On at least TEETH_SHARE of
# them the mutated and the true reference must differ by more than twice the tolerance (test_attention_ext_ref_cpu.py, without a device); the kernel's output
# must then be rejected by the mutated reference on every such row (test_hip_attention_ext_fp64.py).  Why these rows -- shares found on the CPU, per design
# 0 / 1 / 2 / 3 over ALL rows of the head, are in the docstring of test_attention_ext_ref_cpu.py:
#   causal_ge   planted heads, plant 'diag', rows i >= 1: the removed diagonal key carries the row (row 0 has no other key to fall back on in any model).
#   tile_short  planted heads, plant 'diag', the rows of each 128-query block that have keys in its last visited tile (i >= 64 t): their planted key is lost.
#               A plant at a random j <= i sits in that tile for only a part of the rows, and a positive-V row that loses 1 of 65 keys moves by less than 2 tol.
#   bias_shift  the heads of designs 0, 2, 3, all rows: every weight moves by exp(N(0, 2)).  NOT the planted heads the issue names: a planted key holds
#               1 - 1e-6 of its row whatever the table says, so no bias error can move such a row (0.06 .. 0.19 of them separate, by the unplanted tail).
#   kv_mod      planted heads whose two mappings differ (h % Hkv != h // group; where they agree the mutation is the identity), all rows.
#   drop_last   not causal: designs 2 (the last key is the largest weight) and 3 (zero-mean V: |O| ~ 1 / sqrt(S), a key is visible up to S ~ 300), all rows, and
#               the one planted row whose planted key is the last.  Causal: row S - 1 of designs 1 ('diag'), 2, 3.  NOT the positive-V heads the issue names:
#               dropping 1 of S keys moves a mean of V in [1, 2.5] by ~0.9 / S against 2 tol = 0.026: 0.53 of the rows at S = 17, 0.08 .. 0.14 at S = 65.
#   scale_128   designs 2 and 3, rows i >= 1 (row 0 of a causal head has one key: any scale gives O = v_0).  NOT all rows as the issue names: a planted row
#               keeps its key at 14 nats as at 20 (0.2 .. 0.6 separate), and a positive-V row is a mean of V under either scale (0.5 .. 0.98).
#   vt_batch0   planted heads, the rows of batch entries b > 0 (batch 0 reads its own V in either model).
TEETH = {
    'causal_ge': [(1, 65, TOY[1]), (1, 193, TOY[2]), (1, 77, CLIP_L), (2, 65, TOY[2])],
    'tile_short': [(1, 65, TOY[2]), (1, 128, TOY[1]), (1, 193, TOY[2]), (1, 333, TOY[1])],
    'bias_shift': [(1, 17, TOY[0]), (1, 65, TOY[0]), (1, 193, TOY[0]), (2, 65, TOY[0])],
    'kv_mod': [(1, 65, TOY[2]), (1, 193, TOY[2]), (3, 65, TOY[2])],
    'drop_last': [(1, 17, TOY[0]), (1, 65, TOY[0]), (1, 17, TOY[3]), (1, 65, TOY[3]), (1, 65, TOY[1])],
    'scale_128': [(1, 65, TOY[1]), (1, 193, TOY[1]), (1, 77, CLIP_L)],
    'vt_batch0': [(2, 65, TOY[2]), (3, 65, TOY[2]), (2, 65, TOY[0]), (3, 200, TOY[0])],
}
TEETH_SHARE = 0.9


def mutations_of(case):
    return [m for m in MUTATIONS if case.key in [(B, S) + tuple(cfg) for B, S, cfg in TEETH[m]]]


def teeth_targets(case, mutate, design, plant_key):
    """[B, S, H] bool (on plant_key's device): the rows `mutate` is held on at `case` (see above)."""
    B, S, H, Hkv = case.B, case.S, case.H, case.Hkv
    dev = plant_key.device
    planted = plant_key >= 0
    group = H // Hkv
    i = torch.arange(S, device=dev)[None, :, None]
    heads = lambda *ds: torch.tensor([int(design[h]) in ds for h in range(H)], device=dev)[None, None, :]       # noqa: E731
    every = torch.ones(B, S, H, dtype=torch.bool, device=dev)
    if mutate == 'causal_ge':
        assert case.causal and case.plant == 'diag'
        return planted & (i >= 1)
    if mutate == 'tile_short':
        assert case.causal and case.plant == 'diag'
        last = torch.clamp(2 * (i // QB) + 2, max=-(-S // KVB)) - 1
        return planted & (i >= KVB * last) & (last > 0)
    if mutate == 'bias_shift':
        return every & heads(0, 2, 3)
    if mutate == 'kv_mod':
        differ = torch.tensor([h % Hkv != h // group for h in range(H)], device=dev)[None, None, :]
        return planted & differ
    if mutate == 'drop_last':
        if case.causal:
            return every & heads(1, 2, 3) & (i == S - 1) & (planted | heads(2, 3))
        return (every & heads(2, 3)) | (plant_key == S - 1)
    if mutate == 'scale_128':
        return every & heads(2, 3) & (i >= 1)
    if mutate == 'vt_batch0':
        b = torch.arange(B, device=dev)[:, None, None]
        return planted & (b > 0)
    raise ValueError(mutate)
