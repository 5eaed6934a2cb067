"""Inputs shared by the attention parity tests (test_hip_attention_fp64.py, test_hip_attention_bwd_fp64.py, test_attention_bwd_ref_cpu.py): the four q / k / v
head designs, the two dO designs and the case table of the backward tests."""
import torch


def head_design_inputs(B, S, H, seed, device='cuda'):
    """q, k, v [B, S, H, 128] bf16 with head h of design h % 4 (0 positive-mean V, 1 a planted dominant key per query at a permuted position,
    2 scores growing tile after tile, 3 plain 0.6-scaled heads: see test_hip_attention_fp64.py)."""
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=device)         # noqa: E731
    q, k, v = rn(B, S, H, 128), rn(B, S, H, 128), rn(B, S, H, 128)
    for h in range(H):
        d = h % 4
        if d == 0:
            v[:, :, h] = v[:, :, h].abs() * 0.5 + 1.0
        elif d == 1:
            for b in range(B):
                pi = torch.randperm(S, generator=g, device=device)
                k[b, pi, h] = q[b, :, h] * 1.77                     # score of the planted key ~ 20 nats, the others ~ N(0, 1.8^2)
        elif d == 2:
            base = rn(128)
            base = base / base.norm()
            q[:, :, h] += 6.0 * base
            k[:, :, h] += (torch.arange(S, device=device).float() / S * 60.0)[None, :, None] * base
        else:
            q[:, :, h] *= 0.6
            k[:, :, h] *= 0.6
    return q.bfloat16(), k.bfloat16(), v.bfloat16()


def make_dout(B, S, H, design, seed, device):
    """dO [B, S, H, 128] bf16.  design 0: randn;  1: 0.5 randn + 1 (non-zero mean: delta is large against the spread of dP)."""
    g = torch.Generator(device=device).manual_seed(seed + 977)
    do = torch.randn(B, S, H, 128, generator=g, device=device)
    if design == 1:
        do = 0.5 * do + 1.0
    return do.bfloat16()



# ---- the cases of test_hip_attention_bwd_fp64.py, shared with the CPU test of the teeth criterion ------------------------------------------------------
# (B, S, H, dO design).  Every shape has the four q / k / v head designs (H >= 4); the dO designs alternate, so every head design meets both.
CASES = [(1, 37, 4, 0), (2, 64, 4, 1), (1, 65, 4, 0), (1, 128, 4, 1), (1, 191, 9, 0), (2, 225, 4, 1), (1, 257, 4, 0), (1, 576, 8, 1), (2, 1101, 9, 0)]
# The teeth, per output.  A dropped key or query takes about 1 / S of a dQ or dK row while the bound does not shrink with S: at (1, 191, 9) only 0.73 of the
# random heads' dQ rows and 0.75 of their dK rows separate the two references, so the dQ and the dK teeth sit at the two ragged shapes that meet the share,
# S = 65 and S = 37.  dV (no 1 / sqrt(d), no dP - delta factor) separates on 0.99 of the rows at S = 191 and keeps the two shapes the issue names.
TEETH_DQ = [(1, 65, 4, 0), (1, 37, 4, 0)]
TEETH_DK = [(1, 65, 4, 0), (1, 37, 4, 0)]
TEETH_DV = [(1, 65, 4, 0), (1, 191, 9, 0)]
TEETH_ALL = sorted(set(TEETH_DQ) | set(TEETH_DK) | set(TEETH_DV))
TEETH_SHARE = 0.9


def case_inputs(B, S, H, design, device):
    """q, k, v of the four head designs and dO of `design`, seeded by the shape.  Drawn by the CPU generator whatever the device, so that the CPU test of the
    teeth criterion sees the numbers the GPU test runs."""
    seed = B * 100000 + S * 10 + H
    return tuple(t.to(device) for t in head_design_inputs(B, S, H, seed, device='cpu') + (make_dout(B, S, H, design, seed, 'cpu'),))
