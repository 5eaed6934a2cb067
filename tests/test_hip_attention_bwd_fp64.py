"""fp64 parity of the joint attention backward, per element, for every kernel generation: 3 = the generated dK / dV and dQ streams in one launch (default),
4 = the same as two launches, 1 = generated dK / dV + round-4 dQ, 2 = the round-4 kernels (afx_attn_bwd3.hip + gen/*.inc, afx_attn_bwd.hip).

Reference and bound: attention_bwd_ref.py (the derivation is in its docstring; no constant is fitted to a kernel's output).  Each of dQ, dK, dV is held to
|out - ref| <= ulp_bf16(ref) + bound per element.  q, k, v are the forward test's four head designs (positive-mean V, a planted dominant key at a permuted
position, scores growing tile after tile, plain 0.6-scaled heads); dO is randn or 0.5 randn + 1 (delta large against the spread of dP), alternating by shape,
so that every head design meets both.  o and lse come from attention_fwd_lse_2d, as in the training trunk, and lse is held to the log2 convention the
reference assumes: sum_k exp2(s c - lse) = 1 within the forward test's E_lse (KV-split form: the default forward may split).

Shapes (B, S, H), NH = S_pad / 32 -- the generated loop is unrolled 8 times and leaves behind body3 / body5 / body7 / body1 as NH % 8 = 4 / 6 / 0 / 2:
  (1, 37, 4), (2, 64, 4)   S <= 64: the round-4 kernels whatever the generation (run once)
  (1, 65, 4)               NH = 4, one real row in the last tile: the dQ stream's cold key mask, the clamped rA / rB rows
  (1, 128, 4)              NH = 4, no tail
  (1, 191, 9)              NH = 6: the exit behind body5; S % 64 = 63; two head groups per XCD with work-groups that return at once
  (2, 225, 4)              NH = 8, S % 64 = 33; unpadded batch rows (b S) against the padded stats array; gradient row strides 4 mod 8
  (1, 257, 4)              NH = 10, S % 64 = 1; three stationary row blocks
  (1, 576, 8)              NH = 18, full tiles
  (2, 1101, 9)             NH = 36: several trips round the loop; per_xcd = 36, a non-trivial interleave of the fused launch's order search

Layout, as the trunk calls attention_bwd_2d: q | k | v column slices of one [rows, 3 H 128 + 64] stash, dO a slice of a wider buffer, dV the middle third of a
[rows, 3 H 128] buffer, dQ and dK buffers of their own; every gradient buffer lies inside a larger one filled with a sentinel (guard rows above and below,
guard columns left and right) that must come back unchanged outside the gradient.  q, k, v, dO are 16-byte aligned with row strides of 0 mod 8 (asserted:
otherwise the launcher silently takes the round-4 kernels).  The inputs are bit-equal after the calls; a second call gives bit-equal gradients.

Teeth (mutated references, no kernel variants; the criterion itself -- the two references lie further apart than twice the tolerance on >= 90 % of the random
heads' rows -- is held on the CPU by test_attention_bwd_ref_cpu.py on these same inputs, shares there), for each output on its own: the kernels' dQ must FAIL the
reference without the last real key, their dK and their dV the reference without the last real query, on at least that share of rows -- dQ and dK at (1, 65, 4)
and (1, 37, 4), dV at (1, 65, 4) and (1, 191, 9).  (1, 191, 9) cannot carry the dQ and dK teeth: one key or query is 1 / 191 of such a row and only 0.73 / 0.75
of the rows separate the references.

Worst err / tol measured on an MI355X (printed per output, shape and generation; the four generations agree to these digits, the bf16 roundings of P and dS
carry the error): dQ 0.835 at (2, 64, 4), dK 0.828 at (1, 191, 9), dV 0.804 at (2, 1101, 9).  The kernels failed the mutated references on 0.938 - 1.000 of the rows.
"""
import pytest
import torch
from attention_bwd_ref import attention_bwd_reference, row_share, teeth, tolerance
from attention_inputs import CASES, TEETH_ALL, TEETH_DK, TEETH_DQ, TEETH_DV, TEETH_SHARE, case_inputs
from bf16_parity import check_bf16_bound
from test_hip_attention_fp64 import _reference as _forward_reference

pytestmark = pytest.mark.gpu

SENT = -7.75
IMPLS = (3, 4, 1, 2)
ODD_STRIDE = (2, 225, 4)            # the shape whose gradient buffers get a row stride of 4 mod 8


@pytest.fixture(scope='module')
def ops():
    from arcflow_amd import ops as _ops
    return _ops


def _guarded(rows, cols, pad):
    """A sentinel-filled [rows + 16, cols + 128 + pad] buffer and its [rows, cols] middle (8 guard rows above and below, 64 guard columns left, 64 + pad right)."""
    buf = torch.full((rows + 16, cols + 128 + pad), SENT, dtype=torch.bfloat16, device='cuda')
    return buf, buf[8:8 + rows, 64:64 + cols]


class _Case:
    """One shape: the inputs in the trunk's layout, o / lse of the forward kernel, the fp64 reference (computed once, never written again)."""

    def __init__(self, ops, B, S, H, design):
        self.B, self.S, self.H = B, S, H
        R, D = B * S, H * 128
        self.q4, self.k4, self.v4, self.do4 = case_inputs(B, S, H, design, 'cuda')
        self.stash = torch.zeros(R, 3 * D + 64, dtype=torch.bfloat16, device='cuda')
        self.q, self.k, self.v = self.stash[:, :D], self.stash[:, D:2 * D], self.stash[:, 2 * D:3 * D]
        for dst, src in ((self.q, self.q4), (self.k, self.k4), (self.v, self.v4)):
            dst.copy_(src.reshape(R, D))
        self.dobuf = torch.zeros(R, D + 8, dtype=torch.bfloat16, device='cuda')
        self.do = self.dobuf[:, :D]
        self.do.copy_(self.do4.reshape(R, D))
        for t in (self.q, self.k, self.v, self.do):
            assert t.data_ptr() % 16 == 0 and t.stride(0) % 8 == 0 and t.stride(1) == 1      # else the launcher takes the round-4 kernels
        self.o = torch.empty(R, D, dtype=torch.bfloat16, device='cuda')
        self.lse = ops.attention_fwd_lse_2d(self.q, self.k, self.v, self.o, B, S, H)
        torch.cuda.synchronize()
        self.o4 = self.o.view(B, S, H, 128)
        self.kept = [t.clone() for t in (self.stash, self.dobuf, self.o, self.lse)]
        self.ref = attention_bwd_reference(self.q4, self.k4, self.v4, self.o4, self.do4, self.lse)
        self.out = {}

    def inputs_untouched(self):
        return all(torch.equal(a, b) for a, b in zip((self.stash, self.dobuf, self.o, self.lse), self.kept))

    def run(self, ops, impl):
        """dq, dk, dv [rows, H 128] of generation impl, called twice into fresh guarded buffers (cached per impl)."""
        if impl in self.out:
            return self.out[impl]
        R, D = self.B * self.S, self.H * 128
        pad = 4 if (self.B, self.S, self.H) == ODD_STRIDE else 0
        res = []
        ops.set_attn_bwd_impl(impl)
        try:
            for _ in range(2):
                (bq, dq), (bk, dk), (bv, dqkv) = _guarded(R, D, pad), _guarded(R, D, pad), _guarded(R, 3 * D, pad)
                assert dq.stride(0) % 8 == pad and dqkv.stride(0) % 8 == pad
                ops.attention_bwd_2d(self.q, self.k, self.v, self.o, self.do, self.lse, dq, dk, dqkv[:, D:2 * D], self.B, self.S, self.H)
                torch.cuda.synchronize()
                for name, buf, c0, n in (('dq', bq, 64, D), ('dk', bk, 64, D), ('dv', bv, 64 + D, D)):
                    mask = torch.ones(buf.shape, dtype=torch.bool, device='cuda')
                    mask[8:8 + R, c0:c0 + n] = False
                    assert bool((buf[mask] == SENT).all()), f'impl {impl}: a {name} write landed outside the gradient'
                res.append((dq, dk, dqkv[:, D:2 * D]))
        finally:
            ops.set_attn_bwd_impl(3)
        for name, a, b in zip(('dq', 'dk', 'dv'), *res):
            assert torch.equal(a, b), f'impl {impl}: {name} differs between two calls'
        assert self.inputs_untouched(), f'impl {impl}: an input was written'
        self.out[impl] = res[0]
        return res[0]


@pytest.fixture(scope='module')
def case(ops):
    """The cases of this module, each built once and shared by its tests; released with the module."""
    made = {}

    def get(B, S, H, design):
        if (B, S, H, design) not in made:
            made[B, S, H, design] = _Case(ops, B, S, H, design)
        return made[B, S, H, design]
    yield get
    made.clear()


def _impls(S):
    return IMPLS if S > 64 else (3,)


def _ids(cases):
    return [f'{b}x{s}x{h}' for b, s, h, _ in cases]


@pytest.mark.parametrize('B,S,H,design', CASES, ids=_ids(CASES))
def test_attention_backward_vs_fp64(ops, case, B, S, H, design):
    """dQ, dK, dV of every generation per element against the fp64 reference; guard bands, untouched inputs and call-to-call bit equality on the way."""
    c = case(B, S, H, design)
    # the convention the reference assumes: lse is the log2-domain log-sum-exp of s c, to the forward's own bound
    _, _, L, LB = _forward_reference(c.q4, c.k4, c.v4, split=True)
    off = (c.ref['rowsum'] - 1).abs()
    margin = torch.exp2(LB) - 1
    assert bool((off <= margin).all()), f'B={B} S={S} H={H}: sum_k exp2(s c - lse) off 1 by {off.max().item():.3e} (margin {margin.max().item():.3e})'
    for impl in _impls(S):
        got = c.run(ops, impl)
        worst = {}
        for name, out in zip(('dq', 'dk', 'dv'), got):
            assert bool(torch.isfinite(out.float()).all()), (impl, name)
            worst[name] = check_bf16_bound(out, c.ref[name], c.ref['b' + name[1]], f'B={B} S={S} H={H} impl={impl}: {name}')
        print(f'attention bwd B={B} S={S} H={H} impl={impl}: worst err / tol  ' + '  '.join(f'{n} {w:.3f}' for n, w in worst.items()))


def _fails(out, mut, n):
    return (out.double() - mut['d' + n]).abs() > tolerance(mut['d' + n], mut['b' + n])


@pytest.mark.parametrize('B,S,H,design', TEETH_ALL, ids=_ids(TEETH_ALL))
def test_attention_backward_bounds_catch_a_dropped_key_or_query(ops, case, B, S, H, design):
    """Teeth, per output: the kernels' dQ fails the reference without the last real key, their dK and their dV the reference without the last real query, each on
    >= 90 % of the random heads' rows, at the shapes where the references themselves lie that far apart (attention_inputs.TEETH_*; that criterion involves no
    kernel and is held by test_attention_bwd_ref_cpu.py).  In the planted-key heads the dropped query empties the dV row of its key: the kernels' row must miss
    the mutated reference there."""
    c = case(B, S, H, design)
    true, mk, mq, _, planted = teeth(c.q4, c.k4, c.v4, c.o4, c.do4, c.lse, true=c.ref)
    rnd = [h for h in range(H) if h % 4 == 3]
    plant = [h for h in range(H) if h % 4 == 1]
    on = {n: (B, S, H, design) in where for n, where in (('q', TEETH_DQ), ('k', TEETH_DK), ('v', TEETH_DV))}
    if on['v']:
        assert float(planted.min()) > 0.5, planted
        moved = (true['dv'] - mq['dv']).abs().view(B * S, H, 128).amax(-1)
        krow = [[int(moved[b * S:(b + 1) * S, h].argmax()) + b * S for h in plant] for b in range(B)]       # the dropped query's planted key
    for impl in _impls(S):
        got = dict(zip('qkv', c.run(ops, impl)))
        what = f'B={B} S={S} H={H} impl={impl}'
        for n, mut, dropped in (('q', mk, 'key'), ('k', mq, 'query'), ('v', mq, 'query')):
            if not on[n]:
                continue
            fails = _fails(got[n], mut, n)
            caught = row_share(fails, B, S, H, rnd)
            print(f'attention bwd teeth {what}: d{n.upper()} fails the dropped-{dropped} reference on {caught:.3f} of the random heads\' rows')
            assert caught >= TEETH_SHARE, f'{what}: the d{n.upper()} bound misses a dropped {dropped} on {1 - caught:.3f} of the random rows'
            if n == 'v':
                for b in range(B):
                    for i, h in enumerate(plant):
                        gross = fails.reshape(B * S, H, 128)[krow[b][i], h].double().mean().item()
                        assert gross >= TEETH_SHARE, f'{what}: dV of the planted key of head {h} satisfies the dropped-query reference in {1 - gross:.3f} of its elements'
