"""fp64 parity of the forward's GEMMs: bf16 ``ops.linear`` with every epilogue in every kernel mode, and the fp8 GEMMs (row scales, block scales,
the block-scaled producer epilogue) on both tile shapes of the one-wave-per-SIMD fp8 kernel and on the 8-phase kernel.

Every case compares with plain fp64 torch built from the same bf16 / e4m3 inputs, on the device (tests/bf16_parity.py):
  * bf16 outputs: within one bf16 ulp of the fp64 value plus a floor F, and >= 99 % of the elements equal to the fp64 value rounded to nearest
    even.  The ulp covers the output's own rounding; F bounds the fp32 arithmetic in front of it.
  * F of the product y = A W^T + b: depth * 2^-24 * (|A| |W|^T + |b|) -- recursive summation, depth = one rounding per MFMA K-step into the
    accumulator + a serial chain over one instruction's products + 1 for the bias (bf16: K / 32 + 33, v_mfma_f32_16x16x32_bf16; fp8:
    K / 128 + 129, v_mfma_f32_16x16x128_f8f6f4).  e4m3 codes times power-of-two or fp32 scales multiply exactly in fp64, so the fp8 reference is
    the exact product of the dequantised operands; the row-scaled epilogue's two multiplies (a_scale * w_scale, then the accumulator) add 2 u |y|
    in the same units.
  * pre operand (bf16, added in fp32): + 2^-24 |y + pre|.
  * gelu (tanh form): F carried through the derivative, (|gelu'(y64)| + F) F (|gelu''| <= 0.8 < 1), + 8 u |y| for the fp32 evaluation (exp2 +
    reciprocal: a few ulp).
  * gate_res: out = r + g y; F scaled by |g|, + 2 u (|g y| + |r|) for the fp32 multiply and the residual add.
  * E8M0 bytes of the producer epilogue: ceil(log2(blockmax64 / 448)), except where [blockmax64 -+ (F_max + 2 u blockmax64)] / 448 crosses a power
    of two (mx_exp multiplies by the fp32 1/448: + 2 u); the byte then lies between the two candidates.  e4m3 codes: RNE(y64 / 2^e) with the
    kernel's own e (the division is exact), except where (y64 -+ F) / 2^e straddles an e4m3 rounding midpoint; the code then lies between the two.
    The exempt share is printed and asserted below 2 % (bytes) / 5 % (codes).
  * fp8 outputs: >= 97 % (not 99 %) of the bf16 elements equal RNE(y64).  The share these cases give is 98.7 - 99.1 %, at every K from 1024 to 15360,
    on the 8-phase and the one-wave-per-SIMD fp8 kernels and with row or block scales alike (print it with -s), while the bf16 GEMMs reach 99 %.
    A 1.2 % miss rate is an RMS relative error near 2e-5, far above fp32 accumulation.  HYPOTHESIS, not shown here: the fp8 matrix instruction
    keeps less than a full fp32 sum inside one 128-deep step.  For these instructions the floor therefore does not follow from the fp32 model
    above; it holds for every element as measured, with the margin the serial-chain depth leaves.
Teeth: the per-element bound alone (no equal-share test) passes against the reference and fails once one K column (k = K - 1) is left out of
it, for every case.
Every output is a view of a larger buffer whose guard bands hold a sentinel that must survive (bf16 outputs: a bf16-exact value; fp8 bytes
and scale bytes: 0xA5).
"""
import math

import pytest
import torch
from bf16_parity import U32, check_bf16, check_f32, gelu64, proj64

pytestmark = pytest.mark.gpu

SENT = -7.75
GEMM_MODES = [(3, 0), (3, 1), (3, 2), (3, 3), (3, 4), (3, 5), (3, 6), (2, 0)]      # as test_hip_kernels.py: auto, six forced v3 tiles, 8-phase


@pytest.fixture(scope='module')
def ops():
    from arcflow_amd import ops as _ops
    return _ops


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def _guarded(M, N, dtype=torch.bfloat16):
    buf = torch.full((M + 16, N + 128), SENT, dtype=dtype, device='cuda')
    return buf, buf[8:8 + M, 64:64 + N]


def _unchanged(buf, M, N, what):
    mask = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    mask[8:8 + M, 64:64 + N] = False
    assert bool((buf[mask] == SENT).all()), f'{what}: a write landed in the guard band'


def _head_n():
    """N of the forward's head launch, as the engine reports it (afx_head_width)."""
    from arcflow_amd import MMDiTEngine
    return MMDiTEngine('flux', 1, 1).head_n


# The text length is an input of the forward (encoder_hidden_states.shape[1]), not a property of the engine: these are the flagship workload's
# (bench.py: FLUX 4096 image + 512 T5 tokens, Qwen-Image 4096 + 128).
T_FLUX, T_QWEN = 512, 128

# (id, rows, K, N, epilogue, options)   epilogue: none | gelu (gelu_col0) | gelu_all | gate_res (rows_per_batch, batch)
BF16_CASES = [
    ('flux-qkv', 4096 + T_FLUX, 3072, 9216, 'none', {}),
    ('flux-mlp1', 4096 + T_FLUX, 3072, 12288, 'gelu_all', {}),
    ('flux-single-fused', 4096 + T_FLUX, 3072, 21504, 'gelu', {'col0': 9216}),
    ('flux-out-proj', 4096 + T_FLUX, 3072, 3072, 'gate_res', {}),
    ('flux-mlp2', 4096 + T_FLUX, 12288, 3072, 'gate_res', {}),
    ('flux-single-out', 4096 + T_FLUX, 15360, 3072, 'gate_res', {}),
    ('t5-ctx-embed', T_FLUX, 4096, 3072, 'none', {}),
    ('x-embed', 4096, 64, 3072, 'none', {}),
    ('head', 4096, 3072, 'head_n', 'none', {}),          # N read from the engine when the test runs
    ('qwen-qkv', 4096 + T_QWEN, 3072, 9216, 'none', {}),
    ('qwen-ragged-mlp1', 4173, 3072, 12288, 'gelu_all', {}),
    ('qwen-txt-in', T_QWEN, 3584, 3072, 'none', {}),
    ('b2-gate-4608', 2 * 4608, 3072, 3072, 'gate_res', {'rpb': 4608}),
    ('b2-gate-4173', 2 * 4173, 3072, 3072, 'gate_res', {'rpb': 4173}),
    ('no-bias', 4608, 3072, 3072, 'none', {'nobias': True}),
    ('strided-a', 1000, 3072, 1152, 'none', {'lda': 3072 + 192}),
    ('gelu-col1000', 1000, 1024, 3072, 'gelu', {'col0': 1000}),
    ('pre', 1000, 3072, 3072, 'gelu', {'col0': 1536, 'pre': True}),
]


def _dgelu64(x):
    k = math.sqrt(2 / math.pi)
    t = torch.tanh(k * (x + 0.044715 * x ** 3))
    return 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * k * (1 + 3 * 0.044715 * x * x)


def _teeth(out, ref, ref_drop, floor, what):
    """The per-element bound alone (min_equal = 0) holds against ref and fails against ref_drop (one K column left out)."""
    check_bf16(out, ref, floor=floor, min_equal=0.0, what=what)
    with pytest.raises(AssertionError, match='beyond one bf16 ulp'):
        check_bf16(out, ref_drop, floor=floor, min_equal=0.0, what=f'{what}: one K column dropped')


def _epi_ref(y, e, epi, col0, gate_rows, r):
    """fp64 value and floor of the epilogue applied to (y, its floor e)."""
    if epi in ('gelu', 'gelu_all'):
        c = 0 if epi == 'gelu_all' else col0
        out, fl = y.clone(), e.clone()
        out[:, c:] = gelu64(y[:, c:])
        fl[:, c:] = (_dgelu64(y[:, c:]).abs() + e[:, c:]) * e[:, c:] + 8 * U32 * y[:, c:].abs()
        return out, fl
    if epi == 'gate_res':
        gy = gate_rows * y
        return r + gy, gate_rows.abs() * e + 2 * U32 * (gy.abs() + r.abs())
    return y, e


@pytest.mark.parametrize('cid,M,K,N,epi,opt', BF16_CASES, ids=[c[0] for c in BF16_CASES])
def test_linear_vs_fp64_every_mode(ops, cid, M, K, N, epi, opt):
    """One forward launch shape in all eight GEMM modes against one fp64 reference; then the teeth check on the last mode's output."""
    if N == 'head_n':
        N = _head_n()
    g = _gen(M * 7 + K * 3 + N)
    lda = opt.get('lda', K)
    a = (torch.randn(M, lda, generator=g, device='cuda') * 1.2 + 0.1).bfloat16()[:, lda - K:]
    w = (torch.randn(N, K, generator=g, device='cuda') * K ** -0.5).bfloat16()
    b = None if opt.get('nobias') else (torch.randn(N, generator=g, device='cuda') * 0.2).bfloat16()
    pre = (torch.randn(M, N, generator=g, device='cuda') * 0.3).bfloat16() if opt.get('pre') else None
    rpb = opt.get('rpb', M)
    nb = M // rpb
    gate = torch.randn(nb, N, generator=g, device='cuda') if epi == 'gate_res' else None
    r0 = torch.randn(M, N, generator=g, device='cuda').bfloat16() if epi == 'gate_res' else None
    y, e = proj64(a, w, b)
    if pre is not None:
        y += pre.double()
        e += U32 * y.abs()
    gate_rows = gate.double().repeat_interleave(rpb, 0) if gate is not None else None
    r = r0.double() if r0 is not None else None
    col0 = opt.get('col0', 0)
    ref, fl = _epi_ref(y, e, epi, col0, gate_rows, r)
    buf, out = _guarded(M, N)
    kw = dict(epilogue={'none': 'none', 'gelu': 'gelu', 'gelu_all': 'gelu', 'gate_res': 'gate_res'}[epi], gelu_col0=col0, pre=pre)
    if epi == 'gate_res':
        kw.update(gate=gate, residual=out, rows_per_batch=rpb)
    try:
        for mode in GEMM_MODES:
            if r0 is not None:
                out.copy_(r0)                         # in place on the residual, as the forward runs it
            ops.set_gemm_mode(*mode)
            got = ops.linear(a, w, b, out=out, **kw)
            torch.cuda.synchronize()
            assert got.data_ptr() == out.data_ptr()
            what = f'{cid} {M}x{N}x{K} {epi} mode={mode}'
            _unchanged(buf, M, N, what)
            check_bf16(out, ref, floor=fl, what=what)
    finally:
        ops.set_gemm_mode(3, 0)
    # teeth: the per-element bound against the reference without the last K column fails
    yd = y - a[:, K - 1].double()[:, None] * w[:, K - 1].double()[None, :]
    _teeth(out, ref, _epi_ref(yd, e, epi, col0, gate_rows, r)[0], fl, cid)


# The two linear entry points no Python wrapper calls (ops.linear goes through afx_linear_bf16_pre, ops.linear_tn_f32out through the _ws entry),
# straight through the C ABI at the smallest shape that spans a tile edge and leaves a ragged row tile.
EDGE_M, EDGE_N, EDGE_K = 264, 136, 128


def test_afx_linear_bf16_entry_vs_fp64(ops):
    """afx_linear_bf16 itself (bias, no epilogue) in all eight GEMM modes: the bound and the equal share of the cases above, then the teeth check."""
    from arcflow_amd import _lib
    lib = _lib.load()
    M, N, K = EDGE_M, EDGE_N, EDGE_K
    g = _gen(M * 7 + K * 3 + N)
    a = (torch.randn(M, K, generator=g, device='cuda') * 1.2 + 0.1).bfloat16()
    w = (torch.randn(N, K, generator=g, device='cuda') * K ** -0.5).bfloat16()
    b = (torch.randn(N, generator=g, device='cuda') * 0.2).bfloat16()
    ref, fl = proj64(a, w, b)
    buf, out = _guarded(M, N)
    try:
        for mode in GEMM_MODES:
            ops.set_gemm_mode(*mode)
            out.fill_(SENT)
            _lib.check(lib.afx_linear_bf16(ops._p(a), a.stride(0), ops._p(w), w.stride(0), ops._p(b), ops._p(out), out.stride(0), M, N, K, 0, 0, None, 0, 1,
                                           None, 0, ops._s()))
            torch.cuda.synchronize()
            what = f'afx_linear_bf16 {M}x{N}x{K} mode={mode}'
            _unchanged(buf, M, N, what)
            check_bf16(out, ref, floor=fl, what=what)
    finally:
        ops.set_gemm_mode(3, 0)
    _teeth(out, ref, ref - a[:, K - 1].double()[:, None] * w[:, K - 1].double()[None, :], fl, 'afx_linear_bf16')


def test_afx_linear_tn_f32out_entry_vs_fp64(ops):
    """afx_linear_tn_f32out itself (no workspace: one work-group per tile): C [N, K] = X^T Y over M tokens, X [M, N], Y [M, K].  The output is fp32, so the
    bound is the product's floor F of the cases above (proj64 over the M-deep sum) plus the fp32 rounding of the stored value, 2^-24 |y|, where
    those cases allow one bf16 ulp; then the accumulate mode with the add's rounding on top, and the bound against a reference without the last
    token fails."""
    from arcflow_amd import _lib
    lib = _lib.load()
    M, N1, N2 = EDGE_M, EDGE_N, EDGE_K
    g = _gen(M * 7 + N2 * 3 + N1)
    x = (torch.randn(M, N1 + 64, generator=g, device='cuda') * 1.2 + 0.1).bfloat16()[:, 32:32 + N1]      # views: row stride != width
    y = (torch.randn(M, N2 + 8, generator=g, device='cuda') * M ** -0.5).bfloat16()[:, 8:8 + N2]
    ref, fl = proj64(x.T, y.T, None)
    buf = torch.full((N1 + 16, N2 + 128), SENT, dtype=torch.float32, device='cuda')
    out = buf[8:8 + N1, 64:64 + N2]

    def run(accumulate):
        _lib.check(lib.afx_linear_tn_f32out(ops._p(x), x.stride(0), ops._p(y), y.stride(0), ops._p(out), out.stride(0), M, N1, N2, accumulate, ops._s()))
        torch.cuda.synchronize()
        _unchanged(buf, N1, N2, f'afx_linear_tn_f32out accumulate={accumulate}')
    run(0)
    bound = fl + U32 * ref.abs()
    check_f32(out, ref, bound, what='afx_linear_tn_f32out')
    with pytest.raises(AssertionError, match='beyond the bound'):
        check_f32(out, ref - x[M - 1].double()[:, None] * y[M - 1].double()[None, :], bound, what='afx_linear_tn_f32out: last token dropped')
    c0 = torch.randn(N1, N2, generator=g, device='cuda')
    out.copy_(c0)
    run(1)
    check_f32(out, c0.double() + ref, bound + U32 * (c0.double() + ref).abs(), what='afx_linear_tn_f32out accumulate')


# ------------------------------------------------------------------------------------------------ fp8
def _e4m3(codes):
    return codes.view(torch.float8_e4m3fn).double()


def _fp8_operands(ops, M, N, K, g, mx):
    a = (torch.randn(M, K, generator=g, device='cuda') * 2.0)
    if mx:                                             # test_fp8_block_scaled_quant_and_linear's construction: outlier rows, a small block that matters
        a[::7, 5] = 2000.0
        a[:, 128:256] *= 1e-2
    a = a.bfloat16()
    w = torch.randn(N, K, generator=g, device='cuda') * K ** -0.5
    if mx:
        w[:, 128:256] *= 1e2
        w[:, 5] = 0
    w = w.bfloat16()
    wq, wsc = ops.quant_rows_fp8(w)
    wd = _e4m3(wq) * wsc.double()[:, None]
    if mx:
        aq, amx = ops.quant_rows_mx8(a)
        ad = (_e4m3(aq).view(M, K // 128, 128) * torch.exp2(amx.double() - 127)[..., None]).view(M, K)
        return (aq, amx), ad, (wq, wsc), wd
    aq, asc = ops.quant_rows_fp8(a)
    return (aq, asc), _e4m3(aq) * asc.double()[:, None], (wq, wsc), wd


# (M, N, K, kernels)   kernels: fp8 tile settings to force (1 = 256x256, 2 = 224x256) or 'v2' (a launch below half a round: the 8-phase fp8 kernel)
FP8_ROW_CASES = [(4608, 9216, 3072, (1, 2)), (4224, 3072, 3072, (1, 2)), (4173, 3072, 12288, (1, 2)), (4645, 3640, 1152, (1, 2)),
                 (300, 520, 1024, ('v2',))]
FP8_EQUAL = 0.97                   # share of fp8 GEMM outputs equal to RNE(y64) (module docstring)
FP8_MX_CASES = [(4224, 3072, 3072), (4608, 3072, 12288), (4173, 3072, 15360)]


def _fp8_check_all(ops, run, M, N, K, ad, wd, b, g, extra_scale, what):
    """run(epilogue, **kw) -> bf16 out; every epilogue against fp64; teeth on the plain one.  extra_scale: the epilogue's scale multiplies."""
    y, e = proj64(ad, wd, b, kstep=128)
    e += extra_scale * U32 * (ad.abs() @ wd.abs().T)
    gate = torch.randn(N, generator=g, device='cuda')
    r0 = torch.randn(M, N, generator=g, device='cuda').bfloat16()
    col0 = N // 2 - N // 2 % 128
    for epi in ('none', 'gelu', 'gate_res'):
        buf, out = _guarded(M, N)
        kw = dict(epilogue=epi, out=out)
        if epi == 'gelu':
            kw['gelu_col0'] = col0
        if epi == 'gate_res':
            out.copy_(r0)
            kw.update(gate=gate, residual=out)
        run(**kw)
        torch.cuda.synchronize()
        _unchanged(buf, M, N, f'{what} {epi}')
        ref, fl = _epi_ref(y, e, epi, col0, gate.double()[None, :].expand(M, N) if epi == 'gate_res' else None, r0.double())
        print(f'{what} {epi}: equal share {(out == ref.float().bfloat16()).double().mean().item():.4f}')
        check_bf16(out, ref, floor=fl, min_equal=FP8_EQUAL, what=f'{what} {epi}')
        if epi == 'none':
            plain = out.clone()
    _teeth(plain, y, y - ad[:, K - 1][:, None] * wd[:, K - 1][None, :], e, what)


@pytest.mark.parametrize('M,N,K,kernels', FP8_ROW_CASES)
def test_linear_fp8_row_scaled_vs_fp64(ops, M, N, K, kernels):
    """linear_fp8: a_scale[m] w_scale[n] (codes_a . codes_w) + bias with every epilogue, each forced fp8 tile shape -- 4645 x 3640 x 1152 has an odd
    number of K-tiles (9: the peeled tile) and ragged edges; 300 x 520 x 1024 runs the 8-phase fp8 kernel."""
    g = _gen(M + N + K)
    (aq, asc), ad, (wq, wsc), wd = _fp8_operands(ops, M, N, K, g, mx=False)
    b = (torch.randn(N, generator=g, device='cuda') * 0.2).bfloat16()
    try:
        for kern in kernels:
            assert ops.set_fp8_tile(kern if kern != 'v2' else 0) == (kern if kern != 'v2' else 0)
            run = lambda **kw: ops.linear_fp8(aq, asc, wq, wsc, b, **kw)       # noqa: E731
            _fp8_check_all(ops, run, M, N, K, ad, wd, b, g, 2, f'linear_fp8 {M}x{N}x{K} tile={kern}')
    finally:
        ops.set_fp8_tile(0)


@pytest.mark.parametrize('M,N,K', FP8_MX_CASES)
def test_linear_fp8_block_scaled_vs_fp64(ops, M, N, K):
    """linear_fp8_mx: block-scaled activations (E8M0 per row and 128 columns, applied by the MFMA: exact), row-scaled weights, every epilogue, both tiles."""
    g = _gen(M * 3 + K)
    (aq, amx), ad, (wq, wsc), wd = _fp8_operands(ops, M, N, K, g, mx=True)
    b = (torch.randn(N, generator=g, device='cuda') * 0.2).bfloat16()
    try:
        for kern in (1, 2):
            assert ops.set_fp8_tile(kern) == kern
            run = lambda **kw: ops.linear_fp8_mx(aq, amx, wq, wsc, b, **kw)     # noqa: E731
            _fp8_check_all(ops, run, M, N, K, ad, wd, b, g, 1, f'linear_fp8_mx {M}x{N}x{K} tile={kern}')
    finally:
        ops.set_fp8_tile(0)


def _e4m3_ord(codes):
    c = codes.long()
    mag = c & 0x7f
    return torch.where((c & 0x80) != 0, -mag, mag)


def _rne_e4m3_ord(x):
    return _e4m3_ord(x.clamp(-448, 448).float().to(torch.float8_e4m3fn).view(torch.uint8))


def _mx_exp64(x):
    """ceil(log2(x / 448)) + 127, clamped to [1, 254] as afx_common.h mx_exp."""
    return (torch.ceil(torch.log2(x.clamp_min(1e-300) / 448.0)) + 127).clamp(1, 254).long()


def check_mx8(q, mx, y, fl, what):
    """E8M0 bytes and e4m3 codes of a block-scaled output against fp64 y with floor fl (see the module docstring); returns the exempt counts."""
    M, n8 = y.shape
    blocks, fb = y.view(M, n8 // 128, 128), fl.view(M, n8 // 128, 128)
    bm = blocks.abs().amax(-1)
    slack = fb.amax(-1) + 2 * U32 * bm
    lo, hi, want = _mx_exp64((bm - slack).clamp_min(0)), _mx_exp64(bm + slack), _mx_exp64(bm)
    got = mx.long()
    assert bool(((got >= lo) & (got <= hi)).all()), f'{what}: an E8M0 byte outside its candidates'
    ex_b = lo != hi
    assert bool((got[~ex_b] == want[~ex_b]).all()), f'{what}: {int((got[~ex_b] != want[~ex_b]).sum())} E8M0 bytes off ceil(log2(max / 448))'
    sc = torch.exp2(got.double() - 127)[..., None]
    clo, chi = _rne_e4m3_ord((blocks - fb) / sc), _rne_e4m3_ord((blocks + fb) / sc)
    gq = _e4m3_ord(q).view(M, n8 // 128, 128)
    assert bool(((gq >= clo) & (gq <= chi)).all()), f'{what}: {int(((gq < clo) | (gq > chi)).sum())} e4m3 codes outside their candidates'
    ex_c = clo != chi
    assert bool((gq[~ex_c] == clo[~ex_c]).all()), f'{what}: {int((gq[~ex_c] != clo[~ex_c]).sum())} e4m3 codes off RNE(y / 2^e)'
    nb, nc = int(ex_b.sum()), int(ex_c.sum())
    print(f'{what}: exempt {nb} of {ex_b.numel()} scale bytes, {nc} of {ex_c.numel()} codes')
    assert nb <= 0.02 * ex_b.numel() and nc <= 0.05 * ex_c.numel(), f'{what}: too many exempt elements ({nb}, {nc})'


@pytest.mark.parametrize('M,N,K,col0,gelu', [(4608, 9216, 3072, 3072, True), (4224, 3072, 3072, 0, True), (4173, 1792, 3072, 768, False)])
def test_linear_fp8_to_mx8_vs_fp64(ops, M, N, K, col0, gelu):
    """The producer epilogue: bf16 head columns [0, col0) and block-scaled fp8 columns [col0, N) (gelu on the fp8 part), both fp8 tiles."""
    g = _gen(M + N + col0)
    (aq, amx), ad, (wq, wsc), wd = _fp8_operands(ops, M, N, K, g, mx=True)
    b = (torch.randn(N, generator=g, device='cuda') * 0.2).bfloat16()
    y, e = proj64(ad, wd, b, kstep=128)
    e += U32 * (ad.abs() @ wd.abs().T)
    ref, fl = _epi_ref(y, e, 'gelu' if gelu else 'none', col0, None, None)
    try:
        for kern in (1, 2):
            assert ops.set_fp8_tile(kern) == kern
            n8, nb = N - col0, (N - col0) // 128
            hbuf, head = _guarded(M, col0) if col0 else (None, None)
            qbuf = torch.full((M + 16, n8 + 128), 0xA5, dtype=torch.uint8, device='cuda')
            mbuf = torch.full((M + 16, nb + 8 + (-nb) % 4), 0xA5, dtype=torch.uint8, device='cuda')
            q, mx = qbuf[8:8 + M, 64:64 + n8], mbuf[8:8 + M, 4:4 + nb]
            ops.linear_fp8_to_mx8(aq, amx, wq, wsc, b, gelu=gelu, c8_col0=col0, out=(head, q, mx))
            torch.cuda.synchronize()
            what = f'fp8->mx8 {M}x{N}x{K} col0={col0} tile={kern}'
            if col0:
                _unchanged(hbuf, M, col0, f'{what} head')
            for buf, c0, n in ((qbuf, 64, n8), (mbuf, 4, nb)):
                mask = torch.ones(buf.shape, dtype=torch.bool, device='cuda')
                mask[8:8 + M, c0:c0 + n] = False
                assert bool((buf[mask] == 0xA5).all()), f'{what}: a write landed in the guard band of the fp8 output'
            if col0:
                check_bf16(head, ref[:, :col0], floor=fl[:, :col0], min_equal=FP8_EQUAL, what=f'{what} head')
            check_mx8(q, mx, ref[:, col0:], fl[:, col0:], what)
    finally:
        ops.set_fp8_tile(0)
    yd = y - ad[:, K - 1][:, None] * wd[:, K - 1][None, :]
    ref_d, _ = _epi_ref(yd, e, 'gelu' if gelu else 'none', col0, None, None)
    with pytest.raises(AssertionError):
        check_mx8(q, mx, ref_d[:, col0:], fl[:, col0:], f'{what}: one K column dropped')
