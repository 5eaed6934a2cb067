"""fp64 parity of the GEMM's fp32-output launch forms (GemmProblem::out_f32 1, 2, 3) and of the row quantiser in front of the fp8 GEMMs.

Split-K (``ops.linear_splitk``: afx_linear_bf16_splitk writes one fp32 slab per K chunk on the 8-phase kernel, afx_finish_f32_bf16 sums them):
the two C entry points are called directly so that the slabs can be inspected.  Reference and bound: tests/splitk_ref.py (depth = 2 per + 32
(+ 1 bias) + nslab (+ 1 residual), bound = depth 2^-24 (|A| |W|^T + |b| + |r|); each slab against the fp64 partial product of its own K range with
depth 2 per_s + 32 (+ 1)).  The finished bf16 output: one bf16 ulp + the bound, >= 99 % equal to RNE(y64).  The wrapper ``ops.linear_splitk`` then
has to give the same bits.  Teeth: the five mutated references of splitk_ref.py, each rejected by the same check (min_equal = 0).
fp32 store / accumulate (``ops.linear_f32out``, all eight GEMM modes): bound = (K / 32 + 32) 2^-24 |A| |W|^T (v_mfma_f32_16x16x32_bf16 in every
kernel: one rounding per instruction into the accumulator + the chain inside one; no bias, no output rounding: the accumulator is stored), plus
2^-24 |C_old + y| for the accumulate form's one add.  Teeth: K column K - 1 left out (store); C_old of rows 16..31 replaced by that of rows 0..15
(accumulate: what a stale prefetch register of epi_store_f32_acc would give).
Operands are views of larger buffers whose padding beyond K and beyond the last row holds NaN; outputs and slabs are views whose guard bands hold a
sentinel that must survive.
Row quantiser (``ops.quant_rows_fp8``): the scale equals fp32(max(absmax, 1e-12)) / 448 bit for bit -- arcflow_amd/build.py compiles with
-O3 and no fast-math flag, so the kernels' division is IEEE -- and every code lies in the admissible set of splitk_ref.quant_admissible.
launch_quant_rows_fp8 sends K = 3072, 12288 and 15360 to the register kernel and every other K, 512 included, to the two-pass kernel.
"""
import pytest
import torch
from bf16_parity import U32, bf16_ulp, check_bf16, check_f32
from splitk_ref import (QUANT_KS_REGISTER, QUANT_KS_TWO_PASS, QUANT_M, check_quant_codes, mutants_for, quant_inputs, quant_scale_f32, splitk_chunks,
                        splitk_mutant, splitk_operands, splitk_ref)

pytestmark = pytest.mark.gpu

SENT = -7.75
GUARD = 64                                                                          # floats in front of and behind the slabs
GEMM_MODES = [(3, 0), (3, 1), (3, 2), (3, 3), (3, 4), (3, 5), (3, 6), (2, 0)]      # as test_hip_gemm_fp64.py; forced tile 5 falls back to 256x256 for fp32 output


@pytest.fixture(scope='module')
def ops():
    from arcflow_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def lib():
    from arcflow_amd import _lib
    return _lib.load()


def _guarded(M, N, dtype=torch.bfloat16, strided=True):
    if not strided:
        buf = torch.full((M, N), SENT, dtype=dtype, device='cuda')
        return buf, buf
    buf = torch.full((M + 16, N + 128), SENT, dtype=dtype, device='cuda')
    return buf, buf[8:8 + M, 64:64 + N]


def _unchanged(buf, view, what):
    if buf is view:
        return
    M, N = view.shape
    mask = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    mask[8:8 + M, 64:64 + N] = False
    assert bool((buf[mask] == SENT).all()), f'{what}: a write landed in the guard band'


# ------------------------------------------------------------------------------------------------ split-K
# (id, M, N, K, split_k, bias, residual, strided out, expected (nslab, per) or None, large)
_RAGGED = [(f'ragged-{M}x{N}', M, N, 576, 3, (i % 2) == 0, (i % 3) != 0, (i % 2) == 1, (3, 3), False)
           for i, (M, N) in enumerate((m, n) for m in (1, 255, 257) for n in (8, 248, 264))]
SPLITK_TOY = [
    ('one-tile-per-chunk', 300, 520, 1024, 16, True, True, True, (16, 1), False),          # chunk shorter than the 4-deep DMA pipeline
    ('three-tiles-ragged-last', 130, 264, 640, 4, True, False, False, (4, 3), False),      # 3 + 3 + 3 + 1 K-tiles
    ('more-chunks-than-tiles', 77, 72, 128, 16, False, True, True, (2, 1), False),         # request clamped to nk
    ('single-chunk-auto', 64, 8, 64, 0, False, False, False, (1, 1), False),
    ('single-chunk-1', 200, 256, 512, 1, True, True, False, (1, 8), False),
] + _RAGGED
SPLITK_RELEASED = [
    ('t5-wo', 512, 4096, 10240, 8, False, True, False, (8, 20), True),
    ('qwen-down-162', 162, 3584, 18944, 16, False, True, True, (16, 19), True),            # per 19, last chunk 11
    ('qwen-down-40', 40, 3584, 18944, 16, False, True, False, (16, 19), True),
    ('clip-fc2', 77, 768, 3072, 0, True, True, False, (12, 4), True),
    ('qwen-qkv', 162, 4608, 3584, 0, True, False, False, None, True),
    ('qwen-o', 162, 3584, 3584, 0, False, True, False, None, True),
    ('skinny-4096', 4096, 256, 12288, 8, False, False, False, (8, 24), True),
    ('skinny-512', 512, 256, 15360, 16, False, False, True, (16, 15), True),
]


def _splitk_direct(ops, lib, a, w, b, r, out, split_k):
    """The two entry points on slabs inside a guarded buffer; returns (slab buffer, slabs [nslab, M, N])."""
    from arcflow_amd import _lib
    (M, K), N = a.shape, w.shape[0]
    nslab = lib.afx_linear_splitk_chunks(M, N, K, split_k)
    sbuf = torch.full((nslab * M * N + 2 * GUARD,), SENT, dtype=torch.float32, device='cuda')
    part = sbuf[GUARD:GUARD + nslab * M * N]
    _lib.check(lib.afx_linear_bf16_splitk(ops._p(a), a.stride(0), ops._p(w), w.stride(0), ops._p(b), ops._p(part), M, N, K, split_k, ops._s()))
    _lib.check(lib.afx_finish_f32_bf16(ops._p(part), nslab, ops._p(r), 0 if r is None else r.stride(0), ops._p(out), out.stride(0), M, N, ops._s()))
    torch.cuda.synchronize()
    return sbuf, part.view(nslab, M, N)


@pytest.mark.parametrize('case', SPLITK_TOY + SPLITK_RELEASED, ids=[c[0] for c in SPLITK_TOY + SPLITK_RELEASED])
def test_linear_splitk_vs_fp64(ops, lib, case):
    cid, M, N, K, split_k, bias, res, strided, expect, large = case
    a, w, b, r = splitk_operands(M, N, K, bias, res, seed=M * 7 + N * 3 + K, device='cuda', draw_on='cuda' if large else None)
    nslab, per = splitk_chunks(M, N, K, split_k)
    assert lib.afx_linear_splitk_chunks(M, N, K, split_k) == nslab, f'{cid}: the library cuts {lib.afx_linear_splitk_chunks(M, N, K, split_k)} chunks'
    if expect is not None:
        assert (nslab, per) == expect
    y, bound, parts = splitk_ref(a, w, b, r, nslab)
    buf, out = _guarded(M, N, strided=strided)
    sbuf, slabs = _splitk_direct(ops, lib, a, w, b, r, out, split_k)
    what = f'splitk {cid} {M}x{N}x{K} nslab={nslab} per={per}'
    assert bool((sbuf[:GUARD] == SENT).all() and (sbuf[-GUARD:] == SENT).all()), f'{what}: a write landed outside the slabs'
    _unchanged(buf, out, what)
    worst_s = 0.0
    for s, (p, bs) in enumerate(parts):
        check_f32(slabs[s], p, bs, what=f'{what} slab {s}')
        worst_s = max(worst_s, ((slabs[s].double() - p).abs() / bs.clamp_min(1e-300)).max().item())
    check_bf16(out, y, floor=bound, what=what)
    worst = ((out.double() - y).abs() / (bf16_ulp(y) + bound)).max().item()
    print(f'{what}: worst err / tol {worst:.3f} (output), {worst_s:.4f} (slabs)')
    # the wrapper: same bits, into the same kind of view
    buf2, out2 = _guarded(M, N, strided=strided)
    got = ops.linear_splitk(a, w, b, r, out=out2, split_k=split_k)
    torch.cuda.synchronize()
    assert got.data_ptr() == out2.data_ptr() and torch.equal(out2, out), f'{what}: ops.linear_splitk differs from the two entry points'
    _unchanged(buf2, out2, what)
    # teeth
    for kind in mutants_for(M, nslab, bias, res):
        with pytest.raises(AssertionError, match='beyond one bf16 ulp'):
            check_bf16(out, splitk_mutant(kind, a, w, b, r, nslab), floor=bound, min_equal=0.0, what=f'{what}: {kind}')


def test_linear_splitk_deterministic(ops):
    """Two launches of the Qwen down projection (16 chunks, fixed summation order in the finish) give the same bits."""
    a, w, b, r = splitk_operands(162, 3584, 18944, False, True, seed=5, device='cuda', draw_on='cuda')
    o1 = ops.linear_splitk(a, w, b, r, split_k=16)
    o2 = ops.linear_splitk(a, w, b, r, split_k=16)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2)


def test_linear_splitk_under_graph(ops):
    """One captured ops.linear_splitk (the slab allocated inside the capture, as in the encoders), replayed on two inputs written into the static
    operands: each replay equals the eager call on the same input bit for bit."""
    M, N, K = 77, 768, 3072
    ins = [splitk_operands(M, N, K, True, True, seed=s, device='cuda') for s in (11, 12)]
    w, b = ins[0][1], ins[0][2]
    eager = [ops.linear_splitk(a, w, b, r) for (a, _, _, r) in ins]
    a_s, r_s = ins[0][0].clone(), ins[0][3].clone()
    ops.linear_splitk(a_s, w, b, r_s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_s = ops.linear_splitk(a_s, w, b, r_s)
    for (a, _, _, r), want in zip(ins, eager):
        a_s.copy_(a)
        r_s.copy_(r)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_s, want)
    assert not torch.equal(eager[0], eager[1])


def test_linear_splitk_argument_guards(ops, lib):
    """split_k < 0, N % 8 != 0, K % 64 != 0 and (on the finish) ldo % 8 != 0 return AFX_E_INVALID and write nothing."""
    from arcflow_amd import _lib
    M, N, K = 40, 24, 128
    a, w, b, r = splitk_operands(M, N, K, True, True, seed=3, device='cuda')
    part = torch.full((4 * M * (N + 8),), SENT, dtype=torch.float32, device='cuda')
    out = torch.full((M, N + 12), SENT, dtype=torch.bfloat16, device='cuda')

    def gemm(n, k, sk):
        return lib.afx_linear_bf16_splitk(ops._p(a), a.stride(0), ops._p(w), w.stride(0), ops._p(b), ops._p(part), M, n, k, sk, ops._s())
    assert gemm(N, K, -1) == _lib.AFX_E_INVALID
    assert gemm(N - 4, K, 2) == _lib.AFX_E_INVALID
    assert gemm(N, K - 32, 2) == _lib.AFX_E_INVALID
    assert lib.afx_finish_f32_bf16(ops._p(part), 2, ops._p(r), r.stride(0), ops._p(out), N + 12, M, N, ops._s()) == _lib.AFX_E_INVALID
    assert lib.afx_finish_f32_bf16(ops._p(part), 2, ops._p(r), r.stride(0), ops._p(out), N + 8, M, N - 4, ops._s()) == _lib.AFX_E_INVALID
    torch.cuda.synchronize()
    assert bool((part == SENT).all()) and bool((out == SENT).all())


# ------------------------------------------------------------------------------------------------ fp32 store and accumulate
def _nan_padded(t):
    """A bf16 [R, C] matrix as a view of a buffer whose 8 rows below and 64 columns to the right hold NaN."""
    R, C = t.shape
    buf = torch.full((R + 8, C + 64), float('nan'), dtype=torch.bfloat16, device='cuda')
    buf[:R, :C] = t
    return buf[:R, :C]


def _f32out_operands(cid, M, N, K, g):
    if cid.startswith('lora-grad'):         # the trunk's weight-gradient operands: token-major matrices through ops.transpose(., 64); 4224 is the
        from arcflow_amd import ops         # 4133-token shape padded to whole 128-row tiles, the rows past 4133 zero
        rows = 4133 if K == 4224 else K
        x = (torch.randn(K, M + 8, generator=g, device='cuda') * 1.2 + 0.1).bfloat16()[:, :M]
        t = (torch.randn(K, N, generator=g, device='cuda') * K ** -0.5).bfloat16()
        x[rows:], t[rows:] = 0, 0
        a, w = ops.transpose(x, 64), ops.transpose(t, 64)
        assert a.shape == (M, K) and w.shape == (N, K) and torch.equal(a, x.T) and torch.equal(w, t.T)
        return a, w, rows - 1
    a = _nan_padded((torch.randn(M, K, generator=g, device='cuda') * 1.2 + 0.1).bfloat16())
    w = _nan_padded((torch.randn(N, K, generator=g, device='cuda') * K ** -0.5).bfloat16())
    return a, w, K - 1


F32_CASES = [('edge-ldc272', 264, 264, 128), ('tall-n8', 1000, 8, 192), ('wide-one-ktile', 17, 520, 64), ('lora-grad-4133', 3072, 256, 4224),
             ('lora-grad-4608', 256, 3072, 4608), ('merge', 3072, 3072, 256), ('vae-logits', 1024, 1024, 512)]


@pytest.mark.parametrize('cid,M,N,K', F32_CASES, ids=[c[0] for c in F32_CASES])
def test_linear_f32out_vs_fp64_every_mode(ops, cid, M, N, K):
    g = torch.Generator(device='cuda').manual_seed(M * 7 + K * 3 + N)
    a, w, kd = _f32out_operands(cid, M, N, K, g)          # kd: the last K column that holds values (the one the teeth check leaves out)
    ad, wd = a.double(), w.double()
    y, mag = ad @ wd.T, ad.abs() @ wd.abs().T
    bound = (K // 32 + 32) * U32 * mag
    c_old = torch.randn(M, N, generator=g, device='cuda') * 1.2
    acc_ref = c_old.double() + y
    acc_bound = bound + U32 * acc_ref.abs()
    if cid == 'edge-ldc272':                # ldc = 272: the sentinel columns 264..271 sit inside every row
        buf = torch.full((M + 16, 272), SENT, dtype=torch.float32, device='cuda')
        out = buf[8:8 + M, :N]
        mask = torch.ones(buf.shape, dtype=torch.bool, device='cuda')
        mask[8:8 + M, :N] = False

        def intact(what):
            assert bool((buf[mask] == SENT).all()), f'{what}: a write landed in the guard band'
    else:
        buf, out = _guarded(M, N, dtype=torch.float32)

        def intact(what):
            _unchanged(buf, out, what)
    worst = [0.0, 0.0]
    try:
        for mode in GEMM_MODES:
            ops.set_gemm_mode(*mode)
            what = f'f32out {cid} {M}x{N}x{K} mode={mode}'
            out.fill_(SENT)
            assert ops.linear_f32out(a, w, out=out).data_ptr() == out.data_ptr()
            torch.cuda.synchronize()
            intact(what)
            check_f32(out, y, bound, what=f'{what} store')
            worst[0] = max(worst[0], ((out.double() - y).abs() / bound.clamp_min(1e-300)).max().item())
            store = out.clone()
            out.copy_(c_old)
            ops.linear_f32out(a, w, out=out, accumulate=True)
            torch.cuda.synchronize()
            intact(f'{what} accumulate')
            check_f32(out, acc_ref, acc_bound, what=f'{what} accumulate')
            worst[1] = max(worst[1], ((out.double() - acc_ref).abs() / acc_bound.clamp_min(1e-300)).max().item())
            # teeth, on this mode's own output
            with pytest.raises(AssertionError, match='beyond the bound'):
                check_f32(store, y - ad[:, kd][:, None] * wd[:, kd][None, :], bound, what=f'{what}: one K column dropped')
            stale = c_old.double().clone()
            n = min(32, M) - 16
            stale[16:16 + n] = c_old.double()[:n]
            with pytest.raises(AssertionError, match='beyond the bound'):
                check_f32(out, stale + y, acc_bound, what=f'{what}: C_old of the second row tile stale')
    finally:
        ops.set_gemm_mode(3, 0)
    print(f'f32out {cid} {M}x{N}x{K}: worst err / bound {worst[0]:.4f} (store), {worst[1]:.4f} (accumulate)')


# ------------------------------------------------------------------------------------------------ the row quantiser
def _quant_direct(ops, lib, x):
    """afx_quant_rows_fp8 into views of 0xA5 / sentinel buffers; returns (q, scale) after the guard checks."""
    from arcflow_amd import _lib
    M, K = x.shape
    qbuf = torch.full((M + 16, K + 128), 0xA5, dtype=torch.uint8, device='cuda')
    sbuf = torch.full((M + 16,), SENT, dtype=torch.float32, device='cuda')
    q, sc = qbuf[8:8 + M, 64:64 + K], sbuf[8:8 + M]
    _lib.check(lib.afx_quant_rows_fp8(ops._p(x), x.stride(0), ops._p(q), q.stride(0), ops._p(sc), M, K, ops._s()))
    torch.cuda.synchronize()
    mask = torch.ones(qbuf.shape, dtype=torch.bool, device='cuda')
    mask[8:8 + M, 64:64 + K] = False
    assert bool((qbuf[mask] == 0xA5).all()), f'quant_rows_fp8 K={K}: a write landed in the guard bytes round q'
    assert bool((sbuf[:8] == SENT).all() and (sbuf[8 + M:] == SENT).all()), f'quant_rows_fp8 K={K}: a write landed beside the scales'
    return q, sc


def check_quantiser(x, q, sc, what, cap=0.005):
    """Scale: bit-equal to the fp32 formula (and so within one fp32 ulp of absmax / 448 in fp64); every code admissible.  Returns the two-code share."""
    want = quant_scale_f32(x)
    assert torch.equal(sc.cpu(), want), f'{what}: {int((sc.cpu() != want).sum())} scales differ from fp32(max(absmax, 1e-12)) / 448'
    ref64 = x.double().abs().amax(1).clamp_min(1e-12) / 448.0
    assert bool(((sc.double() - ref64).abs() <= 2 * U32 * ref64).all()), f'{what}: a scale more than one fp32 ulp from absmax / 448'
    return check_quant_codes(x, q, sc, what=what, cap=cap)


@pytest.mark.parametrize('K', QUANT_KS_TWO_PASS + QUANT_KS_REGISTER)
def test_quant_rows_fp8_every_code(ops, lib, K):
    """515 rows (a ragged last block of four) from a strided view, with an all-zero row, a row with one value 2000 x the rest and a row whose
    absmax is 448 * 2^-6; 3072 and 15360 take the register kernel, the others the two-pass kernel."""
    x = quant_inputs(K, 'cuda')
    assert x.shape == (QUANT_M, K) and x.stride(0) == K + 64
    q, sc = _quant_direct(ops, lib, x)
    share = check_quantiser(x, q, sc, f'quant_rows_fp8 K={K}')
    print(f'quant_rows_fp8 K={K}: two-code share {share:.2e}')
    assert bool((q[3] == 0).all()) and sc[7].item() == 2.0 ** -6
    q2, sc2 = ops.quant_rows_fp8(x)                                  # the wrapper (dense q): same bits
    assert torch.equal(q2, q) and torch.equal(sc2, sc)
    bad = q.clone()
    bad[100, K // 3] ^= 0x80 if int(q[100, K // 3]) & 0x7f else 0x01
    with pytest.raises(AssertionError, match='outside their admissible set'):
        check_quant_codes(x, bad, sc)


@pytest.mark.parametrize('K', QUANT_KS_REGISTER)
def test_quant_rows_fp8_kernels_agree(ops, lib, K):
    """The register kernel at K and the two-pass kernel at K + 8 (not a multiple of 512; eight zero columns appended to the same rows) give the
    same scales and the same codes on the K leading columns."""
    x = quant_inputs(K, 'cuda')
    wide = torch.zeros(QUANT_M, K + 72, dtype=torch.bfloat16, device='cuda')
    wide[:, :K] = x
    x8 = wide[:, :K + 8]
    q, sc = _quant_direct(ops, lib, x)
    q8, sc8 = _quant_direct(ops, lib, x8)
    assert torch.equal(sc8, sc) and torch.equal(q8[:, :K], q) and bool((q8[:, K:] == 0).all())
