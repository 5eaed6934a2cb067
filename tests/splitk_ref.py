"""References of tests/test_hip_gemm_f32out_fp64.py (and of the `_linear` table of test_text_encoders.py): the split-K product of
``ops.linear_splitk`` in fp64 with a bound written from the kernels' rounding points, an fp32 emulation of those rounding points, five mutated
references (the teeth checks), and the definition of the row quantiser ``ops.quant_rows_fp8`` with its admissible codes.  Plain torch on
whatever device the operands live on; tests/test_splitk_ref_cpu.py holds the emulation inside the bound and the mutants outside it on the CPU.

Split-K (afx_ops_api.hip afx_linear_splitk_chunks / afx_linear_bf16_splitk, afx_gemm.hip gemm_kernel_v2, afx_text.hip finish_f32_kernel):
  * nk = K / 64 K-tiles; per = ceil(nk / split_k) tiles per chunk; nslab = ceil(nk / per) chunks, none empty.  The kernel recomputes
    per = ceil(nk / nslab) from the chunk count it is handed; the two agree for every (nk, split_k) (test_splitk_ref_cpu.py sweeps it).
  * the 8-phase kernel issues v_mfma_f32_16x16x32_bf16 (AFX_MFMA_QUAD: kk = 0, 1 per 64-wide K-tile): a chunk of `per` tiles is 2 per roundings
    into the accumulator plus a serial chain over one instruction's 32 products;
  * + 1 for the bias (added by chunk 0 only, in fp32, before the slab store), + nslab adds in finish_f32_kernel (v = 0 + slab 0 + slab 1 ...),
    + 1 for the residual; only the adds that the call has are counted.
  depth = 2 per + 32 (+ 1) + nslab (+ 1);  bound = depth 2^-24 mag,  mag = |A| |W|^T + |b| + |r|.
  Slab s holds the fp32 partial product of its own K range (+ bias in slab 0): depth_s = 2 per_s + 32 (+ 1), against its own mag_s.

Row quantiser (afx_text.hip quant_rows_fp8_kernel / quant_rows_fp8_reg_kernel):
  sc = fp32(max(absmax, 1e-12)) / 448 in fp32 (an IEEE division: the build has no fast-math flag), inv = fp32(1 / sc),
  code = RNE_e4m3(clamp(fp32(x inv), -448, 448)).  inv and the product round once each: x inv = (x / sc) (1 + d), |d| < 3 2^-24.  The admissible
  codes of an element are therefore RNE_e4m3 of (x64 / sc64) (1 - 3 2^-24) and of (x64 / sc64) (1 + 3 2^-24): one code, or two neighbours where
  that interval straddles a rounding midpoint.  Where sc is a power of two both fp32 operations are exact and only RNE_e4m3(x / sc) is admissible
  (ties included: they go to the even code).
"""
import torch

U32 = 2.0 ** -24
KTILE = 64          # BK of afx_gemm.hip: the K-tile the chunking counts in
MFMA_K = 32         # v_mfma_f32_16x16x32_bf16: products summed inside one instruction
MUTANTS = ('boundary_tile', 'bias_every_chunk', 'last_chunk', 'residual_row', 'slab_twice')


# ------------------------------------------------------------------------------------------------ chunk arithmetic
def splitk_chunks(M, N, K, split_k):
    """(nslab, per) as afx_linear_splitk_chunks computes them (split_k <= 0: the automatic rule)."""
    tiles, nk = ((M + 255) // 256) * ((N + 255) // 256), K // KTILE
    if split_k <= 0:
        split_k = max(min((512 + tiles // 2) // tiles, nk // 4), 1)
    split_k = min(split_k, nk)
    per = (nk + split_k - 1) // split_k
    return (nk + per - 1) // per, per


def chunk_ranges(K, nslab):
    """[k0, k1) of every chunk as gemm_kernel_v2 cuts them from the chunk count: per = ceil(nk / nslab), t0 = chunk per, min(per, nk - t0) tiles."""
    nk = K // KTILE
    per = (nk + nslab - 1) // nslab
    return [(s * per * KTILE, min((s + 1) * per, nk) * KTILE) for s in range(nslab)]


def splitk_depth(per, nslab, bias, residual):
    return 2 * per + MFMA_K + int(bias) + nslab + int(residual)


# ------------------------------------------------------------------------------------------------ fp64 reference
def splitk_ref(a, w, b, r, nslab):
    """y = a w^T (+ b) (+ r) in fp64 with its bound, and per slab the fp64 partial product (+ b in slab 0) with its own bound.
    Returns (y, bound, parts) with parts = [(p_s, bound_s)]."""
    ad, wd = a.double(), w.double()
    K = a.shape[1]
    ranges = chunk_ranges(K, nslab)
    per = (ranges[0][1] - ranges[0][0]) // KTILE
    y, mag, parts = None, None, []
    for s, (k0, k1) in enumerate(ranges):
        p, m = ad[:, k0:k1] @ wd[:, k0:k1].T, ad[:, k0:k1].abs() @ wd[:, k0:k1].abs().T
        if s == 0 and b is not None:
            p, m = p + b.double(), m + b.double().abs()
        parts.append((p, (2 * ((k1 - k0) // KTILE) + MFMA_K + int(s == 0 and b is not None)) * U32 * m))
        y, mag = (p.clone(), m.clone()) if y is None else (y + p, mag + m)
    if r is not None:
        y, mag = y + r.double(), mag + r.double().abs()
    return y, splitk_depth(per, nslab, b is not None, r is not None) * U32 * mag, parts


def splitk_mutant(kind, a, w, b, r, nslab):
    """The fp64 value a subtly wrong split-K would give:
    boundary_tile: the first K-tile of chunk 1 left out;  bias_every_chunk: the bias added by all nslab chunks;  last_chunk: the last
    (shorter) chunk dropped;  residual_row: row m takes the residual of row m + 1 (the last one that of row 0);  slab_twice: slab s summed
    twice and slab s + 1 not at all (s = 1 where there are three slabs, else 0)."""
    ad, wd = a.double(), w.double()
    ranges = chunk_ranges(a.shape[1], nslab)
    y = ad @ wd.T
    if b is not None:
        y = y + b.double()
    if r is not None:
        y = y + (r.double() if kind != 'residual_row' else torch.roll(r.double(), -1, 0))

    def part(k0, k1):
        return ad[:, k0:k1] @ wd[:, k0:k1].T
    if kind == 'boundary_tile':
        k0 = ranges[1][0]
        return y - part(k0, k0 + KTILE)
    if kind == 'bias_every_chunk':
        return y + (nslab - 1) * b.double()
    if kind == 'last_chunk':
        return y - part(*ranges[-1])
    if kind == 'slab_twice':
        s = 1 if nslab >= 3 else 0
        return y + part(*ranges[s]) + (b.double() if s == 0 and b is not None else 0.0) - part(*ranges[s + 1])
    assert kind == 'residual_row'
    return y


def mutants_for(M, nslab, bias, residual):
    """The mutants that differ from the reference for a call of this form."""
    out = []
    if nslab >= 2:
        out += ['boundary_tile', 'last_chunk', 'slab_twice'] + (['bias_every_chunk'] if bias else [])
    if residual and M >= 2:
        out.append('residual_row')
    return out


def splitk_emulate_f32(a, w, b, r, nslab):
    """The rounding points in fp32: per chunk one accumulator, per MFMA step a serial fp32 chain over its 32 (exact) products added to the
    accumulator; the bias into chunk 0; the slabs summed in order from zero; the residual; one rounding to bf16.  Small shapes only."""
    af, wf = a.float(), w.float()
    slabs = []
    for s, (k0, k1) in enumerate(chunk_ranges(a.shape[1], nslab)):
        acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32, device=a.device)
        for k in range(k0, k1, MFMA_K):
            step = torch.zeros_like(acc)
            for j in range(k, k + MFMA_K):
                step = step + af[:, j, None] * wf[None, :, j]
            acc = acc + step
        if s == 0 and b is not None:
            acc = acc + b.float()
        slabs.append(acc)
    v = torch.zeros_like(slabs[0])
    for p in slabs:
        v = v + p
    if r is not None:
        v = v + r.float()
    return v.bfloat16(), slabs


def splitk_operands(M, N, K, bias, residual, seed, device='cpu', draw_on=None):
    """a [M, K], w [N, K] as views of buffers whose padding (64 columns beyond K, 8 rows beyond the last) holds NaN, bias and residual of order 1
    against products of order 1.  Drawn on the CPU from `seed` (so the CPU tests and the device tests see the same values) unless draw_on names
    the device to draw on (the large released shapes)."""
    gd = draw_on or 'cpu'
    g = torch.Generator(device=gd).manual_seed(seed)
    abuf = torch.full((M + 8, K + 64), float('nan'), device=gd)
    wbuf = torch.full((N + 8, K + 64), float('nan'), device=gd)
    abuf[:M, :K] = torch.randn(M, K, generator=g, device=gd) * 1.2 + 0.1
    wbuf[:N, :K] = torch.randn(N, K, generator=g, device=gd) * K ** -0.5
    a, w = abuf.bfloat16().to(device)[:M, :K], wbuf.bfloat16().to(device)[:N, :K]
    b = torch.randn(N, generator=g, device=gd).bfloat16().to(device) if bias else None
    r = None
    if residual:
        r = torch.randn(M, N + 8, generator=g, device=gd).bfloat16().to(device)[:, :N]       # row stride N + 8
    return a, w, b, r


# ------------------------------------------------------------------------------------------------ the row quantiser
def rne_e4m3(t):
    """fp64 -> the nearest OCP e4m3 value (ties to even), |t| <= 448, as fp64: quantum 2^(e - 3) with e = floor(log2 |t|) >= -6."""
    _, ex = torch.frexp(t)                                  # |t| = m 2^ex, m in [0.5, 1)
    q = torch.exp2((ex - 1).clamp_min(-6).double() - 3)
    return torch.round(t / q) * q                           # exact: power-of-two quantum, torch.round is half-to-even


def e4m3_ord(codes):
    """uint8 e4m3 codes -> signed ordinals (monotonic in the value, +-0 -> 0, the NaN codes -> +-127)."""
    c = codes.long()
    mag = c & 0x7f
    return torch.where((c & 0x80) != 0, -mag, mag)


def _ord_of_value(v):
    return e4m3_ord(v.float().to(torch.float8_e4m3fn).view(torch.uint8))       # v is an e4m3 value: the cast is exact


def quant_scale_f32(x):
    """The scale as the kernel defines it, fp32 on the CPU (IEEE division): fp32(max(absmax, 1e-12)) / 448."""
    return x.float().abs().amax(1).cpu().clamp_min(1e-12) / 448.0


def quant_admissible(x, sc):
    """x bf16 [M, K], sc fp32 [M] (the scale in use).  Returns (lo, hi, two): the ordinals of the admissible codes (lo == hi where there is one) and
    the mask of the two-code elements."""
    t = x.double() / sc.double()[:, None]
    pow2 = (torch.frexp(sc.double())[0] == 0.5)[:, None]
    w = torch.where(pow2, 0.0, 3 * U32)
    t0, t1 = (t * (1 - w)).clamp(-448, 448), (t * (1 + w)).clamp(-448, 448)
    o0, o1 = _ord_of_value(rne_e4m3(t0)), _ord_of_value(rne_e4m3(t1))
    lo, hi = torch.minimum(o0, o1), torch.maximum(o0, o1)
    return lo, hi, lo != hi


def check_quant_codes(x, q, sc, what='', cap=0.005):
    """Every code of q admissible for (x, sc); the two-code share at most cap (None: the per-element check alone).  Returns the share."""
    lo, hi, two = quant_admissible(x, sc)
    assert bool(((hi - lo) <= 1).all()), f'{what}: an admissible set wider than two neighbouring codes'
    got = e4m3_ord(q)
    bad = (got < lo) | (got > hi)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} codes outside their admissible set; first: x {x.flatten()[i].item()} '
                             f'code {int(q.flatten()[i])} admissible ordinals [{int(lo.flatten()[i])}, {int(hi.flatten()[i])}]')
    share = two.double().mean().item()
    assert cap is None or share <= cap, f'{what}: {share:.5f} of the elements have two admissible codes (cap {cap})'
    return share


QUANT_M = 515
QUANT_KS_TWO_PASS = (8, 1152, 3584, 16384, 512)       # K != 3072 / 12288 / 15360: quant_rows_fp8_kernel (512 included: see launch_quant_rows_fp8)
QUANT_KS_REGISTER = (3072, 15360)                     # quant_rows_fp8_reg_kernel<6> / <30>


def quant_inputs(K, device='cpu'):
    """The device test's source: [515, K] as a view (row stride K + 64) of randn * 3, with row 3 all zero, row 5 holding one value 2000 x the
    rest, and row 7 rescaled so that its absmax is exactly 448 * 2^-6 = 7 (values k / 16, |k| <= 112, all bf16).
    Every other row gets a planted maximum +-(129 + 2 j) / 4, j = row % 64: an odd 8-bit significand.  Plain randn rows gave a two-code share of
    0.40 - 0.61 % (measured, every K): x and absmax are both 8-bit significands, so 448 x / absmax is an EXACT e4m3 rounding midpoint for many x
    whenever absmax's significand is 2^k or 7 2^k (1/16 of such a row), and the fp32 rounding of the scale then decides the code.  An odd
    significand >= 129 divides 7 x only for a handful of x, which leaves the ties to row 7, where they are checked exactly."""
    g = torch.Generator().manual_seed(1000 + K)
    big = torch.randn(QUANT_M, K + 64, generator=g) * 3.0
    rows = torch.arange(QUANT_M)
    big[rows, (rows * 5) % K] = (129.0 + 2 * (rows % 64)) / 4 * (1 - 2 * (rows % 2)).float()
    big[3, :K] = 0.0
    big[5, :K] = big[5, :K].clamp(-3, 3) / 3.0
    big[5, K // 2] = 2000.0
    big[7, :K] = torch.round(big[7, :K].clamp(-6.9, 6.9) * 16) / 16
    big[7, K - 1] = -7.0
    return big.bfloat16().to(device)[:, :K]
