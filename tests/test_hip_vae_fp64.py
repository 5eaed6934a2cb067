"""fp64 parity of the VAE kernels (afx_vae.hip and the convolution instances of afx_gemm.hip), per element, at the released widths.

Every reference is plain fp64 torch on the same bf16-rounded inputs, evaluated on the device (tests/bf16_parity.py).  bf16 outputs must lie within one
bf16 ulp of the fp64 value plus a floor F and >= 99 % of them must equal the fp64 value rounded to nearest even (check_bf16); the ulp covers the output's
own rounding, F bounds the fp32 arithmetic in front of it.  u = 2^-24.  Every case prints its worst |error| / bound and its RNE share (-s).  Every output
is a view of a larger buffer: grids start as NaN (every position must be written), their guard rows hold a sentinel that must survive.

1. Convolutions.  Reference conv64: kh kw shifted fp64 matmuls on the padded NHWC grid (held equal to F.conv2d in tests/test_conv64_reference_cpu.py).
   F = (K / 32 + 33) u (|x| |w| + |b|): proj64's model of the MFMA accumulation (one rounding per 32-deep K-step, a serial chain inside one instruction,
   the bias), K as the GEMM runs it: 9 Cin (3x3), 4 Cin (one phase of the folded upsample), 36 Cin (stride 2 on the space-to-depth grid: the 27 zero
   blocks of s2d_weights are multiplied too), 64 (conv_in on afx_image_to_cols27's rows).  A residual launch adds 2 u (|y| + |r|).  The folded upsample is
   held to the four 2x2 convolutions with the STORED bf16 phase weights; the stride-2 route to the stride-2 convolution on the original weights
   (s2d_weights is an exact re-layout).  Shapes: every distinct (H, W, Cin, Cout, kind) of the FLUX 128/256/512/512 and Qwen-Image dim-96 decoders and
   encoders at 1024^2 (the table is held against the models' weight shapes on the CPU, tests/test_conv64_reference_cpu.py), the ragged grids 9x13, 31x33,
   300x70, and 14x62 whose 16 x 64 = 1024 padded rows are a multiple of 256 (258 x 1026 is not).  The released grids keep their WIDTH -- the row pitch
   W + 2 that the tap shifts, the border columns and the guard rows depend on -- and run 256 of their rows where they have more (REF_ROWS): the fp64
   references of the full 512^2 and 1024^2 grids cost 0.7 s more.  258 x 1026 rows are still 1035 tiles of 256 rows, four per compute unit, and a tile
   cannot tell which row of the grid it starts at beyond that row's border test.  Measured on one MI355X: this file 6.0 s (116 cases), tests/
   test_hip_gemm_fp64.py 3.55 s (29 cases); 1.8 s of the 6.0 are the first convolution and the first GroupNorm case (library and fp64 BLAS start-up),
   the remaining cases take 2.0 s together, none above 0.15 s.  That is 0.65 s past "half more than the GEMM file"; what is left to cut is cases
   (the 1024^2 GroupNorm grids alone are 0.25 s), which stay.  Plain and residual launches run in the default mode and on the 8-phase
   kernel (set_gemm_mode(2, 0)); the folded upsample and the statistics epilogue must answer with a status there.
   Teeth (bound alone, min_equal = 0): the reference with tap (1, 1) (one of the four for a phase) left out, with the last 64-channel chunk left out, and
   for stride 2 with the padded row H read as row H - 1, must each fail.
2. GroupNorm sums of the epilogue against fp64 sums of the fp64 convolution (not of the stored grid).  epi_store_fast_acc adds, per lane and quantity,
   4 values of each of the MI = 8 row tiles into one fp32 running sum (gsum / gsq: 32 additions), then 4 DPP additions across the 16 lanes of a row
   (row_sum), then one fp64 atomic: 36 fp32 additions, 37 roundings for a square.  Bound of a group's sum: sum F_e + 36 u sum |y|; of its sum of
   squares: sum (2 |y| F_e + F_e^2) + 37 u sum y^2.
3. GroupNorm apply.  Two-pass fp64 mean / variance over the interior, affine map, SiLU.  gn_stats_kernel: a lane adds 4 values per row it owns into each
   fp32 accumulator, ceil(rows / (blocks * rstep)) rows with blocks = min(2048, ceil(rows / rstep)), rstep = 256 / (C / 8); the block adds its lanes'
   512 / groups values per group in fp64 (a fixed order) and rounds that sum to fp32 once; then fp64.  D = 4 ceil(rows / (blocks rstep)) + 1 (133 at
   1024^2, C = 128), D + 1 for the squares.  dmean = D u E|x|, dvar = (D + 1) u E[x^2] + 2 |mean| dmean.  a = rsqrt(var + eps) gamma lies between gamma / sqrt(var + dvar
   + eps) and gamma / sqrt(max(var - dvar, 0) + eps) -- the variance cannot be negative -- up to 4 u (the fp32 cast, the addition, v_rsq_f32's 1 ulp, the
   product): that interval's half-width is da.  The output is a' (x - mean') + beta evaluated as x a' + (beta - mean' a'), so
   F = da |x - mean| + |a_hi| dmean + 3 u (|x a_hi| + |mean a_hi| + |beta|), which is never above the uncorrelated |x| da + db form.
   SiLU: 1.1 F (|silu'| <= 1.1) + (|t| + 8) u |silu(t)| (__expf: a product by log2(e), 1 u relative on an argument of size |t| log2(e), v_exp_f32 1 ulp, the
   addition, the division).  afx_groupnorm_nhwc_from_stats gets exact fp64 sums spread over the 64 slots: D = 0.
   Two channels per group (C = 64, 32 groups) are refused by afx_groupnorm_nhwc (its statistics kernel owns 4-channel halves) and accepted by
   afx_groupnorm_nhwc_from_stats, which is held to the same reference there.
   Teeth: count = (H + 2)(W + 2) and one channel's group index shifted must fail, for either entry point's output.  A constant group (|x| = 9.9375 in all of its channels) on 1024^2
   must come out finite and equal to beta within F (there da |x - mean| = 0: F = 1000 |gamma| dmean + the apply term).
4. afx_softmax_rows_f32 against fp64 softmax of the same fp32 logits: one ulp + c u (1 + |t|) p, t = (s - max) scale.  The argument t carries 2 u |t| (the
   subtraction, the product), __expf multiplies by log2(e) (1.5 u |t| with the constant's own rounding) and v_exp_f32 is good to 1 ulp (2 u): the numerator
   carries (3.5 |t| + 2) u.  The denominator carries the p-weighted mean of that plus its summation: 64 serial additions per lane in the register kernel
   (NV * 4), ceil(cols / 256) in the three-pass kernel, + 6 (wave_sum) + 3 (four waves); the reciprocal 2 u, the product 1 u.  The stored row must sum
   to 1 within the sum over its elements of half an ulp (round to nearest) + the floor: per element because a peaked row is one element in [1/2, 1)
   whose half ulp alone is 2^-9, so no fixed small figure holds for every row.
   c = depth + 16 + 3.5 E_p|t| per row, depth = 73 or ceil(cols / 256) + 9.  Logits: normal with the standard deviation measured on the mid-block of
   this file's attention chain (printed), and 4x that (peaked rows, as trained decoders give), not only N(0, 4).
   _single_head_attention at N = 16384 (C = 512) and N = 35 x 29: every stage against fp64 of ITS OWN inputs -- gather bit-exact, qkv / PV / projection
   through proj64, fp32 logits within proj64's floor, P as above (padded keys and rows zero; teeth: the softmax over the padded keys too must
   fail), scatter + residual = RNE of the fp32 sum with a zero border.
5. Layout kernels: bit equality with torch indexing.  Where an fp32 map is applied (latent unpack), equality with RNE of the fp64 map wherever the fp32
   evaluation cannot move it across a bf16 rounding boundary (error e: 2 u (|t / s| + |shift|), or 18 u (|A| |t| + |b|) for the 16-term affine map), and a
   value between RNE(v - e) and RNE(v + e) elsewhere: the kernel's output is RNE of SOME value within e of v and rounding is monotone, and where the affine
   map cancels to |v| far below e those two are several bf16 steps apart, so "one of the two neighbours" would be wrong there.  The share of such elements
   is printed and must stay <= 2 %: an element is unsure with probability min(1, 2 e / ulp(v)) = 2 * 18 * 2^-24 * 2^8 (|A| |t| + |b|) / |v| = 5.5e-4 times the
   cancellation ratio, a few 1e-3 on these inputs (measured 6e-5 to 1.2e-2, the latter 3 of 256 elements); a window widened tenfold would show as > 2 %.
6. afx_rmsnorm_nhwc: one ulp + (Cpad / 8 + log2(LP) + 4) u |y|.  The kernel: 8 squares added serially per lane (9 roundings), log2(LP) shuffle additions,
   halved by the square root; sqrtf, sqrtf(Creal), the division, two products: (9 + log2 LP) / 2 + 6 <= Cpad / 8 + log2(LP) + 4 for every Cpad >= 64.
   SiLU as in 3.
"""
import ctypes as C
import math

import pytest
import torch
from bf16_parity import U32, bf16_ulp, check_bf16, check_f32, conv64, proj64, silu64

pytestmark = pytest.mark.gpu

SENT = -7.75
NAN = float('nan')


@pytest.fixture(scope='module')
def ops():
    from arcflow_amd import ops as _ops
    return _ops


@pytest.fixture(scope='module')
def lib():
    from arcflow_amd import _lib
    return _lib.load()


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _s():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ok(rc):
    from arcflow_amd import _lib
    _lib.check(rc)


def _in_grid(x):
    """x [H, W, C] bf16 -> a zero-bordered grid with zero guard rows."""
    from arcflow_amd.vae import _Grid
    H, W, Cn = x.shape
    g = _Grid(H, W, Cn, 'cuda')
    g.t.view(H + 2, W + 2, Cn)[1:-1, 1:-1] = x
    return g


def _out_grid(H, W, Cn):
    """An output grid: NaN everywhere, the guard rows in front of and behind it at the sentinel."""
    from arcflow_amd.vae import _Grid
    rows, guard = (H + 2) * (W + 2), W + 3
    g = _Grid(H, W, Cn, 'cuda', torch.full((rows + 2 * guard, Cn), SENT, dtype=torch.bfloat16, device='cuda'))
    g.t.fill_(NAN)
    return g


def _view(g):
    return g.t.view(g.H + 2, g.W + 2, g.C)


def _guards_intact(g, what):
    rows = (g.H + 2) * (g.W + 2)
    assert bool((g.buf[:g.guard] == SENT).all()) and bool((g.buf[g.guard + rows:] == SENT).all()), f'{what}: a write landed in the guard rows'


def _border_zero(g, what):
    v = _view(g)
    assert bool(torch.isfinite(v.float()).all()), f'{what}: a position of the grid was not written'
    for name, b in (('top', v[0]), ('bottom', v[-1]), ('left', v[:, 0]), ('right', v[:, -1])):
        assert not bool(b.any()), f'{what}: the {name} border is not zero'


def _report(out, ref, floor, what):
    ref = ref.double()
    ratio = ((out.double() - ref).abs() / (bf16_ulp(ref) + floor)).max().item()
    share = (out == ref.float().bfloat16()).double().mean().item()
    print(f'{what}: worst error / bound {ratio:.3f}, RNE share {share:.4f}')


def _check_grid(g, ref, floor, what, min_equal=0.99):
    """The whole grid: written, zero border, guards, interior per element; the first / last interior row and column once more on their own."""
    _border_zero(g, what)
    _guards_intact(g, what)
    out = _view(g)[1:-1, 1:-1]
    _report(out, ref, floor, what)
    check_bf16(out, ref, floor=floor, min_equal=min_equal, what=what)
    for name, sl in (('first row', (0,)), ('last row', (-1,)), ('first column', (slice(None), 0)), ('last column', (slice(None), -1))):
        check_bf16(out[sl], ref[sl], floor=floor[sl], min_equal=min_equal, what=f'{what}, {name}')


def _fails(out, ref, floor, what):
    with pytest.raises(AssertionError, match='beyond one bf16 ulp'):
        check_bf16(out, ref, floor=floor, min_equal=0.0, what=what)


# ------------------------------------------------------------------------------------------------ 1. + 2. convolutions
# (H, W, Cin, Cout, kinds, real Cin, real Cout): H x W the INPUT grid; kinds: plain | res | stats | stats_res | up | s2 | s2_stats | cols.
# The released layer lists at 1024^2 (latent grid 128 x 128), every distinct (H, W, Cin, Cout, kind) once.  FLUX decoder (AutoencoderKLDecoder:
# reversed 512/512/256/128; the <= 128-channel outputs that feed a GroupNorm take the statistics epilogue), FLUX encoder (kl_encoder_shapes), Qwen-Image
# dim 96 decoder (AutoencoderKLQwenImageDecoder: 384/384/192/96, 96 padded to 128, conv_out 3 padded to 8) and encoder (qwen_encoder_shapes: 32 moments).
FLUX_DEC = [(128, 128, 64, 512, ('plain',), 16, 512), (128, 128, 512, 512, ('plain', 'res', 'up'), 512, 512),
            (256, 256, 512, 512, ('plain', 'res', 'up'), 512, 512), (512, 512, 512, 256, ('plain',), 512, 256),
            (512, 512, 256, 256, ('plain', 'res', 'up'), 256, 256), (1024, 1024, 256, 128, ('stats',), 256, 128),
            (1024, 1024, 128, 128, ('stats', 'stats_res'), 128, 128), (1024, 1024, 128, 8, ('plain',), 128, 3)]
FLUX_ENC = [(1024, 1024, 3, 128, ('cols',), 3, 128), (1024, 1024, 128, 128, ('s2_stats',), 128, 128), (512, 512, 128, 256, ('plain',), 128, 256),
            (512, 512, 256, 256, ('s2',), 256, 256), (256, 256, 256, 512, ('plain',), 256, 512), (256, 256, 512, 512, ('s2',), 512, 512),
            (128, 128, 512, 32, ('plain',), 512, 32)]
QWEN_DEC = [(128, 128, 64, 384, ('plain',), 16, 384), (128, 128, 384, 384, ('plain', 'res'), 384, 384), (128, 128, 384, 192, ('up',), 384, 192),
            (256, 256, 192, 384, ('plain',), 192, 384), (256, 256, 384, 384, ('plain', 'res'), 384, 384), (256, 256, 384, 192, ('up',), 384, 192),
            (512, 512, 192, 192, ('plain', 'res'), 192, 192), (512, 512, 192, 128, ('up',), 192, 96), (1024, 1024, 128, 128, ('plain', 'res'), 96, 96)]
QWEN_ENC = [(1024, 1024, 128, 128, ('s2',), 96, 96), (512, 512, 128, 192, ('plain',), 96, 192), (512, 512, 192, 192, ('s2',), 192, 192),
            (256, 256, 384, 384, ('s2',), 384, 384), (128, 128, 384, 32, ('plain',), 384, 32)]
RAGGED = [(9, 13, 64, 72, ('plain', 'res', 'up'), 64, 72), (31, 33, 64, 128, ('plain', 'stats', 'up'), 64, 128),
          (300, 70, 64, 128, ('res', 'stats_res', 'up', 's2', 's2_stats'), 64, 128), (14, 62, 64, 128, ('plain', 'stats_res'), 64, 128),
          (18, 26, 64, 72, ('s2',), 64, 72), (62, 66, 128, 128, ('s2_stats',), 128, 128),
          (9, 13, 3, 72, ('cols',), 3, 72), (31, 33, 3, 128, ('cols',), 3, 96), (300, 70, 3, 64, ('cols',), 3, 64)]
REF_ROWS = 256       # the released grids keep their width (row pitch, border columns, tap shifts) and run REF_ROWS rows: see the module docstring, 1.
CONV_CASES = [(fam,) + ((min(c[0], REF_ROWS),) + c[1:] if fam != 'ragged' else c)
              for fam, cs in (('flux-dec', FLUX_DEC), ('flux-enc', FLUX_ENC), ('qwen-dec', QWEN_DEC), ('qwen-enc', QWEN_ENC), ('ragged', RAGGED)) for c in cs]


def _conv_operands(g, H, W, ci, co, cir, cor, k=3):
    x = torch.randn(H, W, ci, generator=g, device='cuda') * 1.2 + 0.1
    x[..., cir:] = 0
    wt = torch.randn(co, ci, k, k, generator=g, device='cuda') * (k * k * cir) ** -0.5
    wt[cor:] = 0
    wt[:, cir:] = 0
    b = torch.randn(co, generator=g, device='cuda') * 0.2
    b[cor:] = 0
    return x.bfloat16(), wt.bfloat16(), b.bfloat16()


def _w9(wt):
    co, ci = wt.shape[:2]
    return wt.permute(0, 2, 3, 1).reshape(co, 9 * ci).contiguous()


def _check_stats(slots, y, fl, groups, what):
    """slots [64, groups, 2] against fp64 sums over the interior of the fp64 convolution y [H, W, Cout] with per-element floor fl (module docstring, 2.)."""
    got = slots.sum(0)
    co = y.shape[-1]
    yg, fg = y.reshape(-1, groups, co // groups), fl.reshape(-1, groups, co // groups)
    s0, s1 = yg.sum((0, 2)), (yg * yg).sum((0, 2))
    b0 = fg.sum((0, 2)) + 36 * U32 * yg.abs().sum((0, 2))
    b1 = (2 * yg.abs() * fg + fg * fg).sum((0, 2)) + 37 * U32 * s1
    r0, r1 = ((got[:, 0] - s0).abs() / b0).max().item(), ((got[:, 1] - s1).abs() / b1).max().item()
    print(f'{what}: GroupNorm sums worst error / bound {r0:.4f} (sum), {r1:.4f} (sum of squares)')
    assert r0 <= 1 and r1 <= 1, (what, r0, r1)


@pytest.mark.parametrize('fam,H,W,ci,co,kinds,cir,cor', CONV_CASES, ids=[f'{c[0]}-{c[1]}x{c[2]}-{c[3]}-{c[4]}' for c in CONV_CASES])
def test_conv_vs_fp64(ops, lib, fam, H, W, ci, co, kinds, cir, cor):
    from arcflow_amd.vae import phase_weights, s2d_weights
    g = _gen(H * 31 + W * 7 + ci + co)
    assert lib.afx_conv_stats_available() == 1
    for kind in kinds:
        what = f'{fam} {kind} {H}x{W} {ci}->{co}'
        if kind == 'cols':
            _conv_in_case(ops, lib, g, H, W, co, cor, what)
            continue
        x, wt, b = _conv_operands(g, H, W, ci, co, cir, cor)
        gx = _in_grid(x)
        xp = _view(gx)
        s2, up = kind.startswith('s2'), kind == 'up'
        Ho, Wo = (H // 2, W // 2) if s2 else (2 * H, 2 * W) if up else (H, W)
        groups = 32 if co % 32 == 0 and co // 32 >= 4 else 16
        slots = torch.full((64, groups, 2), 7.0, dtype=torch.float64, device='cuda') if 'stats' in kind else None     # the call zeroes it
        r = (torch.randn(Ho, Wo, co, generator=g, device='cuda')).bfloat16() if kind.endswith('res') else None
        if r is not None:
            r[..., cor:] = 0
        gr = _in_grid(r) if r is not None else None
        # ---- reference
        if up:
            w4 = phase_weights(_w9(wt), ci)
            w4k = w4.view(4, co, 2, 2, ci).permute(0, 1, 4, 2, 3)
            y = torch.empty(Ho, Wo, co, dtype=torch.float64, device='cuda')
            fl = torch.empty_like(y)
            for ph in range(4):
                y[ph >> 1::2, ph & 1::2], _, fl[ph >> 1::2, ph & 1::2] = conv64(xp, w4k[ph], b, H, W, oy=ph >> 1, ox=ph & 1)
        elif s2:
            y, mag, _ = conv64(xp, wt, b, Ho, Wo, stride=2, oy=1, ox=1)
            fl = (36 * ci // 32 + 33) * U32 * mag
        else:
            y, _, fl = conv64(xp, wt, b, H, W)
        ref, flr = y, fl
        if r is not None:
            ref = y + r.double()
            flr = fl + 2 * U32 * (y.abs() + r.double().abs())
        # ---- the kernel
        modes = [(3, 0), (2, 0)] if kind in ('plain', 'res') else [(3, 0)]
        try:
            for mode in modes:
                ops.set_gemm_mode(*mode)
                gy = _out_grid(Ho, Wo, co)
                if up:
                    _ok(lib.afx_upconv3x3_bf16(_p(gx.t), _p(w4), _p(b), _p(gy.t), H, W, ci, co, _s()))
                elif s2:
                    gw = _out_grid(Ho, Wo, 4 * ci)
                    _ok(lib.afx_conv3x3s2_bf16(_p(gx.t), _p(s2d_weights(wt.float().cpu(), ci, co).bfloat16().cuda()), _p(b), _p(gy.t), _p(gw.t), H, W,
                                               ci, co, _p(slots), groups if slots is not None else 0, _s()))
                elif slots is not None:
                    _ok(lib.afx_conv3x3_bf16_stats(_p(gx.t), _p(_w9(wt)), _p(b), _p(gy.t), H, W, ci, co, _p(gr.t) if gr else None, _p(slots), groups, _s()))
                else:
                    _ok(lib.afx_conv3x3_bf16(_p(gx.t), _p(_w9(wt)), _p(b), _p(gy.t), H, W, ci, co, _p(gr.t) if gr else None, _s()))
                torch.cuda.synchronize()
                _check_grid(gy, ref, flr, f'{what} mode={mode}')
                if cor < co:
                    assert not bool(_view(gy)[..., cor:].any()), f'{what}: padded output channels are not zero'
                if s2:                                   # the space-to-depth pass, exact: cell (Y, X), channel (2 py + px) Cin + c = x[2Y + py][2X + px][c]
                    _border_zero(gw, f'{what} ws')
                    _guards_intact(gw, f'{what} ws')
                    want = x.view(Ho, 2, Wo, 2, ci).permute(0, 2, 1, 3, 4).reshape(Ho, Wo, 4 * ci)
                    assert torch.equal(_view(gw)[1:-1, 1:-1], want), f'{what}: space-to-depth grid'
                if slots is not None:
                    _check_stats(slots, ref, flr, groups, what)
            if kind == 'plain':                          # the kernels that exist in the default mode only answer with a status on the 8-phase kernel
                ops.set_gemm_mode(2, 0)
                assert lib.afx_conv_stats_available() == 0
                gz = _out_grid(2 * H, 2 * W, co) if H * W <= 300 * 70 else None
                st = torch.zeros(64, groups, 2, dtype=torch.float64, device='cuda')
                if gz is not None:
                    assert lib.afx_upconv3x3_bf16(_p(gx.t), _p(phase_weights(_w9(wt), ci)), _p(b), _p(gz.t), H, W, ci, co, _s()) != 0
                if co in (64, 128):                      # shapes the default mode takes (co % groups == 0, 4 or 8 channels per group): only the mode can refuse
                    go = _out_grid(H, W, co)
                    assert lib.afx_conv3x3_bf16_stats(_p(gx.t), _p(_w9(wt)), _p(b), _p(go.t), H, W, ci, co, None, _p(st), groups, _s()) != 0
        finally:
            ops.set_gemm_mode(3, 0)
        # ---- teeth, on the default mode's output for the stats / up / s2 kinds and on the 8-phase kernel's for plain / res
        out = _view(gy)[1:-1, 1:-1]
        if up:
            m = ref.clone()
            m[1::2, 1::2] -= conv64(xp, w4k[3][:, :, 0:1, 1:2], None, H, W, oy=1, ox=2)[0]
        elif s2:
            m = ref - conv64(xp, wt[:, :, 1:2, 1:2], None, Ho, Wo, stride=2, oy=2, ox=2)[0]
        else:
            m = ref - conv64(xp, wt[:, :, 1:2, 1:2], None, H, W, oy=1, ox=1)[0]
        _fails(out, m, flr, f'{what}: one tap left out')
        del m
        if up:
            m = ref.clone()
            for ph in range(4):
                m[ph >> 1::2, ph & 1::2] -= conv64(xp[..., ci - 64:], w4k[ph][:, ci - 64:], None, H, W, oy=ph >> 1, ox=ph & 1)[0]
        elif s2:
            m = ref - conv64(xp[..., ci - 64:], wt[:, ci - 64:], None, Ho, Wo, stride=2, oy=1, ox=1)[0]
        else:
            m = ref - conv64(xp[..., ci - 64:], wt[:, ci - 64:], None, H, W)[0]
        _fails(out, m, flr, f'{what}: the last 64-channel chunk left out')
        del m
        if s2:
            xm = xp[H - 1:H + 2].clone()
            xm[2] = xm[1]                                # the padded row H read as row H - 1
            m = ref.clone()
            m[-1] = conv64(xm, wt, b, 1, Wo, stride=2, oy=0, ox=1)[0][0]
            _fails(out, m, flr, f'{what}: the padded row read as row H - 1')
        del gy, ref, flr, y, fl
        torch.cuda.empty_cache()


def _conv_in_case(ops, lib, g, H, W, co, cor, what):
    """afx_image_to_cols27 (layout exact, all 64 columns) + the K = 64 GEMM against conv64 of the bf16 image."""
    from arcflow_amd.vae import conv_in_weights
    cop = (co + 63) // 64 * 64
    img = torch.rand(3, H, W, generator=g, device='cuda') * 2 - 1
    wt = (torch.randn(co, 3, 3, 3, generator=g, device='cuda') * 0.2)
    b = torch.randn(co, generator=g, device='cuda') * 0.2
    wt[cor:] = 0
    b[cor:] = 0
    wt, b = wt.bfloat16(), b.bfloat16()
    cols, gy = _out_grid(H, W, 64), _out_grid(H, W, cop)
    _ok(lib.afx_image_to_cols27(_p(img), 0, _p(cols.t), H, W, 0, _s()))
    wm = conv_in_weights(wt.float().cpu(), b.float().cpu(), cop).bfloat16().cuda()
    ops.linear(cols.t, wm, None, out=gy.t)
    torch.cuda.synchronize()
    _border_zero(cols, f'{what} cols')
    _guards_intact(cols, f'{what} cols')
    xb = img.bfloat16().permute(1, 2, 0)
    xp = torch.zeros(H + 2, W + 2, 3, dtype=torch.bfloat16, device='cuda')
    xp[1:-1, 1:-1] = xb
    want = torch.zeros(H, W, 64, dtype=torch.bfloat16, device='cuda')
    for t in range(9):
        want[..., 3 * t:3 * t + 3] = xp[t // 3:t // 3 + H, t % 3:t % 3 + W]
    want[..., 27] = 1
    assert torch.equal(_view(cols)[1:-1, 1:-1], want), f'{what}: column layout'
    y, _, fl = conv64(xp, wt, b, H, W)
    fl = fl * ((64 // 32 + 33) / (27 // 32 + 33))         # the GEMM runs K = 64
    ref, flr = torch.zeros(H, W, cop, dtype=torch.float64, device='cuda'), torch.zeros(H, W, cop, dtype=torch.float64, device='cuda')
    ref[..., :co], flr[..., :co] = y, fl
    _check_grid(gy, ref, flr, what)
    assert not bool(_view(gy)[..., cor:].any()), f'{what}: padded output channels are not zero'
    out = _view(gy)[1:-1, 1:-1]
    m = ref.clone()
    m[..., :co] -= conv64(xp, wt[:, :, 1:2, 1:2], None, H, W, oy=1, ox=1)[0]
    _fails(out, m, flr, f'{what}: one tap left out')


STAT_CASES = [(31, 33, 64, 128, 32, False, False), (300, 70, 64, 128, 16, True, False), (9, 13, 128, 128, 8, True, False),
              (300, 70, 128, 64, 16, False, False), (20, 17, 64, 64, 8, True, False), (64, 48, 64, 64, 4, False, False),
              (300, 70, 64, 128, 32, False, True), (62, 66, 64, 64, 4, False, True)]


@pytest.mark.parametrize('H,W,ci,co,groups,with_res,s2', STAT_CASES)
def test_epilogue_groupnorm_sums_vs_fp64_convolution(lib, H, W, ci, co, groups, with_res, s2):
    """Channels per group 4 / 8 / 16 at Cout 128 and 64, with and without the residual, and the stride-2 route (4 and 16): the sums against the fp64
    convolution (the per-element check of the stored grid is test_conv_vs_fp64's)."""
    from arcflow_amd.vae import s2d_weights
    g = _gen(H * W + co + groups)
    x, wt, b = _conv_operands(g, H, W, ci, co, ci, co)
    gx = _in_grid(x)
    Ho, Wo = (H // 2, W // 2) if s2 else (H, W)
    r = torch.randn(Ho, Wo, co, generator=g, device='cuda').bfloat16() if with_res else None
    gr = _in_grid(r) if with_res else None
    gy = _out_grid(Ho, Wo, co)
    slots = torch.full((64, groups, 2), 7.0, dtype=torch.float64, device='cuda')
    if s2:
        gw = _out_grid(Ho, Wo, 4 * ci)
        _ok(lib.afx_conv3x3s2_bf16(_p(gx.t), _p(s2d_weights(wt.float().cpu(), ci, co).bfloat16().cuda()), _p(b), _p(gy.t), _p(gw.t), H, W, ci, co,
                                   _p(slots), groups, _s()))
        y, mag, _ = conv64(_view(gx), wt, b, Ho, Wo, stride=2, oy=1, ox=1)
        fl = (36 * ci // 32 + 33) * U32 * mag
    else:
        _ok(lib.afx_conv3x3_bf16_stats(_p(gx.t), _p(_w9(wt)), _p(b), _p(gy.t), H, W, ci, co, _p(gr.t) if gr else None, _p(slots), groups, _s()))
        y, _, fl = conv64(_view(gx), wt, b, H, W)
    if with_res:
        fl = fl + 2 * U32 * (y.abs() + r.double().abs())
        y = y + r.double()
    torch.cuda.synchronize()
    what = f'stats {H}x{W} {ci}->{co} groups {groups} res={with_res} s2={s2}'
    _check_grid(gy, y, fl, what)
    _check_stats(slots, y, fl, groups, what)


# ------------------------------------------------------------------------------------------------ 3. GroupNorm apply
def _gn_depth(rows, Cn, groups):
    rstep = 256 // (Cn // 8)
    blocks = min(2048, -(-rows // rstep))
    return 4 * -(-rows // (blocks * rstep)) + 1


def _gn_ref(x, groups, gamma, beta, act, depth, eps=1e-6, count_rows=None, shift_channel=None):
    """x [H, W, C] bf16 -> the fp64 GroupNorm(+SiLU) of the interior and the floor of the module docstring (3.)."""
    H, W, Cn = x.shape
    gs = Cn // groups
    xd = x.double()
    gi = torch.arange(Cn, device='cuda') // gs
    if shift_channel is not None:
        gi[shift_channel] = (gi[shift_channel] + 1) % groups
    n = (count_rows if count_rows is not None else H * W) * gs
    oh = torch.zeros(Cn, groups, dtype=torch.float64, device='cuda')
    oh[torch.arange(Cn, device='cuda'), gi] = 1
    mean = (xd.sum((0, 1)) @ oh) / n
    var = ((xd - (oh @ mean)) ** 2).sum((0, 1)) @ oh / n
    if count_rows is not None:                            # the mutated reference: sums over the interior, divided by the padded count
        var = (xd * xd).sum((0, 1)) @ oh / n - mean * mean
    e1, e2 = (xd.abs().sum((0, 1)) @ oh) / n, ((xd * xd).sum((0, 1)) @ oh) / n
    dmean = depth * U32 * e1
    dvar = (depth + 1) * U32 * e2 + 2 * mean.abs() * dmean
    a = torch.rsqrt(var + eps)
    a_hi = torch.rsqrt((var - dvar).clamp_min(0) + eps) * (1 + 4 * U32)
    a_lo = torch.rsqrt(var + dvar + eps) * (1 - 4 * U32)
    da = torch.maximum(a_hi - a, a - a_lo)
    gm, bt = gamma.double(), beta.double()
    mc, ac, dac, ahc, dmc = oh @ mean, (oh @ a) * gm, (oh @ da) * gm.abs(), (oh @ a_hi) * gm.abs(), oh @ dmean
    t = (xd - mc) * ac + bt
    fl = dac * (xd - mc).abs() + ahc * dmc + 3 * U32 * (xd.abs() * ahc + mc.abs() * ahc + bt.abs())
    if act:
        fl = 1.1 * fl + (t.abs() + 8) * U32 * silu64(t).abs()
        t = silu64(t)
    return t, fl


def _gn_run(lib, x, groups, gamma, beta, act, from_stats):
    H, W, Cn = x.shape
    gx, gy = _in_grid(x), _out_grid(H, W, Cn)
    ws = torch.zeros(lib.afx_groupnorm_ws_bytes(Cn, groups) // 8, dtype=torch.float64, device='cuda')
    if from_stats:                                        # exact fp64 sums of the grid, spread over the 64 slots
        xg = x.double().reshape(-1, groups, Cn // groups)
        tot = torch.stack([xg.sum((0, 2)), (xg * xg).sum((0, 2))], 1)
        frac = torch.rand(64, 1, 1, dtype=torch.float64, device='cuda')
        slots = (tot[None] * frac / frac.sum()).contiguous()
        _ok(lib.afx_groupnorm_nhwc_from_stats(_p(gx.t), _p(gy.t), _p(slots), _p(ws), H, W, Cn, groups, _p(gamma), _p(beta), 1e-6, act, _s()))
    else:
        _ok(lib.afx_groupnorm_nhwc(_p(gx.t), _p(gy.t), _p(ws), H, W, Cn, groups, _p(gamma), _p(beta), 1e-6, act, _s()))
    torch.cuda.synchronize()
    return gy


def _gn_input(g, H, W, Cn):
    x = torch.randn(H, W, Cn, generator=g, device='cuda') + 3.0 * torch.randn(Cn, generator=g, device='cuda')       # channel means of order 3 sigma
    gamma, beta = torch.randn(Cn, generator=g, device='cuda'), torch.randn(Cn, generator=g, device='cuda')
    return x.bfloat16(), gamma, beta


GN_CASES = [(9, 13, 64, 16), (300, 70, 64, 16), (9, 13, 128, 32), (300, 70, 128, 32), (300, 70, 128, 16), (512, 512, 128, 32), (1024, 1024, 128, 32),
            (300, 70, 256, 32), (31, 33, 256, 16), (300, 70, 512, 32), (128, 128, 512, 32), (31, 33, 512, 16)]


@pytest.mark.parametrize('act', [0, 1])
@pytest.mark.parametrize('H,W,Cn,groups', GN_CASES)
def test_groupnorm_vs_fp64(lib, H, W, Cn, groups, act):
    """afx_groupnorm_nhwc and afx_groupnorm_nhwc_from_stats: channels per group 4 (two groups in one 16-byte chunk), 8, 16 and 32.  (Two channels per
    group, C = 64 with 32 groups, is refused by afx_groupnorm_nhwc -- asserted -- and run through afx_groupnorm_nhwc_from_stats.)"""
    g = _gen(H + W + Cn + groups + act)
    x, gamma, beta = _gn_input(g, H, W, Cn)
    if Cn == 64:
        gx = _in_grid(x)
        ws = torch.zeros(lib.afx_groupnorm_ws_bytes(Cn, 32) // 8, dtype=torch.float64, device='cuda')
        assert lib.afx_groupnorm_nhwc(_p(gx.t), _p(gx.t), _p(ws), H, W, Cn, 32, _p(gamma), _p(beta), 1e-6, act, _s()) != 0
    depth = _gn_depth((H + 2) * (W + 2), Cn, groups)
    runs = [(groups, False), (groups, True)] + ([(32, True)] if Cn == 64 else [])      # two channels per group: afx_groupnorm_nhwc_from_stats takes them
    for ng, from_stats in runs:
        what = f'groupnorm{"_from_stats" if from_stats else ""} {H}x{W} C={Cn} groups={ng} act={act} depth={0 if from_stats else depth}'
        gy = _gn_run(lib, x, ng, gamma, beta, act, from_stats)
        ref, fl = _gn_ref(x, ng, gamma, beta, act, 0 if from_stats else depth)
        _check_grid(gy, ref, fl, what)
        out = _view(gy)[1:-1, 1:-1]
        _fails(out, _gn_ref(x, ng, gamma, beta, act, 0, count_rows=(H + 2) * (W + 2))[0], fl, f'{what}: count = (H + 2)(W + 2)')
        _fails(out, _gn_ref(x, ng, gamma, beta, act, 0, shift_channel=Cn // 2)[0], fl, f'{what}: one channel in the wrong group')


@pytest.mark.parametrize('H,W,Cn,groups', [(64, 64, 128, 16), (300, 70, 128, 32), (128, 128, 512, 32)])
def test_groupnorm_statistics_are_bit_reproducible(lib, H, W, Cn, groups):
    """afx_groupnorm_nhwc on the same grid, eight times: the slot sums, the coefficients and the output are the same bits every time (gn_stats_kernel adds
    a block's lanes in a fixed order; with fp32 LDS atomics there the sums followed the order the waves arrived in, and two decodes of one latent differed
    in the last bit -- tests/test_vae_encoder.py::test_pipeline_round_trip_encode_decode)."""
    g = _gen(H + W + Cn)
    x, gamma, beta = _gn_input(g, H, W, Cn)
    gx = _in_grid(x)
    first = None
    for _ in range(8):
        gy = _out_grid(H, W, Cn)
        ws = torch.zeros(lib.afx_groupnorm_ws_bytes(Cn, groups) // 8, dtype=torch.float64, device='cuda')
        _ok(lib.afx_groupnorm_nhwc(_p(gx.t), _p(gy.t), _p(ws), H, W, Cn, groups, _p(gamma), _p(beta), 1e-6, 1, _s()))
        torch.cuda.synchronize()
        got = (ws.view(torch.int64).clone(), gy.t.view(torch.int16).clone())
        if first is None:
            first = got
        assert torch.equal(got[0], first[0]), 'the statistics scratch (slot sums / coefficients) differs between two runs'
        assert torch.equal(got[1], first[1]), 'the output differs between two runs'


def test_groupnorm_constant_group_is_finite_and_beta(lib):
    """One group (4 channels) of the 1024 x 1024 x 128 grid holds the bf16 constant 9.9375 everywhere, the others are random: its true variance is 0, so
    the fp32 partial sums decide the sign of s1 / n - mean^2, and eps = 1e-6 is far below their error bound.  The output must be finite and equal beta
    within the floor (da |x - mean| = 0 there).  Measured figures and the fix: DESIGN.md section 7."""
    H = W = 1024
    Cn, groups = 128, 32
    g = _gen(77)
    x, gamma, beta = _gn_input(g, H, W, Cn)
    x[..., 20:24] = 9.9375
    depth = _gn_depth((H + 2) * (W + 2), Cn, groups)
    for act in (0, 1):
        gy = _gn_run(lib, x, groups, gamma, beta, act, False)
        out = _view(gy)[1:-1, 1:-1]
        ref, fl = _gn_ref(x, groups, gamma, beta, act, depth)
        want = beta.double()[20:24] if not act else silu64(beta.double()[20:24])
        assert bool((ref[..., 20:24] == want).all())
        dev = (out[..., 20:24].double() - want).abs().amax((0, 1))
        print(f'constant group act={act}: finite {bool(torch.isfinite(out.float()).all())}, |out - beta| {dev.tolist()}, floor {fl[0, 0, 20:24].tolist()}, '
              f'|gamma| {gamma[20:24].abs().tolist()}')
        _check_grid(gy, ref, fl, f'groupnorm constant group act={act}')


# ------------------------------------------------------------------------------------------------ 4. softmax and the attention chain
def _softmax_ref(s, scale, depth):
    t = (s.double() - s.double().amax(-1, keepdim=True)) * scale
    p = torch.softmax(t, -1)
    c = depth + 16 + 3.5 * (p * t.abs()).sum(-1, keepdim=True)
    return p, c * U32 * (1 + t.abs()) * p


def _check_p(out, ref, fl, what, min_equal=0.99):
    _report(out, ref, fl, what)
    check_bf16(out, ref, floor=fl, min_equal=min_equal, what=what)


def _attn_weights(g, Cn):
    """to_q | to_k | to_v stacked and to_out with the scale of the oracle's weight generator (oracle/vae_ref.py: N(0, 1 / C), bias 0.05)."""
    w = lambda n: (torch.randn(n, Cn, generator=g, device='cuda') * Cn ** -0.5).bfloat16()       # noqa: E731
    b = lambda n: (torch.randn(n, generator=g, device='cuda') * 0.05).bfloat16()                 # noqa: E731
    return w(3 * Cn), b(3 * Cn), w(Cn), b(Cn)


@pytest.fixture(scope='module')
def logit_std(ops):
    """Standard deviation of the UNSCALED logits q k^T of the mid-block (C = 512) on a normalised input with the weights of the attention chain test
    below: what _single_head_attention hands to the softmax."""
    g = _gen(5)
    w_qkv, b_qkv, _, _ = _attn_weights(g, 512)
    xn = torch.randn(1024, 512, generator=g, device='cuda').bfloat16()
    qkv = ops.linear(xn, w_qkv, b_qkv)
    s = ops.linear_f32out(qkv[:, :512], qkv[:, 512:1024])
    sd = s.std().item()
    print(f'mid-block logits (oracle weights, C = 512): std {sd:.3f} unscaled, {sd * 512 ** -0.5:.4f} scaled, row max - mean {(s.amax(-1) - s.mean(-1)).mean().item():.3f}')
    return sd


@pytest.mark.parametrize('rows,cols,lds,ldp', [(7, 64, 64, 64), (5, 1000, 1000, 1024), (3, 16384, 16384, 16384), (4, 1023, 1024, 1024), (2, 20000, 20000, 20000),
                                               (5, 1000, 1001, 1024), (5, 1000, 1000, 1022), (130, 16384, 16384 + 64, 16384 + 64)])
def test_softmax_rows_vs_fp64(lib, logit_std, rows, cols, lds, ldp):
    """Register kernel (cols % 4 == 0, <= 16384, aligned leading dimensions) and the three-pass kernel (1023 and 20000 columns, lds = 1001, ldp = 1022),
    strided input and output; columns >= cols and rows >= rows of the output keep their sentinel."""
    reg = cols % 4 == 0 and cols <= 16384 and lds % 4 == 0 and ldp % 4 == 0
    depth = 73 if reg else -(-cols // 256) + 9
    scale = 512 ** -0.5
    for spread in (logit_std, 4 * logit_std, 2.0 / scale):
        g = _gen(rows * cols + int(spread))
        sbuf = torch.full((rows + 2, lds), 1e30, device='cuda')
        s = sbuf[:rows, :cols]
        s.copy_(torch.randn(rows, cols, generator=g, device='cuda') * spread)
        pbuf = torch.full((rows + 2, ldp + 8), SENT, dtype=torch.bfloat16, device='cuda')
        pflat = pbuf.view(-1)[:(rows + 2) * ldp].view(rows + 2, ldp)
        _ok(lib.afx_softmax_rows_f32(_p(sbuf), lds, _p(pflat), ldp, rows, cols, scale, _s()))
        torch.cuda.synchronize()
        what = f'softmax {rows}x{cols} lds={lds} ldp={ldp} {"register" if reg else "three-pass"} kernel, logit std {spread:.2f}'
        assert bool((pflat[:rows, cols:] == SENT).all()) and bool((pflat[rows:] == SENT).all()) and bool((pbuf.view(-1)[(rows + 2) * ldp:] == SENT).all()), \
            f'{what}: a write outside [rows, cols]'
        ref, fl = _softmax_ref(s, scale, depth)
        _check_p(pflat[:rows, :cols], ref, fl, what)
        # the stored row sums to 1 within what the elements may carry: half a bf16 ulp of rounding each (nearest) + the floor.  (A peaked row is one
        # element near 1/2 .. 1, whose half ulp alone is 2^-9 .. 2^-8: no fixed small figure holds.)
        rowdev = ((pflat[:rows, :cols].double().sum(-1) - 1).abs() / (0.5 * bf16_ulp(ref) + fl).sum(-1)).max().item()
        print(f'{what}: worst |row sum - 1| / bound {rowdev:.3f}')
        assert rowdev <= 1, (what, rowdev)
        _fails(pflat[:rows, :cols], _softmax_ref(s, scale * 1.02, depth)[0], fl, f'{what}: scale off by 2 %')


@pytest.mark.parametrize('H,W', [(128, 128), (35, 29)])
def test_single_head_attention_stage_by_stage(ops, lib, monkeypatch, H, W):
    """The mid-block chain of both decoders and encoders at C = 512: N = 16384 (1024^2) and N = 1015 (padded to 1024 keys)."""
    from arcflow_amd import vae
    Cn, N = 512, H * W
    Np = (N + 63) // 64 * 64
    g = _gen(N)
    w_qkv, b_qkv, w_out, b_out = _attn_weights(g, Cn)
    x = (torch.randn(H, W, Cn, generator=g, device='cuda') * 1.5).bfloat16()
    xn = torch.randn(H, W, Cn, generator=g, device='cuda').bfloat16()
    gx, gxn = _in_grid(x), _in_grid(xn)
    rec = {'linear': [], 'f32': []}
    lin, f32o = ops.linear, ops.linear_f32out

    def rec_linear(a_, w_, b_=None, **kw):
        out = lin(a_, w_, b_, **kw)
        rec['linear'].append((a_, w_, b_, out))
        return out

    def rec_f32(a_, w_, **kw):
        out = f32o(a_, w_, **kw)
        rec['f32'].append((a_, w_, out))
        return out

    monkeypatch.setattr(vae.ops, 'linear', rec_linear)
    monkeypatch.setattr(vae.ops, 'linear_f32out', rec_f32)
    scale = Cn ** -0.5
    gy = vae._single_head_attention(lib, gxn, gx, w_qkv, b_qkv, w_out, b_out, scale)
    torch.cuda.synchronize()
    monkeypatch.undo()
    (xc, _, _, qkv), (pm, vT, _, o), (o_in, _, _, oc) = rec['linear']
    (q, k, s), = rec['f32']
    what = f'attention N={N}'
    # gather: bit-exact, padded rows zero
    assert xc.shape == (Np, Cn) and torch.equal(xc[:N], xn.reshape(N, Cn)) and not bool(xc[N:].any()), f'{what}: gather'
    # qkv
    y, fl = proj64(xc, w_qkv, b_qkv)
    _check_p(qkv, y, fl, f'{what} qkv')
    _fails(qkv, y - xc[:, -1:].double() * w_qkv[:, -1].double()[None], fl, f'{what} qkv: one K column dropped')
    # logits: fp32, proj64's floor + the store's own rounding
    assert q.data_ptr() == qkv.data_ptr() and s.shape == (Np, Np)
    worst = 0.0
    for r0 in range(0, Np, 4096):                             # (the fp64 product of 16384 x 16384 logits in four row blocks)
        rows = slice(r0, min(Np, r0 + 4096))
        y, fl = proj64(q[rows], k, None)
        worst = max(worst, ((s[rows].double() - y).abs() / fl).max().item())
        check_f32(s[rows], y, fl, f'{what} logits')
        if r0 == 0:
            with pytest.raises(AssertionError):
                check_f32(s[rows], y - q[rows, -1:].double() * k[:, -1].double()[None], fl, f'{what} logits: one K column dropped')
    print(f'{what} logits: worst error / bound {worst:.3f}, scaled std {s[:N, :N].std().item() * scale:.3f}')
    # P: softmax over the N real keys of the kernel's own logits; padded keys and rows stay zero
    assert pm.shape == (Np, Np) and not bool(pm[N:].any()) and not bool(pm[:, N:].any()), f'{what}: P of padded keys / rows'
    for r0 in range(0, N, 4096):
        rows = slice(r0, min(N, r0 + 4096))
        ref, fl = _softmax_ref(s[rows, :N], scale, 73)
        _check_p(pm[rows, :N], ref, fl, f'{what} P rows {r0}+')
        if Np != N and r0 == 0:
            _fails(pm[rows, :N], _softmax_ref(s[rows], scale, 73)[0][:, :N], fl, f'{what} P: padded keys included')
    # PV and the projection
    assert torch.equal(vT[:, :Np], qkv[:, 2 * Cn:].T)
    y, fl = proj64(pm, vT, None)
    _check_p(o, y, fl, f'{what} PV')
    y, fl = proj64(o_in, w_out, b_out)
    _check_p(oc, y, fl, f'{what} projection')
    # scatter + residual: RNE of the fp32 sum, border zero
    want = (oc[:N].float() + x.reshape(N, Cn).float()).bfloat16().view(H, W, Cn)
    assert torch.equal(_view(gy)[1:-1, 1:-1], want), f'{what}: scatter + residual'
    _border_zero(gy, what)


# ------------------------------------------------------------------------------------------------ 5. layout kernels
@pytest.mark.parametrize('H,W,Cn,creal', [(9, 13, 64, 64), (8, 6, 128, 96), (31, 34, 512, 512), (300, 70, 128, 96)])
def test_layout_kernels_exact(lib, H, W, Cn, creal):
    g = _gen(H * W + Cn)
    x = torch.randn(H, W, Cn, generator=g, device='cuda').bfloat16()
    x[..., creal:] = 0
    gx = _in_grid(x)
    # nearest 2x upsample
    gu = _out_grid(2 * H, 2 * W, Cn)
    _ok(lib.afx_upsample2x_nhwc(_p(gx.t), _p(gu.t), H, W, Cn, _s()))
    torch.cuda.synchronize()
    _border_zero(gu, 'upsample2x')
    _guards_intact(gu, 'upsample2x')
    assert torch.equal(_view(gu)[1:-1, 1:-1], x.repeat_interleave(2, 0).repeat_interleave(2, 1))
    # interior gather (rows beyond H W of the compact buffer untouched)
    comp = torch.full((H * W + 5, Cn), SENT, dtype=torch.bfloat16, device='cuda')
    _ok(lib.afx_interior_nhwc(_p(gx.t), _p(comp), None, H, W, Cn, 0, _s()))
    torch.cuda.synchronize()
    assert torch.equal(comp[:H * W], x.reshape(H * W, Cn)) and bool((comp[H * W:] == SENT).all())
    # interior scatter without and with the residual: the kernel writes the interior only (callers hand it a zeroed grid)
    c2 = torch.randn(H * W, Cn, generator=g, device='cuda').bfloat16()
    for res in (None, gx):
        gs = _out_grid(H, W, Cn)
        gs.t.fill_(SENT)
        _ok(lib.afx_interior_nhwc(_p(gs.t), _p(c2), _p(res.t) if res is not None else None, H, W, Cn, 1, _s()))
        torch.cuda.synchronize()
        v = _view(gs)
        want = c2.view(H, W, Cn) if res is None else (c2.view(H, W, Cn).float() + x.float()).bfloat16()
        assert torch.equal(v[1:-1, 1:-1], want)
        assert all(bool((b == SENT).all()) for b in (v[0], v[-1], v[:, 0], v[:, -1]))
        _guards_intact(gs, 'interior scatter')
    # grid -> image
    img = torch.full((3 * H * W + 7,), SENT, device='cuda')
    _ok(lib.afx_nhwc_to_image(_p(gx.t), _p(img), H, W, Cn, _s()))
    torch.cuda.synchronize()
    assert torch.equal(img[:3 * H * W].view(3, H, W), x[..., :3].float().permute(2, 0, 1)) and bool((img[3 * H * W:] == SENT).all())


def _rne_or_neighbour(out, v64, e, what):
    lo, hi, want = (v64 - e).float().bfloat16(), (v64 + e).float().bfloat16(), v64.float().bfloat16()
    sure = lo == hi
    assert torch.equal(out[sure], want[sure]), f'{what}: {int((out[sure] != want[sure]).sum())} elements off RNE of the fp64 map'
    # elsewhere out = RNE(some value within e of v): rounding is monotone, so it lies between RNE(v - e) and RNE(v + e) (where the map cancels to a v far
    # below e, those two are more than one bf16 step apart)
    assert bool(((out.float() >= lo.float()) & (out.float() <= hi.float()))[~sure].all()), f'{what}: an element is outside [RNE(v - e), RNE(v + e)]'
    unsure = 1 - sure.double().mean().item()
    print(f'{what}: {unsure:.5f} of the elements within the fp32 error of a bf16 rounding boundary, '
          f'{(out != want).double().mean().item():.5f} differ from RNE(fp64)')
    assert unsure <= 0.02, f'{what}: the window e leaves {unsure:.4f} of the elements undecided (module docstring, 5.)'


@pytest.mark.parametrize('hp,wp,Cn', [(4, 4, 64), (3, 5, 64), (64, 64, 64), (5, 2, 128)])
def test_latent_unpack_kernels(lib, hp, wp, Cn):
    g = _gen(hp * wp + Cn)
    tok = torch.randn(hp * wp, 64, generator=g, device='cuda')
    H, W = 2 * hp, 2 * wp
    lat = tok.view(hp, wp, 16, 2, 2).permute(0, 3, 1, 4, 2).reshape(H, W, 16).double()          # channel c * 4 + ph * 2 + pw
    sf, sh = 0.3611, 0.1159
    inv, shf = (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(sf, dtype=torch.float32)).double().item(), float(torch.tensor(sh, dtype=torch.float32))
    A, b = torch.randn(16, 16, generator=g, device='cuda') * 0.4, torch.randn(16, generator=g, device='cuda')
    for name in ('latent_to_nhwc', 'latent_to_nhwc_affine'):
        gy = _out_grid(H, W, Cn)
        if name == 'latent_to_nhwc':
            _ok(lib.afx_latent_to_nhwc(_p(tok), _p(gy.t), hp, wp, Cn, sf, sh, _s()))
            v = lat * inv + shf
            e = 2 * U32 * ((lat * inv).abs() + abs(shf))
        else:
            _ok(lib.afx_latent_to_nhwc_affine(_p(tok), _p(gy.t), hp, wp, Cn, _p(A), _p(b), _s()))
            v = lat @ A.double().T + b.double()
            e = 18 * U32 * (lat.abs() @ A.double().abs().T + b.double().abs())
        torch.cuda.synchronize()
        _border_zero(gy, name)
        _guards_intact(gy, name)
        out = _view(gy)[1:-1, 1:-1]
        assert not bool(out[..., 16:].any()), f'{name}: channels >= 16 are not zero'
        _rne_or_neighbour(out[..., :16], v, e, f'{name} {hp}x{wp} C={Cn}')
        _fails(out[..., :16], torch.roll(v, 1, -1), e, f'{name}: channels rotated')


@pytest.mark.parametrize('from01,dt', [(0, torch.float32), (1, torch.float32), (0, torch.bfloat16), (1, torch.bfloat16)])
@pytest.mark.parametrize('H,W', [(9, 13), (8, 6), (300, 70)])
def test_image_to_cols27_layout_exact(lib, H, W, from01, dt):
    """All 64 columns: k = (3 dy + dx) * 3 + channel (zero outside the image), the constant 1 in column 27, zeros above; border rows all zero."""
    g = _gen(H * W + from01)
    img = (torch.rand(3, H, W, generator=g, device='cuda') if from01 else torch.rand(3, H, W, generator=g, device='cuda') * 2 - 1).to(dt)
    cols = _out_grid(H, W, 64)
    _ok(lib.afx_image_to_cols27(_p(img), int(dt == torch.bfloat16), _p(cols.t), H, W, from01, _s()))
    torch.cuda.synchronize()
    _border_zero(cols, 'cols27')
    _guards_intact(cols, 'cols27')
    v = img.float() * 2.0 - 1.0 if from01 else img.float()              # the kernel's fp32 map, one rounding (2 v is exact)
    xp = torch.zeros(H + 2, W + 2, 3, dtype=torch.bfloat16, device='cuda')
    xp[1:-1, 1:-1] = v.bfloat16().permute(1, 2, 0)
    want = torch.zeros(H, W, 64, dtype=torch.bfloat16, device='cuda')
    for t in range(9):
        want[..., 3 * t:3 * t + 3] = xp[t // 3:t // 3 + H, t % 3:t % 3 + W]
    want[..., 27] = 1
    assert torch.equal(_view(cols)[1:-1, 1:-1], want)


# ------------------------------------------------------------------------------------------------ 6. RMS norm
@pytest.mark.parametrize('act', [0, 1])
@pytest.mark.parametrize('cpad,creal,rows', [(64, 64, 37), (128, 96, 37), (192, 192, 37), (384, 384, 37), (512, 512, 37), (128, 96, 302 * 72)])
def test_rmsnorm_nhwc_vs_fp64(lib, cpad, creal, rows, act):
    """All four lane-group widths (LP = 8, 16, 32, 64: 8, 4, 2, 1 rows per wave-load; 37 rows is a multiple of none but 1), a zero row, padded channels."""
    g = _gen(cpad + rows + act)
    x = torch.randn(rows, cpad, generator=g, device='cuda') * 1.3
    x[:, creal:] = 0
    x[5] = 0
    x = x.bfloat16()
    gamma = torch.zeros(cpad, device='cuda')
    gamma[:creal] = 1 + 0.3 * torch.randn(creal, generator=g, device='cuda')
    buf = torch.full((rows + 16, cpad), SENT, dtype=torch.bfloat16, device='cuda')
    y = buf[8:8 + rows]
    _ok(lib.afx_rmsnorm_nhwc(_p(x), _p(y), rows, cpad, creal, _p(gamma), act, _s()))
    torch.cuda.synchronize()
    assert bool((buf[:8] == SENT).all()) and bool((buf[8 + rows:] == SENT).all())
    nch = cpad // 8
    lp = 8 if nch <= 8 else 16 if nch <= 16 else 32 if nch <= 32 else 64
    xd = x.double()
    t = xd / xd.norm(dim=1, keepdim=True).clamp_min(1e-12) * math.sqrt(creal) * gamma.double()
    fl = (cpad // 8 + int(math.log2(lp)) + 4) * U32 * t.abs()
    if act:
        fl = 1.1 * fl + (t.abs() + 8) * U32 * silu64(t).abs()
        t = silu64(t)
    what = f'rmsnorm rows={rows} Cpad={cpad} Creal={creal} LP={lp} act={act}'
    _check_p(y, t, fl, what)
    assert not bool(y[5].any()) and not bool(y[:, creal:].any())
    _fails(y[:, :creal], torch.roll(t[:, :creal], 1, 1), fl[:, :creal], f'{what}: channels rotated')
