"""fp64 parity of the inference forward's attention operands, AdaLN rows and conditioning at the production width (D = 3072, H = 24).

Every case runs the forward's own launch construction (afx_qkv_operands, afx_norm_modulate_joint_bf16 / _mx8, the engine's exported
conditioning buffers) and compares it with plain fp64 torch built from the same bf16 / fp32 inputs, on the device.  How tight:
  * bf16 outputs: within one bf16 ulp of the fp64 value plus a floor derived from a stated fp32 error bound, and >= 99 % of the elements
    equal to the fp64 value rounded to nearest even (tests/bf16_parity.py).
  * fp32 sums: |error| <= depth * 2^-24 * sum |terms| -- the classical bound of recursive summation, depth = the longest chain of fp32
    roundings an output goes through.  For the GEMM: one rounding per MFMA K-step of 32 into the accumulator plus a serial chain over one
    instruction's 32 products, + 1 for the bias (depth K / 32 + 33).
  * q / k after RMSNorm + RoPE: an input error of at most E inside a head moves each output by <= 4 rstd max|w| E (the pair through the
    rotation and the norm's own change), plus 128 u max|n| for the fp32 evaluation of norm and rotation (as test_hip_train_kernels).
The text and image q / k norm weights have opposite signs, the rotary tables of the FLUX shapes are random angles (FLUX's own tables are
the identity on every text row), and every output is a view of a larger buffer whose guard bands hold a sentinel.
"""
import math

import numpy as np
import pytest
import torch
from bf16_parity import U32, bf16_ulp, check_bf16, gelu64 as _gelu64, proj64 as _proj64

pytestmark = pytest.mark.gpu

D, H = 3072, 24
SENT = -7.75                         # guard-band sentinel (bf16-exact)


@pytest.fixture(scope='module')
def ops():
    from arcflow_amd import ops as _ops
    return _ops


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def _key_of_pos(n):
    """afx_attn.hip key_of_pos: column p of V^T holds key (p & ~15) + key_of_pos(p & 15)."""
    p = torch.arange(n, device='cuda')
    j = p & 15
    return (p & ~15) + 4 * (j >> 3) + (j & 3) + 8 * ((j >> 2) & 1)


def _qk64(y, e, w_rows, pos, cos, sin, round_first):
    """RoPE(RMSNorm_128(y) * w) per head in fp64 and its floor.  round_first (kv_prep): the kernel normalises its bf16-rounded projection,
    which may sit one bf16 ulp from RNE of the exact one: that ulp joins the input error."""
    R = y.shape[0]
    if round_first:
        e = e + bf16_ulp(y)
        y = y.bfloat16().double()
    yh, eh = y.view(R, H, 128), e.view(R, H, 128)
    rstd = 1.0 / torch.sqrt((yh * yh).mean(-1, keepdim=True) + 1e-6)
    wr = w_rows.double()[:, None, :]
    n = yh * rstd * wr
    c, s = cos.double()[pos][:, None, :], sin.double()[pos][:, None, :]
    a_, b_ = n[..., 0::2], n[..., 1::2]
    out = torch.stack([a_ * c - b_ * s, a_ * s + b_ * c], -1).flatten(-2)
    floor = 4 * rstd * wr.abs().amax(-1, keepdim=True) * eh.amax(-1, keepdim=True) + U32 * 128 * n.abs().amax(-1, keepdim=True)
    return out.reshape(R, D), floor.expand(R, H, 128).reshape(R, D)


def _vt_ref(v, B, S):
    """[B*S, D] -> [B, H, 128, S_pad] with the key permutation; keys >= S are zero.  Returns (vt, valid column mask)."""
    S_pad = (S + 63) // 64 * 64
    keys = _key_of_pos(S_pad)
    valid = keys < S
    vp = torch.cat([v.reshape(B, S, D), torch.zeros(B, 1, D, dtype=v.dtype, device=v.device)], 1)
    return vp[:, keys.clamp(max=S)].view(B, S_pad, H, 128).permute(0, 2, 3, 1), valid


def _unchanged(buf, inner, what):
    mask = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    mask[inner] = False
    assert bool((buf[mask] == SENT).all()), f'{what}: a write landed in the guard band'


def _rope(kind, S, T, g):
    if kind == 'qwen':
        from arcflow_amd import rope
        c, s = rope.qwen_tables(64, 64, T)
        assert c.shape == (S, 64)
        return c.cuda(), s.cuda()
    ang = torch.rand(S, 64, generator=g, device='cuda', dtype=torch.float64) * (2 * math.pi)
    return torch.cos(ang).float().contiguous(), torch.sin(ang).float().contiguous()


# (kind, family, B, T, gemm mode, the path the forward takes there)
QKV_CASES = [
    ('double', 'flux', 1, 512, (3, 0), 'vt_proj'),
    ('double', 'flux', 2, 77, (3, 0), 'qk_epi'),
    ('double', 'flux', 2, 77, (3, 1), 'qk_epi'),       # 256x256 tiles (MI = 8)
    ('double', 'flux', 2, 77, (3, 6), 'qk_epi'),       # 224x256 tiles (MI = 7)
    ('double', 'flux', 2, 77, (2, 0), 'kv_prep'),      # the 8-phase kernel: no q / k epilogue
    ('single', 'flux', 2, 512, (3, 0), 'vt_proj'),
    ('single', 'flux', 2, 77, (3, 0), 'qk_epi'),
    ('double', 'qwen', 1, 128, (3, 0), 'vt_proj'),
    ('double', 'qwen', 1, 128, (3, 6), 'vt_proj'),
]


@pytest.mark.parametrize('kind,family,B,T,mode,path', QKV_CASES)
def test_qkv_operands_vs_fp64(ops, kind, family, B, T, mode, path):
    """One block's k | v | q (| gelu mlp) and V^T as the forward prepares them (path chosen by the forward for this shape and GEMM mode),
    against fp64: fused paths rope(rmsnorm(A W^T + b) w) rounded once, kv_prep the same on the bf16-rounded projection."""
    N = 4096
    S = N + T
    R, S_pad = B * S, (S + 63) // 64 * 64
    single = kind == 'single'
    width = (7 if single else 3) * D
    g = _gen(B * 1000 + T + mode[1] + 7 * single)
    a = (torch.randn(R, D + 64, generator=g, device='cuda') * 1.2 + 0.1).bfloat16()[:, 32:32 + D]
    nst = 1 if single else 2
    ws = [(torch.randn(width, D, generator=g, device='cuda') * D ** -0.5).bfloat16() for _ in range(nst)]
    bs = [(torch.randn(width, generator=g, device='cuda') * 0.2).bfloat16() for _ in range(nst)]
    img_w = 1 + 0.3 * torch.rand(2, 128, generator=g, device='cuda')
    txt_w = -(1 + 0.3 * torch.rand(2, 128, generator=g, device='cuda'))      # opposite sign: the wrong stream's weight fails
    qkn = (img_w if single else torch.cat([img_w, txt_w])).contiguous()
    cos, sin = _rope(family, S, T, g)
    fbuf = torch.full((R + 16, width + 128), SENT, dtype=torch.bfloat16, device='cuda')
    nvt = B * H * 128 * S_pad
    vbuf = torch.full((nvt + 8192,), SENT, dtype=torch.bfloat16, device='cuda')
    F, vt = fbuf[8:8 + R, 64:64 + width], vbuf[4096:4096 + nvt].view(B, H, 128, S_pad)
    try:
        ops.set_gemm_mode(*mode)
        ops.qkv_operands(kind, a, ws[0] if single else ws, bs[0] if single else bs, qkn, cos, sin, B, N, T, out=F, vt=vt)
        torch.cuda.synchronize()
    finally:
        ops.set_gemm_mode(3, 0)
    _unchanged(fbuf, (slice(8, 8 + R), slice(64, 64 + width)), 'projection buffer')
    _unchanged(vbuf, slice(4096, 4096 + nvt), 'V^T buffer')
    what = f'{kind} {family} B={B} T={T} mode={mode} {path}'
    # the fp64 projection: row j of the joint matrix is text (stream 1) when j % S < T
    pos = torch.arange(R, device='cuda') % S
    txt = pos < T
    y = torch.empty(R, width, dtype=torch.float64, device='cuda')
    e = torch.empty_like(y)
    for s in range(nst):
        rows = ~txt if s == 0 else txt
        if single:
            rows = torch.ones_like(txt)
        y[rows], e[rows] = _proj64(a[rows], ws[s], bs[s])
    kw = lambda i: torch.where(txt[:, None], txt_w[i][None], img_w[i][None]) if not single else img_w[i].expand(R, 128)   # noqa: E731
    kv = path == 'kv_prep'
    k_ref, k_fl = _qk64(y[:, :D], e[:, :D], kw(1), pos, cos, sin, kv)
    q_ref, q_fl = _qk64(y[:, 2 * D:3 * D], e[:, 2 * D:3 * D], kw(0), pos, cos, sin, kv)
    check_bf16(F[:, :D], k_ref, floor=k_fl, what=f'{what}: k')
    check_bf16(F[:, 2 * D:3 * D], q_ref, floor=q_fl, what=f'{what}: q')
    # the rows where a position or a norm weight changes: the text / image boundary (T - 1, T) and, single blocks, row % S across samples
    edge = [T - 1, T, S - 1] + ([S, 2 * S - 1] if B > 1 else [])
    for name, out, ref, fl in (('k', F[:, :D], k_ref, k_fl), ('q', F[:, 2 * D:3 * D], q_ref, q_fl)):
        check_bf16(out[edge], ref[edge], floor=fl[edge], min_equal=0.97, what=f'{what}: {name} rows {edge}')
    vt_ref, valid = _vt_ref(y[:, D:2 * D], B, S)
    assert bool((vt[..., ~valid].view(torch.int16) == 0).all()), f'{what}: V^T pad keys are not +0.0'
    vfl = _vt_ref(e[:, D:2 * D], B, S)[0]
    check_bf16(vt[..., valid], vt_ref[..., valid], floor=vfl[..., valid], what=f'{what}: V^T')
    if path == 'vt_proj':            # V^T came out of the projection: the V columns of the buffer stay unwritten
        assert bool((F[:, D:2 * D] == SENT).all()), f'{what}: V columns written: the forward did not take V^T from the projection'
    else:
        check_bf16(F[:, D:2 * D], y[:, D:2 * D], floor=e[:, D:2 * D], what=f'{what}: v')
        assert torch.equal(vt[..., valid], _vt_ref(F[:, D:2 * D], B, S)[0][..., valid]), f'{what}: V^T is not the permuted V columns'
    if single:                       # the mlp columns: gelu_tanh of the fp32 product (|gelu'| <= 1.13; exp2 + rcp: a few fp32 ulp)
        ym, em = y[:, 3 * D:], e[:, 3 * D:]
        check_bf16(F[:, 3 * D:], _gelu64(ym), floor=1.13 * em + 8 * U32 * ym.abs(), what=f'{what}: mlp')


# ------------------------------------------------------------------------------------------------ joint AdaLN (norm_modulate_rows_kernel<6, 2, *>)
def _mx_exp(amax):
    """afx_common.h mx_exp on fp32 amax: biased exponent of the smallest power of two p with amax <= 448 p, clamped to [1, 254]."""
    u = (amax.float() * np.float32(1.0 / 448.0)).view(torch.int32).long()
    b = ((u >> 23) & 0xff) + ((u & 0x7fffff) != 0).long()
    return b.clamp(1, 254)


def _e4m3_ord(codes):
    """e4m3 bytes -> signed ordinals (adjacent representable values differ by one; +0 and -0 are both 0)."""
    c = codes.long()
    mag = c & 0x7f
    return torch.where((c & 0x80) != 0, -mag, mag)


def _check_e4m3(q, ref_scaled, what):
    """Each e4m3 byte within one step of RNE(ref_scaled), >= 99 % exactly equal."""
    want = _e4m3_ord(ref_scaled.clamp(-448, 448).float().to(torch.float8_e4m3fn).view(torch.uint8))
    d = (_e4m3_ord(q) - want).abs()
    assert int(d.max()) <= 1, f'{what}: an e4m3 byte {int(d.max())} steps from RNE(ref / scale)'
    eq = (d == 0).double().mean().item()
    assert eq >= 0.99, f'{what}: only {eq:.4f} of the e4m3 bytes equal RNE(ref / scale)'


@pytest.mark.parametrize('B,T', [(1, 77), (3, 77), (1, 512), (3, 512)])
def test_joint_adaln_rows_vs_fp64(ops, B, T):
    """The double blocks' LN + modulate of text and image rows in one launch at D = 3072 (two rows per wave, (1 + scale, shift) kept in
    registers and reloaded when (sample, stream) changes -- at T = 77 rows 76 / 77 share a wave), strided input, the modulation vectors
    read from the stacked [B, n_mod] layout.  bf16 output, then both fp8 outputs: block-scaled e4m3 + E8M0 and e4m3 + one scale per row."""
    N = 4096
    S = N + T
    R = B * S
    g = _gen(B * 100 + T)
    x = (torch.randn(R, D + 64, generator=g, device='cuda') * 1.5 + 0.3).bfloat16()[:, 16:16 + D]
    x[5, 7] = 40.0                                         # an outlier row (its block scale differs from its neighbours')
    mod = torch.randn(B, 12 * D, generator=g, device='cuda') * 0.5       # one double block's rows of the stacked modulation output
    mod[:, 7 * D:8 * D] *= -2.0                                            # text scale / shift clearly unlike the image ones
    mod[:, 6 * D:7 * D] += 1.0
    sc, sh, sc_t, sh_t = mod[:, 1 * D:2 * D], mod[:, 0:D], mod[:, 7 * D:8 * D], mod[:, 6 * D:7 * D]
    xd = x.double()
    mu = xd.mean(-1, keepdim=True)
    ln = (xd - mu) / torch.sqrt(((xd - mu) ** 2).mean(-1, keepdim=True) + 1e-6)
    txt = (torch.arange(R, device='cuda') % S) < T
    b_of = torch.arange(R, device='cuda') // S
    scr = torch.where(txt[:, None], sc_t.double()[b_of], sc.double()[b_of])
    shr = torch.where(txt[:, None], sh_t.double()[b_of], sh.double()[b_of])
    ref = ln * (1 + scr) + shr
    # fp32 LayerNorm: one bf16 ulp + fp32 eps x D x the row's scale (as the ln tests of test_hip_train_kernels)
    row_scale = (ln.abs() * (1 + scr).abs() + shr.abs()).amax(-1, keepdim=True)
    floor = U32 * D * row_scale
    obuf = torch.full((R, D + 64), SENT, dtype=torch.bfloat16, device='cuda')
    ops.norm_modulate_joint(x, sc, sh, S, sc_t, sh_t, T, out=obuf[:, 24:24 + D])
    _unchanged(obuf, (slice(None), slice(24, 24 + D)), 'norm_modulate_joint')
    check_bf16(obuf[:, 24:24 + D], ref, floor=floor, what=f'joint AdaLN B={B} T={T}')
    # block-scaled fp8: E8M0 byte of every 128-column block per mx_exp of its amax (the kernel's amax carries the fp32 error of the row)
    q, mx, fused = ops.norm_modulate_mx8(x, sc, sh, S, sc_t, sh_t, T)
    assert fused, 'D = 3072 with >= 1024 rows: the fused LayerNorm -> fp8 kernel must take the launch'
    amax = ref.abs().view(R, D // 128, 128).amax(-1)
    lo, hi = _mx_exp((amax - floor).clamp_min(0)), _mx_exp(amax + floor)
    got = mx.long()
    assert bool(((got >= lo) & (got <= hi)).all()), f'mx8 B={B} T={T}: E8M0 bytes off the mx_exp of the block maxima'
    assert (got == _mx_exp(amax)).double().mean().item() >= 0.99
    scale = torch.exp2(got.double() - 127).repeat_interleave(128, 1)
    _check_e4m3(q, ref / scale, f'mx8 B={B} T={T}')
    # one scale per row: absmax / 448 of the fp32 row (the row's error bound + two fp32 roundings), the bytes RNE(ref / scale)
    q2, rs, fused = ops.norm_modulate_mx8(x, sc, sh, S, sc_t, sh_t, T, row_scale=True)
    assert fused
    ramax = ref.abs().amax(-1)
    err = (rs.double() - ramax / 448).abs()
    assert bool((err <= (floor[:, 0] + 2 * U32 * ramax) / 448).all()), f'row scales B={B} T={T}: max err {err.max().item():.3e}'
    _check_e4m3(q2, ref / rs.double()[:, None], f'row-scaled fp8 B={B} T={T}')


# ------------------------------------------------------------------------------------------------ conditioning chain
def _silu64(x):
    return x * torch.sigmoid(x)


def _sincos64(t, cast):
    """sincos_kernel's documented casts: FLUX (cast 1) feeds bf16(bf16(t) * 1000) to the sinusoid.  The angle is formed in fp32 as the kernel
    forms it (frequency expf(-ln(1e4) i / 128), then the product), its cos / sin in fp64.  Bound: cos / sin in fp32 (2 u) and one fp32 ulp of
    the frequency between the device's expf and torch's (2 u |a| through the product).  Qwen (cast 2) rounds t alone to bf16; the x 1000 is
    the sinusoid's own scale in fp32: a = 1000 * (bf16(t) * f), two fp32 products in the kernel's order (same bound)."""
    assert cast in (1, 2)
    tb = t.bfloat16().float()
    i = torch.arange(128, device=t.device, dtype=torch.float32)
    f = torch.exp(torch.tensor(-9.210340371976184, dtype=torch.float32, device=t.device) * i / 128.0)
    if cast == 1:
        x = (tb * 1000).bfloat16().float()
        a = (x[:, None] * f[None]).double()
    else:
        a = (1000.0 * (tb[:, None] * f[None])).double()
    return torch.cat([torch.cos(a), torch.sin(a)], 1), torch.cat([2 * a.abs() + 2] * 2, 1) * U32


def _gemv64(x, ex, w, b, act=False):
    """gemv_kernel in fp64 with its error bound: a lane sums its 8-column chunks serially (8 K/512 terms at K = D), 6 wave-shuffle levels, the
    bias (depth 8 ceil(K / 512) + 8); the input's own error through |W|; SiLU (<= 1.1 Lipschitz, __expf: 4 u)."""
    wd = w.double()
    K = w.shape[1]
    y = x @ wd.T + b.double()
    e = (8 * ((K + 511) // 512) + 8) * U32 * (x.abs() @ wd.abs().T + b.double().abs()) + ex @ wd.abs().T
    if act:
        return _silu64(y), 1.1 * e + 4 * U32 * y.abs()
    return y, e


def _assert_within(out, ref, bound, what):
    err = (out.double() - ref).abs()
    assert bool((err <= bound).all()), f'{what}: max err / bound {(err / bound).max().item():.3f}'


def test_conditioning_chain_full_width(ops):
    """temb = t_mlp(sincos(t)) + g_mlp(sincos(g)) + p_mlp(pooled), SiLU, and the stacked modulation GEMV of a FLUX engine with 2 double and
    2 single blocks at D = 3072 (n_mod = 32 D rows), read back through afx_mmdit_export; then afx_mmdit_prepare_steps with B x nsteps = 8
    rows (the GEMV's batch limit): each prepared step's temb and modulation rows against the same fp64 chain."""
    from arcflow_amd import MMDiTEngine, _lib
    nd, ns, B = 2, 2, 2
    eng = MMDiTEngine('flux', nd, ns)
    n_mod = eng.n_mod
    assert n_mod == 32 * D
    g = _gen(2024)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, generator=g, device='cuda') * sc).bfloat16()     # noqa: E731
    cond = {'temb.t.l1': (D, 256), 'temb.t.l2': (D, D), 'temb.g.l1': (D, 256), 'temb.g.l2': (D, D), 'temb.p.l1': (D, 768),
            'temb.p.l2': (D, D), 'mod': (n_mod, D)}
    packed = {}
    for n, (o, i) in cond.items():
        packed[n + '.weight'] = rnd(o, i, sc=i ** -0.5)
        packed[n + '.bias'] = rnd(o, sc=0.1)
    # the trunk's weights take no part in stage 1: one zero buffer behind all of them
    trunk = {'x_in': (D, 64), 'ctx_in': (D, 4096), 'head': (1152, D)}
    for i in range(nd):
        for s in ('img', 'txt'):
            trunk.update({f'd{i}.{s}_qkv': (3 * D, D), f'd{i}.{s}_out': (D, D), f'd{i}.{s}_mlp1': (4 * D, D), f'd{i}.{s}_mlp2': (D, 4 * D)})
    for i in range(ns):
        trunk.update({f's{i}.fused': (7 * D, D), f's{i}.out': (D, 5 * D)})
    zero = torch.zeros(7 * D * D, dtype=torch.bfloat16, device='cuda')
    for n, (o, i) in trunk.items():
        packed[n + '.weight'] = zero[:o * i].view(o, i)
        packed[n + '.bias'] = zero[:o]
    zf = torch.ones(4 * 128, device='cuda')
    for i in range(nd):
        packed[f'd{i}.qknorm'] = zf.view(4, 128)
    for i in range(ns):
        packed[f's{i}.qknorm'] = zf[:256].view(2, 128)
    eng.bind_packed(packed)
    N, T = 16, 8
    x = torch.zeros(B, N, 64, dtype=torch.bfloat16, device='cuda')
    ctx = torch.zeros(B, T, 4096, dtype=torch.bfloat16, device='cuda')
    pooled = rnd(B, 768)
    gd = torch.tensor([3.5, 1.25], device='cuda')
    W = {n: (packed[n + '.weight'], packed[n + '.bias']) for n in cond}

    def temb_reference(t):
        sc_t, e_t = _sincos64(t, 1)
        sc_g, e_g = _sincos64(gd, 1)
        h, eh = _gemv64(sc_t, e_t, *W['temb.t.l1'], act=True)
        temb, et = _gemv64(h, eh, *W['temb.t.l2'])
        for lin1, lin2, x0, e0 in (('temb.g.l1', 'temb.g.l2', sc_g, e_g), ('temb.p.l1', 'temb.p.l2', pooled.double(), 0 * pooled.double())):
            h, eh = _gemv64(x0, e0, *W[lin1], act=True)
            y, ey = _gemv64(h, eh, *W[lin2])
            temb, et = temb + y, et + ey + U32 * (temb + y).abs()     # the accumulating GEMV: one more rounding
        return temb, et

    def mod_reference(semb):
        """the stacked modulation GEMV on the engine's own SiLU output (exact fp32 inputs: the summation bound alone)"""
        w, b = W['mod']
        mod = torch.empty(B, n_mod, dtype=torch.float64, device='cuda')
        emod = torch.empty_like(mod)
        for r0 in range(0, n_mod, 16384):
            mod[:, r0:r0 + 16384], emod[:, r0:r0 + 16384] = _gemv64(semb.double(), 0 * semb.double(), w[r0:r0 + 16384], b[r0:r0 + 16384])
        return mod, emod

    def check_all(got, t, what):
        temb, et = temb_reference(t)
        _assert_within(got[0], temb, et, f'{what}temb')
        # SiLU of the engine's own temb: x / (1 + __expf(-x)) in fp32, a few ulp
        _assert_within(got[1], _silu64(got[0].double()), 4 * U32 * got[0].double().abs() + 1e-30, f'{what}silu_temb')
        mod, emod = mod_reference(got[1])
        _assert_within(got[2], mod, emod, f'{what}mod_all')
        return mod, emod

    def exported(k=None):
        if k is not None:
            _lib.check(eng.lib.afx_mmdit_use_prepared_step(eng._ctx, k))
        eng(x, ts[k] if k is not None else t0, ctx, pooled, gd, 4, 4, stage=1)
        outs = [torch.empty(B, D, device='cuda'), torch.empty(B, D, device='cuda'), torch.empty(B, n_mod, device='cuda')]
        for name, o in zip(('temb', 'silu_temb', 'mod_all'), outs):
            eng.export(name, o, B, N, T)
        torch.cuda.synchronize()
        return outs

    t0 = torch.tensor([0.7619, 0.05], device='cuda')
    got = exported()
    mod, emod = check_all(got, t0, '')
    # the bound is not vacuous: one lane chunk of the modulation GEMV's inputs left out exceeds it
    w = W['mod'][0]
    drop = mod - got[1].double()[:, :8] @ w[:, :8].double().T
    assert bool(((got[2].double() - drop).abs() > emod).any()), 'mod_all: the bound cannot tell a dropped chunk'
    ts = torch.tensor([[1.0, 0.9], [0.6, 0.45], [0.3, 0.2], [0.1, 0.0]], device='cuda')
    assert eng.prepare_steps(ts, pooled, gd, batch=B, n_img=N, n_txt=T)
    for k in range(4):
        check_all(exported(k), ts[k], f'prepared step {k}: ')


def test_conditioning_chain_full_width_qwen(ops):
    """The Qwen twin: temb = t_mlp(sincos(t)) alone -- sincos_kernel cast mode 2, no guidance and no pooled branch -- SiLU and the stacked
    modulation GEMV of a Qwen engine with one block at D = 3072 (n_mod = 14 D rows), then afx_mmdit_prepare_steps with B x nsteps = 8 rows.
    t = 0.7619 is moved visibly by the bf16 rounding (to 0.76171875), t = 0 gives cos 1 / sin 0 exactly.  _gemv64 and its bound unchanged."""
    from arcflow_amd import MMDiTEngine, _lib
    nd, B, J = 1, 2, 3584
    eng = MMDiTEngine('qwen', nd, 0, joint_dim=J)
    n_mod = eng.n_mod
    assert n_mod == 14 * D
    g = _gen(2025)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, generator=g, device='cuda') * sc).bfloat16()     # noqa: E731
    cond = {'temb.t.l1': (D, 256), 'temb.t.l2': (D, D), 'mod': (n_mod, D)}
    packed = {}
    for n, (o, i) in cond.items():
        packed[n + '.weight'] = rnd(o, i, sc=i ** -0.5)
        packed[n + '.bias'] = rnd(o, sc=0.1)
    # the trunk's weights take no part in stage 1's conditioning: one zero buffer behind all of them
    trunk = {'x_in': (D, 64), 'ctx_in': (D, J), 'head': (1152, D)}
    for i in range(nd):
        for s in ('img', 'txt'):
            trunk.update({f'd{i}.{s}_qkv': (3 * D, D), f'd{i}.{s}_out': (D, D), f'd{i}.{s}_mlp1': (4 * D, D), f'd{i}.{s}_mlp2': (D, 4 * D)})
    zero = torch.zeros(4 * D * D, dtype=torch.bfloat16, device='cuda')
    for n, (o, i) in trunk.items():
        packed[n + '.weight'] = zero[:o * i].view(o, i)
        packed[n + '.bias'] = zero[:o]
    zf = torch.ones(J, device='cuda')
    for i in range(nd):
        packed[f'd{i}.qknorm'] = zf[:512].view(4, 128)
    packed['txt_norm.weight'] = zf
    eng.bind_packed(packed)
    N, T = 16, 8
    x = torch.zeros(B, N, 64, dtype=torch.bfloat16, device='cuda')
    ctx = torch.zeros(B, T, J, dtype=torch.bfloat16, device='cuda')
    W = {n: (packed[n + '.weight'], packed[n + '.bias']) for n in cond}

    def check_all(got, t, what):
        sc_t, e_t = _sincos64(t, 2)
        h, eh = _gemv64(sc_t, e_t, *W['temb.t.l1'], act=True)
        temb, et = _gemv64(h, eh, *W['temb.t.l2'])
        _assert_within(got[0], temb, et, f'{what}temb')
        # SiLU of the engine's own temb: x / (1 + __expf(-x)) in fp32, a few ulp
        _assert_within(got[1], _silu64(got[0].double()), 4 * U32 * got[0].double().abs() + 1e-30, f'{what}silu_temb')
        # the stacked modulation GEMV on the engine's own SiLU output (exact fp32 inputs: the summation bound alone)
        semb = got[1].double()
        for r0 in range(0, n_mod, 16384):
            mod, emod = _gemv64(semb, 0 * semb, W['mod'][0][r0:r0 + 16384], W['mod'][1][r0:r0 + 16384])
            _assert_within(got[2][:, r0:r0 + 16384], mod, emod, f'{what}mod_all rows {r0}..')

    def exported(t, k=None):
        if k is not None:
            _lib.check(eng.lib.afx_mmdit_use_prepared_step(eng._ctx, k))
        eng(x, t, ctx, None, None, 4, 4, stage=1)
        outs = [torch.empty(B, D, device='cuda'), torch.empty(B, D, device='cuda'), torch.empty(B, n_mod, device='cuda')]
        for name, o in zip(('temb', 'silu_temb', 'mod_all'), outs):
            eng.export(name, o, B, N, T)
        torch.cuda.synchronize()
        return outs

    t0 = torch.tensor([0.7619, 0.0], device='cuda')
    assert t0.bfloat16().float()[0].item() == 0.76171875
    got = exported(t0)
    check_all(got, t0, '')
    # cast mode 2 is what ran: the FLUX cast (bf16(bf16(t) * 1000) = 760.0 against 761.71875) gives another embedding
    sc1, e1 = _sincos64(t0, 1)
    h, eh = _gemv64(sc1, e1, *W['temb.t.l1'], act=True)
    temb1, et1 = _gemv64(h, eh, *W['temb.t.l2'])
    assert bool(((got[0].double() - temb1).abs() > et1)[0].any()), 'temb: the bound cannot tell cast mode 1 from cast mode 2'
    ts = torch.tensor([[1.0, 0.9], [0.7619, 0.45], [0.3, 0.2], [0.1, 0.0]], device='cuda')
    assert eng.prepare_steps(ts, None, None, batch=B, n_img=N, n_txt=T)
    for k in range(4):
        check_all(exported(ts[k], k), ts[k], f'prepared step {k}: ')
