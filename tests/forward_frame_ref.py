"""fp64 references of the frame around the MMDiT blocks -- the embedders into the joint token matrix, the plain AdaLN / RMS rows, norm_out
and the ArcFlow head split -- each with its fp32 error bound, the mutated references of the teeth checks, the seeded inputs and the one
assertion that test_hip_forward_frame_fp64.py (the kernels) and test_forward_frame_ref_cpu.py (the references alone) share.

Bounds (u = 2^-24; every output also gets one bf16 ulp of the reference for its final rounding):
  * LN / RMS rows: u D row_scale, row_scale = max over the row of |ln| |1 + scale| + |shift| (|n w| for RMS): D-term fp32 sums for mean and
    variance, carried to the output at the row's largest magnitude -- the bound test_joint_adaln_rows_vs_fp64 uses.  A row of one constant
    bf16 value c has bound 0: D c (D <= 4096) needs at most 8 + 12 significant bits, so every partial sum of the lane loop and of the wave
    reduction is exact, the correctly rounded quotient D c / D is c, v - mean is exactly 0 and the output is 0 * rstd * (1 + scale) + shift =
    shift, rounded once.
  * GEMMs: proj64's summation bound (depth K / 32 + 33).  Qwen's text rows go through RMSNorm first, stored as bf16: the reference rounds the
    fp64 normed row to bf16, and the kernel's stored operand may sit one bf16 ulp from that (its fp32 row carries the RMS bound), so
    ulp_bf16(n) + rms bound per operand element is carried through |W| into the output bound.
  * log_softmax over K (head_split_kernel: mx = max, se = sum_k expf(x_k - mx) serially, lse = mx + logf(se), out_k = x_k - lse):
      x_k - mx          one rounding, u |z_k|: a relative error u |z_k| of expf's value;
      expf              XE u relative, XE = 2 ULP_ALLOW['expf'] (1 ulp <= 2 u relative);
      the sum           K positive terms, serial: (K - 1) u relative;
      logf(se)          d log = the relative error of se, plus XL u |log se|, XL = 2 ULP_ALLOW['logf'];
      mx + .            u |lse|;         x_k - lse   u |out_k|
    E = u (XE + (K - 1) + max_k |z_k| + XL |log se| + |lse| + |out_k|).  expf and logf: the maxima measured on an MI355X with the project's
    flags (arcflow_policy_ref.ULP_MEASURED: 0.8576 and 2.3006 ulp), doubled -- 1.72 and 4.60 ulp.
    Logits known to within d_k move lse by at most max_k d_k (lse is 1-Lipschitz in the max norm) and out_k by d_k more: 2 max_k d_k.
"""
import torch

from arcflow_policy_ref import ULP_ALLOW
from bf16_parity import U32, bf16_ulp, check_bf16, check_bf16_bound, proj64

D = 3072
K_G, CH, LW = 16, 64, 4                      # gaussians, in_channels, logweights_channels
NM, NW, NG = K_G * CH, K_G * LW, (K_G - 1) * LW
HEAD_N = (NM + NW + NG + 7) // 8 * 8         # 1152
XE, XL = 2.0 * ULP_ALLOW['expf'], 2.0 * ULP_ALLOW['logf']
BIG_LOGIT = (5, 2)                           # (k, p) of the exact-logit table's entry 20 above the rest


def frame_check(out, ref, bound, what, min_equal=0.99, share=None):
    """THE assertion of the frame tests: |out - ref| <= ulp_bf16(ref) + bound on every element, and (min_equal is not None) at least
    min_equal of the elements selected by share (all when None) equal to RNE(ref).  Returns the worst err / tol."""
    ref = ref.double()
    bound = torch.as_tensor(bound, dtype=torch.float64, device=ref.device).expand_as(ref)
    worst = check_bf16_bound(out, ref, bound, what)
    if min_equal is not None:
        o, r, b = (out, ref, bound) if share is None else (out[share], ref[share], bound[share])
        check_bf16(o, r, floor=b, min_equal=min_equal, what=what)
    return worst


def vacuous_share(ref, bound):
    """Share of the elements on which the bound (without the ulp) exceeds the reference's own magnitude."""
    return (torch.as_tensor(bound).expand_as(ref) > ref.abs()).double().mean().item()


# ------------------------------------------------------------------------------------------------ LN / RMS rows
def sample_of_row(rows, rpb, B, shifted=False, device='cpu'):
    """row // rows_per_batch; shifted (the teeth check): (row + 1) // rows_per_batch -- the last row of a sample takes the next one's vectors."""
    return ((torch.arange(rows, device=device) + int(shifted)) // rpb).clamp(max=B - 1)


def adaln64(x, scale_rows, shift_rows):
    """LN(x) (no affine, eps 1e-6) * (1 + scale) + shift with per-row [R, D] vectors.  Returns (ref, bound)."""
    xd, sc, sh = x.double(), scale_rows.double(), shift_rows.double()
    c = xd - xd.mean(-1, keepdim=True)
    ln = c / torch.sqrt((c * c).mean(-1, keepdim=True) + 1e-6)
    ref = ln * (1 + sc) + sh
    row_scale = (ln.abs() * (1 + sc).abs() + sh.abs()).amax(-1, keepdim=True)
    bound = (U32 * xd.shape[1] * row_scale).expand_as(ref).clone()
    bound[(xd == xd[:, :1]).all(-1)] = 0.0             # a constant row: v - mean cancels exactly (module docstring)
    return ref, bound


def rms64(x, w):
    """x * rsqrt(mean x^2 + 1e-6) * w.  Returns (ref, bound)."""
    xd = x.double()
    ref = xd / torch.sqrt((xd * xd).mean(-1, keepdim=True) + 1e-6) * w.double()
    return ref, (U32 * xd.shape[1] * ref.abs().amax(-1, keepdim=True)).expand_as(ref)


def norm_out64(x_img, mod_final, N):
    """norm_out on the image rows x_img [B*N, D]: scale is the FIRST half of mod_final [B, 2D], shift the second."""
    Dm = x_img.shape[1]
    b = torch.arange(x_img.shape[0], device=x_img.device) // N
    return adaln64(x_img, mod_final[:, :Dm][b], mod_final[:, Dm:][b])


# (rows, rows_per_batch, D): what each reaches is said in test_hip_forward_frame_fp64.py
NORM_CASES = [(2050, 1025, 3072), (2049, 683, 3072), (1024, 1024, 3072), (1023, 341, 3072), (37, 19, 4096), (37, 19, 3584), (37, 19, 264)]
N_MOD, SC_COL, SH_COL = 5, 1, 3              # the stacked modulation tensor [B, 5 D]: scale = columns [D, 2D), shift = [3D, 4D)
OUTLIER_ROW, CONST_ROW = 5, 9


def norm_inputs(rows, rpb, Dm, device='cpu'):
    """x: a column view [rows, Dm] of a [rows, Dm + 64] bf16 buffer with one outlier (40.0) and one constant row; the stacked fp32 modulation
    tensor [B, 5 Dm]; the RMS weight [Dm]."""
    g = torch.Generator().manual_seed(rows * 7 + rpb + Dm)
    B = -(-rows // rpb)
    xb = (torch.randn(rows, Dm + 64, generator=g) * 1.5 + 0.3).bfloat16()
    xb[OUTLIER_ROW, 16 + 7] = 40.0
    xb[CONST_ROW] = 1.25
    mod = torch.randn(B, N_MOD * Dm, generator=g) * 0.5
    w = 1 + 0.3 * torch.randn(Dm, generator=g)
    return xb.to(device)[:, 16:16 + Dm], mod.to(device), w.to(device)


def norm_case64(x, mod, rpb, shifted=False):
    rows, Dm = x.shape
    b = sample_of_row(rows, rpb, mod.shape[0], shifted, x.device)
    return adaln64(x, mod[:, SC_COL * Dm:(SC_COL + 1) * Dm][b], mod[:, SH_COL * Dm:(SH_COL + 1) * Dm][b])


# ------------------------------------------------------------------------------------------------ embedders
EMBED_SHAPES = {'flux': (2, 77, 16, 4096), 'qwen': (2, 20, 16, 3584)}        # B, T, N, joint_dim


def embed_inputs(family, device='cpu'):
    B, T, N, J = EMBED_SHAPES[family]
    g = torch.Generator().manual_seed(31 + J)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).bfloat16().to(device)     # noqa: E731
    inp = {'x': rnd(B, N, CH), 'ctx': rnd(B, T, J),
           'x_in': (rnd(D, CH, sc=CH ** -0.5), rnd(D, sc=0.1)), 'ctx_in': (rnd(D, J, sc=J ** -0.5), rnd(D, sc=0.1)), 'txt_norm': None}
    if family == 'qwen':
        inp['txt_norm'] = (1 + 0.3 * torch.randn(J, generator=g)).to(device)
    return inp


def embed64(x, ctx, x_in, ctx_in, txt_norm=None, swapped=False, round_normed=True):
    """The joint token matrix [B*(T+N), Dm] after the embedders, rows [text T | image N] per sample (swapped, the teeth check:
    [image N | text T]).  txt_norm (Qwen): RMSNorm(eps 1e-6, weight) on the text states first, the normed row rounded to bf16 as the
    engine stores it.  Returns (ref, bound, text-row mask)."""
    B, N, _ = x.shape
    T = ctx.shape[1]
    img, e_img = proj64(x.reshape(B * N, -1), *x_in)
    a = ctx.reshape(B * T, -1).double()
    if txt_norm is not None:
        a, e_a = rms64(a, txt_norm)
        if round_normed:
            e_a = e_a + bf16_ulp(a)
            a = a.float().bfloat16().double()
    txt, e_txt = proj64(a, *ctx_in)
    if txt_norm is not None:
        e_txt = e_txt + e_a @ ctx_in[0].double().abs().T
    parts = lambda t, i, b: ([i[b * N:(b + 1) * N], t[b * T:(b + 1) * T]] if swapped else [t[b * T:(b + 1) * T], i[b * N:(b + 1) * N]])   # noqa: E731
    ref = torch.cat([p for b in range(B) for p in parts(txt, img, b)])
    bound = torch.cat([p for b in range(B) for p in parts(e_txt, e_img, b)])
    is_txt = (torch.arange(B * (T + N), device=ref.device) % (T + N)) < T
    return ref, bound, is_txt


# ------------------------------------------------------------------------------------------------ head
HEAD_B, HEAD_T = 2, 77
HEAD_N_IMG = {1025: (25, 41), 256: (16, 16)}          # N: (hp, wp)
TEXT_FILL = 300.0


def exact_logit_table():
    """[K, lw] bf16-exact logits, all different: multiples of 1/8 in [-4, 3.875] in a seeded order, and one entry 20 above the largest."""
    perm = torch.randperm(NW, generator=torch.Generator().manual_seed(5))
    t = (perm.double() * 0.125 - 4.0).view(K_G, LW)
    t[BIG_LOGIT] = t.max() + 20.0
    assert torch.equal(t.float().bfloat16().double(), t) and t.unique().numel() == NW
    return t


def head_inputs(N, teacher=False, device='cpu'):
    """The imported joint token matrix (text rows 300.0), the head's weight and bias, the second binding with exact logits, and a seeded
    stand-in for mod_final (the kernel test takes the engine's exported one instead)."""
    B, T = HEAD_B, HEAD_T
    g = torch.Generator().manual_seed(N + 3 * teacher)
    tokens = (torch.randn(B, T + N, D, generator=g) * 1.5 + 0.3).bfloat16()
    tokens[:, :T] = TEXT_FILL
    hn = CH if teacher else HEAD_N
    w = (torch.randn(hn, D, generator=g) * D ** -0.5).bfloat16()
    b = (torch.randn(hn, generator=g) * 0.1).bfloat16()
    inp = {'tokens': tokens.view(B * (T + N), D).to(device), 'head': (w.to(device), b.to(device)),
           'mod_final': (torch.randn(B, 2 * D, generator=g) * 0.5).to(device)}
    if not teacher:
        wx, bx = w.clone(), b.clone()
        wx[NM:NM + NW] = 0
        bx[NM:NM + NW] = exact_logit_table().flatten().bfloat16()
        inp['head_exact'] = (wx.to(device), bx.to(device))
    return inp


def image_rows(tokens, B, N, T):
    return tokens.view(B, T + N, -1)[:, T:].reshape(B * N, -1)


def head_split64(head, e_head=None, round_first=True, over='k', logg_shift=0):
    """means | logw | logg of head rows [R, >= 1148] (fp64): means and logg are columns [0, K ch) and [K ch + K lw, .. + (K - 1) lw) (logg_shift,
    the teeth check: lw columns further), logw = log_softmax over k of the logits at column K ch + k lw + p, taken from the head row rounded to
    bf16 first (round_first), as the kernel reads it (over='p', the teeth check: the softmax over p at fixed k).  Returns (means, logw [R, K lw],
    logg, bound of logw): the fp32 evaluation term E of the module docstring, plus 2 max_k (ulp_bf16(logit) + e_head) when e_head, the error
    bound of the head row, is given."""
    R = head.shape[0]
    means, logg = head[:, :NM], head[:, NM + NW + logg_shift:NM + NW + logg_shift + NG]
    y = head[:, NM:NM + NW].double()
    x = (y.float().bfloat16().double() if round_first else y).view(R, K_G, LW)
    dim = 1 if over == 'k' else 2
    mx = x.amax(dim, keepdim=True)
    log_se = torch.log(torch.exp(x - mx).sum(dim, keepdim=True))
    lse = mx + log_se
    out = x - lse
    bound = U32 * (XE + (K_G - 1) + (x - mx).abs().amax(dim, keepdim=True) + XL * log_se.abs() + lse.abs() + out.abs())
    if e_head is not None:
        d = (bf16_ulp(y) + e_head[:, NM:NM + NW]).view(R, K_G, LW)
        bound = bound + 2 * d.amax(dim, keepdim=True)
    return means, out.reshape(R, NW), logg, bound.reshape(R, NW)


def big_logit_mask(R, device='cpu'):
    """[R, K lw] True at the exact-logit table's dominant entry: its output, -sum_k' exp(x_k' - x_k) ~ -1e-8, lies below the fp32
    resolution of lse (u |lse| ~ 1.4e-6), so it is held by the bound alone and takes no part in the RNE share."""
    m = torch.zeros(K_G, LW, dtype=torch.bool, device=device)
    m[BIG_LOGIT] = True
    return m.flatten().expand(R, NW)
