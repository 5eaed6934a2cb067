"""References of image editing (``afx_edit_blend``, ``schedule.mask_to_tokens``) for the edit tests: an fp64 numpy statement of the blend,
a loop-written mask reduction, the inputs the kernel test runs on, and MUTANTS -- deliberately wrong references, each of which the
comparison of tests/test_hip_edit_blend_fp64.py must reject on those inputs (tests/test_edit_cpu.py checks without a GPU that every
mutant moves the reference by more than twice the bound on at least 1 % of the elements, so a mutant cannot pass by being too small
to see: the masks differ across the four sub-pixels and across the samples, and so do the sigmas).

The blend, per element e of token tok of sample b (packed channel e = c*4 + ph*2 + pw, so the latent pixel of the patch is e & 3):

    known = (1 - sigma_to[b]) x0 + sigma_to[b] noise          (no noise term when noise is None)
    out   = m x + (1 - m) known,    m = mask[b, tok, e & 3]   (out = known when mask is None)

Bound against fp64 from the same fp32 inputs.  The kernel rounds om = fl(1 - sigma), p = fl(om x0), known = fl(sigma noise + p) (one
fma), q = fl(1 - m), r = fl(q known), out = fl(m x + r) (one fma): six roundings, each of relative size eps = 2^-24 on a term whose
magnitude, carried to the output, is at most |x| + |x0| + |noise| because m and sigma are in [0, 1].  |err| <= 6 eps M to first order,
and 8 eps M leaves room for the second-order terms: |err| <= 8 * 2^-24 * (|x| + |x0| + |noise|).
"""
import numpy as np

EPS = 2.0 ** -24
B, N_TOK, CH = 2, 15, 64
MUTANTS = ('subpixel_shift', 'sigma0', 'swap_m', 'keep_noise', 'token_mask')          # of blend_ref; 'bf16_trunc' is bf16_bits(..., trunc=True)


def bf16_bits(x32: np.ndarray, trunc: bool = False) -> np.ndarray:
    """The bf16 bit pattern (uint16) of fp32 values: round-to-nearest-even, or -- the mutant -- truncation.  Finite inputs."""
    bits = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    if not trunc:
        bits = bits + 0x7fff + ((bits >> 16) & 1)
    return (bits >> 16).astype(np.uint16)


def blend_ref(x, x0, noise, mask, sigma_to, mutate=None, noise_is_null=False):
    """fp64 blend of fp32 inputs -> [B, N, 64] float64.  mask None: everything known.  noise_is_null: the call passes noise = NULL, the
    term is dropped (the 'keep_noise' mutant keeps it, from the ``noise`` array given here)."""
    x0 = np.asarray(x0, dtype=np.float64)
    Bn, N, ch = x0.shape
    sg = np.asarray(sigma_to, dtype=np.float64).reshape(Bn, 1, 1)
    if mutate == 'sigma0':
        sg = np.broadcast_to(sg[:1], sg.shape)
    known = (1.0 - sg) * x0
    if noise is not None and (not noise_is_null or mutate == 'keep_noise'):
        known = known + sg * np.asarray(noise, dtype=np.float64)
    if mask is None:
        return known
    e = np.arange(ch)
    sub = e >> 4 if mutate == 'subpixel_shift' else e & 3
    m = np.asarray(mask, dtype=np.float64)[:, :, sub]                                   # [B, N, 64]
    if mutate == 'token_mask':
        m = np.broadcast_to(np.asarray(mask, dtype=np.float64)[:, :, :1], m.shape)
    if mutate == 'swap_m':
        m = 1.0 - m
    return m * np.asarray(x, dtype=np.float64) + (1.0 - m) * known


def blend_bound(x, x0, noise):
    M = np.abs(np.asarray(x0, dtype=np.float64))
    for t in (x, noise):
        if t is not None:
            M = M + np.abs(np.asarray(t, dtype=np.float64))
    return 8 * EPS * M


def mask_to_tokens_loop(mask, hp, wp, reduce='max'):
    """mask [B, H, W] (H = 16 hp, W = 16 wp) -> [B, hp*wp, 4] float64, written as loops: latent pixel (2r + ph, 2c + pw) is the 8 x 8
    pixel block at rows 8 (2r + ph), columns 8 (2c + pw)."""
    mask = np.asarray(mask, dtype=np.float64)
    out = np.zeros((mask.shape[0], hp * wp, 4))
    for b in range(mask.shape[0]):
        for r in range(hp):
            for c in range(wp):
                for ph in range(2):
                    for pw in range(2):
                        i, j = 8 * (2 * r + ph), 8 * (2 * c + pw)
                        blk = mask[b, i:i + 8, j:j + 8]
                        out[b, r * wp + c, ph * 2 + pw] = blk.max() if reduce == 'max' else blk.sum() / 64.0
    return out


def tie_values():
    """8 fp32 values exactly halfway between two bf16 neighbours (low half 0x8000), four with an even and four with an odd bf16 mantissa
    below them, both signs: round-to-nearest-even goes down on the even ones and up on the odd ones, truncation always goes down."""
    hi = np.array([0x3f80, 0x3f81, 0xbf82, 0xbf83, 0x4049, 0x404a, 0xc2f7, 0x3e2a], dtype=np.uint32)
    return ((hi << 16) | 0x8000).view(np.float32)


def make_case(seed=0):
    """The inputs of the kernel test (numpy fp32): B = 2 samples x 15 tokens x 64 channels, a soft mask that differs across the four
    sub-pixels and across the samples, per-sample sigmas; token 0 of sample 0 carries the bf16 ties in x under m = 1."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((B, N_TOK, CH)).astype(np.float32)
    x0 = g.standard_normal((B, N_TOK, CH)).astype(np.float32)
    noise = g.standard_normal((B, N_TOK, CH)).astype(np.float32)
    mask = g.random((B, N_TOK, 4)).astype(np.float32)
    mask[0, 0] = 1.0
    x[0, 0, :8] = tie_values()
    mask[1, 3] = [0.0, 1.0, 1.0, 0.0]                                                   # exact 0 / 1 inside a soft mask
    sigma_to = np.array([0.7, 0.35], dtype=np.float32)
    return dict(x=x, x0=x0, noise=noise, mask=mask, sigma_to=sigma_to)
