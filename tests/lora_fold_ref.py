"""fp64 reference of ``afx_lora_fold`` (include/arcflow_hip.h) and the per-element criterion its outputs are held to.

The kernel's contract, per element of one adapted linear:

    dst[o, i] = bf16_rne( float(base[o, i]) + sum_j s_j * ( sum_r B_j[o, r] * A_j[r, i] ) )

``fold_reference`` evaluates the argument of the rounding, t, in fp64 on the CPU: the bf16 operands widened exactly, the scales
rounded to fp32 first (that is what the kernel receives) and widened exactly.  Its own error is a few (R + J) 2^-53 relative
roundings, nine orders of magnitude below the bound that follows, and is ignored.

The bound E.  Write u = 2^-24 (the unit roundoff of fp32), R = sum_j r_j and mag = |w| + sum_j |s_j| sum_r |B_j||A_j|.  A product of two
bf16 values has 16 significant bits and is exact in fp32.  A device that accumulates in fp32 commits, in ANY summation order:
  * r_j - 1 additions for adapter j's sum of exact products, each a relative u on a partial sum no larger than sum_r |B_j||A_j|;
  * one multiplication by s_j and one addition into the running total per adapter (a fused multiply-add commits one of the two);
  * one addition of the base weight;
every one of them on a quantity bounded by mag once weighted with its |s_j|.  That is at most R + J + 1 relative roundings of size u to
first order; J + 1 more cover the second-order terms (1 + u)^n - 1 - n u for every n that occurs here (n u < 2^-10), giving

    E = (R + 2 J + 2) * 2^-24 * ( |w| + sum_j |s_j| * sum_r |B_j| |A_j| ).

The criterion.  A device value d passes iff it is the bf16 round-to-nearest-even of SOME number within E of t.  Rounding is monotone, so
this is  rne(t - E) <= d <= rne(t + E):  for E below half a bf16 ulp these are at most two neighbouring bf16 values, and a tie that
falls inside the interval may go either way.  Nothing else may differ and no element is left out.  ``rne_bf16`` rounds fp64 to bf16
directly (no intermediate fp32 rounding, which could move a value onto a tie)."""
import torch

U32 = 2.0 ** -24


def rne_bf16(x: torch.Tensor) -> torch.Tensor:
    """fp64 -> the nearest bf16 value (ties to even), returned as fp64.  bf16 has 8 significant bits: a value in [2^e, 2^(e+1)) is a
    multiple of 2^(e-7); below 2^-126 the spacing stays 2^-133 (subnormals).  torch.round rounds halves to even."""
    x = x.double()
    _, ex = torch.frexp(x)                                  # |x| = m 2^ex, m in [0.5, 1)  ->  e = ex - 1
    e = (ex - 1).clamp(min=-126)
    ulp = torch.ldexp(torch.ones_like(x), e - 7)
    return torch.round(x / ulp) * ulp


def f32(s) -> float:
    """The fp32 value the kernel receives for a python scale, as a python float."""
    return torch.tensor(float(s), dtype=torch.float32).double().item()


def fold_reference(base, A=(), B=(), scales=()):
    """base [O, I], A[j] [r_j, I], B[j] [O, r_j] bf16 (CPU), scales python floats -> (t fp64 [O, I], E fp64 [O, I])."""
    assert base.dtype == torch.bfloat16 and all(a.dtype == torch.bfloat16 for a in A) and all(b.dtype == torch.bfloat16 for b in B)
    t = base.double().cpu().clone()
    mag = t.abs()
    R = 0
    for a, b, s in zip(A, B, scales):
        s = f32(s)
        ad, bd = a.double().cpu(), b.double().cpu()
        t += s * (bd @ ad)
        mag += abs(s) * (bd.abs() @ ad.abs())
        R += a.shape[0]
    J = len(A)
    return t, (R + 2 * J + 2) * U32 * mag


def failing(dev, t, E) -> torch.Tensor:
    """Boolean mask of the elements of the device result (bf16) that violate the criterion against (t, E)."""
    d = dev.double().cpu()
    return (d < rne_bf16(t - E)) | (d > rne_bf16(t + E)) | ~torch.isfinite(d)


def check_fold(dev, t, E, what='') -> float:
    """Raise unless EVERY element passes; returns the share of elements equal to rne(t) (information only)."""
    bad = failing(dev, t, E)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements outside [rne(t - E), rne(t + E)]; first: element {i} '
                             f'device {dev.flatten()[i].item()!r} t {t.flatten()[i].item()!r} E {E.flatten()[i].item():.3e}')
    return (dev.double().cpu() == rne_bf16(t)).double().mean().item()
