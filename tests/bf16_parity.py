"""Shared checks of the fp64 parity tests (test_hip_train_kernels.py, test_text_encoders.py, test_hip_forward_operands.py, test_hip_gemm_fp64.py,
test_hip_attention_fp64.py, test_hip_vae_fp64.py, test_hip_attention_bwd_fp64.py with attention_bwd_ref.py and test_attention_bwd_ref_cpu.py,
test_hip_attention_ext_fp64.py with attention_ext_ref.py and test_attention_ext_ref_cpu.py,
test_hip_forward_frame_fp64.py with forward_frame_ref.py and test_forward_frame_ref_cpu.py,
test_hip_gemm_f32out_fp64.py with splitk_ref.py and test_splitk_ref_cpu.py): bf16 / fp32
outputs against an fp64 reference, the fp64 GEMM reference with its fp32 summation bound and the fp64 convolution reference built from shifted matmuls."""
import math

import torch

U32 = 2.0 ** -24


def bf16_ulp(ref):
    return torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 7)


def check_bf16(out, ref, floor=0.0, min_equal=0.99, what=''):
    """out (bf16) against ref (fp64): per-element |out - ref| <= ulp_bf16(ref) + floor, and the share equal to RNE(ref) >= min_equal."""
    ref = ref.double()
    err = (out.double() - ref).abs()
    tol = bf16_ulp(ref) + floor
    bad = err > tol
    if bool(bad.any()):
        i = int((err - tol).flatten().argmax())
        raise AssertionError(f'{what}: {int(bad.sum())} of {err.numel()} elements beyond one bf16 ulp; worst out {out.flatten()[i].item()} '
                             f'ref {ref.flatten()[i].item()} tol {torch.as_tensor(tol).expand_as(err).flatten()[i].item():.3e}')
    eq = (out == ref.float().bfloat16()).double().mean().item()
    assert eq >= min_equal, f'{what}: only {eq:.4f} of the elements equal the fp64 reference rounded to nearest even (need {min_equal})'


def check_bf16_bound(out, ref, bound, what=''):
    """out (bf16) against ref (fp64) with a derived per-element bound: |out - ref| <= ulp_bf16(ref) + bound.  Returns the worst err / tol."""
    err = (out.double() - ref).abs()
    tol = bf16_ulp(ref) + bound
    bad = err > tol
    if bool(bad.any()):
        i = int((err - tol).flatten().argmax())
        raise AssertionError(f'{what}: {int(bad.sum())} of {err.numel()} elements beyond the bound; worst out {out.flatten()[i].item()} '
                             f'ref {ref.flatten()[i].item()} tol {tol.flatten()[i].item():.3e}')
    return (err / tol).max().item()


def check_f32(out, ref, bound, what=''):
    """out (fp32) against ref (fp64): per-element |out - ref| <= bound."""
    ref = ref.double()
    err = (out.double() - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64, device=err.device).expand_as(err)
    bad = err > bound
    if bool(bad.any()):
        i = int((err - bound).flatten().argmax())
        raise AssertionError(f'{what}: {int(bad.sum())} of {err.numel()} elements beyond the bound; worst out {out.flatten()[i].item()} '
                             f'ref {ref.flatten()[i].item()} bound {bound.flatten()[i].item():.3e}')


def proj64(a, w, b, kstep=32):
    """a @ w.T + b in fp64 and the fp32 summation bound of the GEMM's accumulation: one rounding per MFMA K-step into the accumulator plus a
    serial chain over one instruction's kstep products, + 1 for the bias (depth K / kstep + kstep + 1).  kstep 32: the bf16 kernels
    (v_mfma_f32_16x16x32_bf16); 128: the fp8 kernels (v_mfma_f32_16x16x128_f8f6f4)."""
    ad, wd = a.double(), w.double()
    y, mag = ad @ wd.T, ad.abs() @ wd.abs().T
    if b is not None:
        y += b.double()
        mag += b.double().abs()
    return y, (a.shape[1] // kstep + kstep + 1) * U32 * mag


def gelu64(x):
    return x * torch.sigmoid(2 * math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3))


def silu64(x):
    return x * torch.sigmoid(x)


def conv64(x_pad, w, b, Ho, Wo, stride=1, oy=0, ox=0, skip=None, kstep=32):
    """The convolution reference of the VAE tests: y[i, j, :] = sum over taps (dy, dx) of x_pad[oy + dy + stride i, ox + dx + stride j, :] @ w[:, :, dy, dx].T + b
    as kh * kw shifted fp64 matmuls on the PADDED NHWC grid x_pad [Hp, Wp, Cin] (w [Cout, Cin, kh, kw], any dtype; no fp64 convolution of the backend is
    used).  skip = (dy, dx): that tap is left out (the mutated references of the teeth checks).  Returns y [Ho, Wo, Cout] fp64, mag = |x| |w| + |b| of the
    same shape and the fp32 summation floor of proj64 for K = kh kw Cin: (K / kstep + kstep + 1) 2^-24 mag."""
    xd, wd = x_pad.double(), w.double()
    co, ci, kh, kw = wd.shape
    y = torch.zeros(Ho, Wo, co, dtype=torch.float64, device=xd.device)
    mag = torch.zeros_like(y)
    for dy in range(kh):
        for dx in range(kw):
            if skip == (dy, dx):
                continue
            xs = xd[oy + dy:oy + dy + stride * (Ho - 1) + 1:stride, ox + dx:ox + dx + stride * (Wo - 1) + 1:stride].reshape(Ho * Wo, ci)
            wt = wd[:, :, dy, dx].T.contiguous()
            y += (xs @ wt).view(Ho, Wo, co)
            mag += (xs.abs() @ wt.abs()).view(Ho, Wo, co)
    if b is not None:
        y += b.double()
        mag += b.double().abs()
    return y, mag, (kh * kw * ci // kstep + kstep + 1) * U32 * mag
