"""Shared checks of the fp64 parity tests (test_hip_train_kernels.py, test_text_encoders.py): bf16 outputs against an fp64 reference."""
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
