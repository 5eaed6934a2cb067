"""tests/splitk_ref.py on the CPU: the chunk arithmetic, the fp32 emulation of the split-K rounding points inside the derived bound, the five
mutated references outside it, and the row quantiser's admissible sets on the device test's own inputs."""
import pytest
import torch
from bf16_parity import bf16_ulp, check_bf16, check_f32
from splitk_ref import (MUTANTS, QUANT_KS_REGISTER, QUANT_KS_TWO_PASS, check_quant_codes, chunk_ranges, e4m3_ord, mutants_for, quant_admissible,
                        quant_inputs, quant_scale_f32, rne_e4m3, splitk_chunks, splitk_emulate_f32, splitk_mutant, splitk_operands, splitk_ref)

TOY = (40, 24, 640, 4)       # M, N, K, split_k: per 3, four chunks, the last one a single K-tile


def test_chunk_arithmetic():
    """The cases the device test quotes, and for every (nk, split_k): no empty chunk, the ranges tile [0, K), and the per the kernel recomputes
    from the chunk count equals the per the entry point cut the chunks with."""
    assert splitk_chunks(130, 264, 640, 4) == (4, 3) and chunk_ranges(640, 4)[-1] == (576, 640)
    assert splitk_chunks(77, 72, 128, 16) == (2, 1)
    assert splitk_chunks(300, 520, 1024, 16) == (16, 1)
    assert splitk_chunks(64, 8, 64, 0) == (1, 1) and splitk_chunks(200, 256, 512, 1) == (1, 8)
    assert splitk_chunks(162, 3584, 18944, 16) == (16, 19) and chunk_ranges(18944, 16)[-1] == (15 * 19 * 64, 18944)      # last chunk: 11 tiles
    assert splitk_chunks(512, 4096, 10240, 8) == (8, 20)
    assert splitk_chunks(77, 768, 3072, 0) == (12, 4)          # 3 tiles of 256: 171 chunks wanted, at least 4 K-tiles each
    for nk in range(1, 300):
        for sk in range(1, 40):
            nslab, per = splitk_chunks(256, 256, nk * 64, sk)
            r = chunk_ranges(nk * 64, nslab)
            assert (nk + nslab - 1) // nslab == per, (nk, sk)
            assert r[0][0] == 0 and r[-1][1] == nk * 64 and all(a[1] == b[0] for a, b in zip(r, r[1:])) and all(k1 > k0 for k0, k1 in r)


def test_emulation_inside_the_bound():
    """The fp32 emulation of the kernels' rounding points (40 x 24 x 640, 4 chunks, bias and residual) against the fp64 reference: the bf16
    output within one ulp + the bound, every slab within its own bound.  Measured: worst err / tol 0.50 for the output (the bf16 rounding itself:
    half an ulp), worst err / bound 0.021 for the slabs -- the bound is a worst case over a depth of 2 per + 32 roundings; random roundings
    cancel."""
    M, N, K, sk = TOY
    a, w, b, r = splitk_operands(M, N, K, True, True, seed=1)
    nslab, per = splitk_chunks(M, N, K, sk)
    assert (nslab, per) == (4, 3)
    y, bound, parts = splitk_ref(a, w, b, r, nslab)
    out, slabs = splitk_emulate_f32(a, w, b, r, nslab)
    check_bf16(out, y, floor=bound, what='emulation')
    worst = ((out.double() - y).abs() / (bf16_ulp(y) + bound)).max().item()
    ws = 0.0
    for s, (p, bs) in enumerate(parts):
        check_f32(slabs[s], p, bs, what=f'emulation slab {s}')
        ws = max(ws, ((slabs[s].double() - p).abs() / bs).max().item())
    print(f'split-K emulation: worst err / tol {worst:.3f} (output), {ws:.4f} (slabs)')
    assert worst <= 1.0 and ws <= 1.0


@pytest.mark.parametrize('kind', MUTANTS)
def test_mutant_outside_the_bound(kind):
    """Each mutated reference leaves the bound against the true reference on at least one element, and the emulation (which passes against the true
    reference) is rejected against it."""
    M, N, K, sk = TOY
    a, w, b, r = splitk_operands(M, N, K, True, True, seed=1)
    nslab, _ = splitk_chunks(M, N, K, sk)
    assert kind in mutants_for(M, nslab, True, True)
    y, bound, _ = splitk_ref(a, w, b, r, nslab)
    ym = splitk_mutant(kind, a, w, b, r, nslab)
    assert bool(((ym - y).abs() > 2 * (bf16_ulp(y) + bound)).any()), kind          # beyond the tolerance on both sides of any admissible output
    out, _ = splitk_emulate_f32(a, w, b, r, nslab)
    with pytest.raises(AssertionError, match='beyond one bf16 ulp'):
        check_bf16(out, ym, floor=bound, min_equal=0.0, what=kind)


def test_rne_e4m3_is_the_format():
    """rne_e4m3 against the format's own table: every finite code is a fixed point, every midpoint of two neighbours goes to the even code."""
    codes = torch.arange(0, 0x7f, dtype=torch.uint8)
    vals = codes.view(torch.float8_e4m3fn).double()
    assert torch.equal(rne_e4m3(vals), vals) and torch.equal(rne_e4m3(-vals), -vals)
    mid = (vals[:-1] + vals[1:]) / 2
    even = torch.where(codes[:-1] % 2 == 0, vals[:-1], vals[1:])
    assert torch.equal(rne_e4m3(mid), even)
    assert torch.equal(rne_e4m3(mid * (1 + 2.0 ** -40)), vals[1:]) and torch.equal(rne_e4m3(mid * (1 - 2.0 ** -40)), vals[:-1])


@pytest.mark.parametrize('K', QUANT_KS_TWO_PASS + QUANT_KS_REGISTER)
def test_quantiser_two_code_share(K):
    """On the device test's inputs the admissible set has two codes for at most 0.5 % of the elements.  Measured share: 0 at K = 8 and 512,
    3.4e-6 at 1152, 1.1e-6 at 3584, 1.9e-6 at 16384, 2.5e-6 at 3072, 1.5e-6 at 15360 (plain randn rows gave 0.40 - 0.61 %: quant_inputs says
    why and what it plants against it).  The fp32 emulation of the kernel's arithmetic passes the check the kernel will be held to; a code one
    step off, a flipped sign and a NaN code do not."""
    x = quant_inputs(K)
    sc = quant_scale_f32(x)
    assert sc[7].item() == 2.0 ** -6 and 0 < sc[3].item() < 1e-14 and sc[5].item() == (torch.tensor(2000.0) / 448).item()
    assert bool((x[3] == 0).all()) and x[5].float().abs().sort().values[-2].item() <= 1.0 and x.stride(0) == K + 64
    inv = 1.0 / sc
    q = (x.float() * inv[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    share = check_quant_codes(x, q, sc, what=f'emulation K={K}')
    print(f'quantiser K={K}: two-code share {share:.2e}')
    lo, hi, two = quant_admissible(x, sc)
    assert not bool(two[7].any()) and not bool(two[3].any())              # exact rows: one code each
    # teeth: one code moved by one step where there is a single admissible code, and one sign flipped
    i = int((~two).flatten().nonzero()[K // 2])
    for bad in (q.flatten()[i].item() ^ 1, ):
        q2 = q.clone()
        q2.view(-1)[i] = bad
        with pytest.raises(AssertionError, match='outside their admissible set'):
            check_quant_codes(x, q2, sc)
    j = int((e4m3_ord(q).abs() > 0).flatten().nonzero()[0])
    q3 = q.clone()
    q3.view(-1)[j] ^= 0x80
    with pytest.raises(AssertionError, match='outside their admissible set'):
        check_quant_codes(x, q3, sc)
    q4 = q.clone()
    q4.view(-1)[j] = 0x7f                                                   # a NaN code
    with pytest.raises(AssertionError, match='outside their admissible set'):
        check_quant_codes(x, q4, sc)
