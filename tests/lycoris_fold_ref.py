"""fp64 reference of ``afx_lora_fold_terms`` (include/arcflow_hip.h) -- LoRA, LoHa and LoKr terms folded into one linear -- and the per-element
bound its outputs are held to, derived by counting roundings the way tests/lora_fold_ref.py and tests/lora_dora_ref.py do.  Nothing here comes
from what the kernel returns.  The LoHa / LoKr rules are LyCORIS' as restated in the header: they are NOT checked against LyCORIS or ComfyUI.

The contract, per element:

    dst[o, i] = bf16_rne( c[o] w[o, i] + sum_j (g_j[o] s_j) D_j[o, i] ),      c = 1 + sum_{j with gains} (g_j - 1),  g_j = 1 without gains

    LoRA   D = B A                                   B [O, r], A [r, I] bf16
    LoHa   D = (w1_a w1_b) (*) (w2_a w2_b)           w1_a [O, r1], w1_b [r1, I], w2_a [O, r2], w2_b [r2, I] bf16, (*) element by element
    LoKr   D[o, i] = w1[(row0 + o) / c, i / d] * w2[(row0 + o) % c, i % d]       w1 [a, b], w2 [c, d] fp32: rows row0 .. row0 + O of kron(w1, w2)

``terms_reference`` evaluates the argument of the rounding, t, in fp64 from the operands widened exactly (scales rounded to fp32 first: what the
kernel receives).  Its own error is a few hundred 2^-53 relative roundings and is ignored, as in lora_fold_ref.

The bound E.  u = 2^-24.  A product of two bf16 values is exact in fp32; a device that works in fp32 commits, in ANY summation order,
  * LoRA term:  r - 1 additions for the rank sum; with gains one multiplication g s                                  (r, + 3 per term with gains:
                that product and the two operations of c, as lora_dora_ref counts them)
  * LoHa term:  r1 - 1 and r2 - 1 additions for the two rank sums -- each a relative u on a partial sum no larger than P1abs = |w1_a||w1_b|
                (P2abs) -- and ONE rounding of the fp32 product of the two sums; the sums' errors multiply into the product, so to first order
                the product is off by at most (r1 + r2 - 1) u P1abs P2abs                                            (r1 + r2)
  * LoKr term:  ONE rounding of the fp32 product w1 w2                                                                (1)
  * every term: one fused multiply-add of (g s) D into the running total                                             (J)
  * one fused multiply-add c w + total                                                                                (1)
every one of them on a quantity bounded by  mag = (1 + sum |g_j - 1|) |w| + sum_j |g_j s_j| Dabs_j,  Dabs = |B||A|, P1abs P2abs or |w1||w2|.  With
N = sum_j n_j the roundings inside the terms (n_j = r, r1 + r2 or 1) and JD terms with gains that is N + J + 3 JD + 1 first-order roundings; J + 1
more cover the second-order terms ((1 + u)^n - 1 - n u for n u < 2^-10, the cross terms of the LoHa product among them):

    E = (N + 2 J + 3 JD + 2) u mag.            With LoRA terms alone this IS lora_dora_ref's (and, without gains, lora_fold_ref's) t and E.

The criterion is lora_fold_ref's: a device value d passes iff rne_bf16(t - E) <= d <= rne_bf16(t + E); ``LR.check_fold`` / ``LR.failing`` apply it.

``mutate`` builds the wrong references the GPU test must see fail: 'loha_bf16_products' (each LoHa product rounded to bf16 before the multiply),
'loha_add' (the products added), 'lokr_swap_index' (o / c and o % c exchanged), 'lokr_ignore_row0'."""
import torch

import lora_fold_ref as LR

U32 = LR.U32


def loha_delta(w1_a, w1_b, w2_a, w2_b, mutate=None):
    """-> (D fp64 [O, I], Dabs fp64 [O, I], n roundings)."""
    a1, b1, a2, b2 = (x.double().cpu() for x in (w1_a, w1_b, w2_a, w2_b))
    P1, P2 = a1 @ b1, a2 @ b2
    if mutate == 'loha_bf16_products':
        P1, P2 = LR.rne_bf16(P1), LR.rne_bf16(P2)
    D = P1 + P2 if mutate == 'loha_add' else P1 * P2
    return D, (a1.abs() @ b1.abs()) * (a2.abs() @ b2.abs()), w1_b.shape[0] + w2_b.shape[0]


def lokr_delta(w1, w2, row0, O, mutate=None):
    """Rows row0 .. row0 + O of kron(w1, w2) by the index rule, written out -> (D fp64 [O, b d], |D|, 1)."""
    w1, w2 = w1.double().cpu(), w2.double().cpu()
    (a, b), (c, d) = w1.shape, w2.shape
    rows = torch.arange(O) + (0 if mutate == 'lokr_ignore_row0' else row0)
    cols = torch.arange(b * d)
    p, q = rows // c, rows % c
    if mutate == 'lokr_swap_index':
        p, q = q % a, p % c                                 # (the exchanged indices, kept inside the matrices)
    D = w1[p[:, None], (cols // d)[None, :]] * w2[q[:, None], (cols % d)[None, :]]
    return D, D.abs(), 1


def term_delta(term, O, mutate=None):
    if term['kind'] == 'lora':
        A, B = term['A'].double().cpu(), term['B'].double().cpu()
        return B @ A, B.abs() @ A.abs(), A.shape[0]
    if term['kind'] == 'loha':
        return loha_delta(term['w1_a'], term['w1_b'], term['w2_a'], term['w2_b'], mutate)
    return lokr_delta(term['w1'], term['w2'], int(term.get('row0', 0)), O, mutate)


def terms_reference(base, terms=(), mutate=None):
    """base [O, I] bf16 (CPU), terms as ``ops.lora_fold_terms`` takes them (CPU tensors; a LoRA term's 'row_gain' is taken as exact)
    -> (t fp64 [O, I], E fp64 [O, I])."""
    assert base.dtype == torch.bfloat16
    w = base.double().cpu()
    O = w.shape[0]
    t, mag = w.clone(), w.abs()
    c = torch.ones(O, dtype=torch.float64)
    c_abs = torch.ones(O, dtype=torch.float64)
    N = JD = 0
    for term in terms:
        for k in ('A', 'B', 'w1_a', 'w1_b', 'w2_a', 'w2_b'):
            assert k not in term or term[k].dtype == torch.bfloat16, k
        for k in ('w1', 'w2'):
            assert k not in term or term[k].dtype == torch.float32, k
        s = LR.f32(term['scale'])
        D, Dabs, n = term_delta(term, O, mutate)
        N += n
        g = term.get('row_gain')
        if g is None:
            t += s * D
            mag += abs(s) * Dabs
            continue
        assert term['kind'] == 'lora'
        JD += 1
        g = g.double().cpu()
        t += (g * s)[:, None] * D
        mag += (g.abs() * abs(s))[:, None] * Dabs
        c += g - 1.0
        c_abs += (g - 1.0).abs()
    t += (c - 1.0)[:, None] * w
    mag += (c_abs - 1.0)[:, None] * w.abs()
    return t, (N + 2 * len(terms) + 3 * JD + 2) * U32 * mag


def _fma32(x, y, z):
    """fp32 fused multiply-add of fp32 tensors: the product of two fp32 values is exact in fp64 (48 bits), one addition in fp64, one rounding to
    fp32 -- off from a true fma only where the fp64 sum lands within 2^-53 of an fp32 tie."""
    return (x.double() * y.double() + z.double()).float()


def emulate_fp32(base, terms=()):
    """What an fp32 device that follows the kernel's order returns, on the CPU (torch's own summation order inside the matmuls): the rank sums
    in fp32, the LoHa / LoKr product as one fp32 product, one fma per term in term order, the fma with the base, the store's rounding -> bf16."""
    w = base.float().cpu()
    O = w.shape[0]
    tot = torch.zeros_like(w)
    c = torch.ones(O, dtype=torch.float32)
    for term in terms:
        s = torch.tensor(float(term['scale']), dtype=torch.float32)
        if term['kind'] == 'lora':
            D = term['B'].float() @ term['A'].float()
        elif term['kind'] == 'loha':
            D = (term['w1_a'].float() @ term['w1_b'].float()) * (term['w2_a'].float() @ term['w2_b'].float())
        else:
            w1, w2, row0 = term['w1'], term['w2'], int(term.get('row0', 0))
            D = torch.kron(w1, w2)[row0:row0 + O].contiguous()          # an fp32 product per element: torch.kron forms exactly that
        g = term.get('row_gain')
        gs = s.expand(O) if g is None else g.float() * s
        if g is not None:
            c = c + (g.float() - 1.0)
        tot = _fma32(gs[:, None].expand_as(D), D, tot)
    return _fma32(c[:, None].expand_as(w), w, tot).bfloat16()


def loha_operands(O, I, r1, r2, g, target=0.02):
    """bf16 LoHa operands whose two products have a standard deviation of sqrt(target) each, so that the delta is of the size of a weight of
    standard deviation `target` (otherwise the delta disappears under half an ulp of the base and a check shows nothing)."""
    out = []
    for r in (r1, r2):
        std = (target ** 0.5 / r ** 0.5) ** 0.5
        out += [(torch.randn(O, r, generator=g) * std).bfloat16(), (torch.randn(r, I, generator=g) * std).bfloat16()]
    return dict(kind='loha', w1_a=out[0], w1_b=out[1], w2_a=out[2], w2_b=out[3])


def lokr_operands(a, b, c, d, g, target=0.02):
    """fp32 LoKr factors with standard deviation sqrt(target) each."""
    return dict(kind='lokr', w1=torch.randn(a, b, generator=g) * target ** 0.5, w2=torch.randn(c, d, generator=g) * target ** 0.5)
