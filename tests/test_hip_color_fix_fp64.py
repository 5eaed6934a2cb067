"""afx_color_fix on the GPU against the fp64 reference of tests/color_fix_ref.py: EVERY element of every case satisfies |got - r| <= E in
both modes (E from the fp32 roundings alone, derived in that file), ``stats`` is within its fp64 bound, and the exact properties of the
header hold bit for bit -- s = e returns e, an exactly representable shift returns e + 0.25 up to the borders, a batch equals its single
calls, two runs agree, the per-pass form equals the fused one, and the bytes around ``out`` stay.  On the parent commit every test here
fails: ``ops.color_fix`` does not exist."""
import numpy as np
import pytest
import torch

import color_fix_ref as CR

pytestmark = pytest.mark.gpu

IDS = [c[0] for c in CR.CASES]


@pytest.fixture(scope='module')
def data():
    """Per case: the inputs on the host and on the GPU; computed once, shared, never modified."""
    out = {}
    for case in CR.CASES:
        e, s, bf16 = CR.make_case(case)
        eg = torch.from_numpy(e).cuda()
        out[case[0]] = dict(e=e, s=s, eg=eg.bfloat16() if bf16 else eg, sg=torch.from_numpy(s).cuda(), bf16=bf16)
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def _fix(e, s, mode, **kw):
    from arcflow_amd import ops
    out = ops.color_fix(e, s, mode, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('name', IDS)
def test_wavelet_every_element_within_the_bound(data, name):
    d = data[name]
    if d['bf16']:
        assert torch.equal(d['eg'].float().cpu(), torch.from_numpy(d['e']))           # the cast lost nothing
    r, E = CR.wavelet_ref(d['e'], d['s'])
    got = _fix(d['eg'], d['sg'], 'wavelet')
    assert got.dtype == torch.float32 and got.shape == d['eg'].shape
    err = np.abs(got.cpu().numpy().astype(np.float64) - r)
    print(f'{name}: wavelet max err {err.max():.3e}, max err / E {(err / E).max():.3f}, max E {E.max():.3e}')
    assert np.isfinite(err).all() and (err <= E).all(), (name, (err / E).max(), int((err > E).sum()))
    levels = _fix(d['eg'], d['sg'], 'wavelet_levels')                                  # the per-pass form: the same bits
    assert torch.equal(_bits(levels), _bits(got)), (name, int((_bits(levels) != _bits(got)).sum()))
    assert torch.equal(_bits(_fix(d['eg'], d['sg'], 'wavelet')), _bits(got))           # and a second run


@pytest.mark.parametrize('name', IDS)
def test_adain_every_element_and_stats_within_the_bound(data, name):
    d = data[name]
    r, E, stats, stats_E, a = CR.adain_ref(d['e'], d['s'])
    B, Cn = d['e'].shape[:2]
    st = torch.full((B, Cn, 4), float('nan'), dtype=torch.float64, device='cuda')
    got = _fix(d['eg'], d['sg'], 'adain', stats=st)
    err = np.abs(got.cpu().numpy().astype(np.float64) - r)
    serr = np.abs(st.cpu().numpy() - stats)
    print(f'{name}: adain max err {err.max():.3e}, max err / E {(err / E).max():.3f}, max E {E.max():.3e}, stats err / bound {(serr / stats_E).max():.3e}')
    assert np.isfinite(err).all() and (err <= E).all(), (name, (err / E).max(), int((err > E).sum()))
    assert np.isfinite(serr).all() and (serr <= stats_E).all(), (name, (serr / stats_E).max())
    again = _fix(d['eg'], d['sg'], 'adain')                                            # without stats, a second run: equal bits
    assert torch.equal(_bits(again), _bits(got))


@pytest.mark.parametrize('mode', ['wavelet', 'wavelet_levels', 'adain'])
def test_identical_source_returns_the_edit(data, mode):
    for name in ('clamp_both_sides', 'tiles_and_broadcast', 'odd_bf16'):
        e = data[name]['eg']
        src = e.float().contiguous()
        st = torch.zeros(*e.shape[:2], 4, dtype=torch.float64, device='cuda')
        got = _fix(e, src, mode, src01=False, stats=st)
        assert torch.equal(_bits(got), _bits(e.float())), (name, mode)                 # adain: a == 1 and b == 0
        if mode == 'adain':
            assert torch.equal(st[..., 0], st[..., 2]) and torch.equal(st[..., 1], st[..., 3])


@pytest.mark.parametrize('mode', ['wavelet', 'wavelet_levels'])
def test_exact_shift_is_exact_up_to_the_borders(mode):
    """s = e + 0.25 on multiples of 2^-10 in [-1, 1]: every operation is exact; zero padding would fail at the borders."""
    g = torch.Generator().manual_seed(4)
    for shape in ((1, 2, 20, 37), (1, 1, 70, 150), (1, 1, 3, 1)):
        e = (torch.randint(-1024, 1025, shape, generator=g).float() / 1024).cuda()
        got = _fix(e, (e + 0.25).contiguous(), mode, src01=False)
        assert torch.equal(_bits(got), _bits(e + 0.25)), (shape, mode)


@pytest.mark.parametrize('mode', ['wavelet', 'adain'])
def test_a_batch_equals_its_single_calls(data, mode):
    for name in ('tiles_and_broadcast', 'odd_bf16'):
        d = data[name]
        both = _fix(d['eg'], d['sg'], mode)
        for b in range(2):
            sb = d['sg'] if d['sg'].shape[0] == 1 else d['sg'][b:b + 1]
            assert torch.equal(_bits(_fix(d['eg'][b:b + 1], sb, mode)), _bits(both[b:b + 1])), (name, mode, b)


@pytest.mark.parametrize('mode', ['wavelet', 'wavelet_levels', 'adain'])
def test_guard_bytes_around_out_stay_and_operands_are_checked(data, mode):
    from arcflow_amd import _lib, ops
    d = data['odd_bf16']
    n = d['eg'].numel()
    pad = 4096
    buf = torch.full((n + 2 * pad,), -7.25, dtype=torch.float32, device='cuda')
    out = buf[pad:pad + n].view(d['eg'].shape)
    got = _fix(d['eg'], d['sg'], mode, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(_bits(out), _bits(_fix(d['eg'], d['sg'], mode)))
    assert (buf[:pad] == -7.25).all() and (buf[pad + n:] == -7.25).all()
    e32 = d['eg'].float()
    for bad in (dict(out=e32), dict(out=d['sg'])):                                     # in place: refused, and nothing is written
        keep = bad['out'].clone()
        with pytest.raises(_lib.ArcflowHipError, match='overlaps'):
            ops.color_fix(e32, d['sg'], mode, **bad)
        assert torch.equal(_bits(bad['out']), _bits(keep))
    with pytest.raises(ValueError, match='source'):
        ops.color_fix(e32, d['sg'][:, :, :, :64], mode)                                 # another shape (and not contiguous)
    with pytest.raises(ValueError, match='source'):
        ops.color_fix(e32, d['sg'].double(), mode)
    with pytest.raises(ValueError, match='edit'):
        ops.color_fix(e32.half(), d['sg'], mode)
    with pytest.raises(ValueError, match='edit'):
        ops.color_fix(e32.permute(0, 1, 3, 2), d['sg'].permute(0, 1, 3, 2), mode)
    with pytest.raises(_lib.ArcflowHipError, match='GPU tensors only'):
        ops.color_fix(e32, d['sg'].cpu(), mode)
