"""The fp64 reference of afx_color_fix (tests/color_fix_ref.py) checked against itself, without a GPU: its bound E is small enough to see a
wrong tap, every mutant of either rule leaves [r - E, r + E] on more than half of the elements of at least one case, and the
two-decomposition form high(e) + low(s') equals the one chain on the difference that the header fixes.  On the parent commit the module
does not exist and every test here fails."""
import numpy as np
import pytest

import color_fix_ref as CR

# the cases of the mutant checks: the shared ones without the 66000-row one (a megapixel of fp64 per mutant shows nothing new) ...
SMALL = [c for c in CR.CASES if c[4] * c[5] * c[1] * c[3] < 200000]


@pytest.fixture(scope='module')
def inputs():
    return {c[0]: CR.make_case(c) for c in CR.CASES}


def _flat_inputs():
    """... and two AdaIN ones: channel 0 of the edit constant, channel 1 of low contrast (a variance near the 1e-5 of the rule)."""
    rng = np.random.default_rng(5)
    e = rng.uniform(-1.2, 1.2, (1, 3, 24, 40)).astype(np.float32)
    e[0, 0] = np.float32(0.3)
    e[0, 1] = (0.3 + 0.01 * rng.uniform(-1, 1, (24, 40))).astype(np.float32)
    return e, rng.uniform(0, 1, (1, 3, 24, 40)).astype(np.float32)


def test_bound_is_far_below_a_wrong_tap(inputs):
    for case in CR.CASES:
        e, s, _ = inputs[case[0]]
        r, E = CR.wavelet_ref(e, s)
        assert np.isfinite(r).all() and 0 < E.max() < 2.0 ** -16, (case[0], E.max())
        r, E, stats, stats_E, a = CR.adain_ref(e, s)
        assert np.isfinite(r).all() and 0 < E.max() < 2.0 ** -16 * max(1.0, np.abs(a).max()), (case[0], E.max(), np.abs(a).max())
        assert stats_E.max() < 1e-6 and (stats[..., 1] > 0).all() and (stats[..., 3] > 0).all()


def _moved(ref_fn, e, s, mutate):
    r, E = ref_fn(e, s)[:2]
    with np.errstate(all='ignore'):
        m = ref_fn(e, s, mutate=mutate)[0]
    return np.mean(~(np.abs(m - r) <= E))                   # a NaN or inf counts as moved


@pytest.mark.parametrize('mutate', ['dilations_12345', 'zero_pad', 'four_levels', 'e_minus_s', 'src01_ignored', 'low_of_e_kept'])
def test_every_wavelet_mutant_is_visible(inputs, mutate):
    moved = {c[0]: _moved(CR.wavelet_ref, *inputs[c[0]][:2], mutate) for c in SMALL}
    assert max(moved.values()) > 0.5, moved


@pytest.mark.parametrize('mutate', ['unbiased', 'no_eps', 'wrong_channel', 'src01_ignored'])
def test_every_adain_mutant_is_visible(inputs, mutate):
    moved = {c[0]: _moved(CR.adain_ref, *inputs[c[0]][:2], mutate) for c in SMALL}
    e, s = _flat_inputs()
    r, E, _, _, a = CR.adain_ref(e, s)
    assert np.isfinite(r).all() and np.isfinite(E).all() and a[0, 0] > 100          # the constant channel: sd_e = sqrt(1e-5)
    with np.errstate(all='ignore'):
        m = CR.adain_ref(e, s, mutate=mutate)[0]
    for ch, name in enumerate(('constant_channel', 'low_contrast_channel', 'plain_channel')):
        moved[name] = np.mean(~(np.abs(m[:, ch] - r[:, ch]) <= E[:, ch]))
    assert max(moved.values()) > 0.5, moved
    if mutate == 'no_eps':
        assert moved['constant_channel'] > 0.5, moved


def test_two_decompositions_equal_the_chain_on_the_difference(inputs):
    for case in SMALL:
        e, s, _ = inputs[case[0]]
        r, _ = CR.wavelet_ref(e, s)
        assert np.abs(CR.wavelet_two_decompositions(e, s) - r).max() < 1e-12, case[0]


def test_exact_inputs_stay_exact():
    """s = e + 0.25 on multiples of 2^-10: every operation of the rule is exact and out = e + 0.25, borders included."""
    rng = np.random.default_rng(3)
    e = (rng.integers(-1024, 1025, (1, 2, 20, 37)) / 1024.0).astype(np.float32)
    r, _ = CR.wavelet_ref(e, e + np.float32(0.25), src01=False)
    assert np.array_equal(r, e.astype(np.float64) + 0.25)
    assert not np.array_equal(CR.wavelet_ref(e, e + np.float32(0.25), src01=False, mutate='zero_pad')[0], r)


def test_bf16_case_holds_bf16_values(inputs):
    e, _, bf16 = inputs['odd_bf16']
    assert bf16 and np.array_equal(CR.bf16_round(e), e) and (e.view(np.uint32) & 0xffff == 0).all()
    import torch
    x = np.random.default_rng(0).uniform(-1.2, 1.2, 4096).astype(np.float32)
    assert np.array_equal(CR.bf16_round(x), torch.from_numpy(x).bfloat16().float().numpy())
