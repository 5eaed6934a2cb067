"""The fp64 reference of afx_tiles_merge (tests/tiles_ref.py) on the very inputs of the kernel test (tests/test_hip_tiles_fp64.py), without
a GPU: the admissible byte sets are narrow (at most 1 % of the elements admit two bytes, none admits three -- a condition on the inputs,
met by the reference alone), each mutant leaves the true admissible set somewhere, and the reference agrees with a per-pixel statement of
the formula.  On the parent commit every test here fails: ``schedule.tile_plan``, which the reference takes its tables from, does not exist."""
import numpy as np
import pytest

import tiles_ref as T

_cache = {}


def _case(case):
    if case not in _cache:
        plan, tiles = T.plan_of(case), T.inputs(case)
        r, E = T.merge(tiles, plan)
        for a in (tiles, r, E):
            a.setflags(write=False)
        _cache[case] = (plan, tiles, r, E)
    return _cache[case]


@pytest.mark.parametrize('case', list(T.CASES))
def test_admissible_sets_are_narrow(case):
    plan, tiles, r, E = _case(case)
    lo, hi = T.admissible(r, E)
    width = hi - lo
    print(f'{case}: {plan.ky} x {plan.kx} tiles of {plan.th} x {plan.tw}; {100 * float((width == 1).mean()):.4f} % of the elements admit two bytes; '
          f'max 255 E = {255 * E.max():.2e}')
    assert r.shape == (plan.H, plan.W, 3) and (E > 0).all() and 255 * E.max() < 2e-4
    assert width.min() >= 0 and width.max() <= 1 and float((width == 1).mean()) <= 0.01
    assert lo.min() == 0 and hi.max() == 255 and (r < 0).any() and (r > 1).any()          # the clamp acts on both ends


def test_reference_is_the_formula_per_pixel():
    """The vectorised gather against two nested loops over the covering tiles, on the three-tile overlap."""
    plan, tiles, r, _ = _case('three_by_four')
    (sy, cy, wy), (sx, cx, wx) = plan.y, plan.x
    rng = np.random.default_rng(1)
    for y, x in zip(rng.integers(0, plan.H, 200), rng.integers(0, plan.W, 200)):
        acc = np.zeros(3)
        for a in range(cy[y]):
            iy = sy[y] + a
            for b in range(cx[x]):
                ix = sx[x] + b
                v = tiles[iy * plan.kx + ix, :, y - plan.oy[iy], x - plan.ox[ix]].astype(np.float64)
                acc += float(wy[y, a]) * float(wx[x, b]) * (0.5 * v + 0.5)
        assert np.abs(acc - r[y, x]).max() <= 1e-15
    assert cy.max() == 3 and cx.max() == 2                                               # rows 28 .. 31 lie in all three tile rows


def test_cut_then_merge_is_the_identity_in_the_reference():
    """Tiles cut from one canvas agree wherever they overlap, and the weights sum to 1: r is the canvas' 0.5 v + 0.5 up to the fp32 weights."""
    plan = T.plan_of('three_by_four')
    canvas = (np.random.default_rng(2).random((3, plan.H, plan.W), dtype=np.float32) * 2 - 1).astype(np.float32)
    r, E = T.merge(T.cut(canvas, plan), plan)
    assert np.abs(r - (0.5 * canvas.astype(np.float64) + 0.5).transpose(1, 2, 0)).max() <= 8 * T.U


@pytest.mark.parametrize('mutant', T.MUTANTS)
def test_mutants_leave_the_admissible_set(mutant):
    rejected = {}
    for case in ('two_by_two', 'three_by_four', 'non_square', 'two_groups'):
        plan, tiles, r, E = _case(case)
        lo, hi = T.admissible(r, E)
        mlo, mhi = T.admissible(r, E, trunc=True) if mutant == 'trunc' else T.admissible(*T.merge(tiles, plan, mutant=mutant))
        rejected[case] = float(((mlo > hi) | (mhi < lo)).mean())                          # no byte is admissible under both
    print(mutant, {k: f'{100 * v:.1f} %' for k, v in rejected.items()})
    assert len(T.MUTANTS) >= 5 and min(rejected.values()) > 0.0, mutant
