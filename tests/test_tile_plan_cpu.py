"""``schedule.tile_axis`` / ``schedule.tile_plan``, the host geometry of ``pipe.enhance``: the worked cases, the properties of every plan
for L in 16 .. 300, and the refusals.  Host integer and fp64 arithmetic only.  On the parent commit every test here fails:
``schedule.tile_axis`` does not exist.

On an axis shorter than a tile (t < tile) the rule ``k = 1 + ceil((L - t) / (t - overlap))`` has no value for overlap >= t (L = 40, tile 64,
overlap 32 gives t = 32): the planner caps the overlap at t // 2 there, and the overlap property is checked against min(overlap, t // 2),
which is ``overlap`` itself wherever the axis holds a whole tile."""
import numpy as np
import pytest

from arcflow_amd import schedule

WORKED = [  # L, tile, overlap -> t, origins
    (40, 32, 8, 32, [0, 8]),
    (56, 32, 8, 32, [0, 24]),
    (60, 32, 8, 32, [0, 14, 28]),
    (84, 32, 8, 32, [0, 17, 35, 52]),
    (40, 64, 8, 32, [0, 8]),
    (56, 64, 8, 48, [0, 8]),
    (32, 32, 8, 32, [0]),
]


@pytest.mark.parametrize('L,tile,overlap,t,origins', WORKED)
def test_worked_cases(L, tile, overlap, t, origins):
    got_t, o, start, count, w = schedule.tile_axis(L, tile, overlap)
    assert got_t == t and o.tolist() == origins
    assert o.dtype == np.int32 and start.dtype == np.int32 and count.dtype == np.int32 and w.dtype == np.float32
    assert start.shape == count.shape == (L,) and w.shape == (L, int(count.max()))


def test_worked_weights():
    """40 / 32 / 8: tiles [0, 32) and [8, 40); in the shared span [8, 32) u_0 = 32 - x (falling to 1), u_1 = x - 7 (rising from 1), sum 25."""
    _, _, start, count, w = schedule.tile_axis(40, 32, 8)
    x = np.arange(40)
    assert count.tolist() == [1] * 8 + [2] * 24 + [1] * 8 and start.tolist() == [0] * 32 + [1] * 8
    assert np.array_equal(w[:8], np.tile(np.float32([1, 0]), (8, 1))) and np.array_equal(w[32:], np.tile(np.float32([1, 0]), (8, 1)))
    assert np.array_equal(w[8:32, 0], ((32 - x[8:32]) / 25.0).astype(np.float32)) and np.array_equal(w[8:32, 1], ((x[8:32] - 7) / 25.0).astype(np.float32))


@pytest.mark.parametrize('tile,overlap', [(32, 0), (32, 8), (32, 16), (64, 32), (48, 5)])
def test_properties(tile, overlap):
    for L in range(16, 301):
        t, o, start, count, w = schedule.tile_axis(L, tile, overlap)
        k = o.size
        assert t == min(tile, 16 * (L // 16)) and t % 16 == 0
        assert o[0] == 0 and o[-1] + t == L, (L, o)
        assert (np.diff(o) > 0).all(), (L, o)
        ov = min(overlap, t // 2)
        assert ov == overlap or t < tile
        assert (o[:-1] + t - o[1:] >= ov).all(), (L, o)                                  # neighbours share at least the overlap
        assert k == (1 if L == t else 1 + -(-(L - t) // (t - ov)))
        assert count.min() >= 1 and count.max() <= 4 == schedule.AFX_TILE_MAX_TAPS, (L, count.max())
        x = np.arange(L)
        covers = (o[None, :] <= x[:, None]) & (x[:, None] < o[None, :] + t)             # [L, k]
        assert np.array_equal(covers.sum(1), count) and np.array_equal(covers.argmax(1), start)
        last = k - 1 - covers[:, ::-1].argmax(1)
        assert np.array_equal(last - start + 1, count)                                  # the covering tiles are consecutive
        s64, c64, w64 = schedule.tile_axis_weights(L, t, o)
        assert np.array_equal(s64, start) and np.array_equal(c64, count) and w64.dtype == np.float64
        assert np.abs(w64.sum(1) - 1.0).max() <= 1e-15
        assert np.array_equal(w, w64.astype(np.float32))                                # rounded to fp32 once
        assert (np.abs(w.astype(np.float64).sum(1) - 1.0) <= 2 * count * 2.0 ** -24).all()          # 2 ulp (of 1, below it) per tap
        live = np.arange(w.shape[1])[None] < count[:, None]                             # [L, taps]
        assert (w[count == 1, 0] == np.float32(1.0)).all() and (w[~live] == 0).all() and (w[live] > 0).all()
        assert w[0, 0] == 1.0 and count[0] == 1 and w[-1, 0] == 1.0 and count[-1] == 1  # full weight on the canvas borders


def test_weights_are_the_linear_cross_fade():
    """u_i(x) = min(dl, dr) stated per element, against the vectorised planner, on a three-tile overlap (84 / 32 / 8: origins 0 17 35 52)."""
    L, t = 84, 32
    _, o, start, count, w = schedule.tile_axis(L, 32, 8)
    k = o.size
    for x in range(L):
        u = {}
        for i in range(k):
            if o[i] <= x < o[i] + t:
                dl = x - o[i] + 1 if i > 0 else np.inf
                dr = o[i] + t - x if i < k - 1 else np.inf
                u[i] = 1.0 if np.isinf(min(dl, dr)) else float(min(dl, dr))
        assert sorted(u) == list(range(start[x], start[x] + count[x]))
        tot = sum(u.values())
        assert [np.float32(u[i] / tot) for i in sorted(u)] == w[x, :count[x]].tolist()


def test_tile_plan_is_both_axes():
    p = schedule.tile_plan(60, 84, 32, 8)
    assert (p.H, p.W, p.tile, p.overlap, p.th, p.tw, p.ky, p.kx, p.T) == (60, 84, 32, 8, 32, 32, 3, 4, 12)
    assert p.oy.tolist() == [0, 14, 28] and p.ox.tolist() == [0, 17, 35, 52]
    for got, want in zip(p.y + p.x, schedule.tile_axis(60, 32, 8)[2:] + schedule.tile_axis(84, 32, 8)[2:]):
        assert np.array_equal(got, want)
    q = schedule.tile_plan(40, 56, 64, 8)                                                # non-square tiles: all the short axes have
    assert (q.th, q.tw, q.ky, q.kx) == (32, 48, 2, 2)


def test_refusals_name_the_argument():
    for bad in (15, 0, -3, 16.0, True):
        with pytest.raises(ValueError, match='^L:'):
            schedule.tile_axis(bad, 32, 8)
    for bad in (16, 31, 40, 0, 33, 64.0):
        with pytest.raises(ValueError, match='^tile:'):
            schedule.tile_axis(100, bad, 0)
    for bad in (-1, 17, 8.0, 32):
        with pytest.raises(ValueError, match='^overlap:'):
            schedule.tile_axis(100, 32, bad)
    schedule.tile_axis(100, 32, 16)                                                      # tile // 2 itself is allowed
    with pytest.raises(ValueError, match='H, W'):
        schedule.tile_plan(12, 56, 32, 8)
    with pytest.raises(ValueError, match='^tile:'):
        schedule.tile_plan(40, 56, 40, 8)
    with pytest.raises(ValueError, match='^overlap:'):
        schedule.tile_plan(40, 56, 32, 17)
