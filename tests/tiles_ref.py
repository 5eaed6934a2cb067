"""fp64 numpy statement of afx_tiles_merge on the same fp32 tables the kernel gets (``schedule.tile_plan``), with a per-element error bound E
and the set of bytes that bound admits.

``merge(tiles, plan)`` -> (r, E), both fp64 [H, W, 3]: with v_ab the value of tile (start_y[y] + a, start_x[x] + b) at the pixel, p_ab = 0.5 v_ab
+ 0.5 and the plan's fp32 weights taken as they are,
    r = sum_{a < count_y[y]} wy[y, a] sum_{b < count_x[x]} wx[x, b] p_ab.

Where E comes from (u = 2^-24, half an fp32 ulp relative).  The kernel computes p_ab = fma(0.5, v_ab, 0.5), inner_a = the fma chain over b from
0, acc = the fma chain over a from 0, byte = rint(fl(255 clamp(acc, 0, 1))).  With n_x = count_x[x], n_y = count_y[y] (at most 4 each) and
A = sum_a sum_b wy wx |p_ab| (every term of r with its sign dropped):
  * p_ab: one rounding, u |p_ab|; it reaches acc through the weights: u A;
  * the inner chain: n_x fmas, each one rounding of a partial sum bounded by sum_b wx |p_ab|: n_x u sum_b wx |p_ab|, through wy: n_x u A;
  * the outer chain: n_y fmas on partial sums bounded by A: n_y u A;
  * the scaling by 255 before rint: one more rounding, relative to clamp(acc) <= |r| up to the above: u |r|;
  * second-order terms (products of two of the above, each below 2^-20 of its operand): covered by one further unit u A.
    E = u ((n_x + n_y + 2) A + |r|)                    (at most 11 u x 1.1 = 7.2e-7 for |v| <= 1.2: 255 E < 1.9e-4 of a byte step)
No constant is fitted to the kernel.  The clamp is 1-Lipschitz and 255 x and rint are monotone, so a byte q is admissible iff
rne(255 clamp(r - E, 0, 1)) <= q <= rne(255 clamp(r + E, 0, 1))  (``admissible``, the rule of tests/image_paste_ref.py).

Mutants (``mutant=``), each a wrong statement that must leave the admissible set somewhere: 'swap' (the axes' tables exchanged between the
taps: wy[y, b] wx[x, a] weighs p_ab), 'unnormalised' (the ramps u_i(x) themselves for the weights, not divided by their sum), 'origin' (every
in-tile row and column one too small: an origin off by one), 'half' (0.5 v + 0.5 dropped: p = v), 'order' (tile index ix ky + iy, the
transposed stack) and ``admissible(..., trunc=True)`` (truncation in place of round-to-nearest-even).
"""
import numpy as np

U = 2.0 ** -24
MUTANTS = ('swap', 'unnormalised', 'origin', 'half', 'order', 'trunc')

# The shapes of the kernel test (tests/test_hip_tiles_fp64.py), shared with the CPU test that shows the admissible sets narrow and the
# mutants separable at exactly these shapes: canvas H x W, tile, overlap.
CASES = {
    'two_by_two': (40, 56, 32, 8),              # 2 x 2 tiles of 32 x 32, overlaps of 24 rows and 8 columns
    'three_by_four': (60, 84, 32, 8),           # 3 x 4 tiles, rows 28 .. 31 lie in three tiles
    'non_square': (40, 56, 64, 8),              # tile 64 on short axes: 2 x 2 tiles of 32 x 48
    'one_tile': (32, 32, 32, 8),                # the canvas is the tile: every weight is 1
    'no_overlap': (60, 84, 32, 0),              # overlap 0: only what the even spread leaves (4 rows; 6 or 7 columns)
    'two_groups': (36, 300, 64, 16),            # W = 256 + 44: two work-group strips, the second partly filled; tiles of 32 x 64
    'many_rows': (66000, 16, 1024, 128),        # more rows than the grid's 65535: the row loop's second trip; 74 tiles of 1024 x 16
}


def plan_of(case):
    from arcflow_amd import schedule
    return schedule.tile_plan(*CASES[case])


def inputs(case, seed=0):
    """-> tiles fp32 [T, 3, th, tw] uniform in [-1.2, 1.2): p = 0.5 v + 0.5 covers [-0.1, 1.1), so the clamp acts on both ends."""
    p = plan_of(case)
    rng = np.random.default_rng(seed + sum(map(ord, case)))
    return (rng.random((p.T, 3, p.th, p.tw), dtype=np.float32) * np.float32(2.4) - np.float32(1.2)).astype(np.float32)


def _ramps(L, t, o, start, taps):
    """u_i(x) of the planner's rule for tile start[x] + a, [L, taps] fp64 (0 where the tap does not exist): the 'unnormalised' mutant."""
    k, x = o.size, np.arange(L)
    u = np.zeros((L, taps))
    for a in range(taps):
        i = np.minimum(start + a, k - 1)
        ok = (start + a < k) & (o[i] <= x) & (x < o[i] + t)
        dl = np.where(i > 0, x - o[i] + 1, np.inf)
        dr = np.where(i < k - 1, o[i] + t - x, np.inf)
        m = np.minimum(dl, dr)
        u[:, a] = np.where(ok, np.where(np.isinf(m), 1.0, m), 0.0)
    return u


def merge(tiles, plan, mutant=None):
    tiles = np.asarray(tiles)
    assert tiles.dtype == np.float32 and tiles.shape == (plan.T, 3, plan.th, plan.tw)
    H, W, th, tw, ky, kx = plan.H, plan.W, plan.th, plan.tw, plan.ky, plan.kx
    oy, ox = plan.oy.astype(np.int64), plan.ox.astype(np.int64)
    (sy, cy, wy), (sx, cx, wx) = plan.y, plan.x
    assert wy.dtype == np.float32 and wx.dtype == np.float32
    sy, cy, sx, cx = (a.astype(np.int64) for a in (sy, cy, sx, cx))
    wy4, wx4 = np.zeros((H, 4)), np.zeros((W, 4))
    wy4[:, :wy.shape[1]], wx4[:, :wx.shape[1]] = wy, wx                     # fp32 values, held in fp64
    if mutant == 'unnormalised':
        wy4, wx4 = _ramps(H, th, oy, sy, 4), _ramps(W, tw, ox, sx, 4)
    r, A = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    shift = 1 if mutant == 'origin' else 0
    Y, X = np.arange(H)[:, None], np.arange(W)[None, :]
    for a in range(int(cy.max())):
        iy = np.minimum(sy + a, ky - 1)
        ly = np.clip(np.arange(H) - oy[iy] - shift, 0, th - 1)
        for b in range(int(cx.max())):
            ix = np.minimum(sx + b, kx - 1)
            lx = np.clip(np.arange(W) - ox[ix] - shift, 0, tw - 1)
            live = (a < cy)[:, None] & (b < cx)[None, :]
            tile = ix[None, :] * ky + iy[:, None] if mutant == 'order' else iy[:, None] * kx + ix[None, :]
            v = tiles[tile, :, ly[:, None], lx[None, :]].astype(np.float64)  # [H, W, 3]
            p = v if mutant == 'half' else 0.5 * v + 0.5
            wgt = (wy4[Y, b] * wx4[X, a]) if mutant == 'swap' else (wy4[Y, a] * wx4[X, b])
            wgt = np.where(live, wgt, 0.0)[..., None]
            r += wgt * p
            A += np.abs(wgt) * np.abs(p)
    E = U * ((cy[:, None] + cx[None, :] + 2.0)[..., None] * A + np.abs(r))
    return r, E


def admissible(r, E, trunc=False):
    """-> (lo, hi) int64: the bytes q with lo <= q <= hi are the admissible ones.  trunc: the mutant that truncates 255 x."""
    rnd = np.floor if trunc else np.rint                                     # np.rint rounds ties to even
    lo = rnd(255.0 * np.clip(r - E, 0.0, 1.0)).astype(np.int64)
    hi = rnd(255.0 * np.clip(r + E, 0.0, 1.0)).astype(np.int64)
    return lo, hi


def cut(canvas, plan):
    """tiles [T, 3, th, tw] of a canvas [3, H, W] by slicing: what afx_tiles_cut returns, any dtype."""
    return np.stack([canvas[:, y:y + plan.th, x:x + plan.tw] for y in plan.oy for x in plan.ox])
