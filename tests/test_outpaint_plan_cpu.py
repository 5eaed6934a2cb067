"""``schedule.outpaint_plan``, host integer code: the refusals, two plans window by window, one seeded sweep of geometries replayed with the
numpy restatement of tests/outpaint_ref.py, and that restatement's index rules against ``np.pad``.  On the parent commit every test that
touches the planner fails: ``schedule.outpaint_plan`` does not exist."""
import numpy as np
import pytest

import outpaint_ref as R


def test_refusals():
    from arcflow_amd.schedule import outpaint_plan
    good = dict(H=40, W=56, left=0, top=0, right=24, bottom=16, tile=32, overlap=8, blend=4)
    assert len(outpaint_plan(**good).windows) > 0
    bad = [dict(left=0, top=0, right=0, bottom=0), dict(left=-1), dict(bottom=-8), dict(right=2.0), dict(top=True), dict(left=None),
           dict(tile=40), dict(tile=16), dict(tile=0), dict(tile=33),
           dict(overlap=0), dict(overlap=17), dict(overlap=-1),
           dict(blend=-1), dict(blend=5), dict(overlap=9, blend=5), dict(blend=1.0),
           dict(H=0), dict(W=-3), dict(H=4, W=40, right=0, bottom=8)]                                     # a 12 x 64 canvas
    for kw in bad:
        with pytest.raises(ValueError):
            outpaint_plan(**dict(good, **kw))
    # overlap must stay below the window's sides: a 20 x 200 canvas has 16-pixel-high windows
    assert outpaint_plan(12, 200, 0, 0, 0, 8, tile=64, overlap=15, blend=0).wh == 16
    with pytest.raises(ValueError, match='overlap'):
        outpaint_plan(12, 200, 0, 0, 0, 8, tile=64, overlap=16, blend=0)
    with pytest.raises(ValueError, match='blend'):
        outpaint_plan(**dict(good, blend=5))
    with pytest.raises(ValueError, match='16'):
        outpaint_plan(**dict(good, H=4, W=40, right=0, bottom=8))
    with pytest.raises(ValueError, match='left, top, right, bottom'):
        outpaint_plan(**dict(good, right=0, bottom=0))


def test_two_plans_window_by_window():
    """A photo 3000 wide and 4000 high at the defaults (tile 1024, overlap 256, blend 32)."""
    from arcflow_amd.schedule import outpaint_plan
    p = outpaint_plan(4000, 3000, 0, 0, 1500, 0)
    assert (p.Hc, p.Wc, p.wh, p.ww, p.photo) == (4000, 4500, 1024, 1024, (0, 0, 3000, 4000))
    xs, ys = (2744, 3476), (0, 744, 1488, 2232, 2976)             # 256 back into the photo, then 256 before the end, shifted to the border
    assert list(p.windows) == [(x, y, x + 1024, y + 1024) for x in xs for y in ys] and len(p.windows) == 10
    assert p.windows[0] == (2744, 0, 3768, 1024) and p.windows[-1] == (3476, 2976, 4500, 4000)

    p = outpaint_plan(4000, 3000, 512, 512, 512, 512)
    assert (p.Hc, p.Wc, p.wh, p.ww, p.photo) == (5024, 4024, 1024, 1024, (512, 512, 3512, 4512))
    rows = [512 + (j * 2976) // 4 for j in range(5)]              # the photo's rows: 5 windows
    cols = [(j * 3000) // 4 for j in range(5)]                    # the canvas' width: 5 windows
    want = [(0, y) for y in rows] + [(3000, y) for y in rows] + [(x, 0) for x in cols] + [(x, 4000) for x in cols]
    assert list(p.windows) == [(x, y, x + 1024, y + 1024) for x, y in want] and len(p.windows) == 20
    assert p.windows[0] == (0, 512, 1024, 1536) and p.windows[-1] == (3000, 4000, 4024, 5024)

    # the small plan of the GPU tests: the right band's two rows, then the bottom band across the canvas
    p = outpaint_plan(40, 56, 0, 0, 24, 16, tile=32, overlap=8, blend=4)
    assert (p.Hc, p.Wc, p.wh, p.ww) == (56, 80, 32, 32)
    assert list(p.windows) == [(48, 0, 80, 32), (48, 8, 80, 40), (0, 24, 32, 56), (24, 24, 56, 56), (48, 24, 80, 56)]


def test_sweep_every_window_is_live_and_the_state_ends_at_zero():
    from arcflow_amd.schedule import outpaint_plan
    rng = np.random.default_rng(20)
    done = 0
    while done < 300:
        tile = 16 * int(rng.integers(2, 7))                       # 32 .. 96
        H, W = (int(v) for v in rng.integers(1, 200, 2))
        ext = [int(v) * int(rng.integers(0, 2)) for v in rng.integers(1, 150, 4)]
        overlap = int(rng.integers(1, tile // 2 + 1))
        blend = int(rng.integers(0, overlap // 2 + 1))
        Hc, Wc = H + ext[1] + ext[3], W + ext[0] + ext[2]
        legal = any(ext) and min(Hc, Wc) >= 16 and overlap < min(tile, 16 * (Hc // 16), 16 * (Wc // 16))
        if not legal:
            with pytest.raises(ValueError):
                outpaint_plan(H, W, *ext, tile=tile, overlap=overlap, blend=blend)
            continue
        p = outpaint_plan(H, W, *ext, tile=tile, overlap=overlap, blend=blend)
        done += 1
        key = (H, W, ext, tile, overlap, blend)
        assert (p.Hc, p.Wc, p.photo) == (Hc, Wc, (ext[0], ext[1], ext[0] + W, ext[1] + H)), key
        assert p.wh == min(tile, 16 * (Hc // 16)) and p.ww == min(tile, 16 * (Wc // 16)), key
        assert p.wh % 16 == 0 and p.ww % 16 == 0 and max(p.wh, p.ww) <= tile, key
        covered = np.zeros((Hc, Wc), dtype=bool)
        covered[p.photo[1]:p.photo[3], p.photo[0]:p.photo[2]] = True
        for x0, y0, x1, y1 in p.windows:
            assert 0 <= x0 and 0 <= y0 and x1 <= Wc and y1 <= Hc and (y1 - y0, x1 - x0) == (p.wh, p.ww), (key, (x0, y0, x1, y1))
            covered[y0:y1, x0:x1] = True
        M, live = R.replay(H, W, *ext, blend, p.windows)
        assert all(live), (key, live)                             # each window holds a pixel with M > 0 at its turn
        assert covered.all(), key                                 # the union covers every new pixel
        assert (M == 0).all(), key                                # nothing is left to paint
    assert done == 300


def test_a_window_with_nothing_left_is_dropped():
    """A 56 x 62 photo extended 8 px up and 1 px to the right, tile 64: the canvas is 64 x 63, the windows 64 x 48.  The right band's one
    window (15, 0, 63, 64) covers the canvas' whole height; the top band would lay windows at x = 0 and x = 15, and the second has nothing
    left to paint when its turn comes."""
    from arcflow_amd.schedule import outpaint_plan
    p = outpaint_plan(56, 62, 0, 8, 1, 0, tile=64, overlap=11, blend=1)
    assert (p.wh, p.ww) == (64, 48) and list(p.windows) == [(15, 0, 63, 64), (0, 0, 48, 64)]
    M, live = R.replay(56, 62, 0, 8, 1, 0, 1, [(15, 0, 63, 64), (0, 0, 48, 64), (15, 0, 63, 64)])
    assert live == [True, True, False] and (M == 0).all()


@pytest.mark.parametrize('n', [1, 2, 5, 7])
def test_reference_index_rules_are_np_pad(n):
    a = np.arange(n) + 10
    for before, after in ((0, 0), (1, 2), (n - 1, n - 1), (n, n + 3), (3 * n + 1, 19), (2, 0)):
        i = np.arange(-before, n + after)
        assert np.array_equal(a[R.edge_index(i, n)], np.pad(a, (before, after), mode='edge')), (n, before, after)
        assert np.array_equal(a[R.reflect_index(i, n)], np.pad(a, (before, after), mode='reflect')), (n, before, after)
    src = np.random.default_rng(n).integers(0, 256, (2, n, 3, 3), dtype=np.uint8)                         # the 2-D form, through canvas_extend
    for fill in ('edge', 'reflect'):
        canvas, mask = R.canvas_extend(src, 4, 2 * n + 1, 0, 1, fill, 1)
        assert np.array_equal(canvas, np.pad(src, ((0, 0), (2 * n + 1, 1), (4, 0), (0, 0)), mode=fill))
        assert mask.shape == canvas.shape[1:3] and (mask[:2 * n + 1] == 1).all() and (mask[:, :4] == 1).all()
