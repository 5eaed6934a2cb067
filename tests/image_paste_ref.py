"""fp64 numpy statement of afx_image_paste on the same fp32 tables the kernel gets, with a per-element error bound E and the set of bytes
that bound admits.

``paste(img, mask, src, window, itab_h, itab_w, mtab_h, mtab_w)`` -> (r, E), both fp64 [B, H, W, 3].  Outside the window r = byte / 255 and
E = 0.  Inside, with (v, bv) = ``image_resample_ref.resample(img, itab_h, itab_w, clamp=False)`` and (m', bm) the same of the mask with its
own tables, m = clip(m', 0, 1), p = 0.5 v + 0.5, s = byte / 255:
    r = m p + (1 - m) s.

Where E comes from (u = 2^-24, half an fp32 ulp relative; the kernel: p = fma(0.5, v, 0.5), s = fp32 quotient, t = fl((1 - m) s) with
fl(1 - m), r = fma(m, p, t), byte = rint(fl(255 clamp(r, 0, 1)))):
  * the kernel's v is within bv of v and its m within bm of m (``resample``'s bound; the clamp of m is 1-Lipschitz);
  * p: 0.5 bv carried over, plus one rounding u |p|;
  * the blend is linear in each operand: the error of m enters through d r / d m = p - s, at most (|p| + s) bm; the error of p through m:
    m (0.5 bv + u |p|);
  * the fp32 roundings of the blend itself: s is one rounding (u s), fl(1 - m) one (u (1 - m)), their product one more: 3 u (1 - m) s;
    the fma's result one rounding u |r|; the scaling by 255 before rint one more, relative to clamp(r) <= |r|: another u |r|;
  * second-order terms (products of two of the above; each factor is below 2^-15 of its operand for the <= 128-tap tables): covered by
    two further units u (m |p| + (1 - m) s).
    E = (|p| + s) bm + 0.5 m bv + u (3 m |p| + 5 (1 - m) s + 2 |r|).
No constant is fitted to the kernel.  The clamp to [0, 1] is 1-Lipschitz and 255 x and rint are monotone, so with exact rounding a byte q
is admissible iff  rne(255 clamp(r - E, 0, 1)) <= q <= rne(255 clamp(r + E, 0, 1))  (``admissible``).  Where the kernel's m is exactly 0 it stores
the source byte b; then |m| <= bm, r is within E of s = b / 255 and b = rne(255 s) lies in the interval, so the rule needs no special case.

Mutants (``mutant=``), each a wrong statement the kernel test must reject: 'shift' (the window one pixel to the right and down; the window
must leave room), 'swap' (the horizontal and vertical tables swapped -- for a square call, h == w, that is the paste of the transposed
img and mask), 'invert' (1 - m for m), 'black' (the blend against 0 instead of the source byte), 'rgb' (channels reversed), 'half' (the
+ 0.5 dropped), and ``admissible(..., trunc=True)`` (truncation in place of round-to-nearest-even).
"""
import numpy as np

import image_resample_ref as R

U = 2.0 ** -24
MUTANTS = ('shift', 'swap', 'invert', 'black', 'trunc', 'rgb', 'half')


def tables(h, w, window, filt):
    """(tab_h, tab_w) as numpy triples from ops.resample_tables: h -> window height, w -> window width (the kernel's own fp32 tables)."""
    from arcflow_amd import ops
    x0, y0, x1, y1 = window
    return (tuple(t.numpy() for t in ops.resample_tables(h, y1 - y0, filt)), tuple(t.numpy() for t in ops.resample_tables(w, x1 - x0, filt)))


def paste(img, mask, src, window, itab_h, itab_w, mtab_h=None, mtab_w=None, mutant=None):
    img, src = np.asarray(img, dtype=np.float32), np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 4 and src.shape[3] == 3 and img.ndim == 4 and img.shape[1] == 3
    x0, y0, x1, y1 = window
    if mutant == 'swap':
        assert img.shape[2] == img.shape[3], 'the swapped tables fit a square call only'
        img = img.transpose(0, 1, 3, 2)
        mask = None if mask is None else np.asarray(mask).transpose(0, 1, 3, 2)
    if mutant == 'rgb':
        img = img[:, ::-1]
    v, bv = R.resample(img, itab_h, itab_w, clamp=False)                    # [B, 3, wh, ww]
    if mask is None:
        m, bm = np.ones((1, 1) + v.shape[2:]), np.zeros((1, 1) + v.shape[2:])
    else:
        m, bm = R.resample(np.asarray(mask, dtype=np.float32), mtab_h, mtab_w, clamp=True)
    if mutant == 'invert':
        m = 1.0 - m
    if mutant == 'shift':
        x0, y0, x1, y1 = x0 + 1, y0 + 1, x1 + 1, y1 + 1
        assert x1 <= src.shape[2] and y1 <= src.shape[1], 'the shifted window must stay inside the source'
    r = src.astype(np.float64) / 255.0
    E = np.zeros_like(r)
    s = r[:, y0:y1, x0:x1].transpose(0, 3, 1, 2)                            # [B, 3, wh, ww]
    p = 0.5 * v + (0.0 if mutant == 'half' else 0.5)
    keep = 0.0 if mutant == 'black' else (1.0 - m) * s
    rin = m * p + keep
    Ein = (np.abs(p) + s) * bm + 0.5 * m * bv + U * (3.0 * m * np.abs(p) + 5.0 * (1.0 - m) * s + 2.0 * np.abs(rin))
    r[:, y0:y1, x0:x1] = rin.transpose(0, 2, 3, 1)
    E[:, y0:y1, x0:x1] = Ein.transpose(0, 2, 3, 1)
    return r, E


def admissible(r, E, trunc=False):
    """-> (lo, hi) int64: the bytes q with lo <= q <= hi are the admissible ones.  trunc: the mutant that truncates 255 x."""
    rnd = np.floor if trunc else np.rint                                     # np.rint rounds ties to even
    lo = rnd(255.0 * np.clip(r - E, 0.0, 1.0)).astype(np.int64)             # (both ends are clamped to [0, 1]: r itself may lie outside)
    hi = rnd(255.0 * np.clip(r + E, 0.0, 1.0)).astype(np.int64)
    return lo, hi


# The shapes of the kernel test (tests/test_hip_image_paste_fp64.py), shared with the CPU test that shows the mutants separable and the
# admissible sets narrow at exactly these shapes: (source H x W), window (x0, y0, x1, y1), (call h x w).  B = 2 everywhere.
CASES = {
    'mixed': ((37, 53), (5, 3, 45, 30), (32, 48)),                # up on one axis, down on the other
    'up4': ((150, 200), (20, 10, 140, 130), (32, 32)),            # about 4x up
    'down': ((64, 64), (7, 9, 27, 39), (64, 64)),                 # down, a square call with a window that is not: the swap mutant
    'two_groups': ((40, 300), (0, 0, 300, 40), (16, 64)),         # the whole image; W = 256 + 44: two work-groups, the second partly filled
    'border': ((33, 35), (0, 0, 35, 33), (16, 16)),               # the window on all four borders
    'one_pixel': ((33, 35), (34, 32, 35, 33), (16, 16)),          # a 1 x 1 window in the last corner
    'many_rows': ((33000, 5), (1, 32900, 4, 33000), (16, 16)),    # 2 x 33000 rows > 65535: the second trip of the paste's row loop pastes
}


def inputs(case, seed=0):
    """-> (img fp32 [2, 3, h, w] uniform in [-1.2, 1.2] (the clamp acts), mask fp32 [2, 1, h, w] (image 0: 0 on the left third, 1 on the
    right third, a linear ramp between; image 1: the same from top to bottom), src uint8 [2, H, W, 3] uniform over all 256 values)."""
    (H, W), _, (h, w) = CASES[case]
    rng = np.random.default_rng(seed + sum(map(ord, case)))
    img = (rng.random((2, 3, h, w), dtype=np.float32) * np.float32(2.4) - np.float32(1.2)).astype(np.float32)
    src = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    rx = np.clip((np.arange(w, dtype=np.float32) - w / 3.0) / (w / 3.0), 0.0, 1.0).astype(np.float32)
    ry = np.clip((np.arange(h, dtype=np.float32) - h / 3.0) / (h / 3.0), 0.0, 1.0).astype(np.float32)
    mask = np.stack([np.broadcast_to(rx[None, :], (h, w)), np.broadcast_to(ry[:, None], (h, w))])[:, None].astype(np.float32).copy()
    return img, mask, src
